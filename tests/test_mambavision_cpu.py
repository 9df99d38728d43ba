"""Host side of the MambaVision mixer, Block and hybrid stage (reference ConNexT/models/block/mamba_vision.py): the drop-in module
imports and constructs without timm / mamba_ssm, its state-dict layout equals the one recorded from the reference, the yardstick
`mambavision_ref` reproduces the recorded float64 output and input gradient, the refusals, and the C ABI declarations.  No GPU.

tests/golden/mambavision_layer.npz is written by tests/gen_mambavision_golden.py from the reference's own MambaVisionLayer; it
pins everything except the arithmetic of the scan, which is the yardstick's loop on both sides."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import mambavision_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mambavision_layer.npz")
LAYER_KW = dict(dim=32, depth=2, num_heads=2, window_size=3, conv=False, downsample=False, transformer_blocks=[1], layer_scale=0.5)


def _golden():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    return z, sd


def test_module_imports_without_timm_and_mamba_ssm():
    import ConNexT.models.block.mamba_vision as mv
    for name in ("MambaVisionMixer", "Attention", "Block", "MambaVisionLayer", "window_partition", "window_reverse"):
        assert hasattr(mv, name), name
    for dep in ("timm", "mamba_ssm", "einops"):
        assert not re.search(r"^\s*(import|from)\s+" + dep + r"\b", inspect.getsource(mv), flags=re.M), dep
    assert "mamba_ssm" not in sys.modules and "timm" not in sys.modules


def test_constructor_attributes_and_state_dict_equal_the_reference():
    from ConNexT.models.block.mamba_vision import Attention, Block, MambaVisionLayer, MambaVisionMixer
    _, sd = _golden()
    layer = MambaVisionLayer(**LAYER_KW)
    ours = layer.state_dict()
    assert list(ours.keys()) == list(sd.keys())
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    layer.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in layer.state_dict().items())
    assert layer.window_size == 3 and layer.downsample is None and layer.transformer_block and not layer.conv and not layer.do_gt
    mixer, attn = layer.blocks[0].mixer, layer.blocks[1].mixer
    assert isinstance(mixer, MambaVisionMixer) and isinstance(attn, Attention)
    assert (mixer.d_model, mixer.d_state, mixer.d_conv, mixer.expand, mixer.d_inner, mixer.dt_rank) == (32, 8, 3, 1, 32, 2)
    fresh = MambaVisionMixer(32, d_state=8, d_conv=3, expand=1)            # Mamba's initialisation
    assert torch.equal(fresh.A_log, torch.log(torch.arange(1, 9, dtype=torch.float32)).repeat(16, 1))
    assert torch.equal(fresh.D, torch.ones(16)) and fresh.A_log._no_weight_decay and fresh.D._no_weight_decay
    dt = torch.nn.functional.softplus(fresh.dt_proj.bias.detach())
    assert dt.min().item() >= 1e-3 * (1 - 1e-5) and dt.max().item() <= 1e-1 * (1 + 1e-5) and fresh.dt_proj.bias._no_reinit
    assert fresh.dt_proj.weight.abs().max().item() <= 2 ** -0.5
    assert (attn.num_heads, attn.head_dim, attn.scale, attn.fused_attn) == (2, 16, 0.25, True)
    assert attn.qkv.bias is not None                       # MambaVisionLayer's qkv_bias default is True ...
    assert Attention(32, 2).qkv.bias is None               # ... Attention's and Block's is False
    assert Block(32, 2, 0, [0]).mixer.qkv.bias is None
    # the signatures the reference declares
    assert list(inspect.signature(MambaVisionMixer.__init__).parameters)[1:] == [
        "d_model", "d_state", "d_conv", "expand", "dt_rank", "dt_min", "dt_max", "dt_init", "dt_scale", "dt_init_floor", "conv_bias",
        "bias", "use_fast_path", "layer_idx", "device", "dtype"]
    assert list(inspect.signature(Attention.__init__).parameters)[1:] == [
        "dim", "num_heads", "qkv_bias", "qk_norm", "attn_drop", "proj_drop", "norm_layer"]
    assert list(inspect.signature(Block.__init__).parameters)[1:] == [
        "dim", "num_heads", "counter", "transformer_blocks", "mlp_ratio", "qkv_bias", "qk_scale", "drop", "attn_drop", "drop_path",
        "act_layer", "norm_layer", "Mlp_block", "layer_scale"]
    assert list(inspect.signature(MambaVisionLayer.__init__).parameters)[1:] == [
        "dim", "depth", "num_heads", "window_size", "conv", "downsample", "mlp_ratio", "qkv_bias", "qk_scale", "drop", "attn_drop",
        "drop_path", "layer_scale", "layer_scale_conv", "transformer_blocks"]
    d = {k: v.default for k, v in inspect.signature(MambaVisionMixer.__init__).parameters.items()}
    assert (d["d_state"], d["d_conv"], d["expand"], d["dt_rank"], d["conv_bias"], d["bias"]) == (16, 4, 2, "auto", True, False)
    assert inspect.signature(MambaVisionLayer.__init__).parameters["downsample"].default is True


def test_mixer_has_no_conv_bias_and_the_dt_rank_of_the_reference():
    from ConNexT.models.block.mamba_vision import MambaVisionMixer
    m = MambaVisionMixer(80, d_state=8, d_conv=3, expand=1)
    keys = sorted(m.state_dict().keys())
    assert keys == sorted(["A_log", "D", "in_proj.weight", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "out_proj.weight",
                           "conv1d_x.weight", "conv1d_z.weight"])
    assert m.conv1d_x.bias is None and m.conv1d_z.bias is None
    assert tuple(m.conv1d_x.weight.shape) == (40, 1, 3) and tuple(m.x_proj.weight.shape) == (5 + 16, 40)
    assert tuple(m.dt_proj.weight.shape) == (40, 5) and tuple(m.in_proj.weight.shape) == (80, 80)
    assert tuple(MambaVisionMixer(320, 8, 3, 1).x_proj.weight.shape) == (20 + 16, 160)


def test_gamma_is_a_parameter_only_with_a_numeric_layer_scale():
    from ConNexT.models.block.mamba_vision import Block
    plain = Block(32, 2, 0, [])
    assert plain.gamma_1 == 1 and plain.gamma_2 == 1 and not any("gamma" in k or "unit" in k for k in plain.state_dict())
    assert not any("gamma" in n for n, _ in plain.named_parameters())
    for scale in (0.5, 1):
        b = Block(32, 2, 0, [], layer_scale=scale)
        assert isinstance(b.gamma_1, torch.nn.Parameter) and torch.equal(b.gamma_2.detach(), scale * torch.ones(32))
        assert "gamma_1" in b.state_dict() and "gamma_2" in b.state_dict()
    assert Block(32, 2, 0, [], layer_scale="1e-5").gamma_1 == 1            # not a number: the reference ignores it too


def test_yardstick_reproduces_the_reference_in_float64():
    """the same arithmetic on both sides apart from summation order: relative error <= 1e-10"""
    z, sd = _golden()
    params = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    out = mr.layer_ref(x, params, num_heads=2, window_size=3)
    (out * torch.from_numpy(z["cotangent"]).double()).sum().backward()
    ref_out, ref_dx = torch.from_numpy(z["out"]), torch.from_numpy(z["dx"])
    assert ref_out.dtype == torch.float64 and tuple(ref_out.shape) == (2, 32, 5, 5)
    e_out = ((out.detach() - ref_out).norm() / ref_out.norm()).item()
    e_dx = ((x.grad - ref_dx).norm() / ref_dx.norm()).item()
    print(f"yardstick against the recorded reference: out {e_out:.2e} dx {e_dx:.2e}")
    assert e_out <= 1e-10 and e_dx <= 1e-10


def test_refusals_raise_on_the_cpu():
    from ConNexT.models.block.mamba_vision import Attention, Block, MambaVisionLayer, MambaVisionMixer
    with pytest.raises(NotImplementedError, match="d_state 16"):
        MambaVisionMixer(32, d_state=16, d_conv=3, expand=1)
    with pytest.raises(NotImplementedError, match="d_conv 4"):
        MambaVisionMixer(32, d_state=8, d_conv=4, expand=1)
    with pytest.raises(NotImplementedError):
        MambaVisionMixer(32)                                # the reference's own defaults are d_state 16, d_conv 4
    with pytest.raises(NotImplementedError, match="qk_norm"):
        Attention(32, 2, qk_norm=True)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        Block(32, 2, 0, [0], qk_scale=True)
    kw = {k: v for k, v in LAYER_KW.items() if k not in ("conv", "downsample")}
    with pytest.raises(NotImplementedError, match="follow-up"):
        MambaVisionLayer(conv=True, downsample=False, **kw)
    with pytest.raises(NotImplementedError, match="follow-up"):
        MambaVisionLayer(conv=False, downsample=True, **kw)
    with pytest.raises(NotImplementedError, match="follow-up"):
        MambaVisionLayer(conv=False, **kw)                  # downsample defaults to True


def test_header_declares_and_binding_lists_the_new_entry_points():
    import ctypes
    import hamspine._lib as L
    names = {"hs_conv1d_same_silu_fwd": "hs_status", "hs_conv1d_same_silu_bwd": "hs_status", "hs_conv1d_same_silu_ws_bytes": "int64_t",
             "hs_window_partition": "hs_status", "hs_window_reverse": "hs_status", "hs_selective_scan_chunk_len_nogate": "int32_t",
             "hs_selective_scan_ws_bytes_nogate": "int64_t"}
    syms = L.exported_symbols()
    header = open(L.HEADER_PATH).read()
    lib = L.lib()
    restypes = {"hs_status": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for n, ret in names.items():
        assert n in syms, n
        assert re.search(ret + r"\s+" + n + r"\s*\(", header), n
        # the binding is derived from the header: as many argument types as the prototype has parameters, and its return type
        args = re.search(ret + r"\s+" + n + r"\s*\(([^()]*)\)\s*;", header)[1]
        assert len(getattr(lib, n).argtypes) == (0 if args.strip() == "void" else args.count(",") + 1), n
        assert getattr(lib, n).restype is restypes[ret], n
    # every new declaration carries the reference lines it replaces
    for n in ("hs_conv1d_same_silu_fwd", "hs_conv1d_same_silu_bwd", "hs_window_partition", "hs_window_reverse",
              "hs_selective_scan_chunk_len_nogate"):
        head = header[:header.index(n + "(")]
        assert "ConNexT/models/block/mamba_vision.py:" in head[head.rindex("/*"):], n
    for n in names:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    # host logic only: 8 states without a gate save a state every 16 steps and reduce over blocks of 32 channels
    assert lib.hs_selective_scan_chunk_len_nogate(8) == 16
    assert lib.hs_selective_scan_ws_bytes_nogate(3, 21, 80, 8) == (3 * 3 * 21 * 16 + 3 * 80 * 10) * 4
    for n in (0, 16, 24, 128):
        assert lib.hs_selective_scan_chunk_len_nogate(n) < 0 and lib.hs_selective_scan_ws_bytes_nogate(3, 21, 80, n) < 0
    assert lib.hs_conv1d_same_silu_ws_bytes(3, 80) == 3 * 4 * 80 * 4
