"""Host side of the convolutional half of MambaVision, the full model, its factories and the encoder (reference
ConNexT/models/block/mamba_vision.py:1333-1524,1833-2472): the names import and construct without timm / mamba_ssm / einops, the
state-dict layouts equal the ones recorded from the reference, the yardstick `mambavision_model_ref` reproduces the recorded
float64 results, nothing ever downloads, checkpoint wrappers and prefixes, and the C ABI declarations.  No GPU.

tests/golden/mambavision_model.npz and mambavision_variants.json are written by tests/gen_mambavision_model_golden.py from the
reference's own classes."""
import hashlib
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import mambavision_model_ref as mm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mambavision_model.npz")
VARIANTS = os.path.join(HERE, "golden", "mambavision_variants.json")
SMALL_KW = dict(dim=8, in_dim=8, depths=[1, 2, 2, 2], num_heads=[1, 1, 2, 2], window_size=[8, 8, 4, 2], mlp_ratio=2,
                drop_path_rate=0., num_classes=5, layer_scale=0.5, layer_scale_conv=0.5)
NEW_NAMES = ("PatchEmbed", "ConvBlock", "Downsample", "MambaVisionStage", "MambaVision", "MambaVisionEncoder",
             "create_mamba_vision_encoder", "_load_checkpoint", "_load_state_dict")
FACTORIES = ("mamba_vision_T", "mamba_vision_T2", "mamba_vision_S", "mamba_vision_B", "mamba_vision_B_21k", "mamba_vision_L",
             "mamba_vision_L_21k", "mamba_vision_L2", "mamba_vision_L2_512_21k", "mamba_vision_L3_256_21k", "mamba_vision_L3_512_21k")


def _golden():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    return z, sd


def test_the_names_import_without_timm_mamba_ssm_and_einops():
    import ConNexT.models.block.mamba_vision as mv
    for name in NEW_NAMES + FACTORIES:
        assert hasattr(mv, name), name
    for dep in ("timm", "mamba_ssm", "einops"):
        assert not re.search(r"^\s*(import|from)\s+" + dep + r"\b", inspect.getsource(mv), flags=re.M), dep
    assert "mamba_ssm" not in sys.modules and "timm" not in sys.modules


def test_small_model_state_dict_equals_the_reference():
    from ConNexT.models.block.mamba_vision import Block, ConvBlock, Downsample, MambaVision, MambaVisionStage
    _, sd = _golden()
    model = MambaVision(**SMALL_KW)
    ours = model.state_dict()
    assert list(ours.keys()) == list(sd.keys())
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    assert tuple(ours["levels.0.downsample.reduction.0.weight"].shape) == (16, 8, 3, 3)
    assert tuple(ours["patch_embed.conv_down.0.weight"].shape) == (8, 3, 3, 3)
    for i, level in enumerate(model.levels):
        assert isinstance(level, MambaVisionStage)
        assert level.conv == (i < 2) and level.transformer_block == (i >= 2) and not level.do_gt
        assert (level.downsample is None) == (i == 3) and level.window_size == SMALL_KW["window_size"][i]
        assert all(isinstance(b, ConvBlock if i < 2 else Block) for b in level.blocks)
        assert level.downsample is None or isinstance(level.downsample, Downsample)
    # the transformer_blocks rule of lines 1877-1895: the second half of an even depth is attention
    assert "mixer.qkv.weight" in "".join(model.levels[2].blocks[1].state_dict()) and "mixer.A_log" in model.levels[2].blocks[0].state_dict()
    assert model.patch_embed.conv_down[1].eps == 1e-4 and model.levels[0].blocks[0].norm1.eps == 1e-5 and model.norm.eps == 1e-5
    assert model.no_weight_decay_keywords() == {"rpb"}
    assert MambaVision(resolution=224, **SMALL_KW).num_classes == 5            # **kwargs are swallowed


def test_conv_block_gamma_and_signatures():
    from ConNexT.models.block.mamba_vision import ConvBlock, Downsample, MambaVision, MambaVisionStage, PatchEmbed
    assert "gamma" not in ConvBlock(8).state_dict() and not ConvBlock(8).layer_scale
    assert "gamma" not in ConvBlock(8, layer_scale="1e-5").state_dict()
    b = ConvBlock(8, layer_scale=0.5)
    assert b.layer_scale is True and torch.equal(b.gamma.detach(), 0.5 * torch.ones(8))
    assert sorted(b.state_dict()) == sorted(["gamma"] + [f"{m}.{p}" for m in ("conv1", "conv2") for p in ("weight", "bias")] +
                                            [f"{m}.{p}" for m in ("norm1", "norm2")
                                             for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")])
    assert list(Downsample(8).state_dict()) == ["reduction.0.weight"] and tuple(Downsample(8, keep_dim=True).reduction[0].weight.shape) == (8, 8, 3, 3)
    assert [k.rsplit(".", 1)[0] for k in PatchEmbed().state_dict() if k.endswith("weight")] == ["conv_down.0", "conv_down.1", "conv_down.3", "conv_down.4"]
    assert list(inspect.signature(ConvBlock.__init__).parameters)[1:] == ["dim", "drop_path", "layer_scale", "kernel_size"]
    assert list(inspect.signature(PatchEmbed.__init__).parameters)[1:] == ["in_chans", "in_dim", "dim"]
    assert list(inspect.signature(Downsample.__init__).parameters)[1:] == ["dim", "keep_dim"]
    assert list(inspect.signature(MambaVision.__init__).parameters)[1:] == [
        "dim", "in_dim", "depths", "window_size", "mlp_ratio", "num_heads", "drop_path_rate", "in_chans", "num_classes", "qkv_bias",
        "qk_scale", "drop_rate", "attn_drop_rate", "layer_scale", "layer_scale_conv", "kwargs"]
    assert list(inspect.signature(MambaVisionStage.__init__).parameters)[1:] == [
        "dim", "depth", "num_heads", "window_size", "conv", "downsample", "mlp_ratio", "qkv_bias", "qk_scale", "drop", "attn_drop",
        "drop_path", "layer_scale", "layer_scale_conv", "transformer_blocks"]


def test_init_weights_trunc_normal_on_every_linear():
    from ConNexT.models.block.mamba_vision import MambaVision
    torch.manual_seed(0)
    model = MambaVision(**SMALL_KW)
    for n, m in model.named_modules():
        if isinstance(m, torch.nn.Linear):
            assert m.weight.abs().max().item() <= 2.0 and m.weight.std().item() < 0.04, n       # std 0.02, cut at +-2
            assert m.bias is None or "dt_proj" in n or not m.bias.any(), n
        elif isinstance(m, (torch.nn.BatchNorm2d, torch.nn.LayerNorm)):
            assert torch.equal(m.weight.detach(), torch.ones_like(m.weight)) and not m.bias.any(), n


def _signature(model):
    sd = model.state_dict()
    lines = "\n".join(f"{k}:{tuple(v.shape)}" for k, v in sd.items())
    return {"keys": len(sd), "parameters": sum(p.numel() for p in model.parameters()),
            "sha256": hashlib.sha256(lines.encode()).hexdigest()}


@pytest.mark.parametrize("name", FACTORIES)
def test_factory_matches_the_reference_on_the_meta_device(name):
    import ConNexT.models.block.mamba_vision as mv
    want = json.load(open(VARIANTS))["factories"][name]
    with torch.device("meta"):
        model = getattr(mv, name)(pretrained=False)
    assert _signature(model) == want
    assert model.default_cfg is model.pretrained_cfg and model.pretrained_cfg["num_classes"] == 1000


def test_encoder_shape_arithmetic_and_members():
    import ConNexT.models.block.mamba_vision as mv
    want = json.load(open(VARIANTS))["encoder"]
    for variant in ("T", "S"):
        with torch.device("meta"):
            enc = mv.MambaVisionEncoder(output_dim=768, pretrained=False, model_variant=variant)
        assert isinstance(enc.mamba_vision.head, torch.nn.Identity)
        assert tuple(enc.projection.weight.shape) == (768, want[variant]["num_features"])
        C, H, W = want[variant]["map"]
        assert enc.mamba_vision.norm.num_features == C and C * H * W == 1568 * want[variant]["tokens"][1]
    with pytest.raises(ValueError, match="Unsupported"):
        mv.MambaVisionEncoder(pretrained=False, model_variant="B")
    with pytest.raises(ValueError, match="Unsupported"):
        mv.create_mamba_vision_encoder(pretrained=False, model_variant="nope")


def test_yardstick_reproduces_the_reference_in_float64():
    """the same arithmetic on both sides apart from summation order: relative error <= 1e-10"""
    z, sd = _golden()
    params = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    stats = {}
    logits, fusion = mm.model_ref(x, params, SMALL_KW["num_heads"], SMALL_KW["window_size"], new_stats=stats)
    (logits * torch.from_numpy(z["cotangent"]).double()).sum().backward()
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    errs = {"logits": rel(logits.detach(), torch.from_numpy(z["logits"])), "fusion": rel(fusion.detach(), torch.from_numpy(z["fusion"])),
            "dx": rel(x.grad, torch.from_numpy(z["dx"]))}
    assert tuple(fusion.shape) == (2, 64, 3, 3) and z["logits"].dtype == np.float64
    after = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("after.") and "running_" in k}
    assert sorted(after) == sorted(stats)
    errs["running"] = max(rel(stats[k], after[k]) for k in after)
    params.update(stats)
    errs["eval_logits"] = rel(mm.model_ref(x.detach(), params, SMALL_KW["num_heads"], SMALL_KW["window_size"], training=False)[0],
                              torch.from_numpy(z["eval_logits"]))
    print("yardstick against the recorded reference:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= 1e-10 for v in errs.values()), errs


def test_pretrained_without_a_file_raises_and_never_downloads(tmp_path, monkeypatch):
    import ConNexT.models.block.mamba_vision as mv

    def refuse(*a, **k):
        raise AssertionError("a download was attempted")
    monkeypatch.setattr(torch.hub, "download_url_to_file", refuse)
    missing = str(tmp_path / "absent.pth.tar")
    for name in FACTORIES:
        with pytest.raises(FileNotFoundError, match="absent.pth.tar"):
            getattr(mv, name)(pretrained=True, model_path=missing)
    monkeypatch.setattr(mv.MambaVisionEncoder, "_PATHS", {"T": ("mamba_vision_T", missing)})
    with pytest.raises(FileNotFoundError, match="absent.pth.tar"):
        mv.MambaVisionEncoder(pretrained=True, model_variant="T")


@pytest.mark.parametrize("wrapper", [None, "state_dict", "model"])
@pytest.mark.parametrize("prefix", ["", "module.", "encoder."])
def test_checkpoint_wrappers_and_prefixes(tmp_path, capsys, wrapper, prefix):
    from ConNexT.models.block.mamba_vision import MambaVision
    _, sd = _golden()
    state = {prefix + k: v for k, v in sd.items()}
    path = str(tmp_path / "ck.pth.tar")
    torch.save({wrapper: state} if wrapper else state, path)
    model = MambaVision(**SMALL_KW)
    model._load_state_dict(path, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    assert "do not match" not in capsys.readouterr().out


def test_non_strict_loading_reports_instead_of_raising(tmp_path, capsys):
    from ConNexT.models.block.mamba_vision import MambaVision, _load_checkpoint
    _, sd = _golden()
    state = {k: v for k, v in sd.items() if k != "head.bias" and "num_batches_tracked" not in k}
    state["stray.weight"] = torch.zeros(1)
    path = str(tmp_path / "ck.pth.tar")
    torch.save({"state_dict": state}, path)
    model = MambaVision(**SMALL_KW)
    model._load_state_dict(path)
    out = capsys.readouterr().out
    assert "stray.weight" in out and "head.bias" in out and "num_batches_tracked" not in out
    assert torch.equal(model.head.weight.detach(), sd["head.weight"])
    with pytest.raises(RuntimeError, match="do not match"):
        _load_checkpoint(MambaVision(**SMALL_KW), path, strict=True)
    torch.save([1, 2], path)
    with pytest.raises(RuntimeError, match="No state_dict"):
        _load_checkpoint(model, path)


def test_header_declares_and_binding_lists_the_new_entry_points():
    import ctypes
    import hamspine._lib as L
    names = {"hs_conv3x3_fwd": "hs_status", "hs_conv3x3_dgrad": "hs_status", "hs_conv3x3_pack_filter": "hs_status",
             "hs_conv3x3_unpack_wgrad": "hs_status", "hs_pack_image_nhwc": "hs_status", "hs_unpack_image_nhwc": "hs_status",
             "hs_bn_gelu_tanh_fwd": "hs_status", "hs_bn_scale_residual_fwd": "hs_status", "hs_bn_epilogue_bwd": "hs_status",
             "hs_bn_epilogue_ws_bytes": "int64_t", "hs_window_partition_nhwc": "hs_status", "hs_window_reverse_nhwc": "hs_status"}
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
        head = header[:header.index(n + "(")]          # every new declaration carries the reference lines it replaces
        assert "ConNexT/models/block/mamba_vision.py:" in head[head.rindex("/*"):], n
    for n in names:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    # host logic only: row blocks of at least 64 rows, at most 256 of them, two sums per channel and three coefficients
    assert lib.hs_bn_epilogue_ws_bytes(98, 80) == (2 * 80 * 2 + 3 * 80) * 4
    assert lib.hs_bn_epilogue_ws_bytes(3, 8) == (1 * 8 * 2 + 3 * 8) * 4
    assert lib.hs_bn_epilogue_ws_bytes(100352, 196) == (256 * 196 * 2 + 3 * 196) * 4
    assert lib.hs_bn_epilogue_ws_bytes(0, 8) < 0
