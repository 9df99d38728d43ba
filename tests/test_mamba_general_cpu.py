"""Host side of the general-d_state Mamba and of the multimodal Mamba blocks (reference ConNexT/models/block/len4mamba.py):
constructor and state-dict layout, the yardstick `mamba_general_ref` against an independent implementation, and the C ABI
declarations.  No GPU."""
import re

import pytest
import torch

import mamba_general_ref as gr


def _mixer(hidden, state):
    mm = pytest.importorskip("transformers.models.mamba.modeling_mamba")
    cfg = mm.MambaConfig(hidden_size=hidden, state_size=state, conv_kernel=4, expand=2, num_hidden_layers=1, vocab_size=8)
    return mm.MambaMixer(cfg, layer_idx=0)


def test_mamba_takes_d_state_and_matches_the_mixer_state_dict():
    from hamspine.nn import Mamba
    m = Mamba(32, d_state=128)
    assert m.d_state == 128 and m.d_conv == 4 and m.expand == 2 and m.d_inner == 64 and m.dt_rank == 2
    assert torch.equal(m.A_log, torch.log(torch.arange(1, 129, dtype=torch.float32)).repeat(64, 1))
    mixer = _mixer(32, 128)
    ours, theirs = m.state_dict(), mixer.state_dict()
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in theirs.items()}
    assert tuple(ours["A_log"].shape) == (64, 128) and tuple(ours["x_proj.weight"].shape) == (2 + 256, 64)
    mixer.load_state_dict(ours, strict=True)
    m.load_state_dict(theirs, strict=True)
    # the defaults build what Mamba(d_model) built before: mamba_ssm's d_state 16, d_conv 4, expand 2, dt_rank "auto"
    d = Mamba(32)
    assert tuple(d.A_log.shape) == (64, 16) and tuple(d.x_proj.weight.shape) == (34, 64) and d.dt_rank == 2
    assert Mamba(32, 16, 4, 2, "auto").dt_rank == 2 and Mamba(32, dt_rank=5).dt_rank == 5
    for bad in (dict(d_state=24), dict(d_state=512), dict(d_conv=3)):
        with pytest.raises(NotImplementedError):
            Mamba(32, **bad)


_ATTN_KEYS = [f"attn.{p}_proj.layers.0.{n}" for p in "qkv" for n in ("base_weight", "grid", "spline_scaler", "spline_weight")] + [
    "attn.out_proj.bias", "attn.out_proj.weight"]
_MAMBA_KEYS = ["mamba.A_log", "mamba.D", "mamba.conv1d.bias", "mamba.conv1d.weight", "mamba.dt_proj.bias", "mamba.dt_proj.weight",
               "mamba.in_proj.weight", "mamba.out_proj.weight", "mamba.x_proj.weight"]
_PROJ_KEYS = [f"proj_{n}.{w}" for n in ("first", "img", "last", "text") for w in ("bias", "weight")]
_NORM_KEYS = ["norm1.bias", "norm1.weight", "norm2.bias", "norm2.weight"]


def test_len4mamba_blocks_import_and_construct_on_the_cpu():
    import inspect
    from ConNexT.models.block.len4mamba import KANMultiheadAttention, MultimodalMamba, MultimodalMambaWithKANAttention
    a = MultimodalMambaWithKANAttention(text_dim=24, img_dim=40, hidden_dim=56, proj_dim=32, num_heads=4)
    assert sorted(a.state_dict().keys()) == sorted(_ATTN_KEYS + _MAMBA_KEYS + _PROJ_KEYS + _NORM_KEYS)
    assert "attn.q_proj.layers.0.grid" in a.state_dict()
    b = MultimodalMamba(text_dim=24, img_dim=40, hidden_dim=56, proj_dim=32)
    assert sorted(b.state_dict().keys()) == sorted(_MAMBA_KEYS + _PROJ_KEYS)
    for m in (a, b):
        assert "positional_encoding" not in m.state_dict() and "positional_encoding" not in dict(m.named_buffers())
        assert tuple(m.positional_encoding.shape) == (1, 2048, 32)
        # against an independent float64 evaluation.  The f32 angle t * w carries the rounding of w (exp of an argument up to
        # 9.2 rounded to f32: about 9 * 2^-24 relative, plus exp's own ulp) and of the product, under 12 * 2^-24 relative in all;
        # sin / cos add an ulp of a value <= 1
        rows = torch.arange(2048, dtype=torch.float64)[None, :, None]
        err = (m.positional_encoding.double() - gr.sinusoid_table(2048, 32)).abs()
        assert m.positional_encoding.dtype == torch.float32 and bool((err <= rows * 12 * 2.0 ** -24 + 2.0 ** -22).all())
        assert m.mamba.d_state == 128 and tuple(m.mamba.A_log.shape) == (64, 128)
        assert tuple(m.proj_img.weight.shape) == (32, 40) and tuple(m.proj_first.weight.shape) == (32, 56)
    k = KANMultiheadAttention(32)
    assert k.num_heads == 8 and k.dropout == 0.0 and k.head_dim == 4
    assert sorted(k.state_dict().keys()) == sorted(n[len("attn."):] for n in _ATTN_KEYS)
    # the reference's signatures and defaults (len4mamba.py:22,65,131,37,86)
    defaults = lambda f: {n: p.default for n, p in inspect.signature(f).parameters.items() if n != "self"}
    assert defaults(MultimodalMambaWithKANAttention.__init__) == dict(text_dim=768, img_dim=640, hidden_dim=3584, proj_dim=256,
                                                                       num_heads=4)
    assert defaults(MultimodalMamba.__init__) == dict(text_dim=768, img_dim=1568, hidden_dim=3584, proj_dim=256)
    assert defaults(KANMultiheadAttention.__init__) == dict(embed_dim=inspect.Parameter.empty, num_heads=8, dropout=0.0)
    assert list(defaults(MultimodalMamba.forward)) == ["text", "img", "first_hidden", "last_hidden"]
    assert defaults(KANMultiheadAttention.forward) == dict(x=inspect.Parameter.empty, mask=None)
    src = inspect.getsource(inspect.getmodule(MultimodalMamba))
    assert "mamba_ssm" not in src.replace("`mamba_ssm.Mamba`", "")


@pytest.mark.parametrize("state", [32, 128, 256])
def test_general_ref_equals_the_transformers_mixer_in_float64(state):
    torch.manual_seed(5 + state)
    mixer = _mixer(32, state).double().eval()
    with torch.no_grad():
        for p in mixer.parameters():        # away from any special initial value
            p.add_(0.05 * torch.randn_like(p))
    x = torch.randn(2, 7, 32, dtype=torch.float64)
    with torch.no_grad():
        want = mixer(x)
        got = gr.mamba_ref(x, {k: v.double() for k, v in mixer.state_dict().items()})
    err = (got - want).abs().max().item()
    print(f"mamba_general_ref vs MambaMixer(state_size={state}): max |diff| {err:.3e} on max |ref| {want.abs().max().item():.3e}")
    assert err <= 1e-6 * want.abs().max().item()


def test_header_declares_and_binding_lists_the_general_scan_entry_points():
    import hamspine._lib as L
    names = {"hs_selective_scan_chunk_len_n": "int32_t", "hs_selective_scan_ws_bytes_n": "int64_t"}
    syms = L.exported_symbols()
    header = open(L.HEADER_PATH).read()
    lib = L.lib()
    for n, ret in names.items():
        assert n in syms, n
        assert re.search(ret + r"\s+" + n + r"\s*\(", header), n
        head = header[:header.index(n + "(")]
        assert "ConNexT/models/block/len4mamba.py:74-79,138-143" in head[head.rindex("/*"):], n
        assert hasattr(lib, n) and getattr(lib, n).argtypes, n
    # host logic only: the N = 16 values are those of the entry points without N, any other N is negative
    assert lib.hs_selective_scan_chunk_len_n(16) == lib.hs_selective_scan_chunk_len() == 16
    assert lib.hs_selective_scan_ws_bytes_n(3, 21, 80, 16) == lib.hs_selective_scan_ws_bytes(3, 21, 80)
    for n in (32, 64, 128, 256):
        lc = lib.hs_selective_scan_chunk_len_n(n)
        assert 1 <= lc <= 16 and lc * (n // 16) <= 64          # chunk x states per lane: the backward's register budget
        assert lib.hs_selective_scan_ws_bytes_n(3, 21, 80, n) == (5 * 3 * 21 * 2 * n + 3 * 80 * (n + 2)) * 4
    for n in (0, 8, 24, 48, 512):
        assert lib.hs_selective_scan_chunk_len_n(n) < 0 and lib.hs_selective_scan_ws_bytes_n(3, 21, 80, n) < 0
