"""Host side of the Mamba / SSM fusion (reference modules/fusion_blocks.py:264-292): the yardstick `mamba_ref` against an
independent implementation, the module's parameter layout and initialisation, and the C ABI declarations.  No GPU."""
import re

import pytest
import torch

import mamba_ref as mr


def _mixer(hidden):
    mm = pytest.importorskip("transformers.models.mamba.modeling_mamba")
    cfg = mm.MambaConfig(hidden_size=hidden, state_size=16, conv_kernel=4, expand=2, num_hidden_layers=1, vocab_size=8)
    return mm.MambaMixer(cfg, layer_idx=0)


def test_mamba_ref_equals_the_transformers_mixer_in_float64():
    torch.manual_seed(5)
    mixer = _mixer(32).double().eval()
    with torch.no_grad():
        for p in mixer.parameters():        # away from any special initial value
            p.add_(0.05 * torch.randn_like(p))
    x = torch.randn(2, 7, 32, dtype=torch.float64)
    with torch.no_grad():
        want = mixer(x)
        got = mr.mamba_ref(x, {k: v.double() for k, v in mixer.state_dict().items()})
    err = (got - want).abs().max().item()
    print(f"mamba_ref vs MambaMixer: max |diff| {err:.3e} on max |ref| {want.abs().max().item():.3e}")
    assert err <= 1e-6 * want.abs().max().item()


def test_ssm_fusion_module_constructs_on_the_cpu():
    from modules.fusion_blocks import SSMFusionModule
    m = SSMFusionModule(768, 64)
    assert m.text_pool == "cls"
    assert tuple(m.txt_proj.weight.shape) == (64, 768)
    assert isinstance(m.pool, torch.nn.AdaptiveAvgPool1d)
    assert m.mamba.d_inner == 128 and m.mamba.dt_rank == 4
    assert SSMFusionModule(768, 64, text_pool="mean").text_pool == "mean"


def test_mamba_state_dict_matches_the_mixer_and_loads_strictly_both_ways():
    from modules.fusion_blocks import SSMFusionModule
    mixer = _mixer(32)
    m = SSMFusionModule(48, 32)
    ours = {k[len("mamba."):]: v for k, v in m.state_dict().items() if k.startswith("mamba.")}
    theirs = mixer.state_dict()
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in theirs.items()}
    assert {k: tuple(v.shape) for k, v in ours.items()} == {
        "A_log": (64, 16), "D": (64,), "in_proj.weight": (128, 32), "conv1d.weight": (64, 1, 4), "conv1d.bias": (64,),
        "x_proj.weight": (34, 64), "dt_proj.weight": (64, 2), "dt_proj.bias": (64,), "out_proj.weight": (32, 64)}
    mixer.load_state_dict(ours, strict=True)
    m.mamba.load_state_dict(theirs, strict=True)
    assert sorted(k for k in m.state_dict() if not k.startswith("mamba.")) == ["txt_proj.bias", "txt_proj.weight"]


def test_mamba_initialisation_follows_the_package():
    from hamspine.nn import Mamba
    torch.manual_seed(0)
    m = Mamba(256)
    assert m.d_inner == 512 and m.dt_rank == 16 and Mamba(40).dt_rank == 3
    assert m.A_log._no_weight_decay is True and m.D._no_weight_decay is True
    assert not hasattr(m.in_proj.weight, "_no_weight_decay")
    assert torch.equal(m.A_log, torch.log(torch.arange(1, 17, dtype=torch.float32)).repeat(512, 1))
    assert torch.equal(m.D, torch.ones(512))
    dt = torch.nn.functional.softplus(m.dt_proj.bias.detach().double())
    assert dt.min().item() >= 1e-4 * (1 - 1e-5) and dt.max().item() <= 1e-1 * (1 + 1e-5)
    assert dt.max().item() / dt.min().item() > 10          # log-uniform over two decades, not one value
    assert m.dt_proj.weight.abs().max().item() <= 16 ** -0.5
    assert m.in_proj.bias is None and m.x_proj.bias is None and m.out_proj.bias is None and m.conv1d.bias is not None


def test_dict_tokens_raise_value_error():
    from modules.fusion_blocks import SSMFusionModule
    m = SSMFusionModule(16, 32)
    tokens = {k: torch.zeros(1, 4, 32) for k in ("layer2", "layer3", "layer4")}
    with pytest.raises(ValueError):
        m(tokens, torch.zeros(1, 3, 16))


def test_vmamba_fusion_still_raises_import_error():
    from modules.fusion_blocks import VMambaFusionModule
    with pytest.raises(ImportError):
        VMambaFusionModule(768, 64)


def test_header_declares_and_binding_lists_the_ssm_entry_points():
    import hamspine._lib as L
    names = ["hs_causal_conv1d_fwd", "hs_causal_conv1d_bwd", "hs_selective_scan_fwd", "hs_selective_scan_bwd"]
    syms = L.exported_symbols()
    header = open(L.HEADER_PATH).read()
    for n in names:
        assert n in syms, n
        assert re.search(r"hs_status\s+" + n + r"\s*\(", header), n
    # each declaration cites the reference lines it implements
    for n in names:
        head = header[:header.index(n + "(")]
        assert "modules/fusion_blocks.py:264-292" in head[head.rindex("/*"):], n
    lib = L.lib()
    for n in names:
        assert hasattr(lib, n) and getattr(lib, n).argtypes, n
