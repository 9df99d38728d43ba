"""Mamba / SSM fusion on the GPU (reference modules/fusion_blocks.py:264-292) against tests/mamba_ref.py in float64.

Gates: f32 mode, outputs <= 1e-4 * max|ref| and every gradient <= 1e-3 in relative L2 norm;
bf16 mode, outputs <= 3e-2 * max|ref| and gradients <= 5e-2 in relative L2 norm.  A_log and dt_proj.bias
come from the real initialiser, so dt and the decays are in their working range."""
import ctypes as C
import os

import pytest
import torch

import mamba_ref as mr

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import rt, ssm  # noqa: E402

DEV = "cuda"


def _chunk():
    return int(L.lib().hs_selective_scan_chunk_len())


def _scan_shapes():
    lc = _chunk()
    return [(1, 1, 64), (2, 49, 128), (3, 7, 80), (2, lc + 1, 64), (1, 2 * lc + 3, 128)]


SHAPE_IDS = ["1x1x64", "2x49x128", "3x7x80", "2x(Lc+1)x64", "1x(2Lc+3)x128"]


@pytest.fixture
def f32_mode():
    hamspine.set_compute_dtype("f32")
    yield
    hamspine.set_compute_dtype("bf16")


def _rel(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def _maxrel(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _scan_inputs(B, Lt, d, seed):
    """float64 CPU leaves laid out as the module lays them out: z is the right half of the (B, L, 2d) in_proj output, Bm / Cm
    the halves of the (B, L, 32) copy of the x_proj output's tail; the per-channel parameters come from Mamba's initialiser."""
    from hamspine.nn import Mamba
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    blk = Mamba(d // 2)
    t = {
        "u": torch.randn(B, Lt, d, generator=g),
        "dt": 0.5 * torch.randn(B, Lt, d, generator=g),
        "xz": torch.randn(B, Lt, 2 * d, generator=g),
        "bc": torch.randn(B, Lt, 32, generator=g),
        "A_log": blk.A_log.detach() + 0.1 * torch.randn(d, 16, generator=g),
        "D": blk.D.detach() + 0.3 * torch.randn(d, generator=g),
        "dt_bias": blk.dt_proj.bias.detach().clone(),
        "w": torch.randn(B, Lt, d, generator=g),
    }
    return {k: v.double() for k, v in t.items()}


def _scan_run(t, d, dtype=torch.float32, device=DEV):
    """forward + backward of the scan on `device`: the HIP kernels on the GPU, mamba_ref's loop on the CPU"""
    acts = ("u", "dt", "xz", "bc", "w")
    if device == "cpu":
        leaf = {k: v.clone().requires_grad_(k != "w") for k, v in t.items()}
    else:
        leaf = {k: v.to(device, dtype if k in acts else torch.float32).requires_grad_(k != "w") for k, v in t.items()}
    z = leaf["xz"][..., d:]
    if device == "cpu":
        out = mr.scan_ref(leaf["u"], leaf["dt"], leaf["dt_bias"], leaf["A_log"], leaf["bc"][..., :16], leaf["bc"][..., 16:],
                          leaf["D"], z)
    else:
        out = ssm.selective_scan(leaf["u"], leaf["dt"], leaf["dt_bias"], leaf["A_log"], leaf["bc"], leaf["D"], z)
    (out * leaf["w"]).sum().backward()
    grads = {k: leaf[k].grad for k in ("u", "dt", "xz", "bc", "A_log", "D", "dt_bias")}
    return out.detach(), grads


@pytest.mark.parametrize("shape", range(5), ids=SHAPE_IDS)
def test_selective_scan_f32_against_float64(shape, f32_mode):
    B, Lt, d = _scan_shapes()[shape]
    t = _scan_inputs(B, Lt, d, 100 + shape)
    ref_out, ref_g = _scan_run(t, d, device="cpu")
    out, g = _scan_run(t, d)
    torch.cuda.synchronize()
    e = _maxrel(out, ref_out)
    print(f"scan {B}x{Lt}x{d}: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" for k in g})
    assert e <= 1e-4
    assert torch.count_nonzero(g["xz"][..., :d]).item() == 0        # the xs half of the in_proj output gets nothing from the scan
    for k in g:
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


def _conv_inputs(B, Lt, d, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    conv = torch.nn.Conv1d(d, d, 4, groups=d, padding=3)
    return {"xz": torch.randn(B, Lt, 2 * d, generator=g).double(), "weight": conv.weight.detach().double(),
            "bias": conv.bias.detach().double(), "w": torch.randn(B, Lt, d, generator=g).double()}


def _conv_run(t, d, device=DEV):
    dt = torch.float64 if device == "cpu" else torch.float32
    leaf = {k: v.detach().clone().to(device=device, dtype=dt).requires_grad_(k != "w") for k, v in t.items()}
    xs = leaf["xz"][..., :d]
    fn = mr.conv_ref if device == "cpu" else ssm.causal_conv1d
    out = fn(xs, leaf["weight"], leaf["bias"])
    (out * leaf["w"]).sum().backward()
    return out.detach(), {k: leaf[k].grad for k in ("xz", "weight", "bias")}


@pytest.mark.parametrize("shape", range(5), ids=SHAPE_IDS)
def test_causal_conv1d_f32_against_float64(shape, f32_mode):
    B, Lt, d = _scan_shapes()[shape]
    t = _conv_inputs(B, Lt, d, 200 + shape)
    ref_out, ref_g = _conv_run(t, d, device="cpu")
    out, g = _conv_run(t, d)
    torch.cuda.synchronize()
    scale = ref_out.abs().max().item()
    head = (out[:, :3].double().cpu() - ref_out[:, :3]).abs().max().item() / scale      # steps that see the zero left padding
    e = _maxrel(out, ref_out)
    print(f"conv {B}x{Lt}x{d}: out {e:.2e} head {head:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" for k in g})
    assert head <= 1e-4
    assert e <= 1e-4
    ghead = (g["xz"][:, :3, :d].double().cpu() - ref_g["xz"][:, :3, :d]).abs().max().item() / ref_g["xz"].abs().max().item()
    assert ghead <= 1e-4
    for k in g:
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


# ---------------------------------------------------------------------------------------------------- module
_MODULE_CASES = [(2, 49, 64, "cls"), (2, 49, 64, "mean"), (3, 5, 40, "cls"), (3, 5, 40, "mean")]
_module_cache = {}


def _module_case(B, Lt, H, pool):
    """seeded module + inputs + the float64 reference (outputs, parameter and input gradients), computed once per case"""
    key = (B, Lt, H, pool)
    if key in _module_cache:
        return _module_cache[key]
    from modules.fusion_blocks import SSMFusionModule
    torch.manual_seed(300 + B + Lt + H)
    m = SSMFusionModule(24, H, text_pool=pool)
    with torch.no_grad():      # generic values where the initialiser gives constants; A_log and dt_proj.bias stay as initialised
        m.mamba.D.add_(0.3 * torch.randn_like(m.mamba.D))
    g = torch.Generator().manual_seed(301)
    img = torch.randn(B, Lt, H, generator=g)
    txt = torch.randn(B, 6, 24, generator=g)
    w = torch.randn(B, H, generator=g)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    img64, txt64 = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    params = {k[len("mamba."):]: v for k, v in sd.items() if k.startswith("mamba.")}
    ref = mr.fusion_ref(img64, txt64, sd["txt_proj.weight"], sd["txt_proj.bias"], params, pool)
    (ref * w.double()).sum().backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads["image_tokens"], grads["text_tokens"] = img64.grad, txt64.grad
    _module_cache[key] = (m, img, txt, w, ref.detach(), grads)
    return _module_cache[key]


def _module_run(m, img, txt, w, dtype):
    import copy
    m = copy.deepcopy(m).to(DEV).train()
    a = img.to(DEV, dtype).requires_grad_(True)
    b = txt.to(DEV, dtype).requires_grad_(True)
    out = m(a, b)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(w.shape)
    (out * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m.named_parameters()}
    grads["image_tokens"], grads["text_tokens"] = a.grad, b.grad
    return out.detach(), grads


@pytest.mark.parametrize("case", _MODULE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_ssm_fusion_module_f32(case, f32_mode):
    m, img, txt, w, ref, ref_g = _module_case(*case)
    out, g = _module_run(m, img, txt, w, torch.float32)
    e = _maxrel(out, ref)
    print(f"module f32 {case}: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" for k in ref_g})
    assert e <= 1e-4
    for k in ref_g:
        assert g[k] is not None, k
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


@pytest.mark.parametrize("case", _MODULE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_ssm_fusion_module_bf16(case):
    hamspine.set_compute_dtype("bf16")
    m, img, txt, w, ref, ref_g = _module_case(*case)
    out, g = _module_run(m, img, txt, w, torch.bfloat16)
    e = _maxrel(out, ref)
    print(f"module bf16 {case}: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" for k in ref_g})
    assert e <= 3e-2
    for k in ref_g:
        assert g[k] is not None, k
        assert _rel(g[k], ref_g[k]) <= 5e-2, k


# ---------------------------------------------------------------------------------------- determinism, causality
def test_scan_forward_and_backward_repeat_bitwise(f32_mode):
    B, Lt, d = 2, _chunk() + 1, 128
    t = _scan_inputs(B, Lt, d, 400)
    out1, g1 = _scan_run(t, d)
    out2, g2 = _scan_run(t, d)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    c1 = _conv_run(_conv_inputs(B, Lt, d, 401), d)
    c2 = _conv_run(_conv_inputs(B, Lt, d, 401), d)
    assert torch.equal(c1[0], c2[0]) and all(torch.equal(c1[1][k], c2[1][k]) for k in c1[1])


@pytest.mark.parametrize("t_cut", ["1", "Lc"])
def test_scan_is_causal(t_cut, f32_mode):
    lc = _chunk()
    cut = 1 if t_cut == "1" else lc
    B, Lt, d = 2, 2 * lc + 3, 64
    t = _scan_inputs(B, Lt, d, 500)
    base, _ = _scan_run(t, d)
    g = torch.Generator().manual_seed(501)
    t2 = dict(t)
    for k in ("u", "dt", "xz", "bc"):
        v = t[k].clone()
        v[:, cut:] = torch.randn(v[:, cut:].shape, generator=g).double()
        t2[k] = v
    other, _ = _scan_run(t2, d)
    torch.cuda.synchronize()
    assert torch.equal(base[:, :cut], other[:, :cut])
    assert not torch.equal(base[:, cut:], other[:, cut:])


# ------------------------------------------------------------------------------------------------ end to end
def test_mamba_fusion_model_trains_end_to_end(tmp_path, f32_mode):
    import golden_cases as gc
    import model as product_model
    from hamspine import functional as F
    from hamspine.optim import FusedAdamW
    torch.manual_seed(600)
    bert = gc.save_bert_dir(gc.TINY_BERT, os.path.join(str(tmp_path), "bert"))
    m = product_model.MultimodalBaselineModel(pretrained_image=False, image_weights_path=None, text_model_name=bert,
                                              fusion_type="mamba", classifier_type="mlp", **gc.E2E_COMMON)
    m = m.to(DEV).train()
    images, ids, mask, labels, _ = gc.e2e_inputs()
    images, ids, mask, labels = images.to(DEV), ids.to(DEV), mask.to(DEV), labels.to(DEV)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = F.cross_entropy(m.classifier(m.forward_features(images, ids, mask)), labels)
        loss.backward()
        if step == 0:
            for p in (m.fusion.mamba.A_log, m.fusion.mamba.D):
                assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(l == l and abs(l) < float("inf") for l in losses)
    assert losses[2] < losses[0]
    m.eval()
    with_grad = m.classifier(m.forward_features(images, ids, mask)).detach()
    with torch.no_grad():
        without = m.classifier(m.forward_features(images, ids, mask))
    assert not without.requires_grad
    assert (with_grad - without).abs().max().item() <= 1e-4 * with_grad.abs().max().item()


# ------------------------------------------------------------------------------------------------ argument checks
def _status_and_message(fn, *args):
    st = fn(*args)
    return st, L.lib().hs_last_error().decode()


def test_unsupported_arguments_are_refused_without_a_launch():
    lib = L.lib()
    B, Lt, d = 1, 4, 64
    x = torch.zeros(B, Lt, d, device=DEV)
    bc = torch.zeros(B, Lt, 32, device=DEV)
    par = torch.zeros(d, 16, device=DEV)
    out = torch.full((B, Lt, d), 7.0, device=DEV)
    p = rt.p

    def scan(n_state, length):
        return _status_and_message(lib.hs_selective_scan_fwd, L.HS_F32, p(x), d, p(x), d, p(par), p(par), p(bc), p(bc, 64), 32,
                                   p(par), p(x), d, p(out), d, None, B, length, d, n_state, rt.stream())

    def conv(k, length, ldx=d):
        return _status_and_message(lib.hs_causal_conv1d_fwd, L.HS_F32, p(x), ldx, p(par), p(par), p(out), d, B, length, d, k,
                                   rt.stream())
    for st, msg in (scan(8, Lt), scan(16, 0), conv(3, Lt), conv(4, 0), conv(4, Lt, ldx=d + 1)):
        assert st == 3 and msg, (st, msg)          # HS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))      # nothing ran
    with pytest.raises(L.HamspineError, match="d_state 8"):
        ssm.selective_scan(x, x, par[:, 0].contiguous(), par[:, :8].contiguous(), bc[..., :16].contiguous(), par[:, 0].contiguous(), x)
