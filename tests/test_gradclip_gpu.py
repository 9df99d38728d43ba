"""Global gradient-norm clipping on the GPU: the kernels of csrc/gradclip.hip and the _clip step entry points called directly
through the C ABI on guarded buffers against the float64 yardstick of tests/gradclip_ref.py, then the optimizers of
hamspine.optim and the Lightning module on top of them.

The bound on the norm, NORM_TOL = 2^-23 relative, is derived, not measured: the kernels square and add in float64.  A sum of N
non-negative float64 terms added in any order of depth d carries a relative error of at most d 2^-53; here d is a few hundred
(128 fused multiply-adds per thread, an 8-level tree, the slots of the finish launch), so the sum is good to 1e-13, its root
to half of that plus one float64 rounding, and so is the float64 reference.  The one float32 rounding of the root then adds at
most half a unit in the last place, 2^-24 relative; 2^-23 is one whole unit, which also covers the reference's own error and
the double rounding.  (Norms in the float32 subnormal range are not in the data.)  The coefficient is checked bitwise: it is
the stated float32 arithmetic on the float32 norm the kernel wrote.

"Bitwise" is kernel_ref.bits_equal, "gated" kernel_ref.gate with elem_ref.update_floor exactly as tests/test_elem_gpu.py gates
the unclipped steps.  Every call asserts HS_OK and intact guard bands; refused calls assert that every output still holds its
sentinel.
"""
import numpy as np
import pytest
import torch

import elem_ref as er
import gradclip_ref as gr
import kernel_ref as kr

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402

DEV = "cuda"
F32 = torch.float32
TOL = gr.NORM_TOL
MAXT = gr.GRADCLIP_MAX


def _ok(r, what):
    assert r["status"] == 0, f"{what}: status {r['status']}"
    assert r["guards"], f"{what}: a guard band was written"


def _refused(r, what, word, status=1):
    assert r["status"] == status, f"{what}: status {r['status']}, expected {status}"
    assert r["untouched"], f"{what}: refused, but an output or a guard band was written"
    with pytest.raises(L.HamspineError):
        L.check(r["status"], what)
    msg = L.lib().hs_last_error().decode("utf-8", "replace")
    assert word in msg, f"{what}: hs_last_error() says {msg!r}"


def _check_rec(what, r, gs, max_norm, skip=0):
    """rec[0] against float64 to 2^-23, rec[1] bitwise the float32 formula on rec[0], the flags"""
    _ok(r, what)
    assert r["g_kept"], f"{what}: a gradient was written"
    rec = r["rec"].numpy()
    want = gr.norm64(gs)
    print(f"{what}: norm gpu {rec[0]!r} float64 {want!r} rel {abs(float(rec[0]) - want) / max(want, 1e-300):.3e}")
    if want == 0.0:
        assert rec[0] == 0.0 and rec[1] == 1.0, f"{what}: zero gradients gave {rec}"
    else:
        assert abs(float(rec[0]) - want) <= TOL * want, f"{what}: norm {rec[0]!r} against {want!r}"
    assert kr.bits_equal(r["rec"][1:2], torch.tensor([gr.coef(rec[0], max_norm)])), f"{what}: coefficient {rec[1]!r}"
    assert rec[2] == 1.0 and rec[3] == 0.0, f"{what}: flags {rec[2:]}"
    return rec


# ======================================================================================================================
# the norm
# ======================================================================================================================
# (elements, element offset of the pointer).  1029 + 1: a pointer that is only 4-byte aligned; 262151: nine workgroups whose
# shares are no multiple of the block; 70001 + 1 / + 3: several workgroups, each share starting off a 16-byte boundary
NORM_SIZES = [(0, 0), (1, 0), (3, 0), (255, 0), (256, 0), (257, 0), (1023, 0), (1029, 1), (4100, 0), (262151, 0), (70001, 1),
              (70001, 3), (5, 2)]
_DATA = {}


def _grad(n, seed):
    if (n, seed) not in _DATA:
        _DATA[(n, seed)] = torch.randn(n, generator=kr.gen(seed))
    return _DATA[(n, seed)]


@pytest.mark.parametrize("n,off", NORM_SIZES)
def test_norm_of_one_tensor(n, off):
    gs = [_grad(n, 100 + n)]
    what = f"norm n={n} +{off}"
    r = gr.call_norm(gs, 1.0, offs=[off])
    _check_rec(what, r, gs, 1.0)
    again = gr.call_norm(gs, 1.0, offs=[off])
    assert kr.bits_equal(again["rec"], r["rec"]) and kr.bits_equal(again["partials"], r["partials"]), f"{what}: a rerun differs"
    assert r["partials"].numel() == max(1, -(-n // 32768))


@pytest.mark.parametrize("count", (MAXT, MAXT + 1))
def test_norm_of_many_tensors(count):
    """the per-call maximum in one launch; one more: two launches whose partials lie end to end"""
    sizes = [NORM_SIZES[i % len(NORM_SIZES)] for i in range(count - 1)] + [(4100, 1)]
    gs = [_grad(n, 300 + i) for i, (n, _) in enumerate(sizes)]
    offs = [o for _, o in sizes]
    what = f"norm count={count}"
    r = gr.call_norm(gs, 3.0, offs=offs)
    rec = _check_rec(what, r, gs, 3.0)
    assert rec[1] < 1.0
    again = gr.call_norm(gs, 3.0, offs=offs)
    assert kr.bits_equal(again["rec"], r["rec"]) and kr.bits_equal(again["partials"], r["partials"]), f"{what}: a rerun differs"
    # every slot is the float64 sum of squares of its tensor's share; per tensor the slots add up to its own sum
    parts, at = r["partials"].numpy(), 0
    for g in gs:
        k = max(1, -(-g.numel() // 32768))
        want = float((g.double() ** 2).sum())
        assert abs(parts[at:at + k].sum() - want) <= 1e-12 * want, f"{what}: slots {at}..{at + k}"
        at += k
    assert at == parts.size


def test_norm_beyond_the_workgroup_cap():
    """more than 1024 shares of 32768 elements: the shares grow, the grid does not (one tensor, 134 MB)"""
    n = 32768 * 1024 + 4099
    g = torch.empty(n).uniform_(-1.0, 1.0, generator=kr.gen(7))
    r = gr.call_norm([g], 100.0)
    _check_rec("norm n=2^25+4099", r, [g], 100.0)
    assert r["partials"].numel() == 1024


def test_norm_of_zero_gradients():
    gs = [torch.zeros(n) for n in (5, 1029, 40000)]
    r = gr.call_norm(gs, 0.5, offs=[0, 1, 0])
    rec = _check_rec("zero gradients", r, gs, 0.5)
    assert kr.bits_equal(r["rec"], torch.tensor([0.0, 1.0, 1.0, 0.0]))
    assert rec[0] == 0.0


def test_norm_with_a_square_beyond_float32():
    """g = 1e20: its square overflows float32, not float64 -- the norm is finite"""
    g = _grad(4100, 11).clone()
    g[1234] = 1e20
    r = gr.call_norm([g, _grad(257, 12)], 1.0)
    rec = _check_rec("planted 1e20", r, [g, _grad(257, 12)], 1.0)
    assert np.isfinite(rec[0]) and 0.0 < rec[1] < 1.1e-20


@pytest.mark.parametrize("skip", (0, 1))
def test_norm_beyond_the_float32_range(skip):
    """four elements of 3e38: the float64 norm 6e38 exceeds float32 -> inf, coefficient 0, not finite"""
    g = _grad(1023, 13).clone()
    g[[0, 100, 500, 1022]] = 3e38
    r = gr.call_norm([g], 1.0, skip=skip)
    _ok(r, "norm overflow")
    assert kr.bits_equal(r["rec"], torch.tensor([float("inf"), 0.0, 0.0, float(skip)])), r["rec"]
    assert kr.bits_equal(r["rec"], torch.from_numpy(gr.record([g], 1.0, bool(skip))))


@pytest.mark.parametrize("skip", (0, 1))
def test_norm_with_a_nan(skip):
    g = _grad(70001, 14).clone()
    g[40000] = float("nan")
    r = gr.call_norm([_grad(5, 15), g], 1.0, offs=[0, 1], skip=skip)
    _ok(r, "norm nan")
    rec = r["rec"].numpy()
    assert np.isnan(rec[0]) and np.isnan(rec[1]) and rec[2] == 0.0 and rec[3] == float(skip), rec


def test_finish_coefficient_around_max_norm():
    """one slot holding 4.0: the norm is exactly 2.  max_norm below, at, a unit either side of norm + 1e-6, above, inf, 0"""
    f = np.float32
    denom = f(2.0) + f(1e-6)
    cases = [f(2.0) * f(0.999), f(2.0), np.nextafter(denom, f(0)), denom, np.nextafter(denom, f(4)), f(2.0) * f(1.001),
             f(np.inf), f(0.0)]
    for mx in cases:
        r = gr.call_finish(torch.tensor([4.0], dtype=torch.float64), 1, float(mx))
        _ok(r, f"finish max_norm={mx!r}")
        rec = r["rec"].numpy()
        want = gr.coef(f(2.0), mx)
        print(f"finish max_norm={mx!r}: coefficient {rec[1]!r} (formula {want!r})")
        assert rec[0] == 2.0 and kr.bits_equal(r["rec"][1:2], torch.tensor([want])) and rec[2] == 1.0 and rec[3] == 0.0
        assert (rec[1] == 1.0) == bool(mx >= denom), (mx, rec[1])
    # inf / inf follows the arithmetic: NaN
    r = gr.call_finish(torch.tensor([float("inf")], dtype=torch.float64), 1, float("inf"), skip=1)
    rec = r["rec"].numpy()
    assert np.isinf(rec[0]) and np.isnan(rec[1]) and rec[2] == 0.0 and rec[3] == 1.0


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 1000, 9001))
def test_finish_adds_every_slot_once(n):
    parts = torch.rand(n + 3, generator=kr.gen(20 + n), dtype=torch.float64) * 1e3
    r = gr.call_finish(parts, n, float("inf"))
    _ok(r, f"finish n={n}")
    want = float(np.sqrt(parts[:n].numpy().sum()))
    assert abs(float(r["rec"][0]) - want) <= TOL * want and r["rec"][1] == 1.0
    assert kr.bits_equal(gr.call_finish(parts, n, float("inf"))["rec"], r["rec"])


# ======================================================================================================================
# the scale pass
# ======================================================================================================================
def test_scale_multi():
    sizes = NORM_SIZES + [(4100, 1)]
    gs = [_grad(n, 400 + i) for i, (n, _) in enumerate(sizes)]
    offs = [o for _, o in sizes]
    c = np.float32(0.37)
    r = gr.call_scale(gs, [5.0, c, 1.0, 0.0], offs=offs)
    _ok(r, "scale")
    assert r["rec_kept"]
    for g, out, (n, o) in zip(gs, r["g"], sizes):
        assert kr.bits_equal(out, torch.from_numpy(g.numpy() * c)), f"scale n={n} +{o}: not the float32 product"
    # coefficient 1: nothing is written (the read-only copy keeps its bits); a skipped step likewise
    for rec in ([0.1, 1.0, 1.0, 0.0], [float("inf"), 0.0, 0.0, 1.0], [float("nan"), float("nan"), 0.0, 1.0]):
        r = gr.call_scale(gs, rec, offs=offs)
        assert r["status"] == 0 and r["untouched"], f"scale with rec {rec}: a gradient was written"
    # propagate: a NaN coefficient scales, as torch does
    r = gr.call_scale(gs[:3], [float("nan"), float("nan"), 0.0, 0.0])
    _ok(r, "scale nan")
    assert all(torch.isnan(out).all() for out in r["g"])


# ======================================================================================================================
# the fused steps
# ======================================================================================================================
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
STEP_SIZES = (1, 3, 4, 5, 1023, 4096, 262144 + 7, 0)
COEF = float(np.float32(0.37))
REC = [2.7, COEF, 1.0, 0.0]


def _opt_tensor(g, n, off=0, h=0, tag=None):
    return {"p": 4.0 * torch.rand(n, generator=g) - 2.0, "g": torch.randn(n, generator=g), "m": 0.1 * torch.randn(n, generator=g),
            "v": 0.01 * torch.rand(n, generator=g), "buf": torch.randn(n, generator=g), "off": off, "h": h, "tag": tag or f"n={n}"}


def _opt_set():
    if "opt" not in _DATA:
        g = kr.gen(60)
        ts = [_opt_tensor(g, n) for n in STEP_SIZES]
        ts.append(_opt_tensor(g, 1029, off=1, tag="n=1029 all pointers +1"))
        ts.append(_opt_tensor(g, 1029, h=1, tag="n=1029 shadow +1"))
        ts.append(_opt_tensor(g, 77, h=None, tag="n=77 NULL shadow"))
        _DATA["opt"] = ts
    return _DATA["opt"]


def _gate_state(name, tag, gpu, yard, ref, floor=kr.F32_NOISE):
    gpu, yard, ref = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in (gpu, yard, ref))
    assert torch.isfinite(gpu).all(), f"{tag} {name}: not finite"
    kr.gate(f"{tag} {name}", gpu, yard, ref, floor=floor)


@pytest.mark.parametrize("wd,step,grad_scale", ((0.0, 1, 1.0), (0.05, 2, 0.125)))
@pytest.mark.parametrize("decoupled", (0, 1))
def test_adam_clip_step(decoupled, wd, step, grad_scale):
    ts = _opt_set()
    hyper = (LR, B1, B2, EPS, wd, step, decoupled, grad_scale)
    tag = f"adam_clip dec={decoupled} wd={wd} step={step} gs={grad_scale}"
    r = gr.call_adam_clip(ts, *hyper, REC)
    _ok(r, tag)
    assert r["g_kept"], f"{tag}: a gradient or the record was written"
    for i, t in enumerate(ts):
        if t["p"].numel() == 0:
            continue
        ref = gr.adam_clip_ref64(t["p"], t["g"], t["m"], t["v"], *hyper, COEF)
        yard = gr.adam_clip_yard(t["p"], t["g"], t["m"], t["v"], *hyper, COEF)
        p0 = t["p"].double().numpy()
        tg = f"{tag} {t['tag']}"
        _gate_state("update", tg, r["p"][i].double().numpy() - p0, yard["p"].astype(np.float64) - p0, ref["p"] - p0,
                    er.update_floor(p0, ref["p"], 3))
        _gate_state("exp_avg", tg, r["m"][i].numpy(), yard["m"], ref["m"])
        _gate_state("exp_avg_sq", tg, r["v"][i].numpy(), yard["v"], ref["v"])
        if r["h"][i] is not None:
            assert kr.bits_equal(r["h"][i], r["p"][i].bfloat16()), f"{tg}: the shadow is not bf16(p)"
    # the clipped step is not the unclipped one (the coefficient is read)
    plain = er.call_adam(ts, *hyper)
    assert not kr.bits_equal(plain["m"][4], r["m"][4])


@pytest.mark.parametrize("decoupled", (0, 1))
def test_adam_clip_with_coefficient_one_is_the_existing_step_bitwise(decoupled):
    ts = _opt_set()
    hyper = (LR, B1, B2, EPS, 0.05, 2, decoupled, 0.125)
    a, b = er.call_adam(ts, *hyper), gr.call_adam_clip(ts, *hyper, [1e-3, 1.0, 1.0, 0.0])
    _ok(a, "adam")
    _ok(b, "adam_clip coefficient 1")
    for k in ("p", "m", "v", "h"):
        for i, t in enumerate(ts):
            if a[k][i] is not None:
                assert kr.bits_equal(a[k][i], b[k][i]), f"adam_clip with coefficient 1 differs from the existing step: {k} of {t['tag']}"


def test_adam_and_sgd_clip_skip_leave_everything_untouched():
    ts = _opt_set()
    for rec in ([float("inf"), 0.0, 0.0, 1.0], [float("nan"), float("nan"), 0.0, 1.0]):
        r = gr.call_adam_clip(ts, LR, B1, B2, EPS, 0.05, 3, 1, 1.0, rec)
        assert r["status"] == 0 and r["untouched"] and r["g_kept"], f"adam_clip skip {rec}: p, m, v or a shadow was written"
        assert all(kr.bits_equal(h, torch.full_like(h, kr.SENT)) for h in r["h"] if h is not None)
        r = gr.call_sgd_clip(ts, 0.05, 0.9, 1e-2, 1, 0, 1.0, rec)
        assert r["status"] == 0 and r["untouched"] and r["g_kept"], f"sgd_clip skip {rec}: p or a buffer was written"
    # propagate (rec[3] = 0) with an infinite norm: the coefficient 0 makes it a step on a zero gradient
    r = gr.call_adam_clip(ts[:3], LR, B1, B2, EPS, 0.0, 3, 1, 1.0, [float("inf"), 0.0, 0.0, 0.0])
    _ok(r, "adam_clip coefficient 0")
    for i, t in enumerate(ts[:3]):
        assert kr.bits_equal(r["m"][i], torch.from_numpy(np.float32(B1) * t["m"].numpy())), f"coefficient 0: exp_avg of {t['tag']}"


@pytest.mark.parametrize("grad_scale", (1.0, 0.5))
@pytest.mark.parametrize("momentum,nesterov,first", ((0.0, 0, 0), (0.9, 0, 1), (0.9, 0, 0), (0.9, 1, 0), (0.9, 1, 1)))
def test_sgd_clip_step(momentum, nesterov, first, grad_scale):
    ts = _opt_set()
    hyper = (0.05, momentum, 1e-2, nesterov, first, grad_scale)
    tag = f"sgd_clip mom={momentum} nes={nesterov} first={first} gs={grad_scale}"
    r = gr.call_sgd_clip(ts, *hyper, REC, null_buf=momentum == 0)
    _ok(r, tag)
    assert r["g_kept"], f"{tag}: a gradient or the record was written"
    if momentum == 0:
        assert r["buf_kept"], f"{tag}: momentum 0 wrote a buffer"
    for i, t in enumerate(ts):
        if t["p"].numel() == 0:
            continue
        ref, yard = gr.sgd_clip_ref64(t["p"], t["g"], t["buf"], *hyper, COEF), gr.sgd_clip_yard(t["p"], t["g"], t["buf"], *hyper, COEF)
        p0 = t["p"].double().numpy()
        tg = f"{tag} {t['tag']}"
        _gate_state("update", tg, r["p"][i].double().numpy() - p0, yard["p"].astype(np.float64) - p0, ref["p"] - p0,
                    er.update_floor(p0, ref["p"], 2))
        if momentum:
            _gate_state("buf", tg, r["buf"][i].numpy(), yard["buf"], ref["buf"])
    # coefficient 1: the existing entry point's bits
    a = er.call_sgd(ts, *hyper, null_buf=momentum == 0)
    b = gr.call_sgd_clip(ts, *hyper, [9.0, 1.0, 1.0, 0.0], null_buf=momentum == 0)
    _ok(b, tag + " coefficient 1")
    for k in ("p", "buf"):
        for i, t in enumerate(ts):
            assert kr.bits_equal(a[k][i], b[k][i]), f"{tag}: coefficient 1 differs from hs_sgd_step_multi: {k} of {t['tag']}"


def test_clip_steps_of_33_tensors_take_two_launches():
    g = kr.gen(61)
    ts = [_opt_tensor(g, 5 + (7 * i) % 36) for i in range(er.ADAM_MAX + 1)]
    hyper = (LR, B1, B2, EPS, 0.05, 3, 1, 1.0)
    r = gr.call_adam_clip(ts, *hyper, REC)
    _ok(r, "adam_clip 33 tensors")
    t = ts[-1]
    ref, yard = gr.adam_clip_ref64(t["p"], t["g"], t["m"], t["v"], *hyper, COEF), gr.adam_clip_yard(t["p"], t["g"], t["m"], t["v"], *hyper, COEF)
    _gate_state("exp_avg", "adam_clip count=33, the last tensor", r["m"][-1].numpy(), yard["m"], ref["m"])
    r32 = gr.call_adam_clip(ts, *hyper, REC, count=er.ADAM_MAX)
    _ok(r32, "adam_clip count=32 of 33")
    assert kr.bits_equal(r32["p"][-1], t["p"])
    hs = (0.05, 0.9, 1e-2, 1, 0, 1.0)
    r = gr.call_sgd_clip(ts, *hs, REC)
    _ok(r, "sgd_clip 33 tensors")
    ref, yard = gr.sgd_clip_ref64(t["p"], t["g"], t["buf"], *hs, COEF), gr.sgd_clip_yard(t["p"], t["g"], t["buf"], *hs, COEF)
    _gate_state("buf", "sgd_clip count=33, the last tensor", r["buf"][-1].numpy(), yard["buf"], ref["buf"])


# ======================================================================================================================
# refusals: every output keeps its sentinel
# ======================================================================================================================
def test_refusals():
    g = kr.gen(62)
    gs = [torch.randn(9, generator=g), torch.randn(16, generator=g)]
    _refused(gr.call_sumsq(gs, count=-1, check=False), "sumsq count=-1", "grad_sumsq")
    many = [torch.randn(2, generator=g) for _ in range(MAXT + 1)]
    _refused(gr.call_sumsq(many, slots=MAXT + 8, check=False), "sumsq count=max+1", "grad_sumsq")
    for null in ("grads", "n", "partials", ("entry", 1)):
        _refused(gr.call_sumsq(gs, null=null, check=False), f"sumsq NULL {null}", "grad_sumsq")
    _refused(gr.call_sumsq(gs, n_arg=[9, -1], check=False), "sumsq n < 0", "grad_sumsq")
    parts = torch.ones(8, dtype=torch.float64)
    for null in ("partials", "rec"):
        _refused(gr.call_finish(parts, 8, 1.0, null=null, check=False), f"finish NULL {null}", "grad_norm_finish")
    _refused(gr.call_finish(parts, 0, 1.0, check=False), "finish n_partials=0", "grad_norm_finish", status=3)
    _refused(gr.call_finish(parts, -5, 1.0, check=False), "finish n_partials<0", "grad_norm_finish", status=3)
    _refused(gr.call_finish(parts, 8, -1.0, check=False), "finish max_norm<0", "grad_norm_finish")
    _refused(gr.call_finish(parts, 8, float("nan"), check=False), "finish max_norm NaN", "grad_norm_finish")
    rec = [2.0, 0.5, 1.0, 0.0]
    _refused(gr.call_scale(gs, rec, count=-1, check=False), "scale count=-1", "grad_scale")
    _refused(gr.call_scale(many, rec, check=False), "scale count=max+1", "grad_scale")
    for null in ("grads", "n", "rec"):
        _refused(gr.call_scale(gs, rec, null=null, check=False), f"scale NULL {null}", "grad_scale")
    _refused(gr.call_scale(gs, rec, n_arg=[-2, 16], check=False), "scale n < 0", "grad_scale")
    ts = [_opt_tensor(g, 9), _opt_tensor(g, 16)]
    A = (LR, B1, B2, EPS, 0.0)
    _refused(gr.call_adam_clip(ts, *A, 1, 1, 1.0, rec, null="rec", check=False), "adam_clip NULL rec", "adam_clip")
    _refused(gr.call_adam_clip(ts, *A, 0, 1, 1.0, rec, check=False), "adam_clip step=0", "adam")
    _refused(gr.call_adam_clip(ts, *A, 1, 1, 1.0, rec, count=-1, check=False), "adam_clip count=-1", "adam")
    for null in ("p", "g", "m", "v", "n"):
        _refused(gr.call_adam_clip(ts, *A, 1, 1, 1.0, rec, null=null, check=False), f"adam_clip NULL {null}", "adam_clip")
    S = (0.05, 0.9, 0.0, 0, 0, 1.0)
    _refused(gr.call_sgd_clip(ts, *S, rec, null="rec", check=False), "sgd_clip NULL rec", "sgd_clip")
    _refused(gr.call_sgd_clip(ts, *S, rec, null_buf=True, check=False), "sgd_clip momentum without buffers", "sgd")
    _refused(gr.call_sgd_clip(ts, *S, rec, count=-1, check=False), "sgd_clip count=-1", "sgd")
    for null in ("p", "g", "n"):
        _refused(gr.call_sgd_clip(ts, *S, rec, null=null, check=False), f"sgd_clip NULL {null}", "sgd_clip")


# ======================================================================================================================
# the optimizers
# ======================================================================================================================
@pytest.fixture()
def f32_mode():
    hamspine.set_compute_dtype("f32")
    try:
        yield
    finally:
        hamspine.set_compute_dtype("bf16")


DIMS = (24, 40, 16, 8)


class _Stack(torch.nn.Module):
    """three hamspine.nn.Linear layers with GELU between them, and one layer that the forward never uses"""

    def __init__(self):
        super().__init__()
        from hamspine.nn import Linear
        self.l1, self.l2, self.l3 = (Linear(a, b) for a, b in zip(DIMS[:-1], DIMS[1:]))
        self.unused = Linear(8, 8)

    def forward(self, x):
        return self.l3(self.l2(self.l1(x, act="gelu"), act="gelu"))


def _stack_data(step):
    g = kr.gen(70 + step)
    return 2.0 * torch.randn(16, DIMS[0], generator=g), torch.randint(0, DIMS[-1], (16,), generator=g)


def _groups(m, **kw):
    used = [m.l1, m.l2, m.l3]
    return [dict(params=[l.weight for l in used], weight_decay=0.05, **kw),
            dict(params=[l.bias for l in used] + list(m.unused.parameters()), weight_decay=0.0, lr=2e-2)]


def _new_stack():
    torch.manual_seed(5)
    return _Stack()


def _backward(m, step):
    from hamspine import functional as F
    x, y = _stack_data(step)
    for p in m.parameters():
        p.grad = None
    loss = 4.0 * F.cross_entropy(m(x.to(DEV)), y.to(DEV))
    loss.backward()


def _ref64_trajectory(steps, max_norm):
    """the same stack in float64 on the CPU: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW"""
    import torch.nn.functional as TF
    m = _new_stack().double()
    opt = torch.optim.AdamW(_groups(m), lr=1e-2)
    norms = []
    for s in range(steps):
        x, y = _stack_data(s)
        opt.zero_grad(set_to_none=True)
        h = TF.gelu(TF.linear(x.double(), m.l1.weight, m.l1.bias))
        h = TF.gelu(TF.linear(h, m.l2.weight, m.l2.bias))
        (4.0 * TF.cross_entropy(TF.linear(h, m.l3.weight, m.l3.bias), y)).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for p in m.parameters() if p.grad is not None], max_norm)))
        opt.step()
    return m, norms


def _grads64(m):
    return [p.grad.detach().cpu() for p in m.parameters() if p.grad is not None]


def test_fused_adamw_with_max_grad_norm_against_the_torch_route(f32_mode):
    from hamspine.optim import FusedAdamW
    MAX = 0.5
    ref, ref_norms = _ref64_trajectory(3, MAX)
    a, b = _new_stack().to(DEV), _new_stack().to(DEV)
    p0 = {k: v.detach().cpu().clone() for k, v in a.named_parameters()}
    oa = FusedAdamW(_groups(a), lr=1e-2, max_grad_norm=MAX)
    ob = FusedAdamW(_groups(b), lr=1e-2)
    assert oa.grad_norm is None
    for s in range(3):
        _backward(a, s)
        _backward(b, s)
        assert a.unused.weight.grad is None and a.unused.bias.grad is None
        before = [p.grad.detach().clone() for p in a.parameters() if p.grad is not None]
        want = gr.norm64(_grads64(a))
        oa.step()
        tn = torch.nn.utils.clip_grad_norm_(b.parameters(), MAX)
        ob.step()
        torch.cuda.synchronize()
        # the record: the float64 norm of the gradients (the unused layer has none: it is left out), the stated coefficient
        got, c, fin = float(oa.grad_norm), oa.grad_clip_coef, float(oa.grad_finite)
        print(f"step {s}: grad_norm {got!r} float64 {want!r} torch-route {float(tn)!r} float64-model {ref_norms[s]!r} coef {float(c)!r}")
        assert oa.grad_norm.is_cuda and oa.grad_norm.shape == () and oa.grad_norm.dtype == F32
        assert abs(got - want) <= TOL * want and fin == 1.0
        assert kr.bits_equal(c.reshape(1), torch.tensor([gr.coef(np.float32(got), MAX)])) and float(c) < 1.0
        assert abs(float(tn) - want) <= 1e-5 * want
        # .grad is left unscaled (the torch route scaled b's)
        for g0, g1 in zip(before, [p.grad for p in a.parameters() if p.grad is not None]):
            assert kr.bits_equal(g0, g1), "the fused route changed .grad"
    assert float(oa.state[a.l1.weight]["step"]) == 3
    # a parameter without a gradient: out of the norm (above) and out of the update
    for k in ("unused.weight", "unused.bias"):
        assert kr.bits_equal(dict(a.named_parameters())[k].detach(), p0[k]) and not oa.state[dict(a.named_parameters())[k]]
    # the parameters of the two routes agree within the gate: error of the fused route against the float64 trajectory
    # <= max(2 x the torch route's error, the rounding floor of three stored steps)
    pa, pb, pr = dict(a.named_parameters()), dict(b.named_parameters()), dict(ref.named_parameters())
    for k in pa:
        if k.startswith("unused"):
            continue
        z = p0[k].double().numpy()
        r64 = pr[k].detach().numpy()
        floor = er.update_floor(z, r64, 9)
        kr.gate(f"3 steps {k}", torch.from_numpy(pa[k].detach().cpu().double().numpy() - z),
                torch.from_numpy(pb[k].detach().cpu().double().numpy() - z), torch.from_numpy(r64 - z), floor=floor)


def test_skip_mode_keeps_parameters_and_moments(f32_mode):
    from hamspine.optim import FusedAdam, FusedSGD
    for make in (lambda m: FusedAdam(_groups(m), lr=1e-2, max_grad_norm=0.5, nonfinite="skip"),
                 lambda m: FusedSGD(_groups(m, lr=1e-2), momentum=0.9, max_grad_norm=0.5, nonfinite="skip")):
        m = _new_stack().to(DEV)
        o = make(m)
        _backward(m, 0)
        o.step()
        assert float(o.grad_finite) == 1.0 and float(o.grad_clip_coef) < 1.0
        _backward(m, 1)
        m.l2.weight.grad[3, 5] = float("inf")
        keep = {k: v.detach().clone() for k, v in m.named_parameters()}
        state = {k: {n: t.clone() for n, t in o.state[p].items() if torch.is_tensor(t) and t.is_cuda} for k, p in m.named_parameters()}
        o.step()
        torch.cuda.synchronize()
        assert float(o.grad_finite) == 0.0 and np.isinf(float(o.grad_norm)) and float(o.grad_clip_coef) == 0.0
        for k, p in m.named_parameters():
            assert kr.bits_equal(p.detach(), keep[k]), f"{type(o).__name__} skip: {k} was written"
            for n, t in state[k].items():
                assert kr.bits_equal(o.state[p][n], t), f"{type(o).__name__} skip: {n} of {k} was written"
        if isinstance(o, FusedAdam):
            assert float(o.state[m.l1.weight]["step"]) == 2          # a skipped step still counts: the counter is a host integer
        # the next finite step goes on
        _backward(m, 2)
        o.step()
        assert float(o.grad_finite) == 1.0 and not kr.bits_equal(m.l1.weight.detach(), keep["l1.weight"])
        assert all(torch.isfinite(p).all() for p in m.parameters())
    # propagate (the default): the infinite norm gives coefficient 0 -- a step on zero gradients, as on the torch route
    m = _new_stack().to(DEV)
    o = FusedSGD(_groups(m, lr=1e-2), max_grad_norm=0.5)
    _backward(m, 0)
    m.l2.weight.grad[3, 5] = float("inf")
    keep = m.l3.bias.detach().clone()
    o.step()
    assert float(o.grad_clip_coef) == 0.0 and kr.bits_equal(m.l3.bias.detach(), keep)          # bias group: no weight decay


@pytest.mark.parametrize("nesterov", (False, True))
def test_sgd_skip_on_the_first_momentum_step(f32_mode, nesterov):
    """The first batch has an infinite norm: the launch that would have seeded the momentum buffers is skipped on the device.
    The buffers must then hold nothing that reaches the parameters: the next, finite step equals, bit for bit, the first step
    of a fresh optimizer on the same gradients (and so does the step after it).  Also a parameter whose FIRST gradient arrives
    on a skipped step later on (an unused layer, an expert without tokens)."""
    from hamspine.optim import FusedSGD
    kw = dict(momentum=0.9, nesterov=nesterov, max_grad_norm=0.5, nonfinite="skip")
    a, b = _new_stack().to(DEV), _new_stack().to(DEV)
    oa, ob = FusedSGD(_groups(a, lr=5e-2), **kw), FusedSGD(_groups(b, lr=5e-2), **kw)
    p0 = {k: v.detach().clone() for k, v in a.named_parameters()}
    _backward(a, 0)
    a.l1.weight.grad[2, 3] = float("inf")
    oa.step()
    torch.cuda.synchronize()
    assert float(oa.grad_finite) == 0.0
    for k, p in a.named_parameters():
        assert kr.bits_equal(p.detach(), p0[k]), f"skipped first step: {k} was written"
        if p.grad is not None:
            assert not oa.state[p]["momentum_buffer"].any(), f"skipped first step: the buffer of {k} is not zero"
    for s in (1, 2):
        _backward(a, s)
        _backward(b, s)
        if s == 2:          # the unused layer gets its first gradient on a step that is skipped ...
            for m in (a, b):
                m.unused.weight.grad = torch.full_like(m.unused.weight, 0.25)
            a.l2.bias.grad[1] = float("nan")
            keep = {k: v.detach().clone() for k, v in a.named_parameters()}
            oa.step()
            assert float(oa.grad_finite) == 0.0
            for k, p in a.named_parameters():
                assert kr.bits_equal(p.detach(), keep[k]), f"skipped step: {k} was written"
            _backward(a, s)          # ... and the same batch again, finite
            a.unused.weight.grad = torch.full_like(a.unused.weight, 0.25)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        assert float(oa.grad_finite) == 1.0 and kr.bits_equal(oa.grad_norm.reshape(1), ob.grad_norm.reshape(1))
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.isfinite(p).all(), k
            assert kr.bits_equal(p.detach(), q.detach()), f"step {s} after a skipped seeding step: {k} differs from a fresh optimizer"
            if p.grad is not None:
                assert kr.bits_equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"]), f"step {s}: buffer of {k}"
    assert not kr.bits_equal(a.unused.weight.detach(), p0["unused.weight"])


def test_fused_sgd_with_max_grad_norm_against_the_torch_route(f32_mode):
    from hamspine.optim import FusedSGD
    a, b = _new_stack().to(DEV), _new_stack().to(DEV)
    oa = FusedSGD(_groups(a, lr=5e-2), momentum=0.9, nesterov=True, max_grad_norm=float("inf"))
    ob = FusedSGD(_groups(b, lr=5e-2), momentum=0.9, nesterov=True)
    for s in range(2):          # monitor only: the coefficient is 1 and the steps are those of the plain optimizer, bit for bit
        _backward(a, s)
        _backward(b, s)
        want = gr.norm64(_grads64(a))
        oa.step()
        ob.step()
        assert float(oa.grad_clip_coef) == 1.0 and abs(float(oa.grad_norm) - want) <= TOL * want
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert kr.bits_equal(p.detach(), q.detach()), f"monitor-only step {s}: {k}"
    with pytest.raises(hamspine.HamspineError, match="grad_scale"):
        oa.step(grad_scale=0.5)


def test_clip_grad_norm_in_front_of_muon(f32_mode):
    """the stand-alone function on the parameters of a MuonWithAuxAdam set-up: scales in place, then the optimizer steps"""
    from hamspine.optim import MuonWithAuxAdam, clip_grad_norm_
    g = kr.gen(80)
    shapes = [(300, 7), (64, 3, 3, 3), (128, 64, 1, 1), (40,), (5,)]
    ts = [torch.randn(*s, generator=g) for s in shapes]
    ts[1] = ts[1].contiguous(memory_format=torch.channels_last)
    params = [torch.nn.Parameter(t.to(DEV)) for t in ts]
    opt = MuonWithAuxAdam([dict(params=[p for p in params if p.ndim >= 2], use_muon=True, lr=0.05, momentum=0.9, weight_decay=0.1),
                           dict(params=[p for p in params if p.ndim < 2], use_muon=False, lr=1e-2, betas=(0.9, 0.95), eps=1e-10,
                                weight_decay=0.05)])
    assert opt.max_grad_norm is None and opt.grad_norm is None
    grads = [torch.randn(*s, generator=g) for s in shapes]
    grads[1] = grads[1].contiguous(memory_format=torch.channels_last)
    for p, x in zip(params[:-1], grads[:-1]):          # the last parameter has no gradient
        p.grad = x.to(DEV)
    want = gr.norm64(grads[:-1])
    norm = clip_grad_norm_(params, 0.5)
    assert norm.is_cuda and norm.shape == () and abs(float(norm) - want) <= TOL * want
    c = gr.coef(np.float32(float(norm)), 0.5)
    for p, x in zip(params[:-1], grads[:-1]):
        assert p.grad.stride() == x.stride()
        assert kr.bits_equal(p.grad.cpu(), torch.from_numpy(x.numpy() * c)), "clip_grad_norm_ did not scale by the float32 product"
    again = clip_grad_norm_(params, 0.5)          # the norm of the clipped gradients
    assert abs(float(again) - 0.5) <= 1e-5
    before = [p.detach().clone() for p in params]
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in params)
    assert all(not torch.equal(p.detach(), q) for p, q in zip(params[:-1], before[:-1])) and torch.equal(params[-1].detach(), before[-1])
    # error_if_nonfinite: raises before scaling, as torch does; without it the NaN coefficient scales
    params[0].grad[0, 0] = float("inf")
    keep = params[3].grad.clone()
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(params, 0.5, error_if_nonfinite=True)
    assert kr.bits_equal(params[3].grad, keep)
    n = clip_grad_norm_(params, 0.5)
    assert np.isinf(float(n)) and not params[3].grad.any()          # coefficient 0, as torch


# ======================================================================================================================
# the Lightning module
# ======================================================================================================================
def test_lightning_module_takes_gradient_clip_val(f32_mode, tmp_path):
    import golden_cases as gc
    from oracle.procedural import load_procedural
    from ConNexT.models.pl_model_MOE2 import Model4AAAI_MoE
    from hamspine.optim import FusedAdam
    dirs = (gc.save_bert_dir(gc.MIBF_BERT, str(tmp_path / "bert768")), gc.save_convnext_dir(gc.CONNEXT_CFG, str(tmp_path / "convnext")))
    cfg = {"model": {"num_classes": 5, "moe": {"balance_weight": 0.01}, "pretrained_path": dirs[1], "bert_path": dirs[0]},
           "train": {"gradient_clip_val": 0.5}}
    m = Model4AAAI_MoE(learning_rate=3e-4, config=cfg)
    load_procedural(m.net.net, gc.SEED + 310)
    m = m.to(DEV).train()
    images, ids, mask, labels = [t.to(DEV) for t in gc.connext_inputs()]
    batch = {"imgs": images, "texts": {"input_ids": ids, "attention_mask": mask}, "labels": labels}
    opts, _ = m.configure_optimizers()
    assert isinstance(opts[0], FusedAdam) and opts[0].max_grad_norm == 0.5 and opts[0].nonfinite == "propagate"
    assert "max_grad_norm" not in opts[0].param_groups[0] and "max_grad_norm" not in opts[0].state_dict()
    m.training_step(batch, 0).backward()
    want = gr.norm64([p.grad for p in m.parameters() if p.grad is not None])
    before = m.net.net.fc.weight.detach().clone()
    opts[0].step()
    torch.cuda.synchronize()
    got = float(opts[0].grad_norm)
    print(f"lightning step: grad_norm {got!r} float64 {want!r} coef {float(opts[0].grad_clip_coef)!r}")
    assert abs(got - want) <= TOL * want and float(opts[0].grad_finite) == 1.0
    after = m.net.net.fc.weight.detach()
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    # without the key nothing changes: the optimizer carries no setting
    cfg2 = {"model": cfg["model"], "train": {}}
    m.hparams["config"] = cfg2
    assert m.configure_optimizers()[0][0].max_grad_norm is None
