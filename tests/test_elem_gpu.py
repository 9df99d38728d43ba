"""The optimizer, embedding, pooling, packing and small elementwise kernels of csrc/elem.hip, each called directly through the C
ABI on guarded buffers and compared per element with float64 (tests/elem_ref.py).

"Bitwise" is kernel_ref.bits_equal.  "Gated" is kernel_ref.gate: err(gpu) <= max(2 * err(yardstick), floor), max-relative, the
yardstick being the same formula in sequential float32 on the CPU; every gate prints both numbers.  The floor is 1e-6 except for
the update p_new - p_old of the optimizers, where it is the rounding of the stored parameter (elem_ref.update_floor, derived
there from the data alone).  Nothing is tuned against what the GPU returns.  Every call asserts HS_OK and intact guard bands;
refused calls assert that every output still holds its sentinel.

Largest error over the cases of each gated output, as printed by a run on the MI355X: gpu / yardstick / floor, and the case
(records, not thresholds; see MEASURED).  Value-only mutations of the kernels tried on a scratch build, and the first test that
failed on each: eps inside Adam's square root -> test_adam_step (update of n=1023: 9.3e-05 against 4.3e-06); lr instead of
lr / bc1 -> test_adam_step at step 1 and 2 (at step 1000 float32 bc1 is exactly 1); `first` ignored in SGD -> test_sgd_step
with first=1; `>=` in the max-pool scan -> test_maxpool (taps of the "ties" data); src / L for src % L -> test_embed_fwd
(sum_out bitwise); 1 / (Nt + 1) -> test_mean_tokens.
"""
import numpy as np
import pytest
import torch

import elem_ref as er
import kernel_ref as kr

pytestmark = pytest.mark.gpu

from hamspine import _lib as L  # noqa: E402

F32, BF16 = er.F32, er.BF16
REC = {}

MEASURED = """
  adam.update          6.03e-05 / 6.03e-05 / 1.32e-04   dec=1 wd=0.05 step=2 gs=0.125, planted tensor, element 4
  adam.update (n=262151, dec=1 wd=0 step=1 gs=1)  5.94e-06 / 6.24e-06 / 2.54e-06
  adam.exp_avg         6.11e-07 / 6.11e-07              dec=0 wd=0.05 step=1 gs=1 n=1   (1 - beta1 rounded to float32)
  adam.exp_avg_sq      1.28e-05 / 1.28e-05              the g = 1e20 element             (1 - beta2 rounded to float32)
  adam 3 steps         update 6.82e-06 / 6.82e-06 / 4.45e-06, exp_avg 2.26e-07 / 2.26e-07, exp_avg_sq 1.08e-05 / 1.07e-05
  sgd.update           1.73e-06 / 1.73e-06 / 5.34e-06   mom=0.9 nes=1 first=1 wd=0 gs=0.5 n=5;   sgd.buf 7.87e-08 / 7.87e-08
  embed f32            y 1.03e-07 / 2.81e-07, mean 3.61e-08 / 3.61e-08, rstd 3.90e-08 / 3.55e-07, with dropout 1.43e-07 / 2.91e-07,
                       zero-variance row: y 0 / 0, rstd 2.00e-09 / 2.00e-09
  embed bf16           y 3.37e-03 / 3.37e-03, with dropout 2.64e-03 / 2.64e-03, zero-variance row y 2.18e-03 / 2.18e-03,
                       rstd 3.43e-08 / 3.57e-07 (one bf16 rounding of the output; gpu = yardstick)
  embed_bwd (plain)    dword 8.46e-08 / 8.46e-08, dpos 6.69e-08 / 6.69e-08
  mean                 y f32 3.26e-07 / 2.72e-07, bf16 2.99e-03 / 2.99e-03; dx f32 6.62e-08 / 6.62e-08, bf16 3.52e-03 / 3.52e-03
  axpby                f32->f32 5.13e-08 / 7.48e-08, bf16->f32 4.64e-08 / 8.45e-08, f32->bf16 3.08e-03 / 3.08e-03,
                       bf16->bf16 3.24e-03 / 3.24e-03
  gelu_bwd             f32 6.61e-08 / 6.61e-08, bf16 2.14e-03 / 2.14e-03
Everything else is bitwise.
"""


def _T(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _gate(name, tag, gpu, yard, ref, floor=kr.F32_NOISE):
    eg, ey = kr.gate(f"{tag} {name}", _T(gpu), _T(yard), _T(ref), floor=floor)
    if name not in REC or eg > REC[name][0]:
        REC[name] = (eg, ey, max(floor, kr.F32_NOISE), tag)


def _report(prefix):
    for name, (eg, ey, fl, tag) in sorted(REC.items()):
        if name.startswith(prefix):
            print(f"RECORD {name}: {eg:.2e} / {ey:.2e} / {fl:.2e}   {tag}")


def _bits(t, ref, what):
    assert kr.bits_equal(t, _T(ref).to(t.dtype)), f"{what}: differs bitwise"


def _ok(r, what):
    assert r["status"] == 0, f"{what}: status {r['status']}"
    assert r["guards"], f"{what}: a guard band or a skipped lane was written"


UNSUPPORTED = 3          # HS_ERR_UNSUPPORTED: the status of the empty / negative extents refused since this file exists


def _refused(r, what, word=None, status=None):
    assert r["status"] != 0, f"{what}: accepted"
    assert status is None or r["status"] == status, f"{what}: status {r['status']}, expected {status}"
    assert r["untouched"], f"{what}: refused, but an output or a guard band was written"
    with pytest.raises(L.HamspineError):
        L.check(r["status"], what)
    msg = L.lib().hs_last_error().decode("utf-8", "replace")
    assert msg and (word is None or word in msg), f"{what}: hs_last_error() says {msg!r}"


# ======================================================================================================================
# Adam / AdamW
# ======================================================================================================================
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
ADAM_SIZES = (1, 3, 4, 5, 1023, 4096, 262144 + 7, 0)          # 262144 + 7: 256 blocks x 256 lanes x 4 wrap once, tail of 3
PLANTED = "planted"


def _opt_tensor(g, n, off=0, h=0, tag=None):
    return {"p": 4.0 * torch.rand(n, generator=g) - 2.0, "g": torch.randn(n, generator=g), "m": 0.1 * torch.randn(n, generator=g),
            "v": 0.01 * torch.rand(n, generator=g), "buf": torch.randn(n, generator=g), "off": off, "h": h, "tag": tag or f"n={n}"}


def _opt_set(seed, sizes):
    """the sizes, then: every pointer one float off (the scalar path), only the shadow one bf16 element off, a NULL shadow entry
    between non-NULL ones, and the planted tensor -- element 0: p = g = m = v = 0 (the update is 0 / eps = 0, not NaN);
    element 1: g = 1e20, whose square overflows float32 ((1 - beta2) g g, evaluated left to right, does not);
    element 2: g = v = 0 with m = 0.1: the denominator is eps alone (an eps inside the square root would be 1e-4 instead)."""
    g = kr.gen(seed)
    ts = [_opt_tensor(g, n) for n in sizes]
    ts.append(_opt_tensor(g, 1029, off=1, tag="n=1029 all pointers +1"))
    ts.append(_opt_tensor(g, 1029, h=1, tag="n=1029 shadow +1"))
    ts.append(_opt_tensor(g, 77, h=None, tag="n=77 NULL shadow"))
    t = _opt_tensor(g, 8, tag=PLANTED)
    for k in ("p", "g", "m", "v"):
        t[k][0] = 0.0
    t["g"][1] = 1e20
    t["g"][2], t["v"][2], t["m"][2] = 0.0, 0.0, 0.1
    ts.append(t)
    return ts


_SETS = {}


def _cached_set(key, seed, sizes):
    if key not in _SETS:
        _SETS[key] = _opt_set(seed, sizes)
    return _SETS[key]


def _parts(t, n):
    return [slice(j, j + 1) for j in range(n)] if t["tag"] == PLANTED else [slice(None)]


def _gate_state(name, tag, gpu, yard, ref, floor=kr.F32_NOISE):
    gpu, yard, ref = (np.asarray(a, dtype=np.float64) for a in (gpu, yard, ref))
    assert np.isfinite(gpu).all(), f"{tag} {name}: not finite"
    if not ref.any():
        assert not gpu.any(), f"{tag} {name}: the reference is exactly 0, the GPU returned {gpu}"
    else:
        _gate(name, tag, gpu, yard, ref, floor)


def _check_adam(tag, ts, r, hyper, roundings=3):
    for i, t in enumerate(ts):
        n = t["p"].numel()
        if n == 0:
            continue
        ref, yard = er.adam_ref64(t["p"], t["g"], t["m"], t["v"], *hyper), er.adam_yard(t["p"], t["g"], t["m"], t["v"], *hyper)
        p0 = t["p"].double().numpy()
        gp = r["p"][i].double().numpy()
        for sl in _parts(t, n):
            tg = f"{tag} {t['tag']}" + (f" [{sl.start}]" if sl.start is not None else "")
            _gate_state("adam.update", tg, gp[sl] - p0[sl], yard["p"][sl].astype(np.float64) - p0[sl], ref["p"][sl] - p0[sl],
                        er.update_floor(p0[sl], ref["p"][sl], roundings))
            _gate_state("adam.exp_avg", tg, r["m"][i].numpy()[sl], yard["m"][sl], ref["m"][sl])
            _gate_state("adam.exp_avg_sq", tg, r["v"][i].numpy()[sl], yard["v"][sl], ref["v"][sl])
        if r["h"][i] is not None:
            assert kr.bits_equal(r["h"][i], r["p"][i].bfloat16()), f"{tag} {t['tag']}: the shadow is not bf16(p)"


@pytest.mark.parametrize("grad_scale", (1.0, 0.125))
@pytest.mark.parametrize("step", (1, 2, 1000))
@pytest.mark.parametrize("wd", (0.0, 0.05))
@pytest.mark.parametrize("decoupled", (0, 1))
def test_adam_step(decoupled, wd, step, grad_scale):
    ts = _cached_set("adam", 40, ADAM_SIZES)
    hyper = (LR, B1, B2, EPS, wd, step, decoupled, grad_scale)
    tag = f"adam dec={decoupled} wd={wd} step={step} gs={grad_scale}"
    r = er.call_adam(ts, *hyper)
    _ok(r, tag)
    assert r["g_kept"], f"{tag}: a gradient was written"
    assert r["h"][-2] is None and all(h is not None for h in r["h"][:-2])
    _check_adam(tag, ts, r, hyper)
    _report("adam.")


def test_adam_without_shadow_table_is_the_same_step():
    ts = _cached_set("adam", 40, ADAM_SIZES)
    hyper = (LR, B1, B2, EPS, 0.05, 2, 1, 0.125)
    a, b = er.call_adam(ts, *hyper), er.call_adam(ts, *hyper, shadow=False)
    _ok(a, "adam shadow")
    _ok(b, "adam plain")
    for k in ("p", "m", "v"):
        for i, t in enumerate(ts):
            assert kr.bits_equal(a[k][i], b[k][i]), f"hs_adam_step_multi differs from the shadow form: {k} of {t['tag']}"


def test_adam_33_tensors_take_two_launches():
    g = kr.gen(41)
    ts = [_opt_tensor(g, 5 + (7 * i) % 36) for i in range(er.ADAM_MAX + 1)]
    hyper = (LR, B1, B2, EPS, 0.05, 3, 1, 1.0)
    r = er.call_adam(ts, *hyper)
    _ok(r, "adam 33 tensors")
    _check_adam("adam count=33", ts, r, hyper)
    # the last entry alone (count = 32 leaves it as it was)
    r32 = er.call_adam(ts, *hyper, count=er.ADAM_MAX)
    _ok(r32, "adam count=32 of 33")
    assert kr.bits_equal(r32["p"][-1], ts[-1]["p"]) and kr.bits_equal(r32["h"][-1], torch.full_like(r32["h"][-1], kr.SENT))


def test_adam_three_steps_on_its_own_state():
    """the GPU's own p, m, v are fed forward; the float64 sequence never rounds.  Floor of the total update: three stores."""
    g = kr.gen(42)
    ts = [_opt_tensor(g, n) for n in (5, 1023, 4100)] + [_opt_tensor(g, 1029, off=1, tag="n=1029 +1")]
    grads = [[torch.randn(t["p"].numel(), generator=g) for t in ts] for _ in range(3)]
    wd, dec = 0.05, 1
    cur = [dict(t) for t in ts]
    ref = [{k: t[k].double().numpy() for k in ("p", "m", "v")} for t in ts]
    yard = [{k: t[k].numpy() for k in ("p", "m", "v")} for t in ts]
    for k in range(3):
        hyper = (LR, B1, B2, EPS, wd, k + 1, dec, 1.0)
        for i, t in enumerate(cur):
            t["g"] = grads[k][i]
            ref[i] = er.adam_ref64(_T(ref[i]["p"]), t["g"], _T(ref[i]["m"]), _T(ref[i]["v"]), *hyper)
            yard[i] = er.adam_yard(_T(yard[i]["p"]), t["g"], _T(yard[i]["m"]), _T(yard[i]["v"]), *hyper)
        r = er.call_adam(cur, *hyper)
        _ok(r, f"adam sequence step {k + 1}")
        for i, t in enumerate(cur):
            t["p"], t["m"], t["v"] = r["p"][i], r["m"][i], r["v"][i]
    for i, t in enumerate(ts):
        p0 = t["p"].double().numpy()
        tg = f"adam 3 steps {t['tag']}"
        _gate_state("adam3.update", tg, cur[i]["p"].double().numpy() - p0, yard[i]["p"].astype(np.float64) - p0, ref[i]["p"] - p0,
                    er.update_floor(p0, ref[i]["p"], 9))
        _gate_state("adam3.exp_avg", tg, cur[i]["m"].numpy(), yard[i]["m"], ref[i]["m"])
        _gate_state("adam3.exp_avg_sq", tg, cur[i]["v"].numpy(), yard[i]["v"], ref[i]["v"])
    _report("adam3.")


def test_adam_refusals():
    g = kr.gen(43)
    ts = [_opt_tensor(g, 9), _opt_tensor(g, 16)]
    _refused(er.call_adam(ts, LR, B1, B2, EPS, 0.0, 0, 1, 1.0, check=False), "adam step=0", "adam")
    _refused(er.call_adam(ts, LR, B1, B2, EPS, 0.0, 1, 1, 1.0, count=-1, check=False), "adam count=-1", "adam")
    _refused(er.call_adam(ts, LR, B1, B2, EPS, 0.0, 0, 1, 1.0, shadow=False, check=False), "adam (plain) step=0", "adam")


# ======================================================================================================================
# SGD
# ======================================================================================================================
SGD_SIZES = (1, 3, 4, 5, 1023, 4096, 512 * 256 + 5, 0)        # 512 blocks x 256 lanes wrap once
SGD_LR = 0.05


def _check_sgd(tag, ts, r, hyper, momentum):
    for i, t in enumerate(ts):
        n = t["p"].numel()
        if n == 0:
            continue
        ref, yard = er.sgd_ref64(t["p"], t["g"], t["buf"], *hyper), er.sgd_yard(t["p"], t["g"], t["buf"], *hyper)
        p0 = t["p"].double().numpy()
        tg = f"{tag} {t['tag']}"
        _gate_state("sgd.update", tg, r["p"][i].double().numpy() - p0, yard["p"].astype(np.float64) - p0, ref["p"] - p0,
                    er.update_floor(p0, ref["p"], 2))
        if momentum:
            _gate_state("sgd.buf", tg, r["buf"][i].numpy(), yard["buf"], ref["buf"])


def _int_set(seed, sizes):
    g = kr.gen(seed)
    ts = []
    for n, off in [(n, 0) for n in sizes] + [(1029, 1)]:
        ts.append({k: torch.randint(-8, 9, (n,), generator=g).float() for k in ("p", "g", "buf")} | {"off": off, "tag": f"int n={n} +{off}"})
    return ts


@pytest.mark.parametrize("grad_scale", (1.0, 0.5))
@pytest.mark.parametrize("wd", (0.0, 1e-2))
@pytest.mark.parametrize("first", (0, 1))
@pytest.mark.parametrize("nesterov", (0, 1))
@pytest.mark.parametrize("momentum", (0.0, 0.9))
def test_sgd_step(momentum, nesterov, first, wd, grad_scale):
    ts = _cached_set("sgd", 50, SGD_SIZES)[:-1]          # (without the Adam planted tensor)
    hyper = (SGD_LR, momentum, wd, nesterov, first, grad_scale)
    tag = f"sgd mom={momentum} nes={nesterov} first={first} wd={wd} gs={grad_scale}"
    r = er.call_sgd(ts, *hyper, null_buf=momentum == 0)
    _ok(r, tag)
    assert r["g_kept"], f"{tag}: a gradient was written"
    if momentum == 0:
        assert r["buf_kept"], f"{tag}: momentum 0 wrote a buffer"
    _check_sgd(tag, ts, r, hyper, momentum)
    # integer data in [-8, 8], hyper-parameters powers of two: every product and sum is exact, so the result is the float64 one
    if "sgd-int" not in _SETS:
        _SETS["sgd-int"] = _int_set(51, SGD_SIZES)
    ti = _SETS["sgd-int"]
    hi = (0.5, 0.5 if momentum else 0.0, 0.25 if wd else 0.0, nesterov, first, grad_scale)
    ri = er.call_sgd(ti, *hi, null_buf=momentum == 0)
    _ok(ri, tag + " integer")
    for i, t in enumerate(ti):
        ref = er.sgd_ref64(t["p"], t["g"], t["buf"], *hi)
        _bits(ri["p"][i], ref["p"], f"{tag} {t['tag']} p")
        if momentum:
            _bits(ri["buf"][i], ref["buf"], f"{tag} {t['tag']} buf")
    _report("sgd.")


def test_sgd_33_tensors_and_refusal():
    g = kr.gen(52)
    ts = [_opt_tensor(g, 5 + (7 * i) % 36) for i in range(er.ADAM_MAX + 1)]
    hyper = (SGD_LR, 0.9, 1e-2, 1, 0, 1.0)
    r = er.call_sgd(ts, *hyper)
    _ok(r, "sgd 33 tensors")
    _check_sgd("sgd count=33", ts, r, hyper, 0.9)
    _refused(er.call_sgd(ts[:2], SGD_LR, 0.9, 0.0, 0, 0, 1.0, null_buf=True, check=False), "sgd momentum without buffers", "sgd")
    _refused(er.call_sgd(ts[:2], SGD_LR, 0.9, 0.0, 0, 0, 1.0, count=-1, check=False), "sgd count=-1", "sgd")


# ======================================================================================================================
# BERT embeddings
# ======================================================================================================================
EMB_SHAPES = ((5, 5, 4), (7, 3, 260), (9, 4, 768), (4, 4, 1024))      # (tokens, L, H); 260: lane 0 holds chunks 0 and 64
EMB_V = 11
EMB_EPS = 1e-12


def _q8(g, shape, lim):
    """multiples of 2^-8 with |v| <= lim / 256: the three-term sum is exact in float32"""
    return torch.randint(-lim, lim + 1, shape, generator=g).float() / 256.0


def _emb_data(seed, tokens, L, H, V=EMB_V):
    """ids: token 1 holds -3, token 2 holds V + 5 (clamped to rows 0 and V - 1); the last token holds id V - 2, whose table row
    is 0.25 - pos - type0 (|v| <= 1.75): its sum is 0.25 on every h, the variance exactly 0"""
    g = kr.gen(seed)
    ids = torch.randint(0, V, (tokens,), generator=g)
    word, pos, type0 = _q8(g, (V, H), 512), _q8(g, (L, H), 192), _q8(g, (H,), 192)
    gamma, beta = 1.0 + 0.3 * torch.randn(H, generator=g), torch.randn(H, generator=g)
    if tokens >= 4:
        ids[1], ids[2], ids[tokens - 1] = -3, V + 5, V - 2
        word[V - 2] = 0.25 - pos[(tokens - 1) % L] - type0
    return ids, word, pos, type0, gamma, beta


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_embed_fwd(dtype):
    for si, (tokens, L, H) in enumerate(EMB_SHAPES):
        a = _emb_data(60 + si, tokens, L, H)
        ids, word, pos, type0, gamma, beta = a
        dn = er.dname(dtype)
        tag = f"embed tokens={tokens} L={L} H={H} {dn}"
        ref, yard = er.embed_fwd_ref64(*a, L, EMB_EPS, dtype), er.embed_fwd_yard(*a, L, EMB_EPS, dtype)
        r = er.call_embed_fwd(*a, L, EMB_EPS, dtype)
        _ok(r, tag)
        _bits(r["sum"], ref["sum"], tag + " sum_out")
        _gate(f"embed.y[{dn}]", tag, r["y"], yard["y"], ref["y"])
        _gate(f"embed.mean[{dn}]", tag, r["mean"], yard["mean"], ref["mean"])
        t0 = tokens - 1                                     # the zero-variance row: rstd = 1 / sqrt(eps) = 1e6, y == beta
        _gate(f"embed.rstd[{dn}]", tag, r["rstd"][:t0], yard["rstd"][:t0], ref["rstd"][:t0])
        _gate(f"embed.rstd_const_row[{dn}]", tag, r["rstd"][t0:], yard["rstd"][t0:], ref["rstd"][t0:])
        _gate(f"embed.y_const_row[{dn}]", tag, r["y"][t0], yard["y"][t0], beta.double())
        for t, row in ((1, 0), (2, EMB_V - 1)):             # the id clamp
            _bits(r["sum"][t], (word[row].double() + pos[t % L].double() + type0.double()).to(dtype), f"{tag} clamped id of token {t}")
        # dropout: element index t * H + h
        p, seed = 0.1, 0x0123456789ABCDEF
        refd, yardd = er.embed_fwd_ref64(*a, L, EMB_EPS, dtype, p, seed), er.embed_fwd_yard(*a, L, EMB_EPS, dtype, p, seed)
        rd = er.call_embed_fwd(*a, L, EMB_EPS, dtype, p, seed)
        _ok(rd, tag + " dropout")
        keep = torch.from_numpy(er.dropout_keep_ref(seed, np.arange(tokens * H).reshape(tokens, H), p))
        assert torch.equal(rd["y"] == 0, ~keep), f"{tag}: the zeros of y are not the mask of (seed, t * H + h)"
        _gate(f"embed.y_dropout[{dn}]", tag, rd["y"], yardd["y"], refd["y"])
        for k in ("sum", "mean", "rstd"):
            assert kr.bits_equal(rd[k], r[k]), f"{tag}: dropout changed {k}"
    _report("embed.")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_embed_fwd_refusals(dtype):
    for H in (6, 1028):
        a = _emb_data(70, 4, 4, H)
        _refused(er.call_embed_fwd(*a, 4, EMB_EPS, dtype, check=False), f"embed H={H}", "bert_embed")
    a = _emb_data(71, 5, 5, 8)
    for name in ("ids", "word", "pos", "type0", "gamma", "beta", "sum", "y", "mean", "rstd"):
        _refused(er.call_embed_fwd(*a, 5, EMB_EPS, dtype, null=name, check=False), f"embed {name}=NULL", "bert_embed")
    for k in ("tokens", "L", "V"):
        for bad in (0, -1):
            _refused(er.call_embed_fwd(*a, 5, EMB_EPS, dtype, args={k: bad}, check=False), f"embed {k}={bad}", "bert_embed", UNSUPPORTED)


EMB_BWD_SHAPES = ((1, 5, 8, 3), (4, 96, 48, 50), (2, 200, 12, 1), (3, 5120, 8, 17), (1, 15361, 8, 17))     # (B, L, H, V)


def _emb_bwd_ids(g, tokens, V):
    """random ids with -7 and V + 3 planted (clamped); for V >= 4 id V - 2 never occurs"""
    ids = torch.randint(0, V, (tokens,), generator=g)
    if V >= 4:
        ids[ids == V - 2] = V - 3
    if tokens >= 3:
        ids[0], ids[tokens - 1] = -7, V + 3
    return ids


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_embed_bwd(dtype):
    """integer-valued dsum in [-8, 8]: up to 15361 terms stay below 2^24, every order of addition is exact -> all bitwise"""
    for si, (B, Lq, H, V) in enumerate(EMB_BWD_SHAPES):
        g = kr.gen(80 + si)
        tokens = B * Lq
        ids = _emb_bwd_ids(g, tokens, V)
        dsum = torch.randint(-8, 9, (tokens, H), generator=g).to(dtype)
        occurring = int(ids.clamp(0, V - 1)[tokens // 2])
        for pad in (-1, occurring):
            tag = f"embed_bwd B={B} L={Lq} H={H} V={V} pad={pad} {er.dname(dtype)}"
            ref = er.embed_bwd_ref64(ids, dsum, B, Lq, V, pad)
            r = er.call_embed_bwd(ids, dsum, B, Lq, V, pad)
            _ok(r, tag)
            _bits(r["dword"], ref["dword"], tag + " dword")
            _bits(r["dpos"], ref["dpos"], tag + " dpos")
            if pad >= 0:
                assert not r["dword"][pad].any(), f"{tag}: the padding row received a gradient"
            if V >= 4:
                _bits(r["dword"][V - 2], torch.zeros(H), tag + ": the row of an id that does not occur")
        a = er.call_embed_bwd(ids, dsum, B, Lq, V, -1, want_dword=False)
        _ok(a, tag + " dpos alone")
        assert "dword" not in a
        _bits(a["dpos"], ref["dpos"], tag + " dpos alone")
        b = er.call_embed_bwd(ids, dsum, B, Lq, V, -1, want_dpos=False)
        _ok(b, tag + " dword alone")
        _bits(b["dword"], er.embed_bwd_ref64(ids, dsum, B, Lq, V, -1)["dword"], tag + " dword alone")


def test_embed_bwd_ordered_path_is_reproducible():
    B, Lq, H, V = 4, 96, 48, 50
    g = kr.gen(90)
    ids = _emb_bwd_ids(g, B * Lq, V)
    dsum = torch.randn(B * Lq, H, generator=g)
    ref, yard = er.embed_bwd_ref64(ids, dsum, B, Lq, V, -1), er.embed_bwd_yard(ids, dsum, B, Lq, V, -1)
    r1, r2 = er.call_embed_bwd(ids, dsum, B, Lq, V, -1), er.call_embed_bwd(ids, dsum, B, Lq, V, -1)
    _ok(r1, "embed_bwd plain")
    _gate("embed_bwd.dword", "plain data", r1["dword"], yard["dword"], ref["dword"])
    _gate("embed_bwd.dpos", "plain data", r1["dpos"], yard["dpos"], ref["dpos"])
    assert kr.bits_equal(r1["dword"], r2["dword"]) and kr.bits_equal(r1["dpos"], r2["dpos"]), "two runs differ"
    _report("embed_bwd.")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_embed_bwd_refusals(dtype):
    g = kr.gen(91)
    ids, dsum = torch.randint(0, 3, (6,), generator=g), torch.randint(-8, 9, (6, 8), generator=g).to(dtype)
    for args in ({"B": 0}, {"L": 0}, {"B": -1}, {"H": 0}, {"V": 0}):
        _refused(er.call_embed_bwd(ids, dsum, 2, 3, 3, -1, zero=False, args=args, check=False), f"embed_bwd {args}", "bert_embed_bwd", UNSUPPORTED)


# ======================================================================================================================
# max pool
# ======================================================================================================================
POOL_CASES = ((2, 7, 5, 3, 2, 1), (1, 6, 6, 3, 1, 1), (2, 4, 6, 2, 2, 0), (1, 1, 1, 3, 2, 1), (1, 5, 5, 3, 2, 0))      # N H W k s p
POOL_C = {F32: (4, 12), BF16: (8, 24)}


def _pool_x(g, kind, shape, dtype):
    if kind == "ties":
        return torch.randint(-2, 3, shape, generator=g).float().clamp_min(0.0).to(dtype)      # post-ReLU zeros: many exact ties
    return (-1.0 - torch.rand(shape, generator=g)).to(dtype)              # all negative: a padding tap started at 0 would win


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_maxpool(dtype):
    for ci, (N, H, W, k, s, p) in enumerate(POOL_CASES):
        for Cc in POOL_C[dtype]:
            for kind in ("ties", "negative"):
                g = kr.gen(100 + ci)
                tag = f"maxpool N={N} H={H} W={W} C={Cc} k={k} s={s} p={p} {kind} {er.dname(dtype)}"
                x = _pool_x(g, kind, (N, H, W, Cc), dtype)
                y, idx, bwd = er.maxpool_ref(x, k, s, p)
                r = er.call_maxpool_fwd(x, k, s, p)
                _ok(r, tag)
                _bits(r["y"], y.reshape(-1, Cc), tag + " y")
                assert torch.equal(r["idx"], idx.reshape(-1, Cc)), f"{tag}: arg-max taps differ"
                dy = torch.randint(-8, 9, (r["y"].shape[0], Cc), generator=g).to(dtype)
                b = er.call_maxpool_bwd(dy, r["idx"], N, H, W, Cc, k, s, p)
                _ok(b, tag + " bwd")
                _bits(b["dx"], bwd(dy).reshape(-1, Cc), tag + " dx")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_maxpool_refusals(dtype):
    g = kr.gen(110)
    Cc = POOL_C[dtype][0]
    x = _pool_x(g, "ties", (1, 4, 4, Cc), dtype)
    x6 = _pool_x(g, "ties", (1, 4, 4, 6), dtype)
    bad = [("C=6", x6, 3, 2, 1, None), ("ksize=16", x, 16, 2, 8, None), ("stride=0", x, 3, 0, 1, None), ("stride=-2", x, 3, -2, 1, None),
           ("ksize=0", x, 0, 2, 0, None), ("pad=-1", x, 3, 2, -1, None), ("window 7 > padded 4+2", x, 7, 1, 1, None)]
    bad += [(f"{k}={v}", x, 3, 2, 1, {k: v}) for k in ("N", "H", "W", "C") for v in (0, -1)]
    for what, xx, k, s, p, args in bad:
        st = None if what in ("C=6", "ksize=16") else UNSUPPORTED
        _refused(er.call_maxpool_fwd(xx, k, s, p, out_rows=4, args=args, check=False), f"maxpool {what}", "maxpool", st)
        cc = xx.shape[3]
        _refused(er.call_maxpool_bwd(torch.zeros(4, cc, dtype=dtype), torch.zeros(4, cc, dtype=torch.uint8), 1, 4, 4, cc, k, s, p,
                                     args=args, check=False), f"maxpool_bwd {what}", "maxpool_bwd", st)
    for name in ("x", "y", "idx"):
        _refused(er.call_maxpool_fwd(x, 3, 2, 1, null=name, check=False), f"maxpool {name}=NULL", "maxpool")


# ======================================================================================================================
# mean over tokens
# ======================================================================================================================
MEAN_SHAPES = ((1, 1, 8), (3, 197, 8), (2, 49, 768), (2, 5, 520))       # 520: 65 bf16 chunks, one live column in the 2nd block


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_mean_tokens(dtype):
    for si, (B, Nt, H) in enumerate(MEAN_SHAPES):
        g = kr.gen(120 + si)
        x = (torch.randn(B, Nt, H, generator=g) + 0.5).to(dtype)
        for f32 in (0, 1):
            tag = f"mean B={B} Nt={Nt} H={H} {er.dname(dtype)} f32={f32}"
            odt = F32 if f32 else dtype
            dy = torch.randn(B, H, generator=g).to(odt)
            ref, yard = er.mean_tokens_ref64(x, dy), er.mean_tokens_yard(x, dy, odt, dtype)
            r = er.call_mean_tokens_fwd(x, f32)
            _ok(r, tag)
            _gate(f"mean.y[{er.dname(dtype)}]", tag, r["y"], yard["y"], ref["y"])
            b = er.call_mean_tokens_bwd(dy, dtype, Nt, f32)
            _ok(b, tag + " bwd")
            _bits(b["dx"], yard["dx"].reshape(B * Nt, H), tag + " dx = dy * f32(1 / Nt)")
            _gate(f"mean.dx[{er.dname(dtype)}]", tag, b["dx"], yard["dx"].reshape(B * Nt, H), ref["dx"].reshape(B * Nt, H))
    _report("mean.")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_mean_tokens_refusals(dtype):
    H = 6 if dtype == F32 else 12
    x = torch.ones(2, 3, H, dtype=dtype)
    _refused(er.call_mean_tokens_fwd(x, 0, check=False), f"mean H={H}", "mean_tokens")
    _refused(er.call_mean_tokens_bwd(x[:, 0].contiguous(), dtype, 3, 0, check=False), f"mean_bwd H={H}", "mean_tokens_bwd")
    x = torch.ones(2, 3, 8, dtype=dtype)
    for args in ({"B": 0}, {"Nt": 0}):
        _refused(er.call_mean_tokens_fwd(x, 0, args=args, check=False), f"mean {args}", "mean_tokens")
        _refused(er.call_mean_tokens_bwd(x[:, 0].contiguous(), dtype, 3, 0, args=args, check=False), f"mean_bwd {args}", "mean_tokens_bwd")


# ======================================================================================================================
# packing and casts
# ======================================================================================================================
@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_pack_image(dtype):
    H, W, pad = 5, 7, 3
    Hp, Wp = H + 2 * pad, W + 2 * pad + 4
    for Cin in (1, 3, 4):
        x = torch.randn(2, Cin, H, W, generator=kr.gen(130 + Cin))
        r = er.call_pack_image(x, Hp, Wp, pad, dtype)
        _ok(r, f"pack_image Cin={Cin}")
        _bits(r["y"], er.pack_image_ref(x, Hp, Wp, pad, dtype), f"pack_image Cin={Cin} {er.dname(dtype)}")
    x = torch.randn(1, 5, H, W, generator=kr.gen(135))
    _refused(er.call_pack_image(x, Hp, Wp, pad, dtype, check=False), "pack_image Cin=5", "pack_image")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_pack_stem_weight(dtype):
    for K, R, S, Cin in ((5, 7, 7, 3), (2, 3, 8, 4)):
        w = torch.randn(K, R, S, Cin, generator=kr.gen(140 + K))
        r = er.call_pack_stem_weight(w, dtype)
        _ok(r, "pack_stem_weight")
        _bits(r["out"], er.pack_stem_weight_ref(w, dtype), f"pack_stem_weight {(K, R, S, Cin)} {er.dname(dtype)}")
        if dtype == F32:
            u = er.call_unpack_stem_wgrad(r["out"], S, Cin)
            _ok(u, "unpack_stem_wgrad")
            _bits(u["dw"], w, f"unpack(pack(w)) {(K, R, S, Cin)}")
            _bits(u["dw"], er.unpack_stem_wgrad_ref(r["out"], S, Cin), "unpack_stem_wgrad")


def test_cast_multi():
    """sizes 0, 1, 7, 8, 9 and 524288 + 3 (256 blocks x 256 lanes x 8: the last full pass plus a tail), 524288 + 8 + 3 (one chunk
    more: the vector loop wraps), a source one float off at 65536 + 9 elements (the scalar loop wraps); 49 tensors: two launches"""
    g = kr.gen(150)
    sizes = [0, 1, 7, 8, 9, 524288 + 3, 524288 + 11, 65536 + 9] + [1 + (5 * i) % 23 for i in range(er.CAST_MAX + 1 - 8)]
    offs = [0] * len(sizes)
    offs[7] = 1
    srcs = [torch.randn(n, generator=g) for n in sizes]
    special = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, float("inf"), float("-inf"), 3.4028234663852886e38, 1e-40, -0.0,
                            -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20, 3.3961775e38])
    for i in (5, 7, len(sizes) - 1):
        n = min(special.numel(), srcs[i].numel())
        srcs[i][:n] = special[:n]
    srcs[5][-3:] = special[:3]                                   # the scalar tail too
    r = er.call_cast_multi(srcs, offs)
    _ok(r, "cast_multi")
    assert len(srcs) == er.CAST_MAX + 1
    for i, x in enumerate(srcs):
        _bits(r["dst"][i], er.cast_ref(x), f"cast entry {i} n={x.numel()} +{offs[i]}")
    assert er.call_cast_multi([], [])["status"] == 0


# ======================================================================================================================
# small elementwise kernels
# ======================================================================================================================
WRAP_N = 4096 * 256 * 4 + 1203          # 4096 blocks x 256 lanes x 4 floats wrap once; 1203 = 300 chunks + a tail of 3
EW = ((1, 0), (3, 0), (1029, 0), (1029, 1), (WRAP_N, 0))           # (n, element offset of every pointer)


def _ew(g, n, dtype):
    return torch.randn(n, generator=g).to(dtype)


@pytest.mark.parametrize("odt", er.DTYPES, ids=er.dname)
@pytest.mark.parametrize("idt", er.DTYPES, ids=er.dname)
def test_axpby(idt, odt):
    g = kr.gen(160)
    a, b = 0.3, -1.7
    for n, off in EW:
        x, y = _ew(g, n, idt), _ew(g, n, idt)
        tag = f"axpby {er.dname(idt)}->{er.dname(odt)} n={n} +{off}"
        r = er.call_map("hs_axpby", idt, [x, y], off=off, out_dtype=odt, extra=(a, b))
        _ok(r, tag)
        _gate(f"axpby.out[{er.dname(idt)}->{er.dname(odt)}]", tag, r["out"], er.axpby_yard(x, y, a, b, odt), er.axpby_ref64(x, y, a, b))
        if n <= 1029:
            r = er.call_map("hs_axpby", idt, [x, None], off=off, out_dtype=odt, extra=(a, b))
            _ok(r, tag + " y=NULL")
            _bits(r["out"], er.axpby_yard(x, None, a, b, odt), tag + " y=NULL (one product, one rounding)")
    xi, yi = (torch.randint(-8, 9, (1029,), generator=g).to(idt) for _ in range(2))
    r = er.call_map("hs_axpby", idt, [xi, yi], out_dtype=odt, extra=(1.0, 1.0))
    _ok(r, "axpby integers")
    _bits(r["out"], er.axpby_ref64(xi, yi, 1.0, 1.0), f"axpby a=b=1 on integers {er.dname(idt)}->{er.dname(odt)}")
    r = er.call_map("hs_axpby", idt, [xi, yi], n=0, out_dtype=odt, extra=(1.0, 1.0))
    assert r["status"] == 0 and r["untouched"], "axpby n=0 wrote something"
    _refused(er.call_map("hs_axpby", idt, [xi, yi], out_dtype=odt, extra=(1.0, 1.0), null=(0,), check=False), "axpby x=NULL", "axpby")
    _report("axpby.")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_relu(dtype):
    g = kr.gen(170)
    for n, off in EW:
        x, dy = _ew(g, n, dtype), _ew(g, n, dtype)
        if n >= 3:
            x[0], x[1], x[n - 1] = -0.0, 0.0, -0.0
        tag = f"relu {er.dname(dtype)} n={n} +{off}"
        r = er.call_map("hs_relu_fwd", dtype, [x], off=off)
        _ok(r, tag)
        _bits(r["out"], er.relu_ref(x), tag + " fwd")
        y = er.relu_ref(x)
        if n >= 3:
            y[0], dy[2] = -0.0, -0.0
        b = er.call_map("hs_relu_bwd", dtype, [dy, y], off=off)
        _ok(b, tag + " bwd")
        _bits(b["out"], er.relu_bwd_ref(dy, y), tag + " bwd")


def test_mul_dev_scalar():
    g = kr.gen(180)
    s = torch.tensor([0.37])
    for n, off in EW:
        x = _ew(g, n, F32)
        r = er.call_map("hs_mul_dev_scalar", F32, [x, s], off=off)
        _ok(r, f"mul_dev_scalar n={n} +{off}")
        _bits(r["out"], x * s, f"mul_dev_scalar n={n} +{off}")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_dropout(dtype):
    g = kr.gen(190)
    for seed, p in ((1234, 0.1), (0x0123456789ABCDEF, 0.5)):
        masks = []
        for off in (0, 1):
            ones = torch.ones(1029, dtype=dtype)
            r = er.call_map("hs_dropout", dtype, [ones], off=off, extra=(p, seed))
            tag = f"dropout {er.dname(dtype)} p={p} seed={seed:#x} +{off}"
            _ok(r, tag)
            want, keep = er.dropout_ref(ones, p, seed)
            _bits(r["out"], want, tag + " on ones")
            assert torch.equal(r["out"] != 0, keep), tag + ": the mask is not keep(seed, i)"
            masks.append(r["out"] != 0)
        assert torch.equal(masks[0], masks[1]), "the aligned and the offset call draw different masks"
        for n, off in EW:
            if n == WRAP_N and dtype == BF16 and p != 0.1:
                continue
            x = _ew(g, n, dtype)
            r = er.call_map("hs_dropout", dtype, [x], off=off, extra=(p, seed))
            _ok(r, f"dropout n={n}")
            _bits(r["out"], er.dropout_ref(x, p, seed)[0], f"dropout {er.dname(dtype)} n={n} +{off} p={p}: x * f32(1 / (1 - p))")
    x = _ew(g, 1029, dtype)
    r = er.call_map("hs_dropout", dtype, [x], extra=(0.0, 7))
    _ok(r, "dropout p=0")
    _bits(r["out"], x, "dropout p=0 is a copy")
    for p in (1.0, -0.25, 1.5):
        _refused(er.call_map("hs_dropout", dtype, [x], extra=(p, 7), check=False), f"dropout p={p}", "dropout")


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_gelu_bwd(dtype):
    """The measure is max|err| / max|dx| and must stay so: 0.5 (1 + erf(u / sqrt 2)) cancels for u << 0 in float32 (at u = -6 the
    float64 value is 1e-9, the float32 sum 1 + erf is 0 or 6e-8), so no per-element relative bound exists there."""
    g = kr.gen(200)
    u = torch.cat([12.0 * torch.rand(1024, generator=g) - 6.0, torch.tensor([0.0, 10.0, -10.0, 40.0, -40.0])]).to(dtype)
    dy = torch.randn(u.numel(), generator=g).to(dtype)
    ref, yard = er.gelu_bwd_ref64(dy, u), er.gelu_bwd_yard(dy, u, dtype)
    for off in (0, 1):
        tag = f"gelu_bwd {er.dname(dtype)} n={u.numel()} +{off}"
        r = er.call_map("hs_gelu_bwd", dtype, [dy, u], off=off)
        _ok(r, tag)
        assert bool(torch.isfinite(r["out"].float()).all()), tag
        _gate(f"gelu_bwd.dx[{er.dname(dtype)}]", tag, r["out"], yard, ref)
    _report("gelu_bwd.")
