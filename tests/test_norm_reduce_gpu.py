"""LayerNorm, BatchNorm, the attention-fallback softmax and the two-stage column sum, each called directly through the C ABI
and compared with float64 (tests/kernel_ref.py).

Gate: err(gpu) <= max(2 * err(yardstick), 1e-6), the yardstick being the same formula in sequential float32 on the CPU --
max|t - ref| / max|ref| for elementwise outputs, relative L2 for reduced vectors.  Nothing is tuned against what the GPU
returns; every comparison prints both numbers.  Where a result must be exact (integer data, zero padding, guard bands,
dropout masks, repeat runs) it is compared bitwise.  The shapes are the smallest that reach each register layout, loop and
kernel body.

Where the floor is not 1e-6.  Three outputs cancel in float32, so that max|reference| is small against the operands and the
realised error of one float32 evaluation (the yardstick's) says little about another's.  There the floor is the a-priori
rounding bound of the evaluation, computed from the inputs and the float64 reference alone and derived in the docstrings of
kernel_ref.softmax_bwd_floor (dS where one key holds the probability mass: 1.1e-6 measured at Lk = 1024),
kernel_ref.bn_fwd_floors (float32 scale / shift / block means at |mean| / std up to 5000: save_invstd 1.5e-5 .. 3.6e-5 measured
against 3e-7 of the two-pass yardstick, y 2e-4 at M = 2) and kernel_ref.bn_bwd_floor (dx at M = 2, where the three terms cancel
but for eps: 1.3e-6; dgamma in eval mode: 1.3e-6).  The bf16 "one rounding" checks of dx_dropped and P_drop are stated against
the two returned tensors, both of which are rounded: see _one_bf16_rounding.
"""
import pytest
import torch

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from hamspine import _lib as L  # noqa: E402

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
SEED = 0x5EED1234


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def _half_ulp_bf16(v):
    """half the spacing of bf16 (8 significant bits) at |v|: 2^(floor(log2 |v|) - 8), at most 2^-8 |v|"""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 8.0)


def _one_bf16_rounding(what, got, base, keep):
    """got = bf16(v * keep) and base = bf16(v) are roundings of one float32 value v that the kernel does not return.  One bf16
    rounding is 2^-8 relative (8 significant bits), and each output is held to it: v lies within half a bf16 spacing of
    base, and got within half a spacing of the float32 product fl(v * keep), itself within 2^-24 of v * keep, so
    |got - base * keep| <= halfulp(base) * keep + halfulp(got) + 2^-24 |base * keep| (ties are reached: 1.000 of the first
    two terms was measured).
    (Measured against base * keep, which has itself been rounded once, the distance reaches 1.4 * 2^-8 on the MI355X; the
    bound here is the sharpest that the two returned tensors allow.)"""
    want = base.double() * keep.double()
    got = got.double()
    dist, allowed = (got - want).abs(), _half_ulp_bf16(base) * keep.double() + _half_ulp_bf16(got) + kr.EPS32 * want.abs()
    live = want != 0
    print(f"{what}: worst distance {(dist[live] / want.abs()[live]).max().item():.3e} relative, "
          f"{(dist[live] / allowed[live]).max().item():.3f} of the allowed two half-spacings")
    assert bool((dist <= allowed)[live].all())


def _same(a, b, keys):
    for k in keys:
        assert kr.bits_equal(a[k], b[k]), f"{k} differs bitwise"


# ======================================================================================================================
# LayerNorm
# ======================================================================================================================
def _ln_shapes(dtype):
    """(M, H, kind): every register layout NV = 1..4 at its limits and with idle lanes, M not a multiple of 4, 65 partial
    rows (unrolled + remainder loop of the final kernel), the 512-block cap"""
    hs = (8, 504, 512, 520, 768, 1032, 1544, 2048) if dtype == torch.bfloat16 else (4, 252, 256, 260, 768, 1024)
    shapes = [(M, H, "plain") for H in hs for M in (5, 67)]
    shapes += [(M, 768, "plain") for M in (1, 3, 17)]
    shapes += [(1040, 24, "plain"), (8209, 8, "plain"), (5, 768, "tight"), (17, hs[3], "const")]
    return shapes


@DTYPES
def test_layernorm_forward(dtype):
    for i, (M, H, kind) in enumerate(_ln_shapes(dtype)):
        x, _, gamma, beta = kr.ln_data(kr.gen(10 + i), M, H, dtype, kind)
        for eps in (1e-5, 1e-12):
            ref = kr.ln_fwd_ref64(x, gamma, beta, eps)
            yard = kr.ln_fwd_yard(x, gamma, beta, eps, dtype)
            r = kr.call_ln_fwd(x, gamma, beta, eps)
            assert r["guards"]
            for k in ("y", "mean", "rstd"):
                kr.gate(f"ln_fwd {_name(dtype)} M={M} H={H} {kind} eps={eps:g} {k}", r[k], yard[k], ref[k])
            if kind == "const":
                assert kr.bits_equal(r["y"][M // 2].float(), beta.to(dtype).float())          # variance exactly 0: y = beta
        again = kr.call_ln_fwd(x, gamma, beta, eps)
        _same(r, again, ("y", "mean", "rstd"))
        nostats = kr.call_ln_fwd(x, gamma, beta, eps, want_stats=False)      # mean / rstd = NULL is accepted
        assert nostats["guards"]
        _same(r, nostats, ("y",))


def _ln_bwd_inputs(i, M, H, kind, dtype):
    x, dy, gamma, beta = kr.ln_data(kr.gen(40 + i), M, H, dtype, kind)
    f = kr.ln_fwd_ref64(x, gamma, beta, 1e-5)
    return x, dy, gamma, f["mean"].float(), f["rstd"].float()     # the kernel reads float32 statistics: so does the reference


@DTYPES
def test_layernorm_backward(dtype):
    for i, (M, H, kind) in enumerate(_ln_shapes(dtype)):
        x, dy, gamma, mean, rstd = _ln_bwd_inputs(i, M, H, kind, dtype)
        ref = kr.ln_bwd_ref64(dy, x, gamma, mean, rstd)
        yard = kr.ln_bwd_yard(dy, x, gamma, mean, rstd, dtype)
        r = kr.call_ln_bwd(dy, x, gamma, mean, rstd)
        assert r["guards"]
        tag = f"ln_bwd {_name(dtype)} M={M} H={H} {kind}"
        kr.gate(f"{tag} dx", r["dx"], yard["dx"], ref["dx"])
        kr.gate(f"{tag} dgamma", r["dgamma"], yard["dgamma"], ref["dgamma"], reduced=True)
        kr.gate(f"{tag} dbeta", r["dbeta"], yard["dbeta"], ref["dbeta"], reduced=True)
        _same(r, kr.call_ln_bwd(dy, x, gamma, mean, rstd), ("dx", "dgamma", "dbeta"))
        nodx = kr.call_ln_bwd(dy, x, gamma, mean, rstd, want_dx=False)       # dx = NULL: parameter gradients only
        assert nodx["guards"]
        _same(r, nodx, ("dgamma", "dbeta"))
        dyi = kr.int_data(kr.gen(70 + i), M, H, dtype)                       # integer dy: dbeta is exact in any order
        ri = kr.call_ln_bwd(dyi, x, gamma, mean, rstd)
        assert kr.bits_equal(ri["dbeta"], dyi.double().sum(0).float())


@DTYPES
def test_layernorm_backward_pre(dtype):
    """hs_layernorm_bwd_pre: dx * dropout mask (element index row * H + col) and its column sums, next to the plain outputs"""
    p = 0.3
    for i, (M, H, kind) in enumerate(_ln_shapes(dtype)):
        x, dy, gamma, mean, rstd = _ln_bwd_inputs(i, M, H, kind, dtype)
        tag = f"ln_bwd_pre {_name(dtype)} M={M} H={H} {kind}"
        plain = kr.call_ln_bwd(dy, x, gamma, mean, rstd)
        # p = 0
        ref = kr.ln_bwd_ref64(dy, x, gamma, mean, rstd)
        yard = kr.ln_bwd_yard(dy, x, gamma, mean, rstd, dtype)
        r0 = kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, p=0.0, seed=SEED)
        assert r0["guards"]
        _same(plain, r0, ("dx", "dgamma", "dbeta"))
        assert kr.bits_equal(r0["dx_dropped"], r0["dx"])
        kr.gate(f"{tag} p=0 dbias", r0["dbias"], yard["dbias"], ref["dbias"], reduced=True)
        n0 = kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, p=0.0, seed=SEED, want_dxd=False)    # dx_dropped = NULL
        assert n0["guards"]
        _same(r0, n0, ("dx", "dgamma", "dbeta", "dbias"))
        # p = 0.3
        keep = kr.call_dropout_keep(M * H, p, SEED).view(M, H)
        assert 0.2 < (keep == 0).float().mean().item() < 0.4 or M * H < 200
        ref = kr.ln_bwd_ref64(dy, x, gamma, mean, rstd, keep)
        yard = kr.ln_bwd_yard(dy, x, gamma, mean, rstd, dtype, keep)
        r = kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, p=p, seed=SEED)
        assert r["guards"]
        _same(plain, r, ("dx", "dgamma", "dbeta"))
        dx, dxd = r["dx"].float(), r["dx_dropped"].float()
        live = dx != 0
        assert torch.equal((dxd == 0)[live], (keep == 0)[live]), "zeros of dx_dropped are not the zeros of the hs_dropout mask"
        assert bool((dxd[~live] == 0).all())
        if dtype == torch.float32:
            assert kr.bits_equal(dxd, dx * keep)
        else:
            _one_bf16_rounding(f"{tag} dx_dropped vs dx * scale", dxd, dx, keep)
        kr.gate(f"{tag} p={p} dbias", r["dbias"], yard["dbias"], ref["dbias"], reduced=True)
        _same(r, kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, p=p, seed=SEED), ("dx", "dgamma", "dbeta", "dx_dropped", "dbias"))


# ======================================================================================================================
# softmax
# ======================================================================================================================
# (rows, Lk, ldS, ldP): vector bodies with 16 / 32 / 64 lanes per row at and between their limits, the scalar body for
# ldP > 256, Lk % 4 != 0, ldS % 4 != 0, one and three keys, the longest rows
SM_SHAPES = [(5, 4, 4, 8), (17, 60, 60, 64), (33, 64, 64, 64), (9, 68, 72, 72), (9, 128, 128, 128), (7, 132, 132, 136),
             (6, 256, 256, 256), (5, 260, 260, 264), (5, 65, 65, 72), (5, 64, 65, 64), (3, 1, 1, 8), (3, 3, 3, 8),
             (2, 511, 511, 512), (2, 1024, 1024, 1024)]
P_ATT = 0.1


def _vec_ok(Lk, ld_in, ldP):
    return Lk % 4 == 0 and ldP % 4 == 0 and ldP <= 256 and ld_in % 4 == 0


def _scores(g, rows, Lk, kind):
    if kind == "randn":
        return 4.0 * torch.randn(rows, Lk, generator=g)
    S = 80.0 * (2.0 * torch.randint(0, 2, (rows, Lk), generator=g).float() - 1.0)     # +-80, and one 1e4 per row
    S[torch.arange(rows), torch.randint(0, Lk, (rows,), generator=g)] = 1.0e4
    return S


def _check_padding(t_full, Lk):
    pad = t_full[:, Lk:]
    assert kr.bits_equal(pad, torch.zeros_like(pad)), "padding columns are not exactly zero"


def _check_pdrop(tag, P, Pd, keep, dtype):
    P, Pd = P.float(), Pd.float()
    live = P != 0
    assert torch.equal((Pd == 0)[live], (keep == 0)[live]), "zeros of P_drop are not the hs_dropout mask at r * Lk + k"
    if dtype == torch.float32:
        assert kr.bits_equal(Pd, P * keep)
    else:
        _one_bf16_rounding(f"{tag} P_drop vs P / (1 - p)", Pd, P, keep)


@DTYPES
def test_softmax_forward(dtype):
    for i, (rows, Lk, ldS, ldP) in enumerate(SM_SHAPES):
        g = kr.gen(200 + i)
        rpb = -(-rows // 3)                       # three batches share the rows
        mask = kr.softmax_mask(3, Lk, g)
        keep = kr.call_dropout_keep(rows * Lk, P_ATT, SEED).view(rows, Lk)
        for kind in ("randn", "big"):
            S = _scores(g, rows, Lk, kind)
            for m in (mask, None):
                tag = f"softmax_fwd {_name(dtype)} {rows}x{Lk} ldS={ldS} ldP={ldP} {kind} {'mask' if m is not None else 'nomask'}"
                ref = kr.softmax_fwd_ref64(S, m, rpb, keep)
                yard = kr.softmax_fwd_yard(S, m, rpb, dtype, keep)
                bodies = [False, True] if _vec_ok(Lk, ldS, ldP) else [False]     # True: S misaligned -> scalar body
                got = []
                for mis in bodies:
                    r = kr.call_softmax_fwd(S, m, dtype, Lk, ldS, ldP, rpb, p=P_ATT, seed=SEED, want_drop=True, misalign=mis)
                    assert r["guards"]
                    _check_padding(r["P"], Lk)
                    _check_padding(r["P_drop"], Lk)
                    P, Pd = r["P"][:, :Lk], r["P_drop"][:, :Lk]
                    kr.gate(f"{tag} {'scalar' if mis or len(bodies) == 1 else 'vector'} P", P, yard["P"], ref["P"])
                    _check_pdrop(tag, P, Pd, keep, dtype)
                    got.append((P, Pd))
                if m is not None and rows >= 3:
                    b2 = slice(2 * rpb, min(3 * rpb, rows))       # all keys masked: uniform, as the finite fill defines it
                    assert kr.bits_equal(got[0][0][b2].float(), torch.full((b2.stop - b2.start, Lk), 1.0 / Lk).to(dtype).float())
                if len(got) == 2:
                    e = kr.maxrel(got[0][0], got[1][0])
                    print(f"{tag} vector vs scalar: {e:.3e}")
                    assert e <= max(2.0 * kr.maxrel(yard["P"], ref["P"]), kr.F32_NOISE), f"{tag}: bodies differ by {e:.3e}"
                    assert torch.equal(got[0][1] == 0, got[1][1] == 0), "dropout pattern differs between the bodies"
                if kind == "randn" and m is not None:             # no dropout, P_drop = NULL: the same P
                    r0 = kr.call_softmax_fwd(S, m, dtype, Lk, ldS, ldP, rpb)
                    assert r0["guards"] and kr.bits_equal(r0["P"][:, :Lk], got[0][0])


@DTYPES
def test_softmax_forward_misaligned_scores(dtype):
    """a vector-eligible shape whose S starts one float off a 16-byte boundary takes the scalar body"""
    rows, Lk, ldS, ldP = 33, 64, 64, 64
    g = kr.gen(260)
    S = _scores(g, rows, Lk, "randn")
    mask = kr.softmax_mask(3, Lk, g)
    ref = kr.softmax_fwd_ref64(S, mask, 11)
    yard = kr.softmax_fwd_yard(S, mask, 11, dtype)
    r = kr.call_softmax_fwd(S, mask, dtype, Lk, ldS, ldP, 11, misalign=True)
    assert r["guards"]
    kr.gate(f"softmax_fwd {_name(dtype)} misaligned S P", r["P"][:, :Lk], yard["P"], ref["P"])


@DTYPES
def test_softmax_backward(dtype):
    for i, (rows, Lk, ldS, ldP) in enumerate(SM_SHAPES):
        g = kr.gen(300 + i)
        ldG = ldS if ldS != ldP else ldP + 4          # ldG != ldP
        rpb = -(-rows // 3)
        S = _scores(g, rows, Lk, "randn")
        P = kr.softmax_fwd_ref64(S, kr.softmax_mask(3, Lk, g), rpb)["P"].to(dtype)     # what the kernel reads: P rounded
        dP = torch.randn(rows, Lk, generator=g)
        keep = kr.call_dropout_keep(rows * Lk, P_ATT, SEED).view(rows, Lk)
        for p, kp in ((0.0, None), (P_ATT, keep)):
            tag = f"softmax_bwd {_name(dtype)} {rows}x{Lk} ldG={ldG} ldP={ldP} p={p}"
            ref = kr.softmax_bwd_ref64(dP, P, kp)
            yard = kr.softmax_bwd_yard(dP, P, dtype, kp)
            floor = kr.softmax_bwd_floor(dP, P, kp)          # g - dot cancels where one key dominates: see its docstring
            bodies = [False, True] if _vec_ok(Lk, ldG, ldP) else [False]
            got = []
            for mis in bodies:
                r = kr.call_softmax_bwd(dP, P, Lk, ldG, ldP, p=p, seed=SEED, misalign=mis)
                assert r["guards"]
                _check_padding(r["dS"], Lk)
                dS = r["dS"][:, :Lk]
                kr.gate(f"{tag} {'scalar' if mis or len(bodies) == 1 else 'vector'} dS", dS, yard["dS"], ref["dS"], floor=floor)
                got.append(dS)
            if len(got) == 2:
                e = kr.maxrel(got[0], got[1])
                print(f"{tag} vector vs scalar: {e:.3e}")
                assert e <= max(2.0 * kr.maxrel(yard["dS"], ref["dS"]), floor, kr.F32_NOISE), f"{tag}: bodies differ by {e:.3e}"


# ======================================================================================================================
# column sum
# ======================================================================================================================
# (M, N, ld, accumulate, misalign)
CS_CASES = [(1, 8, 8, 0, False), (64, 24, 24, 0, False), (65, 24, 32, 0, False), (64, 24, 24, 1, False),
            (1000, 512, 512, 0, False), (1000, 520, 520, 0, False), (300, 12, 16, 0, False), (20000, 8, 8, 0, False),
            (37, 7, 9, 0, False), (37, 257, 257, 0, False), (37, 1, 3, 0, False), (1000, 512, 512, 0, True),
            (300, 24, 24, 1, True)]


@DTYPES
def test_colsum(dtype):
    for i, (M, N, ld, acc, mis) in enumerate(CS_CASES):
        g = kr.gen(400 + i)
        tag = f"colsum {_name(dtype)} M={M} N={N} ld={ld} acc={acc} {'misaligned' if mis else 'aligned'}"
        prior_i = torch.randint(-100, 101, (N,), generator=g).float() if acc else None
        xi = kr.int_data(g, M, N, dtype)               # integers: the sums are exact in any order, in both bodies
        r = kr.call_colsum(xi, ld, accumulate=acc, prior=prior_i, misalign=mis)
        assert r["guards"], "out beyond N (or before it) was written"
        exact = xi.double().sum(0) + (prior_i.double() if acc else 0.0)
        assert kr.bits_equal(r["out"], exact.float()), f"{tag}: integer sums are not exact (padding leaked, or rows were lost)"
        x = (torch.randn(M, N, generator=g) * 3.0 + 0.25).to(dtype)
        prior = torch.randn(N, generator=g) if acc else None
        ref, yard = kr.colsum_ref64(x, prior), kr.colsum_yard(x, prior)
        r = kr.call_colsum(x, ld, accumulate=acc, prior=prior, misalign=mis)
        assert r["guards"]
        kr.gate(tag, r["out"], yard["out"], ref["out"], reduced=True)
        assert kr.bits_equal(r["out"], kr.call_colsum(x, ld, accumulate=acc, prior=prior, misalign=mis)["out"])


# ======================================================================================================================
# BatchNorm (plain path: partial_rows = 0, stats_done = 0, sums_done = 0)
# ======================================================================================================================
EPS, MOM = 1e-5, 0.1
STATS = ("save_mean", "save_invstd", "scale", "shift")


def _bn_fwd_gate(tag, r, yard, ref, keys, floors):
    """floors: kr.bn_fwd_floors -- the a-priori rounding bounds of float32 scale / shift / y when |mean| >> std"""
    assert r["guards"]
    for k in keys:
        kr.gate(f"{tag} {k}", r[k], yard[k], ref[k], floor=floors.get(k, kr.F32_NOISE))


@DTYPES
def test_batchnorm_forward(dtype):
    for Cc, M, kind, seed in kr.bn_cases(dtype):
        x, res, _, gamma, beta, rm, rv = kr.bn_data(Cc, M, kind, seed, dtype)
        tag = f"bn_fwd {_name(dtype)} C={Cc} M={M} {kind}"
        # training, two calls on one layer
        st = kr.BnState(gamma, beta, rm, rv)
        ref = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, EPS, MOM, 1, 0)
        yard = kr.bn_fwd_yard(x, gamma, beta, rm, rv, EPS, MOM, 1, 0, dtype)
        r1 = kr.call_bn_fwd(x, st, EPS, MOM)
        fl = kr.bn_fwd_floors(x, gamma, beta, ref, 1, EPS)
        _bn_fwd_gate(f"{tag} train", r1, yard, ref, STATS + ("y", "running_mean", "running_var"), fl)
        r2 = kr.call_bn_fwd(x, st, EPS, MOM)
        _same(r1, r2, STATS + ("y",))
        ref2 = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, EPS, MOM, 1, 0, calls=2)
        yard2 = kr.bn_fwd_yard(x, gamma, beta, rm, rv, EPS, MOM, 1, 0, dtype, calls=2)
        _bn_fwd_gate(f"{tag} train, second call", r2, yard2, ref2, ("running_mean", "running_var"), {})
        if kind == "const":
            c = Cc // 2
            assert r1["save_mean"][c].item() == 3.0                                               # variance exactly 0
            assert abs(r1["save_invstd"][c].item() - EPS ** -0.5) <= 1e-6 * EPS ** -0.5
        rn = kr.call_bn_fwd(x, kr.BnState(gamma, beta), EPS, MOM)                  # running_* = NULL is accepted
        assert rn["guards"]
        _same(r1, rn, STATS + ("y",))
        rs = kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), EPS, MOM, want_y=False)   # y = NULL: statistics only
        assert rs["guards"]
        _same(r1, rs, STATS + ("running_mean", "running_var"))
        for relu, rr in ((1, None), (0, res), (1, res)):
            ref = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, EPS, MOM, 1, relu, rr)
            yard = kr.bn_fwd_yard(x, gamma, beta, rm, rv, EPS, MOM, 1, relu, dtype, rr)
            r = kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), EPS, MOM, relu=relu, res=rr)
            _bn_fwd_gate(f"{tag} train relu={relu} res={rr is not None}", r, yard, ref, ("y",),
                         kr.bn_fwd_floors(x, gamma, beta, ref, 1, EPS, rr))
        # eval: from the given running statistics, which stay as they are
        ref = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, EPS, MOM, 0, 1, res)
        yard = kr.bn_fwd_yard(x, gamma, beta, rm, rv, EPS, MOM, 0, 1, dtype, res)
        r = kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), EPS, MOM, training=0, relu=1, res=res)
        _bn_fwd_gate(f"{tag} eval", r, yard, ref, ("save_invstd", "scale", "shift", "y"),
                     kr.bn_fwd_floors(x, gamma, beta, ref, 0, EPS, res))
        assert kr.bits_equal(r["save_mean"], rm) and kr.bits_equal(r["running_mean"], rm) and kr.bits_equal(r["running_var"], rv)


def _bn_bwd_gate(tag, r, yard, ref, floor):
    """floor: kr.bn_bwd_floor -- the three terms of dx cancel (entirely, but for eps, when M = 2)"""
    assert r["guards"]
    kr.gate(f"{tag} dx", r["dx"], yard["dx"], ref["dx"], floor=floor["dx"])
    kr.gate(f"{tag} dgamma", r["dgamma"], yard["dgamma"], ref["dgamma"], reduced=True, floor=floor["dgamma"])
    kr.gate(f"{tag} dbeta", r["dbeta"], yard["dbeta"], ref["dbeta"], reduced=True, floor=floor["dbeta"])


def _relu_mask(y_gpu, ref, yard, pre_abs, tag):
    """the forward's ReLU mask as the kernel sees it (y > 0).  It must agree with the float64 pre-activation's sign outside
    the band in which the yardstick itself cannot decide the sign; the band holds less than 0.1% of the elements."""
    band = kr.bn_relu_band(ref, yard, pre_abs)
    mk = y_gpu.float() > 0
    share = band.double().mean().item()
    bad = ((mk != (ref["pre"] > 0)) & ~band).sum().item()
    print(f"{tag} relu mask: {bad} disagreements outside the band, band share {share:.2e}")
    assert share < 1e-3 and bad == 0
    return mk


@DTYPES
def test_batchnorm_backward(dtype):
    for Cc, M, kind, seed in kr.bn_cases(dtype):
        x, res, dy, gamma, beta, rm, rv = kr.bn_data(Cc, M, kind, seed, dtype)
        for training in (1, 0):
            tag = f"bn_bwd {_name(dtype)} C={Cc} M={M} {kind} {'train' if training else 'eval'}"
            fargs = (x, gamma, beta, rm, rv, EPS, MOM, training, 1)
            fw = kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), EPS, MOM, training=training, relu=1, res=res)
            mean, invstd = fw["save_mean"], fw["save_invstd"]          # the float32 statistics the backward reads
            # no ReLU
            ref = kr.bn_bwd_ref64(dy, x, gamma, mean, invstd, training)
            yard = kr.bn_bwd_yard(dy, x, gamma, mean, invstd, training, dtype)
            r = kr.call_bn_bwd(dy, x, gamma, mean, invstd, training=training)
            _bn_bwd_gate(f"{tag} plain", r, yard, ref, kr.bn_bwd_floor(dy, x, gamma, mean, invstd, training, ref))
            _same(r, kr.call_bn_bwd(dy, x, gamma, mean, invstd, training=training), ("dx", "dgamma", "dbeta"))
            nodx = kr.call_bn_bwd(dy, x, gamma, mean, invstd, training=training, want_dx=False)     # dx = NULL
            assert nodx["guards"]
            _same(r, nodx, ("dgamma", "dbeta"))
            dyi = kr.int_data(kr.gen(seed + 7), M, Cc, dtype)
            ri = kr.call_bn_bwd(dyi, x, gamma, mean, invstd, training=training)
            assert kr.bits_equal(ri["dbeta"], dyi.double().sum(0).float()), f"{tag}: dbeta of integer dy is not exact"
            # ReLU from y, residual: dres = masked dy
            fref = kr.bn_fwd_ref64(*fargs, res)
            pre_abs = kr.bn_fwd_floors(x, gamma, beta, fref, training, EPS, res)["pre_abs"]
            mk = _relu_mask(fw["y"], fref, kr.bn_fwd_yard(*fargs, dtype, res), pre_abs, f"{tag} y")
            ref = kr.bn_bwd_ref64(dy, x, gamma, mean, invstd, training, mk)
            yard = kr.bn_bwd_yard(dy, x, gamma, mean, invstd, training, dtype, mk)
            r = kr.call_bn_bwd(dy, x, gamma, mean, invstd, training=training, relu=1, y=fw["y"], want_dres=True)
            _bn_bwd_gate(f"{tag} relu from y", r, yard, ref, kr.bn_bwd_floor(dy, x, gamma, mean, invstd, training, ref, mk))
            assert kr.bits_equal(r["dres"], torch.where(mk, dy, torch.zeros_like(dy))), f"{tag}: dres is not the masked dy"
            # ReLU recomputed from scale / shift, y = NULL (no residual in the forward)
            fw2 = kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), EPS, MOM, training=training, relu=1)
            fref = kr.bn_fwd_ref64(*fargs)
            pre_abs = kr.bn_fwd_floors(x, gamma, beta, fref, training, EPS)["pre_abs"]
            mk = _relu_mask(fw2["y"], fref, kr.bn_fwd_yard(*fargs, dtype), pre_abs, f"{tag} scale/shift")
            ref = kr.bn_bwd_ref64(dy, x, gamma, mean, invstd, training, mk)
            yard = kr.bn_bwd_yard(dy, x, gamma, mean, invstd, training, dtype, mk)
            r = kr.call_bn_bwd(dy, x, gamma, mean, invstd, training=training, relu=1, scale=fw2["scale"], shift=fw2["shift"])
            _bn_bwd_gate(f"{tag} relu from scale/shift", r, yard, ref, kr.bn_bwd_floor(dy, x, gamma, mean, invstd, training, ref, mk))
            _same(r, kr.call_bn_bwd(dy, x, gamma, mean, invstd, training=training, relu=1, y=fw2["y"]), ("dx", "dgamma", "dbeta"))


# ======================================================================================================================
# refusals: arguments the host code rejects ahead of its first launch
# ======================================================================================================================
def _refused(r, what):
    assert r["status"] != 0, f"{what}: accepted"
    assert r["untouched"], f"{what}: refused, but an output or its guard band was written"
    with pytest.raises(L.HamspineError):
        L.check(r["status"], what)


def test_refusals():
    bf, f32 = torch.bfloat16, torch.float32
    for dtype, H in ((bf, 12), (f32, 6), (bf, 2056), (f32, 1028)):
        x, dy, gamma, beta = kr.ln_data(kr.gen(1), 5, H, dtype)
        _refused(kr.call_ln_fwd(x, gamma, beta, 1e-5, check=False), f"layernorm H={H}")
        mean, rstd = torch.zeros(5), torch.ones(5)
        _refused(kr.call_ln_bwd(dy, x, gamma, mean, rstd, check=False), f"layernorm_bwd H={H}")
        _refused(kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, check=False), f"layernorm_bwd_pre H={H}")
    for dtype in (f32, bf):
        x, dy, gamma, beta = kr.ln_data(kr.gen(2), 37, 64, dtype)
        mean, rstd = torch.zeros(37), torch.ones(37)
        _refused(kr.call_ln_bwd(dy, x, gamma, mean, rstd, ws_short=1, check=False), "layernorm_bwd, workspace one byte short")
        _refused(kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, ws_short=1, check=False), "layernorm_bwd_pre, workspace one byte short")
        _refused(kr.call_ln_bwd(dy, x, gamma, mean, rstd, pre=True, p=1.0, check=False), "layernorm_bwd_pre p=1")
        # softmax
        S = torch.randn(2, 1025)
        _refused(kr.call_softmax_fwd(S, None, dtype, 1025, 1025, 1032, 1, check=False), "softmax Lk=1025")
        _refused(kr.call_softmax_bwd(S, S.to(dtype), 1025, 1025, 1032, check=False), "softmax_bwd Lk=1025")
        S = torch.randn(2, 1024)
        _refused(kr.call_softmax_fwd(S, None, dtype, 1024, 1024, 1032, 1, check=False), "softmax ldP=1032")
        _refused(kr.call_softmax_bwd(S, S.to(dtype), 1024, 1024, 1032, check=False), "softmax_bwd ldP=1032")
        _refused(kr.call_softmax_fwd(torch.randn(2, 64), None, dtype, 64, 64, 64, 1, rows=0, check=False), "softmax rows=0")
        # column sum
        x = torch.randn(1000, 24).to(dtype)
        _refused(kr.call_colsum(x, 24, M=0, check=False), "colsum M=0")
        _refused(kr.call_colsum(x, 24, ws_short=1, check=False), "colsum, workspace one byte short")
        # BatchNorm
        Cc, M = 64, 257
        x, res, dy, gamma, beta, rm, rv = kr.bn_data(Cc, M, "plain", 3, dtype)
        _refused(kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), ws_bytes=8, check=False), "batchnorm, workspace too small")
        mean, invstd = torch.zeros(Cc), torch.ones(Cc)
        _refused(kr.call_bn_bwd(dy, x, gamma, mean, invstd, ws_bytes=8, check=False), "batchnorm_bwd, workspace too small")
        _refused(kr.call_bn_bwd(dy, x, gamma, mean, invstd, relu=1, check=False), "batchnorm_bwd, ReLU without y or scale / shift")
    x, res, dy, gamma, beta, rm, rv = kr.bn_data(12, 65, "plain", 4, bf)
    _refused(kr.call_bn_fwd(x, kr.BnState(gamma, beta, rm, rv), check=False), "batchnorm C=12 in bf16")
    _refused(kr.call_bn_bwd(dy, x, gamma, torch.zeros(12), torch.ones(12), check=False), "batchnorm_bwd C=12 in bf16")
