"""The loss kernels (cross entropy, focal, softmax entropy, row KL, MP-Loss, SupCon, KAN regularisation), the LSTM / GRU
cells and the KAN features, each called directly through the C ABI and compared with float64 (tests/head_ref.py).

Gate: err(gpu) <= max(2 * err(yardstick), 1e-6), the yardstick being the same formula in sequential float32 on the CPU with
__expf modelled as exp2(fl32(log2(e) x)) -- max|t - ref| / max|ref| for elementwise outputs, relative error for scalars.
Nothing is tuned against what the GPU returns; every comparison prints both numbers.  Exact results are compared bitwise:
a repeat of every call (the kernels are single-block or fixed-order), outputs with optional pointers NULL against the full
call, and values that must be exactly 0 (C = 1, a label class leading by 200, SupCon without positives, bases outside the
grid).  Every output sits in a guard band that must stay untouched, in refused calls too.  The cases are those of
head_ref.*_cases(): the smallest shapes that reach every strided loop and every clamp.

Where the floor is not 1e-6.  Some outputs cancel in float32, so that the realised error of one float32 evaluation says
little about another's; there the floor is the a-priori rounding bound derived in the docstring of the *_floors helper,
from the inputs and the float64 reference alone:
  ce_floors / focal_floors   lse - z[y] of a confidently right row with large |z| (logits shifted by 1e4: |lse| u = 6e-4 absolute)
  kl_rows_floors             lp - lq with p within 1e-4 of q
  mp_floors                  the same inside the symmetric KL and its gradient (lp - lq + 1 - q / p vanishes at p = q)
  entropy_floors             t_c - sum_k p_k t_k where one class holds the mass
  supcon_floors              s_ij - max_j s_ij with near-duplicate rows, and 1 / T magnifying the error of the dot products
  lstm_bwd_floors / gru_bwd_floors   1 - g, 1 - g^2 of gates saturated to within a few float32 spacings of 1
  kan_reg_floors             log A - S / A and log(l / A) + E for a single row, where the entropy is 0
Errors measured on the MI355X for these outputs (records, not thresholds): see MEASURED below.
"""
import pytest
import torch

import head_ref as hr
import kernel_ref as kr

pytestmark = pytest.mark.gpu

from hamspine import _lib as L  # noqa: E402

# Largest errors over the cases of each output that takes an a-priori floor, as printed by a run on the MI355X: gpu / yardstick /
# floor of that case.  Records, not thresholds.  "vacuous": cases whose floor is 1e-2 or more -- a single saturated row or
# element whose reference output all but vanishes (|ent| of 1e-8, a gradient of 1e-30), so that any bound relative to it
# exceeds 1; there the GPU's error equalled the yardstick's, and the other cases carry the comparison.
MEASURED = """
  ce      loss      7.30e-05 / 7.28e-05 / 6.36e-04   B=33 C=2 logits + 1e4                         (49 cases floored, 0 vacuous)
  ce      row_loss  1.98e-04 / 1.98e-04 / 2.73e-04   B=33 C=2 logits + 1e4                         (22, 0)
                    4.90e-06 / 4.90e-06 / 6.40e-06   B=33 C=130 logits + 1e4, s=0.1: the closest any case came to its floor
  focal   loss      1.29e-04 / 1.29e-04 / 3.00e-04   B=1 C=7 gamma=1.5 logits + 1e4                (26, 0)
  focal   dlogits   2.28e-04 / 2.28e-04 / 2.93e-04   B=600 C=7 gamma=2 logits + 1e4                (25, 0)
  entropy ent       1.08e-06 / 1.09e-06 / 3.66e-05   rows=4 C=7 saturated                          (25, 7)
  entropy dlogits   3.95e-06 / 3.95e-06 / 1.99e-04   rows=9 C=7 saturated                          (20, 2)
  kl      out, dp   1.13e-07 / 5.52e-07, 3.04e-07 / 1.54e-07: no case's floor exceeded 1e-6
  mp      loss      1.08e-07 / 1.08e-07 / 2.21e-06   B=7 C=2 disagreeing towers                    (15, 0)
  mp      d_image   7.87e-07 / 6.84e-07 / 7.81e-05   B=1 C=7 agreeing towers                       (13, 3: margin cases, 5.44e-04 = yardstick)
  mp      d_text    1.53e-06 / 1.16e-06 / 5.35e-05   B=256 C=12 margin                             (13, 0)
  mp      d_fused   2.73e-07 / 9.03e-07 / 6.85e-06   B=256 C=12 margin                             (15, 0)
  supcon  loss      5.75e-07 / 3.41e-07 / 9.72e-05   B=5 D=65 T=0.07                               (22, 2)
  supcon  dfeat     1.86e-06 / 2.76e-06 / 1.40e-03   B=256 D=3 T=0.5 one singleton class           (20, 1)
                    3.68e-06 / 9.34e-07 / 2.93e+01   B=5 D=65 T=0.07 bit-identical rows (the vacuous one)
  kan_reg loss, dw  2.82e-05 / 2.42e-08 / 1.12e-03   rows=1 coeffs=8 (entropy 0: log A - S / A cancels; the yardstick's two logs
                                                     happen to cancel exactly)                      (8 and 6, 0)
  lstm    dgates    1.15e-07 / 1.15e-07 / 1.25e-06   B=3 H=33 pre-activations * 40                 (14, 3)
  lstm    dc_prev   9.62e-08 / 1.24e-07 / 1.04e-06   B=5 H=128                                     (4, 0)
  gru     dgx, dgh  3.93e-08 / 3.93e-08 / 1.35e-06, 1.02e-07 / 1.02e-07 / 6.64e-06   pre-activations * 40   (4 each, 0)
Without a floor (1e-6): ce dlogits 1.90e-07 / 3.21e-07, kl dq 5.22e-08 / 5.22e-08, lstm h, c, act at most 1.42e-07 / 1.51e-07,
gru h, act at most 1.59e-07 / 2.92e-07, kan feat 2.70e-07 / 2.27e-07, kan dx 1.47e-06 / 2.15e-06.
"""


def _same(a, b, keys, what):
    for k in keys:
        assert kr.bits_equal(a[k], b[k]), f"{what}: {k} differs bitwise"


def _zero(t):
    return bool((t == 0).all())


def _refused(r, what):
    assert r["status"] != 0, f"{what}: accepted"
    assert r["untouched"], f"{what}: refused, but an output or its guard band was written"
    with pytest.raises(L.HamspineError):
        L.check(r["status"], what)


# ======================================================================================================================
# cross entropy
# ======================================================================================================================
def test_cross_entropy():
    for c in hr.ce_cases():
        z, y, w, s, tag = c["z"], c["y"], c["weight"], c["s"], c["tag"]
        B, Cn = z.shape
        ref, yard = hr.ce_ref64(z, y, w, s), hr.ce_yard(z, y, w, s)
        fl = hr.ce_floors(z, y, w, s, ref)
        r = hr.call_ce(z, y, w, s)
        assert r["guards"], tag
        kr.gate(f"{tag} loss", r["loss"], yard["loss"], ref["loss"], reduced=True, floor=fl["loss"])
        kr.gate(f"{tag} row_loss", r["row_loss"], yard["row_loss"], ref["row_loss"], floor=fl["row_loss"])
        kr.gate(f"{tag} dlogits", r["dlogits"], yard["dlogits"], ref["dlogits"])
        _same(r, hr.call_ce(z, y, w, s), ("loss", "row_loss", "dlogits"), tag + " repeat")
        nod = hr.call_ce(z, y, w, s, want_d=False)                 # dlogits = NULL
        assert nod["guards"]
        _same(r, nod, ("loss", "row_loss"), tag + " dlogits NULL")
        nor = hr.call_ce(z, y, w, s, want_rows=False)              # row_loss = NULL
        assert nor["guards"]
        _same(r, nor, ("loss", "dlogits"), tag + " row_loss NULL")
        if Cn == 1:
            assert _zero(r["loss"]) and _zero(r["row_loss"]) and _zero(r["dlogits"]), tag + ": C = 1 is not exactly 0"
        if c["margin_row"] is not None and s == 0.0:               # p is exactly 1: the row's loss and gradient are exactly 0
            m = c["margin_row"]
            assert _zero(r["row_loss"][m]) and _zero(r["dlogits"][m]), tag + ": the margin row is not exactly 0"


# ======================================================================================================================
# focal loss
# ======================================================================================================================
def test_focal_loss():
    for c in hr.focal_cases():
        z, y, w, gamma, tag = c["z"], c["y"], c["weight"], c["gamma"], c["tag"]
        B, Cn = z.shape
        ref, yard = hr.focal_ref64(z, y, w, gamma), hr.focal_yard(z, y, w, gamma)
        fl = hr.focal_floors(z, y, w, gamma, ref)
        r = hr.call_focal(z, y, w, gamma)
        assert r["guards"], tag
        kr.gate(f"{tag} loss", r["loss"], yard["loss"], ref["loss"], reduced=True, floor=fl["loss"])
        kr.gate(f"{tag} dlogits", r["dlogits"], yard["dlogits"], ref["dlogits"], floor=fl["dlogits"])
        _same(r, hr.call_focal(z, y, w, gamma), ("loss", "dlogits"), tag + " repeat")
        nod = hr.call_focal(z, y, w, gamma, want_d=False)
        assert nod["guards"]
        _same(r, nod, ("loss",), tag + " dlogits NULL")
        if gamma == 0.0:                                           # plain CE, against the CE reference
            ce = hr.ce_ref64(z, y, w, 0.0)
            scale = 1.0 if w is None else w.double()[y].sum().item() / B
            kr.gate(f"{tag} loss vs CE", r["loss"], yard["loss"], ce["loss"] * scale, reduced=True, floor=fl["loss"])
            kr.gate(f"{tag} dlogits vs CE", r["dlogits"], yard["dlogits"], ce["dlogits"] * scale, floor=fl["dlogits"])
        if Cn == 1:
            assert _zero(r["loss"]) and _zero(r["dlogits"]), tag + ": C = 1 is not exactly 0"
        if c["margin_row"] is not None:                            # ce = 0, p = 1: the gradient row is exactly 0 for every gamma here
            assert _zero(r["dlogits"][c["margin_row"]]), tag + ": the margin row is not exactly 0"


# ======================================================================================================================
# softmax entropy
# ======================================================================================================================
def test_softmax_entropy():
    for c in hr.entropy_cases():
        z, g, tag = c["z"], c["g"], c["tag"]
        ref, yard = hr.entropy_ref64(z, g), hr.entropy_yard(z, g)
        fl = hr.entropy_floors(z, g, ref)
        r = hr.call_entropy(z, g)
        assert r["guards"], tag
        kr.gate(f"{tag} ent", r["ent"], yard["ent"], ref["ent"], floor=fl["ent"])
        kr.gate(f"{tag} dlogits", r["dlogits"], yard["dlogits"], ref["dlogits"], floor=fl["dlogits"])
        _same(r, hr.call_entropy(z, g), ("ent", "dlogits"), tag + " repeat")
        fwd = hr.call_entropy(z)                                   # g = dlogits = NULL
        assert fwd["guards"]
        _same(r, fwd, ("ent",), tag + " forward only")
        bwd = hr.call_entropy(z, g, want_ent=False)                # ent = NULL
        assert bwd["guards"]
        _same(r, bwd, ("dlogits",), tag + " ent NULL")


# ======================================================================================================================
# row KL
# ======================================================================================================================
def test_kl_rows():
    for c in hr.kl_cases():
        p, q, w, eps, tag = c["p"], c["q"], c["w"], c["eps"], c["tag"]
        ref, yard = hr.kl_rows_ref64(p, q, eps, w), hr.kl_rows_yard(p, q, eps, w)
        fl = hr.kl_rows_floors(p, q, eps, w, ref)
        r = hr.call_kl_rows(p, q, eps, w, want_out=True, want_dp=True, want_dq=True)
        assert r["guards"], tag
        kr.gate(f"{tag} out", r["out"], yard["out"], ref["out"], floor=fl["out"])
        kr.gate(f"{tag} dp", r["dp"], yard["dp"], ref["dp"], floor=fl["dp"])
        kr.gate(f"{tag} dq", r["dq"], yard["dq"], ref["dq"])
        e32 = torch.tensor(eps, dtype=torch.float32)
        for t, k in ((p, "dp"), (q, "dq")):                        # the clamp passes the gradient on both bounds, and only there
            on = (t == 1.0) | (t == e32)
            assert bool((r[k][on] != 0).all()), f"{tag}: {k} is 0 on a clamp bound"
            assert _zero(r[k][(t > 1.0) | (t < e32)]), f"{tag}: {k} is not 0 where the clamp is active"
        _same(r, hr.call_kl_rows(p, q, eps, w, want_out=True, want_dp=True, want_dq=True), ("out", "dp", "dq"), tag + " repeat")
        o = hr.call_kl_rows(p, q, eps)                             # out only (w = NULL)
        assert o["guards"]
        _same(r, o, ("out",), tag + " out only")
        d = hr.call_kl_rows(p, q, eps, w, want_out=False, want_dp=True, want_dq=True)
        assert d["guards"]
        _same(r, d, ("dp", "dq"), tag + " out NULL")
        d = hr.call_kl_rows(p, q, eps, w, want_out=False, want_dp=True)
        assert d["guards"]
        _same(r, d, ("dp",), tag + " dp only")


# ======================================================================================================================
# MP-Loss
# ======================================================================================================================
def test_mp_loss():
    for c in hr.mp_cases():
        zi, zt, zf, y, tag = c["zi"], c["zt"], c["zf"], c["y"], c["tag"]
        ref, yard = hr.mp_ref64(zi, zt, zf, y), hr.mp_yard(zi, zt, zf, y)
        fl = hr.mp_floors(zi, zt, zf, y, ref)
        r = hr.call_mp(zi, zt, zf, y)
        assert r["guards"], tag
        kr.gate(f"{tag} loss", r["loss"], yard["loss"], ref["loss"], reduced=True, floor=fl["loss"])
        for k in ("d_image", "d_text", "d_fused"):
            kr.gate(f"{tag} {k}", r[k], yard[k], ref[k], floor=fl[k])
        _same(r, hr.call_mp(zi, zt, zf, y), ("loss", "d_image", "d_text", "d_fused"), tag + " repeat")
        lo = hr.call_mp(zi, zt, zf, y, want_d=False)               # d_image = NULL: the loss only
        assert lo["guards"]
        _same(r, lo, ("loss",), tag + " loss only")
        if c["kind"] == "identical":                               # kl exactly 0: the weight exp(kl) is exactly 1
            assert bool((r["scratch"] == 1.0).all()), tag + ": exp(kl) of identical towers is not exactly 1"


# ======================================================================================================================
# SupCon
# ======================================================================================================================
def test_supcon_loss():
    for c in hr.supcon_cases():
        f, lab, T, tag = c["feat"], c["labels"], c["T"], c["tag"]
        ref, yard = hr.supcon_ref64(f, lab, T), hr.supcon_yard(f, lab, T)
        fl = hr.supcon_floors(f, lab, T, ref)
        r = hr.call_supcon(f, lab, T)
        assert r["guards"], tag
        kr.gate(f"{tag} loss", r["loss"], yard["loss"], ref["loss"], reduced=True, floor=fl["loss"])
        if f.shape[1] == 1:          # D = 1: the projection off the unit vector leaves nothing (1e-16 in float64); absolute bound
            worst = r["dfeat"].double().abs().max().item()
            print(f"{tag} dfeat: gpu max|.| {worst:.3e}, a-priori absolute bound {fl['dfeat_abs']:.3e}")
            assert ref["dfeat"].abs().max().item() <= 1e-9 * fl["dfeat_abs"] and worst <= fl["dfeat_abs"]
        else:
            kr.gate(f"{tag} dfeat", r["dfeat"], yard["dfeat"], ref["dfeat"], floor=fl["dfeat"])
        _same(r, hr.call_supcon(f, lab, T), ("loss", "dfeat"), tag + " repeat")
        lo = hr.call_supcon(f, lab, T, want_d=False)
        assert lo["guards"]
        _same(r, lo, ("loss",), tag + " dfeat NULL")
        if c["pattern"] == "distinct":                             # no anchor has a positive
            assert _zero(r["loss"]) and _zero(r["dfeat"]), tag + ": loss / gradient without positives is not exactly 0"


def test_supcon_refuses_more_than_256_rows():
    g = hr.gen(7)
    f, lab = torch.randn(257, 3, generator=g), torch.randint(0, 7, (257,), generator=g)
    _refused(hr.call_supcon(f, lab, 0.07, check=False), "supcon B=257")
    _refused(hr.call_supcon(f, lab, 0.07, want_d=False, check=False), "supcon B=257, dfeat NULL")


# ======================================================================================================================
# KAN regularisation
# ======================================================================================================================
def test_kan_regularization():
    for c in hr.kan_reg_cases():
        w, ra, re, tag = c["w"], c["ra"], c["re"], c["tag"]
        ref, yard = hr.kan_reg_ref64(w, ra, re), hr.kan_reg_yard(w, ra, re)
        fl = hr.kan_reg_floors(w, ra, re, ref)
        r = hr.call_kan_reg(w, ra, re)
        assert r["guards"], tag
        kr.gate(f"{tag} loss", r["loss"], yard["loss"], ref["loss"], reduced=True, floor=fl["loss"])
        kr.gate(f"{tag} dw", r["dw"], yard["dw"], ref["dw"], floor=fl["dw"])
        _same(r, hr.call_kan_reg(w, ra, re), ("loss", "dw"), tag + " repeat")
        lo = hr.call_kan_reg(w, ra, re, want_dw=False)             # loss only
        assert lo["guards"]
        _same(r, lo, ("loss",), tag + " loss only")
        go = hr.call_kan_reg(w, ra, re, want_loss=False)           # gradient only
        assert go["guards"]
        _same(r, go, ("dw",), tag + " gradient only")


# ======================================================================================================================
# LSTM / GRU cells
# ======================================================================================================================
def _saturation(tag, s, act, sigmoid):
    """pre-activations beyond float32's reach: sigmoid is exactly 0 below -90 (exp overflows) and exactly 1 above 18
    (exp(-18) < 2^-25); tanh is exactly +-1 beyond +-12"""
    if sigmoid:
        assert bool((act[s < -90.0] == 0).all()) and bool((act[s > 18.0] == 1).all()), tag + ": sigmoid does not saturate exactly"
    else:
        assert bool((act[s > 12.0] == 1).all()) and bool((act[s < -12.0] == -1).all()), tag + ": tanh does not saturate exactly"


def test_lstm_cell():
    for c in hr.cell_cases(4):
        gx, gh, cp, dh, dc, tag = c["gx"], c["gh"], c["prev"], c["dh"], c["dc"], c["tag"]
        H = cp.shape[1]
        ref, yard = hr.lstm_fwd_ref64(gx, gh, cp), hr.lstm_fwd_yard(gx, gh, cp)
        r = hr.call_lstm_fwd(gx, gh, cp, c["ldx"], c["ldh"])
        assert r["guards"], tag
        for k in ("h", "c", "act"):
            kr.gate(f"{tag} {k}", r[k], yard[k], ref[k])
        _same(r, hr.call_lstm_fwd(gx, gh, cp, c["ldx"], c["ldh"]), ("h", "c", "act"), tag + " repeat")
        s = gx + gh
        for k, sig in enumerate((True, True, False, True)):
            _saturation(f"{tag} gate {k}", s[:, k * H:(k + 1) * H], r["act"][:, k * H:(k + 1) * H], sig)
        act, cc = ref["act"].float(), ref["c"].float()             # what the backward reads: float32 activations and cell state
        for a, b, what in ((dh, dc, "dh, dc"), (None, dc, "dh NULL"), (dh, None, "dc NULL")):
            bref, byard = hr.lstm_bwd_ref64(a, b, act, cp, cc), hr.lstm_bwd_yard(a, b, act, cp, cc)
            fl = hr.lstm_bwd_floors(a, b, act, cp, cc, bref)
            rb = hr.call_lstm_bwd(a, b, act, cp, cc)
            assert rb["guards"], tag
            for k in ("dgates", "dc_prev"):
                kr.gate(f"{tag} bwd {what} {k}", rb[k], byard[k], bref[k], floor=fl[k])
            _same(rb, hr.call_lstm_bwd(a, b, act, cp, cc), ("dgates", "dc_prev"), f"{tag} bwd {what} repeat")
            if a is None:                                          # without dh the o gate gets exactly nothing
                assert _zero(rb["dgates"][:, 3 * H:]), tag + ": d_o without dh is not exactly 0"


def test_gru_cell():
    for c in hr.cell_cases(3):
        gx, gh, hp, dh, tag = c["gx"], c["gh"], c["prev"], c["dh"], c["tag"]
        H = hp.shape[1]
        ref, yard = hr.gru_fwd_ref64(gx, gh, hp), hr.gru_fwd_yard(gx, gh, hp)
        r = hr.call_gru_fwd(gx, gh, hp, c["ldx"], c["ldh"])
        assert r["guards"], tag
        for k in ("h", "act"):
            kr.gate(f"{tag} {k}", r[k], yard[k], ref[k])
        _same(r, hr.call_gru_fwd(gx, gh, hp, c["ldx"], c["ldh"]), ("h", "act"), tag + " repeat")
        s = gx + gh
        for k in range(2):
            _saturation(f"{tag} gate {k}", s[:, k * H:(k + 1) * H], r["act"][:, k * H:(k + 1) * H], True)
        assert kr.bits_equal(r["act"][:, 3 * H:], gh[:, 2 * H:].contiguous()), tag + ": the saved hn is not gh's n slice"
        act = ref["act"].float()
        bref, byard = hr.gru_bwd_ref64(dh, act, hp), hr.gru_bwd_yard(dh, act, hp)
        fl = hr.gru_bwd_floors(dh, act, hp, bref)
        rb = hr.call_gru_bwd(dh, act, hp)
        assert rb["guards"], tag
        for k in ("dgx", "dgh", "dh_prev"):
            kr.gate(f"{tag} bwd {k}", rb[k], byard[k], bref[k], floor=fl.get(k, kr.F32_NOISE))
        _same(rb, hr.call_gru_bwd(dh, act, hp), ("dgx", "dgh", "dh_prev"), tag + " bwd repeat")


# ======================================================================================================================
# KAN features
# ======================================================================================================================
def test_kan_features():
    for c in hr.kan_cases():
        x, grid, gs, order, act, dfeat, tag = c["x"], c["grid"], c["gs"], c["order"], c["act"], c["dfeat"], c["tag"]
        B, in_f = x.shape
        nb = gs + order
        ref, yard = hr.kan_ref64(x, grid, order, act, dfeat), hr.kan_yard(x, grid, order, act, dfeat)
        r = hr.call_kan_fwd(x, grid, gs, order, act)
        assert r["guards"], tag
        kr.gate(f"{tag} feat", r["feat"], yard["feat"], ref["feat"])
        _same(r, hr.call_kan_fwd(x, grid, gs, order, act), ("feat",), tag + " repeat")
        bases = r["feat"][:, in_f:].reshape(B, in_f, nb)
        outside = (x < grid[None, :, 0]) | (x >= grid[None, :, -1])
        assert _zero(bases[outside]), tag + ": a basis outside the grid is not exactly 0"
        if order == 0:                                             # the indicators themselves: x >= g[j] && x < g[j + 1]
            assert kr.bits_equal(r["feat"][:, in_f:], ref["feat"][:, in_f:].float().contiguous()), tag + ": order-0 bases"
        if act in (2, 3):                                          # ReLU / identity copy x
            assert kr.bits_equal(r["feat"][:, :in_f], ref["feat"][:, :in_f].float().contiguous()), tag + ": base activation"
        rb = hr.call_kan_bwd(x, grid, dfeat, gs, order, act)
        assert rb["guards"], tag
        kr.gate(f"{tag} dx", rb["dx"], yard["dx"], ref["dx"])
        _same(rb, hr.call_kan_bwd(x, grid, dfeat, gs, order, act), ("dx",), tag + " bwd repeat")


def test_kan_features_refuse_more_than_32_knots():
    g = hr.gen(8)
    gs, order, in_f, B = 26, 3, 3, 5                               # 26 + 2 * 3 + 1 = 33 knots
    grid = hr.kan_grid(in_f, gs, order, True, g)
    x = hr.kan_x(B, grid, g)
    _refused(hr.call_kan_fwd(x, grid, gs, order, 0, check=False), "kan_features_fwd with 33 knots")
    dfeat = torch.randn(B, in_f * (1 + gs + order), generator=g)
    _refused(hr.call_kan_bwd(x, grid, dfeat, gs, order, 0, check=False), "kan_features_bwd with 33 knots")
