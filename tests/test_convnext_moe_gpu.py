"""The ConvNeXt kernels (depthwise convolution, layer scale, patchify) and the MoE routing / KAN weight-pack kernels, each called
directly through the C ABI and compared with float64 (tests/convnext_moe_ref.py).

Gate: err(gpu) <= max(2 * err(yardstick), 1e-6), the yardstick being the same formula in sequential float32 on the CPU (bf16
cases: inputs rounded to bf16, the output rounded once) -- max|t - ref| / max|ref| for elementwise outputs, relative L2 for
reduced vectors.  Nothing is tuned against what the GPU returns; every comparison prints both numbers.  Exact results are
compared bitwise: a repeat of every call, calls with optional pointers NULL against the full call, all pure data movement
(patchify, dispatch, gather, the pack), integer-valued cases, and every guard band, in refused calls too.  The workspaces are
exactly as large as the *_ws_bytes functions say, inside a guard band of their own.

Where the floor is not 1e-6 (outputs whose float32 evaluation cancels; each bound is derived in the helper's docstring from
the inputs and the float64 reference alone):
  dwconv_wgrad_floor   dw, db: sums of N*H*W signed products
  layerscale_floor     dgamma: the same over M rows, folded through LDS in chains of up to 256
  elem_floor           y of the combine: up to 16 signed terms
  sum_floor            dgates of combine_bwd and scatter_add_bwd (a dot product of signed terms), d_scaler
  gate_aux_floors      loss, d_imp, d_load: x - mean(x) of evenly used experts
  gate_bwd_floors      d_clean, d_raw: dp - sum p dp of rows whose gates barely move, and the threshold terms
Errors measured on the MI355X for these outputs (records, not thresholds): see MEASURED below.
"""
import pytest
import torch

import convnext_moe_ref as cm
import kernel_ref as kr

pytestmark = pytest.mark.gpu

from hamspine import _lib as L  # noqa: E402

# Largest error over the cases of each output, as printed by a run on the MI355X: gpu / yardstick / floor, and the case.
# Records, not thresholds.
MEASURED = """
  dwconv  dw        1.13e-07 / 1.60e-07 / 1.01e-05   N=1 H=2 W=33 C=8 ks=5 f32
  dwconv  db        1.10e-07 / 1.76e-07 / 1.34e-05   N=1 H=2 W=33 C=8 ks=5 f32
  layerscale dgamma 5.65e-07 / 3.38e-06 / 1.35e-03   M=4112 C=4 rps=7 f32 (the LDS fold of 256 rows: D = 293)
  combine y         1.39e-07 / 1.39e-07 / 1.28e-06   B=67 E=16 O=64
  combine dgates    1.32e-07 / 1.30e-07 / 3.69e-06   B=1 E=16 O=63
  rows    dgates    1.66e-07 / 1.81e-07 / 1.43e-05   B=70 n=5 D=65
  kan     d_scaler  6.37e-08 / 5.50e-08 / 1.47e-06   out=3 in=5 nb=8
  gate    loss      6.82e-06 / 6.82e-06 / 1.11e-03   B=200 E=2 k=1 noisy
  gate    d_imp     2.96e-06 / 2.96e-06 / 5.12e-04   B=63 E=2 k=1 noisy
  gate    d_load    7.31e-06 / 7.31e-06 / 6.41e-04   B=200 E=2 k=1 noisy
  gate    (built-in noise, B=4096 E=16 k=4) loss 6.60e-06 / 7.36e-06 / 3.02e-02, d_imp 1.16e-05 / 1.03e-05 / 8.45e-03,
                    d_load 6.58e-05 / 6.58e-05 / 2.59e-02; z: mean 3.06e-03 (bound 1.95e-02), var - 1 3.51e-03 (bound 2.76e-02)
  gate_bwd d_clean  2.31e-05 / 2.31e-05 / 1.00e-03   B=1 E=16 k=1 noisy       (largest among the floors below 1e-2)
  gate_bwd d_raw    4.19e-06 / 4.19e-06 / 9.80e-05   B=1 E=16 k=1 noisy
  gate_bwd vacuous: 53 of the 175 comparisons have a floor of 1e-2 or more, all of them k = 1: dp = gi (1 - p / (p + 1e-6)) / (p + 1e-6)
                    is 1e-6 of what its roundings scale with.  Largest: d_clean 4.63e-02 / 4.63e-02 / 5.23 (B=64 E=2 k=1 plain,
                    g_loss NULL), d_raw 4.44e-02 / 4.44e-02 / 5.06 (B=65 E=2 k=1 noisy, g_loss NULL): the GPU's error equals the
                    yardstick's to every printed digit there, and the cases with k >= 2 carry the comparison.
Without a floor (1e-6): f32 dwconv y 2.20e-07 / 2.20e-07, dx 1.88e-07 / 1.62e-07, layerscale out 6.10e-08 / 5.56e-08, du 7.08e-08 / 7.08e-08;
their bf16 runs at most 3.40e-03 / 3.40e-03 (one bf16 rounding; gpu = yardstick); gate gates 1.81e-07 / 1.24e-07, p 2.99e-07 / 2.99e-07, sigma 1.32e-08 / 1.32e-08, loadrow 1.13e-07 / 1.74e-07;
scatter_add 5.45e-08 / 5.45e-08.
"""

REC = {}


def _gate(name, tag, gpu, yard, ref, reduced=False, floor=kr.F32_NOISE):
    eg, ey = kr.gate(f"{tag} {name}", gpu, yard, ref, reduced=reduced, floor=floor)
    if name not in REC or eg > REC[name][0]:
        REC[name] = (eg, ey, max(floor, kr.F32_NOISE), tag)


def _report(prefix):
    for name, (eg, ey, fl, tag) in sorted(REC.items()):
        if name.startswith(prefix):
            print(f"RECORD {name}: {eg:.2e} / {ey:.2e} / {fl:.2e}   {tag}")


def _same(a, b, keys, what):
    for k in keys:
        assert kr.bits_equal(a[k], b[k]), f"{what}: {k} differs bitwise"


def _bits(t, ref, what):
    assert kr.bits_equal(t, ref.to(t.dtype)), f"{what}: differs bitwise"


def _zero(t):
    return bool((t == 0).all())


def _refused(r, what, word=None):
    assert r["status"] != 0, f"{what}: accepted"
    assert r["untouched"], f"{what}: refused, but an output, the workspace or a guard band was written"
    with pytest.raises(L.HamspineError) as ei:
        L.check(r["status"], what)
    msg = L.lib().hs_last_error().decode("utf-8", "replace")
    assert msg and (word is None or word in msg), f"{what}: hs_last_error() says {msg!r}"
    assert msg in str(ei.value)


# ======================================================================================================================
# depthwise convolution
# ======================================================================================================================
@pytest.mark.parametrize("dtype", cm.DTYPES, ids=cm.dname)
def test_dwconv_fwd_and_dgrad(dtype):
    for c in cm.dwconv_fwd_cases():
        x, dy, w, bias = cm.dwconv_data(c, dtype)
        ks, tag = c["ks"], f"{c['tag']} {cm.dname(dtype)}"
        ref, yard = cm.dwconv_ref64(x, w, bias, dy, ks), cm.dwconv_yard(x, w, bias, dy, ks)
        r = cm.call_dwconv_fwd(x, w, bias, ks)
        assert r["guards"], tag
        _gate("dwconv.y", tag, r["y"], yard["y"], ref["y"])
        _same(r, cm.call_dwconv_fwd(x, w, bias, ks), ("y",), tag + " repeat")
        b = cm.call_dwconv_bwd(x, w, dy, ks, want_dw=False, want_db=False)
        assert b["guards"], tag
        _gate("dwconv.dx", tag, b["dx"], yard["dx"], ref["dx"])
        _same(b, cm.call_dwconv_bwd(x, w, dy, ks, want_dw=False, want_db=False), ("dx",), tag + " dgrad repeat")
        if c["kind"] == "int":
            _bits(r["y"], ref["y"], tag + " integer y")
            _bits(b["dx"], ref["dx"], tag + " integer dx")
    _report("dwconv.")


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=cm.dname)
def test_dwconv_wgrad(dtype):
    for c in cm.dwconv_wgrad_cases():
        x, dy, w, bias = cm.dwconv_data(c, dtype)
        ks, tag = c["ks"], f"{c['tag']} {cm.dname(dtype)}"
        ref, yard = cm.dwconv_ref64(x, w, None, dy, ks), cm.dwconv_yard(x, w, None, dy, ks)
        fl = cm.dwconv_wgrad_floor(ref, c["N"], c["H"], c["W"], c["C"])
        r = cm.call_dwconv_bwd(x, w, dy, ks)
        assert r["guards"], tag + ": a guard band (outputs or workspace) was written"
        _gate("wgrad.dw", tag, r["dw"], yard["dw"], ref["dw"], reduced=True, floor=fl["dw"])
        _gate("wgrad.db", tag, r["db"], yard["db"], ref["db"], reduced=True, floor=fl["db"])
        _gate("wgrad.dx", tag, r["dx"], yard["dx"], ref["dx"])
        _same(r, cm.call_dwconv_bwd(x, w, dy, ks), ("dx", "dw", "db"), tag + " repeat")
        v = cm.call_dwconv_bwd(x, w, dy, ks, want_dx=False)
        assert v["guards"]
        _same(r, v, ("dw", "db"), tag + " dx NULL")
        v = cm.call_dwconv_bwd(x, w, dy, ks, want_dw=False, want_db=False)
        assert v["guards"]
        _same(r, v, ("dx",), tag + " dw NULL")
        v = cm.call_dwconv_bwd(x, w, dy, ks, want_db=False)
        assert v["guards"]
        _same(r, v, ("dx", "dw"), tag + " db NULL")
        if c["kind"] == "int":
            _bits(r["dw"], ref["dw"], tag + " integer dw")
            _bits(r["db"], ref["db"], tag + " integer db")
    _report("wgrad.")


# ======================================================================================================================
# layer scale
# ======================================================================================================================
@pytest.mark.parametrize("dtype", cm.DTYPES, ids=cm.dname)
def test_layerscale(dtype):
    for c in cm.layerscale_cases():
        u, res, dy, gamma, rs = cm.layerscale_data(c, dtype)
        M, Cc, rps, tag = c["M"], c["C"], c["rps"], f"{c['tag']} {cm.dname(dtype)}"
        ref, yard = cm.layerscale_ref64(u, res, dy, gamma, rs, rps), cm.layerscale_yard(u, res, dy, gamma, rs, rps)
        f = cm.call_layerscale_fwd(u, res, gamma, rs, rps)
        assert f["guards"], tag
        _gate("layerscale.out", tag, f["out"], yard["out"], ref["out"])
        _same(f, cm.call_layerscale_fwd(u, res, gamma, rs, rps), ("out",), tag + " repeat")
        b = cm.call_layerscale_bwd(dy, u, gamma, rs, rps)
        assert b["guards"], tag + ": a guard band (outputs or workspace) was written"
        _gate("layerscale.du", tag, b["du"], yard["du"], ref["du"])
        _gate("layerscale.dgamma", tag, b["dgamma"], yard["dgamma"], ref["dgamma"], reduced=True, floor=cm.layerscale_floor(ref, M, Cc))
        _same(b, cm.call_layerscale_bwd(dy, u, gamma, rs, rps), ("du", "dgamma"), tag + " bwd repeat")
        nod = cm.call_layerscale_bwd(dy, u, gamma, rs, rps, want_du=False)
        assert nod["guards"]
        _same(b, nod, ("dgamma",), tag + " du NULL")
        if rs is None:                    # rowscale NULL against a rowscale of ones
            ones = torch.ones(M)
            _same(f, cm.call_layerscale_fwd(u, res, gamma, ones, 1), ("out",), tag + " rowscale NULL / ones")
            _same(b, cm.call_layerscale_bwd(dy, u, gamma, ones, 1), ("du", "dgamma"), tag + " rowscale NULL / ones")
        else:
            for s in torch.nonzero(rs == 0).reshape(-1).tolist():
                rows = slice(s * rps, min((s + 1) * rps, M))
                assert kr.bits_equal(f["out"][rows], res[rows]), f"{tag}: sample {s} (rowscale 0): out is not res"
                assert _zero(b["du"][rows]), f"{tag}: sample {s} (rowscale 0): du is not 0"
        if c["kind"] == "int":
            _bits(b["dgamma"], ref["dgamma"], tag + " integer dgamma")
            _bits(f["out"], ref["out"], tag + " integer out")          # (exact in float32, so bf16 rounds the exact value once)
    _report("layerscale.")


# ======================================================================================================================
# patchify
# ======================================================================================================================
@pytest.mark.parametrize("dtype", cm.DTYPES, ids=cm.dname)
def test_patchify(dtype):
    for c in cm.patchify_cases():
        N, H, W, Cc, k, ld = c["N"], c["H"], c["W"], c["C"], c["k"], c["ld"]
        tag = f"{c['tag']} {cm.dname(dtype)}"
        x = cm.patchify_data(c, dtype)
        ref = cm.patchify_ref(x, k)
        kk = k * k * Cc
        f = cm.call_patchify_fwd(x, k, ld)                               # the output starts out filled with the sentinel
        assert f["guards"], tag
        assert kr.bits_equal(f["out"][:, :kk].contiguous(), ref), tag + ": out differs from the index formula"
        assert kr.bits_equal(f["out"][:, kk:].contiguous(), torch.zeros(ref.shape[0], ld - kk, dtype=dtype)), tag + ": padding columns not +0"
        _same(f, cm.call_patchify_fwd(x, k, ld), ("out",), tag + " repeat")
        g = cm.gen(c["seed"] + 1)
        dp = torch.full((ref.shape[0], ld), cm.HUGE, dtype=dtype)         # padding columns must not be read
        dp[:, :kk] = (torch.randn(ref.shape[0], kk, generator=g) + 2.0).to(dtype)
        b = cm.call_patchify_bwd(dp, N, H, W, Cc, k)
        assert b["guards"], tag
        dxr = cm.patchify_bwd_ref(dp[:, :kk].contiguous(), N, H, W, Cc, k)
        assert kr.bits_equal(b["dx"], dxr), tag + ": dx differs (the uncovered border must be +0)"
        _same(b, cm.call_patchify_bwd(dp, N, H, W, Cc, k), ("dx",), tag + " bwd repeat")
        rt = cm.call_patchify_bwd(f["out"], N, H, W, Cc, k)              # bwd(fwd(x)) == x where covered
        P, Q = H // k, W // k
        xr = torch.zeros_like(x)
        xr[:, :P * k, :Q * k] = x[:, :P * k, :Q * k]
        assert kr.bits_equal(rt["dx"], xr), tag + ": round trip"


# ======================================================================================================================
# MoE gating
# ======================================================================================================================
_GATE_REF = {}


def _gate_case(c):
    """data, float64 reference (with gradients) and yardsticks of a gating case, computed once and left unchanged"""
    if c["tag"] not in _GATE_REF:
        clean, raw, z, _ = cm.gate_data(c["B"], c["E"], c["k"], c["noisy"], c["seed"])
        dg, gl = cm.gate_bwd_inputs(c)
        ref = cm.gate_fwd64(clean, raw, z, c["k"], c["noisy"], grad=(dg, gl))
        _GATE_REF[c["tag"]] = (clean, raw, z, dg, gl, ref)
    return _GATE_REF[c["tag"]]


def _check_gate_fwd(tag, r, ref, yard, B, E, k, noisy, pre="gate."):
    m = min(k + 1, E)
    assert r["guards"], tag
    assert torch.equal(r["top"][:, :m], ref["top"]), tag + ": top differs"
    assert bool((r["top"][:, m:] == int(kr.SENT)).all()), tag + ": top written beyond min(k + 1, E)"
    fl = cm.gate_aux_floors(ref, B, E)
    for kk in ("gates", "p", "loadrow") + (("sigma",) if noisy else ()):
        _gate(pre + kk, tag, r[kk], yard[kk], ref[kk])
    if not noisy:
        assert _zero(r["sigma"]) and _zero(r["z"]), tag + ": sigma / z of plain gating not 0"
    if not (noisy and k < E):
        _bits(r["loadrow"], ref["loadrow"], tag + " loadrow (gates > 0)")
    for kk in ("loss", "d_imp", "d_load"):
        if ref[kk].abs().max() > 0:
            _gate(pre + kk, tag, r[kk], yard[kk], ref[kk], reduced=(kk == "loss"), floor=fl[kk])
        else:
            assert _zero(r[kk]), f"{tag}: {kk} is not exactly 0"


@pytest.mark.parametrize("B", cm.GATE_BS)
def test_moe_gate_fwd(B):
    for c in (c for c in cm.gate_cases() if c["B"] == B):
        E, k, noisy, tag = c["E"], c["k"], c["noisy"], c["tag"]
        clean, raw, z, dg, gl, ref = _gate_case(c)
        yard = cm.gate_fwd_yard(clean, raw, z, k, noisy)
        args = (clean, raw if noisy else None, z if noisy else None, k, noisy)
        r = cm.call_gate_fwd(*args)
        _check_gate_fwd(tag, r, ref, yard, B, E, k, noisy)
        if noisy:
            _bits(r["z"], z, tag + ": z is not the supplied noise")
        _same(r, cm.call_gate_fwd(*args), ("gates", "p", "top", "z", "sigma", "loadrow", "loss", "d_imp", "d_load"), tag + " repeat")
    _report("gate.")


def test_moe_gate_ties():
    """equal logits, no noise: the documented rule (lowest index first), not torch.topk"""
    clean = torch.zeros(66, 5)
    clean[1] = torch.tensor([1.0, 2.0, 2.0, 1.0, 2.0])
    clean[65] = torch.tensor([0.0, 0.0, 3.0, 3.0, -1.0])
    for k in (1, 2, 4, 5):
        r = cm.call_gate_fwd(clean, None, None, k, 0)
        ref = cm.gate_fwd64(clean, None, None, k, 0)
        m = min(k + 1, 5)
        assert r["guards"]
        assert torch.equal(r["top"][:, :m], ref["top"]), f"ties k={k}"
        assert r["top"][0, :m].tolist() == list(range(m)) and r["top"][1, :min(m, 3)].tolist() == [1, 2, 4][:min(m, 3)]
        assert r["top"][65, :2].tolist() == [2, 3][:m]
        kr.gate(f"ties k={k} gates", r["gates"], cm.gate_fwd_yard(clean, None, None, k, 0)["gates"], ref["gates"])


def test_moe_gate_builtin_noise():
    """noise = NULL: the counter RNG's Box-Muller draw (B * E = 65536 values)"""
    B, E, k = 4096, 16, 4
    n = B * E
    g = cm.gen(77)
    clean, raw = 1.5 * torch.randn(B, E, generator=g), 0.5 * torch.randn(B, E, generator=g)
    r = cm.call_gate_fwd(clean, raw, None, k, 1, seed=1234)
    z = r["z"]
    assert r["guards"] and bool(torch.isfinite(z).all())
    assert kr.bits_equal(z, cm.call_gate_fwd(clean, raw, None, k, 1, seed=1234)["z"]), "z differs on a repeat with the same seed"
    assert not kr.bits_equal(z, cm.call_gate_fwd(clean, raw, None, k, 1, seed=1235)["z"]), "z does not depend on the seed"
    mean, var = z.double().mean().item(), z.double().var().item()
    print(f"built-in noise: mean {mean:.3e} (<= {5 / n ** 0.5:.3e})  var - 1 {var - 1:.3e} (<= {5 * (2 / n) ** 0.5:.3e})")
    assert abs(mean) <= 5 / n ** 0.5 and abs(var - 1) <= 5 * (2 / n) ** 0.5
    # the other outputs against float64 on the returned z (a function of seed and index alone): rows of which this z leaves a
    # selection undecided get new clean logits until every row passes both margins, then the call is made again
    for _ in range(100):
        bad = cm.gate_bad_rows(clean, raw, z, k, 1)
        if not bad.any():
            break
        clean[bad] = 1.5 * torch.randn(int(bad.sum()), E, generator=g)
    assert not bad.any()
    r = cm.call_gate_fwd(clean, raw, None, k, 1, seed=1234)
    _bits(r["z"], z, "z changed with the logits")
    ref, yard = cm.gate_fwd64(clean, raw, z, k, 1), cm.gate_fwd_yard(clean, raw, z, k, 1)
    _check_gate_fwd("built-in noise B=4096 E=16 k=4", r, ref, yard, B, E, k, 1, pre="gaterng.")
    _report("gaterng.")


@pytest.mark.parametrize("B", cm.GATE_BS)
def test_moe_gate_bwd(B):
    for c in (c for c in cm.gate_cases() if c["B"] == B):
        E, k, noisy, tag = c["E"], c["k"], c["noisy"], c["tag"]
        clean, raw, z, dg, gl, ref = _gate_case(c)
        rw = raw if noisy else None
        sv = cm.gate_saved32(ref)
        svk = dict(sv, top=cm.top_rows(ref["top"], B))
        yard = cm.gate_bwd_yard(clean, raw, sv, dg, gl, k, noisy)
        fl = cm.gate_bwd_floors(clean, raw, ref, dg, gl, k, noisy)
        r = cm.call_gate_bwd(clean, rw, svk, dg, gl, k, noisy)
        assert r["guards"], tag
        for kk in ("d_clean", "d_raw"):
            if ref[kk].abs().max() > 0:
                _gate("gatebwd." + kk, tag, r[kk], yard[kk], ref[kk], floor=fl[kk])
            else:
                assert _zero(r[kk]), f"{tag}: {kk} is not exactly 0"
        _same(r, cm.call_gate_bwd(clean, rw, svk, dg, gl, k, noisy), ("d_clean", "d_raw"), tag + " repeat")
        nr = cm.call_gate_bwd(clean, rw, svk, dg, gl, k, noisy, want_raw=False)
        assert nr["guards"]
        _same(r, nr, ("d_clean",), tag + " d_raw NULL")
        # g_loss NULL: the gradient of sum(gates * dgates) alone
        ref0 = cm.gate_fwd64(clean, raw, z, k, noisy, grad=(dg, None))
        yard0 = cm.gate_bwd_yard(clean, raw, sv, dg, None, k, noisy)
        fl0 = cm.gate_bwd_floors(clean, raw, ref0, dg, None, k, noisy)
        r0 = cm.call_gate_bwd(clean, rw, svk, dg, None, k, noisy)
        assert r0["guards"]
        for kk in ("d_clean", "d_raw"):
            if ref0[kk].abs().max() > 0:
                _gate("gatebwd0." + kk, tag + " g_loss NULL", r0[kk], yard0[kk], ref0[kk], floor=fl0[kk])
            else:
                assert _zero(r0[kk]), f"{tag} g_loss NULL: {kk} is not exactly 0"
    _report("gatebwd")


# ======================================================================================================================
# combine, dispatch, row gather / scatter
# ======================================================================================================================
def test_moe_combine():
    for c in cm.combine_cases():
        gates, outs, dy = cm.combine_data(c)
        E, tag = c["E"], c["tag"]
        ref, yard = cm.combine_ref64(gates, outs, dy), cm.combine_yard(gates, outs, dy)
        f = cm.call_combine_fwd(gates, outs)
        assert f["guards"], tag
        assert bool(torch.isfinite(f["y"]).all()) and f["y"].abs().max() < 1e3, tag + ": a zero-gate row (1e30) leaked into y"
        _gate("combine.y", tag, f["y"], yard["y"], ref["y"], floor=cm.elem_floor(ref["terms"], E + 1))
        _same(f, cm.call_combine_fwd(gates, outs), ("y",), tag + " repeat")
        b = cm.call_combine_bwd(gates, outs, dy)
        assert b["guards"], tag
        live = gates != 0
        for e in range(E):
            _bits(b[f"dout{e}"], yard["douts"][e], f"{tag} dout{e} (one float32 product)")
            assert _zero(b[f"dout{e}"][~live[:, e]]), f"{tag}: dout{e} of zero-gate rows is not 0"
        m = live.reshape(-1)                 # (the dot products with the 1e30 rows are of no interest)
        _gate("combine.dgates", tag, b["dgates"].reshape(-1)[m], yard["dgates"].reshape(-1)[m], ref["dgates"].reshape(-1)[m],
              reduced=True, floor=kr.sum_floor(ref["dterms"][:, m]))
        _same(b, cm.call_combine_bwd(gates, outs, dy), ["dgates"] + [f"dout{e}" for e in range(E)], tag + " bwd repeat")
    _report("combine.")


def test_moe_dispatch_index():
    for c in cm.dispatch_cases():
        gates = cm.dispatch_data(c)
        idx, count = cm.dispatch_ref(gates)
        r = cm.call_dispatch(gates)
        assert r["guards"], c["tag"]
        assert torch.equal(r["count"], count), f"{c['tag']}: count {r['count'].tolist()} != {count.tolist()}"
        assert torch.equal(r["idx"], idx), c["tag"] + ": idx differs (or was written beyond count)"
        _same(r, cm.call_dispatch(gates), ("idx", "count"), c["tag"] + " repeat")


def test_rows_gather_scatter():
    for c in cm.rows_cases():
        full, rows, idx, gates = cm.rows_data(c)
        B, n, D, E, tag = c["B"], c["n"], c["D"], c["E"], c["tag"]
        il = idx.long()
        col = E - 1
        r = cm.call_rows_gather(full, idx)
        assert r["guards"], tag
        _bits(r["dst"], full[il], tag + " gather")
        # scatter-add without a scale: one exact float32 addition per element, rows not named in idx unchanged
        want = full.clone()
        want[il] = full[il] + rows
        s = cm.call_rows_scatter_add(full, idx, None, 0, rows)
        assert s["guards"], tag
        _bits(s["dst"], want, tag + " scatter_add, scale NULL")
        # with a scale: dst + scale * src through the gate
        s = cm.call_rows_scatter_add(full, idx, gates, col, rows)
        assert s["guards"], tag
        sc = gates[il, col:col + 1]
        ref = full.double()
        ref[il] = full[il].double() + sc.double() * rows.double()
        yard = full.clone()
        yard[il] = full[il] + sc * rows
        _gate("rows.scatter_add", tag, s["dst"], yard, ref)
        keep = torch.ones(B, dtype=torch.bool)
        keep[il] = False
        _bits(s["dst"][keep], full[keep], tag + ": rows not named in idx changed")
        _same(s, cm.call_rows_scatter_add(full, idx, gates, col, rows), ("dst",), tag + " repeat")
        # backward: dsrc = gates[idx][col] * dy[idx] (one product), dgates[idx][col] = <dy[idx], src>; nothing else written
        b = cm.call_rows_scatter_add_bwd(full, idx, gates, col, rows)
        assert b["guards"], tag
        _bits(b["dsrc"], sc * full[il], tag + " dsrc")
        t = (full[il].double() * rows.double()).t()
        yd = torch.from_numpy(kr.seq_sum32((full[il] * rows).numpy(), 1))
        _gate("rows.dgates", tag, b["dgates"][il, col], yd, t.sum(0), reduced=True, floor=kr.sum_floor(t))
        rest = b["dgates"].clone()
        rest[il, col] = kr.SENT
        assert kr.bits_equal(rest, torch.full_like(rest, kr.SENT)), tag + ": dgates written outside (idx, col)"
        _same(b, cm.call_rows_scatter_add_bwd(full, idx, gates, col, rows), ("dsrc", "dgates"), tag + " bwd repeat")
        # n = 0: OK, nothing touched
        for z in (cm.call_rows_gather(full, idx, n=0), cm.call_rows_scatter_add_bwd(full, idx, gates, col, rows, n=0)):
            assert z["status"] == 0 and z["untouched"], tag + " n = 0"
        z = cm.call_rows_scatter_add(full, idx, gates, col, rows, n=0)
        assert z["status"] == 0 and z["guards"] and kr.bits_equal(z["dst"], full), tag + " n = 0"
    _report("rows.")


# ======================================================================================================================
# KAN weight pack / unpack
# ======================================================================================================================
def test_kan_pack_unpack():
    for i, (o, n, nb) in enumerate(cm.KAN_SHAPES):
        bw, sw, sc, dw = cm.kan_pack_data(o, n, nb, 1100 + i)
        for scaler in (sc, None):
            tag = f"kan out={o} in={n} nb={nb} scaler={'given' if scaler is not None else 'NULL'}"
            p = cm.call_kan_pack(bw, sw, scaler)
            assert p["guards"], tag
            _bits(p["wcat"], cm.kan_pack_ref32(bw, sw, scaler), tag + " wcat")
            _same(p, cm.call_kan_pack(bw, sw, scaler), ("wcat",), tag + " repeat")
            ref = cm.kan_unpack_ref(dw, sw, scaler)
            r = cm.call_kan_unpack(dw, sw, scaler)
            assert r["guards"], tag
            _bits(r["d_base"], ref["d_base"], tag + " d_base")
            _bits(r["d_spline"], ref["d_spline"].reshape(o, n * nb), tag + " d_spline")
            _gate("kan.d_scaler", tag, r["d_scaler"], ref["d_scaler_yard"], ref["d_scaler"], reduced=True, floor=kr.sum_floor(ref["terms"]))
            _same(r, cm.call_kan_unpack(dw, sw, scaler), ("d_base", "d_spline", "d_scaler"), tag + " repeat")
            keys = ("d_base", "d_spline", "d_scaler")
            for j in range(3):                                # each d_* pointer NULL in turn
                want = tuple(q != j for q in range(3))
                v = cm.call_kan_unpack(dw, sw, scaler, want=want)
                assert v["guards"]
                _same(r, v, [kk for q, kk in enumerate(keys) if q != j], f"{tag} {keys[j]} NULL")
    _report("kan.")


# ======================================================================================================================
# refused calls: nonzero status, hs_last_error() set, every output, workspace and guard band untouched.  Each of these
# returns from its HS_REQUIRE before any launch.
# ======================================================================================================================
def test_refused_convnext():
    for dtype in cm.DTYPES:
        c = cm._dwc(1, 2, 3, 8, 3, 1)
        x, dy, w, bias = cm.dwconv_data(c, dtype)
        _refused(cm.call_dwconv_fwd(x, w, bias, 3, C_arg=6, check=False), "dwconv_fwd C=6", "multiple of 4")
        _refused(cm.call_dwconv_fwd(x, torch.randn(8, 16), bias, 4, check=False), "dwconv_fwd ksize=4", "kernel size")
        _refused(cm.call_dwconv_bwd(x, torch.randn(8, 16), dy, 4, check=False), "dwconv_bwd ksize=4", "kernel size")
        _refused(cm.call_dwconv_fwd(x, w, bias, 3, ws_short=1, check=False), "dwconv_fwd ws one byte short", "workspace")
        _refused(cm.call_dwconv_bwd(x, w, dy, 3, ws_short=1, check=False), "dwconv_bwd ws one byte short", "workspace")
        _refused(cm.call_dwconv_bwd(x, w, dy, 3, want_dw=False, want_db=True, check=False), "dwconv_bwd db without dw", "db needs dw")
        lc = cm._lsc(5, 8, 1, 2)
        u, res, dy, gamma, rs = cm.layerscale_data(lc, dtype)
        _refused(cm.call_layerscale_fwd(u, res, gamma, rs, 1, C_arg=6, check=False), "layerscale_fwd C=6", "multiple of 4")
        _refused(cm.call_layerscale_bwd(dy, u, gamma, rs, 1, C_arg=6, check=False), "layerscale_bwd C=6", "multiple of 4")
        _refused(cm.call_layerscale_bwd(dy, u, gamma, rs, 1, ws_short=1, check=False), "layerscale_bwd ws one byte short", "workspace")
        _refused(cm.call_layerscale_bwd(dy, u, gamma, rs, 0, check=False), "layerscale_bwd rows_per_sample=0", "rows_per_sample")
        xp = torch.randn(1, 4, 4, 4).to(dtype)
        _refused(cm.call_patchify_fwd(xp, 2, 15, check=False), "patchify_fwd ldo < k*k*C", "ldo")
        _refused(cm.call_patchify_bwd(torch.randn(4, 16).to(dtype), 1, 4, 4, 4, 2, ld_arg=15, check=False), "patchify_bwd ldp < k*k*C", "ldp")


def test_refused_moe_kan():
    g = cm.gen(3)
    B = 5

    def gate_bwd(E, k, noisy=1, raw=True, **kw):
        clean, rw = torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)
        sv = {"p": torch.full((B, E), 1.0 / E), "z": torch.zeros(B, E), "sigma": torch.ones(B, E), "d_imp": torch.zeros(E),
              "d_load": torch.zeros(E), "top": cm.top_rows(torch.arange(min(max(k, 0) + 1, E, 16)).expand(B, -1).to(torch.int32), B)}
        return cm.call_gate_bwd(clean, rw if raw else None, sv, torch.randn(B, E, generator=g), 0.5, k, noisy, check=False, **kw)

    _refused(gate_bwd(17, 2), "moe_gate_bwd E=17", "moe_gate_bwd")
    _refused(gate_bwd(4, 0), "moe_gate_bwd k=0", "moe_gate_bwd")
    _refused(gate_bwd(4, 5), "moe_gate_bwd k=5 > E=4", "moe_gate_bwd")
    _refused(gate_bwd(4, 2, B_arg=0), "moe_gate_bwd B=0", "moe_gate_bwd")
    _refused(gate_bwd(4, 2, E_arg=0), "moe_gate_bwd E=0", "moe_gate_bwd")
    _refused(gate_bwd(4, 2, noisy=1, raw=False), "moe_gate_bwd noisy, d_raw wanted, raw_noise NULL", "raw_noise")
    ok = gate_bwd(4, 2, noisy=1, raw=False, want_raw=False)          # ... but fine when d_raw is not wanted
    assert ok["status"] == 0 and ok["guards"]
    clean = torch.randn(B, 17, generator=g)
    _refused(cm.call_gate_fwd(clean, None, None, 2, 0, check=False), "moe_gate_fwd E=17", "moe_gate_fwd")
    _refused(cm.call_gate_fwd(clean[:, :4].contiguous(), None, None, 5, 0, check=False), "moe_gate_fwd k=5 > E=4", "moe_gate_fwd")
    gates, outs, dy = cm.combine_data({"B": 5, "E": 3, "O": 7, "seed": 4})
    _refused(cm.call_combine_fwd(gates, outs, B_arg=0, check=False), "moe_combine_fwd B=0", "moe_combine")
    _refused(cm.call_combine_fwd(gates, outs, O_arg=0, check=False), "moe_combine_fwd O=0", "moe_combine")
    _refused(cm.call_combine_bwd(gates, outs, dy, B_arg=0, check=False), "moe_combine_bwd B=0", "moe_combine_bwd")
    _refused(cm.call_combine_bwd(gates, outs, dy, O_arg=-1, check=False), "moe_combine_bwd O=-1", "moe_combine_bwd")
    bw, sw, sc, dw = cm.kan_pack_data(3, 5, 8, 5)
    for dims in ((0, 5, 8), (3, 0, 8), (3, 5, 0), (3, -5, 8)):
        _refused(cm.call_kan_pack(bw, sw, sc, dims=dims, check=False), f"kan_pack_weight {dims}", "kan_pack_weight")
        _refused(cm.call_kan_unpack(dw, sw, sc, dims=dims, check=False), f"kan_unpack_wgrad {dims}", "kan_unpack_wgrad")
