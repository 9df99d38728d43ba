"""KAN grid update on the device (csrc/kan_grid.hip: hs_kan_grid_knots, hs_kan_refit) through the C ABI on guarded buffers,
and through KANLinear / KAN1.  References, yardsticks and inputs: tests/kan_grid_ref.py (their guards are asserted by
tests/test_kan_grid_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import kan_grid_ref as R
import kernel_ref as KR
from oracle.procedural import load_procedural

pytestmark = pytest.mark.gpu
DEV = KR.DEV


def _err():
    from hamspine import _lib as L
    return L.lib().hs_last_error().decode()


def _ok(r, what):
    assert r["status"] == 0, f"{what}: status {r['status']}: {_err()}"
    assert r["guards"], f"{what}: wrote outside its output"


# --------------------------------------------------------------------------------------------------------------------
# knots
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,in_f,gs,order", [(B, i, 5, 3) for B, i in R.KNOT_SHAPES] + [(40, 16, 8, 2), (40, 16, 3, 1)])
def test_knots_are_bit_equal_to_the_restatement(B, in_f, gs, order):
    x = R.knot_input(B, in_f)
    r = R.call_knots(x, gs, order)
    _ok(r, "knots")
    assert KR.bits_equal(r["grid"], R.knot_rows(x, gs, order))


def test_knots_with_ties_and_signed_zeros():
    x = R.ties_input()
    r = R.call_knots(x, 5, 3)
    _ok(r, "knots")
    want = R.knot_rows(x, 5, 3)
    others = [i for i in range(16) if i != 3]
    assert KR.bits_equal(r["grid"][others], want[others])               # runs of equal values: the selected values are torch.sort's
    assert torch.equal(r["grid"][3], want[3])                           # +0.0 and -0.0 are one value: compared numerically


def test_knots_keep_a_nan_column_to_itself():
    x = R.knot_input(40, 16)
    xn = x.clone()
    xn[:, 5] = float("nan")
    a, b = R.call_knots(x, 5, 3), R.call_knots(xn, 5, 3)
    _ok(b, "knots")
    others = [i for i in range(16) if i != 5]
    assert KR.bits_equal(a["grid"][others], b["grid"][others])
    assert bool(torch.isnan(b["grid"][5]).all())                        # torch.sort puts a NaN last: min, max and every knot


# --------------------------------------------------------------------------------------------------------------------
# refit
# --------------------------------------------------------------------------------------------------------------------
def _s_mode(x, grid_old, w, sc, gs, order, full_rank):
    """reference, yardstick and device result of one S-mode case; the new knots come from the restatement"""
    coeff = R.scaled_coeff(w, sc)
    knots = R.knot_rows(x, gs, order)
    ref = R.refit_ref64(x, knots, order, R.targets64(x, grid_old, coeff, order))
    R.assert_comparable(ref, x.shape[0], gs + order, full_rank)
    yard = (R.lstsq_yard32 if full_rank else R.pinv_yard32)(x, knots, order, R.targets32(x, grid_old, coeff, order))
    r = R.call_refit(x, knots, gs, order, grid_old=grid_old, spline_w=w, scaler=sc)
    _ok(r, "refit")
    return ref, yard, r["out"].view(w.shape)


@pytest.mark.parametrize("case", R.FULL_RANK, ids=lambda c: "x".join(map(str, c[:5])))
def test_refit_full_rank_against_lstsq(case):
    B, in_f, out_f, gs, order, seed = case
    ref, yard, got = _s_mode(*R.full_rank_case(*case), gs, order, True)
    assert bool(torch.isfinite(got).all())
    KR.gate(f"coefficients {case[:5]}", got, yard, ref["sol"])


@pytest.mark.parametrize("name", sorted(R.RANK_DEFICIENT))
def test_refit_rank_deficient_against_pinv(name):
    ref, yard, got = _s_mode(*R.deficient_case(name), 5, 3, False)
    assert bool(torch.isfinite(got).all())
    KR.gate(f"coefficients {name}", got, yard, ref["sol"])
    KR.gate(f"fitted values {name}", R.fitted64(ref, got), R.fitted64(ref, yard), ref["fitted"])


def test_curve2coeff_y_mode():
    from hamspine import kan as K
    g = KR.gen(11)
    x = torch.randn(40, 16, generator=g) * 0.9
    y = torch.randn(40, 16, 12, generator=g)
    knots = R.knot_rows(x, 5, 3)
    Y = y.permute(1, 0, 2).contiguous()
    ref = R.refit_ref64(x, knots, 3, Y.double())
    R.assert_comparable(ref, 40, 8, True)
    yard = R.lstsq_yard32(x, knots, 3, Y)
    r = R.call_refit(x, knots, 5, 3, y=y)
    _ok(r, "refit y-mode")
    KR.gate("y-mode coefficients", r["out"].view(12, 16, 8), yard, ref["sol"])
    got = K.kan_curve2coeff(x.to(DEV), y.to(DEV), knots.to(DEV), 5, 3)
    assert KR.bits_equal(got, r["out"].view(12, 16, 8))


def test_refit_properties():
    case = R.FULL_RANK[0]
    B, in_f, out_f, gs, order, seed = case
    x, grid_old, w, sc = R.full_rank_case(*case)
    knots = R.call_knots(x, gs, order)["grid"]
    a = R.call_refit(x, knots, gs, order, grid_old=grid_old, spline_w=w, scaler=sc)
    b = R.call_refit(x, knots, gs, order, grid_old=grid_old, spline_w=w, scaler=sc)
    c = R.call_refit(x, knots, gs, order, grid_old=grid_old, spline_w=w, scaler=sc, in_place=True)
    for r in (a, b, c):
        _ok(r, "refit")
    assert KR.bits_equal(a["out"], b["out"]), "two runs differ"
    assert KR.bits_equal(a["out"], c["out"]), "in place differs from out of place"
    # without the scaler: the coefficients of the pre-scaled weights
    d = R.call_refit(x, knots, gs, order, grid_old=grid_old, spline_w=R.scaled_coeff(w, sc))
    _ok(d, "refit")
    assert KR.bits_equal(a["out"], d["out"])
    # another column replaced, by other numbers and by NaN: every other feature keeps its bits
    others = [i for i in range(in_f) if i != 5]
    for fill in (torch.randn(B, generator=KR.gen(9)) * 0.5, torch.full((B,), float("nan"))):
        x2 = x.clone()
        x2[:, 5] = fill
        k2 = R.call_knots(x2, gs, order)
        _ok(k2, "knots")
        assert KR.bits_equal(k2["grid"][others], knots[others])
        e = R.call_refit(x2, k2["grid"], gs, order, grid_old=grid_old, spline_w=w, scaler=sc)
        _ok(e, "refit")                                                          # the call with the NaN column returns
        got, base = e["out"].view(w.shape), a["out"].view(w.shape)
        assert KR.bits_equal(got[:, others], base[:, others])
        assert bool(torch.isfinite(got[:, others]).all())


# --------------------------------------------------------------------------------------------------------------------
# refusals: nothing is written, and the text names the cause
# --------------------------------------------------------------------------------------------------------------------
def _refused(r, *words):
    assert r["status"] != 0 and r["untouched"], f"status {r['status']}, untouched {r['untouched']}"
    text = _err()
    assert all(w in text for w in words), text


def test_knots_refusals():
    x = R.knot_input(40, 16)
    for name in ("x", "ranks", "grid"):
        _refused(R.call_knots(x, 5, 3, null=(name,), check=False), "NULL")
    _refused(R.call_knots(x, 5, 3, B=0, check=False), "B = 0")
    _refused(R.call_knots(x, 20, 6, check=False), "unsupported knot count")
    _refused(R.call_knots(x, 0, 3, check=False), "unsupported knot count")
    _refused(R.call_knots(x, 5, 3, ws_bytes=-1, check=False), "workspace", "short")
    _refused(R.call_knots(x, 5, 3, ranks=torch.tensor([0, 8, 16, 24, 32, 40]), check=False), "ranks[5]")


def test_refit_refusals():
    B, in_f, out_f, gs, order, seed = R.FULL_RANK[0]
    x, grid_old, w, sc = R.full_rank_case(*R.FULL_RANK[0])
    knots = R.knot_rows(x, gs, order)
    s = dict(grid_old=grid_old, spline_w=w, scaler=sc)
    for name in ("x", "grid_new", "out", "ws"):
        _refused(R.call_refit(x, knots, gs, order, null=(name,), check=False, **s), "NULL")
    _refused(R.call_refit(x, knots, gs, order, B=0, check=False, **s), "B = 0")
    wide = torch.zeros(out_f, in_f, 26)
    _refused(R.call_refit(x, torch.zeros(in_f, 33), 20, 6, grid_old=torch.zeros(in_f, 33), spline_w=wide, check=False),
             "unsupported knot count")
    _refused(R.call_refit(x, knots, gs, order, ws_short=8, check=False, **s), "workspace", "short")
    _refused(R.call_refit(x, knots, gs, order, y=torch.zeros(B, in_f, out_f), check=False, **s), "both")
    _refused(R.call_refit(x, knots, gs, order, out_f=out_f, check=False), "neither")
    _refused(R.call_refit(x, knots, gs, order, grid_old=grid_old, out_f=out_f, check=False), "S-mode needs")


# --------------------------------------------------------------------------------------------------------------------
# KANLinear / KAN1
# --------------------------------------------------------------------------------------------------------------------
def _kan1():
    from ConNexT.models.block import kan1
    return kan1


def test_update_grid_does_not_synchronise():
    kan1 = _kan1()
    x = (torch.randn(40, 16, generator=KR.gen(5)) * 0.9).to(DEV)
    warm = load_procedural(kan1.KANLinear(16, 12), 1).to(DEV)
    warm.update_grid(x)
    warm(x)                                                              # library loaded, allocator pools warm
    lay = load_procedural(kan1.KANLinear(16, 12), 2).to(DEV)
    net = load_procedural(kan1.KAN1([16, 24, 8]), 3).to(DEV)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            probe.cpu()
        except RuntimeError:
            raised = True
        assert raised, "torch.cuda.set_sync_debug_mode('error') does not raise for .cpu() in this build: the test cannot see a sync"
        lay.update_grid(x)
        with torch.no_grad():
            y = net(x, update_grid=True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lay.spline_weight).all())


def test_update_grid_casts_a_non_f32_batch():
    kan1 = _kan1()
    x = (torch.randn(40, 16, generator=KR.gen(5)) * 0.9)
    a = load_procedural(kan1.KANLinear(16, 12), 2).to(DEV)
    b = load_procedural(kan1.KANLinear(16, 12), 2).to(DEV)
    a.update_grid(x.to(DEV).double())
    b.update_grid(x.to(DEV))
    assert KR.bits_equal(a.grid, b.grid) and KR.bits_equal(a.spline_weight.detach(), b.spline_weight.detach())


def test_module_curve2coeff_takes_the_device_route_on_gpu_tensors():
    from hamspine import kan as K
    kan1 = _kan1()
    g = KR.gen(12)
    x = torch.rand(60, 16, generator=g) * 2 - 1                          # spread over the initial knots' [-1, 1]: full rank
    y = torch.randn(60, 16, 12, generator=g)
    cpu = load_procedural(kan1.KANLinear(16, 12), 4)
    dev = load_procedural(kan1.KANLinear(16, 12), 4).to(DEV)
    got = dev.curve2coeff(x.to(DEV), y.to(DEV))
    assert got.is_cuda and tuple(got.shape) == (12, 16, 8)
    assert KR.bits_equal(got, K.kan_curve2coeff(x.to(DEV), y.to(DEV), dev.grid, 5, 3))
    ref = R.refit_ref64(x, cpu.grid, 3, y.permute(1, 0, 2).double())
    R.assert_comparable(ref, 60, 8, True)
    KR.gate("KANLinear.curve2coeff", got, cpu.curve2coeff(x, y), ref["sol"])     # the CPU module keeps the host lstsq


def test_module_route_reproduces_the_reference_vectors():
    kan1 = _kan1()
    g = np.load(os.path.join(gc.GOLDEN, "kan_update_grid.npz"))
    x = torch.from_numpy(g["x"]).to(DEV)
    lay = load_procedural(kan1.KANLinear(16, 12), gc.SEED + 87).to(DEV)
    host = load_procedural(kan1.KANLinear(16, 12), gc.SEED + 87).to(DEV)
    lay.update_grid(x)
    assert KR.bits_equal(lay.grid, torch.from_numpy(g["grid"]))
    assert torch.allclose(lay.grid.cpu(), torch.from_numpy(g["grid"]), atol=1e-6)
    assert torch.allclose(lay.spline_weight.detach().cpu(), torch.from_numpy(g["spline_weight"]), atol=2e-4, rtol=1e-3)
    assert torch.allclose(lay(x).cpu(), torch.from_numpy(g["out_after"]), atol=1e-4)
    # the host route stays reachable and agrees
    host._update_grid_host(x)
    assert KR.bits_equal(host.grid, lay.grid)
    assert torch.allclose(host.spline_weight.detach().cpu(), lay.spline_weight.detach().cpu(), atol=2e-4, rtol=1e-3)


def test_layer_output_is_preserved_within_the_fits_own_residual():
    kan1 = _kan1()
    x = torch.randn(40, 16, generator=KR.gen(5)) * 0.9
    lay = load_procedural(kan1.KANLinear(16, 12), gc.SEED + 87)
    coeff = R.scaled_coeff(lay.spline_weight.detach(), lay.spline_scaler.detach())
    knots = R.knot_rows(x, 5, 3, lay.grid_eps)
    ref = R.refit_ref64(x, knots, 3, R.targets64(x, lay.grid, coeff, 3))
    R.assert_comparable(ref, 40, 8, True)
    delta64 = (ref["fitted"] - R.targets64(x, lay.grid, coeff, 3)).sum(0)          # (B, out): what the exact fit changes
    after_coeff = ref["sol"].float() * lay.spline_scaler.detach().unsqueeze(-1)    # the forward scales the new weights again
    rounding = R.forward_rounding(x, lay.grid, 3, coeff, lay.base_weight.detach()) \
        + R.forward_rounding(x, knots, 3, after_coeff, lay.base_weight.detach())
    # the layer re-applies the scaler to coefficients that were fitted to the scaled ones (kan1.py:214): the output after the
    # update is the forward of sol * scaler, and that is what the float64 side evaluates too
    after64 = torch.einsum("ibp,oip->bo", ref["A"], after_coeff.double())
    before64 = R.targets64(x, lay.grid, coeff, 3).sum(0)
    lay = lay.to(DEV)
    with torch.no_grad():
        out_before = lay(x.to(DEV)).cpu().double()
        lay.update_grid(x.to(DEV))
        out_after = lay(x.to(DEV)).cpu().double()
    change, change64 = out_after - out_before, after64 - before64
    scale = float(out_before.abs().max())
    print(f"relative change {float(change.abs().max()) / scale:.3e}, float64 fit {float(change64.abs().max()) / scale:.3e} "
          f"(unscaled fit residual {float(delta64.abs().max()) / scale:.3e}), forward rounding {rounding / scale:.3e}, "
          f"change - float64 change {float((change - change64).abs().max()) / scale:.3e}")
    assert float(change.abs().max()) <= float(change64.abs().max()) + rounding
    assert float((change - change64).abs().max()) <= rounding


def test_update_grid_does_not_materialise_the_batch_in_out_tensor():
    kan1 = _kan1()
    B, in_f, out_f = 64, 1536, 512
    lay = kan1.KANLinear(in_f, out_f).to(DEV)
    x = (torch.randn(B, in_f, generator=KR.gen(6)) * 0.9).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lay.update_grid(x)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print(f"peak growth {growth} bytes, the (batch, in, out) tensor {B * in_f * out_f * 4}")
    assert growth < B * in_f * out_f * 4 // 4
    assert bool(torch.isfinite(lay.spline_weight).all()) and bool(torch.isfinite(lay.grid).all())
