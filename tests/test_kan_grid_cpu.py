"""The float64 restatement of the KAN grid update (tests/kan_grid_ref.py) against the reference's recorded vectors, the
formulation the kernels use against the materialised one, the input guards of every compared case, and the new C ABI entries.
No GPU; the ABI test needs the built library."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import kan_grid_ref as R
import kernel_ref as KR
from oracle.procedural import load_procedural


def _layer(in_f, out_f, seed):
    from ConNexT.models.block import kan1
    return load_procedural(kan1.KANLinear(in_f, out_f), seed)


def _update64(lay, x):
    """the restated update on a CPU layer's parameters -> knots (f32), coefficients (f64), the reference's figures"""
    coeff = R.scaled_coeff(lay.spline_weight.detach(), lay.spline_scaler.detach())
    knots = R.knot_rows(x, lay.grid_size, lay.spline_order, lay.grid_eps)
    ref = R.refit_ref64(x, knots, lay.spline_order, R.targets64(x, lay.grid, coeff, lay.spline_order))
    return knots, ref


def test_reference_reproduces_the_single_layer_vectors():
    g = np.load(os.path.join(gc.GOLDEN, "kan_update_grid.npz"))
    x = torch.from_numpy(g["x"])
    knots, ref = _update64(_layer(16, 12, gc.SEED + 87), x)
    assert KR.bits_equal(knots, torch.from_numpy(g["grid"]))
    want = torch.from_numpy(g["spline_weight"])
    print("coefficients: max |diff|", float((ref["sol"].float() - want).abs().max()))
    assert torch.allclose(ref["sol"].float(), want, atol=R.ATOL, rtol=R.RTOL)


def test_reference_reproduces_the_stack_vectors():
    from ConNexT.models.block import kan1
    g = np.load(os.path.join(gc.GOLDEN, "kan1_stack_update_grid.npz"))
    net = load_procedural(kan1.KAN1([16, 24, 8]), gc.SEED + 88)
    x = torch.from_numpy(g["x"])
    for n, lay in enumerate(net.layers):
        knots, ref = _update64(lay, x)
        assert KR.bits_equal(knots, torch.from_numpy(g[f"grid{n}"])), f"layer {n}"
        assert torch.allclose(ref["sol"].float(), torch.from_numpy(g[f"spline{n}"]), atol=R.ATOL, rtol=R.RTOL), f"layer {n}"
        # the next layer's input: this layer's forward on the recorded knots and coefficients, operation by operation as the
        # reference computed it (kan1.py:152-165), so that the next layer's knots can be compared bitwise
        with torch.no_grad():
            coeff = R.scaled_coeff(torch.from_numpy(g[f"spline{n}"]), lay.spline_scaler)
            S = R.bases(x, torch.from_numpy(g[f"grid{n}"]), lay.spline_order)
            x = torch.nn.functional.linear(torch.nn.functional.silu(x), lay.base_weight) \
                + torch.nn.functional.linear(S.view(x.size(0), -1), coeff.view(coeff.size(0), -1))
    assert torch.allclose(x, torch.from_numpy(g["out"]), atol=2e-4)


def test_pseudo_inverse_form_equals_the_materialised_form():
    """(A^+ S) C, the form the kernels evaluate, against A^+ (S C) over the (batch, in, out) tensor, both in float64"""
    x, grid_old, w, sc = R.full_rank_case(*R.FULL_RANK[0])
    order = R.FULL_RANK[0][4]
    coeff = R.scaled_coeff(w, sc).double()
    knots = R.knot_rows(x, R.FULL_RANK[0][3], order)
    ref = R.refit_ref64(x, knots, order, R.targets64(x, grid_old, coeff, order))
    A = ref["A"]
    S = R.bases(x.double(), grid_old, order).permute(1, 0, 2)
    M = torch.stack([torch.linalg.pinv(A[i]) @ S[i] for i in range(A.shape[0])])              # (in, nb, nb)
    sol = torch.einsum("ipq,oiq->oip", M, coeff)
    err = KR.maxrel(sol, ref["sol"])
    print("(A^+ S) C against A^+ (S C):", err)
    assert err <= 1e-11


@pytest.mark.parametrize("case", R.FULL_RANK, ids=lambda c: "x".join(map(str, c[:5])))
def test_full_rank_inputs_satisfy_the_guard(case):
    B, in_f, out_f, gs, order, seed = case
    x, grid_old, w, sc = R.full_rank_case(*case)
    coeff = R.scaled_coeff(w, sc)
    ref = R.refit_ref64(x, R.knot_rows(x, gs, order), order, R.targets64(x, grid_old, coeff, order))
    print(f"condition <= {max(ref['cond']):.3g}, kept >= {min(ref['kept']):.3g}x the cutoff")
    R.assert_comparable(ref, B, gs + order, full_rank=True)


@pytest.mark.parametrize("name", sorted(R.RANK_DEFICIENT))
def test_rank_deficient_inputs_satisfy_the_guard(name):
    B, in_f, out_f, rank = R.RANK_DEFICIENT[name]
    x, grid_old, w, sc = R.deficient_case(name)
    ref = R.refit_ref64(x, R.knot_rows(x, 5, 3), 3, R.targets64(x, grid_old, R.scaled_coeff(w, sc), 3))
    print(f"rank {set(ref['rank'])}, kept >= {min(ref['kept']):.3g}x, dropped <= {max(ref['dropped']):.3g}x the cutoff")
    assert set(ref["rank"]) == {rank}
    R.assert_comparable(ref, B, 8, full_rank=False)
    assert bool(torch.isfinite(ref["sol"]).all())


def test_guard_refuses_an_input_on_the_cutoff():
    """the guard is not vacuous: a feature whose smallest singular value sits within 10x of the cutoff is refused"""
    fake = {"kept": [3.0], "dropped": [0.0], "rank": [8], "cond": [50.0]}
    with pytest.raises(AssertionError):
        R.assert_comparable(fake, 40, 8, full_rank=True)
    fake = {"kept": [1e3], "dropped": [0.0], "rank": [8], "cond": [4e5]}
    with pytest.raises(AssertionError):
        R.assert_comparable(fake, 8, 8, full_rank=True)


def test_header_declares_and_the_binding_types_the_new_entries():
    import hamspine._lib as L
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    expected = {
        "hs_kan_grid_knots_ws_bytes": (i64, [i64, i32, i32, i32]),
        "hs_kan_grid_knots": (i32, [vp, vp, vp, i64, i32, i32, i32, f32, f32, f32, vp, i64, vp]),
        "hs_kan_refit_ws_bytes": (i64, [i64, i32, i32, i32, i32, i32]),
        "hs_kan_refit": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, i64, vp]),
    }
    names = L.exported_symbols()
    lib = L.lib()
    for n, (ret, args) in expected.items():
        assert n in names, n
        assert getattr(lib, n).restype is ret and list(getattr(lib, n).argtypes) == args, n
    # the size queries run on the host: supported and refused shapes
    assert lib.hs_kan_grid_knots_ws_bytes(40, 16, 5, 3) == 0
    assert lib.hs_kan_grid_knots_ws_bytes(0, 16, 5, 3) == -1 and lib.hs_kan_grid_knots_ws_bytes(40, 16, 20, 6) == -1
    assert lib.hs_kan_refit_ws_bytes(40, 16, 12, 5, 3, 0) == 1 * 16 * 8 * 16 * 8
    assert lib.hs_kan_refit_ws_bytes(3000, 16, 12, 5, 3, 0) == 12 * 16 * 8 * 16 * 8          # 12 chunks of 256 rows
    assert lib.hs_kan_refit_ws_bytes(40, 16, 12, 5, 3, 1) == 1 * 16 * 8 * (8 + 12) * 8
    assert lib.hs_kan_refit_ws_bytes(40, 16, 12, 27, 2, 0) > 0 and lib.hs_kan_refit_ws_bytes(40, 16, 12, 28, 2, 0) == -1
    assert lib.hs_kan_refit_ws_bytes(0, 16, 12, 5, 3, 0) == -1
