"""The attention core (hs_attention_fwd / hs_attention_bwd) element by element against float64: the four fused forward
instantiations, the four fused backward kernels and the GEMM + softmax path behind them, through the C ABI so that strides,
seed and the saved buffer are the test's own.  References, error scales, constants and the case list are attn_ref's;
test_attn_ref_cpu.py shows on the CPU that these gates reject a dropped key, a dropped query row, a mask from the wrong batch,
a delta over one key block, a missing query chunk, a missing 1 / (1 - p), a shifted dropout mask, a scale off by 2^-4 and a
truncated P.

Every case first asserts the path that ran (GEMM launches of the profile hook: 0 = fused), then gates o, P, dq, dk, dv and
the row sums of P with no element left out, and checks that nothing outside the addressed elements was written."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402,F401

import attn_ref as R  # noqa: E402

_BY_NAME = {c.name: c for c in R.CASES}


@functools.lru_cache(maxsize=None)
def _run(name):
    """inputs, float64 reference and the library's results of a case, computed once and left unchanged"""
    case = _BY_NAME[name]
    inp = R.inputs(case)
    return case, inp, R.attention_ref(**inp), R.run_case(case, inp)


def _where(case, what, at):
    if what in ("P", "rowsum"):
        return "(batch, head, row" + (", key) " if what == "P" else ") ") + str(at)
    b, row, col = at
    return f"(batch, head, row, column) {(b, col // case.hd, row, col % case.hd)}"


def _gate_all(case, ref, res):
    fwd_k, bwd_k = R.kernels_of(case)
    ratios = R.output_ratios(res, ref, case.u, rowsum=case.dtype == "bf16")
    print(f"{case.name}: " + "  ".join(f"{n} {w:.3f}/{case.consts[n]}" for n, (w, _) in ratios.items())
          + f"   [{fwd_k} | {bwd_k}]")
    bad = [f"{n}: worst element {_where(case, n, at)} is off by {w:.4g} x u x S, allowed {case.consts[n]} "
           f"({fwd_k if n in ('o', 'P', 'rowsum') else bwd_k})"
           for n, (w, at) in ratios.items() if not w <= case.consts[n]]
    assert not bad, f"{case.name}: " + "; ".join(bad)
    return ratios


def _bf16_ulp(x):
    """one unit in the last place of bf16 at |x| (normal range)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_attention_matches_float64(name):
    case, inp, ref, res = _run(name)
    # the path meant is the one that ran
    if case.fused:
        assert (res["fwd_gemms"], res["bwd_gemms"]) == (0, 0), f"{name}: GEMM launches {res['fwd_gemms']}, {res['bwd_gemms']}"
    else:
        assert res["fwd_gemms"] > 0 and res["bwd_gemms"] > 0, f"{name}: GEMM launches {res['fwd_gemms']}, {res['bwd_gemms']}"
    for n in ("o", "dq", "dk", "dv", "P"):
        assert torch.isfinite(res[n]).all(), f"{name}: {n} has inf or NaN"
    _gate_all(case, ref, res)
    # nothing outside the addressed elements changed; the padding columns of P are zeros
    assert res["outside_untouched"], f"{name}: an element outside the o / dq / dk / dv windows was written"
    assert res["saved_tail_untouched"], f"{name}: bytes past saved_bytes were written"
    assert (res["P_pad"] == 0).all(), f"{name}: padding columns of P are not zero"
    if case.mask == "full":
        P1 = res["P"][1]
        assert (P1 == P1.flatten()[0]).all(), f"{name}: P of the fully masked batch is not uniform"
    if case.p > 0:
        keep, ik = inp["keep"], inp["inv_keep"]
        P, Pd = res["P"], res["Pd"]
        assert Pd is not None and (res["Pd_pad"] == 0).all()
        sure = ref.P > 2.0 ** -126
        assert torch.equal((Pd != 0)[sure], keep[sure]), (
            f"{name}: {int(((Pd != 0) != keep)[sure].sum())} kept positions differ from keep_mask")
        assert (Pd[~keep] == 0).all()
        # the forward rounds its float32 p * inv_keep, the stored P is that p rounded: the two roundings are grid neighbours at most
        want = (P * keep.double() * ik).float().bfloat16().double()
        off = ((Pd - want).abs() / _bf16_ulp(torch.maximum(Pd.abs(), want.abs()))).max().item()
        print(f"{name}: Pd against bf16(P * inv_keep) of the kernel's own P: {off:.3f} ulp")
        assert off <= 1.0, f"{name}: Pd is {off:.3f} bf16 ulp from its own P * inv_keep"
    else:
        assert res["Pd"] is None


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_and_fallback_draw_the_same_mask(p):
    """Same seed, B, H, Lq and Lk: the fused kernels (head dim 32) and the GEMM + softmax path (head dim 16) keep the same
    positions.  49 keys: the flat index of a row's first key is not a multiple of 4, the element-by-element hash path."""
    cf, _, ref_f, fused = _run(f"hd32_49x49_p{p}")
    cu, _, ref_u, unfused = _run(f"hd16_49x49_p{p}")
    assert (cf.B, cf.H, cf.Lq, cf.Lk) == (cu.B, cu.H, cu.Lq, cu.Lk)
    assert (fused["fwd_gemms"], fused["bwd_gemms"]) == (0, 0) and unfused["fwd_gemms"] > 0 and unfused["bwd_gemms"] > 0
    sure = (ref_f.P > 2.0 ** -126) & (ref_u.P > 2.0 ** -126)
    assert torch.equal((fused["Pd"] != 0)[sure], (unfused["Pd"] != 0)[sure])


@pytest.mark.parametrize("override,word", [({"Lk": 1025}, "1025"), ({"B": 0}, "bad dims"), ({"hd": 0}, "bad dims")])
def test_refused_shapes_touch_nothing(override, word):
    """Lk = 1025, B = 0 and hd = 0: every entry point returns an error status, hs_last_error says why, and the sentinel-filled
    outputs and the saved buffer stay as they were."""
    from hamspine import _lib as L
    case = _BY_NAME["hd64_40x37_bf16"]
    res = R.run_case(case, R.inputs(case), desc_override=override, check=False)
    for call in ("query_status", "fwd_status", "bwd_status"):
        assert res[call] != L.HS_OK, f"{override}: {call} reports success"
    assert word in res["error"], res["error"]
    assert res["outputs_untouched"] and res["saved_untouched"], f"{override}: a refused call wrote to its outputs"
    assert res["fwd_gemms"] == 0 and res["bwd_gemms"] == 0
