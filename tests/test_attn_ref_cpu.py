"""The attention reference of attn_ref.py against float64 autograd, the constants of its gates against the emulation, and
the gates against subtly wrong kernels (mutants of the emulation).  No GPU."""
import pytest
import torch

import attn_ref as R


@pytest.fixture(scope="module")
def table():
    """per case: inputs, reference and emulation, computed once and left unchanged"""
    out = {}
    for c in R.CASES:
        inp = R.inputs(c)
        out[c.name] = (c, inp, R.attention_ref(**inp), R.attention_emulated(**inp, dtype=c.dtype))
    return out


def _autograd(q, k, v, d_o, heads, scale, key_mask, keep, inv_keep):
    B, Lq, D = q.shape
    Lk, hd = k.shape[1], D // heads
    qr, kr, vr = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    s = qr.view(B, Lq, heads, hd).transpose(1, 2) @ kr.view(B, Lk, heads, hd).transpose(1, 2).transpose(-1, -2) * scale
    if key_mask is not None:
        # added, as BERT's extended mask is: the sum rounds to exactly the fill value, and the gradient of a fully masked (uniform)
        # row still reaches q and k, as in the kernels, where masked_fill would cut it
        s = s + (key_mask[:, None, None, :] == 0).double() * R.MASK_FILL
        assert torch.equal(s[(key_mask == 0)[:, None, None, :].expand_as(s)].unique(), torch.tensor([R.MASK_FILL]).double())
    P = torch.softmax(s, -1)
    Pd = P if keep is None else P * keep.double() * inv_keep
    o = (Pd @ vr.view(B, Lk, heads, hd).transpose(1, 2)).transpose(1, 2).reshape(B, Lq, D)
    (o * d_o.double()).sum().backward()
    return P.detach(), Pd.detach(), o.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("name", ["hd32_49x49_bf16", "hd64_130x200_holes", "hd64_128x128_full", "hd32_49x49_p0.5",
                                  "hd64_130x200_p0.1", "hd64_128x128_sharp", "hd64_130x200_scale0.3"])
def test_reference_matches_float64_autograd(table, name):
    c, inp, ref, _ = table[name]
    auto = _autograd(inp["q"], inp["k"], inp["v"], inp["d_o"], inp["heads"], inp["scale"], inp["key_mask"], inp["keep"],
                     inp["inv_keep"])
    for what, a, b in zip(("P", "Pd", "o", "dq", "dk", "dv"), ref[:6], auto):
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
        assert err <= 1e-12, f"{name} {what}: {err:.3e}"


def test_reference_with_mask_and_keep_matches_autograd():
    """mask and keep together (no case of the list has both)"""
    c = R.Case("mask_and_keep", 32, 21, 19, mask="holes", p=0.5)
    inp = R.inputs(c)
    ref = R.attention_ref(**inp)
    auto = _autograd(inp["q"], inp["k"], inp["v"], inp["d_o"], inp["heads"], inp["scale"], inp["key_mask"], inp["keep"],
                     inp["inv_keep"])
    for what, a, b in zip(("P", "Pd", "o", "dq", "dk", "dv"), ref[:6], auto):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), what


def test_fully_masked_rows_are_uniform(table):
    c, inp, ref, _ = table["hd64_130x200_full"]
    assert torch.equal(ref.P[1], torch.full_like(ref.P[1], 1.0 / c.Lk))
    assert all(torch.isfinite(t).all() for t in ref[:6])


def test_keep_mask_is_the_flat_dropout_mask():
    """keep_mask is elem_ref's mask at flat index ((b * H + h) * Lq + q) * Lk + key, also where Lk is no multiple of 4"""
    B, H, Lq, Lk, p = 2, 3, 5, 7, 0.3
    m = R.keep_mask(R.DROP_SEED, B, H, Lq, Lk, p)
    for b, h, q, key in ((0, 0, 0, 0), (1, 2, 4, 6), (1, 0, 3, 5), (0, 2, 1, 2)):
        idx = ((b * H + h) * Lq + q) * Lk + key
        assert bool(m[b, h, q, key]) == bool(R.dropout_keep_ref(R.DROP_SEED, [idx], p)[0])
    big = R.keep_mask(R.DROP_SEED, 2, 2, 130, 200, 0.1).double().mean().item()
    assert abs(big - 0.9) < 0.01, big


def test_constants_track_the_emulation(table):
    """every constant is at least 4x and at most 8x the worst ratio the emulation reaches over the GPU cases of its type"""
    worst = {"bf16": {}, "f32": {}}
    for c, inp, ref, emu in table.values():
        for n, (w, _) in R.output_ratios(emu, ref, c.u, rowsum=c.dtype == "bf16").items():
            worst[c.dtype][n] = max(worst[c.dtype].get(n, 0.0), w)
    for dt, consts in (("bf16", R.C_BF16), ("f32", R.C_F32)):
        print(dt, {n: round(w, 3) for n, w in worst[dt].items()}, consts)
        assert set(consts) == set(worst[dt])
        for n, cst in consts.items():
            assert 4 * worst[dt][n] <= cst <= 8 * worst[dt][n], f"{dt} {n}: constant {cst}, emulation ratio {worst[dt][n]:.4g}"


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_gates_reject_mutant(table, mutant):
    killed = []
    for c, inp, ref, _ in table.values():
        bad = R.failures(R.attention_emulated(**inp, dtype=c.dtype, mutant=mutant), ref, c)
        if bad:
            killed.append((c.name, bad))
    print(f"{mutant}: rejected on {len(killed)} of {len(table)} cases, first {killed[:3]}")
    assert killed, f"{mutant} passes every case: the scales or the cases are too weak"
    if mutant == "scale":
        sharp = [c.name for c in R.CASES if c.sharp]
        assert sharp and all(any(n == s for n, _ in killed) for s in sharp)


def test_emulation_passes_its_own_gates(table):
    for c, inp, ref, emu in table.values():
        assert R.failures(emu, ref, c) == [], c.name


# ----------------------------------------------------------------------------------------------------------------------
# why the per-element gate exists: the max-norm gate of the older attention tests, with their mask, accepts two of the mutants
# ----------------------------------------------------------------------------------------------------------------------
def _old_inputs(H, hd, Lq, Lk, B=3):
    """test_attention_long_gpu._inputs at (4, 64, 130, 200, masked): batch 2 keeps only 5 keys"""
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q = torch.randn(B, Lq, H * hd, generator=g).bfloat16().float()
    k, v = (torch.randn(B, Lk, H * hd, generator=g).bfloat16().float() for _ in range(2))
    cot = torch.randn(B, Lq, H * hd, generator=g).bfloat16().float()
    mask = torch.ones(B, Lk, dtype=torch.long)
    mask[0, Lk // 2:] = 0
    mask[2, 5:] = 0
    return dict(q=q, k=k, v=v, d_o=cot, heads=H, scale=hd ** -0.5, key_mask=mask)


def _old_gate_ok(res, ref):
    ok = True
    for n, rtol in (("o", 2e-2), ("dq", 3e-2), ("dk", 3e-2), ("dv", 3e-2)):
        got, want = getattr(res, n), getattr(ref, n)
        ok = ok and (got - want).abs().max().item() <= rtol * want.abs().max().item() + 2e-6
    return ok


@pytest.mark.parametrize("mutant", ["delta128", "miss_chunk2_dk", "miss_chunk2_dv"])
def test_old_max_norm_gate_accepts_what_the_new_gate_rejects(mutant):
    """At (4, 64, 130, 200) with the old mask, batch 2 (5 keys, every query's gradient on them) alone sets max|ref|: 8.1 for dk
    and 10.9 for dv, against 0.8 and 0.7 in the unmasked batch 1.  The delta mutant passes the old gate as it is (dq off by
    0.0298 x max|ref|, bound 0.03).  A missing query chunk passes it where it strikes the unmasked batch: there the two lost
    rows cost 0.18 in dk and 0.20 in dv, a quarter of that batch's largest element and under the 0.24 and 0.33 allowed; in
    batches 0 and 2 they cost 0.34 and 1.5, which the old gate sees.  So the mutant is spliced: batch 1 from the mutant, the
    others from the correct emulation."""
    inp = _old_inputs(4, 64, 130, 200)
    ref = R.attention_ref(**inp)
    good = R.attention_emulated(**inp)
    bad = R.attention_emulated(**inp, mutant=mutant)
    if mutant != "delta128":
        bad = bad._replace(**{n: torch.cat([getattr(good, n)[:1], getattr(bad, n)[1:2], getattr(good, n)[2:]]) for n in ("dk", "dv")})
    assert _old_gate_ok(bad, ref), "the old gate was expected to let this mutant through"
    case = R.Case("old", 64, 130, 200, H=4, B=3)
    assert R.failures(bad, ref, case), "the per-element gate must reject it on the same inputs"
    assert R.failures(good, ref, case) == []
