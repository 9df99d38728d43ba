"""The float64 references and float32 yardsticks of tests/kernel_ref.py, checked on the CPU.

Each *_ref64 must equal torch.autograd on the matching float64 torch expression to 1e-12 relative; each *_yard must differ
from it by a non-zero amount below 1e-4 relative on f32 inputs (it really is single precision, and sane); the integer-data
generators keep every partial sum below 2^24; and for the BatchNorm cases and seeds the GPU tests use, the share of elements
whose ReLU sign is undecidable at the yardstick's precision stays below 0.1%.
"""
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr

F64 = torch.float64


def _close(a, b, what):
    e = kr.maxrel(a, b)
    assert e <= 1e-12, f"{what}: {e:.3e}"


def _single(yard, ref, what, reduced=False):
    e = (kr.rel if reduced else kr.maxrel)(yard, ref)
    assert 0.0 < e < 1e-4, f"{what}: {e:.3e}"


@pytest.mark.parametrize("M,H", [(3, 8), (7, 260)])
def test_layernorm_ref64_is_autograd(M, H):
    g = kr.gen(1)
    x, dy, gamma, beta = kr.ln_data(g, M, H, torch.float32)
    eps = 1e-5
    xt, gt, bt = (t.double().requires_grad_() for t in (x, gamma, beta))
    y = F.layer_norm(xt, (H,), gt, bt, kr._f32(eps))
    y.backward(dy.double())
    f = kr.ln_fwd_ref64(x, gamma, beta, eps)
    _close(f["y"], y.detach(), "y")
    _close(f["mean"], x.double().mean(1), "mean")
    _close(f["rstd"], 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + kr._f32(eps)), "rstd")
    keep = (torch.rand(M, H, generator=g) > 0.3).double() / 0.7
    b = kr.ln_bwd_ref64(dy, x, gamma, f["mean"], f["rstd"], keep)
    _close(b["dx"], xt.grad, "dx")
    _close(b["dgamma"], gt.grad, "dgamma")
    _close(b["dbeta"], bt.grad, "dbeta")
    _close(b["dx_dropped"], xt.grad * keep, "dx_dropped")
    _close(b["dbias"], (xt.grad * keep).sum(0), "dbias")
    # the yardstick
    fy = kr.ln_fwd_yard(x, gamma, beta, eps, torch.float32)
    for k in ("y", "mean", "rstd"):
        _single(fy[k], f[k], k)
    m32, r32 = f["mean"].float(), f["rstd"].float()
    br = kr.ln_bwd_ref64(dy, x, gamma, m32, r32, keep.float())
    by = kr.ln_bwd_yard(dy, x, gamma, m32, r32, torch.float32, keep.float())
    for k in ("dx", "dx_dropped"):
        _single(by[k], br[k], k)
    for k in ("dgamma", "dbeta", "dbias"):
        _single(by[k], br[k], k, reduced=True)


@pytest.mark.parametrize("rows,Lk,rpb", [(6, 5, 2), (9, 68, 3)])
def test_softmax_ref64_is_autograd(rows, Lk, rpb):
    g = kr.gen(2)
    S = 4.0 * torch.randn(rows, Lk, generator=g)
    dP = torch.randn(rows, Lk, generator=g)
    mask = kr.softmax_mask(3, Lk, g)
    keep = (torch.rand(rows, Lk, generator=g) > 0.1).float() / 0.9
    st = S.double().requires_grad_()
    b = torch.arange(rows) // rpb
    sm = st.masked_fill(mask[b] == 0, kr.MASK_FILL)
    sm.retain_grad()            # dS is the gradient of the masked scores (the fill cuts it off from S itself)
    P = torch.softmax(sm, dim=1)
    (P * keep.double()).backward(dP.double())
    f = kr.softmax_fwd_ref64(S, mask, rpb, keep)
    _close(f["P"], P.detach(), "P")
    _close(f["P_drop"], P.detach() * keep, "P_drop")
    assert torch.equal(f["P"][2 * rpb:3 * rpb], torch.full((rpb, Lk), 1.0 / Lk, dtype=F64))      # all keys masked: uniform
    _close(kr.softmax_bwd_ref64(dP, f["P"], keep)["dS"], sm.grad, "dS")
    fy = kr.softmax_fwd_yard(S, mask, rpb, torch.float32, keep)
    _single(fy["P"], f["P"], "P")
    _single(fy["P_drop"], f["P_drop"], "P_drop")
    P32 = f["P"].float()
    _single(kr.softmax_bwd_yard(dP, P32, torch.float32, keep)["dS"], kr.softmax_bwd_ref64(dP, P32, keep)["dS"], "dS")


@pytest.mark.parametrize("M,N", [(5, 3), (300, 12)])
def test_colsum_ref64_is_sum(M, N):
    g = kr.gen(3)
    x = torch.randn(M, N, generator=g)
    prior = torch.randn(N, generator=g)
    _close(kr.colsum_ref64(x)["out"], x.double().sum(0), "out")
    _close(kr.colsum_ref64(x, prior)["out"], prior.double() + x.double().sum(0), "out+")
    _single(kr.colsum_yard(x)["out"], kr.colsum_ref64(x)["out"], "yard", reduced=True)
    _single(kr.colsum_yard(x, prior)["out"], kr.colsum_ref64(x, prior)["out"], "yard+", reduced=True)


@pytest.mark.parametrize("M,Cc", [(2, 4), (65, 12)])
@pytest.mark.parametrize("training", [1, 0])
def test_batchnorm_ref64_is_autograd(M, Cc, training):
    x, res, dy, gamma, beta, rm, rv = kr.bn_data(Cc, M, "plain", 7, torch.float32)
    eps, mo = 1e-5, 0.1
    xt, rt_, gt, bt = (t.double().requires_grad_() for t in (x, res, gamma, beta))
    r1, r2 = rm.double().clone(), rv.double().clone()
    pre = F.batch_norm(xt, r1, r2, gt, bt, bool(training), kr._f32(mo), kr._f32(eps)) + rt_
    y = torch.relu(pre)
    y.backward(dy.double())
    f = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, eps, mo, training, 1, res)
    _close(f["y"], y.detach(), "y")
    _close(f["pre"], pre.detach(), "pre")
    if training:
        _close(f["running_mean"], r1, "running_mean")
        _close(f["running_var"], r2, "running_var")
        F.batch_norm(x.double(), r1, r2, gt, bt, True, kr._f32(mo), kr._f32(eps))
        f2 = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, eps, mo, 1, 1, res, calls=2)
        _close(f2["running_mean"], r1, "running_mean after two calls")
        _close(f2["running_var"], r2, "running_var after two calls")
        _close(f["save_mean"], x.double().mean(0), "save_mean")
    _close(f["scale"] * x.double() + f["shift"] + res.double(), pre.detach(), "scale / shift")
    b = kr.bn_bwd_ref64(dy, x, gamma, f["save_mean"], f["save_invstd"], training, f["pre"] > 0)
    _close(b["dx"], xt.grad, "dx")
    _close(b["dres"], rt_.grad, "dres")
    _close(b["dgamma"], gt.grad, "dgamma")
    _close(b["dbeta"], bt.grad, "dbeta")
    fy = kr.bn_fwd_yard(x, gamma, beta, rm, rv, eps, mo, training, 1, torch.float32, res)
    keys = ["scale", "shift", "y", "save_invstd"] + (["save_mean", "running_mean", "running_var"] if training else [])
    for k in keys:
        _single(fy[k], f[k], k)
    m32, i32 = f["save_mean"].float(), f["save_invstd"].float()
    mask = f["pre"] > 0
    br = kr.bn_bwd_ref64(dy, x, gamma, m32, i32, training, mask)
    by = kr.bn_bwd_yard(dy, x, gamma, m32, i32, training, torch.float32, mask)
    _single(by["dx"], br["dx"], "dx")
    _single(by["dgamma"], br["dgamma"], "dgamma", reduced=True)
    _single(by["dbeta"], br["dbeta"], "dbeta", reduced=True)
    assert kr.bits_equal(by["dres"], br["dres"].float())


def test_integer_data_keeps_partial_sums_exact():
    """the largest integer-data case of the GPU tests: any partial sum, in any order, is bounded by the sum of magnitudes"""
    for rows, cols in ((20000, 8), (8209, 8), (5003, 64), (1000, 520)):
        x = kr.int_data(kr.gen(5), rows, cols)
        assert x.abs().max().item() <= 8 and torch.equal(x, x.round())
        assert x.abs().double().sum(0).max().item() < 2 ** 24
        assert kr.bits_equal(kr.colsum_yard(x)["out"], kr.colsum_ref64(x)["out"].float())
    assert 8 * 2 ** 20 < 2 ** 24


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_batchnorm_relu_band_is_thin_for_the_seeds_used(dtype):
    """the share of elements whose ReLU sign the yardstick cannot decide stays below 0.1% in every case (reference alone)"""
    for Cc, M, kind, seed in kr.bn_cases(dtype):
        x, res, dy, gamma, beta, rm, rv = kr.bn_data(Cc, M, kind, seed, dtype)
        for training in (1, 0):
            for r in (None, res):
                ref = kr.bn_fwd_ref64(x, gamma, beta, rm, rv, 1e-5, 0.1, training, 1, r)
                yard = kr.bn_fwd_yard(x, gamma, beta, rm, rv, 1e-5, 0.1, training, 1, dtype, r)
                fl = kr.bn_fwd_floors(x, gamma, beta, ref, training, 1e-5, r)
                share = kr.bn_relu_band(ref, yard, fl["pre_abs"]).double().mean().item()
                assert share < 1e-3, (Cc, M, kind, seed, training, r is not None, share)
