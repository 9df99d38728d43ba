"""The references of tests/elem_ref.py against independent code (torch.optim, autograd, F.max_pool2d), and every yardstick
against its own a-priori float32 bound -- so that a wrong reference cannot pass a wrong kernel.  No GPU."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import elem_ref as er
from kernel_ref import EPS32, gen

U = EPS32
F64 = torch.float64


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_import_loads_no_gpu_library():
    import subprocess          # (a fresh interpreter: other tests of the session may have loaded the library)
    code = ("import sys; sys.path[:0] = %r; import elem_ref; "
            "assert not any(m.startswith('hamspine') for m in sys.modules), 'elem_ref imported hamspine'" % (sys.path,))
    subprocess.run([sys.executable, "-c", code], check=True)


# ----------------------------------------------------------------------------------------------------------------------
# optimizers
# ----------------------------------------------------------------------------------------------------------------------
def _opt_state(seed, n=257):
    g = gen(seed)
    p = 4.0 * torch.rand(n, generator=g) - 2.0
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    return p, grads


@pytest.mark.parametrize("decoupled", (0, 1))
@pytest.mark.parametrize("wd", (0.0, 0.05))
def test_adam_ref64_is_torch_adam(decoupled, wd):
    p0, grads = _opt_state(1)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    tp = p0.double().clone().requires_grad_(True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double()
    for k, g in enumerate(grads):
        tp.grad = g.double().clone()
        opt.step()
        r = er.adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, k + 1, decoupled, 1.0)
        p, m, v = (torch.from_numpy(r[kk]) for kk in ("p", "m", "v"))
        st = opt.state[tp]
        assert _rel(p, tp.detach()) <= 1e-12 and _rel(m, st["exp_avg"]) <= 1e-12 and _rel(v, st["exp_avg_sq"]) <= 1e-12


def test_adam_ref64_grad_scale_is_a_scaled_gradient():
    p0, grads = _opt_state(2)
    m, v = 0.1 * grads[1], 0.01 * grads[2].abs()
    a = er.adam_ref64(p0, grads[0], m, v, 1e-2, 0.9, 0.999, 1e-8, 0.05, 3, 0, 0.125)
    b = er.adam_ref64(p0, grads[0] * 0.125, m, v, 1e-2, 0.9, 0.999, 1e-8, 0.05, 3, 0, 1.0)
    for k in ("p", "m", "v"):
        assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize("momentum,nesterov", ((0.0, 0), (0.9, 0), (0.9, 1)))
@pytest.mark.parametrize("wd", (0.0, 1e-2))
def test_sgd_ref64_is_torch_sgd(momentum, nesterov, wd):
    p0, grads = _opt_state(3)
    lr = 0.05
    tp = p0.double().clone().requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum, weight_decay=wd, nesterov=bool(nesterov))
    p, buf = p0.double(), None
    for k, g in enumerate(grads):
        tp.grad = g.double().clone()
        opt.step()
        r = er.sgd_ref64(p, g, buf, lr, momentum, wd, nesterov, 1 if k == 0 else 0, 1.0)
        p = torch.from_numpy(r["p"])
        buf = None if r["buf"] is None else torch.from_numpy(r["buf"])
        assert _rel(p, tp.detach()) <= 1e-12
        if momentum:
            assert _rel(buf, opt.state[tp]["momentum_buffer"]) <= 1e-12


def test_optimizer_yardsticks_within_float32_bounds():
    """Adam: exp_avg carries the rounding of beta1 and 1 - beta1 and three operations: 6 u max|m|.  exp_avg_sq carries 1 - beta2
    rounded (u / (1 - beta2) relative on the new term) and four operations.  The update: sqrt(1 - beta2^step) inherits
    step u beta2^step / (1 - beta2^step) / 2 from beta2, the quotient chain ten roundings, denom half the error of exp_avg_sq,
    and the store update_floor.  SGD: six roundings on the gradient chain and the store."""
    p0, grads = _opt_state(4, 4096)
    m, v = 0.1 * grads[1], 0.01 * torch.rand(4096, generator=gen(5))
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    for step in (1, 2, 1000):
        for dec in (0, 1):
            a = (p0, grads[0], m, v, lr, b1, b2, eps, 0.05, step, dec, 0.125)
            r, y = er.adam_ref64(*a), er.adam_yard(*a)
            assert _rel(y["m"], r["m"]) <= 6 * U
            relv = U / (1 - b2) + 5 * U
            assert _rel(y["v"], r["v"]) <= relv
            bt = b2 ** step
            rel_u = 0.5 * step * U * bt / (1 - bt) + 0.5 * relv + 12 * U + step * U * b1 ** step / (1 - b1 ** step)
            bound = rel_u + er.update_floor(p0, r["p"])
            assert _rel(y["p"].astype(np.float64) - p0.double().numpy(), r["p"] - p0.double().numpy()) <= bound
    buf = grads[2]
    for mo, nes, first in ((0.0, 0, 0), (0.9, 0, 0), (0.9, 1, 0), (0.9, 1, 1)):
        a = (p0, grads[0], buf, 0.05, mo, 1e-2, nes, first, 0.5)
        r, y = er.sgd_ref64(*a), er.sgd_yard(*a)
        assert _rel(y["p"].astype(np.float64) - p0.double().numpy(), r["p"] - p0.double().numpy()) <= 8 * U + er.update_floor(p0, r["p"], 2)
        if mo:
            assert _rel(y["buf"], r["buf"]) <= 5 * U


def test_adam_yard_survives_a_gradient_whose_square_overflows():
    one = torch.ones(1)
    a = (one, 1e20 * one, 0.1 * one, 0.01 * one, 1e-2, 0.9, 0.999, 1e-8, 0.0, 1, 1, 1.0)
    r, y = er.adam_ref64(*a), er.adam_yard(*a)
    assert np.isfinite(y["p"]).all() and np.isfinite(y["v"]).all()
    assert _rel(y["p"] - 1.0, r["p"] - 1.0) <= 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# embeddings
# ----------------------------------------------------------------------------------------------------------------------
def _embed_data(seed, tokens, L, H, V):
    g = gen(seed)
    q = lambda *s, lim: torch.randint(-lim, lim + 1, s, generator=g).float() / 256.0     # multiples of 2^-8
    ids = torch.randint(0, V, (tokens,), generator=g)
    return (ids, q(V, H, lim=512), q(L, H, lim=192), q(H, lim=192), 1.0 + 0.3 * torch.randn(H, generator=g),
            torch.randn(H, generator=g))


def test_embed_refs_against_autograd():
    tokens, L, H, V = 12, 4, 20, 7
    ids, word, pos, type0, gamma, beta = _embed_data(10, tokens, L, H, V)
    ids[3], ids[5] = -3, V + 5
    eps = 1e-12
    r = er.embed_fwd_ref64(ids, word, pos, type0, gamma, beta, L, eps, torch.float32)
    w = word.double().requires_grad_(True)
    ps = pos.double().requires_grad_(True)
    s = TF.embedding(ids.clamp(0, V - 1), w) + ps[torch.arange(tokens) % L] + type0.double()
    y = TF.layer_norm(s, (H,), gamma.double(), beta.double(), float(np.float32(eps)))
    assert _rel(r["sum"].double(), s.detach()) == 0.0
    assert _rel(r["y"], y.detach()) <= 1e-12
    assert _rel(r["mean"], s.detach().mean(1)) <= 1e-12
    assert _rel(r["rstd"], 1.0 / torch.sqrt(s.detach().var(1, unbiased=False) + float(np.float32(eps)))) <= 1e-9
    # the backward: scatter of dsum into the word table (padding row untouched) and the sum over the batch for positions
    B = tokens // L
    dsum = torch.randn(tokens, H, generator=gen(11))
    pad = int(ids.clamp(0, V - 1)[0])
    w2 = word.double().requires_grad_(True)
    s2 = TF.embedding(ids.clamp(0, V - 1), w2, padding_idx=pad) + ps[torch.arange(tokens) % L]
    gw, gp = torch.autograd.grad((s2 * dsum.double()).sum(), (w2, ps))
    b = er.embed_bwd_ref64(ids, dsum, B, L, V, pad)
    assert _rel(b["dword"], gw) <= 1e-12 and bool((b["dword"][pad] == 0).all())
    assert _rel(b["dpos"], gp) <= 1e-12
    b2 = er.embed_bwd_ref64(ids, dsum, B, L, V, -1)
    assert _rel(b2["dword"], torch.autograd.grad((TF.embedding(ids.clamp(0, V - 1), w2) * dsum.double()).sum(), w2)[0]) <= 1e-12
    yb = er.embed_bwd_yard(ids, dsum, B, L, V, pad)
    assert _rel(yb["dword"], b["dword"]) <= tokens * U and _rel(yb["dpos"], b["dpos"]) <= B * U


@pytest.mark.parametrize("dtype", er.DTYPES, ids=er.dname)
def test_embed_yard_within_bound(dtype):
    """LayerNorm over H values of magnitude <= 6: the sequential sums carry H u, the rest a handful of roundings; bf16 adds one
    rounding of the output, 2^-8 relative."""
    tokens, L, H, V = 9, 4, 260, 11
    a = _embed_data(12, tokens, L, H, V)
    r = er.embed_fwd_ref64(*a, L, 1e-12, dtype, 0.1, 1234)
    y = er.embed_fwd_yard(*a, L, 1e-12, dtype, 0.1, 1234)
    assert er.bits_equal(y["sum"], r["sum"])
    out = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    assert _rel(y["y"].double(), r["y"]) <= (2 * H + 10) * U + out
    assert _rel(y["mean"], r["mean"]) <= (H + 2) * U and _rel(y["rstd"], r["rstd"]) <= (2 * H + 6) * U
    keep = r["keep"]
    assert bool(((r["y"] == 0) == ~keep).all()) and bool(((y["y"] == 0) == ~keep).all())


# ----------------------------------------------------------------------------------------------------------------------
# dropout mask
# ----------------------------------------------------------------------------------------------------------------------
SEEDS = (1234, 7, 0x0123456789ABCDEF)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", (0.1, 0.25, 0.5, 0.9))
def test_dropout_keep_fraction(seed, p):
    n = 1 << 20
    keep = er.dropout_keep_ref(seed, np.arange(n), p)
    q = 1.0 - np.floor(float(np.float32(p)) * 65536.0) / 65536.0
    sd = np.sqrt(q * (1.0 - q) / n)
    dev = abs(keep.mean() - q) / sd
    print(f"seed {seed:#x} p {p}: kept {keep.mean():.6f}, expected {q:.6f}, {dev:.2f} standard deviations")
    assert dev <= 4.0


def test_dropout_keep_properties():
    idx = np.arange(5000)
    assert er.dropout_keep_ref(1234, idx, 0.0).all()
    a = er.dropout_keep_ref(1234, idx, 0.25)
    assert np.array_equal(a, er.dropout_keep_ref(1234, idx[::-1], 0.25)[::-1])            # a function of (seed, index) only
    assert np.array_equal(a[1000:1003], er.dropout_keep_ref(1234, np.array([1000, 1001, 1002]), 0.25))
    assert not np.array_equal(a, er.dropout_keep_ref(1235, idx, 0.25))
    assert not np.array_equal(a, er.dropout_keep_ref(1234 + (1 << 32), idx, 0.25))          # the high seed word counts
    big = np.array([1 << 34, (1 << 34) + 1], dtype=np.uint64)                                # and so does the high index word
    assert er.dropout_keep_ref(7, big, 0.5).shape == (2,)
    # a keep at p is a keep at every smaller p (one threshold on the same bits)
    assert not (er.dropout_keep_ref(7, idx, 0.5) & ~er.dropout_keep_ref(7, idx, 0.1)).any()
    assert er.dropout_thresh16(0.1) == 6553 and er.dropout_thresh16(0.0) == 0
    x = torch.arange(1, 9, dtype=torch.float32)
    y, keep = er.dropout_ref(x, 0.5, 7)
    assert torch.equal(y, torch.where(keep, x * 2.0, torch.zeros(8)))


# ----------------------------------------------------------------------------------------------------------------------
# max pool
# ----------------------------------------------------------------------------------------------------------------------
POOL_CASES = ((2, 7, 5, 3, 2, 1), (1, 6, 6, 3, 1, 1), (2, 4, 6, 2, 2, 0), (1, 1, 1, 3, 2, 1), (1, 5, 5, 3, 2, 0))


@pytest.mark.parametrize("case", POOL_CASES)
@pytest.mark.parametrize("kind", ("ties", "negative"))
def test_maxpool_ref_is_torch(case, kind):
    N, H, W, k, s, p = case
    Cc = 4
    g = gen(20)
    if kind == "ties":
        x = torch.randint(-2, 3, (N, H, W, Cc), generator=g).float().clamp_min(0.0)          # many exact ties (post-ReLU zeros)
    else:
        x = -1.0 - torch.rand(N, H, W, Cc, generator=g)
    y, idx, bwd = er.maxpool_ref(x, k, s, p)
    xt = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    yt, it = TF.max_pool2d(xt, k, s, p, return_indices=True)
    assert torch.equal(y.double(), yt.detach().permute(0, 2, 3, 1))
    P, Q = yt.shape[2:]
    r, c = (idx // k).long(), (idx % k).long()
    hh = torch.arange(P)[None, :, None, None] * s - p + r
    ww = torch.arange(Q)[None, None, :, None] * s - p + c
    assert torch.equal(hh * W + ww, it.permute(0, 2, 3, 1)), "arg-max tap differs from torch's index"
    dy = torch.randint(-8, 9, (N, P, Q, Cc), generator=g).float()
    (gx,) = torch.autograd.grad(yt, xt, dy.permute(0, 3, 1, 2).double())
    assert torch.equal(bwd(dy.reshape(-1, Cc)).double(), gx.permute(0, 2, 3, 1))


# ----------------------------------------------------------------------------------------------------------------------
# the rest
# ----------------------------------------------------------------------------------------------------------------------
def test_gelu_bwd_ref_and_yard():
    """yardstick: erf correctly rounded, exp and five operations: 8 u of max|dy gelu'|, plus the output rounding for bf16"""
    g = gen(30)
    u = torch.cat([12.0 * torch.rand(2000, generator=g) - 6.0, torch.tensor([0.0, 10.0, -10.0, 40.0, -40.0])])
    dy = torch.randn(u.numel(), generator=g)
    ut = u.double().requires_grad_(True)
    (ga,) = torch.autograd.grad(TF.gelu(ut), ut, dy.double())
    ref = er.gelu_bwd_ref64(dy, u)
    assert _rel(ref, ga) <= 1e-12
    assert _rel(er.gelu_bwd_yard(dy, u, torch.float32).double(), ref) <= 8 * U
    ub, db = u.bfloat16(), dy.bfloat16()
    assert _rel(er.gelu_bwd_yard(db, ub, torch.bfloat16).double(), er.gelu_bwd_ref64(db, ub)) <= 8 * U + 2.0 ** -8


def test_mean_tokens_refs():
    g = gen(31)
    x, dy = torch.randn(3, 197, 8, generator=g), torch.randn(3, 8, generator=g)
    xt = x.double().requires_grad_(True)
    yt = xt.mean(1)
    (gx,) = torch.autograd.grad(yt, xt, dy.double())
    r = er.mean_tokens_ref64(x, dy)
    assert _rel(r["y"], yt.detach()) <= 1e-13 and _rel(r["dx"], gx) <= 1e-13
    y = er.mean_tokens_yard(x, dy, torch.float32, torch.float32)
    # (a sequential sum of Nt terms: (Nt + 1) u of sum|x| / Nt, here relative to max|mean|)
    bound = 198 * U * float(x.abs().mean(1).max() / r["y"].abs().max())
    assert _rel(y["y"].double(), r["y"]) <= bound and _rel(y["dx"].double(), r["dx"]) <= 2 * U


def test_pack_refs_and_simple_maps():
    g = gen(32)
    x = torch.randn(2, 3, 5, 7, generator=g)
    y = er.pack_image_ref(x, 11, 17, 3, torch.float32)
    assert y.shape == (2, 11, 17, 4) and torch.equal(y[:, 3:8, 3:10, :3], x.permute(0, 2, 3, 1))
    assert int((y != 0).sum()) == x.numel() and bool((y[..., 3] == 0).all())
    w = torch.randn(5, 7, 7, 3, generator=g)
    pw = er.pack_stem_weight_ref(w, torch.float32)
    assert pw.shape == (5, 7, 8, 4) and torch.equal(er.unpack_stem_wgrad_ref(pw, 7, 3), w)
    assert int((pw != 0).sum()) == w.numel()
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])            # exact ties go to the even mantissa
    assert torch.equal(er.cast_ref(t).float(), torch.tensor([1.0, 1.0 + 2.0 ** -6]))
    z = torch.tensor([-1.0, -0.0, 0.0, 2.0])
    r = er.relu_ref(z)
    assert torch.equal(r, torch.tensor([0.0, 0.0, 0.0, 2.0])) and not bool(torch.signbit(r).any())
    assert torch.equal(er.relu_bwd_ref(torch.ones(4), z), torch.tensor([0.0, 0.0, 0.0, 1.0]))
    a, b = torch.randn(100, generator=g), torch.randn(100, generator=g)
    ref = er.axpby_ref64(a, b, 0.3, -1.7)
    assert _rel(ref, np.float32(0.3).astype(np.float64) * a.double() + np.float32(-1.7).astype(np.float64) * b.double()) <= 1e-15
    assert _rel(er.axpby_yard(a, b, 0.3, -1.7, torch.float32).double(), ref) <= 3 * U
    assert _rel(er.axpby_yard(a, None, 0.3, 0.0, torch.float32).double(), er.axpby_ref64(a, None, 0.3, 0.0)) <= U
