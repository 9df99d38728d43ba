"""Float64 references, float32 yardsticks and guarded ctypes callers for the norm / softmax / column-sum kernels.

For every operation there is
  *_ref64  the formula in float64 on exactly the values the kernel reads (bf16 inputs are rounded first, then widened;
           float32 side inputs such as mean / rstd / scale are widened as they are),
  *_yard   the same formula in float32 on the CPU: every reduction strictly sequential (np.add.accumulate, float32
           accumulator), elementwise outputs rounded to the kernel's output type at the end -- the worst ordinary float32
           evaluation, and the only source of tolerances (gate()),
  a thin ctypes caller that allocates every output inside a sentinel-filled guard band and reports whether the band is
  untouched.

Importing this module needs no GPU; the callers load the library on first use.
"""
import ctypes as C

import numpy as np
import torch

F32_NOISE = 1e-6
DEV = "cuda"
SENT = -12345.0          # guard-band fill (any write shows: the band is compared bitwise)
BIG = 1.0e30             # fill of pitch-padding columns of inputs: a leak into a sum is unmistakable
MASK_FILL = float(np.float32(-3.0e38))   # the kernel's finite "minus infinity"


# --------------------------------------------------------------------------------------------------------------------
# error measures and the gate
# --------------------------------------------------------------------------------------------------------------------
def maxrel(t, ref):
    ref = ref.double()
    return ((t.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def rel(t, ref):
    ref = ref.double()
    return ((t.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def gate(what, gpu, yard, ref, reduced=False, floor=F32_NOISE):
    """err(gpu) <= max(2 * err(yard), floor); prints the numbers first.  reduced: relative L2, else max-relative.
    floor: F32_NOISE, or for an output whose float32 evaluation cancels, the a-priori rounding bound of that evaluation
    (softmax_bwd_floor, bn_fwd_floors, bn_bwd_floor: each derived in its docstring from the data alone)."""
    f = rel if reduced else maxrel
    eg, ey = f(gpu, ref), f(yard, ref)
    floor = max(floor, F32_NOISE)
    print(f"{what}: gpu {eg:.3e} yard {ey:.3e}" + (f" floor {floor:.3e}" if floor > F32_NOISE else ""))
    assert eg == eg and eg <= max(2.0 * ey, floor), f"{what}: gpu {eg:.3e} vs yardstick {ey:.3e}, floor {floor:.3e}"
    return eg, ey


EPS32 = 2.0 ** -24       # unit roundoff of float32


def bits_equal(a, b):
    """bitwise equality of two tensors of one dtype"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


def seq_sum32(a, axis=0):
    """strictly sequential float32 sum along `axis`"""
    a = np.moveaxis(np.asarray(a, dtype=np.float32), axis, 0)
    return np.add.accumulate(a, axis=0, dtype=np.float32)[-1]


def _np32(t):
    return t.detach().float().cpu().numpy().astype(np.float32)


def _out(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def _f32(v):
    return float(np.float32(v))


# --------------------------------------------------------------------------------------------------------------------
# data
# --------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def int_data(g, rows, cols, dtype=torch.float32):
    """integer-valued data in [-8, 8]: every partial sum of up to 2^20 rows stays below 2^24, so any summation order is exact"""
    return torch.randint(-8, 9, (rows, cols), generator=g).to(dtype)


def ln_data(g, M, H, dtype, kind="plain"):
    """-> x, dy (kernel dtype), gamma, beta (f32)"""
    if kind == "tight":          # tiny spread around a large mean
        if dtype == torch.float32:
            x = 100.0 + 0.01 * torch.randn(M, H, generator=g)
        else:
            x = 16.0 + 0.125 * torch.randint(-4, 5, (M, H), generator=g).float()      # exact in bf16
    else:
        x = 2.0 * torch.randn(M, H, generator=g) + 0.5
        if kind == "const":
            x[M // 2] = 1.5      # a constant row whose sums are exact in float32: variance exactly 0
    dy = torch.randn(M, H, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(H, generator=g)
    beta = torch.randn(H, generator=g)
    return x.to(dtype), dy.to(dtype), gamma, beta


# BatchNorm cases shared by the CPU and the GPU tests: (C, M, kind, seed); kind in plain / trend / const
def bn_cases(dtype):
    bf = dtype == torch.bfloat16
    small = (8, 24, 64) if bf else (4, 12, 64)
    wide = (520, 2056) if bf else (260, 1028)
    cases = []
    for i, Cc in enumerate(small):
        for j, M in enumerate((2, 63, 64, 65, 257)):
            cases.append((Cc, M, "plain", 100 + 10 * i + j))
    cases += [(64, 1000, "plain", 140), (64, 5003, "plain", 141), (64, 1000, "trend", 142), (64, 5003, "trend", 143),
              (small[1], 257, "const", 144)]
    cases += [(wide[0], 65, "plain", 150), (wide[1], 65, "plain", 151), (wide[1], 65, "trend", 152)]
    return [(Cc, M, kind, _BN_SEEDS.get((bf, Cc, M, kind), seed)) for Cc, M, kind, seed in cases]


# Seeds replaced because the default one puts 0.05% or more of the case's elements inside the ReLU band (bn_relu_band) -- in the
# small cases a single element is more than the 0.1% allowed.  Chosen from the float64 reference and the yardstick alone
# (tests/test_kernel_ref_cpu.py asserts the share for every case); key: (bf16, C, M, kind).
_BN_SEEDS = {(False, 4, 64, "plain"): 1102, (False, 4, 65, "plain"): 1103, (False, 4, 257, "plain"): 2104,
             (False, 12, 63, "plain"): 1111, (False, 64, 64, "plain"): 1122, (False, 64, 5003, "plain"): 8141, (True, 24, 2, "plain"): 1110,
             (True, 24, 63, "plain"): 1111, (True, 24, 64, "plain"): 1112, (True, 64, 257, "plain"): 4124,
             (True, 64, 1000, "plain"): 1140, (True, 64, 5003, "plain"): 3141, (True, 2056, 65, "plain"): 2151}


def bn_data(Cc, M, kind, seed, dtype):
    """-> x, res, dy (kernel dtype), gamma, beta, running_mean, running_var (f32)"""
    g = gen(seed)
    off = 50.0 * (2.0 * torch.rand(Cc, generator=g) - 1.0)
    sc = 10.0 ** (3.0 * torch.rand(Cc, generator=g) - 2.0)          # 0.01 .. 10
    x = torch.randn(M, Cc, generator=g) * sc + off
    if kind == "trend":
        x = x + 0.01 * torch.arange(M, dtype=torch.float32)[:, None]
    if kind == "const":
        x[:, Cc // 2] = 3.0
    res = torch.randn(M, Cc, generator=g)
    dy = torch.randn(M, Cc, generator=g)
    gamma = 0.5 + torch.rand(Cc, generator=g)
    beta = 0.3 * torch.randn(Cc, generator=g)
    rm = torch.randn(Cc, generator=g)
    rv = 0.5 + torch.rand(Cc, generator=g)
    return x.to(dtype), res.to(dtype), dy.to(dtype), gamma, beta, rm, rv


def softmax_mask(B, Lk, g):
    """ragged key mask [B][Lk] (int64, 0 = masked): batch 0 ragged, batch 1 a single valid key, batch 2 all masked"""
    m = torch.zeros(B, Lk, dtype=torch.int64)
    for b in range(B):
        if b % 3 == 0:
            m[b, :max(1, (2 * Lk + 2) // 3)] = 1
            if Lk > 4:
                m[b, torch.randperm(Lk, generator=g)[:Lk // 5]] = 0
                m[b, 0] = 1
        elif b % 3 == 1:
            m[b, Lk // 2] = 1
    return m


# --------------------------------------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------------------------------------
def ln_fwd_ref64(x, gamma, beta, eps):
    x, g, b = x.double(), gamma.double(), beta.double()
    H = x.shape[1]
    mean = x.sum(1) / H
    d = x - mean[:, None]
    var = (d * d).sum(1) / H
    rstd = 1.0 / torch.sqrt(var + _f32(eps))
    return {"y": d * rstd[:, None] * g + b, "mean": mean, "rstd": rstd}


def ln_fwd_yard(x, gamma, beta, eps, out_dtype):
    x, g, b = _np32(x), _np32(gamma), _np32(beta)
    H = np.float32(x.shape[1])
    mean = seq_sum32(x, 1) / H
    d = x - mean[:, None]
    var = seq_sum32(d * d, 1) / H
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    y = d * rstd[:, None] * g + b
    return {"y": _out(y, out_dtype), "mean": _out(mean, torch.float32), "rstd": _out(rstd, torch.float32)}


def ln_bwd_ref64(dy, x, gamma, mean, rstd, keep=None):
    """keep: dropout factors keep / (1 - p) per element [M][H], or None"""
    dy, x, g, mean, rstd = dy.double(), x.double(), gamma.double(), mean.double(), rstd.double()
    H = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * g
    s1 = gg.sum(1) / H
    s2 = (gg * xh).sum(1) / H
    dx = rstd[:, None] * (gg - s1[:, None] - xh * s2[:, None])
    dxd = dx if keep is None else dx * keep.double()
    return {"dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0), "dx_dropped": dxd, "dbias": dxd.sum(0)}


def ln_bwd_yard(dy, x, gamma, mean, rstd, out_dtype, keep=None):
    dy, x, g, mean, rstd = _np32(dy), _np32(x), _np32(gamma), _np32(mean), _np32(rstd)
    H = np.float32(x.shape[1])
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * g
    s1 = seq_sum32(gg, 1) / H
    s2 = seq_sum32(gg * xh, 1) / H
    dx = rstd[:, None] * (gg - s1[:, None] - xh * s2[:, None])
    dxd = dx if keep is None else dx * _np32(keep)
    return {"dx": _out(dx, out_dtype), "dgamma": _out(seq_sum32(dy * xh, 0), torch.float32),
            "dbeta": _out(seq_sum32(dy, 0), torch.float32), "dx_dropped": _out(dxd, out_dtype),
            "dbias": _out(seq_sum32(dxd, 0), torch.float32)}


# --------------------------------------------------------------------------------------------------------------------
# softmax
# --------------------------------------------------------------------------------------------------------------------
def _masked_scores(S, mask, rows_per_batch, fill):
    if mask is None:
        return S
    rows = S.shape[0]
    b = torch.arange(rows) // rows_per_batch
    return torch.where(mask[b] == 0, torch.full_like(S, fill), S)


def softmax_fwd_ref64(S, mask, rows_per_batch, keep=None):
    """S [rows][Lk] f32; mask [B][Lk] or None; keep [rows][Lk] dropout factors or None"""
    s = _masked_scores(S.double(), mask, rows_per_batch, MASK_FILL)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    P = e / e.sum(1, keepdim=True)
    return {"P": P, "P_drop": P if keep is None else P * keep.double()}


def softmax_fwd_yard(S, mask, rows_per_batch, out_dtype, keep=None):
    s = _np32(_masked_scores(S.float(), mask, rows_per_batch, MASK_FILL))
    e = np.exp(s - s.max(1, keepdims=True), dtype=np.float32)
    P = e * (np.float32(1.0) / seq_sum32(e, 1))[:, None]
    Pd = P if keep is None else P * _np32(keep)
    return {"P": _out(P, out_dtype), "P_drop": _out(Pd, out_dtype)}


def softmax_bwd_ref64(dP, P, keep=None):
    g = dP.double() if keep is None else dP.double() * keep.double()
    p = P.double()
    return {"dS": p * (g - (p * g).sum(1, keepdim=True))}


def softmax_bwd_yard(dP, P, out_dtype, keep=None):
    g = _np32(dP) if keep is None else _np32(dP) * _np32(keep)
    p = _np32(P)
    return {"dS": _out(p * (g - seq_sum32(p * g, 1)[:, None]), out_dtype)}


def softmax_bwd_floor(dP, P, keep=None):
    """Relative floor for dS = p * (g - dot), dot = sum_k p * g.  Where one key holds most of the probability, dot is
    close to that key's g and g - dot cancels, so max|dS| is small while the rounding of dot is not: dot is a float32 sum
    of Lk products, and a lane's chain of ceil(Lk / 64) additions followed by the six butterfly steps of a wave carries at
    most D = ceil(Lk / 64) + 6 roundings, plus one each for the product, the subtraction and the final multiply:
        |err dS[r][k]| <= 2^-24 * (D + 3) * p[r][k] * (|g[r][k]| + sum_j |p[r][j] * g[r][j]|).
    The floor is the largest such bound over the elements, relative to max|dS| -- a property of the data, not of any result."""
    g = dP.double() if keep is None else dP.double() * keep.double()
    p = P.double()
    Lk = p.shape[1]
    D = -(-Lk // 64) + 6 + 3
    bound = EPS32 * D * p * (g.abs() + (p * g).abs().sum(1, keepdim=True))
    top = (p * (g - (p * g).sum(1, keepdim=True))).abs().max()
    return (bound.max() / top).item() if top > 0 else 0.0          # (one key: dS is exactly 0, nothing to bound)


# --------------------------------------------------------------------------------------------------------------------
# column sum
# --------------------------------------------------------------------------------------------------------------------
def colsum_ref64(x, prior=None):
    s = x.double().sum(0)
    return {"out": s if prior is None else prior.double() + s}


def colsum_yard(x, prior=None):
    s = seq_sum32(_np32(x), 0)
    return {"out": _out(s if prior is None else _np32(prior) + s, torch.float32)}


# --------------------------------------------------------------------------------------------------------------------
# BatchNorm
# --------------------------------------------------------------------------------------------------------------------
def bn_fwd_ref64(x, gamma, beta, rm, rv, eps, momentum, training, relu, res=None, calls=1):
    """-> save_mean, save_invstd, scale, shift, pre (before the ReLU), y, running_mean, running_var (after `calls` calls)"""
    x, g, b = x.double(), gamma.double(), beta.double()
    M = x.shape[0]
    o = {}
    if training:
        mean = x.sum(0) / M
        d = x - mean
        var = (d * d).sum(0) / M
        if rm is not None:
            unb = var * M / (M - 1) if M > 1 else var
            r1, r2, mo = rm.double(), rv.double(), _f32(momentum)
            for _ in range(calls):
                r1 = (1.0 - mo) * r1 + mo * mean
                r2 = (1.0 - mo) * r2 + mo * unb
            o["running_mean"], o["running_var"] = r1, r2
    else:
        mean, var = rm.double(), rv.double()
    invstd = 1.0 / torch.sqrt(var + _f32(eps))
    scale = g * invstd
    shift = b - mean * scale
    pre = x * scale + shift
    if res is not None:
        pre = pre + res.double()
    o.update(save_mean=mean, save_invstd=invstd, scale=scale, shift=shift, pre=pre, y=pre.clamp_min(0.0) if relu else pre)
    return o


def bn_fwd_yard(x, gamma, beta, rm, rv, eps, momentum, training, relu, out_dtype, res=None, calls=1):
    x, g, b = _np32(x), _np32(gamma), _np32(beta)
    M = np.float32(x.shape[0])
    one = np.float32(1.0)
    o = {}
    if training:
        mean = seq_sum32(x, 0) / M
        d = x - mean
        var = seq_sum32(d * d, 0) / M
        if rm is not None:
            unb = seq_sum32(d * d, 0) / np.float32(x.shape[0] - 1) if x.shape[0] > 1 else var
            r1, r2, mo = _np32(rm), _np32(rv), np.float32(momentum)
            for _ in range(calls):
                r1 = (one - mo) * r1 + mo * mean
                r2 = (one - mo) * r2 + mo * unb
            o["running_mean"], o["running_var"] = _out(r1, torch.float32), _out(r2, torch.float32)
    else:
        mean, var = _np32(rm), _np32(rv)
    invstd = one / np.sqrt(var + np.float32(eps), dtype=np.float32)
    scale = g * invstd
    shift = b - mean * scale
    pre = x * scale + shift
    if res is not None:
        pre = pre + _np32(res)
    y = np.maximum(pre, np.float32(0.0)) if relu else pre
    f = torch.float32
    o.update(save_mean=_out(mean, f), save_invstd=_out(invstd, f), scale=_out(scale, f), shift=_out(shift, f),
             pre=_out(pre, f), y=_out(y, out_dtype))
    return o


def bn_bwd_ref64(dy, x, gamma, mean, invstd, training, mask=None):
    """mask: bool [M][C] of the forward's ReLU (None: no ReLU) -> dx, dgamma, dbeta, dres"""
    dy, x, g, mean, invstd = dy.double(), x.double(), gamma.double(), mean.double(), invstd.double()
    M = x.shape[0]
    dz = dy if mask is None else dy * mask.double()
    xh = (x - mean) * invstd
    dbeta = dz.sum(0)
    dgamma = (dz * xh).sum(0)
    if training:
        dx = g * invstd * (dz - dbeta / M - xh * dgamma / M)
    else:
        dx = g * invstd * dz
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "dres": dz}


def bn_bwd_yard(dy, x, gamma, mean, invstd, training, out_dtype, mask=None):
    dy, x, g, mean, invstd = _np32(dy), _np32(x), _np32(gamma), _np32(mean), _np32(invstd)
    M = np.float32(x.shape[0])
    dz = dy if mask is None else dy * mask.numpy().astype(np.float32)
    xh = (x - mean) * invstd
    dbeta = seq_sum32(dz, 0)
    dgamma = seq_sum32(dz * xh, 0)
    if training:
        dx = g * invstd * (dz - dbeta / M - xh * dgamma / M)
    else:
        dx = g * invstd * dz
    return {"dx": _out(dx, out_dtype), "dgamma": _out(dgamma, torch.float32), "dbeta": _out(dbeta, torch.float32),
            "dres": _out(dz, out_dtype)}


def _depth(M):
    """roundings along a tree-like float32 reduction over M rows: a thread's short chain, the wave and block folds, the merge
    over row blocks"""
    return 8 + int(np.ceil(np.log2(max(M, 2))))


def bn_fwd_floors(x, gamma, beta, ref, training, eps, res=None):
    """A-priori float32 rounding bounds of the BatchNorm forward, from the data alone (u = 2^-24, D = _depth(M)).

    The kernel keeps save_mean, scale = gamma * invstd and shift = beta - mean * scale in float32 and applies
    y = fma(x, scale, shift): with |mean| >> std the two operands are large and cancel, and their roundings do not.
      variance (training): single pass over d = x - x0 (x0 a row of the channel), var = (sum d^2 - (sum d)^2 / n) / n merged
        over row blocks.  With (x - x0)^2 <= 2 (x - mean)^2 + 2 (x0 - mean)^2 the two sums are at most
        4 (1 + z^2) n var, z = max |x - mean| / std of the channel, so rel(var) <= u D 4 (1 + z^2).  The row blocks hand
        over (count, mean, M2) in float32, so every block mean carries u |mean|, which the merge term n_b (mean_b - mean)^2
        turns into 2 n_b |mean_b - mean| u |mean|; over the blocks at most 2 u |mean| n std, i.e. another 2 u |mean| / std
        on rel(var) -- first order in u |mean| / std, where the two-pass yardstick is second order (measured on the MI355X:
        1.5e-5 on save_invstd at |mean| / std = 5000, C = 260, M = 65, against 3e-7 of the yardstick).  Then
        rel(invstd) <= rel(var) / 2 * var / (var + eps) + 2 u (rsqrt, and the final rounding).  Eval: 2 u.
      mean (training): |err| <= u (|mean| + D std (1 + z)).
      scale: rel(invstd) + u.   shift: |mean scale| (rel(invstd) + 3 u) + |scale| err(mean) + u |beta|.
      y: max|x - mean| |scale| rel(invstd) + |scale| err(mean) + u (2 max|x scale| + 3 |mean scale| + 2 |beta| + 2 max|res|).
    -> relative floors for save_invstd / scale / shift / y (each: largest bound over the channels / max|reference|), and
    "pre_abs": the bound of y per channel (the ReLU band)."""
    x, g, b = x.double(), gamma.double(), beta.double()
    M = x.shape[0]
    D = _depth(M)
    u = EPS32
    mean, invstd, scale = ref["save_mean"], ref["save_invstd"], ref["scale"]
    var = (1.0 / invstd ** 2 - _f32(eps)).clamp_min(0.0)
    dev = (x - mean).abs().max(0).values
    if training:
        std = var.sqrt()
        z = torch.where(std > 0, dev / std.clamp_min(1e-300), torch.zeros_like(std))
        kappa = torch.where(std > 0, mean.abs() / std.clamp_min(1e-300), torch.zeros_like(std))
        rel_is = 0.5 * u * (D * 4.0 * (1.0 + z * z) + 2.0 * kappa) * var / (var + _f32(eps)) + 2.0 * u
        err_mean = u * (mean.abs() + D * std * (1.0 + z))
    else:
        rel_is = torch.full_like(mean, 2.0 * u)
        err_mean = torch.zeros_like(mean)
    ms = (mean * scale).abs()
    rmax = res.double().abs().max(0).values if res is not None else torch.zeros_like(mean)
    y_abs = dev * scale.abs() * rel_is + scale.abs() * err_mean + u * (
        2.0 * (x * scale).abs().max(0).values + 3.0 * ms + 2.0 * b.abs() + 2.0 * rmax)
    shift_abs = ms * (rel_is + 3.0 * u) + scale.abs() * err_mean + u * b.abs()

    def relmax(bound, r):
        return (bound.max() / r.abs().max().clamp_min(1e-300)).item()

    return {"save_invstd": relmax(invstd * rel_is, invstd), "scale": relmax(scale.abs() * (rel_is + u), scale),
            "shift": relmax(shift_abs, ref["shift"]), "y": relmax(y_abs, ref["y"]), "pre_abs": y_abs}


def bn_bwd_floor(dy, x, gamma, mean, invstd, training, ref, mask=None):
    """A-priori float32 rounding bound of dx = ca dz + cb (x - mean) + cc (ca = gamma invstd, cb = -ca invstd dgamma / M,
    cc = -ca dbeta / M; eval: ca dz alone), relative to max|dx|.  The three terms cancel (for M = 2 they cancel entirely but
    for eps), their roundings do not: six roundings on the magnitudes of the terms, and dbeta, dgamma are float32 sums over
    M rows with D = _depth(M) roundings on sum|dz|, sum|dz xhat|:
        |err dx| <= u (6 (|ca dz| + |cb (x - mean)| + |cc|) + D ca (mean|dz| + |xhat| mean|dz xhat|)).
    -> relative floors for dx, and for dbeta / dgamma (sum_floor: in eval mode xhat is far from centred, so dgamma cancels)."""
    dy, x, g, mean, invstd = dy.double(), x.double(), gamma.double(), mean.double(), invstd.double()
    M = x.shape[0]
    dz = dy if mask is None else dy * mask.double()
    ca = (g * invstd).abs()
    if not training:
        bound = EPS32 * 3.0 * ca * dz.abs()
    else:
        xh = (x - mean) * invstd
        cb = ca * invstd * ref["dgamma"].abs() / M
        cc = ca * ref["dbeta"].abs() / M
        bound = EPS32 * (6.0 * (ca * dz.abs() + cb * (x - mean).abs() + cc)
                         + _depth(M) * ca * (dz.abs().mean(0) + xh.abs() * (dz * xh).abs().mean(0)))
    xh = (x - mean) * invstd
    return {"dx": (bound.max() / ref["dx"].abs().max().clamp_min(1e-300)).item(), "dbeta": sum_floor(dz),
            "dgamma": sum_floor(dz * xh)}


def sum_floor(terms):
    """Relative-L2 floor of float32 column sums that cancel: a tree-like reduction over M rows puts at most D = _depth(M)
    roundings on sum_m |term|, so ||err|| <= 2^-24 D ||sum_m |term| ||, relative to ||sum_m term||."""
    t = terms.double()
    return (EPS32 * _depth(t.shape[0]) * t.abs().sum(0).norm() / t.sum(0).norm().clamp_min(1e-300)).item()


def bn_relu_band(ref, yard, pre_abs):
    """Elements whose float64 pre-activation lies within float32's reach of 0, per channel: twice the yardstick's own largest
    error on the pre-activation in that channel (the factor of the gate), or the a-priori bound bn_fwd_floors()["pre_abs"].
    -> bool [M][C], True = the sign is undecidable in float32."""
    band = torch.maximum(2.0 * (yard["pre"].double() - ref["pre"]).abs().max(0).values, pre_abs)
    return ref["pre"].abs() <= band


# --------------------------------------------------------------------------------------------------------------------
# guarded device buffers and the ctypes callers
# --------------------------------------------------------------------------------------------------------------------
class GBuf:
    """[rows][ld] device array of which columns < cols belong to the contract, inside a band of at least two sentinel rows on
    either side (a multiple of 64 elements, so the array keeps the alignment of the allocation)."""

    def __init__(self, rows, ld, dtype, cols=None, fill=SENT, is_vec=False):
        self.is_vec = is_vec
        self.rows, self.ld, self.cols, self.fill = rows, ld, ld if cols is None else cols, fill
        self.n = rows * ld
        self.g = -(-2 * ld // 64) * 64
        self.flat = torch.full((self.n + 2 * self.g,), fill, dtype=dtype, device=DEV)
        self.t = self.flat[self.g:self.g + self.n].view(rows, ld)
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t[:, :self.cols].cpu().clone()

    def vec(self):
        return self.get().reshape(-1)

    def _ok(self, part):
        return bits_equal(part, torch.full_like(part, self.fill))

    def intact(self):
        f = self.flat.cpu()
        ok = self._ok(f[:self.g]) and self._ok(f[self.g + self.n:])
        if self.cols < self.ld:
            ok = ok and self._ok(f[self.g:self.g + self.n].view(self.rows, self.ld)[:, self.cols:])
        return ok

    def untouched(self):
        return self._ok(self.flat.cpu())


def _fresh(t, dtype=None):
    """a fresh, contiguous device allocation (per-channel vectors are read as 16-byte vectors: never a sliced view)"""
    if t is None:
        return None
    t = t.to(dtype) if dtype is not None else t
    return t.contiguous().clone().to(DEV)


def _env():
    from hamspine import _lib as L
    from hamspine import rt
    return L, L.lib(), rt


def _p(t):
    if t is None:
        return None
    return t.ptr if isinstance(t, GBuf) else t.data_ptr()


def _finish(L, status, what, bufs, check):
    torch.cuda.synchronize()
    r = {"status": status, "guards": all(b.intact() for b in bufs.values() if b is not None),
         "untouched": all(b.untouched() for b in bufs.values() if b is not None)}
    for k, b in bufs.items():
        if b is not None:
            r[k] = b.vec() if b.is_vec else b.get()
    if check:
        L.check(status, what)
    return r


def _wsbuf(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def call_dropout_keep(n, p, seed):
    """hs_dropout on n ones: keep / (1 - p) per element index (f32, CPU)"""
    L, lib, rt = _env()
    ones = torch.ones(n, device=DEV)
    out = torch.empty(n, device=DEV)
    L.check(lib.hs_dropout(L.HS_F32, ones.data_ptr(), out.data_ptr(), n, p, seed, rt.stream()), "hs_dropout")
    torch.cuda.synchronize()
    return out.cpu()


def call_ln_fwd(x, gamma, beta, eps, want_stats=True, check=True):
    L, lib, rt = _env()
    M, H = x.shape
    xd, gd, bd = _fresh(x), _fresh(gamma), _fresh(beta)
    bufs = {"y": GBuf(M, H, x.dtype), "mean": GBuf(1, M, torch.float32, is_vec=True) if want_stats else None,
            "rstd": GBuf(1, M, torch.float32, is_vec=True) if want_stats else None}
    st = lib.hs_layernorm_fwd(rt.hs_dtype(x.dtype), _p(xd), _p(gd), _p(bd), _p(bufs["y"]), _p(bufs["mean"]), _p(bufs["rstd"]),
                              M, H, eps, rt.stream())
    return _finish(L, st, "hs_layernorm_fwd", bufs, check)


def call_ln_bwd(dy, x, gamma, mean, rstd, want_dx=True, pre=False, p=0.0, seed=0, want_dxd=True, ws_short=0, check=True):
    """hs_layernorm_bwd, or with pre=True hs_layernorm_bwd_pre.  ws_short: bytes by which the stated workspace size falls
    short of what the call needs (the allocation itself stays whole)."""
    L, lib, rt = _env()
    M, H = x.shape
    dyd, xd, gd, md, rd = _fresh(dy), _fresh(x), _fresh(gamma), _fresh(mean), _fresh(rstd)
    f = torch.float32
    bufs = {"dx": GBuf(M, H, x.dtype) if want_dx else None, "dgamma": GBuf(1, H, f, is_vec=True), "dbeta": GBuf(1, H, f, is_vec=True)}
    full = int(lib.hs_layernorm_bwd_ws_bytes(M, H))
    ws = _wsbuf(full)
    if pre:
        bufs["dx_dropped"] = GBuf(M, H, x.dtype) if want_dxd else None
        bufs["dbias"] = GBuf(1, H, f, is_vec=True)
        st = lib.hs_layernorm_bwd_pre(rt.hs_dtype(x.dtype), _p(dyd), _p(xd), _p(gd), _p(md), _p(rd), _p(bufs["dx"]),
                                      _p(bufs["dgamma"]), _p(bufs["dbeta"]), _p(bufs["dx_dropped"]), _p(bufs["dbias"]), p, seed,
                                      _p(ws), full - ws_short, M, H, rt.stream())
    else:
        need = full // 3 * 2          # two of the three partial vectors per block
        st = lib.hs_layernorm_bwd(rt.hs_dtype(x.dtype), _p(dyd), _p(xd), _p(gd), _p(md), _p(rd), _p(bufs["dx"]),
                                  _p(bufs["dgamma"]), _p(bufs["dbeta"]), _p(ws), (need if ws_short else full) - ws_short, M, H,
                                  rt.stream())
    return _finish(L, st, "hs_layernorm_bwd_pre" if pre else "hs_layernorm_bwd", bufs, check)


def _pitched(t, ld, offset=0, fill=BIG):
    """device copy of [rows][n] with pitch ld (padding = fill), starting `offset` elements into its allocation"""
    rows, n = t.shape
    flat = torch.full((rows * ld + offset,), fill, dtype=t.dtype)
    flat[offset:].view(rows, ld)[:, :n] = t
    flat = flat.to(DEV)
    return flat, flat[offset:]


def call_softmax_fwd(S, mask, dtype, Lk, ldS, ldP, rows_per_batch, p=0.0, seed=0, want_drop=False, misalign=False,
                     rows=None, check=True):
    """S [rows][Lk] f32 (CPU); misalign: S starts one float into its allocation (forces the scalar body)"""
    L, lib, rt = _env()
    n = S.shape[0]
    keepalive, Sd = _pitched(S.float(), ldS, 1 if misalign else 0)
    md = _fresh(mask)
    bufs = {"P": GBuf(n, ldP, dtype), "P_drop": GBuf(n, ldP, dtype) if want_drop else None}
    st = lib.hs_softmax_fwd(rt.hs_dtype(dtype), _p(Sd), _p(md), _p(bufs["P"]), _p(bufs["P_drop"]), n if rows is None else rows,
                            Lk, ldS, ldP, rows_per_batch, p, seed, rt.stream())
    return _finish(L, st, "hs_softmax_fwd", bufs, check)


def call_softmax_bwd(dP, P, Lk, ldG, ldP, p=0.0, seed=0, misalign=False, check=True):
    """dP [rows][Lk] f32, P [rows][Lk] in the kernel dtype (its padding columns are given as zeros)"""
    L, lib, rt = _env()
    n = P.shape[0]
    keepalive, Gd = _pitched(dP.float(), ldG, 1 if misalign else 0)
    _, Pd = _pitched(P, ldP, 0, fill=0.0)
    bufs = {"dS": GBuf(n, ldP, P.dtype)}
    st = lib.hs_softmax_bwd(rt.hs_dtype(P.dtype), _p(Gd), _p(Pd), _p(bufs["dS"]), n, Lk, ldG, ldP, p, seed, rt.stream())
    return _finish(L, st, "hs_softmax_bwd", bufs, check)


def call_colsum(x, ld, accumulate=0, prior=None, misalign=False, M=None, ws_short=0, check=True):
    """x [M][N] (CPU, kernel dtype); columns N..ld-1 of the device copy hold BIG"""
    L, lib, rt = _env()
    rows, N = x.shape
    keepalive, xd = _pitched(x, ld, 1 if misalign else 0)
    out = GBuf(1, N, torch.float32, is_vec=True)
    if prior is not None:
        out.t[0].copy_(prior.to(DEV))
    full = int(lib.hs_colsum_ws_bytes(rows, N))
    ws = _wsbuf(full)
    st = lib.hs_colsum(rt.hs_dtype(x.dtype), _p(xd), rows if M is None else M, N, ld, _p(out), _p(ws), full - ws_short,
                       accumulate, rt.stream())
    r = _finish(L, st, "hs_colsum", {"out": out}, check)
    if prior is not None:     # "untouched" then means: still the prior values inside an intact band
        r["untouched"] = r["guards"] and bits_equal(r["out"], prior.float())
    return r


class BnState:
    """device-side per-channel state of one BatchNorm layer across calls (fresh allocations)"""

    def __init__(self, gamma, beta, rm=None, rv=None):
        self.gamma, self.beta, self.rm, self.rv = _fresh(gamma), _fresh(beta), _fresh(rm), _fresh(rv)


def call_bn_fwd(x, state, eps=1e-5, momentum=0.1, training=1, relu=0, res=None, want_y=True, ws_bytes=None, check=True):
    L, lib, rt = _env()
    M, Cc = x.shape
    xd, rd = _fresh(x), _fresh(res)
    f = torch.float32
    bufs = {"y": GBuf(M, Cc, x.dtype) if want_y else None}
    for k in ("save_mean", "save_invstd", "scale", "shift"):
        bufs[k] = GBuf(1, Cc, f, is_vec=True)
    full = int(lib.hs_batchnorm_ws_bytes(M, Cc, rt.hs_dtype(x.dtype)))
    ws = _wsbuf(full)
    q = L.BnParams()
    q.dtype, q.C, q.M, q.training, q.relu = rt.hs_dtype(x.dtype), Cc, M, training, relu
    q.eps, q.momentum = eps, momentum
    q.x, q.residual, q.y, q.gamma, q.beta = _p(xd), _p(rd), _p(bufs["y"]), _p(state.gamma), _p(state.beta)
    q.running_mean, q.running_var = _p(state.rm), _p(state.rv)
    q.save_mean, q.save_invstd, q.scale, q.shift = (_p(bufs[k]) for k in ("save_mean", "save_invstd", "scale", "shift"))
    q.ws, q.ws_bytes = _p(ws), full if ws_bytes is None else ws_bytes
    st = lib.hs_batchnorm_fwd(C.byref(q), rt.stream())
    r = _finish(L, st, "hs_batchnorm_fwd", bufs, check)
    if state.rm is not None:
        r["running_mean"], r["running_var"] = state.rm.cpu().clone(), state.rv.cpu().clone()
    return r


def call_bn_bwd(dy, x, gamma, mean, invstd, training=1, relu=0, y=None, scale=None, shift=None, want_dx=True,
                want_dres=False, ws_bytes=None, check=True):
    L, lib, rt = _env()
    M, Cc = x.shape
    dyd, xd, yd = _fresh(dy), _fresh(x), _fresh(y)
    gd, md, isd, scd, shd = _fresh(gamma), _fresh(mean), _fresh(invstd), _fresh(scale), _fresh(shift)
    f = torch.float32
    bufs = {"dx": GBuf(M, Cc, x.dtype) if want_dx else None, "dres": GBuf(M, Cc, x.dtype) if want_dres else None,
            "dgamma": GBuf(1, Cc, f, is_vec=True), "dbeta": GBuf(1, Cc, f, is_vec=True)}
    full = int(lib.hs_batchnorm_ws_bytes(M, Cc, rt.hs_dtype(x.dtype)))
    ws = _wsbuf(full)
    q = L.BnBwdParams()
    q.dtype, q.C, q.M, q.training, q.relu = rt.hs_dtype(x.dtype), Cc, M, training, relu
    q.dy, q.y, q.x, q.gamma, q.save_mean, q.save_invstd = _p(dyd), _p(yd), _p(xd), _p(gd), _p(md), _p(isd)
    q.dx, q.dres, q.dgamma, q.dbeta = _p(bufs["dx"]), _p(bufs["dres"]), _p(bufs["dgamma"]), _p(bufs["dbeta"])
    q.ws, q.ws_bytes = _p(ws), full if ws_bytes is None else ws_bytes
    q.scale, q.shift = _p(scd), _p(shd)
    st = lib.hs_batchnorm_bwd(C.byref(q), rt.stream())
    return _finish(L, st, "hs_batchnorm_bwd", bufs, check)
