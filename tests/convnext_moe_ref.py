"""Float64 references, float32 yardsticks, a-priori floors, case lists and guarded ctypes callers for the ConvNeXt kernels
(depthwise convolution, layer scale, patchify) and the MoE routing / KAN weight-pack kernels.

Same scheme as kernel_ref and head_ref (whose gate, guard bands, data helpers and __expf model are imported, not copied):
  *_ref64   the formula of the header comment in float64 (torch, double) on exactly the values the kernel reads (bf16 inputs
            are rounded first, float32 side inputs widened as they are).  The gating gradient is autograd through the float64
            forward; everything else is written out.
  *_yard    the same formula in float32 on the CPU, separate multiply and add, every reduction strictly sequential
            (seq_sum32), elementwise outputs rounded once to the kernel's output type.
  *_floor   where a float32 evaluation cancels, the a-priori rounding bound of that evaluation from the inputs and the
            float64 reference alone (derived in each docstring), for gate(floor=).
  *_cases   the smallest shapes that reach every loop, tile edge and launch geometry of the kernels.
  call_*    ctypes callers: every output, and the workspace, inside a GBuf guard band.

Layouts: activations NHWC, given here as [N][H][W][C] tensors; depthwise filters [C][ks*ks] float32.
Importing this module needs no GPU.
"""
import ctypes as C

import numpy as np
import torch

from head_ref import expf32
from kernel_ref import (DEV, EPS32, SENT, GBuf, _depth, _env, _f32, _finish, _fresh, _np32, _out, _p, _wsbuf,  # noqa: F401
                        bits_equal, gate, gen, int_data, maxrel, rel, seq_sum32, sum_floor)

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
I32 = torch.int32
DTYPES = (F32, BF16)
U = EPS32
MOE_TOPW = 17                # ints per row of `top`
HUGE = 1.0e30                # rows an expert never sees: a leak into a sum is unmistakable


def dname(dt):
    return "bf16" if dt == BF16 else "f32"


def chain_floor(terms, D):
    """Relative-L2 floor of float32 column sums over axis 0 whose longest chain of additions is D long: any order of summation
    with at most D roundings on a path puts at most 2^-24 D sum|term| on a sum, so ||err|| <= 2^-24 D || sum|term| ||,
    relative to || sum term ||.  (sum_floor is this with D = 8 + log2 M of a tree; the kernels served here fold long
    sequential chains, so their D is counted from the launch geometry by the caller.)"""
    t = terms.double()
    return (U * D * t.abs().sum(0).norm() / t.sum(0).norm().clamp_min(1e-300)).item()


def elem_floor(terms, D):
    """The same for an elementwise output judged by max|err| / max|ref|: 2^-24 D max(sum|term|) / max|sum term|."""
    t = terms.double()
    return (U * D * t.abs().sum(0).max() / t.sum(0).abs().max().clamp_min(1e-300)).item()


# ======================================================================================================================
# depthwise convolution
# ======================================================================================================================
def _padhw(x, pad):
    return torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))


def _dw_corr(x, w, bias, ks, flip):
    """y[n,h,w,c] = b[c] + sum_{r,s} x[n,h+r-pad,w+s-pad,c] * w[c][r*ks+s] (flip: the filter read back to front), in the
    dtype of x; taps accumulate in (r, s) order, multiply and add rounded separately"""
    N, H, W, Cc = x.shape
    xp = _padhw(x, ks // 2)
    acc = torch.zeros_like(x) if bias is None else bias.to(x.dtype).expand(N, H, W, Cc).clone()
    for r in range(ks):
        for s in range(ks):
            t = r * ks + s
            acc = acc + xp[:, r:r + H, s:s + W, :] * w[:, ks * ks - 1 - t if flip else t]
    return acc


def _dw_terms(x, dy, ks):
    """per-pixel products dy[n,h,w,c] * x[n,h+r-pad,w+s-pad,c] -> [N*H*W][ks*ks][C] in the dtype of x"""
    N, H, W, Cc = x.shape
    xp = _padhw(x, ks // 2)
    return torch.stack([(dy * xp[:, r:r + H, s:s + W, :]).reshape(-1, Cc) for r in range(ks) for s in range(ks)], 1)


def dwconv_ref64(x, w, bias, dy, ks):
    """-> y, dx [N][H][W][C], dw [C][ks*ks], db [C]"""
    x, w, dy = x.double(), w.double(), dy.double()
    b = None if bias is None else bias.double()
    t = _dw_terms(x, dy, ks)
    return {"y": _dw_corr(x, w, b, ks, False), "dx": _dw_corr(dy, w, None, ks, True), "dw": t.sum(0).t().contiguous(),
            "db": dy.reshape(-1, x.shape[3]).sum(0), "terms": t, "db_terms": dy.reshape(-1, x.shape[3])}


def dwconv_yard(x, w, bias, dy, ks):
    dt = x.dtype
    xf, wf, gf = x.float(), w.float(), dy.float()
    t = _dw_terms(xf, gf, ks)
    dw = torch.from_numpy(seq_sum32(t.numpy(), 0)).t().contiguous()
    db = torch.from_numpy(seq_sum32(gf.reshape(-1, x.shape[3]).numpy(), 0))
    return {"y": _dw_corr(xf, wf, bias, ks, False).to(dt), "dx": _dw_corr(gf, wf, None, ks, True).to(dt), "dw": dw, "db": db}


def dw_chunks(N, H, Cc):
    """chunk count of the filter-gradient kernel as the header of dwconv_wgrad_kernel states it: ceil(2048 / ceil(C / 64))
    chunks of image rows, at most N * H"""
    g = -(-Cc // 64)
    return max(1, min(-(-2048 // g), N * H))


def dwconv_wgrad_floor(ref, N, H, W, Cc):
    """dw and db are float32 sums of N*H*W signed products per entry.  A chunk's wave walks ceil(N*H / chunks) image rows of W
    columns in one chain, the final kernel adds ceil(chunks / 8) partials per accumulator and folds 2 * 4 accumulators in
    three steps: D = ceil(N*H / chunks) * W + ceil(chunks / 8) + 3 roundings at most on any path (the products themselves
    are fused).  -> relative-L2 floors {"dw", "db"} by chain_floor."""
    ch = dw_chunks(N, H, Cc)
    D = -(-(N * H) // ch) * W + -(-ch // 8) + 3
    t = ref["terms"]
    return {"dw": chain_floor(t.reshape(t.shape[0], -1), D), "db": chain_floor(ref["db_terms"], D)}


def dwconv_data(c, dtype):
    """-> x, dy (kernel dtype, [N][H][W][C]), w [C][ks*ks], bias [C] or None.  Filters are asymmetric (random), so a missing
    flip shows.  kind "int": integers in [-3, 3]; every sum of at most 49 products plus the bias stays below 2^24."""
    N, H, W, Cc, ks = c["N"], c["H"], c["W"], c["C"], c["ks"]
    g = gen(c["seed"])
    if c["kind"] == "int":
        x = torch.randint(-3, 4, (N, H, W, Cc), generator=g).float()
        dy = torch.randint(-3, 4, (N, H, W, Cc), generator=g).float()
        w = torch.randint(-3, 4, (Cc, ks * ks), generator=g).float()
        w[:, 0], w[:, -1] = 3.0, -2.0                                  # never symmetric
        bias = torch.randint(-3, 4, (Cc,), generator=g).float()
    else:
        x = torch.randn(N, H, W, Cc, generator=g)
        dy = torch.randn(N, H, W, Cc, generator=g)
        w = 0.3 * torch.randn(Cc, ks * ks, generator=g)
        bias = torch.randn(Cc, generator=g)
    return x.to(dtype), dy.to(dtype), w, (bias if c["bias"] else None)


def _dwc(N, H, W, Cc, ks, seed, bias=True, kind="plain"):
    return {"N": N, "H": H, "W": W, "C": Cc, "ks": ks, "seed": seed, "bias": bias, "kind": kind,
            "tag": f"dwconv N={N} H={H} W={W} C={Cc} ks={ks}" + ("" if bias else " nobias") + (" int" if kind == "int" else "")}


def dwconv_fwd_cases():
    """forward / data gradient: a thread owns 4 channels x 4 columns.  W in {1, 3, 4, 5, 9} (W < pad, ragged and exact column
    tiles), H in {1, 2, 7}, C in {4, 8, 132}; N=2 H=7 W=9 C=132 has 2*7*3*33 = 1386 threads: six blocks, the last one ragged."""
    cases = []
    for i, ks in enumerate((3, 5, 7)):
        s = 300 + 10 * i
        cases += [_dwc(1, 1, 1, 4, ks, s), _dwc(2, 2, 3, 8, ks, s + 1, bias=False), _dwc(1, 7, 4, 4, ks, s + 2),
                  _dwc(1, 2, 5, 8, ks, s + 3), _dwc(2, 7, 9, 132, ks, s + 4), _dwc(2, 7, 9, 8, ks, s + 5, kind="int")]
    return cases


def dwconv_wgrad_cases():
    """filter / bias gradient: W in {1, 15, 16, 17, 33} (one segment of 16 columns, an exact one, a second ragged one, a third),
    C in {4, 124, 128, 132, 260} (lane pairs and 128-channel groups), N*H in {1, 3, 4, 5, 8, 9, 12, 13} at C=8 W=3 (the chunk
    count equals N*H: the unrolled and the remainder loop of the final kernel), and C=1024 N=3 H=50 W=2: 128 chunks for 150
    rows, so the row loop strides."""
    cases = []
    for i, W in enumerate((1, 15, 16, 17, 33)):
        cases.append(_dwc(1, 2, W, 8, (3, 5, 7)[i % 3], 400 + i))
    for i, Cc in enumerate((4, 124, 128, 132, 260)):
        cases.append(_dwc(1, 2, 3, Cc, (7, 3, 5)[i % 3], 410 + i))
    for i, (N, H) in enumerate(((1, 1), (1, 3), (2, 2), (1, 5), (2, 4), (3, 3), (3, 4), (1, 13))):
        cases.append(_dwc(N, H, 3, 8, (3, 7, 5)[i % 3], 420 + i))
    cases.append(_dwc(3, 50, 2, 1024, 3, 430))
    cases.append(_dwc(2, 5, 17, 8, 5, 431, kind="int"))
    return cases


class _Ws(GBuf):
    """a workspace of exactly nbytes bytes inside a guard band"""

    def __init__(self, nbytes):
        super().__init__(1, max(int(nbytes) // 4, 1), F32, is_vec=True)


def _act(N, H, W, Cc, dtype):
    return GBuf(N * H * W, Cc, dtype)


def call_dwconv_fwd(x, w, bias, ks, C_arg=None, ws_short=0, check=True):
    L, lib, rt = _env()
    N, H, W, Cc = x.shape
    xd, wd, bd = _fresh(x), _fresh(w), _fresh(bias)
    full = ks * ks * Cc * 4
    bufs = {"y": _act(N, H, W, Cc, x.dtype), "ws": _Ws(full)}
    st = lib.hs_dwconv_fwd(rt.hs_dtype(x.dtype), _p(xd), _p(wd), _p(bd), _p(bufs["y"]), N, H, W, Cc if C_arg is None else C_arg,
                           ks, _p(bufs["ws"]), full - ws_short, rt.stream())
    r = _finish(L, st, "hs_dwconv_fwd", bufs, check)
    r["y"] = r["y"].view(N, H, W, Cc)
    return r


def call_dwconv_bwd(x, w, dy, ks, want_dx=True, want_dw=True, want_db=True, ws_short=0, check=True):
    L, lib, rt = _env()
    N, H, W, Cc = x.shape
    xd, wd, gd = _fresh(x), _fresh(w), _fresh(dy)
    full = int(lib.hs_dwconv_ws_bytes(N, H, W, Cc, ks)) if ks in (3, 5, 7) else 64
    bufs = {"dx": _act(N, H, W, Cc, x.dtype) if want_dx else None, "dw": GBuf(Cc, ks * ks, F32) if want_dw else None,
            "db": GBuf(1, Cc, F32, is_vec=True) if want_db else None, "ws": _Ws(full)}
    st = lib.hs_dwconv_bwd(rt.hs_dtype(x.dtype), _p(xd), _p(wd), _p(gd), _p(bufs["dx"]), _p(bufs["dw"]), _p(bufs["db"]), N, H, W,
                           Cc, ks, _p(bufs["ws"]), full - ws_short, rt.stream())
    r = _finish(L, st, "hs_dwconv_bwd", bufs, check)
    if want_dx:
        r["dx"] = r["dx"].view(N, H, W, Cc)
    r["ws_bytes"] = full
    return r


# ======================================================================================================================
# layer scale
# ======================================================================================================================
def _rowfac(rowscale, rps, M, dtype):
    if rowscale is None:
        return torch.ones(M, 1, dtype=dtype)
    return rowscale.to(dtype)[torch.arange(M) // rps][:, None]


def layerscale_ref64(u, res, dy, gamma, rowscale, rps):
    """out = res + gamma * rs[m / rps] * u;  du = gamma * rs * dy;  dgamma[c] = sum_m rs * dy * u"""
    M = u.shape[0]
    rs = _rowfac(rowscale, rps, M, F64)
    u, res, dy, g = u.double(), res.double(), dy.double(), gamma.double()
    t = rs * dy * u
    return {"out": res + (g * rs) * u, "du": (dy * rs) * g, "dgamma": t.sum(0), "terms": t}


def layerscale_yard(u, res, dy, gamma, rowscale, rps):
    dt = u.dtype
    M = u.shape[0]
    rs = _rowfac(rowscale, rps, M, F32)
    u, res, dy, g = u.float(), res.float(), dy.float(), gamma.float()
    d = dy * rs
    return {"out": (res + (g * rs) * u).to(dt), "du": (d * g).to(dt), "dgamma": torch.from_numpy(seq_sum32((d * u).numpy(), 0))}


def ls_geometry(M, Cc):
    """launch geometry of layerscale_bwd as its header states it: gy = clamp(M / 16, 1, 256) row groups; per column block
    ncol = min(256, C/4 - 256 * block) four-channel columns and rpb = 256 / ncol rows per pass -> gy, [(ncol, rpb)]"""
    gy = min(max(M // 16, 1), 256)
    c4 = Cc // 4
    blocks = []
    for b in range(-(-c4 // 256)):
        ncol = min(256, c4 - 256 * b)
        blocks.append((ncol, 256 // ncol))
    return gy, blocks


def layerscale_floor(ref, M, Cc):
    """dgamma[c] is a float32 sum of M signed products.  A thread chains ceil(M / (gy * rpb)) fused products, the block folds
    rpb rows through LDS one after the other, the final kernel adds ceil(gy / 8) partials per accumulator and folds the
    accumulators in three steps: D = ceil(M / (gy * rpb)) + rpb + ceil(gy / 8) + 3 + 1 (the product rs * dy), the largest over
    the column blocks.  -> relative-L2 floor by chain_floor."""
    gy, blocks = ls_geometry(M, Cc)
    D = max(-(-M // (gy * rpb)) + rpb + -(-gy // 8) + 4 for _, rpb in blocks)
    return chain_floor(ref["terms"], D)


def _lsc(M, Cc, rps, seed, kind="plain", zero=True):
    return {"M": M, "C": Cc, "rps": rps, "seed": seed, "kind": kind, "zero": zero,
            "tag": f"layerscale M={M} C={Cc} rps={rps}" + (" int" if kind == "int" else "")}


def layerscale_cases():
    """C in {4, 12, 132, 1024, 1028, 1540}: ncol = 1, 3, 33, 256, then 256 + 1 and 256 + 129 over two column blocks (rpb = 256,
    85, 7, 1, 256, 1); M in {1, 5, 31, 32, 257}, and M = 4112 at C = 4 and C = 1028 (gy at its cap of 256; with rpb = 1 the row
    loop strides 16 times).  rps None = rowscale NULL, else rows_per_sample in {1, 7, M}."""
    return [_lsc(1, 4, None, 500), _lsc(5, 12, 1, 501), _lsc(31, 132, 7, 502), _lsc(32, 1024, 32, 503), _lsc(257, 1028, 7, 504),
            _lsc(5, 1540, None, 505), _lsc(257, 4, 1, 506), _lsc(32, 12, 7, 507), _lsc(1, 1540, 1, 508, zero=False),
            _lsc(31, 1028, 31, 509, zero=False), _lsc(4112, 4, 7, 510), _lsc(4112, 1028, 7, 511), _lsc(4112, 4, None, 512),
            _lsc(257, 132, 7, 513, kind="int"), _lsc(4112, 1028, None, 514, kind="int")]


def layerscale_data(c, dtype):
    """-> u, res, dy [M][C] (kernel dtype), gamma [C], rowscale [ceil(M / rps)] or None: stochastic-depth factors, about one in
    five of them 0.  With two samples or more, sample 0 is kept and, when c["zero"], sample 1 is exactly 0."""
    M, Cc, rps = c["M"], c["C"], c["rps"]
    g = gen(c["seed"])
    if c["kind"] == "int":         # |rs dy u| <= 2 * 8 * 8, M <= 2^13: every partial sum below 2^24
        u, res, dy = (int_data(g, M, Cc) for _ in range(3))
        gamma = torch.randint(-2, 3, (Cc,), generator=g).float()
    else:
        u, res, dy = (torch.randn(M, Cc, generator=g) for _ in range(3))
        gamma = 0.5 * torch.randn(Cc, generator=g)
    rs = None
    if rps is not None:
        ns = -(-M // rps)
        if c["kind"] == "int":
            rs = torch.randint(0, 3, (ns,), generator=g).float()
        else:
            rs = torch.where(torch.rand(ns, generator=g) < 0.8, torch.tensor(1.25), torch.tensor(0.0)) + 0.01 * torch.rand(ns, generator=g)
        if ns >= 2:
            rs[0] = 1.25 if c["kind"] != "int" else 2.0
            if c["zero"]:
                rs[1] = 0.0
    return u.to(dtype), res.to(dtype), dy.to(dtype), gamma, rs


def call_layerscale_fwd(u, res, gamma, rowscale, rps, C_arg=None, check=True):
    L, lib, rt = _env()
    M, Cc = u.shape
    ud, rd, gd, sd = _fresh(u), _fresh(res), _fresh(gamma), _fresh(rowscale)
    bufs = {"out": GBuf(M, Cc, u.dtype)}
    st = lib.hs_layerscale_fwd(rt.hs_dtype(u.dtype), _p(ud), _p(gd), _p(sd), rps or 0, _p(rd), _p(bufs["out"]), M,
                               Cc if C_arg is None else C_arg, rt.stream())
    return _finish(L, st, "hs_layerscale_fwd", bufs, check)


def call_layerscale_bwd(dy, u, gamma, rowscale, rps, want_du=True, C_arg=None, ws_short=0, check=True):
    L, lib, rt = _env()
    M, Cc = u.shape
    gd_, ud, gd, sd = _fresh(dy), _fresh(u), _fresh(gamma), _fresh(rowscale)
    full = int(lib.hs_layerscale_ws_bytes(M, Cc))
    bufs = {"du": GBuf(M, Cc, u.dtype) if want_du else None, "dgamma": GBuf(1, Cc, F32, is_vec=True), "ws": _Ws(full)}
    st = lib.hs_layerscale_bwd(rt.hs_dtype(u.dtype), _p(gd_), _p(ud), _p(gd), _p(sd), rps or 0, _p(bufs["du"]), _p(bufs["dgamma"]),
                               _p(bufs["ws"]), full - ws_short, M, Cc if C_arg is None else C_arg, rt.stream())
    return _finish(L, st, "hs_layerscale_bwd", bufs, check)


# ======================================================================================================================
# patchify (pure data movement)
# ======================================================================================================================
def patchify_ref(x, k):
    """out[(n,p,q)][(r*k+s)*C + c] = x[n][p*k+r][q*k+s][c], P = H // k, Q = W // k -> [N*P*Q][k*k*C] in the dtype of x"""
    N, H, W, Cc = x.shape
    P, Q = H // k, W // k
    return x[:, :P * k, :Q * k, :].reshape(N, P, k, Q, k, Cc).permute(0, 1, 3, 2, 4, 5).reshape(N * P * Q, k * k * Cc).contiguous()


def patchify_bwd_ref(dp, N, H, W, Cc, k):
    """the inverse scatter; rows / columns of x beyond P*k / Q*k get exact zeros.  dp: [N*P*Q][k*k*C]"""
    P, Q = H // k, W // k
    dx = torch.zeros(N, H, W, Cc, dtype=dp.dtype)
    dx[:, :P * k, :Q * k, :] = dp.reshape(N, P, Q, k, k, Cc).permute(0, 1, 3, 2, 4, 5).reshape(N, P * k, Q * k, Cc)
    return dx


def patchify_cases():
    """C in {3, 4, 8, 12, 24}: the 16-byte vector path needs C % 4 == 0 (f32) or C % 8 == 0 (bf16), so each dtype sees both
    paths; k in {1, 2, 3, 4}; H % k and W % k nonzero wherever k > 1; totals that are no multiple of 256.
    pad: 0 (ldo = k*k*C), 8 (a multiple of both vector widths) and 3 (none: forces the scalar path)."""
    shapes = [(2, 5, 7, 3, 2), (1, 9, 10, 4, 4), (2, 7, 5, 8, 3), (1, 4, 3, 12, 1), (2, 6, 9, 24, 4), (3, 5, 5, 8, 2), (1, 11, 7, 4, 3)]
    cases = []
    for i, (N, H, W, Cc, k) in enumerate(shapes):
        for pad in (0, 8, 3):
            cases.append({"N": N, "H": H, "W": W, "C": Cc, "k": k, "ld": k * k * Cc + pad, "seed": 600 + i,
                          "tag": f"patchify N={N} H={H} W={W} C={Cc} k={k} ld=k*k*C+{pad}"})
    return cases


def patchify_data(c, dtype):
    """x: every element a distinct small integer where the dtype can hold them apart (f32), random values otherwise"""
    g = gen(c["seed"])
    shape = (c["N"], c["H"], c["W"], c["C"])
    n = int(np.prod(shape))
    x = (torch.arange(1, n + 1).float().reshape(shape) if dtype == F32 else torch.randn(shape, generator=g) + 3.0)
    return x.to(dtype)


def call_patchify_fwd(x, k, ld, check=True):
    L, lib, rt = _env()
    N, H, W, Cc = x.shape
    rows = N * (H // k) * (W // k)
    xd = _fresh(x)
    bufs = {"out": GBuf(max(rows, 1), ld, x.dtype)}
    st = lib.hs_patchify_fwd(rt.hs_dtype(x.dtype), _p(xd), _p(bufs["out"]), N, H, W, Cc, k, ld, rt.stream())
    return _finish(L, st, "hs_patchify_fwd", bufs, check)


def call_patchify_bwd(dp, N, H, W, Cc, k, ld_arg=None, check=True):
    """dp [rows][ld] as the kernel reads it (padding columns included)"""
    L, lib, rt = _env()
    dd = _fresh(dp)
    bufs = {"dx": GBuf(N * H * W, Cc, dp.dtype)}
    st = lib.hs_patchify_bwd(rt.hs_dtype(dp.dtype), _p(dd), _p(bufs["dx"]), N, H, W, Cc, k, dp.shape[1] if ld_arg is None else ld_arg,
                             rt.stream())
    r = _finish(L, st, "hs_patchify_bwd", bufs, check)
    r["dx"] = r["dx"].view(N, H, W, Cc)
    return r


# ======================================================================================================================
# MoE gating
# ======================================================================================================================
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
GATE_EPS = 1e-2              # noise_eps of the cases
GATE_COEF = 1e-2
REL_MARGIN = 1e-3            # the leading probabilities of a row differ pairwise by at least this, relative
THR_MARGIN = 1e-3            # every noisy logit lies at least this far from the row's in-threshold
GATE_BS = (1, 63, 64, 65, 200)
GATE_EK = ((1, 1), (2, 1), (4, 2), (4, 4), (16, 1), (16, 15), (16, 16))


def _cv2(x):
    """moe.py:171-186: unbiased variance / (mean^2 + 1e-10); 0 for a single expert"""
    if x.shape[0] == 1:
        return x.sum() * 0.0
    return x.var() / (x.mean() ** 2 + _f32(1e-10))


def _stable_top(p, m):
    """indices of the m largest per row, ties: lowest index first (a stable descending sort)"""
    return torch.sort(p, dim=1, descending=True, stable=True).indices[:, :m]


def gate_fwd64(clean, raw, z, k, noisy, noise_eps=GATE_EPS, coef=GATE_COEF, grad=None):
    """The gating of the header / moe.py:231-291 in float64: sigma = softplus(raw) (threshold 20) + noise_eps, h = clean + z sigma,
    p = softmax(h), top-(k+1) of p, gates = p / (sum of the top k + 1e-6) scattered, load = Phi((clean - thr) / sigma) summed
    (thr = p[top[k]] where h > p[top[k]], else p[top[k-1]]: the thresholds are probabilities compared with logits, as in the
    reference) or the count of gates > 0, loss = coef (cv^2(importance) + cv^2(load)).
    grad = (dgates, g_loss or None): also d_clean, d_raw of sum(gates * dgates) + g_loss * loss by autograd."""
    B, E = clean.shape
    c = clean.double().clone().requires_grad_(grad is not None)
    r = None
    if noisy:
        r = raw.double().clone().requires_grad_(grad is not None)
        sigma = torch.where(r > 20.0, r, torch.log1p(torch.exp(torch.clamp(r, max=20.0)))) + _f32(noise_eps)
        zz = z.double()
        h = c + zz * sigma
    else:
        sigma, zz, h = torch.zeros(B, E, dtype=F64), torch.zeros(B, E, dtype=F64), c
    e = torch.exp(h - h.max(1, keepdim=True).values.detach())
    p = e / e.sum(1, keepdim=True)
    m = min(k + 1, E)
    top = _stable_top(p.detach(), m)
    pk = p.gather(1, top[:, :k])
    gates = torch.zeros(B, E, dtype=F64).scatter(1, top[:, :k], pk / (pk.sum(1, keepdim=True) + _f32(1e-6)))
    if noisy and k < E:
        thr_in, thr_out = p.gather(1, top[:, k:k + 1]), p.gather(1, top[:, k - 1:k])
        is_in = h > thr_in
        loadrow = 0.5 * (1.0 + torch.erf((c - torch.where(is_in, thr_in, thr_out)) / sigma * SQRT1_2))
        thr_gap = (h - thr_in).abs().min().item()
    else:
        loadrow = (gates > 0).double()
        thr_gap = float("inf")
    imp, load = gates.sum(0), loadrow.sum(0)
    loss = _f32(coef) * (_cv2(imp) + _cv2(load))
    il, ll = imp.detach().clone().requires_grad_(True), load.detach().clone().requires_grad_(True)
    lleaf = _f32(coef) * (_cv2(il) + _cv2(ll))
    d_imp, d_load = torch.autograd.grad(lleaf, (il, ll), allow_unused=True) if E > 1 else (torch.zeros(E, dtype=F64),) * 2
    srt = torch.sort(p.detach(), dim=1, descending=True).values[:, :min(k + 2, E)]
    rel_gap = ((srt[:, :-1] - srt[:, 1:]) / srt[:, :-1]).min().item() if srt.shape[1] > 1 else float("inf")
    o = {"gates": gates.detach(), "p": p.detach(), "sigma": sigma.detach(), "z": zz, "loadrow": loadrow.detach(),
         "loss": loss.detach().reshape(1), "d_imp": d_imp, "d_load": d_load, "top": top.to(I32), "h": h.detach(),
         "imp": imp.detach(), "load": load.detach(), "rel_gap": rel_gap, "thr_gap": thr_gap}
    if grad is not None:
        dg, gl = grad
        obj = (gates * dg.double()).sum() + (0.0 if gl is None else float(gl) * loss)
        gs = torch.autograd.grad(obj, (c, r) if noisy else (c,), allow_unused=True)
        o["d_clean"] = gs[0] if gs[0] is not None else torch.zeros(B, E, dtype=F64)
        o["d_raw"] = (gs[1] if noisy and gs[1] is not None else torch.zeros(B, E, dtype=F64))
    return o


def _erf32(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def _cv2_32(x, E):
    """cv^2 and its gradient in sequential float32, as the formula reads"""
    f = np.float32
    if E == 1:
        return f(0.0), np.zeros(1, dtype=np.float32)
    mu = seq_sum32(x, 0) / f(E)
    d = x - mu
    var = seq_sum32(d * d, 0) / f(E - 1)
    den = mu * mu + f(1e-10)
    return var / den, f(2.0) * d / f(E - 1) / den - var * (f(2.0) * mu / f(E)) / (den * den)


def gate_fwd_yard(clean, raw, z, k, noisy, noise_eps=GATE_EPS, coef=GATE_COEF):
    f = np.float32
    c = _np32(clean)
    B, E = c.shape
    if noisy:
        r, zz = _np32(raw), _np32(z)
        sigma = np.where(r > f(20.0), r, np.log1p(expf32(np.minimum(r, f(20.0))))).astype(np.float32) + f(noise_eps)
        h = c + zz * sigma
    else:
        sigma, zz, h = np.zeros_like(c), np.zeros_like(c), c
    e = expf32(h - h.max(1, keepdims=True))
    p = e / seq_sum32(e, 1)[:, None]
    m = min(k + 1, E)
    top = _stable_top(torch.from_numpy(p), m).numpy()
    pk = np.take_along_axis(p, top[:, :k], 1)
    gk = pk / (seq_sum32(pk, 1)[:, None] + f(1e-6))
    gates = np.zeros_like(p)
    np.put_along_axis(gates, top[:, :k], gk, 1)
    if noisy and k < E:
        thr_in, thr_out = np.take_along_axis(p, top[:, k:k + 1], 1), np.take_along_axis(p, top[:, k - 1:k], 1)
        uu = (c - np.where(h > thr_in, thr_in, thr_out)) / sigma
        loadrow = f(0.5) * (f(1.0) + _erf32(uu * f(SQRT1_2)))
    else:
        loadrow = (gates > 0).astype(np.float32)
    l1, d1 = _cv2_32(seq_sum32(gates, 0), E)
    l2, d2 = _cv2_32(seq_sum32(loadrow, 0), E)
    o = {"gates": gates, "p": p, "sigma": sigma, "z": zz, "loadrow": loadrow, "loss": np.reshape(f(coef) * (l1 + l2), 1),
         "d_imp": f(coef) * d1, "d_load": f(coef) * d2}
    o = {kk: _out(v, F32) for kk, v in o.items()}
    o["top"] = torch.from_numpy(top).to(I32)
    return o


def gate_aux_floors(ref, B, E, coef=GATE_COEF):
    """loss = coef (cv2(imp) + cv2(load)), cv2(x) = var / (mean^2 + 1e-10), with imp and load float32 sums of B non-negative
    terms each (one thread, sequential: rel error B u).  x - mean cancels when the experts are evenly used:
        |err (x_e - mu)| <= 2 (B + E) u max|x|,
        |err var| <= (2 * 2 (B + E) u max|x| sum_e |x_e - mu| + (E + 3) u sum_e (x_e - mu)^2) / (E - 1),
        |err cv2| <= |err var| / den + (2 (B + E) + 3) u cv2,
        |err dcv2_e| <= 2 |err (x_e - mu)| / (E - 1) / den + (|err var| / var + (4 (B + E) + 8) u) |var 2 mu / (E den^2)|
                        + (2 (B + E) + 4) u |2 (x_e - mu) / ((E - 1) den)|.
    -> floors relative to |loss| (sum of both terms), max|d_imp|, max|d_load| (0 = the plain 1e-6 where undefined)"""
    out = {}
    tot = 0.0
    for name, x in (("d_imp", ref["imp"]), ("d_load", ref["load"])):
        if E == 1:
            out[name] = 0.0
            continue
        n = 2.0 * (B + E) * U
        mu = x.mean()
        d = x - mu
        var = (d * d).sum() / (E - 1)
        den = mu * mu + _f32(1e-10)
        ed = n * x.abs().max()
        evar = (2.0 * ed * d.abs().sum() + (E + 3) * U * (d * d).sum()) / (E - 1)
        tot += (evar / den + (n + 3 * U) * var / den).item()
        second = (var * 2.0 * mu / (E * den * den)).abs()
        first = (2.0 * d / ((E - 1) * den)).abs()
        relvar = (evar / var).item() if var > 0 else 0.0
        bound = 2.0 * ed / (E - 1) / den + (relvar + 2 * n + 8 * U) * second + (n + 4 * U) * first
        top = ref[name].abs().max().item()
        out[name] = (bound.max().item() / (top / _f32(coef))) if top > 0 else 0.0
    lt = ref["loss"].abs().item()
    out["loss"] = (_f32(coef) * tot / lt) if lt > 0 else 0.0
    return out


def gate_data(B, E, k, noisy, seed):
    """-> clean, raw, z [B][E] float32, redraws.  raw holds values on both sides of the softplus threshold 20 (their z is kept
    small so the logits stay moderate).  Selection is discontinuous, so the inputs decide it: a row whose leading
    min(k + 2, E) probabilities (float64) are closer than REL_MARGIN relative, or of which a noisy logit lies within THR_MARGIN
    of the in-threshold, is redrawn from the same generator until every row passes."""
    g = gen(seed)

    def draw(n):
        return 1.5 * torch.randn(n, E, generator=g), torch.randn(n, E, generator=g), torch.randn(n, E, generator=g)

    clean, raw, z = draw(B)
    for (i, v) in (((B * E) // 3, 20.0), ((B * E) // 2, 25.0), (B * E - 1, 19.5), (0, 20.5)):     # (the later ones win a clash)
        raw.view(-1)[i], z.view(-1)[i] = v, 0.05 * (1 if i % 2 == 0 else -1)
    redraws = 0
    while True:
        bad = gate_bad_rows(clean, raw, z, k, noisy)
        if not bad.any():
            return clean, raw, z, redraws
        redraws += 1
        if redraws > 1000:
            raise RuntimeError("gate_data: margins not reached")
        n = int(bad.sum())
        c2, r2, z2 = draw(n)
        clean[bad], z[bad] = c2, z2
        rr = raw[bad]
        keep = rr >= 19.0                      # the threshold probes stay where they are
        raw[bad] = torch.where(keep, rr, r2)
        zb = z[bad]
        z[bad] = torch.where(keep, 0.05 * torch.sign(zb + 1e-9), zb)


def gate_bad_rows(clean, raw, z, k, noisy):
    B, E = clean.shape
    f = gate_fwd64(clean, raw, z, k, noisy)
    srt = torch.sort(f["p"], dim=1, descending=True).values[:, :min(k + 2, E)]
    bad = torch.zeros(B, dtype=torch.bool)
    if srt.shape[1] > 1:
        bad |= (((srt[:, :-1] - srt[:, 1:]) / srt[:, :-1]) < REL_MARGIN).any(1)
    if noisy and k < E:
        thr = f["p"].gather(1, f["top"][:, k:k + 1].long())
        bad |= ((f["h"] - thr).abs() < THR_MARGIN).any(1)
    return bad


def gate_cases():
    cases = []
    for i, B in enumerate(GATE_BS):
        for j, (E, k) in enumerate(GATE_EK):
            for noisy in (1, 0):
                cases.append({"B": B, "E": E, "k": k, "noisy": noisy, "seed": 700 + 10 * i + j,
                              "tag": f"gate B={B} E={E} k={k} noisy={noisy}"})
    return cases


def gate_bwd_inputs(c):
    """-> dgates [B][E], g_loss (a float): the upstream gradients of the case"""
    g = gen(c["seed"] + 5000)
    return torch.randn(c["B"], c["E"], generator=g), 0.75


def gate_bwd_yard(clean, raw, sv, dgates, g_loss, k, noisy):
    """The hand-derived gradient in sequential float32 on the float32 saved tensors sv (p, top, z, sigma, d_imp, d_load):
    gates_i = p_i / (S + 1e-6) -> dp; the load term Phi((c - thr) / sigma) -> d clean, d sigma and minus the same on the
    threshold's probability; softmax backward; d raw through the softplus."""
    f = np.float32
    c, p, z, sg = _np32(clean), _np32(sv["p"]), _np32(sv["z"]), _np32(sv["sigma"])
    dg = _np32(dgates)
    B, E = c.shape
    top = sv["top"].long().numpy()
    gl = f(0.0 if g_loss is None else g_loss)
    gi = dg + gl * _np32(sv["d_imp"])[None, :]
    tk = top[:, :k]
    pk, gk = np.take_along_axis(p, tk, 1), np.take_along_axis(gi, tk, 1)
    inv = f(1.0) / (seq_sum32(pk, 1) + f(1e-6))
    dot = seq_sum32(gk * pk * inv[:, None], 1)
    dp = np.zeros_like(p)
    np.put_along_axis(dp, tk, (gk - dot[:, None]) * inv[:, None], 1)
    dc, dsg = np.zeros_like(p), np.zeros_like(p)
    if noisy and k < E:
        thr_in, thr_out = np.take_along_axis(p, top[:, k:k + 1], 1), np.take_along_axis(p, top[:, k - 1:k], 1)
        h = c + z * sg
        is_in = h > thr_in
        uu = (c - np.where(is_in, thr_in, thr_out)) / sg
        gq = gl * _np32(sv["d_load"])[None, :] * (f(INV_SQRT_2PI) * expf32(f(-0.5) * uu * uu)) / sg
        dc += gq
        dsg += -gq * uu
        for e in range(E):                                           # sequential over e, as one thread does it
            col = np.where(is_in[:, e], top[:, k], top[:, k - 1])
            dp[np.arange(B), col] -= gq[:, e]
    sp = seq_sum32(p * dp, 1)
    dh = p * (dp - sp[:, None])
    dc = dc + dh
    d_raw = np.zeros_like(p)
    if noisy:
        dsg = dsg + dh * z
        d_raw = dsg / (f(1.0) + expf32(-_np32(raw)))
    return {"d_clean": _out(dc, F32), "d_raw": _out(d_raw, F32)}


def gate_bwd_floors(clean, raw, ref, dgates, g_loss, k, noisy):
    """A-priori float32 rounding bounds of d_clean and d_raw, in units of u = 2^-24, following the kernel's formula step by
    step.  Every saved tensor carries one rounding of its own.
      gi_e = dgates_e + g_loss d_imp_e, of magnitude G_e = |dgates_e| + |g_loss d_imp_e|:                err <= 3 G_e
      inv = 1 / (sum of the top k p + 1e-6):                                                            rel <= k + 4
      dot = sum_i gi_i p_i inv, of magnitude Dm = sum_i G_i p_i inv:                                     err <= (2 k + 11) Dm
      dp_e = (gi_e - dot) inv.  For k = 1 this is gi (1 - p inv) inv with 1 - p inv = 1e-6 / (p + 1e-6): the difference cancels
        all but entirely, while the roundings scale with A_e = (G_e + Dm) inv:            err <= (2 k + 12) A_e + (k + 5) |dp_e|
      load term (noisy, k < E): uu = (c - thr) / sigma, gq = g_loss d_load pdf(uu) / sigma; c - thr is rounded on |c| + |thr|
        and pdf'(uu) / pdf = -uu magnifies that:             rel(gq) <= 8 + 3 uu^2 + 2 |uu| (|c| + |thr|) / sigma =: Q_e / |gq_e|
        the threshold's dp takes -gq of every expert routed to it, one after the other: err += sum Q + E (|dp| + sum |gq|)
      sp = sum_j p_j dp_j:                                            err <= sum_j p_j err(dp_j) + (E + 2) sum_j p_j |dp_j|
      dh_e = p_e (dp_e - sp):        err <= p_e (err(dp_e) + sum_j p_j err(dp_j) + (E + 3) (|dp_e| + sum_j p_j |dp_j|)) + 2 |dh_e|
      d_clean_e = gq_e + dh_e:       err <= Q_e + err(dh_e) + |gq_e| + |dh_e|
      d_raw_e = (-gq_e uu_e + dh_e z_e) sigmoid(raw_e), the sigmoid through __expf (rel <= 4 + |raw_e|):
        err <= sigmoid (Q_e |uu_e| + |gq_e| (2 (|c| + |thr|) / sigma + 3 |uu_e|) + |z_e| err(dh_e) + 3 |dh_e z_e|) + (6 + |raw_e|) |d_raw_e|
    -> floors relative to max|d_clean|, max|d_raw| (0 where the reference vanishes).  Where k = 1 and the load term is absent
    or small, the reference is of the order 1e-6 |dgates| and the floor approaches or exceeds 1: float32 cannot do better there."""
    B, E = clean.shape
    c, p, z, sg = clean.double(), ref["p"], ref["z"], ref["sigma"]
    top = ref["top"].long()
    gl = 0.0 if g_loss is None else float(g_loss)
    gi = dgates.double() + gl * ref["d_imp"][None, :]
    G = dgates.double().abs() + abs(gl) * ref["d_imp"].abs()[None, :]
    tk = top[:, :k]
    pk = p.gather(1, tk)
    inv = 1.0 / (pk.sum(1, keepdim=True) + _f32(1e-6))
    gk, Gk = gi.gather(1, tk), G.gather(1, tk)
    zero = torch.zeros(B, E, dtype=F64)
    dp = zero.scatter(1, tk, (gk - (gk * pk * inv).sum(1, keepdim=True)) * inv)
    A = zero.scatter(1, tk, (Gk + (Gk * pk * inv).sum(1, keepdim=True)) * inv)
    edp = (2 * k + 12) * A + (k + 5) * dp.abs()
    Q, uu, gq, spread = zero, zero, zero, zero
    if noisy and k < E:
        thr_in, thr_out = p.gather(1, top[:, k:k + 1]), p.gather(1, top[:, k - 1:k])
        is_in = ref["h"] > thr_in
        thr = torch.where(is_in, thr_in, thr_out)
        uu = (c - thr) / sg
        gq = gl * ref["d_load"][None, :] * INV_SQRT_2PI * torch.exp(-0.5 * uu * uu) / sg
        spread = (c.abs() + thr) / sg
        Q = gq.abs() * (8.0 + 3.0 * uu * uu + 2.0 * uu.abs() * spread)
        to = torch.where(is_in, top[:, k:k + 1], top[:, k - 1:k])
        edp = edp + zero.scatter_add(1, to, Q) + E * (dp.abs() + zero.scatter_add(1, to, gq.abs()))
        dp = dp - zero.scatter_add(1, to, gq)
    pdp = (p * dp.abs()).sum(1, keepdim=True)
    dh = p * (dp - (p * dp).sum(1, keepdim=True))
    edh = p * (edp + (p * edp).sum(1, keepdim=True) + (E + 3) * (dp.abs() + pdp)) + 2.0 * dh.abs()
    out = {"d_clean": U * (Q + edh + gq.abs() + dh.abs()), "d_raw": zero}
    if noisy:
        r = raw.double()
        out["d_raw"] = U * (torch.sigmoid(r) * (Q * uu.abs() + gq.abs() * (2.0 * spread + 3.0 * uu.abs()) + z.abs() * edh
                                                + 3.0 * (dh * z).abs()) + (6.0 + r.abs()) * ref["d_raw"].abs())
    for name in ("d_clean", "d_raw"):
        t = ref[name].abs().max().item()
        out[name] = (out[name].max().item() / t) if t > 0 else 0.0
    return out


def gate_saved32(ref):
    """the float32 tensors the backward kernel reads: the float64 forward rounded once"""
    return {kk: ref[kk].float() for kk in ("p", "z", "sigma", "d_imp", "d_load")} | {"top": ref["top"]}


def _ibuf(rows, ld):
    return GBuf(rows, ld, I32)


def call_gate_fwd(clean, raw, noise, k, noisy, seed=0, noise_eps=GATE_EPS, coef=GATE_COEF, B_arg=None, E_arg=None, check=True):
    L, lib, rt = _env()
    B, E = clean.shape
    cd, rd, nd = _fresh(clean), _fresh(raw), _fresh(noise)
    bufs = {kk: GBuf(B, E, F32) for kk in ("gates", "p", "z", "sigma", "loadrow")}
    bufs["top"] = _ibuf(B, MOE_TOPW)
    bufs["loss"] = GBuf(1, 1, F32, is_vec=True)
    bufs["d_imp"], bufs["d_load"] = GBuf(1, E, F32, is_vec=True), GBuf(1, E, F32, is_vec=True)
    st = lib.hs_moe_gate_fwd(_p(cd), _p(rd), _p(nd), B if B_arg is None else B_arg, E if E_arg is None else E_arg, k, noisy,
                             noise_eps, seed, coef, _p(bufs["gates"]), _p(bufs["p"]), _p(bufs["top"]), _p(bufs["z"]),
                             _p(bufs["sigma"]), _p(bufs["loadrow"]), _p(bufs["loss"]), _p(bufs["d_imp"]), _p(bufs["d_load"]),
                             rt.stream())
    return _finish(L, st, "hs_moe_gate_fwd", bufs, check)


def call_gate_bwd(clean, raw, sv, dgates, g_loss, k, noisy, want_raw=True, B_arg=None, E_arg=None, check=True):
    """sv: p, top ([B][17] int32), z, sigma, d_imp, d_load (CPU)"""
    L, lib, rt = _env()
    B, E = clean.shape
    cd, rd, dg = _fresh(clean), _fresh(raw), _fresh(dgates)
    s = {kk: _fresh(v) for kk, v in sv.items()}
    gl = None if g_loss is None else torch.tensor([g_loss], dtype=F32, device=DEV)
    bufs = {"d_clean": GBuf(B, E, F32), "d_raw": GBuf(B, E, F32) if want_raw else None}
    st = lib.hs_moe_gate_bwd(_p(cd), _p(rd), _p(s["p"]), _p(s["top"]), _p(s["z"]), _p(s["sigma"]), _p(dg), _p(gl), _p(s["d_imp"]),
                             _p(s["d_load"]), B if B_arg is None else B_arg, E if E_arg is None else E_arg, k, noisy,
                             _p(bufs["d_clean"]), _p(bufs["d_raw"]), rt.stream())
    return _finish(L, st, "hs_moe_gate_bwd", bufs, check)


def top_rows(top, B):
    """[B][m] indices -> the [B][17] int32 rows the kernels exchange, unused entries sentinel"""
    t = torch.full((B, MOE_TOPW), int(SENT), dtype=I32)
    t[:, :top.shape[1]] = top
    return t


# ======================================================================================================================
# MoE combine, dispatch, row gather / scatter
# ======================================================================================================================
def routing_gates(B, E, g, k=None):
    """gates [B][E] with exact zeros: each row keeps k (default about half) of its experts, normalised"""
    k = max(1, (E + 1) // 2) if k is None else k
    gt = torch.zeros(B, E)
    for b in range(B):
        sel = torch.randperm(E, generator=g)[:k]
        v = torch.rand(k, generator=g) + 0.1
        gt[b, sel] = v / v.sum()
    return gt


def combine_cases():
    """E in {1, 3, 16}, O in {1, 63, 64, 65, 200} (a wave walks a row 64 at a time), B in {1, 5, 67} (B * E not a multiple of the
    four waves of a block)"""
    cases = []
    for i, (B, E, O) in enumerate(((1, 1, 1), (5, 3, 63), (67, 16, 64), (5, 16, 65), (67, 3, 200), (1, 3, 200), (67, 1, 65),
                                   (5, 1, 64), (1, 16, 63), (67, 3, 1))):
        cases.append({"B": B, "E": E, "O": O, "seed": 800 + i, "tag": f"combine B={B} E={E} O={O}"})
    return cases


def combine_data(c):
    """-> gates [B][E], outs: E tensors [B][O] (rows of an expert whose gate is 0 hold HUGE), dy [B][O]"""
    g = gen(c["seed"])
    B, E, O = c["B"], c["E"], c["O"]
    gates = routing_gates(B, E, g)
    outs = []
    for e in range(E):
        o = torch.randn(B, O, generator=g)
        o[gates[:, e] == 0] = HUGE
        outs.append(o)
    return gates, outs, torch.randn(B, O, generator=g)


def combine_ref64(gates, outs, dy):
    """y = sum_e gates[:, e] out_e over the experts with a nonzero gate (a zero gate contributes nothing);
    d out_e = gates[:, e] dy; dgates[b][e] = <dy[b], out_e[b]>.  terms: [E][B*O] of y, dterms: [O][B*E] of dgates."""
    gd, dyd = gates.double(), dy.double()
    od = torch.stack([o.double() for o in outs], 0)                       # [E][B][O]
    live = (gd != 0).t()[:, :, None]
    t = torch.where(live, gd.t()[:, :, None] * od, torch.zeros_like(od))
    dt = (dyd[None] * od).permute(2, 1, 0)                                # [O][B][E]
    return {"y": t.sum(0), "douts": [gd[:, e:e + 1] * dyd for e in range(len(outs))], "dgates": dt.sum(0),
            "terms": t.reshape(t.shape[0], -1), "dterms": dt.reshape(dt.shape[0], -1)}


def combine_yard(gates, outs, dy):
    g = _np32(gates)
    B, E = g.shape
    acc = np.zeros_like(_np32(dy))
    for e in range(E):
        with np.errstate(over="ignore", invalid="ignore"):
            acc = acc + np.where(g[:, e:e + 1] != 0, g[:, e:e + 1] * _np32(outs[e]), np.float32(0.0))
    dgt = np.stack([seq_sum32(_np32(dy) * _np32(outs[e]), 1) for e in range(E)], 1)
    return {"y": _out(acc, F32), "douts": [_out(g[:, e:e + 1] * _np32(dy), F32) for e in range(E)], "dgates": _out(dgt, F32)}


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[_p(t) for t in ts])


def call_combine_fwd(gates, outs, B_arg=None, O_arg=None, check=True):
    L, lib, rt = _env()
    B, E = gates.shape
    O = outs[0].shape[1]
    gd, od = _fresh(gates), [_fresh(o) for o in outs]
    bufs = {"y": GBuf(B, O, F32)}
    st = lib.hs_moe_combine_fwd(_p(gd), _ptrs(od), _p(bufs["y"]), B if B_arg is None else B_arg, E, O if O_arg is None else O_arg,
                                rt.stream())
    return _finish(L, st, "hs_moe_combine_fwd", bufs, check)


def call_combine_bwd(gates, outs, dy, B_arg=None, O_arg=None, check=True):
    L, lib, rt = _env()
    B, E = gates.shape
    O = outs[0].shape[1]
    gd, od, dd = _fresh(gates), [_fresh(o) for o in outs], _fresh(dy)
    bufs = {f"dout{e}": GBuf(B, O, F32) for e in range(E)}
    bufs["dgates"] = GBuf(B, E, F32)
    st = lib.hs_moe_combine_bwd(_p(gd), _ptrs(od), _p(dd), _ptrs([bufs[f"dout{e}"] for e in range(E)]), _p(bufs["dgates"]),
                                B if B_arg is None else B_arg, E, O if O_arg is None else O_arg, rt.stream())
    return _finish(L, st, "hs_moe_combine_bwd", bufs, check)


def dispatch_cases():
    """B in {1, 63, 64, 65, 129, 200} (the ballot loop walks 64 rows at a time), E in {1, 3, 16}"""
    return [{"B": B, "E": E, "seed": 900 + 10 * i + j, "tag": f"dispatch B={B} E={E}"}
            for i, B in enumerate((1, 63, 64, 65, 129, 200)) for j, E in enumerate((1, 3, 16))]


def dispatch_data(c):
    """gates [B][E]: expert 0 takes every row; for E >= 3 expert 1 takes none -- its column holds negative values, -0.0 and NaN,
    none of which is selected -- and expert 2 alternates; the others are random with zeros, and a few unselected entries
    anywhere are -0.0, negative or NaN."""
    g = gen(c["seed"])
    B, E = c["B"], c["E"]
    gt = torch.where(torch.rand(B, E, generator=g) < 0.5, torch.rand(B, E, generator=g) + 0.01, torch.tensor(0.0))
    gt[:, 0] = torch.rand(B, generator=g) + 0.01
    if E >= 3:
        gt[:, 1] = torch.tensor([-1.0, -0.0, float("nan")])[torch.arange(B) % 3]
        gt[:, 2] = (torch.arange(B) % 2).float() * 0.5
    if E >= 4:
        for j, v in enumerate((-0.0, -0.25, float("nan"))):
            gt[(7 * j + 3) % B, 3 + j % (E - 3)] = v
    return gt


def dispatch_ref(gates):
    """-> idx [E][B] int32 (the rows with gates[b][e] > 0 ascending, then sentinel), count [E] int32"""
    B, E = gates.shape
    idx = torch.full((E, B), int(SENT), dtype=I32)
    count = torch.zeros(E, dtype=I32)
    for e in range(E):
        rows = torch.nonzero(gates[:, e] > 0).reshape(-1).to(I32)
        idx[e, :rows.numel()] = rows
        count[e] = rows.numel()
    return idx, count


def call_dispatch(gates, check=True):
    L, lib, rt = _env()
    B, E = gates.shape
    gd = _fresh(gates)
    bufs = {"idx": _ibuf(E, B), "count": GBuf(1, E, I32, is_vec=True)}
    st = lib.hs_moe_dispatch_index(_p(gd), B, E, _p(bufs["idx"]), _p(bufs["count"]), rt.stream())
    return _finish(L, st, "hs_moe_dispatch_index", bufs, check)


def rows_cases():
    """D in {1, 63, 64, 65, 200}, n in {1, 5, B} with unique ascending idx; B = 9 and 70 (more rows than the four waves of a
    block, and n * D no multiple of 256)"""
    cases = []
    for i, D in enumerate((1, 63, 64, 65, 200)):
        for j, (B, n) in enumerate(((9, 1), (9, 5), (9, 9), (70, 5), (70, 70))):
            cases.append({"B": B, "n": n, "D": D, "E": 3, "seed": 1000 + 10 * i + j, "tag": f"rows B={B} n={n} D={D}"})
    return cases


def rows_data(c):
    """-> src_full [B][D] (gather source / scatter destination / dy), rows [n][D], idx [n] int32, gates [B][E]"""
    g = gen(c["seed"])
    B, n, D, E = c["B"], c["n"], c["D"], c["E"]
    idx = torch.sort(torch.randperm(B, generator=g)[:n]).values.to(I32)
    return torch.randn(B, D, generator=g), torch.randn(n, D, generator=g), idx, torch.rand(B, E, generator=g) + 0.1


def call_rows_gather(src, idx, n=None, check=True):
    L, lib, rt = _env()
    nn = idx.numel() if n is None else n
    D = src.shape[1]
    sd, idd = _fresh(src), _fresh(idx)
    bufs = {"dst": GBuf(max(idx.numel(), 1), D, F32)}
    st = lib.hs_rows_gather(_p(sd), _p(idd), _p(bufs["dst"]), nn, D, rt.stream())
    return _finish(L, st, "hs_rows_gather", bufs, check)


def call_rows_scatter_add(dst0, idx, scale, col, rows, n=None, check=True):
    """dst0 [B][D]: the destination before the call; scale [B][E] or None (ld_scale = E)"""
    L, lib, rt = _env()
    B, D = dst0.shape
    nn = idx.numel() if n is None else n
    idd, sc, rd = _fresh(idx), _fresh(scale), _fresh(rows)
    dst = GBuf(B, D, F32)
    dst.t.copy_(dst0.to(DEV))
    st = lib.hs_rows_scatter_add(_p(dst), _p(idd), _p(sc), scale.shape[1] if scale is not None else 0, col, _p(rd), nn, D, rt.stream())
    return _finish(L, st, "hs_rows_scatter_add", {"dst": dst}, check)


def call_rows_scatter_add_bwd(dy, idx, gates, col, rows, n=None, check=True):
    """-> dsrc [n][D], dgates [B][E] (sentinel where the call does not write)"""
    L, lib, rt = _env()
    B, E = gates.shape
    D = dy.shape[1]
    nn = idx.numel() if n is None else n
    dd, idd, gd, rd = _fresh(dy), _fresh(idx), _fresh(gates), _fresh(rows)
    bufs = {"dsrc": GBuf(max(idx.numel(), 1), D, F32), "dgates": GBuf(B, E, F32)}
    st = lib.hs_rows_scatter_add_bwd(_p(dd), _p(idd), _p(gd), E, col, _p(rd), _p(bufs["dsrc"]), _p(bufs["dgates"]), nn, D, rt.stream())
    return _finish(L, st, "hs_rows_scatter_add_bwd", bufs, check)


# ======================================================================================================================
# KAN weight pack / unpack
# ======================================================================================================================
KAN_SHAPES = ((1, 1, 1), (3, 5, 8), (17, 33, 11))


def kan_pack_data(out_f, in_f, nb, seed):
    """-> base_w [out][in], spline_w [out][in][nb], scaler [out][in], dwcat [out][in * (1 + nb)]"""
    g = gen(seed)
    return (torch.randn(out_f, in_f, generator=g), torch.randn(out_f, in_f, nb, generator=g), torch.randn(out_f, in_f, generator=g),
            torch.randn(out_f, in_f * (1 + nb), generator=g))


def kan_pack_ref32(base_w, spline_w, scaler):
    """wcat[o] = [base_w[o, :] | spline_w[o, i, :] * scaler[o, i] ...]: one float32 product (or a copy) per element"""
    out_f, in_f, nb = spline_w.shape
    sw = spline_w if scaler is None else spline_w * scaler[:, :, None]
    return torch.cat([base_w, sw.reshape(out_f, in_f * nb)], 1)


def kan_unpack_ref(dwcat, spline_w, scaler):
    """d_base = dwcat[:, :in]; d_spline = dwcat[:, in:] * scaler (one float32 product); d_scaler = sum_j dwcat * spline_w in
    float64, its float32 sequential yardstick, and the terms [nb][out*in] for sum_floor"""
    out_f, in_f, nb = spline_w.shape
    gs = dwcat[:, in_f:].reshape(out_f, in_f, nb)
    t = (gs.double() * spline_w.double()).permute(2, 0, 1).reshape(nb, -1)
    yard = torch.from_numpy(seq_sum32((gs * spline_w).numpy(), 2))
    return {"d_base": dwcat[:, :in_f].contiguous(), "d_spline": gs if scaler is None else gs * scaler[:, :, None],
            "d_scaler": t.sum(0).reshape(out_f, in_f), "d_scaler_yard": yard, "terms": t}


def call_kan_pack(base_w, spline_w, scaler, dims=None, check=True):
    L, lib, rt = _env()
    out_f, in_f, nb = spline_w.shape
    bd, sd, cd = _fresh(base_w), _fresh(spline_w), _fresh(scaler)
    bufs = {"wcat": GBuf(out_f, in_f * (1 + nb), F32)}
    a = (out_f, in_f, nb) if dims is None else dims
    st = lib.hs_kan_pack_weight(_p(bd), _p(sd), _p(cd), _p(bufs["wcat"]), a[0], a[1], a[2], rt.stream())
    return _finish(L, st, "hs_kan_pack_weight", bufs, check)


def call_kan_unpack(dwcat, spline_w, scaler, want=(True, True, True), dims=None, check=True):
    L, lib, rt = _env()
    out_f, in_f, nb = spline_w.shape
    dd, sd, cd = _fresh(dwcat), _fresh(spline_w), _fresh(scaler)
    bufs = {"d_base": GBuf(out_f, in_f, F32) if want[0] else None, "d_spline": GBuf(out_f, in_f * nb, F32) if want[1] else None,
            "d_scaler": GBuf(out_f, in_f, F32) if want[2] else None}
    a = (out_f, in_f, nb) if dims is None else dims
    st = lib.hs_kan_unpack_wgrad(_p(dd), _p(sd), _p(cd), _p(bufs["d_base"]), _p(bufs["d_spline"]), _p(bufs["d_scaler"]), a[0], a[1],
                                 a[2], rt.stream())
    return _finish(L, st, "hs_kan_unpack_wgrad", bufs, check)
