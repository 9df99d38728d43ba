"""Float64 references, float32 yardsticks and guarded ctypes callers for the optimizer, embedding, pooling, packing and small
elementwise kernels of csrc/elem.hip.

Same scheme as kernel_ref (whose gate, error measures, guard bands and data helpers are imported, not copied):
  *_ref64   the formula in float64 (numpy) on exactly the values the kernel reads: bf16 inputs are rounded first, then widened;
            float arguments of the C ABI are the float32 the call passes, except where stated (the optimizers' hyper-parameters
            are the Python doubles of the caller, as torch.optim uses them).
  *_yard    the same formula in float32 numpy, multiply and add rounded separately, every reduction strictly sequential
            (seq_sum32), the output rounded once to the kernel's output type.
  *_floor   where the judged quantity is a small difference of stored float32 values, the a-priori rounding bound of that
            store, from the data alone (derived in the docstring), for gate(floor=).
  call_*    ctypes callers: every output (and every array updated in place) inside a sentinel-filled guard band.
Pure data movement and selections (max pool, packing, casts, ReLU, the dropout mask) have one exact reference.

Importing this module needs no GPU; the callers load the library on first use.
"""
import ctypes as C

import numpy as np
import torch

from kernel_ref import (BIG, DEV, EPS32, SENT, GBuf, _env, _f32, _finish, _fresh, _np32, _out, _p,  # noqa: F401
                        bits_equal, gate, gen, maxrel, rel, seq_sum32)

F32 = torch.float32
BF16 = torch.bfloat16
DTYPES = (F32, BF16)
U = EPS32
ADAM_MAX = 32                # HS_ADAM_MAX: tensors per launch of the optimizer kernels
CAST_MAX = 48                # HS_CAST_MAX
U8_FILL = 0xA5               # guard fill of byte arrays


def dname(dt):
    return "bf16" if dt == BF16 else "f32"


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _np64(t):
    """the values a kernel reads from t (any float dtype), widened to float64"""
    return t.detach().cpu().double().numpy()


# ======================================================================================================================
# optimizers
# ======================================================================================================================
def adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, step, decoupled, grad_scale):
    """torch.optim.Adam (decoupled = 0: weight decay added to the gradient) / AdamW (decoupled = 1: p *= 1 - lr wd) on float64
    copies of the float32 state; the hyper-parameters are the Python doubles the caller passed.  -> p, m, v (float64 numpy)"""
    p, g, m, v = (_np64(t) for t in (p, g, m, v))
    g = g * grad_scale
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2s = np.sqrt(1.0 - b2 ** step)
    denom = np.sqrt(v) / bc2s + eps
    return {"p": p - (lr / bc1) * (m / denom), "m": m, "v": v}


def adam_yard(p, g, m, v, lr, b1, b2, eps, wd, step, decoupled, grad_scale):
    """the same with everything an np.float32, 1 - b1**step and sqrt(1 - b2**step) included: its error contains the float32
    rounding of beta1, beta2 and 1 - beta2 (relative 2^-24 / (1 - beta2) on the new term of exp_avg_sq), which the C ABI, taking
    floats, cannot avoid.  (1 - b2) * g * g is evaluated left to right, so a g whose square overflows does not."""
    f = np.float32
    p, g, m, v = (_np32(t) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gs, one = f(lr), f(b1), f(b2), f(eps), f(wd), f(grad_scale), f(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        g = g * gs
        if decoupled:
            p = p * (one - lr * wd)
        else:
            g = g + wd * p
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * g * g
        bc1 = one - np.power(b1, f(step), dtype=np.float32)
        bc2s = np.sqrt(one - np.power(b2, f(step), dtype=np.float32), dtype=np.float32)
        denom = np.sqrt(v, dtype=np.float32) / bc2s + eps
        p = p - (lr / bc1) * (m / denom)
    return {"p": p.astype(np.float32), "m": m.astype(np.float32), "v": v.astype(np.float32)}


def sgd_ref64(p, g, buf, lr, momentum, wd, nesterov, first, grad_scale):
    """torch.optim.SGD with dampening 0: g += wd p; buf = g if first else momentum buf + g; g = g + momentum buf if nesterov else
    buf; p -= lr g.  momentum == 0 (buf None): no buffer, nesterov has no effect.  -> p, buf (float64 numpy; buf None)"""
    p, g = _np64(p), _np64(g) * grad_scale
    if wd != 0:
        g = g + wd * p
    b = None
    if momentum != 0:
        b = g if first else momentum * _np64(buf) + g
        g = g + momentum * b if nesterov else b
    return {"p": p - lr * g, "buf": b}


def sgd_yard(p, g, buf, lr, momentum, wd, nesterov, first, grad_scale):
    f = np.float32
    lr, mo, wdf, gs = f(lr), f(momentum), f(wd), f(grad_scale)
    p, g = _np32(p), _np32(g) * gs
    if wd != 0:
        g = g + wdf * p
    b = None
    if momentum != 0:
        b = g if first else mo * _np32(buf) + g
        g = g + mo * b if nesterov else b
    return {"p": (p - lr * g).astype(np.float32), "buf": None if b is None else b.astype(np.float32)}


def update_floor(p_old, ref_p, roundings=3, chain=12):
    """Relative floor for the update p_new - p_old of an optimizer step, judged by max|err| / max|update|.  The kernel stores
    p_new, not the update: the store rounds by up to 2^-24 |p_new|, and so do the product p (1 - lr wd) of AdamW and the factor
    1 - lr wd itself (`roundings` = 3; 2 for SGD: the product lr g and the store; times the number of steps for a sequence).
    With |p| near 2 and updates near 1e-2 this is 1e-5 of the update: float32 holds the update of a stored parameter no better.
    The update's own chain (Adam: the scaled gradient, exp_avg, exp_avg_sq, the root, two quotients, eps, lr / bc1, the product)
    carries at most `chain` roundings relative to the update itself.
        floor = 2^-24 (roundings max(|p_old|, |p_new|) / max|p_new - p_old| + chain)"""
    p0, p1 = np.asarray(p_old, dtype=np.float64), np.asarray(ref_p, dtype=np.float64)
    top = np.abs(p1 - p0).max() if p0.size else 0.0
    if top == 0:
        return 0.0
    return float(U * (roundings * max(np.abs(p0).max(), np.abs(p1).max()) / top + chain))


class VBuf(GBuf):
    """n elements that start `off` elements into a 16-byte aligned array, inside a band of 1024 sentinel elements on either
    side; the `off` skipped elements belong to the band.  init: the values the call starts from (arrays updated in place)."""

    def __init__(self, n, dtype, off=0, init=None, fill=SENT):
        self.is_vec = True
        self.rows, self.ld, self.cols, self.fill = 1, n, n, fill
        self.n, self.off, self.g = n, off, 1024
        self.flat = torch.full((n + off + 2 * self.g,), fill, dtype=dtype, device=DEV)
        self.t = self.flat[self.g + off:self.g + off + n]
        self.ptr = self.flat.data_ptr() + (self.g + off) * self.flat.element_size()
        if init is not None and n:
            self.t.copy_(torch.as_tensor(init).to(dtype))
        self.init = None if init is None else self.get()

    def get(self):
        return self.t.cpu().clone()

    vec = get

    def intact(self):
        f = self.flat.cpu()
        lo = self.g + self.off
        return self._ok(f[:lo]) and self._ok(f[lo + self.n:])

    def untouched(self):
        if self.init is None:
            return self._ok(self.flat.cpu())
        return self.intact() and bits_equal(self.get(), self.init)


def _ptrs(bufs):
    return (C.c_void_p * max(len(bufs), 1))(*[(_p(b) if b is not None else None) for b in bufs])


def _counts(ns):
    return (C.c_int64 * max(len(ns), 1))(*[int(n) for n in ns])


def _collect(L, st, what, groups, check):
    """groups: {name: [VBuf or None, ...]} -> status, guards, untouched, and per name the list of CPU tensors"""
    torch.cuda.synchronize()
    allb = [b for bs in groups.values() for b in bs if b is not None]
    r = {"status": st, "guards": all(b.intact() for b in allb), "untouched": all(b.untouched() for b in allb)}
    for k, bs in groups.items():
        r[k] = [None if b is None else b.get() for b in bs]
    if check:
        L.check(st, what)
    return r


def call_adam(ts, lr, b1, b2, eps, wd, step, decoupled, grad_scale, shadow=True, count=None, check=True):
    """ts: list of {"p", "g", "m", "v": float32 CPU tensors, "off": 0 / 1 element offset of all four arrays, "h": None (NULL
    entry), 0 or 1 (element offset of the bf16 shadow)}.  shadow False: hs_adam_step_multi (no table)."""
    L, lib, rt = _env()
    G = {k: [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t[k]) for t in ts] for k in ("p", "m", "v")}
    gs = [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["g"]) for t in ts]
    G["h"] = [None if (t.get("h") is None or not shadow) else VBuf(t["p"].numel(), BF16, t["h"]) for t in ts]
    n = len(ts) if count is None else count
    cnt = _counts([t["p"].numel() for t in ts])
    if shadow:
        st = lib.hs_adam_step_multi_shadow(n, _ptrs(G["p"]), _ptrs(gs), _ptrs(G["m"]), _ptrs(G["v"]), _ptrs(G["h"]), cnt, lr, b1, b2,
                                           eps, wd, step, decoupled, grad_scale, rt.stream())
    else:
        st = lib.hs_adam_step_multi(n, _ptrs(G["p"]), _ptrs(gs), _ptrs(G["m"]), _ptrs(G["v"]), cnt, lr, b1, b2, eps, wd, step,
                                    decoupled, grad_scale, rt.stream())
    G["g"] = gs
    r = _collect(L, st, "hs_adam_step_multi", G, check)
    r["g_kept"] = all(b.untouched() for b in gs)
    return r


def call_sgd(ts, lr, momentum, wd, nesterov, first, grad_scale, null_buf=False, count=None, check=True):
    """ts: list of {"p", "g", "buf": float32 CPU tensors, "off"}; null_buf: pass NULL for the momentum table"""
    L, lib, rt = _env()
    G = {"p": [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["p"]) for t in ts],
         "buf": [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["buf"]) for t in ts]}
    gs = [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["g"]) for t in ts]
    n = len(ts) if count is None else count
    st = lib.hs_sgd_step_multi(n, _ptrs(G["p"]), _ptrs(gs), None if null_buf else _ptrs(G["buf"]),
                               _counts([t["p"].numel() for t in ts]), lr, momentum, wd, nesterov, first, grad_scale, rt.stream())
    G["g"] = gs
    r = _collect(L, st, "hs_sgd_step_multi", G, check)
    r["g_kept"] = all(b.untouched() for b in gs)
    r["buf_kept"] = all(b.untouched() for b in G["buf"])
    return r


# ======================================================================================================================
# dropout mask (csrc/hs_common.h: mix32, dropout_bits4, dropout_scale, dropout_thresh) in integer numpy
# ======================================================================================================================
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def dropout_thresh16(p):
    """the 16-bit threshold: uint32(float32(p) * 2^32) >> 16"""
    t = min(max(float(np.float32(p)) * 4294967296.0, 0.0), 4294967295.0)
    return int(t) >> 16


def dropout_keep_ref(seed, idx, p):
    """keep(seed, i) for every element index in idx (any shape) -> bool array.  Element i takes 16 bits of group q = i >> 2:
    x = lo32(q) * 0x9E3779B1 + lo32(seed) + hi32(q) * 0x85EBCA77; r0 = mix32(x ^ hi32(seed)); r1 = mix32(r0 + 0x6C8E9CF5 +
    hi32(seed)); elements 4q .. 4q+3 take lo16(r0), hi16(r0), lo16(r1), hi16(r1); kept iff bits16 >= thresh16(p)."""
    i = np.asarray(idx).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0, s1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    q = i >> np.uint64(2)
    x = ((q & _M32) * np.uint64(0x9E3779B1) + s0 + ((q >> np.uint64(32)) & _M32) * np.uint64(0x85EBCA77)) & _M32
    r0 = _mix32(x ^ s1)
    r1 = _mix32((r0 + np.uint64(0x6C8E9CF5) + s1) & _M32)
    w = np.where((i & np.uint64(2)) != 0, r1, r0)
    b = np.where((i & np.uint64(1)) != 0, w >> np.uint64(16), w & np.uint64(0xFFFF))
    return b >= np.uint64(dropout_thresh16(p))


def inv_keep32(p):
    """1.f / (1.f - p) as the host wrappers compute it"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_ref(x, p, seed):
    """hs_dropout: x * (keep ? float32(1 / (1 - p)) : 0), one float32 product rounded to the dtype of x"""
    keep = dropout_keep_ref(seed, np.arange(x.numel()), p)
    sc = np.where(keep, inv_keep32(p), np.float32(0.0)).astype(np.float32)
    return _out(_np32(x) * sc, x.dtype), torch.from_numpy(keep)


# ======================================================================================================================
# BERT embeddings
# ======================================================================================================================
def _clamp_ids(ids, V):
    return np.clip(ids.cpu().numpy().astype(np.int64), 0, V - 1)


def _embed_sum64(ids, word, pos, type0, L, dtype):
    """the pre-LayerNorm sum, rounded ONCE to dtype (float64 -> dtype), as [tokens][H] torch tensor of that dtype"""
    V = word.shape[0]
    idc = _clamp_ids(ids, V)
    l = np.arange(idc.shape[0]) % L
    s = _np64(word)[idc] + _np64(pos)[l] + _np64(type0)[None, :]
    return _t64(s).to(dtype)


def _embed_scale(tokens, H, p, seed, f):
    if not p > 0:
        return None
    keep = dropout_keep_ref(seed, np.arange(tokens * H).reshape(tokens, H), p)
    return np.where(keep, f(inv_keep32(p)), f(0.0))


def embed_fwd_ref64(ids, word, pos, type0, gamma, beta, L, eps, dtype, p=0.0, seed=0):
    """sum = word[clamp(id, 0, V-1)] + pos[t % L] + type0, rounded to dtype; LayerNorm over H of the rounded sum (biased variance,
    eps the float32 of the call); dropout with element index t * H + h.  -> sum (dtype), y, mean, rstd (float64), keep"""
    s = _embed_sum64(ids, word, pos, type0, L, dtype)
    v = _np64(s)
    T, H = v.shape
    mean = v.sum(1) / H
    d = v - mean[:, None]
    var = (d * d).sum(1) / H
    rstd = 1.0 / np.sqrt(var + _f32(eps))
    y = d * rstd[:, None] * _np64(gamma) + _np64(beta)
    sc = _embed_scale(T, H, p, seed, np.float64)
    return {"sum": s, "y": _t64(y if sc is None else y * sc), "mean": _t64(mean), "rstd": _t64(rstd),
            "keep": None if sc is None else torch.from_numpy(sc != 0)}


def embed_fwd_yard(ids, word, pos, type0, gamma, beta, L, eps, dtype, p=0.0, seed=0):
    f = np.float32
    V = word.shape[0]
    idc = _clamp_ids(ids, V)
    l = np.arange(idc.shape[0]) % L
    s = (_np32(word)[idc] + _np32(pos)[l]) + _np32(type0)[None, :]
    s = _out(s, dtype)
    v = _np32(s)
    T, H = v.shape
    mean = seq_sum32(v, 1) / f(H)
    d = v - mean[:, None]
    var = seq_sum32(d * d, 1) / f(H)
    rstd = f(1.0) / np.sqrt(var + f(eps), dtype=np.float32)
    y = d * rstd[:, None] * _np32(gamma) + _np32(beta)
    sc = _embed_scale(T, H, p, seed, np.float32)
    return {"sum": s, "y": _out(y if sc is None else y * sc, dtype), "mean": _out(mean, F32), "rstd": _out(rstd, F32)}


def embed_bwd_ref64(ids, dsum, B, L, V, pad_id):
    """dword[id] = sum of dsum[t] over the tokens t with clamp(ids[t]) == id, in token order, none for id == pad_id (rows of ids
    that do not occur stay 0); dpos[l] = sum_b dsum[b * L + l].  -> dword [V][H], dpos [L][H] (float64)"""
    d = _np64(dsum)
    H = d.shape[1]
    idc = _clamp_ids(ids, V)
    dword = np.zeros((V, H))
    live = idc != pad_id
    np.add.at(dword, idc[live], d[live])
    return {"dword": _t64(dword), "dpos": _t64(d.reshape(B, L, H).sum(0))}


def embed_bwd_yard(ids, dsum, B, L, V, pad_id):
    """float32, each table row summed sequentially in token order, each position sequentially over b"""
    d = _np32(dsum)
    H = d.shape[1]
    idc = _clamp_ids(ids, V)
    dword = np.zeros((V, H), dtype=np.float32)
    for i in np.unique(idc):
        if i != pad_id:
            dword[i] = seq_sum32(d[idc == i], 0)
    return {"dword": _out(dword, F32), "dpos": _out(seq_sum32(d.reshape(B, L, H), 0), F32)}


def call_embed_fwd(ids, word, pos, type0, gamma, beta, L, eps, dtype, p=0.0, seed=0, null=None, args=None, check=True):
    """null: name of one argument passed as NULL; args: {"tokens" / "L" / "H" / "V": value passed instead of the real one}"""
    Lb, lib, rt = _env()
    tokens, (V, H) = ids.numel(), word.shape
    a = {"tokens": tokens, "L": L, "H": H, "V": V}
    a.update(args or {})
    d = {"ids": _fresh(ids), "word": _fresh(word), "pos": _fresh(pos), "type0": _fresh(type0), "gamma": _fresh(gamma),
         "beta": _fresh(beta)}
    bufs = {"sum": GBuf(max(tokens, 1), H, dtype), "y": GBuf(max(tokens, 1), H, dtype),
            "mean": GBuf(1, max(tokens, 1), F32, is_vec=True), "rstd": GBuf(1, max(tokens, 1), F32, is_vec=True)}
    ptr = {k: _p(v) for k, v in list(d.items()) + list(bufs.items())}
    if null is not None:
        ptr[null] = None
    st = lib.hs_bert_embed_fwd(rt.hs_dtype(dtype), ptr["ids"], ptr["word"], ptr["pos"], ptr["type0"], ptr["gamma"], ptr["beta"],
                               ptr["sum"], ptr["y"], ptr["mean"], ptr["rstd"], a["tokens"], a["L"], a["H"], a["V"], eps, p, seed,
                               rt.stream())
    return _finish(Lb, st, "hs_bert_embed_fwd", bufs, check)


def call_embed_bwd(ids, dsum, B, L, V, pad_id, want_dword=True, want_dpos=True, zero=True, args=None, check=True):
    """dword is zero-filled before the call as the contract asks (zero=False: left at the sentinel, for refused calls)"""
    Lb, lib, rt = _env()
    H = dsum.shape[1]
    a = {"B": B, "L": L, "H": H, "V": V}
    a.update(args or {})
    idd, dd = _fresh(ids), _fresh(dsum)
    bufs = {"dword": GBuf(V, H, F32) if want_dword else None, "dpos": GBuf(max(L, 1), H, F32) if want_dpos else None}
    if want_dword and zero:
        bufs["dword"].t.zero_()
    st = lib.hs_bert_embed_bwd(rt.hs_dtype(dsum.dtype), _p(idd), _p(dd), _p(bufs["dword"]), _p(bufs["dpos"]), a["B"], a["L"], a["H"],
                               a["V"], pad_id, rt.stream())
    return _finish(Lb, st, "hs_bert_embed_bwd", bufs, check)


# ======================================================================================================================
# max pool (NHWC)
# ======================================================================================================================
def pool_out(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def maxpool_ref(x, k, s, p):
    """x [N][H][W][C] (any float dtype, no NaN).  -> y (dtype of x), idx (uint8: the tap r * k + s of the first maximum in
    (r, s) scan order; taps outside the image never win), and bwd(dy) -> dx: every pixel collects dy of the windows whose
    arg-max it is (float64 sums, returned in the dtype of dy)."""
    xv = _np64(x)
    N, H, W, Cc = xv.shape
    P, Q = pool_out(H, k, s, p), pool_out(W, k, s, p)
    best = np.full((N, P, Q, Cc), -np.inf)
    bi = np.zeros((N, P, Q, Cc), dtype=np.uint8)
    taps = []
    for r in range(k):
        hh = np.arange(P) * s - p + r
        pv = np.nonzero((hh >= 0) & (hh < H))[0]
        for c in range(k):
            ww = np.arange(Q) * s - p + c
            qv = np.nonzero((ww >= 0) & (ww < W))[0]
            taps.append((r * k + c, pv, hh[pv], qv, ww[qv]))
            if pv.size == 0 or qv.size == 0:
                continue
            f = xv[:, hh[pv]][:, :, ww[qv]]
            sub = best[np.ix_(np.arange(N), pv, qv)]
            win = f > sub
            best[np.ix_(np.arange(N), pv, qv)] = np.where(win, f, sub)
            bsub = bi[np.ix_(np.arange(N), pv, qv)]
            bi[np.ix_(np.arange(N), pv, qv)] = np.where(win, np.uint8(r * k + c), bsub)

    def bwd(dy):
        g = _np64(dy).reshape(N, P, Q, Cc)
        dx = np.zeros((N, H, W, Cc))
        for tap, pv, hv, qv, wv in taps:
            if pv.size == 0 or qv.size == 0:
                continue
            ix = np.ix_(np.arange(N), pv, qv)
            dx[np.ix_(np.arange(N), hv, wv)] += np.where(bi[ix] == tap, g[ix], 0.0)
        return _t64(dx).to(dy.dtype)

    return _t64(best).to(x.dtype), torch.from_numpy(bi), bwd


def call_maxpool_fwd(x, k, s, p, out_rows=None, args=None, null=None, check=True):
    """x [N][H][W][C].  out_rows: rows to allocate for y / idx when the arguments are about to be refused"""
    L, lib, rt = _env()
    N, H, W, Cc = x.shape
    a = {"N": N, "H": H, "W": W, "C": Cc}
    a.update(args or {})
    rows = out_rows if out_rows is not None else N * pool_out(H, k, s, p) * pool_out(W, k, s, p)
    xd = _fresh(x)
    bufs = {"y": GBuf(rows, Cc, x.dtype), "idx": GBuf(rows, Cc, torch.uint8, fill=U8_FILL)}
    ptr = {"x": _p(xd), "y": _p(bufs["y"]), "idx": _p(bufs["idx"])}
    if null:
        ptr[null] = None
    st = lib.hs_maxpool_fwd(rt.hs_dtype(x.dtype), ptr["x"], ptr["y"], ptr["idx"], a["N"], a["H"], a["W"], a["C"], k, s, p, rt.stream())
    return _finish(L, st, "hs_maxpool_fwd", bufs, check)


def call_maxpool_bwd(dy, idx, N, H, W, Cc, k, s, p, args=None, check=True):
    """dy, idx [rows][C]"""
    L, lib, rt = _env()
    a = {"N": N, "H": H, "W": W, "C": Cc}
    a.update(args or {})
    gd, idd = _fresh(dy), _fresh(idx)
    bufs = {"dx": GBuf(N * H * W, Cc, dy.dtype)}
    st = lib.hs_maxpool_bwd(rt.hs_dtype(dy.dtype), _p(gd), _p(idd), _p(bufs["dx"]), a["N"], a["H"], a["W"], a["C"], k, s, p, rt.stream())
    return _finish(L, st, "hs_maxpool_bwd", bufs, check)


# ======================================================================================================================
# mean over tokens
# ======================================================================================================================
def mean_tokens_ref64(x, dy):
    """x [B][Nt][H], dy [B][H] -> y = mean_t x, dx[b][t] = dy[b] / Nt (float64)"""
    Nt = x.shape[1]
    return {"y": _t64(_np64(x).sum(1) / Nt), "dx": _t64(np.repeat((_np64(dy) / Nt)[:, None, :], Nt, 1))}


def mean_tokens_yard(x, dy, y_dtype, dx_dtype):
    """the sequential float32 sum times float32(1 / Nt); dx = dy * float32(1 / Nt): one product, rounded once"""
    Nt = x.shape[1]
    sc = np.float32(1.0) / np.float32(Nt)
    return {"y": _out(seq_sum32(_np32(x), 1) * sc, y_dtype), "dx": _out(np.repeat((_np32(dy) * sc)[:, None, :], Nt, 1), dx_dtype)}


def call_mean_tokens_fwd(x, out_f32, args=None, check=True):
    L, lib, rt = _env()
    B, Nt, H = x.shape
    a = {"B": B, "Nt": Nt, "H": H}
    a.update(args or {})
    xd = _fresh(x)
    bufs = {"y": GBuf(max(B, 1), H, F32 if out_f32 else x.dtype)}
    st = lib.hs_mean_tokens_fwd(rt.hs_dtype(x.dtype), _p(xd), _p(bufs["y"]), a["B"], a["Nt"], a["H"], out_f32, rt.stream())
    return _finish(L, st, "hs_mean_tokens_fwd", bufs, check)


def call_mean_tokens_bwd(dy, dtype, Nt, dy_f32, args=None, check=True):
    """dy [B][H]: float32 when dy_f32 = 1 (or dtype is float32), else in dtype"""
    L, lib, rt = _env()
    B, H = dy.shape
    a = {"B": B, "Nt": Nt, "H": H}
    a.update(args or {})
    gd = _fresh(dy)
    bufs = {"dx": GBuf(max(B * Nt, 1), H, dtype)}
    st = lib.hs_mean_tokens_bwd(rt.hs_dtype(dtype), _p(gd), _p(bufs["dx"]), a["B"], a["Nt"], a["H"],
                                dy_f32, rt.stream())
    return _finish(L, st, "hs_mean_tokens_bwd", bufs, check)


# ======================================================================================================================
# packing and casts (pure data movement plus one rounding)
# ======================================================================================================================
def pack_image_ref(x, Hp, Wp, pad, dtype):
    """x [N][Cin][H][W] f32 -> [N][Hp][Wp][4] of dtype: pixel (h, w) at (h + pad, w + pad), borders and channels >= Cin zero"""
    N, Cin, H, W = x.shape
    y = torch.zeros(N, Hp, Wp, 4)
    y[:, pad:pad + H, pad:pad + W, :Cin] = x.permute(0, 2, 3, 1)
    return y.to(dtype)


def pack_stem_weight_ref(w, dtype):
    """w [K][R][S][Cin] f32 -> [K][R][8][4] of dtype, zero padded"""
    K, R, S, Cin = w.shape
    o = torch.zeros(K, R, 8, 4)
    o[:, :, :S, :Cin] = w
    return o.to(dtype)


def unpack_stem_wgrad_ref(g, S, Cin):
    """g [K][R][8][4] f32 -> [K][R][S][Cin]"""
    return g[:, :, :S, :Cin].contiguous()


def cast_ref(x):
    return x.bfloat16()


def call_pack_image(x, Hp, Wp, pad, dtype, Cin_arg=None, check=True):
    L, lib, rt = _env()
    N, Cin, H, W = x.shape
    xd = _fresh(x)
    bufs = {"y": GBuf(N * Hp, Wp * 4, dtype)}
    st = lib.hs_pack_image(rt.hs_dtype(dtype), _p(xd), _p(bufs["y"]), N, Cin if Cin_arg is None else Cin_arg, H, W, Hp, Wp, pad,
                           rt.stream())
    r = _finish(L, st, "hs_pack_image", bufs, check)
    r["y"] = r["y"].view(N, Hp, Wp, 4)
    return r


def call_pack_stem_weight(w, dtype, check=True):
    L, lib, rt = _env()
    K, R, S, Cin = w.shape
    wd = _fresh(w)
    bufs = {"out": GBuf(K * R, 32, dtype)}
    st = lib.hs_pack_stem_weight(rt.hs_dtype(dtype), _p(wd), _p(bufs["out"]), K, R, S, Cin, rt.stream())
    r = _finish(L, st, "hs_pack_stem_weight", bufs, check)
    r["out"] = r["out"].view(K, R, 8, 4)
    return r


def call_unpack_stem_wgrad(g, S, Cin, check=True):
    L, lib, rt = _env()
    K, R = g.shape[:2]
    gd = _fresh(g)
    bufs = {"dw": GBuf(K * R, S * Cin, F32)}
    st = lib.hs_unpack_stem_wgrad(_p(gd), _p(bufs["dw"]), K, R, S, Cin, rt.stream())
    r = _finish(L, st, "hs_unpack_stem_wgrad", bufs, check)
    r["dw"] = r["dw"].view(K, R, S, Cin)
    return r


def _src(x, off):
    """device copy of the flat tensor x that starts `off` elements into a 16-byte aligned allocation -> keepalive, address"""
    flat = torch.full((x.numel() + off + 8,), BIG, dtype=x.dtype)
    flat[off:off + x.numel()] = x.reshape(-1)
    flat = flat.to(DEV)
    return flat, flat.data_ptr() + off * flat.element_size()


def call_cast_multi(srcs, offs=None, check=True):
    """srcs: float32 CPU vectors; offs[i]: element offset of source i inside its allocation"""
    L, lib, rt = _env()
    offs = offs or [0] * len(srcs)
    keep = [_src(x, o) for x, o in zip(srcs, offs)]
    G = {"dst": [VBuf(x.numel(), BF16) for x in srcs]}
    n = len(srcs)
    src = (C.c_void_p * max(n, 1))(*[k[1] for k in keep])
    st = lib.hs_cast_f32_to_bf16_multi(n, src, _ptrs(G["dst"]), _counts([x.numel() for x in srcs]), rt.stream())
    return _collect(L, st, "hs_cast_f32_to_bf16_multi", G, check)


# ======================================================================================================================
# small elementwise kernels
# ======================================================================================================================
def axpby_ref64(x, y, a, b):
    """a x + b y on the float32 a, b of the call (y None: a x)"""
    v = _f32(a) * _np64(x)
    return _t64(v if y is None else v + _f32(b) * _np64(y))


def axpby_yard(x, y, a, b, out_dtype):
    v = np.float32(a) * _np32(x)
    return _out(v if y is None else v + np.float32(b) * _np32(y), out_dtype)


def relu_ref(x):
    """max(x, 0) as the kernel defines it: x where x > 0, else +0.0 (also for -0.0; NaN is left out of the data)"""
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_bwd_ref(dy, y):
    """dy where y > 0, else +0.0"""
    return torch.where(y > 0, dy, torch.zeros_like(dy))


SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


def gelu_bwd_ref64(dy, u):
    """dy * (Phi(u) + u phi(u)), Phi = 0.5 (1 + erf(u / sqrt 2)), phi the normal density"""
    g, uu = _t64(_np64(dy)), _t64(_np64(u))
    return g * (0.5 * (1.0 + torch.erf(uu * SQRT1_2)) + uu * INV_SQRT_2PI * torch.exp(-0.5 * uu * uu))


def gelu_bwd_yard(dy, u, out_dtype):
    """erf evaluated in float64 and rounded to float32 (a correctly rounded erff), then the formula in float32"""
    f = np.float32
    g, uu = _np32(dy), _np32(u)
    er = torch.erf(_t64(uu.astype(np.float64) * SQRT1_2)).numpy().astype(np.float32)
    with np.errstate(under="ignore"):
        d = f(0.5) * (f(1.0) + er) + uu * f(INV_SQRT_2PI) * np.exp(f(-0.5) * uu * uu, dtype=np.float32)
    return _out(g * d, out_dtype)


def call_map(name, dtype, ins, n=None, off=0, out_dtype=None, extra=(), null=(), check=True):
    """One of the elementwise entry points `name(dtype.., ins.., out, n, extra.., stream)`.  ins: flat CPU tensors (None = NULL),
    every input and the output start `off` elements into their allocations.  -> out (n elements, guarded)"""
    L, lib, rt = _env()
    n = ins[0].numel() if n is None else n
    keep = [None if x is None else _src(x, off) for x in ins]
    out = VBuf(ins[0].numel(), out_dtype or dtype, off)
    ptrs = [None if (k is None or i in null) else k[1] for i, k in enumerate(keep)]
    po = None if "out" in null else _p(out)
    s = rt.stream()
    hd = rt.hs_dtype(dtype)
    if name == "hs_axpby":
        st = lib.hs_axpby(hd, rt.hs_dtype(out_dtype or dtype), ptrs[0], ptrs[1], po, n, extra[0], extra[1], s)
    elif name == "hs_dropout":
        st = lib.hs_dropout(hd, ptrs[0], po, n, extra[0], extra[1], s)
    elif name == "hs_relu_fwd":
        st = lib.hs_relu_fwd(hd, ptrs[0], po, n, s)
    elif name == "hs_relu_bwd":
        st = lib.hs_relu_bwd(hd, ptrs[0], ptrs[1], po, n, s)
    elif name == "hs_gelu_bwd":
        st = lib.hs_gelu_bwd(hd, ptrs[0], ptrs[1], po, n, s)
    elif name == "hs_mul_dev_scalar":
        st = lib.hs_mul_dev_scalar(ptrs[0], ptrs[1], po, n, s)
    else:
        raise ValueError(name)
    r = _collect(L, st, name, {"out": [out]}, check)
    r["out"] = r["out"][0]
    return r
