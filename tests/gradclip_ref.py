"""Float64 yardstick, float32 forms and guarded ctypes callers for global gradient-norm clipping (csrc/gradclip.hip and the
_clip entry points of csrc/elem.hip).

Same scheme as kernel_ref / elem_ref (whose gate, guard bands and optimizer references are imported, not copied):
  norm64          the global 2-norm of a list of gradients in float64 (numpy), on the float32 values the kernel reads
  coef            min(max_norm / (norm + 1e-6), 1) with a NaN kept: in float32 (every operand and operation an np.float32: the
                  arithmetic the finish kernel states, fminf(max_norm / (rec[0] + 1e-6f), 1.0f)), or in float64 (what
                  torch.nn.utils.clip_grad_norm_ computes on float64 gradients)
  record          the four floats the finish kernel writes: [float32(norm64), coef32 of that float32, finite, skip]
  adam_clip_* /   the clipped step: elem_ref.adam_ref64 / sgd_ref64 with the gradient pre-multiplied by the coefficient (float64), and
  sgd_clip_*      the sequential-float32 form for kernel_ref.gate with the kernel's order (g * grad_scale) * coefficient
  call_*          ctypes callers: every output (and every array updated in place) inside a sentinel-filled guard band.

Importing this module needs no GPU; the callers load the library on first use.
"""
import ctypes as C

import numpy as np
import torch

import elem_ref as er
from elem_ref import F32, VBuf, _collect, _counts, _ptrs
from kernel_ref import SENT, _env, _np32, _p, bits_equal  # noqa: F401

F64 = torch.float64
GRADCLIP_MAX = 128           # HS_GRADCLIP_MAX: tensors per call of the sum-of-squares and scale kernels
NORM_TOL = 2.0 ** -23        # see test_gradclip_gpu.py: one float32 rounding of the root of a float64 sum


# ======================================================================================================================
# the yardstick
# ======================================================================================================================
def norm64(grads):
    """sqrt(sum_i sum_j g_i[j]^2) in float64 over a list of tensors (any float dtype; the values as stored, widened)"""
    total = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for g in grads:
            v = g.detach().cpu().double().numpy().reshape(-1)
            total = total + float(np.dot(v, v)) if v.size else total
        return float(np.sqrt(total))


def coef(norm, max_norm, dtype=np.float32):
    """min(max_norm / (norm + 1e-6), 1), NaN kept, every operand and operation in `dtype`"""
    f = dtype
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = f(max_norm) / (f(norm) + f(1e-6))
    return c if not c > f(1.0) else f(1.0)


def record(grads, max_norm, skip_nonfinite=False):
    """[norm rounded once to float32, float32 coefficient of that rounded norm, finite, skip] as np.float32[4]"""
    with np.errstate(over="ignore"):
        n32 = np.float32(norm64(grads))
    finite = bool(np.isfinite(n32))
    return np.array([n32, coef(n32, max_norm), 1.0 if finite else 0.0, 1.0 if (skip_nonfinite and not finite) else 0.0],
                    dtype=np.float32)


def _pre64(g, c):
    return torch.from_numpy(g.detach().cpu().double().numpy() * float(c))


def adam_clip_ref64(p, g, m, v, lr, b1, b2, eps, wd, step, decoupled, grad_scale, c):
    """elem_ref.adam_ref64 on the gradient pre-multiplied by the coefficient c (float64 product, never rounded)"""
    return er.adam_ref64(p, _pre64(g, c), m, v, lr, b1, b2, eps, wd, step, decoupled, grad_scale)


def adam_clip_yard(p, g, m, v, lr, b1, b2, eps, wd, step, decoupled, grad_scale, c):
    """sequential float32 in the kernel's order: (g * grad_scale) rounded, then * c rounded, then elem_ref.adam_yard's step"""
    g1 = torch.from_numpy(_np32(g) * np.float32(grad_scale))
    return er.adam_yard(p, g1, m, v, lr, b1, b2, eps, wd, step, decoupled, float(np.float32(c)))


def sgd_clip_ref64(p, g, buf, lr, momentum, wd, nesterov, first, grad_scale, c):
    return er.sgd_ref64(p, _pre64(g, c), buf, lr, momentum, wd, nesterov, first, grad_scale)


def sgd_clip_yard(p, g, buf, lr, momentum, wd, nesterov, first, grad_scale, c):
    g1 = torch.from_numpy(_np32(g) * np.float32(grad_scale))
    return er.sgd_yard(p, g1, buf, lr, momentum, wd, nesterov, first, float(np.float32(c)))


# ======================================================================================================================
# guarded callers
# ======================================================================================================================
def rec_tensor(values):
    """a device record holding the four given floats (inside a guard band) -> VBuf"""
    return VBuf(4, F32, init=torch.tensor([float(x) for x in values], dtype=torch.float32))


def n_partials(ns, count=None):
    """hs_grad_norm_partials for the sizes ns"""
    _, lib, _ = _env()
    return int(lib.hs_grad_norm_partials(len(ns) if count is None else count, _counts(ns)))


def call_norm(gs, max_norm, skip=0, offs=None, check=True):
    """gs: float32 CPU vectors; offs[i]: element offset of gradient i inside its 16-byte aligned allocation.  The gradients are
    split into calls of at most GRADCLIP_MAX tensors whose partials are laid end to end, then one finish launch.
    -> status, guards, rec [4], partials [slots] (float64), g_kept (no gradient was written)"""
    L, lib, rt = _env()
    offs = offs or [0] * len(gs)
    G = [VBuf(g.numel(), F32, o, init=g) for g, o in zip(gs, offs)]
    calls = [(b, min(GRADCLIP_MAX, len(gs) - b)) for b in range(0, len(gs), GRADCLIP_MAX)]
    slots = [n_partials([g.numel() for g in gs[b:b + c]]) for b, c in calls]
    assert all(s >= 1 for s in slots)
    part, rec = VBuf(sum(slots), F64), VBuf(4, F32)
    st, at = 0, 0
    for (b, c), s in zip(calls, slots):
        st = st or lib.hs_grad_sumsq_multi(c, _ptrs(G[b:b + c]), _counts([g.numel() for g in gs[b:b + c]]), part.ptr + 8 * at, rt.stream())
        at += s
    st = st or lib.hs_grad_norm_finish(part.ptr, sum(slots), max_norm, skip, rec.ptr, rt.stream())
    r = _collect(L, st, "hs_grad_sumsq_multi / hs_grad_norm_finish", {"rec": [rec], "partials": [part], "g": G}, check)
    r["rec"], r["partials"] = r["rec"][0], r["partials"][0]
    r["g_kept"] = all(b.untouched() for b in G)
    return r


def call_sumsq(gs, count=None, null=None, n_arg=None, slots=64, check=True):
    """one hs_grad_sumsq_multi call with arguments about to be refused.  null: "grads" / "n" / "partials" / ("entry", i)"""
    L, lib, rt = _env()
    G = [VBuf(g.numel(), F32, init=g) for g in gs]
    part = VBuf(slots, F64)
    ptrs = _ptrs(G)
    if isinstance(null, tuple):
        ptrs[null[1]] = None
    ns = _counts([g.numel() for g in gs] if n_arg is None else n_arg)
    st = lib.hs_grad_sumsq_multi(len(gs) if count is None else count, None if null == "grads" else ptrs, None if null == "n" else ns,
                                 None if null == "partials" else part.ptr, rt.stream())
    return _collect(L, st, "hs_grad_sumsq_multi", {"partials": [part], "g": G}, check)


def call_finish(partials, n, max_norm, skip=0, null=None, check=True):
    """hs_grad_norm_finish over the given float64 CPU vector.  null: "partials" / "rec" """
    L, lib, rt = _env()
    part = VBuf(partials.numel(), F64, init=partials)
    rec = VBuf(4, F32)
    st = lib.hs_grad_norm_finish(None if null == "partials" else part.ptr, n, max_norm, skip, None if null == "rec" else rec.ptr,
                                 rt.stream())
    r = _collect(L, st, "hs_grad_norm_finish", {"rec": [rec], "partials": [part]}, check)
    r["rec"] = r["rec"][0]
    return r


def call_scale(gs, rec_values, offs=None, count=None, null=None, n_arg=None, check=True):
    """hs_grad_scale_multi in place on guarded copies of gs.  -> g: the list of results"""
    L, lib, rt = _env()
    offs = offs or [0] * len(gs)
    G = [VBuf(g.numel(), F32, o, init=g) for g, o in zip(gs, offs)]
    rec = rec_tensor(rec_values)
    ns = _counts([g.numel() for g in gs] if n_arg is None else n_arg)
    st = lib.hs_grad_scale_multi(len(gs) if count is None else count, None if null == "grads" else _ptrs(G),
                                 None if null == "n" else ns, None if null == "rec" else rec.ptr, rt.stream())
    r = _collect(L, st, "hs_grad_scale_multi", {"g": G, "rec": [rec]}, check)
    r["rec_kept"] = rec.untouched()
    return r


def call_adam_clip(ts, lr, b1, b2, eps, wd, step, decoupled, grad_scale, rec_values, count=None, null=None, check=True):
    """elem_ref.call_adam for hs_adam_step_multi_clip; rec_values: the four floats of the record.  null: "rec" or a table name"""
    L, lib, rt = _env()
    G = {k: [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t[k]) for t in ts] for k in ("p", "m", "v")}
    gs = [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["g"]) for t in ts]
    G["h"] = [None if t.get("h") is None else VBuf(t["p"].numel(), er.BF16, t["h"]) for t in ts]
    rec = rec_tensor(rec_values)
    n = len(ts) if count is None else count
    tab = {"p": _ptrs(G["p"]), "g": _ptrs(gs), "m": _ptrs(G["m"]), "v": _ptrs(G["v"]), "n": _counts([t["p"].numel() for t in ts])}
    if null in tab:
        tab[null] = None
    st = lib.hs_adam_step_multi_clip(n, tab["p"], tab["g"], tab["m"], tab["v"], _ptrs(G["h"]), tab["n"], lr, b1, b2, eps, wd, step,
                                     decoupled, grad_scale, None if null == "rec" else rec.ptr, rt.stream())
    G["g"] = gs
    r = _collect(L, st, "hs_adam_step_multi_clip", G, check)
    r["g_kept"] = all(b.untouched() for b in gs) and rec.untouched()
    return r


def call_sgd_clip(ts, lr, momentum, wd, nesterov, first, grad_scale, rec_values, null_buf=False, count=None, null=None, check=True):
    L, lib, rt = _env()
    G = {"p": [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["p"]) for t in ts],
         "buf": [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["buf"]) for t in ts]}
    gs = [VBuf(t["p"].numel(), F32, t.get("off", 0), init=t["g"]) for t in ts]
    rec = rec_tensor(rec_values)
    n = len(ts) if count is None else count
    tab = {"p": _ptrs(G["p"]), "g": _ptrs(gs), "n": _counts([t["p"].numel() for t in ts])}
    if null in tab:
        tab[null] = None
    st = lib.hs_sgd_step_multi_clip(n, tab["p"], tab["g"], None if null_buf else _ptrs(G["buf"]), tab["n"], lr, momentum, wd, nesterov,
                                    first, grad_scale, None if null == "rec" else rec.ptr, rt.stream())
    G["g"] = gs
    r = _collect(L, st, "hs_sgd_step_multi_clip", G, check)
    r["g_kept"] = all(b.untouched() for b in gs) and rec.untouched()
    r["buf_kept"] = all(b.untouched() for b in G["buf"])
    return r
