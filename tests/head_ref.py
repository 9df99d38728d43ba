"""Float64 references, float32 yardsticks, a-priori floors and guarded ctypes callers for the loss kernels (cross entropy,
focal, softmax entropy, row KL, MP-Loss, SupCon, KAN regularisation), the LSTM / GRU cells and the KAN features.

Same scheme as kernel_ref (whose gate, error measures, guard bands and helpers are imported, not copied):
  *_ref64   the formula in float64 (torch, double) on exactly the float32 values the kernel reads.  Forward formulas are
            written out here; gradients of the losses come from autograd on that float64 forward, so a clamp passes its
            gradient at both bounds, as torch.clamp does.  Additive constants (1e-8, 1e-12, eps) are the float32 values
            widened; clamp and indicator decisions are taken in float64 on the float32 inputs.
  *_yard    the same formula in float32 on the CPU with every reduction strictly sequential (seq_sum32).  __expf(x) is
            modelled as the HIP headers define it, exp2(fl32(0x1.715476p+0f * x)) in float32, so its argument-rounding
            error (|x| 2^-24 relative) is part of the yardstick; __logf is the library logf (np.log in float32).
  *_floors  where a float32 evaluation cancels, the a-priori rounding bound of that evaluation relative to the largest
            reference value, from the inputs and the float64 reference alone (derived in each docstring), for gate(floor=).
  call_*    ctypes callers: every output inside a GBuf guard band, pitched inputs padded with BIG.

Importing this module needs no GPU.
"""
import numpy as np
import torch

from kernel_ref import (BIG, DEV, EPS32, F32_NOISE, SENT, GBuf, _env, _f32, _finish, _fresh, _np32, _out, _p,  # noqa: F401
                        _pitched, _wsbuf, bits_equal, gate, gen, maxrel, rel, seq_sum32)

F64 = torch.float64
F32 = torch.float32
LOG2E32 = np.float32(float.fromhex("0x1.715476p+0"))
E8 = _f32(1e-8)              # the kernels' 1e-8f, widened
E12 = _f32(1e-12)
U = EPS32


def expf32(x):
    """__expf in float32: exp2(fl32(log2(e) * x))"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(LOG2E32 * np.asarray(x, dtype=np.float32)).astype(np.float32)


def _one(v):
    return torch.as_tensor(v, dtype=F64).reshape(1)


def _s32(v):
    return _out(np.asarray(v, dtype=np.float32).reshape(1), F32)


def _relmax(bound, ref):
    """largest bound relative to the largest reference value; 0 (= the plain 1e-6 of the gate) where that is undefined"""
    top = ref.double().abs().max().item()
    v = (bound.max().item() / top) if top > 0 else 0.0
    return v if np.isfinite(v) else 0.0


def _onehot(y, Cn, dtype=F64):
    return torch.nn.functional.one_hot(y, Cn).to(dtype)


def _softmax_parts64(z):
    """-> mx [B], p [B][C], lse [B] in float64"""
    z = z.double()
    mx = z.max(1).values
    e = (z - mx[:, None]).exp()
    s = e.sum(1)
    return mx, e / s[:, None], mx + s.log()


def _softmax_parts32(z):
    """-> mx, e = __expf(z - mx), s (sequential) in float32"""
    mx = z.max(1)
    e = expf32(z - mx[:, None])
    return mx, e, seq_sum32(e, 1)


def lse_err(z, y, depth):
    """A-priori bound of the float32 error of lse - z[y] with lse = fl(mx + logf(s)), s = sum_c __expf(z_c - mx) over `depth`
    roundings.  Each summand carries 2u of exp2 and the argument rounding |z_c - mx| u, so rel(s) <= u (depth + 2 + sum_c
    p_c |z_c - mx|); logf adds u |log s| + u, the sum mx + log s one rounding u |lse|, the difference u |lse - z_y|:
        |err| <= u (|lse| + |lse - mx| + depth + 3 + sum_c p_c |z_c - mx| + |lse - z_y|).
    For a confidently correct row lse - z_y is tiny and |lse| is not: this is the cancellation.  -> err [B], err_lse [B]"""
    zd = z.double()
    mx, p, lse = _softmax_parts64(zd)
    arg = (p * (zd - mx[:, None]).abs()).sum(1)
    e_lse = U * (lse.abs() + (lse - mx).abs() + depth + 3.0 + arg)
    zy = zd[torch.arange(zd.shape[0]), y]
    return e_lse + U * (lse - zy).abs(), e_lse


def prob_relerr(z, depth):
    """relative float32 error bound of softmax probabilities: exp2 2u, its argument rounding |z_c - mx| u, the sum's `depth`
    roundings and the argument roundings of its terms (at most max |z - mx| u, weighted: sum_k p_k |z_k - mx| u), one
    division -> [B][C]"""
    zd = z.double()
    mx, p, _ = _softmax_parts64(zd)
    d = (zd - mx[:, None]).abs()
    return U * (depth + 5.0 + d + (p * d).sum(1, keepdim=True))


# --------------------------------------------------------------------------------------------------------------------
# cross entropy
# --------------------------------------------------------------------------------------------------------------------
def ce_ref64(z, y, weight, s):
    """mean-reduced CrossEntropyLoss(weight, label_smoothing = s) -> loss [1], row_loss [B], dlogits [B][C]"""
    zd = z.double().clone().requires_grad_(True)
    B, Cn = zd.shape
    w = torch.ones(Cn, dtype=F64) if weight is None else weight.double()
    sd = _f32(s)
    mx = zd.max(1).values.detach()
    lse = mx + (zd - mx[:, None]).exp().sum(1).log()
    wy = w[y]
    row = (1.0 - sd) * wy * (lse - zd[torch.arange(B), y]) + sd / Cn * (w[None, :] * (lse[:, None] - zd)).sum(1)
    loss = row.sum() / wy.sum()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "row_loss": row.detach(), "dlogits": zd.grad}


def ce_yard(z, y, weight, s):
    z = _np32(z)
    B, Cn = z.shape
    yy = y.numpy()
    ar = np.arange(B)
    w = np.ones(Cn, dtype=np.float32) if weight is None else _np32(weight)
    s, one, cf = np.float32(s), np.float32(1.0), np.float32(Cn)
    mx, e, se = _softmax_parts32(z)
    lse = mx + np.log(se)
    wy = w[yy]
    sm = seq_sum32(w[None, :] * (lse[:, None] - z), 1)
    row = (one - s) * wy * (lse - z[ar, yy]) + s / cf * sm
    td = seq_sum32(wy, 0)
    loss = seq_sum32(row, 0) / td
    p = e * (one / se)[:, None]
    oh = np.zeros_like(z)
    oh[ar, yy] = one
    g = (one - s) * wy[:, None] * (p - oh) + s / cf * (seq_sum32(w, 0) * p - w[None, :])
    return {"loss": _s32(loss), "row_loss": _out(row, F32), "dlogits": _out(g / td, F32)}


def ce_floors(z, y, weight, s, ref):
    """row_loss = (1 - s) w_y (lse - z_y) + s / C sum_c w_c (lse - z_c): with E_y, E_lse of lse_err (a lane's chain of
    ceil(C / 64) additions and six butterfly steps: depth Dc = ceil(C / 64) + 6),
        |err row| <= (1 - s) w_y (E_y + 3u |lse - z_y|) + s / C (sum_c w_c (E_lse + u |lse - z_c|) + (Dc + 3) u sum_c w_c |lse - z_c|)
                     + u |row|.
    loss = sum_r row / sum_r w_y: the rows of a wave are added in sequence (at most ceil(B / 4)), then up to 16 wave partials:
    DB = ceil(B / 4) + 18 roundings on sum |row|, and as many on the denominator.  -> relative floors of row_loss and loss"""
    zd = z.double()
    B, Cn = zd.shape
    w = torch.ones(Cn, dtype=F64) if weight is None else weight.double()
    sd = _f32(s)
    Dc = -(-Cn // 64) + 6
    Ey, El = lse_err(z, y, Dc)
    _, _, lse = _softmax_parts64(zd)
    d = (lse[:, None] - zd).abs()
    wy = w[y]
    dy = d[torch.arange(B), y]
    row = ref["row_loss"].double()
    rb = ((1.0 - sd) * wy * (Ey + 3.0 * U * dy) + sd / Cn * ((w[None, :] * (El[:, None] + U * d)).sum(1)
                                                          + (Dc + 3.0) * U * (w[None, :] * d).sum(1)) + U * row.abs())
    DB = -(-B // 4) + 18
    lb = (rb.sum() + DB * U * row.abs().sum()) / wy.sum() + DB * U * ref["loss"].abs().sum()
    return {"row_loss": _relmax(rb, row), "loss": _relmax(lb, ref["loss"])}


# --------------------------------------------------------------------------------------------------------------------
# focal loss
# --------------------------------------------------------------------------------------------------------------------
def _focal_terms64(ce, gamma):
    """(1 - exp(-ce))^gamma * ce and d/d ce of it, elementwise in float64 with the limits torch's pow takes:
    x^0 = 1 and its derivative 0, also at x = 0"""
    pt = torch.exp(-ce)
    om = 1.0 - pt
    pw = om ** gamma
    if gamma == 0.0:
        return pw * ce, pw
    return pw * ce, pw + gamma * om ** (gamma - 1.0) * pt * ce


def focal_ref64(z, y, weight, gamma):
    """FocalLoss(gamma, weight), mean reduction -> loss [1], dlogits [B][C]"""
    zd = z.double().clone().requires_grad_(True)
    B, Cn = zd.shape
    w = torch.ones(Cn, dtype=F64) if weight is None else weight.double()
    mx = zd.max(1).values.detach()
    lse = mx + (zd - mx[:, None]).exp().sum(1).log()
    ce = w[y] * (lse - zd[torch.arange(B), y])
    loss = (((1.0 - torch.exp(-ce)) ** _f32(gamma)) * ce).mean()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "dlogits": zd.grad}


def focal_yard(z, y, weight, gamma):
    z = _np32(z)
    B, Cn = z.shape
    yy = y.numpy()
    ar = np.arange(B)
    w = np.ones(Cn, dtype=np.float32) if weight is None else _np32(weight)
    g, one, bf = np.float32(gamma), np.float32(1.0), np.float32(B)
    mx, e, se = _softmax_parts32(z)
    wy = w[yy]
    ce = wy * (mx + np.log(se) - z[ar, yy])
    pt = expf32(-ce)
    om = one - pt
    with np.errstate(all="ignore"):
        pw = np.power(om, g)
        second = np.zeros_like(ce) if gamma == 0.0 else g * np.power(om, g - one) * pt * ce
    loss = seq_sum32(pw * ce, 0) / bf
    dce = (pw + second) / bf
    oh = np.zeros_like(z)
    oh[ar, yy] = one
    dz = (dce * wy)[:, None] * (e / se[:, None] - oh)
    return {"loss": _s32(loss), "dlogits": _out(dz, F32)}


def focal_floors(z, y, weight, gamma, ref):
    """ce = w_y (lse - z_y) carries E = w_y E_y + u |ce| (lse_err, a thread's chain over C classes: depth C).  The loss term
    h(ce) = (1 - exp(-ce))^gamma ce and the factor h'(ce) of the gradient are smooth in ce, and E is small against the scale
    on which they turn, so the change over [ce - E, ce + E] (cut at 0) is taken at the end points:
        dh = max |h(ce +- E) - h(ce)|,  dh' likewise,
    plus 1 - exp(-ce) itself: exp2 and the subtraction give 3u absolute on (1 - pt), i.e. gamma (1 - pt)^(gamma - 1) 3u on the
    power (bounded here by the same end-point change with E >= 3u), and 6u on the products.
        |err loss| <= mean_r (dh_r + 6u |h_r|) + DB u mean_r |h_r|,  DB = ceil(B / 256) + 12 (chain, wave, four partials)
        |err dz_rc| <= (dh'_r + 8u |h'_r|) w_y |p_c - 1[c = y]| / B + h'_r w_y relp_c p_c / B + 4u |dz_rc|   (relp: prob_relerr)
    -> relative floors of loss and dlogits"""
    zd = z.double()
    B, Cn = zd.shape
    w = torch.ones(Cn, dtype=F64) if weight is None else weight.double()
    g = _f32(gamma)
    Ey, _ = lse_err(z, y, Cn)
    _, p, lse = _softmax_parts64(zd)
    wy = w[y]
    ce = wy * (lse - zd[torch.arange(B), y])
    E = wy * Ey + U * ce.abs() + 3.0 * U
    h, hd = _focal_terms64(ce, g)
    hp, hdp = _focal_terms64(ce + E, g)
    hm, hdm = _focal_terms64((ce - E).clamp_min(0.0), g)
    dh = torch.maximum((hp - h).abs(), (hm - h).abs())
    dhd = torch.maximum((hdp - hd).abs(), (hdm - hd).abs())
    DB = -(-B // 256) + 12
    lb = (dh + 6.0 * U * h.abs()).mean() + DB * U * h.abs().mean()
    pm = (p - _onehot(y, Cn)).abs()
    relp = prob_relerr(z, Cn)
    db = (((dhd + 8.0 * U * hd.abs()) * wy)[:, None] * pm + (hd.abs() * wy)[:, None] * relp * p) / B + 4.0 * U * ref["dlogits"].abs()
    return {"loss": _relmax(lb, ref["loss"]), "dlogits": _relmax(db, ref["dlogits"])}


# --------------------------------------------------------------------------------------------------------------------
# softmax entropy
# --------------------------------------------------------------------------------------------------------------------
def entropy_ref64(z, g=None):
    """ent[r] = -sum_c p log(p + 1e-8f), p = softmax(z[r]); with g [rows]: dlogits of sum_r g[r] ent[r]"""
    zd = z.double().clone().requires_grad_(True)
    p = torch.softmax(zd, 1)
    ent = -(p * torch.log(p + E8)).sum(1)
    o = {"ent": ent.detach()}
    if g is not None:
        (g.double() * ent).sum().backward()
        o["dlogits"] = zd.grad
    return o


def entropy_yard(z, g=None):
    z = _np32(z)
    one, e8 = np.float32(1.0), np.float32(1e-8)
    mx, e, se = _softmax_parts32(z)
    p = e * (one / se)[:, None]
    lp = np.log(p + e8)
    ent = -seq_sum32(p * lp, 1)
    o = {"ent": _out(ent, F32)}
    if g is not None:
        t = -(lp + p / (p + e8))
        pt = seq_sum32(p * t, 1)
        o["dlogits"] = _out(_np32(g)[:, None] * p * (t - pt[:, None]), F32)
    return o


def entropy_floors(z, g, ref):
    """With relp the relative error of p (prob_relerr, depth Dc = ceil(C / 64) + 6): log(p + 1e-8) carries relp + 2u
    absolute, so a term p log(p + 1e-8) carries p (relp (|lp| + 1) + 2u + u |lp|), and the sum Dc u sum p |lp|:
        |err ent| <= sum_c p (relp (|lp| + 1) + 2u + u |lp|) + Dc u sum_c p |lp|.
    dz = g p (t - sum_k p_k t_k), t = -(lp + p / (p + 1e-8)), err t <= 2 relp + u (|t| + 2): where one class holds the mass,
    t of that class and the sum cancel (as in kernel_ref.softmax_bwd_floor):
        |err dz_c| <= |g| p_c ((Dc + 3) u (|t_c| + sum_k p_k |t_k|) + err t_c + sum_k p_k (err t_k + relp_k |t_k|)) + relp_c |dz_c|.
    -> relative floors of ent and dlogits"""
    zd = z.double()
    Cn = zd.shape[1]
    Dc = -(-Cn // 64) + 6
    relp = prob_relerr(z, Dc)
    _, p, _ = _softmax_parts64(zd)
    lp = torch.log(p + E8)
    eb = (p * (relp * (lp.abs() + 1.0) + 2.0 * U + U * lp.abs())).sum(1) + Dc * U * (p * lp.abs()).sum(1)
    o = {"ent": _relmax(eb, ref["ent"])}
    if g is not None:
        t = -(lp + p / (p + E8))
        et = 2.0 * relp + U * (t.abs() + 2.0)
        db = (g.double().abs()[:, None] * p * ((Dc + 3.0) * U * (t.abs() + (p * t.abs()).sum(1, keepdim=True)) + et
                                               + (p * (et + relp * t.abs())).sum(1, keepdim=True)) + relp * ref["dlogits"].abs())
        o["dlogits"] = _relmax(db, ref["dlogits"])
    return o


# --------------------------------------------------------------------------------------------------------------------
# row KL on clamped probabilities
# --------------------------------------------------------------------------------------------------------------------
def kl_rows_ref64(p, q, eps, w=None):
    """out[r] = sum_c pc (log pc - log qc), pc = clamp(p, eps, 1); with w [rows]: dp, dq of sum_r w[r] out[r]
    (torch.clamp passes the gradient at both bounds)"""
    pd, qd = p.double().clone().requires_grad_(True), q.double().clone().requires_grad_(True)
    ed = _f32(eps)
    pc, qc = pd.clamp(ed, 1.0), qd.clamp(ed, 1.0)
    out = (pc * (pc.log() - qc.log())).sum(1)
    o = {"out": out.detach()}
    if w is not None:
        (w.double() * out).sum().backward()
        o["dp"], o["dq"] = pd.grad, qd.grad
    return o


def kl_rows_yard(p, q, eps, w=None):
    p, q = _np32(p), _np32(q)
    e, one = np.float32(eps), np.float32(1.0)
    pc, qc = np.minimum(np.maximum(p, e), one), np.minimum(np.maximum(q, e), one)
    lp, lq = np.log(pc), np.log(qc)
    o = {"out": _out(seq_sum32(pc * (lp - lq), 1), F32)}
    if w is not None:
        wr = _np32(w)[:, None]
        o["dp"] = _out(np.where((p >= e) & (p <= one), wr * (lp - lq + one), np.float32(0.0)), F32)
        o["dq"] = _out(np.where((q >= e) & (q <= one), -wr * pc / qc, np.float32(0.0)), F32)
    return o


def kl_rows_floors(p, q, eps, w, ref):
    """lp - lq with p close to q cancels: logf carries u |log| + u each, the difference u |lp - lq|, so
        e_c = u (|lp| + |lq| + 2 + |lp - lq|),
        |err out| <= sum_c pc (e_c + u |lp - lq|) + Dc u sum_c pc |lp - lq|   (Dc = ceil(cols / 64) + 6),
        |err dp_c| <= |w| (e_c + 2u |lp - lq + 1|).
    -> relative floors of out and dp"""
    ed = _f32(eps)
    pc, qc = p.double().clamp(ed, 1.0), q.double().clamp(ed, 1.0)
    lp, lq = pc.log(), qc.log()
    Dc = -(-p.shape[1] // 64) + 6
    e = U * (lp.abs() + lq.abs() + 2.0 + (lp - lq).abs())
    ob = (pc * (e + U * (lp - lq).abs())).sum(1) + Dc * U * (pc * (lp - lq).abs()).sum(1)
    o = {"out": _relmax(ob, ref["out"])}
    if w is not None:
        o["dp"] = _relmax(w.double().abs()[:, None] * (e + 2.0 * U * (lp - lq + 1.0).abs()), ref["dp"])
    return o


# --------------------------------------------------------------------------------------------------------------------
# MP-Loss
# --------------------------------------------------------------------------------------------------------------------
C03, C06, C11 = _f32(0.3), _f32(0.6), _f32(1.1)


def _sym_kl64(pi, pt):
    p, q = pi.clamp(E8, 1.0), pt.clamp(E8, 1.0)
    return (0.5 * (p - q) * (p.log() - q.log())).sum(1)


def mp_raw_kl64(zi, zt):
    """the raw symmetric KL per row in float64 (before nan_to_num and the clamp to [0, 10])"""
    return _sym_kl64(torch.softmax(zi.double(), 1), torch.softmax(zt.double(), 1))


def mp_ref64(zi, zt, zf, y):
    """0.3 CE(img) + 0.6 CE(txt) + 1.1 mean_b(exp(clamp(symKL_b, 0, 10))) CE(fused) -> loss [1], d_image, d_text, d_fused"""
    a, t, f = (v.double().clone().requires_grad_(True) for v in (zi, zt, zf))
    B = a.shape[0]
    ar = torch.arange(B)

    def ce(v):
        return (torch.logsumexp(v, 1) - v[ar, y]).mean()

    kl = _sym_kl64(torch.softmax(a, 1), torch.softmax(t, 1))
    kl = torch.nan_to_num(kl, nan=0.0, posinf=10.0, neginf=0.0).clamp(0.0, 10.0)
    loss = C03 * ce(a) + C06 * ce(t) + C11 * torch.exp(kl).mean() * ce(f)
    loss.backward()
    return {"loss": loss.detach().reshape(1), "d_image": a.grad, "d_text": t.grad, "d_fused": f.grad}


def mp_yard(zi, zt, zf, y):
    a, t, f = _np32(zi), _np32(zt), _np32(zf)
    B, Cn = a.shape
    yy = y.numpy()
    ar = np.arange(B)
    one, half, e8, zero = np.float32(1.0), np.float32(0.5), np.float32(1e-8), np.float32(0.0)
    invB = one / np.float32(B)
    c03, c06, c11 = np.float32(0.3), np.float32(0.6), np.float32(1.1)
    pr, ce = [], []
    for v in (a, t, f):
        mx, e, s = _softmax_parts32(v)
        ce.append(seq_sum32(mx + np.log(s) - v[ar, yy], 0) * invB)
        pr.append(e / s[:, None])
    pa, qa, fa = pr
    p, q = np.minimum(np.maximum(pa, e8), one), np.minimum(np.maximum(qa, e8), one)
    lp, lq = np.log(p), np.log(q)
    kl = seq_sum32(half * (p - q) * (lp - lq), 1)
    klc = np.minimum(np.maximum(np.where(kl == kl, kl, zero), zero), np.float32(10.0))
    wgt = expf32(klc)
    wmean = seq_sum32(wgt, 0) * invB
    loss = c03 * ce[0] + c06 * ce[1] + c11 * wmean * ce[2]
    live = (kl == kl) & (kl >= zero) & (kl <= np.float32(10.0))
    gk = np.where(live, c11 * ce[2] * wgt * invB, zero)[:, None]
    gp = np.where((pa >= e8) & (pa <= one), half * (lp - lq + one - q / p), zero)
    gq = np.where((qa >= e8) & (qa <= one), half * (lq - lp + one - p / q), zero)
    dot_p, dot_q = seq_sum32(pa * gp, 1)[:, None], seq_sum32(qa * gq, 1)[:, None]
    oh = np.zeros_like(a)
    oh[ar, yy] = one
    return {"loss": _s32(loss),
            "d_image": _out(c03 * (pa - oh) * invB + gk * pa * (gp - dot_p), F32),
            "d_text": _out(c06 * (qa - oh) * invB + gk * qa * (gq - dot_q), F32),
            "d_fused": _out(c11 * wmean * (fa - oh) * invB, F32)}


def mp_floors(zi, zt, zf, y, ref):
    """The three CE means carry lse_err per row (a thread's chain over C: depth C).  The symmetric KL
    sum_c (p - q)(lp - lq) / 2 carries, with relp / relq of prob_relerr and e_l = u (|lp| + |lq| + 2) + relp + relq on lp - lq,
        e_kl = sum_c (|lp - lq| (relp p + relq q) + |p - q| e_l) / 2 + (C + 2) u |kl|,
    and exp(kl) the relative error e_kl + u (kl + 2) while the outer clamp is not active (else u (10 + 2)).  With
    DB = ceil(B / 256) + 12 roundings in each batch reduction:
        |err loss| <= 0.3 mean E_i + 0.6 mean E_t + 1.1 (wmean mean E_f + ce_f mean e_w) + (DB + 4) u (0.3 ce_i + 0.6 ce_t + 1.1 wmean ce_f).
    Gradients: gp = (lp - lq + 1 - q / p) / 2 vanishes at p = q, its roundings do not:
        e_gp = (e_l + 2u + (relp + relq + u) q / p) / 2   (0 where the inner clamp is active),
        |err d_image| <= 0.3 / B (relp p + u |p - 1[y]|) + gk p (e_gp + sum_k p_k (e_gp_k + relp_k |gp_k|) + (C + 3) u (|gp| + sum_k p_k |gp_k|))
                         + (rel_gk + relp) gk p |gp - sum_k p_k gp_k|,      rel_gk = e_w / w + mean E_f / ce_f + (DB + 4) u,
        d_text alike with p and q exchanged, and
        |err d_fused| <= 1.1 / B (wmean (relf f + u |f - 1[y]|) + |f - 1[y]| (mean e_w + (DB + 2) u wmean)).
    -> relative floors of loss, d_image, d_text, d_fused"""
    a, t, f = zi.double(), zt.double(), zf.double()
    B, Cn = a.shape
    Ei, Et, Ef = (lse_err(v, y, Cn)[0] for v in (zi, zt, zf))
    ar = torch.arange(B)
    pa, qa, fa = torch.softmax(a, 1), torch.softmax(t, 1), torch.softmax(f, 1)
    ce_i, ce_t, ce_f = ((torch.logsumexp(v, 1) - v[ar, y]).mean() for v in (a, t, f))
    relp, relq, relf = prob_relerr(zi, Cn), prob_relerr(zt, Cn), prob_relerr(zf, Cn)
    p, q = pa.clamp(E8, 1.0), qa.clamp(E8, 1.0)
    lp, lq = p.log(), q.log()
    kl = (0.5 * (p - q) * (lp - lq)).sum(1)
    e_l = U * (lp.abs() + lq.abs() + 2.0) + relp + relq
    e_kl = 0.5 * ((lp - lq).abs() * (relp * p + relq * q) + (p - q).abs() * e_l).sum(1) + (Cn + 2.0) * U * kl.abs()
    live = (kl >= 0.0) & (kl <= 10.0)
    klc = kl.clamp(0.0, 10.0)
    wgt = klc.exp()
    e_w = wgt * torch.where(live, e_kl + U * (klc + 2.0), torch.full_like(kl, 12.0 * U))
    wmean = wgt.mean()
    DB = -(-B // 256) + 12
    lb = (C03 * Ei.mean() + C06 * Et.mean() + C11 * (wmean * Ef.mean() + ce_f * e_w.mean())
          + (DB + 4.0) * U * (C03 * ce_i + C06 * ce_t + C11 * wmean * ce_f))
    oh = _onehot(y, Cn)
    gk = torch.where(live, C11 * ce_f * wgt / B, torch.zeros_like(kl))[:, None]
    rel_gk = (e_w / wgt + Ef.mean() / ce_f.clamp_min(1e-300) + (DB + 4.0) * U)[:, None]

    def side(pr, pc, qc, l1, l2, r1, r2, c0):
        on = (pr >= E8) & (pr <= 1.0)
        gp = torch.where(on, 0.5 * (l1 - l2 + 1.0 - qc / pc), torch.zeros_like(pr))
        e_gp = torch.where(on, 0.5 * (e_l + 2.0 * U + (r1 + r2 + U) * qc / pc), torch.zeros_like(pr))
        dot = (pr * gp).sum(1, keepdim=True)
        return (c0 / B * (r1 * pr + U * (pr - oh).abs())
                + gk * pr * (e_gp + (pr * (e_gp + r1 * gp.abs())).sum(1, keepdim=True)
                             + (Cn + 3.0) * U * (gp.abs() + (pr * gp.abs()).sum(1, keepdim=True)))
                + (rel_gk + r1) * gk * pr * (gp - dot).abs())

    db_i = side(pa, p, q, lp, lq, relp, relq, C03)
    db_t = side(qa, q, p, lq, lp, relq, relp, C06)
    db_f = C11 / B * (wmean * (relf * fa + U * (fa - oh).abs()) + (fa - oh).abs() * (e_w.mean() + (DB + 2.0) * U * wmean))
    return {"loss": _relmax(lb, ref["loss"]), "d_image": _relmax(db_i, ref["d_image"]), "d_text": _relmax(db_t, ref["d_text"]),
            "d_fused": _relmax(db_f, ref["d_fused"])}


# --------------------------------------------------------------------------------------------------------------------
# SupCon
# --------------------------------------------------------------------------------------------------------------------
def supcon_ref64(feat, labels, T):
    """SupConLoss(temperature) on (B, D) features, mean over anchors -> loss [1], dfeat [B][D]"""
    fd = feat.double().clone().requires_grad_(True)
    B = fd.shape[0]
    Td = _f32(T)
    fn = fd / fd.norm(dim=1, keepdim=True).clamp_min(E12)
    sim = fn @ fn.T / Td
    sim = sim - sim.max(1, keepdim=True).values.detach()
    off = ~torch.eye(B, dtype=torch.bool)
    pos = (off & (labels[:, None] == labels[None, :])).double()
    logp = sim - torch.log((sim.exp() * off.double()).sum(1, keepdim=True) + E8)
    loss = -((pos * logp).sum(1) / (pos.sum(1) + E8)).mean()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "dfeat": fd.grad}


def supcon_yard(feat, labels, T):
    f = _np32(feat)
    B, D = f.shape
    lab = labels.numpy()
    one, e8, zero, bf, Tf = np.float32(1.0), np.float32(1e-8), np.float32(0.0), np.float32(B), np.float32(T)
    nrm = np.maximum(np.sqrt(seq_sum32(f * f, 1)), np.float32(1e-12))
    fn = f / nrm[:, None]
    sim = seq_sum32(fn[:, None, :] * fn[None, :, :], 2) / Tf
    mx = sim.max(1)
    off = ~np.eye(B, dtype=bool)
    ex = np.where(off, expf32(sim - mx[:, None]), zero)
    Ei = seq_sum32(np.concatenate([np.full((B, 1), e8, dtype=np.float32), ex], 1), 1)
    lE = np.log(Ei)
    pos = off & (lab[:, None] == lab[None, :])
    P = pos.sum(1).astype(np.float32)
    msum = seq_sum32(np.where(pos, sim - mx[:, None] - lE[:, None], zero), 1)
    loss = seq_sum32(-msum / (P + e8) / bf, 0)
    w = one / (bf * (P + e8))
    q = ex / Ei[:, None]
    G = np.where(off, -w[:, None] * (pos.astype(np.float32) - P[:, None] * q), zero)
    S = G + G.T
    g = seq_sum32(S[:, :, None] * fn[None, :, :], 1) / Tf
    dot = seq_sum32(g * fn, 1)
    return {"loss": _s32(loss), "dfeat": _out((g - dot[:, None] * fn) / nrm[:, None], F32)}


def supcon_floors(feat, labels, T, ref):
    """s_ij = fn_i . fn_j / T: a normalised feature carries (Dd + 3) u relative (Dd = ceil(D / 64) + 6 roundings of the norm
    and of the dot), so |err s_ij| <= Es = (3 Dd + 8) u / T for |fn_i . fn_j| <= 1.  With near-duplicate rows s_ij - max_j s_ij
    cancels to far below 1 / T while Es does not shrink.  E_i = 1e-8 + sum_j exp(s_ij - mx) is a chain of B additions whose
    terms move by 2 Es relative, so log E_i carries (B + 4) u + 2 Es + u |log E_i|, and a positive's term s_ij - mx - log E_i
        e_term = 4 Es + (B + 4) u + u |log E_i| + 2u |term|;   |err loss| <= mean_i (e_term_i + (P_i + 3) u max_j |term_ij|).
    Gradient: q_ij = exp(s_ij - mx) / E_i has the relative error Eq = 4 Es + (B + 6) u, so
        |err G_ij| <= w_i P_i q_ij Eq + 3u |G_ij|,
        e_i = ((errG + errG^T) |fn| + (B + Dd + 6) u |G + G^T| |fn|) / T                 (the error of d loss / d fn_i, per column)
        |err dfeat_id| <= (e_id + |fn_id| sum_k e_ik |fn_ik| + (Dd + 4) u (|g_id| + |fn_id| sum_k |g_ik fn_ik|)) / |f_i|,
    g = d loss / d fn.  -> relative floors of loss and dfeat, and "dfeat_abs": the largest absolute bound (for D = 1, where
    the projection leaves exactly 0)"""
    fd = feat.double()
    B, D = fd.shape
    Td = _f32(T)
    Dd = -(-D // 64) + 6
    Es = (3.0 * Dd + 8.0) * U / Td
    nrm = fd.norm(dim=1, keepdim=True).clamp_min(E12)
    fn = fd / nrm
    sim = fn @ fn.T / Td
    sim = sim - sim.max(1, keepdim=True).values
    off = ~torch.eye(B, dtype=torch.bool)
    offd = off.double()
    pos = (off & (labels[:, None] == labels[None, :])).double()
    P = pos.sum(1)
    Ei = (sim.exp() * offd).sum(1) + E8
    lE = Ei.log()
    term = (sim - lE[:, None]) * pos
    e_term = 4.0 * Es + (B + 4.0) * U + U * lE.abs()
    rows = torch.where(P > 0, e_term + (P + 5.0) * U * term.abs().max(1).values, torch.zeros_like(P))
    lb = rows.mean()
    Eq = 4.0 * Es + (B + 6.0) * U
    w = 1.0 / (B * (P + E8))
    q = sim.exp() * offd / Ei[:, None]
    G = -w[:, None] * (pos - P[:, None] * q) * offd
    eG = (w * P)[:, None] * q * Eq + 3.0 * U * G.abs()
    A = fn.abs()
    S = G + G.T
    e = ((eG + eG.T) @ A + (B + Dd + 6.0) * U * (S.abs() @ A)) / Td
    g = S @ fn / Td
    db = (e + A * (e * A).sum(1, keepdim=True) + (Dd + 4.0) * U * (g.abs() + A * (g * fn).abs().sum(1, keepdim=True))) / nrm
    return {"loss": _relmax(lb, ref["loss"]), "dfeat": _relmax(db, ref["dfeat"]), "dfeat_abs": db.max().item()}


# --------------------------------------------------------------------------------------------------------------------
# KAN regularisation
# --------------------------------------------------------------------------------------------------------------------
def kan_reg_ref64(w, ra, re):
    """l_j = mean_c |w[j][c]|, A = sum l, p = l / A: loss = ra A - re sum p log p -> loss [1], dw [rows][coeffs]"""
    wd = w.double().clone().requires_grad_(True)
    l = wd.abs().mean(1)
    A = l.sum()
    p = l / A
    loss = _f32(ra) * A - _f32(re) * (p * p.log()).sum()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "dw": wd.grad}


def kan_reg_yard(w, ra, re):
    w = _np32(w)
    ra, re = np.float32(ra), np.float32(re)
    invc = np.float32(1.0) / np.float32(w.shape[1])
    l = seq_sum32(np.abs(w), 1) * invc
    A = seq_sum32(l, 0)
    S = seq_sum32(l * np.log(l), 0)
    E = np.log(A) - S / A
    dl = ra - re * (np.log(l / A) + E) / A
    return {"loss": _s32(ra * A + re * E), "dw": _out(np.sign(w) * (dl * invc)[:, None], F32)}


def kan_reg_floors(w, ra, re, ref):
    """E = log A - S / A, S = sum_j l_j log l_j: for a single row, or rows of nearly one size, the entropy is far below log A
    and the two terms cancel.  With rel_l = (C + 1) u of a row mean over C coefficients, DB = ceil(rows / 256) + 11 roundings
    of a batch reduction (chain, wave, four partials), relA = rel_l + DB u, and logf good to 2u relative:
        |err E| <= 2u |log A| + relA + (sum_j |l_j log l_j| / A) (4u + rel_l + DB u + relA) + u |E|,
        |err loss| <= |ra| A (relA + u) + |re| err E + u |loss|.
    Gradient: d loss / d l = ra - re (log(l / A) + E) / A, where log(l / A) + E cancels in the same way:
        |err dl| <= |re| (2u |log(l / A)| + rel_l + relA + u + err E) / A + (relA + 2u) |dl - ra| + u |dl|,   dw = +-dl / C.
    -> relative floors of loss and dw"""
    wd = w.double()
    rows, Cn = wd.shape
    rad, red = abs(_f32(ra)), abs(_f32(re))
    l = wd.abs().mean(1)
    A = l.sum()
    p = l / A
    E = -(p * p.log()).sum()
    rel_l = (Cn + 1.0) * U
    DB = -(-rows // 256) + 11
    relA = rel_l + DB * U
    eE = 2.0 * U * A.log().abs() + relA + ((l * l.log()).abs().sum() / A) * (4.0 * U + rel_l + DB * U + relA) + U * E.abs()
    lb = rad * A * (relA + U) + red * eE + U * ref["loss"].abs().sum()
    dl = _f32(ra) - _f32(re) * (p.log() + E) / A
    edl = red * (2.0 * U * p.log().abs() + rel_l + relA + U + eE) / A + (relA + 2.0 * U) * (dl - _f32(ra)).abs() + U * dl.abs()
    return {"loss": _relmax(lb, ref["loss"]), "dw": _relmax(edl / Cn, ref["dw"])}


# --------------------------------------------------------------------------------------------------------------------
# LSTM / GRU cells
# --------------------------------------------------------------------------------------------------------------------
def _sig64(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _sig32(x):
    return np.float32(1.0) / (np.float32(1.0) + expf32(-x))


def lstm_fwd_ref64(gx, gh, c_prev):
    """gx, gh [B][4H] (gate order i, f, g, o), c_prev [B][H] -> h, c [B][H], act [B][4H]"""
    s = gx.double() + gh.double()
    H = c_prev.shape[1]
    ig, fg, gg, og = _sig64(s[:, :H]), _sig64(s[:, H:2 * H]), torch.tanh(s[:, 2 * H:3 * H]), _sig64(s[:, 3 * H:])
    c = fg * c_prev.double() + ig * gg
    return {"h": og * torch.tanh(c), "c": c, "act": torch.cat([ig, fg, gg, og], 1)}


def lstm_fwd_yard(gx, gh, c_prev):
    s = _np32(gx) + _np32(gh)
    H = c_prev.shape[1]
    ig, fg, gg, og = _sig32(s[:, :H]), _sig32(s[:, H:2 * H]), np.tanh(s[:, 2 * H:3 * H]), _sig32(s[:, 3 * H:])
    c = fg * _np32(c_prev) + ig * gg
    return {"h": _out(og * np.tanh(c), F32), "c": _out(c, F32), "act": _out(np.concatenate([ig, fg, gg, og], 1), F32)}


def _lstm_bwd(dh, dc, act, c_prev, c, tanh, cat):
    H = c.shape[1]
    ig, fg, gg, og = act[:, :H], act[:, H:2 * H], act[:, 2 * H:3 * H], act[:, 3 * H:]
    tc = tanh(c)
    dcn = dh * og * (1 - tc * tc)
    if dc is not None:
        dcn = dc + dcn
    return {"dgates": cat([dcn * gg * ig * (1 - ig), dcn * c_prev * fg * (1 - fg), dcn * ig * (1 - gg * gg), dh * tc * og * (1 - og)]),
            "dc_prev": dcn * fg}


def lstm_bwd_ref64(dh, dc, act, c_prev, c):
    """dh / dc None = zero -> dgates [B][4H] (gradient of gx + gh), dc_prev [B][H], from the saved activations"""
    z = torch.zeros_like(c, dtype=F64)
    return _lstm_bwd(z if dh is None else dh.double(), None if dc is None else dc.double(), act.double(), c_prev.double(),
                     c.double(), torch.tanh, lambda v: torch.cat(v, 1))


def lstm_bwd_yard(dh, dc, act, c_prev, c):
    z = np.zeros(tuple(c.shape), dtype=np.float32)
    o = _lstm_bwd(z if dh is None else _np32(dh), None if dc is None else _np32(dc), _np32(act), _np32(c_prev), _np32(c),
                  np.tanh, lambda v: np.concatenate(v, 1))
    return {k: _out(v, F32) for k, v in o.items()}


def lstm_bwd_floors(dh, dc, act, c_prev, c, ref):
    """Saturated gates: 1 - ig, 1 - gg^2, 1 - tanh(c)^2 are differences of float32 values next to 1, absolute error u (one
    rounding; 2u with the square), while the factor itself may be far smaller.  With tanhf good to 4u relative,
    e(1 - tc^2) = 10u, and e_dcn = u |dc| + |dh og| 10u + 4u |dcn|, each product carries its factors' errors and 4u of its own:
        |err d_i| <= |gg ig (1 - ig)| e_dcn + |dcn gg ig| u + 4u |d_i|,      |err d_f| alike with c_prev fg (1 - fg),
        |err d_g| <= |ig (1 - gg^2)| e_dcn + |dcn ig| 2u + 4u |d_g|,
        |err d_o| <= |dh og (1 - og)| 4u |tc| + |dh tc og| u + 4u |d_o|,     |err dc_prev| <= fg e_dcn + u |dc_prev|.
    -> relative floors of dgates and dc_prev"""
    a, cp, cc = act.double(), c_prev.double(), c.double()
    H = cc.shape[1]
    z = torch.zeros_like(cc)
    dh, dc = z if dh is None else dh.double(), z if dc is None else dc.double()
    ig, fg, gg, og = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    tc = torch.tanh(cc)
    dcn = dc + dh * og * (1 - tc * tc)
    e_dcn = U * dc.abs() + (dh * og).abs() * 10.0 * U + 4.0 * U * dcn.abs()
    d = ref["dgates"].double()
    b = torch.cat([(gg * ig * (1 - ig)).abs() * e_dcn + (dcn * gg * ig).abs() * U,
                   (cp * fg * (1 - fg)).abs() * e_dcn + (dcn * cp * fg).abs() * U,
                   (ig * (1 - gg * gg)).abs() * e_dcn + (dcn * ig).abs() * 2.0 * U,
                   (dh * og * (1 - og)).abs() * 4.0 * U * tc.abs() + (dh * tc * og).abs() * U], 1) + 4.0 * U * d.abs()
    return {"dgates": _relmax(b, d), "dc_prev": _relmax(fg * e_dcn + U * ref["dc_prev"].abs(), ref["dc_prev"])}


def gru_bwd_floors(dh, act, h_prev, ref):
    """as lstm_bwd_floors: e(1 - zg) = u, e(1 - ng^2) = 2u absolute,
        e_dn = |dh| ((1 - ng^2) u + (1 - zg) 2u) + 4u |dn|,
        |err dz| <= |dh (h_prev - ng) zg| u + 5u |dz|,   |err dr| <= |hn rg (1 - rg)| e_dn + |dn hn rg| u + 4u |dr|,
        |err dn rg| <= rg e_dn + u |dn rg|.
    -> relative floors of dgx, dgh (dh_prev = dh zg is one product)"""
    a, hp, g = act.double(), h_prev.double(), dh.double()
    H = hp.shape[1]
    rg, zg, ng, hn = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    dn = g * (1 - zg) * (1 - ng * ng)
    e_dn = g.abs() * ((1 - ng * ng) * U + (1 - zg) * 2.0 * U) + 4.0 * U * dn.abs()
    dz = g * (hp - ng) * zg * (1 - zg)
    e_dz = (g * (hp - ng) * zg).abs() * U + 5.0 * U * dz.abs()
    dr = dn * hn * rg * (1 - rg)
    e_dr = (hn * rg * (1 - rg)).abs() * e_dn + (dn * hn * rg).abs() * U + 4.0 * U * dr.abs()
    return {"dgx": _relmax(torch.cat([e_dr, e_dz, e_dn], 1), ref["dgx"]),
            "dgh": _relmax(torch.cat([e_dr, e_dz, rg * e_dn + U * (dn * rg).abs()], 1), ref["dgh"])}


def gru_fwd_ref64(gx, gh, h_prev):
    """gx, gh [B][3H] (gate order r, z, n) -> h [B][H], act [B][4H] = r, z, n, hn (hn = the n slice of gh)"""
    x, r = gx.double(), gh.double()
    H = h_prev.shape[1]
    rg, zg, hn = _sig64(x[:, :H] + r[:, :H]), _sig64(x[:, H:2 * H] + r[:, H:2 * H]), r[:, 2 * H:]
    ng = torch.tanh(x[:, 2 * H:] + rg * hn)
    return {"h": (1.0 - zg) * ng + zg * h_prev.double(), "act": torch.cat([rg, zg, ng, hn], 1)}


def gru_fwd_yard(gx, gh, h_prev):
    x, r = _np32(gx), _np32(gh)
    H = h_prev.shape[1]
    one = np.float32(1.0)
    rg, zg, hn = _sig32(x[:, :H] + r[:, :H]), _sig32(x[:, H:2 * H] + r[:, H:2 * H]), r[:, 2 * H:]
    ng = np.tanh(x[:, 2 * H:] + rg * hn)
    return {"h": _out((one - zg) * ng + zg * _np32(h_prev), F32), "act": _out(np.concatenate([rg, zg, ng, hn], 1), F32)}


def _gru_bwd(dh, act, h_prev, cat):
    H = h_prev.shape[1]
    rg, zg, ng, hn = act[:, :H], act[:, H:2 * H], act[:, 2 * H:3 * H], act[:, 3 * H:]
    dn = dh * (1 - zg) * (1 - ng * ng)
    dz = dh * (h_prev - ng) * zg * (1 - zg)
    dr = dn * hn * rg * (1 - rg)
    return {"dgx": cat([dr, dz, dn]), "dgh": cat([dr, dz, dn * rg]), "dh_prev": dh * zg}


def gru_bwd_ref64(dh, act, h_prev):
    """-> dgx, dgh [B][3H], dh_prev [B][H] (the direct z * dh path only), from the saved activations"""
    return _gru_bwd(dh.double(), act.double(), h_prev.double(), lambda v: torch.cat(v, 1))


def gru_bwd_yard(dh, act, h_prev):
    return {k: _out(v, F32) for k, v in _gru_bwd(_np32(dh), _np32(act), _np32(h_prev), lambda v: np.concatenate(v, 1)).items()}


# --------------------------------------------------------------------------------------------------------------------
# KAN features
# --------------------------------------------------------------------------------------------------------------------
KAN_ACTS = ("silu", "gelu", "relu", "identity")         # base_act codes 0 .. 3


def _bsplines64(x, grid, order):
    """Cox-de Boor recursion: x [B][in], grid [in][nk] -> bases [B][in][nk - 1 - order]"""
    xe = x[:, :, None]
    b = ((xe >= grid[None, :, :-1]) & (xe < grid[None, :, 1:])).to(x.dtype)
    for k in range(1, order + 1):
        n = grid.shape[1] - 1 - k
        d1 = grid[:, k:k + n] - grid[:, :n]
        d2 = grid[:, k + 1:k + 1 + n] - grid[:, 1:1 + n]
        b = (xe - grid[None, :, :n]) / d1 * b[:, :, :n] + (grid[None, :, k + 1:k + 1 + n] - xe) / d2 * b[:, :, 1:n + 1]
    return b


def _act64(x, act):
    if act == 0:
        return x * _sig64(x)
    if act == 1:
        return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))
    return x.clamp_min(0.0) if act == 2 else x


def kan_ref64(x, grid, order, act, dfeat=None):
    """feat [B][in * (1 + nb)] = [act(x) | bases(x[:, 0]) .. bases(x[:, in - 1])]; with dfeat: dx [B][in]"""
    xd = x.double().clone().requires_grad_(True)
    feat = torch.cat([_act64(xd, act), _bsplines64(xd, grid.double(), order).reshape(xd.shape[0], -1)], 1)
    o = {"feat": feat.detach()}
    if dfeat is not None:
        (feat * dfeat.double()).sum().backward()
        o["dx"] = xd.grad
    return o


def kan_yard(x, grid, order, act, dfeat=None):
    xv, g = _np32(x), _np32(grid)
    B, in_f = xv.shape
    nk = g.shape[1]
    nb = nk - 1 - order
    one, half, zero = np.float32(1.0), np.float32(0.5), np.float32(0.0)
    xe = xv[:, :, None]
    b = ((xe >= g[None, :, :-1]) & (xe < g[None, :, 1:])).astype(np.float32)
    db = np.zeros_like(b)
    for k in range(1, order + 1):
        n = nk - 1 - k
        d1 = (g[:, k:k + n] - g[:, :n])[None]
        d2 = (g[:, k + 1:k + 1 + n] - g[:, 1:1 + n])[None]
        a, c = (xe - g[None, :, :n]) / d1, (g[None, :, k + 1:k + 1 + n] - xe) / d2
        b, db = (a * b[:, :, :n] + c * b[:, :, 1:n + 1],
                 b[:, :, :n] / d1 + a * db[:, :, :n] - b[:, :, 1:n + 1] / d2 + c * db[:, :, 1:n + 1])
    erf = torch.erf(torch.from_numpy(xv * np.float32(0.70710678118654752440))).numpy()
    sg = one / (one + expf32(-xv))
    if act == 0:
        av, ag = xv / (one + expf32(-xv)), sg * (one + xv * (one - sg))
    elif act == 1:
        av = half * xv * (one + erf)
        ag = half * (one + erf) + xv * np.float32(0.39894228040143267794) * expf32(np.float32(-0.5) * xv * xv)
    elif act == 2:
        av, ag = np.where(xv > 0, xv, zero), np.where(xv > 0, one, zero)
    else:
        av, ag = xv, np.ones_like(xv)
    o = {"feat": _out(np.concatenate([av, b.reshape(B, -1)], 1), F32)}
    if dfeat is not None:
        d = _np32(dfeat)
        terms = np.concatenate([(d[:, :in_f] * ag)[:, :, None], d[:, in_f:].reshape(B, in_f, nb) * db], 2)
        o["dx"] = _out(seq_sum32(terms, 2), F32)
    return o


def kan_grid(in_f, grid_size, order, uniform, g):
    """(in_f, grid_size + 2 * order + 1) strictly increasing knots per feature: the uniform grid of KANLinear on [-1, 1], or
    spacings drawn from 0.1 .. 0.5 with a per-feature offset"""
    nk = grid_size + 2 * order + 1
    if uniform:
        h = 2.0 / grid_size
        return ((torch.arange(-order, grid_size + order + 1, dtype=F32) * h - 1.0).expand(in_f, -1)).contiguous()
    steps = 0.1 + 0.4 * torch.rand(in_f, nk, generator=g)
    return (torch.cumsum(steps, 1) - 1.0 - torch.rand(in_f, 1, generator=g)).float().contiguous()


def kan_x(B, grid, g):
    """x inside each feature's grid, kept at least 2.5e-4 off every knot, with planted rows: x equal to the first, the last
    and two inner knots, below the first knot and above the last one (as far as B has rows for them)"""
    in_f, nk = grid.shape
    lo, hi = grid[:, 0], grid[:, -1]
    x = (lo + (hi - lo) * torch.rand(B, in_f, generator=g)).float()
    near = ((x[:, :, None] - grid[None]).abs() < 2.5e-4).any(2)
    x = torch.where(near, x + 5.0e-4, x)
    plant = [grid[:, 0], grid[:, -1], grid[:, nk // 2], grid[:, 1], lo - 0.5, hi + 0.5, grid[:, nk - 2]]
    for r, v in enumerate(plant[:max(B - 1, 1)]):
        x[B - 1 - r] = v
    return x.contiguous()


# --------------------------------------------------------------------------------------------------------------------
# the cases, shared by the CPU and the GPU tests (each a dict; "tag" names it in every printed line)
# --------------------------------------------------------------------------------------------------------------------
KINDS = ("randn", "sat", "shift", "margin")
MARGIN = 200.0


def _logits(g, B, Cn, kind, y):
    """randn; randn * 50 (saturated, some rows misclassified); randn + 1e4 (shift invariance); margin: randn with the label
    class of row B // 2 leading by 200 (p exactly 1 in float32)"""
    z = torch.randn(B, Cn, generator=g)
    if kind == "sat":
        z = z * 50.0
    elif kind == "shift":
        z = z + 1.0e4
    elif kind == "margin":
        r = B // 2
        z[r, y[r]] = z[r].max() + MARGIN
    return z


def ce_cases():
    """B: 4 / 8 / 16 waves with idle waves and a second row per wave; C: one class, below / at / above one and two lane
    strides.  Kind, weight and smoothing cycle so that every combination occurs; in the C = 65 and C = 130 cases the maximum
    of row 0 sits in the last class."""
    cases = []
    i = 0
    for B in (1, 3, 15, 16, 17, 31, 32, 33, 70):
        for Cn in (1, 2, 7, 64, 65, 130):
            g = gen(5000 + i)
            kind = KINDS[(i + i // 6) % 4]
            y = torch.randint(0, Cn, (B,), generator=g)
            z = _logits(g, B, Cn, kind, y)
            if Cn in (65, 130) and not (kind == "margin" and B // 2 == 0):
                z[0, Cn - 1] = z[0].max() + 100.0       # (by 100: a maximum taken over the first 64 classes only overflows exp)
            weight = 0.5 + torch.rand(Cn, generator=g) if (i // 2) % 2 else None
            s = 0.1 if (i // 3) % 2 else 0.0
            cases.append({"tag": f"ce B={B} C={Cn} {kind} w={weight is not None} s={s}", "z": z, "y": y, "weight": weight,
                          "s": s, "kind": kind, "margin_row": B // 2 if kind == "margin" else None})
            i += 1
    for j, (B, Cn, weight, s) in enumerate(((17, 7, False, 0.0), (33, 65, True, 0.0), (70, 130, True, 0.1), (3, 2, False, 0.1))):
        g = gen(5100 + j)              # the margin row under every weight / smoothing setting
        y = torch.randint(0, Cn, (B,), generator=g)
        w = 0.5 + torch.rand(Cn, generator=g) if weight else None
        cases.append({"tag": f"ce B={B} C={Cn} margin w={weight} s={s} (extra)", "z": _logits(g, B, Cn, "margin", y), "y": y,
                      "weight": w, "s": s, "kind": "margin", "margin_row": B // 2})
    return cases


GAMMAS = (0.0, 1.0, 1.5, 2.0, 5.0)


def focal_cases():
    """B below / at / above one and two strides of 256 threads; every gamma on every value kind, gamma = 0.5 on randn only.
    "saturated": the case holds a row whose float64 ce is below 1e-16 (1 - exp(-ce) is exactly 0)."""
    cases = []
    i = 0

    def add(B, Cn, gamma, kind, weight, seed):
        g = gen(seed)
        y = torch.randint(0, Cn, (B,), generator=g)
        w = 0.5 + torch.rand(Cn, generator=g) if weight else None
        cases.append({"tag": f"focal B={B} C={Cn} gamma={gamma} {kind} w={weight}", "z": _logits(g, B, Cn, kind, y), "y": y,
                      "weight": w, "gamma": gamma, "kind": kind, "margin_row": B // 2 if kind == "margin" else None})

    for B in (1, 255, 256, 257, 600):
        for Cn in (1, 2, 7, 70):
            add(B, Cn, GAMMAS[i % 5], KINDS[(i + i // 4) % 4], bool((i // 2) % 2), 5200 + i)
            i += 1
    for j, gamma in enumerate(GAMMAS):
        add(257, 7, gamma, "margin", True, 5300 + j)
        add(33, 70, gamma, "sat", False, 5310 + j)
    add(255, 7, 0.5, "randn", True, 5320)
    add(600, 70, 0.5, "randn", False, 5321)
    return cases


# the only cases whose float64 reference is not finite: 0 < gamma < 1 on a saturated row (none is generated: gamma = 0.5
# runs on randn data only; the CPU test builds this one to show that the exclusion is real)
NONFINITE_REFERENCE = ("focal gamma=0.5 on a row whose label class leads by 200",)


def entropy_cases():
    cases = []
    i = 0
    for rows in (1, 3, 4, 5, 9):
        for Cn in (1, 7, 64, 65, 200):
            g = gen(5400 + i)
            kind = ("randn", "sat", "mixed")[(i + i // 5) % 3]
            z = torch.randn(rows, Cn, generator=g) * (30.0 if kind == "sat" else 2.0)
            if kind == "mixed":
                z[::2] = z[::2] * 25.0
            cases.append({"tag": f"entropy rows={rows} C={Cn} {kind}", "z": z, "g": torch.randn(rows, generator=g), "kind": kind})
            i += 1
    return cases


KL_EPS = 1e-8


def kl_planted():
    """values planted into p and q: on the upper bound, on the lower bound, below it (two ways), above the upper bound"""
    e = _f32(KL_EPS)
    return (1.0, e, 0.0, _f32(np.float32(0.5) * np.float32(KL_EPS)), 1.5)


def kl_cases():
    """softmax probabilities with planted entries in p (row 0) and q (last row); every third case has q within 1e-4 of p
    (lp - lq cancels)"""
    cases = []
    i = 0
    for rows in (1, 4, 5):
        for cols in (1, 7, 64, 65, 130):
            g = gen(5500 + i)
            p = torch.softmax(torch.randn(rows, cols, generator=g) * 2.0, 1)
            if i % 3 == 0:
                q = (p * (1.0 + 1.0e-4 * torch.randn(rows, cols, generator=g))).float()
            else:
                q = torch.softmax(torch.randn(rows, cols, generator=g) * 2.0, 1)
            for k, v in enumerate(kl_planted()):
                p[0, k % cols] = v
                q[rows - 1, (k + 2 + i) % cols] = v
            if cols == 1:                           # a single column: the planted value cycles with the case
                p[0, 0] = kl_planted()[i % 5]
                q[rows - 1, 0] = kl_planted()[(i + 1) % 5]
            cases.append({"tag": f"kl rows={rows} cols={cols} {'close' if i % 3 == 0 else 'apart'}", "p": p.float().contiguous(),
                          "q": q.float().contiguous(), "w": torch.randn(rows, generator=g), "eps": KL_EPS})
            i += 1
    return cases


MP_KINDS = ("randn", "agree", "identical", "disagree", "margin")


def mp_cases():
    """towers: randn; agreeing (text = image + 0.05 randn: kl about 1e-3); identical (kl exactly 0); confidently disagreeing
    (different classes lead by 30: raw kl > 10); margin (the image tower leads by 21 to 25: probabilities below 1e-8, the
    inner clamp is active; the fused tower is confidently right in every other row)"""
    cases = []
    i = 0
    for B in (1, 7, 256, 257, 300):
        for Cn in (2, 7, 12):
            g = gen(5600 + i)
            kind = MP_KINDS[(i + i // 5) % 5]
            zi = torch.randn(B, Cn, generator=g) * 2.0
            zt = torch.randn(B, Cn, generator=g) * 2.0
            zf = torch.randn(B, Cn, generator=g) * 2.0
            y = torch.randint(0, Cn, (B,), generator=g)
            ar = torch.arange(B)
            if kind == "agree":
                zt = zi + 0.05 * torch.randn(B, Cn, generator=g)
            elif kind == "identical":
                zt = zi.clone()
            elif kind == "disagree":
                a = torch.randint(0, Cn, (B,), generator=g)
                zi[ar, a] += 30.0
                zt[ar, (a + 1) % Cn] += 30.0
            elif kind == "margin":
                a = torch.randint(0, Cn, (B,), generator=g)
                zi[ar, a] = zi.max(1).values + 21.0 + 4.0 * torch.rand(B, generator=g)
                zf[ar[::2], y[::2]] += 25.0         # (every other row: a row's p - 1 at the label is then 1e-11, below float64's reach
                                                    # relative to it, but not relative to the other rows' gradients)
            for _ in range(4):      # a row whose float64 kl falls next to the clamp at 10 gets a flatter text tower
                kl = mp_raw_kl64(zi, zt)
                bad = (kl > 9.9) & (kl < 10.1)
                if not bool(bad.any()):
                    break
                zt[bad] = zt[bad] * 0.5
            cases.append({"tag": f"mp B={B} C={Cn} {kind}", "zi": zi, "zt": zt, "zf": zf, "y": y, "kind": kind})
            i += 1
    return cases


def _supcon_labels(g, B, pattern):
    if pattern == "equal":
        return torch.full((B,), 3, dtype=torch.int64)
    if pattern == "distinct":
        return torch.randperm(B, generator=g) + 10
    lab = torch.randint(0, 7, (B,), generator=g)
    if pattern == "singleton":
        lab = lab % 2
        lab[B // 2] = 9
    return lab


def supcon_cases():
    """B x D with the label patterns cycling; "dup": rows 0, 1 bit-identical with equal labels and rows 2, 3 bit-identical with
    different labels; "near": row 1 within 1e-3 of row 0, equal labels (msum cancels)"""
    cases = []
    i = 0

    def add(B, D, T, pattern, extra=None):
        nonlocal i
        g = gen(5700 + i)
        f = torch.randn(B, D, generator=g)
        lab = _supcon_labels(g, B, pattern)
        if extra == "dup":
            f[1] = f[0]
            f[3] = f[2]
            lab[1] = lab[0]
            lab[3] = lab[2] + 1
        elif extra == "near":
            f[1] = f[0] * (1.0 + 1.0e-3 * torch.randn(D, generator=g))
            lab[1] = lab[0]
        cases.append({"tag": f"supcon B={B} D={D} T={T} {pattern}{' ' + extra if extra else ''}", "feat": f.contiguous(),
                      "labels": lab, "T": T, "pattern": pattern})
        i += 1

    pats = ("random", "equal", "distinct", "singleton")
    for k, (B, D) in enumerate(((2, 1), (3, 63), (4, 64), (5, 65), (64, 130), (65, 7), (256, 3), (5, 1))):
        add(B, D, (0.07, 0.5)[k % 2], pats[k % 4])
        add(B, D, (0.5, 0.07)[k % 2], pats[(k + 1) % 4])
    for pattern in pats:
        add(5, 65, 0.07, pattern)
    add(256, 3, 0.07, "random")
    for B, D in ((5, 65), (64, 130)):
        for T in (0.07, 0.5):
            add(B, D, T, "random", "dup")
            add(B, D, T, "random", "near")
    return cases


def kan_reg_cases():
    cases = []
    i = 0
    for rows in (1, 5, 257, 1000):
        for co in (1, 8):
            ra, re = ((1.0, 1.0), (0.3, 2.0))[i % 2]
            cases.append({"tag": f"kan_reg rows={rows} coeffs={co} ra={ra} re={re}", "w": 0.1 * torch.randn(rows, co, generator=gen(5800 + i)),
                          "ra": ra, "re": re})
            i += 1
    return cases


CELL_SHAPES = ((1, 1), (3, 33), (5, 128), (2, 256), (7, 37))        # B * H below, at and above one block of 256 threads
_PADS = ((0, 0), (8, 0), (0, 8), (8, 8))


def cell_cases(gates):
    """gates = 4 (LSTM) or 3 (GRU): pre-activations randn, and randn * 40 (sigmoid exactly 0 or 1, tanh exactly +-1); the row
    pitches of gx and gh are gates * H or that + 8, independently"""
    cases = []
    i = 0
    for B, H in CELL_SHAPES:
        for scale in (1.0, 40.0):
            g = gen(5900 + 100 * gates + i)
            G = gates * H
            px, ph = _PADS[i % 4]
            cases.append({"tag": f"{'lstm' if gates == 4 else 'gru'} B={B} H={H} x{scale:g} ldx={G + px} ldh={G + ph}",
                          "gx": scale * torch.randn(B, G, generator=g), "gh": scale * torch.randn(B, G, generator=g),
                          "prev": torch.randn(B, H, generator=g), "dh": torch.randn(B, H, generator=g),
                          "dc": torch.randn(B, H, generator=g), "ldx": G + px, "ldh": G + ph, "scale": scale})
            i += 1
    return cases


KAN_GRIDS = ((5, 3), (3, 0), (8, 2), (25, 3))        # (grid_size, order); the last has 32 knots, the limit


def kan_cases():
    cases = []
    i = 0
    for B in (1, 5, 300):
        for in_f in (1, 3, 17):
            for gs, order in KAN_GRIDS:
                g = gen(6100 + i)
                uniform = i % 2 == 0
                act = (i // 2) % 4
                grid = kan_grid(in_f, gs, order, uniform, g)
                x = kan_x(B, grid, g)
                nb = gs + order
                cases.append({"tag": f"kan B={B} in={in_f} grid={gs} order={order} {'uniform' if uniform else 'nonuniform'} {KAN_ACTS[act]}",
                              "x": x, "grid": grid, "gs": gs, "order": order, "act": act,
                              "dfeat": torch.randn(B, in_f * (1 + nb), generator=g)})
                i += 1
    return cases


# --------------------------------------------------------------------------------------------------------------------
# guarded ctypes callers
# --------------------------------------------------------------------------------------------------------------------
def _scalar():
    return GBuf(1, 1, F32, is_vec=True)


def _vecbuf(n):
    return GBuf(1, n, F32, is_vec=True)


def call_ce(z, y, weight, s, want_d=True, want_rows=True, check=True):
    L, lib, rt = _env()
    B, Cn = z.shape
    zd, yd, wd = _fresh(z), _fresh(y), _fresh(weight)
    bufs = {"loss": _scalar(), "dlogits": GBuf(B, Cn, F32) if want_d else None, "row_loss": _vecbuf(B) if want_rows else None}
    st = lib.hs_cross_entropy(_p(zd), _p(yd), _p(wd), s, B, Cn, _p(bufs["loss"]), _p(bufs["dlogits"]), _p(bufs["row_loss"]),
                              rt.stream())
    return _finish(L, st, "hs_cross_entropy", bufs, check)


def call_focal(z, y, weight, gamma, want_d=True, check=True):
    L, lib, rt = _env()
    B, Cn = z.shape
    zd, yd, wd = _fresh(z), _fresh(y), _fresh(weight)
    bufs = {"loss": _scalar(), "dlogits": GBuf(B, Cn, F32) if want_d else None}
    st = lib.hs_focal_loss(_p(zd), _p(yd), _p(wd), gamma, B, Cn, _p(bufs["loss"]), _p(bufs["dlogits"]), rt.stream())
    return _finish(L, st, "hs_focal_loss", bufs, check)


def call_entropy(z, g=None, want_ent=True, check=True):
    L, lib, rt = _env()
    rows, Cn = z.shape
    zd, gd = _fresh(z), _fresh(g)
    bufs = {"ent": _vecbuf(rows) if want_ent else None, "dlogits": GBuf(rows, Cn, F32) if g is not None else None}
    st = lib.hs_softmax_entropy(_p(zd), _p(gd), _p(bufs["ent"]), _p(bufs["dlogits"]), rows, Cn, rt.stream())
    return _finish(L, st, "hs_softmax_entropy", bufs, check)


def call_kl_rows(p, q, eps, w=None, want_out=True, want_dp=False, want_dq=False, check=True):
    L, lib, rt = _env()
    rows, cols = p.shape
    pd, qd, wd = _fresh(p), _fresh(q), _fresh(w)
    bufs = {"out": _vecbuf(rows) if want_out else None, "dp": GBuf(rows, cols, F32) if want_dp else None,
            "dq": GBuf(rows, cols, F32) if want_dq else None}
    st = lib.hs_kl_rows(_p(pd), _p(qd), _p(bufs["out"]), _p(wd), _p(bufs["dp"]), _p(bufs["dq"]), rows, cols, eps, rt.stream())
    return _finish(L, st, "hs_kl_rows", bufs, check)


def call_mp(zi, zt, zf, y, want_d=True, check=True):
    L, lib, rt = _env()
    B, Cn = zi.shape
    a, t, f, yd = _fresh(zi), _fresh(zt), _fresh(zf), _fresh(y)
    bufs = {"loss": _scalar(), "scratch": _vecbuf(B)}
    for k in ("d_image", "d_text", "d_fused"):
        bufs[k] = GBuf(B, Cn, F32) if want_d else None
    st = lib.hs_mp_loss(_p(a), _p(t), _p(f), _p(yd), B, Cn, _p(bufs["loss"]), _p(bufs["d_image"]), _p(bufs["d_text"]),
                        _p(bufs["d_fused"]), _p(bufs["scratch"]), rt.stream())
    return _finish(L, st, "hs_mp_loss", bufs, check)


def call_supcon(feat, labels, T, want_d=True, check=True):
    L, lib, rt = _env()
    B, D = feat.shape
    fd, ld = _fresh(feat), _fresh(labels)
    ws = _wsbuf(lib.hs_supcon_ws_bytes(B, D))
    bufs = {"loss": _scalar(), "dfeat": GBuf(B, D, F32) if want_d else None}
    st = lib.hs_supcon_loss(_p(fd), _p(ld), B, D, T, _p(bufs["loss"]), _p(bufs["dfeat"]), _p(ws), rt.stream())
    return _finish(L, st, "hs_supcon_loss", bufs, check)


def call_kan_reg(w, ra, re, want_loss=True, want_dw=True, check=True):
    L, lib, rt = _env()
    rows, co = w.shape
    wd = _fresh(w)
    bufs = {"loss": _scalar() if want_loss else None, "dw": GBuf(rows, co, F32) if want_dw else None}
    st = lib.hs_kan_regularization(_p(wd), rows, co, ra, re, _p(bufs["loss"]), _p(bufs["dw"]), rt.stream())
    return _finish(L, st, "hs_kan_regularization", bufs, check)


def call_lstm_fwd(gx, gh, c_prev, ldx, ldh, check=True):
    L, lib, rt = _env()
    B, H = c_prev.shape
    k1, xd = _pitched(gx.float(), ldx)
    k2, hd = _pitched(gh.float(), ldh)
    cd = _fresh(c_prev)
    bufs = {"h": GBuf(B, H, F32), "c": GBuf(B, H, F32), "act": GBuf(B, 4 * H, F32)}
    st = lib.hs_lstm_cell_fwd(_p(xd), ldx, _p(hd), ldh, _p(cd), _p(bufs["h"]), _p(bufs["c"]), _p(bufs["act"]), B, H, rt.stream())
    return _finish(L, st, "hs_lstm_cell_fwd", bufs, check)


def call_lstm_bwd(dh, dc, act, c_prev, c, check=True):
    L, lib, rt = _env()
    B, H = c.shape
    dhd, dcd, ad, cpd, cd = _fresh(dh), _fresh(dc), _fresh(act), _fresh(c_prev), _fresh(c)
    bufs = {"dgates": GBuf(B, 4 * H, F32), "dc_prev": GBuf(B, H, F32)}
    st = lib.hs_lstm_cell_bwd(_p(dhd), _p(dcd), _p(ad), _p(cpd), _p(cd), _p(bufs["dgates"]), _p(bufs["dc_prev"]), B, H, rt.stream())
    return _finish(L, st, "hs_lstm_cell_bwd", bufs, check)


def call_gru_fwd(gx, gh, h_prev, ldx, ldh, check=True):
    L, lib, rt = _env()
    B, H = h_prev.shape
    k1, xd = _pitched(gx.float(), ldx)
    k2, hd = _pitched(gh.float(), ldh)
    hp = _fresh(h_prev)
    bufs = {"h": GBuf(B, H, F32), "act": GBuf(B, 4 * H, F32)}
    st = lib.hs_gru_cell_fwd(_p(xd), ldx, _p(hd), ldh, _p(hp), _p(bufs["h"]), _p(bufs["act"]), B, H, rt.stream())
    return _finish(L, st, "hs_gru_cell_fwd", bufs, check)


def call_gru_bwd(dh, act, h_prev, check=True):
    L, lib, rt = _env()
    B, H = h_prev.shape
    dhd, ad, hp = _fresh(dh), _fresh(act), _fresh(h_prev)
    bufs = {"dgx": GBuf(B, 3 * H, F32), "dgh": GBuf(B, 3 * H, F32), "dh_prev": GBuf(B, H, F32)}
    st = lib.hs_gru_cell_bwd(_p(dhd), _p(ad), _p(hp), _p(bufs["dgx"]), _p(bufs["dgh"]), _p(bufs["dh_prev"]), B, H, rt.stream())
    return _finish(L, st, "hs_gru_cell_bwd", bufs, check)


def call_kan_fwd(x, grid, grid_size, order, act, check=True):
    L, lib, rt = _env()
    B, in_f = x.shape
    xd, gd = _fresh(x), _fresh(grid)
    bufs = {"feat": GBuf(B, in_f * (1 + grid_size + order), F32)}
    st = lib.hs_kan_features_fwd(_p(xd), _p(gd), _p(bufs["feat"]), B, in_f, grid_size, order, act, rt.stream())
    return _finish(L, st, "hs_kan_features_fwd", bufs, check)


def call_kan_bwd(x, grid, dfeat, grid_size, order, act, check=True):
    L, lib, rt = _env()
    B, in_f = x.shape
    xd, gd, dd = _fresh(x), _fresh(grid), _fresh(dfeat)
    bufs = {"dx": GBuf(B, in_f, F32)}
    st = lib.hs_kan_features_bwd(_p(xd), _p(gd), _p(dd), _p(bufs["dx"]), B, in_f, grid_size, order, act, rt.stream())
    return _finish(L, st, "hs_kan_features_bwd", bufs, check)
