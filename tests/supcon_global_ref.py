"""References for the tiled SupCon kernels (hs_supcon_tiled): the float64 reference and the sequential-float32 yardstick are
head_ref's (supcon_ref64, supcon_yard), restated here only in a block-wise form for cases whose N * N * D products do not fit
one numpy array; the a-priori floors are derived anew below from the accumulation order of csrc/supcon.hip; the guarded ctypes
caller follows head_ref.call_supcon.

Importing this module needs no GPU.
"""
import numpy as np
import torch

from head_ref import (E8, E12, F32, U, _scalar, _supcon_labels, expf32, supcon_ref64, supcon_yard)  # noqa: F401
from kernel_ref import (F32_NOISE, GBuf, _env, _f32, _finish, _fresh, _np32, _out, _p, _wsbuf, gen, seq_sum32)  # noqa: F401

F64 = torch.float64
TILE = 64            # anchors per workgroup and keys per tile of csrc/supcon.hip

# (N, D) of the GPU test: the issue's list, then the kernel's own edges that are not at 64: the 32-column staging step of the
# dot product (31, 33) and the 256-column slice of the gradient pass (255 / 256; 257 and 260 are in the list).  From 65 rows on
# the keys are cut into runs (key_splits below), of one tile each up to 1024 rows; MULTI: the smallest kind of shape whose runs
# hold two tiles (18 tiles in 9 runs), so that the running statistics and the gradient chain cross a tile boundary
SHAPES = ((1, 1), (2, 1), (63, 5), (64, 64), (65, 65), (129, 130), (257, 3), (300, 257), (513, 260), (70, 1024),
          (33, 31), (66, 33), (20, 255), (17, 256))
MULTI = (1089, 12)
PATTERNS = ("random", "equal", "distinct", "singleton")


def _s32(v):
    return _out(np.asarray(v, dtype=np.float32).reshape(1), F32)


def tiled_cases():
    """the shapes with temperature 0.07 / 0.5 alternating and the label patterns cycling, then the "dup" and "near" rows of
    head_ref.supcon_cases (rows 0, 1 bit-identical with equal labels and rows 2, 3 bit-identical with different labels; row 1
    within 1e-3 of row 0 with equal labels) on (65, 65) and (129, 130)"""
    cases = []

    def add(N, D, T, pattern, extra=None):
        g = gen(9100 + len(cases))
        f = torch.randn(N, D, generator=g)
        lab = _supcon_labels(g, N, pattern)
        if extra == "dup":
            f[1] = f[0]
            f[3] = f[2]
            lab[1] = lab[0]
            lab[3] = lab[2] + 1
        elif extra == "near":
            f[1] = f[0] * (1.0 + 1.0e-3 * torch.randn(D, generator=g))
            lab[1] = lab[0]
        cases.append({"tag": f"supcon tiled N={N} D={D} T={T} {pattern}{' ' + extra if extra else ''}", "feat": f.contiguous(),
                      "labels": lab, "T": T, "pattern": pattern})

    for k, (N, D) in enumerate(SHAPES):
        add(N, D, (0.07, 0.5)[k % 2], PATTERNS[k % 4])
    add(*MULTI, 0.07, "random")
    for (N, D), T in (((65, 65), 0.07), ((129, 130), 0.5)):
        add(N, D, T, "random", "dup")
        add(N, D, T, "random", "near")
    return cases


# --------------------------------------------------------------------------------------------------------------------
# the yardstick, block-wise
# --------------------------------------------------------------------------------------------------------------------
def supcon_yard_blocked(feat, labels, T, max_elems=1 << 22):
    """head_ref.supcon_yard with the two N x N x D products formed for a block of anchors at a time (at most max_elems
    products per block).  Every sum is the same strictly sequential float32 sum over the same terms in the same order, so the
    result is supcon_yard's bit for bit."""
    f = _np32(feat)
    B, D = f.shape
    lab = labels.numpy()
    one, e8, zero, bf, Tf = np.float32(1.0), np.float32(1e-8), np.float32(0.0), np.float32(B), np.float32(T)
    step = max(1, int(max_elems // max(B * D, 1)))
    nrm = np.maximum(np.sqrt(seq_sum32(f * f, 1)), np.float32(1e-12))
    fn = f / nrm[:, None]
    sim = np.empty((B, B), dtype=np.float32)
    for a in range(0, B, step):
        sim[a:a + step] = seq_sum32(fn[a:a + step, None, :] * fn[None, :, :], 2) / Tf
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
    g = np.empty((B, D), dtype=np.float32)
    for a in range(0, B, step):
        g[a:a + step] = seq_sum32(S[a:a + step, :, None] * fn[None, :, :], 1) / Tf
    dot = seq_sum32(g * fn, 1)
    return {"loss": _s32(loss), "dfeat": _out((g - dot[:, None] * fn) / nrm[:, None], F32)}


# --------------------------------------------------------------------------------------------------------------------
# a-priori floors of the tiled kernels
# --------------------------------------------------------------------------------------------------------------------
def key_splits(N):
    """(key tiles per run, runs) of csrc/supcon.hip: about 512 workgroups per pass, at most 16 runs, from N alone"""
    NT = -(-N // TILE)
    want = min(max(-(-512 // NT), 1), 16, NT)
    tps = -(-NT // want)
    return tps, -(-NT // tps)


def supcon_tiled_floors(feat, labels, T, ref):
    """Rounding bounds of csrc/supcon.hip from its accumulation order, the inputs and the float64 reference alone
    (u = 2^-24, Dp = D rounded up to 4, raw logits s_ij = fn_i . fn_j / T, |s_ij| <= 1 / T).  The kernels cut the ceil(N / 64)
    key tiles into KS runs of tps tiles (key_splits below, the kernel's rule); a row's sums walk the tiles of a run in order and
    then the runs in order, R = tps + KS steps.

    Normalisation: |f_i|^2 is a lane-strided chain of ceil(D / 64) additions and a 6-level tree, Dn = ceil(D / 64) + 6 roundings;
    with the square root and the division an element of fn carries (Dn + 3) u relative (as head_ref.supcon_floors).
    Dot product: the f32-input MFMA is an exact k-ordered fma chain, ONE chain of Dp terms per s_ij with one rounding per term:
    Dp u sum_k |fn_ik fn_jk| <= Dp u, plus 2 (Dn + 3) u from the two inputs and the division by T:
        |err s_ij| <= Es = (Dp + 2 Dn + 8) u / T.
    Row statistics (online softmax over the tiles of a run, then over the runs): a term exp(s_ij - mx_i) moves by 2 Es relative through its
    argument and by (2 / T + 4) u in __expf (argument rounding |x| u, |x| <= 2 / T, exp2 and the subtraction).  The rescale
    factors exp(mx_old - mx_new) are exact in their inputs (exp(a - b) exp(s - a) = exp(s - b) for the computed a, b); their
    evaluation costs (|x| + 4) u each, the |x| telescope to at most 2 / T over the row, so all R of them cost (2 / T + 4 R) u.
    The additions: 4 in the lane, a 4-level tree over the row's 16 lanes, one per step: (R + 8) u on positive terms.  So
        relerr E_i <= eE = 2 Es + (5 R + 4 / T + 13) u             (the 1e-8 joins with one more rounding),
        |err log E_i| <= eL_i = eE + u |log E_i| + u.
    Loss: the kernel forms msum_i = ps_i - P_i (mx_i + log E_i), ps_i = sum over positives of the raw s_ij in that same
    (R + 8)-deep order, A_i = sum over positives of |s_ij|:
        |err msum_i| <= P_i Es + (R + 8) u A_i + P_i (Es + eL_i + 2u |mx_i + log E_i|) + u |msum_i|,
    then / (P_i + 1e-8) / N with 3 roundings; the N row losses are added in float64 and rounded once:
        |err loss| <= mean_i [2 Es + eL_i + (R + 8) u A_i / P_i + 2u |mx_i + log E_i| + 4u |msum_i| / P_i]_{P_i > 0} + u |loss|.
    Gradient: q_ik = exp(s_ik - mx_i) / E_i has the relative error Eq = 2 Es + (2 / T + 4) u + eE + 2u, and
        |err G_ik| <= w_i P_i q_ik (Eq + 2u) + 4u |G_ik|,     errC = errG + errG^T + u |C|,   C = G + G^T.
    g_i = (sum_k C_ik fn_k) / T is one fma chain per run and element (the accumulator lives across the run's key tiles, at most
    Ng = min(N, 64 tps) terms) and KS additions of the runs:
        e_id = (errC |fn| + (Ng + KS + Dn + 5) u |C| |fn|)_id / T.
    The projection uses dot_i = g_i . fn_i = sum_k C_ik s_ik, summed (R + 8) deep from the tiles:
        ed_i = sum_k errC_ik |s_ik| + Es sum_k |C_ik| + (R + 9) u sum_k |C_ik s_ik|,
        |err dfeat_id| <= (e_id + |fn_id| (ed_i + (Dn + 3) u |dot_i|) + (Dn + 6) u (|g_id| + |dot_i fn_id|)) / |f_i|.
    -> relative floors of loss and dfeat, and "dfeat_abs": the largest absolute bound (for D = 1, where the projection leaves
    exactly 0)."""
    fd = feat.double()
    N, D = fd.shape
    Td = _f32(T)
    Dp = -(-D // 4) * 4
    Dn = -(-D // 64) + 6
    tps, KS = key_splits(N)
    R, Ng = tps + KS, min(N, TILE * tps)
    Es = (Dp + 2.0 * Dn + 8.0) * U / Td
    nrm = fd.norm(dim=1, keepdim=True).clamp_min(E12)
    fn = fd / nrm
    raw = fn @ fn.T / Td
    mx = raw.max(1).values
    sim = raw - mx[:, None]
    off = ~torch.eye(N, dtype=torch.bool)
    offd = off.double()
    pos = (off & (labels[:, None] == labels[None, :])).double()
    P = pos.sum(1)
    Ei = (sim.exp() * offd).sum(1) + E8
    lE = Ei.log()
    eE = 2.0 * Es + (5.0 * R + 4.0 / Td + 13.0) * U
    eL = eE + U * lE.abs() + U
    A = (raw.abs() * pos).sum(1)
    msum = ((sim - lE[:, None]) * pos).sum(1)
    Pc = P.clamp_min(1.0)
    rows = torch.where(P > 0, 2.0 * Es + eL + (R + 8.0) * U * A / Pc + 2.0 * U * (mx + lE).abs() + 4.0 * U * msum.abs() / Pc,
                       torch.zeros_like(P))
    lb = rows.mean() + U * ref["loss"].double().abs().max()
    Eq = 2.0 * Es + (2.0 / Td + 4.0) * U + eE + 2.0 * U
    w = 1.0 / (N * (P + E8))
    q = sim.exp() * offd / Ei[:, None]
    G = -w[:, None] * (pos - P[:, None] * q) * offd
    eG = (w * P)[:, None] * q * (Eq + 2.0 * U) + 4.0 * U * G.abs()
    Cm = G + G.T
    eC = eG + eG.T + U * Cm.abs()
    Af = fn.abs()
    e = (eC @ Af + (Ng + KS + Dn + 5.0) * U * (Cm.abs() @ Af)) / Td
    g = Cm @ fn / Td
    dot = (Cm * raw).sum(1, keepdim=True)
    ed = ((eC * raw.abs()).sum(1) + Es * Cm.abs().sum(1) + (R + 9.0) * U * (Cm * raw).abs().sum(1))[:, None]
    db = (e + Af * (ed + (Dn + 3.0) * U * dot.abs()) + (Dn + 6.0) * U * (g.abs() + (dot * fn).abs())) / nrm

    def relmax(bound, r):
        top = r.double().abs().max().item()
        v = (bound.max().item() / top) if top > 0 else 0.0
        return max(v, F32_NOISE) if np.isfinite(v) else F32_NOISE      # undefined (a zero reference): the gate's plain floor

    return {"loss": relmax(lb, ref["loss"]), "dfeat": relmax(db, ref["dfeat"]), "dfeat_abs": db.max().item()}


# --------------------------------------------------------------------------------------------------------------------
# guarded ctypes caller
# --------------------------------------------------------------------------------------------------------------------
def call_supcon_tiled(feat, labels, T, row0=0, M=None, grad_scale=1.0, want_d=True, check=True, N=None, D=None, ws_bytes=None):
    """hs_supcon_tiled on fresh device copies, loss and dfeat inside guard bands.  N, D, M override what is PASSED (for the
    refusals); the buffers keep the sizes of the tensors."""
    L, lib, rt = _env()
    Nt, Dt = feat.shape
    N = Nt if N is None else N
    D = Dt if D is None else D
    Mt = (Nt - row0 if M is None else M)
    fd, ld = _fresh(feat), _fresh(labels)
    nbytes = lib.hs_supcon_tiled_ws_bytes(Nt, Dt) if ws_bytes is None else ws_bytes
    ws = _wsbuf(nbytes)
    bufs = {"loss": _scalar(), "dfeat": GBuf(max(Mt, 1), Dt, F32) if want_d else None}
    st = lib.hs_supcon_tiled(_p(fd), _p(ld), N, D, row0, Mt if M is None else M, T, grad_scale, _p(bufs["loss"]),
                             _p(bufs["dfeat"]), _p(ws), rt.stream())
    return _finish(L, st, "hs_supcon_tiled", bufs, check)
