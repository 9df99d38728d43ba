"""Float64 reference, per-element error scales, bf16 / f32 emulation, case list and guarded ctypes caller for the attention
core (hs_attention_fwd / hs_attention_bwd: csrc/attn_fused.hip and the GEMM + softmax path of csrc/blocks.hip).

The reference works in float64 on exactly the values the kernels read (bf16-rounded inputs, the float32 scale and 1/(1-p) of
the descriptor).  Masked keys are filled with float32(-3.0e38), as the kernels do, so a fully masked row is uniform.

    P  = softmax(scale Q K^T + mask)     Pd = P * keep * inv_keep        o  = Pd V            dv = Pd^T dO
    dP = (dO V^T) * keep * inv_keep      delta = rowsum(P * dP)          dS = P * (dP - delta)
    dq = scale dS K                      dk = scale dS^T Q

Every output element has an error scale of its own: the sum of magnitudes through which one rounding of P or dS to the
storage type (unit u: 2^-8 for bf16, 2^-23 for f32) reaches it,

    S_o = Pd |V|     S_dv = Pd^T |dO|     A = P * (|dP| + rowsum(P * |dP|))     S_dq = scale A |K|     S_dk = scale A^T |Q|

and the gate is |got - ref| <= c * u * S + 1e-30 for EVERY element (P: S = P_ref).  A sharp row in one batch therefore
says nothing about what a diffuse row in another may get wrong, which a max-norm gate cannot tell apart.

The saved P has one more gate: |sum_k P[r][k] - 1| <= c * u * sqrt(sum_k P_ref[r][k]^2) (equal values of a row counted as
one term, see _rowsum_scale).  Independent roundings to nearest add in quadrature, so the row sum of a correctly rounded P
stays near that scale; a P that is truncated instead of rounded is low by about 0.7 * u in every element, which no
per-element gate with c >= 2 can see (truncation errs by at most 2 u) but which adds linearly over a row.
(bf16 only: in f32 the common factor 1 / sum carries a float32 rounding of its own, which is no random walk.)

The constants are 4x the worst ratio |emulated - ref| / (u * S) that attention_emulated -- the same computation with P, Pd,
dS, o, dq, dk, dv rounded to the storage type, the scores and dP to float32 (what the kernels hold them in), everything else
float64 -- reaches over CASES.  The factor 4 covers what the emulation leaves out: float32 accumulation order, the hardware
exp, float32 row sums.  test_attn_ref_cpu.py recomputes the ratios and asserts 4x <= constant <= 8x.  Measured ratios:

    bf16 (47 cases): o 1.606   dq 1.488   dk 2.004   dv 1.754   P 0.996   row sum 1.589
    f32  (1 case):   o 0.746   dq 0.499   dk 0.448   dv 0.643   P 1.467

The kernels themselves, on an MI355X (test_attn_gpu.py prints them per case): the bf16 outputs land on the emulation's own
bf16 values at the worst elements, o 1.606, dq 1.488, dk 2.004, dv 1.754, P 0.996, row sum 1.589; the f32 path, whose
64-term float32 score and 37-term context sums the emulation does not model, reaches o 2.08, dq 1.25, dk 1.23, dv 2.33, P 5.28.

Importing this module needs no GPU; run_case loads the library on first use.
"""
import ctypes as C
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from elem_ref import dropout_keep_ref, inv_keep32
from kernel_ref import DEV, MASK_FILL, SENT, bits_equal

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -23
ABS_FLOOR = 1e-30
DROP_SEED = 0x1234ABCD5678          # both 32-bit halves of the seed take part in the hash

# 4x the measured emulation ratios of the docstring (test_attn_ref_cpu.test_constants_track_the_emulation)
C_BF16 = {"o": 6.5, "dq": 6.0, "dk": 8.1, "dv": 7.1, "P": 4.0, "rowsum": 6.4}
C_F32 = {"o": 3.0, "dq": 2.0, "dk": 1.8, "dv": 2.6, "P": 5.9}
OUTPUTS = ("o", "dq", "dk", "dv", "P")


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    hd: int
    Lq: int
    Lk: int
    fused: bool = True           # the path that must run: fused kernels (0 GEMM launches) or GEMM + softmax (> 0)
    dtype: str = "bf16"
    B: int = 2
    H: int = 2
    mask: str = None             # None | "prefix" | "holes" | "full"
    scale: float = None          # None: hd ** -0.5
    qmul: float = 1.0
    vmul: float = 1.0            # multiplies v and dO
    p: float = 0.0
    strided: bool = False        # q, k, v slices of one [B, L, 3D] buffer; o, dO in [B, L, D + 64]; gradients in a second fused buffer

    @property
    def u(self):
        return U_BF16 if self.dtype == "bf16" else U_F32

    @property
    def consts(self):
        return C_BF16 if self.dtype == "bf16" else C_F32

    @property
    def sharp(self):
        return self.qmul > 1.0


_SHAPES = [  # hd, Lq, Lk, fused, dtype
    (64, 1, 1, True, "bf16"),        # smallest shape
    (64, 128, 128, True, "bf16"),    # one full tile
    (64, 40, 37, True, "bf16"),      # Lk odd, ldP 40
    (64, 129, 64, True, "bf16"),     # general backward, one row into chunk 2
    (64, 130, 100, True, "bf16"),    # general backward, ragged chunk
    (32, 49, 49, True, "bf16"),      # 7x7 image grid
    (32, 7, 128, True, "bf16"),      # few queries
    (32, 130, 33, True, "bf16"),     # ragged in both directions
    (64, 64, 129, True, "bf16"),     # 256-key forward, long backward with one key in block 2
    (64, 130, 200, True, "bf16"),    # long backward, ragged
    (64, 64, 256, True, "bf16"),     # long backward
    (64, 65, 257, True, "bf16"),     # 512-key forward (64-row chunks), one row into chunk 2, one key into block 3
    (64, 130, 384, True, "bf16"),    # 512-key forward, three key blocks
    (64, 70, 512, True, "bf16"),     # 512-key forward, full length
    (16, 40, 37, False, "bf16"),     # fallback: head dim
    (64, 24, 520, False, "bf16"),    # fallback: keys
    (64, 40, 37, False, "f32"),      # fallback: f32 mode
]
_MASKED = [(64, 128, 128), (64, 130, 200), (64, 65, 257), (32, 7, 128)]
_SCALED = [(64, 128, 128), (64, 130, 200)]
_STRIDED = [(64, 40, 40), (64, 130, 130), (32, 49, 49)]
_DROPOUT = [(32, 49, 49, True), (64, 128, 128, True), (64, 130, 200, True), (64, 70, 512, True), (16, 49, 49, False)]


def _cases():
    out = []
    for hd, Lq, Lk, fused, dt in _SHAPES:
        out.append(Case(f"hd{hd}_{Lq}x{Lk}_{dt}", hd, Lq, Lk, fused, dt))
    for hd, Lq, Lk in _MASKED:                       # the unmasked variant is the shape case above
        for m in ("prefix", "holes", "full"):
            B = 3 if (m, Lq, Lk) == ("holes", 130, 200) else 2     # a batch-index slip between b and b + 1 shows
            out.append(Case(f"hd{hd}_{Lq}x{Lk}_{m}", hd, Lq, Lk, mask=m, B=B))
    for hd, Lq, Lk in _SCALED:
        out.append(Case(f"hd{hd}_{Lq}x{Lk}_scale0.3", hd, Lq, Lk, scale=0.3))
        out.append(Case(f"hd{hd}_{Lq}x{Lk}_sharp", hd, Lq, Lk, qmul=8.0))
        out.append(Case(f"hd{hd}_{Lq}x{Lk}_big", hd, Lq, Lk, vmul=100.0))
    for hd, Lq, Lk in _STRIDED:
        out.append(Case(f"hd{hd}_{Lq}x{Lk}_strided", hd, Lq, Lk, strided=True))
    for hd, Lq, Lk, fused in _DROPOUT:
        for p in (0.1, 0.5):
            out.append(Case(f"hd{hd}_{Lq}x{Lk}_p{p}", hd, Lq, Lk, fused, p=p))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def key_mask_of(case):
    """[B, Lk] int64, 0 = masked key"""
    if case.mask is None:
        return None
    m = torch.ones(case.B, case.Lk, dtype=torch.long)
    if case.mask == "prefix":                        # lengths [Lk, 1]
        m[1, 1:] = 0
    elif case.mask == "holes":                       # every third key in batch 0, first and last key in batch 1
        m[0, ::3] = 0
        m[1, 0] = 0
        m[1, -1] = 0
    elif case.mask == "full":                        # batch 1 has no valid key
        m[1, :] = 0
    return m


def keep_mask(seed, B, H, Lq, Lk, p):
    """The dropout mask the kernels must draw: element (b, h, q, key) has flat index row * Lk + key, row = (b * H + h) * Lq + q
    (attn_drop4(seed, prow * a.Lk + key0, ..) in attn_fused.hip, dropout_scale(seed, r * Lk + k, ..) in the softmax kernels)."""
    idx = np.arange(B * H * Lq * Lk, dtype=np.uint64)
    return torch.from_numpy(dropout_keep_ref(seed, idx, p).reshape(B, H, Lq, Lk))


def inputs(case):
    """bf16-rounded q, k, v, dO as float32 [B, L, H * hd], the key mask, the keep mask and the float32 scalars of the call"""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    D = case.H * case.hd

    def rnd(L, mul):
        return (torch.randn(case.B, L, D, generator=g) * mul).bfloat16().float()
    q, k, v, d_o = rnd(case.Lq, case.qmul), rnd(case.Lk, 1.0), rnd(case.Lk, case.vmul), rnd(case.Lq, case.vmul)
    scale = float(np.float32(case.hd ** -0.5 if case.scale is None else case.scale))
    keep = keep_mask(DROP_SEED, case.B, case.H, case.Lq, case.Lk, case.p) if case.p > 0 else None
    ik = float(inv_keep32(case.p)) if case.p > 0 else 1.0
    return dict(q=q, k=k, v=v, d_o=d_o, heads=case.H, scale=scale, key_mask=key_mask_of(case), keep=keep, inv_keep=ik)


# ----------------------------------------------------------------------------------------------------------------------
# reference and emulation
# ----------------------------------------------------------------------------------------------------------------------
AttnRef = namedtuple("AttnRef", "P Pd o dq dk dv S")      # S: the error scales {"o", "dq", "dk", "dv", "P", "rowsum"}


def _split(x, H):
    B, L, D = x.shape
    return x.double().view(B, L, H, D // H).transpose(1, 2)           # [B, H, L, hd]


def _merge(x):
    B, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(B, L, H * hd)


def _softmax(s):
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def _rowsum_scale(P):
    """sqrt of the sum over the DISTINCT values of a row of (count * value)^2: equal probabilities (a fully masked row is
    uniform) round alike, so their errors add linearly; different ones in quadrature"""
    s = P.sort(-1).values
    new = torch.ones_like(s, dtype=torch.long)
    new[..., 1:] = (s[..., 1:] != s[..., :-1]).long()
    groups = torch.zeros_like(s).scatter_add_(-1, new.cumsum(-1) - 1, s)
    return (groups * groups).sum(-1).sqrt()


def attention_ref(q, k, v, d_o, heads, scale, key_mask=None, keep=None, inv_keep=1.0):
    Q, K, V, dO = (_split(t, heads) for t in (q, k, v, d_o))
    s = Q @ K.transpose(-1, -2) * scale
    if key_mask is not None:
        s = s.masked_fill((key_mask == 0)[:, None, None, :], MASK_FILL)
    P = _softmax(s)
    kp = inv_keep if keep is None else keep.double() * inv_keep
    Pd = P * kp
    o = Pd @ V
    dv = Pd.transpose(-1, -2) @ dO
    dP = (dO @ V.transpose(-1, -2)) * kp
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dq = scale * (dS @ K)
    dk = scale * (dS.transpose(-1, -2) @ Q)
    A = P * (dP.abs() + (P * dP.abs()).sum(-1, keepdim=True))
    S = {"o": _merge(Pd @ V.abs()), "dv": _merge(Pd.transpose(-1, -2) @ dO.abs()), "dq": _merge(scale * (A @ K.abs())),
         "dk": _merge(scale * (A.transpose(-1, -2) @ Q.abs())), "P": P, "rowsum": _rowsum_scale(P)}
    return AttnRef(P, Pd, _merge(o), _merge(dq), _merge(dk), _merge(dv), S)


def _to_bf16(x):
    return x.float().bfloat16().double()


def _to_f32(x):
    return x.float().double()


def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


MUTANTS = ("drop_last_key", "drop_last_query_dkdv", "mask_roll", "delta128", "miss_chunk2_dk", "miss_chunk2_dv",
           "no_inv_keep_bwd", "keep_shift", "scale", "trunc_p")


def attention_emulated(q, k, v, d_o, heads, scale, key_mask=None, keep=None, inv_keep=1.0, dtype="bf16", mutant=None):
    """What a correct kernel computes up to float32 effects.  The forward rounds the float32 probabilities once for P and once,
    after the keep-scale, for Pd; the backward reads the stored P and rounds P * keep-scale again for dV (attn_fused.hip).
    mutant: one of MUTANTS, a subtly wrong kernel that the gates must reject."""
    rnd = _to_bf16 if dtype == "bf16" else _to_f32
    rp = _trunc_bf16 if mutant == "trunc_p" else rnd
    Q, K, V, dO = (_split(t, heads) for t in (q, k, v, d_o))
    Lq, Lk = Q.shape[2], K.shape[2]
    if mutant == "scale":
        scale = scale * (1 + 2.0 ** -4)
    if mutant == "mask_roll" and key_mask is not None:
        key_mask = key_mask.roll(1, 0)
    s = _to_f32(Q @ K.transpose(-1, -2) * scale)
    if key_mask is not None:
        s = s.masked_fill((key_mask == 0)[:, None, None, :], MASK_FILL)
    if mutant == "drop_last_key" and Lk > 1:
        s[..., -1] = -float("inf")
    p = _softmax(s)
    kp = torch.ones_like(p) if keep is None else keep.double()
    if mutant == "keep_shift":
        kp = kp.flatten().roll(1).view_as(kp)
    P = rp(p)
    o = rnd(rp(p * kp * inv_keep) @ V)
    ikb = 1.0 if mutant == "no_inv_keep_bwd" else inv_keep
    dP = _to_f32(dO @ V.transpose(-1, -2)) * kp * ikb
    PdP = P * dP
    delta = (PdP[..., :128] if mutant == "delta128" else PdP).sum(-1, keepdim=True)
    dS = rnd(P * (dP - delta))
    Pd = rp(P * kp * ikb)
    dSk, Pdv = dS.clone(), Pd.clone()
    if mutant == "drop_last_query_dkdv":
        dSk[:, :, -1] = 0
        Pdv[:, :, -1] = 0
    if mutant == "miss_chunk2_dk":
        dSk[:, :, 128:256] = 0
    if mutant == "miss_chunk2_dv":
        Pdv[:, :, 128:256] = 0
    dq = rnd(scale * (dS @ K))
    dk = rnd(scale * (dSk.transpose(-1, -2) @ Q))
    dv = rnd(Pdv.transpose(-1, -2) @ dO)
    return AttnRef(P, Pd, _merge(o), _merge(dq), _merge(dk), _merge(dv), None)


# ----------------------------------------------------------------------------------------------------------------------
# gates
# ----------------------------------------------------------------------------------------------------------------------
def ratio_map(got, ref, S, u):
    """per element: the least c at which |got - ref| <= c * u * S + 1e-30 holds (inf where S = 0 and the error is larger)"""
    err = ((got.double() - ref).abs() - ABS_FLOOR).clamp_min(0.0)
    r = err / (u * S).clamp_min(1e-300)
    return torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))


def worst(got, ref, S, u):
    r = ratio_map(got, ref, S, u)
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(x) for x in np.unravel_index(i, tuple(r.shape)))


def gate(got, ref, S, c, u=U_BF16, what=""):
    """assert |got - ref| <= c * u * S + 1e-30 for every element; returns the worst ratio"""
    w, at = worst(got, ref, S, u)
    assert w <= c, (f"{what}: element {at} is off by {w:.3g} x u x S (allowed {c}): got {float(got[at]):.6g}, "
                    f"ref {float(ref[at]):.6g}, S {float(S[at]):.6g}")
    return w


def output_ratios(res, ref, u, rowsum=True):
    """worst ratio and its index per output of res (an AttnRef, or a dict with the same names) against the reference"""
    get = (lambda n: res[n]) if isinstance(res, dict) else (lambda n: getattr(res, n))
    out = {n: worst(get(n), getattr(ref, n), ref.S[n], u) for n in OUTPUTS}
    if rowsum:
        P = get("P").double()
        out["rowsum"] = worst(P.sum(-1), torch.ones_like(ref.S["rowsum"]), ref.S["rowsum"], u)
    return out


def failures(res, ref, case):
    """names of the outputs of res that miss the gates of the case"""
    r = output_ratios(res, ref, case.u, rowsum=case.dtype == "bf16")
    return [n for n, (w, _) in r.items() if not w <= case.consts[n]]


# ----------------------------------------------------------------------------------------------------------------------
# guarded device buffers and the ctypes caller
# ----------------------------------------------------------------------------------------------------------------------
class _Band:
    """a flat device array between two sentinel bands; windows are strided [B, L, D] views of its body"""
    G = 256

    def __init__(self, numel, dtype):
        self.numel = numel
        self.flat = torch.full((numel + 2 * self.G,), SENT, dtype=dtype, device=DEV)
        self.windows = []

    def window(self, B, L, D, bs, ld, offset=0):
        assert offset + (B - 1) * bs + (L - 1) * ld + D <= self.numel
        w = (B, L, D), (bs, ld, 1), self.G + offset
        self.windows.append(w)
        return self.flat.as_strided(*w)

    def outside_untouched(self):
        """every element outside the windows still holds the sentinel"""
        f = self.flat.cpu().clone()
        for w in self.windows:
            f.as_strided(*w).fill_(SENT)
        return bits_equal(f, torch.full_like(f, SENT))

    def untouched(self):
        f = self.flat.cpu()
        return bits_equal(f, torch.full_like(f, SENT))


def _align_up(v, a):
    return (v + a - 1) // a * a


class GemmLaunches:
    """GEMM launches recorded by the GEMM core's profile hook: the score / context products of the unfused path"""

    def __init__(self, lib):
        self.lib = lib
        lib.hs_prof_enable.argtypes = [C.c_int32]
        lib.hs_prof_collect.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]

    def __enter__(self):
        torch.cuda.synchronize()
        self.lib.hs_prof_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        fl, ms, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_int64 * 4)()
        self.lib.hs_prof_collect(fl, ms, cnt)
        self.lib.hs_prof_enable(0)
        self.count = sum(cnt)
        return False


def kernels_of(case):
    """the kernels the routing of attention_fwd_fused / attention_bwd_fused picks for the case"""
    if not case.fused:
        return "GEMM + softmax path", "GEMM + softmax path"
    if case.hd == 32:
        return "attn_fwd_fused_kernel<32>", "attn_bwd_fused_gen_kernel<32>"
    fwd = ("attn_fwd_fused_kernel<64, 512, 1>" if case.Lk > 256 else
           "attn_fwd_fused_kernel<64, 256>" if case.Lk > 128 else "attn_fwd_fused_kernel<64>")
    bwd = ("attn_bwd_fused_long_kernel" if case.Lk > 128 else
           "attn_bwd_fused_kernel" if case.Lq <= 128 else "attn_bwd_fused_gen_kernel<64>")
    return fwd, bwd


def describe(case, B=None, Lk=None, hd=None):
    """(L module, lib, descriptor without strides) for the case; B / Lk / hd override a dimension (the refusal tests)"""
    from hamspine import _lib as L
    d = L.AttnDesc()
    d.dtype = L.HS_BF16 if case.dtype == "bf16" else L.HS_F32
    d.B, d.H, d.Lq = case.B if B is None else B, case.H, case.Lq
    d.Lk, d.hd = case.Lk if Lk is None else Lk, case.hd if hd is None else hd
    d.scale = case.hd ** -0.5 if case.scale is None else case.scale
    d.dropout_p = case.p
    d.seed = DROP_SEED if case.p > 0 else 0
    return L, L.lib(), d


def run_case(case, inp, desc_override=None, check=True):
    """hs_attention_query / _fwd / _bwd on the inputs of the case, every output inside sentinel bands.  Returns o, dq, dk, dv
    ([B, L, D] float64), P and Pd ([B, H, Lq, Lk] float64; Pd None without dropout), the GEMM launches of either call, the
    statuses, and whether anything outside the addressed elements changed."""
    from hamspine import rt
    L, lib, d = describe(case, **(desc_override or {}))
    dt = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    es = 2 if case.dtype == "bf16" else 4
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.H * case.hd
    bands = {}
    if case.strided:
        assert Lq == Lk
        fused_in, grads = _Band(B * Lq * 3 * D, dt), _Band(B * Lq * 3 * D, dt)
        bo, bdo = _Band(B * Lq * (D + 64), dt), _Band(B * Lq * (D + 64), dt)
        wq, wk, wv = (fused_in.window(B, Lq, D, Lq * 3 * D, 3 * D, i * D) for i in range(3))
        wdq, wdk, wdv = (grads.window(B, Lq, D, Lq * 3 * D, 3 * D, i * D) for i in range(3))
        wo, wdo = (b.window(B, Lq, D, Lq * (D + 64), D + 64) for b in (bo, bdo))
        bands.update(grads=grads, o=bo)
    else:
        def own(Lx):
            b = _Band(B * Lx * D, dt)
            return b, b.window(B, Lx, D, Lx * D, D)
        (_, wq), (_, wk), (_, wv), (_, wdo) = own(Lq), own(Lk), own(Lk), own(Lq)
        (bo, wo), (bq, wdq), (bk, wdk), (bv, wdv) = own(Lq), own(Lq), own(Lk), own(Lk)
        bands.update(o=bo, dq=bq, dk=bk, dv=bv)
    for w, name in ((wq, "q"), (wk, "k"), (wv, "v"), (wdo, "d_o")):
        w.copy_(inp[name].to(dt))
    d.q_bs, d.k_bs, d.v_bs, d.o_bs = wq.stride(0), wk.stride(0), wv.stride(0), wo.stride(0)
    d.q_ld, d.k_ld, d.v_ld, d.o_ld = wq.stride(1), wk.stride(1), wv.stride(1), wo.stride(1)
    mask = None if inp["key_mask"] is None else inp["key_mask"].to(DEV).contiguous()
    d.key_mask = rt.p(mask)

    res = {"fwd_gemms": None, "bwd_gemms": None}
    sv, ws = C.c_int64(0), C.c_int64(0)
    res["query_status"] = lib.hs_attention_query(C.byref(d), C.byref(sv), C.byref(ws))
    if check:
        L.check(res["query_status"], "hs_attention_query")
    sv_b, ws_b = max(sv.value, 256), max(ws.value, 256)
    saved = torch.full((sv_b + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    wsbuf = torch.zeros(ws_b, dtype=torch.uint8, device=DEV)
    with GemmLaunches(lib) as f:
        res["fwd_status"] = lib.hs_attention_fwd(C.byref(d), wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), wo.data_ptr(),
                                                 saved.data_ptr(), sv_b, wsbuf.data_ptr(), ws_b, rt.stream())
    res["fwd_gemms"] = f.count
    if check:
        L.check(res["fwd_status"], "hs_attention_fwd")
    with GemmLaunches(lib) as g:
        res["bwd_status"] = lib.hs_attention_bwd(C.byref(d), wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), wdo.data_ptr(),
                                                 wdq.data_ptr(), wdk.data_ptr(), wdv.data_ptr(), saved.data_ptr(), sv_b,
                                                 wsbuf.data_ptr(), ws_b, rt.stream())
    res["bwd_gemms"] = g.count
    if check:
        L.check(res["bwd_status"], "hs_attention_bwd")
    torch.cuda.synchronize()
    res["error"] = lib.hs_last_error().decode("utf-8", "replace")
    for n, w in (("o", wo), ("dq", wdq), ("dk", wdk), ("dv", wdv)):
        res[n] = w.cpu().double()
    res["outside_untouched"] = all(b.outside_untouched() for b in bands.values())
    res["outputs_untouched"] = all(b.untouched() for b in bands.values())
    ldP = _align_up(Lk, 8)
    nP = B * H * Lq * ldP
    sav = saved.cpu()
    res["saved_tail_untouched"] = bool((sav[sv_b:] == 0xA5).all())
    res["saved_untouched"] = bool((sav == 0xA5).all())
    if nP * es <= sv_b:
        P = sav[:nP * es].view(dt).view(B, H, Lq, ldP).double()
        res["P"], res["P_pad"] = P[..., :Lk], P[..., Lk:]
        res["Pd"] = None
        off = _align_up(nP * es, 256)                 # Arena::alloc rounds every allocation up to 256 bytes
        if case.p > 0 and off + nP * es <= sv_b:
            Pd = sav[off:off + nP * es].view(dt).view(B, H, Lq, ldP).double()
            res["Pd"], res["Pd_pad"] = Pd[..., :Lk], Pd[..., Lk:]
    return res
