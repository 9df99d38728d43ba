"""References, yardsticks, inputs and guarded callers for the KAN grid update (csrc/kan_grid.hip; reference
ConNexT/models/block/kan1.py:167-214 update_grid and :112-142 curve2coeff).

  knot_rows        the knot arithmetic of kan1.py:182-211 in float32 with torch CPU operations, in the reference's order
  refit_ref64      the fit in float64: bases in float64 from the float32 inputs, SVD, singular values <= rcond * s_max
                   dropped (rcond = 2^-23 * max(B, nb), torch.linalg.lstsq's default), least-norm solution; returns per
                   feature the condition number, the rank and how far the nearest singular value lies from the cutoff
  lstsq_yard32     torch.linalg.lstsq in float32 on the CPU over the materialised (batch, in, out) tensor: the path the
                   kernels replace, the yardstick of full-rank cases
  pinv_yard32      numpy.linalg.pinv in float32 with the same rcond: the yardstick of rank-deficient cases
  assert_comparable  the input guard: a case is compared only when the reference itself is well away from the cutoff

Importing this module needs no GPU.
"""
import numpy as np
import torch

import kernel_ref as KR

EPS_LSTSQ = 2.0 ** -23           # float32 machine epsilon: torch.linalg.lstsq's rcond is eps * max(m, n)
ATOL, RTOL = 2e-4, 1e-3          # coefficient tolerance of tests/test_product_gpu.py::test_kan_update_grid_matches_reference_vectors


def rcond_of(B, nb):
    return EPS_LSTSQ * max(B, nb)


# --------------------------------------------------------------------------------------------------------------------
# knots
# --------------------------------------------------------------------------------------------------------------------
def knot_rows(x, grid_size, order, grid_eps=0.02, margin=0.01):
    """x (B, in) f32 -> (in, grid_size + 2*order + 1) f32, kan1.py:182-211 operation by operation"""
    x = x.float()
    B = x.shape[0]
    xs = torch.sort(x, dim=0)[0]
    adaptive = xs[torch.linspace(0, B - 1, grid_size + 1, dtype=torch.int64)]
    step = (xs[-1] - xs[0] + 2 * margin) / grid_size
    uniform = torch.arange(grid_size + 1, dtype=torch.float32).unsqueeze(1) * step + xs[0] - margin
    grid = grid_eps * uniform + (1 - grid_eps) * adaptive
    grid = torch.cat([grid[:1] - step * torch.arange(order, 0, -1).unsqueeze(1), grid,
                      grid[-1:] + step * torch.arange(1, order + 1).unsqueeze(1)], dim=0)
    return grid.T.contiguous()


def initial_grid(in_f, grid_size, order, lo=-1.0, hi=1.0):
    """the uniform knots KANLinear starts from"""
    h = (hi - lo) / grid_size
    return ((torch.arange(-order, grid_size + order + 1) * h + lo).expand(in_f, -1).contiguous()).float()


def bases(x, grid, order):
    """Cox-de Boor as kan1.py:77-110 in the dtype of x: x (B, in), grid (in, nk) -> (B, in, nb)"""
    g = grid.to(x.dtype)
    x = x.unsqueeze(-1)
    b = ((x >= g[:, :-1]) & (x < g[:, 1:])).to(x.dtype)
    for k in range(1, order + 1):
        b = (x - g[:, :-(k + 1)]) / (g[:, k:-1] - g[:, :-(k + 1)]) * b[:, :, :-1] \
            + (g[:, k + 1:] - x) / (g[:, k + 1:] - g[:, 1:(-k)]) * b[:, :, 1:]
    return b.contiguous()


# --------------------------------------------------------------------------------------------------------------------
# the fit
# --------------------------------------------------------------------------------------------------------------------
def scaled_coeff(spline_w, scaler):
    """(out, in, nb) f32 * (out, in) f32 in float32, as the reference's scaled_spline_weight"""
    return spline_w.float() * (scaler.float().unsqueeze(-1) if scaler is not None else 1.0)


def targets64(x, grid_old, coeff, order):
    """the materialised (in, B, out) float64 tensor S_i C_i of the old spline outputs per feature"""
    S = bases(x.double(), grid_old, order).permute(1, 0, 2)                     # (in, B, nb)
    return torch.bmm(S, coeff.double().permute(1, 2, 0))                         # (in, B, out)


def refit_ref64(x, grid_new, order, Y):
    """Least-norm least-squares fit per feature in float64.  x (B, in) f32, grid_new (in, nk) f32, Y (in, B, out) float64.
    -> dict: sol (out, in, nb) f64, fitted (in, B, out) f64 = A sol, cond / rank / kept / dropped per feature (kept: smallest
    kept singular value over the cutoff; dropped: largest dropped one over the cutoff, 0 when none), resid = max |A sol - Y|"""
    A = bases(x.double(), grid_new, order).permute(1, 0, 2)                      # (in, B, nb)
    in_f, B, nb = A.shape
    sol = torch.zeros(in_f, nb, Y.shape[2], dtype=torch.float64)
    cond, rank, kept, dropped = [], [], [], []
    for i in range(in_f):
        U, s, Vh = torch.linalg.svd(A[i], full_matrices=False)
        cut = rcond_of(B, nb) * s[0]
        keep = s > cut
        r = int(keep.sum())
        inv = torch.where(keep, 1.0 / s.clamp_min(1e-300), torch.zeros_like(s))
        sol[i] = Vh.T @ (inv[:, None] * (U.T @ Y[i]))
        rank.append(r)
        cond.append(float(s[0] / s[r - 1]) if r else float("inf"))
        kept.append(float(s[r - 1] / cut) if r else 0.0)
        full = torch.cat([s, torch.zeros(nb - s.numel(), dtype=s.dtype)])       # B < nb: the missing values are exact zeros
        dropped.append(float(full[r] / cut) if r < nb else 0.0)
    fitted = torch.bmm(A, sol)
    return {"sol": sol.permute(2, 0, 1).contiguous(), "fitted": fitted, "A": A, "cond": cond, "rank": rank, "kept": kept,
            "dropped": dropped, "resid": float((fitted - Y).abs().max())}


def fitted64(ref, coeff):
    """A sol in float64 for coefficients (out, in, nb) of any float dtype, on the reference's float64 bases"""
    return torch.bmm(ref["A"], coeff.double().permute(1, 2, 0))


def lstsq_yard32(x, grid_new, order, Y32):
    """torch.linalg.lstsq in float32 on the CPU: Y32 (in, B, out) f32 -> (out, in, nb) f32"""
    A = bases(x.float(), grid_new, order).permute(1, 0, 2)
    return torch.linalg.lstsq(A, Y32).solution.permute(2, 0, 1).contiguous()


def pinv_yard32(x, grid_new, order, Y32):
    """numpy.linalg.pinv in float32 with lstsq's rcond"""
    A = bases(x.float(), grid_new, order).permute(1, 0, 2).numpy()
    B, nb = A.shape[1], A.shape[2]
    sol = np.stack([np.linalg.pinv(A[i], rcond=np.float32(rcond_of(B, nb))) @ Y32[i].numpy() for i in range(A.shape[0])])
    return torch.from_numpy(sol.astype(np.float32)).permute(2, 0, 1).contiguous()


def targets32(x, grid_old, coeff, order):
    """the (in, B, out) tensor of the host route in float32"""
    return torch.bmm(bases(x.float(), grid_old, order).permute(1, 0, 2), coeff.float().permute(1, 2, 0))


def assert_comparable(ref, B, nb, full_rank):
    """Every singular value at least 10x away from the cutoff on its side; a gated full-rank case has B >= nb + 1, full rank
    and a condition number of at most 1e5."""
    for i, (k, d, r, c) in enumerate(zip(ref["kept"], ref["dropped"], ref["rank"], ref["cond"])):
        assert k >= 10.0, f"feature {i}: smallest kept singular value only {k:.3g}x the cutoff"
        assert d <= 0.1, f"feature {i}: largest dropped singular value {d:.3g}x the cutoff"
        if full_rank:
            assert B >= nb + 1 and r == nb and c <= 1e5, f"feature {i}: B {B}, rank {r} of {nb}, condition {c:.3g}"


# --------------------------------------------------------------------------------------------------------------------
# inputs.  Seeds and constants are chosen from the float64 reference alone: tests/test_kan_grid_cpu.py asserts the guard for
# every case listed here.
# --------------------------------------------------------------------------------------------------------------------
# (B, in, out, grid_size, order, seed)
FULL_RANK = [(40, 16, 12, 5, 3, 1), (9, 64, 5, 5, 3, 1), (257, 65, 7, 5, 3, 1), (3000, 16, 12, 5, 3, 1),
             (64, 16, 6, 8, 2, 1), (64, 16, 6, 3, 1, 1)]
# name -> (B, in, out, expected rank); all with (grid_size, order) = (5, 3)
RANK_DEFICIENT = {"constant": (50, 16, 12, 1), "two_values": (50, 16, 12, 2), "one_row": (1, 16, 12, 1),
                  "seven_rows": (7, 16, 12, 7)}
KNOT_SHAPES = [(1, 3), (7, 16), (40, 16), (257, 65), (3000, 16), (64, 1)]


def layer_params(in_f, out_f, grid_size, order, g):
    """old knots, unscaled coefficients and scaler of a layer, of the magnitudes KANLinear initialises"""
    nb = grid_size + order
    w = 0.1 * torch.randn(out_f, in_f, nb, generator=g)
    sc = 0.5 + torch.rand(out_f, in_f, generator=g)
    return initial_grid(in_f, grid_size, order), w, sc


def full_rank_case(B, in_f, out_f, grid_size, order, seed):
    g = KR.gen(seed)
    x = torch.randn(B, in_f, generator=g) * 0.9
    return (x,) + layer_params(in_f, out_f, grid_size, order, g)


def deficient_case(name):
    B, in_f, out_f, _ = RANK_DEFICIENT[name]
    g = KR.gen(1)
    if name == "constant":
        x = (torch.rand(in_f, generator=g) * 1.6 - 0.8).expand(B, in_f).contiguous()
    elif name == "two_values":
        a = torch.rand(in_f, generator=g) * 0.7 - 0.8                      # in [-0.8, -0.1]
        b = torch.rand(in_f, generator=g) * 0.7 + 0.1                      # in [0.1, 0.8]
        pick = torch.rand(B, in_f, generator=g) < 0.4
        pick[0], pick[1] = False, True                                     # both values occur in every column
        x = torch.where(pick, b.expand(B, in_f), a.expand(B, in_f)).contiguous()
    else:
        x = torch.randn(B, in_f, generator=g) * 0.9
    return (x,) + layer_params(in_f, out_f, 5, 3, g)


def knot_input(B, in_f, seed=1):
    return torch.randn(B, in_f, generator=KR.gen(seed)) * 0.9


def ties_input():
    """40 rows of values drawn from five levels (every selected rank falls inside a run of equal values), and a column of
    mixed +0.0 / -0.0 with a few other values"""
    g = KR.gen(3)
    x = (torch.randint(-2, 3, (40, 16), generator=g).float() * 0.25)
    z = torch.zeros(40)
    z[::2] = -0.0
    z[5], z[17], z[30] = -0.5, 0.75, 0.25
    x[:, 3] = z
    return x


# --------------------------------------------------------------------------------------------------------------------
# the layer's forward around an update (test "layer output preserved")
# --------------------------------------------------------------------------------------------------------------------
def forward_rounding(x, grid, order, coeff, base_w):
    """A-priori float32 rounding bound of one KANLinear forward, max over the outputs: the GEMM adds Kc = in * (1 + nb) products
    in float32 (at most Kc + 1 roundings on the sum of the magnitudes), each basis value carries the roundings of its
    recursion (3 operations per term and level, two terms: 6 * order + 2 on its own magnitude) and the activation a few ulps
    (8): EPS32 * (Kc + 6 * order + 11) * sum_k |feature_k| |weight_k|."""
    xd = x.double()
    S = bases(xd, grid, order).abs()                                              # (B, in, nb)
    mag = torch.einsum("bip,oip->bo", S, coeff.double().abs()) + torch.nn.functional.silu(xd).abs() @ base_w.double().abs().T
    Kc = x.shape[1] * (1 + S.shape[2])
    return float(KR.EPS32 * (Kc + 6 * order + 11) * mag.max())


# --------------------------------------------------------------------------------------------------------------------
# guarded callers (GPU)
# --------------------------------------------------------------------------------------------------------------------
def ranks_of(B, grid_size):
    return torch.linspace(0, B - 1, grid_size + 1, dtype=torch.int64)


def call_knots(x, grid_size, order, grid_eps=0.02, margin=0.01, B=None, ranks=None, null=(), ws_bytes=0, check=True):
    """hs_kan_grid_knots on x (B, in) -> {"grid": (in, nk), status, guards, untouched}.  null: names of pointers to pass as
    NULL; B / ranks / ws_bytes: overrides of the stated values (the allocations stay whole)."""
    L, lib, rt = KR._env()
    rows, in_f = x.shape
    nk = max(grid_size + 2 * order + 1, 1)
    xd = KR._fresh(x.float())
    r = ranks_of(rows, max(grid_size, 1)) if ranks is None else ranks
    bufs = {"grid": KR.GBuf(in_f, nk, torch.float32)}
    st = lib.hs_kan_grid_knots(None if "x" in null else KR._p(xd), None if "ranks" in null else r.data_ptr(),
                               None if "grid" in null else KR._p(bufs["grid"]), rows if B is None else B, in_f, grid_size, order,
                               grid_eps, 1 - grid_eps, margin, None, ws_bytes, rt.stream())
    return KR._finish(L, st, "hs_kan_grid_knots", bufs, check)


def call_refit(x, grid_new, grid_size, order, grid_old=None, spline_w=None, scaler=None, y=None, out_f=None, in_place=False,
               B=None, null=(), ws_short=0, check=True):
    """hs_kan_refit -> {"out": (out * in, nb), ...}.  S-mode: grid_old, spline_w (scaler optional); y-mode: y (B, in, out).
    in_place: the output aliases spline_w (a guarded buffer preloaded with it)."""
    L, lib, rt = KR._env()
    rows, in_f = x.shape
    nb = max(grid_size + order, 1)
    out_f = out_f or (spline_w.shape[0] if spline_w is not None else y.shape[2])
    xd, gn, go, wd, sd, yd = (KR._fresh(t.float() if t is not None else None) for t in (x, grid_new, grid_old, spline_w, scaler, y))
    bufs = {"out": KR.GBuf(out_f * in_f, nb, torch.float32)}
    if in_place:
        bufs["out"].t.copy_(wd.view(out_f * in_f, nb))
        wd = bufs["out"].t
    full = int(lib.hs_kan_refit_ws_bytes(rows, in_f, out_f, grid_size, order, 1 if y is not None else 0))
    ws = KR._wsbuf(max(full, 0))
    st = lib.hs_kan_refit(None if "x" in null else KR._p(xd), None if "grid_new" in null else KR._p(gn), KR._p(go), KR._p(yd),
                          KR._p(wd), KR._p(sd), None if "out" in null else KR._p(bufs["out"]), rows if B is None else B, in_f, out_f,
                          grid_size, order, None if "ws" in null else KR._p(ws), max(full, 0) - ws_short, rt.stream())
    return KR._finish(L, st, "hs_kan_refit", bufs, check)
