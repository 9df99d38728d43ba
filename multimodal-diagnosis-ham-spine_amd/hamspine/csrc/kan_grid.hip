// KAN grid update on the device (gfx950 / CDNA4 only): KANLinear.update_grid and curve2coeff of reference
// ConNexT/models/block/kan1.py:167-214 and :112-142, without the (batch, in, out) tensor, torch.sort or a vendor solver.
//
//   knots    per feature, the order statistics of its column of x at given ranks (a bitwise radix select on the
//            order-preserving integer image of the floats: 32 counting passes, integer counts, no sort), its minimum and
//            maximum, and the blended, extended knot row in the reference's f32 arithmetic (every operation rounded alone)
//   accum    per (feature, chunk of 256 rows): the Gram matrix A^T A and the right-hand side A^T S (or A^T Y) of the
//            chunk in f64, written to the chunk's own slot of the workspace.  A = bases of x on the new knots,
//            S = bases on the old knots, both from the forward's bspline_eval
//   solve    per feature: the slots added in chunk order, a cyclic Jacobi eigen-decomposition of the Gram matrix in f64
//            with a fixed maximum of sweeps, eigenvalues <= rcond^2 * lambda_max dropped (rcond = 2^-23 * max(B, nb), the
//            default cutoff of torch.linalg.lstsq on the singular values), M = V diag(1/lambda) V^T (A^T S), and
//            out[o, i, :] = M (spline_weight[o, i, :] * spline_scaler[o, i])
//
// Nothing is atomic; every sum has one order that depends on the shapes alone, so a rerun repeats bitwise.  The least-squares
// solution of a rank-deficient feature is the truncated pseudo-inverse (least-norm) one.
#include <algorithm>
#include <math.h>
#include "hs_internal.h"

namespace hs {
namespace {

constexpr int KG_FT = 16;      // knots: features per workgroup (consecutive lanes = consecutive features: coalesced rows)
constexpr int KG_RS = 16;      // knots: row slices per workgroup (thread = one feature of one slice)
constexpr int KG_Q = 8;        // knots: ranks resolved together by one group of 32 counting passes
constexpr int KG_ROWS = 256;   // refit: rows per chunk (one workgroup, one workspace slot)
constexpr int KG_MAXNB = KAN_MAXK - 1;   // coefficients per feature: nb = nk - 1 - order <= 31
constexpr int KG_SWEEPS = 24;  // Jacobi: sweeps at most (f64, nb <= 31 converges in 6..10; nothing can make it spin)

struct KnotRanks {
    long long r[KAN_MAXK];     // grid_size + 1 <= 32 ranks (0-based positions in the sorted column)
};

// order-preserving integer image of a float: -0.0 is +0.0 (equal values), every NaN sorts last as torch.sort puts it
__device__ __forceinline__ unsigned key_of(float v) {
    unsigned b = __float_as_uint(v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// grid: (in_f, nk) knot rows, nk = G + 2 * order + 1
__global__ __launch_bounds__(KG_FT * KG_RS) void kan_knots_kernel(const float* __restrict__ x, const KnotRanks ranks,
                                                                 float* __restrict__ grid, long long B, int in_f, int G, int order,
                                                                 float eps, float one_minus_eps, float margin) {
    __shared__ unsigned cnt[KG_RS][KG_Q][KG_FT];
    __shared__ unsigned sel[KAN_MAXK][KG_FT];
    __shared__ unsigned ext[2][KG_RS][KG_FT];
    const int f = threadIdx.x % KG_FT, rs = threadIdx.x / KG_FT;
    const int feat = blockIdx.x * KG_FT + f;
    const bool live = feat < in_f;
    const float* col = x + (live ? feat : 0);
    const long long first = live ? rs : B;          // a lane past the last feature reads nothing and counts nothing

    // minimum and maximum of the column
    unsigned lo = 0xffffffffu, hi = 0u;
    for (long long r = first; r < B; r += KG_RS) {
        const unsigned k = key_of(col[r * in_f]);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    ext[0][rs][f] = lo;
    ext[1][rs][f] = hi;

    // the ranks, KG_Q at a time: prefix = the largest v with #(key < v) <= rank, built from the top bit down
    for (int q0 = 0; q0 <= G; q0 += KG_Q) {
        unsigned prefix[KG_Q];
        long long rank[KG_Q];
#pragma unroll
        for (int j = 0; j < KG_Q; ++j) {
            prefix[j] = 0u;
            rank[j] = ranks.r[q0 + j <= G ? q0 + j : G];
        }
        for (int bit = 31; bit >= 0; --bit) {
            unsigned cand[KG_Q], c[KG_Q];
#pragma unroll
            for (int j = 0; j < KG_Q; ++j) {
                cand[j] = prefix[j] | (1u << bit);
                c[j] = 0u;
            }
#pragma unroll 4
            for (long long r = first; r < B; r += KG_RS) {
                const unsigned k = key_of(col[r * in_f]);
#pragma unroll
                for (int j = 0; j < KG_Q; ++j) c[j] += k < cand[j] ? 1u : 0u;
            }
#pragma unroll
            for (int j = 0; j < KG_Q; ++j) cnt[rs][j][f] = c[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KG_Q; ++j) {
                long long total = 0;
                for (int s = 0; s < KG_RS; ++s) total += cnt[s][j][f];
                if (total <= rank[j]) prefix[j] = cand[j];
            }
            __syncthreads();
        }
        if (rs == 0) {
#pragma unroll
            for (int j = 0; j < KG_Q; ++j)
                if (q0 + j <= G) sel[q0 + j][f] = prefix[j];
        }
    }
    __syncthreads();
    if (rs != 0 || !live) return;

    for (int s = 0; s < KG_RS; ++s) {
        lo = ext[0][s][f] < lo ? ext[0][s][f] : lo;
        hi = ext[1][s][f] > hi ? ext[1][s][f] : hi;
    }
    // kan1.py:189-211 in f32, one rounding per operation, in the reference's order.  Plain operators under contract(off): the
    // bodies of __fmul_rn / __fadd_rn are compiled outside this block's pragma and would carry the translation unit's
    // contraction into it once inlined.  The division is the correctly rounded one (hipcc's default for f32).
    {
#pragma clang fp contract(off)
        const float mn = float_of(lo), mx = float_of(hi);
        const float span = mx - mn;
        const float step = (span + 2.f * margin) / (float)G;
        const int nk = G + 2 * order + 1;
        float* g = grid + (long long)feat * nk;
        float g0 = 0.f, gG = 0.f;
        for (int j = 0; j <= G; ++j) {
            const float js = (float)j * step;
            const float uniform = (js + mn) - margin;
            const float eu = eps * uniform, ea = one_minus_eps * float_of(sel[j][f]);
            const float v = eu + ea;
            g[order + j] = v;
            if (j == 0) g0 = v;
            if (j == G) gG = v;
        }
        for (int m = 1; m <= order; ++m) {
            const float sm = step * (float)m;
            g[order - m] = g0 - sm;
            g[order + G + m] = gG + sm;
        }
    }
}

// One workgroup = feature i, rows [chunk * KG_ROWS, +KG_ROWS).  slot = partial + (chunk * in_f + i) * ne holds, in f64,
//   [0, nb^2)            G[p][q] = sum_r A[r][p] A[r][q]
//   [nb^2, nb^2 + nb*nc) R[p][q] = sum_r A[r][p] S[r][q] (nc = nb)  or  sum_r A[r][p] y[r][i][q] (nc = out_f)
// each as one sequential sum over the chunk's rows.
__global__ __launch_bounds__(KG_ROWS) void kan_refit_accum_kernel(const float* __restrict__ x, const float* __restrict__ grid_new,
                                                                 const float* __restrict__ grid_old, const float* __restrict__ y,
                                                                 double* __restrict__ partial, long long B, int in_f, int out_f,
                                                                 int nk, int order) {
    extern __shared__ float bases[];               // A[KG_ROWS][nb], then S[KG_ROWS][nb]
    const int nb = nk - 1 - order;
    const int i = (int)(blockIdx.x % (unsigned)in_f);
    const long long chunk = blockIdx.x / (unsigned)in_f;
    const long long row0 = chunk * KG_ROWS;
    const int nr = (int)(B - row0 < KG_ROWS ? B - row0 : KG_ROWS);
    float* A = bases;
    float* S = bases + KG_ROWS * nb;
    const int t = threadIdx.x;
    if (t < nr) {
        const float xv = x[(row0 + t) * in_f + i];
        float Bv[KAN_MAXK], dBv[KAN_MAXK];
        bspline_eval(xv, grid_new + (long long)i * nk, nk, order, Bv, dBv);
        for (int j = 0; j < nb; ++j) A[t * nb + j] = Bv[j];
        if (grid_old) {
            bspline_eval(xv, grid_old + (long long)i * nk, nk, order, Bv, dBv);
            for (int j = 0; j < nb; ++j) S[t * nb + j] = Bv[j];
        }
    }
    __syncthreads();
    const int nc = grid_old ? nb : out_f;
    const long long ne = (long long)nb * (nb + nc);
    double* slot = partial + ((long long)chunk * in_f + i) * ne;
    for (long long e = t; e < ne; e += KG_ROWS) {
        double acc = 0.0;
        if (e < nb * nb) {
            const int p = (int)e / nb, q = (int)e % nb;
            for (int r = 0; r < nr; ++r) acc = fma((double)A[r * nb + p], (double)A[r * nb + q], acc);
        } else {
            const long long e2 = e - nb * nb;
            const int p = (int)(e2 / nc), q = (int)(e2 % nc);
            if (grid_old) {
                for (int r = 0; r < nr; ++r) acc = fma((double)A[r * nb + p], (double)S[r * nb + q], acc);
            } else {
                const float* yc = y + ((row0 * in_f + i) * out_f + q);
                const long long pitch = (long long)in_f * out_f;
                for (int r = 0; r < nr; ++r) acc = fma((double)A[r * nb + p], (double)yc[r * pitch], acc);
            }
        }
        slot[e] = acc;
    }
}

// One wave = feature i.  out may alias spline_w: a thread reads all of spline_w[o][i][:] before it writes out[o][i][:], and no
// other thread touches that row.
__global__ __launch_bounds__(64) void kan_refit_solve_kernel(const double* __restrict__ partial, long long nchunk,
                                                            const float* spline_w, const float* __restrict__ scaler, float* out,
                                                            long long B, int in_f, int out_f, int nb, int ymode) {
    __shared__ double Am[KG_MAXNB * KG_MAXNB], Vm[KG_MAXNB * KG_MAXNB], Rm[KG_MAXNB * KG_MAXNB], Pm[KG_MAXNB * KG_MAXNB];
    __shared__ double inv[KG_MAXNB + 1];
    __shared__ double vec[64 * KG_MAXNB];          // a thread's own row: odd pitch in doubles, no bank conflict
    const int i = blockIdx.x, t = threadIdx.x;
    const int n2 = nb * nb;
    const int nc = ymode ? out_f : nb;
    const long long ne = (long long)nb * (nb + nc);
    const double* slot0 = partial + (long long)i * ne;
    const long long pitch = (long long)in_f * ne;   // from one chunk's slot of this feature to the next

    // the chunks' sums, added in chunk order
    for (int e = t; e < (ymode ? n2 : 2 * n2); e += 64) {
        double s = 0.0;
        for (long long c = 0; c < nchunk; ++c) s += slot0[c * pitch + e];
        if (e < n2) {
            Am[e] = s;
            Vm[e] = (e / nb == e % nb) ? 1.0 : 0.0;
        } else {
            Rm[e - n2] = s;
        }
    }
    __syncthreads();

    // cyclic Jacobi: A = V diag(lambda) V^T.  Every thread takes the same decisions from the same LDS words.
    for (int sweep = 0; sweep < KG_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < nb - 1; ++p) {
            for (int q = p + 1; q < nb; ++q) {
                const double app = Am[p * nb + p], aqq = Am[q * nb + q], apq = Am[p * nb + q];
                const bool rot = apq != 0.0 && fabs(apq) > 0x1p-53 * sqrt(fabs(app) * fabs(aqq));   // false for a NaN
                __syncthreads();
                if (!rot) continue;
                ++rotated;
                const double theta = (aqq - app) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                if (t < nb) {
                    if (t == p) {
                        Am[p * nb + p] = app - tt * apq;
                        Am[q * nb + q] = aqq + tt * apq;
                        Am[p * nb + q] = 0.0;
                        Am[q * nb + p] = 0.0;
                    } else if (t != q) {
                        const double akp = Am[t * nb + p], akq = Am[t * nb + q];
                        const double np = c * akp - s * akq, nq = s * akp + c * akq;
                        Am[t * nb + p] = np;
                        Am[p * nb + t] = np;
                        Am[t * nb + q] = nq;
                        Am[q * nb + t] = nq;
                    }
                    const double vkp = Vm[t * nb + p], vkq = Vm[t * nb + q];
                    Vm[t * nb + p] = c * vkp - s * vkq;
                    Vm[t * nb + q] = s * vkp + c * vkq;
                }
                __syncthreads();
            }
        }
        if (!rotated) break;
    }
    __syncthreads();

    // truncated inverse of the spectrum
    double lmax = 0.0;
    for (int k = 0; k < nb; ++k) {
        const double l = Am[k * nb + k];
        lmax = l > lmax ? l : lmax;
    }
    const double rcond = 0x1p-23 * (double)(B > nb ? B : (long long)nb);
    const double cutoff = rcond * rcond * lmax;
    if (t < nb) {
        const double l = Am[t * nb + t];
        inv[t] = (l > cutoff && l > 0.0) ? 1.0 / l : 0.0;
    }
    __syncthreads();
    for (int e = t; e < n2; e += 64) {
        const int p = e / nb, q = e % nb;
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s = fma(Vm[p * nb + k] * inv[k], Vm[q * nb + k], s);
        Pm[e] = s;
    }
    __syncthreads();
    double* Mm = Pm;                               // y-mode: the solution is P (A^T Y)
    if (!ymode) {                                  // S-mode: M = P (A^T S), into Am (the spectrum is no longer needed)
        for (int e = t; e < n2; e += 64) {
            const int p = e / nb, q = e % nb;
            double s = 0.0;
            for (int k = 0; k < nb; ++k) s = fma(Pm[p * nb + k], Rm[k * nb + q], s);
            Am[e] = s;
        }
        Mm = Am;
        __syncthreads();
    }

    double* mine = vec + t * KG_MAXNB;
    for (int o0 = 0; o0 < out_f; o0 += 64) {
        const int o = o0 + t;
        if (o >= out_f) break;
        const long long at = ((long long)o * in_f + i) * nb;
        if (ymode) {
            for (int q = 0; q < nb; ++q) {
                double s = 0.0;
                for (long long c = 0; c < nchunk; ++c) s += slot0[c * pitch + n2 + (long long)q * out_f + o];
                mine[q] = s;
            }
        } else {
            const float sc = scaler ? scaler[(long long)o * in_f + i] : 1.f;
            for (int q = 0; q < nb; ++q) mine[q] = (double)__fmul_rn(spline_w[at + q], sc);
        }
        for (int p = 0; p < nb; ++p) {
            double s = 0.0;
            for (int q = 0; q < nb; ++q) s = fma(Mm[p * nb + q], mine[q], s);
            out[at + p] = (float)s;
        }
    }
}

// nk, nb of a supported (grid_size, order), or false
bool knot_counts(int grid_size, int order, int& nk, int& nb) {
    if (grid_size < 1 || order < 0 || grid_size > KAN_MAXK || order > KAN_MAXK) return false;
    nk = grid_size + 2 * order + 1;
    nb = grid_size + order;
    return nk <= KAN_MAXK;
}

long long refit_chunks(long long B) { return (B + KG_ROWS - 1) / KG_ROWS; }

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

int64_t hs_kan_grid_knots_ws_bytes(int64_t B, int32_t in_f, int32_t grid_size, int32_t order) {
    int nk, nb;
    if (B < 1 || in_f < 1 || !knot_counts(grid_size, order, nk, nb)) return -1;
    return 0;                                      // the selection keeps its counters in LDS
}

hs_status hs_kan_grid_knots(const float* x, const int64_t* ranks, float* grid, int64_t B, int32_t in_f, int32_t grid_size,
                            int32_t order, float grid_eps, float one_minus_eps, float margin, void* ws, int64_t ws_bytes,
                            void* stream) {
    (void)ws;
    HS_REQUIRE(x && ranks && grid, "kan_grid_knots: NULL pointer (x %p, ranks %p, grid %p)", (const void*)x, (const void*)ranks,
               (const void*)grid);
    HS_REQUIRE(B >= 1, "kan_grid_knots: B = %lld < 1", (long long)B);
    HS_REQUIRE(in_f >= 1, "kan_grid_knots: in_f = %d < 1", in_f);
    int nk, nb;
    HS_REQUIRE(knot_counts(grid_size, order, nk, nb), "kan_grid_knots: unsupported knot count: grid_size %d, order %d (need "
               "grid_size >= 1, order >= 0, grid_size + 2*order + 1 <= %d)", grid_size, order, KAN_MAXK);
    HS_REQUIRE(ws_bytes >= hs_kan_grid_knots_ws_bytes(B, in_f, grid_size, order), "kan_grid_knots: workspace of %lld bytes is short of %lld",
               (long long)ws_bytes, (long long)hs_kan_grid_knots_ws_bytes(B, in_f, grid_size, order));
    KnotRanks kr;
    memset(&kr, 0, sizeof(kr));
    for (int j = 0; j <= grid_size; ++j) {
        HS_REQUIRE(ranks[j] >= 0 && ranks[j] < B, "kan_grid_knots: ranks[%d] = %lld outside [0, B = %lld)", j, (long long)ranks[j],
                   (long long)B);
        kr.r[j] = ranks[j];
    }
    hipLaunchKernelGGL(kan_knots_kernel, dim3((unsigned)ceil_div(in_f, KG_FT)), dim3(KG_FT * KG_RS), 0, (hipStream_t)stream, x, kr, grid,
                       (long long)B, in_f, grid_size, order, grid_eps, one_minus_eps, margin);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int64_t hs_kan_refit_ws_bytes(int64_t B, int32_t in_f, int32_t out_f, int32_t grid_size, int32_t order, int32_t y_mode) {
    int nk, nb;
    if (B < 1 || in_f < 1 || out_f < 1 || !knot_counts(grid_size, order, nk, nb)) return -1;
    const long long ne = (long long)nb * (nb + (y_mode ? out_f : nb));
    return refit_chunks(B) * in_f * ne * (long long)sizeof(double);
}

hs_status hs_kan_refit(const float* x, const float* grid_new, const float* grid_old, const float* y, const float* spline_w,
                       const float* scaler, float* out, int64_t B, int32_t in_f, int32_t out_f, int32_t grid_size, int32_t order,
                       void* ws, int64_t ws_bytes, void* stream) {
    HS_REQUIRE(x && grid_new && out && ws, "kan_refit: NULL pointer (x %p, grid_new %p, out %p, ws %p)", (const void*)x,
               (const void*)grid_new, (const void*)out, ws);
    HS_REQUIRE(B >= 1, "kan_refit: B = %lld < 1", (long long)B);
    HS_REQUIRE(in_f >= 1 && out_f >= 1, "kan_refit: in_f = %d, out_f = %d must be positive", in_f, out_f);
    int nk, nb;
    HS_REQUIRE(knot_counts(grid_size, order, nk, nb), "kan_refit: unsupported knot count: grid_size %d, order %d (need "
               "grid_size >= 1, order >= 0, grid_size + 2*order + 1 <= %d)", grid_size, order, KAN_MAXK);
    const bool smode = grid_old || spline_w, ymode = y != nullptr;
    HS_REQUIRE(smode != ymode, "kan_refit: %s of S-mode (grid_old, spline_w) and y-mode (y) given, need exactly one",
               smode ? "both" : "neither");
    HS_REQUIRE(!smode || (grid_old && spline_w), "kan_refit: S-mode needs grid_old and spline_w");
    const long long need = hs_kan_refit_ws_bytes(B, in_f, out_f, grid_size, order, ymode ? 1 : 0);
    HS_REQUIRE(ws_bytes >= need, "kan_refit: workspace of %lld bytes is short of %lld", (long long)ws_bytes, need);
    HS_REQUIRE(((uintptr_t)ws & 7) == 0, "kan_refit: workspace is not 8-byte aligned");
    const long long nchunk = refit_chunks(B);
    HS_REQUIRE(nchunk * in_f <= 0x7fffffffll, "kan_refit: %lld row chunks x %d features exceed the grid", nchunk, in_f);
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)KG_ROWS * nb * sizeof(float) * (smode ? 2 : 1);
    hipLaunchKernelGGL(kan_refit_accum_kernel, dim3((unsigned)(nchunk * in_f)), dim3(KG_ROWS), lds, s, x, grid_new, grid_old, y,
                       (double*)ws, (long long)B, in_f, out_f, nk, order);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(kan_refit_solve_kernel, dim3((unsigned)in_f), dim3(64), 0, s, (const double*)ws, nchunk, spline_w, scaler, out,
                       (long long)B, in_f, out_f, nb, ymode ? 1 : 0);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
