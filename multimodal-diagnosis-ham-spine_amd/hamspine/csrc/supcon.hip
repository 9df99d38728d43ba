// SupCon loss over any batch size, tiled on the f32-input MFMA (gfx950 / CDNA4 only).  The loss is SupConLoss of the reference
// (scripts/train.py:23-44) over all N rows; the gradient is written for the rows [row0, row0 + M) the caller owns, so that W
// ranks that have gathered the step's N = W * B rows each produce their own rows of the gradient of the GLOBAL loss.
//
//   normalise   one wave per row: nrm_i = max(|f_i|, 1e-12), fn_i = f_i / nrm_i, zero-padded to Dp = 4 * ceil(D / 4) columns
//               (the MFMA's k-step).  The only copy of the features.
//   stats       workgroup (64 anchors, key split z) walks its key tiles j0 = 64 (z tps), ... in order.  S = Fn_a Fn_k^T of a
//               64 x 64 tile comes from mfma_f32_16x16x4f32 (each wave: 16 anchors x 64 keys, four accumulators); running
//               maximum and sum of exponentials are rescaled per tile (online softmax).  Also per anchor the positive count
//               P_i and the positives' logit sum.
//   merge       (only with more than one key split) per row, the splits' (mx, E, sum, count) in split order, rescaled once more.
//               The 1e-8 joins E after the last rescale.  Writes (mx, E, P, w = 1 / (N (P + 1e-8)), loss_i / N).
//   finish      one workgroup adds the N per-anchor losses in f64 in a fixed order.
//   grad        workgroup (64 owned anchors, 256 columns of D, key split z): per key tile S is recomputed, C_ik = G_ik + G_ki is
//               formed from s_ik (= s_ki bitwise: the products commute and the k order is the same) and the statistics of rows
//               i and k, goes through LDS into the A operand of a second MFMA product C x Fn (k = the key index), which
//               accumulates d fn_i over the split's keys in one chain.  The projection through the normalisation needs
//               g_i . fn_i, which is sum_k C_ik s_ik: every column slice computes it from the tiles it has anyway, so no slice
//               waits for another.
//   project     (only with more than one key split) adds the splits' partial d fn_i and dots in split order and projects.
//
// Key splits: a workgroup per 64 anchors alone leaves most of the 256 CUs idle up to several thousand rows, so the keys are cut
// into KS = key_splits(N) contiguous runs of tps tiles (about 512 workgroups per pass; 1 for N <= 64 and for N > 32768).  KS
// depends on N alone, never on the rows a call owns.
//
// No N x N array exists anywhere; nothing is atomic; every sum has one order that depends on (N, D) alone, and the chain of an
// output element does not depend on where its anchor sits in a tile, so a rerun and a sliced call repeat bitwise.
//
// Rounding depth: s_ij is one fma chain of Dp terms in k order (the instruction is an exact k-ordered f32 fma chain), d fn_i[d]
// one fma chain of at most 64 tps terms in key order per split, then KS - 1 additions.  Row sums of a tile: 4 sequential adds in
// the lane, a 4-level xor tree over the 16 lanes of the row, then one add per tile and one per split: tps + KS + 8 deep.
#include <math.h>
#include "hs_common.h"

namespace hs {
namespace {

constexpr int TM = 64;          // anchors per workgroup = keys per tile
constexpr int KC = 32;          // columns of Fn staged per step of the S product
constexpr int LDK = KC + 4;     // 36: lane (row l & 15, k l >> 4) -> bank 36 row + k, 64 distinct banks; rows stay 16-byte aligned
constexpr int LDC = TM + 4;     // 68: the same map for the C tile as A operand
constexpr int DS = 256;         // columns of D per workgroup of the gradient pass (16 accumulator tiles per wave)
constexpr int DC = 64;          // columns of Fn staged per step of the C x Fn product
constexpr int LDD = DC + 16;    // 80: lane (key l >> 4, column l & 15) -> bank 16 key + column, 64 distinct banks
constexpr int NSTAT = 6;        // per-row floats behind fn: nrm, mx, E, P, w, row loss
constexpr int KS_MAX = 16;      // key splits at most
constexpr int KS_GRID = 512;    // workgroups per pass the splits aim at

__host__ __device__ inline int pad4(int D) { return (D + 3) & ~3; }

// key tiles per split and the number of splits, from N alone
inline void key_splits(int N, int& tps, int& KS) {
    const int NT = (N + TM - 1) / TM;
    int want = (KS_GRID + NT - 1) / NT;
    want = want < 1 ? 1 : want > KS_MAX ? KS_MAX : want;
    if (want > NT) want = NT;
    tps = (NT + want - 1) / want;
    KS = (NT + tps - 1) / tps;            // no empty split
}

// sums / maxima over the 16 lanes that hold one row of a 16 x 16 accumulator tile (lanes that differ in l & 15)
__device__ __forceinline__ float row_sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float row_max16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void supcon_normalise_kernel(const float* __restrict__ f, int N, int D, int Dp,
                                                               float* __restrict__ fn, float* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const float* row = f + (long long)i * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += row[d] * row[d];
    s = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    if (lane == 0) nrm[i] = s;
    float* out = fn + (long long)i * Dp;
    for (int d = lane; d < Dp; d += 64) out[d] = d < D ? row[d] / s : 0.f;
}

// dst[64][LDK] = fn[r0 .. r0 + 63][k0 .. k0 + 31]; rows from rend on and columns from Dp on are 0
__device__ __forceinline__ void stage_k(const float* __restrict__ fn, int Dp, int r0, int rend, int k0, float* dst) {
#pragma unroll
    for (int v = threadIdx.x; v < TM * KC / 4; v += 256) {
        const int r = v >> 3, c = (v & 7) * 4;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < rend && k0 + c < Dp) x = *(const f32x4*)(fn + (long long)(r0 + r) * Dp + k0 + c);
        *(f32x4*)(dst + r * LDK + c) = x;
    }
}

// acc[t][r] = fn_i . fn_j for i = a0 + 16 wave + 4 (lane >> 4) + r and j = j0 + 16 t + (lane & 15): one fma chain over k = 0 .. Dp-1
__device__ __forceinline__ void s_tile(const float* __restrict__ fn, int Dp, int a0, int aend, int j0, int N, float* As, float* Bs,
                                       f32x4 acc[4]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int arow = (wv * 16 + (lane & 15)) * LDK + (lane >> 4);
    const int brow = (lane & 15) * LDK + (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Dp; k0 += KC) {
        __syncthreads();
        stage_k(fn, Dp, a0, aend, k0, As);
        stage_k(fn, Dp, j0, N, k0, Bs);
        __syncthreads();
        const int steps = (Dp - k0 < KC ? Dp - k0 : KC) >> 2;
        for (int kk = 0; kk < steps; ++kk) {
            const float a = As[arow + kk * 4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float b = Bs[brow + t * 16 * LDK + kk * 4];
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
            }
        }
    }
}

struct RowStats {
    float *mx, *E, *P, *w, *rowloss;      // [N] each
};

// row i from its merged (mx, E without the 1e-8, logit sum and count of the positives)
__device__ __forceinline__ void stats_finalize(const RowStats& o, int i, int N, float mx, float E, float ps, float pc) {
    const float Ei = 1e-8f + E;
    const float msum = ps - pc * (mx + __logf(Ei));       // sum over positives of s_ij - mx_i - log E_i
    o.mx[i] = mx;
    o.E[i] = Ei;
    o.P[i] = pc;
    o.w[i] = 1.f / ((float)N * (pc + 1e-8f));
    o.rowloss[i] = -msum / (pc + 1e-8f) / (float)N;
}

// grid (anchor tiles, key splits).  part (only with more than one split): [4][KS][N] = mx, E, logit sum, count of every split
__global__ __launch_bounds__(256) void supcon_stats_kernel(const float* __restrict__ fn, const long long* __restrict__ lab, int N,
                                                           int Dp, float T, int tps, RowStats o, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[TM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TM * LDK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15;
    const int i0 = blockIdx.x * TM;
    const int jb = blockIdx.y * tps * TM;
    const int je = min(N, jb + tps * TM);
    int ii[4];
    long long li[4];
    float mx[4], E[4], ps[4], pc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ii[r] = i0 + wv * 16 + (lane >> 4) * 4 + r;
        li[r] = lab[ii[r] < N ? ii[r] : N - 1];
        mx[r] = -INFINITY;
        E[r] = ps[r] = pc[r] = 0.f;
    }
    for (int j0 = jb; j0 < je; j0 += TM) {
        f32x4 acc[4];
        s_tile(fn, Dp, i0, N, j0, N, As, Bs, acc);
        long long lj[4];
        bool vj[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + t * 16 + c;
            vj[t] = j < N;
            lj[t] = lab[vj[t] ? j : N - 1];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s[4], m = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = acc[t][r] / T;
                if (vj[t]) m = fmaxf(m, s[t]);
            }
            const float mn = fmaxf(mx[r], row_max16(m));          // the diagonal takes part in the maximum
            float e = 0.f, p = 0.f, n = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (vj[t] && j0 + t * 16 + c != ii[r]) {
                    e += __expf(s[t] - mn);
                    if (lj[t] == li[r]) {
                        p += s[t];
                        n += 1.f;
                    }
                }
            E[r] = E[r] * __expf(mx[r] - mn) + row_sum16(e);
            mx[r] = mn;
            ps[r] += row_sum16(p);
            pc[r] += row_sum16(n);
        }
    }
    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (ii[r] < N) {
                if (gridDim.y == 1) {
                    stats_finalize(o, ii[r], N, mx[r], E[r], ps[r], pc[r]);
                } else {
                    const long long KN = (long long)gridDim.y * N, at = (long long)blockIdx.y * N + ii[r];
                    part[at] = mx[r];
                    part[KN + at] = E[r];
                    part[2 * KN + at] = ps[r];
                    part[3 * KN + at] = pc[r];
                }
            }
    }
}

// one thread per row: the splits in index order (every split holds at least one key, so its maximum is finite)
__global__ __launch_bounds__(256) void supcon_merge_kernel(const float* __restrict__ part, int KS, int N, RowStats o) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const long long KN = (long long)KS * N;
    float mx = -INFINITY;
    for (int z = 0; z < KS; ++z) mx = fmaxf(mx, part[(long long)z * N + i]);
    float E = 0.f, ps = 0.f, pc = 0.f;
    for (int z = 0; z < KS; ++z) {
        const long long at = (long long)z * N + i;
        E += part[KN + at] * __expf(part[at] - mx);
        ps += part[2 * KN + at];
        pc += part[3 * KN + at];
    }
    stats_finalize(o, i, N, mx, E, ps, pc);
}

// loss = sum_i rowloss[i]: thread t adds its contiguous share in index order in f64, then the 256 sums in a fixed tree
__global__ __launch_bounds__(256) void supcon_finish_kernel(const float* __restrict__ rowloss, int N, float* __restrict__ loss) {
    __shared__ double lds4[4];
    const int per = (N + 255) / 256;
    const int lo = min(per * (int)threadIdx.x, N), hi = min(lo + per, N);
    double v = 0.0;
    for (int i = lo; i < hi; ++i) v += (double)rowloss[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((lds4[0] + lds4[1]) + lds4[2]) + lds4[3]);
}

// d f_i[d] = grad_scale * (g - dot fn_i[d]) / nrm_i,  g = (sum_k C_ik fn_k[d]) / T,  dot = g_i . fn_i = sum_k C_ik s_ik
__device__ __forceinline__ float project(float sum, float T, float dot, float fnid, float nrm, float grad_scale) {
    return (sum / T - dot * fnid) / nrm * grad_scale;
}

// grid (owned anchor tiles, column slices, key splits).  With more than one split the sums go to pout [KS][M][Dp] and
// pdot [KS][M] instead of dfeat
__global__ __launch_bounds__(256) void supcon_grad_kernel(const float* __restrict__ fn, const long long* __restrict__ lab,
                                                          const float* __restrict__ nrm, const float* __restrict__ mx_a,
                                                          const float* __restrict__ E_a, const float* __restrict__ P_a,
                                                          const float* __restrict__ w_a, int N, int D, int Dp, int row0, int M,
                                                          float T, float grad_scale, int tps, float* __restrict__ dfeat,
                                                          float* __restrict__ pout, float* __restrict__ pdot) {
    __shared__ __attribute__((aligned(16))) float As[TM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TM * LDK];
    __shared__ __attribute__((aligned(16))) float Cs[TM * LDC];
    __shared__ __attribute__((aligned(16))) float Fs[TM * LDD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int a0 = row0 + blockIdx.x * TM, aend = row0 + M;
    const int d0 = blockIdx.y * DS;
    const int dn = Dp - d0 < DS ? Dp - d0 : DS;       // columns of this slice (a multiple of 4)
    const int jb = blockIdx.z * tps * TM;
    const int je = min(N, jb + tps * TM);
    int ii[4];
    bool vi[4];
    long long li[4];
    float mxi[4], Ei[4], Pi[4], wi[4], dot[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ii[r] = a0 + wv * 16 + g * 4 + r;
        vi[r] = ii[r] < aend;
        const int ic = vi[r] ? ii[r] : aend - 1;
        li[r] = lab[ic];
        mxi[r] = mx_a[ic];
        Ei[r] = E_a[ic];
        Pi[r] = P_a[ic];
        wi[r] = w_a[ic];
        dot[r] = 0.f;
    }
    f32x4 out[DS / 16];
#pragma unroll
    for (int q = 0; q < DS / 16; ++q) out[q] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j0 = jb; j0 < je; j0 += TM) {
        f32x4 acc[4];
        s_tile(fn, Dp, a0, aend, j0, N, As, Bs, acc);
        long long lj[4];
        bool vj[4];
        float mxj[4], Ej[4], Pj[4], wj[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + t * 16 + c;
            vj[t] = j < N;
            const int jc = vj[t] ? j : N - 1;
            lj[t] = lab[jc];
            mxj[t] = mx_a[jc];
            Ej[t] = E_a[jc];
            Pj[t] = P_a[jc];
            wj[t] = w_a[jc];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float dd = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float s = acc[t][r] / T;
                const float mk = lj[t] == li[r] ? 1.f : 0.f;
                const float gik = -wi[r] * (mk - Pi[r] * (__expf(s - mxi[r]) / Ei[r]));      // d loss / d s_ik
                const float gki = -wj[t] * (mk - Pj[t] * (__expf(s - mxj[t]) / Ej[t]));      // d loss / d s_ki, s_ki = s_ik
                const bool ok = vi[r] && vj[t] && j0 + t * 16 + c != ii[r];
                const float cv = ok ? gik + gki : 0.f;
                Cs[(wv * 16 + g * 4 + r) * LDC + t * 16 + c] = cv;
                dd += cv * s;
            }
            dot[r] += row_sum16(dd);
        }
        // out += C (64 anchors x 64 keys) x Fn (64 keys x dn columns), the keys of the tile in index order
#pragma unroll
        for (int q = 0; q < DS / DC; ++q) {
            if (q * DC < dn) {
                __syncthreads();
#pragma unroll
                for (int v = threadIdx.x; v < TM * DC / 4; v += 256) {
                    const int r = v >> 4, cc = (v & 15) * 4;
                    const int col = d0 + q * DC + cc;
                    f32x4 x = {0.f, 0.f, 0.f, 0.f};
                    if (j0 + r < N && col < Dp) x = *(const f32x4*)(fn + (long long)(j0 + r) * Dp + col);
                    *(f32x4*)(Fs + r * LDD + cc) = x;
                }
                __syncthreads();
#pragma unroll 4
                for (int kk = 0; kk < TM / 4; ++kk) {
                    const float a = Cs[(wv * 16 + c) * LDC + kk * 4 + g];
#pragma unroll
                    for (int u = 0; u < DC / 16; ++u) {
                        const float b = Fs[(kk * 4 + g) * LDD + u * 16 + c];
                        out[q * (DC / 16) + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, out[q * (DC / 16) + u], 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (!vi[r]) continue;
        const long long ir = ii[r] - row0;
        if (gridDim.z == 1) {
            const float ni = nrm[ii[r]];
            const float* fi = fn + (long long)ii[r] * Dp;
            float* o = dfeat + ir * D;
#pragma unroll
            for (int q = 0; q < DS / 16; ++q) {
                const int d = d0 + q * 16 + c;
                if (d < D) o[d] = project(out[q][r], T, dot[r], fi[d], ni, grad_scale);
            }
        } else {
            float* o = pout + ((long long)blockIdx.z * M + ir) * Dp;
#pragma unroll
            for (int q = 0; q < DS / 16; ++q) {
                const int d = d0 + q * 16 + c;
                if (d < Dp) o[d] = out[q][r];
            }
            if (c == 0 && blockIdx.y == 0) pdot[(long long)blockIdx.z * M + ir] = dot[r];     // every slice holds the same dot
        }
    }
}

// grid (M, ceil(D / 256)): the splits' partial sums in split order, then the projection
__global__ __launch_bounds__(256) void supcon_project_kernel(const float* __restrict__ pout, const float* __restrict__ pdot,
                                                             const float* __restrict__ fn, const float* __restrict__ nrm, int KS,
                                                             int M, int D, int Dp, int row0, float T, float grad_scale,
                                                             float* __restrict__ dfeat) {
    const int i = blockIdx.x, d = blockIdx.y * 256 + threadIdx.x;
    if (d >= D) return;
    float sum = 0.f, dot = 0.f;
    for (int z = 0; z < KS; ++z) {
        sum += pout[((long long)z * M + i) * Dp + d];
        dot += pdot[(long long)z * M + i];
    }
    dfeat[(long long)i * D + d] = project(sum, T, dot, fn[(long long)(row0 + i) * Dp + d], nrm[row0 + i], grad_scale);
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

int64_t hs_supcon_tiled_ws_bytes(int32_t N, int32_t D) {
    if (N < 1 || N > HS_SUPCON_TILED_MAX_N || D < 1 || D > HS_SUPCON_TILED_MAX_D) return -1;
    int tps, KS;
    key_splits(N, tps, KS);
    const int64_t Dp = pad4(D);
    int64_t floats = (int64_t)N * Dp + (int64_t)NSTAT * N;
    if (KS > 1) floats += (int64_t)KS * N * (Dp + 5);       // per split and row: partial d fn, dot, (mx, E, sum, count)
    return floats * 4;
}

hs_status hs_supcon_tiled(const float* feat, const int64_t* labels, int32_t N, int32_t D, int32_t row0, int32_t M,
                          float temperature, float grad_scale, float* loss, float* dfeat, void* ws, void* stream) {
    HS_REQUIRE(feat && labels && loss && ws, "supcon_tiled: NULL pointer");
    HS_REQUIRE(N >= 1 && N <= HS_SUPCON_TILED_MAX_N, "supcon_tiled: N %d outside [1, %d]", N, HS_SUPCON_TILED_MAX_N);
    HS_REQUIRE(D >= 1 && D <= HS_SUPCON_TILED_MAX_D, "supcon_tiled: D %d outside [1, %d]", D, HS_SUPCON_TILED_MAX_D);
    HS_REQUIRE(row0 >= 0 && M >= 1 && (int64_t)row0 + M <= N, "supcon_tiled: rows [%d, %d + %d) outside [0, %d)", row0, row0, M, N);
    HS_REQUIRE(((uintptr_t)ws & 15) == 0, "supcon_tiled: ws is not 16-byte aligned");
    const int Dp = pad4(D);
    int tps, KS;
    key_splits(N, tps, KS);
    float* fn = (float*)ws;
    float* nrm = fn + (long long)N * Dp;
    RowStats st;
    st.mx = nrm + N;
    st.E = st.mx + N;
    st.P = st.E + N;
    st.w = st.P + N;
    st.rowloss = st.w + N;
    float* part = st.rowloss + N;                       // [4][KS][N]
    float* pdot = part + 4ll * KS * N;                  // [KS][M]
    float* pout = pdot + (long long)KS * N;             // [KS][M][Dp]
    hipStream_t s = (hipStream_t)stream;
    const long long* lab = (const long long*)labels;
    const int NT = (N + TM - 1) / TM;
    hipLaunchKernelGGL(supcon_normalise_kernel, dim3((N + 3) / 4), dim3(256), 0, s, feat, N, D, Dp, fn, nrm);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_stats_kernel, dim3(NT, KS), dim3(256), 0, s, fn, lab, N, Dp, temperature, tps, st, part);
    HS_LAUNCH_CHECK();
    if (KS > 1) {
        hipLaunchKernelGGL(supcon_merge_kernel, dim3((N + 255) / 256), dim3(256), 0, s, part, KS, N, st);
        HS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(supcon_finish_kernel, dim3(1), dim3(256), 0, s, st.rowloss, N, loss);
    HS_LAUNCH_CHECK();
    if (dfeat) {
        hipLaunchKernelGGL(supcon_grad_kernel, dim3((M + TM - 1) / TM, (Dp + DS - 1) / DS, KS), dim3(256), 0, s, fn, lab, nrm, st.mx,
                           st.E, st.P, st.w, N, D, Dp, row0, M, temperature, grad_scale, tps, dfeat, pout, pdot);
        HS_LAUNCH_CHECK();
        if (KS > 1) {
            hipLaunchKernelGGL(supcon_project_kernel, dim3(M, (D + 255) / 256), dim3(256), 0, s, pout, pdot, fn, nrm, KS, M, D, Dp,
                               row0, temperature, grad_scale, dfeat);
            HS_LAUNCH_CHECK();
        }
    }
    return HS_OK;
}

}  // extern "C"
