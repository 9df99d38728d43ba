// BatchNorm (train/eval, NHWC) and LayerNorm forward/backward -- HBM-bound kernels.
// All 16-byte vector accesses, f32 statistics, deterministic two-stage column reductions.
//
// Replaces torch.nn.BatchNorm2d inside torchvision's ResNet blocks (reference encoder.py:35-42,
// mibf_net/model_resnet.py:15) and torch.nn.LayerNorm (modules/fusion_blocks.py:17-34, heads.py:36,
// transformers BertEmbeddings / BertSelfOutput / BertOutput LayerNorm, eps 1e-12).
#include <algorithm>
#include <type_traits>
#include "hs_internal.h"

namespace hs {

// --------------------------------------------------------------------------------------------
// generic column-reduction geometry over a row-major [M][C] matrix (C % chunk == 0)
// --------------------------------------------------------------------------------------------
struct ColGeom {
    int cg;        // chunk columns = C / EPC
    int tpc;       // threads across columns (<=256, power of two divides 256)
    int rows_par;  // 256 / tpc
    int gx, gy;    // grid
};
static ColGeom col_geom(long long M, int C, int epc) {
    ColGeom g;
    g.cg = C / epc;
    int tpc = 1;
    while (tpc < g.cg && tpc < 256) tpc <<= 1;
    g.tpc = tpc;
    g.rows_par = 256 / tpc;
    g.gx = ceil_div(g.cg, tpc);
    long long want = 2048 / g.gx;
    if (want < 1) want = 1;
    long long maxy = ceil_div(M, (long long)g.rows_par * 4);   // >= 4 rows per thread
    if (maxy < 1) maxy = 1;
    g.gy = (int)(want < maxy ? want : maxy);
    return g;
}

// ============================================================================================
// BatchNorm
// ============================================================================================
// block-level column reduction of per-thread partial sums: lanes of a wave that share a column (tx) first fold with
// xor-shuffles (offsets tpc..32), then the four waves fold through LDS; fixed order -> deterministic.  Returns the
// block total in the threads with ty == 0 (valid for every e).
template <int E, int NV>
__device__ __forceinline__ void block_col_reduce(float (&v)[NV][E], int tpc, float* sh /* [4][64*E*NV] or [256*E*NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (tpc < 64) {
        for (int o = 32; o >= tpc; o >>= 1) {
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e) v[k][e] += __shfl_xor(v[k][e], o, 64);
        }
        // lanes 0..tpc-1 of every wave now hold their wave's column sums
        if (lane < tpc) {
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e) sh[((wave * NV + k) * 64 + lane) * E + e] = v[k][e];
        }
        __syncthreads();
        if (wave == 0 && lane < tpc) {
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e)
                    v[k][e] = (sh[((0 * NV + k) * 64 + lane) * E + e] + sh[((1 * NV + k) * 64 + lane) * E + e]) +
                              (sh[((2 * NV + k) * 64 + lane) * E + e] + sh[((3 * NV + k) * 64 + lane) * E + e]);
        }
    } else {
        // tpc in {64, 128, 256}: rows_par = 256 / tpc row lanes, one per (group of) wave(s)
        const int rows_par = 256 / tpc, tx = threadIdx.x % tpc, ty = threadIdx.x / tpc;
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int e = 0; e < E; ++e) sh[((ty * NV + k) * tpc + tx) * E + e] = v[k][e];
        __syncthreads();
        if (ty == 0) {
            for (int j = 1; j < rows_par; ++j)
#pragma unroll
                for (int k = 0; k < NV; ++k)
#pragma unroll
                    for (int e = 0; e < E; ++e) v[k][e] += sh[((j * NV + k) * tpc + tx) * E + e];
        }
    }
}

// stage 1: per (row block, channel) partials (count, mean, M2).  Sums are taken relative to a per-block, per-channel
// shift x0 (the block's first row), which keeps sum((x-x0)^2) - sum(x-x0)^2/n well conditioned without Welford's
// per-element division; four independent rows are in flight per thread.
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const T* __restrict__ x, long long M, int C, int tpc,
                                                               float* __restrict__ ws) {
    constexpr int E = Chunk<T>::N;
    __shared__ float sh[256 * E * 2];
    const int cg = C / E;
    const int tx = threadIdx.x % tpc, ty = threadIdx.x / tpc, rows_par = 256 / tpc;
    const int cc = blockIdx.x * tpc + tx;
    const bool live = cc < cg;
    const long long r0 = (long long)blockIdx.y * rows_par;
    float x0[E], acc[2][E];
#pragma unroll
    for (int e = 0; e < E; ++e) x0[e] = acc[0][e] = acc[1][e] = 0.f;
    float cnt = 0.f;
    if (live) {
        Chunk<T>::unpack(*(const u32x4*)(x + r0 * C + (long long)cc * E), x0);   // r0 < M by construction of the grid
        const long long step = (long long)gridDim.y * rows_par;
        long long r = r0 + ty;
        const T* px = x + (long long)cc * E;
        for (; r + 3 * step < M; r += 4 * step) {
            float f[4][E];
#pragma unroll
            for (int u = 0; u < 4; ++u) Chunk<T>::unpack(*(const u32x4*)(px + (r + u * step) * C), f[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float d = f[u][e] - x0[e];
                    acc[0][e] += d;
                    acc[1][e] = fmaf(d, d, acc[1][e]);
                }
            cnt += 4.f;
        }
        for (; r < M; r += step) {
            float f[E];
            Chunk<T>::unpack(*(const u32x4*)(px + r * C), f);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float d = f[e] - x0[e];
                acc[0][e] += d;
                acc[1][e] = fmaf(d, d, acc[1][e]);
            }
            cnt += 1.f;
        }
    }
    // row count of the block: every column has the same one
    float cv[1][1] = {{cnt}};
    block_col_reduce<1, 1>(cv, tpc, sh);
    __syncthreads();
    block_col_reduce<E, 2>(acc, tpc, sh);
    if (ty == 0 && live) {
        const float n = cv[0][0];
        float* o = ws + ((long long)blockIdx.y * C + (long long)cc * E) * 3;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const float s1 = acc[0][e];
            o[e * 3 + 0] = n;
            o[e * 3 + 1] = x0[e] + s1 / n;
            o[e * 3 + 2] = fmaxf(acc[1][e] - s1 * s1 / n, 0.f);
        }
    }
}

// stage 2: merge row blocks; produce mean / invstd / (scale, shift); update running statistics.
// One wave per channel: lanes merge a strided subset of the partials (Chan's formula), then a butterfly of
// pairwise merges -- the order is fixed, so the result is deterministic.
__device__ __forceinline__ void chan_merge(float& cnt, float& mean, float& m2, float nb, float mb, float m2b) {
    if (nb > 0.f) {
        const float n = cnt + nb;
        const float d = mb - mean;
        const float w = nb / n;
        mean += d * w;
        m2 += m2b + d * d * cnt * w;
        cnt = n;
    }
}
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ ws, int gy, int C, long long M,
                                                             float eps, float momentum, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, float* __restrict__ mean_out,
                                                             float* __restrict__ invstd_out, float* __restrict__ scale_out,
                                                             float* __restrict__ shift_out) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    for (int b = lane; b < gy; b += 64) {
        const float* p = ws + ((long long)b * C + c) * 3;
        chan_merge(cnt, mean, m2, p[0], p[1], p[2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float nb = __shfl_xor(cnt, o, 64), mb = __shfl_xor(mean, o, 64), qb = __shfl_xor(m2, o, 64);
        // both partners must compute the same merged value: merge (lower lane) + (upper lane) in that order
        float c0 = cnt, m0 = mean, q0 = m2, c1 = nb, m1 = mb, q1 = qb;
        if (lane & o) {
            c0 = nb; m0 = mb; q0 = qb; c1 = cnt; m1 = mean; q1 = m2;
        }
        chan_merge(c0, m0, q0, c1, m1, q1);
        cnt = c0; mean = m0; m2 = q0;
    }
    if (lane != 0) return;
    const float var = m2 / (float)M;                   // biased, used for normalisation
    const float invstd = rsqrtf(var + eps);
    mean_out[c] = mean;
    invstd_out[c] = invstd;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    scale_out[c] = g * invstd;
    shift_out[c] = b - mean * g * invstd;
    if (running_mean) {
        const float unbiased = M > 1 ? m2 / (float)(M - 1) : var;
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
}

// eval mode: scale/shift from running statistics
__global__ void bn_eval_scale_kernel(int C, float eps, const float* gamma, const float* beta,
                                     const float* running_mean, const float* running_var, float* mean_out,
                                     float* invstd_out, float* scale_out, float* shift_out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float invstd = rsqrtf(running_var[c] + eps);
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    mean_out[c] = running_mean[c];
    invstd_out[c] = invstd;
    scale_out[c] = g * invstd;
    shift_out[c] = b - running_mean[c] * g * invstd;
}

// E consecutive per-channel floats (a chunk's channels: 16-byte aligned) read as f32x4
template <int E>
__device__ __forceinline__ void load_chan(const float* __restrict__ p, float (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; e += 4) {
        const f32x4 a = *(const f32x4*)(p + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[e + j] = a[j];
    }
}
__device__ __forceinline__ float round_bf16(float v) { return (float)(bf16_t)v; }

// y = x*scale + shift (+ residual) (relu).  The residual is none (res == nullptr), stored (res), or with DSRES formed from the
// downsample convolution's output res as bf16(fma(res, scale_d, shift_d)): what the downsample BatchNorm's own apply pass would
// have stored as the identity, rounded to bf16 in registers and not read back (lean image-tower passes, see below)
template <typename T, bool DSRES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const T* __restrict__ res,
                                                       const float* __restrict__ scale_d, const float* __restrict__ shift_d,
                                                       T* __restrict__ y, long long nchunks, int cg, int relu) {
    constexpr int E = Chunk<T>::N;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (long long)gridDim.x * 256) {
        const int c0 = (int)(i % cg) * E;
        float f[E], r[E], sc[E], sh[E];
        Chunk<T>::unpack(*(const u32x4*)(x + i * E), f);
        if (DSRES || res) Chunk<T>::unpack(*(const u32x4*)(res + i * E), r);
        load_chan(scale + c0, sc);
        load_chan(shift + c0, sh);
        if constexpr (DSRES) {
            float sd[E], hd[E];
            load_chan(scale_d + c0, sd);
            load_chan(shift_d + c0, hd);
#pragma unroll
            for (int e = 0; e < E; ++e) r[e] = round_bf16(fmaf(r[e], sd[e], hd[e]));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            float v = fmaf(f[e], sc[e], sh[e]);        // (explicit: the backward recomputes this very value for the ReLU mask)
            if (DSRES || res) v += r[e];
            if (relu) v = fmaxf(v, 0.f);
            f[e] = v;
        }
        *(u32x4*)(y + i * E) = Chunk<T>::pack(f);
    }
}

// dx = ca*dz + cb*(x - mean) + cc per channel:  train  ca = g*is, cb = -g*is*is*dgamma/M, cc = -ca*dbeta/M
//                                               eval   ca = g*is, cb = 0, cc = 0
// (x - mean is formed first: folding mean into cc cancels catastrophically when |mean| >> std)
__device__ __forceinline__ void bn_bwd_final_channel(const float* __restrict__ ws, int gy, int C,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, float invM, int train,
                                                     float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                     float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    float a = 0.f, b = 0.f;
    for (int i = lane; i < gy; i += 64) {
        a += ws[((long long)i * C + c) * 2 + 0];
        b += ws[((long long)i * C + c) * 2 + 1];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane != 0) return;
    dbeta[c] = a;
    dgamma[c] = b;
    const float g = gamma ? gamma[c] : 1.f, is = invstd[c];
    const float ca = g * is;
    const float cb = train ? -ca * is * b * invM : 0.f;
    const float cc = train ? -ca * a * invM : 0.f;
    coef[c] = ca;
    coef[C + c] = cb;
    coef[2 * C + c] = cc;
    coef[3 * C + c] = mean[c];
}
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ ws, int gy, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, float invM, int train,
                                                           float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                           float* __restrict__ coef) {
    bn_bwd_final_channel(ws, gy, C, gamma, mean, invstd, invM, train, dbeta, dgamma, coef);
}
// two BatchNorms over the same [M][C] grid in one launch (blockIdx.y picks one): a block's last stage and its downsample branch
struct BnFinalSet {
    const float *ws, *gamma, *mean, *invstd;
    float *dbeta, *dgamma, *coef;
};
__global__ __launch_bounds__(256) void bn_bwd_final_pair_kernel(BnFinalSet a, BnFinalSet b, int gy, int C, float invM, int train) {
    const bool f = blockIdx.y == 0;      // (uniform selects of the pointers: no indexed copy of the argument structs)
    bn_bwd_final_channel(f ? a.ws : b.ws, gy, C, f ? a.gamma : b.gamma, f ? a.mean : b.mean, f ? a.invstd : b.invstd, invM, train,
                         f ? a.dbeta : b.dbeta, f ? a.dgamma : b.dgamma, f ? a.coef : b.coef);
}
// ============================================================================================
// lean image-tower passes (bf16 composites only, HAMSPINE_IMG_LEAN in blocks.hip): the arithmetic of the separate launches, in
// the same order, with one full-size tensor less written to memory and read back.  Every value that used to cross memory as
// bf16 is rounded to bf16 in registers, and the apply and backward passes are instantiations of the bodies the separate
// launches run (bn_apply_kernel above, bn_bwd_partial_kernel / bn_bwd_apply_kernel below), so the results are bitwise theirs.
// ============================================================================================
// stem forward: y, idx = maxpool3x3/2(relu(bn(c))) straight from the convolution output -- bn_apply_kernel (relu) followed by
// maxpool_fwd_kernel (elem.hip) without the activation in between: same window walk, first maximum wins, NaN propagates
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const bf16_t* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, bf16_t* __restrict__ y,
                                                              unsigned char* __restrict__ idx, int N, int H, int W, int C,
                                                              int P, int Q) {
    constexpr int E = 8, ks = 3, st = 2, pad = 1;
    const int cg = C / E;
    const long long total = (long long)N * P * Q * cg;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % cg);
        long long t = i / cg;
        const int q = (int)(t % Q);
        t /= Q;
        const int p = (int)(t % P);
        const int n = (int)(t / P);
        float best[E], sc[E], sf[E];
        unsigned bi[E];
        load_chan(scale + c * E, sc);
        load_chan(shift + c * E, sf);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            best[e] = -INFINITY;
            bi[e] = 0;
        }
#pragma unroll
        for (int r = 0; r < ks; ++r) {
            const int h = p * st - pad + r;
            if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
            for (int s = 0; s < ks; ++s) {
                const int w = q * st - pad + s;
                if ((unsigned)w >= (unsigned)W) continue;
                float f[E];
                Chunk<bf16_t>::unpack(*(const u32x4*)(x + (((long long)n * H + h) * W + w) * C + c * E), f);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float v = round_bf16(fmaxf(fmaf(f[e], sc[e], sf[e]), 0.f));   // what bn_apply_kernel stores
                    if (v > best[e] || v != v) {
                        best[e] = v;
                        bi[e] = (unsigned)(r * ks + s);
                    }
                }
            }
        }
        const long long o = (((long long)n * P + p) * Q + q) * C + c * E;
        *(u32x4*)(y + o) = Chunk<bf16_t>::pack(best);
        u32x2 ib;
        ib[0] = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
        ib[1] = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
        *(u32x2*)(idx + o) = ib;
    }
}

// the value maxpool_bwd_kernel (elem.hip, 3x3 / 2, pad 1) stores at row (n, h, w) of the [N*H*W][C] map, chunk cc: up to four
// (p, q) windows in its order, f32 adds, rounded to bf16
struct PoolGeom {
    int H, W, P, Q;
};
__device__ __forceinline__ void maxpool_grad_at(const bf16_t* __restrict__ dy, const unsigned char* __restrict__ idx,
                                                const PoolGeom& pg, unsigned row, int C, int cc, float (&out)[8]) {
    constexpr int E = 8, ks = 3, st = 2, pad = 1;
    const int w = (int)(row % (unsigned)pg.W);
    const unsigned t = row / (unsigned)pg.W;
    const int h = (int)(t % (unsigned)pg.H);
    const int n = (int)(t / (unsigned)pg.H);
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    const int p_lo = max(0, (h + pad - ks + st) / st), p_hi = min(pg.P - 1, (h + pad) / st);
    const int q_lo = max(0, (w + pad - ks + st) / st), q_hi = min(pg.Q - 1, (w + pad) / st);
    for (int p = p_lo; p <= p_hi; ++p)
        for (int q = q_lo; q <= q_hi; ++q) {
            const int r = h + pad - p * st, s = w + pad - q * st;
            if (r < 0 || r >= ks || s < 0 || s >= ks) continue;
            const unsigned me = (unsigned)(r * ks + s);
            const long long o = (((long long)n * pg.P + p) * pg.Q + q) * C + cc * E;
            float g[E];
            Chunk<bf16_t>::unpack(*(const u32x4*)(dy + o), g);
            const u32x2 ib = *(const u32x2*)(idx + o);
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (((ib[e >> 2] >> (8 * (e & 3))) & 0xffu) == me) acc[e] += g[e];
        }
#pragma unroll
    for (int e = 0; e < E; ++e) out[e] = round_bf16(acc[e]);
}

// ============================================================================================
// BatchNorm backward: one partial-sum body and one apply body.  Their compile-time parameters are the element type, where the
// incoming gradient dy comes from (a gradient source, below) and whether a second BatchNorm fed by the same dz rides along (PAIR).
// A new fused variant is one more gradient source (or residual source of bn_apply_kernel), never a copy of a kernel.
// ============================================================================================
// gradient sources: chunk cc of row `row` of the [M][C] gradient map, at element offset o = row * C + cc * E
// relu_from_x: the ReLU mask is known at compile time to be recomputed from x (else the runtime relu / y == nullptr tests decide)
struct GradStored {          // dy is the map itself
    static constexpr bool relu_from_x = false;
    template <typename T, int E>
    __device__ __forceinline__ void load(const T* __restrict__ dy, long long o, long long, int, int, float (&g)[E]) const {
        Chunk<T>::unpack(*(const u32x4*)(dy + o), g);
    }
};
struct GradPooled {          // dy is the [N][P][Q][C] gradient of a 3x3 / 2 max-pool of the map: gathered, never stored (stem, bf16)
    static constexpr bool relu_from_x = true;     // the stem is relu(bn(c)); with the runtime tests the gather costs an occupancy step
    const unsigned char* idx;
    PoolGeom pg;
    __device__ __forceinline__ void load(const bf16_t* __restrict__ dy, long long, long long row, int cc, int C, float (&g)[8]) const {
        maxpool_grad_at(dy, idx, pg, (unsigned)row, C, cc, g);
    }
};

// backward stage 1: per (row block, channel) sums of dz and dz*xhat, dz = dy * (y > 0 if relu); bn_bwd_final_kernel merges them.
// y == nullptr with relu: the forward output was relu(fma(x, scale, shift)) with no residual, so its sign is recomputed from x
// (one activation read less; bf16 rounding never turns a positive f32 into 0).
// PAIR: x is a block's last stage (relu, mask y > 0) and xd its downsample BatchNorm (no relu), whose incoming gradient is that dz
// -- exactly dy or 0, what the apply pass would store as dres -- known before any coefficient is.  The second sums are what this
// kernel makes alone with relu = 0 over the stored dres: same rows per thread, same order.
template <typename T, typename Src, bool PAIR>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const T* __restrict__ dy, Src src, const T* __restrict__ y,
                                                             const T* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, long long M, int C,
                                                             int tpc, int relu_arg, float* __restrict__ ws,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const T* __restrict__ xd, const float* __restrict__ mean_d,
                                                             const float* __restrict__ invstd_d, float* __restrict__ ws_d) {
    constexpr int E = Chunk<T>::N, NB = PAIR ? 2 : 1;
    const int cg = C / E;
    const int tx = threadIdx.x % tpc, ty = threadIdx.x / tpc, rows_par = 256 / tpc;
    const int cc = blockIdx.x * tpc + tx;
    // (PAIR is by definition relu with the mask from the stored y: a compile-time fact as well, or the runtime branches sit
    // between the loads of the rows in flight -- the pair's partial pass took 58 us where the copy took 34)
    const bool relu = PAIR || Src::relu_from_x || relu_arg, maskx = Src::relu_from_x || (!PAIR && relu && y == nullptr);
    float acc[NB][2][E], mu[NB][E], is[NB][E], sc[E], sf[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        sc[e] = sf[e] = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b][0][e] = acc[b][1][e] = mu[b][e] = is[b][e] = 0.f;
    }
    if (cc < cg) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            mu[0][e] = mean[cc * E + e];
            is[0][e] = invstd[cc * E + e];
            if constexpr (PAIR) {
                mu[1][e] = mean_d[cc * E + e];
                is[1][e] = invstd_d[cc * E + e];
            }
            if (maskx) {
                sc[e] = scale[cc * E + e];
                sf[e] = shift[cc * E + e];
            }
        }
        const long long step = (long long)gridDim.y * rows_par;
        long long r = (long long)blockIdx.y * rows_par + ty;
        auto load = [&](long long rr, float (&g)[E], float (&xv)[NB][E], float (&yv)[E]) {
            const long long o = rr * C + (long long)cc * E;
            src.load(dy, o, rr, cc, C, g);
            Chunk<T>::unpack(*(const u32x4*)(x + o), xv[0]);
            if (relu) {
                if (maskx) {
#pragma unroll
                    for (int e = 0; e < E; ++e) yv[e] = fmaf(xv[0][e], sc[e], sf[e]);
                } else {
                    Chunk<T>::unpack(*(const u32x4*)(y + o), yv);
                }
            }
            if constexpr (PAIR) Chunk<T>::unpack(*(const u32x4*)(xd + o), xv[1]);
        };
        auto fold = [&](const float (&g)[E], const float (&xv)[NB][E], const float (&yv)[E]) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float dz = (relu && !(yv[e] > 0.f)) ? 0.f : g[e];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    acc[b][0][e] += dz;
                    acc[b][1][e] = fmaf(dz, (xv[b][e] - mu[b][e]) * is[b][e], acc[b][1][e]);
                }
            }
        };
        for (; r + step < M; r += 2 * step) {      // two rows in flight (separate arrays: as one struct per row, 8 VGPRs more)
            float g0[E], x0[NB][E], y0[E], g1[E], x1[NB][E], y1[E];
            load(r, g0, x0, y0);
            load(r + step, g1, x1, y1);
            fold(g0, x0, y0);
            fold(g1, x1, y1);
        }
        for (; r < M; r += step) {
            float g0[E], x0[NB][E], y0[E];
            load(r, g0, x0, y0);
            fold(g0, x0, y0);
        }
    }
    __shared__ float sh[256 * E * 2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b) __syncthreads();
        block_col_reduce<E, 2>(acc[b], tpc, sh);
        if (ty == 0 && cc < cg) {
            float* o = (b ? ws_d : ws) + ((long long)blockIdx.y * C + (long long)cc * E) * 2;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                o[e * 2 + 0] = acc[b][0][e];
                o[e * 2 + 1] = acc[b][1][e];
            }
        }
    }
}

// dx = ca*dz + cb*(x - mu) + cc, with contraction off: every BatchNorm backward forms dx here, so no result depends on how the
// compiler would fuse the expression.  Left to it, it had fused it differently per kernel -- a copied lean kernel once came out
// an ulp off the separate launches for that reason.  The two forms below are the ones it had chosen for the plain kernels (read
// from their gfx950 assembly) and are now fixed, so bf16 and f32 results are bit for bit what they were:
//   bf16 (8 elements per thread): fma(cb, x - mu, ca*dz) + cc      f32 (4 per thread): (ca*dz + cb*(x - mu)) + cc, nothing fused.
// They differ for no numerical reason: it is where the optimiser's heuristics happened to land for the two chunk widths.
template <typename T>
__device__ __forceinline__ float bn_bwd_dx(float ca, float dz, float cb, float x, float mu, float cc) {
#pragma clang fp contract(off)
    const float t = x - mu;
    const float p = ca * dz;
    if constexpr (sizeof(T) == 2) return fmaf(cb, t, p) + cc;
    else return (p + cb * t) + cc;
}

// backward stage 2: dx from the coefficients [ca | cb | cc | mean] of bn_bwd_final_kernel; optional dres = dz (the separate
// launches only: the lean forms exist so that it is not stored).  PAIR: also dx_d of the downsample BatchNorm, whose dy is dz.
template <typename T, typename Src, bool PAIR>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, Src src, const T* __restrict__ y,
                                                           const T* __restrict__ x, const float* __restrict__ coef,
                                                           T* __restrict__ dx, T* __restrict__ dres, long long nchunks,
                                                           int cg, int C, int relu_arg, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const T* __restrict__ xd,
                                                           const float* __restrict__ coef_d, T* __restrict__ dx_d) {
    constexpr int E = Chunk<T>::N, NB = PAIR ? 2 : 1;
    constexpr bool plain = !PAIR && std::is_same<Src, GradStored>::value;
    const bool relu = PAIR || Src::relu_from_x || relu_arg, maskx = Src::relu_from_x || (!PAIR && relu && y == nullptr);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % cg), c0 = ci * E;
        float g[E], xv[NB][E], yv[E];
        src.load(dy, i * E, i / cg, ci, C, g);
        Chunk<T>::unpack(*(const u32x4*)(x + i * E), xv[0]);
        if (relu) {
            if (maskx) {
#pragma unroll
                for (int e = 0; e < E; ++e) yv[e] = fmaf(xv[0][e], scale[c0 + e], shift[c0 + e]);
            } else {
                Chunk<T>::unpack(*(const u32x4*)(y + i * E), yv);
            }
        }
        if constexpr (PAIR) Chunk<T>::unpack(*(const u32x4*)(xd + i * E), xv[1]);
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] = (relu && !(yv[e] > 0.f)) ? 0.f : g[e];     // dz
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float* __restrict__ cf = (b ? coef_d : coef) + c0;
            float o[E], ca[E], cb[E], cc[E], mu[E];
            load_chan(cf, ca);
            load_chan(cf + C, cb);
            load_chan(cf + 2 * C, cc);
            load_chan(cf + 3 * C, mu);
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = bn_bwd_dx<T>(ca[e], g[e], cb[e], xv[b][e], mu[e], cc[e]);
            *(u32x4*)((b ? dx_d : dx) + i * E) = Chunk<T>::pack(o);
        }
        if constexpr (plain)
            if (dres) *(u32x4*)(dres + i * E) = Chunk<T>::pack(g);
    }
}

// dsr (DSRES, bf16): the residual is bf16(fma(dsr->c, dsr->scale, dsr->shift)), formed in the apply pass (bn_apply_kernel, DSRES)
struct DsResidual {
    const void* c;
    const float *scale, *shift;
};
template <typename T, bool DSRES = false>
static int bn_fwd_t(const hs_bn_params* p, hipStream_t s, const DsResidual* dsr = nullptr) {
    constexpr int E = Chunk<T>::N;
    HS_REQUIRE(p->C % E == 0, "bn: C %% %d != 0", E);
    const long long M = p->M;
    const int C = p->C;
    if (p->training && p->stats_done) {
        // the producing GEMM finished the statistics as well (hs_gemm_params.bn_finish): scale / shift are in place
    } else if (p->training) {
        ColGeom g = col_geom(M, C, E);
        int rows = g.gy;
        if (p->partial_rows > 0) {     // the producing GEMM already left (count, mean, M2) per row tile in ws
            rows = p->partial_rows;
            HS_REQUIRE(p->ws && p->ws_bytes >= (long long)rows * C * 3 * 4, "bn: workspace smaller than the given partials");
        } else {
            HS_REQUIRE(p->ws && p->ws_bytes >= (long long)g.gy * C * 3 * 4, "bn: workspace too small");
            hipLaunchKernelGGL(bn_stats_partial_kernel<T>, dim3(g.gx, g.gy), dim3(256), 0, s, (const T*)p->x, M, C, g.tpc,
                               (float*)p->ws);
            HS_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(bn_stats_final_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, s, (const float*)p->ws, rows, C, M,
                           p->eps, p->momentum, p->gamma, p->beta, p->running_mean, p->running_var, p->save_mean,
                           p->save_invstd, p->scale, p->shift);
        HS_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(bn_eval_scale_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, C, p->eps, p->gamma, p->beta,
                           p->running_mean, p->running_var, p->save_mean, p->save_invstd, p->scale, p->shift);
        HS_LAUNCH_CHECK();
    }
    if (p->y) {
        const long long nch = M * C / E;
        const int blocks = (int)std::min<long long>((nch + 255) / 256, 4096);
        hipLaunchKernelGGL((bn_apply_kernel<T, DSRES>), dim3(blocks), dim3(256), 0, s, (const T*)p->x, p->scale, p->shift,
                           (const T*)(DSRES ? dsr->c : p->residual), DSRES ? dsr->scale : nullptr, DSRES ? dsr->shift : nullptr,
                           (T*)p->y, nch, C / E, p->relu);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

// backward workspace of one BatchNorm: `rows` rows of per-channel (sum dz, sum dz*xhat) partials, then the coefficients
// [ca | cb | cc | mean] (the layout the GEMM epilogue that finishes the sums writes as well, gemm_core.h)
static long long bn_bwd_ws_bytes(long long rows, int C) { return (rows * C * 2 + 4ll * C) * 4; }

// the backward of p -- and with PAIR of pd, the downsample BatchNorm fed by p's dz, in the same three launches: geometry,
// workspace [partials | coef], then partial sums -> dbeta / dgamma / coefficients -> dx.  y: the stored forward output the ReLU
// mask is taken from, nullptr = recomputed from x.  `who` names the entry point in the refusals.
template <typename T, typename Src, bool PAIR>
static int bn_bwd_run(const char* who, const hs_bn_bwd_params* p, const hs_bn_bwd_params* pd, const void* y, Src src, hipStream_t s) {
    constexpr int E = Chunk<T>::N;
    HS_REQUIRE(p->C % E == 0, "%s: C %% %d != 0", who, E);
    const long long M = p->M;
    const int C = p->C;
    ColGeom g = col_geom(M, C, E);
    if (p->partial_rows > 0) g.gy = p->partial_rows;       // the sums came with the data gradient (hs_gemm_params.bnb_partials)
    const long long need = bn_bwd_ws_bytes(g.gy, C);
    HS_REQUIRE(p->ws && p->ws_bytes >= need && (!PAIR || (pd->ws && pd->ws_bytes >= need)), "%s: workspace too small", who);
    float* coef = (float*)p->ws + (long long)g.gy * C * 2;
    float* coef_d = PAIR ? (float*)pd->ws + (long long)g.gy * C * 2 : nullptr;
    if (p->partial_rows <= 0) {
        hipLaunchKernelGGL((bn_bwd_partial_kernel<T, Src, PAIR>), dim3(g.gx, g.gy), dim3(256), 0, s, (const T*)p->dy, src, (const T*)y,
                           (const T*)p->x, p->save_mean, p->save_invstd, M, C, g.tpc, p->relu, (float*)p->ws, p->scale, p->shift,
                           PAIR ? (const T*)pd->x : nullptr, PAIR ? pd->save_mean : nullptr, PAIR ? pd->save_invstd : nullptr,
                           PAIR ? (float*)pd->ws : nullptr);
        HS_LAUNCH_CHECK();
    }
    if (!(p->partial_rows > 0 && p->sums_done)) {          // (sums_done: the producing GEMM's last workgroups wrote dbeta / dgamma / coef)
        if constexpr (PAIR) {
            const BnFinalSet fa = {(const float*)p->ws, p->gamma, p->save_mean, p->save_invstd, p->dbeta, p->dgamma, coef};
            const BnFinalSet fb = {(const float*)pd->ws, pd->gamma, pd->save_mean, pd->save_invstd, pd->dbeta, pd->dgamma, coef_d};
            hipLaunchKernelGGL(bn_bwd_final_pair_kernel, dim3(ceil_div(C, 4), 2), dim3(256), 0, s, fa, fb, g.gy, C, 1.f / (float)M,
                               p->training);
        } else {
            hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, s, (const float*)p->ws, g.gy, C, p->gamma,
                               p->save_mean, p->save_invstd, 1.f / (float)M, p->training, p->dbeta, p->dgamma, coef);
        }
        HS_LAUNCH_CHECK();
    }
    if (p->dx) {
        const long long nch = M * C / E;
        const int blocks = (int)std::min<long long>((nch + 255) / 256, 4096);
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, Src, PAIR>), dim3(blocks), dim3(256), 0, s, (const T*)p->dy, src, (const T*)y,
                           (const T*)p->x, coef, (T*)p->dx, (T*)p->dres, nch, C / E, C, p->relu, p->scale, p->shift,
                           PAIR ? (const T*)pd->x : nullptr, coef_d, PAIR ? (T*)pd->dx : nullptr);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

int bn_fwd(const hs_bn_params* p, hipStream_t s) {
    HS_REQUIRE(p && p->x && p->scale && p->shift && p->save_mean && p->save_invstd, "bn: null argument");
    return p->dtype == HS_BF16 ? bn_fwd_t<bf16_t>(p, s) : bn_fwd_t<float>(p, s);
}
int bn_bwd(const hs_bn_bwd_params* p, hipStream_t s) {
    HS_REQUIRE(p && p->dy && p->x && p->dbeta && p->dgamma, "bn_bwd: null argument");
    HS_REQUIRE(!p->relu || p->y || (p->scale && p->shift && !p->dres),
               "bn_bwd: a fused ReLU needs the forward output y, or (no residual) the forward's scale / shift to recompute its sign");
    return p->dtype == HS_BF16 ? bn_bwd_run<bf16_t, GradStored, false>("bn_bwd", p, nullptr, p->y, GradStored{}, s)
                               : bn_bwd_run<float, GradStored, false>("bn_bwd", p, nullptr, p->y, GradStored{}, s);
}
// ---- lean forms for the bf16 composites (blocks.hip, HAMSPINE_IMG_LEAN); not part of the C ABI ----
int bn_fwd_dsres(const hs_bn_params* p, const void* c_ds, const float* scale_ds, const float* shift_ds, hipStream_t s) {
    HS_REQUIRE(p && p->x && p->y && p->scale && p->shift && p->save_mean && p->save_invstd && c_ds && scale_ds && shift_ds && !p->residual,
               "bn_fwd_dsres: null argument");
    HS_REQUIRE(p->dtype == HS_BF16, "bn_fwd_dsres: bf16 only");
    const DsResidual dsr = {c_ds, scale_ds, shift_ds};
    return bn_fwd_t<bf16_t, true>(p, s, &dsr);
}
// y, idx = maxpool3x3/2 pad 1 of relu(fma(c, scale, shift)); c is [N][H][W][C] bf16
int bn_relu_maxpool_fwd(const void* c, const float* scale, const float* shift, void* y, void* idx, int N, int H, int W, int C,
                        hipStream_t s) {
    HS_REQUIRE(c && scale && shift && y && idx, "bn_relu_maxpool_fwd: null argument");
    HS_REQUIRE(C % 8 == 0 && ((uintptr_t)idx & 7) == 0, "bn_relu_maxpool_fwd: C %% 8 != 0 or unaligned arg-max buffer");
    const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
    const long long total = (long long)N * P * Q * (C / 8);
    const int blocks = (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(blocks), dim3(256), 0, s, (const bf16_t*)c, scale, shift, (bf16_t*)y,
                       (unsigned char*)idx, N, H, W, C, P, Q);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
// hs_batchnorm_bwd of relu(bn(x)) whose incoming gradient is the max-pool backward of p->dy ([N][P][Q][C], arg-max idx) over
// the [N][H][W][C] map x: the gradient map is formed in registers.  relu = 1, the mask comes from x (p->scale / p->shift).
int bn_bwd_pooled(const hs_bn_bwd_params* p, const void* idx, int N, int H, int W, hipStream_t s) {
    HS_REQUIRE(p && p->dy && p->x && p->dbeta && p->dgamma && p->scale && p->shift && idx && !p->dres, "bn_bwd_pooled: null argument");
    HS_REQUIRE(p->dtype == HS_BF16 && p->relu && p->C % 8 == 0 && ((uintptr_t)idx & 7) == 0 && p->partial_rows <= 0,
               "bn_bwd_pooled: bf16, relu, C %% 8 == 0");
    HS_REQUIRE(p->M == (long long)N * H * W && p->M < (1ll << 31), "bn_bwd_pooled: M != N*H*W");
    const GradPooled src = {(const unsigned char*)idx, {H, W, (H + 2 - 3) / 2 + 1, (W + 2 - 3) / 2 + 1}};
    return bn_bwd_run<bf16_t, GradPooled, false>("bn_bwd_pooled", p, nullptr, nullptr, src, s);
}
// workspace bytes one BatchNorm of bn_bwd_pair needs (partials + coefficients)
long long bn_bwd_pair_ws_bytes(long long M, int C) { return bn_bwd_ws_bytes(col_geom(M, C, 8).gy, C); }
// p: a block's last stage, y = relu(bn(x) + identity), mask y > 0; pd: the BatchNorm (no relu) of the downsample branch that made
// the identity, whose incoming gradient is p's dz.  Three launches do what hs_batchnorm_bwd(p) (with dres) followed by
// hs_batchnorm_bwd(pd) (dy = dres) do in six, and dres is never stored.  pd->dy and p->dres are not used.
int bn_bwd_pair(const hs_bn_bwd_params* p, const hs_bn_bwd_params* pd, hipStream_t s) {
    HS_REQUIRE(p && pd && p->dy && p->y && p->x && p->dx && p->dbeta && p->dgamma && pd->x && pd->dx && pd->dbeta && pd->dgamma,
               "bn_bwd_pair: null argument");
    HS_REQUIRE(p->dtype == HS_BF16 && pd->dtype == HS_BF16 && p->relu && !pd->relu && p->C == pd->C && p->M == pd->M && p->C % 8 == 0 &&
                   p->training == pd->training && p->partial_rows <= 0,
               "bn_bwd_pair: the two BatchNorms must share M, C and mode (bf16)");
    return bn_bwd_run<bf16_t, GradStored, true>("bn_bwd_pair", p, pd, p->y, GradStored{}, s);
}
long long bn_ws_bytes(long long M, int C, int dtype) {
    ColGeom g = col_geom(M, C, dtype == HS_BF16 ? 8 : 4);
    // partials (3 floats/channel/row block; up to one row per 64-row GEMM tile when the convolution supplies them) + bwd
    // coefficients
    // (+ the merge rows of a GEMM that also finishes the statistics: one per 32 tile rows, hs_gemm_bn_finish_rows)
    const long long tiles = (M + 63) / 64;
    const long long rows = std::max<long long>(g.gy, tiles + (tiles + 31) / 32);
    return rows * C * 3 * 4 + bn_bwd_ws_bytes(0, C);
}

// ============================================================================================
// LayerNorm: one wave per row, row cached in registers (H <= 64 * E * LN_MAXV)
// ============================================================================================
constexpr int LN_MAXV = 4;   // chunks per lane: H <= 64*8*4 = 2048 (bf16) / 1024 (f32)

template <typename T, int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     long long M, int H, float eps, const int* __restrict__ nrows) {
    constexpr int E = Chunk<T>::N;
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= packed_rows(nrows, M)) return;
    const int nch = H / E;
    float v[NV][E];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            Chunk<T>::unpack(*(const u32x4*)(x + row * H + (long long)c * E), v[i]);
#pragma unroll
            for (int e = 0; e < E; ++e) sum += v[i][e];
        }
    }
    const float mean = wave_sum(sum) / (float)H;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float d = v[i][e] - mean;
                sq += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)H + eps);
    if (lane == 0) {
        if (mean_out) mean_out[row] = mean;
        if (rstd_out) rstd_out[row] = rstd;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            float o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) o[e] = (v[i][e] - mean) * rstd * gamma[c * E + e] + beta[c * E + e];
            *(u32x4*)(y + row * H + (long long)c * E) = Chunk<T>::pack(o);
        }
    }
}

// backward: each wave walks rows (stride = total waves), writes dx and keeps per-lane dgamma/dbeta
// partials; the block's four waves merge theirs through LDS into ws[block][2][H]; a second kernel reduces over blocks.
// PRE (compile time): also emit what the layer in front of this LayerNorm needs -- dxd = dx * dropout mask (the forward
// applied dropout to that layer's output before the residual add) and the column sums of dxd (its bias gradient), as
// a third partial row.
template <typename T, int NV, bool PRE>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, T* __restrict__ dx,
                                                     float* __restrict__ ws, long long M_pad, int H, T* __restrict__ dxd,
                                                     unsigned thresh, float inv_keep, unsigned long long seed,
                                                     const int* __restrict__ inv) {
    // packed rows (inv != NULL): the walk is over PADDED rows; row r lives at packed row inv[r] and is left out where inv[r] < 0.
    // The padded tower's gradient is an exact zero there, so every partial sum below gets the terms it gets in the padded tower, in
    // the same order, and the dropout draw is that of the padded row.  (A wave without rows still writes its zero partials.)
    // Contraction is off and the fused multiply-adds are written out (fmaf): left to itself the compiler fused the f32
    // instances without PRE differently from NV = 2 on, so hs_layernorm_bwd and hs_layernorm_bwd_pre gave dx that differed
    // in the last bit.  What is fused below (dgamma and the two steps of dx; s2 is not) is what every other instance already
    // compiled to, so their results are bit for bit what they were.
#pragma clang fp contract(off)
    const long long M = M_pad;
    constexpr int E = Chunk<T>::N;
    constexpr int NP = PRE ? 3 : 2;          // partial rows per block: dgamma, dbeta (, bias gradient)
    float dbs[PRE ? NV : 1][E];
#pragma unroll
    for (int i = 0; i < (PRE ? NV : 1); ++i)
#pragma unroll
        for (int e = 0; e < E; ++e) dbs[i][e] = 0.f;
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    const int nch = H / E;
    float dg[NV][E], db[NV][E], gm[NV][E];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            dg[i][e] = db[i][e] = 0.f;
            const int c = lane + 64 * i;
            gm[i][e] = c < nch ? gamma[c * E + e] : 0.f;
        }
    for (long long prow = wid; prow < M; prow += nw) {
        long long row = prow;
        if (inv) {
            row = __builtin_amdgcn_readfirstlane(inv[prow]);
            if (row < 0 || row >= M) continue;                   // (wave-uniform)
        }
        const float mu = mean[row], rs = rstd[row];
        const unsigned long long drow = (unsigned long long)prow;
        float g[NV][E], xh[NV][E];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float xv[E];
                Chunk<T>::unpack(*(const u32x4*)(dy + row * H + (long long)c * E), g[i]);
                Chunk<T>::unpack(*(const u32x4*)(x + row * H + (long long)c * E), xv);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    xh[i][e] = (xv[e] - mu) * rs;
                    dg[i][e] = fmaf(g[i][e], xh[i][e], dg[i][e]);
                    db[i][e] += g[i][e];
                    const float gg = g[i][e] * gm[i][e];
                    s1 += gg;
                    s2 += gg * xh[i][e];
                }
            }
        }
        s1 = wave_sum(s1) / (float)H;
        s2 = wave_sum(s2) / (float)H;
        if (dx || PRE) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = lane + 64 * i;
                if (c < nch) {
                    float o[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) o[e] = rs * fmaf(-xh[i][e], s2, fmaf(g[i][e], gm[i][e], -s1));
                    if (dx) *(u32x4*)(dx + row * H + (long long)c * E) = Chunk<T>::pack(o);
                    if constexpr (PRE) {
                        if (thresh) {
#pragma unroll
                            for (int q4 = 0; q4 < E / 4; ++q4) {
                                float sc[4];
                                dropout_scale4(seed, drow * H + (unsigned long long)c * E + 4 * q4, thresh, inv_keep, sc);
#pragma unroll
                                for (int k = 0; k < 4; ++k) o[4 * q4 + k] *= sc[k];
                            }
                        }
                        if (dxd) *(u32x4*)(dxd + row * H + (long long)c * E) = Chunk<T>::pack(o);
#pragma unroll
                        for (int e = 0; e < E; ++e) dbs[i][e] += o[e];
                    }
                }
            }
        }
    }
    // merge the four waves of the block in a fixed order through LDS, then one partial row per block
    extern __shared__ float ln_sh[];   // [NP][H]
    const int wv = threadIdx.x >> 6;
    for (int turn = 0; turn < 4; ++turn) {
        if (wv == turn) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = lane + 64 * i;
                if (c < nch) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const int k = c * E + e;
                        if (turn == 0) {
                            ln_sh[k] = dg[i][e];
                            ln_sh[H + k] = db[i][e];
                            if constexpr (PRE) ln_sh[2 * H + k] = dbs[i][e];
                        } else {
                            ln_sh[k] += dg[i][e];
                            ln_sh[H + k] += db[i][e];
                            if constexpr (PRE) ln_sh[2 * H + k] += dbs[i][e];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < NP * H; k += 256) ws[(long long)blockIdx.x * NP * H + k] = ln_sh[k];
}
template <int CW>
__global__ __launch_bounds__(256) void ln_bwd_final_kernel(const float* __restrict__ ws, int nw, int H, int np,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ dbias) {
    // block = CW columns x RG = 256/CW row groups; the RG partial sums are merged through LDS in a fixed order.
    // CW = 16 gives H/16 workgroups (48 for BERT-base instead of 12 at CW = 64: the 1.5 MB of partials of a 4096-row
    // call were read by 12 CUs) with 64-byte row segments.
    // partial row w holds np (2 or 3) vectors of H floats: dgamma, dbeta(, bias gradient of the preceding layer)
    constexpr int RG = 256 / CW;
    __shared__ float sh[3][RG][CW];
    const int cl = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int c = blockIdx.x * CW + cl;
    float acc[3] = {0.f, 0.f, 0.f};
    if (c < H) {
        int w = rg;
        for (; w + 3 * RG < nw; w += 4 * RG) {   // 4 independent loads in flight per accumulator
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k < np) {
                    const float v0 = ws[((long long)w * np + k) * H + c], v1 = ws[((long long)(w + RG) * np + k) * H + c];
                    const float v2 = ws[((long long)(w + 2 * RG) * np + k) * H + c];
                    const float v3 = ws[((long long)(w + 3 * RG) * np + k) * H + c];
                    acc[k] += (v0 + v1) + (v2 + v3);
                }
            }
        }
        for (; w < nw; w += RG)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < np) acc[k] += ws[((long long)w * np + k) * H + c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sh[k][rg][cl] = acc[k];
    __syncthreads();
    if (rg < 3 && rg < np && c < H) {             // row group k merges vector k
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < RG; ++r) t += sh[rg][r][cl];
        if (rg == 0) dgamma[c] = t;
        else if (rg == 1) dbeta[c] = t;
        else if (dbias) dbias[c] = t;
    }
}

static int ln_bwd_blocks(long long M) {
    long long b = (M + 15) / 16;   // >= 4 rows per wave
    if (b > 512) b = 512;          // 2 workgroups per CU
    if (b < 1) b = 1;
    return (int)b;
}

template <typename T>
static int ln_fwd_t(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                    long long M, int H, float eps, hipStream_t s, const int* nrows) {
    constexpr int E = Chunk<T>::N;
    HS_REQUIRE(H % E == 0 && H <= 64 * E * LN_MAXV, "layernorm: H=%d unsupported for this dtype", H);
    // NV = 16-byte chunks per lane (registers scale with it: H = 768 in bf16 needs 2, not the maximum of 4)
    const int nv = ceil_div(H / E, 64);
#define LN_FWD(NVV) hipLaunchKernelGGL((ln_fwd_kernel<T, NVV>), dim3(ceil_div(M, 4)), dim3(256), 0, s, (const T*)x, gamma, beta, (T*)y, mean, rstd, M, H, eps, nrows)
    if (nv <= 1) LN_FWD(1);
    else if (nv == 2) LN_FWD(2);
    else if (nv == 3) LN_FWD(3);
    else LN_FWD(4);
#undef LN_FWD
    HS_LAUNCH_CHECK();
    return HS_OK;
}
template <typename T>
static int ln_bwd_t(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                    void* dx, float* dgamma, float* dbeta, float* ws, long long ws_bytes, long long M, int H,
                    hipStream_t s, bool pre = false, void* dxd = nullptr, float* dbias = nullptr, float p = 0.f,
                    unsigned long long seed = 0, const int* inv = nullptr) {
    constexpr int E = Chunk<T>::N;
    HS_REQUIRE(H % E == 0 && H <= 64 * E * LN_MAXV, "layernorm_bwd: H=%d unsupported for this dtype", H);
    const int blocks = ln_bwd_blocks(M);
    const int np = pre ? 3 : 2;
    HS_REQUIRE(ws && ws_bytes >= (long long)blocks * np * H * 4, "layernorm_bwd: workspace too small");
    const int nv = ceil_div(H / E, 64);
    const unsigned th = (pre && p > 0.f) ? dropout_thresh(p) : 0u;
    const float ik = (pre && p > 0.f) ? 1.f / (1.f - p) : 1.f;
#define LN_BWD(NVV, PRE)                                                                                                  \
    hipLaunchKernelGGL((ln_bwd_kernel<T, NVV, PRE>), dim3(blocks), dim3(256), np * H * sizeof(float), s, (const T*)dy,     \
                       (const T*)x, gamma, mean, rstd, (T*)dx, ws, M, H, (T*)dxd, th, ik, seed, inv)
    if (pre) {
        if (nv <= 1) LN_BWD(1, true);
        else if (nv == 2) LN_BWD(2, true);
        else if (nv == 3) LN_BWD(3, true);
        else LN_BWD(4, true);
    } else {
        if (nv <= 1) LN_BWD(1, false);
        else if (nv == 2) LN_BWD(2, false);
        else if (nv == 3) LN_BWD(3, false);
        else LN_BWD(4, false);
    }
#undef LN_BWD
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ln_bwd_final_kernel<16>, dim3(ceil_div(H, 16)), dim3(256), 0, s, ws, blocks, H, np, dgamma, dbeta, dbias);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

// nrows (forward) / inv (backward): packed rows, see packed_rows and ln_bwd_kernel; NULL = every row
int ln_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
           long long M, int H, float eps, hipStream_t s, const int* nrows) {
    HS_REQUIRE(x && gamma && beta && y, "layernorm: null argument");
    return dtype == HS_BF16 ? ln_fwd_t<bf16_t>(x, gamma, beta, y, mean, rstd, M, H, eps, s, nrows)
                            : ln_fwd_t<float>(x, gamma, beta, y, mean, rstd, M, H, eps, s, nrows);
}
int ln_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
           void* dx, float* dgamma, float* dbeta, float* ws, long long ws_bytes, long long M, int H, hipStream_t s,
           const int* inv) {
    HS_REQUIRE(dy && x && gamma && mean && rstd && dgamma && dbeta, "layernorm_bwd: null argument");
    return dtype == HS_BF16 ? ln_bwd_t<bf16_t>(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, ws_bytes, M, H, s, false, nullptr, nullptr, 0.f, 0, inv)
                            : ln_bwd_t<float>(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, ws_bytes, M, H, s, false, nullptr, nullptr, 0.f, 0, inv);
}
// LayerNorm backward that also serves the layer in front of it: dx_dropped = dx * dropout mask(p, seed, element index)
// (p = 0: dx itself; may be NULL) and dbias = column sums of dx_dropped.
int ln_bwd_pre(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
               float* dgamma, float* dbeta, void* dx_dropped, float* dbias, float p, unsigned long long seed, float* ws,
               long long ws_bytes, long long M, int H, hipStream_t s, const int* inv) {
    HS_REQUIRE(dy && x && gamma && mean && rstd && dgamma && dbeta, "layernorm_bwd_pre: null argument");
    HS_REQUIRE(p >= 0.f && p < 1.f, "layernorm_bwd_pre: bad dropout probability");
    return dtype == HS_BF16
               ? ln_bwd_t<bf16_t>(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, ws_bytes, M, H, s, true, dx_dropped, dbias, p, seed, inv)
               : ln_bwd_t<float>(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, ws_bytes, M, H, s, true, dx_dropped, dbias, p, seed, inv);
}
long long ln_bwd_ws_bytes(long long M, int H) { return (long long)ln_bwd_blocks(M) * 3 * H * 4; }

}  // namespace hs

extern "C" {
hs_status hs_batchnorm_fwd(const hs_bn_params* p, void* stream) { return hs::bn_fwd(p, (hipStream_t)stream); }
hs_status hs_batchnorm_bwd(const hs_bn_bwd_params* p, void* stream) { return hs::bn_bwd(p, (hipStream_t)stream); }
int64_t hs_batchnorm_ws_bytes(int64_t M, int32_t C, int32_t dtype) { return hs::bn_ws_bytes(M, C, dtype); }
hs_status hs_layernorm_fwd(int32_t dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean,
                           float* rstd, int64_t M, int32_t H, float eps, void* stream) {
    return hs::ln_fwd(dtype, x, gamma, beta, y, mean, rstd, M, H, eps, (hipStream_t)stream, nullptr);
}
hs_status hs_layernorm_bwd(int32_t dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                           const float* rstd, void* dx, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes,
                           int64_t M, int32_t H, void* stream) {
    return hs::ln_bwd(dtype, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, (float*)ws, ws_bytes, M, H,
                      (hipStream_t)stream, nullptr);
}
hs_status hs_layernorm_bwd_pre(int32_t dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                               const float* rstd, void* dx, float* dgamma, float* dbeta, void* dx_dropped, float* dbias,
                               float dropout_p, uint64_t seed, void* ws, int64_t ws_bytes, int64_t M, int32_t H, void* stream) {
    return hs::ln_bwd_pre(dtype, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dx_dropped, dbias, dropout_p, seed, (float*)ws,
                          ws_bytes, M, H, (hipStream_t)stream, nullptr);
}
int64_t hs_layernorm_bwd_ws_bytes(int64_t M, int32_t H) { return hs::ln_bwd_ws_bytes(M, H); }
}
