// Mamba block of the SSM fusion (reference modules/fusion_blocks.py:264-292 -> mamba_ssm.Mamba, d_state 16, d_conv 4) and of the
// multimodal Mamba blocks (reference ConNexT/models/block/len4mamba.py:74-79,138-143, d_state 128): causal depthwise conv1d +
// SiLU, the selective scan, the broadcast add of the text feature and the token sequence of len4mamba; forward and backward.
//
// Scan mapping, described for d_state 16 (S = 1; for more states see chunk_for below): 16 lanes per (batch, channel) pair,
// lane = state index n.  One 64-lane wave carries 4 channels, a 256-thread block 16 consecutive channels of one batch
// element.  The per-step sum over the 16 states is four DPP adds inside one 16-lane row (no LDS, no ds_bpermute), Bm_t / Cm_t
// are one 16-wide load that the four rows of a wave share, and B*d/4 waves (8192 at B 64, d 512: 32 per CU) hide the latency
// of the dependent chain over L.  The price is that the per-channel scalars (softplus, SiLU) are computed by all 16 lanes of
// a row.
//
// Backward: the forward keeps h only after every full chunk of kChunk steps; the backward walks the chunks last to first,
// recomputes the kChunk states of a chunk into registers and then runs the reverse recurrence over them.
// Reductions: over states -> DPP row sum; over the channels of a block (dBm, dCm) -> wave shuffles + LDS, then per-block
// partials that a second kernel adds in block order; over batch and time (dA_log, dD, ddt_bias) -> registers over time, then
// per-batch partials added in batch order by the same second kernel.  No atomics anywhere.
//
// MambaVision's mixer (reference ConNexT/models/block/mamba_vision.py:1527-1636, built with d_state 8 at 1719-1723) scans 8
// states without the silu(z) gate.  That is the same kernel with two more compile-time parameters: LN = 8 lanes per (batch,
// channel) pair, so a wave carries 8 channels and a block 32, and the state sum is three DPP adds inside a half row; GATE =
// false drops z from the forward and dz from the backward.  Only <S = 1, LN = 8, GATE = false> is instantiated besides the
// 16-lane gated kernels, whose code the two parameters leave as it was.
#include <algorithm>
#include "hs_common.h"

namespace hs {

// Lane n of the 16 lanes of a (batch, channel) pair holds the S = N / 16 consecutive states n*S .. n*S + S - 1 in registers
// (N = d_state in {16, 32, 64, 128, 256}; ConNexT/models/block/len4mamba.py:74-79,138-143 builds d_state 128).  S = 1 is the
// kernel of the SSM fusion.  chunk_for(S): steps between saved states; the backward keeps chunk x S recomputed states in
// registers, so the chunk shrinks as S grows (at most 64 of them).  steps_for(S): steps whose operands the forward requests
// together (2 S values per step and lane).
static constexpr int kLanes = 16;
__host__ __device__ constexpr int chunk_for(int S) { return S <= 4 ? 16 : (S == 8 ? 8 : 4); }
__host__ __device__ constexpr int steps_for(int S) { return S <= 8 ? 4 : 2; }
static constexpr int kChunk = chunk_for(1);

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }
// torch.nn.functional.softplus (threshold 20); log1pf keeps the relative precision of small dt
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(__expf(x)); }

// sum over the 16 lanes of a DPP row; every lane of the row ends with the same bits
__device__ __forceinline__ float row_sum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));  // row_mirror
    return v;
}
// the same over the 8 lanes of a half row: row_half_mirror stays inside 8 lanes, so three adds finish it
__device__ __forceinline__ float row_sum8(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    return v;
}
template <int LN> __device__ __forceinline__ float state_sum(float v) {
    if constexpr (LN == 8) return row_sum8(v);
    else return row_sum16(v);
}

// ------------------------------------------------------------------------------------------------------------
// causal depthwise conv1d (k = 4) + bias + SiLU
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void causal_conv1d_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                                const float* __restrict__ bias, T* __restrict__ y, int ldy,
                                                                long long rows, int L, int d) {
    const long long n = rows * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / d;
        const int c = (int)(i - r * d);
        const int t = (int)(r % L);
        float s = bias[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int back = 3 - j;     // tap j reads x[t - 3 + j]
            if (t >= back) s = fmaf(w[c * 4 + j], to_f32(x[(r - back) * ldx + c]), s);
        }
        y[r * ldy + c] = from_f32<T>(s * sigmoid_f(s));
    }
}

// One thread per (b, c) walks time once: g_t = dy_t * silu'(s_t); dx_t = sum_j w[j] g[t+3-j]; dw[j] += g_t x[t-3+j]; db += g_t.
// part: [B][5][d] (4 taps + bias).
template <typename T>
__global__ __launch_bounds__(256) void causal_conv1d_bwd_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ x,
                                                                int ldx, const float* __restrict__ w,
                                                                const float* __restrict__ bias, T* __restrict__ dx, int lddx,
                                                                float* __restrict__ part, int B, int L, int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * d) return;
    const int b = i / d, c = i - b * d;
    const float w0 = w[c * 4], w1 = w[c * 4 + 1], w2 = w[c * 4 + 2], w3 = w[c * 4 + 3], bs = bias[c];
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;        // x[t-3], x[t-2], x[t-1]
    float g1 = 0.f, g2 = 0.f, g3 = 0.f;        // g[t-1], g[t-2], g[t-3]
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, ab = 0.f;
    const long long r0 = (long long)b * L;
    for (int t = 0; t < L + 3; ++t) {
        float g = 0.f;
        if (t < L) {
            const float xt = to_f32(x[(r0 + t) * ldx + c]);
            const float s = fmaf(w3, xt, fmaf(w2, x2, fmaf(w1, x1, fmaf(w0, x0, bs))));
            const float sg = sigmoid_f(s);
            g = to_f32(dy[(r0 + t) * lddy + c]) * sg * (1.f + s * (1.f - sg));
            a0 = fmaf(g, x0, a0);
            a1 = fmaf(g, x1, a1);
            a2 = fmaf(g, x2, a2);
            a3 = fmaf(g, xt, a3);
            ab += g;
            x0 = x1; x1 = x2; x2 = xt;
        }
        // dx[t-3] = w3 g[t-3] + w2 g[t-2] + w1 g[t-1] + w0 g[t]
        if (t >= 3) dx[(r0 + t - 3) * lddx + c] = from_f32<T>(fmaf(w3, g3, fmaf(w2, g2, fmaf(w1, g1, w0 * g))));
        g3 = g2; g2 = g1; g1 = g;
    }
    float* p = part + (long long)b * 5 * d + c;
    p[0] = a0; p[d] = a1; p[2 * d] = a2; p[3 * d] = a3; p[4 * d] = ab;
}
__global__ void causal_conv1d_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                int B, int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 5 * d) return;
    const int j = i / d, c = i - j * d;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += part[((long long)b * 5 + j) * d + c];
    if (j < 4) dw[c * 4 + j] = acc;
    else db[c] = acc;
}

// ------------------------------------------------------------------------------------------------------------
// selective scan
// ------------------------------------------------------------------------------------------------------------
// the S states of one lane as 16-byte (or smaller) loads; the S = 1 case is one scalar load
template <typename T, int S> struct alignas(S * sizeof(T) < 16 ? S * sizeof(T) : 16) StatePack {
    T e[(S * sizeof(T) < 16 ? S * sizeof(T) : 16) / sizeof(T)];
};
template <typename T, int S>
__device__ __forceinline__ void load_states(const T* __restrict__ p, float (&v)[S]) {
    using P = StatePack<T, S>;
    constexpr int kPer = sizeof(P) / sizeof(T);
#pragma unroll
    for (int i = 0; i < S / kPer; ++i) {
        const P q = reinterpret_cast<const P*>(p)[i];
#pragma unroll
        for (int j = 0; j < kPer; ++j) v[i * kPer + j] = to_f32(q.e[j]);
    }
}
template <int S>
__device__ __forceinline__ void store_states(float* __restrict__ p, const float (&v)[S]) {
    using P = StatePack<float, S>;
    constexpr int kPer = sizeof(P) / sizeof(float);
#pragma unroll
    for (int i = 0; i < S / kPer; ++i) {
        P q;
#pragma unroll
        for (int j = 0; j < kPer; ++j) q.e[j] = v[i * kPer + j];
        reinterpret_cast<P*>(p)[i] = q;
    }
}

template <typename T, int S, int LN = kLanes, bool GATE = true>
__global__ __launch_bounds__(256) void selective_scan_fwd_kernel(const T* __restrict__ u, int ldu, const T* __restrict__ dt,
                                                                 int lddt, const float* __restrict__ dt_bias,
                                                                 const float* __restrict__ A_log, const T* __restrict__ Bm,
                                                                 const T* __restrict__ Cm, int ldbc, const float* __restrict__ D,
                                                                 const T* __restrict__ z, int ldz, T* __restrict__ out, int ldo,
                                                                 float* __restrict__ hck, int L, int d) {
    constexpr int N = LN * S, kCh = chunk_for(S), kSt = steps_for(S);
    const int n = threadIdx.x & (LN - 1);
    const int ch = blockIdx.x * (256 / LN) + threadIdx.x / LN;
    const bool valid = ch < d;
    const int cc = valid ? ch : d - 1;          // lanes past the last channel compute on a copy and store nothing
    const int b = blockIdx.y;
    const long long r0 = (long long)b * L;
    float A[S], h[S];
    load_states<float, S>(A_log + (cc * N + n * S), A);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        A[s] = -__expf(A[s]);
        h[s] = 0.f;
    }
    const float Dv = D[cc], bias = dt_bias[cc];
    const int nck = (L - 1) / kCh;
    for (int t0 = 0; t0 < L; t0 += kSt) {
        float uu[kSt], rr[kSt], bb[kSt][S], cv[kSt][S], zz[kSt];
#pragma unroll
        for (int j = 0; j < kSt; ++j) {         // the steps' operands are requested together
            const long long r = r0 + min(t0 + j, L - 1);
            uu[j] = to_f32(u[r * ldu + cc]);
            rr[j] = to_f32(dt[r * lddt + cc]);
            load_states<T, S>(Bm + (r * ldbc + n * S), bb[j]);
            load_states<T, S>(Cm + (r * ldbc + n * S), cv[j]);
            if constexpr (GATE) zz[j] = to_f32(z[r * ldz + cc]);
        }
#pragma unroll
        for (int j = 0; j < kSt; ++j) {
            const int t = t0 + j;
            if (t < L) {
                const float dl = softplus_f(rr[j] + bias);
                float p;                        // the lane's S products first, the row sum finishes
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    h[s] = fmaf(__expf(dl * A[s]), h[s], dl * bb[j][s] * uu[j]);
                    p = s == 0 ? h[0] * cv[j][0] : fmaf(h[s], cv[j][s], p);
                }
                const float y = state_sum<LN>(p) + Dv * uu[j];
                if constexpr (GATE) {
                    if (n == 0 && valid) out[(r0 + t) * ldo + ch] = from_f32<T>(y * zz[j] * sigmoid_f(zz[j]));
                } else {
                    if (n == 0 && valid) out[(r0 + t) * ldo + ch] = from_f32<T>(y);
                }
                if (hck && ((t + 1) % kCh) == 0 && t + 1 < L && valid)
                    store_states<S>(hck + (((((long long)b * nck) + (t + 1) / kCh - 1) * d + ch) * N + n * S), h);
            }
        }
    }
}

// part_bc: [nblk][B*L][2N] (dBm | dCm summed over the 256 / LN channels of a block); part_p: [B][d][N + 2] (dA_log[N], dD,
// ddt_bias)
template <typename T, int S, int LN = kLanes, bool GATE = true>
__global__ __launch_bounds__(256) void selective_scan_bwd_kernel(
    const T* __restrict__ dout, int lddo, const T* __restrict__ u, int ldu, const T* __restrict__ dt, int lddt,
    const float* __restrict__ dt_bias, const float* __restrict__ A_log, const T* __restrict__ Bm, const T* __restrict__ Cm,
    int ldbc, const float* __restrict__ D, const T* __restrict__ z, int ldz, const float* __restrict__ hck, T* __restrict__ du,
    int lddu, T* __restrict__ ddt, int ldddt, T* __restrict__ dz, int lddz, float* __restrict__ part_bc,
    float* __restrict__ part_p, int B, int L, int d) {
    constexpr int N = LN * S, kCh = chunk_for(S);
    __shared__ float sbc[4][kCh][2 * N];
    const int tid = threadIdx.x;
    constexpr int kSh = LN == 8 ? 3 : 4;        // log2(LN)
    const int n = tid & (LN - 1), wave = tid >> 6, lane = tid & 63;
    const int ch = blockIdx.x * (256 / LN) + (tid >> kSh);
    const bool valid = ch < d;
    const int cc = valid ? ch : d - 1;
    const int b = blockIdx.y;
    const long long r0 = (long long)b * L;
    const long long rows = (long long)B * L;
    float A[S], dh[S], accA[S];
    load_states<float, S>(A_log + (cc * N + n * S), A);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        A[s] = -__expf(A[s]);
        dh[s] = 0.f;
        accA[s] = 0.f;
    }
    const float Dv = D[cc], bias = dt_bias[cc];
    const int nchunks = (L + kCh - 1) / kCh;
    const int nck = nchunks - 1;
    float accD = 0.f, accB = 0.f;
    for (int c = nchunks - 1; c >= 0; --c) {
        const int t0 = c * kCh;
        const int len = min(kCh, L - t0);       // the same for the whole block
        float hs[kCh][S];                        // hs[i]: the state before step t0 + i
        {
            float h[S];
#pragma unroll
            for (int s = 0; s < S; ++s) h[s] = 0.f;
            if (c > 0) load_states<float, S>(hck + ((((long long)b * nck + (c - 1)) * d + cc) * N + n * S), h);
#pragma unroll
            for (int i = 0; i < kCh; ++i) {
#pragma unroll
                for (int s = 0; s < S; ++s) hs[i][s] = h[s];
                if (i < len - 1) {               // the state after the chunk's last step is not needed here
                    const long long r = r0 + t0 + i;
                    const float dl = softplus_f(to_f32(dt[r * lddt + cc]) + bias);
                    float bn[S];
                    load_states<T, S>(Bm + (r * ldbc + n * S), bn);
                    const float uv = to_f32(u[r * ldu + cc]);
#pragma unroll
                    for (int s = 0; s < S; ++s) h[s] = fmaf(__expf(dl * A[s]), h[s], dl * bn[s] * uv);
                }
            }
        }
#pragma unroll
        for (int i = kCh - 1; i >= 0; --i) {
            if (i < len) {
                const long long r = r0 + t0 + i;
                const float uv = to_f32(u[r * ldu + cc]);
                const float pre = to_f32(dt[r * lddt + cc]) + bias;
                float bn[S], cn[S];
                load_states<T, S>(Bm + (r * ldbc + n * S), bn);
                load_states<T, S>(Cm + (r * ldbc + n * S), cn);
                const float zv = GATE ? to_f32(z[r * ldz + cc]) : 0.f;
                const float g = to_f32(dout[r * lddo + cc]);
                const float dl = softplus_f(pre);
                float a[S], ht[S], p;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    a[s] = __expf(dl * A[s]);
                    ht[s] = fmaf(a[s], hs[i][s], dl * bn[s] * uv);
                    p = s == 0 ? ht[0] * cn[0] : fmaf(ht[s], cn[s], p);
                }
                const float y = state_sum<LN>(p) + Dv * uv;
                const float sz = sigmoid_f(zv);
                const float dy = GATE ? g * zv * sz : g;      // without the gate out_t = y_t; y, sz and dzv are then dead
                const float dzv = g * y * sz * (1.f + zv * (1.f - sz));
                float p1, p2;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    dh[s] = fmaf(dy, cn[s], dh[s]);               // d loss / d h_t
                    p1 = s == 0 ? dh[0] * bn[0] : fmaf(dh[s], bn[s], p1);
                    p2 = s == 0 ? dh[0] * hs[i][0] * a[0] * A[0] : fmaf(dh[s] * hs[i][s] * a[s], A[s], p2);
                }
                const float s1 = state_sum<LN>(p1);
                const float s2 = state_sum<LN>(p2);
                const float dr = (uv * s1 + s2) * sigmoid_f(pre);     // through delta = softplus(dt + bias)
#pragma unroll
                for (int s = 0; s < S; ++s) accA[s] = fmaf(dh[s] * hs[i][s], a[s] * dl, accA[s]);
                accD = fmaf(dy, uv, accD);
                accB += dr;
                if (n == 0 && valid) {
                    du[r * lddu + ch] = from_f32<T>(fmaf(dy, Dv, dl * s1));
                    ddt[r * ldddt + ch] = from_f32<T>(dr);
                    if constexpr (GATE) dz[r * lddz + ch] = from_f32<T>(dzv);
                }
                // dBm_t[n], dCm_t[n]: sum over the wave's 64 / LN channels here, over the block's 4 waves below
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    float vb = valid ? dh[s] * dl * uv : 0.f;
                    float vc = valid ? dy * ht[s] : 0.f;
                    if constexpr (LN == 8) {
                        vb += __shfl_xor(vb, 8, 64);
                        vc += __shfl_xor(vc, 8, 64);
                    }
                    vb += __shfl_xor(vb, 16, 64);
                    vc += __shfl_xor(vc, 16, 64);
                    vb += __shfl_xor(vb, 32, 64);
                    vc += __shfl_xor(vc, 32, 64);
                    if (lane < LN) {
                        sbc[wave][i][n * S + s] = vb;
                        sbc[wave][i][N + n * S + s] = vc;
                    }
                    dh[s] *= a[s];                                // carried to step t - 1
                }
            }
        }
        __syncthreads();
        for (int e = tid; e < len * 2 * N; e += 256) {
            const int i = e / (2 * N), j = e % (2 * N);
            const float s = (sbc[0][i][j] + sbc[1][i][j]) + (sbc[2][i][j] + sbc[3][i][j]);
            part_bc[((long long)blockIdx.x * rows + r0 + t0 + i) * (2 * N) + j] = s;
        }
        __syncthreads();
    }
    if (valid) {
        float* p = part_p + ((long long)b * d + ch) * (N + 2);
#pragma unroll
        for (int s = 0; s < S; ++s) p[n * S + s] = accA[s] * A[s];    // dA/dA_log = A
        if (n == 0) {
            p[N] = accD;
            p[N + 1] = accB;
        }
    }
}
// sh = log2(2N): N is a power of two
template <typename T>
__global__ void selective_scan_bwd_reduce_kernel(const float* __restrict__ part_bc, const float* __restrict__ part_p, int nblk,
                                                 long long rows, int B, int d, int N, int sh, T* __restrict__ dBm,
                                                 T* __restrict__ dCm, int lddbc, float* __restrict__ dA_log,
                                                 float* __restrict__ dD, float* __restrict__ ddt_bias) {
    const int np1 = N + 2;
    const long long nbc = rows << sh, np = (long long)d * np1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nbc + np; i += (long long)gridDim.x * 256) {
        if (i < nbc) {
            float acc = 0.f;
            for (int k = 0; k < nblk; ++k) acc += part_bc[(long long)k * nbc + i];
            const long long r = i >> sh;
            const int j = (int)(i & (2 * N - 1));
            if (j < N) dBm[r * lddbc + j] = from_f32<T>(acc);
            else dCm[r * lddbc + j - N] = from_f32<T>(acc);
        } else {
            const long long e = i - nbc;
            const int c = (int)(e / np1), j = (int)(e - (long long)c * np1);
            float acc = 0.f;
            for (int b = 0; b < B; ++b) acc += part_p[((long long)b * d + c) * np1 + j];
            if (j < N) dA_log[c * N + j] = acc;
            else if (j == N) dD[c] = acc;
            else ddt_bias[c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// tokens + text feature
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void add_token_bias_kernel(const T* __restrict__ x, const float* __restrict__ v, T* __restrict__ o, int B, int L,
                                      int H) {
    const long long n = (long long)B * L * H;
    const long long per = (long long)L * H;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        o[i] = from_f32<T>(to_f32(x[i]) + v[(i / per) * H + i % H]);
}
template <typename T>
__global__ void add_token_bias_bwd_kernel(const T* __restrict__ dy, float* __restrict__ dv, int B, int L, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, h = i - b * H;
    float acc = 0.f;
    for (int t = 0; t < L; ++t) acc += to_f32(dy[((long long)b * L + t) * H + h]);
    dv[i] = acc;
}

// ------------------------------------------------------------------------------------------------------------
// token sequence of the multimodal Mamba blocks (reference ConNexT/models/block/len4mamba.py:86-106,147-168), f32
// ------------------------------------------------------------------------------------------------------------
// dst[b][c][r] = src[b][r][c]: the (B, C, P) image feature as the (B P, C) rows the projection GEMM reads; its own backward
__global__ __launch_bounds__(256) void transpose_batched_kernel(const float* __restrict__ src, float* __restrict__ dst, int R,
                                                                int C) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const long long base = (long long)blockIdx.z * R * C;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < R && c < C) tile[k][tx] = src[base + (long long)r * C + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < R && c < C) dst[base + (long long)c * R + r] = tile[tx][k];
    }
}
// seq[b] = [text[b]; img[b][0..P-1]; first[b]; last[b]] + pe[0..P+2], every row H wide
__global__ void token_seq_assemble_kernel(const float* __restrict__ text, const float* __restrict__ img,
                                          const float* __restrict__ first, const float* __restrict__ last,
                                          const float* __restrict__ pe, float* __restrict__ seq, int B, int P, int H) {
    const int Lt = P + 3;
    const long long n = (long long)B * Lt * H;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int h = (int)(i % H);
        const long long row = i / H;
        const int t = (int)(row % Lt);
        const long long b = row / Lt;
        float v;
        if (t == 0) v = text[b * H + h];
        else if (t <= P) v = img[(b * P + t - 1) * H + h];
        else if (t == P + 1) v = first[b * H + h];
        else v = last[b * H + h];
        seq[i] = v + pe[(long long)t * H + h];
    }
}
__global__ void token_seq_assemble_bwd_kernel(const float* __restrict__ dseq, float* __restrict__ dtext, float* __restrict__ dimg,
                                              float* __restrict__ dfirst, float* __restrict__ dlast, int B, int P, int H) {
    const int Lt = P + 3;
    const long long n = (long long)B * Lt * H;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int h = (int)(i % H);
        const long long row = i / H;
        const int t = (int)(row % Lt);
        const long long b = row / Lt;
        const float g = dseq[i];
        if (t == 0) { if (dtext) dtext[b * H + h] = g; }
        else if (t <= P) { if (dimg) dimg[(b * P + t - 1) * H + h] = g; }
        else if (t == P + 1) { if (dfirst) dfirst[b * H + h] = g; }
        else if (dlast) dlast[b * H + h] = g;
    }
}

// ------------------------------------------------------------------------------------------------------------
// MambaVision mixer and stage (reference ConNexT/models/block/mamba_vision.py): centred depthwise conv1d (k = 3) + SiLU, and the
// window partition / reverse between the NCHW feature map and the token rows
// ------------------------------------------------------------------------------------------------------------
// y[t] = silu(bias + w[0] x[t-1] + w[1] x[t] + w[2] x[t+1]), x = 0 outside [0, L) (padding='same'); bias may be NULL
template <typename T>
__global__ __launch_bounds__(256) void conv1d_same_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                              const float* __restrict__ bias, T* __restrict__ y, int ldy,
                                                              long long rows, int L, int d) {
    const long long n = rows * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / d;
        const int c = (int)(i - r * d);
        const int t = (int)(r % L);
        float s = bias ? bias[c] : 0.f;
        if (t > 0) s = fmaf(w[c * 3], to_f32(x[(r - 1) * ldx + c]), s);
        s = fmaf(w[c * 3 + 1], to_f32(x[r * ldx + c]), s);
        if (t + 1 < L) s = fmaf(w[c * 3 + 2], to_f32(x[(r + 1) * ldx + c]), s);
        y[r * ldy + c] = from_f32<T>(s * sigmoid_f(s));
    }
}
// One thread per (b, c) walks time once, one step behind the loads: g_t = dy_t * silu'(s_t) needs x[t+1];
// dx_t = w[0] g[t+1] + w[1] g[t] + w[2] g[t-1]; dw[j] += g_t x[t-1+j]; db += g_t.  part: [B][4][d] (3 taps + bias).
template <typename T>
__global__ __launch_bounds__(256) void conv1d_same_bwd_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ x, int ldx,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              T* __restrict__ dx, int lddx, float* __restrict__ part, int B, int L,
                                                              int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * d) return;
    const int b = i / d, c = i - b * d;
    const float w0 = w[c * 3], w1 = w[c * 3 + 1], w2 = w[c * 3 + 2], bs = bias ? bias[c] : 0.f;
    float xm2 = 0.f, xm1 = 0.f;                 // x[t-2], x[t-1]
    float g1 = 0.f, g2 = 0.f;                   // g[t-2], g[t-3]
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, ab = 0.f;
    const long long r0 = (long long)b * L;
    for (int t = 0; t < L + 2; ++t) {
        const float xt = t < L ? to_f32(x[(r0 + t) * ldx + c]) : 0.f;
        float g = 0.f;                          // g[t-1]
        if (t >= 1 && t <= L) {
            const float s = fmaf(w2, xt, fmaf(w1, xm1, fmaf(w0, xm2, bs)));
            const float sg = sigmoid_f(s);
            g = to_f32(dy[(r0 + t - 1) * lddy + c]) * sg * (1.f + s * (1.f - sg));
            a0 = fmaf(g, xm2, a0);
            a1 = fmaf(g, xm1, a1);
            a2 = fmaf(g, xt, a2);
            ab += g;
        }
        // dx[t-2] = w0 g[t-1] + w1 g[t-2] + w2 g[t-3]
        if (t >= 2) dx[(r0 + t - 2) * lddx + c] = from_f32<T>(fmaf(w2, g2, fmaf(w1, g1, w0 * g)));
        g2 = g1; g1 = g;
        xm2 = xm1; xm1 = xt;
    }
    float* p = part + (long long)b * 4 * d + c;
    p[0] = a0; p[d] = a1; p[2 * d] = a2; p[3 * d] = ab;
}
__global__ void conv1d_same_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int B,
                                              int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * d) return;
    const int j = i / d, c = i - j * d;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += part[((long long)b * 4 + j) * d + c];
    if (j < 3) dw[c * 3 + j] = acc;
    else if (db) db[c] = acc;
}

// Window partition (reference mamba_vision.py:1301-1314 after the zero padding of 1813-1816): map (B, C, H, W) f32 -> tokens
// (B nWh nWw, ws ws, C) of T.  Per window a transpose of [C][ws ws gathered positions] through an LDS tile, so the map side
// moves runs along W and the token side runs along C.  Token p of window (wh, ww) is the position (wh ws + p / ws, ww ws + p %
// ws); positions past H or W read as zero.  grid: (ceil(C / 32), ceil(ws ws / 32), B nWh nWw).
template <typename T>
__global__ __launch_bounds__(256) void window_partition_kernel(const float* __restrict__ map, T* __restrict__ tok, int C, int H,
                                                               int W, int ws, int nWh, int nWw) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int P = ws * ws;
    const int c0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
    const int win = blockIdx.z;
    const int ww = win % nWw, wh = (win / nWw) % nWh;
    const long long b = win / (nWw * nWh);
    const int p = p0 + tx;
    const int row = wh * ws + p / ws, col = ww * ws + p % ws;
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        float v = 0.f;
        if (c < C && p < P && row < H && col < W) v = map[((b * C + c) * H + row) * W + col];
        tile[k][tx] = v;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int q = p0 + k, c = c0 + tx;
        if (q < P && c < C) tok[((long long)win * P + q) * C + c] = from_f32<T>(tile[tx][k]);
    }
}
// Window reverse with the crop (reference mamba_vision.py:1317-1330,1825-1827): tokens of T -> map (B, C, H, W) f32; the
// tokens of padded positions are dropped.  The same grid.
template <typename T>
__global__ __launch_bounds__(256) void window_reverse_kernel(const T* __restrict__ tok, float* __restrict__ map, int C, int H, int W,
                                                             int ws, int nWh, int nWw) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int P = ws * ws;
    const int c0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
    const int win = blockIdx.z;
    const int ww = win % nWw, wh = (win / nWw) % nWh;
    const long long b = win / (nWw * nWh);
    for (int k = ty; k < 32; k += 8) {
        const int q = p0 + k, c = c0 + tx;
        if (q < P && c < C) tile[k][tx] = to_f32(tok[((long long)win * P + q) * C + c]);
    }
    __syncthreads();
    const int p = p0 + tx;
    const int row = wh * ws + p / ws, col = ww * ws + p % ws;
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        if (c < C && p < P && row < H && col < W) map[((b * C + c) * H + row) * W + col] = tile[tx][k];
    }
}

static inline int grid_for(long long n, int cap = 4096) {
    return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap));
}
static inline bool pitch_ok(int ld, int width, int esz) { return ld >= width && ((long long)ld * esz) % 16 == 0; }

#define HS_SUPPORTED(cond, ...)                                                              \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            hs::set_error(__VA_ARGS__);                                                      \
            return HS_ERR_UNSUPPORTED;                                                       \
        }                                                                                    \
    } while (0)

template <typename T, int S, int LN = kLanes, bool GATE = true>
static void launch_scan_fwd(const void* u, int ldu, const void* dt, int lddt, const float* dt_bias, const float* A_log,
                            const void* Bm, const void* Cm, int ldbc, const float* D, const void* z, int ldz, void* out, int ldo,
                            float* hck, int B, int L, int d, hipStream_t stream) {
    hipLaunchKernelGGL((selective_scan_fwd_kernel<T, S, LN, GATE>), dim3(ceil_div(d, 256 / LN), B), dim3(256), 0, stream,
                       (const T*)u, ldu,
                       (const T*)dt, lddt, dt_bias, A_log, (const T*)Bm, (const T*)Cm, ldbc, D, (const T*)z, ldz, (T*)out, ldo,
                       hck, L, d);
}
template <typename T, int S, int LN = kLanes, bool GATE = true>
static void launch_scan_bwd(const void* dout, int lddo, const void* u, int ldu, const void* dt, int lddt, const float* dt_bias,
                            const float* A_log, const void* Bm, const void* Cm, int ldbc, const float* D, const void* z, int ldz,
                            const float* hck, void* du, int lddu, void* ddt, int ldddt, void* dz, int lddz, float* part_bc,
                            float* part_p, int B, int L, int d, hipStream_t stream) {
    hipLaunchKernelGGL((selective_scan_bwd_kernel<T, S, LN, GATE>), dim3(ceil_div(d, 256 / LN), B), dim3(256), 0, stream,
                       (const T*)dout, lddo,
                       (const T*)u, ldu, (const T*)dt, lddt, dt_bias, A_log, (const T*)Bm, (const T*)Cm, ldbc, D, (const T*)z,
                       ldz, hck, (T*)du, lddu, (T*)ddt, ldddt, (T*)dz, lddz, part_bc, part_p, B, L, d);
}
// one case per supported d_state; S = N / 16
#define HS_SCAN_DISPATCH(fn, T, ...)                       \
    switch (N) {                                           \
        case 16: fn<T, 1>(__VA_ARGS__); break;             \
        case 32: fn<T, 2>(__VA_ARGS__); break;             \
        case 64: fn<T, 4>(__VA_ARGS__); break;             \
        case 128: fn<T, 8>(__VA_ARGS__); break;            \
        default: fn<T, 16>(__VA_ARGS__); break;            \
    }

}  // namespace hs

using namespace hs;

extern "C" {
hs_status hs_causal_conv1d_fwd(int32_t dtype, const void* x, int32_t ldx, const float* weight, const float* bias, void* y,
                               int32_t ldy, int32_t B, int32_t L, int32_t d, int32_t k, void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "causal_conv1d_fwd: bad dtype %d", dtype);
    HS_REQUIRE(x && weight && bias && y, "causal_conv1d_fwd: null argument");
    HS_SUPPORTED(k == 4, "causal_conv1d_fwd: kernel size %d is not supported (only 4)", k);
    HS_SUPPORTED(B > 0 && L > 0 && d > 0, "causal_conv1d_fwd: empty shape B %d L %d d %d", B, L, d);
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(ldx, d, esz) && pitch_ok(ldy, d, esz),
                 "causal_conv1d_fwd: row pitches (%d, %d) must be >= d = %d and multiples of 16 bytes", ldx, ldy, d);
    const long long rows = (long long)B * L;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(causal_conv1d_fwd_kernel<bf16_t>, dim3(grid_for(rows * d)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, ldx, weight, bias, (bf16_t*)y, ldy, rows, L, d);
    else
        hipLaunchKernelGGL(causal_conv1d_fwd_kernel<float>, dim3(grid_for(rows * d)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)x, ldx, weight, bias, (float*)y, ldy, rows, L, d);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
int64_t hs_causal_conv1d_ws_bytes(int32_t B, int32_t d) { return (int64_t)B * 5 * d * 4; }
hs_status hs_causal_conv1d_bwd(int32_t dtype, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* weight,
                               const float* bias, void* dx, int32_t lddx, float* dweight, float* dbias, void* ws,
                               int64_t ws_bytes, int32_t B, int32_t L, int32_t d, int32_t k, void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "causal_conv1d_bwd: bad dtype %d", dtype);
    HS_REQUIRE(dy && x && weight && bias && dx && dweight && dbias && ws, "causal_conv1d_bwd: null argument");
    HS_SUPPORTED(k == 4, "causal_conv1d_bwd: kernel size %d is not supported (only 4)", k);
    HS_SUPPORTED(B > 0 && L > 0 && d > 0, "causal_conv1d_bwd: empty shape B %d L %d d %d", B, L, d);
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(lddy, d, esz) && pitch_ok(ldx, d, esz) && pitch_ok(lddx, d, esz),
                 "causal_conv1d_bwd: row pitches (%d, %d, %d) must be >= d = %d and multiples of 16 bytes", lddy, ldx, lddx, d);
    HS_SUPPORTED((long long)B * d < (1ll << 31), "causal_conv1d_bwd: tensor too large");
    HS_REQUIRE(ws_bytes >= hs_causal_conv1d_ws_bytes(B, d), "causal_conv1d_bwd: workspace of %lld bytes is too small",
               (long long)ws_bytes);
    const int grid = ceil_div((long long)B * d, 256);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(causal_conv1d_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                           lddy, (const bf16_t*)x, ldx, weight, bias, (bf16_t*)dx, lddx, (float*)ws, B, L, d);
    else
        hipLaunchKernelGGL(causal_conv1d_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)dy,
                           lddy, (const float*)x, ldx, weight, bias, (float*)dx, lddx, (float*)ws, B, L, d);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(causal_conv1d_bwd_reduce_kernel, dim3(ceil_div(5ll * d, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)ws, dweight, dbias, B, d);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

// lanes per (batch, channel) pair: 8 for the gate-less d_state 8 of MambaVision's mixer, 16 otherwise
static inline int lanes_for(int N) { return N == 8 ? 8 : kLanes; }
// states per lane for a supported d_state, 0 otherwise
static inline int states_per_lane(int N) {
    return (N == 8 || N == 16 || N == 32 || N == 64 || N == 128 || N == 256) ? N / lanes_for(N) : 0;
}
int32_t hs_selective_scan_chunk_len(void) { return kChunk; }
// steps between saved states for any instantiated d_state (gated or not), -1 otherwise
static inline int chunk_len_for(int N) {
    const int S = states_per_lane(N);
    return S ? chunk_for(S) : -1;
}
// the queries with _n describe the gated kernels (N >= 16), those with _nogate the gate-less one (N = 8)
int32_t hs_selective_scan_chunk_len_n(int32_t N) { return N == 8 ? -1 : chunk_len_for(N); }
int32_t hs_selective_scan_chunk_len_nogate(int32_t N) { return N == 8 ? chunk_len_for(N) : -1; }
static int scan_args_ok(const char* who, int32_t dtype, int32_t B, int32_t L, int32_t d, int32_t N) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "%s: bad dtype %d", who, dtype);
    HS_SUPPORTED(states_per_lane(N) != 0, "%s: d_state %d is not supported (only 8 without a gate, 16, 32, 64, 128, 256)", who, N);
    HS_SUPPORTED(B > 0 && L > 0 && d > 0, "%s: empty shape B %d L %d d %d", who, B, L, d);
    HS_SUPPORTED(B <= 65535, "%s: batch %d exceeds the grid limit 65535", who, B);
    return HS_OK;
}
// the gate is compile-time: d_state 8 is instantiated without it only, every other d_state with it only
static int scan_gate_ok(const char* who, const void* z, int32_t N) {
    HS_SUPPORTED(!(N == 8 && z), "%s: d_state 8 with a gate (z != NULL) is not instantiated (only z = NULL)", who);
    HS_SUPPORTED(!(N != 8 && !z), "%s: z = NULL (no gate) is not instantiated for d_state %d (only for d_state 8)", who, N);
    return HS_OK;
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

hs_status hs_selective_scan_fwd(int32_t dtype, const void* u, int32_t ldu, const void* dt, int32_t lddt, const float* dt_bias,
                                const float* A_log, const void* Bm, const void* Cm, int32_t ldbc, const float* D, const void* z,
                                int32_t ldz, void* out, int32_t ldo, float* hck, int32_t B, int32_t L, int32_t d, int32_t N,
                                void* stream) {
    HS_PROPAGATE(scan_args_ok("selective_scan_fwd", dtype, B, L, d, N));
    HS_PROPAGATE(scan_gate_ok("selective_scan_fwd", z, N));
    HS_REQUIRE(u && dt && dt_bias && A_log && Bm && Cm && D && out, "selective_scan_fwd: null argument");
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(ldu, d, esz) && pitch_ok(lddt, d, esz) && (!z || pitch_ok(ldz, d, esz)) && pitch_ok(ldo, d, esz) &&
                     pitch_ok(ldbc, N, esz),
                 "selective_scan_fwd: row pitches (u %d, dt %d, z %d, out %d >= d = %d; Bm/Cm %d >= %d) must be multiples of 16 bytes",
                 ldu, lddt, ldz, ldo, d, ldbc, N);
    HS_SUPPORTED(N <= 16 || (aligned16(A_log) && aligned16(Bm) && aligned16(Cm) && aligned16(hck)),
                 "selective_scan_fwd: A_log, Bm, Cm and hck must be 16-byte aligned for d_state %d", N);
    if (N == 8) {
        if (dtype == HS_BF16)
            launch_scan_fwd<bf16_t, 1, 8, false>(u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, nullptr, 0, out, ldo, hck, B, L, d,
                                                 (hipStream_t)stream);
        else
            launch_scan_fwd<float, 1, 8, false>(u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, nullptr, 0, out, ldo, hck, B, L, d,
                                                (hipStream_t)stream);
    } else if (dtype == HS_BF16) {
        HS_SCAN_DISPATCH(launch_scan_fwd, bf16_t, u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, z, ldz, out, ldo, hck, B, L,
                         d, (hipStream_t)stream);
    } else {
        HS_SCAN_DISPATCH(launch_scan_fwd, float, u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, z, ldz, out, ldo, hck, B, L,
                         d, (hipStream_t)stream);
    }
    HS_LAUNCH_CHECK();
    return HS_OK;
}
static int64_t scan_ws_bytes(int32_t B, int32_t L, int32_t d, int32_t N) {
    if (!states_per_lane(N)) return -1;
    const long long nblk = ceil_div(d, 256 / lanes_for(N));
    return (nblk * B * L * 2 * N + (long long)B * d * (N + 2)) * 4;
}
int64_t hs_selective_scan_ws_bytes_n(int32_t B, int32_t L, int32_t d, int32_t N) { return N == 8 ? -1 : scan_ws_bytes(B, L, d, N); }
int64_t hs_selective_scan_ws_bytes_nogate(int32_t B, int32_t L, int32_t d, int32_t N) {
    return N == 8 ? scan_ws_bytes(B, L, d, N) : -1;
}
int64_t hs_selective_scan_ws_bytes(int32_t B, int32_t L, int32_t d) { return hs_selective_scan_ws_bytes_n(B, L, d, 16); }
hs_status hs_selective_scan_bwd(int32_t dtype, const void* dout, int32_t lddo, const void* u, int32_t ldu, const void* dt,
                                int32_t lddt, const float* dt_bias, const float* A_log, const void* Bm, const void* Cm,
                                int32_t ldbc, const float* D, const void* z, int32_t ldz, const float* hck, void* du, int32_t lddu,
                                void* ddt, int32_t ldddt, void* dBm, void* dCm, int32_t lddbc, void* dz, int32_t lddz,
                                float* dA_log, float* dD, float* ddt_bias, void* ws, int64_t ws_bytes, int32_t B, int32_t L,
                                int32_t d, int32_t N, void* stream) {
    HS_PROPAGATE(scan_args_ok("selective_scan_bwd", dtype, B, L, d, N));
    HS_PROPAGATE(scan_gate_ok("selective_scan_bwd", z, N));
    HS_REQUIRE(dout && u && dt && dt_bias && A_log && Bm && Cm && D && du && ddt && dBm && dCm && (dz || !z) && dA_log && dD &&
                   ddt_bias && ws && (hck || L <= chunk_len_for(N)),
               "selective_scan_bwd: null argument");
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(lddo, d, esz) && pitch_ok(ldu, d, esz) && pitch_ok(lddt, d, esz) && (!z || pitch_ok(ldz, d, esz)) &&
                     pitch_ok(lddu, d, esz) && pitch_ok(ldddt, d, esz) && (!z || pitch_ok(lddz, d, esz)) && pitch_ok(ldbc, N, esz) &&
                     pitch_ok(lddbc, N, esz),
                 "selective_scan_bwd: row pitches must cover their rows (d = %d, Bm/Cm %d) and be multiples of 16 bytes", d, N);
    HS_SUPPORTED(N <= 16 || (aligned16(A_log) && aligned16(Bm) && aligned16(Cm) && aligned16(hck)),
                 "selective_scan_bwd: A_log, Bm, Cm and hck must be 16-byte aligned for d_state %d", N);
    HS_REQUIRE(ws_bytes >= scan_ws_bytes(B, L, d, N), "selective_scan_bwd: workspace of %lld bytes is too small",
               (long long)ws_bytes);
    const int nblk = ceil_div(d, 256 / lanes_for(N));
    const long long rows = (long long)B * L;
    float* part_bc = (float*)ws;
    float* part_p = part_bc + (long long)nblk * rows * 2 * N;
    int sh = 0;
    while ((1 << sh) < 2 * N) ++sh;
    const int rgrid = grid_for(rows * 2 * N + (long long)d * (N + 2));
    if (N == 8) {
        if (dtype == HS_BF16)
            launch_scan_bwd<bf16_t, 1, 8, false>(dout, lddo, u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, nullptr, 0, hck, du,
                                                 lddu, ddt, ldddt, nullptr, 0, part_bc, part_p, B, L, d, (hipStream_t)stream);
        else
            launch_scan_bwd<float, 1, 8, false>(dout, lddo, u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, nullptr, 0, hck, du,
                                                lddu, ddt, ldddt, nullptr, 0, part_bc, part_p, B, L, d, (hipStream_t)stream);
        HS_LAUNCH_CHECK();
        if (dtype == HS_BF16)
            hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<bf16_t>, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, part_bc,
                               part_p, nblk, rows, B, d, N, sh, (bf16_t*)dBm, (bf16_t*)dCm, lddbc, dA_log, dD, ddt_bias);
        else
            hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<float>, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, part_bc,
                               part_p, nblk, rows, B, d, N, sh, (float*)dBm, (float*)dCm, lddbc, dA_log, dD, ddt_bias);
    } else if (dtype == HS_BF16) {
        HS_SCAN_DISPATCH(launch_scan_bwd, bf16_t, dout, lddo, u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, z, ldz, hck, du,
                         lddu, ddt, ldddt, dz, lddz, part_bc, part_p, B, L, d, (hipStream_t)stream);
        HS_LAUNCH_CHECK();
        hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<bf16_t>, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, part_bc,
                           part_p, nblk, rows, B, d, N, sh, (bf16_t*)dBm, (bf16_t*)dCm, lddbc, dA_log, dD, ddt_bias);
    } else {
        HS_SCAN_DISPATCH(launch_scan_bwd, float, dout, lddo, u, ldu, dt, lddt, dt_bias, A_log, Bm, Cm, ldbc, D, z, ldz, hck, du,
                         lddu, ddt, ldddt, dz, lddz, part_bc, part_p, B, L, d, (hipStream_t)stream);
        HS_LAUNCH_CHECK();
        hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<float>, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, part_bc,
                           part_p, nblk, rows, B, d, N, sh, (float*)dBm, (float*)dCm, lddbc, dA_log, dD, ddt_bias);
    }
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_add_token_bias_fwd(int32_t dtype, const void* x, const float* v, void* out, int32_t B, int32_t L, int32_t H,
                                void* stream) {
    HS_REQUIRE((dtype == HS_F32 || dtype == HS_BF16) && x && v && out && B > 0 && L > 0 && H > 0,
               "add_token_bias_fwd: bad argument");
    const long long n = (long long)B * L * H;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(add_token_bias_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                           v, (bf16_t*)out, B, L, H);
    else
        hipLaunchKernelGGL(add_token_bias_kernel<float>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x, v,
                           (float*)out, B, L, H);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
hs_status hs_add_token_bias_bwd(int32_t dtype, const void* dy, float* dv, int32_t B, int32_t L, int32_t H, void* stream) {
    HS_REQUIRE((dtype == HS_F32 || dtype == HS_BF16) && dy && dv && B > 0 && L > 0 && H > 0 && (long long)B * H < (1ll << 31),
               "add_token_bias_bwd: bad argument");
    const int grid = ceil_div((long long)B * H, 256);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(add_token_bias_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                           dv, B, L, H);
    else
        hipLaunchKernelGGL(add_token_bias_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)dy, dv,
                           B, L, H);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_transpose_batched_f32(const float* src, float* dst, int32_t B, int32_t R, int32_t Cc, void* stream) {
    HS_REQUIRE(src && dst && B > 0 && R > 0 && Cc > 0, "transpose_batched_f32: bad argument");
    HS_SUPPORTED(B <= 65535 && ceil_div(R, 32) <= 65535, "transpose_batched_f32: B %d or R %d exceeds the grid limit", B, R);
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(ceil_div(Cc, 32), ceil_div(R, 32), B), dim3(256), 0, (hipStream_t)stream,
                       src, dst, R, Cc);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
hs_status hs_token_seq_assemble_fwd(const float* text, const float* img, const float* first, const float* last, const float* pe,
                                    float* seq, int32_t B, int32_t P, int32_t H, void* stream) {
    HS_REQUIRE(text && img && first && last && pe && seq && B > 0 && P > 0 && H > 0, "token_seq_assemble_fwd: bad argument");
    hipLaunchKernelGGL(token_seq_assemble_kernel, dim3(grid_for((long long)B * (P + 3) * H)), dim3(256), 0, (hipStream_t)stream,
                       text, img, first, last, pe, seq, B, P, H);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
hs_status hs_token_seq_assemble_bwd(const float* dseq, float* dtext, float* dimg, float* dfirst, float* dlast, int32_t B,
                                    int32_t P, int32_t H, void* stream) {
    HS_REQUIRE(dseq && B > 0 && P > 0 && H > 0, "token_seq_assemble_bwd: bad argument");
    hipLaunchKernelGGL(token_seq_assemble_bwd_kernel, dim3(grid_for((long long)B * (P + 3) * H)), dim3(256), 0,
                       (hipStream_t)stream, dseq, dtext, dimg, dfirst, dlast, B, P, H);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_conv1d_same_silu_fwd(int32_t dtype, const void* x, int32_t ldx, const float* weight, const float* bias, void* y,
                                  int32_t ldy, int32_t B, int32_t L, int32_t d, int32_t k, void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "conv1d_same_silu_fwd: bad dtype %d", dtype);
    HS_REQUIRE(x && weight && y, "conv1d_same_silu_fwd: null argument");
    HS_SUPPORTED(k == 3, "conv1d_same_silu_fwd: kernel size %d is not supported (only 3)", k);
    HS_SUPPORTED(B > 0 && L > 0 && d > 0, "conv1d_same_silu_fwd: empty shape B %d L %d d %d", B, L, d);
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(ldx, d, esz) && pitch_ok(ldy, d, esz),
                 "conv1d_same_silu_fwd: row pitches (%d, %d) must be >= d = %d and multiples of 16 bytes", ldx, ldy, d);
    const long long rows = (long long)B * L;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(conv1d_same_fwd_kernel<bf16_t>, dim3(grid_for(rows * d)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, ldx, weight, bias, (bf16_t*)y, ldy, rows, L, d);
    else
        hipLaunchKernelGGL(conv1d_same_fwd_kernel<float>, dim3(grid_for(rows * d)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)x, ldx, weight, bias, (float*)y, ldy, rows, L, d);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
int64_t hs_conv1d_same_silu_ws_bytes(int32_t B, int32_t d) { return (int64_t)B * 4 * d * 4; }
hs_status hs_conv1d_same_silu_bwd(int32_t dtype, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* weight,
                                  const float* bias, void* dx, int32_t lddx, float* dweight, float* dbias, void* ws,
                                  int64_t ws_bytes, int32_t B, int32_t L, int32_t d, int32_t k, void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "conv1d_same_silu_bwd: bad dtype %d", dtype);
    HS_REQUIRE(dy && x && weight && dx && dweight && ws && (!bias == !dbias), "conv1d_same_silu_bwd: null argument");
    HS_SUPPORTED(k == 3, "conv1d_same_silu_bwd: kernel size %d is not supported (only 3)", k);
    HS_SUPPORTED(B > 0 && L > 0 && d > 0, "conv1d_same_silu_bwd: empty shape B %d L %d d %d", B, L, d);
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(lddy, d, esz) && pitch_ok(ldx, d, esz) && pitch_ok(lddx, d, esz),
                 "conv1d_same_silu_bwd: row pitches (%d, %d, %d) must be >= d = %d and multiples of 16 bytes", lddy, ldx, lddx, d);
    HS_SUPPORTED((long long)B * d < (1ll << 31), "conv1d_same_silu_bwd: tensor too large");
    HS_REQUIRE(ws_bytes >= hs_conv1d_same_silu_ws_bytes(B, d), "conv1d_same_silu_bwd: workspace of %lld bytes is too small",
               (long long)ws_bytes);
    const int grid = ceil_div((long long)B * d, 256);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(conv1d_same_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, lddy,
                           (const bf16_t*)x, ldx, weight, bias, (bf16_t*)dx, lddx, (float*)ws, B, L, d);
    else
        hipLaunchKernelGGL(conv1d_same_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)dy, lddy,
                           (const float*)x, ldx, weight, bias, (float*)dx, lddx, (float*)ws, B, L, d);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv1d_same_bwd_reduce_kernel, dim3(ceil_div(4ll * d, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)ws, dweight, dbias, B, d);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

static int window_args_ok(const char* who, int32_t dtype, const void* a, const void* b, int32_t B, int32_t C, int32_t H, int32_t W,
                          int32_t ws) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "%s: bad dtype %d", who, dtype);
    HS_REQUIRE(a && b, "%s: null argument", who);
    HS_SUPPORTED(B > 0 && C > 0 && H > 0 && W > 0 && ws > 0, "%s: empty shape B %d C %d H %d W %d window %d", who, B, C, H, W, ws);
    const long long nwin = (long long)B * ceil_div(H, ws) * ceil_div(W, ws);
    HS_SUPPORTED(nwin <= 65535 && ceil_div((long long)ws * ws, 32) <= 65535 && (long long)C * H * W < (1ll << 31),
                 "%s: %lld windows of %d x %d exceed the grid limit 65535", who, nwin, ws, ws);
    return HS_OK;
}
hs_status hs_window_partition(int32_t dtype, const float* map, void* tokens, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ws,
                              void* stream) {
    HS_PROPAGATE(window_args_ok("window_partition", dtype, map, tokens, B, C, H, W, ws));
    const int nWh = ceil_div(H, ws), nWw = ceil_div(W, ws);
    const dim3 grid(ceil_div(C, 32), ceil_div(ws * ws, 32), B * nWh * nWw);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(window_partition_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, map, (bf16_t*)tokens, C, H, W,
                           ws, nWh, nWw);
    else
        hipLaunchKernelGGL(window_partition_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, map, (float*)tokens, C, H, W, ws,
                           nWh, nWw);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
hs_status hs_window_reverse(int32_t dtype, const void* tokens, float* map, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ws,
                            void* stream) {
    HS_PROPAGATE(window_args_ok("window_reverse", dtype, tokens, map, B, C, H, W, ws));
    const int nWh = ceil_div(H, ws), nWw = ceil_div(W, ws);
    const dim3 grid(ceil_div(C, 32), ceil_div(ws * ws, 32), B * nWh * nWw);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(window_reverse_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)tokens, map, C, H,
                           W, ws, nWh, nWw);
    else
        hipLaunchKernelGGL(window_reverse_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)tokens, map, C, H, W,
                           ws, nWh, nWw);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
}
