// Mamba block of the SSM fusion (reference modules/fusion_blocks.py:264-292 -> mamba_ssm.Mamba, d_state 16, d_conv 4):
// causal depthwise conv1d + SiLU, the selective scan, and the broadcast add of the text feature; forward and backward.
//
// Scan mapping: 16 lanes per (batch, channel) pair, lane = state index n.  One 64-lane wave carries 4 channels, a 256-thread
// block 16 consecutive channels of one batch element.  The per-step sum over the 16 states is four DPP adds inside one
// 16-lane row (no LDS, no ds_bpermute), Bm_t / Cm_t are one 16-wide load that the four rows of a wave share, and B*d/4 waves
// (8192 at B 64, d 512: 32 per CU) hide the latency of the dependent chain over L.  The price is that the per-channel
// scalars (softplus, SiLU) are computed by all 16 lanes of a row.
//
// Backward: the forward keeps h only after every full chunk of kChunk steps; the backward walks the chunks last to first,
// recomputes the kChunk states of a chunk into registers and then runs the reverse recurrence over them.
// Reductions: over states -> DPP row sum; over the channels of a block (dBm, dCm) -> wave shuffles + LDS, then per-block
// partials that a second kernel adds in block order; over batch and time (dA_log, dD, ddt_bias) -> registers over time, then
// per-batch partials added in batch order by the same second kernel.  No atomics anywhere.
#include <algorithm>
#include "hs_common.h"

namespace hs {

static constexpr int kChunk = 16;    // steps between saved states (= registers the backward spends on recomputed states)
static constexpr int kStates = 16;

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
template <typename T>
__global__ __launch_bounds__(256) void selective_scan_fwd_kernel(const T* __restrict__ u, int ldu, const T* __restrict__ dt,
                                                                 int lddt, const float* __restrict__ dt_bias,
                                                                 const float* __restrict__ A_log, const T* __restrict__ Bm,
                                                                 const T* __restrict__ Cm, int ldbc, const float* __restrict__ D,
                                                                 const T* __restrict__ z, int ldz, T* __restrict__ out, int ldo,
                                                                 float* __restrict__ hck, int L, int d) {
    const int n = threadIdx.x & 15;
    const int ch = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool valid = ch < d;
    const int cc = valid ? ch : d - 1;          // lanes past the last channel compute on a copy and store nothing
    const int b = blockIdx.y;
    const long long r0 = (long long)b * L;
    const float A = -__expf(A_log[cc * kStates + n]);
    const float Dv = D[cc], bias = dt_bias[cc];
    const int nck = (L - 1) / kChunk;
    float h = 0.f;
    for (int t0 = 0; t0 < L; t0 += 4) {
        float uu[4], rr[4], bb[4], cv[4], zz[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {           // the four steps' operands are requested together
            const long long r = r0 + min(t0 + j, L - 1);
            uu[j] = to_f32(u[r * ldu + cc]);
            rr[j] = to_f32(dt[r * lddt + cc]);
            bb[j] = to_f32(Bm[r * ldbc + n]);
            cv[j] = to_f32(Cm[r * ldbc + n]);
            zz[j] = to_f32(z[r * ldz + cc]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j;
            if (t < L) {
                const float dl = softplus_f(rr[j] + bias);
                h = fmaf(__expf(dl * A), h, dl * bb[j] * uu[j]);
                const float y = row_sum16(h * cv[j]) + Dv * uu[j];
                if (n == 0 && valid) out[(r0 + t) * ldo + ch] = from_f32<T>(y * zz[j] * sigmoid_f(zz[j]));
                if (hck && ((t + 1) % kChunk) == 0 && t + 1 < L && valid)
                    hck[((((long long)b * nck) + (t + 1) / kChunk - 1) * d + ch) * kStates + n] = h;
            }
        }
    }
}

// part_bc: [nblk][B*L][32] (dBm | dCm summed over the 16 channels of a block); part_p: [B][d][18] (dA_log[16], dD, ddt_bias)
template <typename T>
__global__ __launch_bounds__(256) void selective_scan_bwd_kernel(
    const T* __restrict__ dout, int lddo, const T* __restrict__ u, int ldu, const T* __restrict__ dt, int lddt,
    const float* __restrict__ dt_bias, const float* __restrict__ A_log, const T* __restrict__ Bm, const T* __restrict__ Cm,
    int ldbc, const float* __restrict__ D, const T* __restrict__ z, int ldz, const float* __restrict__ hck, T* __restrict__ du,
    int lddu, T* __restrict__ ddt, int ldddt, T* __restrict__ dz, int lddz, float* __restrict__ part_bc,
    float* __restrict__ part_p, int B, int L, int d) {
    __shared__ float sbc[4][kChunk][32];
    const int tid = threadIdx.x;
    const int n = tid & 15, wave = tid >> 6, lane = tid & 63;
    const int ch = blockIdx.x * 16 + (tid >> 4);
    const bool valid = ch < d;
    const int cc = valid ? ch : d - 1;
    const int b = blockIdx.y;
    const long long r0 = (long long)b * L;
    const long long rows = (long long)B * L;
    const float A = -__expf(A_log[cc * kStates + n]);
    const float Dv = D[cc], bias = dt_bias[cc];
    const int nchunks = (L + kChunk - 1) / kChunk;
    const int nck = nchunks - 1;
    float dh = 0.f, accA = 0.f, accD = 0.f, accB = 0.f;
    for (int c = nchunks - 1; c >= 0; --c) {
        const int t0 = c * kChunk;
        const int len = min(kChunk, L - t0);    // the same for the whole block
        float hs[kChunk];                        // hs[i]: the state before step t0 + i
        {
            float h = c > 0 ? hck[(((long long)b * nck + (c - 1)) * d + cc) * kStates + n] : 0.f;
#pragma unroll
            for (int i = 0; i < kChunk; ++i) {
                hs[i] = h;
                if (i < len - 1) {               // the state after the chunk's last step is not needed here
                    const long long r = r0 + t0 + i;
                    const float dl = softplus_f(to_f32(dt[r * lddt + cc]) + bias);
                    h = fmaf(__expf(dl * A), h, dl * to_f32(Bm[r * ldbc + n]) * to_f32(u[r * ldu + cc]));
                }
            }
        }
#pragma unroll
        for (int i = kChunk - 1; i >= 0; --i) {
            if (i < len) {
                const long long r = r0 + t0 + i;
                const float uv = to_f32(u[r * ldu + cc]);
                const float pre = to_f32(dt[r * lddt + cc]) + bias;
                const float bn = to_f32(Bm[r * ldbc + n]);
                const float cn = to_f32(Cm[r * ldbc + n]);
                const float zv = to_f32(z[r * ldz + cc]);
                const float g = to_f32(dout[r * lddo + cc]);
                const float dl = softplus_f(pre);
                const float a = __expf(dl * A);
                const float hp = hs[i];
                const float ht = fmaf(a, hp, dl * bn * uv);
                const float y = row_sum16(ht * cn) + Dv * uv;
                const float sz = sigmoid_f(zv);
                const float dy = g * zv * sz;
                const float dzv = g * y * sz * (1.f + zv * (1.f - sz));
                dh = fmaf(dy, cn, dh);                        // d loss / d h_t
                const float s1 = row_sum16(dh * bn);
                const float s2 = row_sum16(dh * hp * a * A);
                const float dr = (uv * s1 + s2) * sigmoid_f(pre);     // through delta = softplus(dt + bias)
                accA = fmaf(dh * hp, a * dl, accA);
                accD = fmaf(dy, uv, accD);
                accB += dr;
                if (n == 0 && valid) {
                    du[r * lddu + ch] = from_f32<T>(fmaf(dy, Dv, dl * s1));
                    ddt[r * ldddt + ch] = from_f32<T>(dr);
                    dz[r * lddz + ch] = from_f32<T>(dzv);
                }
                // dBm_t[n], dCm_t[n]: sum over the wave's 4 channels here, over the block's 4 waves below
                float vb = valid ? dh * dl * uv : 0.f;
                float vc = valid ? dy * ht : 0.f;
                vb += __shfl_xor(vb, 16, 64);
                vc += __shfl_xor(vc, 16, 64);
                vb += __shfl_xor(vb, 32, 64);
                vc += __shfl_xor(vc, 32, 64);
                if (lane < 16) {
                    sbc[wave][i][n] = vb;
                    sbc[wave][i][16 + n] = vc;
                }
                dh *= a;                                      // carried to step t - 1
            }
        }
        __syncthreads();
        for (int e = tid; e < len * 32; e += 256) {
            const int i = e >> 5, j = e & 31;
            const float s = (sbc[0][i][j] + sbc[1][i][j]) + (sbc[2][i][j] + sbc[3][i][j]);
            part_bc[((long long)blockIdx.x * rows + r0 + t0 + i) * 32 + j] = s;
        }
        __syncthreads();
    }
    if (valid) {
        float* p = part_p + ((long long)b * d + ch) * 18;
        p[n] = accA * A;                                       // dA/dA_log = A
        if (n == 0) {
            p[16] = accD;
            p[17] = accB;
        }
    }
}
template <typename T>
__global__ void selective_scan_bwd_reduce_kernel(const float* __restrict__ part_bc, const float* __restrict__ part_p, int nblk,
                                                 long long rows, int B, int d, T* __restrict__ dBm, T* __restrict__ dCm,
                                                 int lddbc, float* __restrict__ dA_log, float* __restrict__ dD,
                                                 float* __restrict__ ddt_bias) {
    const long long nbc = rows * 32, np = (long long)d * 18;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nbc + np; i += (long long)gridDim.x * 256) {
        if (i < nbc) {
            float acc = 0.f;
            for (int k = 0; k < nblk; ++k) acc += part_bc[(long long)k * nbc + i];
            const long long r = i >> 5;
            const int j = (int)(i & 31);
            if (j < 16) dBm[r * lddbc + j] = from_f32<T>(acc);
            else dCm[r * lddbc + j - 16] = from_f32<T>(acc);
        } else {
            const long long e = i - nbc;
            const int c = (int)(e / 18), j = (int)(e - (long long)c * 18);
            float acc = 0.f;
            for (int b = 0; b < B; ++b) acc += part_p[((long long)b * d + c) * 18 + j];
            if (j < 16) dA_log[c * 16 + j] = acc;
            else if (j == 16) dD[c] = acc;
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

int32_t hs_selective_scan_chunk_len(void) { return kChunk; }
static int scan_args_ok(const char* who, int32_t dtype, int32_t B, int32_t L, int32_t d, int32_t N) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "%s: bad dtype %d", who, dtype);
    HS_SUPPORTED(N == kStates, "%s: d_state %d is not supported (only 16)", who, N);
    HS_SUPPORTED(B > 0 && L > 0 && d > 0, "%s: empty shape B %d L %d d %d", who, B, L, d);
    HS_SUPPORTED(B <= 65535, "%s: batch %d exceeds the grid limit 65535", who, B);
    return HS_OK;
}
hs_status hs_selective_scan_fwd(int32_t dtype, const void* u, int32_t ldu, const void* dt, int32_t lddt, const float* dt_bias,
                                const float* A_log, const void* Bm, const void* Cm, int32_t ldbc, const float* D, const void* z,
                                int32_t ldz, void* out, int32_t ldo, float* hck, int32_t B, int32_t L, int32_t d, int32_t N,
                                void* stream) {
    HS_PROPAGATE(scan_args_ok("selective_scan_fwd", dtype, B, L, d, N));
    HS_REQUIRE(u && dt && dt_bias && A_log && Bm && Cm && D && z && out, "selective_scan_fwd: null argument");
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(ldu, d, esz) && pitch_ok(lddt, d, esz) && pitch_ok(ldz, d, esz) && pitch_ok(ldo, d, esz) &&
                     pitch_ok(ldbc, kStates, esz),
                 "selective_scan_fwd: row pitches (u %d, dt %d, z %d, out %d >= d = %d; Bm/Cm %d >= 16) must be multiples of 16 bytes",
                 ldu, lddt, ldz, ldo, d, ldbc);
    const dim3 grid(ceil_div(d, 16), B);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(selective_scan_fwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)u, ldu,
                           (const bf16_t*)dt, lddt, dt_bias, A_log, (const bf16_t*)Bm, (const bf16_t*)Cm, ldbc, D,
                           (const bf16_t*)z, ldz, (bf16_t*)out, ldo, hck, L, d);
    else
        hipLaunchKernelGGL(selective_scan_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)u, ldu,
                           (const float*)dt, lddt, dt_bias, A_log, (const float*)Bm, (const float*)Cm, ldbc, D, (const float*)z,
                           ldz, (float*)out, ldo, hck, L, d);
    HS_LAUNCH_CHECK();
    return HS_OK;
}
int64_t hs_selective_scan_ws_bytes(int32_t B, int32_t L, int32_t d) {
    const long long nblk = ceil_div(d, 16);
    return (nblk * B * L * 32 + (long long)B * d * 18) * 4;
}
hs_status hs_selective_scan_bwd(int32_t dtype, const void* dout, int32_t lddo, const void* u, int32_t ldu, const void* dt,
                                int32_t lddt, const float* dt_bias, const float* A_log, const void* Bm, const void* Cm,
                                int32_t ldbc, const float* D, const void* z, int32_t ldz, const float* hck, void* du, int32_t lddu,
                                void* ddt, int32_t ldddt, void* dBm, void* dCm, int32_t lddbc, void* dz, int32_t lddz,
                                float* dA_log, float* dD, float* ddt_bias, void* ws, int64_t ws_bytes, int32_t B, int32_t L,
                                int32_t d, int32_t N, void* stream) {
    HS_PROPAGATE(scan_args_ok("selective_scan_bwd", dtype, B, L, d, N));
    HS_REQUIRE(dout && u && dt && dt_bias && A_log && Bm && Cm && D && z && du && ddt && dBm && dCm && dz && dA_log && dD &&
                   ddt_bias && ws && (hck || L <= kChunk),
               "selective_scan_bwd: null argument");
    const int esz = dtype == HS_BF16 ? 2 : 4;
    HS_SUPPORTED(pitch_ok(lddo, d, esz) && pitch_ok(ldu, d, esz) && pitch_ok(lddt, d, esz) && pitch_ok(ldz, d, esz) &&
                     pitch_ok(lddu, d, esz) && pitch_ok(ldddt, d, esz) && pitch_ok(lddz, d, esz) && pitch_ok(ldbc, kStates, esz) &&
                     pitch_ok(lddbc, kStates, esz),
                 "selective_scan_bwd: row pitches must cover their rows (d = %d, Bm/Cm 16) and be multiples of 16 bytes", d);
    HS_REQUIRE(ws_bytes >= hs_selective_scan_ws_bytes(B, L, d), "selective_scan_bwd: workspace of %lld bytes is too small",
               (long long)ws_bytes);
    const int nblk = ceil_div(d, 16);
    const long long rows = (long long)B * L;
    float* part_bc = (float*)ws;
    float* part_p = part_bc + (long long)nblk * rows * 32;
    const dim3 grid(nblk, B);
    const int rgrid = grid_for(rows * 32 + (long long)d * 18);
    if (dtype == HS_BF16) {
        hipLaunchKernelGGL(selective_scan_bwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout, lddo,
                           (const bf16_t*)u, ldu, (const bf16_t*)dt, lddt, dt_bias, A_log, (const bf16_t*)Bm, (const bf16_t*)Cm,
                           ldbc, D, (const bf16_t*)z, ldz, hck, (bf16_t*)du, lddu, (bf16_t*)ddt, ldddt, (bf16_t*)dz, lddz,
                           part_bc, part_p, B, L, d);
        HS_LAUNCH_CHECK();
        hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<bf16_t>, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, part_bc,
                           part_p, nblk, rows, B, d, (bf16_t*)dBm, (bf16_t*)dCm, lddbc, dA_log, dD, ddt_bias);
    } else {
        hipLaunchKernelGGL(selective_scan_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dout, lddo,
                           (const float*)u, ldu, (const float*)dt, lddt, dt_bias, A_log, (const float*)Bm, (const float*)Cm, ldbc,
                           D, (const float*)z, ldz, hck, (float*)du, lddu, (float*)ddt, ldddt, (float*)dz, lddz, part_bc, part_p,
                           B, L, d);
        HS_LAUNCH_CHECK();
        hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<float>, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, part_bc,
                           part_p, nblk, rows, B, d, (float*)dBm, (float*)dCm, lddbc, dA_log, dD, ddt_bias);
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
}
