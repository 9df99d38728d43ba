// Muon (reference scripts/train.py:262-307, `from muon import MuonWithAuxAdam`): the multi-tensor passes around the
// Newton-Schulz iteration, and the iteration itself as a sequence of hs_gemm launches (gfx950 / CDNA4 only).
//
//   prepare   m <- m + (1-beta)(g-m); u = g + beta(m-g); packed = u / (||u||_F + 1e-7)   f32 -> [rows8][cols8] of the compute dtype
//   iterate   S = b X X^T ; B = S + (c/b^2) S S ; B += a I ; X' = B X                    five times, every product on hs_gemm
//   apply     p <- p (1 - lr wd) - lr s O   (+ the bf16 weight shadow)                     [rows8][cols8] -> f32
//
// The passes are HBM-bound: 16-byte accesses wherever the parameter's row length allows them.  The norm is reduced in a fixed
// order (per-workgroup partials, then one ordered sum per workgroup of the packing pass): no floating-point atomics.
#include <algorithm>
#include <math.h>
#include "hs_common.h"

namespace hs {
namespace {

inline int ceil8(int v) { return (v + 7) / 8 * 8; }

struct MuonPrepTable {
    float* m[HS_MUON_MAX];
    const float* g[HS_MUON_MAX];
    void* x[HS_MUON_MAX];
    int rows[HS_MUON_MAX], cols[HS_MUON_MAX];
};
struct MuonApplyTable {
    float* p[HS_MUON_MAX];
    bf16_t* h[HS_MUON_MAX];
    const void* x[HS_MUON_MAX];
    int rows[HS_MUON_MAX], cols[HS_MUON_MAX];
    float step[HS_MUON_MAX];      // lr * scale
};

// the two lines every pass evaluates identically (explicit fma: the momentum pass and the packing pass must agree bitwise on u)
__device__ __forceinline__ float muon_m(float m, float g, float beta) { return __fmaf_rn(1.f - beta, g - m, m); }
__device__ __forceinline__ float muon_u(float m_new, float g, float beta) { return __fmaf_rn(beta, m_new - g, g); }

// sum over the 256 threads of a workgroup in a fixed order; every thread returns the total
__device__ __forceinline__ float block_sum_256(float v, float* lds4) {
    v = wave_sum(v);
    __syncthreads();                       // lds4 may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// pass 1: momentum in place + per-workgroup sum of squares of u.  grid (gx <= HS_MUON_PARTIALS, tensors)
__global__ __launch_bounds__(256) void muon_momentum_kernel(const MuonPrepTable t, float beta, float* partials) {
    __shared__ float lds4[4];
    const int e = blockIdx.y;
    float* m = t.m[e];
    const float* g = t.g[e];
    const long long n = (long long)t.rows[e] * t.cols[e];
    const bool al = ((((uintptr_t)m) | ((uintptr_t)g)) & 15) == 0;
    const long long n4 = al ? n / 4 : 0;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 mv = ((f32x4*)m)[i];
        const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mv[k] = muon_m(mv[k], gv[k], beta);
            const float u = muon_u(mv[k], gv[k], beta);
            acc = __fmaf_rn(u, u, acc);
        }
        ((f32x4*)m)[i] = mv;
    }
    for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gi = g[i];
        const float mi = muon_m(m[i], gi, beta);
        m[i] = mi;
        const float u = muon_u(mi, gi, beta);
        acc = __fmaf_rn(u, u, acc);
    }
    const float s = block_sum_256(acc, lds4);
    if (threadIdx.x == 0) partials[(long long)e * HS_MUON_PARTIALS + blockIdx.x] = s;
}

// pass 2: u again (from g and the updated m), divided by the norm, into the padded compute-dtype matrix.  One thread per
// 8 packed columns: one 16-byte store (bf16) or two (f32).  gx1: the number of partials pass 1 wrote per tensor.
template <typename T>
__global__ __launch_bounds__(256) void muon_pack_kernel(const MuonPrepTable t, float beta, const float* partials, int gx1) {
    __shared__ float lds4[4];
    const int e = blockIdx.y;
    const float* m = t.m[e];
    const float* g = t.g[e];
    T* x = (T*)t.x[e];
    const int rows = t.rows[e], cols = t.cols[e];
    const int r8 = (rows + 7) / 8 * 8, c8 = (cols + 7) / 8 * 8, cpr = c8 / 8;
    const float pv = (int)threadIdx.x < gx1 ? partials[(long long)e * HS_MUON_PARTIALS + threadIdx.x] : 0.f;
    const float denom = sqrtf(block_sum_256(pv, lds4)) + 1e-7f;
    const bool vec = (cols % 8 == 0) && ((((uintptr_t)m) | ((uintptr_t)g)) & 15) == 0;
    const long long chunks = (long long)r8 * cpr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / cpr), c0 = (int)(i - (long long)r * cpr) * 8;
        float u[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) u[k] = 0.f;
        if (r < rows) {
            const long long src = (long long)r * cols + c0;
            if (vec) {
                const f32x4 m0 = *(const f32x4*)(m + src), m1 = *(const f32x4*)(m + src + 4);
                const f32x4 g0 = *(const f32x4*)(g + src), g1 = *(const f32x4*)(g + src + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    u[k] = muon_u(m0[k], g0[k], beta) / denom;
                    u[4 + k] = muon_u(m1[k], g1[k], beta) / denom;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (c0 + k < cols) u[k] = muon_u(m[src + k], g[src + k], beta) / denom;
            }
        }
        T* dst = x + (long long)r * c8 + c0;
        if constexpr (sizeof(T) == 2) {
            *(u32x4*)dst = Chunk<bf16_t>::pack(u);
        } else {
            *(f32x4*)dst = f32x4{u[0], u[1], u[2], u[3]};
            *(f32x4*)(dst + 4) = f32x4{u[4], u[5], u[6], u[7]};
        }
    }
}

// B[b][i][i] += a over `count` matrices [n8][n8] of T (the value is rounded to T before and after the add)
template <typename T>
__global__ __launch_bounds__(256) void muon_diag_add_kernel(T* B, int n8, long long count, float a) {
    const long long total = count * n8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / n8;
        const int d = (int)(i - b * n8);
        T* q = B + (b * n8 + d) * (long long)n8 + d;
        *q = from_f32<T>(to_f32(*q) + a);
    }
}

// apply: one thread per 8 packed columns of a real row
template <typename T>
__global__ __launch_bounds__(256) void muon_apply_kernel(const MuonApplyTable t, float decay) {
    const int e = blockIdx.y;
    float* p = t.p[e];
    bf16_t* h = t.h[e];
    const T* x = (const T*)t.x[e];
    const int rows = t.rows[e], cols = t.cols[e];
    const int c8 = (cols + 7) / 8 * 8, cpr = c8 / 8;
    const float step = t.step[e];
    const bool vec = (cols % 4 == 0) && (((uintptr_t)p) & 15) == 0 && (((uintptr_t)h) & 7) == 0;
    const long long chunks = (long long)rows * cpr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / cpr), c0 = (int)(i - (long long)r * cpr) * 8;
        float o[8];
        const T* src = x + (long long)r * c8 + c0;
        if constexpr (sizeof(T) == 2) {
            Chunk<bf16_t>::unpack(*(const u32x4*)src, o);
        } else {
            const f32x4 a0 = *(const f32x4*)src, a1 = *(const f32x4*)(src + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { o[k] = a0[k]; o[4 + k] = a1[k]; }
        }
        const long long dst = (long long)r * cols + c0;
        if (vec) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                if (c0 + 4 * half + 4 > cols) break;
                f32x4 pv = *(f32x4*)(p + dst + 4 * half);
#pragma unroll
                for (int k = 0; k < 4; ++k) pv[k] = __fmaf_rn(-step, o[4 * half + k], pv[k] * decay);
                *(f32x4*)(p + dst + 4 * half) = pv;
                if (h) *(bf16x4*)(h + dst + 4 * half) = bf16x4{(bf16_t)pv[0], (bf16_t)pv[1], (bf16_t)pv[2], (bf16_t)pv[3]};
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (c0 + k < cols) {
                    const float pi = __fmaf_rn(-step, o[k], p[dst + k] * decay);
                    p[dst + k] = pi;
                    if (h) h[dst + k] = (bf16_t)pi;
                }
            }
        }
    }
}

inline int grid_chunks(long long work_items, int cap) {
    return (int)std::min<long long>(std::max<long long>((work_items + 255) / 256, 1), cap);
}

hs_gemm_params gemm_defaults(int dt) {
    hs_gemm_params p;
    memset(&p, 0, sizeof(p));
    p.dtype = dt;
    p.out_dtype = dt;
    p.alpha = 1.f;
    p.batch = 1;
    p.batch_inner = 1;
    return p;
}

constexpr float kNsA = 3.4445f, kNsB = -4.7750f, kNsC = 2.0315f;
constexpr int kNsSteps = 5;
inline long long align256(long long v) { return (v + 255) / 256 * 256; }

// the three products of one iteration for `cnt` matrices; split-K factors for a single matrix
struct NsShape {
    int r8, c8, n8;
    bool transposed;
    int split[3];
};
NsShape ns_shape(int dtype, int count, int rows, int cols) {
    NsShape s;
    s.r8 = ceil8(rows);
    s.c8 = ceil8(cols);
    s.transposed = rows > cols;
    s.n8 = s.transposed ? s.c8 : s.r8;
    const int k8 = s.transposed ? s.r8 : s.c8;
    s.split[0] = count == 1 ? hs_gemm_suggest_split(s.n8, s.n8, k8, dtype) : 1;
    s.split[1] = count == 1 ? hs_gemm_suggest_split(s.n8, s.n8, s.n8, dtype) : 1;
    s.split[2] = count == 1 ? hs_gemm_suggest_split(s.r8, s.c8, s.n8, dtype) : 1;
    return s;
}
long long ns_split_bytes(const NsShape& s) {
    long long b = 0;
    const long long mn[3] = {(long long)s.n8 * s.n8, (long long)s.n8 * s.n8, (long long)s.r8 * s.c8};
    for (int i = 0; i < 3; ++i) {
        if (s.split[i] <= 1) continue;
        hs_gemm_params p = gemm_defaults(HS_F32);
        p.split_k = s.split[i];
        p.M = 1;
        p.N = 1;
        b = std::max<long long>(b, hs_gemm_splitk_ws_bytes(&p) * mn[i]);
    }
    return b;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

hs_status hs_muon_prepare_multi(int32_t dtype, int32_t count, float* const* momentum, const float* const* grads,
                                void* const* packed, const int32_t* rows, const int32_t* cols, float beta, float* partials,
                                void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "muon_prepare: bad dtype %d", dtype);
    HS_REQUIRE(count >= 0 && (count == 0 || (momentum && grads && packed && rows && cols && partials)), "muon_prepare: null argument");
    for (int base = 0; base < count; base += HS_MUON_MAX) {
        MuonPrepTable t;
        memset(&t, 0, sizeof(t));
        const int cnt = std::min(HS_MUON_MAX, count - base);
        long long mx = 0, mxc = 0;
        for (int i = 0; i < cnt; ++i) {
            const int j = base + i;
            HS_REQUIRE(momentum[j] && grads[j] && packed[j] && rows[j] > 0 && cols[j] > 0, "muon_prepare: bad tensor %d", j);
            HS_REQUIRE((((uintptr_t)packed[j]) & 15) == 0, "muon_prepare: packed matrix %d is not 16-byte aligned", j);
            t.m[i] = momentum[j];
            t.g[i] = grads[j];
            t.x[i] = packed[j];
            t.rows[i] = rows[j];
            t.cols[i] = cols[j];
            mx = std::max<long long>(mx, (long long)rows[j] * cols[j]);
            mxc = std::max<long long>(mxc, (long long)ceil8(rows[j]) * (ceil8(cols[j]) / 8));
        }
        float* part = partials + (long long)base * HS_MUON_PARTIALS;
        const int gx1 = (int)std::min<long long>(std::max<long long>((mx + 4095) / 4096, 1), HS_MUON_PARTIALS);
        hipLaunchKernelGGL(muon_momentum_kernel, dim3(gx1, cnt), dim3(256), 0, (hipStream_t)stream, t, beta, part);
        HS_LAUNCH_CHECK();
        const int gx2 = grid_chunks((mxc + 1) / 2, 512);      // two chunks per thread
        if (dtype == HS_BF16)
            hipLaunchKernelGGL(muon_pack_kernel<bf16_t>, dim3(gx2, cnt), dim3(256), 0, (hipStream_t)stream, t, beta, (const float*)part, gx1);
        else
            hipLaunchKernelGGL(muon_pack_kernel<float>, dim3(gx2, cnt), dim3(256), 0, (hipStream_t)stream, t, beta, (const float*)part, gx1);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

int64_t hs_muon_ws_bytes(int32_t dtype, int32_t count, int32_t rows, int32_t cols) {
    if ((dtype != HS_F32 && dtype != HS_BF16) || count <= 0 || rows <= 0 || cols <= 0) return -1;
    const NsShape s = ns_shape(dtype, count, rows, cols);
    const long long esz = dtype == HS_BF16 ? 2 : 4;
    const long long sq = align256((long long)count * s.n8 * s.n8 * esz);
    const long long xb = align256((long long)count * s.r8 * s.c8 * esz);
    return 2 * sq + xb + align256(ns_split_bytes(s));
}

hs_status hs_muon_orthogonalize(int32_t dtype, int32_t count, int32_t rows, int32_t cols, void* X, void* ws, int64_t ws_bytes,
                                void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "muon_orthogonalize: bad dtype %d", dtype);
    HS_REQUIRE(count > 0 && rows > 0 && cols > 0 && X && ws, "muon_orthogonalize: bad argument");
    HS_REQUIRE(((((uintptr_t)X) | ((uintptr_t)ws)) & 15) == 0, "muon_orthogonalize: X and ws must be 16-byte aligned");
    HS_REQUIRE(ws_bytes >= hs_muon_ws_bytes(dtype, count, rows, cols), "muon_orthogonalize: workspace too small (%lld < %lld)",
               (long long)ws_bytes, (long long)hs_muon_ws_bytes(dtype, count, rows, cols));
    const NsShape s = ns_shape(dtype, count, rows, cols);
    const long long esz = dtype == HS_BF16 ? 2 : 4;
    const long long xe = (long long)s.r8 * s.c8, se = (long long)s.n8 * s.n8;      // elements per matrix
    char* S = (char*)ws;
    char* Bm = S + align256(count * se * esz);
    char* X2 = Bm + align256(count * se * esz);
    float* split_ws = (float*)(X2 + align256(count * xe * esz));
    // hs_gemm addresses an operand through a 2 GiB buffer descriptor and the batch index through gridDim.z
    const long long per_call = std::max<long long>(1, std::min<long long>(65535, (0x7fffff00ll - 1) / (xe * esz)));
    char* cur = (char*)X;
    char* nxt = X2;
    for (int it = 0; it < kNsSteps; ++it) {
        for (long long b0 = 0; b0 < count; b0 += per_call) {
            const int cnt = (int)std::min<long long>(per_call, count - b0);
            const char* x = cur + b0 * xe * esz;
            char* sb = S + b0 * se * esz;
            char* bb = Bm + b0 * se * esz;
            // S = b X X^T (rows > cols: b X^T X, the same memory read row-contiguously)
            hs_gemm_params p = gemm_defaults(dtype);
            p.a_kind = s.transposed ? HS_A_RC : HS_A_KC;
            p.b_kind = s.transposed ? HS_B_RC : HS_B_KC;
            p.M = p.N = s.n8;
            p.K = s.transposed ? s.r8 : s.c8;
            p.A = p.B = x;
            p.a_elems = p.b_elems = cnt * xe;
            p.lda = p.ldb = s.c8;
            p.batch = cnt;
            p.a_bs0 = p.b_bs0 = xe;
            p.d_bs0 = se;
            p.D = sb; p.ldd = s.n8;
            p.alpha = kNsB;
            p.split_k = s.split[0]; p.splitk_ws = s.split[0] > 1 ? split_ws : nullptr;
            HS_PROPAGATE(hs_gemm(&p, stream));
            // B = S + (c / b^2) S S   (S is symmetric: S S = S S^T, the K-contiguous reading of both operands)
            hs_gemm_params q = gemm_defaults(dtype);
            q.a_kind = HS_A_KC; q.b_kind = HS_B_KC;
            q.M = q.N = q.K = s.n8;
            q.A = q.B = sb;
            q.a_elems = q.b_elems = cnt * se;
            q.lda = q.ldb = s.n8;
            q.batch = cnt;
            q.a_bs0 = q.b_bs0 = q.d_bs0 = se;
            q.D = bb; q.ldd = s.n8;
            q.alpha = kNsC / (kNsB * kNsB);
            q.residual = sb; q.ldr = s.n8;
            q.split_k = s.split[1]; q.splitk_ws = s.split[1] > 1 ? split_ws : nullptr;
            HS_PROPAGATE(hs_gemm(&q, stream));
            // B += a I
            const int gx = grid_chunks((long long)cnt * s.n8, 1024);
            if (dtype == HS_BF16)
                hipLaunchKernelGGL(muon_diag_add_kernel<bf16_t>, dim3(gx), dim3(256), 0, (hipStream_t)stream, (bf16_t*)bb, s.n8, (long long)cnt, kNsA);
            else
                hipLaunchKernelGGL(muon_diag_add_kernel<float>, dim3(gx), dim3(256), 0, (hipStream_t)stream, (float*)bb, s.n8, (long long)cnt, kNsA);
            HS_LAUNCH_CHECK();
            // X' = B X (rows > cols: X' = X B^T on the stored matrix, i.e. the transpose of B X^T)
            hs_gemm_params g = gemm_defaults(dtype);
            if (s.transposed) {
                g.a_kind = HS_A_KC; g.b_kind = HS_B_KC;
                g.A = x; g.a_elems = cnt * xe; g.lda = s.c8; g.a_bs0 = xe;
                g.B = bb; g.b_elems = cnt * se; g.ldb = s.n8; g.b_bs0 = se;
            } else {
                g.a_kind = HS_A_KC; g.b_kind = HS_B_RC;
                g.A = bb; g.a_elems = cnt * se; g.lda = s.n8; g.a_bs0 = se;
                g.B = x; g.b_elems = cnt * xe; g.ldb = s.c8; g.b_bs0 = xe;
            }
            g.M = s.r8; g.N = s.c8; g.K = s.n8;
            g.batch = cnt;
            g.d_bs0 = xe;
            g.D = nxt + b0 * xe * esz; g.ldd = s.c8;
            g.split_k = s.split[2]; g.splitk_ws = s.split[2] > 1 ? split_ws : nullptr;
            HS_PROPAGATE(hs_gemm(&g, stream));
        }
        std::swap(cur, nxt);
    }
    if (cur != (char*)X)       // an odd number of iterations leaves the result in the workspace copy
        HS_CHECK_HIP(hipMemcpyAsync(X, cur, (size_t)(count * xe * esz), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return HS_OK;
}

hs_status hs_muon_apply_multi(int32_t dtype, int32_t count, float* const* params, void* const* bf16_shadow,
                              const void* const* packed, const int32_t* rows, const int32_t* cols, const float* scale,
                              float lr, float weight_decay, void* stream) {
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "muon_apply: bad dtype %d", dtype);
    HS_REQUIRE(count >= 0 && (count == 0 || (params && packed && rows && cols && scale)), "muon_apply: null argument");
    const float decay = 1.f - lr * weight_decay;
    for (int base = 0; base < count; base += HS_MUON_MAX) {
        MuonApplyTable t;
        memset(&t, 0, sizeof(t));
        const int cnt = std::min(HS_MUON_MAX, count - base);
        long long mxc = 0;
        for (int i = 0; i < cnt; ++i) {
            const int j = base + i;
            HS_REQUIRE(params[j] && packed[j] && rows[j] > 0 && cols[j] > 0, "muon_apply: bad tensor %d", j);
            HS_REQUIRE((((uintptr_t)packed[j]) & 15) == 0, "muon_apply: packed matrix %d is not 16-byte aligned", j);
            t.p[i] = params[j];
            t.h[i] = bf16_shadow ? (bf16_t*)bf16_shadow[j] : nullptr;
            t.x[i] = packed[j];
            t.rows[i] = rows[j];
            t.cols[i] = cols[j];
            t.step[i] = lr * scale[j];
            mxc = std::max<long long>(mxc, (long long)rows[j] * (ceil8(cols[j]) / 8));
        }
        const int gx = grid_chunks((mxc + 1) / 2, 512);
        if (dtype == HS_BF16)
            hipLaunchKernelGGL(muon_apply_kernel<bf16_t>, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, t, decay);
        else
            hipLaunchKernelGGL(muon_apply_kernel<float>, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, t, decay);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

}  // extern "C"
