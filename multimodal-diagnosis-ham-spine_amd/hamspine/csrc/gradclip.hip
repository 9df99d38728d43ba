// Global gradient-norm clipping without a host sync (gfx950 / CDNA4 only).  Replaces torch.nn.utils.clip_grad_norm_; no
// reference counterpart (the reference trains without clipping).
//
//   sumsq    every workgroup sums the squares of its fixed share of one f32 tensor in f64 and writes ONE slot of `partials`
//   finish   one workgroup adds the slots in a fixed order and writes the record {norm, coefficient, finite, skip}
//   scale    g *= coefficient in place (the stand-alone route; the fused optimizers multiply inside their own step kernel)
//
// All three are HBM-bound passes.  Nothing is atomic and every sum has one order that depends on the grid alone, so a rerun
// repeats bitwise.  The squares and sums are f64: a square that overflows f32 (|g| > 1.8e19) is an ordinary number there, and
// the sum of 1e8 squares loses nothing that the one final rounding to f32 would keep.  At 4 bytes per element and two f64
// operations the vector f64 rate is far from a bound.
#include <algorithm>
#include <math.h>
#include "hs_common.h"

namespace hs {
namespace {

// elements per workgroup at most tensors: 256 lanes x 4 floats x 32 trips (128 KiB read per workgroup)
constexpr long long kShare = 32768;
constexpr int kMaxBlocks = 1024;          // workgroups of one tensor; beyond kShare * kMaxBlocks elements the shares grow

struct GradTable {
    float* g[HS_GRADCLIP_MAX];
    long long n[HS_GRADCLIP_MAX];
    int first[HS_GRADCLIP_MAX + 1];       // first[i]: the first workgroup (= slot) of tensor i; first[count]: the grid
};

__host__ __device__ inline long long minll(long long a, long long b) { return a < b ? a : b; }
inline int blocks_of(long long n) { return (int)std::min<long long>(std::max<long long>((n + kShare - 1) / kShare, 1), kMaxBlocks); }

// the tensor whose workgroups include `b` (first[] ascends strictly: every tensor has at least one workgroup), wave-uniform
__device__ __forceinline__ int tensor_of(const GradTable& t, int count, int b) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the share [lo, hi) of workgroup `b` of a tensor of n elements split over nb workgroups (a multiple of 4 elements each)
__device__ __forceinline__ void share_of(long long n, int nb, int b, long long& lo, long long& hi) {
    const long long per = ((n + nb - 1) / nb + 3) & ~3ll;
    lo = minll(per * b, n);
    hi = minll(lo + per, n);
}

// f64 sum over the 256 threads in a fixed order (xor tree inside a wave, then the four waves in index order); thread 0 returns it
__device__ __forceinline__ double block_sum_f64(double v, double* lds4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// A share is walked as: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail.  Serves pointers that are only
// 4-byte aligned (a gradient that is a view into a flat buffer).
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const GradTable t, int count, double* partials) {
    __shared__ double lds4[4];
    const int b = blockIdx.x;
    const int e = tensor_of(t, count, b);
    const float* g = t.g[e];
    long long lo, hi;
    share_of(t.n[e], t.first[e + 1] - t.first[e], b - t.first[e], lo, hi);
    const float* p = g + lo;
    const long long len = hi - lo;
    const long long head = minll((long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2), len);
    const long long n4 = (len - head) >> 2;
    double acc = 0.0;
    if ((long long)threadIdx.x < head) {
        const double x = (double)p[threadIdx.x];
        acc = x * x;
    }
    const f32x4* p4 = (const f32x4*)(p + head);
#pragma unroll 4
    for (long long i = threadIdx.x; i < n4; i += 256) {
        const f32x4 v = p4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x = (double)v[k];
            acc = fma(x, x, acc);
        }
    }
    const long long t0 = head + n4 * 4 + threadIdx.x;
    if (t0 < len) {
        const double x = (double)p[t0];
        acc = fma(x, x, acc);
    }
    const double s = block_sum_f64(acc, lds4);
    if (threadIdx.x == 0) partials[b] = s;
}

// one workgroup: thread i adds the slots [i * per, (i + 1) * per) in index order, the 256 sums are then added in the order of
// block_sum_f64.  rec = {norm, coefficient, finite, skip}
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* partials, long long n, float max_norm, int skip_nonfinite,
                                                               float* rec) {
    __shared__ double lds4[4];
    const long long per = (n + 255) / 256;
    const long long lo = minll(per * threadIdx.x, n), hi = minll(lo + per, n);
    double acc = 0.0;
    for (long long i = lo; i < hi; ++i) acc += partials[i];
    const double total = block_sum_f64(acc, lds4);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        const float c = max_norm / (norm + 1e-6f);
        const float coef = c > 1.0f ? 1.0f : c;           // fminf(c, 1) with a NaN kept, as torch.clamp(max=1) keeps it
        const float finite = isfinite(norm) ? 1.0f : 0.0f;
        rec[0] = norm;
        rec[1] = coef;
        rec[2] = finite;
        rec[3] = (skip_nonfinite && finite == 0.0f) ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const GradTable t, int count, const float* rec) {
    const float coef = rec[1];
    if (coef == 1.0f || rec[3] != 0.0f) return;           // nothing to scale, or a skipped step: no write traffic
    const int b = blockIdx.x;
    const int e = tensor_of(t, count, b);
    long long lo, hi;
    share_of(t.n[e], t.first[e + 1] - t.first[e], b - t.first[e], lo, hi);
    float* p = t.g[e] + lo;
    const long long len = hi - lo;
    const long long head = minll((long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2), len);
    const long long n4 = (len - head) >> 2;
    if ((long long)threadIdx.x < head) p[threadIdx.x] *= coef;
    f32x4* p4 = (f32x4*)(p + head);
#pragma unroll 4
    for (long long i = threadIdx.x; i < n4; i += 256) {
        f32x4 v = p4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= coef;
        p4[i] = v;
    }
    const long long t0 = head + n4 * 4 + threadIdx.x;
    if (t0 < len) p[t0] *= coef;
}

// fills the table; -> the grid (number of slots), or -1 for a negative size
long long fill_table(GradTable& t, int count, float* const* grads, const int64_t* n) {
    memset(&t, 0, sizeof(t));
    int at = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] < 0) return -1;
        t.g[i] = grads[i];
        t.n[i] = n[i];
        t.first[i] = at;
        at += blocks_of(n[i]);
    }
    t.first[count] = at;
    return at;
}

int table_args(const char* who, int count, const void* grads, const int64_t* n) {
    HS_REQUIRE(count >= 0 && count <= HS_GRADCLIP_MAX, "%s: count %d outside [0, %d]", who, count, HS_GRADCLIP_MAX);
    HS_REQUIRE(count == 0 || (grads && n), "%s: NULL table", who);
    for (int i = 0; i < count; ++i) {
        HS_REQUIRE(n[i] >= 0, "%s: n[%d] < 0", who, i);
        HS_REQUIRE(n[i] == 0 || ((const void* const*)grads)[i], "%s: grads[%d] is NULL", who, i);
        HS_REQUIRE(n[i] == 0 || ((uintptr_t)((const void* const*)grads)[i] & 3) == 0, "%s: grads[%d] is not 4-byte aligned", who, i);
    }
    return HS_OK;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

int64_t hs_grad_norm_partials(int32_t count, const int64_t* n) {
    if (count < 0 || count > HS_GRADCLIP_MAX || (count > 0 && !n)) return -1;
    long long total = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] < 0) return -1;
        total += blocks_of(n[i]);
    }
    return total;
}

hs_status hs_grad_sumsq_multi(int32_t count, const float* const* grads, const int64_t* n, double* partials, void* stream) {
    HS_PROPAGATE(table_args("grad_sumsq", count, grads, n));
    HS_REQUIRE(count == 0 || partials, "grad_sumsq: partials is NULL");
    HS_REQUIRE(((uintptr_t)partials & 7) == 0, "grad_sumsq: partials is not 8-byte aligned");
    if (count == 0) return HS_OK;
    GradTable t;
    const long long grid = fill_table(t, count, (float* const*)grads, n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, t, count, partials);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_grad_norm_finish(const double* partials, int64_t n_partials, float max_norm, int32_t skip_nonfinite, float* rec,
                              void* stream) {
    HS_REQUIRE(partials && rec, "grad_norm_finish: NULL pointer");
    HS_REQUIRE(((uintptr_t)partials & 7) == 0 && ((uintptr_t)rec & 3) == 0, "grad_norm_finish: misaligned pointer");
    HS_REQUIRE(max_norm >= 0.f, "grad_norm_finish: max_norm is negative or NaN");
    if (n_partials < 1) {
        hs::set_error("grad_norm_finish: n_partials %lld < 1", (long long)n_partials);
        return HS_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (long long)n_partials, max_norm,
                       (int)skip_nonfinite, rec);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_grad_scale_multi(int32_t count, float* const* grads, const int64_t* n, const float* rec, void* stream) {
    HS_PROPAGATE(table_args("grad_scale", count, grads, n));
    HS_REQUIRE(rec, "grad_scale: rec is NULL");
    if (count == 0) return HS_OK;
    GradTable t;
    const long long grid = fill_table(t, count, grads, n);
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, t, count, rec);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
