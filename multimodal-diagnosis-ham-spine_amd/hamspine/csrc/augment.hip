// Device-side image augmentation: the loaders' PIL transforms as kernels, bit-equal to Pillow's arithmetic.
//
//   plan    per output and axis, Pillow's resampling windows and 22-bit fixed-point bilinear coefficients (Resample.c
//           precompute_coeffs / normalize_coeffs_8bpc, f64, weights added in index order), and the output's record
//   resize  crop box -> S x S uint8: horizontal pass over the rows the vertical pass reads, rounded and clipped to uint8,
//           kept in the workspace (its height is the box's, which no LDS tile bounds), then the vertical pass
//   stats   integer sum of the L channel of the image as the contrast op meets it (integer adds: any order, same sum)
//   finish  gather through rotation (16.16 fixed point, Geometry.c affine_fixed) and flips, the colour ops in the output's
//           order with the uint8 store between them (Blend.c, Convert.c rgb2hsv / hsv2rgb), ToTensor + Normalize
//
// Every f32 / f64 expression below is rounded where the C source of Pillow rounds it, so contraction into FMAs is off
// for the whole file.
#include <math.h>
#include <stdlib.h>

#include "hs_common.h"

#pragma clang fp contract(off)

namespace hs {

static constexpr int kAugChunk = 16;         // outputs whose records travel in one plan launch's kernel argument
static constexpr int kAugLdsInts = 8192;     // bounds + coefficients of one axis are staged in LDS up to this many ints
static constexpr int kAugMaxS = 4096;
static constexpr int kAugMaxDim = 1 << 20;   // image sides and resize targets: keeps every byte count far inside int64
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };
enum { IP_SRC = 0, IP_TOP, IP_LEFT, IP_H, IP_W, IP_HFLIP, IP_VFLIP, IP_ROTATE, IP_ORDER, IP_ENABLE = IP_ORDER + 4, IP_COUNT = 16 };
enum { FP_ANGLE = 0, FP_BRIGHTNESS, FP_CONTRAST, FP_SATURATION, FP_HUE, FP_COUNT = 5 };

struct AugRec {
    long long src;            // arena byte offset of the box's first pixel
    long long plan[2];        // workspace byte offsets: axis 0 = x, 1 = y; int bounds[S][2] then int coef[S][taps]
    long long tmp;            // workspace byte offset of the horizontal pass's result [in_h][S][3]
    int pitch;                // source row pitch in bytes
    int in[2], out[2], off[2], taps[2];   // box length, resize target, first output, coefficient row length, per axis
    int hflip, vflip, rotate;
    int rot[6];               // a0 a1 a2 / a3 a4 a5 of the inverse map in 16.16
    int op[4];                // colour ops in order, -1 where the slot is empty
    float factor[3];          // brightness, contrast, saturation
    int hue_add;              // added to the uint8 hue, mod 256
};

struct AugChunk {
    AugRec rec[kAugChunk];
};

struct AugLayout {
    long long recs, lsum, resized, total;
};

static inline long long align16(long long v) { return (v + 15) & ~15LL; }

static inline int aug_grid(long long n, int cap) {
    long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// taps of one axis as Pillow sizes a coefficient row: (int)ceil(support) * 2 + 1
static int aug_taps(int in, int out) {
    double fs = (double)in / (double)out;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(fs) * 2 + 1;
}

// the part of the layout that depends on N and S alone: what the passes after plan need
static AugLayout aug_fixed_layout(int N, int S) {
    AugLayout l;
    l.recs = 0;
    l.lsum = align16((long long)N * (long long)sizeof(AugRec));
    l.resized = align16(l.lsum + (long long)N * 8);
    l.total = align16(l.resized + (long long)N * S * S * 3);
    return l;
}

// fills the workspace offsets of rec[0..N) (their in / out already set) and returns the layout
static AugLayout aug_layout(AugRec* rec, int N, int S) {
    AugLayout l = aug_fixed_layout(N, S);
    long long at = l.total;
    for (int n = 0; n < N; ++n) {
        for (int a = 0; a < 2; ++a) {
            rec[n].taps[a] = aug_taps(rec[n].in[a], rec[n].out[a]);
            rec[n].plan[a] = at;
            at = align16(at + (long long)S * (2 + rec[n].taps[a]) * 4);
        }
        rec[n].tmp = at;
        at = align16(at + (long long)rec[n].in[1] * S * 3);
    }
    l.total = at;
    return l;
}

// --------------------------------------------------------------------------------------------------------------- plan
// The arithmetic below is __host__ __device__: a host build of the same source can be held against the numpy restatement
// without a device.
// window and coefficients of output `xx` of a bilinear resize in -> out (Resample.c precompute_coeffs + normalize_coeffs_8bpc);
// k has K slots, the unused ones are zeroed
__host__ __device__ inline void aug_window(int in, int out, int xx, int K, int* k, int* pxmin, int* pxmax) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > K) xmax = K;
    if (xmax < 0) xmax = 0;
    auto weight = [&](int i) {
        double v = ((i + xmin) - center + 0.5) * ss;
        if (v < 0.0) v = -v;
        return v < 1.0 ? 1.0 - v : 0.0;
    };
    double ww = 0.0;
    for (int i = 0; i < xmax; ++i) ww += weight(i);
    for (int i = 0; i < xmax; ++i) {
        double v = weight(i);
        if (ww != 0.0) v /= ww;
        k[i] = (int)(0.5 + v * (double)(1 << 22));
    }
    for (int i = xmax; i < K; ++i) k[i] = 0;
    *pxmin = xmin;
    *pxmax = xmax;
}

__global__ void aug_plan_kernel(AugChunk c, char* __restrict__ ws, long long recs, long long lsum, int n0, int S) {
    const AugRec r = c.rec[blockIdx.x];
    const int n = n0 + blockIdx.x;
    if (threadIdx.x == 0) {
        reinterpret_cast<AugRec*>(ws + recs)[n] = r;
        reinterpret_cast<unsigned long long*>(ws + lsum)[n] = 0ull;
    }
    for (int t = threadIdx.x; t < 2 * S; t += blockDim.x) {
        const int a = t / S, x = t - a * S;
        const int in = a ? r.in[1] : r.in[0], K = a ? r.taps[1] : r.taps[0];
        const int out = a ? r.out[1] : r.out[0], off = a ? r.off[1] : r.off[0];
        int* bounds = reinterpret_cast<int*>(ws + (a ? r.plan[1] : r.plan[0]));
        int* k = bounds + 2 * S + (long long)x * K;
        int xmin, xmax;
        aug_window(in, out, off + x, K, k, &xmin, &xmax);
        bounds[2 * x] = xmin;
        bounds[2 * x + 1] = xmax;
    }
}

// ------------------------------------------------------------------------------------------------------------- resize
// bounds + coefficients of one axis: from LDS when they fit, else from the workspace
__device__ __forceinline__ const int* aug_stage_plan(const int* plan, int ints, int* lds) {
    if (ints > kAugLdsInts) return plan;
    for (int i = threadIdx.x; i < ints; i += blockDim.x) lds[i] = plan[i];
    __syncthreads();
    return lds;
}

__host__ __device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// tmp[row][x][c] = clip8((2^21 + sum_j k[x][j] * src[row][xmin + j][c]) >> 22) for the rows the vertical pass reads
__global__ void __launch_bounds__(256) aug_resize_h_kernel(const unsigned char* __restrict__ arena, char* __restrict__ ws,
                                                           long long recs, int S) {
    __shared__ int lds[kAugLdsInts];
    const AugRec r = reinterpret_cast<const AugRec*>(ws + recs)[blockIdx.y];
    const int Kx = r.taps[0];
    const int* ply = reinterpret_cast<const int*>(ws + r.plan[1]);
    const int lo = ply[0], hi = ply[2 * (S - 1)] + ply[2 * (S - 1) + 1];   // windows start in ascending order
    const int* pl = aug_stage_plan(reinterpret_cast<const int*>(ws + r.plan[0]), S * (2 + Kx), lds);
    const unsigned char* src = arena + r.src;
    unsigned char* tmp = reinterpret_cast<unsigned char*>(ws + r.tmp);
    const int row_e = S * 3;
    const long long total = (long long)(hi - lo) * row_e;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int row = lo + (int)(e / row_e), xc = (int)(e % row_e);
        const int x = xc / 3, c = xc - 3 * x;
        const int xmin = pl[2 * x], xmax = pl[2 * x + 1];
        const int* k = pl + 2 * S + (long long)x * Kx;
        const unsigned char* s = src + (long long)row * r.pitch + (long long)xmin * 3 + c;
        int acc = 1 << 21;
        for (int j = 0; j < xmax; ++j) acc += k[j] * (int)s[3 * j];
        tmp[(long long)row * row_e + xc] = (unsigned char)clip8(acc >> 22);
    }
}

// resized[n][y][x][c] = clip8((2^21 + sum_j k[y][j] * tmp[ymin + j][x][c]) >> 22)
__global__ void __launch_bounds__(256) aug_resize_v_kernel(char* __restrict__ ws, long long recs, long long resized, int S) {
    __shared__ int lds[kAugLdsInts];
    const AugRec r = reinterpret_cast<const AugRec*>(ws + recs)[blockIdx.y];
    const int Ky = r.taps[1];
    const int* pl = aug_stage_plan(reinterpret_cast<const int*>(ws + r.plan[1]), S * (2 + Ky), lds);
    const unsigned char* tmp = reinterpret_cast<const unsigned char*>(ws + r.tmp);
    unsigned char* dst = reinterpret_cast<unsigned char*>(ws + resized) + (long long)blockIdx.y * S * S * 3;
    const int row_e = S * 3;
    const long long total = (long long)S * row_e;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int y = (int)(e / row_e), xc = (int)(e % row_e);
        const int ymin = pl[2 * y], ymax = pl[2 * y + 1];
        const int* k = pl + 2 * S + (long long)y * Ky;
        const unsigned char* s = tmp + (long long)ymin * row_e + xc;
        int acc = 1 << 21;
        for (int j = 0; j < ymax; ++j) acc += k[j] * (int)s[(long long)j * row_e];
        dst[e] = (unsigned char)clip8(acc >> 22);
    }
}

// ------------------------------------------------------------------------------------------------- gather and colour
struct Rgb {
    int r, g, b;
};

// pixel (x, y) of the flipped, then rotated, resized image; 0 outside
__device__ __forceinline__ Rgb aug_gather(const AugRec& r, const unsigned char* __restrict__ img, int S, int x, int y) {
    int xin = x, yin = y;
    if (r.rotate) {
        xin = (r.rot[2] + r.rot[0] * x + r.rot[1] * y) >> 16;
        yin = (r.rot[5] + r.rot[3] * x + r.rot[4] * y) >> 16;
        if (xin < 0 || xin >= S || yin < 0 || yin >= S) return Rgb{0, 0, 0};
    }
    if (r.hflip) xin = S - 1 - xin;
    if (r.vflip) yin = S - 1 - yin;
    const unsigned char* p = img + ((long long)yin * S + xin) * 3;
    return Rgb{p[0], p[1], p[2]};
}

__host__ __device__ __forceinline__ int aug_gray(Rgb p) { return (p.r * 19595 + p.g * 38470 + p.b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate d, image x, a): f32 d + a * (x - d), product and sum rounded separately
__host__ __device__ __forceinline__ int aug_blend(int d, int x, float a) {
    const float prod = a * (float)(x - d);
    float t = (float)d + prod;
    if (!(a >= 0.f && a <= 1.f)) t = t <= 0.f ? 0.f : t >= 255.f ? 255.f : t;
    return (int)t;
}

__host__ __device__ __forceinline__ Rgb aug_blend3(Rgb d, Rgb p, float a) {
    return Rgb{aug_blend(d.r, p.r, a), aug_blend(d.g, p.g, a), aug_blend(d.b, p.b, a)};
}

__host__ __device__ __forceinline__ Rgb aug_hue(Rgb p, int add) {
    // RGB -> HSV
    const int mx = p.r > p.g ? p.r : p.g, mn = p.r < p.g ? p.r : p.g;
    const int maxc = mx > p.b ? mx : p.b, minc = mn < p.b ? mn : p.b;
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - p.r) / cr, gc = (float)(maxc - p.g) / cr, bc = (float)(maxc - p.b) / cr;
        float h;
        if (p.r == maxc) h = bc - gc;
        else if (p.g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        double hd = (double)h / 6.0 + 1.0;               // in [5/6, 11/6]: fmod(hd, 1.0) is an exact subtraction
        if (hd >= 1.0) hd -= 1.0;
        h = (float)hd;
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + add) & 255;
    // HSV -> RGB
    if (us == 0) return Rgb{uv, uv, uv};
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const float fsf = fs * f;
    const double v = (double)uv;
    const int pp = clip8((int)round(v * (1.0 - (double)fs)));
    const int q = clip8((int)round(v * (1.0 - (double)fsf)));
    const double g1 = 1.0 - (double)f;
    const double g2 = (double)fs * g1;
    const int t = clip8((int)round(v * (1.0 - g2)));
    switch (i % 6) {
        case 0: return Rgb{uv, t, pp};
        case 1: return Rgb{q, uv, pp};
        case 2: return Rgb{pp, uv, t};
        case 3: return Rgb{pp, q, uv};
        case 4: return Rgb{t, pp, uv};
        default: return Rgb{uv, pp, q};
    }
}

// one colour op on one pixel; lmean: the rounded mean of L the contrast op blends towards
__host__ __device__ __forceinline__ Rgb aug_op(const AugRec& r, int op, Rgb p, int lmean) {
    switch (op) {
        case OP_BRIGHTNESS: return aug_blend3(Rgb{0, 0, 0}, p, r.factor[0]);
        case OP_CONTRAST: return aug_blend3(Rgb{lmean, lmean, lmean}, p, r.factor[1]);
        case OP_SATURATION: {
            const int l = aug_gray(p);
            return aug_blend3(Rgb{l, l, l}, p, r.factor[2]);
        }
        case OP_HUE: return aug_hue(p, r.hue_add);
        default: return p;
    }
}

// --------------------------------------------------------------------------------------------------------------- stats
__global__ void __launch_bounds__(256) aug_stats_kernel(char* __restrict__ ws, long long recs, long long lsum, long long resized,
                                                        int S) {
    __shared__ unsigned long long part[4];
    const AugRec r = reinterpret_cast<const AugRec*>(ws + recs)[blockIdx.y];
    int upto = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (r.op[i] == OP_CONTRAST) upto = i;
    if (upto < 0) return;                                  // the same in every thread of the block
    const unsigned char* img = reinterpret_cast<const unsigned char*>(ws + resized) + (long long)blockIdx.y * S * S * 3;
    unsigned long long acc = 0;
    const int total = S * S;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int y = i / S, x = i - y * S;
        Rgb p = aug_gather(r, img, S, x, y);
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (o < upto) p = aug_op(r, r.op[o], p, 0);
        acc += (unsigned long long)aug_gray(p);
    }
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(ws + lsum) + blockIdx.y, part[0] + part[1] + part[2] + part[3]);
}

// -------------------------------------------------------------------------------------------------------------- finish
struct AugNorm {
    float mean[3], std[3];
};

__global__ void __launch_bounds__(256) aug_finish_kernel(const char* __restrict__ ws, long long recs, long long lsum,
                                                         long long resized, float* __restrict__ out, int S, AugNorm nm) {
    const AugRec r = reinterpret_cast<const AugRec*>(ws + recs)[blockIdx.y];
    const unsigned char* img = reinterpret_cast<const unsigned char*>(ws + resized) + (long long)blockIdx.y * S * S * 3;
    const long long n = (long long)S * S;
    const long long sum = (long long)reinterpret_cast<const unsigned long long*>(ws + lsum)[blockIdx.y];
    const int lmean = (int)((2 * sum + n) / (2 * n));
    float* o = out + (long long)blockIdx.y * 3 * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (int)n; i += gridDim.x * 256) {
        const int y = i / S, x = i - y * S;
        Rgb p = aug_gather(r, img, S, x, y);
        for (int k = 0; k < 4; ++k) p = aug_op(r, r.op[k], p, lmean);
        const int ch[3] = {p.r, p.g, p.b};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = (float)ch[c] / 255.f;
            o[c * n + i] = (v - nm.mean[c]) / nm.std[c];
        }
    }
}

// ------------------------------------------------------------------------------------------------------- host: records
static double round15(double v) {      // Python's round(v, 15): the nearest 15-decimal number, read back as a double
    char buf[64];
    snprintf(buf, sizeof buf, "%.15f", v);
    return strtod(buf, nullptr);
}

// Image.rotate(angle, NEAREST) on an S x S image: false when it is a copy, else the six 16.16 values of affine_fixed
static bool aug_rotation(double angle, int S, int* fx) {
    angle = fmod(angle, 360.0);
    if (angle < 0.0) angle += 360.0;
    if (angle == 0.0 || angle == 360.0) return false;
    const double c = S / 2.0, a = -(angle * (M_PI / 180.0));
    double m[6] = {round15(cos(a)), round15(sin(a)), 0.0, round15(-sin(a)), round15(cos(a)), 0.0};
    m[2] = m[0] * -c + m[1] * -c + m[2];
    m[5] = m[3] * -c + m[4] * -c + m[5];
    m[2] += c;
    m[5] += c;
    const double v[6] = {m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5};
    for (int i = 0; i < 6; ++i) fx[i] = (int)floor(v[i] * 65536.0 + 0.5);
    return true;
}

static int aug_check_common(int n_src, const int32_t* src_h, const int32_t* src_w, const int64_t* src_off, int64_t arena_bytes,
                            int N, int S, const void* ws) {
    HS_REQUIRE(src_h && src_w && src_off && ws, "augment: null pointer");
    HS_REQUIRE(n_src >= 1 && N >= 1 && N <= 65535, "augment: needs at least one source and 1..65535 outputs");
    HS_REQUIRE(S >= 1 && S <= kAugMaxS, "augment: output size S must be 1..%d (got %d)", kAugMaxS, S);
    for (int i = 0; i < n_src; ++i) {
        HS_REQUIRE(src_h[i] >= 1 && src_w[i] >= 1 && src_h[i] <= kAugMaxDim && src_w[i] <= kAugMaxDim,
                   "augment: source %d has size %d x %d", i, src_h[i], src_w[i]);
        HS_REQUIRE(src_off[i] >= 0 && src_off[i] + (int64_t)src_h[i] * src_w[i] * 3 <= arena_bytes,
                   "augment: source %d lies outside the arena of %lld bytes", i, (long long)arena_bytes);
    }
    return HS_OK;
}

static int aug_fill_train(AugRec* rec, const int32_t* ip, const double* fp, int N, int S, int n_src, const int32_t* src_h,
                          const int32_t* src_w, const int64_t* src_off) {
    for (int n = 0; n < N; ++n) {
        const int32_t* p = ip + (long long)n * IP_COUNT;
        AugRec& r = rec[n];
        memset(&r, 0, sizeof r);
        const int s = p[IP_SRC];
        HS_REQUIRE(s >= 0 && s < n_src, "augment: output %d names source %d of %d", n, s, n_src);
        HS_REQUIRE(p[IP_H] >= 1 && p[IP_W] >= 1 && p[IP_TOP] >= 0 && p[IP_LEFT] >= 0 &&
                       (long long)p[IP_TOP] + p[IP_H] <= src_h[s] && (long long)p[IP_LEFT] + p[IP_W] <= src_w[s],
                   "augment: output %d: crop box (top %d, left %d, %d x %d) lies outside its %d x %d image", n, p[IP_TOP], p[IP_LEFT],
                   p[IP_H], p[IP_W], src_h[s], src_w[s]);
        for (int f = IP_HFLIP; f <= IP_ROTATE; ++f) HS_REQUIRE(p[f] == 0 || p[f] == 1, "augment: output %d: flags are 0 or 1", n);
        r.pitch = src_w[s] * 3;
        r.src = src_off[s] + (long long)p[IP_TOP] * r.pitch + (long long)p[IP_LEFT] * 3;
        r.in[0] = p[IP_W];
        r.in[1] = p[IP_H];
        r.out[0] = r.out[1] = S;
        r.hflip = p[IP_HFLIP];
        r.vflip = p[IP_VFLIP];
        if (p[IP_ROTATE]) {
            HS_REQUIRE(isfinite(fp[n * FP_COUNT + FP_ANGLE]), "augment: output %d: angle is not finite", n);
            r.rotate = aug_rotation(fp[n * FP_COUNT + FP_ANGLE], S, r.rot) ? 1 : 0;
        }
        int seen = 0;
        for (int k = 0; k < 4; ++k) {
            const int op = p[IP_ORDER + k];
            HS_REQUIRE(op >= 0 && op < 4 && !(seen & (1 << op)), "augment: output %d: the colour order is not a permutation of 0..3", n);
            seen |= 1 << op;
            const int en = p[IP_ENABLE + op];
            HS_REQUIRE(en == 0 || en == 1, "augment: output %d: flags are 0 or 1", n);
            r.op[k] = en ? op : -1;
        }
        for (int k = 0; k < 3; ++k) {
            const double v = fp[n * FP_COUNT + FP_BRIGHTNESS + k];
            HS_REQUIRE(!p[IP_ENABLE + k] || (isfinite(v) && v >= 0.0), "augment: output %d: factor %d must be finite and >= 0", n, k);
            r.factor[k] = (float)v;
        }
        const double hue = fp[n * FP_COUNT + FP_HUE];
        HS_REQUIRE(!p[IP_ENABLE + OP_HUE] || (hue >= -0.5 && hue <= 0.5), "augment: output %d: hue shift must lie in [-0.5, 0.5]", n);
        r.hue_add = p[IP_ENABLE + OP_HUE] ? (int)(hue * 255.0) & 255 : 0;
    }
    return HS_OK;
}

// Resize(R) + CenterCrop(S): shorter side to R, longer to int(R * long / short), window at int(round((len - S) / 2.0))
static int aug_fill_eval(AugRec* rec, const int32_t* src_index, int N, int R, int S, int n_src, const int32_t* src_h,
                         const int32_t* src_w, const int64_t* src_off) {
    HS_REQUIRE(R >= S && R <= kAugMaxDim, "augment: eval resize %d must be at least the crop %d", R, S);
    for (int n = 0; n < N; ++n) {
        AugRec& r = rec[n];
        memset(&r, 0, sizeof r);
        const int s = src_index[n];
        HS_REQUIRE(s >= 0 && s < n_src, "augment: output %d names source %d of %d", n, s, n_src);
        const int h = src_h[s], w = src_w[s];
        const long long lng = w <= h ? (long long)((double)((long long)R * h) / (double)w) : (long long)((double)((long long)R * w) / (double)h);
        HS_REQUIRE(lng <= kAugMaxDim, "augment: source %d is too elongated to resize to %d", s, R);
        r.pitch = w * 3;
        r.src = src_off[s];
        r.in[0] = w;
        r.in[1] = h;
        r.out[0] = w <= h ? R : (int)lng;
        r.out[1] = w <= h ? (int)lng : R;
        for (int a = 0; a < 2; ++a) r.off[a] = (int)nearbyint((r.out[a] - S) / 2.0);   // half to even, as Python's round
        for (int k = 0; k < 4; ++k) r.op[k] = -1;
    }
    return HS_OK;
}

static int aug_launch_plan(AugRec* rec, int N, int S, void* ws, int64_t ws_bytes, void* stream) {
    const AugLayout l = aug_layout(rec, N, S);
    HS_REQUIRE(ws_bytes >= l.total, "augment: workspace of %lld bytes, %lld needed", (long long)ws_bytes, l.total);
    HS_REQUIRE(((uintptr_t)ws & 15) == 0, "augment: the workspace must be 16-byte aligned");
    for (int n0 = 0; n0 < N; n0 += kAugChunk) {
        AugChunk c;
        const int cnt = N - n0 < kAugChunk ? N - n0 : kAugChunk;
        memset(&c, 0, sizeof c);
        memcpy(c.rec, rec + n0, (size_t)cnt * sizeof(AugRec));
        hipLaunchKernelGGL(aug_plan_kernel, dim3(cnt), dim3(256), 0, (hipStream_t)stream, c, (char*)ws, l.recs, l.lsum, n0, S);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

}  // namespace hs

using namespace hs;

extern "C" {

int64_t hs_augment_ws_bytes(const int32_t* iparams, int32_t N, int32_t S) {
    if (!iparams || N < 1 || S < 1 || S > kAugMaxS) return -1;
    AugRec* rec = (AugRec*)calloc((size_t)N, sizeof(AugRec));
    if (!rec) return -1;
    int64_t total = -1;
    bool ok = true;
    for (int n = 0; n < N && ok; ++n) {
        const int32_t* p = iparams + (long long)n * IP_COUNT;
        ok = p[IP_H] >= 1 && p[IP_W] >= 1 && p[IP_H] <= kAugMaxDim && p[IP_W] <= kAugMaxDim;
        rec[n].in[0] = p[IP_W];
        rec[n].in[1] = p[IP_H];
        rec[n].out[0] = rec[n].out[1] = S;
    }
    if (ok) total = aug_layout(rec, N, S).total;
    free(rec);
    return total;
}

int64_t hs_augment_eval_ws_bytes(const int32_t* src_h, const int32_t* src_w, int32_t n_src, const int32_t* src_index, int32_t N,
                                 int32_t R, int32_t S) {
    if (!src_h || !src_w || !src_index || n_src < 1 || N < 1 || S < 1 || S > kAugMaxS) return -1;
    AugRec* rec = (AugRec*)calloc((size_t)N, sizeof(AugRec));
    int64_t* off = (int64_t*)calloc((size_t)n_src, sizeof(int64_t));
    int64_t total = -1;
    bool ok = rec && off;
    for (int i = 0; i < n_src && ok; ++i)
        ok = src_h[i] >= 1 && src_w[i] >= 1 && src_h[i] <= kAugMaxDim && src_w[i] <= kAugMaxDim;
    if (ok && aug_fill_eval(rec, src_index, N, R, S, n_src, src_h, src_w, off) == HS_OK) total = aug_layout(rec, N, S).total;
    free(rec);
    free(off);
    return total;
}

int64_t hs_augment_ws_offset(int32_t what, int32_t N, int32_t S) {
    if (N < 1 || S < 1 || S > kAugMaxS) return -1;
    const AugLayout l = aug_fixed_layout(N, S);
    return what == 0 ? l.lsum : what == 1 ? l.resized : -1;
}

hs_status hs_augment_plan(const int32_t* src_h, const int32_t* src_w, const int64_t* src_off, int32_t n_src, int64_t arena_bytes,
                          const int32_t* iparams, const double* fparams, int32_t N, int32_t S, void* ws, int64_t ws_bytes,
                          void* stream) {
    HS_PROPAGATE(aug_check_common(n_src, src_h, src_w, src_off, arena_bytes, N, S, ws));
    HS_REQUIRE(iparams && fparams, "augment_plan: null parameter table");
    AugRec* rec = (AugRec*)malloc((size_t)N * sizeof(AugRec));
    HS_REQUIRE(rec, "augment_plan: out of host memory");
    int st = aug_fill_train(rec, iparams, fparams, N, S, n_src, src_h, src_w, src_off);
    if (st == HS_OK) st = aug_launch_plan(rec, N, S, ws, ws_bytes, stream);
    free(rec);
    return st;
}

hs_status hs_augment_plan_eval(const int32_t* src_h, const int32_t* src_w, const int64_t* src_off, int32_t n_src, int64_t arena_bytes,
                               const int32_t* src_index, int32_t N, int32_t R, int32_t S, void* ws, int64_t ws_bytes, void* stream) {
    HS_PROPAGATE(aug_check_common(n_src, src_h, src_w, src_off, arena_bytes, N, S, ws));
    HS_REQUIRE(src_index, "augment_plan_eval: null source index");
    AugRec* rec = (AugRec*)malloc((size_t)N * sizeof(AugRec));
    HS_REQUIRE(rec, "augment_plan_eval: out of host memory");
    int st = aug_fill_eval(rec, src_index, N, R, S, n_src, src_h, src_w, src_off);
    if (st == HS_OK) st = aug_launch_plan(rec, N, S, ws, ws_bytes, stream);
    free(rec);
    return st;
}

hs_status hs_augment_resize(const uint8_t* arena, void* ws, int32_t N, int32_t S, void* stream) {
    HS_REQUIRE(arena && ws && N >= 1 && S >= 1 && S <= kAugMaxS, "augment_resize: bad argument");
    const AugLayout l = aug_fixed_layout(N, S);
    hipLaunchKernelGGL(aug_resize_h_kernel, dim3(64, N), dim3(256), 0, (hipStream_t)stream, arena, (char*)ws, l.recs, S);
    HS_LAUNCH_CHECK();
    const int gv = aug_grid((long long)S * S * 3, 64);
    hipLaunchKernelGGL(aug_resize_v_kernel, dim3(gv, N), dim3(256), 0, (hipStream_t)stream, (char*)ws, l.recs, l.resized, S);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_augment_stats(void* ws, int32_t N, int32_t S, void* stream) {
    HS_REQUIRE(ws && N >= 1 && S >= 1 && S <= kAugMaxS, "augment_stats: bad argument");
    const AugLayout l = aug_fixed_layout(N, S);
    hipLaunchKernelGGL(aug_stats_kernel, dim3(aug_grid((long long)S * S, 64), N), dim3(256), 0, (hipStream_t)stream, (char*)ws, l.recs,
                       l.lsum, l.resized, S);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_augment_finish(const void* ws, float* out, int32_t N, int32_t S, const float* mean, const float* std, void* stream) {
    HS_REQUIRE(ws && out && mean && std && N >= 1 && S >= 1 && S <= kAugMaxS, "augment_finish: bad argument");
    AugNorm nm;
    for (int c = 0; c < 3; ++c) {
        HS_REQUIRE(std[c] != 0.f, "augment_finish: std must be non-zero");
        nm.mean[c] = mean[c];
        nm.std[c] = std[c];
    }
    const AugLayout l = aug_fixed_layout(N, S);
    hipLaunchKernelGGL(aug_finish_kernel, dim3(aug_grid((long long)S * S, 64), N), dim3(256), 0, (hipStream_t)stream, (const char*)ws,
                       l.recs, l.lsum, l.resized, out, S, nm);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
