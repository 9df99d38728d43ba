// The convolutional half of MambaVision (reference ConNexT/models/block/mamba_vision.py:1434-1524,1833-1951): 3x3 pad-1
// convolutions at channel counts that are only multiples of 8 in storage, the two BatchNorm epilogues of ConvBlock, the
// window partition / reverse of an NHWC map and the image / filter packing around them.  gfx950 only.
//
// Activations are NHWC rows with a channel pitch ld = ceil8(C); lanes C .. ld-1 are zero and every kernel here that writes an
// activation writes them as zeros.
#include "hs_common.h"

namespace hs {

// ----------------------------------------------------------------------------------------------
// 3x3 convolution as an implicit GEMM on MFMA: D[m][n] = sum over (tap, c) of A(m, tap, c) * Wp[n][tap][c].
//   forward        m = (img, p, q), A = x[img][p stride - 1 + r][q stride - 1 + s][c],     Wp = [Kout][9][ldx]
//   data gradient  m = (img, h, w), A = dy[img][(h + 1 - r) / stride][(w + 1 - s) / stride][ko] where both quotients are
//                  exact and inside the output, else 0,                                     Wp = [C][9][lddy]
// The flattened K axis is cut into 16-byte chunks; with the pitch a multiple of 8 a chunk never straddles a tap, so each chunk
// is one (tap, channel) address or zeros.  Nothing of the im2col matrix ever exists in global memory.
// Workgroup: 256 threads, a 64 x 64 tile of D, 8 chunks of K per step staged through LDS (rows padded to 144 bytes against bank
// conflicts); each wave owns 32 x 32 as 2 x 2 MFMA tiles.  The MFMA runs transposed (filter rows as the A operand) so a lane
// ends with 4 consecutive output channels of one pixel and stores them with one access.
// ----------------------------------------------------------------------------------------------
constexpr int C3_BM = 64, C3_BN = 64, C3_KCH = 8, C3_PITCH = 144;

struct Conv3Args {
    const char* A;
    const char* Wp;
    const float* bias;
    char* D;
    int M, Nrows, Nst;      // rows of D; filter rows that exist; stored columns of D (its pitch)
    int cpk, nchunks;       // chunks per tap, 9 * cpk
    int SH, SW;             // extent of the tensor A gathers from
    int OH, OW;             // extent the rows of D run over
    int lda;                // channel pitch of the gathered tensor (elements)
    int stride;
    FastDiv div_ohw, div_ow, div_cpk;
};

template <typename T, bool DGRAD>
__global__ __launch_bounds__(256) void conv3_kernel(Conv3Args a) {
    constexpr int E = Chunk<T>::N;
    __shared__ __attribute__((aligned(16))) char sA[C3_BM * C3_PITCH];
    __shared__ __attribute__((aligned(16))) char sB[C3_BN * C3_PITCH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * C3_BM, n0 = blockIdx.y * C3_BN;
    const int lc = t & 7, lr = t >> 3;

    int aimg[2], aoh[2], aow[2];
    bool arow[2], brow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + lr + 32 * i;
        arow[i] = m < a.M;
        const unsigned mm = arow[i] ? (unsigned)m : 0u;
        const unsigned img = fdiv(mm, a.div_ohw);
        const unsigned rem = mm - img * (unsigned)(a.OH * a.OW);
        const unsigned oh = fdiv(rem, a.div_ow);
        aimg[i] = (int)img;
        aoh[i] = (int)oh;
        aow[i] = (int)(rem - oh * (unsigned)a.OW);
        brow[i] = (n0 + lr + 32 * i) < a.Nrows;
    }

    u32x4 ra[2], rb[2];
    auto fetch = [&](int ks) {
        const int kc = ks * C3_KCH + lc;
        const bool kok = kc < a.nchunks;
        const unsigned tap = fdiv((unsigned)(kok ? kc : 0), a.div_cpk);
        const int cc = (kok ? kc : 0) - (int)tap * a.cpk;
        const int r = (int)tap / 3, s = (int)tap - 3 * r;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int h, w;
            bool ok = kok && arow[i];
            if constexpr (DGRAD) {
                const int hh = aoh[i] + 1 - r, ww = aow[i] + 1 - s;
                ok = ok && hh >= 0 && ww >= 0 && (hh % a.stride) == 0 && (ww % a.stride) == 0;
                h = hh / a.stride;
                w = ww / a.stride;
                ok = ok && h < a.SH && w < a.SW;
            } else {
                h = aoh[i] * a.stride - 1 + r;
                w = aow[i] * a.stride - 1 + s;
                ok = ok && h >= 0 && h < a.SH && w >= 0 && w < a.SW;
            }
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) {
                const size_t off = (((size_t)aimg[i] * a.SH + h) * a.SW + w) * (size_t)a.lda + (size_t)cc * E;
                v = *(const u32x4*)(a.A + off * sizeof(T));
            }
            ra[i] = v;
            u32x4 b = {0u, 0u, 0u, 0u};
            if (kok && brow[i]) b = *(const u32x4*)(a.Wp + ((size_t)(n0 + lr + 32 * i) * a.nchunks + kc) * 16);
            rb[i] = b;
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = wave & 1, wn = wave >> 1;
    const int nks = (a.nchunks + C3_KCH - 1) / C3_KCH;
    fetch(0);
    for (int ks = 0; ks < nks; ++ks) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(u32x4*)(sA + (lr + 32 * i) * C3_PITCH + lc * 16) = ra[i];
            *(u32x4*)(sB + (lr + 32 * i) * C3_PITCH + lc * 16) = rb[i];
        }
        __syncthreads();
        if (ks + 1 < nks) fetch(ks + 1);
        const char* pa = sA + (wm * 32 + (lane & 15)) * C3_PITCH;
        const char* pb = sB + (wn * 32 + (lane & 15)) * C3_PITCH;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int ksub = 0; ksub < 2; ++ksub) {
                const int co = (ksub * 4 + (lane >> 4)) * 16;
                bf16x8 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = *(const bf16x8*)(pa + i * 16 * C3_PITCH + co);
                    fb[i] = *(const bf16x8*)(pb + i * 16 * C3_PITCH + co);
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[ni], fa[mi], acc[mi][ni], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int co = (kk * 4 + (lane >> 4)) * 4;
                float fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = *(const float*)(pa + i * 16 * C3_PITCH + co);
                    fb[i] = *(const float*)(pb + i * 16 * C3_PITCH + co);
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[ni], fa[mi], acc[mi][ni], 0, 0, 0);
            }
        }
    }

    // lane: pixel m = ... + (lane & 15), channels nb .. nb + 3 with nb = ... + 4 (lane >> 4)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int m = m0 + wm * 32 + mi * 16 + (lane & 15);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int nb = n0 + wn * 32 + ni * 16 + (lane >> 4) * 4;
            if (m >= a.M || nb >= a.Nst) continue;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[mi][ni][j] + ((a.bias && nb + j < a.Nrows) ? a.bias[nb + j] : 0.f);
            char* dst = a.D + ((size_t)m * a.Nst + nb) * sizeof(T);
            if constexpr (sizeof(T) == 2) {
                bf16x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (bf16_t)v[j];
                *(bf16x4*)dst = o;
            } else {
                *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
            }
        }
    }
}

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int conv3_launch(int dtype, bool dgrad, const Conv3Args& a, hipStream_t s) {
    const dim3 grid(ceil_div(a.M, C3_BM), ceil_div(a.Nst, C3_BN));
    if (dtype == HS_BF16) {
        if (dgrad) hipLaunchKernelGGL((conv3_kernel<bf16_t, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv3_kernel<bf16_t, false>), grid, dim3(256), 0, s, a);
    } else {
        if (dgrad) hipLaunchKernelGGL((conv3_kernel<float, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv3_kernel<float, false>), grid, dim3(256), 0, s, a);
    }
    HS_LAUNCH_CHECK();
    return HS_OK;
}

static int conv3_common(const char* who, int dtype, const void* p0, const void* p1, const void* p2, int N, int H, int W, int C, int ldx,
                        int Kout, int ldy, int stride) {
    HS_REQUIRE(dtype == HS_BF16 || dtype == HS_F32, "%s: bad dtype %d", who, dtype);
    HS_REQUIRE(p0 && p1 && p2, "%s: null argument", who);
    HS_REQUIRE(aligned16(p0) && aligned16(p1) && aligned16(p2), "%s: operands must be 16-byte aligned", who);
    HS_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && Kout > 0, "%s: empty shape", who);
    HS_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2, got %d", who, stride);
    HS_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && C <= ldx && Kout <= ldy, "%s: channel pitches must be multiples of 8 that hold C %d / "
               "Kout %d (got %d / %d)", who, C, Kout, ldx, ldy);
    HS_REQUIRE((long long)N * H * W < (1ll << 31) && 9ll * ldx < (1 << 24) && 9ll * ldy < (1 << 24), "%s: shape too large", who);
    return HS_OK;
}

// ----------------------------------------------------------------------------------------------
// filter packing: the parameter (Kout, C, 3, 3) f32 <-> the compute copies
// ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv3_pack_filter_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wt, int Kout,
                                                                int C, int Cp, int Kp) {
    const long long n1 = (long long)Kout * 9 * Cp, n2 = wt ? (long long)C * 9 * Kp : 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n1 + n2; i += gridDim.x * 256ll) {
        if (i < n1) {
            const int c = (int)(i % Cp), tap = (int)((i / Cp) % 9), ko = (int)(i / (9ll * Cp));
            wf[i] = from_f32<T>(c < C ? w[((long long)ko * C + c) * 9 + tap] : 0.f);
        } else {
            const long long j = i - n1;
            const int ko = (int)(j % Kp), tap = (int)((j / Kp) % 9), c = (int)(j / (9ll * Kp));
            wt[j] = from_f32<T>(ko < Kout ? w[((long long)ko * C + c) * 9 + tap] : 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void conv3_unpack_wgrad_kernel(const float* __restrict__ g, float* __restrict__ dw, int Kout, int C, int Cp) {
    const long long n = (long long)Kout * C * 9;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        const int tap = (int)(i % 9), c = (int)((i / 9) % C), ko = (int)(i / (9ll * C));
        dw[i] = g[((long long)ko * 9 + tap) * Cp + c];
    }
}

// ----------------------------------------------------------------------------------------------
// image packing: f32 NCHW <-> NHWC rows of pitch ld
// ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_nhwc_kernel(const float* __restrict__ x, T* __restrict__ y, long long npix, int Cin, int HW, int ld) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix * ld; i += gridDim.x * 256ll) {
        const int c = (int)(i % ld);
        const long long pix = i / ld;
        const long long img = pix / HW, hw = pix % HW;
        y[i] = from_f32<T>(c < Cin ? x[(img * Cin + c) * HW + hw] : 0.f);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void unpack_nhwc_kernel(const T* __restrict__ y, float* __restrict__ x, long long npix, int Cin, int HW, int ld) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < npix * Cin; i += gridDim.x * 256ll) {
        const long long hw = i % HW, c = (i / HW) % Cin, img = i / ((long long)HW * Cin);
        x[i] = to_f32(y[(img * HW + hw) * ld + c]);
    }
}

// ----------------------------------------------------------------------------------------------
// BatchNorm apply passes with ConvBlock's epilogues over [M][ld] rows; z = fma(x, scale, shift)
//   mode 0: y = gelu_tanh(z)          mode 1: y = res + ls[c] * rowscale[row / rows_per_sample] * z
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_tanh(float z) {
    const float u = 0.7978845608028654f * (z + 0.044715f * z * z * z);
    return 0.5f * z * (1.f + tanhf(u));
}
__device__ __forceinline__ float gelu_tanh_grad(float z) {
    const float u = 0.7978845608028654f * (z + 0.044715f * z * z * z);
    const float th = tanhf(u);
    return 0.5f * (1.f + th) + 0.5f * z * (1.f - th * th) * 0.7978845608028654f * (1.f + 3.f * 0.044715f * z * z);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_epi_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const T* __restrict__ res, const float* __restrict__ ls, const float* __restrict__ rowscale,
                                                         T* __restrict__ y, long long nch, int C, int cpr, long long rps) {
    constexpr int E = Chunk<T>::N;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nch; i += gridDim.x * 256ll) {
        const long long row = i / cpr;
        const int c0 = (int)(i - row * cpr) * E;
        float f[E], r[E], o[E];
        Chunk<T>::unpack(*(const u32x4*)((const char*)x + i * 16), f);
        float rs = 1.f;
        if constexpr (MODE == 1) {
            Chunk<T>::unpack(*(const u32x4*)((const char*)res + i * 16), r);
            if (rowscale) rs = rowscale[row / rps];
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int c = c0 + j;
            if (c < C) {
                const float z = fmaf(f[j], scale[c], shift[c]);
                if constexpr (MODE == 0) o[j] = gelu_tanh(z);
                else o[j] = fmaf((ls ? ls[c] : 1.f) * rs, z, r[j]);
            } else {
                o[j] = 0.f;
            }
        }
        *(u32x4*)((char*)y + i * 16) = Chunk<T>::pack(o);
    }
}

// backward: g = dy * gelu_tanh'(z) (mode 0) or dy * rowscale (mode 1); S1 = sum g, S2 = sum g * xhat per channel, through
// ws[row block][C][2] and a fixed-order second pass (deterministic)
static int bn_epi_rows_per_block(long long M) {
    long long rpb = (M + 255) / 256;
    if (rpb < 64) rpb = 64;
    return (int)((rpb + 3) / 4 * 4);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_epi_bwd_partial_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ rowscale, long long M,
                                                                 int C, int ld, int rpb, long long rps, float* __restrict__ ws) {
    __shared__ float red[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    const long long r0 = (long long)blockIdx.y * rpb;
    const long long r1 = r0 + rpb < M ? r0 + rpb : M;
    float s1 = 0.f, s2 = 0.f;
    if (c < C) {
        const float sc = scale[c], sh = shift[c], mu = mean[c], is = invstd[c];
        for (long long r = r0 + ty; r < r1; r += 4) {
            const float xv = to_f32(x[r * ld + c]);
            float g = to_f32(dy[r * ld + c]);
            if constexpr (MODE == 0) g *= gelu_tanh_grad(fmaf(xv, sc, sh));
            else if (rowscale) g *= rowscale[r / rps];
            s1 += g;
            s2 += g * (xv - mu) * is;
        }
    }
    red[0][ty][tx] = s1;
    red[1][ty][tx] = s2;
    __syncthreads();
    if (ty == 0 && c < C) {
        float* o = ws + ((long long)blockIdx.y * C + c) * 2;
        o[0] = ((red[0][0][tx] + red[0][1][tx]) + red[0][2][tx]) + red[0][3][tx];
        o[1] = ((red[1][0][tx] + red[1][1][tx]) + red[1][2][tx]) + red[1][3][tx];
    }
}

__global__ __launch_bounds__(256) void bn_epi_bwd_final_kernel(const float* __restrict__ ws, int gy, int C, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ invstd,
                                                               const float* __restrict__ ls, float inv_m, int training, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, float* __restrict__ dls, float* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s1 = 0.f, s2 = 0.f;
    for (int b = 0; b < gy; ++b) {
        s1 += ws[((long long)b * C + c) * 2];
        s2 += ws[((long long)b * C + c) * 2 + 1];
    }
    const float l = ls ? ls[c] : 1.f;
    if (dls) dls[c] = gamma[c] * s2 + beta[c] * s1;
    dbeta[c] = l * s1;
    dgamma[c] = l * s2;
    const float gi = gamma[c] * invstd[c] * l;
    coef[c * 3] = gi;
    coef[c * 3 + 1] = training ? gi * s1 * inv_m : 0.f;
    coef[c * 3 + 2] = training ? gi * s2 * inv_m : 0.f;
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_epi_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, const float* __restrict__ rowscale,
                                                               const float* __restrict__ coef, T* __restrict__ dx, long long nch, int C, int cpr,
                                                               long long rps) {
    constexpr int E = Chunk<T>::N;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nch; i += gridDim.x * 256ll) {
        const long long row = i / cpr;
        const int c0 = (int)(i - row * cpr) * E;
        float f[E], d[E], o[E];
        Chunk<T>::unpack(*(const u32x4*)((const char*)x + i * 16), f);
        Chunk<T>::unpack(*(const u32x4*)((const char*)dy + i * 16), d);
        float rs = 1.f;
        if constexpr (MODE == 1) {
            if (rowscale) rs = rowscale[row / rps];
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int c = c0 + j;
            if (c < C) {
                float g = d[j];
                if constexpr (MODE == 0) g *= gelu_tanh_grad(fmaf(f[j], scale[c], shift[c]));
                else g *= rs;
                const float xhat = (f[j] - mean[c]) * invstd[c];
                o[j] = coef[c * 3] * g - coef[c * 3 + 1] - xhat * coef[c * 3 + 2];
            } else {
                o[j] = 0.f;
            }
        }
        *(u32x4*)((char*)dx + i * 16) = Chunk<T>::pack(o);
    }
}

// ----------------------------------------------------------------------------------------------
// window partition / reverse of an NHWC map [B][H][W][ld] <-> tokens (B nWh nWw, ws ws, C), both of T
// ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void window_partition_nhwc_kernel(const T* __restrict__ map, T* __restrict__ tok, long long n, int C, int ld,
                                                                    int H, int W, int ws, int nWh, int nWw) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        const int c = (int)(i % C);
        long long q = i / C;
        const int p = (int)(q % (ws * ws));
        q /= ws * ws;
        const int ww = (int)(q % nWw);
        q /= nWw;
        const int wh = (int)(q % nWh);
        const long long b = q / nWh;
        const int h = wh * ws + p / ws, w = ww * ws + p % ws;
        T v = from_f32<T>(0.f);
        if (h < H && w < W) v = map[((b * H + h) * W + w) * ld + c];
        tok[i] = v;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void window_reverse_nhwc_kernel(const T* __restrict__ tok, T* __restrict__ map, long long n, int C, int ld, int H,
                                                                  int W, int ws, int nWh, int nWw) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        const int c = (int)(i % ld);
        long long q = i / ld;
        const int w = (int)(q % W);
        q /= W;
        const int h = (int)(q % H);
        const long long b = q / H;
        T v = from_f32<T>(0.f);
        if (c < C) {
            const long long win = (b * nWh + h / ws) * nWw + w / ws;
            const int p = (h % ws) * ws + w % ws;
            v = tok[(win * (ws * ws) + p) * C + c];
        }
        map[i] = v;
    }
}

static int blocks_for(long long n) {
    long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace hs

using namespace hs;

extern "C" {

hs_status hs_conv3x3_fwd(int32_t dtype, const void* x, const void* wf, const float* bias, void* y, int32_t N, int32_t H, int32_t W, int32_t C,
                         int32_t ldx, int32_t Kout, int32_t ldy, int32_t stride, void* stream) {
    HS_PROPAGATE(conv3_common("conv3x3_fwd", dtype, x, wf, y, N, H, W, C, ldx, Kout, ldy, stride));
    const int E = dtype == HS_BF16 ? 8 : 4;
    const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
    Conv3Args a;
    a.A = (const char*)x;
    a.Wp = (const char*)wf;
    a.bias = bias;
    a.D = (char*)y;
    a.M = N * P * Q;
    a.Nrows = Kout;
    a.Nst = ldy;
    a.cpk = ldx / E;
    a.nchunks = 9 * a.cpk;
    a.SH = H;
    a.SW = W;
    a.OH = P;
    a.OW = Q;
    a.lda = ldx;
    a.stride = stride;
    a.div_ohw = make_fastdiv(P * Q);
    a.div_ow = make_fastdiv(Q);
    a.div_cpk = make_fastdiv(a.cpk);
    return conv3_launch(dtype, false, a, (hipStream_t)stream);
}

hs_status hs_conv3x3_dgrad(int32_t dtype, const void* dy, const void* wt, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t lddx,
                           int32_t Kout, int32_t lddy, int32_t stride, void* stream) {
    HS_PROPAGATE(conv3_common("conv3x3_dgrad", dtype, dy, wt, dx, N, H, W, C, lddx, Kout, lddy, stride));
    const int E = dtype == HS_BF16 ? 8 : 4;
    const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
    Conv3Args a;
    a.A = (const char*)dy;
    a.Wp = (const char*)wt;
    a.bias = nullptr;
    a.D = (char*)dx;
    a.M = N * H * W;
    a.Nrows = C;
    a.Nst = lddx;
    a.cpk = lddy / E;
    a.nchunks = 9 * a.cpk;
    a.SH = P;
    a.SW = Q;
    a.OH = H;
    a.OW = W;
    a.lda = lddy;
    a.stride = stride;
    a.div_ohw = make_fastdiv(H * W);
    a.div_ow = make_fastdiv(W);
    a.div_cpk = make_fastdiv(a.cpk);
    return conv3_launch(dtype, true, a, (hipStream_t)stream);
}

hs_status hs_conv3x3_pack_filter(int32_t dtype, const float* w, void* wf, void* wt, int32_t Kout, int32_t C, int32_t ldc, int32_t ldk,
                                 void* stream) {
    HS_REQUIRE(dtype == HS_BF16 || dtype == HS_F32, "conv3x3_pack_filter: bad dtype %d", dtype);
    HS_REQUIRE(w && wf && Kout > 0 && C > 0 && ldc >= C && ldk >= Kout, "conv3x3_pack_filter: bad argument");
    const long long n = 9ll * Kout * ldc + (wt ? 9ll * C * ldk : 0);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(conv3_pack_filter_kernel<bf16_t>, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)wf, (bf16_t*)wt,
                           Kout, C, ldc, ldk);
    else
        hipLaunchKernelGGL(conv3_pack_filter_kernel<float>, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, w, (float*)wf, (float*)wt, Kout,
                           C, ldc, ldk);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_conv3x3_unpack_wgrad(const float* g, float* dw, int32_t Kout, int32_t C, int32_t ldc, void* stream) {
    HS_REQUIRE(g && dw && Kout > 0 && C > 0 && ldc >= C, "conv3x3_unpack_wgrad: bad argument");
    hipLaunchKernelGGL(conv3_unpack_wgrad_kernel, dim3(blocks_for(9ll * Kout * C)), dim3(256), 0, (hipStream_t)stream, g, dw, Kout, C, ldc);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_pack_image_nhwc(int32_t dtype, const float* x, void* y, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t ld, void* stream) {
    HS_REQUIRE(dtype == HS_BF16 || dtype == HS_F32, "pack_image_nhwc: bad dtype %d", dtype);
    HS_REQUIRE(x && y && N > 0 && Cin > 0 && H > 0 && W > 0 && ld >= Cin, "pack_image_nhwc: bad argument");
    const long long npix = (long long)N * H * W;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(pack_nhwc_kernel<bf16_t>, dim3(blocks_for(npix * ld)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, npix, Cin, H * W,
                           ld);
    else
        hipLaunchKernelGGL(pack_nhwc_kernel<float>, dim3(blocks_for(npix * ld)), dim3(256), 0, (hipStream_t)stream, x, (float*)y, npix, Cin, H * W,
                           ld);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_unpack_image_nhwc(int32_t dtype, const void* y, float* x, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t ld, void* stream) {
    HS_REQUIRE(dtype == HS_BF16 || dtype == HS_F32, "unpack_image_nhwc: bad dtype %d", dtype);
    HS_REQUIRE(x && y && N > 0 && Cin > 0 && H > 0 && W > 0 && ld >= Cin, "unpack_image_nhwc: bad argument");
    const long long npix = (long long)N * H * W;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(unpack_nhwc_kernel<bf16_t>, dim3(blocks_for(npix * Cin)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, x, npix,
                           Cin, H * W, ld);
    else
        hipLaunchKernelGGL(unpack_nhwc_kernel<float>, dim3(blocks_for(npix * Cin)), dim3(256), 0, (hipStream_t)stream, (const float*)y, x, npix, Cin,
                           H * W, ld);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

static int bn_epi_args_ok(const char* who, int32_t dtype, int64_t M, int32_t C, int32_t ld, int64_t rps) {
    HS_REQUIRE(dtype == HS_BF16 || dtype == HS_F32, "%s: bad dtype %d", who, dtype);
    HS_REQUIRE(M > 0 && C > 0 && ld % 8 == 0 && ld >= C && rps > 0, "%s: bad shape M %lld C %d pitch %d", who, (long long)M, C, ld);
    return HS_OK;
}

hs_status hs_bn_gelu_tanh_fwd(int32_t dtype, const void* x, const float* scale, const float* shift, void* y, int64_t M, int32_t C, int32_t ld,
                              void* stream) {
    HS_PROPAGATE(bn_epi_args_ok("bn_gelu_tanh_fwd", dtype, M, C, ld, 1));
    HS_REQUIRE(x && scale && shift && y && aligned16(x) && aligned16(y), "bn_gelu_tanh_fwd: null or unaligned argument");
    const int E = dtype == HS_BF16 ? 8 : 4;
    const long long nch = M * (ld / E);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL((bn_epi_fwd_kernel<bf16_t, 0>), dim3(blocks_for(nch)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, scale, shift,
                           (const bf16_t*)nullptr, (const float*)nullptr, (const float*)nullptr, (bf16_t*)y, nch, C, ld / E, 1ll);
    else
        hipLaunchKernelGGL((bn_epi_fwd_kernel<float, 0>), dim3(blocks_for(nch)), dim3(256), 0, (hipStream_t)stream, (const float*)x, scale, shift,
                           (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)y, nch, C, ld / E, 1ll);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_bn_scale_residual_fwd(int32_t dtype, const void* x, const float* scale, const float* shift, const void* res, const float* ls_gamma,
                                   const float* rowscale, void* y, int64_t M, int32_t C, int32_t ld, int64_t rows_per_sample, void* stream) {
    HS_PROPAGATE(bn_epi_args_ok("bn_scale_residual_fwd", dtype, M, C, ld, rows_per_sample));
    HS_REQUIRE(x && scale && shift && res && y && aligned16(x) && aligned16(y) && aligned16(res),
               "bn_scale_residual_fwd: null or unaligned argument");
    const int E = dtype == HS_BF16 ? 8 : 4;
    const long long nch = M * (ld / E);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL((bn_epi_fwd_kernel<bf16_t, 1>), dim3(blocks_for(nch)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, scale, shift,
                           (const bf16_t*)res, ls_gamma, rowscale, (bf16_t*)y, nch, C, ld / E, (long long)rows_per_sample);
    else
        hipLaunchKernelGGL((bn_epi_fwd_kernel<float, 1>), dim3(blocks_for(nch)), dim3(256), 0, (hipStream_t)stream, (const float*)x, scale, shift,
                           (const float*)res, ls_gamma, rowscale, (float*)y, nch, C, ld / E, (long long)rows_per_sample);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int64_t hs_bn_epilogue_ws_bytes(int64_t M, int32_t C) {
    if (M <= 0 || C <= 0) return -1;
    const int rpb = bn_epi_rows_per_block(M);
    const long long gy = (M + rpb - 1) / rpb;
    return (gy * C * 2 + 3ll * C) * 4;
}

hs_status hs_bn_epilogue_bwd(int32_t dtype, int32_t mode, const void* dy, const void* x, const float* scale, const float* shift,
                             const float* save_mean, const float* save_invstd, const float* bn_gamma, const float* bn_beta, const float* ls_gamma,
                             const float* rowscale, void* dx, float* dgamma, float* dbeta, float* dls_gamma, int32_t training, int64_t M, int32_t C,
                             int32_t ld, int64_t rows_per_sample, void* ws, int64_t ws_bytes, void* stream) {
    HS_PROPAGATE(bn_epi_args_ok("bn_epilogue_bwd", dtype, M, C, ld, rows_per_sample));
    HS_REQUIRE(mode == 0 || mode == 1, "bn_epilogue_bwd: mode %d (0 tanh-GELU, 1 layer scale + residual)", mode);
    HS_REQUIRE(dy && x && scale && shift && save_mean && save_invstd && bn_gamma && bn_beta && dx && dgamma && dbeta && aligned16(dy) &&
                   aligned16(x) && aligned16(dx),
               "bn_epilogue_bwd: null or unaligned argument");
    HS_REQUIRE(!dls_gamma || (mode == 1 && ls_gamma), "bn_epilogue_bwd: d ls_gamma needs mode 1 and ls_gamma");
    HS_REQUIRE(ws && ws_bytes >= hs_bn_epilogue_ws_bytes(M, C), "bn_epilogue_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int E = dtype == HS_BF16 ? 8 : 4;
    const int rpb = bn_epi_rows_per_block(M);
    const int gy = (int)((M + rpb - 1) / rpb);
    float* part = (float*)ws;
    float* coef = part + (long long)gy * C * 2;
    const dim3 pg(ceil_div(C, 64), gy);
    const long long nch = M * (ld / E);
    const long long rps = rows_per_sample;
#define HS_BN_EPI(T, MODE)                                                                                                              \
    do {                                                                                                                                \
        hipLaunchKernelGGL((bn_epi_bwd_partial_kernel<T, MODE>), pg, dim3(256), 0, s, (const T*)dy, (const T*)x, scale, shift, save_mean, \
                           save_invstd, rowscale, (long long)M, C, ld, rpb, rps, part);                                                 \
        HS_LAUNCH_CHECK();                                                                                                              \
        hipLaunchKernelGGL(bn_epi_bwd_final_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, part, gy, C, bn_gamma, bn_beta, save_invstd, \
                           MODE == 1 ? ls_gamma : (const float*)nullptr, 1.f / (float)M, training, dgamma, dbeta, dls_gamma, coef);      \
        HS_LAUNCH_CHECK();                                                                                                              \
        hipLaunchKernelGGL((bn_epi_bwd_apply_kernel<T, MODE>), dim3(blocks_for(nch)), dim3(256), 0, s, (const T*)dy, (const T*)x, scale, shift, \
                           save_mean, save_invstd, rowscale, coef, (T*)dx, nch, C, ld / E, rps);                                        \
        HS_LAUNCH_CHECK();                                                                                                              \
    } while (0)
    if (dtype == HS_BF16) {
        if (mode == 0) HS_BN_EPI(bf16_t, 0);
        else HS_BN_EPI(bf16_t, 1);
    } else {
        if (mode == 0) HS_BN_EPI(float, 0);
        else HS_BN_EPI(float, 1);
    }
#undef HS_BN_EPI
    return HS_OK;
}

static int window_nhwc_ok(const char* who, int32_t dtype, const void* a, const void* b, int32_t B, int32_t C, int32_t ld, int32_t H, int32_t W,
                          int32_t ws) {
    HS_REQUIRE(dtype == HS_BF16 || dtype == HS_F32, "%s: bad dtype %d", who, dtype);
    HS_REQUIRE(a && b && B > 0 && C > 0 && ld >= C && H > 0 && W > 0 && ws > 0, "%s: bad argument", who);
    return HS_OK;
}

hs_status hs_window_partition_nhwc(int32_t dtype, const void* map, void* tokens, int32_t B, int32_t C, int32_t ld, int32_t H, int32_t W, int32_t ws,
                                   void* stream) {
    HS_PROPAGATE(window_nhwc_ok("window_partition_nhwc", dtype, map, tokens, B, C, ld, H, W, ws));
    const int nWh = (H + ws - 1) / ws, nWw = (W + ws - 1) / ws;
    const long long n = (long long)B * nWh * nWw * ws * ws * C;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(window_partition_nhwc_kernel<bf16_t>, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)map,
                           (bf16_t*)tokens, n, C, ld, H, W, ws, nWh, nWw);
    else
        hipLaunchKernelGGL(window_partition_nhwc_kernel<float>, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (const float*)map,
                           (float*)tokens, n, C, ld, H, W, ws, nWh, nWw);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_window_reverse_nhwc(int32_t dtype, const void* tokens, void* map, int32_t B, int32_t C, int32_t ld, int32_t H, int32_t W, int32_t ws,
                                 void* stream) {
    HS_PROPAGATE(window_nhwc_ok("window_reverse_nhwc", dtype, tokens, map, B, C, ld, H, W, ws));
    const int nWh = (H + ws - 1) / ws, nWw = (W + ws - 1) / ws;
    const long long n = (long long)B * H * W * ld;
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(window_reverse_nhwc_kernel<bf16_t>, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)tokens,
                           (bf16_t*)map, n, C, ld, H, W, ws, nWh, nWw);
    else
        hipLaunchKernelGGL(window_reverse_nhwc_kernel<float>, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (const float*)tokens,
                           (float*)map, n, C, ld, H, W, ws, nWh, nWw);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
