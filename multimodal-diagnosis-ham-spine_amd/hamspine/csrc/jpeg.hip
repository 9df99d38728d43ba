// JPEG decode on the device (include/hamspine.h: hs_jpeg_*).  The Huffman stage runs on the host (jpeg_host.h, in the loaders'
// worker processes); what is left is arithmetic with no serial dependence, restated from libjpeg's default path so that the pixels
// equal Pillow's bit for bit (tests/jpeg_ref.py is the numpy form):
//
//   idct   one thread per 8x8 block: dequantise, the "islow" integer inverse DCT (columns, descale 11, rows, descale 18), + 128,
//          clamp; the block's 64 samples go to its component's padded u8 plane in the workspace
//   pack   one thread per aligned 4 bytes of the output arena: the two pixels those bytes belong to are read from the Y plane,
//          their chroma is interpolated by the "fancy" h2v1 / h2v2 triangle filters over the component's true down-sampled size,
//          converted by the 16-bit fixed-point YCbCr tables and clamped; one dword store (byte stores at an image's unaligned
//          head and tail)
//
// All integer arithmetic is int32 with wrap-around (computed unsigned where it may overflow), as in the numpy form.
#include <stdlib.h>

#include "hs_common.h"
#include "jpeg_host.h"

namespace hs {

static constexpr int kJpegMaxDim = 65535;   // the largest side a JPEG frame header can state

struct JpegRec {
    long long coef;        // byte offset of the image's coefficients inside the coefficient arena
    long long out;         // byte offset of its pixels inside the output arena
    long long plane[3];    // byte offsets of the padded planes inside the workspace (16-byte aligned)
    int h, w, comps, hs, vs;
    int cols[2];           // block columns of the luma plane / of a chroma plane (plane pitch = cols * 8)
    int nblk[2];           // blocks of the luma plane / of one chroma plane
    int qtab;              // index of the image's [3][64] tables inside the table arena
};

struct JpegChunk {
    JpegRec rec[HS_JPEG_CHUNK];
};

static inline long long jpeg_align16(long long v) { return (v + 15) & ~15LL; }

// fills everything of `r` that follows from (h, w, comps, hs, vs); returns the image's coefficient bytes
static long long jpeg_geometry(JpegRec& r) {
    const int mx = (r.w + 8 * r.hs - 1) / (8 * r.hs), my = (r.h + 8 * r.vs - 1) / (8 * r.vs);
    r.cols[0] = mx * r.hs;
    r.nblk[0] = r.cols[0] * my * r.vs;
    r.cols[1] = r.comps == 3 ? mx : 0;
    r.nblk[1] = r.comps == 3 ? mx * my : 0;
    return ((long long)r.nblk[0] + 2LL * r.nblk[1]) * 128;
}

static bool jpeg_geom_ok(const int32_t* g) {
    const bool sampling = (g[3] == 1 && g[4] == 1) || (g[2] == 3 && g[3] == 2 && (g[4] == 1 || g[4] == 2));
    return g[0] >= 1 && g[0] <= kJpegMaxDim && g[1] >= 1 && g[1] <= kJpegMaxDim && 3LL * g[0] * g[1] <= 0x7fffffffLL &&
           (g[2] == 1 || g[2] == 3) && sampling && !(g[2] == 3 && g[3] == 2 && g[1] <= 4);
}

// rec[0..n) from the geometry table with the plane offsets assigned; returns the workspace bytes, or -1 on a bad row
static long long jpeg_layout(JpegRec* rec, const int32_t* geom, int n) {
    long long at = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* g = geom + (long long)i * HS_JPEG_GEOM;
        if (!jpeg_geom_ok(g)) return -1;
        JpegRec& r = rec[i];
        memset(&r, 0, sizeof r);
        r.h = g[0];
        r.w = g[1];
        r.comps = g[2];
        r.hs = g[3];
        r.vs = g[4];
        r.qtab = i;
        jpeg_geometry(r);
        for (int c = 0; c < r.comps; ++c) {
            r.plane[c] = at;
            at = jpeg_align16(at + (long long)r.nblk[c ? 1 : 0] * 64);
        }
    }
    return at;
}

// --------------------------------------------------------------------------------------------------------------- idct
__device__ __forceinline__ int jmul(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ __forceinline__ int jadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int jsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int jshl(int a, int s) { return (int)((unsigned)a << s); }

// libjpeg's jidctint butterfly on x[0..7] (stride 1 in registers), every result descaled by SHIFT with the rounding add
template <int SHIFT>
__device__ __forceinline__ void jpeg_idct_1d(int& x0, int& x1, int& x2, int& x3, int& x4, int& x5, int& x6, int& x7) {
    int z1 = jmul(jadd(x2, x6), 4433);
    int tmp2 = jadd(z1, jmul(x6, -15137));
    int tmp3 = jadd(z1, jmul(x2, 6270));
    int tmp0 = jshl(jadd(x0, x4), 13);
    int tmp1 = jshl(jsub(x0, x4), 13);
    const int tmp10 = jadd(tmp0, tmp3), tmp13 = jsub(tmp0, tmp3), tmp11 = jadd(tmp1, tmp2), tmp12 = jsub(tmp1, tmp2);
    tmp0 = x7;
    tmp1 = x5;
    tmp2 = x3;
    tmp3 = x1;
    z1 = jadd(tmp0, tmp3);
    int z2 = jadd(tmp1, tmp2);
    int z3 = jadd(tmp0, tmp2);
    int z4 = jadd(tmp1, tmp3);
    const int z5 = jmul(jadd(z3, z4), 9633);
    tmp0 = jmul(tmp0, 2446);
    tmp1 = jmul(tmp1, 16819);
    tmp2 = jmul(tmp2, 25172);
    tmp3 = jmul(tmp3, 12299);
    z1 = jmul(z1, -7373);
    z2 = jmul(z2, -20995);
    z3 = jadd(jmul(z3, -16069), z5);
    z4 = jadd(jmul(z4, -3196), z5);
    tmp0 = jadd(tmp0, jadd(z1, z3));
    tmp1 = jadd(tmp1, jadd(z2, z4));
    tmp2 = jadd(tmp2, jadd(z2, z3));
    tmp3 = jadd(tmp3, jadd(z1, z4));
    constexpr int half = 1 << (SHIFT - 1);
    x0 = jadd(jadd(tmp10, tmp3), half) >> SHIFT;
    x7 = jadd(jsub(tmp10, tmp3), half) >> SHIFT;
    x1 = jadd(jadd(tmp11, tmp2), half) >> SHIFT;
    x6 = jadd(jsub(tmp11, tmp2), half) >> SHIFT;
    x2 = jadd(jadd(tmp12, tmp1), half) >> SHIFT;
    x5 = jadd(jsub(tmp12, tmp1), half) >> SHIFT;
    x3 = jadd(jadd(tmp13, tmp0), half) >> SHIFT;
    x4 = jadd(jsub(tmp13, tmp0), half) >> SHIFT;
}

__device__ __forceinline__ unsigned jclip8(int v) { return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v); }

// grid (blocks of the largest image / 256, images of the chunk); adjacent lanes take adjacent blocks of a block row, so a wave's
// eight row stores each cover one contiguous run of a plane row
__global__ void __launch_bounds__(256) jpeg_idct_kernel(JpegChunk ch, const char* __restrict__ coef, const unsigned short* __restrict__ qtab,
                                                        char* __restrict__ ws) {
    const JpegRec& r = ch.rec[blockIdx.y];
    const int nY = r.nblk[0], nC = r.nblk[1];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nY + 2 * nC) return;
    const int c = b < nY ? 0 : b < nY + nC ? 1 : 2;
    const int lb = b - (c == 0 ? 0 : c == 1 ? nY : nY + nC);     // block inside its component: the coefficient order
    const int cols = c ? r.cols[1] : r.cols[0];
    const int brow = lb / cols, bcol = lb - brow * cols;
    const u32x4* src = reinterpret_cast<const u32x4*>(coef + r.coef + (long long)b * 128);
    const u32x4* q = reinterpret_cast<const u32x4*>(qtab + ((long long)r.qtab * 3 + c) * 64);
    int v[64];
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        const u32x4 cw = src[row], qw = q[row];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[row * 8 + 2 * k] = jmul((int)(short)(cw[k] & 0xffffu), (int)(qw[k] & 0xffffu));
            v[row * 8 + 2 * k + 1] = jmul((int)(short)(cw[k] >> 16), (int)(qw[k] >> 16));
        }
    }
#pragma unroll
    for (int x = 0; x < 8; ++x)
        jpeg_idct_1d<11>(v[x], v[8 + x], v[16 + x], v[24 + x], v[32 + x], v[40 + x], v[48 + x], v[56 + x]);
    const int pitch = cols * 8;
    char* dst = ws + (c == 0 ? r.plane[0] : c == 1 ? r.plane[1] : r.plane[2]) + ((long long)brow * 8) * pitch + bcol * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        int* p = v + row * 8;
        jpeg_idct_1d<18>(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
        u32x2 o;
        o[0] = jclip8(jadd(p[0], 128)) | (jclip8(jadd(p[1], 128)) << 8) | (jclip8(jadd(p[2], 128)) << 16) | (jclip8(jadd(p[3], 128)) << 24);
        o[1] = jclip8(jadd(p[4], 128)) | (jclip8(jadd(p[5], 128)) << 8) | (jclip8(jadd(p[6], 128)) << 16) | (jclip8(jadd(p[7], 128)) << 24);
        *reinterpret_cast<u32x2*>(dst + (long long)row * pitch) = o;
    }
}

// --------------------------------------------------------------------------------------------------------------- pack
// one chroma sample at full resolution: libjpeg's h2v1 / h2v2 "fancy" upsampling of plane `p` (pitch `pitch`, true down-sampled
// size ch x cw) at pixel (y, x); hs == 1 is a plain read
__device__ __forceinline__ int jpeg_chroma(const unsigned char* __restrict__ p, int pitch, int y, int x, int hs, int vs, int ch, int cw) {
    if (hs == 1) return p[(long long)y * pitch + x];
    const int i = x >> 1, odd = x & 1;
    const int j = odd ? (i + 1 < cw ? i + 1 : i) : (i > 0 ? i - 1 : i);      // the neighbour column; the edge reads itself
    const bool edge = odd ? i == cw - 1 : i == 0;
    if (vs == 1) {
        const unsigned char* row = p + (long long)y * pitch;
        const int a = row[i];
        return edge ? a : (3 * a + row[j] + (odd ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1;
    const int fy = (y & 1) ? (cy + 1 < ch ? cy + 1 : cy) : (cy > 0 ? cy - 1 : cy);   // the context row beyond an edge is the edge row
    const unsigned char* near = p + (long long)cy * pitch;
    const unsigned char* far = p + (long long)fy * pitch;
    const int s = 3 * near[i] + far[i];
    const int t = edge ? s : 3 * near[j] + far[j];          // at an edge column 3 * s + s = 4 * s
    return (3 * s + t + (odd ? 7 : 8)) >> 4;
}

// the three clamped samples of pixel `px` (row-major index) packed as R | G << 8 | B << 16
__device__ __forceinline__ unsigned jpeg_pixel(const JpegRec& r, const unsigned char* __restrict__ ws, unsigned px) {
    const int y = (int)(px / (unsigned)r.w), x = (int)(px - (unsigned)y * (unsigned)r.w);
    const int Y = ws[r.plane[0] + (long long)y * (r.cols[0] * 8) + x];
    if (r.comps == 1) return (unsigned)Y * 0x010101u;
    const int cw = (r.w + r.hs - 1) / r.hs, ch = (r.h + r.vs - 1) / r.vs, pitch = r.cols[1] * 8;
    const int cb = jpeg_chroma(ws + r.plane[1], pitch, y, x, r.hs, r.vs, ch, cw) - 128;
    const int cr = jpeg_chroma(ws + r.plane[2], pitch, y, x, r.hs, r.vs, ch, cw) - 128;
    const int R = Y + ((91881 * cr + 32768) >> 16);
    const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int B = Y + ((116130 * cb + 32768) >> 16);
    return jclip8(R) | (jclip8(G) << 8) | (jclip8(B) << 16);
}

// grid (chunks of the largest image / 256 capped, images of the chunk).  Chunk 0 of an image is its bytes in front of the first
// 4-byte-aligned address, chunk k >= 1 the k-th aligned dword; the last one may be cut short by the image's end.
__global__ void __launch_bounds__(256) jpeg_pack_kernel(JpegChunk ch, const unsigned char* __restrict__ ws, unsigned char* __restrict__ out) {
    const JpegRec& r = ch.rec[blockIdx.y];
    const unsigned total = 3u * (unsigned)r.h * (unsigned)r.w;            // < 2^31: checked on the host
    unsigned char* dst = out + r.out;
    unsigned head = (4u - (unsigned)((uintptr_t)dst & 3)) & 3u;
    if (head > total) head = total;
    const unsigned chunks = 1u + (total - head + 3u) / 4u;
    const unsigned npx = (unsigned)r.h * (unsigned)r.w;
    for (unsigned k = blockIdx.x * 256u + threadIdx.x; k < chunks; k += gridDim.x * 256u) {
        const unsigned lo = k == 0 ? 0u : head + 4u * (k - 1u);
        unsigned hi = k == 0 ? head : lo + 4u;
        if (hi > total) hi = total;
        if (hi <= lo) continue;
        const unsigned len = hi - lo;
        const unsigned px = lo / 3u, sub = lo - 3u * px;                    // first byte's pixel and channel
        unsigned long long bytes = jpeg_pixel(r, ws, px);
        if (sub + len > 3u && px + 1u < npx) bytes |= (unsigned long long)jpeg_pixel(r, ws, px + 1u) << 24;
        const unsigned word = (unsigned)(bytes >> (8u * sub));
        if (len == 4u) {
            *reinterpret_cast<unsigned*>(dst + lo) = word;
        } else {
            for (unsigned i = 0; i < len; ++i) dst[lo + i] = (unsigned char)(word >> (8u * i));
        }
    }
}

// every table of hs_jpeg_decode, checked before any launch; fills rec[0..n)
static int jpeg_check_tables(JpegRec* rec, const int32_t* geom, const int64_t* coef_off, const int64_t* coef_len, const int64_t* out_off,
                             int n, long long coef_bytes, long long out_bytes, long long ws_bytes) {
    const long long need = jpeg_layout(rec, geom, n);
    HS_REQUIRE(need >= 0, "jpeg_decode: a geometry row is not (height, width in 1..65535 with 3 * h * w < 2^31, components 1 or 3, "
                          "luma sampling 1x1, 2x1 or 2x2, width > 4 where chroma is subsampled)");
    HS_REQUIRE(ws_bytes >= need, "jpeg_decode: workspace of %lld bytes, %lld needed", ws_bytes, need);
    long long prev_end = 0;
    for (int i = 0; i < n; ++i) {
        JpegRec& r = rec[i];
        const long long cb = ((long long)r.nblk[0] + 2LL * r.nblk[1]) * 128, ob = 3LL * r.h * r.w;
        HS_REQUIRE(coef_len[i] == cb, "jpeg_decode: image %d: %lld coefficient bytes given, its geometry needs %lld", i,
                   (long long)coef_len[i], cb);
        HS_REQUIRE(coef_off[i] >= 0 && (coef_off[i] & 15) == 0 && coef_off[i] <= coef_bytes - cb,
                   "jpeg_decode: image %d: coefficient offset %lld is misaligned or outside the arena of %lld bytes", i,
                   (long long)coef_off[i], coef_bytes);
        HS_REQUIRE(out_off[i] >= prev_end && out_off[i] <= out_bytes - ob,
                   "jpeg_decode: image %d: output offset %lld overlaps its predecessor or leaves the arena of %lld bytes", i,
                   (long long)out_off[i], out_bytes);
        r.coef = coef_off[i];
        r.out = out_off[i];
        prev_end = out_off[i] + ob;
    }
    return HS_OK;
}

}  // namespace hs

using namespace hs;

extern "C" {

const char* hs_jpeg_status_text(hs_status status) { return hs_jpeg::status_text(status); }

hs_status hs_jpeg_probe(const uint8_t* data, int64_t nbytes, hs_jpeg_info* info) {
    const int st = hs_jpeg::probe(data, nbytes, info);
    if (st != HS_OK) set_error("%s", hs_jpeg::status_text(st));
    return st;
}

hs_status hs_jpeg_entropy_decode(const uint8_t* data, int64_t nbytes, int16_t* coef, int64_t coef_bytes, uint16_t* qtab,
                                 hs_jpeg_info* info) {
    const int st = hs_jpeg::entropy_decode(data, nbytes, coef, coef_bytes, qtab, info);
    if (st != HS_OK) set_error("%s", hs_jpeg::status_text(st));
    return st;
}

int64_t hs_jpeg_ws_bytes(const int32_t* geom, int32_t n) {
    if (!geom || n < 1) return -1;
    JpegRec* rec = (JpegRec*)malloc((size_t)n * sizeof(JpegRec));
    if (!rec) return -1;
    const long long total = jpeg_layout(rec, geom, n);
    free(rec);
    return total;
}

hs_status hs_jpeg_decode(const int16_t* coef, int64_t coef_bytes, const uint16_t* qtab, const int32_t* geom,
                         const int64_t* coef_off, const int64_t* coef_len, const int64_t* out_off, int32_t n, uint8_t* out,
                         int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream) {
    HS_REQUIRE(coef && qtab && geom && coef_off && coef_len && out_off && out && ws, "jpeg_decode: null pointer");
    HS_REQUIRE(n >= 1 && n <= (1 << 20) && coef_bytes >= 0 && out_bytes >= 0, "jpeg_decode: needs 1..2^20 images and non-negative sizes");
    HS_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)coef & 15) == 0 && ((uintptr_t)qtab & 15) == 0,
               "jpeg_decode: the workspace, the coefficient arena and the tables must be 16-byte aligned");
    JpegRec* rec = (JpegRec*)malloc((size_t)n * sizeof(JpegRec));
    HS_REQUIRE(rec, "jpeg_decode: out of host memory");
    const int st0 = jpeg_check_tables(rec, geom, coef_off, coef_len, out_off, n, coef_bytes, out_bytes, ws_bytes);
    if (st0 != HS_OK) {
        free(rec);
        return st0;
    }
    int st = HS_OK;
    for (int n0 = 0; n0 < n && st == HS_OK; n0 += HS_JPEG_CHUNK) {
        const int cnt = n - n0 < HS_JPEG_CHUNK ? n - n0 : HS_JPEG_CHUNK;
        JpegChunk c;
        memset(&c, 0, sizeof c);
        memcpy(c.rec, rec + n0, (size_t)cnt * sizeof(JpegRec));
        long long max_blocks = 0, max_chunks = 0;
        for (int i = 0; i < cnt; ++i) {
            const long long blocks = (long long)c.rec[i].nblk[0] + 2LL * c.rec[i].nblk[1];
            const long long chunks = 2 + 3LL * c.rec[i].h * c.rec[i].w / 4;
            if (blocks > max_blocks) max_blocks = blocks;
            if (chunks > max_chunks) max_chunks = chunks;
        }
        long long gp = (max_chunks + 255) / 256;
        if (gp > 4096) gp = 4096;
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 255) / 256), cnt), dim3(256), 0, (hipStream_t)stream, c,
                           (const char*)coef, (const unsigned short*)qtab, (char*)ws);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)gp, cnt), dim3(256), 0, (hipStream_t)stream, c, (const unsigned char*)ws, out);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            set_error("jpeg_decode: kernel launch -> %s", hipGetErrorString(e));
            st = HS_ERR_HIP;
        }
    }
    free(rec);
    return st;
}

}  // extern "C"
