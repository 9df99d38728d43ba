// Host entropy stage of the JPEG decoder: file bytes -> quantised DCT coefficients (ITU-T T.81 baseline Huffman, one interleaved
// scan).  Plain C++: no HIP, no global state, no allocation; every function is re-entrant.  jpeg.hip wraps probe() and
// entropy_decode() as hs_jpeg_probe / hs_jpeg_entropy_decode, and tools/jpeg_host_check.cpp includes this header on its own to
// run them under the host sanitizers.  tests/jpeg_ref.py is the same decoder in numpy; the two agree on what they accept, what
// they refuse and what is corrupt.
//
// Bounds: every read of the input goes through a length check (Reader::u8 / Bits::fill), every coefficient index is < 64 by
// construction (k <= 63 is checked before the store) and every block address is computed from the geometry that sized the buffer.
// Progress: each Huffman symbol consumes at least one bit and a block takes at most 64 symbols, so decoding cannot loop without
// consuming input.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../../include/hamspine.h"

namespace hs_jpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static constexpr int kLookBits = 9;

struct Huff {
    bool set;
    // codes of at most kLookBits bits, by their left-aligned prefix: (length << 8) | symbol, 0 = a longer code or none
    uint16_t look[1 << kLookBits];
    int32_t maxcode[18];   // largest code of each length, -1 where the length has none; [17] ends every search
    int32_t valptr[17];    // index of the first symbol of each length, minus its first code
    uint8_t symbols[256];
};

struct Header {
    int width, height, ncomp;
    int cid[4], hs[4], vs[4], tq[4], td[4], ta[4];
    bool have_sof, jfif, adobe;
    int restart;
    bool q_set[4];
    uint16_t q[4][64];      // natural order
    Huff dc[4], ac[4];
    int64_t pos;            // offset of the first entropy-coded byte
};

static inline const char* status_text(int st) {
    switch (st) {
        case HS_OK: return "";
        case HS_ERR_ARG: return "jpeg: bad argument (null pointer or a coefficient buffer that is too small)";
        case HS_JPEG_ERR_CORRUPT: return "jpeg: corrupt or truncated stream";
        case HS_JPEG_ERR_PROGRESSIVE: return "jpeg: progressive files are not decoded";
        case HS_JPEG_ERR_ARITHMETIC: return "jpeg: arithmetic coding is not decoded";
        case HS_JPEG_ERR_PROCESS: return "jpeg: lossless and hierarchical files are not decoded";
        case HS_JPEG_ERR_PRECISION: return "jpeg: 12-bit samples are not decoded";
        case HS_JPEG_ERR_QTAB16: return "jpeg: 16-bit quantisation tables are not decoded";
        case HS_JPEG_ERR_COMPONENTS: return "jpeg: only 1 or 3 components are decoded";
        case HS_JPEG_ERR_SAMPLING: return "jpeg: only luma 1x1, 2x1 or 2x2 over 1x1 chroma is decoded";
        case HS_JPEG_ERR_MULTISCAN: return "jpeg: files with more than one scan are not decoded";
        case HS_JPEG_ERR_COLORSPACE: return "jpeg: Adobe-marked or RGB-id files are not decoded";
        case HS_JPEG_ERR_NARROW: return "jpeg: width <= 4 with horizontally subsampled chroma is not decoded";
        case HS_JPEG_ERR_TOO_LARGE: return "jpeg: frames of 2^31 or more output bytes (3 * h * w) are not decoded";
    }
    return "jpeg: unknown status";
}

// DHT: canonical codes from the 16 counts; false when a length holds more codes than it has
static inline bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* symbols, int total) {
    memset(&h, 0, sizeof h);
    memcpy(h.symbols, symbols, (size_t)total);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        h.valptr[len] = k - code;
        if (code + counts[len - 1] > (1 << len)) return false;
        for (int i = 0; i < counts[len - 1]; ++i, ++code, ++k) {
            if (len <= kLookBits) {
                const int first = code << (kLookBits - len);
                for (int f = 0; f < (1 << (kLookBits - len)); ++f) h.look[first + f] = (uint16_t)((len << 8) | symbols[k]);
            }
        }
        h.maxcode[len] = counts[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.set = true;
    return true;
}

static inline int rd16(const uint8_t* d, int64_t p) { return (d[p] << 8) | d[p + 1]; }

// Markers up to the first SOS.  Returns HS_OK, a refusal or HS_JPEG_ERR_CORRUPT.
static inline int parse(const uint8_t* d, int64_t n, Header& H) {
    H.width = H.height = H.ncomp = H.restart = 0;
    H.have_sof = H.jfif = H.adobe = false;
    H.pos = 0;
    for (int i = 0; i < 4; ++i) H.q_set[i] = H.dc[i].set = H.ac[i].set = false;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return HS_JPEG_ERR_CORRUPT;
    int64_t p = 2;
    for (;;) {
        if (p + 2 > n || d[p] != 0xFF) return HS_JPEG_ERR_CORRUPT;
        while (p + 1 < n && d[p + 1] == 0xFF) ++p;
        if (p + 2 > n) return HS_JPEG_ERR_CORRUPT;
        const int m = d[p + 1];
        p += 2;
        if (m == 0x01) continue;
        if (m == 0xD9 || (m >= 0xD0 && m <= 0xD8) || m == 0x00) return HS_JPEG_ERR_CORRUPT;
        if (p + 2 > n) return HS_JPEG_ERR_CORRUPT;
        const int len = rd16(d, p);
        if (len < 2 || p + len > n) return HS_JPEG_ERR_CORRUPT;
        const uint8_t* seg = d + p + 2;
        const int sl = len - 2;
        p += len;
        if (m == 0xC0 || m == 0xC1) {
            if (H.have_sof || sl < 6) return HS_JPEG_ERR_CORRUPT;
            const int prec = seg[0], nf = seg[5];
            if (prec == 12) return HS_JPEG_ERR_PRECISION;
            if (prec != 8) return HS_JPEG_ERR_CORRUPT;
            if (nf == 2 || nf == 4) return HS_JPEG_ERR_COMPONENTS;
            H.height = rd16(seg, 1);
            H.width = rd16(seg, 3);
            if ((nf != 1 && nf != 3) || sl != 6 + 3 * nf || H.height < 1 || H.width < 1) return HS_JPEG_ERR_CORRUPT;
            for (int c = 0; c < nf; ++c) {
                H.cid[c] = seg[6 + 3 * c];
                H.hs[c] = seg[7 + 3 * c] >> 4;
                H.vs[c] = seg[7 + 3 * c] & 15;
                H.tq[c] = seg[8 + 3 * c];
                if (H.hs[c] < 1 || H.hs[c] > 4 || H.vs[c] < 1 || H.vs[c] > 4 || H.tq[c] > 3) return HS_JPEG_ERR_CORRUPT;
            }
            H.ncomp = nf;
            H.have_sof = true;
        } else if (m == 0xC2) {
            return HS_JPEG_ERR_PROGRESSIVE;
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            return HS_JPEG_ERR_PROCESS;
        } else if (m >= 0xC9 && m <= 0xCF) {
            return HS_JPEG_ERR_ARITHMETIC;
        } else if (m == 0xC4) {
            int q = 0;
            while (q < sl) {
                if (q + 17 > sl) return HS_JPEG_ERR_CORRUPT;
                const int tc = seg[q] >> 4, th = seg[q] & 15;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += seg[q + 1 + i];
                if (tc > 1 || th > 3 || total > 256 || q + 17 + total > sl) return HS_JPEG_ERR_CORRUPT;
                if (!build_huff(tc ? H.ac[th] : H.dc[th], seg + q + 1, seg + q + 17, total)) return HS_JPEG_ERR_CORRUPT;
                q += 17 + total;
            }
        } else if (m == 0xDB) {
            int q = 0;
            while (q < sl) {
                const int pq = seg[q] >> 4, tq = seg[q] & 15;
                if (pq == 1) return HS_JPEG_ERR_QTAB16;
                if (pq != 0 || tq > 3 || q + 65 > sl) return HS_JPEG_ERR_CORRUPT;
                for (int i = 0; i < 64; ++i) H.q[tq][kZigzag[i]] = seg[q + 1 + i];
                H.q_set[tq] = true;
                q += 65;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return HS_JPEG_ERR_CORRUPT;
            H.restart = rd16(seg, 0);
        } else if (m == 0xE0) {
            if (sl >= 14 && memcmp(seg, "JFIF\0", 5) == 0) H.jfif = true;      // libjpeg takes a JFIF APP0 of 14 data bytes or more
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) H.adobe = true;
        } else if (m == 0xDA) {
            if (!H.have_sof || sl < 1) return HS_JPEG_ERR_CORRUPT;
            const int ns = seg[0];
            if (ns >= 1 && ns <= 4 && ns != H.ncomp) return HS_JPEG_ERR_MULTISCAN;
            if (ns != H.ncomp || sl != 4 + 2 * ns) return HS_JPEG_ERR_CORRUPT;
            for (int c = 0; c < ns; ++c) {
                H.td[c] = seg[2 + 2 * c] >> 4;
                H.ta[c] = seg[2 + 2 * c] & 15;
                if (seg[1 + 2 * c] != H.cid[c] || H.td[c] > 3 || H.ta[c] > 3) return HS_JPEG_ERR_CORRUPT;
            }
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return HS_JPEG_ERR_CORRUPT;
            H.pos = p;
            return HS_OK;
        }
        // every other marker with a length (APPn, COM, DNL, ...) is skipped
    }
}

// accept or refuse the frame and fill the geometry; `coded_bytes` is what lies behind SOS
static inline int geometry(const Header& H, int64_t coded_bytes, hs_jpeg_info* info) {
    if (H.adobe) return HS_JPEG_ERR_COLORSPACE;
    memset(info, 0, sizeof *info);
    if (H.ncomp == 3) {
        if (!H.jfif && H.cid[0] == 'R' && H.cid[1] == 'G' && H.cid[2] == 'B') return HS_JPEG_ERR_COLORSPACE;
        const bool luma_ok = (H.hs[0] == 1 && H.vs[0] == 1) || (H.hs[0] == 2 && H.vs[0] == 1) || (H.hs[0] == 2 && H.vs[0] == 2);
        if (!luma_ok || H.hs[1] != 1 || H.vs[1] != 1 || H.hs[2] != 1 || H.vs[2] != 1) return HS_JPEG_ERR_SAMPLING;
        if (H.hs[0] == 2 && H.width <= 4) return HS_JPEG_ERR_NARROW;
    }
    if (3LL * H.width * H.height > 0x7fffffffLL) return HS_JPEG_ERR_TOO_LARGE;
    for (int c = 0; c < H.ncomp; ++c)
        if (!H.q_set[H.tq[c]] || !H.dc[H.td[c]].set || !H.ac[H.ta[c]].set) return HS_JPEG_ERR_CORRUPT;
    info->width = H.width;
    info->height = H.height;
    info->components = H.ncomp;
    info->restart_interval = H.restart;
    const int hmax = H.ncomp == 3 ? H.hs[0] : 1, vmax = H.ncomp == 3 ? H.vs[0] : 1;
    const int mx = (H.width + 8 * hmax - 1) / (8 * hmax), my = (H.height + 8 * vmax - 1) / (8 * vmax);
    for (int c = 0; c < H.ncomp; ++c) {
        info->h_samp[c] = H.ncomp == 3 ? H.hs[c] : 1;
        info->v_samp[c] = H.ncomp == 3 ? H.vs[c] : 1;
        info->block_rows[c] = my * info->v_samp[c];
        info->block_cols[c] = mx * info->h_samp[c];
        info->coef_bytes += (int64_t)info->block_rows[c] * info->block_cols[c] * 128;
    }
    // every coded block is at least a DC and an AC symbol of one bit each: a scan of fewer bits is truncated, whatever it holds
    const int64_t coded_blocks = H.ncomp == 1 ? (int64_t)((H.width + 7) / 8) * ((H.height + 7) / 8) : info->coef_bytes / 128;
    if (coded_blocks > coded_bytes * 4) return HS_JPEG_ERR_CORRUPT;
    return HS_OK;
}

// MSB-first bit reader over the entropy-coded segment: FF00 is a stuffed FF, any other FFxx ends the bits (it is not consumed)
struct Bits {
    const uint8_t* d;
    int64_t n, pos;
    uint32_t acc;   // the next bits, left-aligned
    int cnt;

    inline void fill() {
        while (cnt <= 24 && pos < n) {
            const uint32_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || d[pos + 1] != 0) return;
                pos += 2;
            } else {
                ++pos;
            }
            acc |= b << (24 - cnt);
            cnt += 8;
        }
    }
    // k in 1..16; false when the data ends first
    inline bool get(int k, int* v) {
        if (cnt < k) {
            fill();
            if (cnt < k) return false;
        }
        *v = (int)(acc >> (32 - k));
        acc <<= k;
        cnt -= k;
        return true;
    }
    // one Huffman symbol, or -1 (a code outside the table, or the data ends)
    inline int symbol(const Huff& h) {
        if (cnt < 16) fill();
        const int e = h.look[acc >> (32 - kLookBits)];
        if (e) {
            const int len = e >> 8;
            if (len > cnt) return -1;
            acc <<= len;
            cnt -= len;
            return e & 255;
        }
        int len = kLookBits + 1;
        int code = (int)(acc >> (32 - len));
        while (len <= 16 && code > h.maxcode[len]) {
            ++len;
            code = (int)(acc >> (32 - len));
        }
        if (len > 16 || len > cnt) return -1;
        acc <<= len;
        cnt -= len;
        return h.symbols[(h.valptr[len] + code) & 255];
    }
    // byte-align, then RSTn with n = index mod 8
    inline bool restart(int index) {
        if (cnt >= 8) return false;
        acc = 0;
        cnt = 0;
        while (pos + 2 < n && d[pos] == 0xFF && d[pos + 1] == 0xFF) ++pos;
        if (pos + 2 > n || d[pos] != 0xFF || d[pos + 1] != 0xD0 + (index & 7)) return false;
        pos += 2;
        return true;
    }
};

static inline int extend(int v, int s) { return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1; }

// one 8x8 block into blk[64] (natural order, zeroed by the caller)
static inline bool decode_block(Bits& b, const Huff& dc, const Huff& ac, int* pred, int16_t* blk) {
    int s = b.symbol(dc), v = 0;
    if (s < 0 || s > 11) return false;
    if (s) {
        if (!b.get(s, &v)) return false;
        *pred += extend(v, s);
    }
    if (*pred < -32768 || *pred > 32767) return false;
    blk[0] = (int16_t)*pred;
    int k = 1;
    while (k < 64) {
        const int rs = b.symbol(ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r == 15) {
                k += 16;
                if (k > 64) return false;
                continue;
            }
            if (r) return false;
            break;
        }
        k += r;
        if (k > 63 || s > 10) return false;
        if (!b.get(s, &v)) return false;
        blk[kZigzag[k]] = (int16_t)extend(v, s);
        ++k;
    }
    return true;
}

static inline int probe(const uint8_t* data, int64_t nbytes, hs_jpeg_info* info) {
    if (!data || !info || nbytes < 0) return HS_ERR_ARG;
    Header H;
    int st = parse(data, nbytes, H);
    if (st != HS_OK) return st;
    hs_jpeg_info g;
    st = geometry(H, nbytes - H.pos, &g);
    if (st == HS_OK) *info = g;
    return st;
}

static inline int entropy_decode(const uint8_t* data, int64_t nbytes, int16_t* coef, int64_t coef_bytes, uint16_t* qtab,
                                 hs_jpeg_info* info) {
    if (!data || !info || !coef || !qtab || nbytes < 0) return HS_ERR_ARG;
    Header H;
    int st = parse(data, nbytes, H);
    if (st != HS_OK) return st;
    hs_jpeg_info g;
    st = geometry(H, nbytes - H.pos, &g);
    if (st != HS_OK) return st;
    if (coef_bytes < g.coef_bytes) return HS_ERR_ARG;
    *info = g;
    memset(coef, 0, (size_t)g.coef_bytes);
    memset(qtab, 0, sizeof(uint16_t) * HS_JPEG_MAX_COMPONENTS * 64);
    int16_t* base[3] = {coef, coef, coef};
    for (int c = 0; c < g.components; ++c) {
        memcpy(qtab + 64 * c, H.q[H.tq[c]], 64 * sizeof(uint16_t));
        if (c) base[c] = base[c - 1] + (int64_t)g.block_rows[c - 1] * g.block_cols[c - 1] * 64;
    }
    // a one-component scan is not interleaved: its MCU is one block and only the blocks that hold pixels are coded
    const int mcus_x = g.components == 1 ? (g.width + 7) / 8 : g.block_cols[1];
    const int mcus_y = g.components == 1 ? (g.height + 7) / 8 : g.block_rows[1];
    Bits b = {data, nbytes, H.pos, 0u, 0};
    int pred[3] = {0, 0, 0};
    int64_t done = 0;
    for (int my = 0; my < mcus_y; ++my) {
        for (int mx = 0; mx < mcus_x; ++mx, ++done) {
            if (H.restart && done && done % H.restart == 0) {
                if (!b.restart((int)((done / H.restart - 1) & 7))) return HS_JPEG_ERR_CORRUPT;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < g.components; ++c) {
                const Huff& dc = H.dc[H.td[c]];
                const Huff& ac = H.ac[H.ta[c]];
                for (int v = 0; v < g.v_samp[c]; ++v)
                    for (int x = 0; x < g.h_samp[c]; ++x) {
                        const int64_t row = (int64_t)my * g.v_samp[c] + v, col = (int64_t)mx * g.h_samp[c] + x;
                        if (!decode_block(b, dc, ac, &pred[c], base[c] + (row * g.block_cols[c] + col) * 64)) return HS_JPEG_ERR_CORRUPT;
                    }
            }
        }
    }
    return HS_OK;
}

}  // namespace hs_jpeg
