"""Numpy restatement of baseline JPEG decoding as libjpeg does it by default (the yardstick of hamspine.jpeg).

Written from the JPEG standard (ITU-T T.81: markers, Huffman coding, zig-zag order) and libjpeg's documented arithmetic: the
"islow" integer inverse DCT (two passes, columns then rows, CONST_BITS 13, PASS1_BITS 2), the "fancy" triangle upsamplers for
2x1 and 2x2 chroma and the 16-bit fixed-point YCbCr tables.  tests/gen_jpeg_golden.py pins it against Pillow bit for bit.

  parse(data)         markers up to the first scan: frame, tables, restart interval, where the entropy-coded bytes begin
  coefficients(data)  per component the quantised coefficients int16 [block_rows][block_cols][64] in natural (row-major) order,
                      padded to whole MCUs, the 8-bit quantisation tables in natural order, and the geometry
  planes(...)         dequantise + inverse DCT + 128, clamped: one padded uint8 plane per component
  upsample(...)       chroma planes to the image size over the component's true down-sampled size
  to_rgb(...)         YCbCr -> RGB (or Y -> R = G = B)
  decode(data)        all of it: H x W x 3 uint8

All integer arithmetic is int32 with wrap-around (numpy int32 arrays), so a kernel in plain C integer arithmetic equals it on
every coefficient set, hostile ones included.  Equality with libjpeg is claimed only for streams an encoder made from 8-bit
pixels (libjpeg's range-limit table wraps where this clamps).

Refusals raise Refused(status name); damaged streams raise Corrupt.  The names are those of include/hamspine.h without HS_JPEG_.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

CONST_BITS, PASS1_BITS = 13, 2
FIX_0_298631336, FIX_0_390180644, FIX_0_541196100, FIX_0_765366865 = 2446, 3196, 4433, 6270
FIX_0_899976223, FIX_1_175875602, FIX_1_501321110, FIX_1_847759065 = 7373, 9633, 12299, 15137
FIX_1_961570560, FIX_2_053119869, FIX_2_562915447, FIX_3_072711026 = 16069, 16819, 20995, 25172


class Corrupt(ValueError):
    pass


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


# ------------------------------------------------------------------------------------------------------------- markers
def _u16(d, p):
    if p + 2 > len(d):
        raise Corrupt("truncated")
    return (d[p] << 8) | d[p + 1]


def _huffman(counts, symbols):
    """canonical code of a DHT table: {(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= (1 << length):
                raise Corrupt("Huffman table overflows its code length")
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


def parse(data):
    """Read SOI, APPn, DQT, SOF0/SOF1, DHT, DRI up to the first SOS.  Returns a dict: width, height, precision, components
    [(id, h, v, tq)], qtabs {tq: uint16[64] natural order}, dc / ac {th: table}, restart, jfif, adobe, scan [(td, ta)] in
    frame order, pos (offset of the first entropy-coded byte)."""
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Corrupt("no SOI")
    p = 2
    out = {"qtabs": {}, "dc": {}, "ac": {}, "restart": 0, "jfif": False, "adobe": False, "components": None}
    while True:
        if p + 2 > len(d) or d[p] != 0xFF:
            raise Corrupt("marker expected")
        while p + 1 < len(d) and d[p + 1] == 0xFF:
            p += 1
        if p + 2 > len(d):
            raise Corrupt("truncated")
        m = d[p + 1]
        p += 2
        if m == 0x01:
            continue
        if m == 0xD9 or 0xD0 <= m <= 0xD7 or m == 0xD8 or m == 0x00:
            raise Corrupt(f"marker {m:02x} before a scan")
        n = _u16(d, p)
        if n < 2 or p + n > len(d):
            raise Corrupt("bad marker length")
        seg = d[p + 2:p + n]
        p += n
        if m in (0xC0, 0xC1):
            if out["components"] is not None or len(seg) < 6:
                raise Corrupt("SOF")
            prec, h, w, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec == 12:
                raise Refused("PRECISION")
            if prec != 8:
                raise Corrupt("precision")
            if nf in (2, 4):
                raise Refused("COMPONENTS")
            if nf not in (1, 3) or len(seg) != 6 + 3 * nf or h < 1 or w < 1:
                raise Corrupt("SOF")
            comps = []
            for c in range(nf):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                if not (1 <= hv >> 4 <= 4 and 1 <= (hv & 15) <= 4 and tq <= 3):
                    raise Corrupt("SOF component")
                comps.append((cid, hv >> 4, hv & 15, tq))
            out.update(width=w, height=h, precision=prec, components=comps)
        elif m == 0xC2:
            raise Refused("PROGRESSIVE")
        elif m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise Refused("PROCESS")
        elif m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Refused("ARITHMETIC")
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise Corrupt("DHT")
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
                    raise Corrupt("DHT")
                out["ac" if tc else "dc"][th] = _huffman(counts, seg[q + 17:q + 17 + total])
                q += 17 + total
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq == 1:
                    raise Refused("QTAB16")
                if pq != 0 or tq > 3 or q + 65 > len(seg):
                    raise Corrupt("DQT")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                out["qtabs"][tq] = t
                q += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise Corrupt("DRI")
            out["restart"] = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            out["jfif"] = out["jfif"] or (len(seg) >= 14 and seg[:5] == b"JFIF\0")       # libjpeg: 14 data bytes or more
        elif m == 0xEE:
            out["adobe"] = out["adobe"] or (len(seg) >= 12 and seg[:5] == b"Adobe")
        elif m == 0xDA:
            comps = out["components"]
            if comps is None or len(seg) < 1:
                raise Corrupt("SOS before SOF")
            ns = seg[0]
            if 1 <= ns <= 4 and ns != len(comps):
                raise Refused("MULTISCAN")
            if ns != len(comps) or len(seg) != 4 + 2 * ns:
                raise Corrupt("SOS")
            scan = []
            for c in range(ns):
                cs, t = seg[1 + 2 * c], seg[2 + 2 * c]
                if cs != comps[c][0] or t >> 4 > 3 or (t & 15) > 3:
                    raise Corrupt("SOS component")
                scan.append((t >> 4, t & 15))
            if tuple(seg[1 + 2 * ns:]) != (0, 63, 0):
                raise Corrupt("SOS spectral selection")
            out.update(scan=scan, pos=p)
            return out
        # every other marker with a length (APPn, COM, DNL, ...) is skipped


def geometry(hdr, coded_bytes=None):
    """Accept or refuse the frame (`coded_bytes`: what lies behind SOS, when known); returns {width, height, components, h_samp, v_samp, block_rows, block_cols, coef_bytes}"""
    comps = hdr["components"]
    w, h, nc = hdr["width"], hdr["height"], len(comps)
    if hdr["adobe"]:
        raise Refused("COLORSPACE")
    if nc == 3:
        if not hdr["jfif"] and [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
            raise Refused("COLORSPACE")
        if (comps[1][1:3], comps[2][1:3]) != ((1, 1), (1, 1)) or comps[0][1:3] not in ((1, 1), (2, 1), (2, 2)):
            raise Refused("SAMPLING")
        hs, vs = [c[1] for c in comps], [c[2] for c in comps]
        if hs[0] == 2 and w <= 4:
            raise Refused("NARROW")
    else:
        hs, vs = [1], [1]
    if 3 * h * w > 0x7FFFFFFF:
        raise Refused("TOO_LARGE")
    for c, (td, ta) in zip(comps, hdr["scan"]):
        if c[3] not in hdr["qtabs"] or td not in hdr["dc"] or ta not in hdr["ac"]:
            raise Corrupt("missing table")
    mx, my = -(-w // (8 * hs[0])), -(-h // (8 * vs[0]))
    rows, cols = [my * v for v in vs], [mx * x for x in hs]
    # a coded block is at least a DC and an AC symbol of one bit each
    coded_blocks = -(-w // 8) * -(-h // 8) if nc == 1 else sum(r * c for r, c in zip(rows, cols))
    if coded_bytes is not None and coded_blocks > 4 * coded_bytes:
        raise Corrupt("the scan is shorter than its blocks")
    return {"width": w, "height": h, "components": nc, "h_samp": hs, "v_samp": vs, "block_rows": rows, "block_cols": cols,
            "coef_bytes": sum(r * c * 128 for r, c in zip(rows, cols))}


# ------------------------------------------------------------------------------------------------------- entropy stage
class _Bits:
    """MSB-first bit reader over the entropy-coded segment: FF00 is a stuffed FF, any other FFxx ends the bits"""

    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.cnt = d, pos, 0, 0

    def _fill(self):
        d = self.d
        while self.cnt <= 24 and self.pos < len(d):
            b = d[self.pos]
            if b == 0xFF:
                if self.pos + 1 >= len(d) or d[self.pos + 1] != 0:
                    return
                self.pos += 2
            else:
                self.pos += 1
            self.acc = (self.acc << 8) | b
            self.cnt += 8

    def get(self, k):
        if self.cnt < k:
            self._fill()
            if self.cnt < k:
                raise Corrupt("entropy-coded data ends early")
        self.cnt -= k
        v = (self.acc >> self.cnt) & ((1 << k) - 1)
        self.acc &= (1 << self.cnt) - 1
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.get(1)
            s = table.get((length, code))
            if s is not None:
                return s
        raise Corrupt("Huffman code not in the table")

    def restart(self, index):
        """byte-align, then RSTn with n = index mod 8"""
        if self.cnt >= 8:
            raise Corrupt("bytes before a restart marker")
        self.acc = self.cnt = 0
        d = self.d
        while self.pos + 2 < len(d) and d[self.pos] == 0xFF and d[self.pos + 1] == 0xFF:
            self.pos += 1
        if self.pos + 2 > len(d) or d[self.pos] != 0xFF or d[self.pos + 1] != 0xD0 + (index & 7):
            raise Corrupt("missing or wrong restart marker")
        self.pos += 2


def _extend(v, s):
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def coefficients(data):
    """(coefs, qtabs, geometry): coefs[c] int16 [block_rows][block_cols][64] natural order, qtabs uint16 [components][64]"""
    hdr = parse(data)
    geo = geometry(hdr, len(data) - hdr["pos"])
    comps, nc = hdr["components"], geo["components"]
    coefs = [np.zeros((geo["block_rows"][c], geo["block_cols"][c], 64), np.int16) for c in range(nc)]
    qtabs = np.stack([hdr["qtabs"][comps[c][3]] for c in range(nc)])
    bits = _Bits(bytes(data), hdr["pos"])
    if nc == 1:
        mcus_x, mcus_y = -(-geo["width"] // 8), -(-geo["height"] // 8)
    else:
        mcus_x, mcus_y = geo["block_cols"][1], geo["block_rows"][1]
    pred, ri, done = [0] * nc, hdr["restart"], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            if ri and done and done % ri == 0:
                bits.restart(done // ri - 1)
                pred = [0] * nc
            for c in range(nc):
                dc, ac = hdr["dc"][hdr["scan"][c][0]], hdr["ac"][hdr["scan"][c][1]]
                for v in range(geo["v_samp"][c]):
                    for x in range(geo["h_samp"][c]):
                        blk = coefs[c][my * geo["v_samp"][c] + v, mx * geo["h_samp"][c] + x]
                        s = bits.symbol(dc)
                        if s > 11:
                            raise Corrupt("DC category above 11")
                        pred[c] += _extend(bits.get(s), s) if s else 0
                        if not -32768 <= pred[c] <= 32767:
                            raise Corrupt("DC predictor leaves int16")
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r == 15:
                                    k += 16
                                    if k > 64:
                                        raise Corrupt("run past index 63")
                                    continue
                                if r:
                                    raise Corrupt("EOBn in a baseline scan")
                                break
                            k += r
                            if k > 63:
                                raise Corrupt("run past index 63")
                            if s > 10:
                                raise Corrupt("AC category above 10")
                            blk[ZIGZAG[k]] = _extend(bits.get(s), s)
                            k += 1
            done += 1
    return coefs, qtabs, geo


# --------------------------------------------------------------------------------------------------------- inverse DCT
def _i32(a):
    return np.asarray(a).astype(np.int32)


def _idct_1d(x, shift):
    """libjpeg's jidctint butterfly on the eight int32 arrays x[0..7]; every result descaled by `shift` with the rounding add"""
    c = np.int32
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * c(FIX_0_541196100)
    tmp2 = z1 + z3 * c(-FIX_1_847759065)
    tmp3 = z1 + z2 * c(FIX_0_765366865)
    tmp0 = (x[0] + x[4]) << c(CONST_BITS)
    tmp1 = (x[0] - x[4]) << c(CONST_BITS)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c(FIX_1_175875602)
    tmp0 = tmp0 * c(FIX_0_298631336)
    tmp1 = tmp1 * c(FIX_2_053119869)
    tmp2 = tmp2 * c(FIX_3_072711026)
    tmp3 = tmp3 * c(FIX_1_501321110)
    z1 = z1 * c(-FIX_0_899976223)
    z2 = z2 * c(-FIX_2_562915447)
    z3 = z3 * c(-FIX_1_961570560) + z5
    z4 = z4 * c(-FIX_0_390180644) + z5
    tmp0 = tmp0 + (z1 + z3)
    tmp1 = tmp1 + (z2 + z4)
    tmp2 = tmp2 + (z2 + z3)
    tmp3 = tmp3 + (z1 + z4)
    half = c(1 << (shift - 1))
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return [(o + half) >> c(shift) for o in out]


def idct_blocks(coef, qtab):
    """coef int16 [..., 64], qtab [64] -> uint8 [..., 8, 8]: dequantise, columns (descale 11), rows (descale 18), + 128, clamp"""
    with np.errstate(over="ignore"):
        v = (_i32(coef) * _i32(qtab)).reshape(coef.shape[:-1] + (8, 8))
        col = _idct_1d([v[..., r, :] for r in range(8)], CONST_BITS - PASS1_BITS)
        ws = np.stack(col, axis=-2)
        row = _idct_1d([ws[..., :, k] for k in range(8)], CONST_BITS + PASS1_BITS + 3)
        px = np.stack(row, axis=-1) + np.int32(128)
    return np.clip(px, 0, 255).astype(np.uint8)


def planes(coefs, qtabs):
    """one padded uint8 plane [block_rows * 8][block_cols * 8] per component"""
    out = []
    for c, q in zip(coefs, qtabs):
        b = idct_blocks(c, q)
        out.append(np.ascontiguousarray(b.transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8)))
    return out


# ---------------------------------------------------------------------------------------------------------- upsampling
def _h2v1(p):
    """triangle filter along x of int32 [rows][n] -> [rows][2n]; first and last column copied"""
    n = p.shape[1]
    out = np.empty((p.shape[0], 2 * n), np.int32)
    prev, nxt = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2(p):
    """[rows][n] -> [2 rows][2n]: column sums 3 * near + far, then (3 this + last + 8) >> 4 / (3 this + next + 7) >> 4; the edge
    columns use 4 * this; the context rows beyond the first and last row are those rows again"""
    rows, n = p.shape
    out = np.empty((2 * rows, 2 * n), np.int32)
    above, below = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    for v, far in ((0, above), (1, below)):
        s = 3 * p + far
        last, nxt = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + last + 8) >> 4, (3 * s + nxt + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def upsample(pl, geo):
    """component planes cropped / upsampled to [height][width] int32; the filters run over the true down-sampled size"""
    h, w = geo["height"], geo["width"]
    hmax, vmax = geo["h_samp"][0], geo["v_samp"][0]
    out = []
    for c, p in enumerate(pl):
        hs, vs = geo["h_samp"][c], geo["v_samp"][c]
        dw, dh = -(-w * hs // hmax), -(-h * vs // vmax)
        q = p[:dh, :dw].astype(np.int32)
        if hmax // hs == 2 and vmax // vs == 2:
            q = _h2v2(q)
        elif hmax // hs == 2:
            q = _h2v1(q)
        out.append(q[:h, :w])
    return out


def to_rgb(full):
    """[Y] -> R = G = B = Y; [Y, Cb, Cr] -> RGB by libjpeg's 16-bit tables"""
    if len(full) == 1:
        return np.repeat(full[0].astype(np.uint8)[:, :, None], 3, axis=2)
    y, cb, cr = (a.astype(np.int32) for a in full)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def pixels(coefs, qtabs, geo):
    return to_rgb(upsample(planes(coefs, qtabs), geo))


def decode(data):
    return pixels(*coefficients(data))
