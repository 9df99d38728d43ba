"""numpy restatement of the Pillow arithmetic behind the loaders' transforms (torchvision's PIL backend): the yardstick of
csrc/augment.hip.  Integers and singly rounded f32 / f64 only, no Pillow import: tests/gen_augment_golden.py pins every
function below against Pillow itself and records what it saw in tests/golden/augment_*.npz.

  resize      Pillow's antialiased bilinear (Resample.c): f64 windows and weights, 22-bit fixed-point coefficients,
              horizontal pass rounded to uint8, then the vertical pass
  gather      flips, then Image.rotate(angle, NEAREST) about (w/2, h/2) in 16.16 fixed point (Geometry.c affine_fixed), fill 0
  colour ops  ImageEnhance Brightness / Contrast / Color as Image.blend in f32, and the HSV round trip of adjust_hue
  normalize   (v/255 - mean) / std in f32
"""
import math

import numpy as np

PRECISION_BITS = 22
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- resize
def resize_coeffs(in_size, out_size, first=0, count=None):
    """[(xmin, int32 coefficients)] of outputs first .. first+count-1 of a bilinear resize in_size -> out_size"""
    count = out_size - first if count is None else count
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = (x + xmin - center + 0.5) * ss
            v = -v if v < 0.0 else v
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        k = [(v / ww if ww != 0.0 else v) for v in w]
        out.append((xmin, np.array([int(v * (1 << PRECISION_BITS) + 0.5) for v in k], dtype=np.int64)))
    return out


def _pass(img, coeffs, axis):
    """one resampling pass along `axis` of an (h, w, 3) uint8 image, rounded and clipped to uint8"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(coeffs),) + src.shape[1:], dtype=np.uint8)
    for i, (xmin, k) in enumerate(coeffs):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_window(box, out_h, out_w, off_y, off_x, S):
    """rows off_y .. off_y+S-1 and columns off_x .. off_x+S-1 of `box` resized to (out_h, out_w): horizontal pass first"""
    h, w = box.shape[:2]
    cy = resize_coeffs(h, out_h, off_y, S)
    lo = cy[0][0]
    hi = cy[-1][0] + len(cy[-1][1])
    tmp = _pass(box[lo:hi], resize_coeffs(w, out_w, off_x, S), 1)
    return _pass(tmp, [(ymin - lo, k) for ymin, k in cy], 0)


def crop_resize(img, top, left, h, w, S):
    """img.crop((left, top, left + w, top + h)).resize((S, S), BILINEAR)"""
    return resize_window(img[top:top + h, left:left + w], S, S, 0, 0, S)


def eval_geometry(h, w, resize=256, crop=224):
    """(out_h, out_w, off_y, off_x) of Resize(resize) + CenterCrop(crop) on an h x w image"""
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    return oh, ow, int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))


def eval_resize(img, resize=256, crop=224):
    oh, ow, oy, ox = eval_geometry(img.shape[0], img.shape[1], resize, crop)
    return resize_window(img, oh, ow, oy, ox, crop)


# ---------------------------------------------------------------------------------------------------------------- gather
def rotation_fixed(angle, w, h):
    """the six 16.16 fixed-point values of Image.rotate(angle) on a w x h image, or None when it is a copy"""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def gather(img, hflip, vflip, angle):
    """hflip, vflip, then rotate by `angle` degrees (None: no rotation stage), nearest, fill 0"""
    if hflip:
        img = img[:, ::-1]
    if vflip:
        img = img[::-1]
    fx = None if angle is None else rotation_fixed(angle, img.shape[1], img.shape[0])
    if fx is None:
        return np.ascontiguousarray(img)
    h, w = img.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (fx[2] + fx[0] * x + fx[1] * y) >> 16
    yin = (fx[5] + fx[3] * x + fx[4] * y) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


# ------------------------------------------------------------------------------------------------------------ colour ops
def gray(img):
    v = img.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, x, a):
    """Image.blend(d, x, a): f32 d + a * (x - d), product and sum rounded separately, stored to uint8"""
    a = f32(a)
    t = d.astype(f32) + a * (x.astype(np.int32) - d.astype(np.int32)).astype(f32)
    if not (a >= 0 and a <= f32(1.0)):
        t = np.clip(t, f32(0), f32(255))
    return t.astype(np.uint8)


def l_sum(img):
    return int(gray(img).astype(np.int64).sum())


def contrast_mean(total, n):
    return (2 * total + n) // (2 * n)


def brightness(img, a):
    return blend(np.zeros_like(img), img, a)


def contrast(img, a):
    m = contrast_mean(l_sum(img), img.shape[0] * img.shape[1])
    return blend(np.full_like(img, m), img, a)


def saturation(img, a):
    return blend(np.repeat(gray(img)[..., None], 3, axis=2), img, a)


def rgb_to_hsv(img):
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(f32)
    s = cr / np.where(flat, 1, maxc).astype(f32)
    rc = (maxc - r).astype(f32) / cr
    gc = (maxc - g).astype(f32) / cr
    bc = (maxc - b).astype(f32) / cr
    d = np.float64
    h = np.where(r == maxc, (bc - gc).astype(f32),
                 np.where(g == maxc, (d(2.0) + rc.astype(d) - bc.astype(d)).astype(f32),
                          (d(4.0) + gc.astype(d) - rc.astype(d)).astype(f32)))
    h = np.fmod(h.astype(d) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(d) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(d) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(flat, 0, uh), np.where(flat, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _round_half_away(v):
    """C's round() on non-negative doubles (v - floor(v) is exact, v + 0.5 need not be)"""
    fl = np.floor(v)
    return (fl + (v - fl >= 0.5)).astype(np.int64)


def hsv_to_rgb(hsv):
    d = np.float64
    h, s, v = (hsv[..., c] for c in range(3))
    hf = h.astype(f32).astype(d) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int64)
    f = (hf - i.astype(f32).astype(d)).astype(f32)
    fs = (s.astype(f32).astype(d) / 255.0).astype(f32)
    vf = v.astype(f32).astype(d)
    p = np.clip(_round_half_away(vf * (1.0 - fs.astype(d))), 0, 255)
    q = np.clip(_round_half_away(vf * (1.0 - (fs * f).astype(d))), 0, 255)
    t = np.clip(_round_half_away(vf * (1.0 - fs.astype(d) * (1.0 - f.astype(d)))), 0, 255)
    v = v.astype(np.int64)
    sel = i % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(hsv.shape, dtype=np.int64)
    for c in range(3):
        out[..., c] = np.choose(sel, [row[c] for row in table])
    out = np.where((s == 0)[..., None], v[..., None], out)
    return out.astype(np.uint8)


def hue_shift(hue):
    """the uint8 that adjust_hue adds to the hue channel: trunc(hue * 255) mod 256"""
    return int(hue * 255) % 256


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + hue_shift(shift)) % 256
    return hsv_to_rgb(hsv)


_OPS = {BRIGHTNESS: brightness, CONTRAST: contrast, SATURATION: saturation, HUE: hue}


def color_ops(img, order, enable, factors):
    """the enabled ops of `order` (a permutation of 0..3) with factors[op], the uint8 image stored between ops"""
    for op in order:
        if enable[op]:
            img = _OPS[op](img, factors[op])
    return img


# --------------------------------------------------------------------------------------------------------------- the rest
def normalize(img, mean, std):
    """(h, w, 3) uint8 -> (3, h, w) f32, ToTensor then Normalize"""
    v = img.astype(f32) / f32(255.0)
    v = (v - np.asarray(mean, dtype=f32)) / np.asarray(std, dtype=f32)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def train_u8(img, p):
    """the uint8 (S, S, 3) image of one output; p: dict(top, left, h, w, S, hflip, vflip, angle (None: none), order, enable,
    factors)"""
    x = crop_resize(img, p["top"], p["left"], p["h"], p["w"], p["S"])
    x = gather(x, p["hflip"], p["vflip"], p["angle"])
    return color_ops(x, p["order"], p["enable"], p["factors"])


def row_params(ip, fp, S):
    """one row of the C ABI's tables (hamspine.augment: IP_*, FP_*) as train_u8's dict"""
    ip = [int(v) for v in ip]
    return dict(top=ip[1], left=ip[2], h=ip[3], w=ip[4], S=S, hflip=ip[5], vflip=ip[6], angle=float(fp[0]) if ip[7] else None,
                order=ip[8:12], enable=ip[12:16], factors=[float(v) for v in fp[1:5]])


def contrast_l_sum(img, p):
    """the sum of L the contrast op of `p` meets (0 when it has none): after the gather and the colour ops in front of it"""
    if not p["enable"][CONTRAST]:
        return 0
    x = gather(crop_resize(img, p["top"], p["left"], p["h"], p["w"], p["S"]), p["hflip"], p["vflip"], p["angle"])
    before = p["order"][:p["order"].index(CONTRAST)]
    return l_sum(color_ops(x, before, p["enable"], p["factors"]))


def smooth_image(h, w, seed):
    """a smooth, saturated test image: three phase-shifted low-frequency waves, so neighbouring hues stay close"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 3), dtype=np.uint8)
    for c in range(3):
        fy, fx, ph = rng.uniform(0.5, 2.5) / max(h, 2), rng.uniform(0.5, 2.5) / max(w, 2), rng.uniform(0, 2 * np.pi)
        out[..., c] = np.clip(127.5 + 127.5 * np.sin(2 * np.pi * (fy * y + fx * x) + ph + 2.1 * c), 0, 255).astype(np.uint8)
    return out
