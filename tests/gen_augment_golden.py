"""Records Pillow's own results for the transforms that csrc/augment.hip restates, stage by stage and chained, into
tests/golden/augment_stages.npz and augment_chains.npz.  Run where Pillow is installed:

    python tests/gen_augment_golden.py

Every recorded Pillow call is the one torchvision's PIL backend makes.  The script also measures tests/augment_ref.py
against what it records and stores the largest byte difference and the share of differing pixels of the hue stage and of
the chains that contain it (`hue_max_diff`, `hue_share`, `chain_max_diff`, `chain_share`); tests/test_augment_cpu.py allows
exactly that.  With Pillow 12.2.0 all four are 0, also over all 2^24 colours (`hue_exhaustive_*`).
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S = 24


def pil_hue(im, f):
    h, s, v = im.convert("HSV").split()
    np_h = (np.array(h, dtype=np.uint8).astype(np.int64) + int(f * 255) % 256) % 256      # adjust_hue's wrapping uint8 add
    return Image.merge("HSV", (Image.fromarray(np_h.astype(np.uint8), "L"), s, v)).convert("RGB")


PIL_OPS = {R.BRIGHTNESS: lambda im, f: ImageEnhance.Brightness(im).enhance(f),
           R.CONTRAST: lambda im, f: ImageEnhance.Contrast(im).enhance(f),
           R.SATURATION: lambda im, f: ImageEnhance.Color(im).enhance(f),
           R.HUE: pil_hue}


def pil_gather(im, hflip, vflip, angle):
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    if angle is not None:
        im = im.rotate(angle, Image.NEAREST, False, None, fillcolor=0)
    return im


def pil_train(img, p):
    im = Image.fromarray(img).crop((p["left"], p["top"], p["left"] + p["w"], p["top"] + p["h"])).resize((S, S), Image.BILINEAR)
    im = pil_gather(im, p["hflip"], p["vflip"], p["angle"])
    for op in p["order"]:
        if p["enable"][op]:
            im = PIL_OPS[op](im, p["factors"][op])
    return np.array(im)


def diff_stats(ref, got):
    d = np.abs(ref.astype(np.int64) - got.astype(np.int64))
    return int(d.max()), float((d != 0).any(-1).mean())


def stages():
    out = {}
    srcs = [R.smooth_image(45, 61, 1), R.smooth_image(37, 29, 2), R.smooth_image(5, 7, 3), R.smooth_image(1, 1, 4),
            np.random.default_rng(5).integers(0, 256, (40, 33, 3), dtype=np.uint8)]
    # (source, top, left, h, w): interior, each edge touched, 1-pixel-wide and 1-pixel-high boxes, upscaling, the whole image
    boxes = [(0, 3, 5, 30, 40), (0, 0, 7, 20, 30), (0, 9, 0, 30, 25), (0, 15, 4, 30, 41), (0, 2, 21, 33, 40), (0, 0, 0, 45, 61),
             (1, 4, 28, 20, 1), (1, 36, 0, 1, 29), (1, 0, 0, 37, 29), (2, 0, 0, 5, 7), (2, 1, 2, 3, 4), (3, 0, 0, 1, 1),
             (4, 0, 0, 40, 33), (4, 5, 6, 31, 11)]
    for i, s in enumerate(srcs):
        out[f"src{i}"] = s
    out["resize_boxes"] = np.array(boxes, dtype=np.int32)
    out["resize_out"] = np.stack([np.array(Image.fromarray(srcs[s]).crop((l, t, l + w, t + h)).resize((S, S), Image.BILINEAR))
                                  for s, t, l, h, w in boxes])
    # Resize(r) + CenterCrop(24) on small sources, odd and even differences
    ev = [(0, 32), (1, 32), (4, 33), (2, 24), (0, 25)]
    out["eval_cases"] = np.array(ev, dtype=np.int32)
    res = []
    for s, r in ev:
        oh, ow, oy, ox = R.eval_geometry(srcs[s].shape[0], srcs[s].shape[1], r, S)
        res.append(np.array(Image.fromarray(srcs[s]).resize((ow, oh), Image.BILINEAR).crop((ox, oy, ox + S, oy + S))))
    out["eval_out"] = np.stack(res)
    # gather: every flip combination without rotation, then rotations
    base = np.array(Image.fromarray(srcs[0]).resize((S, S), Image.BILINEAR))
    odd = R.smooth_image(25, 25, 6)
    out["gather_base"], out["gather_odd"] = base, odd
    out["flip_out"] = np.stack([np.array(pil_gather(Image.fromarray(base), hf, vf, None)) for hf in (0, 1) for vf in (0, 1)])
    angles = [45.0, -45.0, 0.0, 13.7, 360.0, -15.3, 90.0, 180.0, 270.0, 44.99]
    out["angles"] = np.array(angles)
    out["rot_out"] = np.stack([np.array(pil_gather(Image.fromarray(base), 0, 0, a)) for a in angles])
    out["rot_odd_out"] = np.stack([np.array(pil_gather(Image.fromarray(odd), 0, 0, a)) for a in angles])
    # colour
    col = [R.smooth_image(S, S, 7), np.random.default_rng(8).integers(0, 256, (S, S, 3), dtype=np.uint8),
           np.zeros((S, S, 3), np.uint8), np.full((S, S, 3), 255, np.uint8), np.full((S, S, 3), 128, np.uint8)]
    out["colour_src"] = np.stack(col)
    out["gray_out"] = np.stack([np.array(Image.fromarray(c).convert("L")) for c in col])
    factors = [0.8, 1.2, 0.93, 1.07]
    out["factors"] = np.array(factors)
    for op, name in ((R.BRIGHTNESS, "brightness"), (R.CONTRAST, "contrast"), (R.SATURATION, "saturation")):
        out[name + "_out"] = np.stack([[np.array(PIL_OPS[op](Image.fromarray(c), f)) for f in factors] for c in col])
    hues = [0.1, -0.1, 0.0, 0.037]
    out["hues"] = np.array(hues)
    out["hue_out"] = np.stack([[np.array(pil_hue(Image.fromarray(c), f)) for f in hues] for c in col])
    got = np.stack([[R.hue(c, f) for f in hues] for c in col])
    mx, share = diff_stats(out["hue_out"], got)
    out["hue_max_diff"], out["hue_share"] = np.int64(mx), np.float64(share)
    # all 2^24 colours through the HSV round trip (recorded as figures only)
    v = np.arange(256, dtype=np.uint8)
    full = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(4096, 4096, 3)
    mx, share = diff_stats(np.array(pil_hue(Image.fromarray(full), 0.1)), R.hue(full, 0.1))
    out["hue_exhaustive_max_diff"], out["hue_exhaustive_share"] = np.int64(mx), np.float64(share)
    return out


def chains():
    import itertools
    rng = np.random.default_rng(11)
    srcs = [R.smooth_image(45, 61, 21), R.smooth_image(37, 29, 22), R.smooth_image(5, 7, 23)]
    orders = list(itertools.permutations(range(4)))
    ip, fp = [], []
    for n in range(16):
        s = n % 3
        H, W = srcs[s].shape[:2]
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        t, l = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        order = orders[int(rng.integers(0, 24))]
        enable = [1, 1, 1, 1] if n < 12 else [int(v) for v in rng.integers(0, 2, 4)]
        ip.append([s, t, l, h, w, n & 1, (n >> 1) & 1, int(n % 5 != 4), *order, *enable])
        fp.append([rng.uniform(-45, 45), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.1, 0.1)])
    ip, fp = np.array(ip, dtype=np.int32), np.array(fp, dtype=np.float64)
    ref = np.stack([pil_train(srcs[r[0]], R.row_params(r, f, S)) for r, f in zip(ip, fp)])
    got = np.stack([R.train_u8(srcs[r[0]], R.row_params(r, f, S)) for r, f in zip(ip, fp)])
    mx, share = diff_stats(ref, got)
    out = {f"src{i}": s for i, s in enumerate(srcs)}
    out.update(iparams=ip, fparams=fp, out=ref, chain_max_diff=np.int64(mx), chain_share=np.float64(share))
    return out


if __name__ == "__main__":
    for name, data in (("augment_stages", stages()), ("augment_chains", chains())):
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **data)
        print(name, os.path.getsize(path), "bytes;", {k: data[k].item() for k in data if k.endswith(("_diff", "_share"))})
