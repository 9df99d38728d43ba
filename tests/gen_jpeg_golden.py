"""Writes tests/golden/jpeg_cases.npz: small JPEG files encoded AND decoded by Pillow, pinned against tests/jpeg_ref.py.

Run where Pillow is installed (`python tests/gen_jpeg_golden.py`); the tests only read the fixture.  Every accepted case must
decode to Pillow's pixels bit for bit through jpeg_ref, or nothing is written.  Per case NAME the fixture holds
  bytes/NAME   the file                       pixels/NAME  Pillow's Image.open(...).convert("RGB"), H x W x 3 uint8
  coef/NAME    jpeg_ref's coefficients, int16, the components' [block_rows][block_cols][64] arrays one after another
  qtab/NAME    uint16 [components][64], natural order
  geom/NAME    int32: height, width, components, then h_samp[3], v_samp[3], block_rows[3], block_cols[3] (0 where unused)
plus `accepted` / `refused` (names; refused cases hold bytes, pixels and the expected status name in status/NAME) and the
version strings of Pillow and of the libjpeg-turbo it was built on.
"""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
SIZES = [(1, 5), (8, 8), (16, 16), (9, 6), (17, 23), (33, 50)]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def picture(h, w, seed):
    """smooth colour gradients plus an edge and a little noise: every DCT frequency and both chroma planes carry something"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 3.1 + seed) * np.cos(y / 4.3), 128 + 110 * np.cos((x + 2 * y) / 5.7 + seed),
                    255.0 * ((x + y) % 11 < 5)], axis=2)
    img += rng.normal(0, 12, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def cases():
    out = {}
    for i, (h, w) in enumerate(SIZES):
        for name, sub in SUBSAMPLING.items():
            out[f"{h}x{w}_{name}"] = encode(picture(h, w, i), quality=75, subsampling=sub)
    out["21x19_gray"] = encode(picture(21, 19, 7)[:, :, 0].copy(), quality=75)
    out["17x23_420_q30"] = encode(picture(17, 23, 8), quality=30, subsampling=2)
    out["17x23_422_q95"] = encode(picture(17, 23, 9), quality=95, subsampling=1)
    out["33x50_420_optimize"] = encode(picture(33, 50, 10), quality=75, subsampling=2, optimize=True)
    out["33x50_420_restart3"] = encode(picture(33, 50, 11), quality=75, subsampling=2, restart_marker_blocks=3)
    out["33x50_422_restart3"] = encode(picture(33, 50, 12), quality=75, subsampling=1, restart_marker_blocks=3)
    noise = np.random.default_rng(13).integers(0, 256, (40, 40, 3), dtype=np.uint8)
    out["40x40_444_noise_q100"] = encode(noise, quality=100, subsampling=0)
    out["40x40_420_noise_q100"] = encode(noise, quality=100, subsampling=2)
    refused = {"16x16_progressive": (encode(picture(16, 16, 14), quality=75, subsampling=2, progressive=True), "PROGRESSIVE"),
               "9x4_420": (encode(picture(9, 4, 15), quality=75, subsampling=2), "NARROW")}
    return out, refused


def main():
    import PIL
    from PIL import features
    accepted, refused = cases()
    store = {"accepted": np.array(sorted(accepted)), "refused": np.array(sorted(refused)),
             "pillow_version": np.array(PIL.__version__), "libjpeg_turbo_version": np.array(str(features.version("libjpeg_turbo")))}
    for name, data in accepted.items():
        want = pillow_pixels(data)
        coefs, qtabs, geo = jpeg_ref.coefficients(data)
        got = jpeg_ref.pixels(coefs, qtabs, geo)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad = int((got != want).sum()) if got.shape == want.shape else -1
            raise SystemExit(f"{name}: jpeg_ref differs from Pillow in {bad} samples; fixture NOT written")
        pad = lambda v: list(v) + [0] * (3 - len(v))
        store[f"bytes/{name}"] = np.frombuffer(data, np.uint8)
        store[f"pixels/{name}"] = want
        store[f"coef/{name}"] = np.concatenate([c.reshape(-1) for c in coefs])
        store[f"qtab/{name}"] = qtabs
        store[f"geom/{name}"] = np.array([geo["height"], geo["width"], geo["components"]] + pad(geo["h_samp"]) + pad(geo["v_samp"]) +
                                         pad(geo["block_rows"]) + pad(geo["block_cols"]), np.int32)
    for name, (data, status) in refused.items():
        try:
            jpeg_ref.coefficients(data)
        except jpeg_ref.Refused as e:
            if e.status != status:
                raise SystemExit(f"{name}: jpeg_ref refuses with {e.status}, expected {status}")
        else:
            raise SystemExit(f"{name}: jpeg_ref accepted a case it must refuse")
        store[f"bytes/{name}"] = np.frombuffer(data, np.uint8)
        store[f"pixels/{name}"] = pillow_pixels(data)
        store[f"status/{name}"] = np.array(status)
    np.savez_compressed(OUT, **store)
    print(f"{OUT}: {len(accepted)} accepted + {len(refused)} refused cases, {os.path.getsize(OUT)} bytes "
          f"(Pillow {PIL.__version__}, libjpeg-turbo {features.version('libjpeg_turbo')})")
    if os.path.getsize(OUT) > 300 * 1024:
        raise SystemExit("fixture above 300 KB")


if __name__ == "__main__":
    main()
