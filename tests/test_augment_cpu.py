"""Device-side augmentation, the part that needs no GPU: the numpy restatement (tests/augment_ref.py) against what Pillow
gave when tests/gen_augment_golden.py recorded tests/golden/augment_*.npz, the host-side parameter sampling of
hamspine.augment, and the C ABI's declarations.  Pillow is not imported here."""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
import hamspine._lib as L
from hamspine import augment as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S = 24


@pytest.fixture(scope="module")
def stages():
    return dict(np.load(os.path.join(GOLDEN, "augment_stages.npz")))


@pytest.fixture(scope="module")
def chains():
    return dict(np.load(os.path.join(GOLDEN, "augment_chains.npz")))


def _differing_bytes(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    return int((a != b).sum())


def test_crop_resize_equals_pillow(stages):
    boxes = stages["resize_boxes"]
    assert len(boxes) == 14
    for (s, t, l, h, w), ref in zip(boxes, stages["resize_out"]):
        assert _differing_bytes(R.crop_resize(stages[f"src{s}"], t, l, h, w, S), ref) == 0, (s, t, l, h, w)
    # the cases the issue names are in the fixture: upscaling, a 1-pixel-wide box, a box touching each edge
    src_h = {i: stages[f"src{i}"].shape[0] for i in range(5)}
    src_w = {i: stages[f"src{i}"].shape[1] for i in range(5)}
    assert any(w == 1 for _, _, _, _, w in boxes) and any(h < S and w < S for _, _, _, h, w in boxes)
    assert any(t == 0 for _, t, _, _, _ in boxes) and any(l == 0 for _, _, l, _, _ in boxes)
    assert any(t + h == src_h[s] and t > 0 for s, t, _, h, _ in boxes) and any(l + w == src_w[s] and l > 0 for s, _, l, _, w in boxes)


def test_eval_resize_and_centre_crop_equal_pillow(stages):
    for (s, r), ref in zip(stages["eval_cases"], stages["eval_out"]):
        assert _differing_bytes(R.eval_resize(stages[f"src{s}"], int(r), S), ref) == 0, (s, r)


def test_flips_and_rotation_equal_pillow(stages):
    base, odd = stages["gather_base"], stages["gather_odd"]
    combos = [(hf, vf) for hf in (0, 1) for vf in (0, 1)]
    for (hf, vf), ref in zip(combos, stages["flip_out"]):
        assert _differing_bytes(R.gather(base, hf, vf, None), ref) == 0, (hf, vf)
    angles = list(stages["angles"])
    assert {45.0, -45.0, 0.0, 13.7, 360.0} <= set(angles)
    for a, ref, ref_odd in zip(angles, stages["rot_out"], stages["rot_odd_out"]):
        assert _differing_bytes(R.gather(base, 0, 0, float(a)), ref) == 0, a
        assert _differing_bytes(R.gather(odd, 0, 0, float(a)), ref_odd) == 0, a
    assert R.rotation_fixed(360.0, S, S) is None and R.rotation_fixed(0.0, S, S) is None and R.rotation_fixed(720.0, S, S) is None


def test_gray_brightness_contrast_saturation_equal_pillow(stages):
    factors = list(stages["factors"])
    assert factors == [0.8, 1.2, 0.93, 1.07]
    for i, img in enumerate(stages["colour_src"]):
        assert _differing_bytes(R.gray(img), stages["gray_out"][i]) == 0
        for j, f in enumerate(factors):
            assert _differing_bytes(R.brightness(img, f), stages["brightness_out"][i, j]) == 0, (i, f)
            assert _differing_bytes(R.contrast(img, f), stages["contrast_out"][i, j]) == 0, (i, f)
            assert _differing_bytes(R.saturation(img, f), stages["saturation_out"][i, j]) == 0, (i, f)


def _allowance(ref, got, max_diff, share):
    d = np.abs(ref.astype(np.int64) - got.astype(np.int64))
    assert int(d.max()) <= int(max_diff) and float((d != 0).any(-1).mean()) <= float(share)


def test_hue_within_the_recorded_allowance(stages):
    """the generator measured the restatement against Pillow: 0 differing bytes on the fixture images and over all 2^24
    colours (Pillow 12.2.0), so the allowance is 0"""
    assert int(stages["hue_max_diff"]) == 0 and float(stages["hue_share"]) == 0.0
    assert int(stages["hue_exhaustive_max_diff"]) == 0 and float(stages["hue_exhaustive_share"]) == 0.0
    got = np.stack([[R.hue(c, float(f)) for f in stages["hues"]] for c in stages["colour_src"]])
    _allowance(stages["hue_out"], got, stages["hue_max_diff"], stages["hue_share"])


def test_chains_within_the_recorded_allowance(chains):
    ip, fp = chains["iparams"], chains["fparams"]
    assert int(chains["chain_max_diff"]) == 0 and float(chains["chain_share"]) == 0.0
    got = np.stack([R.train_u8(chains[f"src{r[0]}"], R.row_params(r, f, S)) for r, f in zip(ip, fp)])
    _allowance(chains["out"], got, chains["chain_max_diff"], chains["chain_share"])
    assert ip[:, A.IP_ROTATE].min() == 0 and ip[:, A.IP_ENABLE:A.IP_ENABLE + 4].min() == 0      # copies and skipped ops occur


def test_normalize_is_the_staging_kernels_formula():
    img = np.arange(S * S * 3, dtype=np.int64).reshape(S, S, 3).astype(np.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    ref = (torch.from_numpy(img).permute(2, 0, 1).float() / 255.0 - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    assert np.array_equal(R.normalize(img, mean, std).view(np.int32), ref.numpy().view(np.int32))


# ----------------------------------------------------------------------------------------------------- parameter sampling
BASELINE = dict(scale=(0.2, 1.0), hflip=0.5, vflip=0.5, degrees=45, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1)


def test_sampling_is_deterministic_and_boxes_lie_inside():
    hs, ws = [450, 37, 5, 1, 224], [600, 29, 7, 1, 224]
    a = A.sample_train_params(hs, ws, views=3, generator=torch.Generator().manual_seed(7), **BASELINE)
    b = A.sample_train_params(hs, ws, views=3, generator=torch.Generator().manual_seed(7), **BASELINE)
    c = A.sample_train_params(hs, ws, views=3, generator=torch.Generator().manual_seed(8), **BASELINE)
    assert np.array_equal(a["iparams"], b["iparams"]) and np.array_equal(a["fparams"], b["fparams"])
    assert not np.array_equal(a["fparams"], c["fparams"])
    ip, fp = a["iparams"], a["fparams"]
    assert ip.shape == (15, 16) and ip.dtype == np.int32 and fp.shape == (15, 5) and fp.dtype == np.float64
    assert list(ip[:, A.IP_SRC]) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    for r in ip:
        H, W = hs[r[A.IP_SRC]], ws[r[A.IP_SRC]]
        assert r[A.IP_H] >= 1 and r[A.IP_W] >= 1 and r[A.IP_TOP] >= 0 and r[A.IP_LEFT] >= 0
        assert r[A.IP_TOP] + r[A.IP_H] <= H and r[A.IP_LEFT] + r[A.IP_W] <= W
        assert sorted(r[A.IP_ORDER:A.IP_ORDER + 4]) == [0, 1, 2, 3] and list(r[A.IP_ENABLE:A.IP_ENABLE + 4]) == [1, 1, 1, 1]
    assert (np.abs(fp[:, A.FP_ANGLE]) <= 45).all() and (fp[:, 1:4] >= 0.8).all() and (fp[:, 1:4] <= 1.2).all()
    assert (np.abs(fp[:, A.FP_HUE]) <= 0.1).all() and set(ip[:, A.IP_HFLIP]) | set(ip[:, A.IP_VFLIP]) <= {0, 1}


def test_stages_that_do_not_exist_draw_nothing():
    """the MIBF-Net loader (crop, hflip, 15 degrees) and the ConNeXT one (crop, hflip): no jitter, identity order"""
    g = torch.Generator().manual_seed(3)
    p = A.sample_train_params([45], [61], hflip=0.5, degrees=15, views=4, generator=g)
    assert (p["iparams"][:, A.IP_ENABLE:A.IP_ENABLE + 4] == 0).all() and (p["iparams"][:, A.IP_ROTATE] == 1).all()
    assert (p["iparams"][:, A.IP_VFLIP] == 0).all() and (np.abs(p["fparams"][:, A.FP_ANGLE]) <= 15).all()
    q = A.sample_train_params([45], [61], hflip=0.5, generator=torch.Generator().manual_seed(3))
    assert q["iparams"][0, A.IP_ROTATE] == 0 and list(q["iparams"][0, A.IP_ORDER:A.IP_ORDER + 4]) == [0, 1, 2, 3]
    for t in (A.TrainTransform.baseline(), A.TrainTransform.mibf(), A.TrainTransform.connext()):
        assert t.size == 224
    assert A.TrainTransform.mibf().std == (1.0, 1.0, 1.0) and A.TrainTransform.baseline().sampling["degrees"] == 45
    with pytest.raises(TypeError):
        A.TrainTransform(shear=3)


def test_crop_fallback_on_a_ratio_the_image_cannot_meet():
    """8 x 400 with the default scale (0.08, 1) and ratio (3/4, 4/3): every try asks for h >= sqrt(0.08 * 3200 / (4/3)) = 13.9
    rows of 8, so the ten tries fail; in_ratio 50 > 4/3 gives h = 8, w = int(round(8 * 4/3)) = 11, centred"""
    for seed in range(5):
        p = A.sample_train_params([8], [400], hflip=None, generator=torch.Generator().manual_seed(seed))
        assert list(p["iparams"][0, A.IP_TOP:A.IP_W + 1]) == [0, (400 - 11) // 2, 8, 11]
    p = A.sample_train_params([400], [8], hflip=None, generator=torch.Generator().manual_seed(0))
    assert list(p["iparams"][0, A.IP_TOP:A.IP_W + 1]) == [(400 - 11) // 2, 0, int(round(8 / 0.75)), 8]


def test_eval_geometry_rounds_half_to_even():
    assert A.eval_geometry(257, 300)[:3:2] == (256, 16) and A.eval_geometry(257, 300) == (256, 298, 16, 37)
    assert int(round((257 - 224) / 2.0)) == 16 and A.eval_geometry(450, 600) == (256, 341, 16, 58)     # 58.5 -> 58
    assert A.eval_geometry(600, 450, 259, 224) == (345, 259, 60, 18)                                  # 60.5 -> 60, 17.5 -> 18
    for h, w, r, c in ((37, 29, 32, 24), (450, 600, 256, 224), (5, 7, 24, 24), (301, 300, 257, 224)):
        assert A.eval_geometry(h, w, r, c) == R.eval_geometry(h, w, r, c)
    p = A.eval_params([450, 37], [600, 29], views=2)
    assert list(p["src"]) == [0, 0, 1, 1] and p["geometry"].shape == (4, 4) and list(p["geometry"][0]) == [256, 341, 16, 58]
    with pytest.raises(ValueError):
        A.eval_params([10], [10], resize=200, crop=224)


def test_pack_images_layout():
    imgs = [R.smooth_image(5, 7, 1), torch.from_numpy(R.smooth_image(1, 1, 2)), R.smooth_image(37, 29, 3)]
    pack = A.pack_images(imgs, pin=False)
    assert pack["arena"].dtype == torch.uint8 and pack["arena"].numel() == 105 + 3 + 37 * 29 * 3
    assert list(pack["offsets"]) == [0, 105, 108] and pack["offsets"].dtype == torch.int64
    assert list(pack["heights"]) == [5, 1, 37] and list(pack["widths"]) == [7, 1, 29] and pack["shapes"] == ((5, 7), (1, 1), (37, 29))
    assert np.array_equal(pack["arena"][108:].numpy().reshape(37, 29, 3), imgs[2])
    for bad in ([np.zeros((4, 4), np.uint8)], [np.zeros((4, 4, 3), np.float32)], [np.zeros((0, 4, 3), np.uint8)]):
        with pytest.raises(TypeError):
            A.pack_images(bad, pin=False)


# -------------------------------------------------------------------------------------------------------------- the C ABI
ENTRIES = ["hs_augment_ws_bytes", "hs_augment_eval_ws_bytes", "hs_augment_ws_offset", "hs_augment_plan", "hs_augment_plan_eval",
           "hs_augment_resize", "hs_augment_stats", "hs_augment_finish"]


def test_header_declares_and_library_exports_the_entries():
    lib = L.lib()
    assert set(ENTRIES) <= set(L.exported_symbols())
    for n in ENTRIES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None
    assert lib.hs_augment_ws_bytes.restype is L.C.c_int64 and lib.hs_augment_plan.restype is L.C.c_int32
    assert len(lib.hs_augment_plan.argtypes) == 12 and len(lib.hs_augment_finish.argtypes) == 7


def test_workspace_query_needs_no_device():
    lib = L.lib()
    p = A.sample_train_params([450, 5], [600, 7], generator=torch.Generator().manual_seed(1), **BASELINE)
    ip = np.ascontiguousarray(p["iparams"])
    small, big = lib.hs_augment_ws_bytes(A._ptr(ip), 2, 24), lib.hs_augment_ws_bytes(A._ptr(ip), 2, 224)
    assert 2 * 24 * 24 * 3 < small < big and big >= 2 * 224 * 224 * 3 + int(ip[0, A.IP_H]) * 224 * 3
    assert lib.hs_augment_ws_bytes(A._ptr(ip), 2, 0) == -1 and lib.hs_augment_ws_bytes(A._ptr(ip), 0, 24) == -1
    assert 0 < lib.hs_augment_ws_offset(0, 2, 24) < lib.hs_augment_ws_offset(1, 2, 24) < small
    h, w, src = (np.array(v, dtype=np.int32) for v in ([450, 5], [600, 7], [0, 1, 1]))
    assert lib.hs_augment_eval_ws_bytes(A._ptr(h), A._ptr(w), 2, A._ptr(src), 3, 256, 224) > 3 * 224 * 224 * 3
    assert lib.hs_augment_eval_ws_bytes(A._ptr(h), A._ptr(w), 2, A._ptr(src), 3, 200, 224) == -1          # R < S
