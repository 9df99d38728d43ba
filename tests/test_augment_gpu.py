"""Device-side augmentation on the MI355X (csrc/augment.hip) against the numpy restatement of Pillow's arithmetic
(tests/augment_ref.py, itself pinned to Pillow by tests/test_augment_cpu.py): every kernel output byte for byte, the final
f32 bit for bit.  One pack mixes sources of 1x1 .. 450x600, so source offsets are odd and even.
Pillow is not imported here."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import augment_ref as R
import hamspine._lib as L
from hamspine import augment as A
from hamspine import rt, staging

pytestmark = pytest.mark.gpu

MEAN, STD = staging.IMAGENET_MEAN, staging.IMAGENET_STD
SIZES = [(1, 1), (5, 7), (37, 29), (45, 61), (224, 224), (450, 600), (9, 11), (11, 9), (7, 7), (3, 4000), (4000, 2)]
ANGLES = [45.0, -45.0, 13.7, 0.0, 360.0, -15.3, 31.0]


def _sources():
    srcs = [R.smooth_image(h, w, 100 + i) for i, (h, w) in enumerate(SIZES)]
    srcs[2] = np.random.default_rng(1).integers(0, 256, (37, 29, 3), dtype=np.uint8)      # noise next to the smooth images
    srcs[6][:], srcs[7][:], srcs[8][:] = 0, 255, 128                                       # black, white, gray: RGB->HSV zero guards
    return srcs


def _box(rng, H, W, whole):
    if whole:
        return 0, 0, H, W
    h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
    return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w


def _params_s24():
    """40 outputs: all 24 colour orders with every op on, factors at both ends of (0.8, 1.2), hue +0.1 / -0.1 / 0, every flip
    combination under a rotation, sources shared between outputs; then 16 with ops off, no rotation stage, inner factors"""
    rng = np.random.default_rng(5)
    orders = list(itertools.permutations(range(4)))
    ip, fp = [], []
    for n in range(40):
        s = n % len(SIZES)
        H, W = SIZES[s]
        first = n < 24
        order = orders[n] if first else orders[int(rng.integers(0, 24))]
        enable = [1, 1, 1, 1] if first else [int(v) for v in rng.integers(0, 2, 4)]
        rotate = 1 if first else n % 2
        ends = lambda k: 0.8 if (n >> k) & 1 else 1.2
        fac = [ends(0), ends(1), ends(2)] if first else list(rng.uniform(0.8, 1.2, 3))
        hue = [0.1, -0.1, 0.0][n % 3] if first else float(rng.uniform(-0.1, 0.1))
        ip.append([s, *_box(rng, H, W, n % 7 == 3 or max(H, W) == 4000), n & 1, (n >> 1) & 1, rotate, *order, *enable])
        fp.append([ANGLES[n % len(ANGLES)], *fac, hue])
    return {"iparams": np.array(ip, dtype=np.int32), "fparams": np.array(fp, dtype=np.float64)}


def _params_s224():
    """S = 224: the 224 x 224 source whole (scale 1), a 450 x 600 crop (about 3 taps a side), an upscaled 45 x 61, the 1 x 1,
    and 4000-pixel sides: 37 taps per output, whose 224 x 39 ints per axis exceed what the resize kernels stage in LDS (at
    S = 24 the same sides give 335 taps that still fit: _params_s24 reaches them through its source cycle)"""
    ip = [[4, 0, 0, 224, 224, 1, 0, 1, 3, 1, 0, 2, 1, 1, 1, 1], [5, 20, 30, 400, 520, 0, 1, 1, 1, 3, 2, 0, 1, 1, 1, 1],
          [3, 2, 3, 40, 50, 1, 1, 0, 0, 1, 2, 3, 1, 1, 0, 1], [0, 0, 0, 1, 1, 0, 0, 1, 2, 0, 3, 1, 0, 1, 1, 1],
          [5, 0, 0, 450, 600, 0, 0, 0, 0, 1, 2, 3, 0, 0, 0, 0], [9, 0, 0, 3, 4000, 0, 0, 0, 0, 1, 2, 3, 0, 1, 0, 0],
          [10, 0, 0, 4000, 2, 1, 0, 1, 0, 1, 2, 3, 0, 0, 1, 0]]
    fp = [[45.0, 1.2, 0.8, 1.2, 0.1], [-13.7, 0.8, 1.2, 0.8, -0.1], [0.0, 1.1, 0.9, 1.0, 0.0], [30.0, 1.0, 1.2, 0.8, 0.05],
          [0.0, 1.0, 1.0, 1.0, 0.0], [0.0, 1.0, 1.1, 1.0, 0.0], [5.0, 1.0, 1.0, 0.9, 0.0]]
    return {"iparams": np.array(ip, dtype=np.int32), "fparams": np.array(fp, dtype=np.float64)}


def _reference(srcs, params, S):
    rows = [R.row_params(r, f, S) for r, f in zip(params["iparams"], params["fparams"])]
    src = [srcs[r[0]] for r in params["iparams"]]
    resized = np.stack([R.crop_resize(s, p["top"], p["left"], p["h"], p["w"], S) for s, p in zip(src, rows)])
    lsum = np.array([R.contrast_l_sum(s, p) for s, p in zip(src, rows)], dtype=np.int64)
    final = np.stack([R.train_u8(s, p) for s, p in zip(src, rows)])
    return {"resized": resized, "lsum": lsum, "u8": final, "out": np.stack([R.normalize(u, MEAN, STD) for u in final])}


@pytest.fixture(scope="module")
def world():
    """sources, their pack on the device, the parameter sets and the restatement's results: computed once, read only"""
    srcs = _sources()
    host = A.pack_images(srcs, pin=False)
    assert [int(o) % 2 for o in host["offsets"][1:4]] == [1, 0, 1] and int(host["offsets"][1]) == 3
    pack = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}
    p24, p224 = _params_s24(), _params_s224()
    return {"srcs": srcs, "pack": pack, "p24": p24, "p224": p224, "ref24": _reference(srcs, p24, 24),
            "ref224": _reference(srcs, p224, 224)}


def _same_bits(t, ref):
    return np.array_equal(t.cpu().numpy().view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("S", [24, 224])
def test_every_pass_equals_the_restatement(world, S):
    params, ref = world[f"p{S}"], world[f"ref{S}"]
    got = A.augment_train(world["pack"], params, size=S, stages=True)
    torch.cuda.synchronize()
    resized = got["resized"].cpu().numpy()
    bad = [n for n in range(len(resized)) if not np.array_equal(resized[n], ref["resized"][n])]
    assert not bad, f"resize differs for outputs {bad}"
    has_contrast = params["iparams"][:, A.IP_ENABLE + A.CONTRAST] == 1
    assert np.array_equal(got["lsum"].cpu().numpy()[has_contrast], ref["lsum"][has_contrast])
    out = got["out"]
    assert out.shape == (len(resized), 3, S, S) and out.dtype == torch.float32 and out.is_contiguous()
    bad = [n for n in range(len(resized)) if not _same_bits(out[n], ref["out"][n])]
    assert not bad, f"final batch differs for outputs {bad}"


def test_final_f32_is_the_staging_kernels_normalize_of_the_u8_image(world):
    """(u8 / 255 - mean) / std with the same kernel the stager uses, and MIBF-Net's mean 0 / std 1"""
    u8 = torch.from_numpy(world["ref24"]["u8"]).cuda()
    out = A.augment_train(world["pack"], world["p24"], size=24)
    assert torch.equal(out, staging.normalize_u8(u8, MEAN, STD))
    plain = A.augment_train(world["pack"], world["p24"], size=24, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    assert torch.equal(plain, staging.normalize_u8(u8, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))


def test_running_twice_gives_identical_bytes(world):
    a = A.augment_train(world["pack"], world["p24"], size=24, stages=True)
    b = A.augment_train(world["pack"], world["p24"], size=24, stages=True)
    for k in ("out", "resized", "lsum"):
        assert torch.equal(a[k], b[k]), k


def test_eval_plan_on_the_same_pack(world):
    srcs = world["srcs"]
    got = A.augment_eval(world["pack"], resize=32, crop=24, views=2, stages=True)
    ref = np.stack([R.eval_resize(s, 32, 24) for s in srcs])
    assert np.array_equal(got["resized"].cpu().numpy(), np.repeat(ref, 2, axis=0))
    assert all(_same_bits(got["out"][2 * i], R.normalize(ref[i], MEAN, STD)) for i in range(len(srcs)))
    full = A.EvalTransform()(world["pack"])                      # Resize(256) + CenterCrop(224), odd and even differences
    assert full.shape == (len(srcs), 3, 224, 224)
    for i in (0, 3, 5):
        assert _same_bits(full[i], R.normalize(R.eval_resize(srcs[i]), MEAN, STD)), i
    assert A.EvalTransform(32, 24, views=2)(world["pack"]).shape == (len(srcs), 2, 3, 24, 24)


class _Decoded(torch.utils.data.Dataset):
    """decoded uint8 images of differing sizes, as a worker would hand them over"""

    def __len__(self):
        return 6

    def __getitem__(self, i):
        return R.smooth_image(40 + 7 * i, 65 - 5 * i, i), i % 3


def _collate(items):
    return {**A.pack_images([img for img, _ in items]), "label": torch.tensor([y for _, y in items])}


def test_dataloader_collate_stager_transform(world):
    loader = torch.utils.data.DataLoader(_Decoded(), batch_size=3, num_workers=0, collate_fn=_collate)
    t = A.TrainTransform.baseline(generator=torch.Generator().manual_seed(0))
    seen = 0
    for batch in staging.BatchStager(loader, device="cuda"):
        assert batch["arena"].is_cuda and batch["label"].is_cuda and isinstance(batch["shapes"], tuple)
        params = t.sample(batch)
        x = t(batch, params)
        assert x.shape == (3, 3, 224, 224) and x.dtype == torch.float32 and x.is_cuda and bool(torch.isfinite(x).all())
        if seen == 0:
            img = _Decoded()[0][0]
            ref = R.normalize(R.train_u8(img, R.row_params(params["iparams"][0], params["fparams"][0], 224)), MEAN, STD)
            assert _same_bits(x[0], ref)
        seen += 1
    assert seen == 2
    views = A.TrainTransform.mibf(size=24, views=2, generator=torch.Generator().manual_seed(1))
    batch = next(iter(staging.BatchStager(loader, device="cuda")))
    assert views(batch).shape == (3, 2, 3, 24, 24)


def test_refusals_return_a_status_before_any_launch(world):
    lib, pack = L.lib(), world["pack"]
    h, w, off = A._pack_tables(pack)
    nbytes = pack["arena"].numel()
    good = {k: v[:2].copy() for k, v in world["p24"].items()}
    ws_bytes = lib.hs_augment_ws_bytes(A._ptr(good["iparams"]), 2, 24)
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3, 24, 24), 7.0, device="cuda")

    def plan(ip=good["iparams"], fp=good["fparams"], N=2, S=24, nb=nbytes, wsb=ws_bytes, n_src=len(h)):
        ip, fp = np.ascontiguousarray(ip, dtype=np.int32), np.ascontiguousarray(fp, dtype=np.float64)
        return lib.hs_augment_plan(A._ptr(h), A._ptr(w), A._ptr(off), n_src, nb, A._ptr(ip), A._ptr(fp), N, S, rt.p(ws), wsb, rt.stream())

    def edited(col, value, table="iparams"):
        t = {k: v.copy() for k, v in good.items()}
        t[table][1, col] = value
        return t["iparams"], t["fparams"]

    H, W = SIZES[good["iparams"][1, A.IP_SRC]]
    bad_calls = {
        "box below the image": lambda: plan(*edited(A.IP_TOP, H)),
        "box right of the image": lambda: plan(*edited(A.IP_W, W + 1)),
        "empty box": lambda: plan(*edited(A.IP_H, 0)),
        "negative corner": lambda: plan(*edited(A.IP_LEFT, -1)),
        "S < 1": lambda: plan(S=0),
        "order not a permutation": lambda: plan(*edited(A.IP_ORDER, int(good["iparams"][1, A.IP_ORDER + 1]))),
        "order out of range": lambda: plan(*edited(A.IP_ORDER + 2, 4)),
        "flag not 0 / 1": lambda: plan(*edited(A.IP_HFLIP, 2)),
        "source index": lambda: plan(*edited(A.IP_SRC, len(h))),
        "negative factor": lambda: plan(*edited(A.FP_CONTRAST, -0.5, "fparams")),
        "hue out of range": lambda: plan(*edited(A.FP_HUE, 0.6, "fparams")),
        "arena too small": lambda: plan(nb=nbytes - 1),
        "workspace too small": lambda: plan(wsb=ws_bytes - 16),
        "no outputs": lambda: plan(N=0),
        "eval R < S": lambda: lib.hs_augment_plan_eval(A._ptr(h), A._ptr(w), A._ptr(off), len(h), nbytes,
                                                       A._ptr(np.zeros(2, np.int32)), 2, 20, 24, rt.p(ws), ws_bytes, rt.stream()),
        "std == 0": lambda: lib.hs_augment_finish(rt.p(ws), rt.p(out), 2, 24, (C.c_float * 3)(*MEAN), (C.c_float * 3)(0.2, 0.0, 0.2),
                                                  rt.stream()),
        "resize S < 1": lambda: lib.hs_augment_resize(rt.p(pack["arena"]), rt.p(ws), 2, 0, rt.stream()),
        "stats N < 1": lambda: lib.hs_augment_stats(rt.p(ws), 0, 24, rt.stream()),
    }
    for what, call in bad_calls.items():
        assert call() == L._header.constants["HS_ERR_ARG"], what
        assert lib.hs_last_error(), what
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((out == 7.0).all())          # nothing ran
    with pytest.raises(L.HamspineError, match="crop box"):
        A.augment_train(pack, dict(zip(("iparams", "fparams"), edited(A.IP_TOP, H))), size=24)
    with pytest.raises(L.HamspineError):
        A.augment_train({**pack, "arena": pack["arena"].cpu()}, good, size=24)
    assert plan() == 0                                                      # and the good call is accepted
    torch.cuda.synchronize()
