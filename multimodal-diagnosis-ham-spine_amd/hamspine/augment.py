"""Device-side image augmentation: the loaders' PIL transforms as HIP kernels (csrc/augment.hip).

The reference's `DataLoader` workers run RandomResizedCrop, flips, RandomRotation and ColorJitter (train) or Resize +
CenterCrop (eval) per image in PIL, then ToTensor + Normalize.  Here the workers only decode (or, with
`hamspine.jpeg`, run only the Huffman stage of the decode and leave the rest to `jpeg.decode_pack`): a collate function packs the
raw `uint8` HWC images of whatever size into one byte arena (`pack_images`), `BatchStager` moves the pack to the device, and
`TrainTransform` / `EvalTransform` turn it into the `(N, 3, S, S)` f32 batch on the current stream.  The kernels restate
Pillow's arithmetic exactly (tests/augment_ref.py is the numpy form, pinned against Pillow by tests/gen_augment_golden.py), so
for the same parameters the batch equals what torchvision's PIL backend gives, bit for bit.

The random parameters are drawn on the host (`sample_train_params`) with torchvision's algorithms in torchvision's draw
order.  Equality with torchvision's RNG stream is NOT claimed: torchvision is not available where this project is built, so
nothing pins it.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import rt
from .staging import IMAGENET_MEAN, IMAGENET_STD

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
# columns of the per-output tables of the C ABI (include/hamspine.h: hs_augment_plan)
IP_SRC, IP_TOP, IP_LEFT, IP_H, IP_W, IP_HFLIP, IP_VFLIP, IP_ROTATE, IP_ORDER, IP_ENABLE, IP_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 16
FP_ANGLE, FP_BRIGHTNESS, FP_CONTRAST, FP_SATURATION, FP_HUE, FP_COUNT = 0, 1, 2, 3, 4, 5


# ------------------------------------------------------------------------------------------------------------------ pack
def _as_hwc_u8(img):
    a = img.numpy() if torch.is_tensor(img) else np.asarray(img)       # a PIL image exposes the array interface
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise TypeError(f"pack_images: expected decoded H x W x 3 uint8 images, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def pack_images(images, pin=True):
    """Pack a list of H x W x 3 `uint8` images (arrays, tensors or PIL images, any sizes) for the device.

    Returns a dict of tensors -- `arena` (all bytes, image after image, tightly packed), `offsets` (int64), `heights`,
    `widths` (int32) -- plus `shapes`, the same sizes as a tuple of (h, w): `BatchStager` moves the tensors and passes the
    tuple through, so the transforms plan from the tuple and never read the device back.  One memcpy per image into the
    (pinned) arena, as staging._host_copy does."""
    arrs = [_as_hwc_u8(i) for i in images]
    if not arrs:
        raise ValueError("pack_images: no images")
    sizes = np.array([a.size for a in arrs], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    arena = torch.empty(int(sizes.sum()), dtype=torch.uint8, pin_memory=bool(pin))
    dst = arena.numpy()
    for a, o in zip(arrs, offsets):
        np.copyto(dst[o:o + a.size], a.reshape(-1))
    return {"arena": arena, "offsets": torch.from_numpy(offsets),
            "heights": torch.tensor([a.shape[0] for a in arrs], dtype=torch.int32),
            "widths": torch.tensor([a.shape[1] for a in arrs], dtype=torch.int32),
            "shapes": tuple((int(a.shape[0]), int(a.shape[1])) for a in arrs)}


def _pack_tables(pack):
    """host int32 heights / widths and int64 offsets of a pack (from `shapes` when it is there: no device read-back)"""
    if pack.get("shapes") is not None:
        h = np.array([s[0] for s in pack["shapes"]], dtype=np.int32)
        w = np.array([s[1] for s in pack["shapes"]], dtype=np.int32)
        n = h.astype(np.int64) * w * 3
        off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    else:
        h = pack["heights"].cpu().numpy().astype(np.int32)
        w = pack["widths"].cpu().numpy().astype(np.int32)
        off = pack["offsets"].cpu().numpy().astype(np.int64)
    return np.ascontiguousarray(h), np.ascontiguousarray(w), np.ascontiguousarray(off)


# ------------------------------------------------------------------------------------------------------------ parameters
def _uniform(g, lo, hi):
    return float(torch.empty(1).uniform_(float(lo), float(hi), generator=g).item())


def _randint(g, lo, hi):
    return int(torch.randint(lo, hi, (1,), generator=g).item())


def _crop_box(g, height, width, scale, ratio):
    """torchvision RandomResizedCrop.get_params: (top, left, h, w)"""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target = area * _uniform(g, scale[0], scale[1])
        aspect = math.exp(_uniform(g, log_ratio[0], log_ratio[1]))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= width and 0 < h <= height:
            top = _randint(g, 0, height - h + 1)
            left = _randint(g, 0, width - w + 1)
            return top, left, h, w
    in_ratio = float(width) / float(height)                      # fallback: the centre crop with the nearest allowed ratio
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def _jitter_range(v, center=1.0, clip0=True):
    if v is None:
        return None
    if isinstance(v, (tuple, list)):
        return float(v[0]), float(v[1])
    lo, hi = center - float(v), center + float(v)
    return (max(lo, 0.0) if clip0 else lo), hi


def sample_train_params(heights, widths, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), hflip=0.5, vflip=None, degrees=None,
                        brightness=None, contrast=None, saturation=None, hue=None, views=1, generator=None):
    """Draw one parameter set per output (`views` outputs per source, source-major) on the host.

    Per output, in torchvision's draw order: RandomResizedCrop (ten tries of area * U(scale) with a log-uniform ratio,
    `round(sqrt(...))`, `randint` corners, then the ratio-clamped centre fallback), `rand < p` for each flip that exists,
    U(-degrees, degrees), then ColorJitter's `randperm(4)` and its factors.  A stage whose argument is None does not exist
    and draws nothing.  Returns {"iparams": int32 (N, 16), "fparams": float64 (N, 5)} in the C ABI's layout.

    The algorithms are torchvision's; bitwise equality with torchvision's own RNG stream is not claimed (torchvision is not
    installed where this is built and tested)."""
    g = generator
    if degrees is not None and not isinstance(degrees, (tuple, list)):
        degrees = (-float(degrees), float(degrees))
    ranges = [_jitter_range(brightness), _jitter_range(contrast), _jitter_range(saturation), _jitter_range(hue, 0.0, False)]
    jitter = any(r is not None for r in ranges)
    n_src = len(heights)
    ip = np.zeros((n_src * views, IP_COUNT), dtype=np.int32)
    fp = np.zeros((n_src * views, FP_COUNT), dtype=np.float64)
    fp[:, FP_BRIGHTNESS:FP_HUE] = 1.0
    ip[:, IP_ORDER:IP_ORDER + 4] = np.arange(4)
    for n in range(n_src * views):
        s = n // views
        ip[n, IP_SRC] = s
        ip[n, IP_TOP:IP_W + 1] = _crop_box(g, int(heights[s]), int(widths[s]), scale, ratio)
        if hflip is not None:
            ip[n, IP_HFLIP] = int(torch.rand(1, generator=g).item() < hflip)
        if vflip is not None:
            ip[n, IP_VFLIP] = int(torch.rand(1, generator=g).item() < vflip)
        if degrees is not None:
            ip[n, IP_ROTATE] = 1
            fp[n, FP_ANGLE] = _uniform(g, degrees[0], degrees[1])
        if jitter:
            ip[n, IP_ORDER:IP_ORDER + 4] = torch.randperm(4, generator=g).numpy()
            for op, r in enumerate(ranges):
                if r is not None:
                    ip[n, IP_ENABLE + op] = 1
                    fp[n, FP_BRIGHTNESS + op] = _uniform(g, r[0], r[1])
    return {"iparams": ip, "fparams": fp}


def eval_geometry(h, w, resize=256, crop=224):
    """(out_h, out_w, off_y, off_x) of Resize(resize) + CenterCrop(crop): shorter side to `resize`, longer to
    int(resize * long / short), crop window at int(round((len - crop) / 2.0)) (Python's round: half to even)"""
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    return oh, ow, int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))


def eval_params(heights, widths, resize=256, crop=224, views=1):
    """{"src": int32 (N,) source of each output, "geometry": int32 (N, 4) of eval_geometry} for the eval / predict loaders.
    The eval plan takes `src`; it derives the geometry itself (hs_augment_plan_eval), `geometry` is there to inspect it."""
    if crop < 1 or resize < crop:
        raise ValueError(f"eval_params: resize {resize} must be at least crop {crop} >= 1")
    src = np.repeat(np.arange(len(heights), dtype=np.int32), views)
    geo = np.array([eval_geometry(int(heights[s]), int(widths[s]), resize, crop) for s in src], dtype=np.int32).reshape(-1, 4)
    return {"src": src, "geometry": geo}


# ------------------------------------------------------------------------------------------------------------ the passes
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(pack, N, S, mean, std, ws_bytes, plan, stats, stages):
    arena = pack["arena"]
    rt.need_gpu(arena)
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise TypeError("augment: the pack's arena is a flat contiguous uint8 tensor")
    if ws_bytes < 0:
        raise L.HamspineError("augment: bad arguments (sizes, output size or parameter table)")
    lib = L.lib()
    ws = rt.workspace(ws_bytes, arena.device)
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device=arena.device)
    st = rt.stream()
    plan(lib, rt.p(ws), ws_bytes, st)
    L.check(lib.hs_augment_resize(rt.p(arena), rt.p(ws), N, S, st), "hs_augment_resize")
    if stats:
        L.check(lib.hs_augment_stats(rt.p(ws), N, S, st), "hs_augment_stats")
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    L.check(lib.hs_augment_finish(rt.p(ws), rt.p(out), N, S, m, s, st), "hs_augment_finish")
    if not stages:
        return out
    o_sum, o_img = lib.hs_augment_ws_offset(0, N, S), lib.hs_augment_ws_offset(1, N, S)
    return {"out": out, "resized": ws[o_img:o_img + N * S * S * 3].view(N, S, S, 3).clone(),
            "lsum": ws[o_sum:o_sum + N * 8].view(torch.int64).clone()}


def augment_train(pack, params, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, stages=False):
    """Run plan, resize, stats and finish for explicit `params` (of sample_train_params) on a staged pack: (N, 3, size, size)
    f32 on the pack's device, on the current stream.  stages=True returns {"out", "resized" (N, S, S, 3) uint8, "lsum" (N,)
    int64: the sum of L each contrast op saw, 0 where there is none} for the tests."""
    h, w, off = _pack_tables(pack)
    ip = np.ascontiguousarray(params["iparams"], dtype=np.int32)
    fp = np.ascontiguousarray(params["fparams"], dtype=np.float64)
    if ip.ndim != 2 or ip.shape[1] != IP_COUNT or fp.shape != (ip.shape[0], FP_COUNT):
        raise ValueError("augment_train: iparams is (N, 16) int32 and fparams (N, 5) float64")
    N, S = ip.shape[0], int(size)
    nbytes = pack["arena"].numel()

    def plan(lib, ws, ws_bytes, st):
        L.check(lib.hs_augment_plan(_ptr(h), _ptr(w), _ptr(off), len(h), nbytes, _ptr(ip), _ptr(fp), N, S, ws, ws_bytes, st),
                "hs_augment_plan")

    ws_bytes = L.lib().hs_augment_ws_bytes(_ptr(ip), N, S) if N >= 1 else -1
    return _run(pack, N, S, mean, std, ws_bytes, plan, bool(ip[:, IP_ENABLE + CONTRAST].any()), stages)


def augment_eval(pack, resize=256, crop=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, views=1, stages=False):
    """Resize(resize) + CenterCrop(crop) + ToTensor + Normalize of every source of a staged pack, `views` copies each"""
    h, w, off = _pack_tables(pack)
    src = np.ascontiguousarray(eval_params(h, w, resize, crop, views)["src"])
    N, R, S = len(src), int(resize), int(crop)
    nbytes = pack["arena"].numel()

    def plan(lib, ws, ws_bytes, st):
        L.check(lib.hs_augment_plan_eval(_ptr(h), _ptr(w), _ptr(off), len(h), nbytes, _ptr(src), N, R, S, ws, ws_bytes, st),
                "hs_augment_plan_eval")

    ws_bytes = L.lib().hs_augment_eval_ws_bytes(_ptr(h), _ptr(w), len(h), _ptr(src), N, R, S) if N >= 1 else -1
    return _run(pack, N, S, mean, std, ws_bytes, plan, False, stages)


def _views(out, views):
    return out if views == 1 else out.view(out.shape[0] // views, views, *out.shape[1:])


class TrainTransform:
    """Callable from a staged pack to the f32 training batch: draws the parameters, then runs the kernels.

    The keyword arguments are sample_train_params's; `views` outputs per source give (B, views, 3, S, S) for the
    multi-view and sequence loaders.  `baseline()`, `mibf()` and `connext()` are the reference loaders' settings."""

    def __init__(self, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, views=1, generator=None, **sampling):
        self.size, self.mean, self.std, self.views, self.generator = int(size), tuple(mean), tuple(std), int(views), generator
        self.sampling = sampling
        sample_train_params([1], [1], views=1, generator=torch.Generator().manual_seed(0), **sampling)   # refuses bad keywords now

    @classmethod
    def baseline(cls, **kw):
        """data_loader.py's train transform: crop scale (0.2, 1), both flips, 45 degrees, ColorJitter(0.2, 0.2, 0.2, 0.1)"""
        return cls(scale=(0.2, 1.0), hflip=0.5, vflip=0.5, degrees=45, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, **kw)

    @classmethod
    def mibf(cls, **kw):
        """mibf_net/dataset_spine.py: default crop scale, horizontal flip, 15 degrees, ToTensor without Normalize"""
        return cls(hflip=0.5, degrees=15, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), **kw)

    @classmethod
    def connext(cls, **kw):
        """the ConNeXT loader: crop plus horizontal flip"""
        return cls(hflip=0.5, **kw)

    def sample(self, pack):
        h, w, _ = _pack_tables(pack)
        return sample_train_params(h, w, views=self.views, generator=self.generator, **self.sampling)

    def __call__(self, pack, params=None):
        params = self.sample(pack) if params is None else params
        return _views(augment_train(pack, params, self.size, self.mean, self.std), self.views)


class EvalTransform:
    """Callable from a staged pack to the f32 eval batch: Resize(resize) + CenterCrop(crop) + ToTensor + Normalize"""

    def __init__(self, resize=256, crop=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, views=1):
        if crop < 1 or resize < crop:
            raise ValueError(f"EvalTransform: resize {resize} must be at least crop {crop} >= 1")
        self.resize, self.crop, self.mean, self.std, self.views = int(resize), int(crop), tuple(mean), tuple(std), int(views)

    def __call__(self, pack):
        return _views(augment_eval(pack, self.resize, self.crop, self.mean, self.std, self.views), self.views)
