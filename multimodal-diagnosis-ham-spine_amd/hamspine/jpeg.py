"""JPEG decode split between the loaders' workers and the device (csrc/jpeg_host.h, csrc/jpeg.hip).

The reference's datasets return `Image.open(path).convert("RGB")`; the decode runs on the DataLoader workers' cores.  Only its
Huffman stage is serial.  Here a worker runs that stage alone (`entropy_decode`: file bytes -> quantised DCT coefficients, a plain
host function that never touches the GPU), the collate function packs the coefficients of a batch (`pack_jpegs`), `BatchStager`
moves the pack, and `decode_pack` runs dequantisation, the inverse DCT, chroma upsampling, YCbCr -> RGB and the copy into the
byte arena as two kernels for the whole batch.  The result is exactly what `augment.pack_images` of the Pillow-decoded images
gives, on the device: `TrainTransform` / `EvalTransform` take it unchanged.

The arithmetic is libjpeg's default path (tests/jpeg_ref.py restates it; tests/gen_jpeg_golden.py pins it against Pillow), so the
pixels equal Pillow's bit for bit.  What the host stage does not take (progressive, arithmetic coding, 12-bit, 16-bit tables, 4
components, unusual sampling, several scans, Adobe-marked files, width <= 4 with subsampled chroma, frames of 3 * h * w >= 2^31
bytes) it refuses with a status of its own; `entropy_decode` then decodes that file with Pillow in the worker (fallback="pillow") or raises (fallback="raise").  A
corrupt file always raises.
"""
import ctypes as C
import io

import numpy as np
import torch

from . import _lib as L
from . import rt

GEOM = L.JPEG_GEOM


class JpegRefused(L.HamspineError):
    """the file is a kind of JPEG the host stage does not decode; `.status` is the HS_JPEG_ERR_* value"""

    def __init__(self, status, text):
        super().__init__(text)
        self.status = status


def _status_text(status):
    return L.lib().hs_jpeg_status_text(status).decode("utf-8", "replace")


def probe(data):
    """the geometry of a JPEG file as a dict (see hs_jpeg_info), without decoding it; raises as entropy_decode(fallback="raise")"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = L.JpegInfo()
    st = L.lib().hs_jpeg_probe(buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(info))
    _raise_for(st)
    return _info_dict(info)


def _info_dict(info):
    n = info.components
    return {"height": info.height, "width": info.width, "components": n, "h_samp": tuple(info.h_samp[:n]),
            "v_samp": tuple(info.v_samp[:n]), "block_rows": tuple(info.block_rows[:n]), "block_cols": tuple(info.block_cols[:n]),
            "restart_interval": info.restart_interval, "coef_bytes": info.coef_bytes}


def _raise_for(st):
    if st == L.HS_OK:
        return
    if st in L.JPEG_STATUS and L.JPEG_STATUS[st] != "CORRUPT":
        raise JpegRefused(st, _status_text(st))
    raise L.HamspineError(f"jpeg: status {st}: {_status_text(st)}")


def entropy_decode(data, fallback="pillow"):
    """The worker-side half: file bytes -> a small picklable record of numpy arrays.  Makes no GPU call.

    {"coef": int16, per component [block_rows][block_cols][64] in natural order one after another, "qtab": uint16 (3, 64),
     "geom": int32 (8,) = height, width, components, luma h_samp, luma v_samp, 0, 0, 0}
    A refused file gives {"pixels": H x W x 3 uint8} decoded by Pillow (fallback="pillow"; Pillow must import) or raises
    JpegRefused (fallback="raise").  A corrupt file raises HamspineError with the status text."""
    if fallback not in ("pillow", "raise"):
        raise ValueError("entropy_decode: fallback is 'pillow' or 'raise'")
    raw = bytes(data)
    buf = np.frombuffer(raw, dtype=np.uint8)
    lib = L.lib()
    info = L.JpegInfo()
    ptr = buf.ctypes.data_as(C.c_void_p)
    st = lib.hs_jpeg_probe(ptr, buf.size, C.byref(info))
    if st == L.HS_OK:
        coef = np.empty(info.coef_bytes // 2, dtype=np.int16)
        qtab = np.empty((L.JPEG_MAX_COMPONENTS, 64), dtype=np.uint16)
        st = lib.hs_jpeg_entropy_decode(ptr, buf.size, coef.ctypes.data_as(C.c_void_p), coef.nbytes, qtab.ctypes.data_as(C.c_void_p),
                                        C.byref(info))
        if st == L.HS_OK:
            geom = np.zeros(GEOM, dtype=np.int32)
            geom[:5] = (info.height, info.width, info.components, info.h_samp[0], info.v_samp[0])
            return {"coef": coef, "qtab": qtab, "geom": geom}
    if fallback == "pillow" and st in L.JPEG_STATUS and L.JPEG_STATUS[st] != "CORRUPT":
        from PIL import Image
        return {"pixels": np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(raw)).convert("RGB")))}
    _raise_for(st)


def _is_raw(rec):
    return "pixels" in rec


def pack_jpegs(records, pin=True):
    """Collate the records of entropy_decode (fallback records among them, in any order) for the device.

    Returns a dict of tensors -- `coef` (int16: every coefficient array, each at a 16-byte aligned offset), `qtab` (uint16
    (n_jpeg, 3, 64)), `raw` (uint8: the fallback images' pixels, tightly packed), and the `offsets` (int64), `heights`, `widths`
    (int32) of the decoded pack, which `decode_pack` hands on -- and tuples that `BatchStager` passes through:
    `shapes` ((h, w) per image, in order), `geoms`, `coef_offsets`, `coef_lens` (per coefficient record, in order), `raw_index`
    (positions of the fallback images).  `decode_pack` turns the staged dict into the pack `augment.pack_images` gives."""
    records = list(records)
    if not records:
        raise ValueError("pack_jpegs: no images")
    shapes, geoms, offs, lens, raw_index, at, raw_bytes = [], [], [], [], [], 0, 0
    for i, r in enumerate(records):
        if _is_raw(r):
            px = r["pixels"]
            if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 3:
                raise TypeError(f"pack_jpegs: a fallback record holds H x W x 3 uint8 pixels, got {px.dtype} {px.shape}")
            shapes.append((int(px.shape[0]), int(px.shape[1])))
            raw_index.append(i)
            raw_bytes += px.size
        else:
            g = np.asarray(r["geom"], dtype=np.int32)
            shapes.append((int(g[0]), int(g[1])))
            geoms.append(tuple(int(v) for v in g))
            offs.append(at)
            lens.append(int(r["coef"].nbytes))
            at = (at + r["coef"].nbytes + 15) & ~15
    n_jpeg = len(geoms)
    coef = torch.empty(max(at // 2, 8), dtype=torch.int16, pin_memory=bool(pin))
    qtab = torch.zeros((max(n_jpeg, 1), L.JPEG_MAX_COMPONENTS, 64), dtype=torch.int16, pin_memory=bool(pin))
    raw = torch.empty(max(raw_bytes, 1), dtype=torch.uint8, pin_memory=bool(pin))
    cdst, qdst, rdst = coef.numpy(), qtab.numpy().view(np.uint16), raw.numpy()
    j, rat = 0, 0
    for r in records:
        if _is_raw(r):
            n = r["pixels"].size
            np.copyto(rdst[rat:rat + n], np.ascontiguousarray(r["pixels"]).reshape(-1))
            rat += n
        else:
            end = offs[j] // 2 + r["coef"].size
            np.copyto(cdst[offs[j] // 2:end], r["coef"].reshape(-1))
            cdst[end:(offs[j + 1] // 2 if j + 1 < n_jpeg else cdst.size)] = 0      # the alignment gap (no kernel reads it)
            np.copyto(qdst[j], r["qtab"])
            j += 1
    if not n_jpeg:
        cdst[:] = 0
    sizes = np.array([3 * h * w for h, w in shapes], dtype=np.int64)
    tables = {"offsets": torch.empty(len(shapes), dtype=torch.int64, pin_memory=bool(pin)),
              "heights": torch.empty(len(shapes), dtype=torch.int32, pin_memory=bool(pin)),
              "widths": torch.empty(len(shapes), dtype=torch.int32, pin_memory=bool(pin))}
    np.copyto(tables["offsets"].numpy(), np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    np.copyto(tables["heights"].numpy(), [s[0] for s in shapes])
    np.copyto(tables["widths"].numpy(), [s[1] for s in shapes])
    return {"coef": coef, "qtab": qtab, "raw": raw, **tables, "shapes": tuple(shapes), "geoms": tuple(geoms), "coef_offsets": tuple(offs),
            "coef_lens": tuple(lens), "raw_index": tuple(raw_index)}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def decode_pack(pack):
    """The device half: a staged pack of pack_jpegs -> the pack `augment.pack_images` returns (`arena`, `offsets`, `heights`,
    `widths`, `shapes`), on the device, in the original image order.  Two kernels per 32 JPEG images on the current stream, one
    device-to-device `copy_` per fallback image, and no host-to-device copy at all, so nothing waits on the stream: `offsets`,
    `heights` and `widths` were made by pack_jpegs and staged with the pack; the kernels' tables travel in their arguments."""
    coef, qtab, raw = pack["coef"], pack["qtab"], pack["raw"]
    rt.need_gpu(coef, qtab, raw, pack["offsets"], pack["heights"], pack["widths"])
    if coef.dtype != torch.int16 or qtab.dtype != torch.int16 or raw.dtype != torch.uint8 or not (
            coef.is_contiguous() and qtab.is_contiguous() and raw.is_contiguous()):
        raise TypeError("decode_pack: coef and qtab are contiguous int16 tensors and raw a contiguous uint8 tensor")
    shapes = tuple(pack["shapes"])
    sizes = np.array([3 * h * w for h, w in shapes], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    dev = coef.device
    arena = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=dev)
    raw_index = set(pack["raw_index"])
    jpeg_index = [i for i in range(len(shapes)) if i not in raw_index]
    if len(jpeg_index) != len(pack["geoms"]) or pack["offsets"].numel() != len(shapes):
        raise ValueError("decode_pack: shapes, geoms, raw_index and offsets disagree")
    if jpeg_index:
        n = len(jpeg_index)
        geom = np.ascontiguousarray(np.array(pack["geoms"], dtype=np.int32).reshape(n, GEOM))
        coef_off = np.ascontiguousarray(np.array(pack["coef_offsets"], dtype=np.int64))
        coef_len = np.ascontiguousarray(np.array(pack["coef_lens"], dtype=np.int64))
        out_off = np.ascontiguousarray(offsets[jpeg_index])
        lib = L.lib()
        ws_bytes = lib.hs_jpeg_ws_bytes(_ptr(geom), n)
        if ws_bytes < 0:
            raise L.HamspineError("decode_pack: bad geometry table")
        ws = rt.workspace(ws_bytes, dev)
        L.check(lib.hs_jpeg_decode(rt.p(coef), coef.numel() * 2, rt.p(qtab), _ptr(geom), _ptr(coef_off), _ptr(coef_len), _ptr(out_off),
                                   n, rt.p(arena), arena.numel(), rt.p(ws), ws_bytes, rt.stream()), "hs_jpeg_decode")
    rat = 0
    for i in sorted(raw_index):
        n = int(sizes[i])
        arena[int(offsets[i]):int(offsets[i]) + n].copy_(raw[rat:rat + n])
        rat += n
    return {"arena": arena, "offsets": pack["offsets"], "heights": pack["heights"], "widths": pack["widths"], "shapes": shapes}
