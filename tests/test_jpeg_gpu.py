"""JPEG decode on the MI355X (csrc/jpeg.hip) against Pillow's stored pixels (tests/golden/jpeg_cases.npz, written by
tests/gen_jpeg_golden.py): every byte of every image.  All accepted golden cases form one batch, so image starts in the output
arena have every alignment.  Pillow is not imported here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hamspine._lib as L
import jpeg_ref
from hamspine import augment as A
from hamspine import jpeg as J
from hamspine import rt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
ACCEPTED = [str(n) for n in GOLDEN["accepted"]]
GUARD = 64


def _stage(pack):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in pack.items()}


@pytest.fixture(scope="module")
def world():
    """the records of every accepted golden case (through the C entropy stage), their staged pack, Pillow's pixels: read only"""
    recs = [J.entropy_decode(GOLDEN[f"bytes/{n}"].tobytes(), fallback="raise") for n in ACCEPTED]
    pixels = [GOLDEN[f"pixels/{n}"] for n in ACCEPTED]
    host = J.pack_jpegs(recs, pin=False)
    return {"recs": recs, "pixels": pixels, "host": host, "pack": _stage(host)}


def _images(pack):
    arena = pack["arena"].cpu().numpy()
    off = pack["offsets"].cpu().numpy()
    return [arena[int(o):int(o) + 3 * h * w].reshape(h, w, 3) for o, (h, w) in zip(off, pack["shapes"])]


def _tables(host):
    n = len(host["geoms"])
    geom = np.ascontiguousarray(np.array(host["geoms"], dtype=np.int32).reshape(n, L.JPEG_GEOM))
    coef_off = np.array(host["coef_offsets"], dtype=np.int64)
    coef_len = np.array(host["coef_lens"], dtype=np.int64)
    sizes = np.array([3 * h * w for h, w in host["shapes"]], dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return geom, coef_off, coef_len, out_off, int(sizes.sum())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_batch_of_every_golden_case_equals_pillow_bit_for_bit(world):
    out = J.decode_pack(world["pack"])
    torch.cuda.synchronize()
    assert out["shapes"] == tuple(p.shape[:2] for p in world["pixels"])
    assert out["arena"].dtype == torch.uint8 and out["arena"].is_cuda and out["offsets"].dtype == torch.int64
    # the three tables are the tensors pack_jpegs made and the stager moved: decode_pack copies nothing from the host
    assert all(out[k] is world["pack"][k] and out[k].is_cuda for k in ("offsets", "heights", "widths"))
    assert out["heights"].dtype == out["widths"].dtype == torch.int32
    offs = out["offsets"].cpu().numpy()
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}, "the batch must start images at every byte alignment"
    assert np.array_equal(out["heights"].cpu().numpy(), [p.shape[0] for p in world["pixels"]])
    assert np.array_equal(out["widths"].cpu().numpy(), [p.shape[1] for p in world["pixels"]])
    bad = [n for n, got, want in zip(ACCEPTED, _images(out), world["pixels"]) if not np.array_equal(got, want)]
    assert not bad, f"decoded pixels differ from Pillow's for {bad}"
    again = J.decode_pack(world["pack"])
    torch.cuda.synchronize()
    assert torch.equal(again["arena"], out["arena"])


def test_guard_bytes_and_the_workspace_tail_stay_untouched(world):
    host, pack = world["host"], world["pack"]
    geom, coef_off, coef_len, out_off, total = _tables(host)
    lib = L.lib()
    ws_bytes = lib.hs_jpeg_ws_bytes(_ptr(geom), len(geom))
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    for shift in (0, 1, 3):                                    # the arena itself starts at three alignments
        buf = torch.full((GUARD + shift + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = torch.full((ws_bytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        st = lib.hs_jpeg_decode(rt.p(pack["coef"]), pack["coef"].numel() * 2, rt.p(pack["qtab"]), _ptr(geom), _ptr(coef_off),
                                _ptr(coef_len), _ptr(out_off), len(geom), rt.p(buf, GUARD + shift), total, rt.p(ws), ws_bytes,
                                rt.stream())
        L.check(st, "hs_jpeg_decode")
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD + shift] == 0xA5).all() and (got[GUARD + shift + total:] == 0xA5).all(), f"guard bytes written (shift {shift})"
        assert (ws[ws_bytes:].cpu().numpy() == 0x5A).all(), "the workspace tail was written"
        body = got[GUARD + shift:GUARD + shift + total]
        want = np.concatenate([p.reshape(-1) for p in world["pixels"]])
        assert np.array_equal(body, want), f"pixels differ at arena shift {shift}"


def test_hostile_coefficients_equal_the_restatement(world):
    """full-range random int16 coefficients and 16-bit table entries: every product and sum of the IDCT wraps in int32, half the
    samples saturate, and the kernels still equal the numpy form (int32 with wrap-around) on every byte"""
    rng = np.random.default_rng(5)
    recs, want = [], []
    for name in ACCEPTED:
        g = GOLDEN[f"geom/{name}"]
        nc = int(g[2])
        geo = {"height": int(g[0]), "width": int(g[1]), "components": nc, "h_samp": list(g[3:3 + nc]), "v_samp": list(g[6:6 + nc])}
        coefs = [rng.integers(-32768, 32768, (int(r), int(c), 64)).astype(np.int16) for r, c in zip(g[9:9 + nc], g[12:12 + nc])]
        qtab = rng.integers(0, 65536, (3, 64)).astype(np.uint16)
        geom = np.zeros(L.JPEG_GEOM, dtype=np.int32)
        geom[:5] = (g[0], g[1], nc, g[3], g[6])
        recs.append({"coef": np.concatenate([c.reshape(-1) for c in coefs]), "qtab": qtab, "geom": geom})
        want.append(jpeg_ref.pixels(coefs, qtab[:nc], geo))
    out = J.decode_pack(_stage(J.pack_jpegs(recs, pin=False)))
    torch.cuda.synchronize()
    bad = [n for n, got, ref in zip(ACCEPTED, _images(out), want) if not np.array_equal(got, ref)]
    assert not bad, f"kernels and restatement differ on random coefficients for {bad}"
    flat = np.concatenate([w.reshape(-1) for w in want])
    assert 0.2 < ((flat == 0) | (flat == 255)).mean() < 0.8


def test_a_raw_fallback_image_in_the_middle_keeps_order_and_bytes(world):
    """every case twice around one raw image: 52 JPEG records, so the batch also crosses the 32 images one launch pair takes"""
    raw = GOLDEN["pixels/9x4_420"]
    mid = len(world["recs"])
    recs = list(world["recs"]) + [{"pixels": raw}] + list(world["recs"])
    pixels = list(world["pixels"]) + [raw] + list(world["pixels"])
    assert len(recs) - 1 > L.JPEG_CHUNK
    host = J.pack_jpegs(recs, pin=False)
    assert host["raw_index"] == (mid,)
    out = J.decode_pack(_stage(host))
    torch.cuda.synchronize()
    assert out["shapes"] == tuple(p.shape[:2] for p in pixels)
    for i, (got, want) in enumerate(zip(_images(out), pixels)):
        assert np.array_equal(got, want), f"image {i} differs"


def test_transforms_take_the_decoded_pack_as_they_take_pack_images(world):
    out = J.decode_pack(world["pack"])
    ref = _stage(A.pack_images(world["pixels"], pin=False))
    ev = A.EvalTransform(resize=32, crop=24)
    assert torch.equal(ev(out), ev(ref))
    tt = A.TrainTransform.baseline(size=24, generator=torch.Generator().manual_seed(3))
    params = tt.sample(ref)
    a, b = tt(out, params), tt(ref, params)
    torch.cuda.synchronize()
    assert a.shape == (len(ACCEPTED), 3, 24, 24) and torch.equal(a, b)
    # without `shapes` the transforms read offsets / heights / widths back from the device: those tensors must be right too
    bare = {k: v for k, v in out.items() if k != "shapes"}
    bare["shapes"] = None
    assert torch.equal(ev(bare), ev(ref))


def test_bad_host_tables_are_refused_before_any_launch(world):
    host, pack = world["host"], world["pack"]
    geom, coef_off, coef_len, out_off, total = _tables(host)
    lib = L.lib()
    n = len(geom)
    ws_bytes = lib.hs_jpeg_ws_bytes(_ptr(geom), n)
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_bytes + 65536,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(geom=geom, coef_off=coef_off, coef_len=coef_len, out_off=out_off, ws_given=ws_bytes, out_bytes=total):
        return lib.hs_jpeg_decode(rt.p(pack["coef"]), pack["coef"].numel() * 2, rt.p(pack["qtab"]), _ptr(geom), _ptr(coef_off),
                                  _ptr(coef_len), _ptr(out_off), n, rt.p(buf, GUARD), out_bytes, rt.p(ws), ws_given, rt.stream())

    far_out, far_coef = out_off.copy(), coef_off.copy()
    far_out[-1] += 1                                            # the last image ends one byte past the arena
    far_coef[-1] = pack["coef"].numel() * 2                     # aligned, but its coefficients lie past the arena
    taller = geom.copy()
    taller[3, 0] += 16                                          # at least one more MCU row than coef_len[3] holds
    odd_sampling = geom.copy()
    odd_sampling[0, 3:5] = (1, 2)
    # (changed arguments, a word of the message): each refusal must be the one the case is about
    cases = {"output offset past the arena": (dict(out_off=far_out), "output offset"),
             "coefficient offset past the arena": (dict(coef_off=far_coef), "coefficient offset"),
             "geometry against coef_len": (dict(geom=taller, ws_given=ws_bytes + 65536), "coefficient bytes"),
             "unknown sampling": (dict(geom=odd_sampling), "geometry row"),
             "workspace too small": (dict(ws_given=ws_bytes - 16), "workspace"),
             "output arena too small": (dict(out_bytes=total - 1), "output offset"),
             "overlapping outputs": (dict(out_off=np.ascontiguousarray(out_off[::-1])), "overlaps")}
    for what, (kw, word) in cases.items():
        assert call(**kw) == L.HS_ERR_ARG, what
        assert word in lib.hs_last_error().decode(), (what, lib.hs_last_error())
    assert lib.hs_jpeg_ws_bytes(_ptr(odd_sampling), n) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all() and (ws.cpu().numpy() == 0x5A).all(), "a refused call launched something"
    L.check(call(), "hs_jpeg_decode")                           # and the unchanged tables are taken
    torch.cuda.synchronize()
    assert np.array_equal(buf[GUARD:GUARD + total].cpu().numpy(), np.concatenate([p.reshape(-1) for p in world["pixels"]]))
