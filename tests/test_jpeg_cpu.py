"""JPEG decode, host side: the numpy restatement against the stored Pillow pixels, the C entropy stage against the restatement,
refusals, truncation, the Python records, and the stand-alone sanitizer check of csrc/jpeg_host.h.  Needs the built library,
no GPU (the two host entries make no HIP call)."""
import ctypes as C
import io
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import hamspine._lib as L
import jpeg_ref
from hamspine import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
ACCEPTED = [str(n) for n in GOLDEN["accepted"]]
REFUSED = [str(n) for n in GOLDEN["refused"]]
GUARD = 0x5A5A


def _bytes(name):
    return GOLDEN[f"bytes/{name}"].tobytes()


def _decode_c(data, coef_words=None, short=0):
    """(status, info, coef incl. 64 guard words, qtab incl. 64 guard words) of hs_jpeg_probe + hs_jpeg_entropy_decode"""
    lib = L.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    info = L.JpegInfo()
    st = lib.hs_jpeg_probe(buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(info))
    words = info.coef_bytes // 2 if st == L.HS_OK else (coef_words or 64)
    coef = np.full(words + 64, GUARD, dtype=np.int16)
    qtab = np.full(3 * 64 + 64, GUARD, dtype=np.uint16)
    info2 = L.JpegInfo()
    st2 = lib.hs_jpeg_entropy_decode(buf.ctypes.data_as(C.c_void_p), buf.size, coef.ctypes.data_as(C.c_void_p), words * 2 - short,
                                     qtab.ctypes.data_as(C.c_void_p), C.byref(info2))
    return st, st2, info2, coef, qtab


def test_fixture_holds_the_cases_the_decoder_can_get_wrong():
    for size in ("1x5", "8x8", "16x16", "9x6", "17x23", "33x50"):
        for sub in ("444", "422", "420"):
            assert f"{size}_{sub}" in ACCEPTED
    for name in ("21x19_gray", "17x23_420_q30", "17x23_422_q95", "33x50_420_optimize", "33x50_420_restart3", "40x40_444_noise_q100"):
        assert name in ACCEPTED
    assert REFUSED == ["16x16_progressive", "9x4_420"]
    assert b"\xff\xdd" in _bytes("33x50_420_restart3") and b"\xff\xd0" in _bytes("33x50_420_restart3")
    assert _bytes("33x50_420_optimize") != _bytes("33x50_420")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")) < 300 * 1024
    sat = GOLDEN["pixels/40x40_444_noise_q100"]
    assert (sat == 0).any() and (sat == 255).any()


@pytest.mark.parametrize("name", ACCEPTED)
def test_reference_reproduces_pillows_pixels_and_the_stored_coefficients(name):
    coefs, qtabs, geo = jpeg_ref.coefficients(_bytes(name))
    assert np.array_equal(np.concatenate([c.reshape(-1) for c in coefs]), GOLDEN[f"coef/{name}"])
    assert np.array_equal(qtabs, GOLDEN[f"qtab/{name}"])
    px = jpeg_ref.pixels(coefs, qtabs, geo)
    assert px.dtype == np.uint8 and px.shape == GOLDEN[f"pixels/{name}"].shape
    assert np.array_equal(px, GOLDEN[f"pixels/{name}"])


def test_reference_equals_a_live_pillow_decode():
    Image = pytest.importorskip("PIL.Image")
    for name in ACCEPTED:
        live = np.asarray(Image.open(io.BytesIO(_bytes(name))).convert("RGB"))
        assert np.array_equal(jpeg_ref.decode(_bytes(name)), live), name


@pytest.mark.parametrize("name", ACCEPTED)
def test_c_entropy_stage_equals_the_reference(name):
    st, st2, info, coef, qtab = _decode_c(_bytes(name))
    assert (st, st2) == (L.HS_OK, L.HS_OK)
    g = GOLDEN[f"geom/{name}"]
    nc = int(g[2])
    assert (info.height, info.width, info.components) == tuple(g[:3])
    assert list(info.h_samp)[:nc] == list(g[3:3 + nc]) and list(info.v_samp)[:nc] == list(g[6:6 + nc])
    assert list(info.block_rows)[:nc] == list(g[9:9 + nc]) and list(info.block_cols)[:nc] == list(g[12:12 + nc])
    want = GOLDEN[f"coef/{name}"]
    assert info.coef_bytes == want.nbytes == sum(int(r) * int(c) * 128 for r, c in zip(g[9:9 + nc], g[12:12 + nc]))
    assert np.array_equal(coef[:want.size], want)
    assert (coef[want.size:] == GUARD).all(), "guard words after coef_bytes were written"
    assert np.array_equal(qtab[:64 * nc].reshape(nc, 64), GOLDEN[f"qtab/{name}"])
    assert (qtab[192:] == GUARD).all()
    # a buffer that is too small is refused and stays untouched
    _, st3, _, small, _ = _decode_c(_bytes(name), short=2)
    assert st3 == L.HS_ERR_ARG and (small == GUARD).all()


def _patched(name, find, at, value):
    """the golden stream with one byte changed at offset `at` behind the first occurrence of marker `find`"""
    b = bytearray(_bytes(name))
    i = b.index(find)
    b[i + at] = value
    return bytes(b)


REFUSALS = {
    "progressive": (lambda: _bytes("16x16_progressive"), "PROGRESSIVE"),
    "narrow": (lambda: _bytes("9x4_420"), "NARROW"),
    "12-bit": (lambda: _patched("17x23_420", b"\xff\xc0", 4, 12), "PRECISION"),
    "4 components": (lambda: _patched("17x23_420", b"\xff\xc0", 9, 4), "COMPONENTS"),
    "sampling 1x2": (lambda: _patched("17x23_420", b"\xff\xc0", 11, 0x12), "SAMPLING"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_each_refusal_has_its_own_status_and_writes_nothing(case):
    make, status = REFUSALS[case]
    data = make()
    want = L._header.constants["HS_JPEG_ERR_" + status]
    st, st2, _, coef, qtab = _decode_c(data, coef_words=4096)
    assert (st, st2) == (want, want), (case, st, st2)
    assert (coef == GUARD).all() and (qtab == GUARD).all()
    assert L.lib().hs_jpeg_status_text(want)
    with pytest.raises(jpeg_ref.Refused) as e:
        jpeg_ref.coefficients(data)
    assert e.value.status == status
    statuses = [L._header.constants["HS_JPEG_ERR_" + s] for _, s in REFUSALS.values()]
    assert len(set(statuses)) == len(statuses) and L._header.constants["HS_JPEG_ERR_CORRUPT"] not in statuses


@pytest.mark.parametrize("name", ACCEPTED + REFUSED)
def test_truncation_is_corrupt_or_the_same_image(name):
    data = _bytes(name)
    corrupt = L._header.constants["HS_JPEG_ERR_CORRUPT"]
    own = None if name in ACCEPTED else L._header.constants["HS_JPEG_ERR_" + str(GOLDEN[f"status/{name}"])]
    full = GOLDEN[f"coef/{name}"] if name in ACCEPTED else None
    seen = set()
    for k in range(16):
        cut = len(data) * (k + 1) // 17                                       # 16 evenly spaced points inside the stream
        st, st2, _, coef, qtab = _decode_c(data[:cut], coef_words=4096)
        seen.add(st2)
        if own is not None:
            assert st2 in (corrupt, own) and (coef == GUARD).all(), (name, cut, st2)
        elif st2 == L.HS_OK:
            assert np.array_equal(coef[:full.size], full), (name, cut)
        else:
            assert st2 == corrupt, (name, cut, st2)
            with pytest.raises(jpeg_ref.Corrupt):
                jpeg_ref.coefficients(data[:cut])
    assert corrupt in seen
    # the last two bytes are EOI: without them the last MCU is still whole
    if own is None:
        st, st2, _, coef, _ = _decode_c(data[:-2])
        assert st2 == L.HS_OK and np.array_equal(coef[:full.size], full)


def test_records_pickle_and_a_mixed_batch_packs_in_order():
    """needs no Pillow: the fallback record is made from the stored pixels, as entropy_decode makes it"""
    names = ["17x23_420", "9x6_444", "9x4_420", "21x19_gray", "33x50_422"]
    recs = [{"pixels": GOLDEN[f"pixels/{n}"]} if n in REFUSED else J.entropy_decode(_bytes(n), fallback="raise") for n in names]
    recs = pickle.loads(pickle.dumps(recs))
    for n, r in zip(names, recs):
        if "coef" in r:
            assert r["coef"].dtype == np.int16 and np.array_equal(r["coef"], GOLDEN[f"coef/{n}"])
            assert tuple(r["geom"][:3]) == tuple(GOLDEN[f"geom/{n}"][:3])
    pack = J.pack_jpegs(recs, pin=False)
    assert pack["shapes"] == ((17, 23), (9, 6), (9, 4), (21, 19), (33, 50))
    assert pack["raw_index"] == (2,) and pack["raw"].numel() == 9 * 4 * 3
    assert np.array_equal(pack["raw"].numpy(), GOLDEN["pixels/9x4_420"].reshape(-1))
    assert len(pack["geoms"]) == 4 and pack["qtab"].shape == (4, 3, 64)
    # the decoded pack's tables are made here, on the host, and staged with the pack: pack_images' dtypes and values
    sizes = [3 * h * w for h, w in pack["shapes"]]
    assert pack["offsets"].dtype.is_floating_point is False and str(pack["offsets"].dtype) == "torch.int64"
    assert pack["offsets"].tolist() == [sum(sizes[:i]) for i in range(5)]
    assert str(pack["heights"].dtype) == str(pack["widths"].dtype) == "torch.int32"
    assert pack["heights"].tolist() == [17, 9, 9, 21, 33] and pack["widths"].tolist() == [23, 6, 4, 19, 50]
    at, covered = 0, np.zeros(pack["coef"].numel(), dtype=bool)
    for j, n in enumerate(n for n in names if n != "9x4_420"):
        want = GOLDEN[f"coef/{n}"]
        off, ln = pack["coef_offsets"][j], pack["coef_lens"][j]
        assert off % 16 == 0 and off >= at and ln == want.nbytes
        assert np.array_equal(pack["coef"].numpy()[off // 2:off // 2 + want.size], want)
        covered[off // 2:off // 2 + want.size] = True
        nc = int(GOLDEN[f"geom/{n}"][2])
        assert np.array_equal(pack["qtab"].numpy().view(np.uint16)[j, :nc], GOLDEN[f"qtab/{n}"])
        at = off + ln
    assert pack["coef"].numel() * 2 >= at
    assert (pack["coef"].numpy()[~covered] == 0).all(), "alignment gaps of the coefficient arena are cleared"
    with pytest.raises(J.JpegRefused) as e:
        J.entropy_decode(_bytes("9x4_420"), fallback="raise")
    assert e.value.status == L._header.constants["HS_JPEG_ERR_NARROW"]
    with pytest.raises(J.JpegRefused):
        J.entropy_decode(_bytes("16x16_progressive"), fallback="raise")
    with pytest.raises(L.HamspineError, match="corrupt"):
        J.entropy_decode(_bytes("17x23_420")[:200], fallback="raise")
    assert J.probe(_bytes("33x50_420"))["block_cols"] == (8, 4, 4)
    only_raw = J.pack_jpegs([recs[2]], pin=False)
    assert only_raw["geoms"] == () and only_raw["offsets"].tolist() == [0] and only_raw["raw_index"] == (0,)


def test_refused_files_fall_back_to_pillow_and_corrupt_ones_still_raise():
    pytest.importorskip("PIL.Image")
    for name in REFUSED:
        rec = pickle.loads(pickle.dumps(J.entropy_decode(_bytes(name))))
        assert set(rec) == {"pixels"} and np.array_equal(rec["pixels"], GOLDEN[f"pixels/{name}"])
    with pytest.raises(L.HamspineError, match="corrupt"):          # a corrupt file always raises, with the status text
        J.entropy_decode(_bytes("17x23_420")[:200], fallback="pillow")


def _with_size(name, h, w):
    b = bytearray(_bytes(name))
    i = b.index(b"\xff\xc0")
    b[i + 5:i + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
    return bytes(b)


def test_a_short_file_cannot_claim_a_huge_frame():
    """3 * h * w >= 2^31 is a refusal of its own (the device stage indexes output bytes in 32 bits); below that, a frame whose
    blocks need more than the scan's bits (2 per block at least) is corrupt for probe already, before any buffer is sized"""
    corrupt, too_large = L._header.constants["HS_JPEG_ERR_CORRUPT"], L._header.constants["HS_JPEG_ERR_TOO_LARGE"]
    st, st2, _, coef, qtab = _decode_c(_with_size("17x23_420", 65535, 65535), coef_words=4096)
    assert (st, st2) == (too_large, too_large) and (coef == GUARD).all() and (qtab == GUARD).all()
    with pytest.raises(jpeg_ref.Refused) as e:
        jpeg_ref.coefficients(_with_size("17x23_420", 65535, 65535))
    assert e.value.status == "TOO_LARGE"
    assert 3 * 26754 * 26754 < 2 ** 31 <= 3 * 26755 * 26755
    for name in ("17x23_420", "21x19_gray"):
        st, st2, _, coef, qtab = _decode_c(_with_size(name, 26754, 26754), coef_words=4096)
        assert (st, st2) == (corrupt, corrupt) and (coef == GUARD).all() and (qtab == GUARD).all()
        with pytest.raises(jpeg_ref.Corrupt):
            jpeg_ref.coefficients(_with_size(name, 26754, 26754))
    with pytest.raises(L.HamspineError, match="corrupt"):
        J.entropy_decode(_with_size("17x23_420", 26754, 26754))
    # the bound itself: a frame is probed as long as 4 blocks per byte of scan could hold it
    data = _bytes("8x8_444")
    scan = len(data) - (data.index(b"\xff\xda") + 14)
    fits, over = 8 * int((4 * scan // 3) ** 0.5), 8 * (int((4 * scan // 3) ** 0.5) + 1)
    assert L.lib().hs_jpeg_probe(np.frombuffer(_with_size("8x8_444", fits, fits), np.uint8).ctypes.data_as(C.c_void_p), len(data),
                                 C.byref(L.JpegInfo())) == L.HS_OK
    assert L.lib().hs_jpeg_probe(np.frombuffer(_with_size("8x8_444", over, over), np.uint8).ctypes.data_as(C.c_void_p), len(data),
                                 C.byref(L.JpegInfo())) == corrupt


def test_jfif_marker_counts_only_at_libjpegs_length():
    """component ids 'R','G','B' are YCbCr under a JFIF APP0 of 14 data bytes or more (libjpeg's rule), RGB -- refused -- under a
    shorter one or none"""
    b = bytearray(_bytes("17x23_444"))
    i = b.index(b"\xff\xc0")
    b[i + 10], b[i + 13], b[i + 16] = b"RGB"
    s = b.index(b"\xff\xda")
    b[s + 5], b[s + 7], b[s + 9] = b"RGB"
    a = b.index(b"\xff\xe0")
    alen = (b[a + 2] << 8) | b[a + 3]
    assert alen == 16 and bytes(b[a + 4:a + 9]) == b"JFIF\0"
    colorspace = L._header.constants["HS_JPEG_ERR_COLORSPACE"]
    full = bytes(b)
    short = bytes(b[:a]) + b"\xff\xe0\x00\x0fJFIF\0" + bytes(8) + bytes(b[a + 2 + alen:])     # 13 data bytes
    none = bytes(b[:a]) + bytes(b[a + 2 + alen:])
    st, st2, _, coef, _ = _decode_c(full)
    assert (st, st2) == (L.HS_OK, L.HS_OK) and np.array_equal(coef[:-64], GOLDEN["coef/17x23_444"])
    assert np.array_equal(jpeg_ref.decode(full), GOLDEN["pixels/17x23_444"])
    for data in (short, none):
        st, st2, _, coef, _ = _decode_c(data, coef_words=4096)
        assert (st, st2) == (colorspace, colorspace) and (coef == GUARD).all()
        with pytest.raises(jpeg_ref.Refused) as e:
            jpeg_ref.coefficients(data)
        assert e.value.status == "COLORSPACE"


def test_new_structs_and_constants_agree_with_the_compiled_library():
    lib = L.lib()
    assert [(w, c.__name__) for w, c in L.later_abi_structs()] == [(14, "JpegInfo")]
    assert lib.hs_abi_sizeof(14) == C.sizeof(L.JpegInfo) == 72
    assert [f for f, _ in L.JpegInfo._fields_] == ["width", "height", "components", "h_samp", "v_samp", "block_rows", "block_cols",
                                                   "restart_interval", "coef_bytes"]
    assert lib.hs_jpeg_probe.argtypes == [C.c_void_p, C.c_int64, C.POINTER(L.JpegInfo)]
    assert lib.hs_jpeg_status_text.restype is C.c_char_p
    assert (L.JPEG_GEOM, L.JPEG_MAX_COMPONENTS) == (8, 3) and L.JPEG_STATUS[16] == "CORRUPT" and len(L.JPEG_STATUS) == 12


def test_host_stage_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/jpeg_host_check.cpp: csrc/jpeg_host.h alone, every golden stream and 2000 mutations of each, ASan + UBSan"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    files = []
    for name in ACCEPTED + REFUSED:
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(_bytes(name))
        files.append(str(p))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert f"{len(files)} files, 2000 mutations each" in run.stdout
