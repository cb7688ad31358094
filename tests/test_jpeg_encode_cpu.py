"""CPU: the JPEG encoder's numpy statement (memotr_amd/data/jpeg_write.py) and host stage (csrc/jpeg_encode_core.h
through libjpeg_enc_hip.so) give Pillow's bytes -- on the committed fixture (tests/golden/jpeg_encode_cases.npz, no
PIL needed) and, where PIL imports, on a live sweep; the project's own decoder reads them back; what is out of scope
raises; a short buffer is never overrun; the C ABI is what the header declares; the host stage is memory-safe (a
sanitizer build of a stand-alone program)."""
import ctypes
import io
import os
import re
import shutil
import struct
import subprocess
from functools import partial

import numpy as np
import pytest
import torch

import cabi_helpers
from cabi_helpers import assert_binding_matches_header
from conftest import ROOT, load_golden

from memotr_amd.data import jpeg as J
from memotr_amd.data import jpeg_write as JW

SIZES = [(1, 1), (2, 2), (8, 8), (8, 9), (16, 16), (17, 33), (24, 16), (40, 36), (31, 47), (50, 70), (64, 96),
         (8, 300), (300, 8)]
SUB = {"0": "4:4:4", "2": "4:2:0"}


@pytest.fixture(scope="module")
def enc_lib():
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib
    build_jpeg_enc_lib()
    build_jpeg_lib()                    # the decoder reads the encoder's streams back
    from memotr_amd import _jpeg_enc_lib
    return _jpeg_enc_lib


@pytest.fixture(scope="module")
def cases():
    return load_golden("jpeg_encode_cases")


def streams(cases):
    """(name, image key, quality, subsampling, bytes) per committed stream."""
    off = cases["stream_offsets"]
    for i, name in enumerate(str(n) for n in cases["stream_names"]):
        size, kind, q, s = name.split("_")
        yield name, f"img_{size}_{kind}", int(q[1:]), SUB[s[1:]], cases["streams"][off[i]:off[i + 1]].tobytes()


def segments(data: bytes):
    """Marker segments up to and including SOS: (marker, payload)."""
    i, out = 2, []
    while True:
        assert data[i] == 0xFF
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out


def test_fixture_covers_the_cases_it_promises(cases):
    rows = list(streams(cases))
    assert len(rows) == 9 * 3 * 5 * 2 + 4 * 3 * 3 * 2
    seen = {}
    for name, key, q, sub, data in rows:
        h, w = cases[key].shape[:2]
        seen.setdefault((h, w), set()).add((key.split("_")[2], q, sub))
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    assert sorted(seen) == sorted(SIZES)
    for size, combos in seen.items():
        assert {c[0] for c in combos} == {"noise", "smooth", "sat"}
        assert {c[2] for c in combos} == {"4:4:4", "4:2:0"}
        assert {c[1] for c in combos} >= {10, 75, 100}
        if size[0] * size[1] < 1500:
            assert {c[1] for c in combos} == {10, 50, 75, 95, 100}
    for size in SIZES:
        sat = cases[f"img_{size[0]}x{size[1]}_sat"]
        assert set(np.unique(sat)) <= {0, 255}


def test_cpu_encode_equals_every_committed_pillow_stream(enc_lib, cases):
    for name, key, q, sub, want in streams(cases):
        got = JW.encode_jpeg(torch.from_numpy(cases[key]), quality=q, subsampling=sub)
        assert isinstance(got, bytes) and got == want, name
    # B, G, R input of the reversed channels is the same file
    for name, key, q, sub, want in list(streams(cases))[::17]:
        rev = torch.from_numpy(np.ascontiguousarray(cases[key][..., ::-1]))
        assert JW.encode_jpeg(rev, quality=q, subsampling=sub, bgr=True) == want, name


def test_tables_equal_those_in_the_committed_headers(enc_lib, cases):
    by_name = {name: (q, data) for name, _, q, _, data in streams(cases)}
    q50 = segments(by_name["16x16_noise_q50_s2"][1])
    dqt = [p for m, p in q50 if m == 0xDB]
    assert [p[0] for p in dqt] == [0, 1]
    # a quality-50 stream shows both Annex K tables unscaled, in zigzag order
    assert np.array_equal(np.frombuffer(dqt[0][1:], np.uint8)[np.argsort(JW.ZIGZAG)], JW.BASE_LUMA)
    assert np.array_equal(np.frombuffer(dqt[1][1:], np.uint8)[np.argsort(JW.ZIGZAG)], JW.BASE_CHROMA)
    for name, (q, data) in by_name.items():
        segs = segments(data)
        tables = JW.quant_tables(q)
        out = np.zeros(192, dtype=np.uint16)
        assert enc_lib.lib.jpegenc_quant_tables(q, out.ctypes.data) == 0
        assert np.array_equal(out.reshape(3, 64), tables)
        for t, p in enumerate(p for m, p in segs if m == 0xDB):
            assert np.array_equal(np.frombuffer(p[1:], np.uint8), tables[t][JW.ZIGZAG]), name
    # the four Huffman tables of the library's own header are the committed ones, segment for segment, for any image
    mine = segments(JW.encode_jpeg(torch.zeros((3, 5, 3), dtype=torch.uint8), quality=33, subsampling="4:4:4"))
    dht = [p for m, p in mine if m == 0xC4]
    assert [p[0] for p in dht] == [0x00, 0x10, 0x01, 0x11]
    assert dht == [p for m, p in q50 if m == 0xC4]
    assert [m for m, _ in mine] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert mine[0][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def test_live_sweep_equals_pillow(enc_lib):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for i in range(200):
        h, w, q = int(rng.integers(1, 81)), int(rng.integers(1, 81)), int(rng.integers(1, 101))
        if i % 3 == 0:
            px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif i % 3 == 1:
            px = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        else:
            y, x = np.mgrid[0:h, 0:w]
            px = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x * y) % 256], -1).astype(np.uint8)
        sub, s = (("4:4:4", 0), ("4:2:0", 2))[int(rng.integers(0, 2))]
        f = io.BytesIO()
        Image.fromarray(px).save(f, "JPEG", quality=q, subsampling=s)
        assert JW.encode_jpeg(torch.from_numpy(px), quality=q, subsampling=sub) == f.getvalue(), (h, w, q, sub)


def test_the_decoder_reads_back_the_coefficients_dummies_included(enc_lib, cases):
    for name, key, q, sub, want in streams(cases):
        made = JW.forward_coefficients_host(torch.from_numpy(cases[key]), q, sub)
        back = J.entropy_decode(JW.huffman_encode(made))
        assert back.info == made.info, name
        assert torch.equal(back.flat, made.flat), name
    made = JW.forward_coefficients_host(cases["img_8x9_noise"], 75, "4:2:0")      # (a numpy array is taken too)
    f = made.info
    assert (f.mcus_x, f.mcus_y, f.blocks_w, f.blocks_h, f.sampling) == (1, 1, (2, 1, 1), (2, 1, 1), "4:2:0")
    luma = made.components[0]
    assert int(luma[0, 0].abs().sum()) > 0 and int(luma[0, 1, 0, 0]) != 0         # both columns are real
    for bx in range(2):                 # the dummy row: the DC of the MCU's last upper block, zero AC
        assert int(luma[1, bx, 0, 0]) == int(luma[0, 1, 0, 0])
        assert int(luma[1, bx].abs().sum()) == abs(int(luma[1, bx, 0, 0]))
    made = JW.forward_coefficients_host(cases["img_24x16_noise"], 75, "4:2:0")
    assert [tuple(x.shape) for x in made.components] == [(4, 2, 8, 8), (2, 1, 8, 8), (2, 1, 8, 8)]


def test_decode_of_our_file_equals_pillows_decode_of_pillows_file(enc_lib, cases):
    Image = pytest.importorskip("PIL.Image")
    for name, key, q, sub, want in list(streams(cases))[::7]:
        mine = JW.encode_jpeg(torch.from_numpy(cases[key]), quality=q, subsampling=sub)
        px = np.asarray(Image.open(io.BytesIO(want)).convert("RGB"))
        assert np.array_equal(J.decode_jpeg(mine, "cpu", fallback=False).numpy(), px), name


def test_clips_go_through_the_batch_entry(enc_lib, cases):
    frames = [torch.from_numpy(cases[f"img_{s}_{k}"]) for s in ("31x47", "8x9") for k in ("noise", "smooth", "sat")]
    order = [0, 3, 1, 4, 2, 5]          # mixed sizes keep their places
    out = JW.encode_jpegs([frames[i] for i in order], threads=64, quality=75, subsampling="4:2:0")
    by_name = {name: data for name, _, _, _, data in streams(cases)}
    names = [f"{s}_{k}_q75_s2" for s in ("31x47", "8x9") for k in ("noise", "smooth", "sat")]
    assert out == [by_name[names[i]] for i in order]
    assert JW.encode_jpegs([]) == []
    assert JW.encode_jpegs(torch.stack(frames[:3]), threads=1, subsampling="4:4:4", quality=10) == \
        [by_name[f"31x47_{k}_q10_s0"] for k in ("noise", "smooth", "sat")]


def test_what_is_out_of_scope_raises(enc_lib):
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for sub in ("4:2:2", "4:1:1", 2, None, "gray"):
        with pytest.raises(ValueError, match="subsampling"):
            JW.encode_jpeg(x, subsampling=sub)
    for q in (0, 101, -1, 75.0, True):
        with pytest.raises(ValueError, match="quality"):
            JW.encode_jpeg(x, quality=q)
        with pytest.raises(ValueError, match="quality"):
            JW.forward_coefficients_host(x, q)
    for bad in (torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((8, 8, 3)), torch.zeros((8, 8, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            JW.encode_jpeg(bad)
    with pytest.raises(ValueError, match="threads"):
        JW.encode_jpegs([x], threads=0)
    gray = J.JpegCoefficients(J.JpegInfo(8, 8, 1, 1, 1, 0, 1, 1, (1,), (1,), (1,), (1,), (0,), 64),
                              torch.zeros(64 + 192, dtype=torch.int16))
    with pytest.raises(ValueError, match="three components"):
        JW.huffman_encode(gray)
    made = JW.forward_coefficients_host(x, 75, "4:4:4")
    made.flat[5] = 3000                 # an AC coefficient of 12 bits: no baseline code
    with pytest.raises(ValueError, match="baseline coding cannot express"):
        JW.huffman_encode(made)


def test_a_short_buffer_returns_the_size_and_is_not_overrun(enc_lib, cases):
    lib = enc_lib.lib
    made = JW.forward_coefficients_host(cases["img_17x33_noise"], 75, "4:2:0")
    want = JW.huffman_encode(made)
    info = enc_lib.Info()
    assert lib.jpegenc_geometry(33, 17, 2, ctypes.byref(info)) == 0
    coef, qt = made.flat.data_ptr(), made.flat.data_ptr() + 2 * made.info.coef_count
    assert lib.jpegenc_huffman_encode(coef, qt, ctypes.byref(info), None, 0) == len(want)
    for cap in (len(want) - 1, 700, 3, 1):
        buf = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
        assert lib.jpegenc_huffman_encode(coef, qt, ctypes.byref(info), buf.ctypes.data, cap) == len(want)
        assert buf[:cap].tobytes() == want[:cap] and (buf[cap:] == 0xA5).all(), cap
    buf = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
    assert lib.jpegenc_huffman_encode(coef, qt, ctypes.byref(info), buf.ctypes.data, len(want)) == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()


def test_library_exports_what_the_header_declares(enc_lib):
    syms = assert_binding_matches_header(enc_lib, "jpeg_enc_hip.h", "jpegenc", "JPEGENC_ABI_VERSION")
    assert syms == ["jpegenc_abi_version", "jpegenc_forward_u8", "jpegenc_geometry", "jpegenc_huffman_encode",
                    "jpegenc_huffman_encode_batch", "jpegenc_last_error", "jpegenc_planes_bytes",
                    "jpegenc_quant_tables"]
    define = partial(cabi_helpers.define, "jpeg_enc_hip.h")
    assert enc_lib.ABI_VERSION == 1
    assert define("JPEGENC_ERR_LEN") == enc_lib.ERR_LEN
    assert define("JPEGENC_MAX_THREADS") == enc_lib.MAX_THREADS == 16
    assert define("JPEGENC_QT_WORDS") == enc_lib.QT_WORDS == J.QT_WORDS
    assert (define("JPEGENC_TILE_X"), define("JPEGENC_TILE_Y")) == (enc_lib.TILE_X, enc_lib.TILE_Y)
    from memotr_amd import _jpeg_lib
    assert [f[0] for f in enc_lib.Info._fields_] == [f[0] for f in _jpeg_lib.Info._fields_]
    assert ctypes.sizeof(enc_lib.Info) == 112


def test_bad_arguments_give_error_codes_without_a_device(enc_lib):
    lib, err = enc_lib.lib, enc_lib.lib.jpegenc_last_error
    info = enc_lib.Info()
    assert lib.jpegenc_geometry(33, 31, 2, None) == 1 and b"null pointer" in err()
    assert lib.jpegenc_geometry(33, 31, 3, ctypes.byref(info)) == 2
    assert lib.jpegenc_geometry(0, 31, 2, ctypes.byref(info)) == 2
    assert lib.jpegenc_geometry(33, 31, 2, ctypes.byref(info)) == 0 and err() == b""
    assert (info.mcus_x, info.mcus_y, info.coef_count) == (3, 2, 36 * 64)
    assert JW.frame_info(31, 33, "4:2:0") == J._info(info)
    assert lib.jpegenc_planes_bytes(ctypes.byref(info)) == info.coef_count
    assert lib.jpegenc_planes_bytes(None) == -1
    qt = np.ascontiguousarray(JW.quant_tables(75).astype(np.uint16).reshape(-1))
    assert lib.jpegenc_quant_tables(0, qt.ctypes.data) == 2 and lib.jpegenc_quant_tables(101, qt.ctypes.data) == 2

    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch
    ok = dict(frame=p, row=3 * 33, fp=3 * 33 * 31, info=info, qt=qt.ctypes.data, planes=p, pb=2 * info.coef_count,
              coef=p, cp=info.coef_count, B=2, swap=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.jpegenc_forward_u8(a["frame"], a["row"], a["fp"], ctypes.byref(a["info"]), a["qt"], a["planes"],
                                      a["pb"], a["coef"], a["cp"], a["B"], a["swap"], None)

    assert call(B=0) == 0 and err() == b""
    assert call(B=-1) == 2 and b"negative batch" in err()
    assert call(frame=None) == 1 and b"null pointer" in err() and b"jpegenc_forward_u8" in err()
    assert call(coef=ctypes.c_void_p(4098)) == 3 and b"aligned" in err()
    assert call(cp=info.coef_count + 4) == 3 and b"multiple of 8" in err()
    assert call(cp=info.coef_count - 64) == 4
    assert call(pb=2 * info.coef_count - 1) == 5 and b"workspace" in err()
    assert call(row=3 * 33 - 1) == 6 and b"row pitch" in err()
    assert call(fp=3 * 33 * 30) == 6 and b"overlap" in err()
    assert call(swap=2) == 7
    assert call(B=65536, pb=1 << 40) == 8
    wide = qt.copy()
    wide[70] = 256
    assert call(qt=wide.ctypes.data) == 9 and b"table entry" in err()
    broken = enc_lib.Info.from_buffer_copy(info)
    broken.mcus_x += 1
    assert call(info=broken) == 2 and b"geometry" in err()
    broken = enc_lib.Info.from_buffer_copy(info)
    broken.vmax = 1                       # 4:2:2 is not written
    assert call(info=broken) == 2

    sizes = (ctypes.c_int64 * 3)()
    assert lib.jpegenc_huffman_encode_batch(None, None, None, 3, None, None, sizes, 4) == -1
    assert lib.jpegenc_huffman_encode_batch(None, None, None, 0, None, None, None, 4) == 0


def test_a_cuda_encode_has_no_substitute_for_the_library():
    import inspect
    src = inspect.getsource(JW.forward_coefficients_device)
    assert "L.check(L.lib.jpegenc_forward_u8(" in src and "except" not in src


# ------------------------------------------------------------------------------------ memory safety of the host stage
def test_host_stage_is_memory_safe(enc_lib, cases, tmp_path):
    """tests/native/jpeg_encode_check.cpp under AddressSanitizer and UBSan, a process of its own: every fixture
    coefficient set into exact, one-byte-short and far-too-small heap buffers, and arbitrary coefficients."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "jpeg_encode_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined",
                            os.path.join(ROOT, "tests", "native", "jpeg_encode_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    sets = tmp_path / "sets"
    sets.mkdir()
    count = 0
    for name, key, q, sub, want in streams(cases):
        made = JW.forward_coefficients_host(torch.from_numpy(cases[key]), q, sub)
        h, w = cases[key].shape[:2]
        (sets / f"{count:03d}_{name}.coef").write_bytes(struct.pack("<iii", w, h, made.info.hmax) +
                                                        made.flat.numpy().tobytes())
        (sets / f"{count:03d}_{name}.jpg").write_bytes(want)
        count += 1
    run = subprocess.run([str(exe), str(sets)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    m = re.match(rf"sets {count}: equal {count}; short buffers ok (\d+); arbitrary coefficients sized (\d+) refused (\d+)",
                 run.stdout)
    assert m, run.stdout
    assert int(m.group(1)) >= 3 * count + 600 and int(m.group(2)) > 0 and int(m.group(3)) > 0
    assert int(m.group(2)) + int(m.group(3)) == 20 * count
