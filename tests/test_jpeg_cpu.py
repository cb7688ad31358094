"""CPU: the JPEG decoder's host stage (csrc/jpeg_entropy_core.h through libjpeg_ops_hip.so) and the numpy statement of
the pixel arithmetic (memotr_amd/data/jpeg.py) equal Pillow byte for byte -- on the committed fixture
(tests/golden/jpeg_cases.npz, no PIL needed) and, where PIL imports, on a live sweep; every kind of stream outside
the scope is refused with its own message; the C ABI is what the header declares; the parser is memory-safe on
hostile input (a sanitizer build of a stand-alone program)."""
import ctypes
import io
import os
import re
import shutil
import subprocess
from functools import partial

import numpy as np
import pytest
import torch

import cabi_helpers
from cabi_helpers import assert_binding_matches_header
from conftest import ROOT, load_golden

from memotr_amd.data import jpeg as J


@pytest.fixture(scope="module")
def jpeg_lib():
    from memotr_amd.build import build_jpeg_lib
    build_jpeg_lib()
    from memotr_amd import _jpeg_lib
    return _jpeg_lib


@pytest.fixture(scope="module")
def cases():
    return load_golden("jpeg_cases")


def names(cases):
    return [str(n) for n in cases["names"]]


def stream(cases, name) -> bytes:
    return cases["jpg_" + name].tobytes()


def test_fixture_covers_the_cases_it_promises(jpeg_lib, cases):
    all_names = names(cases)
    assert len(all_names) == 49
    infos = {n: J.parse_jpeg(stream(cases, n)) for n in all_names}
    grid = [n for n in all_names if re.match(r"\d+x\d+_s", n)]
    sizes = {(infos[n].height, infos[n].width) for n in grid}
    assert sizes == {(1, 1), (5, 7), (8, 8), (16, 16), (17, 17), (31, 33), (40, 48), (8, 300), (300, 8)}
    for size in sizes:
        assert {infos[n].sampling for n in grid if (infos[n].height, infos[n].width) == size} == \
            {"4:4:4", "4:2:2", "4:2:0", "gray"}
    for mode in ("s0", "s1", "s2", "sL"):
        of_mode = [n for n in grid if f"_{mode}_" in n]
        assert {n.split("_")[2] for n in of_mode} == {"q30", "q75", "q100"}
        assert {n.split("_")[3] for n in of_mode} == {"r0", "r1", "r3"}
    assert any(infos[n].restart_interval > 0 for n in grid) and any(infos[n].restart_interval == 0 for n in grid)
    assert b"\xff\xfe" in stream(cases, "com_dqt16")[:4] and b"\xff\xc1" in stream(cases, "com_dqt16")
    assert int(J.entropy_decode(stream(cases, "com_dqt16")).qt.max()) > 255
    assert int(J.entropy_decode(stream(cases, "patched_dqt")).qt.min()) == 255


def test_cpu_decode_equals_the_committed_pillow_pixels(jpeg_lib, cases):
    for n in names(cases):
        want = cases["rgb_" + n]
        got = J.decode_jpeg(stream(cases, n), "cpu", fallback=False)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, n
        assert np.array_equal(got.numpy(), want), n
        bgr = J.decode_jpeg(cases["jpg_" + n], "cpu", bgr=True, fallback=False)         # a uint8 array as the stream
        assert np.array_equal(bgr.numpy(), want[..., ::-1]), n


def test_paths_clips_and_coefficient_layout(jpeg_lib, cases, tmp_path):
    p = tmp_path / "a.jpg"
    p.write_bytes(stream(cases, "clip_0"))
    assert np.array_equal(J.decode_jpeg(str(p), "cpu").numpy(), cases["rgb_clip_0"])
    clip = J.decode_jpegs([stream(cases, f"clip_{i}") for i in range(3)], "cpu", threads=2)
    assert tuple(clip.shape) == (3, 31, 33, 3)
    for i in range(3):
        assert np.array_equal(clip[i].numpy(), cases[f"rgb_clip_{i}"])
    mixed = J.decode_jpegs([stream(cases, "clip_0"), stream(cases, "track_0"), p], "cpu")
    assert isinstance(mixed, list) and [tuple(m.shape) for m in mixed] == [(31, 33, 3), (64, 96, 3), (31, 33, 3)]
    assert np.array_equal(mixed[1].numpy(), cases["rgb_track_0"])
    assert J.decode_jpegs([], "cpu") == []

    c = J.entropy_decode(stream(cases, "clip_0"))
    f = c.info
    assert (f.width, f.height, f.ncomp, f.hmax, f.vmax, f.mcus_x, f.mcus_y) == (33, 31, 3, 2, 2, 3, 2)
    assert f.sampling == "4:2:0" and f.chroma_size == (16, 17)
    assert [tuple(x.shape) for x in c.components] == [(4, 6, 8, 8), (2, 3, 8, 8), (2, 3, 8, 8)]
    assert c.flat.numel() == f.coef_count + 192 == (24 + 6 + 6) * 64 + 192 and tuple(c.qt.shape) == (3, 64)
    # every block is written whole: a buffer full of garbage gives the same coefficients
    dirty = torch.full((f.coef_count + 192 + 5,), 12345, dtype=torch.int16)
    again = J.entropy_decode(stream(cases, "clip_0"), pinned=dirty)
    assert torch.equal(again.flat, c.flat) and again.flat.data_ptr() == dirty.data_ptr()
    assert (dirty[f.coef_count + 192:] == 12345).all()
    with pytest.raises(ValueError, match="at least"):
        J.entropy_decode(stream(cases, "clip_0"), pinned=torch.empty(10, dtype=torch.int16))


def test_live_sweep_equals_pillow(jpeg_lib):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2024)
    for i in range(200):
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        y, x = np.mgrid[0:h, 0:w]
        px = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(w + h - 2, 1)], -1)
        px[(x // 5 + y // 7) % 2 == 0] *= 0.3
        px += rng.integers(-40, 41, (h, w, 3)) * (x >= w // 2)[..., None]
        im = Image.fromarray(np.clip(px, 0, 255).astype(np.uint8))
        mode = i % 4
        kw = {"quality": int(rng.choice([30, 75, 90, 100]))}
        if mode == 3:
            im = im.convert("L")
        else:
            kw["subsampling"] = mode
        restart = int(rng.integers(0, 5))
        if restart:
            kw["restart_marker_blocks"] = restart
        buf = io.BytesIO()
        im.save(buf, "JPEG", **kw)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        got = J.decode_jpeg(buf.getvalue(), "cpu", fallback=False).numpy()
        assert np.array_equal(got, want), (i, h, w, mode, kw)


# ------------------------------------------------------------------------------------ what is refused
def segments(data):
    i = 2
    while True:
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        yield m, i, n + 2
        if m == 0xDA:
            return
        i += n + 2


def find(data, marker):
    return next((i, n) for m, i, n in segments(data) if m == marker)


def patched(data, marker, offset, value):
    b = bytearray(data)
    b[find(data, marker)[0] + offset] = value
    return bytes(b)


def insert_before(data, marker, segment):
    i = find(data, marker)[0]
    return data[:i] + segment + data[i:]


def without(data, marker):
    i, n = find(data, marker)
    return data[:i] + data[i + n:]


ADOBE = lambda transform: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])  # noqa: E731


def test_every_rejected_kind_raises_with_its_message(jpeg_lib, cases):
    base_name = next(n for n in names(cases) if n.startswith("17x17_s0"))
    base = stream(cases, base_name)
    assert J.parse_jpeg(base).sampling == "4:4:4"
    sos_i, sos_n = find(base, 0xDA)
    second_scan = base[:-2] + base[sos_i:sos_i + sos_n] + b"\x00\xff\xd9"
    one_component_scan = bytearray(base)
    one_component_scan[sos_i + 4] = 1
    unsupported = {
        "progressive": (stream(cases, "progressive"), "progressive"),
        "cmyk (4 components)": (stream(cases, "cmyk"), "1 or 3 components"),
        "arithmetic": (patched(base, 0xC0, 1, 0xC9), "arithmetic"),
        "lossless": (patched(base, 0xC0, 1, 0xC3), "lossless"),
        "12 bits": (patched(base, 0xC0, 4, 12), "8-bit precision"),
        "adobe rgb": (insert_before(base, 0xC0, ADOBE(0)), "transform 0"),
        "adobe ycck": (insert_before(base, 0xDA, ADOBE(2)), "transform 2"),
        "4:1:1": (patched(base, 0xC0, 11, 0x41), "sampling"),
        "4:4:0": (patched(base, 0xC0, 11, 0x12), "sampling"),
        "subsampled chroma only": (patched(base, 0xC0, 14, 0x21), "sampling"),
        "multiple scans": (bytes(one_component_scan), "multiple scans"),
    }
    for kind, (data, text) in unsupported.items():
        with pytest.raises(J.UnsupportedJpeg, match=text):
            J.decode_jpeg(data, "cpu", fallback=False)
        with pytest.raises(J.UnsupportedJpeg, match=text):
            J.decode_jpegs([base, data], "cpu", fallback=False)
    # (bytes behind a complete scan are never reached: all MCUs are decoded by then)
    assert np.array_equal(J.decode_jpeg(second_scan, "cpu", fallback=False).numpy(), cases["rgb_" + base_name])

    dht = find(base, 0xC4)
    scan = sos_i + sos_n
    no_code = bytearray(base)                       # the first DHT keeps one 1-bit code only: most codes are then unknown
    no_code[dht[0] + 5:dht[0] + 21] = bytes([1] + [0] * 15)
    no_code = bytes(no_code[:dht[0] + 2]) + (2 + 1 + 16 + 1).to_bytes(2, "big") + bytes(no_code[dht[0] + 4:dht[0] + 22]) \
        + base[dht[0] + dht[1]:]
    corrupt = {
        "not a jpeg": (b"\x89PNG\r\n\x1a\n" + base, "no SOI"),
        "empty": (b"", "no SOI"),
        "zero width": (patched(patched(base, 0xC0, 7, 0), 0xC0, 8, 0), "width or height is 0"),
        "zero height": (patched(patched(base, 0xC0, 5, 0), 0xC0, 6, 0), "width or height is 0"),
        "missing DQT": (without(base, 0xDB), "quantisation table that is not defined"),
        "missing DHT": (without(base, 0xC4), "Huffman table that is not defined"),
        "code not in the table": (no_code, "not in the (DC|AC) table"),
        "segment past the end": (base[:find(base, 0xDB)[0] + 20], "ends inside a marker segment"),
    }
    for kind, (data, text) in corrupt.items():
        with pytest.raises(J.CorruptJpeg, match=text):
            J.decode_jpeg(data, "cpu")              # fallback=True: corrupt data still raises
    # a coefficient index past 63: an AC table whose only symbol is run 15 / size 1
    data = coefficient_overrun_stream()
    with pytest.raises(J.CorruptJpeg, match="coefficient index past 63"):
        J.decode_jpeg(data, "cpu")
    # truncation: inside the headers, in the middle of the scan, and with the last data byte missing
    n = len(base)
    for cut, text in ((find(base, 0xC4)[0] + 7, "ends"), ((scan + n) // 2, "before the last MCU"),
                      (n - 3, "before the last MCU")):
        with pytest.raises(J.CorruptJpeg, match=text):
            J.decode_jpeg(base[:cut], "cpu")
    # restart markers: a missing one and one out of order
    rst = stream(cases, next(n for n in names(cases) if n.startswith("16x16_s") and not n.endswith("r0")))
    at = rst.index(b"\xff\xd0", find(rst, 0xDA)[0])
    with pytest.raises(J.CorruptJpeg, match="out of order"):
        J.decode_jpeg(rst[:at + 1] + b"\xd3" + rst[at + 2:], "cpu")
    with pytest.raises(J.CorruptJpeg):
        J.decode_jpeg(rst[:at] + rst[at + 2:], "cpu")


def coefficient_overrun_stream() -> bytes:
    """8 x 8 grayscale, hand-assembled: DC table with one symbol (category 0), AC table with one symbol 0xF1 (run 15,
    size 1): the fifth AC symbol of the block lands on index 64 + ."""
    dqt = b"\xff\xdb\x00\x43\x00" + bytes([1] * 64)
    sof = b"\xff\xc0\x00\x0b\x08\x00\x08\x00\x08\x01\x01\x11\x00"
    dht_dc = b"\xff\xc4\x00\x14\x00" + bytes([1] + [0] * 15) + b"\x00"
    dht_ac = b"\xff\xc4\x00\x14\x10" + bytes([1] + [0] * 15) + b"\xf1"
    sos = b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    return b"\xff\xd8" + dqt + sof + dht_dc + dht_ac + sos + b"\x00" * 8 + b"\xff\xd9"


def test_fallback_decodes_unsupported_streams_with_pillow(jpeg_lib, cases):
    pytest.importorskip("PIL.Image")
    got = J.decode_jpeg(stream(cases, "progressive"), "cpu", fallback=True)
    assert np.array_equal(got.numpy(), cases["rgb_progressive"])
    assert np.array_equal(J.decode_jpeg(stream(cases, "progressive"), "cpu", bgr=True).numpy(),
                          cases["rgb_progressive"][..., ::-1])
    assert np.array_equal(J.decode_jpeg(stream(cases, "cmyk"), "cpu").numpy(), cases["rgb_cmyk"])
    both = J.decode_jpegs([stream(cases, "clip_0"), stream(cases, "progressive")], "cpu")
    assert isinstance(both, list) and np.array_equal(both[1].numpy(), cases["rgb_progressive"])
    assert np.array_equal(both[0].numpy(), cases["rgb_clip_0"])


# ------------------------------------------------------------------------------------ C ABI
def test_library_exports_what_the_header_declares(jpeg_lib):
    syms = assert_binding_matches_header(jpeg_lib, "jpeg_ops_hip.h", "jpegops", "JPEGOPS_ABI_VERSION")
    assert syms == ["jpegops_abi_version", "jpegops_decode_pixels_u8", "jpegops_entropy_decode",
                    "jpegops_entropy_decode_batch", "jpegops_last_error", "jpegops_parse_header",
                    "jpegops_planes_bytes"]
    define = partial(cabi_helpers.define, "jpeg_ops_hip.h")
    assert jpeg_lib.ABI_VERSION == 1
    assert define("JPEGOPS_UNSUPPORTED") == jpeg_lib.UNSUPPORTED
    assert define("JPEGOPS_ERR_LEN") == jpeg_lib.ERR_LEN
    assert define("JPEGOPS_MAX_THREADS") == jpeg_lib.MAX_THREADS == 16
    assert define("JPEGOPS_QT_WORDS") == jpeg_lib.QT_WORDS == J.QT_WORDS
    assert (define("JPEGOPS_TILE_X"), define("JPEGOPS_TILE_Y")) == (jpeg_lib.TILE_X, jpeg_lib.TILE_Y)
    fields = re.search(r"typedef struct jpegops_info \{(.*?)\}", cabi_helpers.header_text("jpeg_ops_hip.h"),
                       flags=re.S).group(1)
    declared = [re.sub(r"\[\d+\]", "", f.strip()) for line in fields.split(";") if line.strip()
                for f in line.strip().split(" ", 1)[1].split(",")]
    assert declared == [f[0] for f in jpeg_lib.Info._fields_]
    assert ctypes.sizeof(jpeg_lib.Info) == 112


def test_bad_arguments_give_error_codes_without_a_device(jpeg_lib, cases):
    lib, err = jpeg_lib.lib, jpeg_lib.lib.jpegops_last_error
    data = cases["jpg_clip_0"]
    info = jpeg_lib.Info()
    assert lib.jpegops_parse_header(None, 10, ctypes.byref(info)) == 1 and b"null pointer" in err()
    assert lib.jpegops_parse_header(data.ctypes.data, data.size, None) == 1
    assert lib.jpegops_parse_header(data.ctypes.data, data.size, ctypes.byref(info)) == 0 and err() == b""
    coef = np.zeros(info.coef_count, dtype=np.int16)
    qt = np.zeros(192, dtype=np.uint16)
    args = (data.ctypes.data, data.size, ctypes.byref(info), coef.ctypes.data)
    assert lib.jpegops_entropy_decode(*args, coef.nbytes - 2, qt.ctypes.data) == 1 and b"smaller than the image" in err()
    assert lib.jpegops_entropy_decode(*args, coef.nbytes, None) == 1 and b"null pointer" in err()
    assert lib.jpegops_entropy_decode(*args, coef.nbytes, qt.ctypes.data) == 0 and err() == b""
    assert lib.jpegops_planes_bytes(ctypes.byref(info)) == info.coef_count
    assert lib.jpegops_planes_bytes(None) == -1

    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch
    ok = dict(coef=p, cp=info.coef_count + 192, qt=p, info=info, planes=p, pb=10 * info.coef_count, out=p,
              row=3 * 33, frame=3 * 33 * 31, B=2, swap=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.jpegops_decode_pixels_u8(a["coef"], a["cp"], a["qt"], a["cp"], ctypes.byref(a["info"]), a["planes"],
                                            a["pb"], a["out"], a["row"], a["frame"], a["B"], a["swap"], None)

    assert call(B=0) == 0 and err() == b""
    assert call(B=-1) == 2 and b"negative batch" in err()
    assert call(coef=None) == 1 and b"null pointer" in err() and b"jpegops_decode_pixels_u8" in err()
    assert call(coef=ctypes.c_void_p(4098)) == 3 and b"aligned" in err()
    assert call(cp=info.coef_count + 191) == 3 and b"multiple of 8" in err()
    assert call(cp=info.coef_count - 64) == 4
    assert call(pb=2 * info.coef_count - 1) == 5 and b"workspace" in err()
    assert call(row=3 * 33 - 1) == 6 and b"row pitch" in err()
    assert call(frame=3 * 33 * 30) == 6 and b"overlap" in err()
    assert call(swap=2) == 7
    assert call(B=65536, pb=1 << 40) == 8
    broken = jpeg_lib.Info.from_buffer_copy(info)
    broken.mcus_x += 1
    assert call(info=broken) == 2 and b"MCU counts" in err()
    broken = jpeg_lib.Info.from_buffer_copy(info)
    broken.hmax = 4
    assert call(info=broken) == 2 and b"sampling" in err()
    with pytest.raises(RuntimeError, match="null pointer"):
        jpeg_lib.check(call(out=None), "jpegops_decode_pixels_u8")

    T = 3
    status = (ctypes.c_int * T)()
    assert lib.jpegops_entropy_decode_batch(None, None, T, None, None, None, None, status, None, 4) == -1
    assert lib.jpegops_entropy_decode_batch(None, None, 0, None, None, None, None, None, None, 4) == 0
    with pytest.raises(J.CorruptJpeg, match="frame 1: .*before the last MCU"):
        J.decode_jpegs([data, data[:data.size - 40], data], "cpu", threads=64)


def test_a_cuda_decode_has_no_substitute_for_the_library():
    import inspect
    src = inspect.getsource(J._device_stage)
    assert "L.check(L.lib.jpegops_decode_pixels_u8(" in src and "except" not in src


# ------------------------------------------------------------------------------------ memory safety of the parser
def test_parser_is_memory_safe_on_hostile_input(cases, tmp_path):
    """tests/native/jpeg_entropy_fuzz.cpp under AddressSanitizer and UBSan, a process of its own: every fixture stream
    whole, every prefix of the two smallest, 2,000 single-byte corruptions of each."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "jpeg_entropy_fuzz"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined",
                            os.path.join(ROOT, "tests", "native", "jpeg_entropy_fuzz.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    streams = tmp_path / "streams"
    streams.mkdir()
    for n in names(cases):
        (streams / f"ok_{n}.jpg").write_bytes(stream(cases, n))
    for n in ("progressive", "cmyk"):
        (streams / f"refused_{n}.jpg").write_bytes(stream(cases, n))
    (streams / "refused_overrun.jpg").write_bytes(coefficient_overrun_stream())
    run = subprocess.run([str(exe), str(streams)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stderr == ""
    m = re.match(r"streams 52: whole ok 49 errors 3; prefixes ok (\d+) errors (\d+); corruptions ok (\d+) errors (\d+)",
                 run.stdout)
    assert m, run.stdout
    assert int(m.group(2)) > 0 and int(m.group(3)) + int(m.group(4)) == 52 * 2000
