"""Writes tests/golden/jpeg_cases.npz: JPEG byte streams and Pillow's decode of the same bytes, the truth the JPEG
decoder (memotr_amd/data/jpeg.py, csrc/jpeg_ops.hip) is held to.  Needs PIL; the tests that read the fixture do not.

    python tests/golden/gen_golden_jpeg.py

Per case ``jpg_<name>`` (uint8 stream) and ``rgb_<name>`` (``np.asarray(Image.open(...).convert("RGB"))``);
``names`` lists the cases the decoder must read, ``versions`` holds the Pillow and libjpeg-turbo versions.  Images are
deterministic from a seed: smooth gradients, hard edges and noise, so DC-only blocks and full blocks both occur.

Cases (the cross product size x sampling x quality x restart interval, pruned: every size meets every sampling mode,
and quality and restart interval rotate so that each of their values meets every size and every mode):
  sizes 1x1 5x7 8x8 16x16 17x17 31x33 40x48 8x300 300x8; Pillow subsampling 0, 1, 2 and mode "L"; quality 30, 75,
  100; restart_marker_blocks absent, 1, 3.
  tiles_*   150 x 210, one per sampling mode: more than three 64 x 16 workgroup tiles of the colour kernel each way,
            neither size a multiple of 16.
  clip_*    three 31 x 33 4:2:0 frames; track_* four 64 x 96 frames (SequenceTracker.track_jpeg).
  patched_dqt   a quality-100 noise image whose DQT payload bytes are overwritten with 255: the IDCT leaves 0..255 by
            hundreds of levels (-750 .. 1055).  The noise is 3 levels wide so that every dequantised value and every intermediate of
            libjpeg-turbo's SIMD IDCT stays inside 16 bits: beyond that its SIMD and C paths differ from each other
            and there is no single truth.  Pillow's bytes show a clamp here, not the wrap of libjpeg's
            range-limit table -- asserted below.
  com_dqt16     hand-assembled from an 8-bit stream: a COM segment behind SOI, SOF1 instead of SOF0, both DQT tables
            rewritten with 16-bit entries (some above 255).
  progressive, cmyk   streams the decoder refuses (and Pillow reads: the fallback's truth).
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz

SIZES = [(1, 1), (5, 7), (8, 8), (16, 16), (17, 17), (31, 33), (40, 48), (8, 300), (300, 8)]      # (height, width)
MODES = [0, 1, 2, "L"]
QUALITIES = [30, 75, 100]
RESTARTS = [None, 1, 3]


def image(h, w, seed, noise=40, noise_from=0.5):
    """(h, w, 3) uint8: three gradients, darkened in a 5 x 7 checker pattern (hard edges), noise right of
    ``noise_from`` of the width."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(w + h - 2, 1)], -1)
    base[(x // 5 + y // 7) % 2 == 0] *= 0.3
    base += rng.integers(-noise, noise + 1, (h, w, 3)) * (x >= w * noise_from)[..., None]
    return np.clip(base, 0, 255).astype(np.uint8)


def encode(pixels, mode, quality, restart=None, **kw):
    im = Image.fromarray(pixels)
    if mode == "L":
        im = im.convert("L")
    else:
        kw["subsampling"] = mode
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def segments(data):
    """(marker, start of the segment's 0xFF, length including the marker) up to and including SOS."""
    i = 2
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        yield m, i, n + 2
        if m == 0xDA:
            return
        i += n + 2


def patch_dqt(data, value=255):
    b = bytearray(data)
    for m, i, n in segments(data):
        if m == 0xDB:
            j = i + 4
            while j < i + n:
                assert b[j] >> 4 == 0
                b[j + 1:j + 65] = bytes([value]) * 64
                j += 65
    return bytes(b)


def com_and_dqt16(data):
    """COM behind SOI, SOF0 -> SOF1, every DQT table rewritten with 16-bit entries; odd entries get 256 added."""
    out = bytearray(data[:2])
    text = b"memotr_amd test stream"
    out += b"\xff\xfe" + (len(text) + 2).to_bytes(2, "big") + text
    end = 0
    for m, i, n in segments(data):
        seg = bytearray(data[i:i + n])
        if m == 0xDB:
            body, j = bytearray(), 4
            while j < n:
                assert seg[j] >> 4 == 0
                body.append(0x10 | (seg[j] & 15))
                for k in range(64):
                    body += (seg[j + 1 + k] + (256 if k % 2 else 0)).to_bytes(2, "big")
                j += 65
            seg = bytearray(b"\xff\xdb") + (len(body) + 2).to_bytes(2, "big") + body
        elif m == 0xC0:
            seg[1] = 0xC1
        out += seg
        end = i + n
    return bytes(out + data[end:])


def main():
    from conftest import save_npz
    arrays, names = {}, []

    def add(name, data, listed=True):
        arrays["jpg_" + name] = np.frombuffer(data, dtype=np.uint8).copy()
        arrays["rgb_" + name] = pillow_rgb(data)
        if listed:
            names.append(name)

    k = 0
    for si, (h, w) in enumerate(SIZES):
        for mi, mode in enumerate(MODES):
            quality = QUALITIES[(si + mi) % 3]
            restart = RESTARTS[(si + 2 * mi + si // 3) % 3]
            name = f"{h}x{w}_s{mode}_q{quality}_r{restart or 0}"
            add(name, encode(image(h, w, seed=k), mode, quality, restart))
            k += 1
    for mode in MODES:
        add(f"tiles_s{mode}", encode(image(150, 210, seed=100, noise=25, noise_from=0.75), mode, 75, 5))
    for i in range(3):
        add(f"clip_{i}", encode(image(31, 33, seed=200 + i), 2, 90))
    for i in range(4):
        add(f"track_{i}", encode(image(64, 96, seed=300 + i), 2, 90))

    rng = np.random.default_rng(7)
    noise = np.clip(128 + rng.integers(-3, 4, (24, 40, 3)), 0, 255).astype(np.uint8)
    patched = patch_dqt(encode(noise, 2, 100))
    add("patched_dqt", patched)
    add("com_dqt16", com_and_dqt16(encode(image(40, 48, seed=400), 1, 50, 2)))
    add("progressive", encode(image(31, 33, seed=500), 2, 75, progressive=True), listed=False)
    buf = io.BytesIO()
    Image.fromarray(image(17, 17, seed=501)).convert("CMYK").save(buf, "JPEG", quality=75)
    add("cmyk", buf.getvalue(), listed=False)

    # the patched stream is far outside 0..255 and Pillow clamps there: libjpeg's range-limit table would wrap
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from memotr_amd.data import jpeg as J
    c = J.entropy_decode(patched)
    d = c.components[0].numpy().astype(np.int64) * c.qt.numpy()[0].reshape(8, 8)
    levels = J._idct_1d(J._idct_1d(d.swapaxes(-1, -2), 11).swapaxes(-1, -2), 18) + 128
    # (the table maps v = level - 128 through its low 10 bits: 512 .. 895 to 0, 896 .. 1023 to 0 .. 127, where a clamp gives 255)
    assert levels.max() > 128 + 511 and levels.min() < 128 - 512, (levels.min(), levels.max())
    assert np.abs(d).sum(axis=2).max() * 4 * 1.5 < 32767          # pass-1 results stay inside 16 bits
    got = {n: J.decode_jpeg(arrays["jpg_" + n].tobytes(), "cpu", fallback=False).numpy() for n in names}
    for n in names:
        assert np.array_equal(got[n], arrays["rgb_" + n]), n

    arrays["names"] = np.array(names)
    arrays["versions"] = np.array([f"Pillow {PIL.__version__}",
                                   f"libjpeg-turbo {features.version_feature('libjpeg_turbo')}"])
    path = os.path.join(OUT, "jpeg_cases.npz")
    save_npz(path, **arrays)
    print(len(names), "cases,", sum(a.nbytes for a in arrays.values()), "bytes raw,", os.path.getsize(path), "on disk")


if __name__ == "__main__":
    main()
