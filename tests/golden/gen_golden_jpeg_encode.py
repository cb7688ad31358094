"""Writes tests/golden/jpeg_encode_cases.npz: source images and the bytes Pillow (libjpeg-turbo) writes for them, the
truth the JPEG encoder (memotr_amd/data/jpeg_write.py, csrc/jpeg_enc.hip, csrc/jpeg_encode_core.h) is held to.  Needs
PIL; the tests that read the fixture do not.

    python tests/golden/gen_golden_jpeg_encode.py

``img_<H>x<W>_<kind>``: (H, W, 3) uint8 source images, deterministic from a seed.  ``streams``: all files end to end;
``stream_names[i]`` = ``<H>x<W>_<kind>_q<quality>_s<0|2>`` is ``streams[stream_offsets[i]:stream_offsets[i + 1]]`` =
``Image.fromarray(img).save(f, "JPEG", quality=quality, subsampling=0 | 2)``.  ``versions``: Pillow and libjpeg-turbo.

  sizes (H, W)  1x1 2x2 8x8 8x9 16x16 17x33 24x16 40x36 31x47 50x70 64x96 8x300 300x8.  24x16 and 40x36 have an even
                height that is no multiple of 16: the block rows below the image replicate the last DOWNSAMPLED chroma
                row; 8x9 has a dummy luma row and a dummy column at once; 8x300 and 300x8 cross workgroup tiles.
  kinds         noise; smooth (a gradient per channel); sat (every byte 0 or 255: the FDCT's largest intermediates).
  qualities     10 50 75 95 100 below 1500 pixels; 10 75 100 on the four larger sizes (the file stays a few hundred KB).
  sampling      4:4:4 (0) and 4:2:0 (2), every size, kind and quality.
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz

SIZES = [(1, 1), (2, 2), (8, 8), (8, 9), (16, 16), (17, 33), (24, 16), (40, 36), (31, 47), (50, 70), (64, 96),
         (8, 300), (300, 8)]
KINDS = ["noise", "smooth", "sat"]
QUALITIES = [10, 50, 75, 95, 100]
QUALITIES_LARGE = [10, 75, 100]
LARGE = 1500                                          # pixels from which a size counts as large


def image(h, w, kind, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "sat":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), 255 - (x + y) * 255 // max(w + h - 2, 1)],
                    -1).astype(np.uint8)


def main():
    from conftest import save_npz
    rng = np.random.default_rng(20251018)
    arrays, names, offsets, blob = {}, [], [0], []
    for h, w in SIZES:
        for kind in KINDS:
            px = image(h, w, kind, rng)
            arrays[f"img_{h}x{w}_{kind}"] = px
            for q in (QUALITIES if h * w < LARGE else QUALITIES_LARGE):
                for s in (0, 2):
                    f = io.BytesIO()
                    Image.fromarray(px).save(f, "JPEG", quality=q, subsampling=s)
                    names.append(f"{h}x{w}_{kind}_q{q}_s{s}")
                    blob.append(f.getvalue())
                    offsets.append(offsets[-1] + len(blob[-1]))
    arrays["streams"] = np.frombuffer(b"".join(blob), dtype=np.uint8)
    arrays["stream_names"] = np.array(names)
    arrays["stream_offsets"] = np.array(offsets, dtype=np.int64)
    arrays["versions"] = np.array([PIL.__version__, str(features.version("jpg"))])
    path = os.path.join(OUT, "jpeg_encode_cases.npz")
    save_npz(path, **arrays)
    print(path, len(names), "streams", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
