"""Golden vectors for the resize part of the training-clip augmentation (memotr_amd/data/augment.py), produced by
Pillow (needs PIL; the tests that read the fixture do not):

    python tests/golden/gen_golden_augment.py        ->  tests/golden/augment_resample.npz

Every case is a seeded random-noise frame of at most 131 pixels a side through ``Image.resize(..., BILINEAR)``,
optionally mirrored first (``Image.transpose(FLIP_LEFT_RIGHT)``) and optionally as resize -> ``Image.crop`` -> resize.
Only the outputs are stored; the fixture carries each case's numbers (``<name>::spec``) and the input is regenerated
from the seed: ``np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)``.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz

# name -> (seed, h, w, flip, h1, w1, i, j, ch, cw, oh, ow); h1 == 0: one resize to oh x ow, else resize to h1 x w1,
# crop ch x cw at row i, column j, resize to oh x ow
CASES = {
    "down_up": (1, 97, 131, 0, 0, 0, 0, 0, 0, 0, 41, 300),
    "identity_rows": (2, 64, 48, 0, 0, 0, 0, 0, 0, 0, 64, 31),
    "vertical_only": (3, 33, 57, 0, 0, 0, 0, 0, 0, 0, 90, 57),
    "horizontal_only": (4, 33, 57, 0, 0, 0, 0, 0, 0, 0, 33, 90),
    "tiny": (5, 7, 5, 0, 0, 0, 0, 0, 0, 0, 3, 11),
    "identity": (6, 20, 30, 0, 0, 0, 0, 0, 0, 0, 20, 30),
    "down_1p78": (7, 108, 131, 0, 0, 0, 0, 0, 0, 0, 61, 74),
    "down_4p4": (8, 120, 131, 0, 0, 0, 0, 0, 0, 0, 27, 30),
    "flip_down_up": (9, 97, 131, 1, 0, 0, 0, 0, 0, 0, 41, 300),
    "flip_tiny": (10, 7, 5, 1, 0, 0, 0, 0, 0, 0, 3, 11),
    "crop_branch": (11, 72, 128, 0, 90, 160, 7, 13, 61, 75, 66, 81),
    "crop_branch_flip": (12, 72, 128, 1, 90, 160, 7, 13, 61, 75, 66, 81),
    "crop_branch_down": (13, 120, 131, 1, 60, 65, 3, 5, 40, 39, 83, 81),
}


def make_input(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def pil_result(spec):
    from PIL import Image
    seed, h, w, flip, h1, w1, i, j, ch, cw, oh, ow = spec
    img = Image.fromarray(make_input(seed, h, w))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if h1:
        img = img.resize((w1, h1), Image.BILINEAR).crop((j, i, j + cw, i + ch))
    return np.asarray(img.resize((ow, oh), Image.BILINEAR))


def main():
    import PIL
    from conftest import save_npz
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for name, spec in CASES.items():
        arrays[name + "::spec"] = np.array(spec, dtype=np.int64)
        arrays[name] = pil_result(spec)
    path = os.path.join(OUT, "augment_resample.npz")
    save_npz(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
