"""Golden vectors for clips made from one still image (memotr_amd/data/static_clip.py), produced by the REFERENCE's own
``MultiRandomShift`` and transform classes on Pillow images (needs PIL and a checkout of the reference; the tests that
read the fixture need neither):

    python tests/golden/gen_golden_static_shift.py --reference /path/to/reference   ->  tests/golden/static_shift.npz

The reference's ``data/transforms.py`` is imported from that checkout as it is.  What it imports and this project does
not need is stood in for here, in ``sys.modules``, before the import: ``cv2`` (unused on this path), ``utils.box_ops``
(this project's ``box_xyxy_to_cxcywh``) and ``torchvision.transforms`` / ``.functional``, stated with Pillow and torch:
``crop`` is ``Image.crop((l, t, l + w, t + h))``, ``resize`` is ``Image.resize((w, h), BILINEAR)``, ``hflip`` is
``Image.transpose(FLIP_LEFT_RIGHT)``, ``to_tensor`` / ``normalize`` their published formulas, and
``RandomCrop.get_params`` returns the window the case asks for.

``MultiRandomShift`` draws (dx, dy) and its reversal from torch's global generator: for every case a seed is searched
whose draws, replayed here in the transform's order (``rand``, ``randn``, ``rand``, ``randn``, then one ``randn``
after the frames are made), give the case's (dx, dy) (and reversal, where the case asks for one); the transform then
runs under that seed.  That pins pixels AND boxes to the reference's code.  It cannot draw a zero: the two cases with
``dx = 0`` or ``dy = 0`` (torch seed -1 in their spec) restate transforms.py:188-215 with ``Image.crop`` /
``Image.resize`` and carry pixels only.

Only outputs and specs are stored.  The image of a case is regenerated from its seed:
``np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)``; the input infos are small and stored.
Frames are stored in chain order (a reversal the reference drew is undone and recorded in the spec), frame 0, the
image itself, left out.
"""
import argparse
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

MAX_SHIFT = 50                                        # the reference's default
# name -> (image seed, h, w, dx, dy, T)
CASES = {
    "left_down": (1, 67, 45, -7, 5, 5),
    "right_up": (2, 67, 45, 7, -5, 5),
    "one_row_all_black": (3, 51, 20, -50, 50, 4),     # hc = 1 and s >= w
    "one_row_up": (4, 51, 20, -1, -50, 3),
    "black_from_frame_1": (5, 90, 33, -40, 17, 5),    # s >= w
    "right_only_moves_rows": (6, 64, 64, 50, 1, 2),
    "dy_zero": (7, 40, 30, -3, 0, 3),
    "dx_zero": (8, 40, 30, 0, -4, 3),
}
# name -> (image seed, h, w, dx, dy, T, shift reversal, flip, reverse, h1, w1, i, j, c, th, tw, overflow_bbox);
# h1 == 0: the plain branch (one resize to th x tw), else resize to h1 x w1, crop c x c at row i, column j, resize
E2E = {}
for _branch, _geo in (("plain", (0, 0, 0, 0, 0, 80, 54)), ("crop", (90, 60, 11, 7, 40, 64, 48))):
    for _srev in (0, 1):
        for _rev in (0, 1):
            E2E[f"e2e_{_branch}_{_srev}{_rev}"] = (9, 67, 45, -7, -5, 4, _srev, 1 - _srev, _rev) + _geo + (_rev,)

CROP_WINDOW = [None]                                  # what the stand-in RandomCrop.get_params returns


def install_stand_ins():
    from PIL import Image

    from memotr_amd.utils.box_ops import box_xyxy_to_cxcywh

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def crop(img, top, left, height, width):
        return img.crop((left, top, left + width, top + height))

    def resize(img, size):
        h, w = size
        return img.resize((w, h), Image.BILINEAR)

    def hflip(img):
        return img.transpose(Image.FLIP_LEFT_RIGHT)

    def to_tensor(img):
        return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)

    def normalize(t, mean, std):
        return (t - torch.as_tensor(mean)[:, None, None]) / torch.as_tensor(std)[:, None, None]

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            i, j = CROP_WINDOW[0]
            return i, j, output_size[0], output_size[1]

    module("cv2")
    fn = module("torchvision.transforms.functional", crop=crop, resize=resize, hflip=hflip, to_tensor=to_tensor,
                normalize=normalize)
    tr = module("torchvision.transforms", functional=fn, RandomCrop=RandomCrop)
    module("torchvision", transforms=tr)
    module("utils.box_ops", box_xyxy_to_cxcywh=box_xyxy_to_cxcywh)
    module("utils", box_ops=sys.modules["utils.box_ops"])


def load_reference_transforms(reference):
    path = os.path.join(reference, "data", "transforms.py")
    if not os.path.exists(path):
        raise SystemExit(f"{path} does not exist: --reference must name a checkout of the reference")
    install_stand_ins()
    spec = importlib.util.spec_from_file_location("reference_data_transforms", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def replay(seed):
    """(dx, dy, reversal) that ``MultiRandomShift(MAX_SHIFT)`` draws under ``torch.manual_seed(seed)``."""
    torch.manual_seed(seed)
    dx = (MAX_SHIFT * torch.rand(1)).ceil() * ((torch.randn(1) > 0.0).int() * 2 - 1)
    dy = (MAX_SHIFT * torch.rand(1)).ceil() * ((torch.randn(1) > 0.0).int() * 2 - 1)
    return int(dx[0].item()), int(dy[0].item()), int(torch.randn(1)[0].item() > 0)


def find_seed(dx, dy, rev=None, limit=2_000_000):
    for seed in range(limit):
        got = replay(seed)
        if got[:2] == (dx, dy) and (rev is None or got[2] == rev):
            return seed, got[2]
    raise SystemExit(f"no seed below {limit} draws {(dx, dy, rev)}")


def make_input(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def info_variants(h, w):
    """full: a box that leaves through the top when the rows move up, one reaching past the right edge, one in the
    middle, one at the left edge; empty: no box; noboxes: an info the shift leaves alone."""
    boxes = torch.tensor([[0.2 * w, 1.0, 0.6 * w, 8.0], [0.5 * w, 0.3 * h, w + 5.0, 0.6 * h],
                          [0.4 * w, 0.4 * h, 0.55 * w, 0.5 * h], [0.0, 0.55 * h, 6.5, 0.9 * h]], dtype=torch.float32)
    n = len(boxes)
    full = {"boxes": boxes, "ids": torch.arange(n) + 10, "labels": torch.zeros(n, dtype=torch.long),
            "areas": (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])}
    empty = {"boxes": torch.zeros((0, 4)), "ids": torch.zeros((0,), dtype=torch.long),
             "labels": torch.zeros((0,), dtype=torch.long), "areas": torch.zeros((0,))}
    return {"full": full, "empty": empty, "noboxes": {"ids": torch.arange(3)}}


def copy_info(info):
    return {k: v.clone() for k, v in info.items()}


def put_infos(arrays, prefix, infos):
    for k, info in enumerate(infos):
        for field in ("boxes", "ids", "labels", "areas"):
            if field in info:
                arrays[f"{prefix}::{k}::{field}"] = info[field].numpy()


def pillow_restatement(img, T, dx, dy):
    w, h = img.size
    frames = [img]
    for _ in range(1, T):
        y_min, y_max, x_min, x_max = max(0, -dy), min(h, h - dy), max(0, -dx), max(w, w - dx)
        frames.append(frames[-1].crop((x_min, y_min, x_max, y_max)).resize((w, h), resample=2))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its data/transforms.py is read)")
    args = ap.parse_args()
    import PIL
    from PIL import Image

    from conftest import save_npz
    R = load_reference_transforms(args.reference)
    arrays = {"pillow_version": np.array(PIL.__version__)}

    for name, (img_seed, h, w, dx, dy, T) in CASES.items():
        img = Image.fromarray(make_input(img_seed, h, w))
        if dx == 0 or dy == 0:
            seed, rev = -1, 0
            frames = pillow_restatement(img, T, dx, dy)
        else:
            seed, rev = find_seed(dx, dy)
            for variant, info in info_variants(h, w).items():
                torch.manual_seed(seed)
                frames, infos = R.MultiRandomShift(MAX_SHIFT)([img] * T, [copy_info(info) for _ in range(T)])
                if rev:
                    frames, infos = frames[::-1], infos[::-1]
                for field, value in info.items():
                    arrays[f"{name}::in::{variant}::{field}"] = value.numpy()
                put_infos(arrays, f"{name}::info::{variant}", infos)
        assert np.array_equal(np.asarray(frames[0]), np.asarray(img))
        arrays[name + "::spec"] = np.array((img_seed, h, w, dx, dy, T, seed, rev), dtype=np.int64)
        arrays[name] = np.stack([np.asarray(f) for f in frames[1:]])

    for name, spec in E2E.items():
        img_seed, h, w, dx, dy, T, srev, flip, rev, h1, w1, i, j, c, th, tw, overflow = spec
        seed, _ = find_seed(dx, dy, srev)
        info = info_variants(h, w)["full"]
        CROP_WINDOW[0] = (i, j)
        branch = R.MultiRandomResize([[tw, th]])
        if h1:
            branch = R.MultiCompose([R.MultiRandomResize([[w1, h1]]),
                                     R.MultiRandomCrop(min_size=c, max_size=c, overflow_bbox=bool(overflow)), branch])
        chain = R.MultiCompose([R.MultiRandomHorizontalFlip(p=float(flip)), R.MultiRandomShift(MAX_SHIFT), branch,
                                R.MultiToTensor(), R.MultiNormalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]),
                                R.MultiReverseClip(reverse=float(rev))])
        torch.manual_seed(seed)
        random.seed(0)
        img = Image.fromarray(make_input(img_seed, h, w))
        imgs, infos = chain([img] * T, [copy_info(info) for _ in range(T)])
        assert all(tuple(t.shape) == (3, th, tw) for t in imgs)
        arrays[name + "::spec"] = np.array(spec + (seed,), dtype=np.int64)
        for field in ("boxes", "ids", "labels", "areas"):
            arrays[f"{name}::in::{field}"] = info[field].numpy()
        put_infos(arrays, name, list(infos))

    path = os.path.join(OUT, "static_shift.npz")
    save_npz(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "+", len(E2E), "cases, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
