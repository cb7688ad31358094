"""The small dataset trees of the dataset and clip-loader tests, and of tests/golden/gen_golden_datasets.py (test
infrastructure).  ``write_trees(root)`` builds, under ``root``, one DATA_ROOT holding

  * ``DanceTrack/train``: two sequences of 7 and 5 frames with a gap-free gt.txt (written in an order that is not the
    sorted one: ``vid_idx`` must not depend on it);
  * ``MOT17/{images,gts}/train``: two ``SDP`` sequences (one frame of the first has no gt file) and one ``DPM``
    sequence that must be ignored; ``CrowdHuman/{images,gts}/val``: three images;
  * ``BDD100K``: two sequences, one with a missing gt file in the middle, one with an empty gt file.

The boxes are a function of the names below; every number is written with two decimals (MOT17: some with a fraction
that the reader truncates).  Images are written by ``write_image(path, index)``; the default writes 48 x 80 frames with
the project's own JPEG encoder (``frame_pixels``: smooth content with mild noise, about 1-2 kB at quality 90).
"""
import os

import numpy as np

DANCE_CONFIG = dict(DATASET="DanceTrack", SAMPLE_STEPS=[2, 4], SAMPLE_LENGTHS=[2, 3, 4],
                    SAMPLE_MODES=["random_interval"], SAMPLE_INTERVALS=[3, 2], COCO_SIZE=False, OVERFLOW_BBOX=False,
                    REVERSE_CLIP=0.5, SEED=7)
MOT_CONFIG = dict(DATASET="MOT17", SAMPLE_STEPS=[3], SAMPLE_LENGTHS=[2, 3], SAMPLE_MODES=["random_interval"],
                  SAMPLE_INTERVALS=[3], SAMPLE_MOT17_JOIN=1, USE_CROWDHUMAN=True, USE_MOTSYNTH=None, MOTSYNTH_RATE=None,
                  COCO_SIZE=True, OVERFLOW_BBOX=True, REVERSE_CLIP=0.0, SEED=7)
BDD_CONFIG = dict(DATASET="BDD100K", SAMPLE_STEPS=[1, 2], SAMPLE_LENGTHS=[2, 3, 3], SAMPLE_MODES=["random_interval"],
                  SAMPLE_INTERVALS=[2, 2, 2], SEED=7)

DANCE_SEQS = {"dancetrack0007": 7, "dancetrack0002": 5}                 # name -> frames 1 .. n (written in this order)
MOT_SEQS = {"MOT17-04-SDP": 6, "MOT17-02-SDP": 5, "MOT17-02-DPM": 4}
MOT_NO_GT = ("MOT17-04-SDP", 3)                                         # this frame has no gt file
CROWDHUMAN = ("273278,c9db000d5146c15", "273271,1017c000ac1360b7", "282555,b9a6000f1c27c5e")
BDD_SEQS = {"b1c81faa-3df17267": 6, "b1c66a42-6f7d68ca": 5}
BDD_MISSING = ("b1c81faa-3df17267", 4)                                  # no gt file
BDD_EMPTY = ("b1c66a42-6f7d68ca", 3)                                    # a gt file without a line
SEEDS = (0, 1)
HEIGHT, WIDTH = 48, 80


def epochs_of(config):
    """Epoch 0 and both sides of every stage boundary (and of SAMPLE_MOT17_JOIN)."""
    marks = list(config["SAMPLE_STEPS"]) + [config.get("SAMPLE_MOT17_JOIN", 0)]
    return sorted({0} | {e for m in marks for e in (m - 1, m, m + 1) if e >= 0})


def boxes_of(name, t, integers=False):
    """[(class, id, x, y, w, h)]: 1 to 3 objects that drift with ``t``; the same ids along a sequence."""
    rs = np.random.RandomState(sum(name.encode()) % 10007)
    n = 1 + rs.randint(0, 3)
    base = rs.uniform(0, 1, (n, 4))
    out = []
    for k in range(n):
        if (t + k) % 5 == 0 and n > 1:
            continue                                                    # an object that is absent now and then
        x, y = 4 + 40 * base[k, 0] + 1.25 * t, 3 + 20 * base[k, 1] + 0.75 * t
        w, h = 6 + 20 * base[k, 2], 5 + 15 * base[k, 3]
        if integers:
            x, y, w, h = int(x), int(y), int(w), int(h)
        out.append((1 + (k + len(name)) % 8, k + 1, x, y, w, h))
    return out


def frame_pixels(index, h=HEIGHT, w=WIDTH):
    yy, xx = np.mgrid[0:h, 0:w]
    rs = np.random.RandomState(1000 + index)
    px = np.stack([(xx * 2 + index * 7) % 256, (yy * 4 + index * 3) % 256, ((xx + yy) * 2 + 40) % 256], -1)
    return np.clip(px + rs.randint(-6, 7, px.shape), 0, 255).astype(np.uint8)


def default_write_image(path, index):
    import torch

    from memotr_amd.data import encode_jpeg
    with open(path, "wb") as f:
        f.write(encode_jpeg(torch.from_numpy(frame_pixels(index)), quality=90, subsampling="4:2:0"))


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def write_trees(root, write_image=default_write_image, only=("DanceTrack", "MOT17", "BDD100K")):
    """Returns ``root`` (the DATA_ROOT)."""
    counter = [0]

    def image(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        write_image(path, counter[0])
        counter[0] += 1

    if "DanceTrack" in only:
        for vid, n in DANCE_SEQS.items():
            lines = []
            for t in range(1, n + 1):
                image(os.path.join(root, "DanceTrack", "train", vid, "img1", f"{t:08d}.jpg"))
                lines += [f"{t},{i},{x:.2f},{y:.2f},{w:.2f},{h:.2f},1,1,1\n" for _, i, x, y, w, h in boxes_of(vid, t)]
            _write(os.path.join(root, "DanceTrack", "train", vid, "gt", "gt.txt"), "".join(lines))
    if "MOT17" in only:
        for vid, n in MOT_SEQS.items():
            for t in range(1, n + 1):
                image(os.path.join(root, "MOT17", "images", "train", vid, "img1", f"{t:06d}.jpg"))
                if (vid, t) == MOT_NO_GT:
                    continue
                lines = [f"0 {i} {x:.2f} {y:.2f} {w:.2f} {h:.2f} 1.0\n" for _, i, x, y, w, h in boxes_of(vid, t)]
                _write(os.path.join(root, "MOT17", "gts", "train", vid, "img1", f"{t:06d}.txt"), "".join(lines))
        for name in CROWDHUMAN:
            image(os.path.join(root, "CrowdHuman", "images", "val", f"{name}.jpg"))
            lines = [f"0 {i} {x} {y} {w} {h}\n" for _, i, x, y, w, h in boxes_of(name, 1, integers=True)]
            _write(os.path.join(root, "CrowdHuman", "gts", "val", f"{name}.txt"), "".join(lines))
    if "BDD100K" in only:
        for vid, n in BDD_SEQS.items():
            for t in range(1, n + 1):
                image(os.path.join(root, "BDD100K", "images", "track", "train", vid, f"{vid}-{t:07d}.jpg"))
                if (vid, t) == BDD_MISSING:
                    continue
                lines = [] if (vid, t) == BDD_EMPTY else [
                    f"{c} {i} {x:.2f} {y:.2f} {w:.2f} {h:.2f}\n" for c, i, x, y, w, h in boxes_of(vid, t)]
                _write(os.path.join(root, "BDD100K", "filter_labels", "track", "train", vid, f"{vid}-{t:07d}.txt"),
                       "".join(lines))
    return root
