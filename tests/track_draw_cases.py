"""Shared by tests/test_track_draw_cpu.py and tests/test_track_draw_gpu.py: frames and track lists for the overlay."""
import numpy as np

SIZES = [(37, 53), (64, 96), (16, 300)]                 # (H, W): ragged both ways; one tile exactly; five tiles wide
IDS = [0, 7, 10, 12345678, 2 ** 31 - 1]


def frame(h, w, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def named_boxes(h, w):
    """name -> list of xyxy boxes (floats, some on .5) for an h x w frame."""
    return {
        "inside": [(12.3, 11.6, w - 9.5, h - 3.2)],
        "across_left": [(-6.0, 12.0, 10.4, h - 5.0)],
        "across_right": [(w - 8.0, 10.0, w + 5.0, h - 2.0)],
        "across_top": [(10.0, -5.0, 30.0, 8.0)],
        "across_bottom": [(12.0, h - 6.0, 40.0, h + 7.0)],
        "across_all": [(-3.0, -3.0, w + 3.0, h + 3.0)],
        "outside": [(w + 10.0, 5.0, w + 30.0, 20.0), (-40.0, -40.0, -20.0, -20.0), (5.0, h + 20.0, 30.0, h + 30.0)],
        "inverted": [(30.0, 12.0, 10.0, 15.0), (10.0, 15.0, 30.0, 12.0)],
        "one_pixel": [(20.0, 12.0, 20.0, 12.0)],
        "thin": [(15.0, 10.0, 17.0, h - 2.0), (20.0, 11.0, 45.0, 13.0)],
        "overlap": [(5.0, 10.0, 30.0, h - 4.0), (18.0, 12.0, 44.0, h - 2.0), (10.0, 11.0, 36.0, h - 6.0)],
        "overlap_reversed": [(10.0, 11.0, 36.0, h - 6.0), (18.0, 12.0, 44.0, h - 2.0), (5.0, 10.0, 30.0, h - 4.0)],
        "tab_above": [(8.0, 10.0, 40.0, h - 1.0)],
        "tab_inside": [(8.0, 4.0, 40.0, h - 1.0)],
        "tab_shifted_left": [(w - 12.0, 10.0, w - 2.0, h - 1.0)],
        "huge_and_nan": [(-1e30, -1e9, 1e30, 3e9), (float("nan"), 2.0, 30.0, 14.0)],
    }


def many(h, w, n=70, seed=5):
    """n random boxes, some off the frame, with ids that repeat the edge values."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(-10, w, n)
    y1 = rng.uniform(-10, h, n)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0, w / 2, n), y1 + rng.uniform(0, h / 2, n)], 1).astype(np.float32)
    ids = np.array([IDS[i % 5] if i % 3 == 0 else int(rng.integers(0, 5000)) for i in range(n)], dtype=np.int64)
    return ids, boxes


OPTIONS = [
    dict(),
    dict(thickness=1, font_scale=2, fill_alpha=128),
    dict(thickness=3, fill_alpha=255, bgr=True),
]
