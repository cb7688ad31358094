"""Writes tests/golden/track_draw_scene.npz: a rendered track overlay, pinned so that the definition
(memotr_amd/render.py draw_tracks_host) cannot drift unseen.

    python tests/golden/gen_golden_track_draw.py

``frame`` (64, 96, 3) uint8 noise; ``ids`` / ``boxes`` (xyxy, float32): boxes inside, across the edges, overlapping,
inverted and off the frame, tabs above, inside and shifted left; ``table`` the int32 table ``track_table`` makes of
them; per option set k: ``options_k`` = (bgr, thickness, font_scale, fill_alpha) and ``expected_k`` the drawn frame.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

OPTIONS = [(0, 2, 1, 0), (1, 1, 2, 128), (0, 3, 1, 255)]


def main():
    from conftest import save_npz
    from memotr_amd.render import draw_tracks_host, track_table
    rng = np.random.default_rng(77)
    frame = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    ids = np.array([0, 7, 10, 12345678, 2 ** 31 - 1, 63, 64, 5, 9], dtype=np.int64)
    boxes = np.array([[10.2, 12.7, 40.5, 50.4], [30, 20, 70, 60], [-5, 30, 12, 70], [60, 3, 100, 30],
                      [20.5, 40.5, 90.5, 62.5], [50, 30, 40, 35], [200, 10, 220, 30], [80, 45, 82, 60],
                      [45, 25, 45, 25]], dtype=np.float32)
    arrays = dict(frame=frame, ids=ids, boxes=boxes, table=track_table(ids, boxes, 96, 64))
    for k, (bgr, t, s, a) in enumerate(OPTIONS):
        arrays[f"options_{k}"] = np.array([bgr, t, s, a], dtype=np.int32)
        arrays[f"expected_{k}"] = draw_tracks_host(frame, ids, boxes, bgr=bool(bgr), thickness=t, font_scale=s,
                                                   fill_alpha=a)
    path = os.path.join(OUT, "track_draw_scene.npz")
    save_npz(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
