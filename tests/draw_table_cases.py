"""Shared by tests/test_draw_table_cpu.py and tests/test_draw_table_gpu.py: banks of slots for ``clip_ops.draw_table``
and the statement it is held to, written out from the parts it is defined by.

A case is ``(boxes (B, cap, 4) cxcywh normalised, scores (B, cap, K), ids (B, cap), ori_wh (B, 2), score_thresh,
area_thresh)``.  A slot is ``(id, (cx, cy, w, h), scores)``; ``FREE`` is a free slot.
"""
import numpy as np
import torch

NAN = float("nan")
FREE = (-1, (0.0, 0.0, 0.0, 0.0), 0.0)
DIGIT_IDS = [0, 9, 10, 63, 64, 99999999, 100000000, 2 ** 31 - 1]
VARIANTS = [(False, 1), (True, 1), (False, 3), (True, 3)]             # (bgr, font_scale)


def pack(streams, ori, K=1, score_thresh=0.5, area_thresh=10.0):
    B, cap = len(streams), len(streams[0])
    boxes, scores = torch.zeros((B, cap, 4)), torch.zeros((B, cap, K))
    ids = torch.full((B, cap), -1, dtype=torch.int64)
    for b, slots in enumerate(streams):
        assert len(slots) == cap
        for s, (tid, box, sc) in enumerate(slots):
            ids[b, s] = tid
            boxes[b, s] = torch.tensor(box, dtype=torch.float32)
            scores[b, s] = torch.tensor(sc, dtype=torch.float32)      # (a scalar fills the K columns)
    return boxes, scores, ids, torch.tensor(ori, dtype=torch.float32), score_thresh, area_thresh


def px(x1, y1, x2, y2, W=96, H=64):
    """A cxcywh normalised box from pixel corners (rounded as float64 -> float32: where the corners land is the
    statement's business, not this helper's)."""
    return ((x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H)


def named_cases():
    good = px(10, 20, 50, 60)
    cases = {}
    cases["holes_out_of_order"] = pack([[(5, px(4, 14, 40, 50), 0.9), FREE, (2, px(20, 22, 70, 60), 0.8),
                                         (9, px(30, 12, 90, 40), 0.7), FREE, (0, good, 0.95), (7, px(1, 30, 30, 63), 0.6),
                                         FREE]], [(96, 64)])
    cases["all_free"] = pack([[FREE] * 4], [(96, 64)])
    cases["all_kept"] = pack([[(4 - i, px(5 + 9 * i, 12 + 3 * i, 40 + 9 * i, 40 + 4 * i), 0.9) for i in range(5)]],
                             [(96, 64)])
    cases["one_class"] = pack([[(3, good, 0.51), (1, good, 0.49), (2, px(30, 30, 60, 60), 0.7)]], [(96, 64)], K=1)
    low = [0.1] * 8
    cases["eight_classes"] = pack([[(1, good, low[:5] + [0.9] + low[6:]), (0, px(40, 20, 80, 50), low),
                                    (2, px(30, 30, 60, 60), [0.8] + low[1:]), (3, good, low[:7] + [0.6])]],
                                  [(96, 64)], K=8)
    # 64 x 32: w = h = 0.25 has the area 0.25 * 64 * 0.25 * 32 = 128 exactly; 0.5 is a float32
    cases["strict_thresholds"] = pack([[(0, (0.5, 0.5, 0.25, 0.25), 0.9), (1, (0.5, 0.5, 0.5, 0.5), 0.5),
                                        (2, (0.5, 0.5, 0.125, 0.25), 0.9), (3, (0.25, 0.5, 0.5, 0.5), 0.75)]], [(64, 32)],
                                      score_thresh=0.5, area_thresh=128.0)
    cases["nan"] = pack([[(0, good, [0.9, NAN, 0.1]), (1, good, [NAN, 0.9, 0.9]), (2, (0.5, 0.5, NAN, 0.5), 0.9),
                          (3, (0.5, 0.5, 0.5, NAN), 0.9), (4, (NAN, 0.5, 0.3, 0.5), 0.9), (5, (0.5, NAN, 0.3, 0.5), 0.9),
                          (6, good, 0.9)]], [(96, 64)], K=3)
    # 64 x 32 and dyadic boxes: (cx -+ w / 2) * 64 is exact, and the corners are k + 0.5
    cases["half_pixel_ties"] = pack([[(0, (12.5 / 64, 16.5 / 32, 8 / 64, 8 / 32), 0.9),
                                      (1, (40.25 / 64, 10.75 / 32, 16.5 / 64, 4.5 / 32), 0.9),
                                      (2, (3.5 / 64, 20.5 / 32, 8 / 64, 16 / 32), 0.9),          # x1 = -0.5
                                      (3, (0.5, 0.5, 63 / 64, 31 / 32), 0.9)]], [(64, 32)])
    cases["off_frame"] = pack([[(0, px(-20, -10, 30, 40), 0.9), (1, px(60, 30, 130, 90), 0.9),
                                (2, px(-50, -50, -10, -10), 0.9), (3, px(100, 70, 140, 110), 0.9),
                                (4, px(-5, -5, 101, 69), 0.9)]], [(96, 64)])
    cases["tabs"] = pack([[(12345, px(10, 3, 50, 40), 0.9), (777, px(80, 20, 95, 60), 0.9),
                           (2 ** 31 - 1, px(70, 2, 94, 30), 0.9), (8, px(10, 9, 30, 30), 0.9),
                           (6, px(12, 8, 30, 30), 0.9)]], [(96, 64)])
    cases["digits"] = pack([[(tid, px(2 + 10 * i, 11 + 5 * i, 30 + 8 * i, 30 + 4 * i), 0.9)
                             for i, tid in enumerate(DIGIT_IDS)]], [(96, 64)])
    cases["two_streams"] = pack([[(3, good, 0.9), FREE, (1, px(30, 12, 90, 40), 0.8), (64, px(40, 30, 80, 50), 0.7)],
                                 [FREE, (2, good, 0.9), (0, px(30, 12, 90, 40), 0.3), (10, px(40, 30, 80, 50), 0.7)]],
                                [(96, 64), (50, 40)])
    return cases


def random_case(B, cap, seed=0, W=160, H=120):
    """Random slots: about a quarter free, ids a random permutation (so ranks interleave across any chunk boundary),
    some scores and areas below the thresholds."""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(4 * cap)[:cap] for _ in range(B)]).astype(np.int64)
    ids[rng.random((B, cap)) < 0.25] = -1
    wh = rng.uniform(0.01, 0.5, (B, cap, 2))
    boxes = np.concatenate((rng.uniform(-0.1, 1.1, (B, cap, 2)), wh), axis=2).astype(np.float32)
    scores = rng.uniform(0.2, 1.0, (B, cap, 2)).astype(np.float32)
    free = ids < 0
    boxes[free], scores[free] = 0, 0
    ori = [(W - 7 * b, H + 5 * b) for b in range(B)]
    return (torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(ids),
            torch.tensor(ori, dtype=torch.float32), 0.5, 40.0)


def draw_case(kept, cap, W=65, H=17, seed=3):
    """One stream of ``kept`` reportable slots among ``cap`` on a W x H frame (ragged against the overlay's 64 x 16
    tile), in random slot order."""
    rng = np.random.default_rng(seed)
    slots = rng.permutation(cap)[:kept]
    ids = np.full((1, cap), -1, dtype=np.int64)
    ids[0, slots] = rng.permutation(3 * cap)[:kept]
    boxes = np.zeros((1, cap, 4), dtype=np.float32)
    boxes[0, slots, :2] = rng.uniform(0.0, 1.0, (kept, 2))
    boxes[0, slots, 2:] = rng.uniform(0.2, 0.7, (kept, 2))
    scores = np.zeros((1, cap, 1), dtype=np.float32)
    scores[0, slots] = 0.9
    return (torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(ids),
            torch.tensor([(W, H)], dtype=torch.float32), 0.5, 1.0)


def statement(boxes, scores, ids, ori_wh, score_thresh, area_thresh, bgr=False, font_scale=1):
    """``track_table(host_rows(...) sorted by id)`` and the padding rows, stream by stream: ``(table (B, cap, 16) int32
    numpy, kept rows per stream)``."""
    from memotr_amd.render import track_table
    from memotr_amd.results import host_rows
    B, cap = ids.shape
    table = np.zeros((B, cap, 16), dtype=np.int32)
    table[:, :, 2:4] = -1
    kept = []
    for b in range(B):
        live = ids[b] >= 0
        W, H = (int(v) for v in ori_wh[b])
        rows_f, rows_i = host_rows(boxes[b][live], scores[b][live], ids[b][live], torch.zeros_like(ids[b][live]), 0,
                                   H, W, score_thresh, area_thresh)
        order = np.argsort(rows_i[:, 1].numpy(), kind="stable")
        table[b, :len(order)] = track_table(rows_i[:, 1].numpy()[order], rows_f[:, :4].numpy()[order], W, H, bgr=bgr,
                                            font_scale=font_scale)
        kept.append(len(order))
    return table, kept
