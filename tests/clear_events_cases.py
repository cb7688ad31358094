"""Shared by tests/test_clear_events_cpu.py and tests/test_clear_events_gpu.py: the fixture TrackEval's CLEAR was
recorded into (tests/golden/clear_events.npz), the set of sequences the events kernel is run on, the hand-made
sequence the error table is checked on, and the small tree of files the public interface is run on."""
import os

import numpy as np

import dataset_trees as T
from conftest import load_golden

from memotr_amd import diagnose as D
from memotr_amd import evaluation as E

SETS = {"mot17": "MOT17", "mot15": "MOT15"}
_GOLDEN = {}


def golden(prefix):
    """(arrays, PackedSequences) of one benchmark of the fixture, loaded once and shared."""
    if not _GOLDEN:
        _GOLDEN["all"] = load_golden("clear_events")
    if prefix not in _GOLDEN:
        g = {k[len(prefix) + 2:]: v for k, v in _GOLDEN["all"].items() if k.startswith(prefix + "::")}
        _GOLDEN[prefix] = g, E.PackedSequences([str(n) for n in g["names"]], *[g[k] for k in E.PackedSequences.ARRAYS])
    return _GOLDEN[prefix]


def concat(parts):
    """One-sequence ``PackedSequences`` (host) one behind the other."""
    seq_off = np.concatenate(([0], np.cumsum([p.seq_off[-1] for p in parts]))).astype(np.int32)
    offs = lambda key: np.concatenate(                                                       # noqa: E731
        [[0]] + [getattr(p, key)[1:] + sum(int(getattr(q, key)[-1]) for q in parts[:i]) for i, p in enumerate(parts)]
    ).astype(np.int32)
    cat = lambda key: np.concatenate([getattr(p, key) for p in parts])                       # noqa: E731
    return E.PackedSequences([p.names[0] for p in parts], seq_off, offs("gt_off"), offs("tr_off"), cat("gt_boxes"),
                             cat("tr_boxes"), cat("gt_ids"), cat("tr_ids"), cat("gt_classes"), cat("gt_zero_marked"))


def kernel_set():
    """The fixture's MOT17 sequences in one call, a sequence of three frames without any row between two that have
    rows, the one-frame sequence second to it: what ``clipops_clear_events_f64`` is run on."""
    _, packed = golden("mot17")
    by_name = {n: packed.select(i) for i, n in enumerate(packed.names)}
    none = E.pack_sequences({"empty": {k: [np.zeros((0, 4)) if "boxes" in k else np.zeros(0, np.int64)] * 3
                                       for k in ("gt_ids", "gt_boxes", "tracker_ids", "tracker_boxes")}})
    order = ["edges", none, "one_frame", "wide_65x7", "no_tracker", "tall_70x9", "no_gt", "walk37", "all_distractors",
             "ids150", "walk130"]
    return concat([by_name[x] if isinstance(x, str) else x for x in order])


def has_every_kind(rows):
    """Every kind on both sides, and a frag flag, in ``clear_events_host``'s arrays (or a ``SequenceEvents``)."""
    get = (lambda k: rows[k]) if isinstance(rows, dict) else (lambda k: getattr(rows, k))
    return (set(np.unique(get("gt_kind"))) == {D.IGNORED, D.MATCH, D.SWITCH, D.MISS}
            and set(np.unique(get("tr_kind"))) == {D.IGNORED, D.TP, D.SWITCH, D.FP} and int(get("gt_frag").sum()) > 0)


# ------------------------------------------------------------------------------------------------ the error table
WIDTH, HEIGHT = 96, 64


def table_events():
    """A hand-made ``SequenceEvents`` for a 96 x 64 frame (the kinds are set by hand: the table does not ask where
    they come from).  Frame 0: ids of 1, 8, 9 and 10 digits on every drawn kind, boxes at the top edge (the tab moves
    inside) and at the right edge (the tab is shifted left), an IGNORED row on each side and a matched ground truth,
    none of which is drawn.  Frame 1: no rows.  Frame 2: 260 ground-truth rows, every third a MISS, and 300 tracker
    rows of all kinds -- more than one chunk of 256 on both sides, and the fullest frame.  Frame 3: half-pixel ties
    and boxes off the frame."""
    frames = [
        # (gt: ids, boxes, kinds), (tracker: ids, boxes, kinds)
        (([7, 12345678, 3, 4], [[10, 3, 20, 30], [80, 20, 30, 30], [40, 40, 10, 10], [1, 1, 5, 5]],
          [D.MISS, D.MISS, D.MATCH, D.IGNORED]),
         ([123456789, 2147483647, 5, 6, 9], [[30, 8, 20.5, 20.5], [90, 30, 20, 20], [40, 40, 10, 10], [50.5, 9.5, 9, 9],
                                             [60, 20, 8, 8]], [D.TP, D.FP, D.SWITCH, D.FP, D.IGNORED])),
        (([], [], []), ([], [], [])),
        None,
        (([1, 2], [[8.5, 12.5, 8.0, 8.0], [-30, -30, 10, 10]], [D.MISS, D.MISS]),
         ([3, 4], [[-0.5, 0.5, 64.0, 31.0], [90.25, 60.75, 40, 40]], [D.FP, D.TP])),
    ]
    rs = np.random.RandomState(5)
    n_gt, n_tr = 260, 300
    box = lambda n: np.concatenate([rs.uniform(-5, 90, (n, 2)), rs.uniform(2, 30, (n, 2))], 1)          # noqa: E731
    frames[2] = ((np.arange(n_gt) * 37 + 1, box(n_gt), np.array([D.MISS, D.MATCH, D.SWITCH])[np.arange(n_gt) % 3]),
                 (np.arange(n_tr) * 1013 + 5, box(n_tr), rs.choice([D.IGNORED, D.TP, D.SWITCH, D.FP], n_tr)))
    off = lambda side: np.concatenate(([0], np.cumsum([len(f[side][0]) for f in frames]))).astype(np.int32)     # noqa: E731
    cat = lambda side, k, dt, shape: np.concatenate(                                                     # noqa: E731
        [np.asarray(f[side][k], dt).reshape(shape) for f in frames])
    n = int(off(0)[-1])
    return D.SequenceEvents("table", off(0), off(1), cat(0, 0, np.int32, (-1,)), cat(0, 1, np.float64, (-1, 4)),
                            cat(0, 2, np.int32, (-1,)), np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n),
                            cat(1, 0, np.int32, (-1,)), cat(1, 1, np.float64, (-1, 4)), cat(1, 2, np.int32, (-1,)),
                            np.full(int(off(1)[-1]), -1, np.int32))


# ------------------------------------------------------------------------------------------------ a tree of files
TREE_SEQ = "seq-a"
TREE_FRAMES = 3


def tree_rows():
    """Three 64 x 96 frames: a miss and a false positive in the first, a clean second, a switch in the third."""
    a, b = [10.0, 20.0, 30.0, 28.0], [55.0, 12.0, 24.0, 40.0]
    gt = {1: [(1, a), (2, b)], 2: [(1, a), (2, b)], 3: [(1, a), (2, b)]}
    tr = {1: [(11, a), (12, [70.0, 2.0, 20.0, 14.0])], 2: [(11, a), (13, b)], 3: [(14, a), (13, b)]}
    return gt, tr


def write_tree(root):
    """``<root>/gt/<seq>/gt/gt.txt`` with seqinfo.ini, ``<root>/tracker/<seq>.txt``, ``<root>/seqmap.txt`` and the
    frames ``<root>/gt/<seq>/img1/0000000t.jpg`` (64 x 96, the project's encoder).  Returns evaluate_files' arguments
    and the frame paths."""
    import torch

    from memotr_amd.data import encode_jpeg
    gt, tr = tree_rows()
    seq_dir = os.path.join(root, "gt", TREE_SEQ)
    os.makedirs(os.path.join(seq_dir, "gt"))
    os.makedirs(os.path.join(seq_dir, "img1"))
    os.makedirs(os.path.join(root, "tracker"))
    line = lambda t, i, b, tail: f"{t},{i},{b[0]},{b[1]},{b[2]},{b[3]},{tail}\n"                  # noqa: E731
    with open(os.path.join(seq_dir, "gt", "gt.txt"), "w") as f:
        f.write("".join(line(t, i, b, "1,1,1") for t, rows in gt.items() for i, b in rows))
    with open(os.path.join(seq_dir, "seqinfo.ini"), "w") as f:
        f.write(f"[Sequence]\nname={TREE_SEQ}\nseqLength={TREE_FRAMES}\n")
    with open(os.path.join(root, "tracker", TREE_SEQ + ".txt"), "w") as f:
        f.write("".join(line(t, i, b, "1,-1,-1,-1") for t, rows in tr.items() for i, b in rows))
    with open(os.path.join(root, "seqmap.txt"), "w") as f:
        f.write(f"name\n{TREE_SEQ}\n")
    paths = []
    for t in range(1, TREE_FRAMES + 1):
        paths.append(os.path.join(seq_dir, "img1", f"{t:08d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(encode_jpeg(torch.from_numpy(T.frame_pixels(t, h=HEIGHT, w=WIDTH)), quality=90, subsampling="4:2:0"))
    return (os.path.join(root, "gt"), os.path.join(root, "tracker"), os.path.join(root, "seqmap.txt")), paths


def expected_frame_files(ev, paths, quality, thickness, font_scale):
    """{frame: bytes}: ``encode_jpeg(draw_table_host(decoded frame, error_table_host(...)[f]))`` of every frame."""
    import torch

    from memotr_amd import render as R
    from memotr_amd.data import encode_jpeg
    from memotr_amd.data.jpeg import decode_jpeg
    table = D.error_table_host(ev, WIDTH, HEIGHT, font_scale=font_scale)
    out = {}
    for f, path in enumerate(paths):
        frame = decode_jpeg(path, "cpu").numpy()
        R.draw_table_host(frame, table[f], thickness, font_scale, 0)
        out[f + 1] = encode_jpeg(torch.from_numpy(frame), quality)
    return out
