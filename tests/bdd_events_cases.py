"""Shared by tests/test_bdd_events_cpu.py and tests/test_bdd_events_gpu.py: builders of BDD100K sequences with class
confusions (scripted frames, random sequences, the grid that fills a wavefront), the brute-force truth of the
cross-class pass, and a small tree of files for the public interface."""
import itertools
import json
import os

import numpy as np

from memotr_amd import diagnose_bdd100k as DB
from memotr_amd import evaluation_bdd100k as B

ID = B.CLASS_NAME_TO_CLASS_ID
CAR, TRUCK, BUS, PED = (B.CLASSES.index(c) for c in ("car", "truck", "bus", "pedestrian"))
GT_BOX = [0.0, 0.0, 100.0, 100.0]
_CACHE = {}


def overlapping(iou, at=(0.0, 0.0)):
    """A box whose IoU with the 100 x 100 box at ``at`` is ``iou``: the same box cut to 100 * iou rows."""
    x, y = at
    return [x, y, x + 100.0, y + 100.0 * iou]


def sequence(frames):
    """``pack_bdd``'s lists from ``[{"gt": [(id, category, box)], "tr": [...], "regions": [box]}]``; a key may be left
    out."""
    out = {k: [] for k in ("gt_ids", "gt_boxes", "gt_classes", "tracker_ids", "tracker_boxes", "tracker_classes",
                           "ignore_regions")}
    for fr in frames:
        for side, key in (("gt", "gt"), ("tr", "tracker")):
            rows = fr.get(side, [])
            out[key + "_ids"].append(np.array([r[0] for r in rows], np.int64))
            out[key + "_classes"].append(np.array([ID[r[1]] for r in rows], np.int64))
            out[key + "_boxes"].append(np.array([r[2] for r in rows], np.float64).reshape(-1, 4))
        out["ignore_regions"].append(np.array(fr.get("regions", []), np.float64).reshape(-1, 4))
    return out


def scripted():
    """{name: frames}: the hand-made sequences, each small.  The tests say what every one of them must give."""
    far = lambda box: [v + 1000.0 for v in box]                                                 # noqa: E731
    shifted = lambda box, dx: [box[0] + dx, box[1], box[2] + dx, box[3]]                        # noqa: E731
    tie_gt = [(1, "car", GT_BOX), (2, "car", GT_BOX)]
    tie_tr = [(7, "truck", overlapping(0.8)), (8, "bus", overlapping(0.8))]
    return {
        "car_as_truck": [{"gt": [(1, "car", GT_BOX)], "tr": [(7, "truck", overlapping(0.9))]}],
        "below_half": [{"gt": [(1, "car", GT_BOX)], "tr": [(7, "truck", overlapping(0.499))]}],
        "above_half": [{"gt": [(1, "car", GT_BOX)], "tr": [(7, "truck", overlapping(0.501))]}],
        # two ground-truth candidates for one tracker row: the larger IoU wins
        "larger_wins": [{"gt": [(1, "car", GT_BOX), (2, "bus", overlapping(0.8))], "tr": [(7, "truck", overlapping(0.7))]}],
        # every entry of the 2 x 2 problem is the same IoU: the pairs are scipy's
        "tie": [{"gt": tie_gt, "tr": tie_tr}],
        "inside_region": [{"gt": [(1, "car", far(GT_BOX))], "tr": [(7, "truck", GT_BOX)],
                           "regions": [overlapping(0.6)]}],
        "outside_region": [{"gt": [(1, "car", far(GT_BOX))], "tr": [(7, "truck", GT_BOX)],
                            "regions": [overlapping(0.4)]}],
        # a crowd region over a box that would have been a cross candidate
        "region_over_candidate": [{"gt": [(1, "car", GT_BOX)], "tr": [(7, "truck", overlapping(0.9))],
                                   "regions": [GT_BOX]}],
        "other_category": [{"gt": [(1, "car", GT_BOX)], "tr": [(7, "other vehicle", overlapping(0.9)),
                                                                (8, "car", far(GT_BOX))]}],
        "empty_sides": [{"tr": [(7, "truck", GT_BOX)]}, {"gt": [(1, "car", GT_BOX)]}, {}],
        "no_tracker": [{"gt": [(1, "car", GT_BOX)]}, {"gt": [(1, "car", GT_BOX)]}],
        "no_gt": [{"tr": [(7, "truck", GT_BOX)]}],
        "swap": [{"gt": [(1, "car", GT_BOX), (2, "truck", far(GT_BOX))],
                  "tr": [(7, "truck", overlapping(0.9)), (8, "car", far(overlapping(0.8)))]}],
        # a track that is right, then labelled bus for two frames, then right again under a new name: every kind
        "every_kind": [
            {"gt": [(1, "car", GT_BOX), (2, "pedestrian", far(GT_BOX))],
             "tr": [(7, "car", overlapping(0.9)), (9, "pedestrian", far(GT_BOX))]},
            {"gt": [(1, "car", shifted(GT_BOX, 5)), (2, "pedestrian", far(GT_BOX))],
             "tr": [(7, "bus", shifted(overlapping(0.9), 5)), (9, "pedestrian", far(GT_BOX))]},
            {"gt": [(1, "car", shifted(GT_BOX, 10)), (2, "pedestrian", far(GT_BOX))],
             "tr": [(7, "bus", shifted(overlapping(0.9), 10)), (5, "rider", [400.0, 400.0, 440.0, 440.0])],
             "regions": [[390.0, 390.0, 450.0, 450.0]]},
            {"gt": [(1, "car", shifted(GT_BOX, 15)), (2, "pedestrian", far(GT_BOX))],
             "tr": [(8, "car", shifted(overlapping(0.9), 15)), (9, "pedestrian", far(GT_BOX))]},
        ],
    }


def scripted_pack():
    """All scripted sequences in one pack (host), built once."""
    if "scripted" not in _CACHE:
        _CACHE["scripted"] = B.pack_bdd({name: sequence(frames) for name, frames in scripted().items()})
    return _CACHE["scripted"]


# ------------------------------------------------------------------------------------------------ random sequences
RANDOM_SEEDS = (7, 11, 29)
RANDOM_FRAMES = (23, 31, 17)            # different lengths: seq_off and the problem-major offsets are no multiples


def confused_sequence(seed, n_frames, n_objects=6, flip=0.15, double=0.3):
    """``synthetic_bdd_sequence`` (two ignore regions a frame) with class confusions: a followed object's detection is
    relabelled to another class now and then, and some of those get a second, differently cut box of a third class
    under a new id, so that two false positives compete for one miss."""
    seq = B.synthetic_bdd_sequence(seed, n_frames, n_objects, n_regions=2, miss=0.08)
    rng = np.random.RandomState(seed + 101)
    next_id = 700000
    for t in range(n_frames):
        ids, boxes, classes = (seq[k][t] for k in ("tracker_ids", "tracker_boxes", "tracker_classes"))
        extra = []
        for j in range(len(ids)):
            if ids[j] >= 500000 or rng.uniform() >= flip:
                continue
            c = B.CLASS_IDS.index(int(classes[j]))
            classes[j] = B.CLASS_IDS[(c + 1 + rng.randint(6)) % 8]
            if rng.uniform() < double:
                third = B.CLASS_IDS[(c + 7) % 8]
                grow = rng.uniform(-6, 6, 4)
                extra.append((next_id, boxes[j] + grow, third))
                next_id += 1
        if extra:
            seq["tracker_ids"][t] = np.concatenate([ids, [e[0] for e in extra]])
            seq["tracker_boxes"][t] = np.concatenate([boxes, [e[1] for e in extra]])
            seq["tracker_classes"][t] = np.concatenate([classes, [e[2] for e in extra]])
    return seq


def candidates(ev, f):
    """(ground-truth rows, tracker rows) of frame ``f`` of a ``BDDSequenceEvents`` that the cross-class pass pairs."""
    g = np.arange(ev.gt_off[f], ev.gt_off[f + 1])
    t = np.arange(ev.tr_off[f], ev.tr_off[f + 1])
    return g[ev.gt_kind[g] == DB.MISS], t[ev.tr_kind[t] == DB.FP]


def random_pack():
    """(pack, host events) of the random sequences, built once.  Every frame stays within 5 x 5 cross candidates, which
    is what the brute force can enumerate; some frame has at least two on a side."""
    if "random" not in _CACHE:
        pack = B.pack_bdd({f"walk{seed}": confused_sequence(seed, n) for seed, n in zip(RANDOM_SEEDS, RANDOM_FRAMES)})
        events = DB.bdd_events(pack)
        sizes = [tuple(len(x) for x in candidates(ev, f)) for ev in events.values() for f in range(ev.n_frames)]
        assert max(g for g, _ in sizes) <= 5 and max(t for _, t in sizes) <= 5, sizes
        assert any(g >= 2 and t >= 2 for g, t in sizes)
        _CACHE["random"] = pack, events
    return _CACHE["random"]


# ------------------------------------------------------------------------------------------------ the brute force
def iou(a, b):
    """Box IoU of two corner boxes, written out once more."""
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    inter = max(w, 0.0) * max(h, 0.0)
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / union if union > 0 else 0.0


def admissible(ev, i, j):
    """The IoU of ground-truth row i and tracker row j where they may be paired, else None."""
    if DB.class_index(ev.gt_classes[i:i + 1])[0] == DB.class_index(ev.tr_classes[j:j + 1])[0]:
        return None
    v = iou(ev.gt_boxes[i], ev.tr_boxes[j])
    return v if v >= 0.5 else None


def brute_force(ev, f):
    """(the largest summed IoU over all injective partial maps of the frame's candidates, the set of pair sets that
    reach it)."""
    g, t = candidates(ev, f)
    assert len(g) <= 5 and len(t) <= 5
    value = {(i, j): admissible(ev, i, j) for i in g for j in t}
    best, optima = 0.0, [frozenset()]
    for choice in itertools.product([None] + list(t), repeat=len(g)):
        taken = [j for j in choice if j is not None]
        if len(set(taken)) != len(taken):
            continue
        pairs = frozenset((i, j) for i, j in zip(g, choice) if j is not None)
        if any(value[p] is None for p in pairs):
            continue
        total = sum(value[p] for p in pairs)
        if total > best + 1e-9:
            best, optima = total, [pairs]
        elif abs(total - best) <= 1e-9 and pairs not in optima:
            optima.append(pairs)
    return best, optima


def cross_pairs(ev, f):
    """The product's pairs of frame ``f`` as (ground-truth row, tracker row), read from the ground-truth side."""
    g0, t0 = int(ev.gt_off[f]), int(ev.tr_off[f])
    return frozenset((i, t0 + int(ev.gt_cross_partner[i])) for i in range(g0, int(ev.gt_off[f + 1]))
                     if ev.gt_cross_partner[i] >= 0)


# --------------------------------------------------------------------------------------- a wavefront's worth of cars
GRID_COUNTS = (1, 63, 64, 65)
GRID_FRAMES = (1, 3, 4, 6)              # the frames that hold them; frames 0, 2, 5 and 7 hold no row


def grid_pack():
    """One sequence of 8 frames: ``GRID_COUNTS[k]`` cars on a grid in frame ``GRID_FRAMES[k]``, each under one box
    labelled truck (IoU 0.6 .. 0.92) and far from every other, which makes the optimum unique.
    A pedestrian that is tracked correctly sits between every seven cars, on both sides, so the candidates are not the
    rows' first.  The frames between hold nothing: a wavefront that overran its frame would write into them."""
    if "grid" not in _CACHE:
        frames = [{} for _ in range(8)]
        for n, f in zip(GRID_COUNTS, GRID_FRAMES):
            gt, tr = [], []
            for k in range(n):
                at = (250.0 * (k % 10), 250.0 * (k // 10))
                gt.append((k + 1, "car", overlapping(1.0, at)))
                tr.append((1000 + k, "truck", overlapping(0.6 + 0.005 * ((k * 37) % 64), at)))
                if k % 7 == 3:
                    box = [at[0] + 120.0, at[1], at[0] + 160.0, at[1] + 90.0]
                    gt.append((500 + k, "pedestrian", box))
                    tr.insert(0, (2000 + k, "pedestrian", box))
            frames[f] = {"gt": gt, "tr": tr}
        _CACHE["grid"] = B.pack_bdd({"grid": sequence(frames)})
    return _CACHE["grid"]


# ------------------------------------------------------------------------------------------------ a tree of files
def write_tree(root, pack):
    """``<root>/gt/<seq>.json`` and ``<root>/tracker/<seq>.json`` of a host pack in ``evaluate_bdd_files``' layout;
    ignore regions become ground-truth rows with the Crowd attribute.  Returns (gt_dir, tracker_dir)."""
    names = {v: k for k, v in ID.items()}
    label = lambda i, c, b, crowd=False: {"id": str(int(i)), "category": names[int(c)],           # noqa: E731
                                          "box2d": dict(zip(("x1", "y1", "x2", "y2"), map(float, b))),
                                          "attributes": {"Crowd": crowd}}
    gt_dir, tracker_dir = os.path.join(root, "gt"), os.path.join(root, "tracker")
    os.makedirs(gt_dir), os.makedirs(tracker_dir)
    for s, name in enumerate(pack.names):
        gt, tr = [], []
        for t, f in enumerate(range(pack.seq_off[s], pack.seq_off[s + 1])):
            g, k, r = (slice(off[f], off[f + 1]) for off in (pack.gt_off, pack.tr_off, pack.ig_off))
            labels = [label(i, c, b) for i, c, b in zip(pack.gt_ids[g], pack.gt_classes[g], pack.gt_boxes[g])]
            labels += [label(900000 + n, ID["car"], b, True) for n, b in enumerate(pack.ig_boxes[r])]
            gt.append({"index": t, "labels": labels})
            tr.append({"index": t, "labels": [label(i, c, b) for i, c, b in
                                              zip(pack.tr_ids[k], pack.tr_classes[k], pack.tr_boxes[k])]})
        for d, frames in ((gt_dir, gt), (tracker_dir, tr)):
            with open(os.path.join(d, name + ".json"), "w") as fh:
                json.dump(frames, fh)
    return gt_dir, tracker_dir


def same_events(a, b):
    """Two ``{name: BDDSequenceEvents}``: every array equal, dtype and bits (``gt_iou`` and the cross IoUs included)."""
    assert list(a) == list(b)
    for name in a:
        for k in DB.BDDSequenceEvents.ARRAYS:
            x, y = getattr(a[name], k), getattr(b[name], k)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (name, k)
