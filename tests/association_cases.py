"""Shared by tests/test_association_cpu.py and tests/test_association_gpu.py: the fixture TrackEval's HOTA and Identity
were recorded into (tests/golden/association.npz; its inputs are clear_events.npz's), the host statement of every set
computed once, and the hand-written sequence the timeline and the two CSVs are checked on."""
import numpy as np

import clear_events_cases as C
from conftest import load_golden

from memotr_amd import association as A
from memotr_amd import evaluation as E

SETS = C.SETS
_GOLDEN, _HOST = {}, {}


def golden(prefix):
    """(recorded arrays, PackedSequences) of one benchmark, loaded once and shared."""
    if not _GOLDEN:
        _GOLDEN["all"] = load_golden("association")
    if prefix not in _GOLDEN:
        g = {k[len(prefix) + 2:]: v for k, v in _GOLDEN["all"].items() if k.startswith(prefix + "::")}
        packed = C.golden(prefix)[1]
        assert [str(n) for n in g["names"]] == packed.names
        _GOLDEN[prefix] = g, packed
    return _GOLDEN[prefix]


def host(prefix):
    """(preprocessed data ``d``, similarity, ``association_host``'s arrays) of one benchmark: computed once, left
    unchanged."""
    if prefix not in _HOST:
        _, packed = golden(prefix)
        _, sim, d = E._preprocess_host(packed, SETS[prefix])
        _HOST[prefix] = d, sim, A.association_host(packed, SETS[prefix])
    return _HOST[prefix]


def levels(sim):
    """The number of HOTA thresholds a similarity reaches."""
    return (np.asarray(sim)[:, None] >= E.ALPHAS[None, :] - E.EPS).sum(1)


def matches_from_pairs(g, d):
    """HOTA's ``matches`` table, int32 [19 * cells] laid out as ``trackeval_hota_match``'s, from the recorded pairs."""
    out = np.zeros(A.N_ALPHA * int(d["cell_off"][-1]), np.int32)
    for s in range(len(d["seq_off"]) - 1):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        m = out[A.N_ALPHA * d["cell_off"][s]:A.N_ALPHA * d["cell_off"][s + 1]].reshape(A.N_ALPHA, G, K)
        a, b = g["pair_off"][d["seq_off"][s]], g["pair_off"][d["seq_off"][s + 1]]
        for gi, ti, lv in zip(g["pair_gt"][a:b], g["pair_tr"][a:b], levels(g["pair_sim"][a:b])):
            m[:lv, gi, ti] += 1
    return out


def int_keys(t):
    return sorted(k for k, v in t.items() if isinstance(v, np.ndarray) and v.dtype.kind in "ib")


NUM_KEYS = ("gt_num", "tr_num")


def num_rtol(d):
    """Two summation orders of n non-negative terms, each term the same bits, differ by at most (n - 1) * 2**-52
    relative; a per-identity sum has at most max(G, K) terms."""
    return float(max(d["n_gt_ids"].max(), d["n_tr_ids"].max())) * 2.0 ** -52


# ------------------------------------------------------------------------------------------ the hand-written case
A_BOX, B_BOX, C_BOX = [0.0, 0.0, 10.0, 10.0], [100.0, 0.0, 10.0, 10.0], [200.0, 0.0, 10.0, 10.0]


def hand_sequences():
    """3 identities, 5 frames.  Identity 1 is followed by tracker 11, missed in frame 3 and matched loosely (IoU 0.42:
    level 8) in frame 5; identity 2 is followed by 12 and from frame 4 by 13 (a swap); identity 3 is absent in frame 2
    and followed by 14; tracker 15 is a false positive of frame 1."""
    loose = [0.0, 0.0, 10.0, 4.2]
    gt = {1: [(1, A_BOX), (2, B_BOX), (3, C_BOX)], 2: [(1, A_BOX), (2, B_BOX)], 3: [(1, A_BOX), (2, B_BOX), (3, C_BOX)],
          4: [(1, A_BOX), (2, B_BOX), (3, C_BOX)], 5: [(1, A_BOX), (2, B_BOX), (3, C_BOX)]}
    tr = {1: [(11, A_BOX), (12, B_BOX), (14, C_BOX), (15, [300.0, 0.0, 10.0, 10.0])], 2: [(11, A_BOX), (12, B_BOX)],
          3: [(12, B_BOX), (14, C_BOX)], 4: [(11, A_BOX), (13, B_BOX), (14, C_BOX)],
          5: [(11, loose), (13, B_BOX), (14, C_BOX)]}
    ids = lambda rows: np.array([i for i, _ in rows], np.int64)                                 # noqa: E731
    boxes = lambda rows: np.array([b for _, b in rows], np.float64).reshape(-1, 4)               # noqa: E731
    return {"hand": {"gt_ids": [ids(gt[t]) for t in range(1, 6)], "gt_boxes": [boxes(gt[t]) for t in range(1, 6)],
                     "tracker_ids": [ids(tr[t]) for t in range(1, 6)],
                     "tracker_boxes": [boxes(tr[t]) for t in range(1, 6)]}}


def hand_association():
    return A.association(E.pack_sequences(hand_sequences()), "MOT17")["hand"]


# render.PALETTE[11 .. 14]
P11, P12, P13, P14 = (196, 255, 112), (0, 255, 160), (64, 93, 255), (255, 112, 246)
GREY, BLACK = (96, 96, 96), (0, 0, 0)
HAND_CELLS = {                  # alpha_index -> rows of identities 1, 2, 3 over frames 1 .. 5
    9: [[P11, P11, GREY, P11, GREY], [P12, P12, P12, P13, P13], [P14, BLACK, P14, P14, P14]],
    7: [[P11, P11, GREY, P11, P11], [P12, P12, P12, P13, P13], [P14, BLACK, P14, P14, P14]],
}

HAND_ROWS_CSV = """frame,side,id,x,y,w,h,kept,partner_id,iou,level
1,gt,1,0.0,0.0,10.0,10.0,1,11,1.0,19
1,gt,2,100.0,0.0,10.0,10.0,1,12,1.0,19
1,gt,3,200.0,0.0,10.0,10.0,1,14,1.0,19
1,tr,11,0.0,0.0,10.0,10.0,1,1,1.0,19
1,tr,12,100.0,0.0,10.0,10.0,1,2,1.0,19
1,tr,14,200.0,0.0,10.0,10.0,1,3,1.0,19
1,tr,15,300.0,0.0,10.0,10.0,1,-1,0.0,0
2,gt,1,0.0,0.0,10.0,10.0,1,11,1.0,19
2,gt,2,100.0,0.0,10.0,10.0,1,12,1.0,19
2,tr,11,0.0,0.0,10.0,10.0,1,1,1.0,19
2,tr,12,100.0,0.0,10.0,10.0,1,2,1.0,19
3,gt,1,0.0,0.0,10.0,10.0,1,-1,0.0,0
3,gt,2,100.0,0.0,10.0,10.0,1,12,1.0,19
3,gt,3,200.0,0.0,10.0,10.0,1,14,1.0,19
3,tr,12,100.0,0.0,10.0,10.0,1,2,1.0,19
3,tr,14,200.0,0.0,10.0,10.0,1,3,1.0,19
4,gt,1,0.0,0.0,10.0,10.0,1,11,1.0,19
4,gt,2,100.0,0.0,10.0,10.0,1,13,1.0,19
4,gt,3,200.0,0.0,10.0,10.0,1,14,1.0,19
4,tr,11,0.0,0.0,10.0,10.0,1,1,1.0,19
4,tr,13,100.0,0.0,10.0,10.0,1,2,1.0,19
4,tr,14,200.0,0.0,10.0,10.0,1,3,1.0,19
5,gt,1,0.0,0.0,10.0,10.0,1,11,0.42,8
5,gt,2,100.0,0.0,10.0,10.0,1,13,1.0,19
5,gt,3,200.0,0.0,10.0,10.0,1,14,1.0,19
5,tr,11,0.0,0.0,10.0,4.2,1,1,0.42,8
5,tr,13,100.0,0.0,10.0,10.0,1,2,1.0,19
5,tr,14,200.0,0.0,10.0,10.0,1,3,1.0,19
"""
