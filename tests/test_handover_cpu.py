"""CPU: the track hand-over as one gather (ClipCriterion.finish_tracks with state["handover"] with clip_ops.handover_reference and
the host-built tables of clip_ops.handover_tables) against the composed path finish_tracks -> select_active_tracks."""
import numpy as np
import pytest
import torch

from handover_cases import CASES, CASE_IDS, active_set, assert_same_grads, assert_same_tracks, backward_through
from memotr_amd.functions import clip_ops

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def composed():
    """The composed path's active set and gradients, once per case."""
    cache = {}

    def get(case):
        if case not in cache:
            tracks, leaves, fused = active_set(case, CPU, fused=False)
            assert not fused
            cache[case] = (tracks, backward_through(tracks, leaves))
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_field_of_the_gathered_set_equals_the_composed_one(case, composed):
    want, want_grads = composed(case)
    got, leaves, fused = active_set(case, CPU, fused=True)
    assert fused
    assert_same_tracks(got, want)
    assert got._packed_base() is not None and got._packed_base()[1] == type(got).PACKED_FLOAT
    assert_same_grads(backward_through(got, leaves), want_grads)


def test_the_cases_contain_every_kind_of_row(composed):
    """What the cases are meant to exercise does occur (a change of the generator must not quietly lose it)."""
    nd, n_tr, n_gt = 300, 7, 10
    tracks, _ = composed((nd, n_tr, n_gt, 8, True, True))
    n = len(tracks)
    assert n_tr - 1 + 1 < n < n_tr + nd                       # track 6 went; some unclaimed detections stay, others go
    carried = tracks[:6]
    assert carried.matched_idx.tolist()[:3] == [9, 8, 7] and carried.matched_idx.tolist()[3:] == [-1, -1, -1]
    assert carried.ids.tolist() == [19, -1, 17, 903, -1, -1]  # IoU below 0.5 (1), ground truth gone (3 kept, 4 not)
    iou = tracks.iou.detach()
    assert float(iou[3]) == pytest.approx(0.8) and float(iou[1]) < 0.5
    rest = tracks.ids[6:]
    assert bool((rest >= 0).any()) and bool((rest < 0).any())     # new identities, and rows without one
    new_rows = tracks.matched_idx[6:] >= 0
    assert bool((iou[6:][new_rows] < 0.5).any())          # a matched detection whose identity goes
    assert bool((iou[6:][~new_rows] == 0).all())


def test_the_tables_invert_each_other():
    nd, n_q, n_tr = 8, 13, 4
    new_q, new_g, free_q = np.array([1, 6]), np.array([2, 0]), np.array([0, 2, 3, 4, 5, 7])
    keep = np.array([0, 2, 3, 4, 5, 7, 11])                    # carried 0 2 3 | new 1 6 | unclaimed 2 7
    t = clip_ops.handover_tables(nd, n_q, n_tr, new_q, new_g, free_q, keep)
    table, inv_q, inv_prev = t[:21].reshape(7, 3), t[21:21 + n_q], t[21 + n_q:]
    assert table.tolist() == [[0, 0, -1], [0, 2, -1], [0, 3, -1], [1, 1, 2], [1, 6, 0], [2, 2, -1], [2, 7, -1]]
    assert inv_prev.tolist() == [0, -1, 1, 2]
    assert inv_q.tolist() == [-1, 3, 5, -1, -1, -1, 4, 6, 0, -1, 1, 2, -1]


def test_an_empty_active_set_takes_the_composed_path():
    tracks, _, fused = active_set((8, 0, 3, 1, True, False), CPU, fused=True, empty_active=True)
    assert not fused
    assert tracks.ids.tolist() == [-2]                          # the query updater's fake track


def test_the_switch_takes_the_composed_path(monkeypatch, composed):
    monkeypatch.setenv("MEMOTR_FUSED_HANDOVER", "0")
    case = CASES[2]
    tracks, _, fused = active_set(case, CPU, fused=True)
    assert not fused
    assert_same_tracks(tracks, composed(case)[0])
