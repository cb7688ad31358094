"""Shared by tests/test_track_eval_cpu.py and tests/test_track_eval_gpu.py: the fixtures TrackEval produced
(tests/golden/trackeval_*.npz) and the bars both the host statement and the kernels are held to."""
import numpy as np

from conftest import load_golden

from memotr_amd import evaluation as E

FLOAT_BAR = 1e-9
SETS = {"trackeval_mot17": "MOT17", "trackeval_mot15": "MOT15"}


_GOLDEN = {}


def golden(name):
    """(arrays, PackedSequences) of a fixture, loaded once and shared."""
    if name not in _GOLDEN:
        g = load_golden(name)
        _GOLDEN[name] = g, E.PackedSequences([str(n) for n in g["names"]], *[g[k] for k in E.PackedSequences.ARRAYS])
    return _GOLDEN[name]


def check_tables(t, g):
    """Similarity and the preprocessed data of ``host_tables`` / ``device_tables`` (as numpy) against the fixture."""
    assert np.array_equal(t["raw_similarity"], g["raw_similarity"])
    assert np.array_equal(t["similarity"], g["pre::similarity"])
    for k in ("gt_off", "tr_off", "gt_ids", "tr_ids", "n_gt_ids", "n_tr_ids", "n_gt_dets", "n_tr_dets"):
        assert np.array_equal(t[k], g["pre::" + k]), k


def check_results(res, g, names):
    """Every field of every sequence and of COMBINED_SEQ against the fixture; returns the largest float difference."""
    fields = [k[5:] for k in g if k.startswith("res::")]
    assert sorted(fields) == sorted(E.HOTA_FLOAT_ARRAYS + E.HOTA_INT_ARRAYS + E.INT_FIELDS + E.FLOAT_FIELDS)
    worst = 0.0
    for row, name in enumerate(list(names) + ["COMBINED_SEQ"]):
        assert sorted(res[name]) == sorted(fields), name
        for k in fields:
            want, got = g["res::" + k][row], np.asarray(res[name][k])
            if k in E.INT_FIELDS or k in E.HOTA_INT_ARRAYS:
                assert np.array_equal(got, want), (name, k, got, want)
            else:
                diff = float(np.max(np.abs(got - want)))
                worst = max(worst, diff)
                assert diff <= FLOAT_BAR, (name, k, diff)
    return worst
