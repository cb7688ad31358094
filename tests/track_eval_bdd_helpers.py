"""Shared by tests/test_track_eval_bdd_cpu.py and tests/test_track_eval_bdd_gpu.py: the fixture TrackEval's BDD100K
code produced (tests/golden/trackeval_bdd100k.npz) and the bars both the host statement and the kernels are held to
(those of tests/track_eval_helpers.py)."""
import numpy as np

from conftest import load_golden
from track_eval_helpers import FLOAT_BAR

from memotr_amd import evaluation as E
from memotr_amd import evaluation_bdd100k as B

FIXTURE = "trackeval_bdd100k"
EXACT_FIELDS = E.INT_FIELDS + E.HOTA_INT_ARRAYS
_GOLDEN = {}


def golden():
    """(arrays, PackedBDD) of the fixture, loaded once and shared."""
    if not _GOLDEN:
        g = load_golden(FIXTURE)
        _GOLDEN["g"] = g, B.PackedBDD([str(n) for n in g["names"]], *[g[k] for k in B.PackedBDD.ARRAYS])
    return _GOLDEN["g"]


def check_tables(t, g):
    """Similarity and the preprocessed data of ``host_tables_bdd`` / ``device_tables_bdd`` (as numpy) against the
    fixture: bit for bit."""
    assert np.array_equal(t["raw_similarity"], g["raw_similarity"])
    assert np.array_equal(t["similarity"], g["pre::similarity"])
    for k in B.TABLE_KEYS:
        assert np.array_equal(t[k], g["pre::" + k]), k


def rows_of(res, names):
    """The result dictionaries in the order of the fixture's ``res_rows``."""
    rows = [(f"{n}/{c}", res[n][c]) for n in names for c in B.CLASSES]
    return rows + [("COMBINED_SEQ/" + k, res["COMBINED_SEQ"][k]) for k in B.CLASSES + B.COMBINED_KEYS]


def check_results(res, g, names):
    """Every field of every (sequence, class), of every class combined and of the five class-combined keys against
    the fixture; returns the largest float difference."""
    fields = [k[5:] for k in g if k.startswith("res::")]
    assert sorted(fields) == sorted(E.HOTA_FLOAT_ARRAYS + E.HOTA_INT_ARRAYS + E.INT_FIELDS + E.FLOAT_FIELDS)
    assert list(res) == list(names) + ["COMBINED_SEQ"]
    assert list(res["COMBINED_SEQ"]) == list(B.CLASSES + B.COMBINED_KEYS)
    rows = rows_of(res, names)
    assert [r[0] for r in rows] == [str(x) for x in g["res_rows"]]
    worst = 0.0
    for row, (name, got_fields) in enumerate(rows):
        assert sorted(got_fields) == sorted(fields), name
        for k in fields:
            want, got = g["res::" + k][row], np.asarray(got_fields[k])
            if k in EXACT_FIELDS:
                assert np.array_equal(got, want), (name, k, got, want)
            else:
                diff = float(np.max(np.abs(got - want)))
                worst = max(worst, diff)
                assert diff <= FLOAT_BAR, (name, k, diff)
    return worst


def same_results(a, b, bar):
    """Two result dictionaries field by field: integer fields equal, float fields within ``bar``; the largest
    float difference."""
    assert list(a) == list(b)
    worst = 0.0
    for name in a:
        assert list(a[name]) == list(b[name]), name
        for cls in a[name]:
            for k in a[name][cls]:
                x, y = np.asarray(a[name][cls][k], np.float64), np.asarray(b[name][cls][k], np.float64)
                diff = float(np.max(np.abs(x - y)))
                worst = max(worst, diff)
                assert diff <= (0 if k in EXACT_FIELDS else bar), (name, cls, k, diff)
    return worst
