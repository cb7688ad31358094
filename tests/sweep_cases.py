"""Shared by tests/test_sweep_cpu.py and tests/test_sweep_gpu.py: the scenario of tests/multi_track_cases.py (three
sequences of 2, 4 and 3 frames, the small model with spread scores) under four threshold settings, the one-sequence runs
each setting is compared with, and their decision margins.

The settings, as (det, track, result, miss), were chosen on the CPU with the oracle's operator
(``python tests/sweep_cases.py [hidden]`` prints the margins) so that no decision score of a one-sequence run lies within
``multi_track_cases.MARGIN`` of its threshold -- smallest margin at hidden 64 / 256: A 0.0146 / 0.0136, D 0.0097 / 0.0034,
F 0.0041 / 0.0052, E 0.0248 / 0.0041 -- every scenario is eventful and the reported track counts differ between the
settings.  ((0.75, 0.55, 0.45, 2) falls to 0.00017 at hidden 256: not used.)"""
import multi_track_cases as M

NAMES = ("A", "D", "F", "E")
SETTINGS = [dict(det_score_thresh=d, track_score_thresh=t, result_score_thresh=r, miss_tolerance=m)
            for d, t, r, m in ((0.8, 0.45, 0.55, 2), (0.6, 0.5, 0.5, 1), (0.85, 0.35, 0.65, 3), (0.8, 0.45, 0.7, 2))]
OPTIONS = dict(use_dab=True, area_thresh=10, raw_size=M.RAW_SIZE)       # what every setting shares


def single_runs(model, seqs, settings=SETTINGS):
    """Every setting's one-sequence runs: ``(want[k][seq][frame], smallest decision margin of all of them)``."""
    want, margin = [], float("inf")
    for s in settings:
        results, m = M.single_runs(model, seqs, dict(OPTIONS, **s))
        want.append(results)
        margin = min(margin, m)
    return want, margin


def sweep_runs(tracker, seqs):
    """The sequences through ``SweepTracker.track``, one after another: ``got[k][seq][frame]``."""
    got = [[[] for _ in seqs] for _ in tracker.settings]
    for s, frames in enumerate(seqs):
        for idx, results in tracker.track(frames):
            assert len(results) == len(tracker.settings)
            for k, r in enumerate(results):
                assert idx == len(got[k][s])
                got[k][s].append(r)
        assert tracker.n_frames == len(frames)
    return got


def some_frame_differs(runs) -> bool:
    """Two settings report different id sets in some frame: the streams do not all apply one setting."""
    first = runs[0]
    return any(a.ids.tolist() != b.ids.tolist() for other in runs[1:] for sa, sb in zip(first, other)
               for a, b in zip(sa, sb))


if __name__ == "__main__":
    import sys

    import model_helpers
    import memotr_amd.modules.ms_deform_attn as mod
    mod.MSDeformAttnFunction = model_helpers.OracleMSDeformAttnFunction
    hidden = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    model, seqs = M.scenario_model(hidden), M.sequences()
    for name, s in zip(NAMES, SETTINGS):
        results, margin = M.single_runs(model, seqs, dict(OPTIONS, **s))
        print(hidden, name, s, round(margin, 5), M.scenario_is_eventful(results),
              [[len(r.ids) for r in seq] for seq in results], flush=True)
