"""Times the gap-filling pass (ResultLog.filled, memotr_amd/postprocess.py) for profiles/postprocess.md:

  * ``filled()`` on the device (warm calls, device events) against ``read()`` + the host statement on the same rows,
    for a DanceTrack-like log (1200 frames x 30 tracks, 10 % of the rows removed in runs of 1 to 10) and a MOT17-like
    one (1050 frames x 300 ids, the same removal);
  * ``submit`` on the tests' small DanceTrack tree with the tests' small model, wall time per sequence, pass on and off.

    python tools/postprocess_probe.py [--no-submit]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

MAX_GAP, MIN_LENGTH, REPEATS = 20, 5, 20


def device_ms(fn, repeats=REPEATS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def wall_ms(fn, repeats=REPEATS):
    for _ in range(3):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t))
    return float(np.median(times)), float(np.min(times))


def log_sizes():
    import postprocess_cases as C
    from memotr_amd import _clip_lib as L
    from memotr_amd.postprocess import fill_gaps
    out = {}
    for name, n_frames, n_ids in (("dancetrack_like", 1200, 30), ("mot17_like", 1050, 300)):
        rows = C.rows_from_mask(C.runs_mask(n_ids, n_frames, 0.10, 10, 0), 0)
        log = C.log_from_rows(rows, "cuda")
        want = fill_gaps(rows, MAX_GAP, MIN_LENGTH)
        C.assert_same_rows(log.filled(MAX_GAP, MIN_LENGTH, n_frames=n_frames, n_ids=n_ids).read(), want)

        def host():
            log._rows = None
            return fill_gaps(log.read(), MAX_GAP, MIN_LENGTH)

        def filled_and_read():
            return log.filled(MAX_GAP, MIN_LENGTH, n_frames=n_frames, n_ids=n_ids).read()

        def read_only():
            log._rows = None
            return log.read()

        t = time.perf_counter()
        for _ in range(REPEATS):
            fill_gaps(rows, MAX_GAP, MIN_LENGTH)
        statement = 1e3 * (time.perf_counter() - t) / REPEATS
        out[name] = {
            "n_frames": n_frames, "n_ids": n_ids, "rows": len(rows.frames), "rows_filled": len(want.frames),
            "cells": n_frames * n_ids, "workspace_bytes": 4 * L.lib.clipops_fill_gaps_workspace(1, n_ids, n_frames),
            "filled_known_sizes_device_ms": device_ms(
                lambda: log.filled(MAX_GAP, MIN_LENGTH, n_frames=n_frames, n_ids=n_ids)),
            "filled_known_sizes_wall_ms": wall_ms(
                lambda: log.filled(MAX_GAP, MIN_LENGTH, n_frames=n_frames, n_ids=n_ids)),
            "filled_small_read_wall_ms": wall_ms(lambda: log.filled(MAX_GAP, MIN_LENGTH)),
            "filled_then_read_wall_ms": wall_ms(filled_and_read),
            "read_wall_ms": wall_ms(read_only),
            "read_plus_host_statement_wall_ms": wall_ms(host),
            "host_statement_alone_ms": statement,
        }
    return out


def submit_times():
    import dataset_trees as T
    import multi_track_cases as M
    from memotr_amd import submit as S
    model = M.scenario_model(256).cuda()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = T.write_trees(os.path.join(tmp, "data"), only=("DanceTrack",))
        n_seq = len(T.DANCE_SEQS)
        for streams in (1, 2):
            for name, pp in (("off", None), ("on", dict(max_gap=MAX_GAP, min_length=2))):
                config = dict(DET_SCORE_THRESH=0.8, TRACK_SCORE_THRESH=0.45, RESULT_SCORE_THRESH=0.62, MISS_TOLERANCE=4,
                              USE_MOTION=False, SUBMIT_DIR=os.path.join(tmp, f"{name}{streams}"), SUBMIT_MODEL=None,
                              SUBMIT_DATA_SPLIT="train", DATA_ROOT=root)

                def run():
                    S.submit(config, model=model, train_config=dict(DATASET="DanceTrack", USE_DAB=True),
                             tracker_options=dict(raw_size=M.RAW_SIZE, area_thresh=10), streams=streams, postprocess=pp)

                med, best = wall_ms(run, repeats=7)
                out[f"streams{streams}_{name}"] = {"per_sequence_ms_median": med / n_seq, "per_sequence_ms_min": best / n_seq}
    return out


if __name__ == "__main__":
    result = {"max_gap": MAX_GAP, "min_length": MIN_LENGTH, "logs": log_sizes()}
    if "--no-submit" not in sys.argv:
        result["submit"] = submit_times()
    print(json.dumps(result, indent=1))
