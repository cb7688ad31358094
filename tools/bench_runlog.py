"""What the run log's component logging costs per clip on one MI355X.  Results: profiles/run_entry.md.

    python tools/bench_runlog.py [--clips 12] [--repeats 5] [--clip-len 5] [--log-every 100] [--out FILE]

Resident synthetic DanceTrack clips (``engine.make_synthetic_clip`` at the benchmark's geometry: 800 x 1333 frames,
10 objects, ``--clip-len`` frames; four clips, cycled) go through ``train.train_one_epoch`` twice per repeat: "plain",
with the arguments the training driver passed before the run log existed, and "logged", with ``runlog=`` a ``RunLog``
on a temporary directory -- per clip one ``criterion.log_components()`` (a stack, a pinned upload of the counts, a
division), one concatenation with the loss, the host's window arithmetic and, per log event, the lines and scalars of
runlog.py.  Model, criterion, optimizer and clips are built once.  Every epoch starts from the same state (parameters,
optimizer state, random generators: ``train_bench._restore_train_state``, not timed), so that every epoch is the same
work on the same track counts: a model that trains on from epoch to epoch changes how many tracks it carries, and a new
count is a new graph capture (tens of ms) in whichever side happens to run then.  One epoch of each side warms up (all
captures); then ``--repeats`` alternating epochs of each are timed between device synchronisations.

Target: mean(logged) - mean(plain) <= max(plain) - min(plain), the plain side's own run-to-run spread.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=12, help="clips per epoch")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clip-len", type=int, default=5)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--out", help="also write the result lines to this file")
    args = ap.parse_args()
    os.environ.setdefault("MEMOTR_REQUIRE_GRAPHS", "1")
    from memotr_amd.configs import dancetrack_config
    from memotr_amd.engine import build_optimizer, clip_to_device, make_synthetic_clip
    from memotr_amd.models import build_model
    from memotr_amd.models.criterion import build as build_criterion
    from memotr_amd.runlog import RunLog
    from memotr_amd.train import train_one_epoch
    from memotr_amd.train_bench import _restore_train_state, _train_state
    from memotr_amd.utils.utils import set_seed

    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = dict(dancetrack_config(), DEVICE="cuda", AVAILABLE_GPUS="0")
    set_seed(cfg["SEED"])
    model = build_model(cfg).to(dev).train()
    criterion = build_criterion(cfg)
    optimizer = build_optimizer(cfg, model)
    clips = [clip_to_device(make_synthetic_clip(args.clip_len, 800, 1333, 10, seed=cfg["SEED"] + i), dev)
             for i in range(4)]
    states = {"start_epoch": 0, "global_iters": 0}
    start = _train_state(model, optimizer, dev)
    lines = []

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        lines.append(line)

    with tempfile.TemporaryDirectory(prefix="runlog_") as tmp:
        runlog = RunLog(os.path.join(tmp, "train"))

        def epoch(logged):
            extra = dict(runlog=runlog, epoch=0, n_iters=args.clips) if logged else {}
            _restore_train_state(model, optimizer, dev, start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            summary = train_one_epoch(model, criterion, optimizer, (clips[i % len(clips)] for i in range(args.clips)),
                                      device=dev, max_norm=cfg["CLIP_MAX_NORM"], use_dab=cfg["USE_DAB"], states=states,
                                      log_every=args.log_every, **extra)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.clips * 1e3, summary["loss"]

        for logged in (False, True):
            ms, loss = epoch(logged)
            emit({"phase": "warmup", "side": "logged" if logged else "plain", "ms_per_clip": ms, "loss": loss})
        times = {"plain": [], "logged": []}
        for r in range(args.repeats):
            for logged in (False, True):
                side = "logged" if logged else "plain"
                ms, loss = epoch(logged)
                times[side].append(ms)
                emit({"phase": "timed", "repeat": r, "side": side, "ms_per_clip": ms, "loss": loss})
        with open(os.path.join(tmp, "train", "log.txt")) as f:
            log_lines = f.read().count("\n")
    plain, logged = times["plain"], times["logged"]
    spread = max(plain) - min(plain)
    diff = statistics.mean(logged) - statistics.mean(plain)
    emit({"phase": "summary", "clips_per_epoch": args.clips, "clip_len": args.clip_len, "repeats": args.repeats,
          "log_every": args.log_every, "log_lines_written": log_lines,
          "plain_ms_per_clip": {"mean": statistics.mean(plain), "median": statistics.median(plain), "min": min(plain),
                                "max": max(plain)},
          "logged_ms_per_clip": {"mean": statistics.mean(logged), "median": statistics.median(logged),
                                 "min": min(logged), "max": max(logged)},
          "difference_of_means_ms": diff, "plain_spread_ms": spread, "within_spread": diff <= spread,
          "max_memory_MB": torch.cuda.max_memory_allocated() // (1024 ** 2), "torch": torch.__version__})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
