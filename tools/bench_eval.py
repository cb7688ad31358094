"""What the tracking evaluation costs on the GPU and on the host (memotr_amd/evaluation.py).

    python tools/bench_eval.py [--out profiles/track_eval.md] [--step-limit 240]

Workloads (``evaluation.synthetic_sequence``, fixed seeds):
  dancetrack   25 sequences of 1,000 frames, about 10 objects  (the size of DanceTrack's validation split)
  mot17        7 sequences of 750 frames, about 40 objects, with distractors

All measuring happens in ONE child process (the parent only waits for it, with a limit, and writes the report); every
step in the child runs under its own time limit (SIGALRM), after which the child stops.  Per workload:
  * GPU path, wall clock: ``evaluate_packed`` on device tensors, from the call to the fields on the host (offsets and
    ids cross the bus, the host relabels ids; all included), best and median of the repeats;
  * the same with the inputs on the host (upload included);
  * per-kernel times from HIP events around each library call;
  * GPU path with ONE sequence per call, summed over the sequences (what the parallelism over sequences buys);
  * the host statement (numpy + scipy) in the same process on one core.
"""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {
    "dancetrack": dict(n_seqs=25, n_frames=1000, n_objects=10, n_distractors=0, n_false=1),
    "mot17": dict(n_seqs=7, n_frames=750, n_objects=40, n_distractors=6, n_false=3),
}


class StepTimeout(Exception):
    pass


def limited(seconds, fn, *args):
    def on_alarm(signum, frame):
        raise StepTimeout()
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(seconds))
    try:
        return fn(*args)
    finally:
        signal.alarm(0)


def child(args):
    import numpy as np
    import torch
    from memotr_amd import evaluation as E
    torch.set_num_threads(1)
    out = {"device": torch.cuda.get_device_name(0), "workloads": {}}
    for name, w in WORKLOADS.items():
        if args.only and name != args.only:
            continue
        r = out["workloads"][name] = dict(w)
        seqs = {f"{name}-{i:02d}": E.synthetic_sequence(1000 + i, w["n_frames"], w["n_objects"],
                                                        n_distractors=w["n_distractors"], n_false=w["n_false"])
                for i in range(w["n_seqs"])}
        packed = E.pack_sequences(seqs)
        dev = packed.to("cuda")
        r["gt_dets"], r["tracker_dets"] = int(len(packed.gt_ids)), int(len(packed.tr_ids))

        def wall(fn, repeats):
            times = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
            return res, {"best_ms": min(times), "median_ms": float(np.median(times))}

        def gpu_steps():
            E.evaluate_packed(dev, device="cuda")                                                      # warm-up: module load, LDS opt-in
            res, r["gpu_wall_device_inputs"] = wall(lambda: E.evaluate_packed(dev, device="cuda"), args.repeats)
            _, r["gpu_wall_host_inputs"] = wall(lambda: E.evaluate_packed(packed, device="cuda"), args.repeats)
            timings = {}
            for _ in range(args.repeats):
                E.device_tables(dev, timings=timings)
            torch.cuda.synchronize()
            r["kernels_ms"] = {}
            for k, v in timings.items():
                per_call = len(v) // args.repeats                                      # (similarity runs twice per call)
                for i in range(per_call):
                    label = k if per_call == 1 else f"{k}[{'raw' if i == 0 else 'preprocessed'}]"
                    r["kernels_ms"][label] = float(np.median([a.elapsed_time(b) for a, b in v[i::per_call]]))
            singles = [packed.select(i).to("cuda") for i in range(len(packed.names))]
            _, r["gpu_wall_one_sequence_per_call"] = wall(lambda: [E.evaluate_packed(s, device="cuda") for s in singles], args.repeats)
            timings = {}
            E.device_tables(singles[0], timings=timings)
            torch.cuda.synchronize()
            r["kernels_ms_one_sequence"] = {k: float(sum(a.elapsed_time(b) for a, b in v)) for k, v in timings.items()}
            return res

        def host_step():
            t = time.perf_counter()
            res = E.evaluate_packed(packed, device="cpu")
            r["host_statement_ms"] = (time.perf_counter() - t) * 1e3
            return res

        try:
            got = limited(args.step_limit, gpu_steps)
            want = limited(args.step_limit, host_step)
        except StepTimeout:
            r["error"] = "a step ran into its time limit"
            break
        c, h = got["COMBINED_SEQ"], want["COMBINED_SEQ"]
        r["agree"] = bool(all(np.array_equal(c[k], h[k]) for k in E.INT_FIELDS + E.HOTA_INT_ARRAYS))
        r["summary"] = {k: E.summary(c)[k] for k in ("HOTA", "MOTA", "IDF1")}
    print("BENCH_EVAL " + json.dumps(out))


def report(out, cmd):
    lines = ["# Tracking evaluation: GPU path against the host statement", "",
             f"Command: `{cmd}` on {out['device']}.  Times in ms.  Wall times are from the call to the fields on the",
             "host, best / median of the repeats; the host statement is numpy + scipy on one core in the same process",
             "(TrackEval itself measured 0.4 + 0.07 ms per frame for HOTA + CLEAR on 12 objects, the same order; the",
             "reference runs it with 8 worker processes, at best an eighth of the one-core figure).", ""]
    for name, r in out["workloads"].items():
        lines += [f"## {name}: {r['n_seqs']} sequences x {r['n_frames']} frames, {r['gt_dets']} ground-truth and "
                  f"{r['tracker_dets']} tracker detections", ""]
        if "error" in r:
            lines += [r["error"], ""]
            continue
        host = r["host_statement_ms"]
        rows = [("GPU path, inputs on the device", r["gpu_wall_device_inputs"]),
                ("GPU path, inputs on the host (upload included)", r["gpu_wall_host_inputs"]),
                ("GPU path, one sequence per call, all sequences", r["gpu_wall_one_sequence_per_call"])]
        lines += ["| path | best | median | host statement / median |", "|---|---|---|---|"]
        lines += [f"| {k} | {v['best_ms']:.1f} | {v['median_ms']:.1f} | {host / v['median_ms']:.1f}x |" for k, v in rows]
        lines += [f"| host statement, one core | {host:.1f} | | 1.0x |",
                  f"| host statement / 8 (the reference's 8 workers at their best) | {host / 8:.1f} | | |", "",
                  "| kernel (HIP events, median) | all sequences in one call | one sequence alone |", "|---|---|---|"]
        lines += [f"| {k} | {v:.3f} | {r['kernels_ms_one_sequence'].get(k.split('[')[0], float('nan')):.3f} |"
                  for k, v in r["kernels_ms"].items()]
        lines += ["", f"Kernel time in all: {sum(r['kernels_ms'].values()):.2f} ms.  Integer fields of COMBINED_SEQ equal "
                  f"the host statement's: {r['agree']}.  Summary: {r['summary']}.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_eval.md"))
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--step-limit", str(args.step_limit), "--repeats",
           str(args.repeats)] + (["--only", args.only] if args.only else [])
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=2 * len(WORKLOADS) * args.step_limit + 120)
    line = next((ln for ln in done.stdout.splitlines() if ln.startswith("BENCH_EVAL ")), None)
    if done.returncode != 0 or line is None:
        sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
        return 1
    out = json.loads(line[len("BENCH_EVAL "):])
    text = report(out, "python tools/bench_eval.py" + (f" --only {args.only}" if args.only else ""))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
