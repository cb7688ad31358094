"""What the BDD100K tracking evaluation costs on the GPU and on the host (memotr_amd/evaluation_bdd100k.py).

    python tools/bench_eval_bdd.py [--out profiles/track_eval_bdd.md] [--sequences 200] [--frames 200] [--step-limit 400]

Workload (``evaluation_bdd100k.synthetic_bdd_sequence``, fixed seeds): a set of the size of BDD100K's validation split,
200 sequences of 200 frames, 16 objects per sequence spread over the 8 classes, 2 false positives and 3 ignore
regions per frame -- 1,600 (sequence, class) problems, 320,000 (frame, class) assignments.

All measuring happens in ONE child process (the parent only waits for it, with a limit, and writes the report); every
step in the child runs under its own time limit (SIGALRM), after which the child stops.  Measured:
  * GPU path, wall clock: ``evaluate_packed_bdd`` on device tensors, from the call to the fields on the host (the
    split offsets, ids and removal flags cross the bus, the host relabels ids; all included), best and median;
  * the same with the inputs on the host (upload included);
  * per-call times from HIP events around each library call (``timings``), median of the repeats;
  * the host statement (numpy + scipy) in the same process on one core, once.
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
    from memotr_amd import evaluation_bdd100k as B
    torch.set_num_threads(1)
    r = {"device": torch.cuda.get_device_name(0), "n_seqs": args.sequences, "n_frames": args.frames,
         "repeats": args.repeats}
    seqs = {f"bdd-{i:03d}": B.synthetic_bdd_sequence(3000 + i, args.frames, 16, n_false=2, n_regions=3)
            for i in range(args.sequences)}
    packed = B.pack_bdd(seqs)
    dev = packed.to("cuda")
    r["gt_dets"], r["tracker_dets"], r["regions"] = len(packed.gt_ids), len(packed.tr_ids), len(packed.ig_boxes)

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
        B.evaluate_packed_bdd(dev, device="cuda")                  # warm-up: module load, LDS opt-in
        res, r["gpu_wall_device_inputs"] = wall(lambda: B.evaluate_packed_bdd(dev, device="cuda"), args.repeats)
        _, r["gpu_wall_host_inputs"] = wall(lambda: B.evaluate_packed_bdd(packed, device="cuda"), args.repeats)
        _, r["gpu_tables_only"] = wall(lambda: B.device_tables_bdd(dev), args.repeats)
        timings = {}
        for _ in range(args.repeats):
            B.device_tables_bdd(dev, timings=timings)
        torch.cuda.synchronize()
        r["kernels_ms"] = {}
        for k, v in timings.items():
            per_call = len(v) // args.repeats                      # (the similarity runs twice per call)
            for i in range(per_call):
                label = k if per_call == 1 else f"{k}[{'raw' if i == 0 else 'preprocessed'}]"
                r["kernels_ms"][label] = float(np.median([a.elapsed_time(b) for a, b in v[i::per_call]]))
        return res

    def host_step():
        t = time.perf_counter()
        res = B.evaluate_packed_bdd(packed, device="cpu")
        r["host_statement_ms"] = (time.perf_counter() - t) * 1e3
        return res

    try:
        got = limited(args.step_limit, gpu_steps)
        want = limited(args.step_limit, host_step)
        c, h = got["COMBINED_SEQ"], want["COMBINED_SEQ"]
        r["agree"] = bool(all(np.array_equal(c[key][k], h[key][k]) for key in c
                              for k in E.INT_FIELDS + E.HOTA_INT_ARRAYS))
        r["summary"] = {k: B.bdd_summary(got)["cls_comb_det_av"][k] for k in ("HOTA", "MOTA", "IDF1")}
    except StepTimeout:
        r["error"] = "a step ran into its time limit"
    print("BENCH_EVAL_BDD " + json.dumps(r))


def report(r, cmd):
    lines = ["# BDD100K tracking evaluation: GPU path against the host statement", "",
             f"Command: `{cmd}` on {r['device']}.  Times in ms.  Wall times are from the call to the fields on the host,",
             f"best / median of {r['repeats']} repeats; the host statement is numpy + scipy on one core in the same process, run once.",
             "No threshold is derived from these numbers and none is tested: the host statement is the default.", "",
             f"Synthetic set: {r['n_seqs']} sequences x {r['n_frames']} frames x 8 classes, {r['gt_dets']} ground-truth and "
             f"{r['tracker_dets']} tracker detections, {r['regions']} ignore regions.", ""]
    if "error" in r:
        lines += [r["error"] + "; what was measured before it:", ""]
    host = r.get("host_statement_ms")
    rows = [("GPU path, inputs on the device", r.get("gpu_wall_device_inputs")),
            ("GPU path, inputs on the host (upload included)", r.get("gpu_wall_host_inputs")),
            ("GPU path, tables only (no fields formed on the host)", r.get("gpu_tables_only"))]
    lines += ["| path | best | median | host statement / median |", "|---|---|---|---|"]
    ratio = lambda v: "{:.1f}x".format(host / v["median_ms"]) if host else "not measured"        # noqa: E731
    lines += [f"| {k} | {v['best_ms']:.1f} | {v['median_ms']:.1f} | {ratio(v)} |" for k, v in rows if v]
    if host:
        lines += [f"| host statement, one core | {host:.1f} | | 1.0x |"]
    if "kernels_ms" in r:
        lines += ["", "| library call (HIP events, median) | ms |", "|---|---|"]
        lines += [f"| {k} | {v:.3f} |" for k, v in r["kernels_ms"].items()]
        lines += ["", f"Library calls in all: {sum(r['kernels_ms'].values()):.2f} ms; the rest of the GPU path's wall time is",
                  "host work between the calls (offsets, relabelling of ids, forming the fields of 1,600 problems) and copies."]
    if "agree" in r:
        lines += ["", f"Integer fields of every key of COMBINED_SEQ equal the host statement's: {r['agree']}.  "
                  f"cls_comb_det_av: {r['summary']}."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_eval_bdd.md"))
    ap.add_argument("--sequences", type=int, default=200)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--step-limit", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    opts = ["--sequences", str(args.sequences), "--frames", str(args.frames), "--step-limit", str(args.step_limit),
            "--repeats", str(args.repeats)]
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + opts, capture_output=True, text=True,
                          timeout=2 * args.step_limit + 300)
    line = next((ln for ln in done.stdout.splitlines() if ln.startswith("BENCH_EVAL_BDD ")), None)
    if done.returncode != 0 or line is None:
        sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
        return 1
    r = json.loads(line[len("BENCH_EVAL_BDD "):])
    text = report(r, "python tools/bench_eval_bdd.py " + " ".join(opts[:4]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
