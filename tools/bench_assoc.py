"""What the association analysis costs on the GPU (memotr_amd/association.py), on the workloads of tools/bench_eval.py.

    python tools/bench_assoc.py [--out profiles/association.md] [--repeats 10] [--only dancetrack]

Per workload (``bench_eval.WORKLOADS``: dancetrack, mot17), in one process on the same device inputs:
  * ``device_association_tables`` and ``evaluation.device_tables`` alternating, HIP events around each library call:
    ``clipops_hota_events_f64`` beside ``trackeval_hota_match``, ``clipops_identity_pairs_i32`` beside
    ``trackeval_identity`` (the pinned library's kernels solve the same assignments and keep less), and
    ``clipops_assoc_reduce_f64`` beside ``trackeval_hota_reduce``; median and best of the repeats; the ``matches`` tables
    of the two are compared;
  * ``association(device="cuda")`` from packed device inputs to the tables on the host, wall clock;
  * ``clipops_timeline_u8`` for the first sequence, HIP events, and ``timeline(device="cuda")`` with its upload, wall.
A run without a GPU fails; nothing is estimated.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

PAIRS = (("clipops_hota_events_f64", "trackeval_hota_match"), ("clipops_identity_pairs_i32", "trackeval_identity"),
         ("clipops_assoc_reduce_f64", "trackeval_hota_reduce"))


def median_best(pairs):
    import numpy as np
    ms = [a.elapsed_time(b) for a, b in pairs]
    return float(np.median(ms)), float(min(ms))


def workload(name, w, repeats, lines):
    import numpy as np
    import torch
    from memotr_amd import association as A
    from memotr_amd import evaluation as E
    seqs = {f"{name}-{i:02d}": E.synthetic_sequence(1000 + i, w["n_frames"], w["n_objects"],
                                                    n_distractors=w["n_distractors"], n_false=w["n_false"])
            for i in range(w["n_seqs"])}
    packed = E.pack_sequences(seqs)
    dev = packed.to("cuda")
    ours = A.device_association_tables(dev)              # warm-up: module load, LDS opt-in
    theirs = E.device_tables(dev)
    torch.cuda.synchronize()
    same = bool(torch.equal(ours["matches"], theirs["matches"]))
    t_ours, t_theirs = {}, {}
    for _ in range(repeats):                            # alternating: both see the same neighbours
        A.device_association_tables(dev, timings=t_ours)
        E.device_tables(dev, timings=t_theirs)
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        assoc = A.association(dev, device="cuda")
        walls.append((time.perf_counter() - t) * 1e3)
    first = assoc[packed.names[0]]
    G, F = len(first.gt_identities), first.n_frames
    A.timeline(first, device="cuda")
    rows = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in A._timeline_rows(first)]
    image = torch.empty((G * 6, F * 2, 3), dtype=torch.uint8, device="cuda")
    spare = torch.zeros(2, dtype=torch.float64, device="cuda")          # (kept outside the events, as the tables' is)
    t_line = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        A.launch_timeline(*rows, G, 9, 2, 6, False, image, spare)
        b.record()
        t_line.append((a, b))
    torch.cuda.synchronize()
    line_walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        A.timeline(first, device="cuda").cpu()
        line_walls.append((time.perf_counter() - t) * 1e3)
    total = {k: sum(int(np.sum(a.totals()[k][9] if k == "HOTA_TP" else a.totals()[k])) for a in assoc.values())
             for k in ("HOTA_TP", "IDTP", "IDFN", "IDFP")}
    lines += [f"## {name}: {w['n_seqs']} sequences x {w['n_frames']} frames, {len(packed.gt_ids)} ground-truth and "
              f"{len(packed.tr_ids)} tracker detections", "",
              "| call | median ms | best ms | its counterpart | median ms | best ms | ratio of medians |",
              "|---|---|---|---|---|---|---|"]
    for new, old in PAIRS:
        (n_med, n_best), (o_med, o_best) = median_best(t_ours[new]), median_best(t_theirs[old])
        lines.append(f"| `{new}` | {n_med:.3f} | {n_best:.3f} | `{old}` | {o_med:.3f} | {o_best:.3f} | "
                     f"{n_med / o_med:.2f}x |")
    l_med, l_best = median_best(t_line)
    lines += ["", "| call | median ms | best ms |", "|---|---|---|",
              f"| `clipops_timeline_u8`, one sequence: {G} identities x {F} frames, cells 2 x 6 | {l_med:.3f} | {l_best:.3f} |",
              f"| `timeline(device=\"cuda\")`, rows on the host to the image on the host (wall) | "
              f"{float(np.median(line_walls)):.2f} | {min(line_walls):.2f} |",
              f"| `association(device=\"cuda\")`, device inputs to tables on the host (wall) | "
              f"{float(np.median(walls)):.1f} | {min(walls):.1f} |", "",
              f"`matches` counted from the new events equals `trackeval_hota_match`'s: {same}.  "
              f"Totals (HOTA_TP at 0.5): {total}.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "association.md"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/bench_assoc.py needs a GPU: nothing is measured without one")
    from bench_eval import WORKLOADS
    torch.set_num_threads(1)
    cmd = "python tools/bench_assoc.py" + (f" --only {args.only}" if args.only else "")
    lines = ["# Association analysis: HOTA events, identity pairs, the per-identity reduction and the timeline", "",
             f"Command: `{cmd}` on {torch.cuda.get_device_name(0)}.  Kernel times are HIP events around one library call,",
             f"{args.repeats} repeats, the two paths alternating in one process on the same device inputs; wall times end in",
             "a copy to the host.", ""]
    for name, w in WORKLOADS.items():
        if args.only and name != args.only:
            continue
        workload(name, w, args.repeats, lines)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
