"""What the BDD100K error analysis costs on the GPU (memotr_amd/diagnose_bdd100k.py).

    python tools/bench_bdd_events.py [--out profiles/bdd_events.md] [--repeats 10] [--seqs 25]

The input is ``--seqs`` synthetic sequences of 200 frames, BDD100K's clip length (``synthetic_bdd_sequence`` with 20
objects, two ignore regions a frame, and one detection in seven relabelled to another class so that the cross-class
pass has pairs to find).  In one process on the same device inputs, alternating:
  * ``diagnose_bdd100k._device_rows`` with HIP events around its two launches: ``clipops_clear_events_f64`` over the
    S * 8 problems and ``clipops_bdd_cross_class_f64`` over the frames;
  * ``evaluation_bdd100k.device_tables_bdd``, the evaluation this analysis stands beside and the yardstick: HIP events
    around each of its library calls (``bddeval_preproc``, a per-frame assignment like the cross-class launch, and
    ``trackeval_clear``, the walk that keeps only counts, among them), and its wall time to a synchronise;
  * ``bdd_events(device="cuda")`` from device inputs to the tables on the host, wall clock.
A run without a GPU fails; nothing is estimated.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median_best(pairs):
    import numpy as np
    ms = [a.elapsed_time(b) for a, b in pairs]
    return float(np.median(ms)), float(min(ms))


def relabelled(seq, seed, share=1 / 7):
    """``seq`` with that share of the followed objects' detections under another class."""
    import numpy as np
    from memotr_amd import evaluation_bdd100k as B
    rng = np.random.RandomState(seed)
    for ids, classes in zip(seq["tracker_ids"], seq["tracker_classes"]):
        for j in np.flatnonzero((ids < 500000) & (rng.uniform(size=len(ids)) < share)):
            classes[j] = B.CLASS_IDS[(B.CLASS_IDS.index(int(classes[j])) + 1 + rng.randint(7)) % 8]
    return seq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bdd_events.md"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--seqs", type=int, default=25)
    ap.add_argument("--frames", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/bench_bdd_events.py needs a GPU: nothing is measured without one")
    from memotr_amd import diagnose_bdd100k as DB
    from memotr_amd import evaluation_bdd100k as B
    torch.set_num_threads(1)
    packed = B.pack_bdd({f"clip-{i:02d}": relabelled(B.synthetic_bdd_sequence(2000 + i, args.frames, 20, n_regions=2),
                                                     3000 + i) for i in range(args.seqs)})
    dev = packed.to("cuda")
    rows = DB._device_rows(dev)                          # warm-up: module load, LDS opt-in
    tables = B.device_tables_bdd(dev)
    torch.cuda.synchronize()
    same = bool(torch.equal(rows["counts"].reshape(-1, 5)[:, :4].long(), tables["clear_ints"][:, :4])
                and torch.equal(rows["counts"].reshape(-1, 5)[:, 4].long(), tables["clear_ints"][:, 7]))
    t_ours, t_theirs, wall_theirs = {}, {}, []
    for _ in range(args.repeats):                       # alternating: both see the same neighbours
        DB._device_rows(dev, timings=t_ours)
        torch.cuda.synchronize()
        t = time.perf_counter()
        B.device_tables_bdd(dev, timings=t_theirs)
        torch.cuda.synchronize()
        wall_theirs.append((time.perf_counter() - t) * 1e3)
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        events = DB.bdd_events(dev, device="cuda")
        walls.append((time.perf_counter() - t) * 1e3)
    counts = sum(ev.class_counts.sum(0) for ev in events.values())
    pairs = int(sum((ev.gt_cross_partner >= 0).sum() for ev in events.values()))
    ignored = int(sum((ev.tr_kind == DB.IGNORED).sum() for ev in events.values()))
    S, F = len(packed.names), len(packed.gt_off) - 1
    lines = ["# BDD100K error analysis: per-class CLEAR events and the cross-class pass", "",
             f"Command: `python tools/bench_bdd_events.py --seqs {args.seqs} --frames {args.frames}` on one MI355X "
             f"(gfx950; the runtime names it \"{torch.cuda.get_device_name(0)}\").  Kernel times are HIP events around",
             f"one library call, {args.repeats} repeats, the two paths alternating in one process on the same device "
             "inputs; wall times end in",
             "a synchronise or a copy to the host.", "",
             f"Input: {S} sequences x {args.frames} frames ({S * 8} problems, {F} frames, {F * 8} split frames), "
             f"{len(packed.gt_ids)} ground-truth and {len(packed.tr_ids)} tracker detections.", "",
             "| call | launches over | median ms | best ms |", "|---|---|---|---|"]
    for name, over, t in (("clipops_clear_events_f64", f"{S * 8} problems", t_ours),
                          ("clipops_bdd_cross_class_f64", f"{F} frames", t_ours),
                          ("trackeval_clear", f"{S * 8} problems", t_theirs),
                          ("bddeval_preproc", f"{F * 8} split frames", t_theirs)):
        med, best = median_best(t[name])
        lines.append(f"| `{name}` | {over} | {med:.3f} | {best:.3f} |")
    lines += ["", "| call | median ms | best ms |", "|---|---|---|",
              f"| `bdd_events(device=\"cuda\")`, device inputs to tables on the host (wall) | "
              f"{float(np.median(walls)):.1f} | {min(walls):.1f} |",
              f"| `device_tables_bdd`, the same inputs to a synchronise (wall) | "
              f"{float(np.median(wall_theirs)):.1f} | {min(wall_theirs):.1f} |", "",
              f"The five counts of the events launch equal `trackeval_clear`'s: {same}.  Totals: "
              f"{dict(zip(DB.COUNTS, (int(v) for v in counts)))}, {pairs} cross-class pairs, {ignored} ignored tracker boxes.",
              ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
