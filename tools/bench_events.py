"""What the error analysis costs on the GPU (memotr_amd/diagnose.py), on the workloads of tools/bench_eval.py.

    python tools/bench_events.py [--out profiles/clear_events.md] [--repeats 20] [--frames 64]

Per workload (``bench_eval.WORKLOADS``: dancetrack, mot17; the preprocessed arrays are made once, on the host):
  * ``clipops_clear_events_f64`` next to ``trackeval_clear`` on the same device arrays, alternating, HIP events around
    each call, median and best of the repeats; the counts of the two are compared;
  * ``clear_events(device="cuda")`` from packed device inputs to the events on the host, wall clock;
  * ``clipops_error_table_f64`` for one sequence (1,920 x 1,080), HIP events.
Then, at 1,080 x 1,920 on ``--frames`` frames of the first dancetrack sequence, from the same JPEG files to JPEG files:
``write_error_frames(device="cuda")`` against ``AnnotatedWriter`` fed by ``decode_jpegs`` (the tracker rows of each
frame as its result), frames per second of wall clock, best of three passes.
A run without a GPU fails; nothing is estimated.
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def median_best(pairs):
    import numpy as np
    ms = [a.elapsed_time(b) for a, b in pairs]
    return float(np.median(ms)), float(min(ms))


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def kernels(name, w, repeats, lines):
    import numpy as np
    import torch
    from bench_eval import WORKLOADS  # noqa: F401  (the workloads are that tool's)
    from memotr_amd import _track_eval_lib as L
    from memotr_amd import diagnose as D
    from memotr_amd import evaluation as E
    seqs = {f"{name}-{i:02d}": E.synthetic_sequence(1000 + i, w["n_frames"], w["n_objects"],
                                                    n_distractors=w["n_distractors"], n_false=w["n_false"])
            for i in range(w["n_seqs"])}
    packed = E.pack_sequences(seqs)
    _, sim, d = E._preprocess_host(packed, "MOT17")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                             # noqa: E731
    inputs = [up(sim), up(d["sim_off"]), up(d["gt_off"]), up(d["tr_off"]), up(d["gt_ids"]), up(d["tr_ids"]),
              up(d["seq_off"]), up(d["n_gt_ids"])]
    sizes = [int(np.diff(d["gt_off"]).max()), int(np.diff(d["tr_off"]).max()), int(d["n_gt_ids"].max())]
    S, n_gt, n_tr = len(packed.names), len(d["gt_ids"]), len(d["tr_ids"])
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")                   # noqa: E731
    outs = [new(n_gt), new(n_gt), new(n_tr), new(S, 5), new(S)]
    ints, motp, status = new(S, 8), torch.empty(S, dtype=torch.float64, device="cuda"), new(S)
    st = torch.cuda.current_stream().cuda_stream

    def events():
        D.launch_clear_events(*inputs, *sizes, *outs)

    def clear():
        L.check(L.lib.trackeval_clear(*[t.data_ptr() for t in inputs[:7]], S, inputs[7].data_ptr(), *sizes,
                                      ints.data_ptr(), motp.data_ptr(), status.data_ptr(), st), "trackeval_clear")

    events(), clear()                                   # warm-up: module load, LDS opt-in
    torch.cuda.synchronize()
    t_events, t_clear = [], []
    for _ in range(repeats):                            # alternating: both see the same neighbours
        t_events.append(timed(events))
        t_clear.append(timed(clear))
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[3][:, :4], ints[:, :4]) and torch.equal(outs[3][:, 4], ints[:, 7]))
    dev = packed.to("cuda")
    D.clear_events(dev, device="cuda")
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        evs = D.clear_events(dev, device="cuda")
        walls.append((time.perf_counter() - t) * 1e3)
    ev = evs[packed.names[0]]
    D.error_table_device(ev, 1920, 1080, "cuda")
    torch.cuda.synchronize()
    up_ev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()                  # noqa: E731
    arrays = [up_ev(ev.gt_boxes, np.float64), up_ev(ev.tr_boxes, np.float64), up_ev(ev.gt_off, np.int32),
              up_ev(ev.tr_off, np.int32), up_ev(ev.gt_ids, np.int32), up_ev(ev.tr_ids, np.int32),
              up_ev(ev.gt_kind, np.int32), up_ev(ev.tr_kind, np.int32)]
    rows = ev.max_drawn_rows()
    table = new(ev.n_frames, rows, 16)
    t_table = [timed(lambda: D.launch_error_table(*arrays, rows, 1920, 1080, False, 2, table)) for _ in range(repeats)]
    torch.cuda.synchronize()
    (e_med, e_best), (c_med, c_best), (t_med, t_best) = median_best(t_events), median_best(t_clear), median_best(t_table)
    total = evs and {k: sum(e.counts()[k] for e in evs.values()) for k in D.COUNTS}
    lines += [f"## {name}: {w['n_seqs']} sequences x {w['n_frames']} frames, {n_gt} ground-truth and {n_tr} tracker "
              "detections after preprocessing", "",
              "| call | median ms | best ms |", "|---|---|---|",
              f"| `clipops_clear_events_f64`, all sequences in one launch | {e_med:.3f} | {e_best:.3f} |",
              f"| `trackeval_clear`, the same arrays | {c_med:.3f} | {c_best:.3f} |",
              f"| `clipops_error_table_f64`, one sequence: {ev.n_frames} frames x {rows} rows | {t_med:.3f} | {t_best:.3f} |",
              f"| `clear_events(device=\"cuda\")`, device inputs to events on the host (wall) | {float(np.median(walls)):.1f} "
              f"| {min(walls):.1f} |", "",
              f"Counts of the two kernels equal: {same}.  Totals: {total}.", ""]
    return ev


def frames_per_second(ev, n_frames, lines):
    import numpy as np
    import torch
    from memotr_amd import diagnose as D
    from memotr_amd.data.jpeg import decode_jpegs
    from memotr_amd.data.jpeg_write import encode_jpegs
    from memotr_amd.render import AnnotatedWriter
    H, W, n = 1080, 1920, min(n_frames, ev.n_frames)
    sub = D.SequenceEvents(ev.name, ev.gt_off[:n + 1], ev.tr_off[:n + 1],
                           *[getattr(ev, k)[:ev.gt_off[n]] for k in ("gt_ids", "gt_boxes", "gt_kind", "gt_frag",
                                                                     "gt_partner", "gt_iou")],
                           *[getattr(ev, k)[:ev.tr_off[n]] for k in ("tr_ids", "tr_boxes", "tr_kind", "tr_partner")])
    with tempfile.TemporaryDirectory() as tmp:
        yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        g = torch.Generator(device="cuda").manual_seed(3)
        paths = []
        for c0 in range(0, n, 16):
            batch = []
            for t in range(c0, min(c0 + 16, n)):
                px = torch.stack([(xx + 5 * t) % 256, (yy * 2 + 3 * t) % 256, (xx + yy) % 256], -1)
                batch.append((px + torch.randint(-6, 7, px.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8))
            for t, data in zip(range(c0, c0 + len(batch)), encode_jpegs(batch, quality=90)):
                paths.append(os.path.join(tmp, f"{t + 1:08d}.jpg"))
                with open(paths[-1], "wb") as f:
                    f.write(data)

        def errors():
            return len(D.write_error_frames(sub, paths, os.path.join(tmp, "errors"), quality=85, font_scale=2,
                                            device="cuda"))

        def annotated():
            with AnnotatedWriter(os.path.join(tmp, "annotated"), quality=85, font_scale=2) as writer:
                for c0 in range(0, n, 16):
                    frames = decode_jpegs(paths[c0:c0 + 16], "cuda")
                    for k in range(len(frames)):
                        t0, t1 = sub.tr_off[c0 + k], sub.tr_off[c0 + k + 1]
                        b = sub.tr_boxes[t0:t1]
                        xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)
                        writer.add(c0 + k, frames[k], (torch.from_numpy(sub.tr_ids[t0:t1].astype(np.int64)),
                                                      torch.from_numpy(xyxy)))
            return n

        rates = {}
        for label, fn in (("write_error_frames(device=\"cuda\")", errors), ("AnnotatedWriter behind decode_jpegs", annotated)):
            fn()                                        # warm-up
            best = 0.0
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                done = fn()
                torch.cuda.synchronize()
                best = max(best, done / (time.perf_counter() - t))
            rates[label] = best
    lines += [f"## Annotated frames, {W} x {H}, {n} frames, JPEG files to JPEG files (quality 85, 4:2:0)", "",
              "| path | frames / s (best of 3 passes) |", "|---|---|"]
    lines += [f"| `{k}` | {v:.1f} |" for k, v in rates.items()] + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clear_events.md"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/bench_events.py needs a GPU: nothing is measured without one")
    from bench_eval import WORKLOADS
    torch.set_num_threads(1)
    cmd = "python tools/bench_events.py" + (f" --only {args.only}" if args.only else "")
    lines = ["# Error analysis: the events kernel, the error table and the annotated frames", "",
             f"Command: `{cmd}` on {torch.cuda.get_device_name(0)}.  Kernel times are HIP events around one library call,",
             f"{args.repeats} repeats, the two CLEAR kernels alternating; wall times end in a synchronise.", ""]
    first = None
    for name, w in WORKLOADS.items():
        if args.only and name != args.only:
            continue
        ev = kernels(name, w, args.repeats, lines)
        first = first or ev
    frames_per_second(first, args.frames, lines)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
