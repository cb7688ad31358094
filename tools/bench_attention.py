"""What the attention maps cost on the GPU (memotr_amd/attention_maps.py).

    python tools/bench_attention.py [--out profiles/attention_maps.md] [--frames 40] [--repeats 3] [--blocks 15]

All at 1,080 x 1,920, cell 4 (270 x 480 cells), radius 2, six decoder layers of 8 heads x 4 levels x 4 points:
  1. the heat launch (fused entry and points entry) and the blend launch for one plane with 40 rows;
  2. the same for 16 planes with one row each;
  3. a device copy of the frame, the project's usual yardstick;
  4. ``track_attention`` against ``track_annotated`` on the same frames, frames per second of wall clock, graphs on;
  5. the same with ``MEMOTR_INFER_GRAPHS=0``: how much of the cost is the eager decoder, how much the maps.
Kernel times are HIP events around blocks of ``--inner`` launches, warmed up, the median over ``--blocks`` blocks.
A run without a GPU fails; nothing is estimated.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W, CELL, RADIUS, LAYERS, M, L, P = 1080, 1920, 4, 2, 6, 8, 4, 4
SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]        # the pyramid of an 800 x 1333 frame


def block_times_us(fn, inner, blocks):
    """Median and best time of one call in microseconds: events around ``inner`` calls, ``blocks`` times."""
    import torch
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 / inner for a, b in pairs]
    return statistics.median(us), min(us)


def kernels(args, lines):
    import numpy as np
    import torch
    from memotr_amd import MultiScaleDeformableAttention as MSDA
    from memotr_amd import attention_maps as A
    from memotr_amd.data.frames import padded_size, target_size
    g = torch.Generator().manual_seed(7)
    Lq = 340
    shapes = torch.tensor(SHAPES, dtype=torch.int64).cuda()
    th, tw = target_size(H, W, 800, 1333)
    Hp, Wp = padded_size(th, tw)
    sx, sy = A.heat_scale(Wp, W, tw, CELL), A.heat_scale(Hp, H, th, CELL)
    hc, wc = -(-H // CELL), -(-W // CELL)
    fused, points = [], []
    for _ in range(LAYERS):
        ref = torch.rand(1, Lq, 1, 4, generator=g).expand(1, Lq, L, 4).clone()
        ref[..., :2] = ref[..., :2] * 0.8 * torch.tensor([tw / Wp, th / Hp]) + 0.05
        ref[..., 2:] = ref[..., 2:] * 0.2 + 0.05
        proj = torch.randn(1, Lq, 3 * M * L * P, generator=g)
        proj[..., :2 * M * L * P] *= 1.5
        proj, ref = proj.cuda().contiguous(), ref.cuda().contiguous()
        loc, attn = MSDA.fused_points(shapes, proj, ref, M, P)
        fused.append((proj[0], ref[0]))
        points.append((loc[0].contiguous(), attn[0].contiguous()))
    stamp = A.tent_stamp(RADIUS)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).cuda()
    out = torch.empty_like(frame)
    lines += [f"## Kernels: {W} x {H}, cell {CELL} ({wc} x {hc} cells), radius {RADIUS}, {LAYERS} layers x {M * L * P} "
              "points per row", "", "| launch | median us | best us |", "|---|---|---|"]
    for label, n_planes, n_rows in (("1 plane, 40 rows", 1, 40), ("16 planes, 1 row each", 16, 16)):
        rows = torch.arange(300, 300 + n_rows, dtype=torch.int32).cuda()
        planes = (torch.arange(n_rows, dtype=torch.int32) % n_planes).cuda()
        heat, peak = A.attention_heat(points, rows, planes, n_planes, hc, wc, sx, sy, stamp)
        same = A.attention_heat_fused(shapes, fused, M, P, rows, planes, n_planes, hc, wc, sx, sy, stamp)
        assert torch.equal(same[0], heat) and torch.equal(same[1], peak) and int(peak.max()) > 0
        lut = np.repeat(A.HEAT_LUT[None], n_planes, 0)
        A.blend_heat(frame, heat, peak, lut, cell=CELL, out=out)
        runs = (("heat, fused entry (projection + reference points)",
                 lambda: A.attention_heat_fused(shapes, fused, M, P, rows, planes, n_planes, hc, wc, sx, sy, stamp,
                                                heat=heat, peak=peak)),
                ("heat, points entry (materialised loc / attn)",
                 lambda: A.attention_heat(points, rows, planes, n_planes, hc, wc, sx, sy, stamp, heat=heat, peak=peak)),
                ("blend", lambda: A.blend_heat(frame, heat, peak, lut, cell=CELL, out=out)))
        for name, fn in runs:
            med, best = block_times_us(fn, args.inner, args.blocks)
            lines.append(f"| {name}: {label} | {med:.1f} | {best:.1f} |")
    med, best = block_times_us(lambda: out.copy_(frame), args.inner, args.blocks)
    lines += [f"| device copy of the frame ({H * W * 3 / 1e6:.1f} MB) | {med:.1f} | {best:.1f} |", ""]


def tracking(args):
    """One process per setting of MEMOTR_INFER_GRAPHS (run as ``--tracking``): prints 'fps <name> <value>' lines."""
    import torch
    from memotr_amd import configs as C
    from memotr_amd.attention_maps import AttentionWriter
    from memotr_amd.data.frames import preprocess_frames, target_size
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.render import AnnotatedWriter
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    g = torch.Generator().manual_seed(cfg["SEED"])
    ramp = torch.linspace(0, 200, W)[None, :, None] + torch.linspace(0, 40, H)[:, None, None]
    raw = [(ramp + torch.randint(0, 16, (H, W, 3), generator=g) + 10 * i).to(torch.uint8).pin_memory() for i in range(4)]
    raw_size = (800, 1333)
    single = SequenceTracker.from_config(model, cfg)
    with torch.no_grad():       # births: the n_track best detections of the first frame, then none
        res = model(frame=preprocess_frames(raw[0].to(dev), size=target_size(H, W, *raw_size)), tracks=single.tracks)
        best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
    top = best.topk(args.n_track + 1).values
    birth = float(top[args.n_track - 1] + top[args.n_track]) / 2
    side = torch.cuda.Stream(dev)
    options = dict(dataset_name=cfg["DATASET"], det_score_thresh=birth, track_score_thresh=0.0, result_score_thresh=0.0,
                   miss_tolerance=cfg["MISS_TOLERANCE"], use_dab=cfg["USE_DAB"], side_stream=side, raw_size=raw_size)

    def frames(t, n):
        for i in range(n):
            if i == 2:
                t.tracker.det_score_thresh = 2.0
            yield raw[i % 4]

    def drop(idx, data):
        pass

    def annotated(n):
        t = SequenceTracker(model, **options)
        with AnnotatedWriter(drop, quality=85) as writer:
            for _ in t.track_annotated(frames(t, n), writer):
                pass

    def attention(n, ids=None):
        t = SequenceTracker(model, **options)
        with AttentionWriter(drop, quality=85, cell=CELL, radius=RADIUS) as writer:
            for _ in t.track_attention(frames(t, n), writer, ids=ids):
                pass

    runs = (("track_annotated", annotated), ("track_attention", attention),
            ("track_attention_16_ids", lambda n: attention(n, list(range(16)))))
    for _, fn in runs:
        fn(args.warmup)
    fps = {name: [] for name, _ in runs}
    for _ in range(args.repeats):           # alternating: the runs see the same machine state
        for name, fn in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.frames)
            torch.cuda.synchronize()
            fps[name].append(args.frames / (time.perf_counter() - t0))
    for name, v in fps.items():
        print(f"fps {name} {statistics.median(v):.2f} {max(v):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps.md"))
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--n-track", type=int, default=40)
    ap.add_argument("--commit", default="", help="what the numbers were taken on, for the report's first line")
    ap.add_argument("--skip-tracking", action="store_true")
    ap.add_argument("--tracking", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/bench_attention.py needs a GPU: nothing is measured without one")
    torch.set_num_threads(1)
    if args.tracking:
        tracking(args)
        return 0
    lines = ["# Attention maps: the heat and blend kernels, and track_attention next to track_annotated", "",
             f"Command: `python tools/bench_attention.py` on {torch.cuda.get_device_name(0)}"
             + (f", {args.commit}" if args.commit else "") + ".  Kernel times are HIP events around blocks of "
             f"{args.inner} launches after a warm-up block, the median and the best of {args.blocks} blocks.", ""]
    kernels(args, lines)
    if not args.skip_tracking:
        lines += [f"## Tracking: full DanceTrack model (random weights), {W} x {H} frames from pinned memory, {args.n_track} "
                  f"tracks, {args.frames} frames per pass, JPEG quality 85 into a sink that drops the bytes", "",
                  f"Frames per second of wall clock, median (best) of {args.repeats} alternating passes, one process per "
                  "setting.", "", "| MEMOTR_INFER_GRAPHS | run | frames / s |", "|---|---|---|"]
        for graphs in ("1", "0"):
            env = dict(os.environ, MEMOTR_INFER_GRAPHS=graphs)
            cmd = [sys.executable, os.path.abspath(__file__), "--tracking", "--frames", str(args.frames), "--warmup",
                   str(args.warmup), "--repeats", str(args.repeats), "--n-track", str(args.n_track)]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            rows = [ln.split() for ln in res.stdout.splitlines() if ln.startswith("fps ")]
            if res.returncode != 0 or not rows:
                lines.append(f"| {graphs} | not measured: the run failed ({res.stderr.strip().splitlines()[-1:]}) | |")
                continue
            lines += [f"| {graphs} | `{name}` | {med} ({best}) |" for _, name, med, best in rows]
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
