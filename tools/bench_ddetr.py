"""The Deformable-DETR variant (configs/train_dancetrack_deformable_detr.yaml, USE_DAB: False) on one MI355X: the clip
train step and online tracking (results: profiles/ddetr_graphs.md).

    python tools/bench_ddetr.py [--workload both|train|track] [--config dancetrack_deformable_detr]
                                [--warmup 6] [--repeats 5] [--steps 8] [--frames 60] [--n-track 10]

train  the step of memotr_amd/train_bench.py (clip_forward_backward + clip-grad + AdamW) on ONE synthetic clip resident
       in HBM: 5 frames of 800 x 1333, 10 ground-truth tracks, random-init weights.  ``--repeats`` blocks of ``--steps``
       steps, a device synchronise around each block; reported: the median block's ms per clip step, the fastest and the
       slowest block, and the decoder / updater capture counts before and after the timed window (a capture inside it
       would be a cold step in the figures).
track  ``SequenceTracker.step`` on four resident 800 x 1333 frames with the next frame's encode half queued ahead, as
       bench.py --workload infer drives it: ``--n-track`` tracks are born on frame 0, none after.  ``--repeats`` blocks
       of ``--frames`` frames; reported: frames/s of the median, fastest and slowest block and the capture counts.
``--config dancetrack`` runs the DAB model through the same two loops, for the level the variant should come near.
Prints one JSON line.  No time here is a pass / fail condition; without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W, CLIP_LEN, N_GTS = 800, 1333, 5, 10


def _config(name):
    from memotr_amd.configs import builtin_config
    return dict(builtin_config(name), DEVICE="cuda", AVAILABLE_GPUS="0")


def _blocks(step, warmup, repeats, steps):
    """Wall time of ``repeats`` blocks of ``steps`` calls of ``step(i)``, each block between two device synchronises."""
    i = 0
    for _ in range(warmup):
        step(i)
        i += 1
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            step(i)
            i += 1
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps)
    return times


def _spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def _train_counts(model):
    d, u = model.transformer.decoder.graphs(), model.query_updater.graphs()
    return {"decoder": {"captures": d.captures, "replays": d.replays, "eager": d.eager, "failed": bool(d.failed)},
            "updater": {"captures": u.captures, "replays": u.replays, "eager": u.eager, "failed": bool(u.failed)}}


def bench_train(args, dev):
    from memotr_amd.engine import build_optimizer, clip_forward_backward, clip_to_device, make_synthetic_clip, \
        optimizer_step
    from memotr_amd.models import build_model
    from memotr_amd.models.criterion import build as build_criterion
    from memotr_amd.utils.utils import set_seed
    cfg = _config(args.config)
    set_seed(cfg["SEED"])
    model = build_model(cfg).to(dev).train()
    criterion = build_criterion(cfg)
    optimizer = build_optimizer(cfg, model)
    batch = clip_to_device(make_synthetic_clip(CLIP_LEN, H, W, N_GTS, seed=cfg["SEED"]), dev)
    last = {}

    def step(_):
        loss, _unused = clip_forward_backward(model, criterion, batch, dev, use_dab=cfg["USE_DAB"])
        optimizer_step(model, optimizer, cfg["CLIP_MAX_NORM"])
        last["loss"] = loss

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    before = _train_counts(model)
    times = _blocks(step, 0, args.repeats, args.steps)
    after = _train_counts(model)
    ms = _spread([t * 1e3 for t in times])
    return {"ms_per_clip_step": ms, "frames_per_sec": _spread([CLIP_LEN / t for t in times]),
            "blocks_ms": [round(t * 1e3, 2) for t in times], "steps_per_block": args.steps, "warmup_steps": args.warmup,
            "graphs_before": before, "graphs_after": after, "final_loss": float(last["loss"].detach()),
            "max_memory_MB": torch.cuda.max_memory_allocated() // (1024 ** 2)}


def bench_track(args, dev):
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor
    from memotr_amd.utils.utils import set_seed
    cfg = _config(args.config)
    set_seed(cfg["SEED"])
    model = build_model(cfg).to(dev).eval()
    tracker = SequenceTracker.from_config(model, cfg)
    tracker.result_score_thresh = 0.0
    g = torch.Generator().manual_seed(cfg["SEED"])
    frames = [torch.randn(3, H, W, generator=g).to(dev) for _ in range(4)]
    # random-init weights score every detection ~0.01: the birth threshold comes from frame 0's scores (half way between
    # the n-th and the next one), and no track is born or retired after it
    with torch.no_grad():
        res = model(frame=tensor_list_to_nested_tensor([frames[0]]).to(dev), tracks=tracker.tracks)
        best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
    top = best.topk(args.n_track + 1).values
    tracker.tracker.det_score_thresh = float(top[args.n_track - 1] + top[args.n_track]) / 2
    tracker.tracker.track_score_thresh = 0.0
    tracker.step(frames[0], H, W)
    tracker.tracker.det_score_thresh = 2.0

    def step(i):
        return tracker.step(frames[i % 4], H, W, next_image=frames[(i + 1) % 4])

    times = _blocks(step, 4 * args.warmup, args.repeats, args.frames)
    e, d = tracker.core.infer_graphs().encode, tracker.core.transformer.decoder.infer_graphs().decode
    fps = _spread([1.0 / t for t in times])
    return {"frames_per_sec": fps, "blocks_frames_per_sec": [round(1.0 / t, 2) for t in times],
            "frames_per_block": args.frames, "warmup_frames": 4 * args.warmup, "live_tracks": int(len(tracker.tracks[0])),
            "graphs": {"encode": {"captures": e.captures, "replays": e.replays, "eager": e.eager, "failed": bool(e.failed)},
                       "decoder": {"captures": d.captures, "replays": d.replays, "eager": d.eager,
                                   "failed": bool(d.failed)}},
            "max_memory_MB": torch.cuda.max_memory_allocated() // (1024 ** 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("both", "train", "track"), default="both")
    ap.add_argument("--config", default="dancetrack_deformable_detr")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--n-track", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ddetr: no GPU (nothing here is measured on the host)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"tool": "bench_ddetr", "config": args.config, "frame": [H, W], "clip_len": CLIP_LEN}
    if args.workload in ("both", "train"):
        out["train"] = bench_train(args, dev)
        torch.cuda.empty_cache()
    if args.workload in ("both", "track"):
        out["track"] = bench_track(args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
