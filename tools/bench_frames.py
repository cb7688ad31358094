"""Raw-frame ingestion on one MI355X (results: profiles/frames_ingest.md).

    python tools/bench_frames.py [--launches 100] [--frames 200] [--repeats 3]

(a) HIP-event time of the resize / normalise kernel, 1080x1920 uint8 -> 800x1440 fp32 padded, next to a stock
    device-to-device copy of its output tensor (`dst.copy_(out)`), same process: median of --launches timed launches
    each after warm-up.  The kernel moves 20 MB, the copy 27.6 MB; the kernel is accepted at <= 2x the copy.
(b) frames/s of SequenceTracker.track() on 1080p uint8 frames in pinned host memory next to step() with lookahead on
    resident normalised 800x1422 frames: same model, same process, --repeats alternating repeats of --frames frames.
(c) context: the CPU restatement of the same definition with 2 threads.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def event_times_ms(fn, warmup, n, blocker):
    """Sorted event times of ``fn``'s device work.  ``blocker()`` queues ~100 us of device work in front of every
    timed launch: the host is then ahead of the queue and the two events bracket the launch's execution alone, not the
    time the host needs to issue it (which for a 10 us kernel called from Python is the larger part)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        blocker()
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in pairs)


def kernel_vs_copy(args):
    from memotr_amd.data.frames import preprocess_frames
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, generator=g).cuda()
    out = preprocess_frames(src).tensors
    dst = torch.empty_like(out)
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")          # 256 MiB: also leaves both cold in cache

    def blocker():
        big.zero_()

    k = event_times_ms(lambda: preprocess_frames(src, out=out), 20, args.launches, blocker)
    c = event_times_ms(lambda: dst.copy_(out), 20, args.launches, blocker)
    read, written = src.numel(), out.numel() * 4
    km, cm = statistics.median(k), statistics.median(c)
    return {"geometry": "1080x1920x3 u8 -> 1x3x800x1440 f32", "launches": args.launches,
            "kernel_us_median": km * 1e3, "kernel_us_min": k[0] * 1e3, "kernel_us_p90": k[int(0.9 * len(k))] * 1e3,
            "copy_us_median": cm * 1e3, "copy_us_min": c[0] * 1e3, "copy_us_p90": c[int(0.9 * len(c))] * 1e3,
            "kernel_over_copy": km / cm, "kernel_bytes": read + written, "copy_bytes": 2 * written,
            "kernel_TBps": (read + written) / km / 1e9, "copy_TBps": 2 * written / cm / 1e9}


def tracking(args):
    from memotr_amd import configs as C
    from memotr_amd.data.frames import preprocess_frames, target_size
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    tracker = SequenceTracker.from_config(model, cfg)
    tracker.result_score_thresh = 0.0
    g = torch.Generator().manual_seed(cfg["SEED"])
    raw = [torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(4)]
    th, tw = target_size(1080, 1920)
    resident = [preprocess_frames(f.to(dev)).tensors[0][:, :th, :tw].contiguous() for f in raw]
    with torch.no_grad():       # births: the n_track best detections of frame 0, then none (as bench.py --workload infer)
        res = model(frame=tensor_list_to_nested_tensor([resident[0]]).to(dev), tracks=tracker.tracks)
        best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
    top = best.topk(args.n_track + 1).values
    tracker.tracker.det_score_thresh = float(top[args.n_track - 1] + top[args.n_track]) / 2
    tracker.tracker.track_score_thresh = 0.0
    tracker.step(resident[0], 1080, 1920)
    tracker.tracker.det_score_thresh = 2.0

    def run_step(n):
        for i in range(n):
            out = tracker.step(resident[i % 4], 1080, 1920, next_image=resident[(i + 1) % 4])
        return out

    def run_track(n):
        for _, out in tracker.track(raw[i % 4] for i in range(n)):
            pass
        return out

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    run_step(args.warmup)
    run_track(args.warmup)
    step_fps, track_fps = [], []
    for _ in range(args.repeats):           # alternating: the two see the same machine state
        step_fps.append(timed(run_step, args.frames))
        track_fps.append(timed(run_track, args.frames))
    e = tracker.core.infer_graphs().encode
    return {"frames_per_repeat": args.frames, "live_tracks": int(len(tracker.tracks[0])),
            "step_resident_fps": step_fps, "track_raw_fps": track_fps,
            "step_resident_fps_median": statistics.median(step_fps), "track_raw_fps_median": statistics.median(track_fps),
            "encode_graph": {"captures": e.captures, "replays": e.replays, "eager": e.eager}}


def cpu_restatement(args):
    from memotr_amd.data.frames import preprocess_frames
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, generator=g)
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    preprocess_frames(src)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        preprocess_frames(src)
        t.append(time.perf_counter() - t0)
    torch.set_num_threads(before)
    return {"threads": 2, "ms_median": statistics.median(t) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-track", type=int, default=20)
    ap.add_argument("--skip-tracking", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py needs a GPU")
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2)
    result = {"device": torch.cuda.get_device_name(0), "kernel": kernel_vs_copy(args)}
    if not args.skip_tracking:
        result["tracking"] = tracking(args)
    result["cpu_restatement"] = cpu_restatement(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
