"""The submit frame loop on one MI355X, with and without the per-frame result read (results: profiles/submit_log.md).

    python tools/bench_submit.py [--frames 150] [--repeats 5] [--launches 100]

(a) frames/s of ``SequenceTracker.track()`` + ``mot_lines`` (every frame's reportable tracks leave the device through
    ``_report``: packed copy, event wait, host filter) next to ``track_logged`` + ``ResultLog.mot_lines`` (one launch
    per frame, one read per sequence): the full model on 800x1333 uint8 frames in pinned host memory, births as in
    ``bench.py --workload infer`` (the --n-track best detections of frame 0, then none), same process, same tracker,
    --repeats alternating repeats of --frames frames after a warm-up of both.  The lines of the two paths are compared once.
(b) HIP-event time of the result-row kernel alone at n = 16, 128 and 512 live tracks (K = 1): median of --launches
    timed launches behind a ~100 us blocker, as tools/bench_frames.py times its kernel.
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

from bench_frames import event_times_ms  # noqa: E402


def kernel_times(args):
    from memotr_amd.results import ResultLog
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    out = {}
    for n in (16, 128, 512):
        g = torch.Generator().manual_seed(n)
        boxes = (torch.rand(n, 4, generator=g) * 0.3 + 0.2).cuda()
        scores = torch.rand(n, 1, generator=g).cuda()
        ids, labels = torch.randperm(n, generator=g).cuda(), torch.zeros(n, dtype=torch.int64).cuda()
        log = ResultLog("cuda", capacity=(args.launches + 21) * n)             # no growth inside the timed launches
        t = event_times_ms(lambda: log.append(boxes, scores, ids, labels, 0, 1080, 1920, 0.5, 100), 20, args.launches,
                           big.zero_)
        rows = len(log)
        out[str(n)] = {"us_median": statistics.median(t) * 1e3, "us_min": t[0] * 1e3, "us_p90": t[int(0.9 * len(t))] * 1e3,
                       "rows_kept_per_launch": rows / (args.launches + 20)}
    return out


def tracking(args):
    from memotr_amd import configs as C
    from memotr_amd.data.frames import preprocess_frames
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.results import ResultLog
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    g = torch.Generator().manual_seed(cfg["SEED"])
    raw = [torch.randint(0, 256, (800, 1333, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(4)]

    def tracker():      # births: the n_track best detections of frame 0, then none (as bench.py --workload infer)
        t = SequenceTracker.from_config(model, cfg)
        t.result_score_thresh = 0.0
        with torch.no_grad():
            res = model(frame=preprocess_frames(raw[0].to(dev)), tracks=t.tracks)
            best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
        top = best.topk(args.n_track + 1).values
        t.tracker.det_score_thresh = float(top[args.n_track - 1] + top[args.n_track]) / 2
        t.tracker.track_score_thresh = 0.0
        t.step_raw(raw[0])
        t.tracker.det_score_thresh = 2.0
        return t

    log = ResultLog(dev)

    def run_track(t, n):
        lines = []
        for idx, out in t.track(raw[i % 4] for i in range(n)):
            lines += t.mot_lines(idx, out)
        return lines

    def run_logged(t, n):
        log.reset()
        t.track_logged((raw[i % 4] for i in range(n)), log)
        return log.mot_lines(t.dataset_name)

    def timed(fn, t, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lines = fn(t, n)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), len(lines)

    # ONE tracker for both paths: a tracker's side stream is a pool stream of its own, and which hardware queue it lands
    # on (4 per process by default) decides whether the next frame's encode half overlaps this frame's updater -- two
    # trackers differ by more than the two paths do (profiles/submit_log.md)
    t = tracker()
    run_track(t, args.warmup)
    run_logged(t, args.warmup)
    track_fps, logged_fps, rows = [], [], []
    for _ in range(args.repeats):           # alternating: the two see the same machine state
        fps, n_a = timed(run_track, t, args.frames)
        track_fps.append(fps)
        fps, n_b = timed(run_logged, t, args.frames)
        logged_fps.append(fps)
        rows.append((n_a, n_b))
    same = run_track(tracker(), args.warmup) == run_logged(tracker(), args.warmup)      # two fresh, equal trackers
    e = model.infer_graphs().encode
    med_a, med_b = statistics.median(track_fps), statistics.median(logged_fps)
    return {"frame": "800x1333x3 u8, pinned host memory", "frames_per_repeat": args.frames, "repeats": args.repeats,
            "live_tracks": int(len(t.tracks[0])), "rows_per_repeat": rows, "lines_equal": same,
            "track_mot_lines_fps": track_fps, "track_logged_fps": logged_fps,
            "track_mot_lines_fps_median": med_a, "track_logged_fps_median": med_b,
            "track_mot_lines_fps_spread": (max(track_fps) - min(track_fps)) / med_a,
            "track_logged_fps_spread": (max(logged_fps) - min(logged_fps)) / med_b,
            "logged_over_track": med_b / med_a,
            "encode_graph": {"captures": e.captures, "replays": e.replays, "eager": e.eager}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-track", type=int, default=20)
    ap.add_argument("--skip-tracking", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_submit.py needs a GPU")
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2)
    result = {"device": torch.cuda.get_device_name(0)}
    if not args.skip_tracking:
        result["tracking"] = tracking(args)
    result["kernel"] = kernel_times(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
