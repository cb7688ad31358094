"""What annotated output costs on the lockstep tracker, on one MI355X (results: profiles/multi_annotated.md).

    python tools/bench_multi_annotated.py [--streams 1 2 4] [--frames 60] [--repeats 3]

Total frames/s of ``MultiSequenceTracker.track_many_logged`` and of ``track_many_annotated_logged`` (the draw table from
the bank, B overlay launches, one batched JPEG device stage, the Huffman stage on worker threads, a sink that drops the
bytes) on B streams, next to B runs of ``SequenceTracker.track_annotated`` with an ``AnnotatedWriter`` one sequence after
another -- the path that existed before, unchanged here.  The full DanceTrack model on 1080 x 1920 uint8 frames in pinned
host memory, resized to at most 800 x 1333; births as in tools/bench_multi_track.py; same process, --repeats alternating
repeats after a warm-up of all three, medians.  Also the HIP-event time of ``clipops_draw_table_f32`` alone at B streams
of 128 slots (median of --launches launches behind a blocker, as tools/bench_multi_track.py times the bank kernels).
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
    from memotr_amd.functions import clip_ops
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    cap, out = 128, {}
    for B in args.streams:
        g = torch.Generator().manual_seed(B)
        boxes = (torch.rand(B, cap, 4, generator=g) * 0.3 + 0.2).cuda()
        scores = torch.rand(B, cap, 1, generator=g).cuda()
        ids = torch.stack([torch.randperm(cap, generator=g) for _ in range(B)]).cuda()
        ori_wh = torch.tensor([[1920.0, 1080.0]] * B, device="cuda")
        table = torch.empty((B, cap, 16), dtype=torch.int32, device="cuda")
        t = event_times_ms(lambda: clip_ops.draw_table(boxes, scores, ids, ori_wh, 0.5, 100, out=table), 20,
                           args.launches, big.zero_)
        out[str(B)] = {"draw_table_us_median": statistics.median(t) * 1e3, "draw_table_us_min": t[0] * 1e3,
                       "rows_kept": int((table[:, :, 2] >= table[:, :, 0]).sum())}
    return out


def tracking(args):
    from memotr_amd import configs as C
    from memotr_amd.data.frames import preprocess_frames, target_size
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.inference_multi import MultiSequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.render import AnnotatedWriter, MultiAnnotatedWriter
    from memotr_amd.results import BankResultLog
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    g = torch.Generator().manual_seed(cfg["SEED"])
    # (smooth frames with noise on top: a JPEG of pure noise is all entropy stage)
    ramp = torch.linspace(0, 200, 1920)[None, :, None] + torch.linspace(0, 40, 1080)[:, None, None]
    raw = [(ramp + torch.randint(0, 16, (1080, 1920, 3), generator=g) + 10 * i).to(torch.uint8).pin_memory()
           for i in range(4)]
    raw_size = (800, 1333)
    size = target_size(1080, 1920, *raw_size)
    single = SequenceTracker.from_config(model, cfg)
    with torch.no_grad():       # births: the n_track best detections of a sequence's first frame, then none
        res = model(frame=preprocess_frames(raw[0].to(dev), size=size), tracks=single.tracks)
        best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
    top = best.topk(args.n_track + 1).values
    birth = float(top[args.n_track - 1] + top[args.n_track]) / 2
    side = torch.cuda.Stream(dev)
    options = dict(dataset_name=cfg["DATASET"], det_score_thresh=birth, track_score_thresh=0.0, result_score_thresh=0.0,
                   miss_tolerance=cfg["MISS_TOLERANCE"], use_dab=cfg["USE_DAB"], side_stream=side, raw_size=raw_size)

    def frames(n, close):
        for i in range(n):
            if i == 2:
                close()
            yield raw[i % 4]

    bank_log = BankResultLog(dev, capacity=1 << 16)
    written = [0, 0]

    def drop(*args):
        written[0] += 1
        written[1] += len(args[-1])

    def multi(B, n):
        t = MultiSequenceTracker(model, n_streams=B, **options)
        bank_log.reset()
        return t, [frames(n, lambda: setattr(t, "det_score_thresh", 2.0)) for _ in range(B)]

    def run_logged(B, n):
        t, sources = multi(B, n)
        t.track_many_logged(sources, bank_log)
        t.bank.check()

    def run_annotated(B, n):
        t, sources = multi(B, n)
        with MultiAnnotatedWriter(drop, quality=args.quality, threads=args.threads) as writer:
            t.track_many_annotated_logged(sources, writer, bank_log)
        t.bank.check()

    def run_single_annotated(B, n):
        for _ in range(B):
            t = SequenceTracker(model, **options)
            with AnnotatedWriter(drop, quality=args.quality) as writer:
                for _ in t.track_annotated(frames(n, lambda: setattr(t.tracker, "det_score_thresh", 2.0)), writer):
                    pass

    def timed(fn, B, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(B, n)                    # (the writers are closed inside: every file has reached the sink)
        torch.cuda.synchronize()
        return B * n / (time.perf_counter() - t0)

    runs = (("lockstep_logged", run_logged), ("lockstep_annotated_logged", run_annotated),
            ("one_after_another_track_annotated", run_single_annotated))
    out = {}
    for B in args.streams:
        for _, fn in runs:
            fn(B if fn is not run_single_annotated else 1, args.warmup)
        fps = {name: [] for name, _ in runs}
        written[0] = written[1] = 0
        for _ in range(args.repeats):           # alternating: the three see the same machine state
            for name, fn in runs:
                fps[name].append(timed(fn, B, args.frames))
        med = {name: statistics.median(v) for name, v in fps.items()}
        out[str(B)] = {"fps": fps, "fps_median": med,
                       "annotated_over_logged": med["lockstep_annotated_logged"] / med["lockstep_logged"],
                       "annotated_over_track_annotated": med["lockstep_annotated_logged"] /
                       med["one_after_another_track_annotated"],
                       "ms_per_step": {k: 1e3 * B / med[k] for k in ("lockstep_logged", "lockstep_annotated_logged")},
                       "files": written[0], "mean_file_bytes": written[1] / max(written[0], 1)}
    return {"frame": "1080x1920x3 u8, pinned host memory", "resized_to": list(size), "quality": args.quality,
            "huffman_threads": args.threads, "frames_per_sequence": args.frames, "repeats": args.repeats,
            "n_track": args.n_track, "streams": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-track", type=int, default=20)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--skip-tracking", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_annotated.py needs a GPU")
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2 + args.threads)
    result = {"device": torch.cuda.get_device_name(0), "kernel": kernel_times(args)}
    if not args.skip_tracking:
        result["tracking"] = tracking(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
