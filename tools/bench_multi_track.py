"""B sequences tracked in lockstep against the same B sequences tracked one after another, on one MI355X (results:
profiles/multi_track.md).

    python tools/bench_multi_track.py [--streams 1 2 4 8] [--frames 60] [--repeats 3] [--launches 100]

(a) total frames/s of ``MultiSequenceTracker.track_many_logged`` on B streams next to B runs of the unchanged
    ``SequenceTracker.track_logged``: the full DanceTrack model on 800x1333 uint8 frames in pinned host memory, births as
    in ``bench.py --workload infer`` (the --n-track best detections of a sequence's first frame, then none), same
    process, --repeats alternating repeats after a warm-up of both, medians.
(b) HIP-event time of the two bank kernels alone at B streams of 128 slots, 300 detect rows, C = 256, K = 1: median of
    --launches timed launches behind a ~100 us blocker, as tools/bench_frames.py times its kernel.
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
    from memotr_amd.models.track_bank import TrackBank
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    n_det, cap, C, K = 300, 128, 256, 1
    out = {}
    for B in args.streams:
        g = torch.Generator().manual_seed(B)
        rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()       # noqa: E731
        res = dict(pred_logits=rnd(B, n_det + cap, K) * 2 - 4, pred_bboxes=rnd(B, n_det + cap, 4).sigmoid(),
                   outputs=rnd(B, n_det + cap, C), last_ref_pts=rnd(B, n_det + cap, 4),
                   aux_outputs=[dict(queries=rnd(B, n_det + cap, C))])
        res["pred_logits"][:, n_det:] += 8          # tracks stay; ~2 % of the detect rows are born until the bank is full
        bank = TrackBank(B, cap, num_classes=K, hidden_dim=C, device="cuda")
        t_up = event_times_ms(lambda: clip_ops.bank_update(res, bank, 0.7, 0.5, 5), 20, args.launches, big.zero_)
        bank.boxes.copy_(torch.rand(B, cap, 4, generator=g).cuda() * 0.3 + 0.2)
        seq_frame = torch.zeros(B, 2, dtype=torch.int64, device="cuda")
        ori_wh = torch.tensor([[1920.0, 1080.0]] * B, device="cuda")
        rows_f = torch.empty((args.launches + 21) * B * cap, 5, device="cuda")
        rows_i = torch.empty((args.launches + 21) * B * cap, 4, dtype=torch.int64, device="cuda")
        counters = torch.zeros(2, dtype=torch.int32, device="cuda")
        t_rows = event_times_ms(lambda: clip_ops.bank_result_rows(bank, seq_frame, ori_wh, 0.5, 100, rows_f, rows_i,
                                                                  counters), 20, args.launches, big.zero_)
        out[str(B)] = {"live_per_stream": bank.counters[:, 0].tolist(),
                       "bank_update_us_median": statistics.median(t_up) * 1e3, "bank_update_us_min": t_up[0] * 1e3,
                       "bank_result_rows_us_median": statistics.median(t_rows) * 1e3,
                       "bank_result_rows_us_min": t_rows[0] * 1e3,
                       "rows_per_launch": int(counters[0]) / (args.launches + 20)}
    return out


def tracking(args):
    from memotr_amd import configs as C
    from memotr_amd.data.frames import preprocess_frames
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.inference_multi import MultiSequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.results import BankResultLog, ResultLog
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    g = torch.Generator().manual_seed(cfg["SEED"])
    raw = [torch.randint(0, 256, (800, 1333, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(4)]
    single = SequenceTracker.from_config(model, cfg)
    with torch.no_grad():       # births: the n_track best detections of a sequence's first frame, then none
        res = model(frame=preprocess_frames(raw[0].to(dev)), tracks=single.tracks)
        best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
    top = best.topk(args.n_track + 1).values
    birth = float(top[args.n_track - 1] + top[args.n_track]) / 2
    side = torch.cuda.Stream(dev)           # one lookahead stream for every tracker (profiles/submit_log.md)
    options = dict(dataset_name=cfg["DATASET"], det_score_thresh=birth, track_score_thresh=0.0, result_score_thresh=0.0,
                   miss_tolerance=cfg["MISS_TOLERANCE"], use_dab=cfg["USE_DAB"], side_stream=side)

    def frames(n, close):
        """A sequence of n frames.  Both loops ask for frame i + 1 before they track frame i, so the births end
        (``close()``) when frame 2 is asked for: frame 0 is tracked with the birth threshold, frame 1 without."""
        for i in range(n):
            if i == 2:
                close()
            yield raw[i % 4]

    log, bank_log = ResultLog(dev), BankResultLog(dev, capacity=1 << 16)

    def run_single(B, n):
        rows = 0
        for _ in range(B):
            t = SequenceTracker(model, **options)
            log.reset()
            t.track_logged(frames(n, lambda: setattr(t.tracker, "det_score_thresh", 2.0)), log)
            rows += len(log)
        return rows

    def run_multi(B, n):
        t = MultiSequenceTracker(model, n_streams=B, **options)
        bank_log.reset()
        t.track_many_logged([frames(n, lambda: setattr(t, "det_score_thresh", 2.0)) for _ in range(B)], bank_log)
        t.bank.check()
        return sum(len(r.ids) for r in bank_log.read().values())

    def timed(fn, B, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = fn(B, n)
        torch.cuda.synchronize()
        return B * n / (time.perf_counter() - t0), rows

    out = {}
    for B in args.streams:
        run_single(1, args.warmup)
        run_multi(B, args.warmup)
        fps_single, fps_multi, rows = [], [], []
        for _ in range(args.repeats):           # alternating: the two see the same machine state
            a, rows_a = timed(run_single, B, args.frames)
            b, rows_b = timed(run_multi, B, args.frames)
            fps_single.append(a), fps_multi.append(b), rows.append((rows_a, rows_b))
        med_a, med_b = statistics.median(fps_single), statistics.median(fps_multi)
        out[str(B)] = {"one_after_another_fps": fps_single, "lockstep_fps": fps_multi,
                       "one_after_another_fps_median": med_a, "lockstep_fps_median": med_b,
                       "lockstep_over_one_after_another": med_b / med_a, "rows_per_repeat": rows,
                       "ms_per_lockstep_step": 1e3 * B / med_b}
    e, d = model.infer_graphs().encode, model.transformer.decoder.infer_graphs().decode
    return {"frame": "800x1333x3 u8, pinned host memory", "frames_per_sequence": args.frames, "repeats": args.repeats,
            "n_track": args.n_track, "streams": out,
            "graphs": {"encode": [e.captures, e.replays, e.eager], "decoder": [d.captures, d.replays, d.eager]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-track", type=int, default=20)
    ap.add_argument("--skip-tracking", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_track.py needs a GPU")
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2)
    result = {"device": torch.cuda.get_device_name(0)}
    result["kernel"] = kernel_times(args)
    if not args.skip_tracking:
        result["tracking"] = tracking(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
