"""One sequence tracked under S threshold settings in one pass (inference_sweep.SweepTracker) against S passes of the
unchanged one-sequence tracker, on one MI355X (results: profiles/threshold_sweep.md).

    python tools/bench_sweep.py [--settings 1 2 4 8] [--frames 40] [--blocks 5]

The full DanceTrack model on 800x1333 uint8 frames resident on the device, births as in tools/bench_multi_track.py (the
--n-track best detections of the first frame, then none; every setting holds the same values, so every stream carries
the same tracks), one process.  Per S, medians of --blocks alternating blocks with the fastest and the slowest:
(a) ms per frame of ``SweepTracker.track_logged`` with S settings;
(b) S x the ms per frame of ``SequenceTracker.track_logged``: what sweeping S settings costs without this tracker;
(c) ms per step of ``MultiSequenceTracker.track_many_logged`` fed the same frames on S streams (S encodes per step).
And how a step of (a) splits: encode, broadcast copy, decoder, bookkeeping (bank update, query updater, count copy,
result rows), each stage alone between two device synchronisations -- without the overlap of the lookahead, so the
stages add up to more than (a).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("MEMOTR_REQUIRE_GRAPHS", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "fastest": min(values), "slowest": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--n-track", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep.py needs a GPU")
    from memotr_amd import configs as C
    from memotr_amd.data.frames import preprocess_frames
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.inference_multi import MultiSequenceTracker, _Step
    from memotr_amd.inference_sweep import SweepTracker
    from memotr_amd.models import build_model
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.results import BankResultLog, ResultLog
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    from memotr_amd.utils.utils import set_seed
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2)
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    g = torch.Generator().manual_seed(cfg["SEED"])
    raw = [torch.randint(0, 256, (800, 1333, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(4)]
    with torch.no_grad():       # births: the n_track best detections of the first frame, then none
        res = model(frame=preprocess_frames(raw[0]), tracks=SequenceTracker.from_config(model, cfg).tracks)
        best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
    top = best.topk(args.n_track + 1).values
    birth = float(top[args.n_track - 1] + top[args.n_track]) / 2
    side = torch.cuda.Stream(dev)
    shared = dict(dataset_name=cfg["DATASET"], use_dab=cfg["USE_DAB"], side_stream=side)
    setting = dict(det_score_thresh=birth, track_score_thresh=0.0, result_score_thresh=0.0,
                   miss_tolerance=cfg["MISS_TOLERANCE"])

    def frames(n, close):
        """Both loops ask for frame i + 1 before they track frame i: the births end when frame 2 is asked for."""
        for i in range(n):
            if i == 2:
                close()
            yield raw[i % 4]

    log, bank_log = ResultLog(dev), BankResultLog(dev, capacity=1 << 16)

    def run_single(S, n):
        t = SequenceTracker(model, **shared, **setting)
        log.reset()
        t.track_logged(frames(n, lambda: setattr(t.tracker, "det_score_thresh", 2.0)), log)
        return len(log)

    def run_sweep(S, n):
        t = SweepTracker(model, [setting] * S, **shared)
        bank_log.reset()
        t.track_logged(frames(n, lambda: t.thresholds.det.fill_(2.0)), bank_log)
        return sum(len(r.ids) for r in bank_log.read().values())

    def run_multi(S, n):
        t = MultiSequenceTracker(model, n_streams=S, **shared, **setting)
        bank_log.reset()
        t.track_many_logged([frames(n, lambda: setattr(t, "det_score_thresh", 2.0)) for _ in range(S)], bank_log)
        t.bank.check()
        return sum(len(r.ids) for r in bank_log.read().values())

    def ms_per_frame(fn, S, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = fn(S, n)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, rows

    def stages(S, n):
        """The stages of a sweep step one at a time, the device drained between them."""
        t = SweepTracker(model, [setting] * S, **shared)
        t.begin(S)
        seq_frame = torch.tensor([[k, 0] for k in range(S)], device=dev)
        ori_wh = torch.tensor([[1333.0, 800.0]] * S, device=dev)
        bank_log.reset()
        times = {"encode": [], "broadcast": [], "decoder": [], "bookkeeping": []}

        def timed(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
            return out

        def books(res):
            t._bank_update(res)
            t.core.query_updater.update_bank(t.bank)
            t._watch_counts()
            bank_log.append_streams(t.bank, seq_frame, ori_wh, t.thresholds)

        with torch.no_grad():
            for i in range(n + 4):
                if i == 1:
                    t.thresholds.det.fill_(2.0)
                enc = timed("encode", lambda: t._encoded(_Step([raw[i % 4]]), False))
                wide = timed("broadcast", lambda: t._broadcast(enc))
                res = timed("decoder", lambda: MultiSequenceTracker._decode(t, wide))
                timed("bookkeeping", lambda: books(res))
        return {name: statistics.median(v[4:]) for name, v in times.items()}

    out = {}
    for S in args.settings:
        run_single(1, args.warmup), run_sweep(S, args.warmup), run_multi(S, args.warmup)
        a, b, c, rows = [], [], [], []
        for _ in range(args.blocks):            # alternating: the three see the same machine state
            one, rows_b = ms_per_frame(run_single, 1, args.frames)
            swept, rows_a = ms_per_frame(run_sweep, S, args.frames)
            multi, rows_c = ms_per_frame(run_multi, S, args.frames)
            a.append(swept), b.append(S * one), c.append(multi), rows.append((rows_a, S * rows_b, rows_c))
        out[str(S)] = {"a_sweep_ms_per_frame": spread(a), "b_S_passes_ms_per_frame": spread(b),
                       "c_lockstep_ms_per_step": spread(c), "b_over_a": statistics.median(b) / statistics.median(a),
                       "rows_per_block": rows, "stages_ms": stages(S, args.frames)}
    e, d = model.infer_graphs().encode, model.transformer.decoder.infer_graphs().decode
    print(json.dumps({"device": torch.cuda.get_device_name(0), "frame": "800x1333x3 u8, resident on the device",
                      "frames_per_block": args.frames, "blocks": args.blocks, "n_track": args.n_track, "settings": out,
                      "graphs": {"encode": [e.captures, e.replays, e.eager], "decoder": [d.captures, d.replays, d.eager]}}))


if __name__ == "__main__":
    main()
