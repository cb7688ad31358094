"""The clip loader (memotr_amd/data/loader.py) on one MI355X: (a) the loader alone, (b) the DanceTrack clip train step
fed by it next to the same step fed by the same clips held resident on the device.  Results: profiles/clip_loader.md.

    python tools/bench_loader.py [--frames 24] [--clip-len 5] [--repeats 3] [--prefetch 2] [--decode-threads 2]
                                 [--only a|b] [--out FILE]

The tool writes its own DanceTrack-layout tree: one sequence of ``--frames`` 1080 x 1920 frames (smooth gradients that
move from frame to frame plus Gaussian noise of sigma 2; profiles/jpeg_decode.md: noise inflates the streams and with
them the entropy stage, so the stream size is reported), encoded by ``encode_jpegs`` at quality 90, 4:2:0, with boxes
that drift.  The augmentation plan is the plain branch to 800 x 1422 (the short side 800 of a 1080p frame) with the
flip and the HSV gains still drawn per clip: ONE geometry, so that every clip replays the same captured graphs and the
two sides of (b) differ in where the clip comes from and in nothing else.

(a) clips/s of ``for batch in loader.epoch(0)`` with a device synchronise at the end; per clip the producer thread's
    CPU time (``time.thread_time``; the library's entropy threads are NOT in it: the process CPU time per clip is
    reported next to it) and the producer's wall time per stage: reading the files, ``decode_jpegs`` (entropy stage +
    queueing the upload and two launches) and augment + ground-truth packing (queueing only); the entropy stage alone,
    ``_entropy_batch`` on the same streams and thread count, separates the first of these.
(b) ms per clip step (``clip_forward_backward`` + ``optimizer_step``) over one epoch, loader-fed and resident-fed,
    ``--repeats`` alternating repeats after a warm-up epoch of each; the resident clips are the loader's own batches of
    the same epoch, collected before the timing and kept on the device (frames and ground truth: what
    ``clip_to_device`` gives).  Target: loader-fed median <= resident-fed median + (max - min) of the resident repeats.
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 1080, 1920
FINAL = (800, 1422)


def frame(index, device, h=H, w=W):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device),
                            torch.arange(w, dtype=torch.float32, device=device), indexing="ij")
    g = torch.Generator(device=device)
    g.manual_seed(index)
    px = torch.stack([96 + 80 * torch.sin((xx + 9 * index) / 170.0) + 40 * torch.cos(yy / 90.0),
                      128 + 90 * torch.sin((yy + 5 * index) / 130.0) + 0 * xx,
                      110 + 70 * torch.cos((xx + yy + 7 * index) / 210.0)], -1)
    px = px + 2.0 * torch.randn(px.shape, generator=g, device=device)
    return px.clamp_(0, 255).to(torch.uint8)


def write_tree(root, n_frames, device, n_gts=8, h=H, w=W):
    from memotr_amd.data import encode_jpegs
    seq = os.path.join(root, "DanceTrack", "train", "dancetrack0001")
    os.makedirs(os.path.join(seq, "img1"))
    os.makedirs(os.path.join(seq, "gt"))
    sizes, lines = [], []
    for lo in range(0, n_frames, 8):
        idx = list(range(lo, min(lo + 8, n_frames)))
        frames = torch.stack([frame(i, device, h, w) for i in idx])
        for i, data in zip(idx, encode_jpegs(frames, threads=4, quality=90, subsampling="4:2:0")):
            with open(os.path.join(seq, "img1", f"{i + 1:08d}.jpg"), "wb") as f:
                f.write(data)
            sizes.append(len(data))
    for t in range(1, n_frames + 1):
        for k in range(n_gts):
            x, y, w, h = 100 + 200 * k + 6 * t, 150 + 60 * (k % 3) + 3 * t, 90 + 10 * k, 260 + 15 * k
            lines.append(f"{t},{k + 1},{x},{y},{w},{h},1,1,1\n")
    with open(os.path.join(seq, "gt", "gt.txt"), "w") as f:
        f.write("".join(lines))
    return sizes


def make_dataset(root, clip_len):
    from memotr_amd.configs import data_config
    from memotr_amd.data.augment import ClipAugment, sample_clip_augment
    from memotr_amd.data.datasets import DanceTrackDataset

    class OneGeometry(DanceTrackDataset):
        def sample_plan(self, h, w, rng, np_rng, static=False):
            drawn = sample_clip_augment(h, w, rng, np_rng)
            return ClipAugment(flip=drawn.flip, first=None, crop=None, final=FINAL, hsv=drawn.hsv, reverse=False)

    return OneGeometry(data_config("DanceTrack", DATA_ROOT=root, SAMPLE_STEPS=[], SAMPLE_LENGTHS=[clip_len],
                                   SAMPLE_INTERVALS=[3]))


def loader_alone(dataset, args, device):
    from memotr_amd.data import ClipLoader, jpeg
    out = {}
    loader = ClipLoader(dataset, device, seed=42, prefetch=args.prefetch, decode_threads=args.decode_threads)
    for _ in loader.epoch(0):                       # warm-up: tables, masks, pinned ring, code objects
        pass
    torch.cuda.synchronize()
    rates, cpu_thread, cpu_process, stages = [], [], [], []
    for _ in range(args.repeats):
        loader.timings = []
        t0, c0 = time.perf_counter(), time.process_time()
        n = sum(1 for _ in loader.epoch(0))
        torch.cuda.synchronize()
        dt, dc = time.perf_counter() - t0, time.process_time() - c0
        rates.append(n / dt)
        cpu_process.append(dc / n * 1e3)
        cpu_thread.append(sum(t["thread_cpu"] for t in loader.timings) / n * 1e3)
        stages.append({k: sum(t[k] for t in loader.timings) / n * 1e3 for k in ("read", "decode", "augment")})
    loader.timings = None
    # the entropy stage alone, on the streams of the first clip
    dataset.set_epoch(0)
    sample = dataset.sample(0, random.Random(0))
    streams = [np.fromfile(p, dtype=np.uint8) for p in sample.paths]
    infos = [jpeg.parse_jpeg(a) for a in streams]
    host = torch.empty((len(streams), infos[0].coef_count + jpeg.QT_WORDS), dtype=torch.int16, pin_memory=True)
    entropy = []
    for _ in range(12):
        t0 = time.perf_counter()
        jpeg._entropy_batch(streams, infos, host, loader.decode_threads)
        entropy.append((time.perf_counter() - t0) * 1e3)
    out.update(clips=n, clips_per_s=rates, producer_thread_cpu_ms_per_clip=cpu_thread,
               process_cpu_ms_per_clip=cpu_process, producer_wall_ms_per_clip=stages,
               entropy_batch_ms_per_clip=statistics.median(entropy[2:]), entropy_threads=loader.decode_threads)
    return out


def clip_step(dataset, args, device):
    from memotr_amd.configs import dancetrack_config
    from memotr_amd.data import ClipLoader
    from memotr_amd.engine import build_optimizer, clip_forward_backward, optimizer_step
    from memotr_amd.models import build_model
    from memotr_amd.models.criterion import build as build_criterion
    from memotr_amd.utils.utils import set_seed
    os.environ.setdefault("MEMOTR_REQUIRE_GRAPHS", "1")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    cfg = dancetrack_config(DEVICE="cuda", AVAILABLE_GPUS="0")
    set_seed(cfg["SEED"])
    model = build_model(cfg).train()
    criterion = build_criterion(cfg)
    optimizer = build_optimizer(cfg, model)
    loader = ClipLoader(dataset, device, seed=42, prefetch=args.prefetch, decode_threads=args.decode_threads)
    resident = [dict(b) for b in loader.epoch(0)]
    torch.cuda.synchronize()

    def epoch(batches):
        n = 0
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        for batch in batches:
            loss, _ = clip_forward_backward(model, criterion, batch, device, use_dab=cfg["USE_DAB"])
            optimizer_step(model, optimizer, cfg["CLIP_MAX_NORM"])
            n += 1
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        return (time.perf_counter() - t0) / n * 1e3, (time.process_time() - c0) / n * 1e3

    epoch(resident)                                 # warm-up of each side: captures, MIOpen, the loader's tables
    epoch(loader.epoch(0))
    res = {"resident": [], "loader": [], "resident_cpu": [], "loader_cpu": []}
    for _ in range(args.repeats):
        ms, cpu = epoch(resident)
        res["resident"].append(ms), res["resident_cpu"].append(cpu)
        ms, cpu = epoch(loader.epoch(0))
        res["loader"].append(ms), res["loader_cpu"].append(cpu)
    spread = max(res["resident"]) - min(res["resident"])
    med_r, med_l = statistics.median(res["resident"]), statistics.median(res["loader"])
    return {"clips_per_epoch": len(resident), "clip_len": args.clip_len, "frame_size": list(FINAL),
            "resident_ms_per_step": res["resident"], "loader_ms_per_step": res["loader"],
            "resident_process_cpu_ms_per_step": res["resident_cpu"], "loader_process_cpu_ms_per_step": res["loader_cpu"],
            "resident_median": med_r, "loader_median": med_l, "resident_spread": spread,
            "target_met": med_l <= med_r + spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--clip-len", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prefetch", type=int, default=2)
    ap.add_argument("--decode-threads", type=int, default=2)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py measures on a GPU: none found")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    result = {"torch_threads": torch.get_num_threads()}
    with tempfile.TemporaryDirectory(prefix="bench_loader_") as root:
        sizes = write_tree(root, args.frames, device)
        result["stream_bytes_median"] = int(statistics.median(sizes))
        result["frames"] = args.frames
        dataset = make_dataset(root, args.clip_len)
        if args.only in (None, "a"):
            result["loader_alone"] = loader_alone(dataset, args, device)
            print(json.dumps(result["loader_alone"]), flush=True)
        if args.only in (None, "b"):
            result["clip_step"] = clip_step(dataset, args, device)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
