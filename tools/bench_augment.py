"""Training-clip augmentation of a 5-frame 1080p clip on one MI355X (results: profiles/clip_augment.md).

    python tools/bench_augment.py [--launches 50] [--cpu-repeats 3] [--threads 2]
    python tools/bench_augment.py --static [--launches 50]         (results: profiles/static_clip.md)

GPU (each step is one child process, started once under its own time limit; the first that fails ends the run):
  plain  HIP-event time of ``augment_clip`` for the plain branch (flip, 1080x1920 -> 800x1422, HSV), one launch,
         next to a stock device copy of its output tensor (`dst.copy_(out)`);
  crop   the same for the crop branch (first resize 1000x1777 computed on an 811x1203 window, -> 800x1186, HSV), two
         launches, next to a device copy of ITS output.
Host (this process, ``--threads`` torch threads; a rank has 2 CPUs):
  the host statement of the same two plans, and where PIL imports the reference's chain on PIL images (transpose,
  resize, crop, resize; one thread, without its cv2 HSV step, which is not available).
--static (one child process, nothing else runs): a 5-frame clip made from ONE 1080p image (data/static_clip.py),
  chain  HIP-event time of ``shift_chain`` with dx = -37, dy = 23: one launch for the whole clip;
  copy   a stock device copy of its 31 MB output, the floor;
  steps  for dx = +37 (no column move: the only sign the resize kernel can express) the same frames made by T - 1
         dependent ``augops_resample_u8`` launches, each reading the frame before it, with and without the copy that
         puts the image into frame 0; checked equal to the chain's frames before anything is timed.
Prints one JSON line.  No time here is a pass / fail condition."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

T, H, W = 5, 1080, 1920


def plans():
    from memotr_amd.data.augment import ClipAugment
    return {"plain": ClipAugment(flip=True, first=None, crop=None, final=(800, 1422), hsv=(-3, 17, -21)),
            "crop": ClipAugment(flip=True, first=(1000, 1777), crop=(101, 333, 811, 1203), final=(800, 1186),
                                hsv=(-3, 17, -21))}


def clip():
    frames = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (T, H, W, 3), dtype=np.uint8))
    empty = {"boxes": torch.zeros((0, 4)), "ids": torch.zeros((0,), dtype=torch.long),
             "labels": torch.zeros((0,), dtype=torch.long), "areas": torch.zeros((0,))}
    return frames, [dict(empty) for _ in range(T)]


def event_times_ms(fn, warmup, n, blocker):
    """Sorted event times of ``fn``'s device work; ``blocker()`` queues device work in front of every timed call, so the
    host is ahead of the queue and the two events bracket execution, not the time the host needs to issue it."""
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


def gpu_step(name, launches):
    from memotr_amd.data.augment import augment_clip
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a GPU")
    plan = plans()[name]
    frames, infos = clip()
    src = frames.cuda()
    out = augment_clip(src, infos, plan)[0].tensors
    dst = torch.empty_like(out)
    big = torch.empty(128 << 20, dtype=torch.float32, device="cuda")        # 512 MiB: also leaves both cold in cache

    k = event_times_ms(lambda: augment_clip(src, infos, plan, out=out), 10, launches, big.zero_)
    c = event_times_ms(lambda: dst.copy_(out), 10, launches, big.zero_)
    read, written = src.numel(), out.numel() * 4
    if plan.crop is not None:
        mid = T * plan.crop[2] * plan.crop[3] * 3
        read, written = read + mid, written + mid
    km, cm = statistics.median(k), statistics.median(c)
    return {"plan": name, "out": list(out.shape), "launches": launches, "device": torch.cuda.get_device_name(0),
            "augment_us_median": km * 1e3, "augment_us_min": k[0] * 1e3, "augment_us_p90": k[int(0.9 * len(k))] * 1e3,
            "copy_us_median": cm * 1e3, "copy_us_min": c[0] * 1e3, "copy_us_p90": c[int(0.9 * len(c))] * 1e3,
            "augment_over_copy": km / cm, "augment_bytes_upper": read + written, "copy_bytes": 2 * written,
            "clips_per_s": 1e3 / km, "frames_per_s": T * 1e3 / km}


def static_step(launches):
    from memotr_amd import _augment_lib, _static_clip_lib
    from memotr_amd.data import augment as A
    from memotr_amd.data import static_clip as S
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a GPU")
    dx, dy = -37, 23
    img = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    out = torch.empty((T, H, W, 3), dtype=torch.uint8, device="cuda")
    dst, steps = torch.empty_like(out), torch.empty_like(out)
    big = torch.empty(128 << 20, dtype=torch.float32, device="cuda")        # 512 MiB: also leaves everything cold in cache
    dev = torch.device("cuda", torch.cuda.current_device())
    tx, ty = A._device_tables(W, W, dev), A._device_tables(H - abs(dy), H, dev)

    def resample_steps(first=True):
        stream = torch.cuda.current_stream().cuda_stream
        if first:
            steps[0].copy_(img)
        for k in range(1, T):
            A._launch(_augment_lib, steps[k - 1:k], 1, H, W, False, False, tx, ty, H, W, out_u8=steps[k:k + 1],
                      stream=stream)

    resample_steps()
    if not torch.equal(steps, S.shift_chain(img, T, -dx, dy)):
        raise SystemExit("the T - 1 resample launches and the chain disagree")
    res = {"clip": f"{T}x{H}x{W}x3 u8 from one image", "dx": dx, "dy": dy, "launches": launches,
           "device": torch.cuda.get_device_name(0), "out_bytes": out.numel()}
    res["strip"], res["lds_bytes"] = _static_clip_lib.launch_plan(H, W)
    timed = {"chain": lambda: S.shift_chain(img, T, dx, dy, out=out),
             "chain_dx_pos": lambda: S.shift_chain(img, T, -dx, dy, out=out),
             "copy": lambda: dst.copy_(out),
             "steps": resample_steps,
             "steps_without_frame0": lambda: resample_steps(False)}
    for name, fn in timed.items():
        t = event_times_ms(fn, 10, launches, big.zero_)
        res[name + "_us_median"], res[name + "_us_min"] = statistics.median(t) * 1e3, t[0] * 1e3
        res[name + "_us_p90"] = t[int(0.9 * len(t))] * 1e3
    res["chain_over_copy"] = res["chain_us_median"] / res["copy_us_median"]
    res["steps_over_chain"] = res["steps_us_median"] / res["chain_dx_pos_us_median"]
    return res


def host_steps(repeats, threads):
    from memotr_amd.data.augment import augment_clip
    frames, infos = clip()
    res = {"threads": threads}
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    for name, plan in plans().items():
        t = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            augment_clip(frames, infos, plan)
            t.append(time.perf_counter() - t0)
        res[f"host_statement_{name}_ms"] = statistics.median(t[1:]) * 1e3
    torch.set_num_threads(before)
    try:
        from PIL import Image
    except ImportError:
        res["pil"] = "not importable"
        return res
    imgs = [Image.fromarray(f.numpy()) for f in frames]
    for name, plan in plans().items():
        t = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            for img in imgs:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
                if plan.crop is not None:
                    i, j, ch, cw = plan.crop
                    img = img.resize(plan.first[::-1], Image.BILINEAR).crop((j, i, j + cw, i + ch))
                np.asarray(img.resize(plan.final[::-1], Image.BILINEAR))
            t.append(time.perf_counter() - t0)
        res[f"pil_resize_only_{name}_ms"] = statistics.median(t[1:]) * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--static", action="store_true", help="the clip made from one still image, nothing else")
    ap.add_argument("--gpu-step", choices=["plain", "crop", "static"],
                    help="(internal) run one GPU step in this process")
    args = ap.parse_args()
    if args.gpu_step:
        step = static_step(args.launches) if args.gpu_step == "static" else gpu_step(args.gpu_step, args.launches)
        print(json.dumps(step))
        return
    if args.static:
        cmd = [sys.executable, os.path.abspath(__file__), "--gpu-step", "static", "--launches", str(args.launches)]
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.step_timeout)
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            raise SystemExit(f"GPU step static failed ({done.returncode})")
        print(done.stdout.strip().splitlines()[-1])
        return
    result = {"clip": f"{T}x{H}x{W}x3 u8"}
    for name in ("plain", "crop"):
        cmd = [sys.executable, os.path.abspath(__file__), "--gpu-step", name, "--launches", str(args.launches)]
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.step_timeout)
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            raise SystemExit(f"GPU step {name} failed ({done.returncode}); nothing more is started")
        result[name] = json.loads(done.stdout.strip().splitlines()[-1])
    result["host"] = host_steps(args.cpu_repeats, args.threads)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
