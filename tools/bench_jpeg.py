"""JPEG decode on one MI355X (results: profiles/jpeg_decode.md).

    python tools/bench_jpeg.py [--runs 20] [--launches 100] [--frames 200] [--repeats 3] [--host-only]

(a) host entropy stage (memotr_amd.data.jpeg.entropy_decode into a preallocated buffer) next to Pillow's full decode
    of the same bytes, one thread each, 1080p quality 90, sampling 4:2:0 and 4:4:4: median of --runs runs.  A CPU
    number: --host-only takes it on a machine without a GPU.  Needs PIL (the encoder and the yardstick).
(b) HIP-event time of the device stage (two launches) for one 1080p frame per sampling, next to a stock
    device-to-device copy of its output tensor, same process: median of --launches timed launches after warm-up.
    Bytes moved per frame are computed from the geometry.
(c) frames/s of SequenceTracker.track_jpeg() from in-memory JPEG bytes next to track() from pre-decoded pinned frames
    of the same sequence: same model, --repeats alternating repeats of --frames frames.
Prints one JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 1080, 1920


def test_frame(seed):
    """Gradients, hard edges and moderate noise: a synthetic stand-in for a video frame (an order of magnitude, not a
    data-set statistic)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    px = np.stack([x * 255.0 / W, y * 255.0 / H, (x + y) * 255.0 / (W + H)], -1)
    px[(x // 97 + y // 61) % 2 == 0] *= 0.6
    px += rng.normal(0, 12, (H, W, 3))
    return np.clip(px, 0, 255).astype(np.uint8)


def encode(pixels, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "JPEG", quality=90, subsampling=subsampling)
    return buf.getvalue()


def median_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def host_stage(args, streams):
    import PIL
    from PIL import Image, features
    from memotr_amd.data import jpeg as J
    out = {"pillow": PIL.__version__, "libjpeg_turbo": features.version_feature("libjpeg_turbo"),
           "runs": args.runs}
    for name, data in streams.items():
        info = J.parse_jpeg(data)
        buf = torch.empty(info.coef_count + J.QT_WORDS, dtype=torch.int16)
        e = median_ms(lambda: J.entropy_decode(data, pinned=buf), args.runs)
        p = median_ms(lambda: Image.open(io.BytesIO(data)).convert("RGB").load(), args.runs)
        assert np.array_equal(J.decode_jpeg(data, "cpu", fallback=False).numpy(),
                              np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        out[name] = {"stream_bytes": len(data), "entropy_ms": e, "pillow_full_decode_ms": p, "entropy_over_pillow": e / p,
                     "upload_bytes": 2 * (info.coef_count + J.QT_WORDS)}
    return out


def event_times_ms(fn, warmup, n, blocker):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        blocker()                           # ~100 us of device work in front: the events bracket execution, not issue
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in pairs)


def device_stage(args, streams):
    import ctypes
    from memotr_amd import _jpeg_lib as L
    from memotr_amd.data import jpeg as J
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    result = {"launches": args.launches}
    for name, data in streams.items():
        coefs = J.entropy_decode(data)
        info = coefs.info
        c = J._cinfo(info)
        words = info.coef_count + J.QT_WORDS
        dev = coefs.flat.cuda()
        planes = torch.empty(L.lib.jpegops_planes_bytes(ctypes.byref(c)), dtype=torch.uint8, device="cuda")
        out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(out)
        stream = torch.cuda.current_stream().cuda_stream

        def run():
            L.check(L.lib.jpegops_decode_pixels_u8(dev.data_ptr(), words, dev.data_ptr() + info.coef_count * 2, words,
                                                   ctypes.byref(c), planes.data_ptr(), planes.numel(), out.data_ptr(),
                                                   3 * W, 3 * W * H, 1, 0, stream), "jpegops_decode_pixels_u8")

        k = event_times_ms(run, 20, args.launches, big.zero_)
        cp = event_times_ms(lambda: dst.copy_(out), 20, args.launches, big.zero_)
        assert torch.equal(out.cpu(), torch.from_numpy(J.decode_coefficients_host(coefs)))
        # launch 1 reads the coefficients and tables and writes the planes; launch 2 reads the planes, writes the pixels
        moved = 2 * words + planes.numel() + planes.numel() + out.numel()
        km, cm = statistics.median(k), statistics.median(cp)
        result[name] = {"launches_per_frame": 2, "bytes_moved": moved, "stage_us_median": km * 1e3,
                        "stage_us_min": k[0] * 1e3, "stage_us_p90": k[int(0.9 * len(k))] * 1e3,
                        "copy_us_median": cm * 1e3, "copy_bytes": 2 * out.numel(), "stage_over_copy": km / cm,
                        "stage_TBps": moved / km / 1e9}
    return result


def tracking(args, frames_u8, streams):
    from memotr_amd import configs as C
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    tracker = SequenceTracker.from_config(model, cfg)
    tracker.result_score_thresh = 0.0
    raw = [torch.from_numpy(f).pin_memory() for f in frames_u8]
    n = len(raw)

    def run_track(count):
        for _, out in tracker.track(raw[i % n] for i in range(count)):
            pass
        return out

    def run_jpeg(count):
        for _, out in tracker.track_jpeg(streams[i % n] for i in range(count)):
            pass
        return out

    def timed(fn, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(count)
        torch.cuda.synchronize()
        return count / (time.perf_counter() - t0)

    run_track(args.warmup)
    run_jpeg(args.warmup)
    track_fps, jpeg_fps = [], []
    for _ in range(args.repeats):           # alternating: the two see the same machine state
        track_fps.append(timed(run_track, args.frames))
        jpeg_fps.append(timed(run_jpeg, args.frames))
    return {"frames_per_repeat": args.frames, "live_tracks": int(len(tracker.tracks[0])),
            "track_predecoded_fps": track_fps, "track_jpeg_fps": jpeg_fps,
            "track_predecoded_fps_median": statistics.median(track_fps),
            "track_jpeg_fps_median": statistics.median(jpeg_fps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--skip-tracking", action="store_true")
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs: at least 20")
    frames = [test_frame(s) for s in range(4)]
    streams = {"4:2:0": encode(frames[0], 2), "4:4:4": encode(frames[0], 0)}
    if args.host_only:
        print(json.dumps({"host": host_stage(args, streams)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py needs a GPU (--host-only: the CPU part alone)")
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2)
    result = {"device": torch.cuda.get_device_name(0), "host": host_stage(args, streams),
              "device_stage": device_stage(args, streams)}
    if not args.skip_tracking:
        from PIL import Image
        clip = [encode(f, 2) for f in frames]
        decoded = [np.array(Image.open(io.BytesIO(s)).convert("RGB")) for s in clip]
        result["tracking"] = tracking(args, decoded, clip)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
