"""Annotated output on one MI355X: track overlay and JPEG encode (results: profiles/jpeg_encode.md).

    python tools/bench_jpeg_encode.py [--runs 20] [--launches 100] [--frames 100] [--repeats 3] [--host-only]

(a) host Huffman stage (memotr_amd.data.jpeg_write.huffman_encode of ready coefficients) next to Pillow's full encode
    of the same frame, one thread each, 1080p quality 90, sampling 4:2:0 and 4:4:4: median of --runs runs; the bytes
    are asserted equal.  A CPU number: --host-only takes it on a machine without a GPU.  Needs PIL (the yardstick).
(b) HIP-event time for one 1080p frame of the draw launch (20 tracks) and of the two encode launches per sampling,
    next to a stock device-to-device copy of the frame, same process: median of --launches timed launches after
    warm-up.  Bytes moved per frame are computed from the geometry.
(c) frames/s of SequenceTracker.track_annotated() into a sink that drops the bytes next to track() without a writer,
    800 x 1333 frames: same model, --repeats alternating repeats of --frames frames.
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
QUALITY = 90


def test_frame(seed, h=H, w=W):
    """Gradients, hard edges and moderate noise: a synthetic stand-in for a video frame (an order of magnitude, not a
    data-set statistic)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([x * 255.0 / w, y * 255.0 / h, (x + y) * 255.0 / (w + h)], -1)
    px[(x // 97 + y // 61) % 2 == 0] *= 0.6
    px += rng.normal(0, 12, (h, w, 3))
    return np.clip(px, 0, 255).astype(np.uint8)


def test_tracks(n, h=H, w=W, seed=3):
    rng = np.random.default_rng(seed)
    x1, y1 = rng.uniform(0, w * 0.8, n), rng.uniform(0, h * 0.8, n)
    boxes = np.stack([x1, y1, x1 + rng.uniform(40, w * 0.2, n), y1 + rng.uniform(80, h * 0.4, n)], 1).astype(np.float32)
    return np.arange(1, n + 1), boxes


def median_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def host_stage(args, frame):
    import PIL
    from PIL import Image, features
    from memotr_amd.data import jpeg_write as JW
    out = {"pillow": PIL.__version__, "libjpeg_turbo": features.version_feature("libjpeg_turbo"), "runs": args.runs,
           "quality": QUALITY}
    im = Image.fromarray(frame)
    for name, s in (("4:2:0", 2), ("4:4:4", 0)):
        coefs = JW.forward_coefficients_host(frame, QUALITY, name)

        def pillow():
            buf = io.BytesIO()
            im.save(buf, "JPEG", quality=QUALITY, subsampling=s)
            return buf.getvalue()

        assert JW.huffman_encode(coefs) == pillow()
        e = median_ms(lambda: JW.huffman_encode(coefs), args.runs)
        p = median_ms(pillow, args.runs)
        out[name] = {"stream_bytes": len(pillow()), "huffman_ms": e, "pillow_full_encode_ms": p, "huffman_over_pillow": e / p,
                     "download_bytes": 2 * coefs.info.coef_count}
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


def summary(times, moved, copy_median):
    m = statistics.median(times)
    return {"bytes_moved": moved, "us_median": m * 1e3, "us_min": times[0] * 1e3,
            "us_p90": times[int(0.9 * len(times))] * 1e3, "over_copy": m / copy_median, "TBps": moved / m / 1e9}


def device_stage(args, frame):
    import ctypes
    from memotr_amd import _jpeg_enc_lib as E
    from memotr_amd import _track_draw_lib as D
    from memotr_amd import render as R
    from memotr_amd.data import jpeg_write as JW
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    dev = torch.from_numpy(frame).cuda()
    dst = torch.empty_like(dev)
    stream = torch.cuda.current_stream().cuda_stream
    cp = event_times_ms(lambda: dst.copy_(dev), 20, args.launches, big.zero_)
    cm = statistics.median(cp)
    result = {"launches": args.launches, "copy_us_median": cm * 1e3, "copy_bytes": 2 * dev.numel()}

    ids, boxes = test_tracks(20)
    table_np = R.track_table(ids, boxes, W, H, font_scale=2)
    table = torch.from_numpy(table_np).cuda()
    for label, out in (("draw_out_of_place", dst), ("draw_in_place", dev.clone())):
        src = dev if out is dst else out

        def draw():
            D.check(D.lib.trackdraw_draw_u8(src.data_ptr(), 3 * W, out.data_ptr(), 3 * W, W, H, table.data_ptr(),
                                            len(ids), 2, 2, 64, stream), "trackdraw_draw_u8")

        t = event_times_ms(draw, 20, args.launches, big.zero_)
        if out is dst:
            assert torch.equal(dst.cpu(), torch.from_numpy(R.draw_tracks_host(frame, ids, boxes, font_scale=2,
                                                                             fill_alpha=64)))
            moved = table.numel() * 4 + 2 * dev.numel()
        else:
            touched = int((dst != dev).any(-1).sum().item())          # a lower bound of the pixels in touched tiles
            moved = table.numel() * 4 + 6 * touched
        result[label] = dict(summary(t, moved, cm), launches_per_frame=1, tracks=len(ids))

    qt = np.ascontiguousarray(JW.quant_tables(QUALITY).astype(np.uint16).reshape(-1))
    for name in ("4:2:0", "4:4:4"):
        info = JW.frame_info(H, W, name)
        c = JW._cinfo(info)
        n = info.coef_count
        planes = torch.empty(E.lib.jpegenc_planes_bytes(ctypes.byref(c)), dtype=torch.uint8, device="cuda")
        coef = torch.empty(n, dtype=torch.int16, device="cuda")

        def run():
            E.check(E.lib.jpegenc_forward_u8(dev.data_ptr(), 3 * W, 3 * W * H, ctypes.byref(c), qt.ctypes.data,
                                             planes.data_ptr(), planes.numel(), coef.data_ptr(), n, 1, 0, stream),
                    "jpegenc_forward_u8")

        t = event_times_ms(run, 20, args.launches, big.zero_)
        want = JW.forward_coefficients_host(frame, QUALITY, name)
        assert torch.equal(coef.cpu(), want.flat[:n])
        # launch 1 reads the pixels and writes the planes; launch 2 reads the planes and writes the coefficients
        moved = dev.numel() + planes.numel() + planes.numel() + 2 * n
        result[name] = dict(summary(t, moved, cm), launches_per_frame=2)
    return result


def tracking(args):
    from memotr_amd import configs as C
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models import build_model
    from memotr_amd.render import AnnotatedWriter
    from memotr_amd.utils.utils import set_seed
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = C.dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    set_seed(cfg["SEED"])
    model = build_model(dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")).to(dev).eval()
    tracker = SequenceTracker.from_config(model, cfg)
    tracker.result_score_thresh = 0.0
    raw = [torch.from_numpy(test_frame(s, 800, 1333)).pin_memory() for s in range(4)]
    n = len(raw)
    written = [0, 0]

    def sink(idx, data):
        written[0] += 1
        written[1] += len(data)

    def run_track(count):
        for _, out in tracker.track(raw[i % n] for i in range(count)):
            pass
        return out

    def run_annotated(count):
        with AnnotatedWriter(sink, quality=QUALITY) as writer:
            for _, out in tracker.track_annotated((raw[i % n] for i in range(count)), writer):
                pass
        return out

    def timed(fn, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(count)                           # (run_annotated returns after close(): every file has been handed over)
        torch.cuda.synchronize()
        return count / (time.perf_counter() - t0)

    run_track(args.warmup)
    run_annotated(args.warmup)
    track_fps, annotated_fps = [], []
    for _ in range(args.repeats):           # alternating: the two see the same machine state
        track_fps.append(timed(run_track, args.frames))
        annotated_fps.append(timed(run_annotated, args.frames))
    return {"frame": [800, 1333], "frames_per_repeat": args.frames, "live_tracks": int(len(tracker.tracks[0])),
            "files": written[0], "mean_file_bytes": written[1] / max(written[0], 1),
            "track_fps": track_fps, "track_annotated_fps": annotated_fps,
            "track_fps_median": statistics.median(track_fps),
            "track_annotated_fps_median": statistics.median(annotated_fps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--skip-tracking", action="store_true")
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs: at least 20")
    frame = test_frame(0)
    if args.host_only:
        print(json.dumps({"host": host_stage(args, frame)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode.py needs a GPU (--host-only: the CPU part alone)")
    from memotr_amd.utils.host import pin_near_gpu, respect_cpu_quota
    respect_cpu_quota()
    pin_near_gpu(torch.cuda.current_device(), 0, n_cpus=2)
    result = {"device": torch.cuda.get_device_name(0), "host": host_stage(args, frame),
              "device_stage": device_stage(args, frame)}
    if not args.skip_tracking:
        result["tracking"] = tracking(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
