"""GPU: the JPEG device stage (memotr_amd/csrc/jpeg_ops.hip: IDCT launch, colour launch) is bit-equal to the numpy
statement of the definition (memotr_amd/data/jpeg.py) and to Pillow's committed pixels on every fixture case and
channel order; clips go through one batched call; nothing outside the pixels is written; SequenceTracker.track_jpeg
equals track() on the Pillow pixels."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_frames_gpu import build_memotr_cuda

from memotr_amd.data import jpeg as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jpeg_lib():
    from memotr_amd.build import build_jpeg_lib
    build_jpeg_lib()
    from memotr_amd import _jpeg_lib
    return _jpeg_lib


@pytest.fixture(scope="module")
def cases():
    return load_golden("jpeg_cases")


@pytest.fixture(scope="module")
def host(jpeg_lib, cases):
    """The host statement's pixels per case, computed once."""
    return {str(n): J.decode_coefficients_host(J.entropy_decode(cases["jpg_" + str(n)])) for n in cases["names"]}


def test_kernels_equal_the_host_statement_and_pillow_on_every_case(jpeg_lib, cases, host):
    for n, want in host.items():
        data = cases["jpg_" + n].tobytes()
        rgb = J.decode_jpeg(data, "cuda", fallback=False)
        bgr = J.decode_jpeg(data, "cuda", bgr=True, fallback=False)
        assert rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == want.shape, n
        assert torch.equal(rgb.cpu(), torch.from_numpy(want)), n
        assert torch.equal(rgb.cpu(), torch.from_numpy(cases["rgb_" + n])), n
        assert torch.equal(bgr.cpu(), torch.from_numpy(want).flip(-1)), n


@pytest.mark.parametrize("mode", ["s0", "s1", "s2", "sL"])
def test_sizes_that_span_several_workgroup_tiles(jpeg_lib, cases, host, mode):
    n = f"tiles_{mode}"
    info = J.parse_jpeg(cases["jpg_" + n])
    assert info.sampling == {"s0": "4:4:4", "s1": "4:2:2", "s2": "4:2:0", "sL": "gray"}[mode]
    for size, tile in ((info.width, jpeg_lib.TILE_X), (info.height, jpeg_lib.TILE_Y)):
        assert size > 3 * tile and size % tile and size % 16
    assert sum(info.blocks_w[c] * info.blocks_h[c] for c in range(info.ncomp)) > 3 * 32       # IDCT workgroups
    got = J.decode_jpeg(cases["jpg_" + n], "cuda", fallback=False).cpu()
    assert torch.equal(got, torch.from_numpy(cases["rgb_" + n])) and torch.equal(got, torch.from_numpy(host[n]))


def test_clips_equal_the_frames_one_by_one(jpeg_lib, cases, host):
    streams = [cases[f"jpg_clip_{i}"].tobytes() for i in range(3)]
    assert J.parse_jpeg(streams[0]).sampling == "4:2:0" and J.parse_jpeg(streams[0]).geometry[:2] == (33, 31)
    clip = J.decode_jpegs(streams, "cuda", threads=2)
    assert torch.is_tensor(clip) and tuple(clip.shape) == (3, 31, 33, 3) and clip.is_cuda
    for i in range(3):
        assert torch.equal(clip[i], J.decode_jpeg(streams[i], "cuda"))
        assert torch.equal(clip[i].cpu(), torch.from_numpy(host[f"clip_{i}"]))
    assert torch.equal(J.decode_jpegs(streams, "cuda", bgr=True).cpu(), clip.cpu().flip(-1))
    mixed = J.decode_jpegs([streams[0], cases["jpg_track_0"], cases["jpg_tiles_sL"]], "cuda")
    assert isinstance(mixed, list) and len(mixed) == 3
    for got, n in zip(mixed, ("clip_0", "track_0", "tiles_sL")):
        assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(host[n]))


@pytest.mark.parametrize("n,offset", [("tiles_s2", 0), ("31x33", 1), ("5x7", 2), ("8x300", 3), ("1x1", 1)])
def test_nothing_outside_the_pixels_is_written(jpeg_lib, cases, host, n, offset):
    """Rows pitched by 7 spare bytes and starting on any byte: the spare bytes, and a margin in front of and behind
    the frame, keep their sentinel."""
    if n not in host:
        n = next(k for k in host if k.startswith(n + "_s2") or k.startswith(n + "_s1"))
    want = torch.from_numpy(host[n])
    H, W, _ = want.shape
    pitch, margin = 3 * W + 7, 64 + offset
    buf = torch.full((margin + H * pitch + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf.as_strided((H, W, 3), (pitch, 3, 1), margin)       # (explicit strides: a view keeps none for a size-1 dim)
    assert out.stride(0) == pitch and out.data_ptr() == buf.data_ptr() + margin
    got = J.decode_jpeg(cases["jpg_" + n], "cuda", fallback=False, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), want)
    whole = buf.cpu()
    assert (whole[:margin] == 0xA5).all() and (whole[margin + H * pitch:] == 0xA5).all()
    assert (whole[margin:margin + H * pitch].view(H, pitch)[:, 3 * W:] == 0xA5).all()


def test_decode_is_ordered_with_the_current_stream(jpeg_lib, cases, host):
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = J.decode_jpeg(cases["jpg_tiles_s2"], "cuda")
        back = torch.empty(got.shape, dtype=torch.uint8, pin_memory=True)
        back.copy_(got, non_blocking=True)
        done = stream.record_event()
    done.synchronize()
    got.record_stream(stream)
    assert torch.equal(back, torch.from_numpy(host["tiles_s2"]))


def test_track_jpeg_equals_track_on_the_pillow_pixels(jpeg_lib, hip_lib, clip_lib, cases, monkeypatch):
    from memotr_amd.inference import SequenceTracker
    import memotr_amd.modules.ms_deform_attn as mod
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "0")
    streams = [cases[f"jpg_track_{i}"].tobytes() for i in range(4)]
    pixels = [torch.from_numpy(cases[f"rgb_track_{i}"]) for i in range(4)]
    assert tuple(pixels[0].shape) == (64, 96, 3)

    def tracker():
        torch.manual_seed(4)
        model = build_memotr_cuda().eval()
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, mod.MSDeformAttn):
                    m.sampling_offsets.weight.normal_(0, 0.02)
                    m.attention_weights.weight.normal_(0, 0.05)
        return SequenceTracker(model, det_score_thresh=0.0, track_score_thresh=0.0, result_score_thresh=0.0,
                               miss_tolerance=5, use_dab=True, area_thresh=0, raw_size=(128, 192))

    want = [r for _, r in tracker().track(pixels)]
    got = list(tracker().track_jpeg(streams))
    assert [i for i, _ in got] == [0, 1, 2, 3] and len(want) == 4 and len(want[-1]) >= 3
    for (_, a), b in zip(got, want):
        assert a.ids.tolist() == b.ids.tolist()
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores)
