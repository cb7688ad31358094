"""GPU: render.AnnotatedWriter (draw launch, two encode launches, download into rotating pinned buffers, Huffman
stage and sink on a worker thread) writes exactly ``encode_jpeg(draw_tracks_host(...))`` of the host; close() drains,
is idempotent and re-raises the sink's error; SequenceTracker.track_annotated yields what track / track_jpeg yield
and its files decode with the project's own decoder."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_frames_gpu import build_memotr_cuda

from memotr_amd import render as R
from memotr_amd.data import jpeg as J
from memotr_amd.data import jpeg_write as JW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib, build_track_draw_lib
    build_jpeg_enc_lib(), build_jpeg_lib(), build_track_draw_lib()


def synthetic(i):
    """Frame i of five and its 'result': (ids, boxes) that move with i."""
    px = np.random.default_rng(50 + i).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    ids = [3, 10 + i, 12345678]
    boxes = [[5.0 + 3 * i, 12.0, 40.0 + 3 * i, 44.5], [30.0, 20.0 + i, 90.0, 60.0], [-4.0, 30.0, 20.0 + i, 70.0]]
    return px, ids, boxes


@pytest.mark.parametrize("sub,opts", [("4:2:0", dict()), ("4:4:4", dict(fill_alpha=128, font_scale=2, bgr=True))])
def test_five_frames_equal_the_host_and_names_are_in_order(libs, tmp_path, sub, opts):
    with R.AnnotatedWriter(tmp_path, quality=85, subsampling=sub, **opts) as writer:
        for i in range(5):
            px, ids, boxes = synthetic(i)
            writer.add(i, torch.from_numpy(px).cuda(), (ids, boxes))
    assert sorted(os.listdir(tmp_path)) == [f"{i:08d}.jpg" for i in range(5)]
    assert writer.paths == [str(tmp_path / f"{i:08d}.jpg") for i in range(5)]
    for i in range(5):
        px, ids, boxes = synthetic(i)
        drawn = R.draw_tracks_host(torch.from_numpy(px), ids, boxes, **opts)
        want = JW.encode_jpeg(drawn, quality=85, subsampling=sub, bgr=opts.get("bgr", False))
        assert (tmp_path / f"{i:08d}.jpg").read_bytes() == want, i
    writer.close()                                      # a second close() is nothing
    with pytest.raises(RuntimeError, match="closed"):
        writer.add(5, torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"), ([], np.zeros((0, 4))))


def test_a_callable_sink_more_frames_than_buffers_and_a_size_change(libs):
    got = {}
    writer = R.AnnotatedWriter(lambda idx, data: got.__setitem__(idx, data), quality=60)
    frames = []
    for i in range(8):                                  # 8 frames through 3 pinned buffers; the size changes at 5
        h, w = (37, 53) if i < 5 else (16, 300)
        px = np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        frames.append(px)
        writer.add(i, torch.from_numpy(px).cuda(), ([i, 7], [[2.0, 10.0, 30.0, 14.0 + i], [20.0, 3.0, 50.0, 15.0]]))
    writer.close()
    writer.close()
    assert list(got) == list(range(8))                  # handed over in order
    for i, px in enumerate(frames):
        drawn = R.draw_tracks_host(px, [i, 7], [[2.0, 10.0, 30.0, 14.0 + i], [20.0, 3.0, 50.0, 15.0]])
        assert got[i] == JW.encode_jpeg(torch.from_numpy(drawn), quality=60), i


def test_a_sink_that_raises_surfaces_on_close(libs):
    calls = []

    def sink(idx, data):
        calls.append(idx)
        raise OSError("disk full")

    writer = R.AnnotatedWriter(sink)
    for i in range(3):
        px, ids, boxes = synthetic(i)
        writer.add(i, torch.from_numpy(px).cuda(), (ids, boxes))
    with pytest.raises(OSError, match="disk full"):
        writer.close()
    assert calls == [0]                                 # nothing more is handed over after the first error
    writer.close()
    with pytest.raises(TypeError, match="unknown draw options"):
        R.AnnotatedWriter(sink, colour="red")
    with pytest.raises(ValueError, match="quality"):
        R.AnnotatedWriter(sink, quality=0)


def test_track_annotated_equals_track_and_its_files_decode(libs, hip_lib, clip_lib, tmp_path, monkeypatch):
    from memotr_amd.inference import SequenceTracker
    import memotr_amd.modules.ms_deform_attn as mod
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "0")
    cases = load_golden("jpeg_cases")
    streams = [cases[f"jpg_track_{i}"].tobytes() for i in range(4)]
    pixels = [torch.from_numpy(cases[f"rgb_track_{i}"]) for i in range(4)]

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
    assert len(want) == 4 and len(want[-1]) >= 3
    for source, out in ((pixels, tmp_path / "frames"), (streams, tmp_path / "jpeg")):
        with R.AnnotatedWriter(out, quality=90) as writer:
            got = list(tracker().track_annotated(source, writer))
        assert [i for i, _ in got] == [0, 1, 2, 3]
        for (_, a), b in zip(got, want):
            assert a.ids.tolist() == b.ids.tolist()
            assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores)
        for i, (_, result) in enumerate(got):
            data = (out / f"{i:08d}.jpg").read_bytes()
            assert data == JW.encode_jpeg(R.draw_tracks_host(pixels[i], result), quality=90), i
            back = J.decode_jpeg(data, "cuda", fallback=False)
            assert tuple(back.shape) == (64, 96, 3)
            assert torch.equal(back.cpu(), J.decode_jpeg(data, "cpu", fallback=False))
    assert list(tracker().track_annotated([], None)) == []
