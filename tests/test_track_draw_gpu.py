"""GPU: the overlay kernel (memotr_amd/csrc/track_draw.hip) is bit-equal to the host statement
(memotr_amd/render.py draw_tracks_host) on every case of tests/track_draw_cases.py: frames that are ragged against the
64 x 16 tile, boxes inside, across every edge, outside, inverted, one pixel, thin and overlapping in both orders;
tables of 0, 1 and 70 rows; in place and out of place, pitched rows, a side stream."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from track_draw_cases import IDS, OPTIONS, SIZES, frame, many, named_boxes

from memotr_amd import render as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def draw_lib():
    from memotr_amd.build import build_track_draw_lib
    build_track_draw_lib()
    from memotr_amd import _track_draw_lib
    return _track_draw_lib


def both_ways(src: np.ndarray, ids, boxes, **kw):
    """Out of place (the input must stay as it was) and in place, against the host statement."""
    want = torch.from_numpy(R.draw_tracks_host(src, ids, boxes, **kw))
    dev = torch.from_numpy(src).cuda()
    out = R.draw_tracks(dev, ids, boxes, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.data_ptr() != dev.data_ptr()
    assert torch.equal(out.cpu(), want)
    assert torch.equal(dev.cpu(), torch.from_numpy(src))
    same = R.draw_tracks(dev, ids, boxes, out=dev, **kw)
    assert same is dev and torch.equal(dev.cpu(), want)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("options", range(len(OPTIONS)))
def test_kernel_equals_the_host_statement_on_every_named_case(draw_lib, size, options):
    h, w = size
    src = frame(h, w, seed=options)
    for name, boxes in named_boxes(h, w).items():
        both_ways(src, [IDS[(i + len(name)) % 5] for i in range(len(boxes))], boxes, **OPTIONS[options])


@pytest.mark.parametrize("size", SIZES)
def test_table_lengths_0_1_and_70(draw_lib, size):
    h, w = size
    src = frame(h, w, seed=9)
    both_ways(src, [], np.zeros((0, 4), np.float32))
    for tid in IDS:
        both_ways(src, [tid], [(3.0, 11.0, w - 4.0, h - 2.0)], fill_alpha=128)
    ids, boxes = many(h, w)
    assert len(ids) == 70                                # more than one cull chunk of 64 rows
    for kw in OPTIONS:
        both_ways(src, ids, boxes, **kw)
    both_ways(src, ids[::-1].copy(), boxes[::-1].copy(), fill_alpha=128)
    ids, boxes = many(h, w, n=200, seed=6)               # four chunks, the last one partial
    both_ways(src, ids, boxes, fill_alpha=200, font_scale=2)


def test_alpha_values_and_font_scales(draw_lib):
    src = frame(64, 96, seed=3)
    boxes = named_boxes(64, 96)["overlap"]
    for alpha in (0, 128, 255):
        for scale in (1, 2, 3):
            both_ways(src, [10, 12345678, 7], boxes, fill_alpha=alpha, font_scale=scale, thickness=1)


def test_the_committed_scene(draw_lib):
    scene = load_golden("track_draw_scene")
    dev = torch.from_numpy(scene["frame"]).cuda()
    for k in range(3):
        bgr, t, s, a = (int(v) for v in scene[f"options_{k}"])
        got = R.draw_tracks(dev, scene["ids"], scene["boxes"], bgr=bool(bgr), thickness=t, font_scale=s, fill_alpha=a)
        assert torch.equal(got.cpu(), torch.from_numpy(scene[f"expected_{k}"])), k


def test_pitched_rows_and_a_side_stream(draw_lib):
    """A column slice of a wider frame, from a column that puts the quads at every byte alignment; nothing outside
    the slice is written."""
    h, w = 37, 53
    src = frame(h, w, seed=4)
    ids, boxes = many(h, w, n=20)
    want = torch.from_numpy(R.draw_tracks_host(src, ids, boxes, fill_alpha=100))
    for left in (1, 2, 3, 4):
        wide = torch.randint(0, 256, (h, w + 9, 3), dtype=torch.uint8, device="cuda")
        wide[:, left:left + w] = torch.from_numpy(src).cuda()
        keep = wide.clone()
        view = wide[:, left:left + w]
        out = R.draw_tracks(view, ids, boxes, fill_alpha=100)
        assert torch.equal(out.cpu(), want)
        dst = torch.zeros((h, w + 5, 3), dtype=torch.uint8, device="cuda")
        R.draw_tracks(view, ids, boxes, fill_alpha=100, out=dst[:, 2:2 + w])
        assert torch.equal(dst[:, 2:2 + w].cpu(), want) and int(dst[:, :2].sum()) == 0 and int(dst[:, 2 + w:].sum()) == 0
        assert torch.equal(wide, keep)
        R.draw_tracks(view, ids, boxes, fill_alpha=100, out=view)
        assert torch.equal(view.cpu(), want)
        assert torch.equal(wide[:, :left], keep[:, :left]) and torch.equal(wide[:, left + w:], keep[:, left + w:])
    dev = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = R.draw_tracks(dev, ids, boxes, fill_alpha=100)
    side.synchronize()
    assert torch.equal(out.cpu(), want)


def test_a_track_instances_and_bad_arguments(draw_lib):
    from memotr_amd.structures.track_instances import TrackInstances
    t = TrackInstances(hidden_dim=8, num_classes=1)
    t.ids = torch.tensor([3, 12])
    t.boxes = torch.tensor([[5.0, 12.0, 30.0, 30.0], [20.0, 15.0, 50.0, 35.0]])
    src = frame(37, 53)
    dev = torch.from_numpy(src).cuda()
    assert torch.equal(R.draw_tracks(dev, t).cpu(), torch.from_numpy(R.draw_tracks_host(src, t)))
    with pytest.raises(ValueError, match="out must"):
        R.draw_tracks(dev, t, out=torch.empty((37, 52, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="pixel stride 3"):
        R.draw_tracks(torch.from_numpy(frame(37, 106)).cuda()[:, ::2], t)
    with pytest.raises(RuntimeError, match="overlap"):
        R.draw_tracks(dev[:-1], t, out=dev[1:])
