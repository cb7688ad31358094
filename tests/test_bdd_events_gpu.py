"""GPU: the device path of the BDD100K error analysis (memotr_amd/diagnose_bdd100k.py) against its host statement, bit
for bit: the random and the scripted sequences of tests/bdd_events_cases.py and the fixture recorded from TrackEval,
``clipops_bdd_cross_class_f64`` (memotr_amd/csrc/clip_tracks.h) at the edges of a wavefront with sentinels in and guard
words around every output, a launch made for fewer candidates than a frame holds, a pack of sequences of different
lengths on a stream of its own, the annotated frames byte for byte, and the evaluator's ``events()``."""
import os

import numpy as np
import pytest
import torch

import bdd_events_cases as C
import dataset_trees as T
from track_eval_bdd_helpers import golden

from memotr_amd import diagnose as D
from memotr_amd import diagnose_bdd100k as DB
from memotr_amd import evaluation_bdd100k as B

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0x5A5A5A5A
CROSS_KEYS = ("gt_cross_partner", "gt_cross_class", "gt_cross_iou", "tr_cross_partner", "tr_cross_class", "tr_cross_iou")


@pytest.fixture(scope="module")
def libs(clip_lib):
    from memotr_amd.build import (build_jpeg_enc_lib, build_jpeg_lib, build_track_draw_lib, build_track_eval_bdd_lib,
                                  build_track_eval_lib)
    build_track_eval_lib(), build_track_eval_bdd_lib(), build_jpeg_lib(), build_jpeg_enc_lib(), build_track_draw_lib()
    return clip_lib


def guarded(n, dtype=torch.int32):
    """A sentinel-filled buffer with GUARD elements on either side of ``n``; (whole, the part the kernel gets)."""
    fill = SENTINEL if dtype == torch.int32 else float(SENTINEL)
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_untouched(whole, n):
    return bool((whole[:GUARD] == whole[0]).all()) and bool((whole[GUARD + n:] == whole[0]).all()) and \
        float(whole[0]) == float(SENTINEL)


@pytest.mark.parametrize("case", ["random", "scripted", "trackeval"])
def test_events_on_the_device_equal_the_host_statement(libs, case):
    pack = {"random": lambda: C.random_pack()[0], "scripted": C.scripted_pack, "trackeval": lambda: golden()[1]}[case]()
    want = C.random_pack()[1] if case == "random" else DB.bdd_events(pack)
    for source in (pack, pack.to("cuda")):
        C.same_events(DB.bdd_events(source, device="cuda"), want)       # (every integer array; the IoUs to the bit)
    fields = B.evaluate_packed_bdd(pack.to("cuda"), device="cuda")
    for name, ev in want.items():
        for cls, counts in ev.counts().items():
            assert counts == {k: int(fields[name][cls][k]) for k in DB.COUNTS}, (name, cls)
    if case != "trackeval":
        assert sum(int((ev.gt_cross_partner >= 0).sum()) for ev in want.values()) > 0


def cross_inputs(pack, ev):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                             # noqa: E731
    return [up(x) for x in (pack.gt_boxes, pack.tr_boxes, pack.gt_classes, pack.tr_classes, pack.gt_off, pack.tr_off,
                            ev.gt_kind, ev.tr_kind)]


def test_the_cross_class_kernel_at_the_edges_of_a_wavefront(libs):
    pack = C.grid_pack()
    ev = DB.bdd_events(pack)["grid"]
    # what the sequence is there for: 1, 63, 64 and 65 candidates on both sides, not the frame's first rows, the frames
    # between without any row, and every candidate paired with the box over it
    sizes = [tuple(len(x) for x in C.candidates(ev, f)) for f in range(ev.n_frames)]
    assert [sizes[f] for f in C.GRID_FRAMES] == [(n, n) for n in C.GRID_COUNTS]
    assert all(sizes[f] == (0, 0) and ev.gt_off[f] == ev.gt_off[f + 1] for f in (0, 2, 5, 7))
    assert ev.tr_kind[ev.tr_off[6]] == DB.TP and ev.gt_kind[ev.gt_off[6]] == DB.MISS
    assert int((ev.gt_cross_partner >= 0).sum()) == sum(C.GRID_COUNTS) == ev.confusion_matrix[C.CAR, C.TRUCK]
    for f in C.GRID_FRAMES:
        for i, j in C.cross_pairs(ev, f):
            assert ev.gt_ids[i] + 999 == ev.tr_ids[j]                   # car k + 1 under truck 1000 + k
    NG, NT, F = len(ev.gt_ids), len(ev.tr_ids), ev.n_frames
    inputs = cross_inputs(pack, ev)
    for limit in (65, 2048):
        outs = [guarded(NG), guarded(NG), guarded(NG, torch.float64), guarded(NT), guarded(NT),
                guarded(NT, torch.float64), guarded(F)]
        DB.launch_cross_class(*inputs, limit, limit, *[inner for _, inner in outs])
        torch.cuda.synchronize()
        for (whole, inner), key in zip(outs[:6], CROSS_KEYS):
            want = torch.from_numpy(getattr(ev, key))
            assert inner.dtype == want.dtype and torch.equal(inner.cpu(), want), (limit, key)
            assert guards_untouched(whole, inner.numel()), (limit, key)
        assert not bool(outs[6][1].any()) and guards_untouched(outs[6][0], F), limit


def test_a_launch_made_for_fewer_candidates_reports_the_frame(libs, monkeypatch):
    pack = C.grid_pack()
    ev = DB.bdd_events(pack)["grid"]
    NG, NT, F = len(ev.gt_ids), len(ev.tr_ids), ev.n_frames
    outs = [guarded(NG), guarded(NG), guarded(NG, torch.float64), guarded(NT), guarded(NT), guarded(NT, torch.float64),
            guarded(F)]
    DB.launch_cross_class(*cross_inputs(pack, ev), 64, 64, *[inner for _, inner in outs])
    torch.cuda.synchronize()
    assert outs[6][1].tolist() == [0, 0, 0, 0, 0, 0, -2, 0]             # the frame of 65; the frame of 64 fits
    g, t = slice(ev.gt_off[6], ev.gt_off[7]), slice(ev.tr_off[6], ev.tr_off[7])
    for (whole, inner), key in zip(outs[:6], CROSS_KEYS):
        want = getattr(ev, key).copy()
        want[g if key.startswith("gt") else t] = 0 if key.endswith("iou") else -1       # nothing is left half written
        assert torch.equal(inner.cpu(), torch.from_numpy(want)), key
        assert guards_untouched(whole, inner.numel()), key
    monkeypatch.setattr(DB, "CROSS_MAX_DIM", 64)
    with pytest.raises(ValueError, match=r"sequence grid, frame 6: .* \(analyse it on the host\)"):
        DB.bdd_events(pack, device="cuda")


def test_sequences_of_different_lengths_on_a_stream_of_their_own(libs):
    pack, want = C.random_pack()
    two = B.pack_bdd({name: {k: v for k, v in zip(
        ("gt_ids", "gt_boxes", "gt_classes", "tracker_ids", "tracker_boxes", "tracker_classes", "ignore_regions"),
        lists(pack.select(pack.names.index(name))))} for name in ("walk29", "walk11")})
    assert np.diff(two.seq_off).tolist() == [17, 31]                    # 8 * 17 = 136 split frames before the second
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        device_pack = two.to("cuda")
        got = DB.bdd_events(device_pack, device="cuda")
    stream.synchronize()
    C.same_events(got, {name: want[name] for name in ("walk29", "walk11")})
    assert torch.cuda.current_stream() != stream


def lists(p):
    """The per-frame lists of a one-sequence host pack."""
    cut = lambda a, off: [a[off[f]:off[f + 1]] for f in range(len(off) - 1)]                    # noqa: E731
    return (cut(p.gt_ids, p.gt_off), cut(p.gt_boxes, p.gt_off), cut(p.gt_classes, p.gt_off), cut(p.tr_ids, p.tr_off),
            cut(p.tr_boxes, p.tr_off), cut(p.tr_classes, p.tr_off), cut(p.ig_boxes, p.ig_off))


# ---------------------------------------------------------------------------------------------------- end to end
WIDTH, HEIGHT = 96, 64


def test_error_frames_on_the_device_are_the_host_paths_bytes(libs, tmp_path):
    from memotr_amd.data import encode_jpeg
    frames = [
        {"gt": [(1, "car", [10.0, 20.0, 40.0, 48.0]), (2, "pedestrian", [55.0, 12.0, 79.0, 52.0])],
         "tr": [(11, "truck", [10.0, 20.0, 40.0, 46.0]), (12, "pedestrian", [55.0, 12.0, 79.0, 52.0])]},
        {"gt": [(1, "car", [12.0, 20.0, 42.0, 48.0]), (2, "pedestrian", [55.0, 12.0, 79.0, 52.0])],
         "tr": [(11, "car", [12.0, 20.0, 42.0, 46.0]), (13, "pedestrian", [55.0, 12.0, 79.0, 52.0]),
                (14, "rider", [70.0, 2.0, 90.0, 16.0])], "regions": [[68.0, 0.0, 92.0, 18.0]]},
    ]
    pack = B.pack_bdd({"clip": C.sequence(frames)})
    paths = []
    for t in range(2):
        paths.append(str(tmp_path / f"{t:08d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(encode_jpeg(torch.from_numpy(T.frame_pixels(t + 1, h=HEIGHT, w=WIDTH)), quality=90,
                                subsampling="4:2:0"))
    ev = DB.bdd_events(pack, device="cuda")["clip"]
    C.same_events({"clip": ev}, DB.bdd_events(pack))
    assert ev.confusions() == [("car", "truck", 1)] and ev.ignored() == [(1, 14, "rider")]
    assert ev.switches() == [(1, 2, 12, 13)]
    events = ev.as_sequence_events()
    assert events.frame_errors().tolist() == [[1, 1, 0], [0, 0, 1]]
    on_host = D.write_error_frames(events, paths, str(tmp_path / "host"), quality=85, font_scale=1)
    on_device = D.write_error_frames(events, paths, str(tmp_path / "device"), quality=85, font_scale=1, device="cuda")
    assert [os.path.basename(p) for p in on_device] == [os.path.basename(p) for p in on_host] == [
        "00000001.jpg", "00000002.jpg"]
    for a, b in zip(on_device, on_host):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read()
    table = D.error_table_device(events, WIDTH, HEIGHT, "cuda")
    assert torch.equal(table.cpu(), torch.from_numpy(D.error_table_host(events, WIDTH, HEIGHT)))


def test_the_evaluator_hands_out_device_events(libs):
    ev = B.BDD100KEvaluator(device="cuda")
    ev.add_ground_truth("v", 0, [1, 2], [C.GT_BOX, [500.0, 500.0, 560.0, 560.0]], ["car", "other person"])
    ev.add_tracker_rows("v", 0, [7, 8], [C.overlapping(0.9), [505.0, 505.0, 555.0, 555.0]], ["truck", "pedestrian"])
    got = ev.events()
    ev.device = None
    C.same_events(got, ev.events())
    assert got["v"].confusions() == [("car", "truck", 1)] and got["v"].ignored() == [(0, 8, "pedestrian")]
