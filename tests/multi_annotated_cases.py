"""Shared by tests/test_multi_annotated_cpu.py and tests/test_multi_annotated_gpu.py: annotated output without a host
result (``track_many_annotated*``, ``track_annotated_logged``, ``submit(annotate_dir=...)``) against the host statements.

The sources: three sequences of 2, 4 and 3 frames on two streams -- the first ends and its stream is reset onto the
third, then the second ends and the bank shrinks.  The second is made of JPEG byte streams; the third has another source
size (128 x 192) than the others (64 x 96) and the same target size, so two steps hold frames of two sizes.
"""
import os

import numpy as np
import pytest
import torch

import dataset_trees as T
import multi_track_cases as M

from memotr_amd import render as R
from memotr_amd import submit as S
from memotr_amd.data import encode_jpeg
from memotr_amd.data.jpeg import decode_jpeg
from memotr_amd.inference import SequenceTracker
from memotr_amd.inference_multi import MultiSequenceTracker
from memotr_amd.results import BankResultLog, ResultLog

DRAW = dict(thickness=1, font_scale=1, fill_alpha=96)
QUALITY = 80


def sources():
    """``(sources, pixels)``: what the tracker is given, and every frame as the (H, W, 3) uint8 CPU tensor it shows."""
    a, b, c = M.sequences()
    b_bytes = [bytes(encode_jpeg(f, quality=90, subsampling="4:2:0")) for f in b]
    c = [f.repeat_interleave(2, 0).repeat_interleave(2, 1).contiguous() for f in c]
    return [a, b_bytes, c], [a, [decode_jpeg(x, "cpu") for x in b_bytes], c]


def tracker_for(model, n_streams=2, cap=32):
    return MultiSequenceTracker(model, n_streams=n_streams, cap=cap, **M.OPTIONS)


class Files:
    """A sink that keeps the files: ``files[(sequence, frame)] = bytes``, none written twice."""

    def __init__(self):
        self.files = {}

    def __call__(self, seq, idx, data):
        assert (seq, idx) not in self.files
        self.files[(seq, idx)] = bytes(data)


def expected(frame, ids, boxes, subsampling, bgr=False):
    drawn = R.draw_tracks_host(frame, ids, boxes, bgr=bgr, **DRAW)
    return bytes(encode_jpeg(drawn, QUALITY, subsampling, bgr))


def assert_files_of_rows(files, pixels, rows_of, subsampling):
    """One file per (sequence, frame), each the host statement's bytes for ``rows_of(seq, frame) -> (ids, boxes)``."""
    assert sorted(files) == [(s, f) for s, frames in enumerate(pixels) for f in range(len(frames))]
    drawn = 0
    for (s, f), data in files.items():
        ids, boxes = rows_of(s, f)
        drawn += len(ids)
        assert data == expected(pixels[s][f], ids, boxes, subsampling), (s, f)
    assert drawn > 0


def log_rows(log):
    rows = log.read()

    def rows_of(s, f):
        r = rows.get(s)
        if r is None:
            return np.zeros((0,), np.int64), np.zeros((0, 4), np.float32)
        pick = r.frames == f
        return r.ids[pick], r.boxes_xyxy[pick]
    return rows_of


def check_logged(model, device, subsampling):
    srcs, pixels = sources()
    sink, log = Files(), BankResultLog(device, capacity=8)
    tracker = tracker_for(model)
    with R.MultiAnnotatedWriter(sink, quality=QUALITY, subsampling=subsampling, **DRAW) as writer:
        assert tracker.track_many_annotated_logged(srcs, writer, log) == [2, 4, 3]
    assert tracker.bank.n_streams == 1
    assert_files_of_rows(sink.files, pixels, log_rows(log), subsampling)
    # ... and the rows are those of the run without a writer
    plain = BankResultLog(device)
    tracker_for(model).track_many_logged(srcs, plain)
    for s, want in plain.read().items():
        for x, y in zip(want, log.read()[s]):
            assert np.array_equal(x, y)


def check_generator(model, device):
    srcs, pixels = sources()
    sink, results = Files(), {}
    with R.MultiAnnotatedWriter(sink, quality=QUALITY, subsampling="4:2:0", threads=2, **DRAW) as writer:
        for s, f, r in tracker_for(model).track_many_annotated(srcs, writer):
            results[(s, f)] = r
    assert_files_of_rows(sink.files, pixels, lambda s, f: (results[(s, f)].ids, results[(s, f)].boxes), "4:2:0")


def check_single(model, device, tmp_path):
    """``track_annotated_logged`` writes ``track_annotated``'s files and ``track_logged``'s rows, for decoded frames and
    for JPEG streams; a directory sink names them by sequence."""
    srcs, pixels = sources()
    for src in (srcs[2], srcs[1]):
        want = {}
        with R.AnnotatedWriter(lambda idx, data: want.__setitem__(idx, bytes(data)), quality=QUALITY, **DRAW) as w:
            for _ in SequenceTracker(model, **M.OPTIONS).track_annotated(src, w):
                pass
        want_log = ResultLog(device)
        SequenceTracker(model, **M.OPTIONS).track_logged(src, want_log)
        got, log = Files(), ResultLog(device)
        with R.MultiAnnotatedWriter(got, quality=QUALITY, **DRAW) as w:
            assert SequenceTracker(model, **M.OPTIONS).track_annotated_logged(src, w, log, sequence=5) == len(src)
        assert got.files == {(5, idx): data for idx, data in want.items()} and len(want) == len(src)
        assert len(want_log) > 0
        for x, y in zip(want_log.read(), log.read()):
            assert np.array_equal(x, y)
    # a plain sink(frame_idx, data) gets a writer of default options, closed when the loop returns
    plain = {}
    n = SequenceTracker(model, **M.OPTIONS).track_annotated_logged(srcs[0], lambda i, d: plain.__setitem__(i, d),
                                                                   ResultLog(device))
    assert n == 2 and sorted(plain) == [0, 1] and all(d[:2] == b"\xff\xd8" for d in plain.values())
    # the directory sink
    out = tmp_path / "frames"
    with R.MultiAnnotatedWriter(str(out), names=["first", "second"], quality=QUALITY, **DRAW) as w:
        SequenceTracker(model, **M.OPTIONS).track_annotated_logged(srcs[2], w, ResultLog(device), sequence=1)
    assert sorted(os.listdir(out)) == ["second"]
    assert sorted(os.listdir(out / "second")) == [f"{i:08d}.jpg" for i in range(3)]
    with open(out / "second" / "00000002.jpg", "rb") as f:
        assert f.read() == got_last(model, device, srcs[2])


def got_last(model, device, src):
    files = Files()
    with R.MultiAnnotatedWriter(files, quality=QUALITY, **DRAW) as w:
        SequenceTracker(model, **M.OPTIONS).track_annotated_logged(src, w, ResultLog(device))
    return files.files[(0, len(src) - 1)]


def check_submit(model, tmp_path, thresholds, options):
    """``submit(annotate_dir=...)``: one file per frame and sequence for one stream and for two, and the result files
    of a run without it."""
    root = T.write_trees(str(tmp_path / "data"), only=("DanceTrack",))
    train_config = dict(DATASET="DanceTrack", USE_DAB=True)

    def run(name, **kwargs):
        config = dict(thresholds, SUBMIT_DIR=str(tmp_path / name), SUBMIT_MODEL=None, SUBMIT_DATA_SPLIT="train",
                      DATA_ROOT=root)
        files = S.submit(config, model=model, train_config=train_config, tracker_options=options, **kwargs)
        texts = []
        for path in files:
            with open(path) as f:
                texts.append(f.read())
        return texts

    for streams in (1, 2):
        plain = run(f"plain{streams}", streams=streams)
        out = tmp_path / f"frames{streams}"
        annotated = run(f"annotated{streams}", streams=streams, annotate_dir=str(out),
                        annotate_options=dict(quality=QUALITY, subsampling="4:4:4", **DRAW))
        assert annotated == plain and sum(len(t) for t in plain) > 0
        assert sorted(os.listdir(out)) == sorted(T.DANCE_SEQS)
        for seq, n in T.DANCE_SEQS.items():
            assert sorted(os.listdir(out / seq)) == [f"{i:08d}.jpg" for i in range(n)]
            with open(out / seq / f"{n - 1:08d}.jpg", "rb") as f:
                px = decode_jpeg(f.read(), "cpu")
            frames = S.sequence_frames("DanceTrack", os.path.join(root, "DanceTrack", "train", seq))
            assert tuple(px.shape) == tuple(decode_jpeg(frames[-1], "cpu").shape)
    with pytest.raises(TypeError, match="annotate options"):
        run("bad", annotate_dir=str(tmp_path / "bad"), annotate_options=dict(colour=1))
    with pytest.raises(ValueError, match="annotate_dir"):
        run("bad", annotate_options=dict(quality=90))


def check_writer_errors():
    with R.MultiAnnotatedWriter(Files()) as w:
        with pytest.raises(TypeError, match="add_step"):
            w.add(0, None, None)
        with pytest.raises(ValueError, match="a step is"):
            w.add_step([(0, 0)], [torch.zeros((8, 8, 3), dtype=torch.uint8)], torch.zeros((2, 4, 16), dtype=torch.int32))
    w.close()                                                   # idempotent
    with pytest.raises(RuntimeError, match="closed"):
        w.add_step([], [], torch.zeros((0, 4, 16), dtype=torch.int32))
    with pytest.raises(TypeError, match="unknown draw options"):
        R.MultiAnnotatedWriter(Files(), colour=3)

    def broken(seq, idx, data):
        raise OSError("disk full")
    w = R.MultiAnnotatedWriter(broken)
    table = torch.zeros((1, 2, 16), dtype=torch.int32)
    table[:, :, 2:4] = -1
    w.add_step([(0, 0)], [torch.zeros((8, 8, 3), dtype=torch.uint8)], table)
    with pytest.raises(OSError, match="disk full"):
        w.close()
