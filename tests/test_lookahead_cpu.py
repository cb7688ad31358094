"""CPU: the frame loop and the source-kind test the trackers share (memotr_amd/lookahead.py)."""
import pathlib

import numpy as np
import pytest
import torch

from memotr_amd.lookahead import frame_pairs, is_stream_like


@pytest.mark.parametrize("n", [0, 1, 3])
def test_frame_pairs_yields_every_item_with_the_one_after_it(n):
    items = [object() for _ in range(n)]
    want = [(i, items[i], items[i + 1] if i + 1 < n else None) for i in range(n)]
    assert list(frame_pairs(iter(items))) == want


@pytest.mark.parametrize("n", [0, 1, 3])
def test_frame_pairs_prepares_each_item_once_the_next_one_before_the_current_is_yielded(n):
    log = []

    def prepare(item, ahead):
        log.append(("prepare", item, ahead))
        return item * 10

    for idx, cur, nxt in frame_pairs(range(1, n + 1), prepare):
        log.append(("step", idx, cur, nxt))
    want = [("prepare", 1, False)] if n else []
    for i in range(n):
        if i + 1 < n:
            want.append(("prepare", i + 2, True))
        want.append(("step", i, (i + 1) * 10, (i + 2) * 10 if i + 1 < n else None))
    assert log == want


def test_frame_pairs_reads_no_further_than_one_item_ahead():
    read = []

    def source():
        for i in range(3):
            read.append(i)
            yield i

    pairs = frame_pairs(source())
    assert next(pairs) == (0, 0, 1) and read == [0, 1]
    assert next(pairs) == (1, 1, 2) and read == [0, 1, 2]


def test_jpeg_streams_are_told_from_decoded_frames():
    for stream in ("a/000001.jpg", b"\xff\xd8", bytearray(b"\xff\xd8"), memoryview(b"\xff\xd8"),
                   pathlib.Path("a/000001.jpg"), np.zeros(16, np.uint8), torch.zeros(16, dtype=torch.uint8)):
        assert is_stream_like(stream), type(stream)
    for frame in (np.zeros((4, 6, 3), np.uint8), torch.zeros((4, 6, 3), dtype=torch.uint8)):
        assert not is_stream_like(frame), type(frame)
