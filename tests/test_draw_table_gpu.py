"""GPU: ``clipops_draw_table_f32`` (memotr_amd/csrc/clip_tracks.h) against ``clip_ops.draw_table_reference`` to the bit
on the cases of tests/draw_table_cases.py, across the 1024-slot chunk, and through the overlay kernel: the padded device
table drawn with ``n = cap`` gives the frame ``draw_table_host`` draws from the compact host table."""
import numpy as np
import pytest
import torch

import draw_table_cases as C

from memotr_amd import render as R
from memotr_amd.functions import clip_ops

pytestmark = pytest.mark.gpu

CASES = C.named_cases()


def on_device(case):
    return tuple(t.cuda() if torch.is_tensor(t) else t for t in case)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_kernel_writes_the_reference_table(clip_lib, name):
    case = CASES[name]
    dev = on_device(case)
    for bgr, font_scale in C.VARIANTS:
        want = clip_ops.draw_table_reference(*case, bgr=bgr, font_scale=font_scale)
        got = clip_ops.draw_table(*dev, bgr=bgr, font_scale=font_scale)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (name, bgr, font_scale)


@pytest.mark.parametrize("cap", [16, 48, 1040])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_streams_and_capacities_across_the_chunk(clip_lib, B, cap):
    case = C.random_case(B, cap, seed=10 * B + cap)
    want = clip_ops.draw_table_reference(*case, font_scale=2)
    if cap > 1024:      # kept slots on both sides of the chunk boundary whose ranks interleave across it
        table, kept = C.statement(*case, font_scale=2)
        for b in range(B):
            boxes, scores, ids = case[0][b], case[1][b], case[2][b]
            keep = (ids >= 0) & (scores.max(-1).values > case[4])
            lo, hi = ids[:1024][keep[:1024]], ids[1024:][keep[1024:]]
            assert len(hi) > 2 and lo.min() < hi.min() < lo.max() and hi.max() > lo.min() and kept[b] > 256
    out = torch.full((B, cap, 16), 12345, dtype=torch.int32, device="cuda")
    got = clip_ops.draw_table(*on_device(case), font_scale=2, out=out)
    again = clip_ops.draw_table(*on_device(case), font_scale=2)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, again)                               # two launches, the same bits


def test_a_larger_id_gets_the_padding_row(clip_lib):
    boxes, scores, ids, ori_wh, st, at = CASES["all_kept"]
    big, free = ids.clone(), ids.clone()
    big[0, 1], free[0, 1] = 2 ** 31, -1
    want = clip_ops.draw_table_reference(boxes, scores, free, ori_wh, st, at)
    got = clip_ops.draw_table(boxes.cuda(), scores.cuda(), big.cuda(), ori_wh.cuda(), st, at)
    assert torch.equal(got.cpu(), want) and want[0, 4].tolist() == [0, 0, -1, -1] + [0] * 12


@pytest.mark.parametrize("kept,cap", [(9, 14), (70, 80)])        # 70 rows cross the overlay's 64-row cull chunk
def test_the_padded_device_table_draws_the_compact_host_table(clip_lib, kept, cap):
    from memotr_amd.build import build_track_draw_lib
    build_track_draw_lib()
    case = C.draw_case(kept, cap)
    W, H = 65, 17
    want_table, n = C.statement(*case)
    assert n == [kept]
    frame = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for options in (dict(thickness=2, font_scale=1, fill_alpha=0), dict(thickness=1, font_scale=1, fill_alpha=128)):
        want = frame.copy()
        R.draw_table_host(want, want_table[0, :kept], **options)
        assert not np.array_equal(want, frame)
        table = clip_ops.draw_table(*on_device(case))
        assert tuple(table.shape) == (1, cap, 16)
        src = torch.from_numpy(frame).cuda()
        out = R.draw_resident_table(src, table[0], torch.empty_like(src), **options)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), options
