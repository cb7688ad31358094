"""CPU: ``clip_ops.draw_table_reference`` -- the statement ``clipops_draw_table_f32`` is held to
(tests/test_draw_table_gpu.py) -- against its parts written out: ``render.track_table`` of ``results.host_rows`` sorted
by id, then the padding rows; the padded table draws what the compact one draws; the C entry's argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import draw_table_cases as C
from cabi_helpers import assert_binding_matches_header

from memotr_amd import render as R
from memotr_amd.functions import clip_ops

CASES = C.named_cases()


@pytest.mark.parametrize("bgr,font_scale", C.VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_reference_is_track_table_of_the_sorted_host_rows_then_padding(name, bgr, font_scale):
    case = CASES[name]
    want, kept = C.statement(*case, bgr=bgr, font_scale=font_scale)
    got = clip_ops.draw_table_reference(*case, bgr=bgr, font_scale=font_scale)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    # CPU tensors take the reference through the public entry, into ``out`` when there is one
    out = torch.full(want.shape, 7, dtype=torch.int32)
    assert clip_ops.draw_table(*case, bgr=bgr, font_scale=font_scale, out=out) is out and np.array_equal(out.numpy(), want)
    for b, m in enumerate(kept):
        assert (want[b, m:] == np.array([0, 0, -1, -1] + [0] * 12, dtype=np.int32)).all()


def test_the_cases_hold_what_they_are_named_for():
    def ids_of(name, **kw):
        table, kept = C.statement(*CASES[name], **kw)
        ids = CASES[name][2]
        rows = []
        for b, m in enumerate(kept):
            # the id of a row, read back from its glyphs
            rows.append([int("".join(str((int(r[11 if k < 8 else 12]) >> (4 * (k % 8))) & 15) for k in range(r[10])))
                         for r in table[b, :m]])
        return rows, ids

    assert ids_of("holes_out_of_order")[0] == [[0, 2, 5, 7, 9]]
    assert ids_of("all_free")[0] == [[]] and ids_of("all_kept")[0] == [[0, 1, 2, 3, 4]]
    assert ids_of("one_class")[0] == [[2, 3]] and ids_of("eight_classes")[0] == [[1, 2, 3]]
    assert ids_of("strict_thresholds")[0] == [[3]]        # equal score, equal area and an area below: dropped
    assert ids_of("nan")[0] == [[4, 5, 6]]                      # a NaN score or extent is dropped, a NaN centre is 0
    assert ids_of("digits")[0] == [C.DIGIT_IDS] and ids_of("two_streams")[0] == [[1, 3, 64], [2, 10]]
    nan = C.statement(*CASES["nan"])[0][0]
    assert nan[0, 0] == 0 and nan[0, 2] == 0 and nan[1, 1] == 0 and nan[1, 3] == 0
    ties = C.statement(*CASES["half_pixel_ties"])[0][0]
    assert ties[0, :4].tolist() == [9, 13, 17, 21]              # 8.5, 12.5, 16.5, 20.5: floor(v + 0.5)
    assert ties[2, 0] == 0 and ties[3, :4].tolist() == [1, 1, 64, 32]        # -0.5 -> 0; 0.5 -> 1, 63.5 -> 64
    off = C.statement(*CASES["off_frame"])[0][0]
    assert off[:, 0].min() < 0 and off[:, 2].max() > 96 and off[:, 3].max() > 64
    tabs = C.statement(*CASES["tabs"])[0][0]                    # rows by id: 6, 8, 777, 12345, 2^31 - 1
    assert tabs[0, 6] == tabs[0, 1] == 8 and tabs[1, 6] == 0 and tabs[1, 1] == 9       # inside at the top; just above
    assert tabs[2, 7] == 95 and tabs[2, 5] < tabs[2, 0] and tabs[4, 7] == 95 and tabs[3, 6] == tabs[3, 1]
    wide = C.statement(*CASES["tabs"], font_scale=3)[0][0]
    assert wide[4, 5] < 0 and wide[4, 7] == 95                  # ten glyphs at scale 3: wider than the frame


def test_the_palette_is_its_integer_formula():
    for i in range(64):
        assert R.palette_entry(i) == R.PALETTE[i], i


@pytest.mark.parametrize("name", ["tabs", "digits", "off_frame", "two_streams", "all_free"])
def test_the_padded_table_draws_what_the_compact_table_draws(name):
    case = CASES[name]
    table, kept = C.statement(*case, font_scale=1)
    for b, m in enumerate(kept):
        W, H = (int(v) for v in case[3][b])
        frame = np.random.default_rng(b).integers(0, 256, (H, W, 3), dtype=np.uint8)
        padded, compact = frame.copy(), frame.copy()
        R.draw_table_host(padded, table[b], 2, 1, 96)
        R.draw_table_host(compact, table[b, :m], 2, 1, 96)
        assert np.array_equal(padded, compact) and (m == 0 or not np.array_equal(padded, frame))


def test_a_larger_id_and_bad_arguments_raise_on_the_host():
    boxes, scores, ids, ori_wh, st, at = CASES["all_kept"]
    big = ids.clone()
    big[0, 0] = 2 ** 31
    with pytest.raises(ValueError, match="track ids"):
        clip_ops.draw_table_reference(boxes, scores, big, ori_wh, st, at)
    with pytest.raises(ValueError, match="font_scale"):
        clip_ops.draw_table(boxes, scores, ids, ori_wh, st, at, font_scale=65)
    with pytest.raises(ValueError, match="ori_wh"):
        clip_ops.draw_table(boxes, scores, ids, ori_wh.double(), st, at)
    with pytest.raises(ValueError, match="ids"):
        clip_ops.draw_table(boxes, scores, ids[:, :3], ori_wh, st, at)
    with pytest.raises(ValueError, match="out"):
        clip_ops.draw_table(boxes, scores, ids, ori_wh, st, at, out=torch.zeros((1, 5, 16)))


def test_the_entry_is_declared_and_the_abi_stays_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert "clipops_draw_table_f32" in declared
    assert clip_lib.ABI_VERSION == 12 and clip_lib.lib.clipops_abi_version() == 12


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, p = clip_lib.lib, ctypes.c_void_p(64)

    def table(boxes=p, scores=p, ids=p, B=2, cap=16, K=1, ori_wh=p, bgr=0, font_scale=1, out=p):
        return lib.clipops_draw_table_f32(boxes, scores, ids, B, cap, K, ori_wh, 0.5, 100.0, bgr, font_scale, out, None)

    for kwargs in (dict(B=-1), dict(cap=-1)):
        assert table(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
    assert table(K=0) == 1 and b"K < 1" in lib.clipops_last_error()
    for scale in (0, 65, -3):
        assert table(font_scale=scale) == 1 and b"font_scale" in lib.clipops_last_error(), scale
    for name in ("boxes", "scores", "ids", "ori_wh", "out"):
        assert table(**{name: None}) == 1 and b"null" in lib.clipops_last_error(), name
    assert table(B=1 << 20, cap=1 << 20) == 1 and b"slots" in lib.clipops_last_error()
    for kwargs in (dict(B=0), dict(cap=0)):
        assert table(boxes=None, scores=None, ids=None, ori_wh=None, out=None, **kwargs) == 0, kwargs
        assert lib.clipops_last_error() == b""
