"""CPU: the host statement of the track overlay (memotr_amd/render.py draw_tracks_host) against the committed scene
(tests/golden/track_draw_scene.npz) and against structural facts that follow from the definition; the palette is its
integer formula; the font in the library is the font in Python; the C ABI is what the header declares."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

import cabi_helpers
from cabi_helpers import assert_binding_matches_header
from conftest import load_golden
from track_draw_cases import IDS, SIZES, frame, many, named_boxes

from memotr_amd import render as R


@pytest.fixture(scope="module")
def draw_lib():
    from memotr_amd.build import build_track_draw_lib
    build_track_draw_lib()
    from memotr_amd import _track_draw_lib
    return _track_draw_lib


@pytest.fixture(scope="module")
def scene():
    return load_golden("track_draw_scene")


def test_the_committed_scene(scene):
    assert np.array_equal(R.track_table(scene["ids"], scene["boxes"], 96, 64), scene["table"])
    for k in range(3):
        bgr, t, s, a = (int(v) for v in scene[f"options_{k}"])
        got = R.draw_tracks_host(scene["frame"], scene["ids"], scene["boxes"], bgr=bool(bgr), thickness=t,
                                 font_scale=s, fill_alpha=a)
        assert isinstance(got, np.ndarray) and np.array_equal(got, scene[f"expected_{k}"]), k
        as_torch = R.draw_tracks(torch.from_numpy(scene["frame"]), torch.from_numpy(scene["ids"]),
                                 torch.from_numpy(scene["boxes"]), bgr=bool(bgr), thickness=t, font_scale=s,
                                 fill_alpha=a)
        assert torch.is_tensor(as_torch) and np.array_equal(as_torch.numpy(), scene[f"expected_{k}"]), k


def test_palette_is_its_formula_and_the_text_colour_follows_the_luma():
    assert len(R.PALETTE) == 64 and len(set(R.PALETTE)) == 64
    assert list(R.PALETTE) == [R.palette_entry(i) for i in range(64)]
    assert all(0 <= c <= 255 for rgb in R.PALETTE for c in rgb)
    t = R.track_table([0, 1, 64 + 1], np.zeros((3, 4), np.float32), 50, 50)
    assert t[0, 4] == 255 and t[0, 9] == 0xFFFFFF          # pure red: luma 76, white text
    r, g, b = R.PALETTE[1]
    assert (77 * r + 150 * g + 29 * b) >> 8 >= 128 and t[1, 9] == 0
    assert t[2, 4] == t[1, 4]                              # id % 64
    swapped = R.track_table([1], np.zeros((1, 4), np.float32), 50, 50, bgr=True)
    assert swapped[0, 4] == (b | g << 8 | r << 16) and t[1, 4] == (r | g << 8 | b << 16)


def test_rectangles_round_half_up_in_float32_and_are_clamped():
    t = R.track_table([1, 2, 3], [[0.5, 1.49, 2.5, -0.5], [-1.5, -0.51, 1e30, float("-inf")],
                                  [float("nan"), 16777217.0, 3.0, 4.0]], 50, 50)
    assert t[0, :4].tolist() == [1, 1, 3, 0]
    assert t[1, :4].tolist() == [-1, -1, 1 << 24, -(1 << 24)]
    assert t[2, :4].tolist() == [0, 1 << 24, 3, 4]


def test_structural_facts():
    h, w = 64, 96
    src = frame(h, w)
    out = R.draw_tracks_host(src, [7], [[20.0, 30.0, 60.0, 50.0]])
    colour = np.array(R.PALETTE[7], np.uint8)
    for y, x in ((30, 20), (30, 60), (50, 20), (50, 60), (31, 21), (49, 59), (40, 21), (31, 40)):
        assert np.array_equal(out[y, x], colour), (y, x)          # corners and the second ring: thickness 2
    assert np.array_equal(out[32:49, 22:59], src[32:49, 22:59])  # fill_alpha = 0: the interior is unchanged
    # nothing outside the rectangle and the tab is written
    mask = np.ones((h, w), bool)
    mask[30:51, 20:61] = False
    mask[21:30, 20:27] = False                                   # the tab: 7 x 9 above the box's top-left corner
    assert np.array_equal(out[mask], src[mask])
    assert np.array_equal(out[21, 20], colour) and np.array_equal(out[29, 26], colour)
    # bgr swaps the bytes
    assert np.array_equal(R.draw_tracks_host(src, [7], [[20.0, 30.0, 60.0, 50.0]], bgr=True)[30, 20], colour[::-1])
    # alpha 255 replaces, 128 blends with rounding
    full = R.draw_tracks_host(src, [7], [[20.0, 30.0, 60.0, 50.0]], fill_alpha=255)
    assert (full[32:49, 22:59] == colour).all()
    half = R.draw_tracks_host(src, [7], [[20.0, 30.0, 60.0, 50.0]], fill_alpha=128)
    want = (colour.astype(np.int64) * 128 + src[40, 40].astype(np.int64) * 127 + 127) // 255
    assert np.array_equal(half[40, 40], want)
    # inverted and wholly outside: nothing; one pixel; thinner than twice the thickness: filled
    for name in ("inverted", "outside"):
        assert np.array_equal(R.draw_tracks_host(src, [3] * len(named_boxes(h, w)[name]), named_boxes(h, w)[name]), src)
    one = R.draw_tracks_host(src, [3], [[20.0, 40.0, 20.0, 40.0]])
    assert np.array_equal(one[40, 20], np.array(R.PALETTE[3], np.uint8))
    assert np.array_equal(one[41, 20], src[41, 20]) and np.array_equal(one[40, 21], src[40, 21])
    thin = R.draw_tracks_host(src, [3], [[15.0, 20.0, 17.0, 50.0]], fill_alpha=0)
    assert (thin[20:51, 15:18] == np.array(R.PALETTE[3], np.uint8)).all()
    # the input is never written, an `out` is, out=frame draws in place
    keep = src.copy()
    dst = np.zeros_like(src)
    assert R.draw_tracks_host(src, [7], [[20.0, 30.0, 60.0, 50.0]], out=dst) is dst
    assert np.array_equal(src, keep) and np.array_equal(dst, out)
    work = src.copy()
    assert R.draw_tracks_host(work, [7], [[20.0, 30.0, 60.0, 50.0]], out=work) is work and np.array_equal(work, out)


@pytest.mark.parametrize("scale", [1, 2])
def test_glyph_area_reproduces_the_font(scale):
    for tid in IDS + [9876543]:
        src = np.full((40, 200, 3), 9, np.uint8)
        out = R.draw_tracks_host(src, [tid], [[5.0, 25.0, 150.0, 38.0]], font_scale=scale)
        colour = np.array(R.PALETTE[tid % 64], np.uint8)
        r, g, b = R.PALETTE[tid % 64]
        text = np.array([0, 0, 0] if (77 * r + 150 * g + 29 * b) >> 8 >= 128 else [255] * 3, np.uint8)
        digits = [int(c) for c in str(tid)]
        tab_w, tab_h = (6 * len(digits) - 1) * scale + 2, 7 * scale + 2
        tab = out[25 - tab_h:25, 5:5 + tab_w]
        want = np.empty_like(tab)
        want[...] = colour
        for k, d in enumerate(digits):
            for gr in range(7):
                for gc in range(5):
                    if (R.FONT[d][gr] >> (4 - gc)) & 1:
                        y0, x0 = 1 + gr * scale, 1 + (6 * k + gc) * scale
                        want[y0:y0 + scale, x0:x0 + scale] = text
        assert np.array_equal(tab, want), tid
        assert (out[25 - tab_h - 1, :] == 9).all() and (out[25 - tab_h:25, 5 + tab_w:] == 9).all()


def test_tab_placement():
    t = R.track_table([7, 7, 12345678, 12345678], [[8, 10, 40, 30], [8, 8, 40, 30], [90, 10, 95, 30], [-20, 10, 5, 30]],
                      96, 64)
    assert t[0, 5:9].tolist() == [8, 1, 14, 9]             # above: 9 rows end at y1 - 1
    assert t[1, 5:9].tolist() == [8, 8, 14, 16]            # y1 - 9 < 0: inside, from y1
    assert t[2, 5:9].tolist() == [96 - 49, 1, 95, 9]       # 8 glyphs: 49 wide, shifted left to end at column 95
    assert t[3, 5:9].tolist() == [-20, 1, 28, 9]           # left of the frame: clipped, not shifted
    assert t[2, 10] == 8 and [(int(t[2, 11]) >> (4 * k)) & 15 for k in range(8)] == [1, 2, 3, 4, 5, 6, 7, 8]
    big = R.track_table([2 ** 31 - 1], [[0, 0, 5, 5]], 96, 64)
    assert big[0, 10] == 10
    assert [(int(big[0, 11]) >> (4 * k)) & 15 for k in range(8)] + [(int(big[0, 12]) >> (4 * k)) & 15 for k in range(2)] \
        == [2, 1, 4, 7, 4, 8, 3, 6, 4, 7]


def test_every_case_draws_and_order_matters():
    for h, w in SIZES:
        src = frame(h, w)
        for name, boxes in named_boxes(h, w).items():
            out = R.draw_tracks_host(src, [IDS[i % 5] for i in range(len(boxes))], boxes, fill_alpha=128)
            assert out.shape == src.shape and out.dtype == np.uint8, name
        a = R.draw_tracks_host(src, [1, 2, 3], named_boxes(h, w)["overlap"])
        b = R.draw_tracks_host(src, [3, 2, 1], named_boxes(h, w)["overlap_reversed"])
        assert not np.array_equal(a, b)                     # the same boxes and ids in the other order
        ids, boxes = many(h, w)
        assert len(ids) == 70 and not np.array_equal(R.draw_tracks_host(src, ids, boxes), src)
        assert np.array_equal(R.draw_tracks_host(src, [], np.zeros((0, 4), np.float32)), src)


def test_a_track_instances_is_taken_whole():
    from memotr_amd.structures.track_instances import TrackInstances
    t = TrackInstances(hidden_dim=8, num_classes=1)
    t.ids = torch.tensor([3, 12])
    t.boxes = torch.tensor([[5.0, 12.0, 30.0, 30.0], [20.0, 15.0, 50.0, 35.0]])
    t.labels = torch.tensor([0, 0])
    src = torch.from_numpy(frame(37, 53))
    assert torch.equal(R.draw_tracks(src, t), R.draw_tracks(src, t.ids, t.boxes, t.labels))


def test_bad_arguments_raise():
    src = frame(16, 16)
    with pytest.raises(ValueError, match="ids for"):
        R.draw_tracks_host(src, [1, 2], [[0, 0, 5, 5]])
    with pytest.raises(ValueError, match="track ids"):
        R.draw_tracks_host(src, [-1], [[0, 0, 5, 5]])
    for kw in (dict(thickness=0), dict(font_scale=0), dict(fill_alpha=256), dict(fill_alpha=0.5), dict(thickness=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            R.draw_tracks_host(src, [1], [[0, 0, 5, 5]], **kw)
    with pytest.raises(ValueError, match="uint8"):
        R.draw_tracks_host(src.astype(np.float32), [1], [[0, 0, 5, 5]])


def test_library_font_header_and_argument_codes(draw_lib):
    lib, err = draw_lib.lib, draw_lib.lib.trackdraw_last_error
    font = np.zeros(70, np.uint8)
    lib.trackdraw_font(font.ctypes.data)
    assert font.reshape(10, 7).tolist() == [list(g) for g in R.FONT]
    syms = assert_binding_matches_header(draw_lib, "track_draw_hip.h", "trackdraw", "TRACKDRAW_ABI_VERSION")
    assert syms == ["trackdraw_abi_version", "trackdraw_draw_u8", "trackdraw_font", "trackdraw_last_error"]
    define = partial(cabi_helpers.define, "track_draw_hip.h")
    assert draw_lib.ABI_VERSION == 1
    assert define("TRACKDRAW_ROW_WORDS") == draw_lib.ROW_WORDS == R.ROW_WORDS
    assert define("TRACKDRAW_MAX_GLYPHS") == draw_lib.MAX_GLYPHS == R.MAX_GLYPHS
    assert (define("TRACKDRAW_TILE_X"), define("TRACKDRAW_TILE_Y"), define("TRACKDRAW_CHUNK")) == \
        (draw_lib.TILE_X, draw_lib.TILE_Y, draw_lib.CHUNK)
    from memotr_amd import _jpeg_lib
    assert (draw_lib.TILE_X, draw_lib.TILE_Y) == (_jpeg_lib.TILE_X, _jpeg_lib.TILE_Y)

    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)   # never dereferenced: validation comes before any launch
    ok = dict(src=p, sp=300, dst=q, dp=300, w=100, h=50, table=p, n=3, t=2, s=1, a=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.trackdraw_draw_u8(a["src"], a["sp"], a["dst"], a["dp"], a["w"], a["h"], a["table"], a["n"], a["t"],
                                     a["s"], a["a"], None)

    assert call(n=-1) == 2 and b"negative" in err()
    assert call(src=None) == 1 and b"null pointer" in err()
    assert call(table=None) == 1
    assert call(w=0) == 2 and call(h=65536) == 2
    assert call(sp=299) == 3 and b"pitch" in err()
    assert call(dst=p, dp=303) == 3 and b"in place" in err()
    assert call(dst=ctypes.c_void_p(4096 + 600)) == 4 and b"overlap" in err()
    assert call(table=ctypes.c_void_p(4098)) == 5
    assert call(t=0) == 6 and call(s=0) == 6 and call(a=256) == 6 and call(a=-1) == 6
    assert call(dst=p, n=0, table=None) == 0 and err() == b""        # in place, no rows: nothing is launched
