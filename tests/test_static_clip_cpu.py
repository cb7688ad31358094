"""CPU: clips made from one still image (memotr_amd/data/static_clip.py).  The host statement of the shift chain
against the frames and boxes the reference's own ``MultiRandomShift`` produced (tests/golden/static_shift.npz, see
gen_golden_static_shift.py) and against live Pillow where PIL imports; the plan sampler's shift draws; the C ABI of
libstatic_clip_ops_hip.so without a device; ``augment_static_clip`` against ``augment_clip`` on the chain's frames and
against the reference's end-to-end infos."""
import ctypes
import dataclasses
import os
import random

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from conftest import ROOT, load_golden

from memotr_amd.data import augment as A
from memotr_amd.data import static_clip as S

# (h, w, dx, dy, T): the fixture's cases; the last two have a zero the reference cannot draw
CASES = {"left_down": (67, 45, -7, 5, 5), "right_up": (67, 45, 7, -5, 5), "one_row_all_black": (51, 20, -50, 50, 4),
         "one_row_up": (51, 20, -1, -50, 3), "black_from_frame_1": (90, 33, -40, 17, 5),
         "right_only_moves_rows": (64, 64, 50, 1, 2), "dy_zero": (40, 30, -3, 0, 3), "dx_zero": (40, 30, 0, -4, 3)}
DRAWN = [n for n, c in CASES.items() if c[2] and c[3]]


def image_of(seed, h, w):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def golden():
    return load_golden("static_shift")


def fields(g, prefix):
    return {f: torch.from_numpy(g[f"{prefix}::{f}"]) for f in ("boxes", "ids", "labels", "areas") if f"{prefix}::{f}" in g}


def same_infos(got, g, prefix):
    for k, info in enumerate(got):
        want = fields(g, f"{prefix}::{k}")
        assert sorted(k_ for k_ in info if k_ in ("boxes", "ids", "labels", "areas")) == sorted(want), (prefix, k)
        for f, v in want.items():
            assert info[f].dtype == v.dtype and torch.equal(info[f], v), (prefix, k, f)


# ---------------------------------------------------------------------------------------------- pixels
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_chain_equals_the_reference_frames(golden, name):
    seed, h, w, dx, dy, T, torch_seed, _ = (int(x) for x in golden[name + "::spec"])
    assert (h, w, dx, dy, T) == CASES[name] and (torch_seed >= 0) == (name in DRAWN)
    img = image_of(seed, h, w)
    got = S.shift_chain_cpu(img, T, dx, dy)
    assert got.shape == (T, h, w, 3) and got.dtype == torch.uint8
    assert torch.equal(got[0], img)
    assert np.array_equal(got[1:].numpy(), golden[name])
    assert torch.equal(S.shift_chain(img.numpy(), T, dx, dy), got)            # the dispatcher, numpy in
    s = max(0, -dx)
    for k in range(1, T):                                                     # the black that PIL pads with
        assert not got[k, :, max(0, w - k * s):].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_chain_equals_live_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    h, w, dx, dy, T = CASES[name]
    a = image_of(h * w, h, w)
    for flip in (False, True):
        got = S.shift_chain_cpu(a, T, dx, dy, flip=flip, swap_rb=flip).numpy()
        img = Image.fromarray(a.numpy()[:, :, ::-1].copy() if flip else a.numpy())
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        for k in range(T):
            assert np.array_equal(got[k], np.asarray(img)), (name, flip, k)
            y_min, y_max, x_min, x_max = max(0, -dy), min(h, h - dy), max(0, -dx), max(w, w - dx)
            img = img.crop((x_min, y_min, x_max, y_max)).resize((w, h), Image.BILINEAR)


def test_chain_arguments():
    img = image_of(0, 12, 9)
    assert torch.equal(S.shift_chain_cpu(img, 1, -3, 2)[0], img)              # T = 1: the image alone
    assert torch.equal(S.shift_chain_cpu(img[None], 2, 5, 0)[1], img)         # dx > 0 moves nothing, dy = 0 neither
    for bad in (dict(T=0), dict(dy=12), dict(dy=-12)):
        with pytest.raises(ValueError):
            S.shift_chain_cpu(img, **{"T": 3, "dx": 1, "dy": 1, **bad})
    with pytest.raises(ValueError):
        S.shift_chain(torch.stack((img, img)), 2, 1, 1)                       # one image, not a clip
    # pitched rows in, pitched rows and frames out: only the frames' bytes are written
    wide = torch.zeros((12, 9 * 3 + 5), dtype=torch.uint8)
    wide[:, :27] = img.reshape(12, 27)
    want = S.shift_chain_cpu(img, 3, -2, -1)
    assert torch.equal(S.shift_chain(wide[:, :27].unflatten(1, (9, 3)), 3, -2, -1), want)
    buf = torch.full((3, 14, 31), 0xA5, dtype=torch.uint8)
    out = buf[:, :12, :27].unflatten(2, (9, 3))
    assert S.shift_chain(img, 3, -2, -1, out=out) is out and torch.equal(out, want)
    assert bool((buf[:, 12:] == 0xA5).all()) and bool((buf[:, :, 27:] == 0xA5).all())
    with pytest.raises(ValueError):
        S.shift_chain(img, 3, -2, -1, out=torch.empty((2, 12, 9, 3), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------- boxes
@pytest.mark.parametrize("name", DRAWN)
def test_shift_infos_equal_the_reference(golden, name):
    h, w, dx, dy, T = CASES[name]
    for variant in ("full", "empty", "noboxes"):
        info = {k[len(f"{name}::in::{variant}::"):]: torch.from_numpy(v) for k, v in golden.items()
                if k.startswith(f"{name}::in::{variant}::")}
        assert ("boxes" in info) == (variant != "noboxes")
        before = {k: v.clone() for k, v in info.items()}
        got = S.shift_infos(info, T, dx, dy, h, w)
        assert len(got) == T and all(torch.equal(info[k], before[k]) for k in info)      # the input is left alone
        same_infos(got, golden, f"{name}::info::{variant}")
        if variant == "noboxes":
            assert all(sorted(i) == ["ids"] and torch.equal(i["ids"], info["ids"]) for i in got)


def test_shift_infos_drop_clip_and_keep_the_areas(golden):
    h, w, dx, dy, T = CASES["right_up"]
    info = fields(golden, "right_up::in::full")
    got = S.shift_infos(info, T, dx, dy, h, w)
    ids = [i["ids"].tolist() for i in got]
    assert ids == [[10, 11, 12, 13], [10, 11, 12, 13], [11, 12, 13], [11, 12, 13], [11, 12, 13]]   # through the top, gone
    assert float(info["boxes"][1, 2]) > w and all(float(i["boxes"][i["ids"] == 11][0, 2]) == w for i in got[1:])
    mid = [i["boxes"][i["ids"] == 12][0] for i in got]                        # never clipped: x as it was, y moved
    assert all(torch.equal(b[[0, 2]], mid[0][[0, 2]]) for b in mid) and all(0 < float(b[1]) < float(b[3]) < h for b in mid)
    for i in got:                                                             # areas are not rescaled
        assert torch.equal(i["areas"], info["areas"][i["ids"] - 10])
    with pytest.raises(ValueError):
        S.shift_infos(info, 3, 1, h, h, w)
    with pytest.raises(ValueError):
        S.shift_infos(info, 0, 1, 1, h, w)


# ---------------------------------------------------------------------------------------------- the plan sampler
def test_sampled_shifts_stay_in_range_and_are_off_by_default():
    seen = set()
    for seed in range(1000):
        base = A.sample_clip_augment(1080, 1920, random.Random(seed), np.random.RandomState(seed), reverse_clip=0.5)
        assert base.shift is None and base.shift_reverse is False
        plan = A.sample_clip_augment(1080, 1920, random.Random(seed), np.random.RandomState(seed), reverse_clip=0.5,
                                     max_shift=7)
        assert dataclasses.replace(plan, shift=None, shift_reverse=False) == base     # the other draws are unchanged
        dx, dy = plan.shift
        assert isinstance(dx, int) and isinstance(dy, int) and 1 <= abs(dx) <= 7 and 1 <= abs(dy) <= 7
        assert isinstance(plan.shift_reverse, bool)
        seen.add((dx, dy, plan.shift_reverse))
    assert {abs(s[0]) for s in seen} == {abs(s[1]) for s in seen} == set(range(1, 8))
    assert {(s[0] > 0, s[1] > 0, s[2]) for s in seen} == {(a, b, c) for a in (False, True) for b in (False, True)
                                                           for c in (False, True)}
    with pytest.raises(ValueError):
        A.sample_clip_augment(1080, 1920, random.Random(0), np.random.RandomState(0), max_shift=0)


# ---------------------------------------------------------------------------------------------- the library, no device
@pytest.fixture(scope="module")
def static_lib():
    from memotr_amd.build import build_static_clip_lib
    build_static_clip_lib()
    from memotr_amd import _static_clip_lib
    return _static_clip_lib


def test_library_exports_every_declared_symbol(static_lib):
    syms = assert_binding_matches_header(static_lib, "static_clip_ops_hip.h", "staticclip", "STATICCLIP_ABI_VERSION")
    assert syms == ["staticclip_abi_version", "staticclip_last_error", "staticclip_plan", "staticclip_shift_chain"]
    # the augmentation library's header is left as it was
    assert "staticclip_" not in open(os.path.join(ROOT, "include", "augment_ops_hip.h")).read()


def test_launch_plan_is_a_function_of_the_size(static_lib):
    assert static_lib.launch_plan(1080, 1920) == (8, 8 * 1080 * 7)
    assert static_lib.launch_plan(1170, 40) == (8, 8 * 1170 * 7) and static_lib.launch_plan(1171, 40) == (4, 8 * 1171 * 5)
    assert static_lib.launch_plan(1638, 5) == (4, 8 * 1638 * 5) and static_lib.launch_plan(1639, 5) == (64, 0)
    assert static_lib.launch_plan(3, 3071)[0] == 8 and static_lib.launch_plan(3, 3072)[0] == 12
    assert static_lib.launch_plan(2, 16384)[0] == 64 and static_lib.launch_plan(2, 40000)[0] == 64
    for h in (1, 96, 744, 745, 1080, 1638):
        strip, lds = static_lib.launch_plan(h, 4096)
        assert strip % 4 == 0 and 4 <= strip <= 64 and 0 < lds <= 64 * 1024 and lds == 8 * h * ((3 * strip // 4 + 1) | 1)
    strip, lds = ctypes.c_int(), ctypes.c_int()
    assert static_lib.lib.staticclip_plan(0, 5, ctypes.byref(strip), ctypes.byref(lds)) == 2
    assert static_lib.lib.staticclip_plan(5, 5, None, ctypes.byref(lds)) == 1


def test_argument_errors_are_reported_without_a_device(static_lib):
    lib = static_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch

    def call(src=p, row_pitch=3 * 64, h=48, w=64, T=3, flip=0, swap=0, s=5, y0=2, hc=40, xmin=p, cnt=p, kk=p, ks=3, out=p,
             orp=3 * 64, ofp=3 * 64 * 48):
        return lib.staticclip_shift_chain(src, row_pitch, h, w, T, flip, swap, s, y0, hc, xmin, cnt, kk, ks, out, orp,
                                          ofp, None)

    def err():
        return lib.staticclip_last_error()

    for name in ("src", "xmin", "cnt", "kk", "out"):
        assert call(**{name: None}) == 1 and b"null" in err(), name
    for name in ("h", "w"):
        for bad in (0, -3):
            assert call(**{name: bad}) == 2 and b"non-positive size" in err(), name
    for bad in (0, -1):
        assert call(T=bad) == 3 and b"clip length" in err()
    assert call(ks=0) == 4 and b"tap count" in err()
    for name in ("flip", "swap"):
        assert call(**{name: 2}) == 5 and b"not 0 or 1" in err(), name
    assert call(row_pitch=3 * 64 - 1) == 6 and b"row pitch" in err()
    assert call(orp=3 * 64 - 1) == 6 and b"output row pitch" in err()
    assert call(ofp=3 * 64 * 48 - 1) == 6 and b"output frame pitch" in err()
    assert call(s=-1) == 7 and b"column shift" in err()
    for bad in (dict(y0=-1), dict(hc=0), dict(y0=9, hc=40)):
        assert call(**bad) == 8 and b"row window" in err(), bad
    with pytest.raises(RuntimeError, match="null pointer"):
        static_lib.check(call(src=None), "staticclip_shift_chain")
    assert b"null" in err()


# ---------------------------------------------------------------------------------------------- augment_static_clip
def e2e_plan(spec):
    _, h, w, dx, dy, T, srev, flip, rev, h1, w1, i, j, c, th, tw, overflow, _ = (int(x) for x in spec)
    plan = A.ClipAugment(flip=bool(flip), first=(h1, w1) if h1 else None, crop=(i, j, c, c) if h1 else None,
                         final=(th, tw), hsv=None, reverse=bool(rev), shift=(dx, dy), shift_reverse=bool(srev))
    return plan, T, bool(overflow)


@pytest.mark.parametrize("branch", ["plain", "crop"])
@pytest.mark.parametrize("srev", [0, 1])
@pytest.mark.parametrize("rev", [0, 1])
def test_augment_static_clip_is_the_chain_through_augment_clip_and_the_reference_infos(golden, branch, srev, rev):
    name = f"e2e_{branch}_{srev}{rev}"
    spec = golden[name + "::spec"]
    plan, T, overflow = e2e_plan(spec)
    assert (plan.first is None) == (branch == "plain") and plan.shift_reverse == bool(srev) and plan.reverse == bool(rev)
    plan = dataclasses.replace(plan, hsv=(2, -9, 11))                         # (boxes do not see the HSV step)
    h, w = int(spec[1]), int(spec[2])
    img = image_of(int(spec[0]), h, w)
    info = fields(golden, name + "::in")
    before = {k: v.clone() for k, v in info.items()}
    nt, infos = S.augment_static_clip(img, info, plan, T, overflow_bbox=overflow)
    assert all(torch.equal(info[k], before[k]) for k in info)
    same_infos(infos, golden, name)                                           # the reference's composed transforms

    # the same, by hand: flip the boxes, the chain's frames and infos, the shift's reversal, then augment_clip
    flipped = dict(info)
    if plan.flip:
        flipped["boxes"] = info["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
    frames = S.shift_chain_cpu(img, T, *plan.shift, flip=plan.flip)
    chain_infos = S.shift_infos(flipped, T, *plan.shift, h, w)
    if plan.shift_reverse:
        frames, chain_infos = frames.flip(0), chain_infos[::-1]
    want, want_infos = A.augment_clip(frames, chain_infos, dataclasses.replace(plan, flip=False), overflow_bbox=overflow)
    assert torch.equal(nt.tensors, want.tensors) and torch.equal(nt.masks, want.masks) and nt.sizes == want.sizes
    for a, b in zip(infos, want_infos):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    if srev != rev:                                                           # the frames really come out last first
        fwd = A.augment_clip(S.shift_chain_cpu(img, T, *plan.shift, flip=plan.flip), chain_infos,
                             dataclasses.replace(plan, flip=False, reverse=False))[0].tensors
        assert torch.equal(nt.tensors, fwd.flip(0)) and not torch.equal(nt.tensors, fwd)


def test_augment_static_clip_arguments_and_export(golden):
    from memotr_amd.data import augment_static_clip, clip_batch
    assert augment_static_clip is S.augment_static_clip
    img = image_of(3, 40, 52)
    info = fields(golden, "left_down::in::full")
    plan = A.ClipAugment(flip=False, first=None, crop=None, final=(64, 83), shift=(-3, 4))
    nt, infos = augment_static_clip(img, info, plan, 3)
    assert nt.tensors.shape == (3, 3, 64, 96) and len(infos) == 3
    batch = clip_batch(nt, infos)
    assert len(batch["imgs"][0]) == 3 and batch["imgs"][0][2].shape == (3, 64, 83)
    bgr = augment_static_clip(img.flip(-1).numpy(), info, plan, 3, bgr=True)[0].tensors
    assert torch.equal(bgr, nt.tensors)
    out = torch.full((3, 3, 64, 96), float("nan"))
    assert augment_static_clip(img, info, plan, 3, out=out)[0].tensors is out and torch.equal(out, nt.tensors)
    with pytest.raises(ValueError, match="no shift"):
        augment_static_clip(img, info, dataclasses.replace(plan, shift=None), 3)
    with pytest.raises(ValueError):
        augment_static_clip(img, info, plan, 0)
    with pytest.raises(ValueError):
        augment_static_clip(img, info, dataclasses.replace(plan, shift=(1, 40)), 3)
