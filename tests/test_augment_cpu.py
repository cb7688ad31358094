"""CPU: training-clip augmentation (memotr_amd/data/augment.py).  The host statement of the resize against Pillow byte
for byte (live where PIL imports, and against committed Pillow outputs everywhere), the reference's size arithmetic,
the integer HSV round trip against float64 over its whole domain, the box bookkeeping against expectations written out
by hand, the plan sampler's ranges, the C ABI of libaugment_ops_hip.so without a device, and one clip through
``clip_forward_backward``."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from conftest import ROOT, load_golden
from model_helpers import build_small_memotr, patch_operator, small_config

from memotr_amd.data import augment as A
from memotr_amd.data import frames as F
from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor

# (h, w) -> (oh, ow): the geometries the definition was established on, one horizontal-only, one identity
GEOMETRIES = [((1080, 1920), (608, 1081)), ((1080, 1920), (1200, 2133)), ((270, 480), (864, 1536)),
              ((97, 131), (41, 300)), ((64, 48), (64, 31)), ((33, 57), (90, 57)), ((1000, 1777), (800, 1422)),
              ((7, 5), (3, 11)), ((33, 57), (33, 90)), ((20, 30), (20, 30))]


def noise(h, w, seed=0, T=None):
    a = np.random.RandomState(seed).randint(0, 256, (h, w, 3) if T is None else (T, h, w, 3), dtype=np.uint8)
    return torch.from_numpy(a)


def plan_of(spec):
    seed, h, w, flip, h1, w1, i, j, ch, cw, oh, ow = (int(x) for x in spec)
    return A.ClipAugment(flip=bool(flip), first=(h1, w1) if h1 else None, crop=(i, j, ch, cw) if h1 else None,
                         final=(oh, ow), hsv=None, reverse=False)


# ---------------------------------------------------------------------------------------------- resize against Pillow
@pytest.mark.parametrize("src,dst", GEOMETRIES)
def test_host_resize_is_pillow_bilinear_to_the_byte(src, dst):
    Image = pytest.importorskip("PIL.Image")
    (h, w), (oh, ow) = src, dst
    img = noise(h, w, seed=h * w)
    plan = A.ClipAugment(flip=False, first=None, crop=None, final=(oh, ow))
    got = A.resample_plan_cpu(img[None], plan)[0].numpy()
    want = np.asarray(Image.fromarray(img.numpy()).resize((ow, oh), Image.BILINEAR))
    assert got.shape == want.shape == (oh, ow, 3) and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("flip", [False, True])
def test_host_flip_and_crop_branch_are_pillow_to_the_byte(flip):
    Image = pytest.importorskip("PIL.Image")
    img = noise(270, 480, seed=3)
    pil = Image.fromarray(img.numpy())
    if flip:
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
    plain = A.ClipAugment(flip=flip, first=None, crop=None, final=(152, 270))
    assert np.array_equal(A.resample_plan_cpu(img[None], plain)[0].numpy(),
                          np.asarray(pil.resize((270, 152), Image.BILINEAR)))
    i, j, ch, cw = 37, 101, 201, 333
    crop = A.ClipAugment(flip=flip, first=(300, 533), crop=(i, j, ch, cw), final=(176, 291))
    want = pil.resize((533, 300), Image.BILINEAR).crop((j, i, j + cw, i + ch)).resize((291, 176), Image.BILINEAR)
    assert np.array_equal(A.resample_plan_cpu(img[None], crop)[0].numpy(), np.asarray(want))


def golden_names():
    return sorted(k[:-6] for k in load_golden("augment_resample") if k.endswith("::spec"))


@pytest.mark.parametrize("name", golden_names())
def test_host_resize_equals_the_committed_pillow_outputs(name):
    g = load_golden("augment_resample")
    spec = g[name + "::spec"]
    seed, h, w = (int(x) for x in spec[:3])
    assert max(h, w) <= 131
    got = A.resample_plan_cpu(noise(h, w, seed=seed)[None], plan_of(spec))[0].numpy()
    assert got.shape == g[name].shape and np.array_equal(got, g[name])


def test_golden_fixture_covers_both_branches_and_flip():
    g = load_golden("augment_resample")
    specs = [g[n + "::spec"] for n in golden_names()]
    assert len(specs) >= 10
    assert any(s[3] and s[4] for s in specs) and any(s[3] and not s[4] for s in specs)
    assert any(not s[3] and s[4] for s in specs) and any(tuple(s[1:3]) == tuple(s[10:12]) for s in specs)


def test_resample_tables_are_pillows_triangle_filter():
    xmin, cnt, kk = A.resample_tables(1920, 1081)
    assert xmin.dtype == cnt.dtype == kk.dtype == torch.int32 and kk.shape == (1081, 5) and len(xmin) == len(cnt) == 1081
    assert int(xmin.min()) == 0 and int((xmin + cnt).max()) == 1920 and int(cnt.min()) >= 1 and int(cnt.max()) <= 5
    assert bool((xmin[1:] >= xmin[:-1]).all()) and bool(((xmin + cnt)[1:] >= (xmin + cnt)[:-1]).all())
    assert int(kk.min()) >= 0 and int((kk.sum(1) - (1 << 22)).abs().max()) <= 5
    assert bool((kk * (torch.arange(5)[None] >= cnt[:, None])).eq(0).all())       # zero past cnt
    assert A.resample_tables(1920, 1081)[2] is kk                                 # cached
    xmin, cnt, kk = A.resample_tables(9, 9)                                       # the identity comes out of the tables
    assert xmin.tolist() == list(range(9)) and kk[:, 0].tolist() == [1 << 22] * 9 and not kk[:, 1:].any()
    assert A.resample_tables(131, 300)[2].shape[1] == 3 and A.resample_tables(97, 41)[2].shape[1] == 7
    with pytest.raises(ValueError):
        A.resample_tables(0, 4)


def test_new_hw_is_the_reference_arithmetic():
    assert A.new_hw(1920, 1080, 608, 1536) == (608, 1080)
    assert A.new_hw(1920, 1080, 992, 1536) == (864, 1536)
    assert A.new_hw(1080, 1920, 800, 1536) == (1422, 800)
    assert A.new_hw(1920, 1080, 800) == (800, 1422)                # no cap: int(800 * 1920 / 1080)
    assert A.new_hw(1920, 1080, [300, 200], 1536) == (200, 300)    # the list form is (w, h) and comes back as (h, w)
    assert A.new_hw(1920, 1080, (300, 200)) == (200, 300)
    with pytest.raises(ValueError):
        A.new_hw(1920, 1080, [300])


# ---------------------------------------------------------------------------------------------- HSV
def test_rgb_to_hsv_is_within_one_of_float64_for_every_rgb_triple():
    lv = torch.arange(256, dtype=torch.int32)
    worst_h = worst_s = 0.0
    for r0 in range(0, 256, 32):
        rgb = torch.stack(torch.meshgrid(lv[r0:r0 + 32], lv, lv, indexing="ij"), -1).reshape(-1, 3)
        hsv = A.rgb_to_hsv(rgb)
        r, g, b = (rgb[:, i].double() for i in range(3))
        v = torch.maximum(torch.maximum(r, g), b)
        d = v - torch.minimum(torch.minimum(r, g), b)
        s = torch.where(v > 0, 255 * d / v.clamp(min=1), torch.zeros_like(v))
        h = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * d, r - g + 4 * d)) * 30 / d.clamp(min=1)
        h = torch.where(d > 0, h, torch.zeros_like(h))
        h = torch.where(h < 0, h + 180, h)
        assert int(hsv[:, 0].min()) >= 0 and int(hsv[:, 0].max()) <= 179
        assert int(hsv[:, 1].min()) >= 0 and int(hsv[:, 1].max()) <= 255
        assert torch.equal(hsv[:, 2].double(), v)
        dh = (hsv[:, 0].double() - h).abs()
        worst_h = max(worst_h, float(torch.minimum(dh, 180 - dh).max()))
        worst_s = max(worst_s, float((hsv[:, 1].double() - s).abs().max()))
    print(f"RGB -> HSV over 2^24 triples: max |dH| {worst_h:.4f} (circular), max |dS| {worst_s:.4f}")
    assert worst_h <= 1.0 and worst_s <= 1.0


def test_hsv_to_rgb_is_within_one_level_of_float64_for_every_hsv_triple():
    lv = torch.arange(256, dtype=torch.int32)
    worst = 0.0
    for h0 in range(0, 180, 20):
        hsv = torch.stack(torch.meshgrid(torch.arange(h0, h0 + 20, dtype=torch.int32), lv, lv, indexing="ij"),
                          -1).reshape(-1, 3)
        got = A.hsv_to_rgb(hsv).double()
        h, s, v = hsv[:, 0].double() / 30, hsv[:, 1].double() / 255, hsv[:, 2].double()
        sec = torch.floor(h)
        f = h - sec
        p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
        table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
        want = torch.zeros_like(got)
        for k in range(6):
            for c in range(3):
                want[:, c] = torch.where(sec == k, table[k][c], want[:, c])
        assert float(got.min()) >= 0 and float(got.max()) <= 255
        worst = max(worst, float((got - want).abs().max()))
    print(f"HSV -> RGB over 180 * 256 * 256 triples: max |d level| {worst:.4f}")
    assert worst <= 1.0


def test_hsv_jitter_wraps_the_hue_and_clamps_saturation_and_value():
    rgb = torch.tensor([[200, 30, 40], [10, 200, 220], [255, 0, 0], [90, 90, 90], [3, 9, 5]], dtype=torch.uint8)
    h, s, v = A.rgb_to_hsv(rgb).unbind(-1)
    assert h.tolist()[0] > 170 and h.tolist()[2] == 0

    def expect(dh, ds, dv):
        return A.hsv_to_rgb(torch.stack(((h + dh) % 180, (s + ds).clamp(0, 255), (v + dv).clamp(0, 255)), -1))

    for dh, ds, dv in ((-5, 0, 0), (5, 0, 0), (0, 30, 0), (0, 0, -30), (-5, 30, -30), (179, -300, 300)):
        got = A.hsv_jitter(rgb, dh, ds, dv)
        assert torch.equal(got, expect(dh, ds, dv)), (dh, ds, dv)
        assert int(got.min()) >= 0 and int(got.max()) <= 255
    # h + dh < 0 wraps to 180 + (h + dh): pure red (h = 0) moved by -5 is hue 175
    assert A.rgb_to_hsv(A.hsv_jitter(rgb[2:3], -5, 0, 0))[0, 0].item() in (174, 175, 176)
    # h + dh >= 180 wraps to below: hue > 170 moved by +20 lands in the reds / oranges
    assert A.rgb_to_hsv(A.hsv_jitter(rgb[0:1], 20, 0, 0))[0, 0].item() < 20
    # s + ds > 255 saturates: the smallest channel of a saturated colour goes to 0;  v + dv < 0 gives black
    assert A.hsv_jitter(rgb[0:1], 0, 250, 0)[0].min().item() == 0
    assert A.hsv_jitter(rgb[4:5], 0, 0, -30)[0].tolist() == [0, 0, 0]
    # the zero-gain round trip is applied, and is not the identity on every colour.  How far it can move a level: H is
    # kept in units of 2 degrees, one unit moves the middle channel by d / 30 <= 8.5 levels and H is within 0.64 of
    # exact (5.5 levels); S within 0.53 / 255 of v (0.53); the rounding of HSV -> RGB (0.5): below 7 levels.
    every = torch.stack(torch.meshgrid(*[torch.arange(0, 256, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    back = A.hsv_jitter(every, 0, 0, 0)
    assert int((back - every).abs().max()) < 7 and not torch.equal(back, every.to(torch.int32))


# ---------------------------------------------------------------------------------------------- boxes
def infos_for(boxes, T=1):
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    n = len(boxes)
    out = []
    for t in range(T):
        b = boxes + t
        out.append({"boxes": b, "ids": torch.arange(n) + 10, "labels": torch.zeros(n, dtype=torch.long),
                    "areas": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])})
    return out


def test_infos_flip_and_plain_resize():
    # 100 x 200 frame (h x w), flipped, resized to 50 x 300: x -> (200 - x) * 1.5, y -> y * 0.5
    plan = A.ClipAugment(flip=True, first=None, crop=None, final=(50, 300))
    src = infos_for([[20, 10, 60, 50]])
    got = A.augment_infos(plan, src, 100, 200)[0]
    x0, x1, y0, y1 = (200 - 60) * 1.5, (200 - 20) * 1.5, 5.0, 25.0
    want = torch.tensor([[(x0 + x1) / 2 / 300, (y0 + y1) / 2 / 50, (x1 - x0) / 300, (y1 - y0) / 50]])
    assert torch.allclose(got["boxes"], want, rtol=0, atol=1e-6)
    assert torch.allclose(got["areas"], torch.tensor([40.0 * 40 * 1.5 * 0.5]))
    assert got["ids"].tolist() == [10] and got["labels"].tolist() == [0]
    assert src[0]["boxes"].tolist() == [[20, 10, 60, 50]]                   # the input is left alone
    same = A.augment_infos(A.ClipAugment(False, None, None, (100, 200)), src, 100, 200)[0]
    assert torch.allclose(same["boxes"], torch.tensor([[0.2, 0.3, 0.2, 0.4]]))


@pytest.mark.parametrize("overflow", [False, True])
def test_infos_crop_branch_cuts_keeps_and_drops(overflow):
    # 100 x 200 -> first 200 x 400 (x2) -> crop rows 40..139, columns 100..299 -> final 50 x 100 (x0.5)
    plan = A.ClipAugment(flip=False, first=(200, 400), crop=(40, 100, 100, 200), final=(50, 100))
    inside, cut, outside = [60, 30, 100, 60], [30, 10, 80, 40], [160, 75, 190, 95]
    got = A.augment_infos(plan, infos_for([inside, cut, outside]), 100, 200, overflow_bbox=overflow)[0]
    assert got["ids"].tolist() == [10, 11] and len(got["labels"]) == 2 and len(got["areas"]) == 2
    # inside: doubled (120, 60, 200, 120), shifted (20, 20, 100, 80), halved (10, 10, 50, 40)
    assert torch.allclose(got["boxes"][0], torch.tensor([30 / 100, 25 / 50, 40 / 100, 30 / 50]), atol=1e-6)
    # cut: doubled (60, 20, 160, 80), shifted (-40, -20, 60, 40); clamped (0, 0, 60, 40) unless boxes may overflow
    x0, y0, x1, y1 = ((-40, -20, 60, 40) if overflow else (0, 0, 60, 40))
    want = torch.tensor([(x0 + x1) / 4 / 100, (y0 + y1) / 4 / 50, (x1 - x0) / 2 / 100, (y1 - y0) / 2 / 50])
    assert torch.allclose(got["boxes"][1], want, atol=1e-6)
    # areas follow the two resizes only (the reference does not recompute them after the crop)
    assert torch.allclose(got["areas"], torch.tensor([40.0 * 30, 50.0 * 30]) * 4 * 0.25)


def test_infos_empty_boxes_and_reversal():
    plan = A.ClipAugment(flip=True, first=(200, 400), crop=(40, 100, 100, 200), final=(50, 100), reverse=True)
    empty = {"boxes": torch.zeros((0, 4)), "ids": torch.zeros((0,), dtype=torch.long),
             "labels": torch.zeros((0,), dtype=torch.long), "areas": torch.zeros((0,))}
    got = A.augment_infos(plan, [empty], 100, 200)[0]
    assert got["boxes"].shape == (0, 4) and got["ids"].shape == (0,) and got["areas"].shape == (0,)
    src = infos_for([[60, 30, 100, 60]], T=3)
    fwd = A.augment_infos(A.ClipAugment(False, None, None, (50, 100)), src, 100, 200)
    rev = A.augment_infos(A.ClipAugment(False, None, None, (50, 100), reverse=True), src, 100, 200)
    assert len(rev) == 3 and not torch.equal(fwd[0]["boxes"], fwd[2]["boxes"])
    for a, b in zip(fwd, rev[::-1]):
        assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["ids"], b["ids"])
    with pytest.raises(ValueError):
        A.augment_infos(A.ClipAugment(False, (50, 50), (0, 0, 60, 10), (50, 100)), src, 100, 200)


# ---------------------------------------------------------------------------------------------- the plan sampler
def test_sampled_plans_stay_inside_the_reference_ranges():
    h, w = 1080, 1920
    seen = set()
    for seed in range(200):
        plan = A.sample_clip_augment(h, w, random.Random(seed), np.random.RandomState(seed), reverse_clip=0.5)
        assert plan == A.sample_clip_augment(h, w, random.Random(seed), np.random.RandomState(seed), reverse_clip=0.5)
        if plan.first is None:
            assert plan.crop is None
            sw, sh = w, h
        else:
            assert plan.first in [A.new_hw(w, h, s) for s in (800, 1000, 1200)]
            i, j, ch, cw = plan.crop
            assert 800 <= ch <= min(plan.first[0], 1200) and 800 <= cw <= min(plan.first[1], 1200)
            assert 0 <= i and i + ch <= plan.first[0] and 0 <= j and j + cw <= plan.first[1]
            sw, sh = cw, ch
        assert plan.final in [A.new_hw(sw, sh, s, 1536) for s in A.SCALES]
        assert max(plan.final) <= 1536 and min(plan.final) <= 992
        assert all(isinstance(x, int) for x in plan.hsv)
        assert abs(plan.hsv[0]) <= 5 and abs(plan.hsv[1]) <= 30 and abs(plan.hsv[2]) <= 30
        seen.add((plan.flip, plan.first is None, plan.reverse))
    assert len(seen) == 8                                           # both flips x both branches x both orders
    assert not A.sample_clip_augment(h, w, random.Random(0), np.random.RandomState(0)).reverse
    coco = [A.sample_clip_augment(480, 640, random.Random(s), np.random.RandomState(s), coco_size=True)
            for s in range(40)]
    assert all(384 <= p.crop[2] <= 600 and 384 <= p.crop[3] <= 600 for p in coco if p.crop is not None)
    small = A.sample_clip_augment(97, 131, random.Random(1), np.random.RandomState(1))     # small frames are upscaled
    assert min(small.final) >= 608 or max(small.final) == 1536


# ---------------------------------------------------------------------------------------------- augment_clip on the host
def test_augment_clip_on_the_host_is_resize_hsv_table_and_padding():
    frames = noise(60, 90, seed=5, T=3)
    plan = A.ClipAugment(flip=True, first=(80, 120), crop=(3, 7, 61, 75), final=(66, 81), hsv=(-4, 20, -25),
                         reverse=True)
    infos = infos_for([[10, 10, 60, 50]], T=3)
    nt, out_infos = A.augment_clip(frames, infos, plan)
    assert nt.tensors.shape == (3, 3, 96, 96) and nt.sizes == ((96, 96), (66, 81), (66, 81), (66, 81))
    q = A.hsv_jitter(A.resample_plan_cpu(frames, plan), -4, 20, -25).long().flip(0)
    lut = F.normalize_table()
    for c in range(3):
        assert torch.equal(nt.tensors[:, c, :66, :81], lut[c][q[..., c]])
    want = tensor_list_to_nested_tensor([t[:, :66, :81] for t in nt.tensors])
    assert torch.equal(nt.tensors, want.tensors) and torch.equal(nt.masks, want.masks)
    assert not torch.signbit(nt.tensors[:, :, 66:]).any() and not torch.signbit(nt.tensors[:, :, :, 81:]).any()
    assert [i["boxes"].tolist() for i in out_infos] == [i["boxes"].tolist() for i in
                                                        A.augment_infos(plan, infos, 60, 90)]
    # bgr, numpy, pitched rows, out=, no HSV
    plain = A.ClipAugment(flip=False, first=None, crop=None, final=(41, 100), hsv=None)
    a = A.augment_clip(frames, infos, plain, bgr=True)[0].tensors
    assert torch.equal(a, A.augment_clip(frames.flip(-1).contiguous(), infos, plain)[0].tensors)
    assert torch.equal(A.augment_clip(frames.numpy(), infos, plain, bgr=True)[0].tensors, a)
    pitched = torch.zeros((3, 60, 90 * 3 + 5), dtype=torch.uint8)
    pitched[:, :, :270] = frames.reshape(3, 60, -1)
    assert torch.equal(A.augment_clip(pitched[:, :, :270].unflatten(2, (90, 3)), infos, plain, bgr=True)[0].tensors, a)
    out = torch.full(tuple(a.shape), float("nan"))
    assert A.augment_clip(frames, infos, plain, bgr=True, out=out)[0].tensors is out and torch.equal(out, a)
    zero = A.augment_clip(frames, infos, dataclass_replace(plain, hsv=(0, 0, 0)), bgr=True)[0].tensors
    assert not torch.equal(zero, a)                                  # the zero-gain round trip is applied
    with pytest.raises(ValueError):
        A.augment_clip(frames, infos[:2], plain)


def dataclass_replace(plan, **kw):
    import dataclasses
    return dataclasses.replace(plan, **kw)


# ---------------------------------------------------------------------------------------------- the library, no device
@pytest.fixture(scope="module")
def augment_lib():
    from memotr_amd.build import build_augment_lib
    build_augment_lib()
    from memotr_amd import _augment_lib
    return _augment_lib


def test_library_exports_every_declared_symbol(augment_lib):
    syms = assert_binding_matches_header(augment_lib, "augment_ops_hip.h", "augops", "AUGOPS_ABI_VERSION")
    assert syms == ["augops_abi_version", "augops_last_error", "augops_resample_u8"]
    header = open(os.path.join(ROOT, "include", "augment_ops_hip.h")).read()
    assert int(re.search(r"#define AUGOPS_STAGE_U8 (\d+)", header).group(1)) == augment_lib.STAGE_U8
    assert int(re.search(r"#define AUGOPS_STAGE_F32 (\d+)", header).group(1)) == augment_lib.STAGE_F32
    # the frame library's header is left as it was
    frame_header = open(os.path.join(ROOT, "include", "frame_ops_hip.h")).read()
    assert "augops_" not in frame_header


def test_argument_errors_are_reported_without_a_device(augment_lib):
    lib = augment_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch

    def call(src=p, row_pitch=3 * 64, frame_pitch=3 * 64 * 48, T=1, h=48, w=64, flip=0, swap=0, xmin_x=p, cnt_x=p,
             kk_x=p, ks_x=3, xmin_y=p, cnt_y=p, kk_y=p, ks_y=3, oh=60, ow=80, stage=1, out_u8=p, orp=3 * 80,
             ofp=3 * 80 * 60, out_f32=p, Hp=64, Wp=96, lut=p, hsv_div=p, use_hsv=1, dh=0, ds=0, dv=0, reverse=0):
        return lib.augops_resample_u8(src, row_pitch, frame_pitch, T, h, w, flip, swap, xmin_x, cnt_x, kk_x, ks_x,
                                      xmin_y, cnt_y, kk_y, ks_y, oh, ow, stage, out_u8, orp, ofp, out_f32, Hp, Wp,
                                      lut, hsv_div, use_hsv, dh, ds, dv, reverse, None)

    def err():
        return lib.augops_last_error()

    for name in ("src", "xmin_x", "cnt_x", "kk_x", "xmin_y", "cnt_y", "kk_y", "out_f32", "lut", "hsv_div"):
        assert call(**{name: None}) == 1 and b"null" in err(), name
    assert call(stage=0, out_u8=None) == 1 and b"null" in err()
    # (a stage does not ask for the other stage's pointers: they pass validation and fail on a size instead)
    assert call(stage=0, out_f32=None, lut=None, hsv_div=None, orp=1) == 6
    assert call(out_u8=None, use_hsv=0, hsv_div=None, Wp=98) == 8
    for name in ("h", "w", "oh", "ow", "Hp", "Wp"):
        for bad in (0, -3):
            assert call(**{name: bad}) == 2 and b"non-positive size" in err(), name
    assert call(T=-1) == 2 and b"negative frame count" in err()
    assert call(stage=2) == 3 and b"stage" in err()
    for name in ("ks_x", "ks_y"):
        assert call(**{name: 0}) == 4 and b"tap count" in err()
    for name in ("flip", "swap", "use_hsv", "reverse"):
        assert call(**{name: 2}) == 5 and b"not 0 or 1" in err(), name
    assert call(row_pitch=3 * 64 - 1) == 6 and b"row pitch" in err()
    assert call(T=2, frame_pitch=-1) == 6 and b"frame pitch" in err()
    assert call(stage=0, orp=3 * 80 - 1) == 6 and b"output row pitch" in err()
    assert call(stage=0, T=2, ofp=-1) == 6 and b"output frame pitch" in err()
    assert call(Hp=32) == 7 and b"padded size" in err()                    # Hp < oh
    assert call(Wp=64) == 7 and b"padded size" in err()                    # Wp < ow
    assert call(Wp=98) == 8 and b"multiple of 4" in err()
    assert call(out_f32=ctypes.c_void_p(4100)) == 9 and b"aligned" in err()
    for name in ("dh", "ds", "dv"):
        assert call(**{name: 40000}) == 10 and b"HSV gain" in err()
    assert call(Hp=16 * 65536 + 16, oh=16 * 65536 + 1) == 11 and b"65535" in err()
    assert call(T=65536) == 11 and b"65535" in err()
    # an empty problem is fine, launches nothing and clears the error text
    assert call(T=0) == 0 and err() == b""
    with pytest.raises(RuntimeError, match="null pointer"):
        augment_lib.check(call(src=None), "augops_resample_u8")


# ---------------------------------------------------------------------------------------------- into the train step
def test_clip_batch_runs_through_clip_forward_backward(monkeypatch):
    from memotr_amd.data import augment_clip, clip_batch
    from memotr_amd.engine import clip_forward_backward
    from memotr_amd.models.criterion import build as build_criterion
    patch_operator(monkeypatch)
    cfg = small_config()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3, 4, 5])
    torch.manual_seed(0)
    model = build_small_memotr().train()
    frames = noise(60, 90, seed=8, T=2)
    infos = infos_for([[10, 10, 50, 40], [40, 20, 80, 55], [5, 30, 30, 58]], T=2)
    plan = A.ClipAugment(flip=True, first=(80, 120), crop=(2, 6, 70, 100), final=(96, 137), hsv=(3, -10, 12),
                         reverse=True)
    nt, new_infos = augment_clip(frames, infos, plan)
    batch = clip_batch(nt, new_infos)
    assert list(batch) == ["imgs", "infos"] and len(batch["imgs"]) == 1 and len(batch["imgs"][0]) == 2
    assert batch["imgs"][0][0].shape == (3, 96, 137) and batch["imgs"][0][0].data_ptr() == nt.tensors.data_ptr()
    assert sorted(batch["infos"][0][0]) == ["boxes", "ids", "labels"] and len(batch["infos"][0][0]["ids"]) == 3
    loss, loss_dict = clip_forward_backward(model, build_criterion(cfg), batch, torch.device("cpu"))
    assert torch.isfinite(loss) and loss_dict
    with pytest.raises(ValueError):
        clip_batch(nt, new_infos[:1])
