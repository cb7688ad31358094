"""GPU: the augmentation kernel (memotr_amd/csrc/augment_ops.hip) is bit-equal to the host statement of the definition
(memotr_amd/data/augment.py) and to the committed Pillow outputs, at the smallest shapes that reach each of its paths;
it is ordered with the stream it is launched on; ``augment_clip`` on device frames equals ``augment_clip`` on host
frames and feeds ``clip_forward_backward``."""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import load_golden
from model_helpers import TinyBackbone, small_config

from memotr_amd.data import augment as A
from memotr_amd.data import frames as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def augment_lib():
    from memotr_amd.build import build_augment_lib
    build_augment_lib()
    from memotr_amd import _augment_lib
    return _augment_lib


def noise(h, w, seed=0, T=1):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (T, h, w, 3), dtype=np.uint8))


def infos_for(T, n=3):
    g = torch.Generator().manual_seed(n)
    out = []
    for t in range(T):
        xy = torch.rand(n, 2, generator=g) * 40
        b = torch.cat((xy, xy + 5 + torch.rand(n, 2, generator=g) * 30), 1) + t
        out.append({"boxes": b, "ids": torch.arange(n), "labels": torch.zeros(n, dtype=torch.long),
                    "areas": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])})
    return out


def pitched_cuda(frames, extra, offset=0):
    """The frames on the device with ``extra`` unused bytes behind every row, the first byte ``offset`` bytes into
    the allocation (rows then start on every residue mod 4)."""
    T, h, w, _ = frames.shape
    pitch = 3 * w + extra
    buf = torch.zeros(offset + T * h * pitch, dtype=torch.uint8, device="cuda")
    view = buf[offset:].view(T, h, pitch)[:, :, :3 * w].unflatten(2, (w, 3))
    view.copy_(frames.cuda())
    assert view.stride(1) == pitch and view.data_ptr() % 4 == offset % 4
    return view


def plain(oh, ow, **kw):
    return A.ClipAugment(flip=kw.pop("flip", False), first=None, crop=None, final=(oh, ow), hsv=kw.pop("hsv", None),
                         reverse=kw.pop("reverse", False))


def same(frames, plan, *, bgr=False, src=None, out=None):
    """augment_clip on device frames against augment_clip on the same host frames; returns the device result."""
    infos = infos_for(frames.shape[0])
    want, want_infos = A.augment_clip(frames, infos, plan, bgr=bgr)
    got, got_infos = A.augment_clip(frames.cuda() if src is None else src, infos, plan, bgr=bgr, out=out)
    assert got.tensors.is_cuda and got.masks.is_cuda and got.sizes == want.sizes
    res = got.tensors.cpu()
    assert not torch.isnan(res).any()
    assert torch.equal(res, want.tensors)
    assert torch.equal(got.masks.cpu(), want.masks)
    th, tw = plan.final
    assert not res[:, :, th:].any() and not res[:, :, :, tw:].any()
    assert not torch.signbit(res[:, :, th:]).any() and not torch.signbit(res[:, :, :, tw:]).any()    # +0.0
    for a, b in zip(got_infos, want_infos):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    return got


# mixed down / up with 7 and 3 taps; one pass the identity; cnt cut at both edges; a > 4x reduction whose tiles do not
# fit the LDS they are given (all but the bottom-right one: 76 rows x 217 dwords against 10240) and a 25x one
GEOMETRIES = [((97, 131), (41, 300)), ((64, 48), (64, 31)), ((7, 5), (3, 11)), ((270, 480), (61, 109)),
              ((200, 64), (8, 16)), ((33, 57), (90, 57)), ((20, 30), (20, 30))]


@pytest.mark.parametrize("src,dst", GEOMETRIES)
def test_kernel_is_bit_equal_to_the_host_path(augment_lib, src, dst):
    same(noise(*src, seed=src[0] + dst[1]), plain(*dst))


@pytest.mark.parametrize("oh", [15, 16, 17])
@pytest.mark.parametrize("ow", [63, 64, 65])
def test_output_sizes_around_the_tile_size(augment_lib, oh, ow):
    same(noise(29, 83, seed=oh * ow), plain(oh, ow, hsv=(2, -7, 9)))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_rows_that_start_on_any_byte(augment_lib, offset):
    frames = noise(61, 131, seed=offset, T=2)
    for flip in (False, True):
        same(frames, plain(96, 200, flip=flip), src=pitched_cuda(frames, 5, offset))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("bgr", [False, True])
def test_flip_and_channel_order(augment_lib, flip, bgr):
    frames = noise(45, 70, seed=7)
    got = same(frames, plain(50, 90, flip=flip), bgr=bgr).tensors
    base = A.augment_clip(frames.cuda(), infos_for(1), plain(50, 90))[0].tensors
    assert torch.equal(got, base) == (not flip and not bgr)
    # the crop branch flips and swaps in its first launch only
    crop = A.ClipAugment(flip=flip, first=(60, 93), crop=(5, 9, 41, 67), final=(50, 90), hsv=(1, 2, 3))
    same(frames, crop, bgr=bgr)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("reverse", [False, True])
def test_frame_index_map(augment_lib, T, reverse):
    frames = noise(40, 52, seed=T, T=T)
    got = same(frames, plain(33, 70, reverse=reverse)).tensors
    fwd = A.augment_clip(frames.cuda(), infos_for(T), plain(33, 70))[0].tensors
    assert torch.equal(got, fwd.flip(0) if reverse else fwd)


def test_crop_window_with_odd_offsets_through_table_slices(augment_lib):
    frames = noise(72, 128, seed=11, T=2)
    for crop in ((7, 13, 61, 75), (1, 3, 17, 65), (0, 0, 90, 160), (89, 159, 1, 1)):
        same(frames, A.ClipAugment(flip=True, first=(90, 160), crop=crop, final=(66, 81), hsv=None))
    # the u8 stage on its own, into a pitched destination at an odd address: only the window is written
    lib = augment_lib
    i, j, ch, cw = 7, 13, 61, 75
    tx = A._slice_tables(A._device_tables(128, 160, torch.device("cuda", 0)), j, cw)
    ty = A._slice_tables(A._device_tables(72, 90, torch.device("cuda", 0)), i, ch)
    buf = torch.full((1 + 2 * ch * (3 * cw + 7),), 201, dtype=torch.uint8, device="cuda")
    dst = buf[1:].view(2, ch, 3 * cw + 7)
    src = frames.cuda()
    A._launch(lib, src, 2, 72, 128, False, False, tx, ty, ch, cw, out_u8=dst[:, :, :3 * cw].unflatten(2, (cw, 3)),
              stream=torch.cuda.current_stream().cuda_stream)
    want = A.resample_cpu(frames, A._slice_tables(A.resample_tables(128, 160), j, cw),
                          A._slice_tables(A.resample_tables(72, 90), i, ch))
    assert torch.equal(dst[:, :, :3 * cw].cpu().reshape(2, ch, cw, 3), want)
    assert bool((dst[:, :, 3 * cw:] == 201).all()) and int(buf[0]) == 201


def test_out_is_fully_overwritten(augment_lib):
    frames = noise(97, 131, seed=10, T=2)
    plan = plain(41, 100, hsv=(0, 0, 0))
    out = torch.full((2, 3, 64, 128), float("nan"), device="cuda")
    got = same(frames, plan, out=out)
    assert got.tensors is out
    with pytest.raises(ValueError):
        A.augment_clip(frames.cuda(), infos_for(2), plan, out=torch.empty((2, 3, 64, 96), device="cuda"))


@pytest.mark.parametrize("hsv", [None, (0, 0, 0), (-5, 30, -30), (5, -30, 30), (-200, 300, -300)])
def test_hsv_stage(augment_lib, hsv):
    frames = noise(50, 60, seed=13)
    frames[0, :2, :, :] = torch.tensor([255, 0, 0], dtype=torch.uint8)       # pure red: h + dh < 0 wraps
    frames[0, 2:4] = 0
    frames[0, 4:6] = 255
    got = same(frames, plain(50, 60, hsv=hsv)).tensors
    off = A.augment_clip(frames.cuda(), infos_for(1), plain(50, 60))[0].tensors
    assert torch.equal(got, off) == (hsv is None)


def golden_names():
    return sorted(k[:-6] for k in load_golden("augment_resample") if k.endswith("::spec"))


@pytest.mark.parametrize("name", golden_names())
def test_kernel_equals_the_committed_pillow_outputs(augment_lib, name):
    g = load_golden("augment_resample")
    seed, h, w, flip, h1, w1, i, j, ch, cw, oh, ow = (int(x) for x in g[name + "::spec"])
    plan = A.ClipAugment(flip=bool(flip), first=(h1, w1) if h1 else None, crop=(i, j, ch, cw) if h1 else None,
                         final=(oh, ow), hsv=None)
    frames = torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8))
    got = A.augment_clip(frames.cuda(), infos_for(1), plan)[0].tensors.cpu()
    lut = F.normalize_table()
    q = torch.from_numpy(g[name]).long()
    for c in range(3):
        assert torch.equal(got[0, c, :oh, :ow], lut[c][q[..., c]])


def test_two_launches_are_bit_identical(augment_lib):
    src = noise(97, 131, seed=1, T=2).cuda()
    plan = A.ClipAugment(flip=True, first=(120, 160), crop=(3, 5, 100, 131), final=(80, 105), hsv=(1, 2, 3))
    a = A.augment_clip(src, infos_for(2), plan)[0]
    b = A.augment_clip(src, infos_for(2), plan)[0]
    assert a.tensors.data_ptr() != b.tensors.data_ptr() and torch.equal(a.tensors, b.tensors) and a.masks is b.masks


def test_launch_is_ordered_with_the_current_stream(augment_lib):
    frames = noise(120, 160, seed=12, T=2)
    plan = A.ClipAugment(flip=False, first=(150, 200), crop=(3, 5, 131, 171), final=(96, 125), hsv=(1, -2, 3))
    infos = infos_for(2)
    want = A.augment_clip(frames, infos, plan)[0].tensors
    host_in = frames.pin_memory()
    host_out = torch.empty(tuple(want.shape), dtype=torch.float32, pin_memory=True)
    src = torch.zeros((2, 120, 160, 3), dtype=torch.uint8, device="cuda")
    A.augment_clip(src, infos, plan)               # the geometry's tables and mask exist; a stale read would give this
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                # fill, launch twice and read back on `stream` only; wait for its event
        src.copy_(host_in, non_blocking=True)
        got = A.augment_clip(src, infos, plan)[0]
        host_out.copy_(got.tensors, non_blocking=True)
        done = stream.record_event()
    done.synchronize()
    assert torch.equal(host_out, want)
    got.tensors.record_stream(stream)


def build_memotr_cuda(hidden=256, ffn=256):
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    cfg = small_config()
    cfg.update(HIDDEN_DIM=hidden, FFN_DIM=ffn, NUM_ENC_LAYERS=1, NUM_DEC_LAYERS=2)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=cfg["NUM_DET_QUERIES"],
                   n_feature_levels=4, hidden_dim=hidden, ffn_dim=ffn, dropout=0.0, use_dab=True)
    return model.cuda(), cfg


@pytest.mark.parametrize("branch", ["plain", "crop"])
def test_augment_clip_on_the_device_equals_the_host_and_feeds_the_train_step(augment_lib, hip_lib, clip_lib, branch):
    from memotr_amd.data import augment_clip, clip_batch
    from memotr_amd.engine import clip_forward_backward
    from memotr_amd.models.criterion import build as build_criterion
    frames = noise(120, 160, seed=21, T=3)
    plan = A.ClipAugment(flip=True, first=None, crop=None, final=(192, 256), hsv=(-3, 12, -20), reverse=True)
    if branch == "crop":
        plan = dataclasses.replace(plan, first=(150, 200), crop=(11, 17, 120, 161), final=(191, 255))
    got = same(frames, plan, bgr=True)
    infos = infos_for(3)
    nested, new_infos = augment_clip(frames.cuda(), infos, plan, bgr=True)
    assert torch.equal(nested.tensors, got.tensors)
    batch = clip_batch(nested, new_infos)
    assert batch["imgs"][0][0].is_cuda and batch["imgs"][0][0].shape == (3,) + tuple(plan.final)
    torch.manual_seed(0)
    model, cfg = build_memotr_cuda()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3, 4, 5])
    loss, _ = clip_forward_backward(model.train(), build_criterion(cfg), batch, torch.device("cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
