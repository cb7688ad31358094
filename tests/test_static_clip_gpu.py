"""GPU: the shift-chain kernel (memotr_amd/csrc/static_clip_ops.hip) is bit-equal to the host statement of the
definition (memotr_amd/data/static_clip.py) and to the frames the reference's ``MultiRandomShift`` produced, at the
smallest shapes that reach each of its paths and on both sides of every switch of its launch plan; it writes every
byte of the frames and none between them; ``augment_static_clip`` on a device image equals the host and feeds
``clip_forward_backward``."""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import load_golden
from model_helpers import TinyBackbone, small_config

from memotr_amd.data import augment as A
from memotr_amd.data import static_clip as S

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def static_lib():
    from memotr_amd.build import build_static_clip_lib
    build_static_clip_lib()
    from memotr_amd import _static_clip_lib
    return _static_clip_lib


def image_of(seed, h, w):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8))


def pitched_cuda(img, extra, offset):
    """The image on the device with ``extra`` unused bytes behind every row, the first byte ``offset`` bytes into the
    allocation (rows then start on every residue mod 4)."""
    h, w, _ = img.shape
    pitch = 3 * w + extra
    buf = torch.zeros(offset + h * pitch, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((h, w, 3), (pitch, 3, 1), offset)
    view.copy_(img.cuda())
    assert view.data_ptr() % 4 == (buf.data_ptr() + offset) % 4
    return view


def same(img, T, dx, dy, *, flip=False, swap=False, src=None, row_slack=5, frame_slack=7, offset=1):
    """The kernel into a 0xA5-filled buffer with slack behind rows and frames and an odd first byte, against the host
    statement: equal frames, and not one byte outside them touched.  Returns the device frames' host copy."""
    h, w, _ = img.shape
    want = S.shift_chain_cpu(img, T, dx, dy, flip=flip, swap_rb=swap)
    pitch = 3 * w + row_slack
    fpitch = h * pitch + frame_slack
    buf = torch.full((offset + T * fpitch + 8,), FILL, dtype=torch.uint8, device="cuda")
    out = buf.as_strided((T, h, w, 3), (fpitch, pitch, 3, 1), offset)
    got = S.shift_chain(img.cuda() if src is None else src, T, dx, dy, flip=flip, swap_rb=swap, out=out)
    assert got is out
    res = out.cpu()
    bad = int((res != want).sum())
    assert bad == 0, f"{bad} of {want.numel()} bytes differ, first at {(res != want).nonzero()[0].tolist()}"
    rest = buf.cpu()
    rest.as_strided((T, h, w, 3), (fpitch, pitch, 3, 1), offset).fill_(FILL)
    assert bool((rest == FILL).all()), "a byte outside the frames was written"
    return res


# ---------------------------------------------------------------------------------------------- the definition's cases
def golden_names():
    return sorted(k[:-6] for k in load_golden("static_shift") if k.endswith("::spec") and not k.startswith("e2e_"))


@pytest.mark.parametrize("name", golden_names())
def test_kernel_equals_the_host_statement_and_the_reference_frames(static_lib, name):
    g = load_golden("static_shift")
    seed, h, w, dx, dy, T = (int(x) for x in g[name + "::spec"][:6])
    img = image_of(seed, h, w)
    got = same(img, T, dx, dy)
    assert torch.equal(got[0], img) and np.array_equal(got[1:].numpy(), g[name])
    plain = S.shift_chain(img.cuda(), T, dx, dy)                              # no out=: a fresh contiguous clip
    assert plain.is_cuda and plain.is_contiguous() and torch.equal(plain.cpu(), got)


# ---------------------------------------------------------------------------------------------- strips and clipping
WIDTHS = {"1": lambda strip: 1, "5": lambda strip: 5, "strip-1": lambda strip: strip - 1, "strip": lambda strip: strip,
          "strip+1": lambda strip: strip + 1, "2*strip+3": lambda strip: 2 * strip + 3}


@pytest.mark.parametrize("dw", list(WIDTHS))
def test_widths_around_the_strip(static_lib, dw):
    h = 37
    strip, lds = static_lib.launch_plan(h, 64)
    assert lds > 0
    w = WIDTHS[dw](strip)
    assert static_lib.launch_plan(h, w)[0] == strip
    img = image_of(w, h, w)
    same(img, 4, -3, 2)            # k * s = 3, 6, 9: inside the first strip, then across its right edge
    same(img, 3, 4, -6)            # s = 0: nothing moves sideways, nothing is black


@pytest.mark.parametrize("w", [22, 21, 20])
def test_last_frame_just_inside_at_and_past_the_left_edge(static_lib, w):
    # T = 4, s = 7: (T - 1) * s = 21 is w - 1 (one column left), w (all black) and w + 1
    got = same(image_of(w, 29, w), 4, -7, -3)
    assert bool(got[3, :, :max(0, w - 21)].any()) == (w == 22) and not got[3, :, max(0, w - 21):].any()


@pytest.mark.parametrize("T", [1, 2, 8])
def test_clip_lengths(static_lib, T):
    same(image_of(T, 45, 52), T, -5, 7)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("swap", [False, True])
def test_flip_and_channel_order(static_lib, flip, swap):
    img = image_of(11, 33, 19)
    got = same(img, 3, -2, 4, flip=flip, swap=swap)
    base = S.shift_chain(img.cuda(), 3, -2, 4).cpu()
    assert torch.equal(got, base) == (not flip and not swap)
    want0 = img.flip(1) if flip else img
    assert torch.equal(got[0], want0.flip(2) if swap else want0)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_source_rows_that_start_on_any_byte(static_lib, offset):
    img = image_of(offset, 31, 27)
    for flip in (False, True):
        src = pitched_cuda(img, 1, offset)                  # row pitch 3 * w + 1: every residue mod 4 occurs
        assert src.stride(0) == 3 * 27 + 1
        same(img, 3, -4, -2, flip=flip, src=src, offset=offset, row_slack=offset)


# ---------------------------------------------------------------------------------------------- the launch plan
# (h, w): both sides of each switch.  8 -> 4 columns at h = 1170 | 1171 (two LDS images of the strip no longer fit),
# LDS -> global memory at h = 1638 | 1639, 8 -> 12 columns at w = 3071 | 3072 (256 strips stay), the widest strip (64)
PLAN_SIDES = [((1170, 9), (8, True)), ((1171, 9), (4, True)), ((1638, 5), (4, True)), ((1639, 5), (64, False)),
              ((3, 3071), (8, True)), ((3, 3072), (12, True)), ((2, 17000), (64, True))]


@pytest.mark.parametrize("size,plan", PLAN_SIDES)
def test_both_sides_of_every_switch_of_the_launch_plan(static_lib, size, plan):
    h, w = size
    strip, lds = static_lib.launch_plan(h, w)
    assert (strip, lds > 0) == plan
    same(image_of(h + w, h, w), 3, -2 if w < 100 else -70, -1 if h < 100 else 37, flip=True, swap=True)


def test_global_memory_path_over_several_strips(static_lib):
    h, w = 1700, 70                                         # two strips of 64; k * s crosses from one into the other
    assert static_lib.launch_plan(h, w) == (64, 0)
    img = image_of(5, h, w)
    same(img, 4, -9, 50)
    same(img, 3, -40, -50, flip=True)                       # (T - 1) * s > w
    same(img, 2, 3, -1, swap=True, src=pitched_cuda(img, 1, 3))


def test_full_hd_clip(static_lib):
    img = image_of(0, 1080, 1920)
    assert static_lib.launch_plan(1080, 1920)[0] == 8
    same(img, 5, -37, 23, row_slack=0, frame_slack=0, offset=0)


# ---------------------------------------------------------------------------------------------- end to end
def info_for(h, w):
    boxes = torch.tensor([[0.2 * w, 1.0, 0.6 * w, 8.0], [0.5 * w, 0.3 * h, w + 5.0, 0.6 * h],
                          [0.4 * w, 0.4 * h, 0.55 * w, 0.5 * h], [0.0, 0.55 * h, 6.5, 0.9 * h]])
    n = len(boxes)
    return {"boxes": boxes, "ids": torch.arange(n), "labels": torch.zeros(n, dtype=torch.long),
            "areas": (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])}


def plan_for(branch, **kw):
    plan = A.ClipAugment(flip=True, first=None, crop=None, final=(192, 256), hsv=(-3, 12, -20), shift=(-9, 6), **kw)
    if branch == "crop":
        plan = dataclasses.replace(plan, first=(150, 200), crop=(11, 17, 120, 161), final=(191, 255))
    return plan


@pytest.mark.parametrize("branch", ["plain", "crop"])
@pytest.mark.parametrize("srev,rev", [(False, False), (True, False), (True, True)])
def test_augment_static_clip_on_the_device_equals_the_host(static_lib, branch, srev, rev):
    img = image_of(21, 120, 160)
    info = info_for(120, 160)
    plan = plan_for(branch, reverse=rev, shift_reverse=srev)
    want, want_infos = S.augment_static_clip(img, info, plan, 4, bgr=True)
    got, got_infos = S.augment_static_clip(img.cuda(), info, plan, 4, bgr=True)
    assert got.tensors.is_cuda and got.masks.is_cuda and got.sizes == want.sizes
    assert torch.equal(got.tensors.cpu(), want.tensors) and torch.equal(got.masks.cpu(), want.masks)
    assert len(got_infos) == len(want_infos) == 4
    for a, b in zip(got_infos, want_infos):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    fwd = S.augment_static_clip(img.cuda(), info, dataclasses.replace(plan, reverse=False, shift_reverse=False), 4,
                                bgr=True)[0].tensors
    assert torch.equal(got.tensors, fwd.flip(0) if srev != rev else fwd)


def test_static_clip_feeds_the_train_step(static_lib, hip_lib, clip_lib):
    from memotr_amd.data import augment_static_clip, clip_batch
    from memotr_amd.engine import clip_forward_backward
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.criterion import build as build_criterion
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    h, w = 96, 128
    plan = A.ClipAugment(flip=True, first=None, crop=None, final=(h, w), hsv=(2, -8, 15), reverse=True, shift=(-6, 5))
    nested, infos = augment_static_clip(image_of(4, h, w).cuda(), info_for(h, w), plan, 3)
    batch = clip_batch(nested, infos)
    assert batch["imgs"][0][0].is_cuda and batch["imgs"][0][0].shape == (3, h, w) and len(batch["infos"][0]) == 3
    cfg = small_config()
    cfg.update(HIDDEN_DIM=256, FFN_DIM=256, NUM_ENC_LAYERS=1, NUM_DEC_LAYERS=2, MATCH_COST_CLASS=2, MATCH_COST_BBOX=5,
               MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5, LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0],
               SAMPLE_LENGTHS=[2, 3, 4, 5])
    torch.manual_seed(0)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=cfg["NUM_DET_QUERIES"],
                   n_feature_levels=4, hidden_dim=256, ffn_dim=256, dropout=0.0, use_dab=True).cuda()
    loss, _ = clip_forward_backward(model.train(), build_criterion(cfg), batch, torch.device("cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
