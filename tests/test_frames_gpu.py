"""GPU: the raw-frame kernel (memotr_amd/csrc/frame_ops.hip) is bit-equal to the host statement of the definition
(memotr_amd/data/frames.py) for every geometry class, batch, channel order, pitch and alignment; it is ordered with
the stream it is launched on; SequenceTracker.step_raw equals step on host-preprocessed frames."""
import pytest
import torch

from model_helpers import TinyBackbone, small_config

from memotr_amd.data import frames as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frame_lib():
    from memotr_amd.build import build_frame_lib
    build_frame_lib()
    from memotr_amd import _frame_lib
    return _frame_lib


def noise(h, w, seed=0, batch=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, ((h, w, 3) if batch is None else (batch, h, w, 3)), dtype=torch.uint8, generator=g)


def pitched_cuda(frames, extra, offset=0):
    """The frames on the device with ``extra`` unused bytes behind every row, the first byte ``offset`` bytes into
    the allocation (rows then start on every residue mod 4)."""
    B, h, w, _ = frames.shape
    pitch = 3 * w + extra
    buf = torch.zeros(offset + B * h * pitch, dtype=torch.uint8, device="cuda")
    view = buf[offset:].view(B, h, pitch)[:, :, :3 * w].unflatten(2, (w, 3))
    view.copy_(frames.cuda())
    assert view.stride(1) == pitch and view.data_ptr() % 4 == offset % 4
    return view


# h, w, batch, bgr, bytes behind a row, out= prefilled with NaN.  3 * w mod 4: 1920, 640, 3840, 1280 -> 0; 131 -> 1;
# 1242, 810 -> 2; 1333 -> 3.  The classes: plain downscale, upscale, more than 2x down, long-side cap, tiny source,
# identity, portrait.
CASES = [
    (1080, 1920, 1, False, 0, False),
    (720, 1280, 1, True, 0, True),
    (480, 640, 2, True, 0, False),
    (1080, 810, 1, False, 0, False),
    (375, 1242, 1, True, 5, False),
    (2160, 3840, 1, False, 0, True),
    (800, 1333, 1, False, 5, False),
    (97, 131, 2, False, 5, True),
]


@pytest.mark.parametrize("h,w,batch,bgr,extra,use_out", CASES)
def test_kernel_is_bit_equal_to_the_host_path(frame_lib, h, w, batch, bgr, extra, use_out):
    frames = noise(h, w, seed=h + w, batch=batch)
    want = F.preprocess_frames(frames, bgr=bgr)
    src = pitched_cuda(frames, extra) if extra else frames.cuda()
    out = torch.full(tuple(want.tensors.shape), float("nan"), device="cuda") if use_out else None
    got = F.preprocess_frames(src, bgr=bgr, out=out)
    if use_out:
        assert got.tensors is out
    assert got.tensors.is_cuda and got.masks.is_cuda and got.sizes == want.sizes
    assert torch.equal(got.masks.cpu(), want.masks)
    res = got.tensors.cpu()
    assert not torch.isnan(res).any()
    assert torch.equal(res, want.tensors)
    assert not torch.signbit(res[:, :, :, want.sizes[1][1]:]).any()          # the padding is +0.0
    assert F.preprocess_frames(src, bgr=bgr).masks is got.masks              # one mask tensor per geometry


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_rows_that_start_on_any_byte(frame_lib, offset):
    frames = noise(61, 131, seed=offset, batch=1)
    want = F.preprocess_frames(frames, size=(96, 200))
    got = F.preprocess_frames(pitched_cuda(frames, 2, offset), size=(96, 200))
    assert torch.equal(got.tensors.cpu(), want.tensors)


def test_a_reduction_too_large_for_the_lds_tile_reads_global_memory(frame_lib):
    # 4 output rows x 128 columns of a 12.5x / 23.4x reduction read a 52-row x 9 KB rectangle: more than a workgroup's LDS
    frames = noise(200, 3000, seed=2, batch=1)
    want = F.preprocess_frames(frames, size=(16, 128), bgr=True)
    got = F.preprocess_frames(frames.cuda(), size=(16, 128), bgr=True)
    assert torch.equal(got.tensors.cpu(), want.tensors)


def test_two_launches_are_bit_identical(frame_lib):
    src = noise(375, 1242, seed=1).cuda()
    a = F.preprocess_frames(src).tensors
    b = F.preprocess_frames(src).tensors
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_launch_is_ordered_with_the_current_stream(frame_lib):
    frames = noise(480, 640, seed=12)
    want = F.preprocess_frames(frames).tensors
    host_in = frames.pin_memory()
    host_out = torch.empty(tuple(want.shape), dtype=torch.float32, pin_memory=True)
    src = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
    F.preprocess_frames(src)                      # the geometry's tables and mask exist; a stale read would give this
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):               # fill, launch and read back on `stream` only; wait for its event
        src.copy_(host_in, non_blocking=True)
        got = F.preprocess_frames(src)
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
    cfg.update(HIDDEN_DIM=hidden, FFN_DIM=ffn, NUM_ENC_LAYERS=2, NUM_DEC_LAYERS=2)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=cfg["NUM_DET_QUERIES"],
                   n_feature_levels=4, hidden_dim=hidden, ffn_dim=ffn, dropout=0.0, use_dab=True)
    return model.cuda()


@pytest.mark.parametrize("graphs", [True, False])
def test_step_raw_with_lookahead_equals_step_on_host_preprocessed_frames(frame_lib, hip_lib, clip_lib, monkeypatch,
                                                                         graphs):
    from memotr_amd.inference import SequenceTracker
    import memotr_amd.modules.ms_deform_attn as mod
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "1" if graphs else "0")
    frames = [noise(150, 200, seed=40 + i) for i in range(6)]
    raw_size = (192, 320)
    th, tw = F.target_size(150, 200, *raw_size)
    assert (th, tw) == (192, 256)

    def tracker():
        torch.manual_seed(4)
        model = build_memotr_cuda().eval()
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, mod.MSDeformAttn):
                    m.sampling_offsets.weight.normal_(0, 0.02)
                    m.attention_weights.weight.normal_(0, 0.05)
        return SequenceTracker(model, det_score_thresh=0.0, track_score_thresh=0.0, result_score_thresh=0.0,
                               miss_tolerance=5, use_dab=True, area_thresh=0, raw_size=raw_size), model

    def run(raw):
        t, model = tracker()
        if raw:
            srcs = [f.numpy() if i % 2 else f for i, f in enumerate(frames)]       # numpy and torch, pageable memory
        else:
            srcs = [F.preprocess_frames(f, bgr=True, size=(th, tw)).tensors[0][:, :th, :tw].cuda() for f in frames]
        outs, masks = [], []
        for i, f in enumerate(srcs):
            if i == 2:
                t.tracker.det_score_thresh = 2.0            # births on the first two frames, then the set settles
            nxt = srcs[i + 1] if i + 1 < len(srcs) else None
            outs.append(t.step_raw(f, nxt, bgr=True) if raw else t.step(f, 150, 200, next_image=nxt))
        return outs, model

    got, model = run(True)
    want, _ = run(False)
    enc = model.infer_graphs().encode
    if graphs:
        assert enc.replays > 0 and enc.eager == 0 and not enc.failed and enc.captures == 2
    else:
        assert enc.replays == 0
    assert len(want[-1]) >= 3
    for a, b in zip(got, want):
        assert a.ids.tolist() == b.ids.tolist()
        print("max box / score difference", float((a.boxes - b.boxes).abs().max()), float((a.scores - b.scores).abs().max()))
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores)


def test_track_reuses_one_mask_per_geometry(frame_lib):
    a = F.preprocess_frames(noise(97, 131, seed=1).cuda())
    b = F.preprocess_frames(noise(97, 131, seed=2).cuda())
    c = F.preprocess_frames(noise(97, 132, seed=2).cuda())
    assert a.masks is b.masks and a.masks is not c.masks and a.tensors.data_ptr() != b.tensors.data_ptr()
