"""CPU: raw-frame ingestion (memotr_amd/data/frames.py).  The host statement of the definition against an independent
float64 bilinear interpolation, its exact properties (identity, constants, padding, channel order, strides, ``out=``),
the C ABI of libframe_ops_hip.so without a device, and SequenceTracker.step_raw / track against step."""
import ctypes

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from model_helpers import build_small_memotr, patch_operator

from memotr_amd.data import frames as F
from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor

SIZES = {(1080, 1920): (800, 1422), (720, 1280): (800, 1422), (480, 640): (800, 1066), (1080, 810): (1066, 800),
         (375, 1242): (463, 1536), (2160, 3840): (800, 1422), (800, 1333): (800, 1333), (97, 131): (799, 1080)}
# plain downscale, upscale, more than 2x down, long-side cap, tiny odd source
GEOMETRIES = [(1080, 1920), (480, 640), (2160, 3840), (375, 1242), (97, 131)]


def noise(h, w, seed=0, batch=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, ((h, w, 3) if batch is None else (batch, h, w, 3)), dtype=torch.uint8, generator=g)


def ramp(h, w):
    y = torch.arange(h, dtype=torch.float64)[:, None, None] / max(h - 1, 1)
    x = torch.arange(w, dtype=torch.float64)[None, :, None] / max(w - 1, 1)
    c = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)[None, None, :]
    return ((y * c + x * (1 - c)) * 255).round().to(torch.uint8)


def bilinear_f64(img, th, tw):
    """Exact bilinear interpolation in float64: half-pixel centres, coordinates clamped to the image.  (th, tw, 3)."""
    h, w = img.shape[:2]

    def axis(src, dst):
        f = ((np.arange(dst, dtype=np.float64) + 0.5) * src / dst - 0.5).clip(0, src - 1)
        i0 = np.floor(f).astype(np.int64)
        return i0, np.minimum(i0 + 1, src - 1), f - i0

    y0, y1, wy = axis(h, th)
    x0, x1, wx = axis(w, tw)
    p = img.numpy().astype(np.float64)
    wy, wx = wy[:, None, None], wx[None, :, None]
    top = p[y0][:, x0] * (1 - wx) + p[y0][:, x1] * wx
    bot = p[y1][:, x0] * (1 - wx) + p[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def test_target_size_is_the_reference_arithmetic():
    for (h, w), want in SIZES.items():
        assert F.target_size(h, w) == want, (h, w)


def test_resize_tables_are_half_pixel_centres_with_edge_clamp():
    s0, s1, a1 = F.resize_tables(1920, 1422)
    assert s0.dtype == s1.dtype == torch.int32 and a1.dtype == torch.int16 and len(s0) == len(s1) == len(a1) == 1422
    assert int(s0.min()) >= 0 and int(s1.max()) == 1919 and bool((s1 - s0 <= 1).all()) and bool((s0[1:] >= s0[:-1]).all())
    assert 0 <= int(a1.min()) and int(a1.max()) <= 2048
    s0, s1, a1 = F.resize_tables(640, 1066)                 # upscale: the first / last centres fall outside the source
    assert int(s0[0]) == 0 and int(a1[0]) == 0 and int(s0[-1]) == int(s1[-1]) == 639 and int(a1[-1]) == 0
    assert F.resize_tables(640, 1066)[0] is s0              # cached
    s0, s1, a1 = F.resize_tables(7, 7)
    assert s0.tolist() == list(range(7)) and not a1.any()


@pytest.mark.parametrize("kind", ["noise", "ramp"])
@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_host_path_is_within_one_level_of_float64_bilinear(h, w, kind):
    img = noise(h, w, seed=h) if kind == "noise" else ramp(h, w)
    th, tw = F.target_size(h, w)
    q = F._resize_levels_cpu(img[None], th, tw)[0]
    assert q.shape == (th, tw, 3) and int(q.min()) >= 0 and int(q.max()) <= 255
    err = float(np.abs(q.numpy().astype(np.float64) - bilinear_f64(img, th, tw)).max())
    print(f"{h}x{w} -> {th}x{tw} {kind}: max distance from float64 bilinear {err:.4f} levels")
    assert err < 1.0
    # and the normalised output is the table entry of that level
    nt = F.preprocess_frames(img)
    lut = F.normalize_table()
    for c in range(3):
        assert torch.equal(nt.tensors[0, c, :th, :tw], lut[c][q[..., c].long()])


def test_constant_image_stays_constant():
    img = torch.empty((480, 640, 3), dtype=torch.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 7, 130, 255
    nt = F.preprocess_frames(img)
    lut = F.normalize_table()
    for c, level in enumerate((7, 130, 255)):
        plane = nt.tensors[0, c, :800, :1066]
        assert bool((plane == lut[c, level]).all())


def test_identity_geometry_is_to_tensor_and_normalize_to_the_bit():
    img = noise(800, 1333, seed=3)
    nt = F.preprocess_frames(img)
    mean = torch.tensor(F.MEAN)[:, None, None]
    std = torch.tensor(F.STD)[:, None, None]
    want = img.permute(2, 0, 1).float().div(255).sub(mean).div(std)
    assert nt.tensors.shape == (1, 3, 800, 1344)
    assert torch.equal(nt.tensors[0, :, :, :1333], want)


@pytest.mark.parametrize("h,w,batch", [(375, 1242, 1), (97, 131, 2)])
def test_padding_masks_and_sizes_are_those_of_the_nested_tensor(h, w, batch):
    imgs = noise(h, w, seed=5, batch=batch)
    th, tw = F.target_size(h, w)
    nt = F.preprocess_frames(imgs)
    Hp, Wp = nt.tensors.shape[-2:]
    assert Hp % 32 == 0 and Wp % 32 == 0 and 0 <= Hp - th < 32 and 0 <= Wp - tw < 32 and (Hp > th or Wp > tw)
    pad = nt.tensors.clone()
    pad[:, :, :th, :tw] = 0
    assert not pad.any() and not torch.signbit(pad).any()            # exactly +0.0
    want = tensor_list_to_nested_tensor([t[:, :th, :tw] for t in nt.tensors])
    assert torch.equal(nt.tensors, want.tensors) and torch.equal(nt.masks, want.masks) and nt.sizes == want.sizes
    assert nt.masks.dtype == torch.bool
    assert F.preprocess_frames(noise(h, w, seed=6, batch=batch)).masks is nt.masks       # one mask per geometry


def test_bgr_is_the_channel_flipped_input():
    img = noise(120, 200, seed=7)
    a = F.preprocess_frames(img, bgr=True)
    b = F.preprocess_frames(img.flip(-1).contiguous())
    assert torch.equal(a.tensors, b.tensors)
    assert not torch.equal(a.tensors, F.preprocess_frames(img).tensors)


def test_pitched_and_non_contiguous_inputs_equal_the_contiguous_one():
    img = noise(90, 131, seed=8)
    want = F.preprocess_frames(img).tensors
    pitched = torch.zeros((90, 131 * 3 + 5), dtype=torch.uint8)
    pitched[:, :131 * 3] = img.reshape(90, -1)
    view = pitched[:, :131 * 3].unflatten(1, (131, 3))
    assert not view.is_contiguous() and view.stride(0) == 131 * 3 + 5
    assert torch.equal(F.preprocess_frames(view).tensors, want)
    planar = img.permute(2, 0, 1).contiguous().permute(1, 2, 0)          # channel stride != 1
    assert torch.equal(F.preprocess_frames(planar).tensors, want)
    crop = noise(100, 150, seed=9)
    assert torch.equal(F.preprocess_frames(crop[5:95, 10:141]).tensors,
                       F.preprocess_frames(crop[5:95, 10:141].contiguous()).tensors)


def test_out_is_fully_overwritten():
    img = noise(97, 131, seed=10, batch=2)
    want = F.preprocess_frames(img)
    out = torch.full(tuple(want.tensors.shape), float("nan"))
    got = F.preprocess_frames(img, out=out)
    assert got.tensors is out and torch.equal(out, want.tensors)
    with pytest.raises(ValueError):
        F.preprocess_frames(img, out=torch.empty((2, 3, 800, 1088), dtype=torch.float64))


def test_numpy_and_torch_inputs_agree():
    img = noise(75, 210, seed=11)
    want = F.preprocess_frames(img)
    got = F.preprocess_frames(img.numpy())
    assert torch.equal(got.tensors, want.tensors) and got.sizes == want.sizes
    batch = np.stack([img.numpy(), img.numpy()[::-1]])                   # (B, H, W, 3)
    assert torch.equal(F.preprocess_frames(batch).tensors[0], want.tensors[0])
    assert torch.equal(F.preprocess_frames(img.numpy()[::-1]).tensors,  # negative stride
                       F.preprocess_frames(img.flip(0)).tensors)
    with pytest.raises(TypeError):
        F.preprocess_frames(img.float())
    with pytest.raises(ValueError):
        F.preprocess_frames(torch.zeros((4, 4), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------- the library, no device
@pytest.fixture(scope="module")
def frame_lib():
    from memotr_amd.build import build_frame_lib
    build_frame_lib()
    from memotr_amd import _frame_lib
    return _frame_lib


def test_library_exports_every_declared_symbol(frame_lib):
    syms = assert_binding_matches_header(frame_lib, "frame_ops_hip.h", "frameops", "FRAMEOPS_ABI_VERSION")
    assert syms == ["frameops_abi_version", "frameops_last_error", "frameops_resize_normalize_u8"]


def test_argument_errors_are_reported_without_a_device(frame_lib):
    lib = frame_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch

    def call(src=p, row_pitch=3 * 64, frame_pitch=3 * 64 * 48, B=1, h=48, w=64, s0x=p, s1x=p, a1x=p, s0y=p, s1y=p,
             b1y=p, th=60, tw=80, Hp=64, Wp=96, lut=p, swap=0, out=p):
        return lib.frameops_resize_normalize_u8(src, row_pitch, frame_pitch, B, h, w, s0x, s1x, a1x, s0y, s1y, b1y,
                                                th, tw, Hp, Wp, lut, swap, out, None)

    for name in ("src", "s0x", "s1x", "a1x", "s0y", "s1y", "b1y", "lut", "out"):
        assert call(**{name: None}) != 0, name
        assert b"null" in lib.frameops_last_error()
    for name in ("h", "w", "th", "tw", "Hp", "Wp"):
        for bad in (0, -3):
            assert call(**{name: bad}) != 0, name
            assert b"non-positive" in lib.frameops_last_error()
    assert call(B=-1) != 0 and b"negative" in lib.frameops_last_error()
    assert call(Hp=32) != 0 and b"padded size" in lib.frameops_last_error()          # Hp < th
    assert call(Wp=64) != 0 and b"padded size" in lib.frameops_last_error()          # Wp < tw
    assert call(Wp=98) != 0 and b"multiple of 4" in lib.frameops_last_error()
    assert call(out=ctypes.c_void_p(4100)) != 0 and b"aligned" in lib.frameops_last_error()
    assert call(row_pitch=3 * 64 - 1) != 0 and b"pitch" in lib.frameops_last_error()
    assert call(swap=2) != 0 and b"swap_rb" in lib.frameops_last_error()
    # an empty problem is fine, launches nothing and clears the error text
    assert call(B=0) == 0 and lib.frameops_last_error() == b""
    with pytest.raises(RuntimeError, match="null pointer"):
        frame_lib.check(call(src=None), "frameops_resize_normalize_u8")


# ---------------------------------------------------------------------------------------------- the tracker
def small_tracker(monkeypatch, seed=4):
    from memotr_amd.inference import SequenceTracker
    patch_operator(monkeypatch)
    torch.manual_seed(seed)
    model = build_small_memotr().eval()
    tracker = SequenceTracker(model, det_score_thresh=0.0, track_score_thresh=0.0, result_score_thresh=0.0,
                              miss_tolerance=5, use_dab=True, area_thresh=0, raw_size=(96, 160))
    tracker.tracker.det_score_thresh = 0.0
    return tracker


def same_result(a, b):
    assert a.ids.tolist() == b.ids.tolist() and len(a) > 0
    assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)


def test_step_raw_equals_step_on_the_preprocessed_frame(monkeypatch, hip_lib, clip_lib):
    frames = [noise(60, 90, seed=20 + i) for i in range(2)]
    th, tw = F.target_size(60, 90, 96, 160)
    assert (th, tw) == (96, 144)
    raw, ref = small_tracker(monkeypatch), small_tracker(monkeypatch)
    for i, f in enumerate(frames):
        src = f.numpy() if i else f                            # numpy and torch frames
        got = raw.step_raw(src, bgr=True)
        image = F.preprocess_frames(f, bgr=True, size=(th, tw)).tensors[0][:, :th, :tw]
        same_result(got, ref.step(image, 60, 90))


def test_track_equals_the_manual_loop(monkeypatch, hip_lib, clip_lib):
    frames = [noise(60, 90, seed=30 + i) for i in range(4)]
    a, b = small_tracker(monkeypatch), small_tracker(monkeypatch)
    got = list(a.track(iter(frames)))
    assert [i for i, _ in got] == [0, 1, 2, 3]
    for (_, res), f in zip(got, frames):
        same_result(res, b.step_raw(f))
    assert list(small_tracker(monkeypatch).track([])) == []
