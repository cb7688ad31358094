"""Attention maps without a device: the two host statements against hand-computed cases, the decoder tap on the CPU
small model (against the module's prologue and the reference's VISUALIZE dumps), the C ABI of the new entry points, and
the runtime tracker's newborn fields."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from conftest import GOLDEN_DIR, load_npz
from fused_helpers import prologue_cpu
from model_helpers import build_small_memotr, load_model_golden, patch_operator, state_from, t

from memotr_amd import attention_maps as A

U = np.uint64


# --------------------------------------------------------------------------------------- host statements
def test_heat_host_hand_computed_points():
    """Heat 5 x 7, r = 1, three points of one query row: one at the corner (stamp clipped), one at x = -0.25 (floors to
    -1, its stamp still reaches column 0), one NaN (dropped)."""
    nan = float("nan")
    loc = np.array([[0.5, 0.5], [-0.25, 2.5], [nan, 1.0]], dtype=np.float32).reshape(1, 1, 1, 3, 2)
    attn = np.array([1.0, 0.5, 1.0], dtype=np.float32).reshape(1, 1, 1, 3)
    heat, peak = A.attention_heat_host([(loc, attn)], np.array([0], np.int32), np.array([0], np.int32), 1, 5, 7,
                                       1.0, 1.0, A.tent_stamp(1))
    want = np.zeros((1, 5, 7), dtype=U)
    want[0, 0, 0], want[0, 0, 1], want[0, 1, 0], want[0, 1, 1] = 4 * 4096, 2 * 4096, 2 * 4096, 1 * 4096
    want[0, 1, 0] += 1 * 2048         # the second point: centre (iy 2, ix -1), its right column lands on column 0
    want[0, 2, 0] += 2 * 2048
    want[0, 3, 0] += 1 * 2048
    assert heat.dtype == U and peak.dtype == U
    assert np.array_equal(heat, want)
    assert peak.tolist() == [4 * 4096]
    # a given heat is summed on top of, in place; rows / planes out of range are skipped
    again, peak2 = A.attention_heat_host([(loc, attn)], np.array([0, -1, 1, 0], np.int32), np.array([0, 0, 0, 1], np.int32),
                                         1, 5, 7, 1.0, 1.0, A.tent_stamp(1), heat=heat)
    assert again is heat and np.array_equal(heat, want * U(2)) and peak2.tolist() == [8 * 4096]


def test_heat_host_range_edges():
    """x = wc + r + 1 is out, just below is in (its stamp misses the plane); x = -(r+1) is in, +-inf are out."""
    r, hc, wc = 1, 3, 4
    inf = float("inf")
    xs = np.array([wc + r + 1, np.nextafter(np.float32(wc + r + 1), np.float32(0)), -(r + 1), wc + 0.5, inf, -inf],
                  dtype=np.float32)
    loc = np.stack([xs, np.full_like(xs, 1.5)], -1).reshape(1, 1, 1, -1, 2)
    attn = np.ones((1, 1, 1, xs.shape[0]), dtype=np.float32)
    heat, _ = A.attention_heat_host([(loc, attn)], [0], [0], 1, hc, wc, 1.0, 1.0, A.tent_stamp(r))
    want = np.zeros((1, hc, wc), dtype=U)
    want[0, :, wc - 1] = np.array([1, 2, 1], dtype=U) * U(4096)      # only x = wc + 0.5 (ix = wc) reaches the plane
    assert np.array_equal(heat, want)


def test_weight_rounding():
    f = np.float32
    a = np.array([0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.3, float("nan"), 1.7, 0.0, 1.0, float("inf")], dtype=f)
    assert A.heat_weights_host(a).tolist() == [0, 2, 2, 0, 0, 4096, 0, 4096, 4096]


def test_stamp_and_lut():
    assert A.tent_stamp(0).tolist() == [[1]]
    assert A.tent_stamp(2)[2].tolist() == [3, 6, 9, 6, 3] and A.tent_stamp(2).dtype == np.uint16
    with pytest.raises(ValueError):
        A.tent_stamp(9)
    lut = A.HEAT_LUT
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [0, 0, 0] and lut[85].tolist() == [255, 0, 0] and lut[100].tolist() == [255, 45, 0]
    assert lut[170].tolist() == [255, 255, 0] and lut[255].tolist() == [255, 255, 255]


def _blend_scalar(frame, heat, peak, lut, cell, max_alpha, full_scale):
    """The definition pixel by pixel, in Python integers."""
    out = frame.copy()
    H, W, _ = frame.shape
    for y in range(H):
        for x in range(W):
            for p in range(heat.shape[0]):
                s = int(full_scale) or int(peak[p])
                level = 0 if s == 0 else min(255, (int(heat[p, y // cell, x // cell]) * 255 + s // 2) // s)
                a = (level * max_alpha + 127) // 255
                if a > 0:
                    for c in range(3):
                        out[y, x, c] = (int(lut[p, level, c]) * a + int(out[y, x, c]) * (255 - a) + 127) // 255
    return out


def test_blend_levels_at_the_rounding_boundary():
    """s = 10: heat * 255 + 5 crosses a multiple of 10 between heat 1 (260 -> 26) and the values around it; peak 0 and
    max_alpha 0 leave the frame alone; max_alpha 255 at level 255 replaces the pixel."""
    frame = np.full((1, 4, 3), 100, dtype=np.uint8)
    heat = np.array([[[0, 1, 5, 10]]], dtype=U)
    lut = np.repeat(A.HEAT_LUT[None], 1, 0)
    out = A.blend_heat_host(frame, heat, np.array([10], U), lut, 1, 255)
    levels = [(h * 255 + 5) // 10 for h in (0, 1, 5, 10)]
    assert levels == [0, 26, 128, 255]
    for x, lv in enumerate(levels):
        want = [(int(lut[0, lv, c]) * lv + 100 * (255 - lv) + 127) // 255 for c in range(3)] if lv else [100] * 3
        assert out[0, x].tolist() == want
    assert out[0, 3].tolist() == [255, 255, 255]
    assert np.array_equal(A.blend_heat_host(frame, heat, np.array([0], U), lut, 1, 255), frame)
    assert np.array_equal(A.blend_heat_host(frame, heat, np.array([10], U), lut, 1, 0), frame)
    # full_scale overrides the peak and saturates at 255
    sat = A.blend_heat_host(frame, heat, np.array([10], U), lut, 1, 255, full_scale=5)
    assert sat[0, 2].tolist() == [255, 255, 255] and sat[0, 3].tolist() == [255, 255, 255]


@pytest.mark.parametrize("cell,max_alpha,full_scale", [(3, 160, 0), (3, 255, 700), (1, 160, 0), (4, 0, 0)])
def test_blend_host_equals_the_scalar_definition(cell, max_alpha, full_scale):
    rng = np.random.default_rng(cell * 1000 + max_alpha)
    H, W, n = 8, 10, 3                       # H is no multiple of 3
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    heat = rng.integers(0, 1000, (n, -(-H // cell), -(-W // cell))).astype(U)
    heat[1] = 0                              # a plane with peak 0
    peak = heat.reshape(n, -1).max(1)
    lut = rng.integers(0, 256, (n, 256, 3), dtype=np.uint8)
    want = _blend_scalar(frame, heat, peak, lut, cell, max_alpha, full_scale)
    got = A.blend_heat_host(frame, heat, peak, lut, cell, max_alpha, full_scale)
    assert np.array_equal(got, want)
    inplace = frame.copy()
    assert A.blend_heat_host(inplace, heat, peak, lut, cell, max_alpha, full_scale, out=inplace) is inplace
    assert np.array_equal(inplace, want)
    # the torch wrapper on CPU tensors: int64 bits in, the same bytes out; bgr flips the table
    tf = torch.from_numpy(frame)
    th, tp = torch.from_numpy(heat.view(np.int64)), torch.from_numpy(peak.view(np.int64))
    assert np.array_equal(A.blend_heat(tf, th, tp, lut, cell=cell, max_alpha=max_alpha, full_scale=full_scale).numpy(),
                          want)
    flipped = A.blend_heat(tf, th, tp, lut, cell=cell, max_alpha=max_alpha, full_scale=full_scale, bgr=True).numpy()
    assert np.array_equal(flipped, _blend_scalar(frame, heat, peak, lut[..., ::-1], cell, max_alpha, full_scale))


def test_heat_wrapper_on_cpu_tensors():
    rng = np.random.default_rng(3)
    loc = torch.from_numpy(rng.random((5, 3, 2, 3, 2), dtype=np.float32))
    attn = torch.from_numpy(rng.random((5, 3, 2, 3), dtype=np.float32) * 0.2)
    rows = torch.tensor([0, 4, -1, 7, 2], dtype=torch.int32)
    planes = torch.tensor([0, 1, 0, 1, 2], dtype=torch.int32)
    sx, sy, stamp = 9.0, 6.0, A.tent_stamp(2)
    want, want_peak = A.attention_heat_host([(loc.numpy(), attn.numpy())], rows.numpy(), planes.numpy(), 2, 6, 9, sx, sy,
                                            stamp)
    heat, peak = A.attention_heat([(loc, attn)], rows, planes, 2, 6, 9, sx, sy, stamp)
    assert heat.dtype == torch.int64 and np.array_equal(heat.numpy().view(U), want)
    assert np.array_equal(peak.numpy().view(U), want_peak)
    # reused buffers: overwritten, or added to
    A.attention_heat([(loc, attn)], rows, planes, 2, 6, 9, sx, sy, stamp, heat=heat, peak=peak)
    assert np.array_equal(heat.numpy().view(U), want)
    A.attention_heat([(loc, attn)], rows, planes, 2, 6, 9, sx, sy, stamp, heat=heat, peak=peak, accumulate=True)
    assert np.array_equal(heat.numpy().view(U), want * U(2)) and np.array_equal(peak.numpy().view(U), want_peak * U(2))


def test_frame_rows():
    ids_before = torch.tensor([4, -1, 9])
    newborn = torch.tensor([2, 17])
    rows, planes = A.frame_rows(ids_before, newborn, 11, 20)
    assert rows.dtype == torch.int32 and rows.tolist() == [20, 21, 22, 2, 17] and planes.tolist() == [0, -1, 0, 0, 0]
    rows, planes = A.frame_rows(ids_before, newborn, 11, 20, [12, 4, 5])
    assert rows.tolist() == [20, 21, 22, 2, 17] and planes.tolist() == [1, -1, -1, -1, 0]
    assert float(A.heat_scale(1344, 1920, 1333, 4)) == float(np.float32(1344 * 1920 / 1333 / 4))


# --------------------------------------------------------------------------------------- the tap
def _m5_model():
    g = load_model_golden("M5_memotr_two_frames")
    model = build_small_memotr()
    model.load_state_dict(state_from(g), strict=True)
    return model.eval(), g


def _two_frames(model, g, tap_factory=None, on_frame=None):
    """The reference's two-frame loop (gen_golden_model.py: case_memotr_two_frames); per frame the model outputs."""
    from memotr_amd.models.runtime_tracker import RuntimeTracker
    from memotr_amd.structures.track_instances import TrackInstances
    from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor
    thresh = float(g["score_thresh"])
    tracker = RuntimeTracker(det_score_thresh=thresh, track_score_thresh=thresh, miss_tolerance=30, use_dab=True)
    tracks = [TrackInstances(hidden_dim=64, num_classes=1, use_dab=True)]
    outs = []
    with torch.no_grad():
        for i in range(2):
            ids_before = tracks[0].ids
            res = model(frame=tensor_list_to_nested_tensor([t(g[f"frame{i}"])]), tracks=tracks)
            outs.append({k: res[k].clone() for k in ("pred_logits", "pred_bboxes", "outputs", "last_ref_pts")})
            prev, new = tracker.update(model_outputs=res, tracks=tracks)
            if on_frame is not None:
                on_frame(i, tracker, ids_before, new[0])
            tracks = model.postprocess_single_frame(prev, new, None)
    return outs, tracks


def test_tap_records_every_layer_and_changes_nothing(monkeypatch, tmp_path):
    patch_operator(monkeypatch)
    model, g = _m5_model()
    plain, _ = _two_frames(model, g)
    decoder = model.transformer.decoder
    n_det, merge = 20, decoder.merge_det_track_layer
    assert merge == 1 and len(decoder.layers) == 2
    seen = []

    with torch.no_grad(), A.AttentionTap(model) as tap:
        assert decoder.__dict__["_attention_tap"] is tap

        def on_frame(i, tracker, ids_before, new):
            n_tr = int(ids_before.shape[0])
            seen.append(n_tr)
            assert tap.layers == [0, 1]
            shapes = tap.spatial_shapes
            for lid in (0, 1):
                Lq = n_det if lid < merge else n_det + n_tr
                proj, cross, ref = tap.projection(lid), tap.cross_reference(lid), tap.reference(lid)
                assert tuple(proj.shape) == (1, Lq, 3 * 8 * 4 * 4)
                assert tuple(cross.shape) == (1, Lq, 4, 4) and tuple(ref.shape) == (1, n_det + n_tr, 4)
                loc, attn = tap.points(lid)
                assert tuple(loc.shape) == (Lq, 8, 4, 4, 2) and tuple(attn.shape) == (Lq, 8, 4, 4)
                want_loc, want_attn = prologue_cpu(proj, cross, shapes, 8, 4, 4)
                assert torch.equal(loc, want_loc[0]) and torch.equal(attn, want_attn[0])
            if i == 1:
                files = tap.dump(tmp_path / "f1")
                assert len(files) == 8 and all(os.path.exists(f) for f in files)
                assert not any("attn_score" in f for f in files)
                assert torch.equal(torch.load(tmp_path / "f1" / "attention_weights_layer_1.tensor"), tap.points(1)[1])

        tapped, _ = _two_frames(model, g, on_frame=on_frame)
    assert seen[0] == 0 and seen[1] > 0                          # the second frame carries tracks
    assert "_attention_tap" not in decoder.__dict__
    assert not decoder.layers[0].cross_attn._forward_pre_hooks
    for a, b in zip(plain, tapped):
        for k in a:
            assert torch.equal(a[k], b[k]), k                    # on the CPU both runs are eager: the same bits


def test_tap_is_for_inference_only():
    model = build_small_memotr().eval()
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference"):
            A.AttentionTap(model).__enter__()
    assert "_attention_tap" not in model.transformer.decoder.__dict__
    with torch.no_grad(), A.AttentionTap(model):
        with pytest.raises(RuntimeError, match="already"):
            A.AttentionTap(model).__enter__()


def test_tap_dump_matches_the_reference_visualize_dumps(monkeypatch, tmp_path):
    """tests/golden/gen_golden_attention.py: the reference's small DAB model with visualize=True on fixture M5's weights
    and frames.  Tolerance: the one model_helpers.assert_tracks_close holds model outputs to."""
    patch_operator(monkeypatch)
    model, g = _m5_model()
    want = load_npz(os.path.join(GOLDEN_DIR, "attention_tap.npz"))
    compared = []

    with torch.no_grad(), A.AttentionTap(model) as tap:
        def on_frame(i, tracker, ids_before, new):
            d = tmp_path / f"frame_{i}"
            tap.dump(d)
            for lid in (0, 1):
                for name in ("sampling_locations", "detection_ref_pts", "track_ref_pts"):
                    got = torch.load(d / f"{name}_layer_{lid}.tensor").numpy()
                    ref = want[f"f{i}_{name}_layer_{lid}"]
                    assert got.shape == ref.shape and got.dtype == ref.dtype, (i, name, lid, got.shape, ref.shape)
                    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5, err_msg=f"f{i}_{name}_layer_{lid}")
                    compared.append(ref.size)
        _two_frames(model, g, on_frame=on_frame)
    assert len(compared) == 12 and want["f1_sampling_locations_layer_1"].shape[0] > 20


def test_runtime_tracker_keeps_the_newborn_rows(monkeypatch):
    patch_operator(monkeypatch)
    model, g = _m5_model()
    checked = []

    def on_frame(i, tracker, ids_before, new):
        idx, first = tracker.last_newborn_rows, tracker.last_newborn_first_id
        assert idx.dtype == torch.long and idx.dim() == 1 and idx.shape[0] == len(new)
        assert first + len(new) == tracker.max_obj_id
        assert new.ids.tolist() == list(range(first, first + len(new)))
        scores = t(g[f"f{i}_pred_logits"]).sigmoid()[0, :20].max(-1).values
        assert idx.tolist() == (scores >= float(g["score_thresh"])).nonzero().squeeze(1).tolist()
        checked.append(len(new))

    from model_helpers import assert_tracks_close
    _, tracks = _two_frames(model, g, on_frame=on_frame)
    assert len(checked) == 2 and checked[0] > 0
    assert_tracks_close(tracks[0], g, "f1_next_", atol=1e-4)        # the existing fields are what they were
    from memotr_amd.models.runtime_tracker import RuntimeTracker
    fresh = RuntimeTracker()
    assert fresh.last_newborn_rows is None and fresh.last_newborn_first_id == 0


# --------------------------------------------------------------------------------------- C ABI
NEW_SYMBOLS = ("msda_attention_heat_points_f32", "msda_attention_heat_f32", "msda_attention_blend_u8")


def test_new_symbols_in_header_library_and_binding(hip_lib):
    declared = assert_binding_matches_header(hip_lib, "msda_hip.h", "msda", "MSDA_ABI_VERSION")
    assert hip_lib.ABI_VERSION == 8
    for s in NEW_SYMBOLS:
        assert s in declared and s in hip_lib.SYMBOLS
    from memotr_amd import build
    assert any(p.endswith("msda_attn_map.h") for p in build.KERNEL_HEADERS)
    assert any(p.endswith("msda_attn_map.h") for p in build.sources("msda"))


def test_argument_errors_are_reported_without_a_device(hip_lib):
    lib = hip_lib.lib
    buf = ctypes.create_string_buffer(4096)          # host memory: every call below fails before it is touched
    ptr = ctypes.addressof(buf)
    layer = (hip_lib.HeatLayer * 9)()
    for d in layer:
        d.a, d.b, d.Lq, d.proj_stride, d.ref_dim = ptr, ptr, 4, 3 * 2 * 2 * 2, 2

    def heat(fused=False, layers=layer, n_layers=1, M=2, L=2, P=2, rows=ptr, planes=ptr, K=1, stamp=ptr, radius=1,
             out=ptr, peak=ptr, n_planes=1, hc=4, wc=4):
        args = (layers, n_layers, M, L, P, rows, planes, K, stamp, radius, 1.0, 1.0, out, peak, n_planes, hc, wc, 0, None)
        if fused:
            return lib.msda_attention_heat_f32(ptr if fused is True else None, *args)
        return lib.msda_attention_heat_points_f32(*args)

    for fused in (False, True):
        assert heat(fused, layers=None) == -1 and "null" in hip_lib.last_error()
        assert heat(fused, stamp=None) == -1 and heat(fused, out=None) == -1 and heat(fused, peak=None) == -1
        assert heat(fused, rows=None) == -1 and heat(fused, planes=None) == -1
        assert heat(fused, radius=9) == -1 and "radius" in hip_lib.last_error()
        assert heat(fused, radius=-1) == -1
        assert heat(fused, n_layers=9) == -1 and "layers" in hip_lib.last_error()
        assert heat(fused, n_layers=0) == -1
        assert heat(fused, n_planes=0) == -1 and heat(fused, hc=0) == -1 and heat(fused, M=0) == -1 and heat(fused, K=-1) == -1
    assert heat("no shapes") == -1 and "null" in hip_lib.last_error()
    bad = (hip_lib.HeatLayer * 1)()
    bad[0].a, bad[0].b, bad[0].Lq, bad[0].proj_stride, bad[0].ref_dim = ptr, None, 4, 24, 2
    assert heat(layers=bad) == -1
    bad[0].b, bad[0].ref_dim = ptr, 3
    assert heat(True, layers=bad) == -1 and "2 or 4" in hip_lib.last_error()
    bad[0].ref_dim, bad[0].proj_stride = 2, 23
    assert heat(True, layers=bad) == -1 and "3*M*L*P" in hip_lib.last_error()
    assert heat(True, L=9, P=8) == -3                                 # fused: L * P <= 64

    def blend(src=ptr, sp=30, dst=ptr, dp=30, W=10, H=4, heat=ptr, peak=ptr, lut=ptr, n_planes=1, cell=4, alpha=160):
        return lib.msda_attention_blend_u8(src, sp, dst, dp, W, H, heat, peak, lut, n_planes, cell, alpha, 0, None)

    assert blend(src=None) == -1 and "null" in hip_lib.last_error()
    assert blend(dst=None) == -1 and blend(heat=None) == -1 and blend(peak=None) == -1 and blend(lut=None) == -1
    assert blend(cell=0) == -1 and "cell" in hip_lib.last_error()
    assert blend(n_planes=17) == -1 and "planes" in hip_lib.last_error()
    assert blend(n_planes=0) == -1 and blend(alpha=256) == -1 and blend(W=0) == -1
    assert blend(sp=29) == -1 and "pitch" in hip_lib.last_error()


# --------------------------------------------------------------------------------------- tracker, writer, command line
def test_command_line_on_the_cpu_small_model(monkeypatch, tmp_path):
    """``python -m memotr_amd.attention_maps`` end to end without a device: JPEG frames in, one JPEG per frame and the
    tensor dumps out; every file equals the host statements on the tap's points (the CPU path IS the host statements;
    this holds the plumbing: row table, scales, writer, dumps)."""
    import memotr_amd.main as main_mod
    import memotr_amd.submit as submit_mod
    from memotr_amd import render as R
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib
    from memotr_amd.data import jpeg as J
    from memotr_amd.data import jpeg_write as JW
    from memotr_amd.data.frames import padded_size, target_size
    from memotr_amd.inference import SequenceTracker
    build_jpeg_enc_lib(), build_jpeg_lib()
    patch_operator(monkeypatch)
    model, g = _m5_model()
    thresh = float(g["score_thresh"])
    config = dict(DATASET="DanceTrack", DET_SCORE_THRESH=thresh, TRACK_SCORE_THRESH=thresh, RESULT_SCORE_THRESH=0.0,
                  MISS_TOLERANCE=30, USE_DAB=True)
    monkeypatch.setattr(main_mod, "load_config", lambda path: dict(config))
    monkeypatch.setattr(submit_mod, "load_model", lambda cfg, ckpt: model)
    raw_size = (96, 160)
    real_init = SequenceTracker.__init__
    monkeypatch.setattr(SequenceTracker, "__init__",
                        lambda self, *a, **k: real_init(self, *a, **dict(k, raw_size=raw_size, area_thresh=0)))
    frames_dir = tmp_path / "img1"
    frames_dir.mkdir()
    rng = np.random.default_rng(9)
    ramp = np.linspace(0, 200, 80)[None, :, None] + np.linspace(0, 40, 48)[:, None, None]
    for i in range(2):
        px = (ramp + rng.integers(0, 30, (48, 80, 3)) + 10 * i).astype(np.uint8)
        (frames_dir / f"{i + 1:08d}.jpg").write_bytes(JW.encode_jpeg(torch.from_numpy(px), quality=95))
    pixels = [J.decode_jpeg(str(frames_dir / f"{i + 1:08d}.jpg"), "cpu") for i in range(2)]

    # what the run must write, from a second tracker under a tap of its own
    st = SequenceTracker.from_config(model, config)
    n_det, cell, radius = 20, 4, 2
    th, tw = target_size(48, 80, *raw_size)
    Hp, Wp = padded_size(th, tw)
    sx, sy = A.heat_scale(Wp, 80, tw, cell), A.heat_scale(Hp, 48, th, cell)
    want, live = [], 0
    with torch.no_grad(), A.AttentionTap(model) as tap:
        for i in range(2):
            ids_before = st.tracks[0].ids
            result = st.step_raw(pixels[i], None)
            rows, planes = A.frame_rows(ids_before, st.tracker.last_newborn_rows, st.tracker.last_newborn_first_id, n_det,
                                        [0, 1])
            live += int((planes >= 0).sum())
            points = [tuple(x.numpy() for x in tap.points(1))]              # --layers 1
            heat, peak = A.attention_heat_host(points, rows.numpy(), planes.numpy(), 2, 12, 20, sx, sy,
                                               A.tent_stamp(radius))
            blended = A.blend_heat_host(pixels[i], heat, peak, A.constant_lut([R.palette_entry(0), R.palette_entry(1)]),
                                        cell, 160)
            want.append((JW.encode_jpeg(R.draw_tracks_host(blended, result), quality=85), bool(heat.any())))
    assert live >= 2 and any(hot for _, hot in want)

    out, dumps = tmp_path / "maps", tmp_path / "tensors"
    rc = A.main(["--config-path", "c.yaml", "--model", "m.pth", "--frames", str(frames_dir), "--out", str(out), "--ids",
                 "0,1", "--layers", "1", "--dump-tensors", str(dumps), "--device", "cpu"])
    assert rc == 0
    for i in range(2):
        assert (out / f"{i:08d}.jpg").read_bytes() == want[i][0], i
        assert sorted(os.listdir(dumps / f"frame_{i + 1}")) == sorted(
            f"{name}_layer_{lid}.tensor" for lid in (0, 1)
            for name in ("sampling_locations", "attention_weights", "detection_ref_pts", "track_ref_pts"))
    assert "_attention_tap" not in model.transformer.decoder.__dict__
    with pytest.raises(ValueError, match="layers"):
        list(SequenceTracker.from_config(model, config).track_attention(pixels, None, layers=[2]))
    with pytest.raises(ValueError, match="ids"):
        list(SequenceTracker.from_config(model, config).track_attention(pixels, None, ids=list(range(17))))
