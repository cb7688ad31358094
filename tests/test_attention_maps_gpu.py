"""Attention maps on the GPU: the heat and blend kernels of libmsda_hip.so against the host statements of
memotr_amd/attention_maps.py, bit for bit, and ``SequenceTracker.track_attention`` end to end on the small model."""
import numpy as np
import pytest
import torch

from fused_helpers import make_case

from memotr_amd import attention_maps as A

pytestmark = pytest.mark.gpu

U = np.uint64
NAN, INF = float("nan"), float("inf")


def bits(t):
    return t.cpu().numpy().view(U)


def random_layer(rng, Lq, M, L, P, spread=0.2):
    loc = (rng.random((Lq, M, L, P, 2), dtype=np.float32) * (1 + 2 * spread) - spread).astype(np.float32)
    attn = (rng.random((Lq, M, L, P), dtype=np.float32) * 0.1).astype(np.float32)
    return loc, attn


def crafted_layer(rng, Lq, M, L, P, hc, wc, r):
    """Locations in cell units (the tests pass sx = sy = 1): row 0 sits on edges and just around the admission bounds,
    row 1 has every point on one cell, the rest is random; weights include the rounding ties, negatives and NaN."""
    loc, attn = random_layer(rng, Lq, M, L, P)
    loc[..., 0] *= wc
    loc[..., 1] *= hc
    f = np.float32
    edge_x = [0.0, -0.0, 1.0, wc - 1.0, float(wc), np.nextafter(f(0), f(-1)), -1.0, -(r + 1.0),
              np.nextafter(f(-(r + 1)), f(-100)), np.nextafter(f(wc + r + 1), f(0)), wc + r + 1.0, 1e9, -1e9, NAN, INF,
              -INF, 31.0, 32.0, np.nextafter(f(32), f(0))]
    flat = loc[0].reshape(-1, 2)
    n = min(len(edge_x), flat.shape[0])
    flat[:n, 0] = edge_x[:n]
    flat[:n, 1] = np.linspace(0, hc, n, dtype=np.float32)
    m = min(n, flat.shape[0] - n)
    flat[n:n + m, 1] = [v * hc / wc if np.isfinite(v) and abs(v) < 1e6 else v for v in edge_x[:m]]   # the same in y
    flat[n:n + m, 0] = np.linspace(0, wc, m, dtype=np.float32)
    loc[0] = flat.reshape(loc[0].shape)
    loc[1, ..., 0], loc[1, ..., 1] = 7.25, 5.75                     # all M * L * P points of row 1 on one cell
    w = attn[0].reshape(-1)
    special = [0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.3, NAN, 1.7, 0.0, 1.0, INF, 3.5 / 4096]
    w[:min(len(special), w.shape[0])] = special[:w.shape[0]]
    attn[0] = w.reshape(attn[0].shape)
    attn[1] = 1.0
    return loc, attn


def dev(pair):
    return tuple(torch.from_numpy(a).cuda() for a in pair)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("Lq,M,L,P", [(70, 8, 4, 4), (5, 3, 2, 3)])
def test_heat_points_entry_equals_the_host(hip_lib, Lq, M, L, P, r):
    hc, wc, n_planes = 37, 53, 3
    rng = np.random.default_rng(Lq * 10 + r)
    layer = crafted_layer(rng, Lq, M, L, P, hc, wc, r)
    # -1, a row >= Lq, a plane out of range (both ways), the same row twice into one plane, one row into two planes
    rows = [0, -1, Lq, 1, 1, 0, 3, 2, 4]
    planes = [0, 1, 1, 2, 2, 1, 3, -1, 0]
    stamp = A.tent_stamp(r)
    want, want_peak = A.attention_heat_host([layer], rows, planes, n_planes, hc, wc, 1.0, 1.0, stamp)
    assert want.any() and want_peak[2] >= U(2 * M * L * P * 4096) * U(stamp.max())
    heat = torch.full((n_planes, hc, wc), -7, dtype=torch.int64, device="cuda")         # garbage: overwritten
    peak = torch.full((n_planes,), -7, dtype=torch.int64, device="cuda")
    got = A.attention_heat([dev(layer)], i32(rows), i32(planes), n_planes, hc, wc, 1.0, 1.0, stamp, heat=heat, peak=peak)
    assert got[0] is heat and got[1] is peak
    assert np.array_equal(bits(heat), want) and np.array_equal(bits(peak), want_peak)
    # the same launch again: the same bits (LDS is zeroed by every workgroup)
    heat2, peak2 = A.attention_heat([dev(layer)], i32(rows), i32(planes), n_planes, hc, wc, 1.0, 1.0, stamp)
    assert torch.equal(heat2, heat) and torch.equal(peak2, peak)
    # a second, accumulating call on the first call's heat, with another scale
    layer_b = random_layer(rng, Lq, M, L, P)
    sx, sy = np.float32(wc * 0.97), np.float32(hc * 1.03)
    want2, want_peak2 = A.attention_heat_host([layer_b], rows, planes, n_planes, hc, wc, sx, sy, stamp, heat=want.copy())
    A.attention_heat([dev(layer_b)], i32(rows), i32(planes), n_planes, hc, wc, sx, sy, stamp, heat=heat, peak=peak,
                     accumulate=True)
    assert np.array_equal(bits(heat), want2) and np.array_equal(bits(peak), want_peak2)
    assert not np.array_equal(want2, want)
    # no rows at all: zeros
    empty = A.attention_heat([dev(layer)], i32([]), i32([]), n_planes, hc, wc, 1.0, 1.0, stamp, heat=heat, peak=peak)
    assert not bits(empty[0]).any() and not bits(empty[1]).any()


@pytest.mark.parametrize("n_planes", [16, 1])
def test_heat_at_1080p_cells_six_layers_in_one_launch(hip_lib, n_planes):
    """270 x 480 cells (1080p / 4), 64 rows over 16 planes or one, six layers with their own query counts: every boundary
    of the 32 x 32-cell tiling is crossed (480 = 15 tiles, 270 = 8 tiles and 14 cells).  Six accumulating single-layer
    launches give the same bits as the one launch.  (The library sizes its workgroups by the rows a plane has: 512
    threads for the sixteen planes, 1024 for the one, 256 in the single-layer launches of the sixteen and in the small
    tests above.)"""
    hc, wc, r = 270, 480, 2
    rng = np.random.default_rng(11)
    lqs = [50, 50, 70, 70, 70, 70]
    layers = [random_layer(rng, lq, 8, 4, 4, spread=0.02) for lq in lqs]
    for loc, _ in layers:                      # a few points exactly on tile boundaries
        loc[0, 0, 0, :, 0] = np.array([32, 64, 448, 479.5], dtype=np.float32) / wc
        loc[0, 0, 1, :, 1] = np.array([32, 256, 269.5, 31.999], dtype=np.float32) / hc
    rows = rng.integers(0, 70, 64).astype(np.int32)
    rows[:4] = [0, 0, 69, 49]
    planes = rng.integers(0, n_planes, 64).astype(np.int32)
    stamp = A.tent_stamp(r)
    sx, sy = np.float32(wc), np.float32(hc)
    want, want_peak = A.attention_heat_host(layers, rows, planes, n_planes, hc, wc, sx, sy, stamp)
    dl = [dev(p) for p in layers]
    heat, peak = A.attention_heat(dl, i32(rows), i32(planes), n_planes, hc, wc, sx, sy, stamp)
    assert np.array_equal(bits(heat), want) and np.array_equal(bits(peak), want_peak)
    step = torch.full_like(heat, 5)
    step_peak = torch.empty_like(peak)
    for i, pair in enumerate(dl):
        A.attention_heat([pair], i32(rows), i32(planes), n_planes, hc, wc, sx, sy, stamp, heat=step, peak=step_peak,
                         accumulate=i > 0)
    assert torch.equal(step, heat) and torch.equal(step_peak, peak)


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("M,L,P,shapes", [(8, 4, 4, [(16, 24), (8, 12), (4, 6), (2, 3)]), (3, 2, 3, [(9, 7), (4, 5)])])
def test_heat_fused_entry_equals_the_points_entry_on_fused_points(hip_lib, ref_dim, M, L, P, shapes):
    from memotr_amd import MultiScaleDeformableAttention as MSDA
    hc, wc, n_planes, r = 37, 53, 3, 2
    cases = [make_case(20 + i + ref_dim, 1, M, 32, L, P, shapes, Lq=lq, ref_dim=ref_dim, with_mask=False)
             for i, lq in enumerate((70, 41))]
    shapes_dev = cases[0]["shapes"].cuda()
    fused, points = [], []
    for c in cases:
        proj, ref = c["proj"].cuda(), c["ref"].cuda()
        loc, attn = MSDA.fused_points(shapes_dev, proj, ref, M, P)
        fused.append((proj[0], ref[0]))
        points.append((loc[0].contiguous(), attn[0].contiguous()))
    rng = np.random.default_rng(5)
    rows = i32(rng.integers(-1, 72, 24))
    planes = i32(rng.integers(-1, n_planes + 1, 24))
    stamp = A.tent_stamp(r)
    sx, sy = np.float32(wc), np.float32(hc)
    want = A.attention_heat(points, rows, planes, n_planes, hc, wc, sx, sy, stamp)
    got = A.attention_heat_fused(shapes_dev, fused, M, P, rows, planes, n_planes, hc, wc, sx, sy, stamp)
    assert bits(want[0]).any()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # ... and the points entry equals the host statement on those points
    host = A.attention_heat_host([(a.cpu().numpy(), b.cpu().numpy()) for a, b in points], rows.cpu().numpy(),
                                 planes.cpu().numpy(), n_planes, hc, wc, sx, sy, stamp)
    assert np.array_equal(bits(got[0]), host[0]) and np.array_equal(bits(got[1]), host[1])
    again = A.attention_heat_fused(shapes_dev, fused, M, P, rows, planes, n_planes, hc, wc, sx, sy, stamp)
    assert torch.equal(again[0], got[0])


def blend_case(rng, H, W, cell, n_planes):
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    hc, wc = -(-H // cell), -(-W // cell)
    heat = rng.integers(0, 5000, (n_planes, hc, wc)).astype(U)
    heat[rng.random(heat.shape) < 0.5] = 0
    if n_planes > 1:
        heat[1] = 0                                # a plane with peak 0
    heat[0, 0, 0] = 10 ** 15                       # 64-bit values; the other cells of plane 0 land on low levels
    heat[0, -1, -1] = 10 ** 15 // 2
    peak = heat.reshape(n_planes, -1).max(1)
    lut = rng.integers(0, 256, (n_planes, 256, 3), dtype=np.uint8)
    return frame, heat, peak, lut


def pitched(frame, pad):
    H, W, _ = frame.shape
    buf = torch.full((H, 3 * W + pad), 0xAB, dtype=torch.uint8, device="cuda")
    view = buf[:, :3 * W].unflatten(1, (W, 3))
    view.copy_(torch.from_numpy(frame).cuda())
    return buf, view


def test_blend_small_frame_every_option(hip_lib):
    rng = np.random.default_rng(21)
    H, W = 67, 131
    n = 0
    for cell in (1, 3, 4):
        for n_planes in (1, 5):
            frame, heat, peak, lut = blend_case(rng, H, W, cell, n_planes)
            th, tp = torch.from_numpy(heat.view(np.int64)).cuda(), torch.from_numpy(peak.view(np.int64)).cuda()
            for max_alpha in (0, 160, 255):
                for full_scale in (0, 3000):
                    want = A.blend_heat_host(frame, heat, peak, lut, cell, max_alpha, full_scale)
                    opts = dict(cell=cell, max_alpha=max_alpha, full_scale=full_scale)
                    src = torch.from_numpy(frame).cuda()
                    out = A.blend_heat(src, th, tp, lut, **opts)                         # out of place, pitch 3 * W
                    assert np.array_equal(out.cpu().numpy(), want), (cell, n_planes, max_alpha, full_scale)
                    assert np.array_equal(src.cpu().numpy(), frame)
                    buf, view = pitched(frame, 5)                                        # in place, padded pitch
                    assert A.blend_heat(view, th, tp, lut, out=view, **opts) is view
                    assert np.array_equal(view.cpu().numpy(), want)
                    assert bool((buf[:, 3 * W:] == 0xAB).all())
                    obuf = torch.full((H, 3 * W + 7), 0xCD, dtype=torch.uint8, device="cuda")   # padded out of place
                    oview = obuf[:, :3 * W].unflatten(1, (W, 3))
                    A.blend_heat(src, th, tp, lut, out=oview, **opts)
                    assert np.array_equal(oview.cpu().numpy(), want) and bool((obuf[:, 3 * W:] == 0xCD).all())
                    assert np.array_equal(want, frame) == (max_alpha == 0)
                    n += 1
    assert n == 36
    flipped = A.blend_heat(torch.from_numpy(frame).cuda(), th, tp, lut, bgr=True, **opts)
    assert np.array_equal(flipped.cpu().numpy(), A.blend_heat_host(frame, heat, peak, lut[..., ::-1], 4, 255, 3000))


def test_blend_1080p_padded_pitch(hip_lib):
    rng = np.random.default_rng(22)
    H, W, cell, n_planes = 1080, 1920, 4, 5
    frame, heat, peak, lut = blend_case(rng, H, W, cell, n_planes)
    th, tp = torch.from_numpy(heat.view(np.int64)).cuda(), torch.from_numpy(peak.view(np.int64)).cuda()
    want = A.blend_heat_host(frame, heat, peak, lut, cell, 160)
    buf, view = pitched(frame, 64)
    out = A.blend_heat(view, th, tp, lut, cell=cell, max_alpha=160)
    assert np.array_equal(out.cpu().numpy(), want)
    again = A.blend_heat(view, th, tp, lut, cell=cell, max_alpha=160)
    assert torch.equal(again, out)
    A.blend_heat(view, th, tp, lut, cell=cell, max_alpha=160, out=view)
    assert np.array_equal(view.cpu().numpy(), want) and bool((buf[:, 3 * W:] == 0xAB).all())


def test_wrappers_reject_what_the_kernels_cannot_take(hip_lib):
    layer = dev(random_layer(np.random.default_rng(0), 4, 2, 2, 2))
    stamp = A.tent_stamp(1)
    with pytest.raises(ValueError, match="int32"):
        A.attention_heat([layer], torch.zeros(1, dtype=torch.int64, device="cuda"), i32([0]), 1, 4, 4, 1.0, 1.0, stamp)
    with pytest.raises(ValueError, match="stamp"):
        A.attention_heat([layer], i32([0]), i32([0]), 1, 4, 4, 1.0, 1.0, np.ones((19, 19), np.uint16))
    with pytest.raises(ValueError, match="accumulate"):
        A.attention_heat([layer], i32([0]), i32([0]), 1, 4, 4, 1.0, 1.0, stamp, accumulate=True)
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    heat, peak = torch.zeros((17, 2, 2), dtype=torch.int64, device="cuda"), torch.zeros(17, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="planes"):
        A.blend_heat(frame, heat, peak)
    with pytest.raises(ValueError, match="heat is int64"):
        A.blend_heat(frame, heat[:1, :1], peak[:1])


def test_the_map_of_a_frame_reads_nothing_from_the_device(hip_lib):
    """What ``track_attention`` adds to a frame -- the row table, the heat launch (both entries), the blend -- under
    ``torch.cuda.set_sync_debug_mode("error")``, after one call has uploaded the stamp and the colour table."""
    from memotr_amd import MultiScaleDeformableAttention as MSDA
    c = make_case(3, 1, 8, 32, 4, 4, [(16, 24), (8, 12), (4, 6), (2, 3)], Lq=30, ref_dim=4, with_mask=False)
    shapes, proj, ref = c["shapes"].cuda(), c["proj"].cuda(), c["ref"].cuda()
    loc, attn = MSDA.fused_points(shapes, proj, ref, 8, 4)
    points, fused = [(loc[0].contiguous(), attn[0].contiguous())], [(proj[0], ref[0])]
    ids_before = torch.tensor([5, -1, 2, 7], device="cuda")
    newborn = torch.tensor([3, 11], device="cuda")
    want = torch.tensor([2, 9, 5], device="cuda")
    frame = torch.zeros((64, 96, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(frame)
    stamp, lut = A.tent_stamp(2), A.constant_lut([(255, 0, 0), (0, 255, 0), (0, 0, 255)])
    heat = peak = None
    for mode in ("default", "error"):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode(mode)
        try:
            for sel in (None, want):
                n_planes = 1 if sel is None else 3
                rows, planes = A.frame_rows(ids_before, newborn, 8, 20, sel)
                heat, peak = A.attention_heat_fused(shapes, fused, 8, 4, rows, planes, n_planes, 16, 24, 24.0, 16.0, stamp)
                A.attention_heat(points, rows, planes, n_planes, 16, 24, 24.0, 16.0, stamp, heat=heat, peak=peak,
                                 accumulate=True)
                A.blend_heat(frame, heat, peak, None if sel is None else lut, cell=4, out=out)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert rows.tolist() == [20, 21, 22, 23, 3, 11] and planes.tolist() == [2, -1, 0, -1, -1, 1]
    assert int(peak.max()) > 0 and bool(out.any())


# --------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("ids", [None, [0, 1]])
def test_track_attention_end_to_end(hip_lib, clip_lib, tmp_path, monkeypatch, ids):
    from test_frames_gpu import build_memotr_cuda
    from memotr_amd import render as R
    from memotr_amd.build import build_frame_lib, build_jpeg_enc_lib, build_jpeg_lib, build_track_draw_lib
    from memotr_amd.data import jpeg_write as JW
    from memotr_amd.data.frames import padded_size, target_size
    from memotr_amd.inference import SequenceTracker
    import memotr_amd.modules.ms_deform_attn as mod
    build_frame_lib(), build_jpeg_enc_lib(), build_jpeg_lib(), build_track_draw_lib()
    frames = [torch.from_numpy(np.random.default_rng(70 + i).integers(0, 256, (64, 96, 3), dtype=np.uint8))
              for i in range(3)]
    raw_size = (128, 192)

    def tracker():
        torch.manual_seed(4)
        model = build_memotr_cuda().eval()
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, mod.MSDeformAttn):
                    m.sampling_offsets.weight.normal_(0, 0.02)
                    m.attention_weights.weight.normal_(0, 0.05)
        return SequenceTracker(model, det_score_thresh=0.0, track_score_thresh=0.0, result_score_thresh=0.0,
                               miss_tolerance=5, use_dab=True, area_thresh=0, raw_size=raw_size)

    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "0")
    want = [r for _, r in tracker().track(frames)]
    assert len(want[-1]) >= 2
    monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "1")

    st = tracker()
    decoder = st.core.transformer.decoder
    n_det = st.core.n_det_queries
    cell, radius, max_alpha = 4, 2, 160
    records = []
    with A.AttentionWriter(tmp_path, quality=85, cell=cell, radius=radius, max_alpha=max_alpha) as writer:
        run = st.track_attention(frames, writer, ids=ids)
        while True:
            ids_before = st.tracks[0].ids.cpu()
            item = next(run, None)
            if item is None:
                break
            tap = st.attention_tap
            assert decoder.__dict__["_attention_tap"] is tap
            points = [tuple(x.cpu().numpy() for x in tap.points(lid)) for lid in tap.layers]
            records.append((item, ids_before, st.tracker.last_newborn_rows.cpu(), st.tracker.last_newborn_first_id, points))
    assert st.attention_tap is None and "_attention_tap" not in decoder.__dict__
    assert decoder.infer_graphs().decode.replays == 0            # under the tap the decoder loop ran eagerly
    assert len(records) == 3 and records[2][1].numel() > 0        # the later frames carry tracks

    th, tw = target_size(64, 96, *raw_size)
    Hp, Wp = padded_size(th, tw)
    sx, sy = A.heat_scale(Wp, 96, tw, cell), A.heat_scale(Hp, 64, th, cell)
    n_planes = 1 if ids is None else len(ids)
    lut = np.repeat(A.HEAT_LUT[None], 1, 0) if ids is None else A.constant_lut([R.palette_entry(i) for i in ids])
    some_heat = False
    for (idx, result), ids_before, newborn, first_id, points in records:
        b = want[idx]
        assert result.ids.tolist() == b.ids.tolist()
        assert torch.equal(result.boxes, b.boxes) and torch.equal(result.scores, b.scores)
        rows, planes = A.frame_rows(ids_before, newborn, first_id, n_det, ids)
        assert [p[0].shape[0] for p in points] == [n_det, n_det + ids_before.numel()]
        heat, peak = A.attention_heat_host(points, rows.numpy(), planes.numpy(), n_planes, 16, 24, sx, sy,
                                           A.tent_stamp(radius))
        some_heat = some_heat or bool(heat.any())
        blended = A.blend_heat_host(frames[idx], heat, peak, lut, cell, max_alpha)
        expect = JW.encode_jpeg(R.draw_tracks_host(blended, result), quality=85)
        assert (tmp_path / f"{idx:08d}.jpg").read_bytes() == expect, idx
    assert some_heat
    # after leaving the tap the decoder replays its graphs again
    before = decoder.infer_graphs().decode.replays
    more = list(st.track(frames[:2]))
    assert len(more) == 2 and decoder.infer_graphs().decode.replays > before
