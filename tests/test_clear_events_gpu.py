"""GPU: the two kernels of the error analysis (memotr_amd/csrc/clip_tracks.h) against their host statements
(memotr_amd/diagnose.py), bit for bit: ``clipops_clear_events_f64`` on the fixture's sequences in one call, with
sentinels in and guard words around every output, and next to ``trackeval_clear`` on the same arrays;
``clipops_error_table_f64`` on the hand-made sequence of tests/clear_events_cases.py; and the annotated frames of
``write_error_frames`` on the device against the host path, byte for byte."""
import os

import numpy as np
import pytest
import torch

import clear_events_cases as C

from memotr_amd import diagnose as D
from memotr_amd import evaluation as E

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0x5A5A5A5A


@pytest.fixture(scope="module")
def libs(clip_lib):
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib, build_track_draw_lib, build_track_eval_lib
    build_track_eval_lib(), build_jpeg_lib(), build_jpeg_enc_lib(), build_track_draw_lib()
    from memotr_amd import _track_eval_lib
    return clip_lib, _track_eval_lib


@pytest.fixture(scope="module")
def kernel_case():
    """The kernel's inputs (the preprocessed, compacted arrays) and the host statement of its outputs: computed once."""
    packed = C.kernel_set()
    _, sim, d = E._preprocess_host(packed, "MOT17")
    return packed, sim, d, D._walk_host(d, sim)


def guarded(n, shape=None):
    """A sentinel-filled int32 buffer with GUARD words on either side of ``n``; (whole, the part the kernel gets)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    inner = whole[GUARD:GUARD + n]
    return whole, inner if shape is None else inner.view(shape)


def guards_untouched(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def device_inputs(sim, d):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                             # noqa: E731
    frame_max = lambda off: int(np.diff(off).max())                                             # noqa: E731
    return ([up(sim), up(d["sim_off"]), up(d["gt_off"]), up(d["tr_off"]), up(d["gt_ids"]), up(d["tr_ids"]),
             up(d["seq_off"]), up(d["n_gt_ids"])],
            [frame_max(d["gt_off"]), frame_max(d["tr_off"]), int(d["n_gt_ids"].max())])


def test_the_events_kernel_equals_the_host_statement(libs, kernel_case):
    packed, sim, d, want = kernel_case
    S, n_gt, n_tr = len(packed.names), len(d["gt_ids"]), len(d["tr_ids"])
    # what the set is there for: an empty sequence between two with rows, a one-frame sequence, frames past one
    # wavefront on either side, frames and sequences with an empty side, and every kind of event with a frag flag
    frames = np.diff(packed.seq_off)
    assert packed.names[1] == "empty" and packed.gt_off[packed.seq_off[1]] == packed.gt_off[packed.seq_off[2]]
    assert frames[1] == 3 and d["n_gt_dets"][0] and d["n_gt_dets"][2] and 1 in frames
    g, k = np.diff(d["gt_off"]), np.diff(d["tr_off"])
    assert ((g == 7) & (k >= 65)).any() and ((g == 70) & (k == 9)).any()
    assert ((g == 0) & (k > 0)).any() and ((g > 0) & (k == 0)).any() and ((g == 0) & (k == 0)).any()
    assert (d["n_gt_dets"] == 0).any() and (d["n_tr_dets"] == 0).any()
    assert C.has_every_kind(D.clear_events_host(packed, "MOT17"))
    assert (want["gt_flags"] == 3).any() and (want["gt_flags"] == 1).any() and (want["gt_flags"] == 2).any()

    inputs, sizes = device_inputs(sim, d)
    outs = [guarded(n_gt), guarded(n_gt), guarded(n_tr), guarded(S * 5, (S, 5)), guarded(S)]
    D.launch_clear_events(*inputs, *sizes, *[inner for _, inner in outs])
    torch.cuda.synchronize()
    for (whole, inner), key in zip(outs[:4], ("gt_partner", "gt_flags", "tr_partner", "counts")):
        assert torch.equal(inner.cpu(), torch.from_numpy(want[key])), key
        assert not bool((inner == SENTINEL).any()) and guards_untouched(whole, inner.numel()), key
    assert torch.equal(outs[4][1].cpu(), torch.zeros(S, dtype=torch.int32)) and guards_untouched(outs[4][0], S)

    # trackeval_clear on the same arrays: the counts behind the fields of the evaluation
    _, L = libs
    ints = torch.zeros((S, 8), dtype=torch.int32, device="cuda")
    motp, status = torch.zeros(S, dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda")
    L.check(L.lib.trackeval_clear(*[t.data_ptr() for t in inputs[:7]], S, inputs[7].data_ptr(), *sizes, ints.data_ptr(),
                                  motp.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "trackeval_clear")
    counts = outs[3][1]
    assert torch.equal(counts[:, :4], ints[:, :4]) and torch.equal(counts[:, 4], ints[:, 7])
    assert not bool(status.any()) and int(counts[:, 3].sum()) > 0 and int(counts[:, 4].sum()) > 0


def test_a_launch_made_for_smaller_frames_reports_it_and_leaves_nothing_half_written(libs, kernel_case):
    packed, sim, d, want = kernel_case
    S, n_gt, n_tr = len(packed.names), len(d["gt_ids"]), len(d["tr_ids"])
    inputs, sizes = device_inputs(sim, d)
    outs = [guarded(n_gt), guarded(n_gt), guarded(n_tr), guarded(S * 5, (S, 5)), guarded(S)]
    D.launch_clear_events(*inputs, 20, sizes[1], sizes[2], *[inner for _, inner in outs])        # (tall_70x9 has 70)
    torch.cuda.synchronize()
    status = outs[4][1].cpu().numpy()
    too_large = np.array([np.diff(d["gt_off"])[d["seq_off"][s]:d["seq_off"][s + 1]].max(initial=0) > 20 for s in range(S)])
    assert np.array_equal(status, np.where(too_large, -2, 0)) and 0 < too_large.sum() < S
    expect = {k: want[k].copy() for k in want}
    for s in np.flatnonzero(too_large):
        f0, f1 = d["seq_off"][s], d["seq_off"][s + 1]
        expect["gt_partner"][d["gt_off"][f0]:d["gt_off"][f1]] = -1
        expect["gt_flags"][d["gt_off"][f0]:d["gt_off"][f1]] = 0
        expect["tr_partner"][d["tr_off"][f0]:d["tr_off"][f1]] = -1
        expect["counts"][s] = 0
    for (whole, inner), key in zip(outs[:4], ("gt_partner", "gt_flags", "tr_partner", "counts")):
        assert torch.equal(inner.cpu(), torch.from_numpy(expect[key])), key
        assert guards_untouched(whole, inner.numel()), key


@pytest.mark.parametrize("prefix", sorted(C.SETS))
def test_clear_events_on_the_device_equals_the_host_statement(libs, prefix):
    _, packed = C.golden(prefix)
    want = D.clear_events(packed, C.SETS[prefix])
    for source in (packed, packed.to("cuda")):
        got = D.clear_events(source, C.SETS[prefix], device="cuda")
        assert list(got) == list(want)
        for name in want:
            for k in D.SequenceEvents.ARRAYS:
                a, b = getattr(got[name], k), getattr(want[name], k)
                assert a.dtype == b.dtype and np.array_equal(a, b), (name, k)        # (gt_iou: the same bits)
    fields = E.evaluate_packed(packed.to("cuda"), C.SETS[prefix], device="cuda")
    for name in want:
        assert got[name].counts() == {k: int(fields[name][k]) for k in D.COUNTS}, name


# ------------------------------------------------------------------------------------------------ the error table
@pytest.mark.parametrize("bgr,font_scale", [(False, 1), (True, 2)])
def test_the_table_kernel_equals_the_host_statement(libs, bgr, font_scale):
    ev = C.table_events()
    assert C.has_every_kind({"gt_kind": ev.gt_kind, "tr_kind": ev.tr_kind, "gt_frag": np.ones(1)})
    full = ev.max_drawn_rows()
    assert full > 256 and len(D._table_rows(ev, 1)[0]) == 0 and len(D._table_rows(ev, 2)[0]) == full
    ids = D._table_rows(ev, 0)[0].tolist()
    assert [len(str(i)) for i in ids[:4]] == [1, 8, 9, 10]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()                      # noqa: E731
    arrays = [up(ev.gt_boxes, np.float64), up(ev.tr_boxes, np.float64), up(ev.gt_off, np.int32), up(ev.tr_off, np.int32),
              up(ev.gt_ids, np.int32), up(ev.tr_ids, np.int32), up(ev.gt_kind, np.int32), up(ev.tr_kind, np.int32)]
    for max_rows in (full, 5, full + 3):                # the fullest frame fills it; rows left out; padding everywhere
        want = D.error_table_host(ev, C.WIDTH, C.HEIGHT, bgr=bgr, font_scale=font_scale, max_rows=max_rows)
        whole, table = guarded(ev.n_frames * max_rows * 16, (ev.n_frames, max_rows, 16))
        D.launch_error_table(*arrays, max_rows, C.WIDTH, C.HEIGHT, bgr, font_scale, table)
        torch.cuda.synchronize()
        assert torch.equal(table.cpu(), torch.from_numpy(want)), max_rows
        assert guards_untouched(whole, table.numel()), max_rows
    got = D.error_table_device(ev, C.WIDTH, C.HEIGHT, "cuda", bgr=bgr, font_scale=font_scale)
    assert torch.equal(got.cpu(), torch.from_numpy(D.error_table_host(ev, C.WIDTH, C.HEIGHT, bgr=bgr, font_scale=font_scale)))
    tabs = got[0].cpu().numpy()
    assert tabs[0, 6] == tabs[0, 1] and tabs[1, 7] == C.WIDTH - 1 and tabs[3, 7] == C.WIDTH - 1      # top edge, right edge


# ---------------------------------------------------------------------------------------------------- end to end
def test_error_frames_on_the_device_are_the_host_paths_bytes(libs, tmp_path):
    args, paths = C.write_tree(str(tmp_path / "tree"))
    ev = D.events_from_files(*args, device="cuda")[C.TREE_SEQ]
    host = D.events_from_files(*args)[C.TREE_SEQ]
    assert all(np.array_equal(getattr(ev, k), getattr(host, k)) for k in D.SequenceEvents.ARRAYS)
    assert ev.frame_errors().sum(1).tolist() == [2, 0, 1]
    want = C.expected_frame_files(ev, paths, 85, 2, 2)
    on_host = D.write_error_frames(ev, paths, str(tmp_path / "host"), quality=85, thickness=2, font_scale=2)
    for chunk, out in ((16, "device"), (2, "chunks")):
        written = D.write_error_frames(ev, paths, str(tmp_path / out), quality=85, thickness=2, font_scale=2,
                                       device="cuda", chunk=chunk)
        assert [os.path.basename(p) for p in written] == [os.path.basename(p) for p in on_host] == [
            "00000001.jpg", "00000002.jpg", "00000003.jpg"]
        for t, (a, b) in enumerate(zip(written, on_host), start=1):
            with open(a, "rb") as fa, open(b, "rb") as fb:
                data = fa.read()
                assert data == fb.read() == want[t], (out, t)
    only = D.write_error_frames(ev, paths, str(tmp_path / "errors"), only_errors=True, quality=85, font_scale=2,
                                device="cuda")
    assert [os.path.basename(p) for p in only] == ["00000001.jpg", "00000003.jpg"]
    assert sorted(os.listdir(tmp_path / "errors")) == ["00000001.jpg", "00000003.jpg"]
    for path, t in zip(only, (1, 3)):
        with open(path, "rb") as f:
            assert f.read() == want[t], t
