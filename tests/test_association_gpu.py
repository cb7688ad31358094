"""GPU: the four kernels of the association analysis (memotr_amd/csrc/clip_tracks.h) against the host statements of
memotr_amd/association.py on both fixture packs: integers and similarities bit for bit, the per-identity float sums
within the derived summation bound; ``matches`` counted from the new events against the pinned library's table; a launch
sized below a frame; the timeline's bytes; and the file entry point on the device against the host's."""
import numpy as np
import pytest
import torch

import association_cases as AC
import clear_events_cases as C

from memotr_amd import association as A
from memotr_amd import evaluation as E

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0x5A5A5A5A


@pytest.fixture(scope="module")
def libs(clip_lib):
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib, build_track_eval_lib
    build_track_eval_lib(), build_jpeg_lib(), build_jpeg_enc_lib()
    return clip_lib


@pytest.fixture(scope="module")
def device_runs(libs):
    """{prefix: (two runs of ``device_association_tables`` as host arrays, ``device_tables``' matches)}: once."""
    out = {}
    for prefix, benchmark in AC.SETS.items():
        packed = AC.golden(prefix)[1].to("cuda")
        runs = []
        for _ in range(2):
            t = A.device_association_tables(packed, benchmark)
            host = t.pop("host")
            runs.append(({k: v.cpu().numpy() for k, v in t.items()}, host))
        out[prefix] = runs, E.device_tables(packed, benchmark)
    return out


def guarded(n, shape=None, dtype=torch.int32, fill=SENTINEL):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    inner = whole[GUARD:GUARD + n]
    return whole, inner if shape is None else inner.view(shape)


def guards_untouched(whole, n, fill=SENTINEL):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_the_device_path_equals_the_host_statement(device_runs, prefix):
    d, _, want = AC.host(prefix)
    (got, ids), _ = device_runs[prefix][0]
    rtol = AC.num_rtol(d)
    assert rtol <= 218 * 2.0 ** -52
    for k in AC.int_keys(want):
        source = ids if k in ids else got
        assert source[k].dtype == want[k].dtype and np.array_equal(source[k], want[k]), k
    for k in ("gt_iou", "tr_iou"):                       # a copy of a similarity entry: the same bits
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), k
    for k in AC.NUM_KEYS:
        print(k, "largest relative difference", float(np.max(np.abs(got[k] - want[k]) / np.maximum(want[k], 1e-300))),
              "bound", rtol)
        assert got[k].shape == want[k].shape
        np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=0, err_msg=k)
    assert set(got) | set(ids) >= set(want)
    assert not got["frame_status"].any() and not got["id_status"].any()
    assert len(got["frame_status"]) == len(d["gt_off"]) - 1 and len(got["id_status"]) == len(d["seq_off"]) - 1
    if prefix == "mot17":                               # what the pack is there for
        g, k = np.diff(d["gt_off"]), np.diff(d["tr_off"])
        assert ((g == 7) & (k >= 65)).any() and ((g == 70) & (k == 9)).any()
        assert (d["n_gt_ids"] + d["n_tr_ids"]).max() == 218 and d["n_tr_ids"].max() > 64 and d["n_gt_ids"].max() > 64
        assert len(d["n_gt_ids"]) == 10 and d["cell_off"][-2] > 0 and d["gid_off"][-2] > 0 and d["tid_off"][-2] > 0
        assert (d["n_gt_dets"] == 0).any() and (d["n_tr_dets"] == 0).any()


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_matches_counted_from_the_events_are_the_pinned_librarys(device_runs, prefix):
    ((got, _), _), tables = device_runs[prefix]
    theirs = tables["matches"].cpu()
    assert torch.equal(torch.from_numpy(got["matches"]), theirs) and int(theirs.sum()) > 0
    d, _, _ = AC.host(prefix)
    for s in range(len(d["seq_off"]) - 1):              # the per-identity sums add up to the evaluation's tables
        gs = slice(d["gid_off"][s], d["gid_off"][s + 1])
        assert np.array_equal(got["gt_tp"][gs].sum(0), tables["hota_tp"][s].cpu().numpy())
        assert int(got["gt_count"][gs].sum()) == int(tables["n_gt_dets"][s])
        if d["n_gt_dets"][s] and d["n_tr_dets"][s]:     # (trackeval_identity: IDFN of a sequence that is walked)
            assert int(got["gt_count"][gs].sum()) - int(got["gt_idtp"][gs].sum()) == int(tables["identity"][s, 0])
        # G * K bit-equal non-negative terms in two summation orders: at most (n - 1) * 2**-52 apart, relative
        np.testing.assert_allclose(got["gt_num"][gs].sum(0), tables["hota_sums"][s, :2].cpu().numpy(),
                                   rtol=float(max(d["n_gt_ids"][s] * d["n_tr_ids"][s], 1)) * 2.0 ** -52, atol=0)


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_two_runs_give_the_same_bits(device_runs, prefix):
    (first, _), (second, _) = device_runs[prefix][0]
    assert sorted(first) == sorted(second)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k


def test_a_launch_sized_below_a_frame_reports_it_and_leaves_the_rest(device_runs):
    d, _, want = AC.host("mot17")
    _, tables = device_runs["mot17"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                             # noqa: E731
    F, n_gt, n_tr = len(d["gt_off"]) - 1, len(d["gt_ids"]), len(d["tr_ids"])
    g, k = np.diff(d["gt_off"]), np.diff(d["tr_off"])
    assert g.max() == 70
    frame_seq = np.repeat(np.arange(len(d["seq_off"]) - 1, dtype=np.int32), np.diff(d["seq_off"]))
    inputs = [tables["similarity"].contiguous(), up(d["sim_off"]), up(d["gt_off"]), up(d["tr_off"]), up(d["gt_ids"]),
              up(d["tr_ids"]), up(frame_seq), up(d["n_tr_ids"]), up(d["cell_off"]), tables["alignment"].contiguous()]
    outs = [guarded(n_gt), guarded(n_gt), guarded(n_tr), guarded(n_tr), guarded(F)]
    A.launch_hota_events(*inputs, 69, int(k.max()), *[inner for _, inner in outs[:4]], None, outs[4][1])
    torch.cuda.synchronize()
    too_large = g > 69
    assert 0 < too_large.sum() < F and np.array_equal(outs[4][1].cpu().numpy(), np.where(too_large, -2, 0))
    expect = {key: want["c::" + key].copy() for key in ("gt_partner", "gt_level", "tr_partner", "tr_level")}
    for f in np.flatnonzero(too_large):
        expect["gt_partner"][d["gt_off"][f]:d["gt_off"][f + 1]] = -1
        expect["gt_level"][d["gt_off"][f]:d["gt_off"][f + 1]] = 0
        expect["tr_partner"][d["tr_off"][f]:d["tr_off"][f + 1]] = -1
        expect["tr_level"][d["tr_off"][f]:d["tr_off"][f + 1]] = 0
    assert not np.array_equal(expect["gt_partner"], want["c::gt_partner"])
    for (whole, inner), key in zip(outs[:4], ("gt_partner", "gt_level", "tr_partner", "tr_level")):
        assert torch.equal(inner.cpu(), torch.from_numpy(expect[key])), key
        assert not bool((inner == SENTINEL).any()) and guards_untouched(whole, inner.numel()), key
    assert guards_untouched(outs[4][0], F)


@pytest.fixture(scope="module")
def sequences(libs):
    return A.association(AC.golden("mot17")[1], "MOT17")


@pytest.mark.parametrize("name", ["walk130", "ids150"])
@pytest.mark.parametrize("cell,bgr", [((1, 1), False), ((3, 5), True), ((1, 1), True), ((3, 5), False)])
def test_the_timeline_kernel_writes_the_host_statements_bytes(sequences, name, cell, bgr):
    assoc = sequences[name]
    want = A.timeline_host(assoc, 9, cell[0], cell[1], bgr)
    G, F = len(assoc.gt_identities), assoc.n_frames
    assert want.shape == (G * cell[1], F * cell[0], 3) and G > 1 and F > 1
    colours = {tuple(c) for c in want.reshape(-1, 3).tolist()}
    assert AC.BLACK in colours and AC.GREY in colours and len(colours) > 4
    got = A.timeline(assoc, 9, cell[0], cell[1], bgr, device="cuda")
    assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    # the launch itself, between guard bytes, at another threshold
    want = A.timeline_host(assoc, 17, cell[0], cell[1], bgr)
    whole, image = guarded(want.size, want.shape, torch.uint8, 0xA5)
    rows = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in A._timeline_rows(assoc)]
    A.launch_timeline(*rows, G, 17, cell[0], cell[1], bgr, image)
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy(), want) and guards_untouched(whole, want.size, 0xA5)


def test_the_timeline_kernel_past_one_pass_of_identities():
    """The kernel builds a frame's column 8,192 identities a pass: 8,200 identities over 3 frames reach the second pass,
    with rows on both sides of the boundary, an absent identity on either side and an empty frame."""
    G, F = 8200, 3
    present = np.ones((F, G), bool)
    present[0, [5, 8191, 8192, 8199]] = False
    present[1] = False
    ids = np.arange(G, dtype=np.int32) * 3 + 7
    frames = [np.flatnonzero(present[f]) for f in range(F)]
    rows = np.concatenate(frames)
    fields = {k: None for k in A.SequenceAssociation.__dataclass_fields__}
    fields.update(name="many", alpha_index=9, gt_off=np.concatenate(([0], np.cumsum([len(r) for r in frames]))).astype(np.int32),
                  gt_ids=ids[rows], gt_kept=np.ones(len(rows), bool), gt_identities=ids,
                  gt_partner_id=np.where(rows % 5 == 0, -1, 1000 + rows % 97).astype(np.int32),
                  gt_level=np.where(rows % 5 == 0, 0, 1 + rows % 19).astype(np.int32))
    assoc = A.SequenceAssociation(**fields)
    for cell, bgr in (((1, 1), False), ((2, 3), True)):
        want = A.timeline_host(assoc, 9, cell[0], cell[1], bgr)
        assert want.shape == (G * cell[1], F * cell[0], 3) and not want[:, cell[0]:2 * cell[0]].any()
        assert want[8191 * cell[1]:].any() and not want[8192 * cell[1], 0].any() and want[8193 * cell[1], 0].any()
        whole, image = guarded(want.size, want.shape, torch.uint8, 0xA5)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in A._timeline_rows(assoc)]
        A.launch_timeline(*dev, G, 9, cell[0], cell[1], bgr, image)
        torch.cuda.synchronize()
        assert np.array_equal(image.cpu().numpy(), want) and guards_untouched(whole, want.size, 0xA5)


def test_association_from_files_on_the_device_equals_the_host(libs, tmp_path):
    (gt_root, tracker_dir, seqmap), _ = C.write_tree(str(tmp_path / "tree"))
    host = A.association_from_files(gt_root, tracker_dir, seqmap, device="cpu")
    dev = A.association_from_files(gt_root, tracker_dir, seqmap, device="cuda")
    assert list(host) == list(dev) == [C.TREE_SEQ]
    a, b = host[C.TREE_SEQ], dev[C.TREE_SEQ]
    for k in A.SequenceAssociation.ROW_ARRAYS + A.SequenceAssociation.INT_TABLES:
        assert getattr(a, k).dtype == getattr(b, k).dtype and np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in A.SequenceAssociation.FLOAT_TABLES:
        np.testing.assert_allclose(getattr(b, k), getattr(a, k), rtol=2 * 2.0 ** -52, atol=0, err_msg=k)
    assert b.fragments(1) == [(1, 2, 11), (3, 3, 14)] and b.totals()["IDTP"] == 4
    path = A.write_timeline(b, str(tmp_path / "t.jpg"), device="cuda")
    with open(path, "rb") as f, open(A.write_timeline(a, str(tmp_path / "h.jpg")), "rb") as h:
        assert f.read() == h.read()
