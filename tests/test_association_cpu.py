"""CPU: the association analysis (memotr_amd/association.py).  The host statement of HOTA's and Identity's matches
against what TrackEval's solvers returned on the fixture's sequences (tests/golden/association.npz: every pair of every
frame with its similarity, the Identity metric's assignment of every sequence) and against the evaluation's own sums;
the timeline and the two CSVs of a hand-written sequence against literal bytes and text; the file entry points and the
command line on a small tree; the four C entry points' declarations and argument errors."""
import ctypes
import os

import numpy as np
import pytest

import association_cases as AC
import clear_events_cases as C
from cabi_helpers import assert_binding_matches_header, define

from memotr_amd import association as A
from memotr_amd import evaluation as E


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_pairs_and_levels_per_frame_are_trackevals(prefix):
    g, packed = AC.golden(prefix)
    d, sim, h = AC.host(prefix)
    n_pairs = n_below = 0
    for f in range(len(d["gt_off"]) - 1):
        g0, g1, t0, t1 = d["gt_off"][f], d["gt_off"][f + 1], d["tr_off"][f], d["tr_off"][f + 1]
        a, b = g["pair_off"][f], g["pair_off"][f + 1]
        level = AC.levels(g["pair_sim"][a:b])
        want = sorted(zip(g["pair_gt"][a:b][level > 0].tolist(), g["pair_tr"][a:b][level > 0].tolist(),
                          level[level > 0].tolist()))
        partner, lv = h["c::gt_partner"][g0:g1], h["c::gt_level"][g0:g1]
        hit = np.flatnonzero(partner >= 0)
        got = sorted(zip(d["gt_ids"][g0 + hit].tolist(), d["tr_ids"][t0 + partner[hit]].tolist(), lv[hit].tolist()))
        assert got == want, f
        # the two sides name each other and carry the same level; a row without a partner has level 0
        assert np.array_equal(h["c::tr_partner"][t0 + partner[hit]], hit)
        assert np.array_equal(h["c::tr_level"][t0 + partner[hit]], lv[hit])
        assert not lv[partner < 0].any() and (lv[hit] > 0).all()
        assert int((h["c::tr_partner"][t0:t1] >= 0).sum()) == len(hit)
        n_pairs, n_below = n_pairs + len(want), n_below + int((level == 0).sum())
    assert n_pairs + n_below == len(g["pair_gt"]) and n_pairs > 0
    seen = set(np.unique(h["c::gt_level"]).tolist())     # unmatched, matched at every threshold, and levels between
    assert seen >= {0, 19} and len(seen) >= 6 and max(seen) == 19
    # the input rows: a pair's iou is TrackEval's similarity entry, bit for bit, and the partner is named as the files do
    assert np.array_equal(np.sort(h["gt_iou"][h["gt_level"] > 0]), np.sort(g["pair_sim"][AC.levels(g["pair_sim"]) > 0]))
    kept = np.zeros(len(packed.gt_ids), bool)
    kept[d["keep_gt"]] = True
    assert np.array_equal(h["gt_kept"], kept) and not h["gt_level"][~kept].any() and (h["gt_partner_id"][~kept] == -1).all()
    assert (~kept).any() and np.array_equal(h["gt_level"][kept], h["c::gt_level"])
    assert np.array_equal(h["tr_level"][d["keep_tr"]], h["c::tr_level"])
    assert np.array_equal(np.sort(h["tr_iou"][h["tr_level"] > 0]), np.sort(h["gt_iou"][h["gt_level"] > 0]))


def test_the_solver_was_recorded_where_the_issue_counts_it():
    g, _ = AC.golden("mot17")
    assert g["hota_calls"].tolist() == [8, 1, 34, 130, 6, 6, 37, 0, 0, 0] and len(g["pair_gt"]) == 3487
    ids150 = [str(n) for n in g["names"]].index("ids150")
    assert int(g["id_shape"].sum(1).max()) == 218 and g["id_shape"][ids150].tolist() == [60, 158]
    assert np.diff(g["id_off"]).tolist() == [int(n) if c else 0 for n, c in zip(g["id_shape"].sum(1), g["hota_calls"])]


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_the_identity_map_is_trackevals(prefix):
    g, _ = AC.golden(prefix)
    d, _, h = AC.host(prefix)
    n_credited = 0
    for s in range(len(d["seq_off"]) - 1):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        gs, ts = slice(d["gid_off"][s], d["gid_off"][s + 1]), slice(d["tid_off"][s], d["tid_off"][s + 1])
        rows, cols = g["id_rows"][g["id_off"][s]:g["id_off"][s + 1]], g["id_cols"][g["id_off"][s]:g["id_off"][s + 1]]
        want_gt, want_tr = np.full(G, -1), np.full(K, -1)
        if len(rows):
            assert g["id_shape"][s].tolist() == [G, K] and len(rows) == G + K
            pair = (rows < G) & (cols < K)
            want_gt[rows[pair]], want_tr[cols[pair]] = cols[pair], rows[pair]
        assert np.array_equal(h["gt_id_partner"][gs], want_gt) and np.array_equal(h["tr_id_partner"][ts], want_tr), s
        credited = np.flatnonzero(want_gt >= 0)
        assert np.array_equal(h["gt_idtp"][gs][credited], h["tr_idtp"][ts][want_gt[credited]])
        assert not h["gt_idtp"][gs][want_gt < 0].any() and not h["tr_idtp"][ts][want_tr < 0].any()
        n_credited += len(credited)
    assert n_credited > 0 and (h["gt_id_partner"] < 0).any()


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_tables_are_those_of_the_matches_rebuilt_from_the_recorded_pairs(prefix):
    g, _ = AC.golden(prefix)
    d, _, h = AC.host(prefix)
    matches = AC.matches_from_pairs(g, d)
    assert np.array_equal(h["matches"], matches) and h["matches"].dtype == np.int32 and matches.any()
    a0 = A.DEFAULT_ALPHA_INDEX
    for s in range(len(d["seq_off"]) - 1):
        G, K = int(d["n_gt_ids"][s]), int(d["n_tr_ids"][s])
        gs, ts = slice(d["gid_off"][s], d["gid_off"][s + 1]), slice(d["tid_off"][s], d["tid_off"][s + 1])
        m = matches[A.N_ALPHA * d["cell_off"][s]:A.N_ALPHA * d["cell_off"][s + 1]].reshape(A.N_ALPHA, G, K)
        assert np.array_equal(h["gt_tp"][gs], m.sum(2).T) and np.array_equal(h["tr_tp"][ts], m.sum(1).T)
        for top, table in ((h["gt_top"][gs], m[a0]), (h["tr_top"][ts], m[a0].T)):
            for i, row in enumerate(table.tolist()):         # the largest count; ties go to the lowest id
                best = max(row, default=0)
                assert top[i].tolist() == [sum(v > 0 for v in row), row.index(best) if best > 0 else -1, best], (s, i)
    assert (h["gt_top"][:, 0] > 1).any() and (h["gt_top"][:, 1] == -1).any()


@pytest.mark.parametrize("prefix", sorted(AC.SETS))
def test_totals_are_the_evaluations_sums(prefix):
    _, packed = AC.golden(prefix)
    d, _, _ = AC.host(prefix)
    tables, fields = E.host_tables(packed, AC.SETS[prefix]), E.evaluate_packed(packed, AC.SETS[prefix])
    got = A.association(packed, AC.SETS[prefix])
    assert list(got) == packed.names
    for s, name in enumerate(packed.names):
        t = got[name].totals()
        assert t["HOTA_TP"].dtype == np.int64 and np.array_equal(t["HOTA_TP"], tables["hota_tp"][s]), name
        assert (t["IDTP"], t["IDFN"], t["IDFP"]) == tuple(int(fields[name][k]) for k in ("IDTP", "IDFN", "IDFP")), name
        if tables["n_gt_dets"][s] and tables["n_tr_dets"][s]:
            assert t["IDTP"] == tables["n_gt_dets"][s] - tables["identity"][s][0]
        rtol = AC.num_rtol(d)
        for k, i in (("AssA", 0), ("AssRe", 1), ("AssPr", 2)):
            np.testing.assert_allclose(t[k], tables["hota_sums"][s][i], rtol=rtol, atol=0, err_msg=f"{name} {k}")
        # the tracker side's AssA numerator is the same sum read by columns
        np.testing.assert_allclose(got[name].tr_num[:, 0].sum(0), tables["hota_sums"][s][0], rtol=rtol, atol=0)
    with pytest.raises(ValueError, match="BDD100K"):
        A.association(packed, benchmark="BDD100K")
    with pytest.raises(ValueError, match="alpha_index"):
        A.association(packed, alpha_index=19)


# ------------------------------------------------------------------------------------------ the hand-written case
@pytest.fixture(scope="module")
def hand():
    return AC.hand_association()


def test_per_identity_scores_and_fragments_of_the_hand_written_case(hand):
    assert hand.gt_identities.tolist() == [1, 2, 3] and hand.tr_identities.tolist() == [11, 12, 13, 14, 15]
    assert hand.gt_count.tolist() == [5, 5, 4] and hand.gt_tp[:, 9].tolist() == [3, 5, 4] and hand.gt_tp[:, 7].tolist() == [4, 5, 4]
    # identity 2: 3 frames under 12 and 2 under 13: (3 * 3 / 5 + 2 * 2 / 5) / 5; identity 1: 0.8 below level 8, then 0.5
    np.testing.assert_allclose(hand.ass_a(), [(8 * 0.8 + 11 * 0.5) / 19, 0.52, 1.0], rtol=1e-15)
    np.testing.assert_allclose(hand.id_f1(), [2 * 3 / 9, 2 * 3 / 8, 1.0], rtol=1e-15)
    np.testing.assert_allclose(hand.id_f1("tr"), [2 * 3 / 9, 2 * 3 / 8, 0.0, 1.0, 0.0], rtol=1e-15)
    assert hand.gt_id_partner.tolist() == [11, 12, 14] and hand.tr_id_partner.tolist() == [1, 2, -1, 3, -1]
    assert hand.gt_n_partners.tolist() == [1, 2, 1] and hand.gt_top_partner.tolist() == [11, 12, 14]
    assert hand.worst_identities(2) == [(2, pytest.approx(0.52), 5, 2), (1, pytest.approx(0.6263157894736843), 5, 1)]
    assert len(hand.worst_identities(10)) == 3 and hand.worst_identities(0) == []
    assert hand.fragments(1) == [(1, 2, 11), (4, 4, 11)] and hand.fragments(2) == [(1, 3, 12), (4, 5, 13)]
    assert hand.fragments(3) == [(1, 1, 14), (3, 5, 14)] and hand.fragments(99) == []
    t = hand.totals()
    assert t["HOTA_TP"].tolist() == [13] * 8 + [12] * 11 and (t["IDTP"], t["IDFN"], t["IDFP"]) == (10, 4, 4)


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("cell", [(1, 1), (3, 2)])
def test_timeline_of_the_hand_written_case_is_these_bytes(hand, bgr, cell):
    cell_w, cell_h = cell
    for alpha_index, cells in AC.HAND_CELLS.items():
        want = np.array(cells, np.uint8)
        if bgr:
            want = want[..., ::-1]
        want = np.repeat(np.repeat(want, cell_h, 0), cell_w, 1)
        got = A.timeline_host(hand, alpha_index, cell_w, cell_h, bgr)
        assert got.dtype == np.uint8 and got.shape == (3 * cell_h, 5 * cell_w, 3) and np.array_equal(got, want)
        assert np.array_equal(A.timeline(hand, alpha_index, cell_w, cell_h, bgr).numpy(), want)


def test_a_timeline_past_the_jpeg_limit_raises(hand):
    for kwargs in (dict(cell_h=21846), dict(cell_w=13108)):
        with pytest.raises(ValueError, match="65535"):
            A.timeline_host(hand, **kwargs)
    assert A.timeline_host(hand, cell_h=21845, cell_w=1).shape == (65535, 5, 3)
    with pytest.raises(ValueError, match="at least 1"):
        A.timeline_host(hand, cell_w=0)


HAND_IDENTITIES_CSV = """side,id,length,tp50,AssA,AssRe_or_AssPr,n_partners,top_partner,top_count,id_partner,idtp,IDF1
gt,1,5,3,0.6263157894736843,0.6842105263157894,1,11,3,11,3,0.6666666666666666
gt,2,5,5,0.5199999999999999,0.5199999999999999,2,12,3,12,3,0.75
gt,3,4,4,1.0,1.0,1,14,4,14,4,1.0
tr,11,4,3,0.6263157894736843,0.8552631578947368,1,1,3,1,3,0.6666666666666666
tr,12,3,3,0.6,1.0,1,2,3,2,3,0.75
tr,13,2,2,0.4000000000000001,1.0,1,2,2,-1,0,0.0
tr,14,4,4,1.0,1.0,1,3,4,3,4,1.0
tr,15,1,0,0.0,0.0,0,-1,0,-1,0,0.0
"""


def test_both_csvs_of_the_hand_written_case_as_text(hand, tmp_path):
    rows, identities = str(tmp_path / "out" / "hand_rows.csv"), str(tmp_path / "out" / "hand_identities.csv")
    hand.write_rows_csv(rows)
    hand.write_identities_csv(identities)
    with open(rows) as f:
        assert f.read() == AC.HAND_ROWS_CSV
    with open(identities) as f:
        assert f.read() == HAND_IDENTITIES_CSV


# ------------------------------------------------------------------------------------- files and the command line
@pytest.fixture(scope="module")
def jpeg_libs():
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib
    build_jpeg_lib(), build_jpeg_enc_lib()


def test_the_command_line_and_the_file_entry_points(tmp_path, jpeg_libs, capsys):
    (gt_root, tracker_dir, seqmap), _ = C.write_tree(str(tmp_path / "tree"))
    out = str(tmp_path / "report")
    assert A.main(["--gt-root", gt_root, "--tracker-dir", tracker_dir, "--seqmap", seqmap, "--out", out,
                   "--device", "cpu", "--worst", "5"]) == 0
    seq = C.TREE_SEQ
    assert sorted(os.listdir(out)) == [seq + "_identities.csv", seq + "_rows.csv", seq + "_timeline.jpg", "summary.txt"]
    fields = E.evaluate_files(gt_root, tracker_dir, seqmap)[seq]
    with open(os.path.join(out, "summary.txt")) as f:
        text = f.read()
    assert capsys.readouterr().out == text
    summary = text.splitlines()
    assert summary[0] == (f"{seq} HOTA_TP@0.50={int(fields['HOTA_TP'][9])} AssA={np.mean(fields['AssA']):.5f} "
                          f"AssRe={np.mean(fields['AssRe']):.5f} AssPr={np.mean(fields['AssPr']):.5f} "
                          f"IDTP={fields['IDTP']} IDFN={fields['IDFN']} IDFP={fields['IDFP']}")
    assert int(fields["HOTA_TP"][9]) == 5 and (fields["IDTP"], fields["IDFN"], fields["IDFP"]) == (4, 2, 2)
    # identity 1 is followed by 11 and then by 14, identity 2 is missed in the first frame
    assert summary[1].startswith("  gt 1: AssA=") and summary[1].endswith("length=3 partners=2 [1-2:11 3-3:14]")
    assert summary[2].startswith("  gt 2: AssA=") and summary[2].endswith("length=3 partners=1 [2-3:13]")
    assert len(summary) == 3
    # the files are what the entry points give
    assoc = A.association_from_files(gt_root, tracker_dir, seqmap)[seq]
    again = E.load_files(gt_root, tracker_dir, seqmap).association()[seq]
    for k in A.SequenceAssociation.ROW_ARRAYS + A.SequenceAssociation.INT_TABLES + A.SequenceAssociation.FLOAT_TABLES:
        assert np.array_equal(getattr(assoc, k), getattr(again, k)), k
    assoc.write_rows_csv(str(tmp_path / "rows.csv"))
    with open(tmp_path / "rows.csv") as a, open(os.path.join(out, seq + "_rows.csv")) as b:
        lines = a.read()
        assert lines == b.read() and lines.splitlines()[0] == A.ROWS_HEADER and len(lines.splitlines()) == 13
    from memotr_amd.data.jpeg import decode_jpeg
    from memotr_amd.data.jpeg_write import encode_jpeg
    with open(os.path.join(out, seq + "_timeline.jpg"), "rb") as f:
        data = f.read()
    assert data == encode_jpeg(A.timeline(assoc), 90, subsampling="4:4:4")
    px = decode_jpeg(os.path.join(out, seq + "_timeline.jpg"), "cpu").numpy().astype(int)
    assert px.shape == (2 * 6, 3 * 2, 3)
    near = lambda p, c: np.abs(p - np.array(c)).max() < 40                                       # noqa: E731
    assert near(px[2, 0], AC.P11) and near(px[2, 4], AC.P14) and near(px[8, 0], AC.GREY) and near(px[8, 3], AC.P13)
    with pytest.raises(SystemExit):
        A.main(["--gt-root", gt_root, "--tracker-dir", tracker_dir, "--seqmap", seqmap, "--out", out, "--alpha", "0.52"])


# ------------------------------------------------------------------------------------------------------ the C ABI
ENTRIES = ("clipops_hota_events_f64", "clipops_identity_pairs_i32", "clipops_assoc_reduce_f64", "clipops_timeline_u8")


def test_the_entries_are_declared_and_the_abi_stays_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert all(name in declared for name in ENTRIES)
    assert clip_lib.ABI_VERSION == 12 and clip_lib.lib.clipops_abi_version() == 12
    assert define("clip_ops_hip.h", "CLIPOPS_ASSOC_ALPHAS") == A.N_ALPHA == 19


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, p = clip_lib.lib, ctypes.c_void_p(64)
    err = lib.clipops_last_error
    alphas = np.ascontiguousarray(E.ALPHAS, np.float64)

    inputs = ("sim", "sim_off", "gt_off", "tr_off", "gt_ids", "tr_ids", "frame_seq")
    tables = ("n_tr_ids", "cell_off", "alignment", "alphas")
    outputs = ("gt_partner", "gt_level", "tr_partner", "tr_level", "matches", "status")

    def events(n_frames=2, max_gt=8, max_tr=8, **ptrs):
        a = {k: ptrs.get(k, p) for k in inputs + tables + outputs}
        if "alphas" not in ptrs:
            a["alphas"] = alphas.ctypes.data
        return lib.clipops_hota_events_f64(*[a[k] for k in inputs], n_frames, *[a[k] for k in tables], max_gt, max_tr,
                                           *[a[k] for k in outputs], None)

    for kwargs in (dict(n_frames=-1), dict(max_gt=-1), dict(max_tr=-1)):
        assert events(**kwargs) == 1 and b"negative" in err(), kwargs
    for kwargs in (dict(max_gt=2049), dict(max_tr=2049)):
        assert events(**kwargs) == 2 and b"CLIPOPS_EVENTS_MAX_DIM" in err(), kwargs
    for name in inputs + tables + outputs:
        if name != "matches":                           # (matches may be null: the table is then not counted)
            assert events(**{name: None}) == 1 and b"null" in err(), name
    assert events(n_frames=0, **{k: None for k in inputs + tables + outputs}) == 0 and err() == b""

    seq_tables = ("n_gt_ids", "n_tr_ids", "cell_off", "gid_off", "tid_off", "gt_count", "tr_count")
    id_out = ("gt_id_partner", "gt_idtp", "tr_id_partner", "tr_idtp", "status")

    def identity(n_seqs=2, max_ids=8, **ptrs):
        a = {k: ptrs.get(k, p) for k in seq_tables + ("id_matches",) + id_out}
        return lib.clipops_identity_pairs_i32(n_seqs, *[a[k] for k in seq_tables], a["id_matches"], max_ids,
                                              *[a[k] for k in id_out], None)

    for kwargs in (dict(n_seqs=-1), dict(max_ids=-1)):
        assert identity(**kwargs) == 1 and b"negative" in err(), kwargs
    assert identity(max_ids=2049) == 2 and b"CLIPOPS_EVENTS_MAX_DIM" in err()
    for name in seq_tables + ("id_matches",) + id_out:
        assert identity(**{name: None}) == 1 and b"null" in err(), name
    assert identity(n_seqs=0, **{k: None for k in seq_tables + ("id_matches",) + id_out}) == 0 and err() == b""

    red_out = ("gt_tp", "gt_num", "gt_top", "tr_tp", "tr_num", "tr_top")

    def reduce(n_seqs=2, max_side_ids=8, alpha_index=9, **ptrs):
        a = {k: ptrs.get(k, p) for k in seq_tables + ("matches",) + red_out}
        return lib.clipops_assoc_reduce_f64(n_seqs, *[a[k] for k in seq_tables], a["matches"], max_side_ids, alpha_index,
                                            *[a[k] for k in red_out], None)

    for kwargs in (dict(n_seqs=-1), dict(max_side_ids=-1)):
        assert reduce(**kwargs) == 1 and b"negative" in err(), kwargs
    for index in (-1, 19):
        assert reduce(alpha_index=index) == 1 and b"alpha_index" in err(), index
    assert reduce(n_seqs=65536) == 2 and b"65535 sequences" in err()
    assert reduce(max_side_ids=2049) == 2 and b"CLIPOPS_EVENTS_MAX_DIM" in err()
    for name in seq_tables + ("matches",) + red_out:
        assert reduce(**{name: None}) == 1 and b"null" in err(), name
    for kwargs in (dict(n_seqs=0), dict(max_side_ids=0)):
        assert reduce(**{k: None for k in seq_tables + ("matches",) + red_out}, **kwargs) == 0 and err() == b"", kwargs

    rows = ("gt_off", "gt_ids", "partner_id", "level")

    def timeline(n_ids=3, n_frames=5, alpha_index=9, cell_w=2, cell_h=6, bgr=0, image=p, **ptrs):
        return lib.clipops_timeline_u8(*[ptrs.get(k, p) for k in rows], n_ids, n_frames, alpha_index, cell_w, cell_h, bgr,
                                       image, None)

    for kwargs in (dict(n_ids=-1), dict(n_frames=-1)):
        assert timeline(**kwargs) == 1 and b"negative" in err(), kwargs
    for kwargs in (dict(cell_w=0), dict(cell_h=-2)):
        assert timeline(**kwargs) == 1 and b"cell_w or cell_h" in err(), kwargs
    for index in (-1, 19):
        assert timeline(alpha_index=index) == 1 and b"alpha_index" in err(), index
    for kwargs in (dict(n_ids=10923), dict(n_frames=32768)):
        assert timeline(**kwargs) == 2 and b"65535" in err(), kwargs
    for name in rows + ("image",):
        assert timeline(**{name: None}) == 1 and b"null" in err(), name
    for kwargs in (dict(n_ids=0), dict(n_frames=0)):
        assert timeline(image=None, **{k: None for k in rows}, **kwargs) == 0 and err() == b"", kwargs
