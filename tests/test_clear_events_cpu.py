"""CPU: the error analysis (memotr_amd/diagnose.py).  The host statement of CLEAR's events against what TrackEval's
CLEAR decided on the fixture's sequences (tests/golden/clear_events.npz: the pairs it kept per frame, its per-frame
IDSW increments, the rows its preprocessing kept) and against the evaluation's own counts on every sequence of the
trackeval_*.npz fixtures; the error table against ``render.track_table``; the CSV, the file entry points and the command
line on a small tree; the two C entry points' declarations and argument errors."""
import ctypes
import os

import numpy as np
import pytest

import clear_events_cases as C
import track_eval_helpers as TE
from cabi_helpers import assert_binding_matches_header, define

from memotr_amd import diagnose as D
from memotr_amd import evaluation as E
from memotr_amd import render as R


@pytest.fixture(scope="module")
def events():
    """{benchmark prefix: (fixture arrays, packed, clear_events_host's arrays)}: computed once, left unchanged."""
    out = {}
    for prefix, benchmark in C.SETS.items():
        g, packed = C.golden(prefix)
        out[prefix] = g, packed, D.clear_events_host(packed, benchmark)
    return out


def ranks(ids, off, seq_off):
    """TrackEval's relabelling: per sequence, the rank of an id among the sequence's distinct ids."""
    return E._relabel(ids, off, seq_off)[0]


@pytest.mark.parametrize("prefix", sorted(C.SETS))
def test_ignored_is_exactly_what_the_preprocessing_drops(events, prefix):
    g, p, rows = events[prefix]
    keep_gt, keep_tr = rows["gt_kind"] != D.IGNORED, rows["tr_kind"] != D.IGNORED
    count = lambda keep, off: np.concatenate(([0], np.cumsum(keep)))[off]                       # noqa: E731
    assert np.array_equal(count(keep_gt, p.gt_off), g["pre::gt_off"])
    assert np.array_equal(count(keep_tr, p.tr_off), g["pre::tr_off"])
    # ids are unique in a frame: the kept rows are TrackEval's when their relabelled ids are, row for row
    assert np.array_equal(ranks(p.gt_ids[keep_gt], g["pre::gt_off"], p.seq_off), g["pre::gt_ids"])
    assert np.array_equal(ranks(p.tr_ids[keep_tr], g["pre::tr_off"], p.seq_off), g["pre::tr_ids"])
    assert (~keep_gt).any() and ((~keep_tr).any() or prefix == "mot15")


@pytest.mark.parametrize("prefix", sorted(C.SETS))
def test_pairs_and_switches_per_frame_are_trackevals(events, prefix):
    g, p, rows = events[prefix]
    keep_gt, keep_tr = rows["gt_kind"] != D.IGNORED, rows["tr_kind"] != D.IGNORED
    gt_rank, tr_rank = np.full(len(p.gt_ids), -1), np.full(len(p.tr_ids), -1)
    gt_rank[keep_gt], tr_rank[keep_tr] = g["pre::gt_ids"], g["pre::tr_ids"]
    n_pairs = 0
    for f in range(len(p.gt_off) - 1):
        g0, g1, t0, t1 = p.gt_off[f], p.gt_off[f + 1], p.tr_off[f], p.tr_off[f + 1]
        matched = np.flatnonzero(rows["gt_partner"][g0:g1] >= 0)
        partner = rows["gt_partner"][g0:g1][matched]
        got = sorted(zip(gt_rank[g0 + matched].tolist(), tr_rank[t0 + partner].tolist()))
        a, b = g["pair_off"][f], g["pair_off"][f + 1]
        assert got == list(zip(g["pair_gt"][a:b].tolist(), g["pair_tr"][a:b].tolist())), f
        assert int((rows["gt_kind"][g0:g1] == D.SWITCH).sum()) == g["idsw"][f], f
        # the two sides name each other, and a kind says whether there is a partner
        assert np.array_equal(rows["tr_partner"][t0 + partner], matched)
        assert np.array_equal(rows["gt_partner"][g0:g1] >= 0, np.isin(rows["gt_kind"][g0:g1], (D.MATCH, D.SWITCH)))
        assert np.array_equal(rows["tr_partner"][t0:t1] >= 0, np.isin(rows["tr_kind"][t0:t1], (D.TP, D.SWITCH)))
        assert np.array_equal(rows["tr_kind"][t0 + partner] == D.SWITCH, rows["gt_kind"][g0 + matched] == D.SWITCH)
        n_pairs += len(got)
    assert n_pairs == len(g["pair_gt"]) > 0 and g["idsw"].sum() > 0


def test_the_fixture_holds_every_kind_and_a_frag_flag(events):
    assert C.has_every_kind(events["mot17"][2])
    assert C.has_every_kind(D.clear_events(C.golden("mot17")[1].select(0))["edges"])


@pytest.mark.parametrize("name", sorted(TE.SETS))
def test_counts_are_the_evaluations_on_every_fixture_sequence(name):
    _, packed = TE.golden(name)
    benchmark = TE.SETS[name]
    tables, fields = E.host_tables(packed, benchmark), E.evaluate_packed(packed, benchmark)
    got = D.clear_events(packed, benchmark)
    rows = D.clear_events_host(packed, benchmark)
    assert list(got) == packed.names
    raw_off = E._sim_offsets(packed.gt_off, packed.tr_off)
    for s, seq in enumerate(packed.names):
        ev, counts = got[seq], got[seq].counts()
        assert list(counts) == list(D.COUNTS) and rows["counts"][s].tolist() == list(counts.values())
        # host_tables leaves the tables of a sequence with an empty side at zero; its fields are then fixed by the
        # counts (_sequence_result), and those are what the events add up to
        assert counts == {k: int(fields[seq][k]) for k in D.COUNTS}, seq
        if tables["n_gt_dets"][s] and tables["n_tr_dets"][s]:
            assert list(counts.values()) == tables["clear_ints"][s][[0, 1, 2, 3, 7]].tolist(), seq
        f0 = packed.seq_off[s]
        for f in range(ev.n_frames):                    # the similarity of a pair: the same bits
            g0, g1 = ev.gt_off[f], ev.gt_off[f + 1]
            k = ev.tr_off[f + 1] - ev.tr_off[f]
            sim = tables["raw_similarity"][raw_off[f0 + f]:raw_off[f0 + f + 1]].reshape(g1 - g0, k)
            hit = np.flatnonzero(ev.gt_partner[g0:g1] >= 0)
            assert np.array_equal(ev.gt_iou[g0:g1][hit], sim[hit, ev.gt_partner[g0:g1][hit]])
            assert (ev.gt_iou[g0:g1][hit] >= 0.5 - E.EPS).all() and not ev.gt_iou[g0:g1][ev.gt_partner[g0:g1] < 0].any()


def test_benchmarks_out_of_scope_raise():
    with pytest.raises(ValueError, match="BDD100K"):
        D.clear_events(C.golden("mot17")[1], benchmark="BDD100K")


# ------------------------------------------------------------------------------------------------ the error table
@pytest.fixture(scope="module")
def table_case():
    ev = C.table_events()
    return ev, {(bgr, s): D.error_table_host(ev, C.WIDTH, C.HEIGHT, bgr=bgr, font_scale=s)
                for bgr in (False, True) for s in (1, 2)}


def test_table_rows_are_track_tables_but_for_the_two_colour_words(table_case):
    ev, tables = table_case
    assert C.has_every_kind({"gt_kind": ev.gt_kind, "tr_kind": ev.tr_kind, "gt_frag": np.ones(1)})
    n = ev.max_drawn_rows()
    assert n > 256 and tables[(False, 1)].shape == (4, n, 16) and tables[(False, 1)].dtype == np.int32
    for (bgr, scale), table in tables.items():
        for f in range(ev.n_frames):
            ids, xyxy, kinds = D._table_rows(ev, f)
            want = R.track_table(ids, xyxy, C.WIDTH, C.HEIGHT, bgr=bgr, font_scale=scale)
            others = [w for w in range(16) if w not in (4, 9)]
            assert np.array_equal(table[f, :len(ids)][:, others], want[:, others]), (bgr, scale, f)
            assert (table[f, len(ids):] == D.PADDING_ROW).all()
            for row, kind in zip(table[f], kinds):
                r, g, b = D.COLOURS[int(kind)]
                assert row[4] == ((b | g << 8 | r << 16) if bgr else (r | g << 8 | b << 16))
                assert row[9] == (0 if (77 * r + 150 * g + 29 * b) >> 8 >= 128 else 0xFFFFFF)
    # misses first, under the ground-truth id; then the tracker rows under theirs; nothing else
    ids, xyxy, kinds = D._table_rows(ev, 0)
    assert ids.tolist() == [7, 12345678, 123456789, 2147483647, 5, 6]
    assert kinds.tolist() == [D.MISS, D.MISS, D.TP, D.FP, D.SWITCH, D.FP]
    assert xyxy.dtype == np.float32 and xyxy[2].tolist() == [30.0, 8.0, 50.5, 28.5]
    first = tables[(False, 1)][0]
    assert first[:6, 10].tolist() == [1, 8, 9, 10] + [1, 1] and first[3, 12] == 0x74 and first[2, 12] == 9
    assert first[0, 6] == first[0, 1] == 3 and first[2, 6] == first[2, 1] == 8 and first[5, 6] == first[5, 1] - 9 == 1
    assert first[1, 7] == C.WIDTH - 1 and first[3, 7] == C.WIDTH - 1 and first[3, 5] < first[3, 0]         # ... on the right
    assert tables[(False, 1)][3, 0, :4].tolist() == [9, 13, 17, 21]        # 8.5, 12.5, 16.5, 20.5: floor(v + 0.5)
    assert tables[(False, 1)][3, 2, :4].tolist() == [0, 1, 64, 32]
    assert ev.max_drawn_rows() == len(D._table_rows(ev, 2)[0]) and len(D._table_rows(ev, 1)[0]) == 0


def test_bgr_swaps_bytes_0_and_2(table_case):
    _, tables = table_case
    rgb, bgr = tables[(False, 2)], tables[(True, 2)]
    swap = lambda w: (w & 0xFF00) | ((w & 0xFF) << 16) | ((w >> 16) & 0xFF)                     # noqa: E731
    assert np.array_equal(swap(rgb[..., 4]), bgr[..., 4]) and not np.array_equal(rgb[..., 4], bgr[..., 4])
    rest = [w for w in range(16) if w != 4]
    assert np.array_equal(rgb[..., rest], bgr[..., rest])


def test_rows_past_max_rows_are_left_out(table_case):
    ev, tables = table_case
    short = D.error_table_host(ev, C.WIDTH, C.HEIGHT, max_rows=5)
    assert short.shape == (4, 5, 16) and np.array_equal(short, tables[(False, 1)][:, :5])
    wide = D.error_table_host(ev, C.WIDTH, C.HEIGHT, max_rows=ev.max_drawn_rows() + 3)
    assert np.array_equal(wide[:, :-3], tables[(False, 1)]) and (wide[:, -3:] == D.PADDING_ROW).all()


@pytest.mark.parametrize("f", [0, 1, 3])
def test_the_padded_table_draws_what_the_unpadded_one_draws(table_case, f):
    ev, tables = table_case
    n = len(D._table_rows(ev, f)[0])
    frame = np.random.default_rng(f).integers(0, 256, (C.HEIGHT, C.WIDTH, 3), dtype=np.uint8)
    padded, compact = frame.copy(), frame.copy()
    R.draw_table_host(padded, tables[(False, 2)][f], 2, 2, 0)
    R.draw_table_host(compact, tables[(False, 2)][f, :n], 2, 2, 0)
    assert np.array_equal(padded, compact) and (n == 0) == np.array_equal(padded, frame)


# ------------------------------------------------------------------------- one sequence: CSV, switches, worst frames
def test_csv_round_trip_switches_and_worst_frames_on_the_edge_sequence(tmp_path):
    ev = D.clear_events(C.golden("mot17")[1].select(0))["edges"]
    # frame 4 swaps both ids; 2 is then followed under 8 again; 1 comes back as 9 in frame 7 and as 7 in frame 8
    assert ev.switches() == [(4, 1, 7, 8), (4, 2, 8, 7), (5, 2, 7, 8), (7, 1, 8, 9), (8, 1, 9, 7)]
    # frame 8: two false positives (one on a badly matched distractor, one on a zero-marked row) and a switch;
    # frame 2 has no detections, frame 3 no ground truth; ties by frame
    assert ev.worst_frames(3) == [(8, 0, 2, 1), (2, 2, 0, 0), (3, 0, 2, 0)]
    assert len(ev.worst_frames(100)) == ev.n_frames == 10 and ev.worst_frames(0) == []
    assert ev.frame_errors().sum(0).tolist() == [ev.counts()[k] for k in ("CLR_FN", "CLR_FP", "IDSW")]
    assert ev.counts() == {"CLR_TP": 12, "CLR_FN": 2, "CLR_FP": 5, "IDSW": 5, "Frag": 2}
    path = str(tmp_path / "events" / "edges.csv")
    ev.write_csv(path)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == D.CSV_HEADER and len(lines) == 1 + len(ev.gt_ids) + len(ev.tr_ids)
    assert lines[1] == "1,gt,1,0.0,0.0,10.0,10.0,MATCH,7,0.5,0" and "4,tr,8,0.0,0.0,10.0,5.0,SWITCH,1,0.5,0" in lines
    back = D.SequenceEvents.read_csv(path)
    assert back.name == "edges"
    for k in D.SequenceEvents.ARRAYS:
        assert np.array_equal(getattr(back, k), getattr(ev, k)) and getattr(back, k).dtype == getattr(ev, k).dtype, k


# ------------------------------------------------------------------------------------- files and the command line
@pytest.fixture(scope="module")
def jpeg_libs():
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib
    build_jpeg_lib(), build_jpeg_enc_lib()


@pytest.fixture()
def tree(tmp_path, jpeg_libs):
    return C.write_tree(str(tmp_path / "tree"))


def test_events_from_files_and_the_evaluator(tree):
    (gt_root, tracker_dir, seqmap), _ = tree
    events = D.events_from_files(gt_root, tracker_dir, seqmap)
    assert list(events) == [C.TREE_SEQ]
    ev = events[C.TREE_SEQ]
    fields = E.evaluate_files(gt_root, tracker_dir, seqmap)[C.TREE_SEQ]
    assert ev.counts() == {k: int(fields[k]) for k in D.COUNTS} == {"CLR_TP": 5, "CLR_FN": 1, "CLR_FP": 1, "IDSW": 1,
                                                                    "Frag": 0}
    assert ev.switches() == [(3, 1, 11, 14)] and ev.worst_frames(1) == [(1, 1, 1, 0)]
    assert ev.frame_errors().tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 1]]
    loaded = E.load_files(gt_root, tracker_dir, seqmap)
    again = loaded.events()[C.TREE_SEQ]
    assert all(np.array_equal(getattr(again, k), getattr(ev, k)) for k in D.SequenceEvents.ARRAYS)


def test_error_frames_on_the_host_are_the_statement(tree, tmp_path):
    args, paths = tree
    ev = D.events_from_files(*args)[C.TREE_SEQ]
    want = C.expected_frame_files(ev, paths, 85, 2, 2)
    written = D.write_error_frames(ev, paths, str(tmp_path / "all"), quality=85, thickness=2, font_scale=2)
    assert [os.path.basename(p) for p in written] == ["00000001.jpg", "00000002.jpg", "00000003.jpg"]
    for t, path in enumerate(written, start=1):
        with open(path, "rb") as f:
            assert f.read() == want[t], t
    with open(paths[1], "rb") as f:                     # the clean frame is drawn into all the same: its matches
        assert f.read() != want[2]
    only = D.write_error_frames(ev, paths, str(tmp_path / "errors"), only_errors=True, quality=85, font_scale=2)
    assert [os.path.basename(p) for p in only] == ["00000001.jpg", "00000003.jpg"]
    assert sorted(os.listdir(tmp_path / "errors")) == ["00000001.jpg", "00000003.jpg"]
    with pytest.raises(ValueError, match="frame paths"):
        D.write_error_frames(ev, paths[:2], str(tmp_path / "bad"))


def test_the_command_line(tree, tmp_path, capsys):
    (gt_root, tracker_dir, seqmap), paths = tree
    out = str(tmp_path / "report")
    assert D.main(["--gt-root", gt_root, "--tracker-dir", tracker_dir, "--seqmap", seqmap, "--out", out,
                   "--frames-root", gt_root, "--only-errors", "--quality", "85", "--font-scale", "2"]) == 0
    assert capsys.readouterr().out.splitlines() == [f"{C.TREE_SEQ} CLR_TP=5 CLR_FN=1 CLR_FP=1 IDSW=1 Frag=0 frames=2"]
    ev = D.SequenceEvents.read_csv(os.path.join(out, C.TREE_SEQ + ".csv"), n_frames=C.TREE_FRAMES)
    fields = E.evaluate_files(gt_root, tracker_dir, seqmap)[C.TREE_SEQ]
    assert ev.counts() == {k: int(fields[k]) for k in D.COUNTS}
    with open(os.path.join(out, "summary.txt")) as f:
        summary = f.read().splitlines()
    assert summary[0] == f"{C.TREE_SEQ} CLR_TP=5 CLR_FN=1 CLR_FP=1 IDSW=1 Frag=0"
    assert summary[1:] == ["  frame 1: FN=1 FP=1 IDSW=0", "  frame 3: FN=0 FP=0 IDSW=1", "  frame 2: FN=0 FP=0 IDSW=0"]
    want = C.expected_frame_files(ev, paths, 85, 2, 2)
    frames = os.path.join(out, C.TREE_SEQ, "frames")
    assert sorted(os.listdir(frames)) == ["00000001.jpg", "00000003.jpg"]
    for t in (1, 3):
        with open(os.path.join(frames, f"{t:08d}.jpg"), "rb") as f:
            assert f.read() == want[t], t
    # misses, false positives and switches are boxed in their colours: the outline's corner pixel, as decoded
    from memotr_amd.data.jpeg import decode_jpeg
    px = decode_jpeg(os.path.join(frames, "00000001.jpg"), "cpu").numpy().astype(int)
    near = lambda p, c: np.abs(p - np.array(c)).max() < 60                                       # noqa: E731
    # (pixels on the left or right edge of a box, two pixels wide on even columns: one chroma sample)
    assert near(px[30, 78], D.COLOURS[D.MISS]) and near(px[9, 70], D.COLOURS[D.FP]) and near(px[34, 10], D.COLOURS[D.TP])
    px = decode_jpeg(os.path.join(frames, "00000003.jpg"), "cpu").numpy().astype(int)
    assert near(px[34, 10], D.COLOURS[D.SWITCH])


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_the_entries_are_declared_and_the_abi_stays_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert "clipops_clear_events_f64" in declared and "clipops_error_table_f64" in declared
    assert clip_lib.ABI_VERSION == 12 and clip_lib.lib.clipops_abi_version() == 12
    names = ("KIND_IGNORED", "KIND_MATCH", "KIND_SWITCH", "KIND_MISS", "KIND_FP", "EVENT_SWITCH", "EVENT_FRAG")
    assert [define("clip_ops_hip.h", "CLIPOPS_" + n) for n in names] == [D.IGNORED, D.MATCH, D.SWITCH, D.MISS, D.FP,
                                                                        D.EVENT_SWITCH, D.EVENT_FRAG]


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, p = clip_lib.lib, ctypes.c_void_p(64)
    inputs = ("sim", "sim_off", "gt_off", "tr_off", "gt_ids", "tr_ids", "seq_off")
    outputs = ("gt_partner", "gt_flags", "tr_partner", "counts", "status")

    def events(n_seqs=2, max_gt=8, max_tr=8, max_gt_ids=8, **ptrs):
        a = {k: ptrs.get(k, p) for k in inputs + ("n_gt_ids",) + outputs}
        return lib.clipops_clear_events_f64(*[a[k] for k in inputs], n_seqs, a["n_gt_ids"], max_gt, max_tr, max_gt_ids,
                                            *[a[k] for k in outputs], None)

    for kwargs in (dict(n_seqs=-1), dict(max_gt=-1), dict(max_tr=-1), dict(max_gt_ids=-1)):
        assert events(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
    for kwargs in (dict(max_gt=2049), dict(max_tr=2049), dict(max_gt_ids=2049)):
        assert events(**kwargs) == 2 and b"CLIPOPS_EVENTS_MAX_DIM" in lib.clipops_last_error(), kwargs
    for name in inputs + ("n_gt_ids",) + outputs:
        assert events(**{name: None}) == 1 and b"null" in lib.clipops_last_error(), name
    assert events(n_seqs=0, **{k: None for k in inputs + outputs}) == 0 and lib.clipops_last_error() == b""

    arrays = ("gt_boxes", "tr_boxes", "gt_off", "tr_off", "gt_ids", "tr_ids", "gt_kind", "tr_kind")

    def table(n_frames=3, max_rows=4, width=96, height=64, bgr=0, font_scale=1, out=p, **ptrs):
        return lib.clipops_error_table_f64(*[ptrs.get(k, p) for k in arrays], n_frames, max_rows, width, height, bgr,
                                           font_scale, out, None)

    for kwargs in (dict(n_frames=-1), dict(max_rows=-1)):
        assert table(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
    for kwargs in (dict(width=0), dict(height=0), dict(width=65536), dict(height=-4)):
        assert table(**kwargs) == 1 and b"width or height" in lib.clipops_last_error(), kwargs
    for scale in (0, 65, -3):
        assert table(font_scale=scale) == 1 and b"font_scale" in lib.clipops_last_error(), scale
    assert table(n_frames=1 << 20, max_rows=1 << 20) == 1 and b"table rows" in lib.clipops_last_error()
    for name in arrays + ("out",):
        assert table(**{name: None}) == 1 and b"null" in lib.clipops_last_error(), name
    for kwargs in (dict(n_frames=0), dict(max_rows=0)):
        assert table(out=None, **{k: None for k in arrays}, **kwargs) == 0 and lib.clipops_last_error() == b"", kwargs
