"""CPU: the track bank (memotr_amd/models/track_bank.py) and the host statements of its two kernels
(memotr_amd/functions/clip_ops.py: bank_update_reference, bank_result_rows_reference).

The bank update is held to ``RuntimeTracker.update`` + the inference branch of ``QueryUpdater.select_active_tracks``
applied stream by stream, over several frames of births, misses and retirements: the live ids, labels, disappear_time and
every carried field are equal, matched by id.  Scores at their thresholds, NaN scores, label ties, a full bank, the
dropped-birth counter, ``reset_stream`` and ``grow``; the result rows against ``ResultLog``'s per stream; the argument
errors of the two entry points through the C ABI and the binding against the header.  ``random_outputs`` /
``random_bank`` are shared with tests/test_track_bank_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from cabi_helpers import assert_binding_matches_header

from memotr_amd.functions import clip_ops
from memotr_amd.models.query_updater import QueryUpdater
from memotr_amd.models.runtime_tracker import RuntimeTracker
from memotr_amd.models.track_bank import ROW_FIELDS, TrackBank
from memotr_amd.results import BankResultLog, ResultLog
from memotr_amd.structures.track_instances import TrackInstances

C = 8
DET_T, TRACK_T, MISS = 0.7, 0.45, 2
CARRIED = ("ids", "labels", "disappear_time", "boxes", "ref_pts", "logits", "scores", "output_embed", "long_memory",
           "last_output", "query_embed")


def random_outputs(B, n_det, cap, K, seed, use_dab=True, birth_rate=0.2, C=C, device="cpu", strided=False):
    """Decoder outputs for queries cat(det, slots): logits such that about ``birth_rate`` of the detect rows are born
    and a third of the tracks are missed.  ``strided``: every tensor is a column / row / batch slice of a larger one."""
    g = torch.Generator().manual_seed(seed)
    n = n_det + cap

    def make(width, scale=1.0, shift=0.0):
        if not strided:
            return (torch.randn(B, n, width, generator=g) * scale + shift).to(device)
        big = torch.randn(B + 1, n + 3, width + 5, generator=g) * scale + shift
        return big.to(device)[1:, 2:2 + n, 3:3 + width]

    logits = make(K, 2.0, -1.5 if birth_rate < 0.5 else 1.5)
    res = dict(pred_logits=logits, pred_bboxes=make(4).sigmoid() if not strided else make(4), outputs=make(C),
               last_ref_pts=make(4), aux_outputs=[dict(queries=make(C))],
               det_query_embed=torch.randn(n_det, 2 * C + 3, generator=g).to(device)[:, :2 * C])
    return res


def random_bank(B, cap, K, seed, pattern="alternating", use_dab=True, C=C, device="cpu"):
    """A bank whose slots hold random tracks where ``pattern`` says so: "alternating", "all" (none free), "none"."""
    g = torch.Generator().manual_seed(seed)
    bank = TrackBank(B, cap, num_classes=K, hidden_dim=C, use_dab=use_dab, device="cpu")
    live = torch.zeros(B, cap, dtype=torch.bool)
    if pattern == "alternating":
        live[:, ::2] = True
    elif pattern == "all":
        live[:] = True
    for b in range(B):
        n = int(live[b].sum())
        ids = torch.randperm(3 * cap, generator=g)[:n]
        bank.ids[b][live[b]] = ids
        bank.next_id[b] = 3 * cap
        bank.labels[b][live[b]] = torch.randint(0, K, (n,), generator=g)
        bank.disappear_time[b][live[b]] = torch.randint(0, MISS, (n,), generator=g)
        for name in ROW_FIELDS[3:]:
            t = getattr(bank, name)
            t[b][live[b]] = torch.randn(n, t.shape[2], generator=g)
        bank.counters[b, 0] = n
    if device != "cpu":
        for name in ROW_FIELDS + ("next_id", "counters", "free_list"):
            setattr(bank, name, getattr(bank, name).to(device))
        bank.device = torch.device(device)
    return bank


def clone_bank(bank):
    other = TrackBank(bank.n_streams, bank.cap, num_classes=bank.num_classes, hidden_dim=bank.hidden_dim,
                      use_dab=bank.use_dab, device=bank.device)
    for name in ROW_FIELDS + ("next_id", "counters"):
        getattr(other, name).copy_(getattr(bank, name))
    return other


def assert_banks_equal(a, b, fields=ROW_FIELDS + ("next_id", "counters")):
    for name in fields:
        x, y = getattr(a, name).cpu(), getattr(b, name).cpu()
        if x.is_floating_point():           # bit for bit, NaN included
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), name


# ---------------------------------------------------------------------------------------------- against the tracker
def pitched(t):
    """``t`` as a column slice of a wider tensor.  torch's CPU sigmoid runs a vector routine over the body of a dense
    tensor and the scalar one over its last few elements, and the two differ in the last bit: the score of a logit then
    depends on where it stands in its tensor.  The tracker and the host statement take the sigmoid of differently shaped
    tensors, so the comparison below is made on pitched tensors, where every element goes through the scalar routine."""
    wide = t.new_zeros(t.shape[:-1] + (t.shape[-1] + 1,))
    wide[..., :-1] = t
    return wide[..., :-1]


def tracker_step(rt, updater, res, tracks):
    """``RuntimeTracker.update`` + the inference branch of ``select_active_tracks`` on one stream's outputs."""
    return updater.select_active_tracks(*rt.update(model_outputs=res, tracks=[tracks]), None)[0]


@pytest.mark.parametrize("use_dab", [True, False])
@pytest.mark.parametrize("K", [1, 8])
def test_the_host_statement_is_the_runtime_tracker_stream_by_stream(K, use_dab):
    # (without DAB the runtime tracker takes the first 256 columns of det_query_embed: the hidden size it is written for)
    B, n_det, cap, frames, C = 3, 20, 96, 6, (8 if use_dab else 256)
    bank = TrackBank(B, cap, num_classes=K, hidden_dim=C, use_dab=use_dab)
    updater = QueryUpdater(hidden_dim=C, ffn_dim=16, tp_drop_ratio=0.0, fp_insert_ratio=0.0, dropout=0.0,
                           use_checkpoint=False, use_dab=use_dab, update_threshold=0.5, long_memory_lambda=0.01).eval()
    trackers = [RuntimeTracker(det_score_thresh=DET_T, track_score_thresh=TRACK_T, miss_tolerance=MISS,
                               use_dab=use_dab) for _ in range(B)]
    tracks = [TrackInstances(hidden_dim=C, num_classes=K, use_dab=use_dab) for _ in range(B)]
    born = retired = missed = 0
    for frame in range(frames):
        res = random_outputs(B, n_det, cap, K, seed=100 * K + frame, use_dab=use_dab, C=C, strided=True)
        before = [set(t.ids.tolist()) for t in tracks]
        # the one-sequence tracker sees its tracks as rows n_det .. n_det + n: gather them from their slots
        for b in range(B):
            ids = bank.ids[b]
            slot_of = {int(i): s for s, i in enumerate(ids.tolist()) if i >= 0}
            slots = torch.tensor([slot_of[i] for i in tracks[b].ids.tolist()], dtype=torch.long)
            rows = torch.cat((torch.arange(n_det), n_det + slots))
            one = dict(pred_logits=pitched(res["pred_logits"][b:b + 1, rows]),
                       pred_bboxes=res["pred_bboxes"][b:b + 1, rows], outputs=res["outputs"][b:b + 1, rows],
                       last_ref_pts=res["last_ref_pts"][b:b + 1, rows],
                       aux_outputs=[dict(queries=res["aux_outputs"][-1]["queries"][b:b + 1, rows])],
                       det_query_embed=res["det_query_embed"])
            tracks[b] = tracker_step(trackers[b], updater, one, tracks[b])
        clip_ops.bank_update(res, bank, DET_T, TRACK_T, MISS)
        for b in range(B):
            got, want = bank.stream_tracks(b), tracks[b]
            order = torch.argsort(want.ids)
            for name in CARRIED:
                assert torch.equal(got[name], getattr(want, name)[order]), (frame, b, name)
            assert int(bank.next_id[b]) == trackers[b].max_obj_id
            assert bank.counters[b].tolist() == [len(want), 0]
            after = set(want.ids.tolist())
            born, retired = born + len(after - before[b]), retired + len(before[b] - after)
            missed += int((want.disappear_time > 0).sum())
        # free slots hold zeros
        free = bank.ids < 0
        for name in ROW_FIELDS[1:]:
            assert not getattr(bank, name)[free].any(), name
    assert born > 20 and retired > 5 and missed > 5


# ---------------------------------------------------------------------------------------------- edges
def one_stream(det_scores, track_scores=(), labels=(), disappear=(), cap=16, K=None):
    """A bank of one stream whose first slots hold tracks, and outputs with the given SCORES (logits are set so that
    torch's sigmoid gives exactly these float32 values where that matters to a test: 0.5)."""
    K = len(det_scores[0]) if K is None else K
    n_det, n_tr = len(det_scores), len(track_scores)
    bank = TrackBank(1, cap, num_classes=K, hidden_dim=C)
    bank.ids[0, :n_tr] = torch.arange(n_tr)
    bank.next_id[0] = n_tr
    bank.labels[0, :n_tr] = torch.tensor(labels, dtype=torch.long)
    bank.disappear_time[0, :n_tr] = torch.tensor(disappear, dtype=torch.long)
    res = random_outputs(1, n_det, cap, K, seed=1)
    to_logit = lambda rows: torch.special.logit(torch.tensor(rows, dtype=torch.float64)).float()    # noqa: E731
    res["pred_logits"][0, :n_det] = to_logit(det_scores)
    res["pred_logits"][0, n_det:] = -20.0
    if n_tr:
        res["pred_logits"][0, n_det:n_det + n_tr] = to_logit(track_scores)
    return bank, res


def test_a_score_equal_to_its_threshold_is_born_and_is_not_missed():
    bank, res = one_stream([(0.5,), (0.25,)], track_scores=[(0.5,), (0.25,)], labels=[0, 0], disappear=[0, 0])
    assert float(res["pred_logits"][0, 0].sigmoid()) == 0.5
    clip_ops.bank_update(res, bank, 0.5, 0.5, 5)
    assert bank.ids[0, :4].tolist() == [0, 1, 2, -1]            # >= : born at the threshold
    assert bank.disappear_time[0, :3].tolist() == [0, 1, 0]     # < : not missed at the threshold
    assert bank.counters[0].tolist() == [3, 0] and int(bank.next_id[0]) == 3


def test_nan_scores_are_never_born_and_do_not_age_a_track():
    nan = float("nan")
    bank, res = one_stream([(0.9, 0.1), (0.9, 0.1), (0.9, 0.1)], track_scores=[(0.9, 0.9)], labels=[1], disappear=[1])
    res["pred_logits"][0, 0, 1] = nan                           # a NaN wins torch's max and fails the comparison
    res["pred_logits"][0, 1, 0] = nan
    res["pred_logits"][0, 3, 1] = nan                           # the track's own score
    clip_ops.bank_update(res, bank, 0.5, 0.5, 5)
    assert bank.ids[0, :3].tolist() == [0, 1, -1] and bank.counters[0].tolist() == [2, 0]
    assert bank.disappear_time[0, 0] == 0 and torch.isnan(bank.scores[0, 0, 1])
    assert torch.equal(bank.logits[0, 1], res["pred_logits"][0, 2])


def test_label_ties_take_the_lowest_index():
    bank, res = one_stream([(0.25, 0.75, 0.75, 0.5), (0.75, 0.75, 0.75, 0.75), (0.25, 0.25, 0.5, 0.75)])
    clip_ops.bank_update(res, bank, 0.5, 0.5, 5)
    assert bank.labels[0, :3].tolist() == [1, 0, 3] and bank.ids[0, :3].tolist() == [0, 1, 2]


def test_births_fill_the_free_slots_in_order_and_the_rest_is_counted():
    K, cap, n_det = 1, 16, 12
    bank = random_bank(1, cap, K, seed=3, pattern="alternating")        # 8 free slots: 1, 3, ..., 15
    res = random_outputs(1, n_det, cap, K, seed=3)
    res["pred_logits"][0, :n_det] = 3.0                                 # twelve births
    res["pred_logits"][0, n_det:] = 3.0                                 # nobody is missed
    exact = clone_bank(bank)
    res_8 = {k: v for k, v in res.items()}
    res_8["pred_logits"] = res["pred_logits"].clone()
    res_8["pred_logits"][0, 8:n_det] = -3.0                             # exactly as many births as free slots
    clip_ops.bank_update(res_8, exact, DET_T, TRACK_T, MISS)
    assert exact.counters[0].tolist() == [16, 0] and int(exact.next_id[0]) == 3 * cap + 8
    assert exact.ids[0, 1::2].tolist() == list(range(3 * cap, 3 * cap + 8))
    exact.check()
    clip_ops.bank_update(res, bank, DET_T, TRACK_T, MISS)
    assert bank.counters[0].tolist() == [16, 4] and int(bank.next_id[0]) == 3 * cap + 8
    assert bank.ids[0, 1::2].tolist() == list(range(3 * cap, 3 * cap + 8))           # the first eight, in row order
    assert torch.equal(bank.boxes[0, 1::2], res["pred_bboxes"][0, :8])
    with pytest.raises(RuntimeError, match="stream 0 dropped 4 births"):
        bank.check()
    clip_ops.bank_update(res_8, bank, DET_T, TRACK_T, MISS)             # a full bank: the counter is sticky and grows
    assert bank.counters[0].tolist() == [16, 12]


def test_a_slot_freed_in_this_frame_is_reused_from_the_next_frame_on():
    bank, res = one_stream([(0.9,), (0.9,)], track_scores=[(0.1,)] * 16, labels=[0] * 16, disappear=[MISS - 1] * 16)
    clip_ops.bank_update(res, bank, DET_T, TRACK_T, MISS)               # all sixteen retire; no slot was free
    assert (bank.ids[0] == -1).all() and bank.counters[0].tolist() == [0, 2] and int(bank.next_id[0]) == 16
    for name in ROW_FIELDS[1:]:
        assert not getattr(bank, name).any(), name
    bank.counters[0, 1] = 0
    clip_ops.bank_update(res, bank, DET_T, TRACK_T, MISS)
    assert bank.ids[0, :3].tolist() == [16, 17, -1] and bank.counters[0].tolist() == [2, 0]


def test_reset_stream_grow_and_check_name_the_stream():
    bank = random_bank(3, 16, 2, seed=8, pattern="all")
    bank.counters[2, 1] = 5
    with pytest.raises(RuntimeError, match="stream 2 dropped 5 births"):
        bank.check()
    keep = clone_bank(bank)
    bank.reset_stream(2)
    bank.check()
    assert (bank.ids[2] == -1).all() and int(bank.next_id[2]) == 0 and bank.counters[2].tolist() == [0, 0]
    for name in ROW_FIELDS[1:]:
        assert not getattr(bank, name)[2].any() and torch.equal(getattr(bank, name)[:2], getattr(keep, name)[:2]), name
    assert bank.query_mask().shape == (3, 16) and bank.query_mask()[2].all() and not bank.query_mask()[:2].any()
    bank.grow(48)
    assert bank.cap == 48 and bank.ids.shape == (3, 48) and bank.query_embed.shape == (3, 48, C)
    for name in ROW_FIELDS:
        t = getattr(bank, name)
        assert torch.equal(t[:2, :16], getattr(keep, name)[:2]) and t.is_contiguous(), name
        assert (t[:, 16:] == (-1 if name == "ids" else 0)).all(), name
    assert torch.equal(bank.next_id[:2], keep.next_id[:2]) and bank.free_list.shape == (3, 48)
    bank.move_stream(0, 2)
    assert torch.equal(bank.ids[2], bank.ids[0]) and torch.equal(bank.output_embed[2], bank.output_embed[0])
    bank.shrink(2)
    assert bank.n_streams == 2 and bank.ids.shape == (2, 48)
    for bad in (0, 8, 20):
        with pytest.raises(ValueError, match="multiple of 16"):
            TrackBank(1, bad)
    with pytest.raises(ValueError, match="does not shrink"):
        bank.grow(16)
    with pytest.raises(IndexError):
        bank.reset_stream(2)


def test_wrong_model_outputs_are_refused():
    bank = TrackBank(2, 16, num_classes=2, hidden_dim=C)
    res = random_outputs(2, 5, 16, 2, seed=0)
    with pytest.raises(ValueError, match="outputs has shape"):
        clip_ops.bank_update(dict(res, outputs=res["outputs"][:, :-1]), bank, DET_T, TRACK_T, MISS)
    with pytest.raises(ValueError, match="pred_logits has shape"):
        clip_ops.bank_update(dict(res, pred_logits=res["pred_logits"].double()), bank, DET_T, TRACK_T, MISS)
    with pytest.raises(ValueError, match="model rows for a bank"):
        clip_ops.bank_update({k: (v[:, :10] if torch.is_tensor(v) and v.dim() == 3 else v) for k, v in res.items()},
                             bank, DET_T, TRACK_T, MISS)


# ---------------------------------------------------------------------------------------------- result rows
def test_the_result_rows_are_result_logs_stream_by_stream():
    B, cap, K = 3, 32, 8
    bank = random_bank(B, cap, K, seed=5)
    bank.boxes.copy_(bank.boxes.sigmoid() * 0.5 * (bank.ids >= 0)[..., None])
    bank.scores.copy_(bank.logits.sigmoid() * (bank.ids >= 0)[..., None])
    sizes = [(1080, 1920), (480, 641), (97, 131)]
    log = BankResultLog("cpu", capacity=16)
    singles = [ResultLog("cpu") for _ in range(B)]
    for frame in range(3):
        seq_frame = torch.tensor([[7 + b, frame + b] for b in range(B)])
        ori_wh = torch.tensor([[w, h] for h, w in sizes], dtype=torch.float32)
        log.append(bank, seq_frame, ori_wh, 0.85, 100)
        for b in range(B):
            t = bank.stream_tracks(b)                                   # id order: the one-sequence tracker's
            singles[b].append(t["boxes"], t["scores"], t["ids"], t["labels"], frame + b, *sizes[b], 0.85, 100)
        bank.scores.mul_(0.9)
    rows = log.read()
    assert sorted(rows) == [7, 8, 9] and log.capacity >= 3 * B * cap
    for b in range(B):
        want, got = singles[b].read(), rows[7 + b]
        assert 0 < len(want.ids) < 3 * cap // 2
        for x, y in zip(want, got):
            assert np.array_equal(x, y) and x.dtype == y.dtype
        assert log.mot_lines(7 + b, "MOT17") == singles[b].mot_lines("MOT17")
    # capacity rule: rows past the table are counted, and reading says so
    small_f, small_i = torch.zeros(4, 5), torch.zeros(4, 4, dtype=torch.int64)
    counters = torch.zeros(2, dtype=torch.int32)
    clip_ops.bank_result_rows(bank, seq_frame, ori_wh, -1.0, -1.0, small_f, small_i, counters)
    assert counters.tolist() == [4, B * cap // 2 - 4] and small_i[:, 0].tolist() == [7] * 4
    log.counters[1] = 3
    log._rows = None
    with pytest.raises(RuntimeError, match="3 rows found no room"):
        log.read()
    with pytest.raises(ValueError, match="seq_frame"):
        clip_ops.bank_result_rows(bank, seq_frame[:2], ori_wh, 0.5, 100, small_f, small_i, counters)


# ---------------------------------------------------------------------------------------------- the library
def test_the_binding_matches_the_header_and_the_abi_stays_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert {"clipops_bank_update_f32", "clipops_bank_result_rows_f32"} <= set(declared)
    assert clip_lib.ABI_VERSION == 12 and clip_lib.lib.clipops_abi_version() == 12
    assert ctypes.sizeof(clip_lib.Bank) == 8 * len(clip_lib.BANK_FIELDS)
    assert ctypes.sizeof(clip_lib.BankModel) == 8 * (3 * len(clip_lib.BANK_MODEL) + 2)


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, d = clip_lib.lib, 64

    def update(B=2, n_det=5, cap=16, K=1, C=8, use_dab=1, model_edit=None, bank_edit=None, model=True, bank=True):
        m, t = clip_lib.BankModel(), clip_lib.Bank()
        for i in range(len(clip_lib.BANK_MODEL)):
            m.ptr[i], m.batch_stride[i], m.row_stride[i] = d, 100, 10
        for name in clip_lib.BANK_FIELDS:
            setattr(t, name, d)
        (model_edit or (lambda m: None))(m)
        (bank_edit or (lambda t: None))(t)
        return lib.clipops_bank_update_f32(ctypes.byref(m) if model else None, ctypes.byref(t) if bank else None, B,
                                           n_det, cap, K, C, use_dab, 0.5, 0.5, 5, None)

    for kwargs in (dict(B=-1), dict(n_det=-1), dict(cap=-16)):
        assert update(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
    assert update(cap=0) == 1 and b"without slots" in lib.clipops_last_error()
    assert update(K=0) == 1 and update(C=0) == 1 and b"K < 1 or C < 1" in lib.clipops_last_error()
    assert update(model=False) == 1 and update(bank=False) == 1 and b"null" in lib.clipops_last_error()
    assert update(model_edit=lambda m: m.ptr.__setitem__(2, None)) == 1 and b"null model" in lib.clipops_last_error()
    assert update(model_edit=lambda m: m.row_stride.__setitem__(0, -1)) == 1 and b"stride" in lib.clipops_last_error()
    assert update(use_dab=0) == 1 and b"det_embed" in lib.clipops_last_error()
    for name in clip_lib.BANK_FIELDS:
        assert update(bank_edit=lambda t, n=name: setattr(t, n, None)) == 1, name
        assert b"null bank" in lib.clipops_last_error()
    assert update(B=0, model=False, bank=False) == 0 and lib.clipops_last_error() == b""

    p = ctypes.c_void_p(d)

    def rows(boxes=p, scores=p, ids=p, labels=p, B=2, cap=16, K=1, seq_frame=p, ori_wh=p, rows_f=p, rows_i=p,
             counters=p, capacity=16):
        return lib.clipops_bank_result_rows_f32(boxes, scores, ids, labels, B, cap, K, seq_frame, ori_wh, 0.5, 100.0,
                                                rows_f, rows_i, counters, capacity, None)

    for kwargs in (dict(B=-1), dict(cap=-1), dict(capacity=-1)):
        assert rows(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
    assert rows(K=0) == 1 and b"K < 1" in lib.clipops_last_error()
    assert rows(B=1 << 20, cap=1 << 20) == 1 and b"slots" in lib.clipops_last_error()
    for name in ("boxes", "scores", "ids", "labels", "seq_frame", "ori_wh", "rows_f", "rows_i", "counters"):
        assert rows(**{name: None}) == 1 and b"null" in lib.clipops_last_error(), name
    assert rows(B=0, boxes=None, counters=None) == 0 and lib.clipops_last_error() == b""
    with pytest.raises(RuntimeError, match="null pointer"):
        clip_lib.check(rows(ids=None), "clipops_bank_result_rows_f32")
