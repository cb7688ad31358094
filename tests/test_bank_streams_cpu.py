"""CPU: the per-stream forms of the two track-bank entries (memotr_amd/functions/clip_ops.py: bank_update_streams,
bank_result_rows_streams and their host statements; include/clip_ops_hip.h: clipops_bank_update_streams_f32,
clipops_bank_result_rows_streams_f32).

The host statement of a B = 3 bank under three settings is held to the scalar ``bank_update_reference`` /
``bank_result_rows_reference`` run on each stream as a bank of its own (a copy, not a view) with that stream's values;
the binding is held to the header, and the argument errors of the two entry points are reported without a device."""
import ctypes

import pytest
import torch

from cabi_helpers import assert_binding_matches_header
from test_track_bank_cpu import assert_banks_equal, clone_bank, random_bank, random_outputs

from memotr_amd.functions import clip_ops
from memotr_amd.models.track_bank import ROW_FIELDS, TrackBank
from memotr_amd.results import BankResultLog

SETTINGS = [dict(det_score_thresh=0.7, track_score_thresh=0.45, result_score_thresh=0.6, miss_tolerance=2),
            dict(det_score_thresh=0.3, track_score_thresh=0.8, result_score_thresh=0.3, miss_tolerance=1),
            dict(det_score_thresh=0.9, track_score_thresh=0.2, result_score_thresh=0.85, miss_tolerance=1000,
                 area_thresh=2000)]


def own_bank(bank, b):
    """Stream ``b`` of ``bank`` as a bank of its own: copies."""
    one = TrackBank(1, bank.cap, num_classes=bank.num_classes, hidden_dim=bank.hidden_dim, use_dab=bank.use_dab,
                    device=bank.device)
    for name in ROW_FIELDS + ("next_id", "counters"):
        getattr(one, name).copy_(getattr(bank, name)[b:b + 1])
    return one


def own_outputs(res, b):
    """(views: torch's CPU sigmoid rounds an element by where it stands in its tensor -- test_track_bank_cpu.pitched)"""
    one = {k: v[b:b + 1] for k, v in res.items() if torch.is_tensor(v) and v.dim() == 3}
    one["aux_outputs"] = [dict(queries=res["aux_outputs"][-1]["queries"][b:b + 1])]
    one["det_query_embed"] = res["det_query_embed"]
    return one


@pytest.mark.parametrize("use_dab", [True, False])
def test_the_host_statement_is_the_scalar_statement_on_every_stream_as_its_own_bank(use_dab):
    B, n_det, cap, K = 3, 40, 32, 4
    th = clip_ops.StreamThresholds(SETTINGS, "cpu")
    assert th.det.dtype == th.track.dtype == th.result.dtype == th.area.dtype == torch.float32
    assert th.miss.dtype == torch.int64 and th.miss.tolist() == [2, 1, 1000] and th.area.tolist() == [100, 100, 2000]
    bank = random_bank(B, cap, K, seed=11, use_dab=use_dab)
    singles = [own_bank(bank, b) for b in range(B)]
    shared = clone_bank(bank)                       # every stream under setting 0: what the scalar entry does
    differ = 0
    for frame in range(3):
        res = random_outputs(B, n_det, cap, K, seed=50 + frame, use_dab=use_dab, strided=frame == 1)
        res["pred_logits"][1, 3, 0] = float("nan")                  # a NaN detect row and a NaN track row
        res["pred_logits"][2, n_det + 2, :] = float("nan")
        clip_ops.bank_update_streams(res, bank, th)                 # CPU tensors: bank_update_streams_reference
        clip_ops.bank_update(res, shared, 0.7, 0.45, 2)
        for b, s in enumerate(SETTINGS):
            clip_ops.bank_update_reference(own_outputs(res, b), singles[b], s["det_score_thresh"],
                                           s["track_score_thresh"], s["miss_tolerance"])
            for name in ROW_FIELDS + ("next_id", "counters"):
                x, y = getattr(bank, name)[b:b + 1], getattr(singles[b], name)
                if x.is_floating_point():
                    x, y = x.view(torch.int32), y.view(torch.int32)
                assert torch.equal(x, y), (frame, b, name)
        assert torch.equal(bank.ids[0], shared.ids[0])
        differ += int((bank.ids[1:] != shared.ids[1:]).sum())
    assert differ > 10                              # streams 1 and 2 did not run under setting 0
    assert int(bank.disappear_time[2].max()) >= 2 and int(bank.disappear_time[1].max()) == 0


def test_the_same_setting_on_every_stream_is_the_scalar_statement():
    B, n_det, cap, K = 3, 20, 16, 2
    th = clip_ops.StreamThresholds([SETTINGS[0]] * B, "cpu")
    bank = random_bank(B, cap, K, seed=4)
    want = clone_bank(bank)
    res = random_outputs(B, n_det, cap, K, seed=4)
    clip_ops.bank_update_streams(res, bank, th)
    clip_ops.bank_update_reference(res, want, 0.7, 0.45, 2)
    assert_banks_equal(want, bank)


def test_the_result_rows_of_every_stream_are_the_scalar_rows_of_that_stream():
    B, cap, K = 3, 32, 8
    bank = random_bank(B, cap, K, seed=5)
    bank.boxes.copy_(bank.boxes.sigmoid() * 0.5 * (bank.ids >= 0)[..., None])
    bank.scores.copy_(bank.logits.sigmoid() * (bank.ids >= 0)[..., None])
    settings = [dict(s, result_score_thresh=r, area_thresh=a) for s, r, a in zip(SETTINGS, (0.8, 0.9, 0.85),
                                                                                  (100, 100, 800))]
    th = clip_ops.StreamThresholds(settings, "cpu")
    sizes = [(1080, 1920), (480, 641), (97, 131)]
    ori_wh = torch.tensor([[w, h] for h, w in sizes], dtype=torch.float32)
    log = BankResultLog("cpu", capacity=16)
    singles = [BankResultLog("cpu", capacity=16) for _ in range(B)]
    for frame in range(3):
        seq_frame = torch.tensor([[b, frame] for b in range(B)])
        log.append_streams(bank, seq_frame, ori_wh, th)
        for b, s in enumerate(settings):
            singles[b].append(own_bank(bank, b), seq_frame[b:b + 1], ori_wh[b:b + 1], s["result_score_thresh"],
                              s["area_thresh"])
        bank.scores.mul_(0.95)
    m = int(log.counters[0])
    counts = [int(s.counters[0]) for s in singles]
    assert m == sum(counts) and log.counters[1] == 0 and all(counts) and len(set(counts)) == B
    # the table holds the streams' rows frame by frame, streams in order
    at, starts = 0, [0] * B
    for frame in range(3):
        for b in range(B):
            one = singles[b]
            pick = (one.rows_i[:counts[b], 1] == frame).nonzero().squeeze(1)
            n = int(pick.shape[0])
            assert torch.equal(log.rows_i[at:at + n], one.rows_i[pick]), (frame, b)
            assert torch.equal(log.rows_f[at:at + n].view(torch.int32), one.rows_f[pick].view(torch.int32)), (frame, b)
            at += n
    assert at == m
    for b in range(B):
        assert log.mot_lines(b, "MOT17") == singles[b].mot_lines(b, "MOT17")
    with pytest.raises(ValueError, match="2 settings"):
        log.append_streams(bank, seq_frame, ori_wh, clip_ops.StreamThresholds(SETTINGS[:2], "cpu"))
    with pytest.raises(ValueError, match="lacks"):
        clip_ops.StreamThresholds([dict(det_score_thresh=0.5)], "cpu")
    with pytest.raises(ValueError, match="unknown keys"):
        clip_ops.StreamThresholds([dict(SETTINGS[0], update_thresh=0.5)], "cpu")


# ---------------------------------------------------------------------------------------------- the library
def test_the_binding_matches_the_header_and_the_abi_stays_12(clip_lib):
    declared = assert_binding_matches_header(clip_lib, "clip_ops_hip.h", "clipops", "CLIPOPS_ABI_VERSION")
    assert {"clipops_bank_update_streams_f32", "clipops_bank_result_rows_streams_f32"} <= set(declared)
    assert clip_lib.ABI_VERSION == 12 and clip_lib.lib.clipops_abi_version() == 12


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib, d = clip_lib.lib, 64
    p = ctypes.c_void_p(d)

    def update(B=2, n_det=5, cap=16, K=1, C=8, use_dab=1, model_edit=None, bank_edit=None, model=True, bank=True,
               det=p, track=p, miss=p):
        m, t = clip_lib.BankModel(), clip_lib.Bank()
        for i in range(len(clip_lib.BANK_MODEL)):
            m.ptr[i], m.batch_stride[i], m.row_stride[i] = d, 100, 10
        for name in clip_lib.BANK_FIELDS:
            setattr(t, name, d)
        (model_edit or (lambda m: None))(m)
        (bank_edit or (lambda t: None))(t)
        return lib.clipops_bank_update_streams_f32(ctypes.byref(m) if model else None, ctypes.byref(t) if bank else None,
                                                   B, n_det, cap, K, C, use_dab, det, track, miss, None)

    for kwargs in (dict(B=-1), dict(n_det=-1), dict(cap=-16)):
        assert update(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
        assert lib.clipops_last_error().startswith(b"clipops_bank_update_streams_f32: ")
    assert update(cap=0) == 1 and b"without slots" in lib.clipops_last_error()
    assert update(K=0) == 1 and update(C=0) == 1 and b"K < 1 or C < 1" in lib.clipops_last_error()
    assert update(model=False) == 1 and update(bank=False) == 1 and b"null" in lib.clipops_last_error()
    assert update(model_edit=lambda m: m.ptr.__setitem__(2, None)) == 1 and b"null model" in lib.clipops_last_error()
    assert update(model_edit=lambda m: m.row_stride.__setitem__(0, -1)) == 1 and b"stride" in lib.clipops_last_error()
    assert update(use_dab=0) == 1 and b"det_embed" in lib.clipops_last_error()
    for name in clip_lib.BANK_FIELDS:
        assert update(bank_edit=lambda t, n=name: setattr(t, n, None)) == 1, name
        assert b"null bank" in lib.clipops_last_error()
    for name in ("det", "track", "miss"):
        assert update(**{name: None}) == 1 and b"null threshold array" in lib.clipops_last_error(), name
    assert update(B=0, model=False, bank=False, det=None, track=None, miss=None) == 0
    assert lib.clipops_last_error() == b""

    def rows(boxes=p, scores=p, ids=p, labels=p, B=2, cap=16, K=1, seq_frame=p, ori_wh=p, score=p, area=p, rows_f=p,
             rows_i=p, counters=p, capacity=16):
        return lib.clipops_bank_result_rows_streams_f32(boxes, scores, ids, labels, B, cap, K, seq_frame, ori_wh, score,
                                                        area, rows_f, rows_i, counters, capacity, None)

    for kwargs in (dict(B=-1), dict(cap=-1), dict(capacity=-1)):
        assert rows(**kwargs) == 1 and b"negative" in lib.clipops_last_error(), kwargs
        assert lib.clipops_last_error().startswith(b"clipops_bank_result_rows_streams_f32: ")
    assert rows(K=0) == 1 and b"K < 1" in lib.clipops_last_error()
    assert rows(B=1 << 20, cap=1 << 20) == 1 and b"slots" in lib.clipops_last_error()
    for name in ("boxes", "scores", "ids", "labels", "seq_frame", "ori_wh", "rows_f", "rows_i", "counters"):
        assert rows(**{name: None}) == 1 and b"null pointer" in lib.clipops_last_error(), name
    for name in ("score", "area"):
        assert rows(**{name: None}) == 1 and b"null threshold array" in lib.clipops_last_error(), name
    assert rows(B=0, boxes=None, counters=None, score=None, area=None) == 0 and lib.clipops_last_error() == b""
    with pytest.raises(RuntimeError, match="null threshold array"):
        clip_lib.check(rows(area=None), "clipops_bank_result_rows_streams_f32")
