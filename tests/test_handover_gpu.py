"""MI355X: the hand-over kernels (clipops_handover_fwd_f32 / _bwd_f32 behind ClipCriterion.finish_tracks with state["handover"])
against the composed path finish_tracks -> select_active_tracks on the device: every field and every gradient bit for bit
(the forward copies, the backward sums at most two terms per element)."""
import ctypes

import pytest
import torch

from handover_cases import C, CASES, CASE_IDS, active_set, assert_same_grads, assert_same_tracks, backward_through
from memotr_amd.functions import clip_ops


@pytest.fixture(scope="module")
def composed():
    """The composed path's active set and gradients on the device, once per case."""
    cache = {}

    def get(case):
        if case not in cache:
            tracks, leaves, fused = active_set(case, torch.device("cuda"), fused=False)
            assert not fused
            cache[case] = (tracks, backward_through(tracks, leaves))
        return cache[case]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_kernels_equal_the_composed_path(case, composed):
    want, want_grads = composed(case)
    got, leaves, fused = active_set(case, torch.device("cuda"), fused=True)
    assert fused
    assert_same_tracks(got, want)
    assert got._packed_base() is not None
    grads = backward_through(got, leaves)
    # logits, boxes (and the auxiliary layer, which the hand-over does not read) take no gradient from either route
    for name in ("pred_logits", "pred_bboxes", "aux_logits", "aux_bboxes"):
        assert grads[name] is None and (want_grads[name] is None or not bool(want_grads[name].any()))
    reached = {"outputs", "queries", "last_ref_pts", "init_ref_pts"} | ({"det_query_embed"} if not case[4] else set()) | \
        ({"prev_ref_pts", "prev_long_memory", "prev_last_output", "prev_query_embed"} if case[1] else set())
    assert {k for k, g in grads.items() if g is not None} == reached
    assert_same_grads(grads, want_grads)


@pytest.mark.gpu
def test_the_kernels_equal_the_torch_formulation_of_the_same_contract():
    """Node level: clip_ops.handover against clip_ops.handover_reference on the same tensors and table."""
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(3)
    nd, n_tr, n_gt, K, n_q = 8, 4, 3, 2, 8 + 4 + 2             # two padded query slots behind the live ones
    new_q, new_g, free_q, keep = [1, 6], [2, 0], [0, 2, 3, 4, 5, 7], [0, 2, 3, 4, 5, 7, 11]
    tables = torch.as_tensor(clip_ops.handover_tables(nd, n_q, n_tr, new_q, new_g, free_q, keep)).to(dev)
    rn = lambda *s: torch.randn(*s, generator=gen).to(dev)                                        # noqa: E731
    boxes = (0.2 + 0.2 * torch.rand(n_q, 4, generator=gen)).to(dev)
    gt_boxes = boxes[[6, 9, 1]] + 0.01
    for use_dab in (True, False):
        QW = C if use_dab else 2 * C
        values = [rn(n_q, C), rn(n_q, C), rn(n_q, 4), rn(n_q, 4), None if use_dab else rn(nd, QW), rn(n_tr, 4),
                  rn(n_tr, C), rn(n_tr, C), rn(n_tr, QW)]
        rest = (rn(n_q, K), boxes, torch.rand(n_tr, generator=gen).to(dev), torch.tensor([5, -1, 7, 8], device=dev),
                torch.tensor([1, -1, -1, 0], device=dev), gt_boxes, torch.tensor([40, 41, 42], device=dev), tables,
                len(keep), nd)
        weight = rn(len(keep), K + 8 + 3 * C + QW + 1)
        results = []
        for fn in (clip_ops.handover, clip_ops.handover_reference):
            diff = [None if v is None else v.clone().requires_grad_(True) for v in values]
            base, ids, matched = fn(*diff, *rest)
            grads = torch.autograd.grad((base * weight).sum(), [t for t in diff if t is not None])
            results.append((base, ids, matched) + grads)
        for a, b in zip(*results):
            assert a.shape == b.shape and torch.equal(a, b)


@pytest.mark.gpu
def test_a_table_row_that_points_nowhere_gives_zeros():
    dev = torch.device("cuda")
    nd, n_tr, n_gt, K = 4, 2, 2, 1
    z = lambda *s: torch.ones(*s, device=dev)                                                    # noqa: E731
    table = torch.tensor([[0, 2, -1], [1, 4, 0], [1, 0, 2], [2, -1, -1], [3, 0, 0], [0, 1, -1], [1, 3, 1]], device=dev)
    tables = torch.cat((table.reshape(-1), torch.full((nd + n_tr + n_tr,), -1, device=dev)))
    prev_matched = torch.tensor([0, 2], device=dev)             # track 1 owns a ground truth that does not exist
    base, ids, matched = clip_ops.handover(z(6, C), z(6, C), z(6, 4), z(6, 4), None, z(2, 4), z(2, C), z(2, C), z(2, C),
                                           z(6, K), z(6, 4), z(2), torch.tensor([7, 8], device=dev), prev_matched,
                                           z(n_gt, 4), torch.tensor([5, 6], device=dev), tables, 7, nd)
    assert not bool(base[:6].any()) and ids[:6].tolist() == [-1] * 6 and matched[:6].tolist() == [-1] * 6
    assert bool((base[6] == 1).all()) and ids[6].item() == 6 and matched[6].item() == 1


@pytest.mark.gpu
def test_an_empty_active_set_takes_the_composed_path_on_the_device():
    tracks, _, fused = active_set((8, 0, 3, 1, True, False), torch.device("cuda"), fused=True, empty_active=True)
    assert not fused and tracks.ids.tolist() == [-2]


@pytest.mark.gpu
def test_the_switch_takes_the_composed_path_on_the_device(monkeypatch, composed):
    monkeypatch.setenv("MEMOTR_FUSED_HANDOVER", "0")
    tracks, _, fused = active_set(CASES[2], torch.device("cuda"), fused=True)
    assert not fused
    assert_same_tracks(tracks, composed(CASES[2])[0])


@pytest.mark.gpu
def test_a_clip_step_takes_the_fused_route_and_computes_what_the_composed_one_does(monkeypatch, hip_lib):
    """engine.clip_forward_backward on the golden model of tests/test_model_gpu.py (decoder and updater graphs on, a
    threshold that keeps some unclaimed detections and drops others): with the hand-over nothing is concatenated or
    selected, the last frame gathers nothing, and the active sets, the loss and every parameter gradient that
    does not pass through float atomics are those of the composed route."""
    from memotr_amd.engine import clip_forward_backward
    from memotr_amd.models.criterion import build as build_criterion
    from memotr_amd.models.query_updater import QueryUpdater
    from memotr_amd.structures.track_instances import TrackInstances
    from model_helpers import load_model_golden, small_config, t
    from test_model_gpu import build_memotr_cuda
    g = load_model_golden("M6_train_step")
    T = 3
    batch = {"imgs": [[t(g[f"img{i}"]).cuda() for i in range(T)]],
             "infos": [[{"ids": t(g[f"gt{i}_ids"]).cuda(), "labels": torch.zeros(6, dtype=torch.long).cuda(),
                         "boxes": t(g[f"gt{i}_boxes"]).cuda()} for i in range(T)]]}
    results = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MEMOTR_FUSED_HANDOVER", mode)
        model = build_memotr_cuda(g).train()
        model.query_updater.update_threshold = 0.50915       # scores of this model: 0.5085-0.5093
        model.encode_chunks = "all"
        cfg = small_config()
        cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
                   LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3, 4, 5])
        criterion = build_criterion(cfg)
        calls, sets = {"gathers": 0, "composed": 0}, []
        gather, cat_packed = clip_ops.handover, TrackInstances.cat_packed
        update = QueryUpdater.update_tracks_embedding

        def spy_gather(*a):
            calls["gathers"] += 1
            return gather(*a)

        def spy_cat(*parts):
            calls["composed"] += 1
            return cat_packed(*parts)

        def spy_update(self, tracks, **k):
            sets.append({name: getattr(tracks[0], name).detach().clone()
                         for name in ("ids", "matched_idx") + type(tracks[0]).PACKED_FLOAT})
            return update(self, tracks, **k)

        monkeypatch.setattr(clip_ops, "handover", spy_gather)
        monkeypatch.setattr(TrackInstances, "cat_packed", staticmethod(spy_cat))
        monkeypatch.setattr(QueryUpdater, "update_tracks_embedding", spy_update)
        loss, _ = clip_forward_backward(model, criterion, batch, torch.device("cuda"))
        monkeypatch.setattr(clip_ops, "handover", gather)
        monkeypatch.setattr(TrackInstances, "cat_packed", staticmethod(cat_packed))
        monkeypatch.setattr(QueryUpdater, "update_tracks_embedding", update)
        assert calls == ({"gathers": T - 1, "composed": 0} if mode == "1" else {"gathers": 0, "composed": T - 1})
        results[mode] = (loss.detach().clone(), sets,
                         {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    (l1, s1, g1), (l0, s0, g0) = results["1"], results["0"]
    assert len(s1) == len(s0) == T - 1
    # The node is held to the composed path bit for bit above.  Two clip steps of ONE process are not bit-equal even on one
    # route: the deformable-attention operator chooses its kernels per call site from what earlier calls measured, and its
    # backward accumulates with float atomics.  So: identities exact, values to float32 rounding of a few operations
    # (the sibling test's 1e-6), gradients to 1e-3 of the tensor's largest element (a lost path would be of order 1).
    for a, b in zip(s1, s0):
        for name in a:
            assert a[name].shape == b[name].shape, name
            if a[name].dtype == torch.int64:
                assert torch.equal(a[name], b[name]), name
            else:
                torch.testing.assert_close(a[name], b[name], rtol=1e-6, atol=1e-6, msg=name)
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0)
    assert g1.keys() == g0.keys()
    for n in g1:
        assert float((g1[n] - g0[n]).abs().max()) <= 1e-3 * float(g0[n].abs().max()) + 1e-7, n


def test_argument_errors_are_reported_without_a_device(clip_lib):
    lib = clip_lib.lib
    dummy = ctypes.c_void_p(16)
    src, grads = clip_lib.HandoverSources(), clip_lib.HandoverGrads()
    fwd = lambda s, n_keep=1, n_det=2, K=1, table=dummy: lib.clipops_handover_fwd_f32(                 # noqa: E731
        s, None, None, dummy, dummy, table, n_keep, n_det, 0, 1, K, 4, 1, dummy, dummy, dummy, None)
    assert fwd(ctypes.byref(src)) != 0 and b"null source" in lib.clipops_last_error()
    assert fwd(None) != 0 and b"null pointer" in lib.clipops_last_error()
    assert fwd(ctypes.byref(src), n_keep=-1) != 0 and b"negative" in lib.clipops_last_error()
    assert fwd(ctypes.byref(src), K=0) != 0
    assert fwd(ctypes.byref(src), n_keep=0) == 0                 # an empty set is fine and launches nothing
    bwd = lambda g, n_q=4, n_det=2, n_tr=0: lib.clipops_handover_bwd_f32(                         # noqa: E731
        dummy, dummy, dummy, None, 1, n_q, n_det, n_tr, 1, 4, 1, 0, g, None)
    assert bwd(None) != 0 and b"null pointer" in lib.clipops_last_error()
    assert bwd(ctypes.byref(grads), n_q=1) != 0 and b"n_q" in lib.clipops_last_error()
    grads.ptr[0] = 16                                            # a gradient for the logits
    assert bwd(ctypes.byref(grads)) != 0 and b"no gradient" in lib.clipops_last_error()
    assert bwd(ctypes.byref(clip_lib.HandoverGrads()), n_q=0, n_det=0) == 0
