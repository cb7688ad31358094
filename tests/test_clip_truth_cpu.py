"""CPU: the float64 truth helpers of tests/clip_truth.py restate the project's own formulas (each is pinned to the
``*_reference`` / module formulation of memotr_amd run in float64, to 1e-12 of the output scale), and the inputs of
tests/test_clip_ops_truth_gpu.py meet the conditions their cases rely on -- checked here, before anything reaches a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import clip_truth as T

clip_ops = None


@pytest.fixture(scope="module", autouse=True)
def _package(hip_lib, clip_lib):
    global clip_ops
    from memotr_amd.functions import clip_ops as module
    clip_ops = module


def close12(got, want):
    scale = float(want.abs().max()) if want.numel() else 0.0
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1e-300), float((got - want).abs().max())


def grads(fn, *inputs, up):
    xs = [t.clone().requires_grad_(True) for t in inputs]
    out = fn(*xs)
    (out * up).sum().backward()
    return [out.detach()] + [x.grad for x in xs]


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("mask_name", [None, "starved_lane", "even_keys"])
def test_attention_truth_is_the_reference_formulation(mask_name):
    B, L, mask = (2, 17, None) if mask_name is None else T.attn_mask_case(mask_name)
    H = 3
    q, k, v, up = (t.double() for t in T.attn_inputs(B, L, H))
    want = grads(lambda a, c: clip_ops.self_attention_reference(a, c, mask, H), torch.cat((q, k), -1), v, up=up)
    got = grads(lambda a, b, c: T.attention_truth(a, b, c, H, mask, scale=1.0 / 32 ** 0.5), q, k, v, up=up)
    close12(got[0], want[0])
    close12(torch.cat((got[1], got[2]), -1), want[1])
    close12(got[3], want[2])


def test_add_layer_norm_truth_is_layer_norm_of_the_sum():
    x, res, gamma, beta, up = (t.double() for t in T.ln_inputs("randn", 5))
    want = grads(lambda a, b, g, be: F.layer_norm(a + b, (256,), g, be, 1e-5), x, res, gamma, beta, up=up)
    got = grads(lambda a, b, g, be: T.add_layer_norm_truth(a, b, g, be, 1e-5), x, res, gamma, beta, up=up)
    for a, b in zip(got, want):
        close12(a, b)


def test_box_truths_are_the_reference_formulations():
    pred, tgt, up = (t.double() for t in T.box_pairs())
    n = pred.shape[0]
    lay, q = torch.zeros(n, dtype=torch.long), torch.arange(n)
    w = torch.rand(n, generator=torch.Generator().manual_seed(1)).double()
    for weight in (None, w):
        want = grads(lambda b: torch.stack(clip_ops.pair_box_loss_reference(b.view(1, 1, n, 4), lay, q, 0, tgt, None, weight)),
                     pred, up=up)
        got = grads(lambda b: torch.stack(T.pair_box_loss_truth(b, tgt, weight)), pred, up=up)
        close12(got[0], want[0])
        close12(got[1], want[1])          # tie rows included: the same autograd rules on both sides
    close12(T.pair_iou_truth(pred, tgt), clip_ops.pair_iou_reference(pred, tgt))


@pytest.mark.parametrize("K", [1, 8])
def test_match_cost_truth_is_the_stacked_matcher_cost(K):
    from memotr_amd.models.matcher import HungarianMatcher
    logits, boxes, labels, gt_boxes = T.match_cost_inputs(3, 2, 9, 11, K, 5)
    lg, bx = logits[:, 1, :9].double(), boxes[:, 1, :9].double()
    want = HungarianMatcher(2.0, 5.0, 2.0).cost_matrix_stacked(lg, bx, labels, gt_boxes.double())
    close12(T.match_cost_truth(lg, bx, labels, gt_boxes.double(), 2.0, 5.0, 2.0), want)
    # out-of-range labels: truth clamps (the matcher's fancy index would wrap -1 and raise on K)
    lo = T.match_cost_truth(lg, bx, torch.tensor([-1, K, 0, K - 1, 0]), gt_boxes.double(), 2.0, 5.0, 2.0)
    hi = T.match_cost_truth(lg, bx, torch.tensor([0, K - 1, 0, K - 1, 0]), gt_boxes.double(), 2.0, 5.0, 2.0)
    assert torch.equal(lo, hi)
    assert float(logits.abs().max()) == T.MATCH_COST_MAX_LOGIT


@pytest.mark.parametrize("alpha,gamma", T.FOCAL_PARAMS)
def test_focal_truth_is_the_reference_formulation(alpha, gamma):
    g = torch.Generator().manual_seed(2)
    logits = (torch.randn(2, 40, 3, generator=g) * 1.5).clamp(-4, 4).double()       # 1 - p_t >= 0.018: no cancellation
    labels = torch.randint(0, 4, (2, 40), generator=g)
    up = torch.randn(2, generator=g).double()
    want = grads(lambda x: clip_ops.focal_loss_per_layer_reference(x, labels, alpha, gamma), logits, up=up)
    got = grads(lambda x: T.focal_truth(x, labels, alpha, gamma), logits, up=up)
    close12(got[0], want[0])
    close12(got[1], want[1])


def test_sine_embed_truth_is_pos_to_pos_embed():
    from memotr_amd.models.utils import _sine_dims, pos_to_pos_embed
    pos = T.sine_positions().double()
    dim_t = _sine_dims(128, 10000, torch.device("cpu")).double()
    up = torch.randn(11, 512, generator=torch.Generator().manual_seed(0)).double()
    want = grads(lambda p: pos_to_pos_embed(p, num_pos_feats=128), pos, up=up)
    got = grads(lambda p: T.sine_embed_truth(p, dim_t, 2 * math.pi), pos, up=up)
    close12(got[0], want[0])
    close12(got[1], want[1])
    assert float(T.sine_positions()[0, 3]) == 1.0 - 2.0 ** -24 < 1.0


def test_linear_and_colsum_truths_are_the_reference_formulations():
    x, w, b, gy = (t.double() for t in T.linear_inputs(33, 36, 33))
    y = T.linear_truth(x, w, b, True)
    got = grads(lambda a, c, d: T.linear_truth(a, c, d, True), x, w, b, up=gy)
    want = clip_ops.linear_bwd_reference(gy, y, x, w)
    for a, b_ in zip(got[1:], want):
        close12(a, b_)
    close12(got[0], F.relu(F.linear(x, w, b)))
    close12(T.colsum_truth(gy), clip_ops.linear_bwd_reference(gy, None, x, w)[2])


# ------------------------------------------------------------------------------------------------ input conditions
def test_attention_mask_cases_reach_the_lanes_they_name():
    B, L, m = T.attn_mask_case("starved_lane")
    live = (~m[0]).nonzero().flatten()
    assert L > 16 and not bool((live % 16 == 5).any()) and all(bool((live % 16 == s).any()) for s in range(16) if s != 5)
    B, L, m = T.attn_mask_case("single_live_key")
    assert (~m).nonzero().tolist() == [[0, 17]] and L == 33
    B, L, m = T.attn_mask_case("even_keys")
    assert L == 64 and bool(m[0, 0::2].all()) and not bool(m[0, 1::2].any())
    B, L, m = T.attn_mask_case("dead_batch")
    assert B == 2 and bool(m[1].all()) and not bool(m[0].any())
    assert set(T.ATTN_LENGTHS) == {1, 15, 16, 17, 31, 33, 255, 257, 511, 512} and max(T.ATTN_LENGTHS) == clip_ops.MHA_MAX_L
    for L in (1, 17):
        q, k, v, up = T.attn_inputs(2, L, 3)
        assert q.shape == (2, L, 96) and q.dtype == torch.float32


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_large_logit_inputs_span_80_and_keep_a_finite_lse(order):
    q, k, v, up = T.attn_large_logit_inputs(order)
    lse, s = T.attention_lse_truth(q.double(), k.double(), T.ATTN_LARGE_H)
    assert bool(torch.isfinite(lse.float()).all())                     # the fp32-rounded lse of every row
    assert 70.0 < float(s.max()) < 88.0 and -88.0 < float(s.min()) < -70.0, (float(s.min()), float(s.max()))
    row0 = s[0, :, 0]                                                   # (H, L): the order the case is named after
    d = row0[:, 1:] - row0[:, :-1]
    if order == "ascending":
        assert bool((d >= 0).all())
    elif order == "descending":
        assert bool((d <= 0).all())
    else:
        assert bool((d > 0).any()) and bool((d < 0).any())
    out, gq, gk, gv = T.attention_truth_with_grads(q, k, v, up, T.ATTN_LARGE_H)
    assert all(bool(torch.isfinite(t).all()) for t in (out, gq, gk, gv))


@pytest.mark.parametrize("kind", T.LN_DATA)
def test_layer_norm_inputs(kind):
    for rows in (1, 5, 35):
        x, res, gamma, beta, up = T.ln_inputs(kind, rows)
        s32, s64 = (x + res).double(), x.double() + res.double()
        if kind == "large_mean":
            assert torch.equal(s32, s64)                               # the fp32 add is exact
            var = s64.var(-1, unbiased=False)
            assert 5e-5 < float(var.min()) and float(var.max()) < 2e-4 and abs(float(s64.mean()) - 1000) < 0.01
            one_pass = (s32.float() ** 2).mean(-1) - s32.float().mean(-1) ** 2      # what E[s^2] - mean^2 gives in fp32
            assert float((one_pass.double() - var).abs().max()) > 100 * float(var.max())
        if kind == "constant_rows":
            for r in T.ln_constant_rows(rows):
                assert torch.equal(s32[r], s64[r]) and float(s64[r].var(unbiased=False)) == 0.0
            xs = [t.double().requires_grad_(True) for t in (x, res, gamma, beta)]
            y = T.add_layer_norm_truth(*xs, T.f32_scalar(1e-5))
            (y * up.double()).sum().backward()
            assert all(bool(torch.isfinite(t.grad).all()) for t in xs)
            for r in T.ln_constant_rows(rows):
                assert torch.equal(y[r].detach(), beta.double())


def test_box_inputs_decide_alike_in_fp32_and_float64():
    pred, tgt, up = T.box_pairs()
    assert pred.shape[0] == len(T.BOX_EDGE_PAIRS) + T.N_RANDOM_BOX_PAIRS
    for t in (pred, tgt):
        assert torch.equal((t * 64).round() / 64, t) and float(t.min()) >= 0.125 and float(t.max()) <= 0.875
    assert torch.equal(T.xyxy(pred).double(), T.xyxy(pred.double())) and torch.equal(T.xyxy(tgt).double(), T.xyxy(tgt.double()))
    d32, d64 = T.box_decisions(pred, tgt), T.box_decisions(pred.double(), tgt.double())
    assert torch.equal(d32.double(), d64)
    names = [n for n, _, _ in T.BOX_EDGE_PAIRS]
    d = d64[:len(names)]
    assert bool((d[names.index("identical"), :4] == 0).all())                      # all four corners tie
    assert float(d[names.index("shared_vertical_edge"), 4]) == 0.0 and float(d[names.index("shared_vertical_edge"), 5]) == 1.0
    assert bool((d[names.index("shared_corner"), 4:6] == 0).all())
    assert float(d[names.index("nested_common_side"), 0]) == 0.0 and float(d[names.index("disjoint"), 4]) == -1.0
    logits, boxes, labels, gt_boxes = T.match_cost_inputs(2, 2, 7, 9, 8, 4, labels="out_of_range")
    assert labels[:2].tolist() == [-1, 8]
    assert torch.equal(T.box_decisions(boxes[:, 1, :7, None], gt_boxes).double(),
                       T.box_decisions(boxes[:, 1, :7, None].double(), gt_boxes.double()))


def test_focal_inputs_cover_the_grid_and_truth_is_finite_there():
    grid = T.FOCAL_GRID
    assert all(float(v) in grid.tolist() for v in (0.0, 88.0, -88.0, 89.0, -89.0, 90.0, -90.0))
    assert sorted({K * Nq for K, Nq in T.FOCAL_SHAPES}) == [5, 255, 256, 257, 2479] and {K for K, _ in T.FOCAL_SHAPES} == {1, 3, 8}
    for K, Nq in T.FOCAL_SHAPES:
        for kind in T.FOCAL_LABELS:
            buf, labels, up = T.focal_inputs(K, Nq, kind)
            view = buf[:, 1, :Nq]
            assert not view.is_contiguous() and labels.shape == (2, Nq) and int(labels.max()) <= K
            assert float(view.abs().max()) >= 89.0
            for alpha, gamma in T.FOCAL_PARAMS:
                x = view.double().requires_grad_(True)
                loss = T.focal_truth(x, labels, alpha, gamma)
                (loss * up.double()).sum().backward()
                assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(x.grad).all())


def test_colsum_inputs_cancel_and_linear_integer_inputs_are_exact():
    for rows in (clip_ops.COLSUM_MAX_ROWS - 1, clip_ops.COLSUM_MAX_ROWS, clip_ops.COLSUM_CHUNK_ROWS + 1):
        x = T.colsum_inputs(rows, 33)
        s = T.colsum_truth(x.double())
        assert float(s.abs().max()) < 1.1e4 and float(x.abs().sum(0).min()) > 0.99e4 * rows
        assert float((x[0::2].double().sum(0)).abs().min()) > 0.99e4 * (rows // 2)      # a strided subset does not cancel
    x, w, gy, y = T.linear_integer_inputs()
    assert bool(torch.isnan(y[0, 0])) and math.copysign(1.0, float(y[1, 1])) == -1.0 and float(y[1, 1]) == 0.0
    for t in (gy.double() @ w.double(), gy.double().t() @ x.double(), gy.double().abs().sum(0)):
        assert float(t.abs().max()) < 2 ** 24                      # every partial sum is an exactly representable integer
    assert {v for s in T.LINEAR_SHAPES for v in s[:1]} == {1, 31, 32, 33}
    assert {s[1] for s in T.LINEAR_SHAPES} == {4, 8, 12, 36} and {s[2] for s in T.LINEAR_SHAPES} == {1, 31, 32, 33, 36}
    assert len(T.LINEAR_SHAPES) == 12


def test_bound_helpers():
    assert T.ulp32(1.0) == 2.0 ** -23 and T.ulp32(1.5) == 2.0 ** -23 and T.ulp32(0.75) == 2.0 ** -24 and T.ulp32(0.0) == 0.0
    assert T.measured_bound(0.0, 1.0) == 2.0 ** -23 and T.measured_bound(1e-6, 0.0) == 4e-6
    assert T.max_err(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 2.0])) == float("inf")
    assert T.colsum_bound(4, 2.0) == 2.0 ** -22
