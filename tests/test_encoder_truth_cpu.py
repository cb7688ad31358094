"""CPU: the conditions under which tests/test_encoder_truth_gpu.py holds the deformable-encoder stack to float64 truth
(tests/encoder_truth.py).

* Decisions.  For both cases the float32 and the float64 CPU run take the same decisions, every one -- the sign under
  each ReLU, the bilinear cell of each sampling point -- and no decision of the float64 run sits closer to its edge than
  ``RELU_MARGIN`` / ``CELL_MARGIN``.
* Reach.  ``rows10880`` sits on the training side of every row switch of ``EncoderLayerNode`` (read from the product's
  constants), every hidden unit of the first layer switches over its rows and every level samples every level;
  ``small`` has padded rows in both batch items and sampling points outside the valid area.
* The rule has teeth.  ``EncoderLayerNode`` restated on the CPU in plain float32 torch (``PlainNode``: the algebra of its
  forward and backward, LayerNorm backward by formula, the oracle operator, no kernels) with one switch per planted
  defect: the untouched restatement stays inside ``measured_bound`` of the float32 CPU composition against float64
  truth on ``small``; every defect lands outside it, on the tensors it must reach.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import encoder_truth as et
from model_helpers import OracleMSDeformAttnFunction


@pytest.fixture(scope="module", autouse=True)
def _libraries(hip_lib, clip_lib):
    """The package has no CPU fallback to import: its libraries are built first (nothing here launches a kernel)."""


@pytest.fixture(scope="module", params=et.CASES, ids=lambda c: c.name)
def decisions(request):
    with pytest.MonkeyPatch.context() as mp:
        return request.param, et.encoder_decisions(mp, request.param)


# ------------------------------------------------------------------------------------------------ decisions and reach
def test_float32_and_float64_take_the_same_decisions(decisions):
    case, d = decisions
    on = [float(r.float().mean()) for r in d.relus64]
    print(f"DECISIONS {case.name} seed={case.seed} taken={d.taken} relu={d.relu} cell={d.cell} "
          f"relu_margin={d.relu_margin:.2e} cell_margin={d.cell_margin:.2e} units_on={on[0]:.2f}/{on[1]:.2f}")
    per_layer = case.rows * et.D_FFN + case.rows * et.N_HEADS * et.N_LEVELS * et.N_POINTS * 2
    assert d.taken == et.N_LAYERS * per_layer
    assert d.taken > (6e6 if case is et.ROWS10880 else 2e5)
    assert d.relu == 0 and d.cell == 0, (case.name, d.relu, d.cell, d.taken)
    assert d.relu_margin >= et.RELU_MARGIN and d.cell_margin >= et.CELL_MARGIN, (case.name, d.relu_margin, d.cell_margin)
    # ... and with them the float32 composition is round-off away from truth
    assert len(d.got64) == et.N_TENSORS == 35
    for k, e in et.dt.errors(d.got32, d.got64).items():
        scale = et.out_scale(d.got64[k])
        assert scale > 0 and e / scale < et.REF_ERROR_CAP, (k, e, scale)


def _inside(cells, lvl, h, w):
    """Sampling points of level ``lvl`` with all four bilinear corners inside the (h, w) area."""
    cx, cy = cells[:, :, :, lvl, :, 0], cells[:, :, :, lvl, :, 1]
    return (cx >= 0) & (cx + 1 < w) & (cy >= 0) & (cy + 1 < h)


def test_the_cases_reach_what_they_are_meant_to_reach(decisions):
    from memotr_amd.functions import clip_ops
    from memotr_amd.modules import linear
    case, d = decisions
    if case is et.ROWS10880:
        assert case.rows == 10880 and case.n == 1
        assert case.rows >= linear.MIN_ROWS and case.rows > clip_ops.COLSUM_MAX_ROWS and case.rows > 4096
        assert case.rows < linear.ROCBLAS_DGRAD_ROWS                       # (the switch this case leaves out)
        assert clip_ops._fanin_chunk_rows(case.rows) == 64 != clip_ops._fanin_chunk_rows(et.SMALL.rows)
        switching = [int((r.any(0) & ~r.all(0)).sum()) for r in d.relus64]
        assert switching[0] == et.D_FFN, switching                          # every hidden unit of the first layer is on
        assert switching[1] >= 61, switching                                #   for some rows and off for others
        assert encoder_mask(case) is None
        level = et.level_of_rows(case)
        for cells in d.cells64:             # every level receives sampling points from every level
            for q_lvl in range(et.N_LEVELS):
                for v_lvl, (h, w) in enumerate(case.shapes):
                    assert bool(_inside(cells[:, level == q_lvl], v_lvl, h, w).any()), (q_lvl, v_lvl)
    else:
        assert case.rows == 336 < linear.MIN_ROWS and case.rows <= clip_ops.LINEAR_BWD_MAX_ROWS
        assert case.rows <= clip_ops.COLSUM_MAX_ROWS and clip_ops._fanin_chunk_rows(case.rows) == 16
        mask = encoder_mask(case)
        assert bool(mask[0].any()) and bool(mask[1].any()) and not bool(mask.all(1).any())
        x = et.encoder_inputs(case)
        outside = 0
        for cells in d.cells64:             # some sampling point leaves the valid (unpadded) area of its level
            for lvl, (h, w) in enumerate(case.shapes):
                for b in range(case.n):
                    vw = float(x["valid_ratios"][b, lvl, 0]) * w
                    vh = float(x["valid_ratios"][b, lvl, 1]) * h
                    outside += int((~_inside(cells[b:b + 1], lvl, round(vh), round(vw))).sum())
        assert outside > 0


def encoder_mask(case):
    return et.encoder_inputs(case)["mask"]


# ------------------------------------------------------------------------------------------------ planted defects
DEFECTS = ("no_g_q_in_norm2_fanin", "q_next_without_pos", "no_residual_into_dx1", "no_residual_into_g_src",
           "no_relu_mask_on_dh", "linear2_bias_from_g_y", "padded_g_value_not_zeroed", "g_q_not_handed_to_pos")


def _ln_fwd(s, gamma, beta, eps):
    mean = s.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((s - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (s - mean) * rstd
    return xhat * gamma + beta, xhat, rstd


def _ln_bwd(g, xhat, rstd, gamma):
    """(d/d sum, d/d gamma, d/d beta) of y = xhat * gamma + beta."""
    dxhat = g * gamma
    ds = rstd * (dxhat - dxhat.mean(-1, keepdim=True) - xhat * (dxhat * xhat).mean(-1, keepdim=True))
    return ds, (g * xhat).sum(0), g.sum(0)


class PlainNode(torch.autograd.Function):
    """``EncoderLayerNode`` in plain torch: same inputs and outputs ((src, q) -> (y, q_next)), the same algebra forward
    and backward, one switch per planted defect (``defect`` None: the node as it is meant)."""

    @staticmethod
    def forward(ctx, src, q, pos_next, reference_points, shapes, level_start, pad_mask, n_heads, n_points, eps1, eps2,
                defect, wv, bv, wq, bq, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2):
        N, S, C = src.shape
        rows = N * S
        src2, q2 = src.reshape(rows, C), q.reshape(rows, C)
        pad = None if pad_mask is None else pad_mask.reshape(rows)
        value = src2 @ wv.t() + bv
        if pad is not None:
            value = value.masked_fill(pad[:, None], 0.0)
        proj = q2 @ wq.t() + bq
        # the operator, on leaves of its own: its backward is autograd's of the oracle's statement
        with torch.enable_grad():
            value_l, proj_l = value.detach().requires_grad_(True), proj.detach().requires_grad_(True)
            L = shapes.shape[0]
            n_off = n_heads * L * n_points * 2
            p3 = proj_l.view(N, S, -1)
            offsets = p3[..., :n_off].unflatten(-1, (n_heads, L, n_points, 2))
            attn = F.softmax(p3[..., n_off:].unflatten(-1, (n_heads, L * n_points)), -1).view(N, S, n_heads, L, n_points)
            wh = shapes.flip(-1).to(src.dtype)
            loc = reference_points[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
            out = OracleMSDeformAttnFunction.apply(value_l.view(N, S, n_heads, C // n_heads), shapes, level_start, loc,
                                                   attn, 64).reshape(rows, C)
        out_d = out.detach()
        s1 = src2 + (out_d @ wo.t() + bo)
        x1, xhat1, rstd1 = _ln_fwd(s1, g1, be1, eps1)
        hidden = torch.relu(x1 @ w1.t() + b1)
        s2 = x1 + (hidden @ w2.t() + b2)
        y, xhat2, rstd2 = _ln_fwd(s2, g2, be2, eps2)
        q_next = None
        if pos_next is not None:
            q_next = y.clone() if defect == "q_next_without_pos" else y + pos_next.reshape(rows, C)
        ctx.save_for_backward(src2, q2, out_d, xhat1, rstd1, x1, hidden, xhat2, rstd2, pad, wv, wq, wo, g1, w1, w2, g2)
        ctx.graph = (out, value_l, proj_l)
        ctx.dims, ctx.defect = (N, S, C), defect
        ctx.set_materialize_grads(False)
        return y.view(N, S, C), (None if q_next is None else q_next.view(N, S, C))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y, g_q):
        src2, q2, out, xhat1, rstd1, x1, hidden, xhat2, rstd2, pad, wv, wq, wo, g1, w1, w2, g2 = ctx.saved_tensors
        (N, S, C), defect = ctx.dims, ctx.defect
        rows = N * S
        flat = lambda g: None if g is None else g.reshape(rows, C)      # noqa: E731
        g_y, g_q = flat(g_y), flat(g_q)
        # norm2: the gradients of the layer's two outputs meet here
        g = g_y if g_q is None else (g_q if g_y is None else g_y + g_q)
        if defect == "no_g_q_in_norm2_fanin":
            g = g_y
        dz2, gg2, gbe2 = _ln_bwd(g, xhat2, rstd2, g2)
        gb2 = g_y.sum(0) if defect == "linear2_bias_from_g_y" else dz2.sum(0)
        gw2 = dz2.t() @ hidden
        dh = dz2 @ w2
        if defect != "no_relu_mask_on_dh":
            dh = dh * (hidden > 0)
        gb1, gw1 = dh.sum(0), dh.t() @ x1
        dx1 = dh @ w1 if defect == "no_residual_into_dx1" else dz2 + dh @ w1
        # norm1
        dz1, gg1, gbe1 = _ln_bwd(dx1, xhat1, rstd1, g1)
        gbo, gwo = dz1.sum(0), dz1.t() @ out
        d_out = dz1 @ wo
        graph_out, value_l, proj_l = ctx.graph
        g_value, g_proj = torch.autograd.grad(graph_out, (value_l, proj_l), d_out)
        if pad is not None and defect != "padded_g_value_not_zeroed":
            g_value = g_value.masked_fill(pad[:, None], 0.0)
        gwv, gbv = g_value.t() @ src2, g_value.sum(0)
        gwq, gbq = g_proj.t() @ q2, g_proj.sum(0)
        g_src = g_value @ wv if defect == "no_residual_into_g_src" else dz1 + g_value @ wv
        g_q_in = g_proj @ wq
        g_pos = None if (g_q is None or defect == "g_q_not_handed_to_pos") else g_q.view(N, S, C)
        return (g_src.view(N, S, C), g_q_in.view(N, S, C), g_pos, None, None, None, None, None, None, None, None, None,
                gwv, gbv, gwq, gbq, gwo, gbo, gg1, gbe1, gw1, gb1, gw2, gb2, gg2, gbe2)


def plain_encoder_forward(enc, defect):
    """``DeformableEncoder.forward`` along its node branch, every layer a ``PlainNode``."""
    def forward(src, spatial_shapes, level_start_index, valid_ratios, pos=None, padding_mask=None, shapes_list=None):
        ref = enc.get_reference_points(shapes_list, valid_ratios, device=src.device)
        output, q = src, src + pos
        for i, layer in enumerate(enc.layers):
            at = layer.self_attn
            wq = torch.cat((at.sampling_offsets.weight, at.attention_weights.weight), 0)
            bq = torch.cat((at.sampling_offsets.bias, at.attention_weights.bias), 0)
            output, q = PlainNode.apply(
                output, q, pos if i + 1 < enc.num_layers else None, ref, spatial_shapes, level_start_index, padding_mask,
                at.n_heads, at.n_points, layer.norm1.eps, layer.norm2.eps, defect, at.value_proj.weight,
                at.value_proj.bias, wq, bq, at.output_proj.weight, at.output_proj.bias, layer.norm1.weight,
                layer.norm1.bias, layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias,
                layer.norm2.weight, layer.norm2.bias)
        return output
    return forward


@pytest.fixture(scope="module")
def defect_ground():
    """``small``: truth, the float32 CPU composition and its error -- computed once, shared by the defects."""
    case = et.SMALL
    enc, x = et.build_encoder(case), et.encoder_inputs(case)
    truth = et.encoder_truth(enc, x)
    with pytest.MonkeyPatch.context() as mp:
        et.truth_operator(mp)
        ref = et.run_encoder(enc, x)
    return case, enc, x, truth, ref, et.dt.errors(ref, truth)


def _planted_run(ground, defect):
    case, enc, x, truth, ref, ref_err = ground
    bad = copy.deepcopy(enc)
    bad.forward = plain_encoder_forward(bad, defect)
    return et.run_encoder(bad, x)


def _p(layer, *names):
    return {f"grad::p::layers.{layer}.{n}" for n in names}


def test_the_untouched_restatement_stays_inside_the_bound(defect_ground):
    case, enc, x, truth, ref, ref_err = defect_ground
    et.reference_inside_cap(case.name, ref_err, truth)
    got = _planted_run(defect_ground, None)
    rows, bad = et.check(case.name, "cpu-plain-node", got, truth, ref_err, truth)
    assert len(rows) == et.N_TENSORS
    assert not bad, [(r.tensor, r.err, r.bound) for r in bad]


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_planted_defect_lands_outside_the_bound(defect_ground, defect):
    case, enc, x, truth, ref, ref_err = defect_ground
    got = _planted_run(defect_ground, defect)
    rows, bad = et.check(case.name, "cpu-" + defect, got, truth, ref_err, truth)
    caught = {r.tensor for r in bad}
    print(f"DEFECT {defect}: {len(caught)} tensors outside the bound: {sorted(caught)}")
    assert caught, defect
    layer0 = {k for k in truth if k.startswith("grad::p::layers.0.")}
    weights0 = {k for k in layer0 if truth[k].dim() == 2}
    if defect == "no_g_q_in_norm2_fanin":       # the next layer's query gradient dropped: layer 0 and what is in front
        assert {"grad::src"} | weights0 <= caught and "out" not in caught
        assert not any(k.startswith("grad::p::layers.1.") for k in caught)
    elif defect == "q_next_without_pos":
        assert "out" in caught
    elif defect in ("no_residual_into_dx1", "no_residual_into_g_src"):
        assert "grad::src" in caught and "out" not in caught
    elif defect == "no_relu_mask_on_dh":
        assert _p(0, "linear1.weight", "linear1.bias") | _p(1, "linear1.weight", "linear1.bias") <= caught
        assert "out" not in caught
    elif defect == "linear2_bias_from_g_y":     # that tensor only (of both layers)
        assert caught == _p(0, "linear2.bias") | _p(1, "linear2.bias")
    elif defect == "padded_g_value_not_zeroed":
        assert _p(0, "self_attn.value_proj.weight", "self_attn.value_proj.bias") \
            | _p(1, "self_attn.value_proj.weight", "self_attn.value_proj.bias") <= caught
        assert "out" not in caught
    elif defect == "g_q_not_handed_to_pos":     # nothing else reads that return value
        assert caught == {"grad::pos"}
