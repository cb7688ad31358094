"""One autograd node per deformable-encoder layer (fp32, CUDA, no checkpointing, no autocast).

Composed from separate nodes (value / query / output projections, the fused operator, two add + LayerNorm, two FFN
linears) the layer makes autograd join every fan-out of the backward with a full-size element-wise add, and the bias
gradients of ``output_proj`` and ``linear2`` re-read the tensor the LayerNorm backward has just written.  Here the
forward issues the same GEMMs and kernels on the same values and saves the same tensors; the backward is written out
so that those joins happen where the data already is:

* the gradients of the layer's output (from the next layer's residual + value projection, and from its query) go into
  the ``norm2`` backward as separate inputs and are summed in registers (clip_ops.add_layer_norm_bwd_fanin);
* both LayerNorm backwards emit the column sums of their result: the bias gradients of ``linear2`` / ``output_proj``;
* ``linear1``'s input gradient is accumulated by its GEMM (beta = 1) into the ``norm2`` backward's result, which is the
  other gradient of that tensor, and the value projection's input gradient into the ``norm1`` backward's result;
* ``norm2`` of layer i writes layer i + 1's query ``y + pos`` in the same pass as ``y``.

The node takes (src, q = src + pos) and returns (y, q_next): the two gradients of a layer's input travel to the layer
in front as the gradients of its two outputs, never summed in memory.  (The gradient of q_next is also that of ``pos``,
which carries the learnt level embedding: it is handed on unchanged, and autograd accumulates the layers' shares as
it does for the composed layers.)
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import MultiScaleDeformableAttention as MSDA
from ..modules import linear as L
from . import clip_ops


def enabled() -> bool:
    return os.environ.get("MEMOTR_ENC_LAYER_NODE", "1") != "0"


def _linear(x2: torch.Tensor, w: torch.Tensor, b: torch.Tensor, relu: bool = False) -> torch.Tensor:
    """The product ``long_linear`` issues for these rows (modules/linear.py): the library GEMM with the bias (and the
    ReLU) in its epilogue, or the query-sized kernel for a few hundred rows."""
    if x2.shape[0] < L.MIN_ROWS:
        if clip_ops.linear_fwd_usable(x2, w, b):
            return clip_ops.linear_fwd(x2, w, b, relu)
        return torch._addmm_activation(b, x2, w.t(), use_gelu=False) if relu else torch.addmm(b, x2, w.t())
    return torch._addmm_activation(b, x2, w.t(), use_gelu=False) if relu else F.linear(x2, w, b)


class EncoderLayerNode(torch.autograd.Function):
    calls = 0          # forward calls so far (tests read it to see which path a configuration took)

    @staticmethod
    def forward(ctx, src, q, pos_next, reference_points, spatial_shapes, level_start_index, pad_mask, zero_rows,
                n_heads, n_points, site, eps1, eps2, wv, bv, wq, bq, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2):
        EncoderLayerNode.calls += 1
        N, S, C = src.shape
        rows = N * S
        src2, q2 = src.reshape(rows, C), q.reshape(rows, C)
        # self-attention: value and query projections, the fused operator, the output projection
        value = _linear(src2, wv, bv)
        if zero_rows is not None and zero_rows.numel():
            value.index_fill_(0, zero_rows, 0)          # (the padded rows, where the projection wrote them)
        proj = _linear(q2, wq, bq)
        MSDA.set_call_site(site)
        value4 = value.view(N, S, n_heads, C // n_heads)
        out = MSDA.ms_deform_attn_fused_forward(value4, spatial_shapes, level_start_index, proj.view(N, S, -1),
                                                reference_points, pad_mask, n_heads, n_points)
        attn = _linear(out.reshape(rows, C), wo, bo)
        s1, x1, _, stats1 = clip_ops.add_layer_norm_fwd(src2, attn, g1, be1, eps1)
        del attn
        # FFN
        hidden = _linear(x1, w1, b1, relu=True)
        ffn = _linear(hidden, w2, b2)
        s2, y, q_next, stats2 = clip_ops.add_layer_norm_fwd(x1, ffn, g2, be2, eps2,
                                                            None if pos_next is None else pos_next.reshape(rows, C))
        ctx.save_for_backward(src2, q2, value4, proj, out, s1, stats1, x1, hidden, s2, stats2, reference_points,
                              spatial_shapes, level_start_index, pad_mask, zero_rows, wv, wq, wo, g1, w1, w2, g2)
        ctx.dims = (N, S, C, int(n_heads), int(n_points))
        ctx.site = site
        ctx.shapes_host = getattr(spatial_shapes, "_msda_host", None)
        ctx.set_materialize_grads(False)
        return y.view(N, S, C), (None if q_next is None else q_next.view(N, S, C))

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_q):
        (src2, q2, value4, proj, out, s1, stats1, x1, hidden, s2, stats2, reference_points, shapes, level_start,
         pad_mask, zero_rows, wv, wq, wo, g1, w1, w2, g2) = ctx.saved_tensors
        N, S, C, n_heads, n_points = ctx.dims
        rows = N * S
        dgrad = lambda: L.prefer_blas(L.dgrad_blas(rows))      # noqa: E731  (the library _SplitKLinear picks)
        cont = lambda g: None if g is None else g.reshape(rows, C).contiguous()      # noqa: E731

        # norm2: the gradient inputs are summed in registers; the column sums of dz2 are linear2's bias gradient
        dz2, gg2, gbe2, gb2 = clip_ops.add_layer_norm_bwd_fanin((cont(g_y), cont(g_q), None), s2, stats2, g2)
        del g_y
        gw2 = L.splitk_weight_grad(dz2, hidden)
        with dgrad():
            dh = dz2 @ w2
        if clip_ops.relu_bwd_colsum_usable(dh, hidden):
            dh, gb1 = clip_ops.relu_bwd_colsum(dh, hidden)
        else:
            dh = torch.ops.aten.threshold_backward(dh, hidden, 0.0)
            gb1 = clip_ops.colsum(dh)
        gw1 = L.splitk_weight_grad(dh, x1)
        with dgrad():
            dz2.addmm_(dh, w1)            # d/dx1 = dz2 (residual) + dh W1: the GEMM accumulates into dz2 (beta = 1)
        del dh
        # norm1: column sums of dz1 = output_proj's bias gradient
        dz1, gg1, gbe1, gbo = clip_ops.add_layer_norm_bwd_fanin((dz2, None, None), s1, stats1, g1)
        del dz2
        gwo = L.splitk_weight_grad(dz1, out.view(rows, C))
        with dgrad():
            d_out = dz1 @ wo
        if ctx.shapes_host is not None and getattr(shapes, "_msda_host", None) is None:
            shapes._msda_host = (ctx.shapes_host[0], shapes._version)
        MSDA.set_call_site(ctx.site)
        g_value, g_proj, _ = MSDA.ms_deform_attn_fused_backward(value4, shapes, level_start, proj.view(N, S, -1),
                                                                reference_points, pad_mask, d_out.view(N, S, C), n_heads,
                                                                n_points, need_ref_grad=False, fwd_output=out)
        MSDA.set_call_site(0)
        del d_out
        g_value = g_value.view(rows, C)
        if zero_rows is not None and zero_rows.numel():
            g_value.index_fill_(0, zero_rows, 0)
        g_proj = g_proj.reshape(rows, -1)
        gwv, gbv = L.splitk_weight_grad(g_value, src2), clip_ops.colsum(g_value)
        gwq, gbq = L.splitk_weight_grad(g_proj, q2), clip_ops.colsum(g_proj)
        g_src = g_q_in = None
        with dgrad():
            if ctx.needs_input_grad[0]:
                g_src = dz1.addmm_(g_value, wv).view(N, S, C)      # dz1 (residual) + g_value Wv, again beta = 1
            if ctx.needs_input_grad[1]:
                g_q_in = (g_proj @ wq).view(N, S, C)
        # (q_next = y + pos_next: the gradient of the next layer's query is also pos_next's, passed through as it came)
        return (g_src, g_q_in, g_q if ctx.needs_input_grad[2] else None, None, None, None, None, None, None, None, None, None, None,
                gwv, gbv, gwq, gbq, gwo, gbo, gg1, gbe1, gw1, gb1, gw2, gb2, gg2, gbe2)
