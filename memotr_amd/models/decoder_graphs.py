"""hipGraph capture of the decoder loop (forward AND backward), one graph pair per (frame slot, query bucket).

Why: the decoder / box-refinement chain of one frame is ~150 tiny kernels per layer forward and ~2x that backward,
each costing the host 13-27 us to issue; with the encoder batched per clip the train step is bound by that launch
rate.  A captured graph replays the whole per-layer chain with one launch.

What is captured: ``DeformableDecoder.forward``'s loop as a tensor-in / tensor-out module (``DecoderLoop``): per layer anchors -> sine embedding -> ``ref_point_head`` (x ``query_scale``) -> the decoder layer
(self-attention over the queries, MSDeformAttn cross-attention through the fused HIP kernels, FFN) -> box head ->
refined reference (detached for the next layer).  ``torch.cuda.make_graphed_callables`` records its forward and its
backward as two graphs.  The Deformable-DETR variant (``use_dab=False``) has a loop of its own, ``PlainDecoderLoop``: the
query position is an input and layer 0 works on 2-d references.

Constraints handled here:
  * static shapes: the query count (300 detect + n track queries) is padded to a multiple of ``BUCKET`` with masked
    slots (padded keys are excluded from the self-attention softmax exactly; padded queries are sliced away, so
    their rows receive zero gradient);
  * a graphed callable owns its activations: it cannot run twice before its backward.  A clip holds T frames of
    activations at once, so every frame index gets its own capture ("slot");
  * the pyramid geometry is part of the key (multi-scale training re-captures per geometry, LRU-bounded);
  * parameters are shared by all slots and enter a graph as ONE flat tensor (made once per clip): the frames'
    parameter gradients meet in one add per frame and DistributedDataParallel's hooks fire once per parameter.
Anything that cannot be captured (CPU tensors, checkpointing, no grad mode mismatch, a capture error) takes the eager
path -- same arithmetic, kernel by kernel.
"""
from __future__ import annotations

import os
import torch
import torch.nn as nn

from ..functions import clip_ops
from ..utils.utils import inverse_sigmoid, refine_boxes
from .graph_cache import GraphCache
from .graph_capture import FlatParameters, capture_pair
from .utils import pos_to_pos_embed

BUCKET = 32
# (frame slots x geometries x query buckets) kept alive; least recently used go first.  A clip of five frames whose track
# counts wander over five buckets of 32 is already 25 keys -- one more than round 5's limit of 24, and an LRU cache one
# entry short of its working set misses on EVERY lookup (a capture costs two warm-up passes and the capture: ~0.1 s).
# A graph pair holds ~0.25 GB (its static copies of `src`, the flat parameters and the value bank): 48 of them is 12 GB
# of 288.
MAX_GRAPHS = int(os.environ.get("MEMOTR_MAX_DECODER_GRAPHS", "48"))


class DecoderLoop(nn.Module):
    """All iterations of the decoder loop of one frame (what ``DeformableDecoder.forward`` does with DAB anchors and
    box refinement, reference models/deformable_decoder.py:70-140), tensors in -> four stacks out.  One capture per
    frame slot: `src` and the parameters enter the graph once per frame.

    Holds references to modules owned by the decoder and is never attached to the model tree.  Every module appears
    exactly ONCE in this tree: ``torch.func.functional_call`` does not restore parameters of a module that is
    reachable under two names (it leaves the substituted tensors behind -- observed with torch 2.10), so the heads
    shared by all layers (``ref_point_head``, ``query_scale``) live at this level, not inside per-layer children."""

    def __init__(self, decoder, spatial_shapes, level_start_index):
        super().__init__()
        self.layers = nn.ModuleList(decoder.layers)
        self.bbox_embed = nn.ModuleList(decoder.bbox_embed)
        self.ref_point_head = decoder.ref_point_head
        self.query_scale = decoder.query_scale
        self.nd = decoder.n_det_queries
        self.merge_from = decoder.merge_det_track_layer
        self.d_model = decoder.d_model
        # constants of the geometry: closed over, not graph inputs (the operator plans from their host tag)
        self._shapes = spatial_shapes
        self._lsi = level_start_index

    def forward(self, output, reference_points, src, ratios4, query_mask, src_padding_mask):
        outs, refs, layer_inputs, boxes = [], [], [], []
        from ..modules.ms_deform_attn import project_values
        # the six value projections of `src` as one GEMM, each layer reading its columns in place
        values = project_values([layer.cross_attn for layer in self.layers], src, src_padding_mask)
        for lid, layer in enumerate(self.layers):
            layer_inputs.append(output)
            ref_in = reference_points[:, :, None] * ratios4
            anchor = pos_to_pos_embed(ref_in[:, :, 0, :], num_pos_feats=self.d_model // 2)
            raw_pos = self.ref_point_head(anchor)
            query_pos = raw_pos if lid == 0 else self.query_scale(output) * raw_pos
            merge = lid >= self.merge_from
            output = layer(output, query_pos, ref_in, src, self._shapes, self._lsi, query_mask, src_padding_mask, merge,
                           None if values is None else values[lid])
            new_ref = refine_boxes(self.bbox_embed[lid](output), reference_points)
            boxes.append(new_ref)
            if merge:
                reference_points = new_ref.detach()
            else:   # track queries did not go through the layer: keep their anchors
                reference_points = torch.cat((new_ref[:, :self.nd].detach(), reference_points[:, self.nd:]), dim=1)
            outs.append(output)
            refs.append(reference_points)
        return torch.stack(outs), torch.stack(refs), torch.stack(layer_inputs), torch.stack(boxes)


class PlainDecoderLoop(nn.Module):
    """``DecoderLoop`` for the Deformable-DETR variant (``use_dab=False`` with box refinement, the eager branch of
    ``DeformableDecoder.forward``): the query position is an input, constant over the layers -- no anchor embedding, no
    ``ref_point_head``, no ``query_scale`` (the decoder does not own them).  Layer 0 samples around the 2-d slice of the
    4-d input reference and refines only xy; the model's box head refines all four at that level, so the one ``delta``
    of layer 0 gives two boxes (``clip_ops.refine_boxes_split``): ``boxes[0]`` is the head's, with its graph, ``refs[0]``
    the decoder's, detached.  From layer 1 on both are the same expression, as with DAB anchors.

    Every module appears once in this tree (see ``DecoderLoop``): ``layers`` and ``bbox_embed``."""

    def __init__(self, decoder, spatial_shapes, level_start_index):
        super().__init__()
        self.layers = nn.ModuleList(decoder.layers)
        self.bbox_embed = nn.ModuleList(decoder.bbox_embed)
        self.nd = decoder.n_det_queries
        self.merge_from = decoder.merge_det_track_layer
        self._shapes = spatial_shapes
        self._lsi = level_start_index

    def forward(self, output, reference_points, query_pos, src, valid_ratios, ratios4, query_mask, src_padding_mask):
        outs, refs, layer_inputs, boxes = [], [], [], []
        from ..modules.ms_deform_attn import project_values
        values = project_values([layer.cross_attn for layer in self.layers], src, src_padding_mask)
        anchors = reference_points              # what track queries keep until the layers merge them
        for lid, layer in enumerate(self.layers):
            layer_inputs.append(output)
            if lid == 0:
                ref_in = reference_points[:, :, None, :2] * valid_ratios[:, None]
            else:
                ref_in = reference_points[:, :, None] * ratios4
            merge = lid >= self.merge_from
            output = layer(output, query_pos, ref_in, src, self._shapes, self._lsi, query_mask, src_padding_mask, merge,
                           None if values is None else values[lid])
            delta = self.bbox_embed[lid](output)
            if lid == 0:
                box, new_ref = clip_ops.refine_boxes_split(delta, reference_points)
            else:
                box = new_ref = refine_boxes(delta, reference_points)
            boxes.append(box)
            if merge:
                reference_points = new_ref.detach()
            else:   # track queries did not go through the layer: keep their anchors
                reference_points = torch.cat((new_ref[:, :self.nd].detach(), anchors[:, self.nd:]), dim=1)
            outs.append(output)
            refs.append(reference_points)
        return torch.stack(outs), torch.stack(refs), torch.stack(layer_inputs), torch.stack(boxes)


def uses_dab(decoder) -> bool:
    """Which of the two loops ``decoder`` runs (DAB anchors unless the owner says otherwise); part of the cache keys."""
    return bool(getattr(decoder, "use_dab", True))


def loop_for(decoder, spatial_shapes, level_start_index) -> nn.Module:
    """The capturable loop of ``decoder``; the arguments are those ``DeformableDecoder._forward_graphed`` assembles."""
    cls = DecoderLoop if uses_dab(decoder) else PlainDecoderLoop
    return cls(decoder, spatial_shapes, level_start_index)


def enabled() -> bool:
    return os.environ.get("MEMOTR_DECODER_GRAPHS", "1") != "0"


class DecoderGraphs(GraphCache):
    """Cache of captured decoder steps, owned by a ``DeformableDecoder``."""

    def __init__(self, decoder):
        super().__init__("decoder", MAX_GRAPHS, grow_cap=2)
        self.decoder = decoder
        self._flat = {}          # the flat parameters of the current clip, shared by the captures of all frame slots

    def usable(self, output, src) -> bool:
        d = self.decoder
        # use_checkpoint: the graph pair replaces the per-layer checkpoints of the decoder -- its activations are
        # (300 + n) x 256 per layer, nothing next to the backbone / encoder segments that stay checkpointed
        # (MEMOTR_CHECKPOINT_DECODER=1 keeps the reference's per-layer recompute, eager).
        # extra_track_attn: a frame without tracks still carries one masked (padded) track slot in the graphed path,
        # and attention over keys that are ALL masked is 0 * inf -- its rows are sliced away, but the NaN reaches the
        # parameter gradients through the norms; those models keep the eager loop
        return (enabled() and not self.failed and output.is_cuda and d.bbox_embed is not None
                and (not d.use_checkpoint or os.environ.get("MEMOTR_CHECKPOINT_DECODER", "0") != "1")
                and torch.is_grad_enabled() and src.requires_grad
                and not torch.is_autocast_enabled() and output.dtype == torch.float32
                and not any(getattr(layer, "extra_track_attn", False) for layer in d.layers))

    @staticmethod
    def bucket(n_queries: int, n_det: int) -> int:
        # the TOTAL is rounded up to a multiple of BUCKET (the fused attention kernels want aligned key counts) with
        # at least one (masked) track slot: a zero-sized track part would put empty copy nodes into the capture
        n = max(n_queries, n_det + 1)
        return (n + BUCKET - 1) // BUCKET * BUCKET

    def run(self, frame_slot: int, args, shapes, lsi, clip_key=None):
        """The decoder loop of frame ``frame_slot`` through its graph (captured on first use); None if capture failed."""
        # (a capture bakes the kernel choice in; `use_dab`: a decoder toggled between the two loops never replays the other's)
        key = (frame_slot, tuple(a.shape for a in args), tuple(bool(a.requires_grad) for a in args),
               self._geometry(shapes), clip_ops.config_key(), uses_dab(self.decoder))
        entry = self.lookup(key, lambda: self._capture(args, shapes, lsi))
        if entry is None:
            return None
        self.replays += 1
        return entry.fn(*args, entry.params.flat(clip_key))

    @staticmethod
    def _geometry(shapes):
        """The pyramid as a hashable value ((H, W), ...): the identity of the tensor object is not a key -- an id can
        be recycled once the geometry cache evicts the tensor."""
        from ..MultiScaleDeformableAttention import host_shapes
        return tuple(map(tuple, host_shapes(shapes).tolist()))

    def _capture(self, args, shapes, lsi):
        """Capture the decoder's loop as a function of (inputs..., flat parameters)."""
        loop = loop_for(self.decoder, shapes, lsi)
        params = FlatParameters(loop, loop.named_parameters(), True, shared=self._flat)

        def run(*flat_in):           # (inputs..., flat parameters)
            return torch.func.functional_call(loop, params.substitution(flat_in[-1]), tuple(flat_in[:-1]))

        sample = tuple(a.detach().clone().requires_grad_(a.requires_grad) for a in args)
        return capture_pair(self, params, run, sample)
