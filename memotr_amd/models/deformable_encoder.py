"""Deformable encoder: 6 x {MSDeformAttn self-attention over the pyramid, LN, FFN, LN}
(reference models/deformable_encoder.py:21-131)."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from .. import MultiScaleDeformableAttention as MSDA
from ..modules import MSDeformAttn
from ..modules import linear as linear_mod
from ..modules import ms_deform_attn as msda_mod
from ..functions import clip_ops, encoder_layer
from ..functions.clip_ops import add_layer_norm
from ..modules.linear import long_linear
from .utils import get_activation_layer, get_clones


class DeformableEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers, use_checkpoint: bool, layer_node: bool = True):
        super().__init__()
        self.layers = get_clones(module=encoder_layer, n=num_layers)
        self.num_layers = num_layers
        self.use_checkpoint = use_checkpoint
        # layers as single autograd nodes (functions/encoder_layer.py); the owner switches it off when it wraps the
        # encoder in activation checkpointing
        self.layer_node = layer_node

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        """Pixel centres normalised by the valid extent of their own level, re-scaled to every level:
        (B, S, L, 2) in (x, y).  ``spatial_shapes`` may be a tensor or a python list of (H, W)."""
        shapes = spatial_shapes.tolist() if torch.is_tensor(spatial_shapes) else spatial_shapes
        refs = []
        for lvl, (h, w) in enumerate(shapes):
            h, w = int(h), int(w)
            ys = torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=device)
            xs = torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=device)
            ry, rx = torch.meshgrid(ys, xs, indexing="ij")
            ry = ry.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * h)
            rx = rx.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * w)
            refs.append(torch.stack((rx, ry), -1))
        ref = torch.cat(refs, 1)
        return ref[:, :, None] * valid_ratios[:, None]

    def forward(self, src, spatial_shapes, level_start_index, valid_ratios, pos=None, padding_mask=None,
                shapes_list=None, reference_points=None):
        if reference_points is None:        # (the caller may hold them for this pyramid / mask geometry)
            reference_points = self.get_reference_points(shapes_list if shapes_list is not None else spatial_shapes,
                                                         valid_ratios, device=src.device)
        output = src
        if self.use_checkpoint:
            # CHECKPOINT_LEVEL 1: recompute in groups of three layers (reference :46-57)
            def run_group(x, first):
                for i in range(first, min(first + 3, self.num_layers)):
                    x = self.layers[i](x, pos, reference_points, spatial_shapes, level_start_index, padding_mask)
                return x
            for first in range(0, self.num_layers, 3):
                output = checkpoint(run_group, output, first, use_reentrant=False)
            return output
        if not self.layer_node:
            for layer in self.layers:
                output = layer(output, pos, reference_points, spatial_shapes, level_start_index, padding_mask)
            return output
        q = None        # a layer that ran as one node hands the next one its query, output + pos, from its last kernel
        for i, layer in enumerate(self.layers):
            output, q = layer(output, pos, reference_points, spatial_shapes, level_start_index, padding_mask, q=q,
                              emit_q=i + 1 < self.num_layers)
        return output


class DeformableEncoderLayer(nn.Module):
    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="ReLU", n_levels=4, n_heads=8, n_points=4,
                 sigmoid_attn=False):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model=d_model, n_levels=n_levels, n_heads=n_heads, n_points=n_points,
                                      sigmoid_attn=sigmoid_attn)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = get_activation_layer(activation=activation)
        self.dropout2 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout3 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, src):
        hidden = self.dropout2(long_linear(src, self.linear1.weight, self.linear1.bias, activation=self.activation))
        return add_layer_norm(src, self.dropout3(long_linear(hidden, self.linear2.weight, self.linear2.bias)), self.norm2)

    def node_usable(self, src, pos, reference_points) -> bool:
        """Whether this call can run as ``EncoderLayerNode``: fp32 CUDA training-graph calls of the configuration the
        fused operator and the 256-wide LayerNorm kernels cover, with nothing between the sublayers (no active dropout)."""
        at = self.self_attn
        return (encoder_layer.enabled() and pos is not None and src.is_cuda and src.dim() == 3 and pos.shape == src.shape
                and src.dtype == torch.float32 and pos.dtype == torch.float32
                and torch.is_grad_enabled() and not torch.is_autocast_enabled()
                and not torch.cuda.is_current_stream_capturing()
                and not (self.training and any(d.p > 0 for d in (self.dropout1, self.dropout2, self.dropout3)))
                and isinstance(self.activation, nn.ReLU) and linear_mod.FUSE_RELU_EPILOGUE
                and msda_mod.FUSED_PROLOGUE and not at.sigmoid_attn
                and MSDA.fused_supported(src.dtype, at.d_model // at.n_heads, at.n_levels, at.n_points)
                and reference_points.dtype == torch.float32 and not reference_points.requires_grad
                and reference_points.shape[-1] in (2, 4)
                and clip_ops.add_layer_norm_supported(src, src, self.norm1)
                and clip_ops.add_layer_norm_supported(src, src, self.norm2)
                and all(p.requires_grad and p.dtype == torch.float32 for p in self.parameters()))

    def forward_node(self, src, q, pos_next, reference_points, spatial_shapes, level_start_index, padding_mask):
        """The layer as one autograd node: (output, output + pos_next or None)."""
        at = self.self_attn
        site = at.__dict__.get("_msda_site")
        if site is None:
            site = at.__dict__["_msda_site"] = MSDA.new_call_site()
        # (as MSDeformAttn.forward: a mask that carries its padded rows is applied by zeroing those rows of `value`)
        mask = padding_mask
        rows = getattr(mask, msda_mod.MASKED_ROWS_ATTR, None) if mask is not None else None
        if rows is not None:
            mask = None
        wq, bq = at._fused_query_projection()
        return encoder_layer.EncoderLayerNode.apply(
            src.contiguous(), q.contiguous(), None if pos_next is None else pos_next.contiguous(),
            reference_points.contiguous(), spatial_shapes, level_start_index,
            None if mask is None else mask.contiguous(), rows, at.n_heads, at.n_points, site, float(self.norm1.eps),
            float(self.norm2.eps), at.value_proj.weight, at.value_proj.bias, wq, bq, at.output_proj.weight,
            at.output_proj.bias, self.norm1.weight, self.norm1.bias, self.linear1.weight, self.linear1.bias,
            self.linear2.weight, self.linear2.bias, self.norm2.weight, self.norm2.bias)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None, q=None,
                emit_q=None):
        """``emit_q`` given (the encoder's loop): returns (output, query of the next layer or None) and may run as one
        autograd node; ``q``: this layer's query ``src + pos`` when the layer in front produced it."""
        if emit_q is not None and self.node_usable(src, pos, reference_points):
            return self.forward_node(src, self.with_pos_embed(src, pos) if q is None else q, pos if emit_q else None,
                                     reference_points, spatial_shapes, level_start_index, padding_mask)
        attn = self.self_attn(self.with_pos_embed(src, pos) if q is None else q, reference_points, src, spatial_shapes,
                              level_start_index, padding_mask)
        src = add_layer_norm(src, self.dropout1(attn), self.norm1)
        out = self.forward_ffn(src)
        return out if emit_q is None else (out, None)
