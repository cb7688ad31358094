"""CPU: the Deformable-DETR variant (USE_DAB: False) of the decoder loop as a capturable module
(models/decoder_graphs.py: PlainDecoderLoop) against the eager branch of ``DeformableDecoder.forward``, the boxes the
decoder hands to the model's heads against the per-level head as the reference states it (models/memotr.py:148-158), and
the torch composition behind ``clip_ops.refine_boxes_split``.  Everything here is the same arithmetic in the same
order, so every comparison is bit for bit."""
import pytest
import torch

from model_helpers import TinyBackbone, patch_operator, small_config

ND, NT, C = 20, 3, 256


def _variant_model(merge):
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    import memotr_amd.modules.ms_deform_attn as mod
    cfg = small_config()
    cfg.update(HIDDEN_DIM=C, FFN_DIM=256, NUM_ENC_LAYERS=1, NUM_DEC_LAYERS=2, USE_DAB=False, MERGE_DET_TRACK_LAYER=merge)
    torch.manual_seed(0)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=ND, n_feature_levels=4, hidden_dim=C,
                   ffn_dim=256, dropout=0.0, use_dab=False).train()
    with torch.no_grad():       # (the offsets, the attention logits and the last box layer start at zero: give them values)
        for m in model.modules():
            if isinstance(m, mod.MSDeformAttn):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
        for head in model.bbox_embed:
            head.layers[-1].weight.normal_(0, 0.05)
    return model


def _frame_and_tracks(model):
    from memotr_amd.structures.track_instances import TrackInstances
    from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor
    g = torch.Generator().manual_seed(7)
    frame = tensor_list_to_nested_tensor([torch.randn(3, 96, 160, generator=g)])
    tr = TrackInstances(hidden_dim=C, num_classes=1, use_dab=False)
    tr.ref_pts = torch.randn(NT, 4, generator=g)
    tr.ref_pts[0, 2:] = torch.tensor([-1.5, 0.75])               # a carried box: its wh is not sigmoid(0) = 0.5
    tr.query_embed = torch.randn(NT, 2 * C, generator=g)
    return frame, [tr]


def _decoder_inputs(model, enc, tracks):
    """What ``DeformableTransformer.decode`` hands to the decoder (models/deformable_transformer.py)."""
    query_embed = model.get_query_embed(tracks)
    query_pos, tgt = torch.split(query_embed, C, dim=2)
    init_ref = model.get_reference_points(tracks).sigmoid()
    return tgt, init_ref, query_pos, model.get_query_mask(tracks)


@pytest.mark.parametrize("merge", [0, 1])
def test_variant_loop_module_equals_the_eager_loop(monkeypatch, merge):
    from memotr_amd.models.decoder_graphs import PlainDecoderLoop, loop_for
    patch_operator(monkeypatch)
    model = _variant_model(merge)
    dec = model.transformer.decoder
    assert not dec.use_dab and not hasattr(dec, "ref_point_head") and dec.merge_det_track_layer == merge
    frame, tracks = _frame_and_tracks(model)
    with torch.no_grad():
        enc = model.encode_frame(frame)
        tgt, init_ref, query_pos, query_mask = _decoder_inputs(model, enc, tracks)
        assert tgt.shape == (1, ND + NT, C) and init_ref.shape == (1, ND + NT, 4)
        eager = dec(tgt=tgt, reference_points=init_ref, src=enc["memory"], src_spatial_shapes=enc["spatial_shapes"],
                    src_level_start_index=enc["level_start_index"], src_valid_ratios=enc["valid_ratios"],
                    query_pos=query_pos, query_mask=query_mask, src_padding_mask=enc["mask_flatten"])
        loop = loop_for(dec, enc["spatial_shapes"], enc["level_start_index"])
        assert isinstance(loop, PlainDecoderLoop)
        assert sorted(n for n, _ in loop.named_children()) == ["bbox_embed", "layers"]
        vr = enc["valid_ratios"]
        ratios4 = torch.cat([vr, vr], -1)[:, None].contiguous()
        looped = loop(tgt, init_ref, query_pos, enc["memory"], vr, ratios4, query_mask, enc["mask_flatten"])
    for name, a, b in zip(("outs", "refs", "layer_inputs", "boxes"), looped, eager):
        assert a.shape == b.shape and torch.equal(a, b), name
    outs, refs, _, boxes = looped
    if merge == 1:      # the track rows did not go through layer 0: they keep their 4-d input anchors
        assert torch.equal(refs[0][:, ND:], init_ref[:, ND:])
    else:               # ... or were refined around the 2-d reference: wh = sigmoid(delta wh) whatever the input wh was
        delta = model.bbox_embed[0](outs[0])
        assert torch.equal(refs[0][..., 2:], delta.sigmoid()[..., 2:])


@pytest.mark.parametrize("merge", [0, 1])
def test_decoder_boxes_equal_the_models_per_level_head(monkeypatch, merge):
    """``boxes`` of the decoder are what ``MeMOTR.decode_frame`` computed per level before it reused them:
    sigmoid(bbox_embed[lvl](output[lvl]) + inverse_sigmoid(reference)), the reference being the 4-d initial one at level
    0 and the decoder's own from then on."""
    from memotr_amd.utils.utils import inverse_sigmoid
    patch_operator(monkeypatch)
    model = _variant_model(merge)
    frame, tracks = _frame_and_tracks(model)
    with torch.no_grad():
        enc = model.encode_frame(frame)
        outputs, init_reference, inter_references, _, refined = model.transformer.decode(
            enc, query_embed=model.get_query_embed(tracks), ref_pts=model.get_reference_points(tracks),
            query_mask=model.get_query_mask(tracks), return_boxes=True)
        heads = []
        for lvl in range(outputs.shape[0]):
            reference = inverse_sigmoid(init_reference if lvl == 0 else inter_references[lvl - 1])
            box = model.bbox_embed[lvl](outputs[lvl])
            assert reference.shape[-1] == 4
            heads.append((box + reference).sigmoid())
        heads = torch.stack(heads)
        res = model.decode_frame(enc, tracks)
    assert refined is not None and torch.equal(refined, heads)
    assert torch.equal(res["pred_bboxes_all"], heads) and torch.equal(res["pred_bboxes"], heads[-1])
    # level 0 carries the 4-d reference: for a track row whose wh is not 0.5 that is not the decoder's 2-d refinement
    wh = init_reference[0, ND, 2:]
    assert (wh - 0.5).abs().min() > 0.1
    delta0 = model.bbox_embed[0](outputs[0])
    two_d = torch.cat((delta0[..., :2] + inverse_sigmoid(init_reference[..., :2]), delta0[..., 2:]), -1).sigmoid()
    assert torch.equal(heads[0][..., :2], two_d[..., :2])
    assert (heads[0][0, ND, 2:] - two_d[0, ND, 2:]).abs().min() > 1e-2
    # the detect queries' wh reference is sigmoid(0) = 0.5: inverse sigmoid exactly 0, head box == decoder box
    assert torch.equal(heads[0][:, :ND], two_d[:, :ND])


def test_split_refine_composition_and_its_gradient():
    from memotr_amd.functions import clip_ops
    from memotr_amd.utils.utils import inverse_sigmoid_reference
    g = torch.Generator().manual_seed(3)
    delta = torch.randn(2, 23, 4, generator=g, requires_grad=True)
    ref = torch.rand(2, 23, 4, generator=g)
    ref[0, 0] = torch.tensor([0.0, 1.0, 1e-5, 0.5])
    ref.requires_grad_(True)
    head, dec = clip_ops.refine_boxes_split(delta, ref)
    assert torch.equal(head, (delta + inverse_sigmoid_reference(ref)).sigmoid())
    xy = delta[..., :2] + inverse_sigmoid_reference(ref[..., :2])          # models/deformable_decoder.py, 2-d references
    assert torch.equal(dec, torch.cat((xy, delta[..., 2:]), -1).sigmoid())
    assert head.requires_grad and not dec.requires_grad
    w = torch.randn(2, 23, 4, generator=g)
    gd, gr = torch.autograd.grad((head * w).sum() + dec.sum(), (delta, ref))
    d2, r2 = delta.detach().clone().requires_grad_(True), ref.detach().clone().requires_grad_(True)
    gd2, gr2 = torch.autograd.grad(((d2 + inverse_sigmoid_reference(r2)).sigmoid() * w).sum(), (d2, r2))
    assert torch.equal(gd, gd2) and torch.equal(gr, gr2)
    with pytest.raises(RuntimeError, match="same"):
        clip_ops.refine_boxes_split(delta, ref[:, :5])
    with pytest.raises(RuntimeError, match="same"):
        clip_ops.refine_boxes_split(delta[..., :2], ref[..., :2])
