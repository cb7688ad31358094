"""GPU: the Deformable-DETR variant (USE_DAB: False) on the captured decoder paths -- the split box refinement of its
layer 0 (include/clip_ops_hip.h: clipops_refine_boxes_split_fwd_f32), the training capture (models/decoder_graphs.py:
PlainDecoderLoop), the inference capture (models/infer_graphs.py) and the one head evaluation per layer
(``MeMOTR.decode_frame`` reusing the decoder's boxes).  The recipes are those of tests/test_model_gpu.py for the DAB
model, restated here with ``USE_DAB=False``."""
import pytest
import torch

from model_helpers import TinyBackbone, small_config

pytestmark = pytest.mark.gpu

SPECIAL = [0.0, 1.0, 1e-5, 5e-6, 1 - 5e-6, 0.5, -0.2, 1.3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build_variant_cuda(**cfg_over):
    from memotr_amd.models.backbone import BackboneWithPE
    from memotr_amd.models.deformable_transformer import build as build_tr
    from memotr_amd.models.memotr import MeMOTR
    from memotr_amd.models.position_embedding import build as build_pe
    from memotr_amd.models.query_updater import build as build_qu
    import memotr_amd.modules.ms_deform_attn as mod
    cfg = small_config()
    cfg.update(HIDDEN_DIM=256, FFN_DIM=256, USE_DAB=False, **cfg_over)
    model = MeMOTR(backbone=BackboneWithPE(TinyBackbone(), build_pe(cfg)), transformer=build_tr(cfg),
                   query_updater=build_qu(cfg), num_classes=1, n_det_queries=cfg["NUM_DET_QUERIES"],
                   n_feature_levels=4, hidden_dim=256, ffn_dim=256, dropout=0.0, use_dab=False)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, mod.MSDeformAttn):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
    return model.cuda()


# ----------------------------------------------------------------------------- the kernel
def _bits(x):
    return x.contiguous().view(torch.int32)


def _split_raw(delta, ref, shift=0):
    """The C entry point on outputs with guard words behind them; ``shift``: floats by which every pointer is moved off
    its 16-byte alignment (the kernel's scalar path)."""
    from memotr_amd.functions import clip_ops
    L = clip_ops._lib()
    n = delta.numel()
    guard = 64
    d = torch.zeros(n + shift, device="cuda")
    r = torch.zeros(n + shift, device="cuda")
    d[shift:] = delta.reshape(-1)
    r[shift:] = ref.reshape(-1)
    head = torch.full((shift + n + guard,), -7.25, device="cuda")
    dec = torch.full((shift + n + guard,), -9.5, device="cuda")
    L.check(L.lib.clipops_refine_boxes_split_fwd_f32(d.data_ptr() + 4 * shift, r.data_ptr() + 4 * shift, n // 4, 1e-5,
                                                     head.data_ptr() + 4 * shift, dec.data_ptr() + 4 * shift,
                                                     torch.cuda.current_stream().cuda_stream),
            "clipops_refine_boxes_split_fwd_f32")
    torch.cuda.synchronize()
    assert bool((head[:shift] == -7.25).all()) and bool((head[shift + n:] == -7.25).all())
    assert bool((dec[:shift] == -9.5).all()) and bool((dec[shift + n:] == -9.5).all())
    return head[shift:shift + n].view(delta.shape), dec[shift:shift + n].view(delta.shape)


def _check_split(delta, ref):
    from memotr_amd.functions import clip_ops
    from memotr_amd.utils.utils import inverse_sigmoid_reference
    want_head = clip_ops.refine_boxes(delta, ref)
    want_wh = clip_ops.refine_boxes(delta, torch.full_like(ref, 0.5))[..., 2:]
    comp_head = (delta + inverse_sigmoid_reference(ref)).sigmoid()
    comp_dec = torch.cat((delta[..., :2] + inverse_sigmoid_reference(ref[..., :2]), delta[..., 2:]), -1).sigmoid()
    for shift in (0, 1):
        head, dec = _split_raw(delta, ref, shift)
        # bit patterns: torch.equal on every element, a NaN row included
        assert torch.equal(_bits(head), _bits(want_head)), shift
        assert torch.equal(_bits(dec[..., :2]), _bits(head[..., :2])), shift
        assert torch.equal(_bits(dec[..., 2:]), _bits(want_wh)), shift
        torch.testing.assert_close(head, comp_head, rtol=1e-5, atol=1e-6, equal_nan=True)
        torch.testing.assert_close(dec, comp_dec, rtol=1e-5, atol=1e-6, equal_nan=True)
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(head), nan)
        assert torch.equal(torch.isnan(dec[..., :2]), nan[..., :2]) and not torch.isnan(dec[..., 2:]).any()
    # the wrapper: the same two tensors, `dec` outside the graph
    d = delta.clone().requires_grad_(True)
    head, dec = clip_ops.refine_boxes_split(d, ref)
    assert torch.equal(_bits(head), _bits(want_head)) and torch.equal(_bits(dec[..., 2:]), _bits(want_wh))
    assert head.requires_grad and not dec.requires_grad
    return d, head, dec


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_split_refine_kernel_is_bit_equal_to_the_refine_kernel(rows):
    from memotr_amd.functions import clip_ops
    g = torch.Generator().manual_seed(rows)
    delta = (torch.randn(rows, 4, generator=g) * 2).cuda()
    if rows == 1:       # four elements: the special values in two halves, then the NaN row
        refs = [torch.tensor([SPECIAL[:4]]), torch.tensor([SPECIAL[4:]]), torch.full((1, 4), float("nan"))]
    else:
        ref = torch.rand(rows, 4, generator=g)
        ref.view(-1)[:8] = torch.tensor(SPECIAL)
        ref[-1] = float("nan")
        refs = [ref]
    for ref in refs:
        ref = ref.cuda()
        d, head, dec = _check_split(delta, ref)
        # the gradient of delta: the refine kernel's backward on `head`, nothing from `dec`
        up = torch.randn(rows, 4, generator=g).cuda()
        (gd,) = torch.autograd.grad((head * up).sum() + dec.sum(), d)
        d2 = delta.clone().requires_grad_(True)
        (gd2,) = torch.autograd.grad((clip_ops.refine_boxes(d2, ref) * up).sum(), d2)
        assert torch.equal(_bits(gd), _bits(gd2))


def test_split_refine_entry_point_refuses_bad_arguments():
    from memotr_amd.functions import clip_ops
    L = clip_ops._lib()
    x = torch.zeros(8, device="cuda")
    f = L.lib.clipops_refine_boxes_split_fwd_f32
    assert f(x.data_ptr(), x.data_ptr(), -1, 1e-5, x.data_ptr(), x.data_ptr(), None) != 0
    assert f(x.data_ptr(), x.data_ptr(), 2, 1e-5, None, x.data_ptr(), None) != 0
    assert f(x.data_ptr(), x.data_ptr(), 2, 1e-5, x.data_ptr(), x.data_ptr(), None) != 0       # aliased outputs
    assert f(None, None, 0, 1e-5, None, None, None) == 0


# ----------------------------------------------------------------------------- training capture
def _variant_clip_step(monkeypatch, graphs: bool, merge: int, clip_len=3):
    """``_d32_clip_step`` of tests/test_model_gpu.py for the variant: hidden 256, ffn 256, one encoder and two decoder
    layers, 192 x 256 frames, 5 ground truths; returns (loss, {param: grad}, decoder graph cache, model)."""
    from memotr_amd.engine import clip_forward_backward, make_synthetic_clip, clip_to_device
    from memotr_amd.models.criterion import build as build_criterion
    monkeypatch.setenv("MEMOTR_DECODER_GRAPHS", "1" if graphs else "0")
    monkeypatch.setenv("MEMOTR_UPDATER_GRAPHS", "1")
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    torch.manual_seed(0)
    over = dict(NUM_ENC_LAYERS=1, NUM_DEC_LAYERS=2, MERGE_DET_TRACK_LAYER=merge)
    model = build_variant_cuda(**over).train()
    cfg = small_config()
    cfg.update(HIDDEN_DIM=256, FFN_DIM=256, USE_DAB=False, MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2,
               LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5, LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0],
               SAMPLE_LENGTHS=[2, 3, 4, 5], **over)
    criterion = build_criterion(cfg)
    batch = clip_to_device(make_synthetic_clip(clip_len=clip_len, height=192, width=256, n_gts=5, seed=3),
                           torch.device("cuda"))
    loss, _ = clip_forward_backward(model, criterion, batch, torch.device("cuda"), use_dab=False)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    cache = model.transformer.decoder.graphs()
    cache.updater = model.query_updater.graphs()
    return float(loss), grads, cache, model


@pytest.mark.parametrize("merge", [0, 1])
def test_variant_decoder_graphs_are_captured_and_match_the_eager_loop(monkeypatch, merge):
    T = 3
    loss_g, grads_g, cache, model = _variant_clip_step(monkeypatch, True, merge, clip_len=T)
    print(f"merge={merge}: captures={cache.captures} replays={cache.replays} eager={cache.eager} failed={cache.failed} "
          f"updater captures={cache.updater.captures}")
    assert cache.captures == T and cache.replays == T and cache.eager == 0 and not cache.failed
    assert cache.updater.captures == T - 1
    # every parameter of the captured loop receives a gradient (DistributedDataParallel, find_unused_parameters=False)
    dec = model.transformer.decoder
    assert dec.bbox_embed is model.bbox_embed
    for n, p in list(dec.layers.named_parameters(prefix="layers")) + list(dec.bbox_embed.named_parameters(prefix="bbox_embed")):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    loss_e, grads_e, cache_e, _ = _variant_clip_step(monkeypatch, False, merge, clip_len=T)
    assert cache_e.captures == 0 and cache_e.replays == 0
    print(f"merge={merge}: loss graphs {loss_g} eager {loss_e} rel {abs(loss_g - loss_e) / abs(loss_e):.3g}")
    worst = max((float((grads_g[n] - grads_e[n]).norm()) / (float(grads_e[n].norm()) + 1e-6), n)
                for n in grads_e if n in grads_g)
    print(f"merge={merge}: worst relative gradient difference {worst}")
    assert abs(loss_g - loss_e) <= 2e-4 * abs(loss_e), (loss_g, loss_e)
    assert grads_g.keys() == grads_e.keys()
    for n in grads_e:
        denom = float(grads_e[n].norm()) + 1e-6
        # float atomics in the operator backward make both runs order-dependent at the 1e-3 level
        assert float((grads_g[n] - grads_e[n]).norm()) / denom < 2e-2, n


# ----------------------------------------------------------------------------- inference capture
def test_variant_inference_graphs_match_the_eager_tracker(monkeypatch):
    from memotr_amd.inference import SequenceTracker
    from memotr_amd.models.utils import logits_to_scores
    from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    g = torch.Generator().manual_seed(11)
    frames = [torch.randn(3, 192, 256, generator=g).cuda() for _ in range(6)]

    def run(graphs):
        monkeypatch.setenv("MEMOTR_INFER_GRAPHS", "1" if graphs else "0")
        torch.manual_seed(4)
        model = build_variant_cuda(NUM_ENC_LAYERS=2, NUM_DEC_LAYERS=2).eval()
        tracker = SequenceTracker(model, det_score_thresh=0.5, track_score_thresh=0.0, result_score_thresh=0.0,
                                  miss_tolerance=5, use_dab=False, area_thresh=0)
        with torch.no_grad():       # random-init scores sit near 0.01: give birth to the three best detections per frame
            res = model(frame=tensor_list_to_nested_tensor([frames[0]]).to(torch.device("cuda")), tracks=tracker.tracks)
            best = logits_to_scores(res["pred_logits"])[0, :len(res["det_query_embed"])].max(-1).values
        tracker.tracker.det_score_thresh = float(best.topk(3).values[-1]) - 1e-6
        outs = []
        for i, f in enumerate(frames):
            if i == 3:
                tracker.tracker.det_score_thresh = 2.0      # ... then none: the live set settles
            outs.append(tracker.step(f, 192, 256))
        return outs, model

    eager, model_e = run(False)
    graphed, model = run(True)
    dec = model.transformer.decoder.infer_graphs().decode
    print(f"decoder inference cache: captures={dec.captures} replays={dec.replays} eager={dec.eager} failed={dec.failed}")
    assert model_e.transformer.decoder.infer_graphs().decode.captures == 0
    assert dec.captures >= 1 and dec.replays >= len(frames) and dec.eager == 0 and not dec.failed
    assert len(eager[-1]) >= 3
    for a, b in zip(eager, graphed):
        assert a.ids.tolist() == b.ids.tolist()
        print("boxes", float((a.boxes - b.boxes).abs().max()) if len(a) else 0.0,
              "scores", float((a.scores - b.scores).abs().max()) if len(a) else 0.0)
        assert torch.allclose(a.boxes, b.boxes, atol=1e-2, rtol=1e-4)          # pixels
        assert torch.allclose(a.scores, b.scores, atol=1e-4)


# ----------------------------------------------------------------------------- heads: one evaluation per layer
def test_variant_level0_head_carries_the_4d_reference_on_the_captured_path(monkeypatch):
    from memotr_amd.structures.track_instances import TrackInstances
    from memotr_amd.utils.nested_tensor import tensor_list_to_nested_tensor
    monkeypatch.setenv("MEMOTR_REQUIRE_GRAPHS", "1")
    nt = 3
    g = torch.Generator().manual_seed(5)
    image = torch.randn(3, 192, 256, generator=g)
    ref_pts = torch.randn(nt, 4, generator=g)
    ref_pts[:, 2:] = torch.tensor([[-1.5, 0.75], [1.0, -2.0], [-0.8, -0.6]])       # carried boxes: wh far from 0.5
    query_embed = torch.randn(nt, 512, generator=g)

    def run(graphs):
        monkeypatch.setenv("MEMOTR_DECODER_GRAPHS", "1" if graphs else "0")
        torch.manual_seed(2)
        model = build_variant_cuda(NUM_ENC_LAYERS=1, NUM_DEC_LAYERS=2, MERGE_DET_TRACK_LAYER=1).train()
        with torch.no_grad():
            for head in model.bbox_embed:
                head.layers[-1].weight.normal_(0, 0.05)
        tr = TrackInstances(hidden_dim=256, num_classes=1, use_dab=False).to(torch.device("cuda"))
        tr.ref_pts, tr.query_embed = ref_pts.cuda(), query_embed.cuda()
        frame = tensor_list_to_nested_tensor([image]).to(torch.device("cuda"))
        enc = dict(model(frame=frame, stage="encode"), frame_slot=0, clip_key=object())
        res = model(tracks=[tr], encoded=enc)
        return res, model

    res_g, model = run(True)
    cache = model.transformer.decoder.graphs()
    assert cache.captures == 1 and cache.replays == 1 and cache.eager == 0 and not cache.failed
    res_e, model_e = run(False)
    assert model_e.transformer.decoder.graphs().captures == 0
    nd = len(res_g["det_query_embed"])
    box0 = res_g["pred_bboxes_all"][0]
    assert box0.shape[1] == nd + nt and box0.requires_grad
    with torch.no_grad():
        delta = model.bbox_embed[0](res_g["aux_outputs"][0]["queries"])          # layer 0's output through its box head
        full = (delta + res_g["init_ref_pts"]).sigmoid()
        two_d = torch.cat((delta[..., :2] + res_g["init_ref_pts"][..., :2], delta[..., 2:]), -1).sigmoid()
    torch.testing.assert_close(box0, full, rtol=1e-5, atol=1e-6)
    assert float((box0[0, nd:, 2:] - two_d[0, nd:, 2:]).abs().min()) > 1e-2
    for k in ("pred_bboxes_all", "pred_logits_all"):
        print(k, float((res_g[k] - res_e[k]).abs().max()))
    torch.testing.assert_close(res_g["pred_bboxes_all"][0], res_e["pred_bboxes_all"][0], rtol=1e-5, atol=1e-6)
