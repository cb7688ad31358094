"""GPU: the deformable-encoder layer as one autograd node (memotr_amd/functions/encoder_layer.py) against the layer
composed from separate nodes (MEMOTR_ENC_LAYER_NODE=0): same forward bits, gradients no further from a float64 run of
the composed layer (CPU, the oracle's torch statement of the operator) than the composed path's own."""
import copy

import pytest
import torch

from model_helpers import patch_operator

pytestmark = pytest.mark.gpu

SHAPES = [(9, 13), (5, 7), (3, 4), (2, 2)]
N, C = 2, 256


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib, clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build_encoder(n_layers=2, use_checkpoint=False, seed=0):
    import torch.nn as nn
    from memotr_amd.models.deformable_encoder import DeformableEncoder, DeformableEncoderLayer
    torch.manual_seed(seed)
    layer = DeformableEncoderLayer(d_model=C, d_ffn=64, dropout=0.0, n_levels=4, n_heads=8, n_points=4)
    enc = DeformableEncoder(layer, n_layers, use_checkpoint=use_checkpoint)
    with torch.no_grad():        # layers that differ, non-degenerate offsets / logits, every bias and gain in play
        for name, p in enc.named_parameters():
            if name.endswith("sampling_offsets.weight"):
                p.normal_(0, 0.02)
            elif name.endswith("attention_weights.weight"):
                p.normal_(0, 0.05)
            elif isinstance(p, nn.Parameter) and p.dim() == 1 and "sampling_offsets" not in name:
                p.add_(torch.randn_like(p) * 0.1)
            elif p.dim() == 2:
                p.add_(torch.randn_like(p) * 0.01)
    return enc.cuda().train()


def make_inputs(seed=1):
    from memotr_amd.models.deformable_transformer import DeformableTransformer
    from memotr_amd.modules.ms_deform_attn import tag_masked_rows
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in SHAPES)
    masks, ratios = [], []
    for h, w in SHAPES:          # a padded border: the last row of every image, one or two columns on the right
        m = torch.zeros(N, h, w, dtype=torch.bool)
        m[:, h - 1:, :] = True
        m[0, :, w - 1:] = True
        m[1, :, max(w - 2, 1):] = True
        masks.append(m.flatten(1))
        ratios.append(DeformableTransformer.get_valid_ratio(m))
    start = [0]
    for h, w in SHAPES[:-1]:
        start.append(start[-1] + h * w)
    return dict(src=torch.randn(N, S, C, generator=g), pos=torch.randn(N, S, C, generator=g) * 0.5,
                up=torch.randn(N, S, C, generator=g), mask=tag_masked_rows(torch.cat(masks, 1).cuda()),
                valid_ratios=torch.stack(ratios, 1), spatial_shapes=torch.tensor(SHAPES, dtype=torch.int64),
                level_start_index=torch.tensor(start, dtype=torch.int64))


def run(enc, x, device, dtype):
    enc.zero_grad()
    to = lambda t: t.to(device=device, dtype=dtype if t.is_floating_point() else None)      # noqa: E731
    src = to(x["src"]).requires_grad_(True)
    pos = to(x["pos"]).requires_grad_(True)          # (the model's carries the learnt level embedding)
    mask = x["mask"] if device == "cuda" else x["mask"].cpu()
    out = enc(src=src, spatial_shapes=to(x["spatial_shapes"]), level_start_index=to(x["level_start_index"]),
              valid_ratios=to(x["valid_ratios"]), pos=pos, padding_mask=mask, shapes_list=SHAPES)
    (out * to(x["up"])).sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in enc.named_parameters()}
    grads["input"] = src.grad.detach().clone()
    grads["pos"] = pos.grad.detach().clone()
    return out.detach(), grads


def test_node_path_equals_the_composed_path_and_is_as_close_to_float64(monkeypatch):
    from memotr_amd.functions.encoder_layer import EncoderLayerNode
    enc, x = build_encoder(), make_inputs()
    n0 = EncoderLayerNode.calls
    out_n, g_n = run(enc, x, "cuda", torch.float32)
    assert EncoderLayerNode.calls == n0 + 2                      # both layers ran as nodes
    monkeypatch.setenv("MEMOTR_ENC_LAYER_NODE", "0")
    out_c, g_c = run(enc, x, "cuda", torch.float32)
    assert EncoderLayerNode.calls == n0 + 2
    assert torch.equal(out_n, out_c)
    # float64 truth: the composed layer on the CPU with the oracle's torch statement of the operator
    patch_operator(monkeypatch)
    out_t, g_t = run(copy.deepcopy(enc).cpu().double(), x, "cpu", torch.float64)
    assert float((out_c.double().cpu() - out_t).abs().max()) < 1e-4
    assert g_n.keys() == g_c.keys() == g_t.keys() and len(g_t) == 2 * 16 + 2
    for name, t in g_t.items():
        scale = float(t.abs().max())
        assert scale > 0, name
        e_n = float((g_n[name].double().cpu() - t).abs().max()) / scale
        e_c = float((g_c[name].double().cpu() - t).abs().max()) / scale
        d_nc = float((g_n[name] - g_c[name]).abs().max()) / scale
        print(f"{name}: node {e_n:.3e} composed {e_c:.3e} node - composed {d_nc:.3e}")
        assert e_n <= 2.0 * e_c + 1e-7, (name, e_n, e_c)
        # (a ReLU or a bilinear cell that falls the other way in float64 puts both paths 1e-3 .. 1e-2 from the truth; the
        #  two fp32 paths see the same cells and differ by the order of fp32 sums over at most 336 rows and by the
        #  operator's float atomics, far below that)
        assert d_nc <= 1e-4, (name, d_nc)


def test_checkpointing_and_autocast_take_the_composed_path():
    from memotr_amd.functions.encoder_layer import EncoderLayerNode
    x = make_inputs()
    n0 = EncoderLayerNode.calls
    run(build_encoder(use_checkpoint=True), x, "cuda", torch.float32)           # CHECKPOINT_LEVEL 1
    assert EncoderLayerNode.calls == n0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        run(build_encoder(), x, "cuda", torch.float32)
    assert EncoderLayerNode.calls == n0
    run(build_encoder(), x, "cuda", torch.float32)
    assert EncoderLayerNode.calls == n0 + 2


def test_bf16_encode_capture_of_one_layer_replays_to_the_eager_output():
    """The add + LayerNorm entry points stay legal inside a hipGraph capture: a 1-layer encoder under bf16 autocast,
    captured and replayed, against the same call run eagerly."""
    from memotr_amd.functions.encoder_layer import EncoderLayerNode
    enc, x = build_encoder(n_layers=1), make_inputs()
    args = dict(src=x["src"].cuda(), spatial_shapes=x["spatial_shapes"].cuda(),
                level_start_index=x["level_start_index"].cuda(), valid_ratios=x["valid_ratios"].cuda(),
                pos=x["pos"].cuda(), padding_mask=x["mask"], shapes_list=SHAPES)
    n0 = EncoderLayerNode.calls

    def call():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return enc(**args)

    eager = call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call()
    for _ in range(2):
        captured.zero_()
        graph.replay()
        assert torch.equal(captured, eager)
    assert EncoderLayerNode.calls == n0
