"""GPU: the clip-step kernels (include/clip_ops_hip.h) against float64 CPU truth (tests/clip_truth.py) at their lane, tile
and tie edges.  Every comparison is against float64 truth, or against an aten / same-kernel result that has to match bit
for bit.  Bounds come from two rules only (tests/clip_truth.py): the analytic fp32 round-off of a sum, or 4 x the error
the fp32 torch formulation makes on the same inputs on the same GPU + one fp32 ulp of the output scale -- measured inside
the test, never taken from the kernel.  Each check prints `TRUTH <case> <what> ref=<err> kernel=<err> bound=<b>`
(pytest -s); profiles/clip_truth.md records a run.

What an all-masked batch gets (documented in the header, nothing asserted beyond the call returning): out NaN,
lse -inf, all three gradients zero.
"""
import pytest
import torch

import clip_truth as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def check(case, what, got, ref, truth, failures):
    """The measured rule for one tensor; collects instead of stopping so that a run reports every figure."""
    kern, base, scale = T.max_err(got, truth), T.max_err(ref, truth), T.out_scale(truth)
    bound = T.measured_bound(base, scale)
    print(f"TRUTH {case} {what} ref={base:.3e} kernel={kern:.3e} bound={bound:.3e} scale={scale:.3e}")
    if not kern <= bound:
        failures.append(f"{case} {what}: kernel error {kern:.3e} > bound {bound:.3e} (reference error {base:.3e}, scale {scale:.3e})")


def check_analytic(case, what, got, truth, bound, failures):
    kern = T.max_err(got, truth)
    print(f"TRUTH {case} {what} kernel={kern:.3e} bound={bound:.3e}")
    if not kern <= bound:
        failures.append(f"{case} {what}: kernel error {kern:.3e} > analytic bound {bound:.3e}")


def cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------------ attention
def run_attention(q, k, v, up, H, mask, packed):
    """(out, grad q, grad k, grad v) through clip_ops.attention, or clip_ops.self_attention on the packed [q | k]."""
    from memotr_amd.functions import clip_ops
    q, k, v, up, mask = cuda(q, k, v, up, mask)
    if packed:
        qk = torch.cat((q, k), -1).requires_grad_(True)
        vv = v.clone().requires_grad_(True)
        out = clip_ops.self_attention(qk, vv, mask, H)
        (out * up).sum().backward()
        E = q.shape[-1]
        return out.detach(), qk.grad[..., :E], qk.grad[..., E:], vv.grad
    a, b, c = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = clip_ops.attention(a, b, c, H, mask)
    (out * up).sum().backward()
    return out.detach(), a.grad, b.grad, c.grad


def run_attention_reference(q, k, v, up, H, mask):
    from memotr_amd.functions import clip_ops
    q, k, v, up, mask = cuda(q, k, v, up, mask)
    qk = torch.cat((q, k), -1).requires_grad_(True)
    vv = v.clone().requires_grad_(True)
    out = clip_ops.self_attention_reference(qk, vv, mask, H)
    (out * up).sum().backward()
    E = q.shape[-1]
    return out.detach(), qk.grad[..., :E], qk.grad[..., E:], vv.grad


ATTN_NAMES = ("out", "grad_q", "grad_k", "grad_v")


def attention_case(case, q, k, v, up, H, mask, failures):
    truth = T.attention_truth_with_grads(q, k, v, up, H, mask)
    ref = run_attention_reference(q, k, v, up, H, mask)
    got = run_attention(q, k, v, up, H, mask, packed=False)
    for name, g, r, t in zip(ATTN_NAMES, got, ref, truth):
        check(case, name, g, r, t, failures)
    packed = run_attention(q, k, v, up, H, mask, packed=True)          # other strides, same kernels: same bits
    for name, g, p in zip(ATTN_NAMES, got, packed):
        if not torch.equal(g, p):
            failures.append(f"{case} {name}: packed (B, L, 2E) layout differs from three contiguous tensors")
    return got


@pytest.mark.parametrize("L", T.ATTN_LENGTHS)
def test_attention_lengths_heads_batches(L):
    """16 rows x 16 lanes per workgroup: L = 17 leaves a second workgroup one row, 15 / 31 / 33 leave lanes without a
    key, 511 / 512 fill the LDS; H = 1 and 3 besides the model's 8."""
    failures = []
    for H in T.ATTN_HEADS:
        for B in T.ATTN_BATCHES:
            q, k, v, up = T.attn_inputs(B, L, H)
            attention_case(f"attn L={L} H={H} B={B}", q, k, v, up, H, None, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", ["starved_lane", "single_live_key", "even_keys"])
def test_attention_interior_masks(name):
    failures = []
    B, L, mask = T.attn_mask_case(name)
    for H in (1, 8):
        q, k, v, up = T.attn_inputs(B, L, H, seed=L + H)
        got = attention_case(f"attn mask={name} H={H}", q, k, v, up, H, mask, failures)
        dead = mask.cuda()
        assert float(got[2][dead].abs().max()) == 0.0 and float(got[3][dead].abs().max()) == 0.0       # exactly zero
    assert not failures, "\n".join(failures)


def test_attention_dead_batch_leaves_its_neighbour_alone():
    """All keys of batch 1 masked: batch 0 is bit-equal to the same call with B = 1.  Batch 1 itself gets out = NaN
    (0 * inf: there is no softmax over nothing), lse = -inf and zero gradients -- documented, not asserted."""
    B, L, mask = T.attn_mask_case("dead_batch")
    H = 3
    q, k, v, up = T.attn_inputs(B, L, H)
    both = run_attention(q, k, v, up, H, mask, packed=False)
    alone = run_attention(q[:1], k[:1], v[:1], up[:1], H, mask[:1], packed=False)
    torch.cuda.synchronize()
    for name, a, b in zip(ATTN_NAMES, both, alone):
        assert torch.equal(a[:1], b), name
    failures = []
    truth = T.attention_truth_with_grads(q[:1], k[:1], v[:1], up[:1], H, mask[:1])
    ref = run_attention_reference(q[:1], k[:1], v[:1], up[:1], H, mask[:1])
    for name, g, r, t in zip(ATTN_NAMES, alone, ref, truth):
        check("attn dead_batch batch0", name, g, r, t, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_attention_large_logits(order):
    """Scores of about +-80 (q, k ~ N(0, 4.4^2)), keys sorted by row 0's score: ascending makes every key a new running
    maximum of the online softmax (corr = exp(m - m_new) each step), and exp(s - lse) of the backward sees |s| near 80."""
    failures = []
    q, k, v, up = T.attn_large_logit_inputs(order)
    attention_case(f"attn large_logits {order}", q, k, v, up, T.ATTN_LARGE_H, None, failures)
    assert not failures, "\n".join(failures)


def test_attention_strided_operands_and_outputs():
    """q, k, v as three column slices of one (B, L, 5E) buffer and the gradients into slices of a sentinel-filled
    (B, L, 5E) buffer, through the C ABI: bit-equal to the contiguous call, sentinel untouched elsewhere."""
    from memotr_amd import _clip_lib as L_
    B, L, H = 2, 33, 3
    E = 32 * H
    q, k, v, up = cuda(*T.attn_inputs(B, L, H))
    want = run_attention(q, k, v, up, H, None, packed=False)
    buf = torch.full((B, L, 5 * E), 123.0, device="cuda")
    buf[..., 3 * E:4 * E], buf[..., E:2 * E], buf[..., 4 * E:] = q, k, v          # q, k, v at columns 3E, E, 4E
    qs, ks, vs = buf[..., 3 * E:4 * E], buf[..., E:2 * E], buf[..., 4 * E:]
    SENT = -7.25
    gbuf = torch.full((B, L, 5 * E), SENT, device="cuda")
    gq, gk, gv = gbuf[..., 0:E], gbuf[..., 2 * E:3 * E], gbuf[..., 4 * E:]
    out = torch.empty(B, L, E, device="cuda")
    lse = torch.empty(B, H, L, device="cuda")
    scale = 1.0 / 32 ** 0.5
    bs, rs = L * 5 * E, 5 * E
    stream = torch.cuda.current_stream().cuda_stream
    L_.check(L_.lib.clipops_mha_fwd_f32(qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), bs, rs, bs, rs, bs, rs, None, B, H, L,
                                        scale, out.data_ptr(), lse.data_ptr(), stream), "clipops_mha_fwd_f32")
    L_.check(L_.lib.clipops_mha_bwd_f32(qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), bs, rs, bs, rs, bs, rs, None,
                                        out.data_ptr(), lse.data_ptr(), up.data_ptr(), B, H, L, scale, gq.data_ptr(), bs, rs,
                                        gk.data_ptr(), bs, rs, gv.data_ptr(), bs, rs, stream), "clipops_mha_bwd_f32")
    torch.cuda.synchronize()
    for name, a, b in zip(ATTN_NAMES, (out, gq, gk, gv), want):
        assert torch.equal(a, b), name
    assert bool((gbuf[..., E:2 * E] == SENT).all()) and bool((gbuf[..., 3 * E:4 * E] == SENT).all())


# ------------------------------------------------------------------------------------------------ add + LayerNorm
@pytest.fixture(scope="module")
def ln_chunk_rows():
    """The chunk_rows clip_ops.add_layer_norm passes for a few rows, read off the call it makes."""
    return _ln_run(*T.ln_inputs("randn", 5), want_chunk=True)[-1]


def _ln_run(x, res, gamma, beta, up, want_chunk=False):
    import torch.nn as nn
    from memotr_amd import _clip_lib as L_
    from memotr_amd.functions import clip_ops
    norm = nn.LayerNorm(T.LN_COLS).cuda()
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    a, b, up = (t.cuda() for t in (x, res, up))
    a.requires_grad_(True), b.requires_grad_(True)
    assert clip_ops.add_layer_norm_supported(a, b, norm)
    seen = []
    real = L_.lib.clipops_add_layer_norm_bwd_f32

    def spy(*args):
        seen.append(int(args[5]))
        return real(*args)

    L_.lib.clipops_add_layer_norm_bwd_f32 = spy
    try:
        y = clip_ops.add_layer_norm(a, b, norm)
        (y * up).sum().backward()
    finally:
        L_.lib.clipops_add_layer_norm_bwd_f32 = real
    assert len(seen) == 1
    res_ = (y.detach(), a.grad, b.grad, norm.weight.grad, norm.bias.grad)
    return res_ + (seen[0],) if want_chunk else res_


def _ln_reference(x, res, gamma, beta, up):
    import torch.nn.functional as F
    a, b, g, be, up = (t.cuda() for t in (x, res, gamma, beta, up))
    for t in (a, b, g, be):
        t.requires_grad_(True)
    y = F.layer_norm(a + b, (T.LN_COLS,), g, be, 1e-5)
    (y * up).sum().backward()
    return y.detach(), a.grad, b.grad, g.grad, be.grad


def _ln_truth(x, res, gamma, beta, up):
    xs = [T.f64(t).requires_grad_(True) for t in (x, res, gamma, beta)]
    y = T.add_layer_norm_truth(*xs, T.f32_scalar(1e-5))
    (y * T.f64(up)).sum().backward()
    return (y.detach(),) + tuple(t.grad for t in xs)


LN_NAMES = ("y", "grad_x", "grad_res", "grad_gamma", "grad_beta")
LN_ROWS = ("1", "3", "4", "5", "c-1", "c", "c+1", "2c+3")      # c = chunk_rows of the backward's partial sums


@pytest.mark.parametrize("kind", T.LN_DATA)
@pytest.mark.parametrize("rows_spec", LN_ROWS)
def test_add_layer_norm_truth(kind, rows_spec, ln_chunk_rows):
    c = ln_chunk_rows
    rows = {"c-1": c - 1, "c": c, "c+1": c + 1, "2c+3": 2 * c + 3}.get(rows_spec) or int(rows_spec)
    inputs = T.ln_inputs(kind, rows)
    got = _ln_run(*inputs, want_chunk=True)
    assert got[-1] == c                                   # the row counts do straddle the chunk this call used
    truth, ref = _ln_truth(*inputs), _ln_reference(*inputs)
    failures = []
    for name, g, r, t in zip(LN_NAMES, got, ref, truth):
        check(f"ln {kind} rows={rows}", name, g, r, t, failures)
    if kind == "constant_rows":
        for r in T.ln_constant_rows(rows):
            assert torch.equal(got[0][r].cpu(), inputs[3])                 # var = 0: y == beta exactly
        assert all(bool(torch.isfinite(g).all()) for g in got[:5])
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ box kernels
def test_pair_box_loss_and_iou_on_ties_and_shared_edges():
    """Values and the FULL gradient against float64 autograd, tie rows included: the kernel's half-and-half rule on
    max / min ties and its >= 0 clamp sub-gradient are torch's (which fp32 and float64 autograd share here: every
    decision is exact on the 1/64 grid)."""
    from memotr_amd.functions import clip_ops
    pred, tgt, up = T.box_pairs()
    n = pred.shape[0]
    lay, qi = torch.zeros(n, dtype=torch.long).cuda(), torch.arange(n).cuda()
    w = torch.rand(n, generator=torch.Generator().manual_seed(1))
    failures = []
    for weight in (None, w):
        res = {}
        for name, fn in (("kernel", clip_ops.pair_box_loss), ("torch", clip_ops.pair_box_loss_reference)):
            x = pred.cuda().view(1, 1, n, 4).clone().requires_grad_(True)
            l1, gl = fn(x, lay, qi, 0, tgt.cuda(), None, None if weight is None else weight.cuda())
            (l1 * up[0].cuda() + gl * up[1].cuda()).sum().backward()
            res[name] = (l1.detach(), gl.detach(), x.grad.view(n, 4))
        x = pred.double().requires_grad_(True)
        l1, gl = T.pair_box_loss_truth(x, tgt.double(), None if weight is None else weight.double())
        (l1 * up[0].double() + gl * up[1].double()).sum().backward()
        truth = (l1.detach(), gl.detach(), x.grad)
        case = "pair_box_loss" + ("" if weight is None else " weighted")
        for what, g, r, t in zip(("l1", "giou_loss", "grad_boxes"), res["kernel"], res["torch"], truth):
            check(case, what, g, r, t, failures)
        ne = len(T.BOX_EDGE_PAIRS)              # the edge rows on their own: the random rows do not set their bound
        check(case, "grad_boxes[edge rows]", res["kernel"][2][:ne], res["torch"][2][:ne], truth[2][:ne], failures)
    got = clip_ops.pair_iou(pred.cuda(), tgt.cuda())
    ref = clip_ops.pair_iou_reference(pred.cuda(), tgt.cuda())
    check("pair_iou", "iou", got, ref, T.pair_iou_truth(pred.double(), tgt.double()), failures)
    gidx = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    got = clip_ops.pair_iou(pred.cuda(), tgt.cuda(), gidx.cuda())
    ref = clip_ops.pair_iou_reference(pred.cuda(), tgt.cuda(), gidx.cuda())
    check("pair_iou indexed", "iou", got, ref, T.pair_iou_truth(pred.double(), tgt.double()[gidx]), failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("labels", ["random", "out_of_range"])
def test_match_cost_truth(K, labels):
    """|logit| <= 12: beyond that the reference's +1e-8 inside the logarithms is absorbed by 1 - p in fp32 but not in
    float64, and truth stops being the function the reference computes.  Labels -1 and K are clamped into [0, K).
    Strided (layer, batch, query) views, as the criterion passes them."""
    from memotr_amd.functions import clip_ops
    from memotr_amd.models.matcher import HungarianMatcher
    n_layers, B, Q, Nq, Tn = 3, 2, 37, 41, 7
    logits, boxes, gt_labels, gt_boxes = T.match_cost_inputs(n_layers, B, Q, Nq, K, Tn, labels)
    lg, bx = logits.cuda()[:, 1, :Q], boxes.cuda()[:, 1, :Q]
    assert not lg.is_contiguous()
    got = clip_ops.match_cost(lg, bx, gt_labels.cuda(), gt_boxes.cuda(), 2.0, 5.0, 2.0)
    ref = HungarianMatcher(2.0, 5.0, 2.0).cost_matrix_stacked(lg, bx, gt_labels.clamp(0, K - 1).cuda(), gt_boxes.cuda())
    truth = T.match_cost_truth(lg.cpu().double(), bx.cpu().double(), gt_labels, gt_boxes.double(), 2.0, 5.0, 2.0)
    failures = []
    check(f"match_cost K={K} labels={labels}", "cost", got, ref, truth, failures)
    empty = clip_ops.match_cost(lg, bx, gt_labels[:0].cuda(), gt_boxes[:0].cuda(), 2.0, 5.0, 2.0)       # T = 0
    torch.cuda.synchronize()
    assert empty.shape == (n_layers, Q, 0)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ focal loss
@pytest.mark.parametrize("K,Nq", T.FOCAL_SHAPES)
def test_focal_loss_truth(K, Nq):
    """Logits on an even grid over [-90, 90] (expf(-x) overflows at 88.72), gamma != 2 (powf) and gamma == 0,
    alpha < 0, Nq * K on both sides of the 256 threads of a workgroup, strided logits."""
    from memotr_amd.functions import clip_ops
    failures = []
    for kind in T.FOCAL_LABELS:
        buf, labels, up = T.focal_inputs(K, Nq, kind)
        for alpha, gamma in T.FOCAL_PARAMS:
            res = {}
            for name, fn in (("kernel", clip_ops.focal_loss_per_layer), ("torch", clip_ops.focal_loss_per_layer_reference)):
                x = buf.cuda().requires_grad_(True)
                loss = fn(x[:, 1, :Nq], labels.cuda(), alpha, gamma)
                (loss * up.cuda()).sum().backward()
                res[name] = (loss.detach(), x.grad[:, 1, :Nq])
            x = buf[:, 1, :Nq].double().requires_grad_(True)
            loss = T.focal_truth(x, labels, alpha, gamma)
            (loss * up.double()).sum().backward()
            case = f"focal K={K} Nq={Nq} labels={kind} alpha={alpha} gamma={gamma}"
            assert bool(torch.isfinite(res["kernel"][0]).all()) and bool(torch.isfinite(res["kernel"][1]).all()), case
            check(case, "loss", res["kernel"][0], res["torch"][0], loss.detach(), failures)
            check(case, "grad_logits", res["kernel"][1], res["torch"][1], x.grad, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ sine embedding
def test_sine_embed_truth():
    from memotr_amd.functions import clip_ops
    from memotr_amd.models.utils import _sine_dims
    pos = T.sine_positions()
    dim_t = _sine_dims(128, 10000, torch.device("cuda"))
    scale = 6.283185307179586
    up = torch.randn(pos.shape[0], 4 * 128, generator=torch.Generator().manual_seed(0))
    res = {}
    for name in ("kernel", "torch"):
        x = pos.cuda().requires_grad_(True)
        if name == "kernel":
            y = clip_ops.sine_embed(x, dim_t, scale)
        else:
            e = (x * scale)[..., None] / dim_t
            y = torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-3)
        (y * up.cuda()).sum().backward()
        res[name] = (y.detach(), x.grad)
    x = pos.double().requires_grad_(True)
    y = T.sine_embed_truth(x, dim_t.cpu().double(), T.f32_scalar(scale))
    (y * up.double()).sum().backward()
    failures = []
    check("sine_embed", "out", res["kernel"][0], res["torch"][0], y.detach(), failures)
    check("sine_embed", "grad_pos", res["kernel"][1], res["torch"][1], x.grad, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ linears
@pytest.mark.parametrize("rows,in_f,out_f", T.LINEAR_SHAPES)
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_linear_tiles_at_their_edges(rows, in_f, out_f, relu, monkeypatch):
    """in_features 4, 8, 12: the contraction is shorter than the four wavefronts that split it (chunks of 8 k: 1, 1, 2);
    31 / 32 / 33 rows and outputs sit on either side of a 32 x 32 tile.  The suite's 4e-7 sqrt(K) bound against
    float64 products (fp32 MFMA is an fmaf chain: fp32 round-off of a K-term sum)."""
    from memotr_amd.functions import clip_ops
    monkeypatch.setattr(clip_ops, "LINEAR_FWD_MAX_IN", 4096)
    x, w, b, gy = cuda(*T.linear_inputs(rows, in_f, out_f))
    assert clip_ops.linear_fwd_usable(x, w, b) and clip_ops.linear_bwd_usable(gy, x, w)
    failures = []
    got = clip_ops.linear_fwd(x, w, b, relu)
    want = T.linear_truth(T.f64(x), T.f64(w), T.f64(b), relu)
    case = f"linear {rows}x{in_f}->{out_f} relu={relu}"
    check_analytic(case, "y", got, want, 4e-7 * in_f ** 0.5 * (float(want.abs().max()) + 1.0), failures)
    y = got if relu else None
    gx, gw, gb = clip_ops.linear_bwd(gy, y, x, w)
    gm = T.f64(gy) * ((T.f64(y) > 0).double() if relu else 1.0)
    for what, g, t, k in (("grad_x", gx, gm @ T.f64(w), out_f), ("grad_w", gw, gm.t() @ T.f64(x), rows),
                          ("grad_b", gb, gm.sum(0), rows)):
        check_analytic(case, what, g, t, 4e-7 * k ** 0.5 * (float(t.abs().max()) + 1e-6) + 1e-6, failures)
    assert not failures, "\n".join(failures)


def test_linear_backward_masks_like_threshold_backward_on_nan_and_negative_zero():
    """y_relu with a NaN and a -0.0: the masked gradient that feeds grad_x, grad_w and grad_b is aten's
    threshold_backward bit for bit (NaN passes g, -0.0 blocks it).  Small-integer operands make every sum exact in
    any order, so the three results expose the mask exactly."""
    from memotr_amd.functions import clip_ops
    x, w, gy, y = cuda(*T.linear_integer_inputs())
    masked = torch.ops.aten.threshold_backward(gy, y, 0.0)
    assert float(masked[0, 0]) == 7.0 and float(masked[1, 1]) == 0.0
    gx, gw, gb = clip_ops.linear_bwd(gy, y, x, w)
    m = T.f64(masked)
    assert torch.equal(T.f64(gx), m @ T.f64(w))
    assert torch.equal(T.f64(gw), m.t() @ T.f64(x))
    assert torch.equal(T.f64(gb), m.sum(0))


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_rows():
    from memotr_amd.functions import clip_ops
    return (clip_ops.COLSUM_MAX_ROWS - 1, clip_ops.COLSUM_MAX_ROWS, clip_ops.COLSUM_MAX_ROWS + 1,
            clip_ops.COLSUM_CHUNK_ROWS - 1, clip_ops.COLSUM_CHUNK_ROWS + 1)


@pytest.mark.parametrize("cols", [1, 31, 32, 33])
def test_column_sums_of_cancelling_rows(cols):
    """Alternating +-1e4 rows plus randn at partial 32-column tiles and around the one-pass / two-pass and chunk
    boundaries; bound 2^-24 * sqrt(rows) * max|x| (fp32 round-off of a sum whose partial sums stay at the size of its
    terms).  The same for the fused ReLU mask + column sums, whose mask must be aten's bit for bit."""
    from memotr_amd.functions import clip_ops
    failures = []
    for rows in _colsum_rows():
        x = T.colsum_inputs(rows, cols)
        xg = x.cuda()
        got = clip_ops.colsum(xg)
        bound = T.colsum_bound(rows, float(x.abs().max()))
        check_analytic(f"colsum {rows}x{cols}", "sum", got, T.colsum_truth(x.double()), bound, failures)
        assert torch.equal(clip_ops.colsum(xg), got)                                  # a second call: identical bits
        # the activation blocks whole PAIRS of neighbouring rows (every fifth pair, and one column more often), so
        # that what is summed is still the alternating, cancelling data the bound is stated for; a mask that is random
        # per element leaves sums of ~1e5 per chunk, whose fp32 partials (the ABI's float buffer) cost half an ulp of
        # that each -- 0.031 against 0.027 measured at 2048 x 31, see profiles/clip_truth.md
        pair = torch.arange(rows) // 2
        y = torch.where((pair % 5 == 0)[:, None] | ((pair % 3 == 0)[:, None] & (torch.arange(cols) == cols - 1)),
                        -1.0, 1.0).cuda()
        g2, gb = clip_ops.relu_bwd_colsum(xg, y)
        masked = torch.ops.aten.threshold_backward(xg, y, 0.0)
        assert torch.equal(g2, masked)
        check_analytic(f"relu_bwd_colsum {rows}x{cols}", "sum", gb, T.f64(masked).sum(0), bound, failures)
        g2b, gbb = clip_ops.relu_bwd_colsum(xg, y)
        assert torch.equal(g2b, g2) and torch.equal(gbb, gb)
    assert not failures, "\n".join(failures)
