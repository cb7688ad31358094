"""GPU: the add + LayerNorm kernels of clip_ops ABI 11 -- the forward with the second output q = y + pos and the
backward with up to three gradient inputs and the column sums of its result -- against the kernels they extend (bit
for bit where the arithmetic is the same) and against a float64 statement of the backward."""
import itertools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

C = 256
# a partial wavefront group, a partial workgroup, more than one column-sum chunk (COLSUM_CHUNK_ROWS = 256), many chunks
# of the backward; then the sizes at which the code takes another path: COLSUM_MAX_ROWS + 1 (the existing column sum
# goes from one pass to two) and 4097 (the fan-in backward's rows per workgroup go from 16 to 64)
ROWS = [1, 63, 257, 1037, 2049, 4097]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(clip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_case(rows):
    g = torch.Generator().manual_seed(1000 + rows)
    norm = nn.LayerNorm(C).cuda()
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(C, generator=g) * 0.2)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.3).cuda()
    res = torch.randn(rows, C, generator=g).cuda()
    pos = torch.randn(rows, C, generator=g).cuda()
    grads = [(torch.randn(rows, C, generator=g) * s).cuda() for s in (1.0, 0.5, 2.0)]
    return norm, x, res, pos, grads


@pytest.mark.parametrize("rows", ROWS)
def test_forward_with_pos_is_the_existing_forward_plus_the_query(rows):
    from memotr_amd.functions import clip_ops
    norm, x, res, pos, _ = make_case(rows)
    assert clip_ops.add_layer_norm_supported(x, res, norm)
    y_old = clip_ops.add_layer_norm(x, res, norm).detach()
    s0, y0, q0, st0 = clip_ops.add_layer_norm_fwd(x, res, norm.weight, norm.bias, float(norm.eps))
    s, y, q, st = clip_ops.add_layer_norm_fwd(x, res, norm.weight, norm.bias, float(norm.eps), pos)
    assert q0 is None
    assert torch.equal(y0, y_old) and torch.equal(y, y_old)
    assert torch.equal(s, s0) and torch.equal(st, st0) and torch.equal(s, x + res)
    assert torch.equal(q, y_old + pos)
    s2, y2, q2, st2 = clip_ops.add_layer_norm_fwd(x, res, norm.weight, norm.bias, float(norm.eps), pos)
    assert torch.equal(y2, y) and torch.equal(q2, q) and torch.equal(st2, st)


def backward_truth(gsum64, s64, gamma64, eps):
    mean = s64.mean(-1, keepdim=True)
    rstd = (s64.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (s64 - mean) * rstd
    gh = gsum64 * gamma64
    dz = (gh - gh.mean(-1, keepdim=True) - xh * (gh * xh).mean(-1, keepdim=True)) * rstd
    return dz, (gsum64 * xh).sum(0), gsum64.sum(0), dz.sum(0)


def nerr(got, want64):
    return float((got.double() - want64).abs().max() / want64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("rows", ROWS)
def test_fanin_backward_is_no_less_exact_than_the_existing_backward_and_colsum(rows):
    """Every non-empty choice of the three gradient slots (so: 1, 2 and 3 inputs, a null in every position).  The
    existing kernel gets the gradients summed by torch in the same order, then ``colsum`` over its result.  Both are
    measured against float64 as max |error| / max |truth| per output; the fused kernel may not exceed the existing
    one's figure by more than the factor 2 that covers the order in which the gradient inputs are summed."""
    from memotr_amd.functions import clip_ops
    norm, x, res, _, grads = make_case(rows)
    eps = float(norm.eps)
    s, _, _, stats = clip_ops.add_layer_norm_fwd(x, res, norm.weight, norm.bias, eps)
    s64, gamma64 = x.double() + res.double(), norm.weight.detach().double()
    names = ("dz", "dgamma", "dbeta", "colsum")
    for used in itertools.product((False, True), repeat=3):
        if not any(used):
            continue
        slots = tuple(g if u else None for g, u in zip(grads, used))
        given = [g for g in slots if g is not None]
        truth = backward_truth(sum(g.double() for g in given), s64, gamma64, eps)
        got = clip_ops.add_layer_norm_bwd_fanin(slots, s, stats, norm.weight)
        again = clip_ops.add_layer_norm_bwd_fanin(slots, s, stats, norm.weight)
        for a, b, what in zip(got, again, names):
            assert torch.equal(a, b), f"{what}: two launches differ"
        # the existing path on the same inputs: torch's sum of the gradients, the plain backward, colsum
        gsum = given[0]
        for g in given[1:]:
            gsum = gsum + g
        norm.zero_grad()
        a = x.clone().requires_grad_(True)
        clip_ops.add_layer_norm(a, res, norm).backward(gsum)
        old = (a.grad, norm.weight.grad, norm.bias.grad, clip_ops.colsum(a.grad.contiguous()))
        for f, o, t, what in zip(got, old, truth, names):
            ef, eo = nerr(f, t), nerr(o, t)
            print(f"rows {rows} slots {''.join('x' if u else '-' for u in used)} {what}: fused {ef:.3e} "
                  f"existing {eo:.3e} ratio {ef / eo if eo > 0 else float(ef > 0):.3f}")
            assert ef <= 2.0 * eo, (what, used, ef, eo)


def test_fanin_backward_refuses_a_call_without_a_gradient():
    from memotr_amd.functions import clip_ops
    norm, x, res, _, _ = make_case(4)
    s, _, _, stats = clip_ops.add_layer_norm_fwd(x, res, norm.weight, norm.bias, float(norm.eps))
    with pytest.raises(RuntimeError, match="no gradient input"):
        clip_ops.add_layer_norm_bwd_fanin((None, None, None), s, stats, norm.weight)
