"""GPU: the two kernels of memotr_amd/csrc/opt_ops.hip through ``ClipAdamW`` against the float64 truth and the derived
bound of tests/optim_truth.py -- every path of the kernels (16-byte, 4-byte, tails, one and several chunks per tensor,
tensors without a gradient), non-finite gradients, run-to-run identity and the exchange of state with torch's AdamW."""
import copy

import numpy as np
import pytest
import torch

import optim_truth as T

pytestmark = pytest.mark.gpu

GROUP_LR = (1e-3, 0.0, 2e-4, 5e-3)
GROUP_WD = (1e-2, 5e-4, 0.0, 0.1)


@pytest.fixture(scope="module")
def opt():
    from memotr_amd.build import build_opt_lib
    build_opt_lib()
    from memotr_amd import _opt_lib, optim
    return optim, _opt_lib


def sizes(C):
    return (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 7)


def make_params(seed, shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=g) * 0.5).cuda()) for n in shapes]


def grouped(params):
    return [{"params": params[i::4], "lr": GROUP_LR[i], "weight_decay": GROUP_WD[i]} for i in range(4)]


def set_grads(params, seed, scale, skip=()):
    """Gaussian gradients; |g| >= 2^-20 * scale, so that no g, g^2 (1 - b2) or product with the clip factor is subnormal."""
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        grad = torch.randn(p.shape, generator=g)
        grad = torch.where(grad.abs() < 2.0 ** -20, torch.full_like(grad, 2.0 ** -20), grad) * scale
        p.grad = None if i in skip else grad.cuda()


def checked_step(optimizer, max_norm):
    """One step held to the bound; returns (worst ratios, the norm tensor)."""
    before = T.snapshot(optimizer)
    grads = [None if b["g"] is None else b["g"].copy() for b in before]
    norm = optimizer.step(max_norm=max_norm)
    assert norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float32
    after = T.snapshot(optimizer)
    for a, g in zip(after, grads):                                    # .grad is as the backward wrote it
        assert (a["g"] is None and g is None) or np.array_equal(a["g"].view(np.uint32), g.view(np.uint32))
    worst = T.check_step(before, after, T.hyper(optimizer), max_norm, float(norm))
    print(worst)
    return worst, norm


@pytest.mark.parametrize("max_norm,scale", [(0.1, 1.0), (0.1, 1e-4), (None, 1.0)],
                         ids=["clip-active", "clip-inactive", "no-clip"])
def test_every_length_five_steps_within_the_bound(opt, max_norm, scale):
    optim, L = opt
    params = make_params(0, sizes(L.CHUNK))
    optimizer = optim.ClipAdamW(grouped(params))
    for step in range(5):
        set_grads(params, 10 + step, scale)
        coef = T.one_step(T.snapshot(optimizer), T.hyper(optimizer), max_norm)["coef"]
        assert (coef < 0.01) if (max_norm and scale == 1.0) else (coef == 1.0)       # clipping is active / is not
        worst, _ = checked_step(optimizer, max_norm)
        assert max(worst.values()) <= 1.0, (step, worst)
    assert all(float(optimizer.state[p]["step"]) == 5.0 for p in params)
    assert optimizer._plan.n_chunks == 14 + 1 + 2          # C + 1 spans two chunks, 2 C + 7 three


def test_views_at_any_4_byte_offset_take_the_scalar_path(opt):
    optim, L = opt
    C = L.CHUNK
    g = torch.Generator().manual_seed(1)
    lengths = (257, C + 5, 64, 2 * C)
    offsets = ((1, 1), (0, 3), (3, 0), (1, 2))              # (parameter, gradient) start, in floats
    bufs = [(torch.randn(n + 8, generator=g) * 0.5).cuda() for n in lengths]
    guard = [b.clone() for b in bufs]
    params = [torch.nn.Parameter(b[po:po + n]) for b, n, (po, _) in zip(bufs, lengths, offsets)]
    assert [p.data_ptr() % 16 for p in params] == [4, 0, 12, 4]
    optimizer = optim.ClipAdamW(params, lr=1e-3, weight_decay=0.01)
    for step in range(2):
        gbufs = [torch.randn(n + 8, generator=g).cuda() for n in lengths]
        for p, gb, n, (_, go) in zip(params, gbufs, lengths, offsets):
            p.grad = gb[go:go + n]
        assert [p.grad.data_ptr() % 16 for p in params] == [4, 12, 0, 8]
        worst, _ = checked_step(optimizer, 0.1)
        assert max(worst.values()) <= 1.0, (step, worst)
    for b, g0, n, (po, _) in zip(bufs, guard, lengths, offsets):      # nothing outside the views was written
        assert torch.equal(b[:po], g0[:po]) and torch.equal(b[po + n:], g0[po + n:])


def test_tensors_without_a_gradient_are_not_touched(opt):
    optim, L = opt
    params = make_params(2, (L.CHUNK + 3, 130, 517))
    optimizer = optim.ClipAdamW(params, lr=1e-3)
    set_grads(params, 3, 1.0)
    optimizer.step(0.1)
    set_grads(params, 4, 1.0, skip=(1,))
    worst, _ = checked_step(optimizer, 0.1)                 # (check_step asserts row 1 bit-unchanged: p, m, v, step)
    assert max(worst.values()) <= 1.0, worst
    assert [float(optimizer.state[p]["step"]) for p in params] == [2.0, 1.0, 2.0]
    set_grads(params, 5, 1.0, skip=(0, 1, 2))
    before = T.snapshot(optimizer)
    norm = optimizer.step(0.1)
    assert float(norm) == 0.0
    T.check_step(before, T.snapshot(optimizer), T.hyper(optimizer), 0.1, 0.0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradients_follow_torch(opt, bad):
    optim, L = opt
    params = make_params(6, (9, L.CHUNK + 40))
    optimizer = optim.ClipAdamW(params, lr=1e-3)
    set_grads(params, 7, 1.0)
    optimizer.step(0.1)
    set_grads(params, 8, 1.0)
    params[1].grad[L.CHUNK + 3] = bad
    before = T.snapshot(optimizer)
    norm = optimizer.step(0.1)
    after = T.snapshot(optimizer)
    worst = T.check_step(before, after, T.hyper(optimizer), 0.1, float(norm))    # equal NaN masks, bound where finite
    assert max(worst.values()) <= 1.0, worst
    if bad == float("inf"):
        assert float(norm) == float("inf")
        assert np.isnan(after[1]["p"]).sum() == 1 and not np.isnan(after[0]["p"]).any()
    else:
        assert np.isnan(float(norm)) and all(np.isnan(a[k]).all() for a in after for k in ("p", "m", "v"))


def test_two_runs_give_the_same_bits(opt):
    optim, L = opt
    runs = []
    for _ in range(2):
        params = make_params(0, sizes(L.CHUNK))
        optimizer = optim.ClipAdamW(grouped(params))
        norms = []
        for step in range(2):
            set_grads(params, 50 + step, 1.0)
            norms.append(optimizer.step(0.1))
        runs.append((T.snapshot(optimizer), torch.stack(norms).cpu()))
    (a, na), (b, nb) = runs
    assert torch.equal(na, nb)
    for ra, rb in zip(a, b):
        for k in ("p", "m", "v"):
            assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k


def small_model_and_config():
    from model_helpers import build_small_memotr, small_config
    cfg = small_config()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3], LR=2e-4, LR_BACKBONE=2e-5,
               LR_POINTS=1e-5, WEIGHT_DECAY=5e-4, CLIP_MAX_NORM=0.1)
    torch.manual_seed(0)
    return build_small_memotr().cuda().train(), cfg


def test_the_models_parameter_list_and_the_way_back_to_torch(opt):
    optim, L = opt
    from memotr_amd.engine import get_param_groups
    model, cfg = small_model_and_config()
    groups, _ = get_param_groups(cfg, model)
    optimizer = optim.ClipAdamW(groups, lr=cfg["LR"], weight_decay=cfg["WEIGHT_DECAY"])
    params = [p for g in groups for p in g["params"]]
    assert len(params) > 100 and any(p.dim() > 1 for p in params)
    set_grads(params, 9, 1.0, skip=(3, 40, 41, len(params) - 1))
    worst, _ = checked_step(optimizer, 0.1)
    assert max(worst.values()) <= 1.0, worst
    theirs = torch.optim.AdamW(get_param_groups(cfg, model)[0], lr=cfg["LR"], weight_decay=cfg["WEIGHT_DECAY"])
    theirs.load_state_dict(copy.deepcopy(optimizer.state_dict()))
    assert float(theirs.state[params[0]]["step"]) == 1.0 and float(theirs.state[params[3]]["step"]) == 0.0
    assert torch.equal(theirs.state[params[0]]["exp_avg"], optimizer.state[params[0]]["exp_avg"])
    before = T.snapshot(theirs)
    theirs.step()                                           # torch goes on from our state, by its own rule
    worst = T.check_step(before, T.snapshot(theirs), T.hyper(theirs), None, float("nan"))
    assert max(worst["p"], worst["m"], worst["v"]) <= 1.0, worst


def test_clip_step_of_the_small_model_through_the_engine(opt):
    optim, L = opt
    from memotr_amd.engine import (build_optimizer, clip_forward_backward, clip_to_device, make_synthetic_clip,
                                   optimizer_step)
    from memotr_amd.models.criterion import build as build_criterion
    model, cfg = small_model_and_config()
    optimizer = build_optimizer(cfg, model, impl="hip")
    assert isinstance(optimizer, optim.ClipAdamW) and len(optimizer.param_groups) == 4
    dev = torch.device("cuda")
    batch = clip_to_device(make_synthetic_clip(clip_len=2, height=96, width=128, n_gts=3, seed=1), dev)
    before = [p.detach().clone() for p in model.parameters()]
    loss, _ = clip_forward_backward(model, build_criterion(cfg), batch, dev)
    norm = optimizer_step(model, optimizer, cfg["CLIP_MAX_NORM"])
    assert torch.isfinite(loss) and torch.isfinite(norm) and float(norm) > 0.0
    assert all(p.grad is None for p in model.parameters())
    assert sum(not torch.equal(a, p) for a, p in zip(before, model.parameters())) > 100
    assert all(torch.isfinite(p).all() for p in model.parameters())
