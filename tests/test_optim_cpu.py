"""CPU: ``ClipAdamW`` (the torch-ops statement of the kernels) against the float64 truth and its derived bound
(tests/optim_truth.py), its state-dict exchange with torch.optim.AdamW, the schedulers, and the training driver
(memotr_amd/train.py): epoch policies, scheduler choice, checkpoint cadence and an exact resume."""
import os

import numpy as np
import pytest
import torch

import optim_truth as T
from memotr_amd.optim import ClipAdamW

SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023)
GROUP_LR = (1e-3, 0.0, 2e-4, 5e-3)
GROUP_WD = (1e-2, 5e-4, 0.0, 0.1)


def make_params(seed, sizes=SIZES, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=g) * 0.5).to(device)) for n in sizes]


def grouped(params):
    return [{"params": params[i::4], "lr": GROUP_LR[i], "weight_decay": GROUP_WD[i]} for i in range(4)]


def set_grads(params, seed, scale, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        grad = torch.randn(p.shape, generator=g) * scale
        p.grad = None if i in skip else grad.to(p.device)


@pytest.mark.parametrize("max_norm,scale", [(0.1, 1.0), (0.1, 1e-4), (None, 1.0)],
                         ids=["clip-active", "clip-inactive", "no-clip"])
def test_five_steps_stay_within_the_derived_bound(max_norm, scale):
    params = make_params(0)
    opt = ClipAdamW(grouped(params), betas=(0.9, 0.999), eps=1e-8)
    for step in range(5):
        set_grads(params, 10 + step, scale)
        before = T.snapshot(opt)
        grads = [p.grad.clone() for p in params]
        norm = opt.step(max_norm=max_norm)
        assert norm.dim() == 0 and norm.dtype == torch.float32
        truth = T.one_step(before, T.hyper(opt), max_norm)
        assert (truth["coef"] < 0.5) if (max_norm and scale == 1.0) else (truth["coef"] == 1.0)
        worst = T.check_step(before, T.snapshot(opt), T.hyper(opt), max_norm, float(norm))
        print(step, worst)
        assert max(worst.values()) <= 1.0, (step, worst)
        assert all(torch.equal(p.grad, g) for p, g in zip(params, grads)), ".grad was written"
    assert all(float(opt.state[p]["step"]) == 5.0 for p in params)
    lr0 = [p for p in grouped(params)[1]["params"]]
    fresh = make_params(0)
    assert all(torch.equal(p, q) for p, q in zip(lr0, fresh[1::4])), "lr = 0 with weight decay 5e-4 * 0 moved p"


def test_sparse_gradients_and_no_gradient_at_all():
    params = make_params(2, sizes=(7, 130, 5))
    opt = ClipAdamW(params, lr=1e-3)
    set_grads(params, 3, 1.0)
    opt.step(0.1)
    set_grads(params, 4, 1.0, skip=(1,))
    before = T.snapshot(opt)
    norm = opt.step(0.1)
    worst = T.check_step(before, T.snapshot(opt), T.hyper(opt), 0.1, float(norm))     # asserts row 1 bit-unchanged
    assert max(worst.values()) <= 1.0
    assert [float(opt.state[p]["step"]) for p in params] == [2.0, 1.0, 2.0]
    set_grads(params, 5, 1.0, skip=(0, 1, 2))
    before = T.snapshot(opt)
    norm = opt.step(0.1)
    assert float(norm) == 0.0
    T.check_step(before, T.snapshot(opt), T.hyper(opt), 0.1, 0.0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradients_follow_torch(bad):
    params = make_params(6, sizes=(9, 40))
    opt = ClipAdamW(params, lr=1e-3)
    set_grads(params, 7, 1.0)
    opt.step(0.1)
    set_grads(params, 8, 1.0)
    params[1].grad[3] = bad
    before = T.snapshot(opt)
    norm = opt.step(0.1)
    after = T.snapshot(opt)
    worst = T.check_step(before, after, T.hyper(opt), 0.1, float(norm))          # equal NaN masks, bound where finite
    assert max(worst.values()) <= 1.0, worst
    if bad == float("inf"):
        assert float(norm) == float("inf")
        assert np.isnan(after[1]["p"]).sum() == 1 and not np.isnan(after[0]["p"]).any()
    else:
        assert np.isnan(float(norm)) and all(np.isnan(a[k]).all() for a in after for k in ("p", "m", "v"))


def test_defaults_and_refused_flags():
    p = make_params(0, sizes=(4,))
    assert set(ClipAdamW(p).defaults) == set(torch.optim.AdamW(p).defaults)
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            ClipAdamW(p, **{flag: True})
        sd = torch.optim.AdamW(p).state_dict()
        sd["param_groups"][0][flag] = True
        with pytest.raises(ValueError, match=flag):
            ClipAdamW(p).load_state_dict(sd)
    for kwargs in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)),
                   dict(weight_decay=-1.0)):
        with pytest.raises(ValueError, match="Invalid"):
            ClipAdamW(p, **kwargs)


def test_unusable_gradients_are_errors_naming_the_parameter():
    params = [torch.nn.Parameter(torch.randn(*shape)) for shape in ((4,), (3, 4), (8,))]
    opt = ClipAdamW(params)
    set_grads(params, 1, 1.0)
    params[1].grad = torch.randn(4, 3).t()
    with pytest.raises(ValueError, match="parameter 1"):
        opt.step()
    set_grads(params, 1, 1.0)
    params[2].grad = torch.randn(16)[::2]
    with pytest.raises(ValueError, match="parameter 2"):
        opt.step()
    with pytest.raises(ValueError, match="parameter 0"):
        ClipAdamW([torch.nn.Parameter(torch.randn(4, 4).t())]).step()


def test_state_dict_goes_both_ways_with_torch_adamw():
    ours_p, torch_p = make_params(3), make_params(3)
    ours = ClipAdamW(grouped(ours_p))
    theirs = torch.optim.AdamW(grouped(torch_p))
    for step in range(2):
        set_grads(ours_p, 30 + step, 1.0, skip=(2,))
        set_grads(torch_p, 30 + step, 1.0, skip=(2,))
        ours.step()
        theirs.step()
    sd = ours.state_dict()
    assert list(sd["state"][0]) == ["step", "exp_avg", "exp_avg_sq"]
    assert sd["state"][0]["step"].dtype == torch.float32 and sd["state"][0]["step"].dim() == 0
    # ours -> torch: torch takes a further step from our state, within the bound
    fresh_p = [torch.nn.Parameter(p.detach().clone()) for p in ours_p]
    into_torch = torch.optim.AdamW(grouped(fresh_p))
    into_torch.load_state_dict(sd)
    set_grads(fresh_p, 40, 1.0)
    before = T.snapshot(into_torch)
    skipped = [id(p) for g in into_torch.param_groups for p in g["params"]].index(id(fresh_p[2]))   # row, group order
    assert [b["step"] for b in before] == [2.0 if i != skipped else 0.0 for i in range(len(fresh_p))]
    into_torch.step()
    worst = T.check_step(before, T.snapshot(into_torch), T.hyper(into_torch), None, float("nan"))
    assert max(worst["p"], worst["m"], worst["v"]) <= 1.0, worst
    # torch -> ours: steps arrive as CPU tensors (and, from older checkpoints, as numbers)
    for as_number in (False, True):
        sd_t = theirs.state_dict()
        if as_number:
            for st in sd_t["state"].values():
                st["step"] = int(st["step"])
        fresh_p = [torch.nn.Parameter(p.detach().clone()) for p in torch_p]
        into_ours = ClipAdamW(grouped(fresh_p))
        into_ours.load_state_dict(sd_t)
        st0 = into_ours.state[fresh_p[0]]
        assert st0["step"].dtype == torch.float32 and float(st0["step"]) == 2.0
        assert torch.equal(st0["exp_avg"], theirs.state[torch_p[0]]["exp_avg"])
        set_grads(fresh_p, 41, 1.0)
        before = T.snapshot(into_ours)
        assert torch_p[2] not in theirs.state and before[skipped]["step"] == 0.0
        norm = into_ours.step(0.1)
        worst = T.check_step(before, T.snapshot(into_ours), T.hyper(into_ours), 0.1, float(norm))
        assert max(worst.values()) <= 1.0, worst
        # the moments still live in the packed buffers
        plan = into_ours._plan
        assert st0["exp_avg"].untyped_storage().data_ptr() == plan.exp_avg.untyped_storage().data_ptr()
        assert into_ours.state[fresh_p[0]]["step"].untyped_storage().data_ptr() == \
            plan.steps.untyped_storage().data_ptr()


def test_add_param_group_keeps_the_state():
    params = make_params(4, sizes=(5, 70))
    opt = ClipAdamW(params[:1], lr=1e-3)
    set_grads(params, 1, 1.0)
    opt.step()
    m = opt.state[params[0]]["exp_avg"].clone()
    opt.add_param_group({"params": params[1:], "lr": 1e-2})
    before = T.snapshot(opt)
    assert before[0]["step"] == 1.0 and before[1]["step"] == 0.0 and np.array_equal(before[0]["m"], m.numpy())
    norm = opt.step(0.1)
    assert max(T.check_step(before, T.snapshot(opt), T.hyper(opt), 0.1, float(norm)).values()) <= 1.0


def test_state_assigned_from_outside_is_adopted_again():
    """memotr_amd/train_bench.py restores a snapshot by clearing ``optimizer.state`` and assigning clones."""
    params = make_params(4, sizes=(5, 70, 9))
    opt = ClipAdamW(params, lr=1e-3)
    set_grads(params, 1, 1.0)
    opt.step(0.1)
    saved = {p: {k: v.clone() for k, v in st.items()} for p, st in opt.state.items()}
    set_grads(params, 2, 1.0)
    opt.step(0.1)
    opt.state.clear()
    for p, st in list(saved.items())[:2]:               # the third parameter comes back without state
        opt.state[p] = {k: v.clone() for k, v in st.items()}
    set_grads(params, 3, 1.0)
    before = T.snapshot(opt)
    assert [b["step"] for b in before] == [1.0, 1.0, 0.0] and np.array_equal(before[1]["m"], saved[params[1]]["exp_avg"])
    norm = opt.step(0.1)
    assert max(T.check_step(before, T.snapshot(opt), T.hyper(opt), 0.1, float(norm)).values()) <= 1.0
    assert [float(opt.state[p]["step"]) for p in params] == [2.0, 2.0, 1.0]
    assert opt.state[params[0]]["exp_avg"].untyped_storage().data_ptr() == opt._plan.exp_avg.untyped_storage().data_ptr()


def test_torch_schedulers_drive_it():
    from torch.optim.lr_scheduler import CosineAnnealingLR, MultiStepLR
    import math
    params = make_params(5, sizes=(8, 9, 10, 11))
    opt = ClipAdamW(grouped(params))
    sched = MultiStepLR(opt, milestones=[2], gamma=0.1)
    seen = []
    for epoch in range(4):
        set_grads(params, epoch, 1.0)
        before = T.snapshot(opt)
        norm = opt.step(0.1)
        assert max(T.check_step(before, T.snapshot(opt), T.hyper(opt), 0.1, float(norm)).values()) <= 1.0
        seen.append([g["lr"] for g in opt.param_groups])
        sched.step()
    for epoch, lrs in enumerate(seen):
        assert lrs == pytest.approx([lr * (0.1 if epoch >= 2 else 1.0) for lr in GROUP_LR])
    opt = ClipAdamW(grouped(make_params(5, sizes=(8, 9, 10, 11))))
    sched = CosineAnnealingLR(opt, T_max=10)
    for epoch in range(3):
        assert opt.param_groups[0]["lr"] == pytest.approx(GROUP_LR[0] * (1 + math.cos(math.pi * epoch / 10)) / 2)
        opt.step()
        sched.step()


# ------------------------------------------------------------------------------------------------ the driver
def test_build_scheduler_follows_the_reference():
    from torch.optim.lr_scheduler import CosineAnnealingLR, MultiStepLR
    from memotr_amd.train import build_scheduler
    opt = ClipAdamW(make_params(0, sizes=(4,)), lr=2e-4)
    s = build_scheduler(dict(LR_SCHEDULER="MultiStep", LR_DROP_MILESTONES=[12], LR_DROP_RATE=0.1, EPOCHS=20), opt)
    assert isinstance(s, MultiStepLR) and dict(s.milestones) == {12: 1} and s.gamma == 0.1
    s = build_scheduler(dict(LR_SCHEDULER="Cosine", EPOCHS=20), opt)
    assert isinstance(s, CosineAnnealingLR) and s.T_max == 20
    with pytest.raises(ValueError, match="Do not support lr scheduler 'Step'"):
        build_scheduler(dict(LR_SCHEDULER="Step", EPOCHS=20), opt)


def test_apply_epoch_policy_follows_the_reference():
    from memotr_amd.train import apply_epoch_policy
    params = make_params(0, sizes=(4, 5, 6, 7))
    opt = ClipAdamW(grouped(params))
    cfg = dict(ONLY_TRAIN_QUERY_UPDATER_AFTER=3)
    assert apply_epoch_policy(cfg, opt, 2) is None                       # no NO_GRAD_FRAMES key: every frame trains
    assert [g["lr"] for g in opt.param_groups] == list(GROUP_LR)
    cfg.update(NO_GRAD_STEPS=[8, 4, 0], NO_GRAD_FRAMES=[3, 2, 0])        # the first matching step, in list order
    assert [apply_epoch_policy(cfg, opt, e) for e in (0, 2)] == [0, 0]
    assert [g["lr"] for g in opt.param_groups] == list(GROUP_LR)
    assert apply_epoch_policy(cfg, opt, 3) == 0
    assert [g["lr"] for g in opt.param_groups] == [0.0, 0.0, GROUP_LR[2], 0.0]      # groups 0, 1, 3 stop
    assert [apply_epoch_policy(cfg, opt, e) for e in (4, 7, 8, 30)] == [2, 2, 3, 3]
    cfg.update(NO_GRAD_STEPS=[5], NO_GRAD_FRAMES=[1])
    assert apply_epoch_policy(cfg, opt, 4) is None and apply_epoch_policy(cfg, opt, 5) == 1


def test_build_optimizer_opt_in_and_default(monkeypatch):
    from memotr_amd.engine import build_optimizer, optimizer_step
    monkeypatch.delenv("MEMOTR_OPTIMIZER", raising=False)
    model = torch.nn.Linear(3, 2)
    cfg = dict(LR=2e-4, LR_BACKBONE=2e-5, LR_POINTS=1e-5, WEIGHT_DECAY=5e-4)
    default = build_optimizer(cfg, model)
    assert type(default) is torch.optim.AdamW
    hip = build_optimizer(cfg, model, impl="hip")
    assert isinstance(hip, ClipAdamW) and len(hip.param_groups) == 4
    assert [g["lr"] for g in hip.param_groups] == [g["lr"] for g in default.param_groups]
    assert [len(g["params"]) for g in hip.param_groups] == [len(g["params"]) for g in default.param_groups]
    assert hip.defaults["weight_decay"] == 5e-4
    monkeypatch.setenv("MEMOTR_OPTIMIZER", "hip")
    assert isinstance(build_optimizer(cfg, model), ClipAdamW)
    assert type(build_optimizer(cfg, model, impl="torch")) is torch.optim.AdamW
    with pytest.raises(ValueError, match="triton"):
        build_optimizer(cfg, model, impl="triton")
    # optimizer_step: a ClipAdamW clips at the reference's 0.1 inside its step and hands the norm back
    model.weight.grad, model.bias.grad = torch.ones(2, 3), torch.ones(2)
    norm = optimizer_step(model, hip, 0.3)
    assert float(norm) == pytest.approx(8 ** 0.5) and model.weight.grad is None
    model.weight.grad, model.bias.grad = torch.ones(2, 3), torch.ones(2)
    assert optimizer_step(model, default, 0.3) is None and model.weight.grad is None


def _fit_config(**over):
    from model_helpers import small_config
    cfg = small_config()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3], LR=2e-4, LR_BACKBONE=2e-5,
               LR_POINTS=1e-5, WEIGHT_DECAY=5e-4, CLIP_MAX_NORM=0.1, LR_SCHEDULER="MultiStep", LR_DROP_MILESTONES=[1],
               LR_DROP_RATE=0.1, EPOCHS=2, ONLY_TRAIN_QUERY_UPDATER_AFTER=2, ACCUMULATION_STEPS=1, RESUME=None,
               RESUME_SCHEDULER=False)
    cfg.update(over)
    return cfg


def _run_fit(cfg, seed, outputs_dir, impl, log=None):
    from model_helpers import build_small_memotr
    from memotr_amd.engine import make_synthetic_clip
    from memotr_amd.models.criterion import build as build_criterion
    from memotr_amd.train import fit
    torch.manual_seed(seed)
    model = build_small_memotr()

    def make_batches(epoch):
        for i in range(2):
            yield make_synthetic_clip(clip_len=2, height=96, width=128, n_gts=3, seed=100 + 10 * epoch + i)

    opt, sched, states = fit(cfg, model, build_criterion(cfg), make_batches, device=torch.device("cpu"),
                             outputs_dir=outputs_dir, impl=impl, log_every=1, on_log=log)
    return model, opt, sched, states


@pytest.mark.parametrize("impl", ["hip", None], ids=["ClipAdamW", "torch"])
def test_fit_resumes_to_the_same_parameters(impl, tmp_path, monkeypatch):
    from model_helpers import patch_operator
    patch_operator(monkeypatch)
    monkeypatch.delenv("MEMOTR_OPTIMIZER", raising=False)
    torch.set_num_threads(2)
    out = str(tmp_path / "run")
    events = []
    model, opt, sched, states = _run_fit(_fit_config(), 0, out, impl, log=events.append)
    assert isinstance(opt, ClipAdamW) == (impl == "hip")
    assert states == {"start_epoch": 2, "global_iters": 4}
    assert sorted(os.listdir(out)) == ["checkpoint_0.pth", "checkpoint_1.pth"]
    assert [e["iter"] for e in events if "iter" in e] == [0, 1, 0, 1] and [e["epoch"] for e in events if "epoch" in e] == [0, 1]
    assert all(np.isfinite(e["loss"]) for e in events)
    # epoch 1 ran behind the milestone (the random-init updater gets zero gradients from these clips, so the groups
    # that do learn stay on: ONLY_TRAIN_QUERY_UPDATER_AFTER has its own test above)
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([2e-6, 1e-6, 2e-5, 2e-5])
    ckpt = torch.load(os.path.join(out, "checkpoint_0.pth"))
    assert sorted(ckpt) == ["model", "optimizer", "scheduler", "states"]
    assert ckpt["states"] == {"start_epoch": 1, "global_iters": 2}
    # resumed from epoch 0's checkpoint into a differently initialised model: same parameters, bit for bit
    cfg = _fit_config(RESUME=os.path.join(out, "checkpoint_0.pth"), RESUME_SCHEDULER=True)
    resumed, opt2, _, states2 = _run_fit(cfg, 1, None, impl)
    assert states2 == {"start_epoch": 2, "global_iters": 4}
    for (name, a), b in zip(model.named_parameters(), resumed.parameters()):
        assert torch.equal(a, b), name
    moved = sum(not torch.equal(a, b) for a, b in zip(ckpt["model"].values(), model.state_dict().values()))
    assert moved > 0, "epoch 1 trained nothing"
    # without RESUME_SCHEDULER the optimizer starts fresh and the scheduler is stepped start_epoch times
    cfg = _fit_config(RESUME=os.path.join(out, "checkpoint_0.pth"), RESUME_SCHEDULER=False, EPOCHS=1)
    _, opt3, sched3, states3 = _run_fit(cfg, 2, None, impl)
    assert states3["start_epoch"] == 1 and sched3.last_epoch == 1
    assert [g["lr"] for g in opt3.param_groups] == pytest.approx([2e-6, 1e-6, 2e-5, 2e-5])


def test_checkpoint_cadence_follows_the_reference(tmp_path, monkeypatch):
    """train_engine.py:146 with an empty epoch: DanceTrack or fewer than 100 epochs write every epoch, else every 5th."""
    from memotr_amd.train import fit
    model = torch.nn.Linear(3, 2)
    base = dict(LR=2e-4, LR_BACKBONE=2e-5, LR_POINTS=1e-5, WEIGHT_DECAY=5e-4, CLIP_MAX_NORM=0.1, LR_SCHEDULER="Cosine",
                ONLY_TRAIN_QUERY_UPDATER_AFTER=1000)
    for dataset, epochs, multi, want in (("MOT17", 101, False, list(range(4, 101, 5))), ("MOT17", 3, False, [0, 1, 2]),
                                         ("DanceTrack", 101, False, list(range(101))), ("MOT17", 3, True, [])):
        out = tmp_path / f"{dataset}_{epochs}_{multi}"
        cfg = dict(base, DATASET=dataset, EPOCHS=epochs, MULTI_CHECKPOINT=multi, OUTPUTS_DIR=str(out))
        fit(cfg, model, None, lambda epoch: iter(()), device=torch.device("cpu"), impl="hip")
        got = sorted(int(f[len("checkpoint_"):-4]) for f in os.listdir(out)) if out.exists() else []
        assert got == want, (dataset, epochs, multi)
