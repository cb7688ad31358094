"""What the optimizer step costs on the full DanceTrack model's parameter list, three ways on the same build:

  torch    clip_grad_norm_(0.1) + torch.optim.AdamW(fused=True).step() + zero_grad()      (engine.optimizer_step today)
  hip      ClipAdamW.step(0.1) + zero_grad()                                              (MEMOTR_OPTIMIZER=hip)
  floor    one device copy that moves 32 B per parameter (16 read + 16 written): the update pass moves 28 B and the
           norm pass 4 B, so this is the traffic floor of the whole step

Every parameter's gradient is a view into one flat buffer that is refilled from a master copy before each timed step
(clip_grad_norm_ rescales .grad in place; zero_grad() drops it), outside the timed window.  Timed with device events
around each step, the three alternating round by round; the launch count of one step comes from torch.profiler.
Prints one JSON line.  Needs the GPU: there is no CPU fallback for a timing.

    python tools/bench_optim.py [--rounds 5] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU: no device, no number")
    from memotr_amd.configs import dancetrack_config
    from memotr_amd.engine import build_optimizer, get_param_groups, optimizer_step
    from memotr_amd.models import build_model
    from memotr_amd.optim import ClipAdamW

    dev = torch.device("cuda", 0)
    cfg = dancetrack_config(DEVICE="cuda", AVAILABLE_GPUS="0")
    sides = {}
    for name in ("torch", "hip"):                       # the same initial weights on both sides
        torch.manual_seed(0)
        model = build_model(cfg).train()
        opt = build_optimizer(cfg, model, impl=name)
        assert isinstance(opt, ClipAdamW) == (name == "hip")
        params = [p for g in get_param_groups(cfg, model)[0] for p in g["params"]]
        sides[name] = (model, opt, params)
    params = sides["torch"][2]
    n_tensors, n_params = len(params), sum(p.numel() for p in params)
    starts, at = [], 0
    for p in params:                                    # 16-byte aligned views, as autograd's own allocations are
        starts.append(at)
        at += -(-p.numel() // 4) * 4
    gen = torch.Generator(device=dev).manual_seed(1)
    master = torch.randn(at, device=dev, generator=gen) * 1e-2
    flat = {name: torch.empty_like(master) for name in sides}
    floor_src = torch.empty(4 * n_params, device=dev)
    floor_dst = torch.empty_like(floor_src)

    def refill(name):
        flat[name].copy_(master)
        for p, s in zip(sides[name][2], starts):
            p.grad = flat[name][s:s + p.numel()].view(p.shape)

    def one(name):
        if name == "floor":
            floor_dst.copy_(floor_src)
            return
        model, opt, _ = sides[name]
        optimizer_step(model, opt, cfg["CLIP_MAX_NORM"])

    def timed(name, steps):
        out = []
        for _ in range(steps):
            if name != "floor":
                refill(name)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            one(name)
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    order = ("torch", "hip", "floor")
    for name in order:
        timed(name, 3)                                  # warm-up: code objects, allocator, the optimizer's state
    samples = {name: [] for name in order}
    for _ in range(args.rounds):
        for name in order:
            samples[name] += timed(name, args.steps)

    launches = {}
    for name in order:
        try:
            from torch.profiler import ProfilerActivity, profile
            if name != "floor":
                refill(name)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                one(name)
                torch.cuda.synchronize()
            launches[name] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as e:                          # noqa: BLE001  (the profiler is optional: say so, do not guess)
            launches[name] = f"not measured ({type(e).__name__})"

    # the two sides took the same steps from the same weights: how far apart they ended
    drift = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(sides["torch"][2], sides["hip"][2]))
    res = {"n_tensors": n_tensors, "n_params": n_params, "steps_per_side": args.rounds * args.steps,
           "max_abs_param_difference_torch_vs_hip": drift}
    for name in order:
        xs = samples[name]
        res[name] = {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
                     "p90_ms": round(sorted(xs)[int(0.9 * (len(xs) - 1))], 4), "device_ops": launches[name]}
    res["floor"]["bytes"] = 32 * n_params
    res["floor"]["TB_per_s"] = round(32 * n_params / (res["floor"]["median_ms"] * 1e-3) / 1e12, 3)
    res["hip"]["TB_per_s_of_32B_per_param"] = round(32 * n_params / (res["hip"]["median_ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
