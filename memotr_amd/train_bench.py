"""bench.py --workload train: one clip train step of train_dancetrack.yaml per "step".

Step = the body of the reference's train loop (train_engine.py:183-246) on a synthetic clip resident in
HBM: T sequential frames through ResNet-50 -> deformable encoder/decoder (HIP MSDeformAttn) -> criterion
-> query updater, one backward, RCCL gradient all-reduce (DDP), clip-grad, AdamW.  Random-init weights,
random 800x1333 frames, persistent ground-truth identities.  value = frames/s over all ranks.
"""
from __future__ import annotations

import os
import sys
import time

import torch


def load_gemm_tuning() -> int:
    """Opt-in (MEMOTR_GEMM_TUNING=<csv>): load rocBLAS / hipBLASLt solution picks for the pyramid-sized fp32
    GEMMs (a TunableOp CSV written by tools/tune_gemm.py), read-only -- nothing is tuned at run time and GEMMs
    missing from the file keep the library default.  Measured on MI355X: the tuner's tight-loop winners (28-46 us
    for the 22323x256 projections vs 80 us default) do not carry over in situ (step time 262 vs 257 ms on the
    same box), so no file ships and the default is off.  Returns the number of entries in effect."""
    path = os.environ.get("MEMOTR_GEMM_TUNING", "0")
    if path == "0" or not os.path.exists(path):
        return 0
    import torch.cuda.tunable as tn
    try:
        tn.enable(True)
        tn.tuning_enable(False)
        tn.set_filename(os.devnull, False)      # never write next to the given file
        ok = tn.read_file(path)
        n = len(tn.get_results()) if ok else 0
        if not n:
            tn.enable(False)
        return n
    except Exception as exc:  # noqa: BLE001  (an optimisation only: the default library path stays valid)
        print(f"[memotr_amd] GEMM tuning file ignored: {exc}", file=sys.stderr)
        tn.enable(False)
        return 0


def run_train(args, rank: int, world: int, clip_len: int = None, height: int = 800, width: int = 1333,
              n_gts: int = 10, config: dict = None, dtype: str = "f32", collect=None):
    """``collect``: called on rank 0 after the timed steps with what the last one computed -- ``loss``, ``loss_dict``
    and ``model`` (its parameters as that step's optimizer update left them).  With ``collect`` the last timed step
    starts from the state the warm-up started from (parameters, optimizer, random generators), so that its inputs are
    the same in every run: the steps before it differ from run to run by the order of float atomics, and a training
    run amplifies that step after step.  The restore is not timed."""
    from .configs import dancetrack_config
    from .engine import build_optimizer, clip_forward_backward, clip_to_device, make_synthetic_clip, optimizer_step
    from .models import build_model
    from .models.criterion import build as build_criterion
    from .utils.utils import set_seed

    # a decoder-graph capture that fails is an error in the benchmark, not a silent eager run (models/graph_cache.py)
    os.environ.setdefault("MEMOTR_REQUIRE_GRAPHS", "1")
    clip_len = clip_len or int(os.environ.get("MEMOTR_BENCH_CLIP_LEN", "5"))
    cfg = config or dancetrack_config()
    torch.backends.cuda.matmul.allow_tf32 = False     # main.py:96-97 of the reference: strict fp32
    torch.backends.cudnn.allow_tf32 = False
    # MIOpen exhaustive find (cudnn.benchmark) was measured on MI355X: no gain for these shapes (13.2 vs 13.7
    # frames/s) and minutes of search per process, so immediate mode stays the default.
    torch.backends.cudnn.benchmark = os.environ.get("MEMOTR_MIOPEN_FIND", "0") == "1"
    dev = torch.device("cuda", torch.cuda.current_device())
    n_tuned = load_gemm_tuning()
    set_seed(cfg["SEED"])
    cfg = dict(cfg, DEVICE="cuda", AVAILABLE_GPUS="0")
    model = build_model(cfg).to(dev)
    model.train()
    criterion = build_criterion(cfg)
    optimizer = build_optimizer(cfg, model)
    if world > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        # the only buffers are frozen-BatchNorm constants (identical on every rank after DDP's initial state sync):
        # no per-forward buffer broadcast
        # gradient_as_bucket_view: the all-reduce runs in place on the parameters' own .grad storage (no bucket <-> grad
        # copies, 170 MB less traffic per step); covered by tests/test_distributed_gpu.py's two-rank test.  (static_graph
        # stays off: a clip makes T forwards per backward and the decoder graphs hand DDP one flat gradient.)
        model = DDP(model, device_ids=[dev.index], find_unused_parameters=False, broadcast_buffers=False,
                    gradient_as_bucket_view=True)
    batch = clip_to_device(make_synthetic_clip(clip_len, height, width, n_gts, seed=cfg["SEED"] + rank), dev)

    def step():
        if dtype == "bf16":     # extension: bf16 GEMMs/convs/value under autocast, fp32 master weights and optimizer
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss, loss_dict = clip_forward_backward(model, criterion, batch, dev, use_dab=cfg["USE_DAB"])
        else:
            loss, loss_dict = clip_forward_backward(model, criterion, batch, dev, use_dab=cfg["USE_DAB"])
        optimizer_step(model, optimizer, cfg["CLIP_MAX_NORM"])
        return loss, loss_dict

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    start = _train_state(model, optimizer, dev) if collect is not None else None
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    cpu0 = time.process_time()       # CPU time of this PROCESS, all its threads (launch thread, autograd's, torch's pool)
    paused, paused_cpu = 0.0, 0.0
    for i in range(args.steps):
        if start is not None and i == args.steps - 1:
            barrier()
            p0, pc0 = time.perf_counter(), time.process_time()
            _restore_train_state(model, optimizer, dev, start)
            barrier()
            paused, paused_cpu = time.perf_counter() - p0, time.process_time() - pc0
        loss, loss_dict = step()
    barrier()
    dt = time.perf_counter() - t0 - paused
    host_ms = (time.process_time() - cpu0 - paused_cpu) / args.steps * 1e3
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    per_rank = [dt / args.steps * 1e3]
    per_rank_host = [host_ms]
    backend = None
    if world > 1:
        # every rank's own step time (the reported number is the slowest rank's) and what the process group saw
        every = [torch.zeros_like(t) for _ in range(world)]
        torch.distributed.all_gather(every, t)
        per_rank = [float(x.item()) / args.steps * 1e3 for x in every]
        h = torch.tensor([host_ms], device=dev, dtype=torch.float64)
        every_h = [torch.zeros_like(h) for _ in range(world)]
        torch.distributed.all_gather(every_h, h)
        per_rank_host = [float(x.item()) for x in every_h]
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        backend = f"{torch.distributed.get_backend()} world_size={torch.distributed.get_world_size()}"
    dt = float(t.item())
    if rank != 0:
        return None
    n_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    from .utils.host import cpu_quota
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    result = {
        "metric": "train_frames_per_sec", "value": world * clip_len * args.steps / dt, "unit": "frames/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
        "config": {"workload": f"train_{cfg['DATASET'].lower()}.yaml clip step"
                               f"{' (--use-checkpoint)' if cfg['USE_CHECKPOINT'] else ''}: R50 + 6-enc/6-dec deformable transformer + query "
                               f"updater, clip length {clip_len}, {height}x{width} frames, bs=1/GPU, {n_gts} GT "
                               f"tracks, AdamW, grad-clip 0.1, random-init weights",
                   "parallelism": f"dp{world}", "trainable_params": n_params, "tuned_gemms": n_tuned,
                   "frames_per_gpu_per_sec": clip_len * args.steps / dt, "final_loss": float(loss.detach())},
        "max_memory_MB": torch.cuda.max_memory_allocated() // (1024 ** 2),
        "per_rank_ms_per_step": per_rank, "rank_skew_ms": max(per_rank) - min(per_rank), "process_group": backend,
        # multi-GPU readiness (round-5 verdict, item 7): a step issues ~9 k launches from one Python thread per rank, and the
        # ranks of a node share the container's CPU quota -- host time per step next to the wall time says how far a rank
        # is from being host-bound once eight of them share it
        "host_ms_per_step": max(per_rank_host), "per_rank_host_ms_per_step": per_rank_host,
        "cpu_quota_per_rank": cpu_quota() / max(1, local_world), "torch_threads": torch.get_num_threads(),
        "decoder_graphs": _graph_stats(model)["captures"], "decoder_graph_stats": _graph_stats(model),
    }
    if collect is not None:
        collect(loss=loss, loss_dict=loss_dict, model=getattr(model, "module", model))
    return result


def _train_state(model, optimizer, dev) -> dict:
    """What a clip train step reads besides its batch: parameters and buffers (copies), the optimizer's state and the
    random generators the model and the criterion draw from."""
    import random

    import numpy as np
    with torch.no_grad():
        tensors = [t.detach().clone() for t in list(model.parameters()) + list(model.buffers())]
    return {"tensors": tensors, "optimizer": {p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                                               for p, st in optimizer.state.items()},
            "random": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state(),
            "cuda": torch.cuda.get_rng_state(dev)}


def _restore_train_state(model, optimizer, dev, state: dict) -> None:
    """Back to ``state`` (_train_state), in place: the captured hipGraphs keep reading the same tensors."""
    import random

    import numpy as np
    with torch.no_grad():
        for t, v in zip(list(model.parameters()) + list(model.buffers()), state["tensors"]):
            t.copy_(v)
    optimizer.state.clear()
    for p, st in state["optimizer"].items():
        optimizer.state[p] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
    optimizer.zero_grad()
    random.setstate(state["random"])
    np.random.set_state(state["numpy"])
    torch.set_rng_state(state["torch"])
    torch.cuda.set_rng_state(state["cuda"], dev)


def _graph_stats(model) -> dict:
    g = getattr(model, "module", model).transformer.decoder.graphs()
    e = getattr(model, "module", model).encode_graphs()
    u = getattr(model, "module", model).query_updater.graphs()
    return {"captures": g.captures, "replays": g.replays, "eager": g.eager, "failed": bool(g.failed),
            "encode_captures": e.captures, "encode_replays": e.replays, "encode_eager": e.eager,
            "updater_captures": u.captures, "updater_replays": u.replays, "updater_eager": u.eager}
