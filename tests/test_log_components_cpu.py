"""CPU: ``ClipCriterion.log_components`` (memotr_amd/models/criterion.py) hands out, as one tensor and without a read,
the values that ``get_mean_by_n_gts(with_log=True)`` returns as python floats -- in a single process (host counts,
uploaded) and on two gloo ranks whose clips hold different numbers of objects (the counts of the existing all-reduce).
Both divide the same float32 value by the same count, one in float32 and one in float64: the bound is one float32 ulp."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"frame{i}_{k}" for i in (0, 1, 2) for k in ("box_l1_loss", "box_giou_loss", "label_focal_loss")]


def _config():
    from model_helpers import small_config
    cfg = small_config()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], SAMPLE_LENGTHS=[2, 3])
    return cfg


def _one_clip(model, n_gts, seed):
    """(names, components as floats, the with_log=True dict, the loss dicts of with_log False / True)."""
    from memotr_amd.engine import clip_forward_backward, make_synthetic_clip
    from memotr_amd.models.criterion import build as build_criterion
    criterion = build_criterion(_config())
    batch = make_synthetic_clip(clip_len=3, height=96, width=128, n_gts=n_gts, seed=seed)
    _, quiet = clip_forward_backward(model, criterion, batch, torch.device("cpu"), backward=False)
    names, components = criterion.log_components()
    assert components.dtype == torch.float32 and components.shape == (len(names),) and not components.requires_grad
    loud, log = criterion.get_mean_by_n_gts(with_log=True)
    again_names, again = criterion.log_components()                 # after either call
    assert again_names == names and torch.equal(again, components)
    quiet, loud = ({k: float(v.detach()) for k, v in d.items()} for d in (quiet, loud))
    return names, components.tolist(), log, quiet, loud


def _assert_within_an_ulp(names, components, log, objects=True):
    assert names == NAMES == list(log)
    for name, got in zip(names, components):
        want, count = log[name]
        assert count == 1 and (want > 0 if objects or "focal" in name else want == 0)
        assert abs(got - want) <= float(np.spacing(np.float32(want))), (name, got, want)


def test_the_components_are_the_with_log_values(monkeypatch):
    from model_helpers import build_small_memotr, patch_operator
    patch_operator(monkeypatch)
    torch.set_num_threads(2)
    torch.manual_seed(0)
    model = build_small_memotr().train()
    for n_gts, seed in ((3, 7), (0, 8)):                            # a clip without objects divides by 1
        names, components, log, quiet, loud = _one_clip(model, n_gts, seed)
        _assert_within_an_ulp(names, components, log, objects=n_gts > 0)
        assert quiet == loud                                        # with_log changes the log alone


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    import memotr_amd.modules.ms_deform_attn as mod
    from model_helpers import OracleMSDeformAttnFunction, build_small_memotr
    mod.MSDeformAttnFunction = OracleMSDeformAttnFunction           # CPU stand-in for the HIP operator (tests only)
    torch.manual_seed(3)
    model = build_small_memotr().train()
    names, components, log, _, _ = _one_clip(model, n_gts=2 + 4 * rank, seed=20 + rank)
    torch.save({"names": names, "components": components, "log": log}, f"{out_path}.{rank}")
    dist.destroy_process_group()


def test_two_ranks_divide_by_the_world_average_count(tmp_path):
    world, port = 2, _free_port()
    out = str(tmp_path / "rank")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for rank in range(world):
        r = torch.load(f"{out}.{rank}")
        _assert_within_an_ulp(r["names"], r["components"], r["log"])
