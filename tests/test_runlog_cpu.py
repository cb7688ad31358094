"""The run log (memotr_amd/runlog.py): ``MetricWindow`` against its definition -- the mean of the last 100 values and
the total over the count -- alone and over two gloo ranks (the union of the windows, the summed totals and counts, one
all-reduce), the printed line, and ``RunLog``'s files, which only rank 0 writes."""
import json
import math
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from memotr_amd.runlog import TIME, TOTAL, MetricWindow, RunLog, lr_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream(n, rank=0):
    """Values without a pattern that a wrong window would reproduce."""
    return [math.sin(1.0 + 0.37 * i + 5.0 * rank) * (3.0 + rank) + 0.01 * i for i in range(n)]


@pytest.mark.parametrize("n", [1, 100, 101, 250])
def test_the_window_mean_and_the_global_mean_follow_the_definition(n):
    m = MetricWindow()
    values = stream(n)
    for v in values:
        m.update("x", v)
    with pytest.raises(RuntimeError, match="sync"):
        m.avg("x")
    m.sync()
    last = values[-100:]
    assert math.isclose(m.avg("x"), math.fsum(last) / len(last), rel_tol=1e-12)
    assert math.isclose(m.global_avg("x"), math.fsum(values) / n, rel_tol=1e-12)
    assert m.get("x", "avg") == m.avg("x") and m.get("x", "global_avg") == m.global_avg("x")
    if n > 100:
        assert not math.isclose(m.avg("x"), m.global_avg("x"), rel_tol=1e-6)
    m.update("x", 1.0)                                  # a new value: the numbers must be fixed again before use
    with pytest.raises(RuntimeError):
        m.global_avg("x")


def test_a_smaller_window_and_the_printed_line():
    m = MetricWindow(window=2)
    for a, b, t in ((1.0, 10.0, 0.5), (2.0, 20.0, 0.7), (6.0, 60.0, 0.9)):
        m.update(TOTAL, a)
        m.update("frame0_box_l1_loss", b)
        m.update(TIME, t)
    m.sync()
    assert m.avg(TOTAL) == 4.0 and m.global_avg(TOTAL) == 3.0 and m.avg(TIME) == pytest.approx(0.8)
    # MetricLog.__str__ of the reference: the loss first, the time left out, four decimals
    assert str(m) == "loss = 4.0000 (3.0000); frame0_box_l1_loss = 40.0000 (30.0000); "
    with pytest.raises(ValueError):
        MetricWindow(window=0)
    assert lr_info([1, 2, 3, 4]) == [{"lr_backbone": 1}, {"lr_points": 2}, {"lr_query_updater": 3}, {"lr": 4}]


def test_runlog_writes_config_lines_and_scalars(tmp_path):
    from memotr_amd.configs import load_yaml
    log = RunLog(str(tmp_path / "train"))
    config = dict(MODE="train", LR=2.0e-5, SAMPLE_STEPS=[6, 10], RESUME=None, USE_DAB=True, OUTPUTS_DIR="./out/")
    log.write_config(config)
    assert load_yaml(str(tmp_path / "train" / "config.yaml")) == config
    m = MetricWindow()
    for name, v in ((TOTAL, 3.0), ("frame0_box_l1_loss", 1.0), ("frame0_box_giou_loss", 2.0),
                    ("frame0_label_focal_loss", 4.0), ("frame1_box_l1_loss", 5.0), (TIME, 0.25)):
        m.update(name, v)
    m.sync()
    log.write(head="[Epoch=0, Iter=0/7]", log=m)
    log.write(head="[Epoch 0] lr=[]")
    log.metric_scalars(m, step=12, mode="iters")
    log.scalar("lr", 2e-4, step=0, mode="epochs")
    with open(tmp_path / "train" / "log.txt") as f:
        lines = f.read().splitlines()
    assert lines == ["[Epoch=0, Iter=0/7] " + str(m), "[Epoch 0] lr=[] "]
    with open(tmp_path / "train" / "scalars.jsonl") as f:
        scalars = [json.loads(line) for line in f]
    assert scalars == [
        {"mode": "iters", "step": 12, "tag": "box_l1_loss/frame0", "value": 1.0},
        {"mode": "iters", "step": 12, "tag": "box_l1_loss/frame1", "value": 5.0},
        {"mode": "iters", "step": 12, "tag": "box_giou_loss/frame0", "value": 2.0},
        {"mode": "iters", "step": 12, "tag": "label_focal_loss/frame0", "value": 4.0},
        {"mode": "iters", "step": 12, "tag": "loss", "value": 3.0},
        {"mode": "epochs", "step": 0, "tag": "lr", "value": 2e-4}]


# ------------------------------------------------------------------------------------------------ two gloo ranks
COUNTS = (130, 70)              # rank 0 has a full window, rank 1 a partial one


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from memotr_amd.runlog import MetricWindow, RunLog
    m = MetricWindow()
    for v in stream(COUNTS[rank], rank):
        m.update("total_loss", v)
        m.update("frame0_box_l1_loss", 2.0 * v + rank)
    m.sync()
    log = RunLog(os.path.join(out_dir, f"train_by_rank{rank}"))           # a directory per rank: who wrote is visible
    log.write_config({"RANK": rank})
    log.write(head="[Epoch=0, Iter=0/1]", log=m)
    log.metric_scalars(m, step=0, mode="iters")
    torch.save({k: (m.avg(k), m.global_avg(k)) for k in m.metrics}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_report_the_union_of_their_windows_and_only_rank_0_writes(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0 == r1
    streams = [stream(COUNTS[rank], rank) for rank in range(world)]
    union = [v for s in streams for v in s[-100:]]
    assert len(union) == 170
    everything = [v for s in streams for v in s]
    avg, global_avg = r0["total_loss"]
    assert math.isclose(avg, math.fsum(union) / len(union), rel_tol=1e-12)
    assert math.isclose(global_avg, math.fsum(everything) / len(everything), rel_tol=1e-12)
    second = [[2.0 * v + rank for v in s] for rank, s in enumerate(streams)]
    avg, global_avg = r0["frame0_box_l1_loss"]
    assert math.isclose(avg, math.fsum(v for s in second for v in s[-100:]) / 170, rel_tol=1e-12)
    assert math.isclose(global_avg, math.fsum(v for s in second for v in s) / 200, rel_tol=1e-12)
    assert sorted(os.listdir(tmp_path / "train_by_rank0")) == ["config.yaml", "log.txt", "scalars.jsonl"]
    assert not os.path.exists(tmp_path / "train_by_rank1")
    with open(tmp_path / "train_by_rank0" / "config.yaml") as f:
        assert yaml.safe_load(f) == {"RANK": 0}
