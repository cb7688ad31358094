"""`python bench.py --gpus N` must be runnable as is: with no launcher around it (WORLD_SIZE unset) it starts one rank
per GPU itself -- the reference's launch line is `python -m torch.distributed.run --nproc_per_node=8 main.py`
(README.md:104, main.py:100-101).  No GPU here: the device count is stubbed through MEMOTR_BENCH_DEVICE_COUNT and the
ranks stop at the "needs a GPU" check, which is far enough to prove the spawn path parses and forwards the arguments."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    # the ranks see no device on a machine with GPUs too: they all stop at the same check as on a host without one
    e.update(HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)


def test_gpus_2_without_devices_fails_on_the_device_count_not_on_a_launcher():
    r = _run(["--gpus", "2"], MEMOTR_BENCH_DEVICE_COUNT="1")
    assert r.returncode != 0
    assert "only 1 GPU(s) visible" in r.stderr and "device count" in r.stderr, r.stderr[-400:]
    assert "launch with" not in r.stderr


def test_dry_launch_prints_the_rank_launcher_command_with_the_script_arguments():
    r = _run(["--gpus", "4", "--steps", "3", "--warmup", "1"], MEMOTR_BENCH_DEVICE_COUNT="8", MEMOTR_BENCH_DRY_LAUNCH="1")
    assert r.returncode == 0, r.stderr[-400:]
    argv = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    assert argv[1:3] == ["-m", "torch.distributed.run"]
    assert argv[argv.index("--nproc-per-node") + 1] == "4"
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1"
    tail = argv[argv.index(BENCH) + 1:]
    assert tail == ["--gpus", "4", "--steps", "3", "--warmup", "1"]


def test_self_launch_starts_one_rank_per_gpu_and_each_reaches_the_gpu_check():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], MEMOTR_BENCH_DEVICE_COUNT="2")
    assert r.returncode != 0                       # no GPU in this container: the ranks stop at the device check
    assert r.stderr.count("bench.py needs a GPU") == 2, r.stderr[-800:]


def test_a_launcher_that_started_the_wrong_world_is_reported_as_such():
    r = _run(["--gpus", "2"], WORLD_SIZE="3", RANK="0", LOCAL_RANK="0", MEMOTR_BENCH_DEVICE_COUNT="4")
    assert r.returncode != 0
    assert "WORLD_SIZE=3" in r.stderr or "needs a GPU" in r.stderr


def test_eight_rank_launch_rehearsal_rendezvous_thread_pools_and_one_json_line():
    """Round-5 verdict, item 7: the 8-GPU launch minus the GPUs.  `python bench.py --gpus 8` with a stubbed device count
    starts eight ranks itself; they rendezvous on 127.0.0.1, size their torch thread pools by an eighth of the
    container's CPU quota (eight ranks share it on the driver's box: 16 CPUs -> 2 per rank, one of them for the pool),
    all-reduce once, and exactly one JSON line comes out -- rank 0's."""
    r = _run(["--gpus", "8", "--steps", "1", "--warmup", "0"], MEMOTR_BENCH_DEVICE_COUNT="8", MEMOTR_BENCH_REHEARSAL="1")
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-800:]
    out = json.loads(lines[0])
    assert out["rehearsal"] and out["n_gpus"] == 8 and out["local_world"] == 8
    assert out["rank_sum"] == 36.0                                    # 1 + 2 + ... + 8: every rank took part
    from memotr_amd.utils.host import cpu_quota
    want = max(1, int(cpu_quota() * 0.5 / 8))
    assert out["torch_threads"] == want and out["torch_threads_sum"] == 8.0 * want, out
    assert abs(out["cpu_quota_per_rank"] - cpu_quota() / 8) < 1e-9


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr, r.stderr[-400:]


_DUMP = """
import sys
root, dirs = sys.argv[1], sys.argv[2:]
sys.path.insert(0, root)
import torch
import bench
big = torch.arange(bench.DUMP_SAMPLE * 3 + 7, dtype=torch.float64)
for out in dirs:
    bench.dump_outputs(out, {"big": big, "small": torch.arange(5), "half": torch.ones(3, dtype=torch.bfloat16)})
"""


def test_dump_outputs_writes_floats_and_the_same_sample_every_time(tmp_path):
    import numpy as np
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    e = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _DUMP, ROOT] + dirs, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    a = {n: np.load(os.path.join(dirs[0], n + ".npy")) for n in ("big", "small", "half")}
    b = {n: np.load(os.path.join(dirs[1], n + ".npy")) for n in ("big", "small", "half")}
    assert a["big"].dtype == np.float64 and a["small"].dtype == np.float32 and a["half"].dtype == np.float32
    assert np.array_equal(a["small"], np.arange(5, dtype=np.float32)) and np.array_equal(a["half"], np.ones(3))
    assert 0 < a["big"].size < 3 * 2 ** 21 + 7          # a sample of the large array ...
    assert np.all(np.diff(a["big"]) > 0) and a["big"][-1] < 3 * 2 ** 21 + 7   # ... of distinct elements, in order
    for k in a:                                          # ... and the same one on every run
        assert np.array_equal(a[k], b[k])
