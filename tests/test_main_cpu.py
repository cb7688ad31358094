"""CPU: the command-line entry (memotr_amd/main.py).  Options and their merge into a config by the reference's rules,
the six built-in configs against the reference's files (tests/golden/configs), the keys that fail loudly, pretrained
weights, and the chain that the entry exists for: one epoch on the small DanceTrack tree writes
``train/config.yaml``, the log files and a checkpoint, and ``submit`` and ``evaluate`` then run on that directory with
no file written by hand."""
import dataclasses
import json
import os
import subprocess
import sys

import pytest
import torch

import clip_loader_helpers as H
import dataset_trees as T
from conftest import GOLDEN_DIR
from model_helpers import build_small_memotr, patch_operator, small_config

from memotr_amd import main as M
from memotr_amd.configs import BUILTIN_CONFIGS, builtin_config, load_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = dict(raw_size=(96, 160), area_thresh=0)
PLAN = dataclasses.replace(H.PLAIN, final=(96, 128))        # the small model's frame size in the other tests


def merged(argv, config=None):
    options = M.parse_options(argv)
    return M.merge_config(builtin_config("dancetrack") if config is None else config, options)


# ------------------------------------------------------------------------------------------------ options and merge
def test_an_option_replaces_the_key_of_its_name_and_none_leaves_it():
    config = merged(["--mode", "submit", "--epochs", "3", "--lr", "1e-3", "--miss-tolerance", "15",
                     "--outputs-dir", "out/x", "--data-root", "/data"])
    want = builtin_config("dancetrack")
    want.update(MODE="submit", EPOCHS=3, LR=1e-3, MISS_TOLERANCE=15.0, OUTPUTS_DIR="out/x", DATA_ROOT="/data",
                CONFIG_PATH="dancetrack")
    assert config == want and isinstance(config["MISS_TOLERANCE"], float)
    # the two flags are never None: absent they put False, as the reference's store_true options do
    assert merged([], dict(builtin_config("dancetrack"), USE_DISTRIBUTED=True))["USE_DISTRIBUTED"] is False
    assert merged(["--use-distributed", "--use-checkpoint"])["USE_CHECKPOINT"] is True


def test_the_strings_true_and_false_become_bools():
    config = merged(["--resume-scheduler", "False", "--coco-size", "True", "--use-crowdhuman", "True",
                     "--overflow-bbox", "False", "--dataset", "True story"])
    assert config["RESUME_SCHEDULER"] is False and config["COCO_SIZE"] is True and config["USE_CROWDHUMAN"] is True
    assert config["OVERFLOW_BBOX"] is False and config["DATASET"] == "True story"


def test_list_options_replace_the_whole_list():
    config = merged(["--sample-steps", "3", "5", "--sample-lengths", "2", "--lr-drop-milestones", "7", "9"])
    assert config["SAMPLE_STEPS"] == [3, 5] and config["SAMPLE_LENGTHS"] == [2] and config["LR_DROP_MILESTONES"] == [7, 9]


def test_an_option_without_a_key_and_a_key_that_appears_twice_are_errors():
    config = builtin_config("bdd100k")                          # this file has no COCO_SIZE
    with pytest.raises(RuntimeError) as e:
        merged(["--coco-size", "True"], config)
    assert str(e.value) == "The option '--coco_size' is not appeared in .yaml config file."
    with pytest.raises(RuntimeError, match="not unique"):
        merged([], dict(builtin_config("dancetrack"), NESTED={"EPOCHS": 1}))
    nested = merged(["--epochs", "9"], {"A": {"EPOCHS": 1}, "USE_DISTRIBUTED": False, "USE_CHECKPOINT": False})
    assert nested["A"] == {"EPOCHS": 9}


def test_config_path_is_recorded_for_names_and_files(tmp_path):
    assert merged([])["CONFIG_PATH"] == "dancetrack"            # the default
    path = os.path.join(GOLDEN_DIR, "configs", "train_mot17.yaml")
    options = M.parse_options(["--config-path", path, "--epochs", "2"])
    config = M.merge_config(M.load_config(options.config_path), options)
    assert config == dict(builtin_config("mot17"), EPOCHS=2, CONFIG_PATH=path)
    with pytest.raises(FileNotFoundError):
        M.load_config(str(tmp_path / "dancetrack.yaml"))


def test_the_options_are_the_reference_s():
    options = vars(M.parse_options([]))
    assert len(options) == 44 and options.pop("config_path") == "dancetrack"
    assert options.pop("use_distributed") is False and options.pop("use_checkpoint") is False
    assert all(v is None for v in options.values())
    assert set(k.upper() for k in options) - set(builtin_config("mot17")) == set()        # every option has its key


@pytest.mark.parametrize("name", ["dancetrack", "sportsmot", "mot17", "bdd100k", "dancetrack_deformable_detr",
                                  "sportsmot_deformable_detr"])
def test_a_built_in_config_equals_the_reference_s_file(name):
    assert name in BUILTIN_CONFIGS
    want = load_yaml(os.path.join(GOLDEN_DIR, "configs", f"train_{name}.yaml"))
    got = builtin_config(name)
    assert got == want and len(got) == len(want) >= 80
    got["SAMPLE_STEPS"].append(1)                               # a fresh dict on every call
    assert builtin_config(name) == want
    with pytest.raises(ValueError, match="built-in"):
        builtin_config(name + "x")


# ------------------------------------------------------------------------------------------------ loud failures
def base_config(**over):
    cfg = small_config()
    cfg.update(MATCH_COST_CLASS=2, MATCH_COST_BBOX=5, MATCH_COST_GIOU=2, LOSS_WEIGHT_FOCAL=2, LOSS_WEIGHT_L1=5,
               LOSS_WEIGHT_GIOU=2, AUX_LOSS_WEIGHT=[1.0], LR=2e-4, LR_BACKBONE=2e-5, LR_POINTS=1e-5, WEIGHT_DECAY=5e-4,
               CLIP_MAX_NORM=0.1, LR_SCHEDULER="MultiStep", LR_DROP_MILESTONES=[1], LR_DROP_RATE=0.1, EPOCHS=1,
               ONLY_TRAIN_QUERY_UPDATER_AFTER=2, ACCUMULATION_STEPS=1, RESUME=None, RESUME_SCHEDULER=False,
               MODE="train", BATCH_SIZE=1, USE_DISTRIBUTED=False, PRETRAINED_MODEL=None, MULTI_CHECKPOINT=False,
               GIT_VERSION=None, EVAL_PORT=None, EVAL_THREADS=1, USE_MOTSYNTH=None,
               DET_SCORE_THRESH=0.0, TRACK_SCORE_THRESH=0.0, RESULT_SCORE_THRESH=0.0, MISS_TOLERANCE=5,
               USE_MOTION=False)
    cfg.update(T.DANCE_CONFIG)
    cfg.update(over)
    return cfg


def test_keys_that_nothing_implements_fail_with_a_sentence(monkeypatch):
    touched = []
    monkeypatch.setattr(M, "set_up_process", lambda config: touched.append(config))
    with pytest.raises(NotImplementedError, match="BATCH_SIZE is 2: the clip loader makes one clip per batch"):
        M.run(base_config(BATCH_SIZE=2))
    with pytest.raises(NotImplementedError, match="VISUALIZE is set"):
        M.run(base_config(VISUALIZE=True, MODE="submit"))
    with pytest.raises(NotImplementedError, match="USE_MOTSYNTH is set"):
        M.run(base_config(USE_MOTSYNTH=True))
    with pytest.raises(ValueError) as e:
        M.run(base_config(MODE="test"))
    assert str(e.value) == "Unsupported mode 'test'"
    assert touched == []                                        # all of them before anything is set up


def test_the_process_is_set_up_before_a_device_is_touched(monkeypatch):
    for key in ("CUDA_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "LOCAL_RANK"):
        monkeypatch.setenv(key, "")                             # recorded, so that what set_up_process writes is undone
        monkeypatch.delenv(key)
    monkeypatch.setenv("PYTHONHASHSEED", "0")
    state = torch.get_rng_state()
    try:
        assert M.set_up_process(base_config(AVAILABLE_GPUS="2,3", SEED=5)) == torch.device("cpu")
        assert os.environ["CUDA_VISIBLE_DEVICES"] == os.environ["HIP_VISIBLE_DEVICES"] == "2,3"
        assert torch.initial_seed() == 5 and os.environ["PYTHONHASHSEED"] == "5"
        monkeypatch.setenv("LOCAL_RANK", "1")                   # a launcher's choice stands
        monkeypatch.setenv("HIP_VISIBLE_DEVICES", "4")
        M.set_up_process(base_config(AVAILABLE_GPUS="2,3", SEED=5))
        assert os.environ["HIP_VISIBLE_DEVICES"] == "4"
        M.set_up_process(base_config(AVAILABLE_GPUS="", SEED=5))
        with pytest.raises(ValueError, match="DEVICE"):
            M.set_up_process(base_config(DEVICE="tpu", SEED=5))
    finally:
        torch.set_rng_state(state)


def test_help_exits_0_in_a_child_process():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-m", "memotr_amd", "--help"], env=env, cwd=ROOT, capture_output=True,
                          text=True)
    assert done.returncode == 0, done.stderr
    assert "--config-path" in done.stdout and "sportsmot_deformable_detr" in done.stdout


# ------------------------------------------------------------------------------------------------ train / submit / eval
@pytest.fixture(scope="module")
def root(tmp_path_factory, request):
    from memotr_amd.build import build_jpeg_enc_lib, build_jpeg_lib
    request.getfixturevalue("hip_lib"), request.getfixturevalue("clip_lib")
    build_jpeg_lib(), build_jpeg_enc_lib()
    root = T.write_trees(str(tmp_path_factory.mktemp("data")), only=("DanceTrack",))
    with open(os.path.join(root, "DanceTrack", "train_seqmap.txt"), "w") as f:      # part of the dataset, as downloaded
        f.write("name\n" + "".join(seq + "\n" for seq in sorted(T.DANCE_SEQS)))
    return root


@pytest.fixture()
def quiet_env(monkeypatch):
    monkeypatch.setenv("PYTHONHASHSEED", "0")                   # set_seed writes it: restored after the test
    patch_operator(monkeypatch)
    torch.set_num_threads(2)
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


def small_model(seed):
    torch.manual_seed(seed)
    return build_small_memotr()


def coco_named(state):
    """The model's own parameters under the key names of a DAB-Deformable-DETR COCO checkpoint, i.e. what
    ``remap_pretrained_state_dict`` maps back."""
    out = {}
    for k, v in state.items():
        if k.startswith("backbone.backbone.backbone"):
            k = "backbone.0.body" + k[len("backbone.backbone.backbone"):]
        elif k.startswith("feature_projs"):
            k = "input_proj" + k[len("feature_projs"):]
        elif k == "det_query_embed":
            k = "tgt_embed.weight"
        elif k == "det_anchor":
            k = "refpoint_embed.weight"
        out[k] = v.clone()
    return out


def test_pretrained_weights_are_loaded_and_none_leaves_the_model(root, tmp_path, quiet_env):
    source, target = small_model(1), small_model(2)
    renamed = coco_named(source.state_dict())
    assert sum(k not in target.state_dict() for k in renamed) > 10          # the remap has work to do
    path = str(tmp_path / "coco.pth")
    torch.save({"model": renamed}, path)
    config = base_config(EPOCHS=0, DATA_ROOT=root, OUTPUTS_DIR=str(tmp_path / "out"), PRETRAINED_MODEL=path)
    model, _, _, states = M.run(config, model=target, dataset=H.dance_dataset(root, plans=[PLAN]))
    assert model is target and states == {"start_epoch": 0, "global_iters": 0}
    for (name, a), b in zip(source.state_dict().items(), target.state_dict().values()):
        assert torch.equal(a, b), name
    assert load_yaml(str(tmp_path / "out" / "train" / "config.yaml")) == config
    # PRETRAINED_MODEL: None -- the parameters stay as they were
    untouched = small_model(3)
    before = {k: v.clone() for k, v in untouched.state_dict().items()}
    M.run(dict(config, PRETRAINED_MODEL=None), model=untouched, dataset=H.dance_dataset(root, plans=[PLAN]))
    assert all(torch.equal(v, untouched.state_dict()[k]) for k, v in before.items())
    assert any(not torch.equal(v, source.state_dict()[k]) for k, v in before.items())
    with pytest.raises(FileNotFoundError, match="PRETRAINED_MODEL"):
        M.run(dict(config, PRETRAINED_MODEL=str(tmp_path / "missing.pth")), model=small_model(3),
              dataset=H.dance_dataset(root, plans=[PLAN]))


def test_one_epoch_then_submit_then_evaluate_with_no_file_written_by_hand(root, tmp_path, quiet_env, capsys):
    out = str(tmp_path / "run")
    config = base_config(DATA_ROOT=root, OUTPUTS_DIR=out, SEED=11)
    model = small_model(0)
    before = [p.detach().clone() for p in model.parameters()]
    events = []
    trained, _, _, states = M.run(config, model=model, dataset=H.dance_dataset(root, plans=[PLAN]), log_every=4,
                                  prefetch=1, decode_threads=1, on_log=events.append)
    assert trained is model and states == {"start_epoch": 1, "global_iters": 10}
    assert sum(not torch.equal(a, p) for a, p in zip(before, model.parameters())) > 50
    # the files of the run
    assert load_yaml(os.path.join(out, "train", "config.yaml")) == config
    assert os.path.isfile(os.path.join(out, "checkpoint_0.pth"))
    with open(os.path.join(out, "train", "log.txt")) as f:
        lines = f.read().splitlines()
    assert lines[0] == ("[Epoch 0] lr=[{'lr_backbone': 2e-05}, {'lr_points': 1e-05}, {'lr_query_updater': 0.0002}, "
                        "{'lr': 0.0002}] ")
    assert [line.split("]")[0] for line in lines[1:-1]] == [f"[Epoch=0, Iter={i}/10" for i in (0, 4, 8)]
    assert lines[-1].startswith("[Epoch: 0, Total Time: 0min] loss = ")
    names = ["loss"] + [f"frame{i}_{k}" for i in (0, 1) for k in ("box_l1_loss", "box_giou_loss", "label_focal_loss")]
    for line in lines[1:]:
        fields = line.split("] ", 1)[1].split("; ")
        assert [f.split(" = ")[0] for f in fields[:-1]] == names and fields[-1] == ""
        assert "time per iter" not in line
    # iteration 0's line holds one clip: window mean == global mean == that clip's loss, which on_log saw too
    first = dict(f.split(" = ") for f in lines[1].split("] ", 1)[1].split("; ")[:-1])
    assert first["loss"] == f"{events[0]['loss']:.4f} ({events[0]['loss']:.4f})"
    assert [e["iter"] for e in events if "iter" in e] == [0, 4, 8]
    with open(os.path.join(out, "train", "scalars.jsonl")) as f:
        scalars = [json.loads(line) for line in f]
    assert scalars[0] == {"mode": "epochs", "step": 0, "tag": "lr", "value": 2e-4}
    assert [s["step"] for s in scalars if s["tag"] == "loss"] == [0, 4, 8, 0]
    assert sum(s["mode"] == "epochs" for s in scalars) == 1 + 7
    assert {s["tag"] for s in scalars} == {"lr", "loss"} | {f"{k}/frame{i}" for i in (0, 1) for k in
                                                           ("box_l1_loss", "box_giou_loss", "label_focal_loss")}
    # the epoch's global mean of the loss is the mean that fit reports
    epoch_loss = [s["value"] for s in scalars if s["tag"] == "loss" and s["mode"] == "epochs"][0]
    assert epoch_loss == pytest.approx(events[-1]["loss"], rel=1e-12)
    console = capsys.readouterr().out
    assert "Configs:" in console and "s/iter, 4/10 iters, rest time: 0 min, Max Memory=0MB]" in console

    # submit, then evaluate, on that directory: both read train/config.yaml
    files = M.run(dict(config, MODE="submit", SUBMIT_DIR=out, SUBMIT_MODEL="checkpoint_0.pth",
                       SUBMIT_DATA_SPLIT="train"), model=model.eval(), tracker_options=OPTIONS)
    assert [os.path.relpath(f, out) for f in files] == [os.path.join("train", "tracker", seq + ".txt")
                                                       for seq in sorted(T.DANCE_SEQS)]
    submitted = {}
    for seq, path in zip(sorted(T.DANCE_SEQS), files):
        with open(path) as f:
            submitted[seq] = f.read()
        assert submitted[seq].count("\n") >= T.DANCE_SEQS[seq]
    metrics = M.run(dict(config, MODE="eval", EVAL_DIR=out, EVAL_MODE="specific", EVAL_MODEL="checkpoint_0.pth",
                         EVAL_DATA_SPLIT="train"), model=small_model(9).eval(), tracker_options=OPTIONS)
    assert all(k in metrics for k in ("HOTA", "MOTA", "IDF1")) and metrics["Dets"] > 0
    for seq in T.DANCE_SEQS:                                    # the checkpoint holds the trained model's weights
        with open(os.path.join(out, "train", "checkpoint_0_tracker", seq + ".txt")) as f:
            assert f.read() == submitted[seq]
    with open(os.path.join(out, "train", "metrics.jsonl")) as f:
        (line,) = [json.loads(x) for x in f]
    assert line["checkpoint"] == "checkpoint_0.pth" and line["metrics"] == metrics
