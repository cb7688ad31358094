"""Dataset preparation (memotr_amd/data/prepare.py) against a recording of the reference's own scripts
(tests/golden/prepare.json, made by tests/golden/gen_golden_prepare.py on the trees of tests/prepare_trees.py): the same
files with the same bytes, a second run that changes nothing, and a prepared tree that ``data/datasets.py`` reads."""
import json
import os
import subprocess
import sys

import pytest

import dataset_trees
import prepare_trees as T
from conftest import GOLDEN_DIR

from memotr_amd.data import prepare as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "prepare.json")) as f:
        return json.load(f)


@pytest.fixture()
def root(tmp_path):
    return T.write_inputs(str(tmp_path / "data"))


def run_all(root):
    return {"mot17": P.prepare_mot17(root), "crowdhuman": P.prepare_crowdhuman(root), "bdd100k": P.prepare_bdd100k(root)}


def test_the_recording_holds_the_cases_it_is_there_for(golden):
    mot = golden["mot17"]
    # the running track number does not go up where a sequence starts with the id the one before it ended with
    assert mot["MOT17/gts/train/MOT17-02-SDP/img1/000003.txt"].split()[1] == "3"
    assert mot["MOT17/gts/train/MOT17-04-SDP/img1/000001.txt"].split()[1] == "3"
    assert mot["MOT17/gts/train/MOT17-09-SDP/img1/000001.txt"].split()[1] == "5"
    assert sum(text.count("\n") for text in mot.values()) == sum(
        1 for rows in T.MOT_ROWS.values() for r in rows if r[6] != 0 and r[7] == 1)
    crowd = golden["crowdhuman"]
    assert sorted(crowd) == ["CrowdHuman/gts/train/273271,c9db000d5146c15.txt",
                             "CrowdHuman/gts/train/282555,b9a6000f1c27c5e.txt",
                             "CrowdHuman/gts/val/273278,1017c000ac1360b7.txt"]
    assert [line.split()[1] for line in crowd["CrowdHuman/gts/val/273278,1017c000ac1360b7.txt"].splitlines()] == ["0", "1"]
    bdd = golden["bdd100k"]
    vid = "b1c66a42-6f7d68ca"
    assert f"BDD100K/filter_labels/track/train/{vid}/{vid}-0000002.txt" not in bdd           # a frame without labels
    assert bdd[f"BDD100K/filter_labels/track/train/{vid}/{vid}-0000004.txt"] == ""           # all labels dropped
    assert [line.split()[1] for line in
            bdd[f"BDD100K/filter_labels/track/train/{vid}/{vid}-0000003.txt"].splitlines()] == ["101", "106"]


@pytest.mark.parametrize("dataset", ["mot17", "crowdhuman", "bdd100k"])
def test_a_converter_writes_the_files_of_the_reference_script(root, golden, dataset):
    written = run_all(root)[dataset]
    got = T.read_outputs(root)[dataset]
    assert sorted(got) == sorted(golden[dataset])
    for path, text in golden[dataset].items():
        assert got[path].encode() == text.encode(), path
    listed = {os.path.relpath(p, root).replace(os.sep, "/") for p in written}
    assert listed == {p for p in got if p.endswith(".txt")} and len(written) == len(listed)


def test_a_second_run_leaves_the_tree_unchanged(root, golden):
    run_all(root)
    first = T.read_outputs(root)
    run_all(root)
    assert T.read_outputs(root) == first == golden


def test_the_command_line_writes_the_same_tree(root, golden):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args in (["mot17"], ["crowdhuman", "--split", "train", "val"], ["bdd100k", "--split", "train"]):
        done = subprocess.run([sys.executable, "-m", "memotr_amd.data.prepare", *args, "--data-root", root], env=env,
                              cwd=ROOT, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        assert done.stdout.startswith(args[0] + ": ")
    assert T.read_outputs(root) == golden


def test_the_datasets_read_a_prepared_mot17_and_crowdhuman_tree(root, golden):
    from memotr_amd.data import datasets as D
    P.prepare_mot17(root)
    P.prepare_crowdhuman(root)
    ds = D.build_dataset(dict(dataset_trees.MOT_CONFIG, DATA_ROOT=root, SAMPLE_MOT17_JOIN=0, SAMPLE_LENGTHS=[2]))
    assert sorted(ds.mot17_gts) == sorted(T.MOT_ROWS) and sorted(ds.crowdhuman_gts) == ["273278,1017c000ac1360b7"]
    assert ds.mot17_gts["MOT17-04-SDP"][2] == [(3, 11, 21, 30, 40), (4, 51, 61, 20, 45), (5, 90, 10, 12, 33)]
    assert ds.crowdhuman_gts["273278,1017c000ac1360b7"] == [(0, 72, 202, 163, 503), (1, 310, 200, 162, 497)]
    assert len(ds) > 1
    info = ds.frame_info("MOT17", "MOT17-02-SDP", 1)
    assert info["ids"].tolist() == [1, 2, 3] and info["boxes"].shape == (3, 4)
