"""Golden vectors for the clip datasets (memotr_amd/data/datasets.py), produced by the REFERENCE's own ``DanceTrack``,
``MOT17`` and ``BDD100K`` classes on the trees of tests/dataset_trees.py (needs a checkout of the reference and Pillow;
the tests that read the fixture need neither):

    python tests/golden/gen_golden_datasets.py --reference /path/to/reference   ->  tests/golden/datasets.npz

The reference's ``data`` package is imported from that checkout as it is.  What it imports and this project does not
need is stood in for here, in ``sys.modules``, before the import: ``cv2``, ``torchvision`` (``.transforms``,
``.transforms.functional``, ``.ops.boxes.box_area``); the dataset classes are built with ``transform=None`` (MOT17:
a dict of identity callables) and no transform ever runs.  Three things are arranged so that the reference's answers
do not depend on the machine: ``os.listdir`` is patched to return sorted names (``vid_idx`` follows it), the trees are
written under a temporary directory whose own name holds none of ``MOT17``, ``CrowdHuman``, ``MOTSynth`` (the reference
looks for these substrings in the FULL path), and every BDD100K gt line ends with a newline (it cuts the last
character).

Recorded, arrays only (paths relative to DATA_ROOT, with ``/``):

  * per dataset and epoch (0 and both sides of every stage boundary): the sample length and the full begin list;
  * under ``random.seed(s)`` for s in dataset_trees.SEEDS: ``sample_frames_idx`` / ``sample_frame_paths`` of every
    entry, in order, the global generator running on from entry to entry;
  * ``get_single_frame``'s info of every frame of every used sequence (BDD100K: of every frame that has ground truth,
    and last of all of the frame whose gt file is empty -- the call enters it into the reference's dictionary).
"""
import argparse
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: conftest.save_npz, dataset_trees
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


def install_stand_ins():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def box_area(boxes):
        return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])

    module("cv2")
    fn = module("torchvision.transforms.functional")
    tr = module("torchvision.transforms", functional=fn, ToPILImage=object, RandomCrop=object)
    boxes = module("torchvision.ops.boxes", box_area=box_area)
    ops = module("torchvision.ops", boxes=boxes)
    module("torchvision", transforms=tr, ops=ops)


def load_reference(reference):
    if not os.path.exists(os.path.join(reference, "data", "dancetrack.py")):
        raise SystemExit(f"{reference}/data/dancetrack.py does not exist: --reference must name a checkout")
    install_stand_ins()
    sys.path.insert(0, reference)
    from data.bdd100k import BDD100K
    from data.dancetrack import DanceTrack
    from data.mot17 import MOT17
    return DanceTrack, MOT17, BDD100K


def put_info(arrays, prefix, info):
    for field in ("boxes", "ids", "labels", "areas"):
        arrays[f"{prefix}::{field}"] = info[field].numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its data/ package is imported)")
    args = ap.parse_args()
    import dataset_trees as trees
    from conftest import save_npz
    DanceTrack, MOT17, BDD100K = load_reference(os.path.abspath(args.reference))

    listdir = os.listdir
    os.listdir = lambda *a, **k: sorted(listdir(*a, **k))
    arrays = {}
    with tempfile.TemporaryDirectory(prefix="clip_trees_") as root:
        assert not any(s in root for s in ("MOT17", "CrowdHuman", "MOTSynth"))
        trees.write_trees(root)

        def rel(path):
            return os.path.relpath(path, root).replace(os.sep, "/")

        # ---------------------------------------------------------------- DanceTrack, BDD100K: (vid, t) entries
        for key, cls, config in (("dance", DanceTrack, trees.DANCE_CONFIG), ("bdd", BDD100K, trees.BDD_CONFIG)):
            ds = cls(config=dict(config, DATA_ROOT=root), split="train", transform=None)
            for epoch in trees.epochs_of(config):
                ds.set_epoch(epoch)
                arrays[f"{key}::epoch{epoch}::length"] = np.array(ds.sample_length, dtype=np.int64)
                arrays[f"{key}::epoch{epoch}::begin_vid"] = np.array([v for v, _ in ds.sample_begin_frames])
                arrays[f"{key}::epoch{epoch}::begin_t"] = np.array([t for _, t in ds.sample_begin_frames],
                                                                   dtype=np.int64)
                for seed in trees.SEEDS:
                    random.seed(seed)
                    arrays[f"{key}::epoch{epoch}::seed{seed}::frames"] = np.array(
                        [ds.sample_frames_idx(vid=v, begin_frame=t) for v, t in ds.sample_begin_frames],
                        dtype=np.int64).reshape(len(ds), ds.sample_length)
            for vid in list(ds.gts.keys()):
                for t in sorted(ds.gts[vid].keys()):
                    put_info(arrays, f"{key}::info::{vid}::{t}", ds.get_single_frame(vid, t)[1])
            if key == "dance":
                arrays["dance::vids"] = np.array([ds.idx_vid[k] for k in range(len(ds.idx_vid))])
            else:
                vid, t = trees.BDD_EMPTY
                assert t not in ds.gts[vid]
                put_info(arrays, f"bdd::info::{vid}::{t}", ds.get_single_frame(vid, t)[1])

        # ---------------------------------------------------------------- MOT17 + CrowdHuman: path entries
        identity = {"MOT17": lambda imgs, infos: (imgs, infos), "CrowdHuman": lambda imgs, infos: (imgs, infos)}
        ds = MOT17(config=dict(trees.MOT_CONFIG, DATA_ROOT=root), split="train", transform=identity)
        for epoch in trees.epochs_of(trees.MOT_CONFIG):
            ds.set_epoch(epoch)
            arrays[f"mot::epoch{epoch}::length"] = np.array(ds.sample_length, dtype=np.int64)
            arrays[f"mot::epoch{epoch}::begin"] = np.array([rel(p) for p in ds.sample_begin_frame_paths])
            for seed in trees.SEEDS:
                random.seed(seed)
                arrays[f"mot::epoch{epoch}::seed{seed}::paths"] = np.array(
                    [[rel(p) for p in ds.sample_frame_paths(begin_frame_path=b)] for b in ds.sample_begin_frame_paths]
                ).reshape(len(ds), ds.sample_length)
        frames = [os.path.join(ds.crowdhuman_seq_dir, f"{name}.jpg") for name in ds.crowdhuman_gts]
        for vid in list(ds.mot17_gts.keys()):
            ts = sorted(ds.mot17_gts[vid].keys())
            frames += [os.path.join(ds.mot17_seqs_dir, vid, "img1", str(t).zfill(6) + ".jpg")
                       for t in range(ts[0], ts[-1] + 1)]
        arrays["mot::frames"] = np.array([rel(p) for p in frames])
        for k, p in enumerate(frames):                  # keyed by the index into mot::frames
            put_info(arrays, f"mot::info::{k}", ds.get_single_frame(frame_path=p)[1])
    os.listdir = listdir

    path = os.path.join(OUT, "datasets.npz")
    save_npz(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays, torch", torch.__version__)


if __name__ == "__main__":
    main()
