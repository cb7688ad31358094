"""Dataset preparation: the ground-truth trees that ``data/datasets.py`` reads, made from the datasets as they are
downloaded (the reference's ``data/gen_mot17_gts.py``, ``gen_crowdhuman_gts.py`` and ``gen_bdd100k_gts.py``, as
functions with arguments in place of scripts with path literals).

    python -m memotr_amd.data.prepare mot17 --data-root /data
    python -m memotr_amd.data.prepare crowdhuman --data-root /data --split train val
    python -m memotr_amd.data.prepare bdd100k --data-root /data --split train

They write the same files with the same bytes as the reference's scripts do for the same inputs (held by
tests/test_prepare_cpu.py against a recording of those scripts).  Three differences are deliberate:

  * directory listings are sorted (the MOT17 track ids run on from sequence to sequence, so the reference's numbers
    depend on the order ``os.listdir`` happens to give);
  * every output file is written whole: the reference appends line by line, so running it twice doubles every MOT17 and
    CrowdHuman file; here a second run leaves the same tree;
  * no image is opened: the reference reads each CrowdHuman and BDD100K image (and each MOT17 ``seqinfo.ini``) for a
    size that it never uses.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional, Sequence

BDD_CATEGORY_IDS = {"train": 6, "car": 3, "bus": 5, "other person": 1, "rider": 2, "pedestrian": 1, "other vehicle": 3,
                    "motorcycle": 7, "bicycle": 8, "trailer": 4, "truck": 4}
BDD_KEPT = ("pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")     # the eight classes


def _write_whole(path: str, text: str) -> None:
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def prepare_mot17(data_root: str, split: str = "train") -> List[str]:
    """``<data_root>/MOT17/images/<split>/<seq>/gt/gt.txt`` -> ``<data_root>/MOT17/gts/<split>/<seq>/img1/%06d.txt``
    with lines ``0 {track} {x} {y} {w} {h} {visibility:f}`` (coordinates truncated to integers).  Rows with mark 0 or a
    class other than 1 are dropped.  ``track`` is a running number over ALL sequences in sorted order: it goes up
    whenever the id column differs from the previous kept row's, and is not reset between sequences -- so a sequence
    whose first id equals the previous sequence's last id continues that track number, as in the reference.  Returns
    the files written."""
    import numpy as np
    seq_root = os.path.join(data_root, "MOT17", "images", split)
    label_root = os.path.join(data_root, "MOT17", "gts", split)
    os.makedirs(label_root, exist_ok=True)
    written = []
    tid_curr, tid_last = 0, -1
    for seq in sorted(os.listdir(seq_root)):
        gt = np.loadtxt(os.path.join(seq_root, seq, "gt", "gt.txt"), dtype=np.float64, delimiter=",", ndmin=2)
        seq_label_root = os.path.join(label_root, seq, "img1")
        os.makedirs(seq_label_root, exist_ok=True)
        files: Dict[int, List[str]] = {}
        for fid, tid, x, y, w, h, mark, label, visibility in gt:
            if mark == 0 or not label == 1:
                continue
            fid, tid = int(fid), int(tid)
            if not tid == tid_last:
                tid_curr += 1
                tid_last = tid
            files.setdefault(fid, []).append("0 {:d} {:d} {:d} {:d} {:d} {:f}\n".format(
                tid_curr, int(x), int(y), int(w), int(h), float(visibility)))
        for fid, lines in files.items():
            path = os.path.join(seq_label_root, "{:06d}.txt".format(fid))
            _write_whole(path, "".join(lines))
            written.append(path)
    return written


def prepare_crowdhuman(data_root: str, splits: Sequence[str] = ("train", "val")) -> List[str]:
    """``<data_root>/CrowdHuman/annotation_<split>.odgt`` (one JSON record per line) ->
    ``<data_root>/CrowdHuman/gts/<split>/<ID>.txt``: the label file of ``images/<split>/<ID>.jpg``, with lines
    ``0 {id} {x} {y} {w} {h}`` of the full boxes (``fbox``, truncated to integers).  Boxes whose ``extra.ignore`` is 1
    are dropped; ``id`` counts the kept boxes of the whole file from 0; an image without a kept box gets no file.
    Returns the files written."""
    written = []
    for split in splits:
        label_root = os.path.join(data_root, "CrowdHuman", "gts", split)
        os.makedirs(label_root, exist_ok=True)
        with open(os.path.join(data_root, "CrowdHuman", f"annotation_{split}.odgt")) as f:
            records = [json.loads(line.strip("\n")) for line in f.readlines()]
        tid_curr = 0
        files: Dict[str, List[str]] = {}
        for record in records:
            for box in record["gtboxes"]:
                if "extra" in box and "ignore" in box["extra"] and box["extra"]["ignore"] == 1:
                    continue
                x, y, w, h = box["fbox"]
                files.setdefault("{}.txt".format(record["ID"]), []).append(
                    "0 {:d} {:d} {:d} {:d} {:d}\n".format(tid_curr, int(x), int(y), int(w), int(h)))
                tid_curr += 1
        for name, lines in files.items():
            path = os.path.join(label_root, name)
            _write_whole(path, "".join(lines))
            written.append(path)
    return written


def prepare_bdd100k(data_root: str, split: str = "train", list_path: Optional[str] = None) -> List[str]:
    """``<data_root>/BDD100K/labels/box_track_20/<split>/<vid>.json`` ->
    ``<data_root>/BDD100K/filter_labels/track/<split>/<vid>/<frame>.txt`` with lines
    ``{class} {id} {x1:.6f} {y1:.6f} {w:.6f} {h:.6f}``, for every video folder of ``images/track/<split>``.  Crowd
    labels and categories outside the eight classes are dropped (the reference's ``filter_crowd`` and
    ``filter_ignore``); a frame without labels gets no file, a frame whose labels are all dropped an empty one.  Then
    the frames that have a label file are listed, one ``images/track/<split>/<vid>/<frame>`` per line, in ``list_path``
    (default ``<data_root>/BDD100K/filter.bdd100k.<split>``; the reference's ``generate_txt``).  Returns the label
    files written."""
    root = os.path.join(data_root, "BDD100K")
    img_dir = os.path.join(root, "images", "track", split)
    label_dir = os.path.join(root, "labels", "box_track_20", split)
    save_dir = os.path.join(root, "filter_labels", "track", split)
    written = []
    vids = sorted(os.listdir(img_dir))
    for vid in vids:
        txt_label_dir = os.path.join(save_dir, vid)
        os.makedirs(txt_label_dir, exist_ok=True)
        with open(os.path.join(label_dir, vid + ".json")) as f:
            annos = json.load(f)
        for anno in annos:
            labels = anno["labels"]
            if len(labels) < 1:
                continue
            lines = []
            for label in labels:
                category = label["category"]
                if label["attributes"]["crowd"] or category not in BDD_KEPT:
                    continue
                box = label["box2d"]
                x1, x2, y1, y2 = box["x1"], box["x2"], box["y1"], box["y2"]
                w, h = x2 - x1, y2 - y1
                cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
                lines.append("{:d} {:d} {:.6f} {:.6f} {:.6f} {:.6f}\n".format(
                    BDD_CATEGORY_IDS[category], int(label["id"]), cx - 0.5 * w, cy - 0.5 * h, w, h))     # x1 y1 w h
            path = os.path.join(txt_label_dir, anno["name"].replace("jpg", "txt"))
            _write_whole(path, "".join(lines))
            written.append(path)
    frames = []
    for vid in vids:
        for fid in sorted(os.listdir(os.path.join(img_dir, vid))):
            if os.path.exists(os.path.join(save_dir, vid, fid.replace("jpg", "txt"))):
                frames.append(f"images/track/{split}/{vid}/{fid}")
    if list_path is None:
        list_path = os.path.join(root, f"filter.bdd100k.{split}")
    _write_whole(list_path, "".join(frame + "\n" for frame in frames))
    return written


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = argparse.ArgumentParser("python -m memotr_amd.data.prepare",
                                     description="Write the ground-truth trees that training reads.")
    parser.add_argument("dataset", choices=("mot17", "crowdhuman", "bdd100k"))
    parser.add_argument("--data-root", required=True, help="The directory that holds MOT17/, CrowdHuman/, BDD100K/.")
    parser.add_argument("--split", nargs="*", help="Default: train (crowdhuman: train val).")
    args = parser.parse_args(argv)
    splits = args.split or (["train", "val"] if args.dataset == "crowdhuman" else ["train"])
    if args.dataset == "crowdhuman":
        written = prepare_crowdhuman(args.data_root, splits)
    else:
        fn = prepare_mot17 if args.dataset == "mot17" else prepare_bdd100k
        written = [p for split in splits for p in fn(args.data_root, split)]
    print(f"{args.dataset}: {len(written)} files")


if __name__ == "__main__":
    main()
