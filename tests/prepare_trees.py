"""The tiny downloaded-dataset trees of the dataset-preparation tests and of tests/golden/gen_golden_prepare.py (test
infrastructure).  ``write_inputs(root)`` builds, under ``root`` (a DATA_ROOT), what ``memotr_amd/data/prepare.py`` reads:

  * ``MOT17/images/train/<seq>/gt/gt.txt`` (+ ``seqinfo.ini``) for three sequences.  The rows hold a ``mark == 0`` row,
    a row of another class, fractional and negative coordinates, two frames of one sequence that interleave, and --
    twice -- a sequence whose first kept id equals the last kept id of the sequence before it (the running track number
    then does NOT go up: ids 3 -> 3 between the first two, 7 -> 7 between the last two, once behind a dropped row);
  * ``CrowdHuman/annotation_{train,val}.odgt`` and an (empty) image file per record: an ignored box, a box without
    ``extra``, an ``extra`` without ``ignore``, float box values, a record whose boxes are all ignored;
  * ``BDD100K/labels/box_track_20/train/<vid>.json`` and (empty) frame files under ``images/track/train/<vid>/``: a
    crowd label, the three categories outside the eight classes, a frame without labels, a frame whose labels are all
    dropped, a frame file that the annotations do not mention.

``read_tree(root, sub)`` is {relative path with "/": text} of every file under ``root/sub``.
"""
import json
import os

MOT_ROWS = {
    # frame, id, x, y, w, h, mark, class, visibility
    "MOT17-02-SDP": [
        (1, 1, 912.0, 484.0, 97.0, 109.0, 1, 1, 1.0),
        (1, 2, 1338.5, 418.25, 167.0, 379.0, 1, 1, 0.33333),
        (2, 1, 914.9, 484.9, 97.0, 109.0, 0, 1, 1.0),               # mark == 0: dropped
        (2, 2, 1342.0, 417.0, 168.0, 380.0, 1, 1, 0.5),
        (1, 3, -6.5, 100.75, 40.0, 90.5, 1, 1, 0.86014),            # frame 1 again: its file gets a third line
        (2, 9, 300.0, 200.0, 30.0, 60.0, 1, 7, 1.0),                # another class: dropped
        (3, 3, -4.0, 101.0, 40.0, 90.0, 1, 1, 0.25),
    ],
    "MOT17-04-SDP": [
        (1, 3, 10.0, 20.0, 30.0, 40.0, 1, 1, 1.0),                  # first id == the last id before: no new track number
        (2, 3, 11.0, 21.0, 30.0, 40.0, 1, 1, 0.0),
        (1, 4, 50.7, 60.2, 20.0, 45.0, 1, 1, 0.75),
        (2, 4, 51.7, 61.2, 20.0, 45.0, 1, 1, 0.125),
        (2, 7, 90.0, 10.0, 12.0, 33.0, 1, 1, 1.0),
    ],
    "MOT17-09-SDP": [
        (1, 5, 1.0, 1.0, 5.0, 5.0, 1, 2, 1.0),                      # dropped: the id of the first KEPT row decides
        (1, 7, 91.0, 11.0, 12.0, 33.0, 1, 1, 0.4),
        (2, 7, 92.0, 12.0, 12.0, 33.0, 1, 1, 0.6),
        (2, 1, 200.0, 150.0, 25.0, 70.0, 1, 1, 1.0),
    ],
}

CROWDHUMAN = {
    "train": [
        {"ID": "273271,c9db000d5146c15", "gtboxes": [
            {"tag": "person", "hbox": [123, 129, 63, 64], "fbox": [61, 123, 191, 453], "vbox": [62, 126, 154, 446],
             "extra": {"box_id": 0, "occ": 1}},
            {"tag": "person", "fbox": [214, 97, 91, 324], "extra": {"ignore": 0}},
            {"tag": "mask", "fbox": [318, 109, 60, 38], "extra": {"ignore": 1}},
            {"tag": "person", "fbox": [-12, 70.9, 55.5, 200]}]},
        {"ID": "273275,cd061000af95f691", "gtboxes": [
            {"tag": "mask", "fbox": [1, 2, 3, 4], "extra": {"ignore": 1}}]},
        {"ID": "282555,b9a6000f1c27c5e", "gtboxes": [
            {"tag": "person", "fbox": [5, 6, 70, 80], "extra": {}}]},
    ],
    "val": [
        {"ID": "273278,1017c000ac1360b7", "gtboxes": [
            {"tag": "person", "fbox": [72, 202, 163, 503], "extra": {"ignore": 0}},
            {"tag": "person", "fbox": [199, 180, 144, 499], "extra": {"ignore": 1}},
            {"tag": "person", "fbox": [310, 200, 162, 497]}]},
    ],
}


def _bdd_label(obj_id, category, x1, y1, x2, y2, crowd=False):
    return {"id": str(obj_id), "category": category, "attributes": {"occluded": False, "truncated": False, "crowd": crowd},
            "box2d": {"x1": x1, "x2": x2, "y1": y1, "y2": y2}}


BDD = {
    # vid: [labels of frame 1, 2, ...]; a frame file without an entry here: BDD_EXTRA_FRAMES
    "b1c66a42-6f7d68ca": [
        [_bdd_label(101, "car", 100.25, 200.5, 180.75, 260.125), _bdd_label(102, "pedestrian", 10.1, 20.2, 30.3, 80.4),
         _bdd_label(103, "car", 400.0, 210.0, 640.0, 330.0, crowd=True)],
        [],                                                                                 # no labels: no file
        [_bdd_label(101, "car", 104.3333333, 201.6666667, 185.1, 262.7), _bdd_label(104, "other vehicle", 1, 2, 3, 4),
         _bdd_label(105, "trailer", 5, 6, 70, 80), _bdd_label(106, "truck", 500.123456789, 100.0, 700.987654321, 300.5)],
        [_bdd_label(107, "other person", 9, 9, 19, 39), _bdd_label(108, "bus", 0, 0, 10, 10, crowd=True)],   # an empty file
    ],
    "b1c81faa-3df17267": [
        [_bdd_label(7, "rider", 300.5, 100.5, 340.0, 190.0), _bdd_label(8, "bicycle", 298.0, 140.0, 345.5, 200.25),
         _bdd_label(9, "motorcycle", 20.0, 150.0, 90.0, 210.0), _bdd_label(10, "train", 0.0, 50.0, 1279.0, 400.0),
         _bdd_label(11, "bus", 600.6, 120.2, 820.4, 330.9)],
        [_bdd_label(7, "rider", 302.0, 101.0, 341.5, 190.5)],
    ],
}
BDD_EXTRA_FRAMES = {"b1c81faa-3df17267": 3}          # this frame has a file and no annotation entry


def bdd_frame_name(vid, t):
    return f"{vid}-{t:07d}.jpg"


def _write(path, text=""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def write_inputs(root):
    """Returns ``root``."""
    for seq, rows in MOT_ROWS.items():
        seq_dir = os.path.join(root, "MOT17", "images", "train", seq)
        _write(os.path.join(seq_dir, "gt", "gt.txt"),
               "".join(",".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n" for row in rows))
        _write(os.path.join(seq_dir, "seqinfo.ini"),
               f"[Sequence]\nname={seq}\nimDir=img1\nframeRate=30\nseqLength=3\nimWidth=1920\nimHeight=1080\nimExt=.jpg\n")
    for split, records in CROWDHUMAN.items():
        _write(os.path.join(root, "CrowdHuman", f"annotation_{split}.odgt"),
               "".join(json.dumps(r) + "\n" for r in records))
        for r in records:
            _write(os.path.join(root, "CrowdHuman", "images", split, r["ID"] + ".jpg"))
    for vid, frames in BDD.items():
        annos = [{"name": bdd_frame_name(vid, t + 1), "videoName": vid, "frameIndex": t, "labels": labels}
                 for t, labels in enumerate(frames)]
        _write(os.path.join(root, "BDD100K", "labels", "box_track_20", "train", vid + ".json"), json.dumps(annos))
        for t in list(range(1, len(frames) + 1)) + [BDD_EXTRA_FRAMES.get(vid)]:
            if t is not None:
                _write(os.path.join(root, "BDD100K", "images", "track", "train", vid, bdd_frame_name(vid, t)))
    return root


def read_tree(root, sub):
    out = {}
    top = os.path.join(root, sub)
    for directory, _, names in os.walk(top):
        for name in names:
            path = os.path.join(directory, name)
            with open(path) as f:
                out[os.path.relpath(path, root).replace(os.sep, "/")] = f.read()
    return out


def read_outputs(root):
    """What the three converters leave under ``root``, by dataset: {"mot17" | "crowdhuman" | "bdd100k": {path: text}}."""
    bdd = read_tree(root, os.path.join("BDD100K", "filter_labels"))
    with open(os.path.join(root, "BDD100K", "filter.bdd100k.train")) as f:
        bdd["BDD100K/filter.bdd100k.train"] = f.read()
    return {"mot17": read_tree(root, os.path.join("MOT17", "gts")),
            "crowdhuman": read_tree(root, os.path.join("CrowdHuman", "gts")), "bdd100k": bdd}
