"""Clip datasets: which frames make a training clip, and their ground truth.  No pixels are read here.

One class per directory layout of the reference (data/dancetrack.py, data/mot17.py, data/bdd100k.py), with one small
interface that ``loader.ClipLoader`` drives:

    dataset = build_dataset(config)                       # dispatches on config["DATASET"], data/__init__.py:27-39
    dataset.set_epoch(epoch); len(dataset)
    sample = dataset.sample(index, rng)                   # ClipSample(paths, infos, static, overflow_bbox)
    plan = dataset.sample_plan(h, w, rng, np_rng, sample.static)          # a ClipAugment

``set_epoch`` picks the sampling stage from SAMPLE_STEPS (length, mode and interval are the ``min(len - 1, stage)``
entries of their lists) and lists the epoch's begin frames, ``t_min .. t_max - (length - 1)`` of every sequence.
``sample`` draws ``interval = min(rng.randint(1, sample_interval), floor((t_max - begin) / (length - 1)))`` from the
``random.Random`` it is given -- the one draw the reference takes from the global generator at this point -- and
returns the file paths with the reference's pre-transform infos: ``boxes`` xyxy in pixels (float32), ``ids`` and
``labels`` (int64) and ``areas``, each with the dtype the reference's ``torch.as_tensor`` gives it.  Only the
``random_interval`` mode exists; any other raises as in the reference.

Where this differs from the reference, on purpose:

  * sequences (and CrowdHuman images) are taken in ``sorted(os.listdir(...))`` order.  The reference takes whatever
    order the file system returns, and DanceTrack's id offset ``vid_idx * 100000`` depends on it;
  * datasets are told apart by where an entry came from, never by substrings of its path (the reference asks whether
    "CrowdHuman" or "MOT17" occurs anywhere in the full path, DATA_ROOT included);
  * a malformed ground-truth line raises ``ValueError`` naming the file and the line.

Kept from the reference, because its dictionaries behave that way: a sequence, frame or image whose ground-truth file
has no line does not exist for sampling (BDD100K: such a frame counts as missing when begin frames are filtered and
when a drawn interval is checked; DanceTrack: such a sequence takes no ``vid_idx``; CrowdHuman: such an image is not
in the epoch).  ``BDD100KDataset.frame_info`` still gives such a frame the reference's one fake box.
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Dict, List, Sequence, Tuple

import torch

from .augment import SCALES, ClipAugment, sample_clip_augment

COCO_SCALES = (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)      # reference data/bdd100k.py:202
STATIC_MAX_SHIFT = 50                                                      # MultiRandomShift's default
CROWDHUMAN_ID_OFFSET = 100000
VIDEO_ID_OFFSET = 100000


@dataclasses.dataclass
class ClipSample:
    """``paths``: one file per frame (a still image: the same path ``length`` times); ``infos``: one dict per frame;
    ``static``: the clip is made from one still image (``augment_static_clip``); ``overflow_bbox``: what the crop
    branch does with boxes that leave the window."""
    paths: List[str]
    infos: List[dict]
    static: bool
    overflow_bbox: bool


def _fields(path: str, n: int, line: str, sep, count: int) -> List[str]:
    parts = line.split(sep)
    if len(parts) < count if sep == "," else len(parts) != count:
        raise ValueError(f"{path}:{n}: expected {count} fields separated by {sep!r}, got {len(parts)}: {line!r}")
    return parts


def _numbers(path: str, n: int, line: str, parts: Sequence[str], kinds: str) -> list:
    """``kinds``: one letter per field, i: int(), f: float(), t: int(float()), the reference's truncation."""
    try:
        return [int(p) if k == "i" else float(p) if k == "f" else int(float(p)) for p, k in zip(parts, kinds)]
    except (ValueError, OverflowError):
        raise ValueError(f"{path}:{n}: not a number in {line!r}") from None


def _info(boxes_xywh: list, ids: list, labels: list, areas: list) -> dict:
    """The reference's tensors (dancetrack.py:134-144): xywh -> xyxy in float32; no box: the empty tensors it builds."""
    if not ids:
        return {"boxes": torch.zeros((0, 4)), "ids": torch.zeros((0,), dtype=torch.long),
                "labels": torch.zeros((0,), dtype=torch.long), "areas": torch.as_tensor([])}
    boxes = torch.as_tensor(boxes_xywh, dtype=torch.float32)
    boxes[:, 2:] += boxes[:, :2]
    return {"boxes": boxes, "ids": torch.as_tensor(ids, dtype=torch.long),
            "labels": torch.as_tensor(labels, dtype=torch.long), "areas": torch.as_tensor(areas)}


class ClipDataset:
    """Stage selection, the begin list and the interval draw, shared by the layouts.  ``entries`` is the epoch's list;
    a subclass fills it in ``_list_epoch`` and resolves one entry in ``_frames_of``."""
    unknown_mode_error = ValueError

    def __init__(self, config: dict):
        self.config = config
        self.sample_steps = list(config["SAMPLE_STEPS"])
        self.sample_lengths = list(config["SAMPLE_LENGTHS"])
        self.sample_modes = list(config["SAMPLE_MODES"])
        self.sample_intervals = list(config["SAMPLE_INTERVALS"])
        self.sample_stage = self.sample_length = self.sample_mode = self.sample_interval = None
        self.sample_vid_tmax: Dict[str, int] = {}
        self.entries: list = []

    def __len__(self) -> int:
        return len(self.entries)

    def set_epoch(self, epoch: int) -> None:
        stage = sum(1 for step in self.sample_steps if epoch >= step)
        self.sample_stage = stage
        self.sample_length = self.sample_lengths[min(len(self.sample_lengths) - 1, stage)]
        self.sample_mode = self.sample_modes[min(len(self.sample_modes) - 1, stage)]
        self.sample_interval = self.sample_intervals[min(len(self.sample_intervals) - 1, stage)]
        self.sample_vid_tmax = {}
        self.entries = []
        self._list_epoch(epoch)

    def _begin_frames(self, vid: str, frames) -> List[int]:
        t_min, t_max = min(frames), max(frames)
        self.sample_vid_tmax[vid] = t_max
        return list(range(t_min, t_max - (self.sample_length - 1) + 1))

    def frame_indices(self, vid: str, begin: int, rng) -> List[int]:
        """The reference's ``sample_frames_idx``: one ``rng.randint`` and the ``sample_length`` frame numbers."""
        if self.sample_mode != "random_interval":
            raise self.unknown_mode_error(f"Sample mode {self.sample_mode} is not supported.")
        if self.sample_length < 2:
            raise ValueError("Sample length is less than 2.")
        max_interval = math.floor((self.sample_vid_tmax[vid] - begin) / (self.sample_length - 1))
        interval = min(rng.randint(1, self.sample_interval), max_interval)
        return [begin + interval * k for k in range(self.sample_length)]

    def sample(self, index: int, rng) -> ClipSample:
        raise NotImplementedError

    def sample_plan(self, h: int, w: int, rng, np_rng, static: bool = False) -> ClipAugment:
        raise NotImplementedError

    def _list_epoch(self, epoch: int) -> None:
        raise NotImplementedError


class DanceTrackDataset(ClipDataset):
    """``<DATA_ROOT>/<DATASET>/<split>/<vid>/gt/gt.txt`` with lines ``t,i,x,y,w,h,1,1,1`` and frames
    ``img1/%08d.jpg`` (DanceTrack) or ``img1/%06d.jpg`` (SportsMOT, anything else).  ``ids + vid_idx * 100000`` with
    ``vid_idx`` counted over the sorted sequence names, labels 0, ``areas = w * h``."""

    def __init__(self, config: dict, split: str = "train"):
        super().__init__(config)
        self.dataset_name = config["DATASET"]
        self.split_dir = os.path.join(config["DATA_ROOT"], self.dataset_name, split)
        if not os.path.isdir(self.split_dir):
            raise FileNotFoundError(f"Dir {self.split_dir} is not exist.")
        self.gts: Dict[str, Dict[int, list]] = {}
        for vid in sorted(os.listdir(self.split_dir)):
            path = os.path.join(self.split_dir, vid, "gt", "gt.txt")
            frames: Dict[int, list] = {}
            with open(path) as f:
                for n, line in enumerate(f, 1):
                    parts = _fields(path, n, line.strip(), ",", 9)[:9]
                    t, i, x, y, w, h, a, b, c = _numbers(path, n, line, parts, "iiffffiii")
                    if not a == b == c == 1:
                        raise ValueError(f"{path}:{n}: the three check digits must be 1, got {a}, {b}, {c}")
                    frames.setdefault(t, []).append((i, x, y, w, h))
            if frames:
                self.gts[vid] = frames
        self.vid_idx = {vid: k for k, vid in enumerate(self.gts)}
        self.set_epoch(0)

    def _list_epoch(self, epoch: int) -> None:
        for vid, frames in self.gts.items():
            self.entries.extend((vid, t) for t in self._begin_frames(vid, frames))

    def frame_path(self, vid: str, t: int) -> str:
        name = f"{t:08d}.jpg" if self.dataset_name == "DanceTrack" else f"{t:06d}.jpg"
        return os.path.join(self.split_dir, vid, "img1", name)

    def frame_info(self, vid: str, t: int) -> dict:
        gt = self.gts[vid].get(t, ())
        offset = self.vid_idx[vid] * VIDEO_ID_OFFSET
        return _info([[x, y, w, h] for _, x, y, w, h in gt], [i + offset for i, *_ in gt], [0] * len(gt),
                     [w * h for *_, w, h in gt])

    def sample(self, index: int, rng) -> ClipSample:
        vid, begin = self.entries[index]
        ts = self.frame_indices(vid, begin, rng)
        return ClipSample([self.frame_path(vid, t) for t in ts], [self.frame_info(vid, t) for t in ts], False,
                          bool(self.config["OVERFLOW_BBOX"]))

    def sample_plan(self, h, w, rng, np_rng, static=False) -> ClipAugment:
        return sample_clip_augment(h, w, rng, np_rng, coco_size=bool(self.config["COCO_SIZE"]),
                                   reverse_clip=float(self.config["REVERSE_CLIP"]), scales=SCALES, max_size=1536)


class MOT17Dataset(ClipDataset):
    """MOT17 (or MOT17_SPLIT) joint with CrowdHuman.  Sequences: the names under ``<DATA_ROOT>/<DATASET>/images/train``
    that contain ``SDP``; per-frame files ``<DATA_ROOT>/<DATASET>/gts/train/<vid>/img1/%06d.txt`` with lines
    ``_ i x y w h v`` separated by single blanks, the values truncated to int; ids as they are.  CrowdHuman:
    ``<DATA_ROOT>/CrowdHuman/{images,gts}/val``, ``<name>.txt`` with lines ``_ i x y w h`` of integers,
    ``ids + 100000``; a sample is the image ``length`` times with ``static=True``, and its plan carries a shift drawn
    with ``max_shift=50``.  The epoch lists CrowdHuman first (USE_CROWDHUMAN), then MOT17 from epoch SAMPLE_MOT17_JOIN
    on.  ``areas = w * h`` of the integers (an int64 tensor, as in the reference).

    USE_MOTSYNTH raises ``NotImplementedError``: MOTSynth is not read here, and no shipped config sets the key."""
    unknown_mode_error = NotImplementedError

    def __init__(self, config: dict, split: str = "train"):
        super().__init__(config)
        if config.get("USE_MOTSYNTH"):
            raise NotImplementedError("USE_MOTSYNTH is set: MOTSynth is not supported (no shipped config uses it)")
        if split != "train":
            raise ValueError(f"Split {split} is NOT supported.")
        root, name = config["DATA_ROOT"], config["DATASET"]
        self.use_crowdhuman = bool(config.get("USE_CROWDHUMAN"))
        self.sample_mot17_join = int(config["SAMPLE_MOT17_JOIN"])
        self.mot17_seqs_dir = os.path.join(root, name, "images", split)
        self.mot17_gts_dir = os.path.join(root, name, "gts", split)
        self.crowdhuman_seq_dir = os.path.join(root, "CrowdHuman", "images", "val")
        self.crowdhuman_gts_dir = os.path.join(root, "CrowdHuman", "gts", "val")
        self.mot17_gts: Dict[str, Dict[int, list]] = {}
        self.crowdhuman_gts: Dict[str, list] = {}
        for vid in sorted(os.listdir(self.mot17_seqs_dir)):
            if "SDP" not in vid:
                continue
            gts_dir = os.path.join(self.mot17_gts_dir, vid, "img1")
            frames: Dict[int, list] = {}
            for filename in sorted(os.listdir(gts_dir)):
                path = os.path.join(gts_dir, filename)
                try:
                    t = int(filename.split(".")[0])
                except ValueError:
                    raise ValueError(f"{path}: the file name is not a frame number") from None
                with open(path) as f:
                    for n, line in enumerate(f, 1):
                        parts = _fields(path, n, line.strip("\n"), " ", 7)
                        i, x, y, w, h, _ = _numbers(path, n, line, parts[1:], "tttttf")
                        frames.setdefault(t, []).append((i, x, y, w, h))
            if frames:
                self.mot17_gts[vid] = frames
        if self.use_crowdhuman:
            for filename in sorted(os.listdir(self.crowdhuman_gts_dir)):
                path = os.path.join(self.crowdhuman_gts_dir, filename)
                with open(path) as f:
                    for n, line in enumerate(f, 1):
                        parts = _fields(path, n, line.strip("\n"), " ", 6)
                        box = tuple(_numbers(path, n, line, parts[1:], "iiiii"))
                        self.crowdhuman_gts.setdefault(filename.split(".")[0], []).append(box)
        self.set_epoch(0)

    def _list_epoch(self, epoch: int) -> None:
        self.entries.extend(("CrowdHuman", name, None) for name in self.crowdhuman_gts)
        if epoch >= self.sample_mot17_join:
            for vid, frames in self.mot17_gts.items():
                self.entries.extend(("MOT17", vid, t) for t in self._begin_frames(vid, frames))

    def frame_path(self, source: str, name: str, t=None) -> str:
        if source == "CrowdHuman":
            return os.path.join(self.crowdhuman_seq_dir, f"{name}.jpg")
        return os.path.join(self.mot17_seqs_dir, name, "img1", str(t).zfill(6) + ".jpg")

    def frame_info(self, source: str, name: str, t=None) -> dict:
        gt = self.crowdhuman_gts[name] if source == "CrowdHuman" else self.mot17_gts[name].get(t, ())
        offset = CROWDHUMAN_ID_OFFSET if source == "CrowdHuman" else 0
        return _info([[float(v) for v in box[1:]] for box in gt], [box[0] + offset for box in gt], [0] * len(gt),
                     [box[3] * box[4] for box in gt])

    def sample(self, index: int, rng) -> ClipSample:
        source, name, begin = self.entries[index]
        overflow = bool(self.config["OVERFLOW_BBOX"])
        if source == "CrowdHuman":
            info = self.frame_info(source, name)
            infos = [{k: v.clone() for k, v in info.items()} for _ in range(self.sample_length)]
            return ClipSample([self.frame_path(source, name)] * self.sample_length, infos, True, overflow)
        ts = self.frame_indices(name, begin, rng)
        return ClipSample([self.frame_path(source, name, t) for t in ts],
                          [self.frame_info(source, name, t) for t in ts], False, overflow)

    def sample_plan(self, h, w, rng, np_rng, static=False) -> ClipAugment:
        return sample_clip_augment(h, w, rng, np_rng, coco_size=bool(self.config["COCO_SIZE"]),
                                   reverse_clip=float(self.config["REVERSE_CLIP"]), scales=SCALES, max_size=1536,
                                   max_shift=STATIC_MAX_SHIFT if static else None)


class BDD100KDataset(ClipDataset):
    """``<DATA_ROOT>/BDD100K/images/track/train/<vid>/<vid>-%07d.jpg`` and
    ``filter_labels/track/train/<vid>/<vid>-%07d.txt`` with lines ``c i x y w h``; ``labels = c - 1``, ids as they
    are, ``areas = w * h``.  A begin frame is kept only if all ``length`` consecutive frames have ground truth, and a
    drawn interval that meets a frame without falls back to consecutive frames.  A frame without boxes gets the
    reference's one fake box: ``[0.5, 0.5, 0.5, 0.5]`` as xywh, id 0, label 0, area 0.  The plan: the COCO scale list
    480 .. 800, ``max_size=1333``, the small crop sizes, ``overflow_bbox=True``, no reversal (bdd100k.py:200-225)."""

    def __init__(self, config: dict, split: str = "train"):
        super().__init__(config)
        if split != "train":
            raise ValueError(f"Split {split} is not supported!")
        self.images_dir = os.path.join(config["DATA_ROOT"], "BDD100K", "images", "track", "train")
        self.gts_dir = os.path.join(config["DATA_ROOT"], "BDD100K", "filter_labels", "track", "train")
        if not os.path.isdir(self.images_dir):
            raise FileNotFoundError(f"Dir {self.images_dir} is not exist.")
        self.gts: Dict[str, Dict[int, list]] = {}
        for vid in sorted(os.listdir(self.images_dir)):
            frames: Dict[int, list] = {}
            for frame_name in sorted(os.listdir(os.path.join(self.images_dir, vid))):
                gt_name = frame_name.replace(".jpg", ".txt")
                path = os.path.join(self.gts_dir, vid, gt_name)
                if not os.path.exists(path):
                    continue
                try:
                    t = int(gt_name[:-4].split("-")[-1])
                except ValueError:
                    raise ValueError(f"{path}: the file name does not end in a frame number") from None
                with open(path) as f:
                    for n, line in enumerate(f, 1):
                        parts = _fields(path, n, line.rstrip("\n"), " ", 6)
                        frames.setdefault(t, []).append(tuple(_numbers(path, n, line, parts, "iiffff")))
            if frames:
                self.gts[vid] = frames
        self.set_epoch(0)

    def _list_epoch(self, epoch: int) -> None:
        for vid, frames in self.gts.items():
            for t in self._begin_frames(vid, frames):
                if all(t + k in frames for k in range(self.sample_length)):
                    self.entries.append((vid, t))

    def frame_indices(self, vid: str, begin: int, rng) -> List[int]:
        ts = super().frame_indices(vid, begin, rng)
        if any(t not in self.gts[vid] for t in ts):
            ts = [begin + k for k in range(self.sample_length)]
        return ts

    def frame_path(self, vid: str, t: int) -> str:
        return os.path.join(self.images_dir, vid, f"{vid}-{t:07d}.jpg")

    def frame_info(self, vid: str, t: int) -> dict:
        gt = self.gts[vid].get(t, ())
        if not gt:
            return _info([[0.5, 0.5, 0.5, 0.5]], [0], [0], [0.0])
        return _info([[x, y, w, h] for _, _, x, y, w, h in gt], [i for _, i, *_ in gt], [c - 1 for c, *_ in gt],
                     [w * h for *_, w, h in gt])

    def sample(self, index: int, rng) -> ClipSample:
        vid, begin = self.entries[index]
        ts = self.frame_indices(vid, begin, rng)
        return ClipSample([self.frame_path(vid, t) for t in ts], [self.frame_info(vid, t) for t in ts], False, True)

    def sample_plan(self, h, w, rng, np_rng, static=False) -> ClipAugment:
        return sample_clip_augment(h, w, rng, np_rng, coco_size=True, reverse_clip=0.0, scales=COCO_SCALES,
                                   max_size=1333)


def build_dataset(config: dict, split: str = "train") -> ClipDataset:
    """The reference's dispatch on config["DATASET"] (data/__init__.py:27-39)."""
    name = config["DATASET"]
    if name in ("DanceTrack", "SportsMOT"):
        if split != "train":
            raise ValueError(f"Data split {split} is not supported for DanceTrack dataset.")
        return DanceTrackDataset(config, split)
    if name in ("MOT17", "MOT17_SPLIT"):
        return MOT17Dataset(config, split)
    if name == "BDD100K":
        return BDD100KDataset(config, split)
    raise ValueError(f"Dataset {name} is not supported!")
