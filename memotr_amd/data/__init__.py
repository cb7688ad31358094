"""Input side: raw decoded frames to the padded normalised batch the model reads (frames.py, the per-frame path) and
the training-clip augmentation (augment.py)."""
from .augment import augment_clip, clip_batch  # noqa: F401
