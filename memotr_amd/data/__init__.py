"""Input side: raw decoded frames to the padded normalised batch the model reads (frames.py, the per-frame path) and
the training-clip augmentation (augment.py), for clips of a sequence and for clips made from one still image
(static_clip.py); in front of both, JPEG files to uint8 frames (jpeg.py); and the way back out, uint8 frames to JPEG
files (jpeg_write.py).  Around them, from dataset folders to training batches: which frames make a clip and their ground
truth (datasets.py) and the prefetching clip loader that drives the stages above one clip ahead of the train step
(loader.py)."""
from .augment import augment_clip, clip_batch  # noqa: F401
from .static_clip import augment_static_clip  # noqa: F401
from .jpeg import (CorruptJpeg, JpegCoefficients, JpegInfo, UnsupportedJpeg, decode_coefficients_host,  # noqa: F401
                   decode_jpeg, decode_jpegs, entropy_decode, parse_jpeg)
from .jpeg_write import encode_jpeg, encode_jpegs, forward_coefficients_host, huffman_encode  # noqa: F401
from .datasets import (BDD100KDataset, ClipDataset, ClipSample, DanceTrackDataset, MOT17Dataset,  # noqa: F401
                       build_dataset)
from .loader import ClipLoader  # noqa: F401
