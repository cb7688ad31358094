"""Input side of the per-frame path: raw decoded frames to the padded normalised batch the model reads."""
