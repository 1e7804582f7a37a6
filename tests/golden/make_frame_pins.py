#!/usr/bin/env python3
"""Generates tests/golden/frame_pins.npz by RUNNING THE REFERENCE's own `CameraDataset.__getitem__` (scene/__init__.py:38-63; read-only checkout
beside this repository) on the CPU -- it does not travel to the GPU box, so the results it produces are committed, as make_eval_golden.py's are.

    python tests/golden/make_frame_pins.py

Pins of the resident frame store (include/gfs.h, gaussianavatars_amd/frames.py).  The inputs are built procedurally (tests/frame_cases.py builds
the same ones) and are not stored:

    all pairs     a 256x256 RGBA image whose pixel (row c, column a) has colour byte c in all three channels and alpha a: every (colour, alpha)
                  pair there is, composited over each background of BACKGROUNDS
    rand0..2      three odd-sized random RGBA images (SIZES), each over its own background

Recorded:

    table                 (256,) fp32: what the reference makes of every byte value (read off the opaque column of the all-pairs image over black)
    all_<k>_rgb           (256,256,3) uint8: the composited bytes over BACKGROUNDS[k], recovered EXACTLY from the reference's floats through `table`
    rand<k>_rgb           (H,W,3) uint8, likewise;  rand<k>_image  (3,H,W) fp32: `original_image` as the reference returns it

Numeric arrays only.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from gaussianavatars_amd import shims  # noqa: E402

shims.install()
from scene import CameraDataset  # noqa: E402  (the reference's)

from frame_cases import BACKGROUNDS, RAND_BGS, SIZES, all_pairs_rgba, random_rgba  # noqa: E402


def reference_image(rgba, bg):
    """`original_image` of a camera whose in-memory image is `rgba`, from the reference's dataset."""
    from PIL import Image

    cam = types.SimpleNamespace(image=Image.fromarray(rgba, "RGBA"), image_path=None, bg=np.array(bg), image_width=rgba.shape[1],
                                image_height=rgba.shape[0])
    out = CameraDataset([cam])[0].original_image
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, rgba.shape[0], rgba.shape[1])
    return out.contiguous().numpy()


def to_bytes(image, table):
    """(3,H,W) floats -> (H,W,3) bytes through the strictly increasing table; every float must BE a table entry."""
    idx = np.searchsorted(table, image)
    assert idx.max() < 256 and np.array_equal(table[idx], image)
    return np.ascontiguousarray(idx.astype(np.uint8).transpose(1, 2, 0))


def main():
    out = {}
    pairs = all_pairs_rgba()
    black = reference_image(pairs, (0, 0, 0))
    table = black[0, :, 255].copy()   # row c, alpha 255, over black: byte c
    assert np.all(np.diff(table) > 0) and table[0] == 0.0 and table[255] == 1.0
    out["table"] = table
    for k, bg in enumerate(BACKGROUNDS):
        out[f"all_{k}_rgb"] = to_bytes(reference_image(pairs, bg), table)
    for k, (hw, bg) in enumerate(zip(SIZES, RAND_BGS)):
        image = reference_image(random_rgba(k), bg)
        out[f"rand{k}_image"], out[f"rand{k}_rgb"] = image, to_bytes(image, table)
    path = os.path.join(HERE, "frame_pins.npz")
    np.savez_compressed(path, **out)
    print("frame_pins.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
