"""What tests/test_frames_cpu.py, tests/test_frames_gpu.py and tests/golden/make_frame_pins.py share: the procedural inputs of the frame store's
pins (they are rebuilt, never stored), the pins of tests/golden/frame_pins.npz, and stand-in cameras shaped like scene/cameras.py's.

Every comparison against the pins is EXACT: the composite is fp64 arithmetic in a stated order followed by a truncation, the fetch is a table
look-up -- there is no rounding left to grant a tolerance for."""
import functools
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS_PATH = os.path.join(ROOT, "tests", "golden", "frame_pins.npz")
#: black, white (the reference's two: scene/dataset_readers.py) and one triple no byte / 255 equals
BACKGROUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.3, 0.55, 0.9))
#: (H, W) of the three random images: H*W mod 4 = 3, 3 and 0
SIZES = ((3, 5), (7, 9), (17, 64))
RAND_BGS = ((1.0, 1.0, 1.0), (0.3, 0.55, 0.9), (0.0, 0.0, 0.0))
#: (H, W) the fetch is held to: H*W mod 4 = 1, 3, 3, 0, 3, 0, 0 and -- (1,2), added for it -- 2: both plane alignments, a one-lane frame, a last
#: lane of 1, 2 and 3 pixels, one workgroup and more than one
FETCH_SIZES = ((1, 1), (1, 3), (3, 5), (2, 2), (7, 9), (16, 16), (17, 64), (1, 2))


def pins():
    return np.load(PINS_PATH)


def all_pairs_rgba():
    """(256,256,4) uint8: pixel (row c, column a) = (c, c, c, a)."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(np.stack([c, c, c, a], axis=-1))


@functools.lru_cache(maxsize=None)
def _random_rgba(k):
    g = np.random.default_rng(9100 + k)
    img = g.integers(0, 256, (*SIZES[k], 4), dtype=np.uint8)
    img[0, 0] = (255, 0, 128, 255)   # an opaque and a transparent pixel are present
    img[-1, -1] = (17, 200, 3, 0)
    return img


def random_rgba(k):
    return _random_rgba(k).copy()


def random_rgb(hw, seed):
    """(H, W, 3) uint8 for the fetch tests; byte values 0 and 255 present when there is room."""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    img.flat[0] = 255
    img.flat[-1] = 0
    return img


def expected_image(rgb, table):
    """What the reference makes of composited bytes: table[byte], planar."""
    return np.ascontiguousarray(np.asarray(table)[rgb.astype(np.int64)].transpose(2, 0, 1))


def stand_in_camera(rgba=None, bg=(1.0, 1.0, 1.0), path=None, width=None, height=None, seed=0):
    """An object with the attributes of scene/cameras.py's Camera that the dataset and the renderer read: the image (in memory or by path), the
    background, the size and three fp32 camera tensors (the matrices as transposed views, as the reference holds them)."""
    from PIL import Image

    g = torch.Generator().manual_seed(100 + seed)
    wvt = torch.rand(4, 4, generator=g).transpose(0, 1)
    fpt = torch.rand(4, 4, generator=g).transpose(0, 1)
    if rgba is not None:
        height, width = (rgba.shape[0] if height is None else height), (rgba.shape[1] if width is None else width)
    return types.SimpleNamespace(image=None if rgba is None else Image.fromarray(rgba, "RGBA"), image_path=path, bg=np.array(bg), image_width=width,
                                 image_height=height, image_name=f"cam{seed}", uid=seed, timestep=seed, world_view_transform=wvt,
                                 full_proj_transform=fpt, camera_center=torch.rand(3, generator=g), FoVx=0.5, FoVy=0.6)


def reference_getitem(camera):
    """scene/__init__.py:41-63 restated for a stand-in dataset (the tests that have the reference use ITS class; the others need a fallback
    that behaves like it): numpy fp64 composite, bytes, / 255, clamp."""
    from copy import deepcopy

    from PIL import Image

    camera = deepcopy(camera)
    image = Image.open(camera.image_path) if camera.image is None else camera.image
    n = np.array(image.convert("RGBA")) / 255.0
    arr = n[:, :, :3] * n[:, :, 3:4] + camera.bg * (1 - n[:, :, 3:4])
    image = Image.fromarray(np.array(arr * 255.0, dtype=np.byte).view(np.uint8), "RGB").resize((camera.image_width, camera.image_height))
    camera.original_image = (torch.from_numpy(np.array(image)) / 255.0).permute(2, 0, 1).clamp(0.0, 1.0)
    return camera


class StandInDataset(torch.utils.data.Dataset):
    """scene.CameraDataset's shape: `cameras`, `__len__`, int and slice indexing."""

    def __init__(self, cameras):
        self.cameras = cameras

    def __len__(self):
        return len(self.cameras)

    def __getitem__(self, idx):
        if isinstance(idx, int):
            return reference_getitem(self.cameras[idx])
        elif isinstance(idx, slice):
            return StandInDataset(self.cameras[idx])
        raise TypeError("Invalid argument type")
