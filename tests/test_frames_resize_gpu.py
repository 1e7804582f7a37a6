"""GPU tests of the frame store's resize (include/gfs.h: gfs_resample) on the MI355X: the two passes against the installed Pillow's
`Image.resize` at every shape where a kernel of this kind breaks, byte for byte, with the padding and the neighbouring slots checked; a
device store over cameras at their file's size and at another against the reference's `__getitem__`, through `image`, the dataset and the
batched fetch; and the adoption switch.

Every comparison is exact (tests/test_frames_resize_cpu.py says why).  No test reads the reference; DataLoaders run with num_workers=0."""
import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib
from gaussianavatars_amd import frames as FR

import frame_cases as FC

pytestmark = pytest.mark.gpu
MARK = 0xA5

#: (H, W) -> (H, W).  The first eight: both axes down by a non-integer with an odd pixel count (padding bytes); one axis down and one up;
#: horizontal only; vertical only; one output pixel, its window clipped at both borders; 13 taps over a source of three rows; a factor of 4
#: (17 taps); a pure up-scale (5 taps).  The last two are the other paths of the horizontal pass: a second band of rows and a second
#: workgroup along the row ((40,300) -> (40,280)), and a piece of source too long for LDS, read from global memory ((3,6000) -> (2,300)).
SHAPES = (((7, 9), (4, 5)), ((16, 16), (15, 17)), ((33, 17), (33, 9)), ((33, 17), (11, 17)), ((5, 5), (1, 1)), ((3, 200), (2, 67)),
          ((64, 48), (16, 12)), ((40, 40), (41, 57)), ((40, 300), (40, 280)), ((3, 6000), (2, 300)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _pillow(rgb, hw):
    from PIL import Image

    return np.array(Image.fromarray(rgb, "RGB").resize((hw[1], hw[0])))


def _three_frames(hw):
    """A random frame, a 0 / 255 checkerboard (the negative lobes overshoot at both ends) and constant 255 (the coefficients of a row must sum
    to exactly one after rounding, or 254 appears)."""
    y, x = np.mgrid[0:hw[0], 0:hw[1]]
    board = np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return [FC.random_rgb(hw, 900 + hw[0] + hw[1]), np.ascontiguousarray(board), np.full((*hw, 3), 255, np.uint8)]


def _filled_group(frames, first, capacity, dev):
    H, W = frames[0].shape[:2]
    g = FR._Group(H, W, capacity, dev)
    g.frames.fill_(MARK)
    rows = g.frames.view(g.capacity, g.stride)
    for i, f in enumerate(frames):
        rows[first + i, :H * W * 3] = torch.from_numpy(f.reshape(-1)).to(dev)
    return g


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_resample_equals_pillow_writes_zero_padding_and_leaves_the_other_slots(dev, src, dst):
    frames = _three_frames(src)
    want = [_pillow(f, dst) for f in frames]
    assert np.all(want[2] == 255)                                                          # (what Pillow makes of a constant frame)
    source = _filled_group(frames, 1, 5, dev)                                              # source slots 1 .. 3 of 5
    out = FR._Group(dst[0], dst[1], 6, dev)
    out.frames.fill_(MARK)
    staging = FR._Staging(dev)
    kx, bx, ksx = staging.axis(src[1], dst[1])
    ky, by, ksy = staging.axis(src[0], dst[0])
    lib = _lib.gfs()
    tmp = torch.full((lib.gfs_resample_tmp_bytes(src[0], dst[1], 3) + 16,), MARK, dtype=torch.uint8, device=dev)
    rc = lib.gfs_resample(src[0], src[1], source.frames.data_ptr(), source.capacity, 1, dst[0], dst[1], kx, bx, ksx, ky, by, ksy,
                          tmp.data_ptr() if ksx and ksy else None, out.frames.data_ptr(), out.capacity, 2, 3, _lib.raw_stream(dev))
    assert rc == 0, _lib.gfs_error()
    rows = out.frames.view(out.capacity, out.stride).cpu().numpy()
    n = dst[0] * dst[1] * 3
    for i in range(3):
        got = rows[2 + i, :n].reshape(*dst, 3)
        assert np.array_equal(got, want[i]), (i, int((got != want[i]).sum()))
        assert not rows[2 + i, n:].any(), i                                                 # every byte behind the last pixel, up to the stride
    assert np.all(rows[[0, 1, 5]] == MARK)                                                  # slots 0, 1 and 5: untouched
    assert np.all(tmp[-16:].cpu().numpy() == MARK)                                          # nothing behind the staging it was told of
    assert np.all(source.frames.view(source.capacity, source.stride)[[0, 4]].cpu().numpy() == MARK)


def _mixed_cameras():
    """Six cameras over files of 7 x 9 and 16 x 16: at the file's size, smaller on both axes, one axis only, larger; three backgrounds."""
    g = np.random.default_rng(17)
    sizes = [((7, 9), (7, 9)), ((7, 9), (4, 5)), ((16, 16), (15, 17)), ((7, 9), (4, 5)), ((16, 16), (16, 16)), ((16, 16), (16, 7))]
    cams = []
    for i, (file_hw, hw) in enumerate(sizes):
        cam = FC.stand_in_camera(g.integers(0, 256, (*file_hw, 4), dtype=np.uint8), FC.BACKGROUNDS[i % 3], seed=i)
        cam.image_height, cam.image_width = hw
        cams.append(cam)
    return cams


def test_device_store_over_mixed_cameras_returns_the_references_images_every_way(dev, monkeypatch):
    cams = _mixed_cameras()
    want = [FC.reference_getitem(c).original_image for c in cams]
    store = FR.FrameStore.from_cameras(cams, dev, resample=True)
    try:
        assert all(store.resident(i) for i in range(6)) and store.groups[(4, 5)].capacity == 2
        assert store.bytes == sum(FR.frame_stride(c.image_height, c.image_width) for c in cams)
        for i in range(6):
            got = store.image(i)
            assert got.is_cuda and got.shape == want[i].shape and torch.equal(got, want[i].to(dev)), i
        ds = FR.ResidentCameraDataset(cams, store, fallback=None)
        for i, cam in enumerate(torch.utils.data.DataLoader(ds, batch_size=None, num_workers=0)):
            assert isinstance(cam.original_image, FR.FrameRef) and cam._gaa_frame == (store.key, i)
            assert torch.equal(cam.original_image.cuda(), want[i].to(dev)), i
        slots = torch.tensor([1, 0, 1], dtype=torch.int64, device=dev)                      # the (4,5) group holds cameras 1 and 3
        batch = FR.fetch_batch(store, (4, 5), slots)
        assert torch.equal(batch[0], want[3].to(dev)) and torch.equal(batch[1], want[1].to(dev)) and torch.equal(batch[2], want[3].to(dev))
        monkeypatch.setenv("GAA_FRAME_STORE", "0")                                          # the composed path on the device: the same frames
        composed = FR.FrameStore.from_cameras(cams, dev, resample=True)
        try:
            for i in range(6):
                assert torch.equal(composed.rgb(i), store.rgb(i)), i
        finally:
            composed.release()
    finally:
        store.release()


def test_adopted_dataset_holds_resized_cameras_only_under_the_switch(dev, monkeypatch):
    from gaussianavatars_amd import patch

    cams = _mixed_cameras()
    want = [FC.reference_getitem(c).original_image.to(dev) for c in cams]
    monkeypatch.delenv("GAA_FRAME_STORE", raising=False)
    monkeypatch.delenv("GAA_FRAME_STORE_EVAL", raising=False)
    for value, refs in ((None, [True, False, False, False, True, False]), ("1", [True] * 6)):   # (the variable is read when the store is built)
        class Scene:
            def getTrainCameras(self, scale=1.0):
                return FC.StandInDataset(cams)

        if value is None:
            monkeypatch.delenv("GAA_FRAME_STORE_RESIZE", raising=False)
        else:
            monkeypatch.setenv("GAA_FRAME_STORE_RESIZE", value)
        assert patch.adopt_frame_store(Scene) == ["Scene.getTrainCameras"]
        ds = Scene().getTrainCameras()
        try:
            assert FR.lookup(ds.key).device == dev
            assert [isinstance(ds[i].original_image, FR.FrameRef) for i in range(6)] == refs
            assert all(torch.equal(ds[i].original_image.cuda(), want[i]) for i in range(6))
        finally:
            FR.release(ds.key)
            patch.unpatch_classes(Scene)
