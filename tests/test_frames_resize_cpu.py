"""CPU tests of the frame store's resize (include/gfs.h: gfs_resample; gaussianavatars_amd/frames.py: resample_tables, resample_composed,
from_cameras(..., resample=True)): the host restatement against the installed Pillow's `Image.resize`, byte for byte, the tables against
the rules of Resample.c, a host store over a camera that asks for another size than its file's against the reference's `__getitem__`, and
the argument checks of the entry.  Nothing here launches.

Every comparison is exact: an 8-bit resize in Pillow is integer arithmetic on coefficients rounded once (tests/frame_cases.py says the same
of the composite and the fetch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib
from gaussianavatars_amd import frames as FR

import frame_cases as FC

#: (H, W) -> (H, W): both axes down by a non-integer, by exactly two, by non-integer factors that differ, one axis only (each), both up, one
#: output pixel, 13 taps on a three-row image, a down-scale whose last window is clipped, one axis down and one up
SHAPES = (((7, 9), (4, 5)), ((550, 802), (275, 401)), ((64, 48), (21, 13)), ((33, 17), (33, 9)), ((33, 17), (11, 17)), ((40, 40), (41, 57)),
          ((5, 5), (1, 1)), ((3, 200), (2, 67)), ((101, 203), (50, 100)), ((16, 16), (15, 17)))


def _pillow(rgb, hw):
    from PIL import Image

    return np.array(Image.fromarray(rgb, "RGB").resize((hw[1], hw[0])))


@pytest.mark.parametrize("kind", ["bytes", "extremes"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_resample_composed_equals_pillows_resize(src, dst, kind):
    g = np.random.default_rng(src[0] * 1000 + src[1] + dst[0])
    rgb = g.integers(0, 256, (*src, 3), dtype=np.uint8)
    if kind == "extremes":   # 0 / 255 only: the negative lobes overshoot at both ends and the clamp is what is tested
        rgb = (rgb >> 7) * np.uint8(255)
    want = _pillow(rgb, dst)
    got = FR.resample_composed(torch.from_numpy(rgb), (dst[1], dst[0]))
    assert got.dtype is torch.uint8 and tuple(got.shape) == (*dst, 3) and got.is_contiguous()
    assert np.array_equal(got.numpy(), want), int((got.numpy() != want).sum())
    assert np.array_equal(FR.resample_composed(rgb, (dst[1], dst[0])), want)                                  # numpy in, numpy out
    two = FR.resample_composed(torch.from_numpy(np.stack([rgb, rgb[::-1].copy()])), (dst[1], dst[0]))          # leading dimensions
    assert np.array_equal(two[0].numpy(), want) and np.array_equal(two[1].numpy(), _pillow(rgb[::-1].copy(), dst))


def test_resample_composed_refuses_what_is_not_an_rgb_byte_image_and_copies_at_the_same_size():
    rgb = torch.from_numpy(FC.random_rgb((7, 9), 5))
    same = FR.resample_composed(rgb, (9, 7))
    assert torch.equal(same, rgb)
    for bad in (rgb.float(), rgb[..., :2], rgb[0, 0]):
        with pytest.raises(ValueError):
            FR.resample_composed(bad, (5, 4))


def _by_the_rules(n_in, n_out):
    """ksize and the bounds of one axis, from Resample.c's precompute_coeffs in Python floats (IEEE doubles), index by index."""
    scale = n_in / n_out
    support = 2.0 * max(scale, 1.0)
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        bounds.append((first, min(int(center + support + 0.5), n_in) - first))
    return ksize, bounds


@pytest.mark.parametrize("n_in,n_out,ksize", [(9, 5, 9), (200, 67, 13), (40, 57, 5), (64, 16, 17)])
def test_resample_tables_ksize_bounds_and_coefficients(n_in, n_out, ksize):
    coef, bounds = FR.resample_tables(n_in, n_out)
    want_ks, want_bounds = _by_the_rules(n_in, n_out)
    assert want_ks == ksize
    assert coef.dtype is torch.int32 and tuple(coef.shape) == (n_out, ksize) and bounds.dtype is torch.int32 and tuple(bounds.shape) == (n_out, 2)
    assert bounds.tolist() == [list(b) for b in want_bounds]
    first, taps = bounds[:, 0], bounds[:, 1]
    assert int(first.min()) >= 0 and int(taps.min()) >= 1 and int((first + taps).max()) <= n_in and int(taps.max()) <= ksize
    assert bool((first[1:] >= first[:-1]).all()) and bool(((first + taps)[1:] >= (first + taps)[:-1]).all())   # windows only move forward
    for i in range(n_out):
        assert not coef[i, int(taps[i]):].any()                                  # behind its taps a coefficient is zero
    # a row of weights sums to one: in 22 fractional bits, to within half a unit per tap
    assert int((coef.to(torch.int64).sum(1) - (1 << 22)).abs().max()) <= ksize // 2 + 1
    assert int(coef.abs().max()) < 1 << 23                                       # 24 bits with the sign
    assert FR.resample_tables(n_in, n_out)[0] is coef                            # computed once per pair


def test_resample_tables_of_an_unchanged_axis_is_none_and_bad_sizes_raise():
    assert FR.resample_tables(17, 17) is None
    for bad in ((0, 4), (4, 0), (-1, 3)):
        with pytest.raises(ValueError):
            FR.resample_tables(*bad)


def _cameras():
    g = np.random.default_rng(3)
    cams = [FC.stand_in_camera(g.integers(0, 256, (7, 9, 4), dtype=np.uint8), FC.BACKGROUNDS[i % 3], seed=i) for i in range(4)]
    cams[1].image_width, cams[1].image_height = 5, 4      # the file is 9 x 7
    return cams


def test_host_store_with_resample_holds_the_resized_camera_and_returns_the_references_image():
    cams = _cameras()
    store = FR.FrameStore.from_cameras(cams, "cpu", resample=True)
    try:
        assert [store.resident(i) for i in range(4)] == [True] * 4
        assert sorted(store.groups) == [(4, 5), (7, 9)] and store.groups[(4, 5)].capacity == 1 and store.groups[(7, 9)].capacity == 3
        assert store.where[1] == ((4, 5), 0) and store.shape(1) == (3, 4, 5)
        assert store.bytes == 3 * FR.frame_stride(7, 9) + FR.frame_stride(4, 5)            # the budget counts what is stored
        for i, cam in enumerate(cams):
            want = FC.reference_getitem(cam).original_image
            got = store.image(i)
            assert got.dtype is torch.float32 and got.is_contiguous() and got.shape == want.shape and torch.equal(got, want), i
        ds = FR.ResidentCameraDataset(cams, store, fallback=FC.StandInDataset(cams))
        small = ds[1]
        assert isinstance(small.original_image, FR.FrameRef) and small.original_image.shape == (3, 4, 5) and small._gaa_frame == (store.key, 1)
        assert torch.equal(small.original_image.to("cpu"), FC.reference_getitem(cams[1]).original_image)
    finally:
        store.release()


def test_without_the_argument_the_resized_camera_is_not_resident_and_bad_targets_never_are():
    cams = _cameras()
    store = FR.FrameStore.from_cameras(cams, "cpu")
    try:
        assert [store.resident(i) for i in range(4)] == [True, False, True, True] and sorted(store.groups) == [(7, 9)]
    finally:
        store.release()
    cams[1].image_width = 0
    cams[2].bg = np.array([1.0, 1.0])
    stride = FR.frame_stride(7, 9)
    store = FR.FrameStore.from_cameras(cams, "cpu", budget_bytes=stride + stride // 2, resample=True)      # room for one frame of 7 x 9
    try:
        assert [store.resident(i) for i in range(4)] == [True, False, False, False] and store.bytes == stride
    finally:
        store.release()


def test_the_switch_is_off_unless_set(monkeypatch):
    monkeypatch.delenv("GAA_FRAME_STORE_RESIZE", raising=False)
    assert FR.resize_default() is False
    monkeypatch.setenv("GAA_FRAME_STORE_RESIZE", "1")
    assert FR.resize_default() is True
    monkeypatch.setenv("GAA_FRAME_STORE_RESIZE", "0")
    assert FR.resize_default() is False


def test_adopted_dataset_holds_resized_cameras_only_under_the_switch(monkeypatch):
    from gaussianavatars_amd import patch

    cams = _cameras()
    monkeypatch.delenv("GAA_FRAME_STORE", raising=False)
    monkeypatch.delenv("GAA_FRAME_STORE_EVAL", raising=False)
    for value, resident in ((None, False), ("1", True)):
        class Scene:
            def getTrainCameras(self, scale=1.0):
                return FC.StandInDataset(cams)

        if value is None:
            monkeypatch.delenv("GAA_FRAME_STORE_RESIZE", raising=False)
        else:
            monkeypatch.setenv("GAA_FRAME_STORE_RESIZE", value)
        assert patch.adopt_frame_store(Scene, device="cpu") == ["Scene.getTrainCameras"]
        ds = Scene().getTrainCameras()
        try:
            assert isinstance(ds[0].original_image, FR.FrameRef)
            assert isinstance(ds[1].original_image, FR.FrameRef) is resident
            assert torch.equal(ds[1].original_image.to("cpu"), FC.reference_getitem(cams[1]).original_image)
        finally:
            FR.release(ds.key)
            patch.unpatch_classes(Scene)


def test_resample_argument_checks_need_no_gpu():
    lib = _lib.gfs()
    p16, p4, p2 = C.c_void_p(4096), C.c_void_p(4100), C.c_void_p(4098)   # (never dereferenced: every call below is refused before it launches)
    err = lambda: lib.gfs_last_error()

    def call(Hin=8, Win=8, src=p16, scap=4, sfirst=0, Hout=4, Wout=4, kx=p4, bx=p4, ksx=9, ky=p4, by=p4, ksy=9, tmp=p16, store=p16, cap=4, first=0, count=2):
        return lib.gfs_resample(Hin, Win, src, scap, sfirst, Hout, Wout, kx, bx, ksx, ky, by, ksy, tmp, store, cap, first, count, None)

    assert call(Hin=0) == -1 and b"bad image shape" in err()
    assert call(Wout=-3) == -1 and b"bad image shape" in err()
    assert call(Hin=1 << 20, Wout=1 << 20) == -1 and b"bad image shape" in err()             # (the image between the passes)
    assert call(Hout=8, Wout=8, kx=None, bx=None, ky=None, by=None) == -1 and b"nothing to resample" in err()
    assert call(src=None) == -1 and b"null pointer" in err()
    assert call(store=None) == -1 and b"null pointer" in err()
    assert call(tmp=None) == -1 and b"null pointer" in err()
    assert call(kx=None) == -1 and b"tables of an axis" in err()
    assert call(by=None) == -1 and b"tables of an axis" in err()
    assert call(Wout=8) == -1 and b"tables of an axis" in err()                              # a table for an axis that does not change
    assert call(ksx=0) == -1 and b"ksize must be positive" in err()
    assert call(ksy=-1) == -1 and b"ksize must be positive" in err()
    assert call(count=0) == -1 and b"count must be" in err()
    assert call(count=_lib.GFS_MAX_BATCH + 1, scap=1 << 20, cap=1 << 20) == -1 and b"count must be" in err()
    assert call(sfirst=3) == _lib.GFS_E_RANGE and b"source frames [3, 5) outside a store of 4" in err()
    assert call(sfirst=-1) == _lib.GFS_E_RANGE
    assert call(first=3) == _lib.GFS_E_RANGE and b"frames [3, 5) outside a store of 4" in err()
    assert call(cap=0) == _lib.GFS_E_RANGE
    assert call(src=p4) == -1 and b"16-byte aligned" in err()
    assert call(store=p4) == -1 and b"16-byte aligned" in err()
    assert call(tmp=p4) == -1 and b"16-byte aligned" in err()
    assert call(kx=p2) == -1 and b"4-byte aligned" in err()
    assert call(by=p2) == -1 and b"4-byte aligned" in err()
    # the staging size: `count` frames of the (Hin, Wout) stride
    assert lib.gfs_resample_tmp_bytes(7, 5, 3) == 3 * FR.frame_stride(7, 5) and lib.gfs_resample_tmp_bytes(2200, 802, 32) == 32 * FR.frame_stride(2200, 802)
    assert lib.gfs_resample_tmp_bytes(0, 5, 3) == 0 and lib.gfs_resample_tmp_bytes(7, 5, 0) == 0
