"""GPU tests of the resident frame store (include/gfs.h, gaussianavatars_amd/frames.py) on the MI355X: the composite against the reference's
bytes for every (colour, alpha) pair, the fetch against the reference's floats at every size where it takes another path, the device-indexed
and batched fetches (bounds flag, graph replay), byte offsets past 4 GiB, and a resident camera through the renderer and the loss.

Every comparison is exact (tests/frame_cases.py says why).  No test reads the reference; DataLoaders run with num_workers=0."""
import math

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib
from gaussianavatars_amd import frames as FR

import frame_cases as FC

pytestmark = pytest.mark.gpu
PINS = FC.pins()
TABLE = PINS["table"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _store_of(rgb_frames, dev, capacity=None):
    """A device store with one group holding the given (H,W,3) byte images as frames 0 .. n-1 (of `capacity`), written there as they are."""
    H, W = rgb_frames[0].shape[:2]
    n = len(rgb_frames)
    store = FR.FrameStore(dev)
    g = store.groups[(H, W)] = FR._Group(H, W, capacity or n, dev)
    g.frames.fill_(0xA5)   # (padding that is not zero: nothing may depend on it)
    rows = g.frames.view(g.capacity, g.stride)
    for i, f in enumerate(rgb_frames):
        rows[i, :H * W * 3] = torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).to(dev)
    g.count = n
    store.where = [((H, W), i) for i in range(n)]
    store.cameras = torch.zeros((n, 35), device=dev)
    return store, g


@pytest.fixture(scope="module")
def five_frames(dev):
    """Per FETCH size: five random byte images, a store of them and what the reference makes of each -- built once, never written again."""
    out = {}
    for hw in FC.FETCH_SIZES:
        frames = [FC.random_rgb(hw, 700 + 10 * i + hw[0] * hw[1]) for i in range(5)]
        store, g = _store_of(frames, dev)
        out[hw] = (store, g, [FC.expected_image(f, TABLE) for f in frames])
    yield out
    for store, _, _ in out.values():
        store.release()


# ---- gfs_compose ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3))
def test_compose_equals_the_pins_for_every_colour_alpha_pair(dev, k):
    store = FR.FrameStore(dev)
    try:
        store.groups[(256, 256)] = FR._Group(256, 256, 2, dev)
        store.where = [((256, 256), 0), ((256, 256), 1)]
        rgba = torch.from_numpy(FC.all_pairs_rgba())
        store.ingest((256, 256), 1, rgba[None], FC.BACKGROUNDS[k])            # frame 1 alone ...
        store.ingest((256, 256), 0, torch.stack([rgba, rgba.flip(0)]), FC.BACKGROUNDS[k])   # ... then two frames in one launch, over it
        want = PINS[f"all_{k}_rgb"]
        assert np.array_equal(store.rgb(0).cpu().numpy(), want) and np.array_equal(store.rgb(1).cpu().numpy(), want[::-1])
        assert np.array_equal(FR.compose_composed(rgba.to(dev), FC.BACKGROUNDS[k]).cpu().numpy(), want)    # the composed path on the device: the same bytes
    finally:
        store.release()


def test_store_from_cameras_of_odd_sizes_equals_the_pins_bytes_and_floats(dev, monkeypatch):
    cams = [FC.stand_in_camera(FC.random_rgba(k), FC.RAND_BGS[k], seed=k) for k in range(3)]
    cams += [FC.stand_in_camera(FC.random_rgba(1), FC.RAND_BGS[1], seed=7)]        # a second frame of the (7,9) group
    store = FR.FrameStore.from_cameras(cams, dev)
    try:
        assert store.device == dev and all(store.resident(i) for i in range(4)) and store.groups[(7, 9)].capacity == 2
        for i, k in enumerate((0, 1, 2, 1)):
            assert np.array_equal(store.rgb(i).cpu().numpy(), PINS[f"rand{k}_rgb"])
            img = store.image(i)
            assert img.is_cuda and img.dtype is torch.float32 and np.array_equal(img.cpu().numpy(), PINS[f"rand{k}_image"])
            ref = store.ref(i)
            assert torch.equal(ref.cuda(), img) and torch.equal(ref.to("cuda"), img) and torch.equal(ref[0:3, :, :], img) and ref.device == dev
            for got, want in zip(store.camera(i), (cams[i].world_view_transform, cams[i].full_proj_transform, cams[i].camera_center)):
                assert got.is_contiguous() and torch.equal(got.cpu(), want)
        # the pad bytes of a frame's last group of four are zeros (3*5 = 15 pixels: one pad pixel)
        g = store.groups[(3, 5)]
        assert g.frames.view(g.capacity, g.stride)[0, 45:48].tolist() == [0, 0, 0]
        monkeypatch.setenv("GAA_FRAME_STORE", "0")                                   # the composed path on the device: the same floats
        assert np.array_equal(store.image(1).cpu().numpy(), PINS["rand1_image"])
    finally:
        store.release()


# ---- gfs_fetch --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", FC.FETCH_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_fetch_equals_table_of_bytes_first_middle_last_and_writes_nothing_else(dev, five_frames, hw):
    store, g, want = five_frames[hw]
    n = 3 * hw[0] * hw[1]
    for i in (0, 2, 4):
        got = store.image(i)
        assert got.shape == (3, *hw) and np.array_equal(got.cpu().numpy(), want[i])
        # into the middle of a poisoned buffer, at a 16-byte and at a 4-byte aligned address: the floats before and behind stay
        for lead in (4, 1):
            buf = torch.full((n + 8,), float("nan"), device=dev)
            out = buf[lead:lead + n]
            rc = _lib.gfs().gfs_fetch(hw[0], hw[1], g.frames.data_ptr(), g.capacity, i, store.table.data_ptr(), out.data_ptr(), _lib.raw_stream(dev))
            assert rc == 0, _lib.gfs_error()
            assert np.array_equal(out.cpu().numpy().reshape(3, *hw), want[i])
            assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all())
    with pytest.raises(IndexError):
        store.image(5)
    assert _lib.gfs().gfs_fetch(hw[0], hw[1], g.frames.data_ptr(), g.capacity, 5, store.table.data_ptr(), got.data_ptr(), None) == _lib.GFS_E_RANGE


# ---- gfs_fetch_indexed ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(7, 9), (17, 64)], ids=["7x9", "17x64"])
def test_fetch_indexed_equals_fetch_flags_a_bad_index_and_replays_in_a_graph(dev, five_frames, hw):
    store, g, want = five_frames[hw]
    slot = torch.zeros(1, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty((3, *hw), device=dev)
    for i in (0, 1, 3, 4):
        slot.fill_(i)
        out.fill_(float("nan"))
        FR.fetch_indexed(store, hw, slot, out, flag)
        assert np.array_equal(out.cpu().numpy(), want[i]) and torch.equal(out, store.image(i))
    assert int(flag) == 0
    for bad in (5, -1, 1 << 40):
        slot.fill_(bad)
        out.fill_(float("nan"))
        flag.zero_()
        FR.fetch_indexed(store, hw, slot, out, flag)
        assert bool(torch.isnan(out).all()) and int(flag) == _lib.GFS_FLAG_RANGE, bad
    # one capture, three replays with the index changed on the device in between (a single-branch graph)
    flag.zero_()
    slot.fill_(2)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        FR.fetch_indexed(store, hw, slot, out, flag)   # (warm: the library is mapped, the code object loaded)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        FR.fetch_indexed(store, hw, slot, out, flag)
    for i in (4, 0, 3):
        slot.fill_(i)
        out.fill_(float("nan"))
        graph.replay()
        assert np.array_equal(out.cpu().numpy(), want[i]), i
    assert int(flag) == 0
    with pytest.raises(ValueError):
        FR.fetch_indexed(store, hw, slot.int(), out, flag)


# ---- gfs_fetch_batch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("hw", [(3, 5), (17, 64)], ids=["3x5", "17x64"])
def test_fetch_batch_equals_k_single_fetches(dev, five_frames, hw, K):
    store, g, want = five_frames[hw]
    order = [4, 0, 2, 2, 1][:K]
    slots = torch.tensor(order, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = FR.fetch_batch(store, hw, slots, flag)
    assert got.shape == (K, 3, *hw) and int(flag) == 0
    for j, i in enumerate(order):
        assert torch.equal(got[j], store.image(i)) and np.array_equal(got[j].cpu().numpy(), want[i])
    if K > 1:   # one index outside the store: its image stays as it was, the others arrive, the flag says so
        bad = slots.clone()
        bad[1] = 5
        out = torch.full((K, 3, *hw), float("nan"), device=dev)
        FR.fetch_batch(store, hw, bad, flag, out=out)
        assert int(flag) == _lib.GFS_FLAG_RANGE and bool(torch.isnan(out[1]).all())
        assert all(np.array_equal(out[j].cpu().numpy(), want[order[j]]) for j in range(K) if j != 1)


# ---- offsets beyond 2^32 bytes ----------------------------------------------------------------------------------------------------------------
def test_a_frame_that_starts_past_4_gib_is_composited_and_fetched(dev):
    if torch.cuda.mem_get_info(dev)[0] < 6 << 30:
        pytest.skip("needs 6 GiB of free device memory")
    hw = (16, 16)
    stride = FR.frame_stride(*hw)
    n = (1 << 32) // stride + 2
    last = n - 1
    assert last * stride > 1 << 32
    store = FR.FrameStore(dev)
    try:
        g = store.groups[hw] = FR._Group(hw[0], hw[1], n, dev)        # uninitialised: only the last frame is ever written
        store.where = [(hw, last)]                                     # camera 0 -> the last slot
        rgb = FC.random_rgb(hw, 41)
        g.frames[last * stride:last * stride + rgb.size] = torch.from_numpy(rgb.reshape(-1)).to(dev)
        want = FC.expected_image(rgb, TABLE)
        assert np.array_equal(store.image(0).cpu().numpy(), want)                                   # by host index
        slot = torch.tensor([last], dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.full((3, *hw), float("nan"), device=dev)
        FR.fetch_indexed(store, hw, slot, out, flag)                                               # by device index
        assert np.array_equal(out.cpu().numpy(), want) and int(flag) == 0
        assert np.array_equal(FR.fetch_batch(store, hw, slot, flag)[0].cpu().numpy(), want) and int(flag) == 0
        g2 = np.random.default_rng(43)
        rgba = torch.from_numpy(g2.integers(0, 256, (1, *hw, 4), dtype=np.uint8))
        store.ingest(hw, last, rgba, FC.BACKGROUNDS[2])                                            # the composite's store offset, too
        assert torch.equal(store.rgb(0).cpu(), FR.compose_composed(rgba[0], FC.BACKGROUNDS[2]))
        assert int(g.frames[(last - 1) * stride:last * stride].to(torch.int64).sum()) >= 0         # (the frame before it is still addressable)
    finally:
        store.release()
        del g, store
        torch.cuda.empty_cache()


# ---- a resident camera through the renderer and the loss --------------------------------------------------------------------------------------
class _Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def test_tagged_camera_renders_the_same_frame_and_the_loss_sees_the_same_ground_truth(dev):
    from gaussianavatars_amd import loss as L
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.gaussian_model import GaussianModel
    from gaussianavatars_amd.gaussian_renderer import render

    sp = S.random_splats(3000, 3, 31, xyz_sigma=0.05, log_scale_mean=math.log(0.004))
    op = np.clip(sp["opacities"], 1e-6, 1 - 1e-6)
    model = GaussianModel(3)
    model.load_arrays(dict(_xyz=sp["means3D"], _scaling=np.log(sp["scales"]), _rotation=sp["rotations"], _opacity=np.log(op / (1 - op)),
                           _features_dc=sp["shs"][:, :1], _features_rest=sp["shs"][:, 1:]), device=dev, requires_grad=True)
    H, W = 45, 37                                                        # H*W mod 4 = 1: the unaligned planes, through the loss kernels too
    cams = []
    for i, yaw in enumerate((15.0, -20.0)):
        c = S.orbit_camera(W, H, yaw_deg=yaw, pitch_deg=-8)
        cam = FC.stand_in_camera(np.random.default_rng(60 + i).integers(0, 256, (H, W, 4), dtype=np.uint8), FC.BACKGROUNDS[2], seed=i)
        cam.world_view_transform = torch.as_tensor(c.world_view_transform.T.copy()).transpose(0, 1)     # host, fp32, transposed views: as scene/cameras.py:44-46
        cam.full_proj_transform = torch.as_tensor(c.full_proj_transform.T.copy()).transpose(0, 1)
        cam.camera_center = torch.as_tensor(c.camera_center)
        cam.FoVx, cam.FoVy = c.FoVx, c.FoVy
        assert torch.equal(cam.world_view_transform, torch.as_tensor(c.world_view_transform))
        cams.append(cam)
    fallback = FC.StandInDataset(cams)
    store = FR.FrameStore.from_cameras(cams, dev)
    try:
        ds = FR.ResidentCameraDataset(cams, store, fallback=fallback)
        bg = torch.tensor([0.3, 0.55, 0.9], device=dev)
        for i, tagged in enumerate(torch.utils.data.DataLoader(ds, batch_size=None, num_workers=0)):
            plain = fallback[i]                                                              # the same camera, untagged, with a host ground truth
            assert tagged._gaa_frame == (store.key, i) and not hasattr(plain, "_gaa_frame")
            hit = FR.resident_camera(tagged, dev)
            assert hit is not None and hit[0].data_ptr() == store.cameras[i].data_ptr() and FR.resident_camera(plain, dev) is None
            with torch.no_grad():
                a, b = render(tagged, model, _Pipe, bg), render(plain, model, _Pipe, bg)
            assert int((a["radii"] > 0).sum()) > 500
            assert torch.equal(a["render"], b["render"]) and torch.equal(a["radii"], b["radii"]) and torch.equal(a["visibility_filter"], b["visibility_filter"])
            gt_a, gt_b = tagged.original_image.cuda(), plain.original_image.cuda()          # train.py:128 on both
            assert torch.equal(gt_a, gt_b)
            la, lb = L.l1_ssim(a["render"], gt_a), L.l1_ssim(b["render"], gt_b.contiguous())
            assert la[0].item() == lb[0].item() and la[1].item() == lb[1].item() and 0 < la[0].item() < 1
    finally:
        store.release()
