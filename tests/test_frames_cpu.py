"""CPU tests of the resident frame store (include/gfs.h, gaussianavatars_amd/frames.py): the host restatement against
tests/golden/frame_pins.npz (the reference's own composited bytes and floats, exactly), the placeholder across pickle and DataLoader workers,
the dataset against the reference's (order under shuffle, fall-through of frames the store does not hold), the adoption on the reference's
Scene, and the ninth library's description against its header.  Nothing here launches.

Inputs and stand-ins: tests/frame_cases.py."""
import ctypes as C
import os
import pickle
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from gaussianavatars_amd import _lib
from gaussianavatars_amd import frames as FR

import frame_cases as FC

ROOT = FC.ROOT
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "scene")), reason="reference checkout not present on this box")
PINS = FC.pins()


# ---- the constants _lib.py mirrors and the stride rule (names, ABI and load failures: tests/test_lib_loader_cpu.py) ------------------------
def test_description_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "gfs.h")).read()
    lib = _lib.gfs()
    mirrored = 0
    for name, value in re.findall(r"#define\s+(GFS_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", txt):   # the constants _lib.py mirrors
        if hasattr(_lib, name):
            assert getattr(_lib, name) == int(value), name
            mirrored += 1
    assert mirrored >= 5
    for hw in FC.FETCH_SIZES + ((550, 802), (1, 4), (1, 5)):   # the stride rule, on both sides of the ABI
        s = lib.gfs_frame_stride(*hw)
        assert s == FR.frame_stride(*hw) and s % 16 == 0 and s >= 12 * ((hw[0] * hw[1] + 3) // 4) and s - 16 < 12 * ((hw[0] * hw[1] + 3) // 4)
    assert lib.gfs_frame_stride(0, 4) == 0


def test_argument_checks_need_no_gpu():
    lib = _lib.gfs()
    p16, p4, p8 = C.c_void_p(4096), C.c_void_p(4100), C.c_void_p(4104)   # (never dereferenced: every call below is refused before it launches)
    bg = (C.c_double * 3)(0, 0, 0)
    err = lambda: lib.gfs_last_error()
    assert lib.gfs_compose(0, 4, p16, bg, p16, 1, 0, 1, None) == -1 and b"bad image shape" in err()
    assert lib.gfs_compose(2, 2, None, bg, p16, 1, 0, 1, None) == -1 and b"null pointer" in err()
    assert lib.gfs_compose(2, 2, p16, bg, p16, 4, 3, 2, None) == _lib.GFS_E_RANGE and b"outside a store of 4" in err()
    assert lib.gfs_compose(2, 2, p16, bg, p16, 4, -1, 1, None) == _lib.GFS_E_RANGE
    assert lib.gfs_compose(2, 2, p16, bg, p16, 4, 0, 0, None) == -1 and b"count must be" in err()
    assert lib.gfs_compose(2, 2, p16, bg, p4, 4, 0, 1, None) == -1 and b"16-byte aligned" in err()
    assert lib.gfs_fetch(2, 2, p16, 3, 3, p16, p16, None) == _lib.GFS_E_RANGE and b"outside [0, 3)" in err()
    assert lib.gfs_fetch(2, 2, p16, 3, -1, p16, p16, None) == _lib.GFS_E_RANGE
    assert lib.gfs_fetch(2, 2, p4, 3, 0, p16, p16, None) == -1 and b"16-byte aligned" in err()
    assert lib.gfs_fetch(2, 2, p16, 0, 0, p16, p16, None) == -1 and b"count must be positive" in err()
    assert lib.gfs_fetch(2, 2, p16, 3, 0, None, p16, None) == -1 and b"null pointer" in err()
    assert lib.gfs_fetch_indexed(2, 2, p16, 3, None, p16, p16, p16, None) == -1 and b"null pointer" in err()
    assert lib.gfs_fetch_indexed(2, 2, p16, 3, p4, p16, p16, p16, None) == -1 and b"8-byte aligned" in err()
    assert lib.gfs_fetch_batch(2, 2, p16, 3, p8, 0, p16, p16, p16, None) == -1 and b"K must be" in err()
    assert lib.gfs_fetch_batch(2, 2, p16, 3, p8, _lib.GFS_MAX_BATCH + 1, p16, p16, p16, None) == -1
    assert lib.gfs_fetch_batch(2, 2, p16, 3, p8, 2, p16, p16, None, None) == -1 and b"null pointer" in err()


def test_bare_import_maps_no_frame_library():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gaussianavatars_amd\n"
            "from gaussianavatars_amd import _lib\n"
            "import gaussianavatars_amd.frames, gaussianavatars_amd.patch, gaussianavatars_amd.gaussian_renderer\n"
            "print('MAPPED', 'libgfs_hip.so' in open('/proc/self/maps').read())\n"
            "print('LOADED', _lib.gfs() is not None and 'libgfs_hip.so' in open('/proc/self/maps').read())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "MAPPED False" in r.stdout and "LOADED True" in r.stdout, r.stdout


# ---- the host restatement against the pins ---------------------------------------------------------------------------------------------------
def test_pins_file_is_small_and_complete():
    assert os.path.getsize(FC.PINS_PATH) < 256 * 1024
    assert PINS["table"].dtype == np.float32 and PINS["table"].shape == (256,)
    for k in range(3):
        assert PINS[f"all_{k}_rgb"].shape == (256, 256, 3) and PINS[f"all_{k}_rgb"].dtype == np.uint8
        assert PINS[f"rand{k}_rgb"].shape == (*FC.SIZES[k], 3) and PINS[f"rand{k}_image"].shape == (3, *FC.SIZES[k])
    assert all(PINS[k].dtype.kind in "fu" for k in PINS.files)


def test_byte_table_is_the_references():
    t = FR.byte_table()
    assert t.dtype is torch.float32 and np.array_equal(t.numpy(), PINS["table"])


@pytest.mark.parametrize("k", range(3))
def test_composed_composite_equals_the_pins_for_every_colour_alpha_pair(k):
    got = FR.compose_composed(torch.from_numpy(FC.all_pairs_rgba()), FC.BACKGROUNDS[k])
    assert got.dtype is torch.uint8 and np.array_equal(got.numpy(), PINS[f"all_{k}_rgb"])


def test_host_store_holds_the_pinned_bytes_and_returns_the_pinned_images():
    cams = [FC.stand_in_camera(FC.random_rgba(k), FC.RAND_BGS[k], seed=k) for k in range(3)]
    store = FR.FrameStore.from_cameras(cams, "cpu")
    try:
        assert len(store) == 3 and all(store.resident(i) for i in range(3)) and len(store.groups) == 3
        assert store.bytes == sum(FR.frame_stride(*hw) for hw in FC.SIZES)
        for k in range(3):
            assert np.array_equal(store.rgb(k).numpy(), PINS[f"rand{k}_rgb"])
            img = store.image(k)
            assert img.dtype is torch.float32 and img.is_contiguous() and np.array_equal(img.numpy(), PINS[f"rand{k}_image"])
            wv, fp, cc = store.camera(k)
            assert torch.equal(wv, cams[k].world_view_transform) and torch.equal(fp, cams[k].full_proj_transform) and torch.equal(cc, cams[k].camera_center)
            assert wv.is_contiguous() and fp.is_contiguous() and wv.dtype is torch.float32
        with pytest.raises(IndexError):
            store.image(3)
    finally:
        store.release()


def test_an_image_read_from_a_file_is_the_same_frame(tmp_path):
    from PIL import Image

    path = str(tmp_path / "f.png")
    Image.fromarray(FC.random_rgba(1), "RGBA").save(path)
    store = FR.FrameStore.from_cameras([FC.stand_in_camera(None, FC.RAND_BGS[1], path=path, width=9, height=7)], "cpu")
    try:
        assert np.array_equal(store.image(0).numpy(), PINS["rand1_image"])
    finally:
        store.release()


# ---- the placeholder ---------------------------------------------------------------------------------------------------------------------------
class _Refs(torch.utils.data.Dataset):
    """Yields the FrameRefs themselves; item 100 + i instead tries to materialise ref i INSIDE the worker and reports what happened."""

    def __init__(self, refs):
        self.refs = refs

    def __len__(self):
        return len(self.refs)

    def __getitem__(self, i):
        return self.refs[i]


class _Probe(_Refs):
    def __getitem__(self, i):
        try:
            self.refs[i].to("cpu")
        except RuntimeError as e:
            return f"{os.getpid()} RuntimeError {e}"
        return f"{os.getpid()} materialised"


def test_frameref_survives_pickle_and_worker_queues_and_materialises_in_the_parent():
    cams = [FC.stand_in_camera(FC.random_rgba(k), FC.RAND_BGS[k], seed=k) for k in range(3)]
    store = FR.FrameStore.from_cameras(cams, "cpu")
    try:
        refs = [store.ref(k) for k in range(3)]
        r = pickle.loads(pickle.dumps(refs[1]))
        assert isinstance(r, FR.FrameRef) and (r.key, r.index, r.shape, r.dtype, r.device) == (store.key, 1, torch.Size((3, 7, 9)), torch.float32, torch.device("cpu"))
        assert len(pickle.dumps(refs[1])) < 200                          # no tensor inside
        assert r.pin_memory() is r and r.dim() == 3 and r.size(1) == 7
        got = list(DataLoader(_Refs(refs), batch_size=None, num_workers=2))
        assert [type(g) for g in got] == [FR.FrameRef] * 3 and [g.index for g in got] == [0, 1, 2]
        for k, g in enumerate(got):
            assert np.array_equal(g.to("cpu").numpy(), PINS[f"rand{k}_image"])
            assert np.array_equal(g[0:3, :, :].numpy(), PINS[f"rand{k}_image"]) and np.array_equal(g[1].numpy(), PINS[f"rand{k}_image"][1])
            assert float(g.max()) == float(PINS[f"rand{k}_image"].max())      # anything else is the fetched tensor's
            assert g.to("cpu") is not g.to("cpu")                                 # a fresh tensor every time: the caller may write to it
        # a forked worker inherits the registry's dictionary and still may not use it
        said = list(DataLoader(_Probe(refs), batch_size=None, num_workers=2))
        assert all(int(s.split()[0]) != os.getpid() and "RuntimeError" in s and "is not held by this process" in s for s in said), said
    finally:
        store.release()


def test_materialising_without_a_store_raises_the_documented_error():
    ref = FR.FrameRef("no-such-store", 0, (3, 2, 2), "cpu")
    for act in (lambda: ref.cuda(), lambda: ref.to("cpu"), lambda: ref[0], lambda: ref.mean()):
        with pytest.raises(RuntimeError, match="is not held by this process .* only in the process that built its FrameStore"):
            act()
    assert ref.shape == (3, 2, 2) and ref.dtype is torch.float32      # these never fetch
    with pytest.raises(AttributeError):
        ref.__deepcopy__


# ---- the dataset -----------------------------------------------------------------------------------------------------------------------------
def _seven_cameras():
    g = np.random.default_rng(3)
    return [FC.stand_in_camera(g.integers(0, 256, (7, 9, 4), dtype=np.uint8), FC.BACKGROUNDS[i % 3], seed=i) for i in range(7)]


def test_shuffled_loader_yields_the_reference_datasets_order_and_int_and_slice_indexing_match():
    cams = _seven_cameras()
    ref_ds = FC.StandInDataset(cams)
    store = FR.FrameStore.from_cameras(cams, "cpu")
    try:
        ds = FR.ResidentCameraDataset(cams, store, fallback=ref_ds)
        assert len(ds) == len(ref_ds) == 7
        torch.manual_seed(31)
        a = [c.uid for c in DataLoader(ds, shuffle=True, batch_size=None)]
        torch.manual_seed(31)
        b = [c.uid for c in DataLoader(ref_ds, shuffle=True, batch_size=None)]
        assert a == b and sorted(a) == list(range(7)) and a != list(range(7))
        for i in (0, 3, 6, -1):
            c, r = ds[i], ref_ds[i]
            assert c is not cams[i] and c.uid == r.uid and c._gaa_frame == (store.key, i % 7) and not hasattr(cams[i], "_gaa_frame")
            assert isinstance(c.original_image, FR.FrameRef) and torch.equal(c.original_image.to("cpu"), r.original_image)
        sub = ds[2:5]
        assert isinstance(sub, FR.ResidentCameraDataset) and len(sub) == 3 and [sub[j].uid for j in range(3)] == [2, 3, 4]
        assert sub[1]._gaa_frame == (store.key, 3) and torch.equal(sub[1].original_image.to("cpu"), ref_ds[3].original_image)
        assert [c.uid for c in ds[::3]] == [0, 3, 6] and ds[::3][1]._gaa_frame == (store.key, 3)
        with pytest.raises(TypeError):
            ds["0"]
        got = list(DataLoader(ds, batch_size=None, num_workers=2, pin_memory=False))      # cameras cross the worker queue with their placeholder
        assert [c._gaa_frame[1] for c in got] == list(range(7)) and torch.equal(got[5].original_image.to("cpu"), ref_ds[5].original_image)
    finally:
        store.release()


def test_budget_overflow_and_size_mismatch_fall_through_to_the_fallbacks_getitem():
    cams = _seven_cameras()
    cams[1].image_width, cams[1].image_height = 5, 4           # asks for a resize: PIL's resampling is not restated
    cams[2].bg = np.array([1.0, 1.0])                          # not three numbers
    cams[3].camera_center = cams[3].camera_center.double()     # not what the renderer would upload as it is
    stride = FR.frame_stride(7, 9)
    store = FR.FrameStore.from_cameras(cams, "cpu", budget_bytes=3 * stride + stride // 2)
    try:
        assert [store.resident(i) for i in range(7)] == [True, False, False, False, True, True, False] and store.bytes == 3 * stride
        calls = []

        class Fallback(FC.StandInDataset):
            def __getitem__(self, idx):
                calls.append(idx)
                if idx == 2:
                    return "the fallback's own business"
                return super().__getitem__(idx)

        ds = FR.ResidentCameraDataset(cams, store, fallback=Fallback(cams))
        for i in (0, 4, 5):
            assert isinstance(ds[i].original_image, FR.FrameRef)
        assert calls == []
        small = ds[1]
        assert calls == [1] and isinstance(small.original_image, torch.Tensor) and small.original_image.shape == (3, 4, 5) and not hasattr(small, "_gaa_frame")
        assert ds[2] == "the fallback's own business"
        over = ds[6]
        assert calls == [1, 2, 6] and isinstance(over.original_image, torch.Tensor) and not hasattr(over, "_gaa_frame")
        assert torch.equal(over.original_image, FC.reference_getitem(cams[6]).original_image)
        with pytest.raises(IndexError):
            store.camera(6)
        assert FR.resident_camera(over, torch.device("cpu")) is None and FR.resident_camera(ds[4], torch.device("cpu")) is not None
        assert FR.resident_camera(ds[4], torch.device("cuda", 0)) is None            # a store on another device: the camera's own tensors go up
    finally:
        store.release()
    assert FR.resident_camera(ds[4], torch.device("cpu")) is None                     # and a released store


def test_default_budget_reads_the_variable_and_says_what_it_is(monkeypatch):
    monkeypatch.setenv("GAA_FRAME_STORE_GB", "0.5")
    assert FR.default_budget(torch.device("cpu")) == 1 << 29 and FR.default_budget(torch.device("cuda", 0)) == 1 << 29
    monkeypatch.delenv("GAA_FRAME_STORE_GB")
    assert FR.default_budget(torch.device("cpu")) is None
    assert "policy" in FR.default_budget.__doc__ and "not a measurement" in FR.default_budget.__doc__
    assert FR.MAX_DECODE_THREADS == 16


# ---- adoption ---------------------------------------------------------------------------------------------------------------------------------
def test_adopt_frame_store_wraps_is_idempotent_honours_the_switches_and_is_undone(monkeypatch):
    from gaussianavatars_amd import patch

    cams = _seven_cameras()

    def make():
        class Scene:
            def getTrainCameras(self, scale=1.0):
                return FC.StandInDataset(cams)

            def getValCameras(self, scale=1.0):
                return FC.StandInDataset(cams[:2])

            def getTestCameras(self, scale=1.0):
                return FC.StandInDataset(cams[2:4])
        return Scene

    S = make()
    orig = S.__dict__["getTrainCameras"]
    monkeypatch.delenv("GAA_FRAME_STORE", raising=False)
    monkeypatch.delenv("GAA_FRAME_STORE_EVAL", raising=False)
    assert patch.adopt_frame_store(S, device="cpu") == ["Scene.getTrainCameras"] and patch.adopt_frame_store(S, device="cpu") == []
    sc = S()
    ds = sc.getTrainCameras()
    assert isinstance(ds, FR.ResidentCameraDataset) and isinstance(ds[0].original_image, FR.FrameRef) and isinstance(ds.fallback, FC.StandInDataset)
    assert sc.getTrainCameras().key == ds.key and len(sc._gaa_frame_stores) == 1              # one store per Scene, built once
    assert isinstance(sc.getValCameras(), FC.StandInDataset)
    monkeypatch.setenv("GAA_FRAME_STORE", "0")
    assert isinstance(sc.getTrainCameras(), FC.StandInDataset)                                # read at every call
    monkeypatch.delenv("GAA_FRAME_STORE")
    FR.release(ds.key)
    patch.unpatch_classes(S)
    assert S.__dict__["getTrainCameras"] is orig and not hasattr(S, "_gaa_patched_frames") and (S, "getTrainCameras") not in patch._ORIG
    S2 = make()
    monkeypatch.setenv("GAA_FRAME_STORE_EVAL", "1")
    assert patch.adopt_frame_store(S2, device="cpu") == ["Scene.getTrainCameras", "Scene.getValCameras", "Scene.getTestCameras"]
    sc2 = S2()
    val = sc2.getValCameras()
    assert isinstance(val, FR.ResidentCameraDataset) and len(val) == 2 and val.key != sc2.getTestCameras().key
    for _, store in sc2._gaa_frame_stores.values():
        store.release()
    patch.unpatch_classes(S2)


def test_patch_reference_reports_frames_and_gaa_frame_store_0_opts_out():
    import inspect

    from gaussianavatars_amd import patch

    src = inspect.getsource(patch.patch_reference)
    assert 'adopt_frame_store() if os.environ.get("GAA_FRAME_STORE", "1") != "0" else []' in src and "frames=frames" in src


@needs_ref
def test_adopted_reference_scene_gives_the_unadopted_images_bit_for_bit(tmp_path):
    from gaussianavatars_amd import synthetic as S

    data, model = str(tmp_path / "data"), str(tmp_path / "model")
    os.makedirs(model)
    info = S.write_reference_dataset(data, os.path.join(REF, "flame_model", "assets", "flame", "head_template_mesh.obj"), n_timesteps=3, width=45, height=37)
    code = textwrap.dedent(f"""
        import types
        import torch
        from torch.utils.data import DataLoader
        from gaussianavatars_amd import frames, patch
        info = patch.patch_reference(pin=False)
        assert info["frames"] == ["Scene.getTrainCameras"], info["frames"]
        import scene
        g = types.SimpleNamespace(binding=True, load_meshes=lambda *a, **k: None, create_from_pcd=lambda *a, **k: None)
        args = types.SimpleNamespace(model_path={model!r}, source_path={data!r}, white_background=True, eval=True, target_path="", images="images",
                                     resolution=-1, select_camera_id=-1, data_device="cpu")
        sc = scene.Scene(args, g, shuffle=False)
        ds = sc.getTrainCameras()
        assert isinstance(ds, frames.ResidentCameraDataset) and len(ds) == {info["train"]} and sc.getTrainCameras().key == ds.key
        assert type(sc.getValCameras()) is scene.CameraDataset                      # evaluation splits: only under GAA_FRAME_STORE_EVAL=1
        store = frames.lookup(ds.key)
        assert all(store.resident(i) for i in range(len(ds)))
        orig = patch._ORIG[(scene.Scene, "getTrainCameras")](sc)
        assert type(orig) is scene.CameraDataset
        covered = 0
        for i in range(len(ds)):
            a, b = ds[i], orig[i]
            assert isinstance(a.original_image, frames.FrameRef) and a._gaa_frame == (ds.key, i) and a.image_name == b.image_name
            t = a.original_image.to("cpu")
            assert t.dtype == b.original_image.dtype and t.shape == b.original_image.shape == (3, 37, 45) and torch.equal(t, b.original_image)
            covered += int((t < 1).any())
            for x, y in zip(store.camera(i), (b.world_view_transform, b.full_proj_transform, b.camera_center)):
                assert x.dtype == y.dtype and torch.equal(x, y)
        assert covered == len(ds)                                                   # (not blank frames)
        torch.manual_seed(11); o1 = [c.uid for c in DataLoader(ds, shuffle=True, batch_size=None)]
        torch.manual_seed(11); o2 = [c.uid for c in DataLoader(orig, shuffle=True, batch_size=None)]
        assert o1 == o2 and sorted(o1) == list(range(len(ds)))
        got = list(DataLoader(ds, batch_size=None, num_workers=2))
        assert all(torch.equal(c.original_image.to("cpu"), orig[i].original_image) for i, c in enumerate(got))
        patch.unpatch_classes(scene.Scene)
        assert type(sc.getTrainCameras()) is scene.CameraDataset and not hasattr(scene.Scene, "_gaa_patched_frames")
        print("ADOPTED-OK")
    """)
    env = dict(os.environ, PYTHONPATH=ROOT, MPLBACKEND="Agg")
    env.pop("GAA_FRAME_STORE", None)
    env.pop("GAA_FRAME_STORE_EVAL", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=REF, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADOPTED-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
