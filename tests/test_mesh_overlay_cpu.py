"""CPU tests of the shaded mesh overlay (gaussianavatars_amd.mesh_renderer, include/gmr_overlay.h): the pins file, every argument check on
host tensors, the render-size rule, the topology cache, the C ABI of ABI 2, and the adoption by patch_reference() with its opt-out."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import mesh_overlay_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = os.path.join(ROOT, "tests", "golden", "mesh_overlay_pins.npz")
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "mesh_renderer")), reason="reference checkout not present on this box")


# ---- the pins ------------------------------------------------------------------------------------------------------------------------
def test_pins_hold_every_case_with_its_keys():
    assert os.path.getsize(PINS) < 1 << 20
    P = np.load(PINS)
    names = [str(n) for n in P["names"]]
    assert names == [c[0] for c in OC.case_table()] and len(names) == 17
    combos = set()
    for name, mesh, s, light, colors, image_bg, through in OC.case_table():
        W, H = (int(v) for v in P[name + "/size"])
        assert (W, H) == OC.SIZES[s]
        verts, faces = OC.MESHES[mesh]()
        assert np.array_equal(P[name + "/verts"], verts) and np.array_equal(P[name + "/faces"], faces)
        assert P[name + "/world_view_transform"].shape == (4, 4) and P[name + "/full_proj_transform"].shape == (4, 4)
        for k, c in (("albedo", 3), ("normal", 3), ("diffuse", 3), ("rgba", 4)):
            a = P[name + "/" + k]
            assert a.shape == (1, H, W, c) and a.dtype == np.float32 and np.isfinite(a).all(), (name, k)
        amb = P[name + "/amb"]
        assert amb.shape == OC.render_hw(W, H) and amb.dtype == bool
        assert OC.excluded(amb, H, W).mean() <= 1e-3, name     # the reference alone: at most 0.1 % of an image is left out
        alpha = P[name + "/rgba"][0, ..., 3]
        assert 0.05 < (alpha > 0.5).mean() and (through or ((alpha > 0) & (alpha < 1)).any()), name   # drawn, and its silhouette is blended
        if not through:
            combos.add((mesh, s, light, colors, image_bg))
    assert len({c[1:] for c in combos}) == 16 and len(combos) == 16   # every (size, lighting, colours, background) once; four per mesh
    v, f = OC.MESHES["cube"]()
    cam = OC.camera(OC.THROUGH, 64, 48)
    w = (np.concatenate([v, np.ones((8, 1), np.float32)], 1) @ cam.full_proj_transform)[:, 3]
    assert (w <= 0).any() and (w > 0).any()


# ---- the size rule -------------------------------------------------------------------------------------------------------------------
def test_render_size_rule():
    from gaussianavatars_amd.mesh_renderer import render_size

    assert render_size(544, 800) == (544, 800)
    assert render_size(550, 802) == (544, 800)
    assert render_size(77, 53) == (72, 48)
    assert render_size(2048, 2048) == (2048, 2048)
    assert render_size(2049, 100) == (2048, 2048) and render_size(100, 4096) == (2048, 2048)
    assert render_size(2047, 2047) == (2040, 2040)
    assert render_size(550, 802, use_opengl=True) == (550, 802) and render_size(4000, 3, use_opengl=True) == (4000, 3)
    for bad in ((7, 100), (100, 5), (0, 10)):
        with pytest.raises(ValueError):
            render_size(*bad)


# ---- argument checks on host tensors ---------------------------------------------------------------------------------------------------
def _ok():
    verts = torch.zeros(1, 4, 3)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    eye = torch.eye(4)[None]
    return dict(verts=verts, faces=faces, RT=eye, full_proj=eye, image_size=(8, 16), background_color=[1.0, 1.0, 1.0], face_colors=None)


def test_render_mesh_argument_checks():
    from gaussianavatars_amd.mesh_renderer import MeshRenderer

    r = MeshRenderer()
    cases = [
        (dict(verts=torch.zeros(1, 4, 4)), r"\(B, V, 3\)"),
        (dict(verts=torch.zeros(4, 3)), "rank 3"),
        (dict(verts=torch.zeros(1, 4, 3, dtype=torch.float64)), "float32"),
        (dict(verts="x"), "torch.Tensor"),
        (dict(faces=torch.zeros(2, 3)), "int32 or int64"),
        (dict(faces=torch.zeros(2, 4, dtype=torch.int64)), r"\(F, 3\)"),
        (dict(faces=torch.tensor([[0, 1, 4]])), "outside"),
        (dict(faces=torch.tensor([[0, -1, 2]])), "outside"),
        (dict(RT=torch.eye(4)), "RT must have rank 3"),
        (dict(RT=torch.zeros(2, 4, 4)), "RT must be"),
        (dict(full_proj=torch.zeros(1, 3, 4)), "full_proj must be"),
        (dict(image_size=(0, 8)), "at least 1"),
        (dict(image_size=5), "image_size"),
        (dict(background_color=[1.0, 1.0]), "three numbers"),
        (dict(background_color="white"), "Unknown background type"),
        (dict(background_color=torch.zeros(1, 8, 8, 3)), "background image"),
        (dict(face_colors=torch.zeros(1, 3, 3)), "face_colors"),
        (dict(), "CUDA"),      # everything else valid: the host tensor is refused last
    ]
    for kw, msg in cases:
        args = _ok()
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            r.render_mesh(**args)
    args = _ok()
    args["RT"] = torch.zeros(1, 3, 4)      # a 3 x 4 world-to-camera matrix is accepted, like the reference pads it
    with pytest.raises(ValueError, match="CUDA"):
        r.render_mesh(**args)


def test_render_from_camera_and_lighting_argument_checks():
    from gaussianavatars_amd import mesh_renderer as M
    from gaussianavatars_amd import synthetic as S

    cam = S.orbit_camera(53, 77)
    a = _ok()
    r = M.MeshRenderer(lighting_type="front")
    with pytest.raises(ValueError, match="CUDA"):
        r.render_from_camera(a["verts"], a["faces"], cam)
    with pytest.raises(ValueError, match="one camera"):
        r.render_from_camera(torch.zeros(2, 4, 3), a["faces"], cam)
    with pytest.raises(ValueError, match="background image"):      # an image background has the render size, not the camera's
        r.render_from_camera(a["verts"], a["faces"], cam, background_color=torch.zeros(1, 77, 53, 3))
    with pytest.raises(ValueError, match="CUDA"):
        r.render_from_camera(a["verts"], a["faces"], cam, background_color=torch.zeros(1, 72, 48, 3))
    with pytest.raises(ValueError, match="at least 8"):
        r.render_from_camera(a["verts"], a["faces"], S.orbit_camera(5, 77))
    with pytest.raises(NotImplementedError, match="Unknown lighting type"):
        M.MeshRenderer(lighting_type="phong")
    r.lighting_type = "phong"
    with pytest.raises(NotImplementedError, match="Unknown lighting type: phong"):
        r.render_mesh(**_ok())


def test_resize_flip_and_compose_argument_checks():
    from gaussianavatars_amd.mesh_renderer import compose_overlay, resize_flip

    for kw, msg in [(dict(image=torch.zeros(8, 8, 3)), "rank 4"), (dict(image=torch.zeros(1, 8, 8, 3).double()), "float32"),
                    (dict(size=(0, 4)), "at least 1"), (dict(size=3), "size"), (dict(image=torch.zeros(1, 8, 8, 0)), "channel"),
                    (dict(), "CUDA")]:
        args = dict(image=torch.zeros(1, 8, 8, 3), size=(9, 9))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            resize_flip(args["image"], args["size"])
    rgba, splat = torch.zeros(8, 6, 4), torch.zeros(3, 8, 6)
    for kw, msg in [(dict(rgba_mesh=torch.zeros(8, 6, 3)), "rgba_mesh must be"), (dict(rgba_mesh=rgba.double()), "float32"),
                    (dict(rgba_mesh=torch.zeros(2, 8, 6, 4)), "rgba_mesh must be"), (dict(splat_image=torch.zeros(3, 6, 8)), "splat_image must be"),
                    (dict(splat_image=torch.zeros(8, 6, 3)), "splat_image must be"), (dict(mesh_opacity="half"), "mesh_opacity"),
                    (dict(), "CUDA"), (dict(splat_image=None, rgba_mesh=rgba[None]), "CUDA")]:
        args = dict(splat_image=splat, rgba_mesh=rgba, mesh_opacity=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            compose_overlay(args["splat_image"], args["rgba_mesh"], args["mesh_opacity"])


# ---- the topology cache ----------------------------------------------------------------------------------------------------------------
def test_topology_cache_hits_on_the_same_tensor_and_misses_on_an_edit_or_another_tensor(monkeypatch):
    from gaussianavatars_amd import mesh_raster
    from gaussianavatars_amd import mesh_renderer as M

    calls = []

    def counted(tri, n):
        calls.append((tri.data_ptr(), n))
        return mesh_raster.edge_neighbours(tri, n)

    monkeypatch.setattr(M, "_build_adjacency", counted)
    M.clear_topology_cache()
    _, faces_np = OC.head200()
    faces = torch.from_numpy(faces_np)
    t0 = M.topology(faces)
    assert len(calls) == 1 and t0.tri.dtype == torch.int32 and (t0.lo, t0.hi) == (0, 104) and t0.faces is faces
    import mesh_ref as R

    assert np.array_equal(t0.neighbours.numpy(), R.edge_neighbours_ref(faces_np))
    assert M.topology(faces) is t0 and M.topology(faces) is t0 and len(calls) == 1           # same tensor: hits
    verts = torch.zeros(1, 105, 3)
    for _ in range(2):                                                                        # and through the public entry: still one build
        with pytest.raises(ValueError, match="CUDA"):
            M.MeshRenderer().render_mesh(verts, faces, torch.eye(4)[None], torch.eye(4)[None], (8, 8))
    assert len(calls) == 1
    faces[0] = faces[0].roll(1)                                                               # in-place edit: a new version misses
    t1 = M.topology(faces)
    assert len(calls) == 2 and t1 is not t0 and np.array_equal(t1.tri.numpy(), faces.numpy())
    clone = faces.clone()                                                                     # another tensor with the same values misses
    t2 = M.topology(clone)
    assert len(calls) == 3 and t2.faces is clone
    assert M.topology(faces) is t1 and len(calls) == 3
    as_int = faces.int()                                                                      # another dtype is another tensor
    assert M.topology(as_int).faces is as_int and len(calls) == 4
    # the entry keeps its tensor alive, so a freed-and-reused address cannot alias a live entry
    key = M._topology_key(clone)
    del clone
    assert M._TOPOLOGY[key].faces.data_ptr() == key[0]
    for i in range(M.TOPOLOGY_CACHE_ENTRIES + 2):                                             # bounded
        M.topology(torch.tensor([[0, 1, 2 + i]]))
    assert len(M._TOPOLOGY) == M.TOPOLOGY_CACHE_ENTRIES
    empty = M.topology(torch.zeros((0, 3), dtype=torch.int64))
    assert empty.tri.shape == (0, 3) and empty.neighbours.shape == (0, 3)
    M.clear_topology_cache()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return txt, sorted(set(re.findall(r"\b(gmr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))))


def test_abi_2_header_description_and_library_agree():
    from gaussianavatars_amd import _lib

    txt, names = _declared("gmr_overlay.h")
    assert names == ["gmr_compose_overlay", "gmr_mesh_prepare", "gmr_mesh_shade", "gmr_resize_flip"]
    assert names == sorted(_lib.GMR_OVERLAY_SYMBOLS)
    main, _ = _declared("gmr.h")
    assert '#include "gmr_overlay.h"' in main
    abi = int(re.search(r"#define\s+GMR_ABI_VERSION\s+(\d+)", main).group(1))
    lib = _lib.gmr()
    assert lib.gmr_abi_version() == _lib.GMR_ABI_VERSION == abi == 2
    for n in names:
        fn = getattr(lib, n)
        res, args = _lib.GMR_OVERLAY_SYMBOLS[n]
        assert fn.restype is res and list(fn.argtypes) == list(args), n
    for macro in ("GMR_LIGHT_CONSTANT", "GMR_LIGHT_FRONT", "GMR_MAT_ROWS", "GMR_MAT_CAMERA", "GMR_MAX_MAPS"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, txt).group(1)) == getattr(_lib, macro), macro
    # a library without the new entries is refused by the loader, whatever version it reports
    with pytest.raises(AttributeError):
        _lib._load(_lib.LIBS["gmr"]._replace(symbols={**_lib.GMR_SYMBOLS, **_lib.GMR_OVERLAY_SYMBOLS, "gmr_no_such_entry": (C.c_int, [])}))
    with pytest.raises(RuntimeError, match="ABI version 2 != 1"):
        _lib._load(_lib.LIBS["gmr"]._replace(abi=1))
    # host-side argument checks of the C entry points (nothing is launched)
    one = C.c_void_p(16)
    err = lambda: lib.gmr_last_error()
    assert lib.gmr_mesh_prepare(1, 3, 1, one, one, one, 5, one, 0, one, one, None) < 0 and b"bad arguments" in err()
    assert lib.gmr_mesh_prepare(1, 3, 1, one, one, one, 3, one, 1, one, one, None) < 0 and b"bad arguments" in err()
    assert lib.gmr_mesh_prepare(1, 3, 1, None, one, one, 4, one, 0, one, one, None) < 0 and b"NULL" in err()
    assert lib.gmr_mesh_prepare(1, 0, 0, None, None, None, 4, None, 0, None, None, None) == 0
    assert lib.gmr_mesh_shade(1, 1, 8, 8, one, one, None, 2, 0.0, 0.0, 0.0, None, one, one, one, one, None) < 0 and b"bad arguments" in err()
    assert lib.gmr_mesh_shade(1, 1, 8, 8, one, None, None, 0, 0.0, 0.0, 0.0, None, one, one, one, one, None) < 0 and b"NULL" in err()
    maps = (_lib.GmrMap * 1)(_lib.GmrMap(16, 32, 3))
    assert lib.gmr_resize_flip(1, 8, 8, 9, 9, 5, maps, None) < 0 and b"bad arguments" in err()
    assert lib.gmr_resize_flip(1, 8, 8, 0, 9, 1, maps, None) < 0 and b"bad arguments" in err()
    maps[0].dst = 16
    assert lib.gmr_resize_flip(1, 8, 8, 9, 9, 1, maps, None) < 0 and b"alias" in err()
    maps[0].C = 0
    assert lib.gmr_resize_flip(1, 8, 8, 9, 9, 1, maps, None) < 0 and b"C=0" in err()
    assert lib.gmr_compose_overlay(8, 8, None, one, 0.5, 0.5, one, one, None) < 0 and b"exactly one" in err()
    assert lib.gmr_compose_overlay(8, 8, None, one, 0.5, 0.5, None, None, None) < 0 and b"exactly one" in err()
    assert lib.gmr_compose_overlay(0, 8, None, one, 0.5, 0.5, one, None, None) < 0 and b"bad arguments" in err()


def test_mesh_renderer_imports_neither_oracle_nor_tests_nor_the_reference():
    txt = open(os.path.join(ROOT, "gaussianavatars_amd", "mesh_renderer.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests|mesh_ref|mesh_cases|mesh_overlay_cases|nvdiffrast|utils|scene)\b", txt, flags=re.M)


# ---- adoption ----------------------------------------------------------------------------------------------------------------------------
def test_adopt_mesh_overlay_rebinds_a_class_and_honours_its_attributes(monkeypatch):
    from gaussianavatars_amd import mesh_renderer as M
    from gaussianavatars_amd import patch

    class Renderer:
        def __init__(self, use_opengl, lighting_type):
            self.use_opengl, self.lighting_type = use_opengl, lighting_type

        def render_mesh(self, *a, **k):
            return "original"

        def render_from_camera(self, *a, **k):
            return "original"

    seen = []
    monkeypatch.setattr(M, "render_mesh", lambda *a, **k: seen.append(("mesh", k)) or "fused")
    monkeypatch.setattr(M, "render_from_camera", lambda *a, **k: seen.append(("camera", k)) or "fused")
    assert patch.adopt_mesh_overlay(Renderer) == ["Renderer.render_mesh", "Renderer.render_from_camera"]
    assert patch.adopt_mesh_overlay(Renderer) == []      # idempotent
    r = Renderer(True, "front")
    assert r.render_mesh(1, 2, 3, 4, (8, 8)) == "fused" and r.render_from_camera(1, 2, 3) == "fused"
    assert seen == [("mesh", dict(lighting_type="front")), ("camera", dict(lighting_type="front", use_opengl=True))]
    patch.unpatch_classes(Renderer)
    assert Renderer(False, "constant").render_mesh() == "original" and "_gaa_patched_overlay" not in Renderer.__dict__


def _run(code, **env):
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=REF, env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@needs_ref
def test_patch_reference_adopts_the_overlay_and_gaa_fused_overlay_0_opts_out():
    code = """
        import torch
        from gaussianavatars_amd import patch
        info = patch.patch_reference(pin=False)
        import mesh_renderer
        R = mesh_renderer.NVDiffRenderer
        print("OVERLAY", info["overlay"], R.render_mesh is patch._overlay_render_mesh, R.render_from_camera is patch._overlay_render_from_camera)
        r = R(use_opengl=False, lighting_type="front")
        try:
            r.render_mesh(torch.zeros(1, 3, 3), torch.tensor([[0, 1, 2]]), torch.eye(4)[None], torch.eye(4)[None], (8, 8))
        except ValueError as e:
            print("HOST", "no CPU path" in str(e))
        """
    out = _run(code)
    assert "OVERLAY ['NVDiffRenderer.render_mesh', 'NVDiffRenderer.render_from_camera'] True True" in out and "HOST True" in out
    out = _run(code[:code.index("        r = R(")], GAA_FUSED_OVERLAY="0")      # (the reference's own method is not called: it needs a GPU)
    assert "OVERLAY [] False False" in out
