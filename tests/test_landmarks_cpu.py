"""Landmarks and the root-centred output of FlameHead.forward (include/gab_landmarks.h; flame_model/flame.py:532-553), the parts
that need no GPU: the five new entries in header, description and library; unfused.py's float64 restatement against the reference's recorded
outputs (tests/golden/landmark_pins.npz, written by tests/golden/make_landmark_pins.py); the CSR of the landmark backward; FlameHead's
default call; and the two load_ply keywords of scene/flame_gaussian_model.py:239-269."""
import os
import re

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib
from gaussianavatars_amd import synthetic as S
from tests import binding_ref as BR
from tests import landmark_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"gab_landmarks_forward": 10, "gab_landmarks_backward": 13, "gab_root_joint": 4, "gab_root_center": 6, "gab_root_center_backward": 5}


def test_the_new_entries_in_header_description_and_library():
    """include/gab_landmarks.h (the companion of gab.h, whose own list of entries is pinned by tests/test_binding_cpu.py and
    tests/test_lib_loader_cpu.py), _lib.GAB_LANDMARK_SYMBOLS and the built libgab_hip.so agree, in header order; ABI 5 did not move."""
    txt = open(os.path.join(ROOT, "include", "gab_landmarks.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert '#include "gab.h"' in code
    assert re.findall(r"\b(gab_[a-z0-9_]+)\s*\(", code) == list(NEW_ENTRIES) == list(_lib.GAB_LANDMARK_SYMBOLS)
    assert not set(NEW_ENTRIES) & set(_lib.GAB_SYMBOLS)
    lib = _lib.gab_landmarks()
    assert lib is _lib.gab() and _lib.gab_landmarks() is lib and "raises (never falls" in _lib.gab_landmarks.__doc__
    for name, nargs in NEW_ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/gab_landmarks.h"
        assert len(m.group(1).split(",")) == nargs, name
        res, args = _lib.GAB_LANDMARK_SYMBOLS[name]
        assert res is _lib.C.c_int and len(args) == nargs, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert _lib.GAB_ABI_VERSION == 5 and lib.gab_abi_version() == 5


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("pose", LC.POSES)
def test_unfused_float64_reproduces_the_reference_pins(pose):
    z, rig, p = LC.pins(), LC.rig(), LC.pose_inputs(pose)
    idx, bary = LC.embedding()
    rows = z["vert_rows"]
    for rc, suffix in ((False, ""), (True, "_rc")):
        verts, vs, lm, _ = LC.unfused_eval(rig, p, rig["faces"], idx, bary, torch.float64, zero_centered=rc)
        for name, got in (("verts", verts[0].numpy()[rows]), ("landmarks", lm[0].numpy())):
            err = _rel(got, z[pose + "_" + name + suffix])
            print(f"{pose} {name}{suffix}: rel err {err:.2e}")
            assert err < 1e-12, f"{pose} {name}{suffix}: {err:.2e}"
    root = torch.as_tensor(rig["J_regressor"]).double()[0] @ vs[0]
    assert _rel(root.numpy(), z[pose + "_root"]) < 1e-12


def test_landmark_csr_on_shared_vertices():
    from gaussianavatars_amd import binding as B

    faces, lf = torch.as_tensor(LC.SHARED_FACES), torch.as_tensor(LC.SHARED_LMK_FACE)
    order, begin = B.landmark_csr(faces, lf, LC.SHARED_V)
    L = lf.shape[0]
    assert order.dtype == begin.dtype == torch.int32 and tuple(order.shape) == (3 * L,) and tuple(begin.shape) == (LC.SHARED_V + 1,)
    order, begin = order.tolist(), begin.tolist()
    assert sorted(order) == list(range(3 * L)), "every (l, k) exactly once"
    assert begin[0] == 0 and begin[-1] == 3 * L and all(a <= b for a, b in zip(begin, begin[1:]))
    triples = [(int(LC.SHARED_FACES[LC.SHARED_LMK_FACE[o // 3], o % 3]), o // 3, o % 3) for o in order]
    assert triples == sorted(triples), "rows sorted by (vertex, l, k)"
    for v in range(LC.SHARED_V):
        assert all(t[0] == v for t in triples[begin[v]: begin[v + 1]])
    # vertex 2: landmarks 0, 1, 2 and 4 meet there (as corners 2, 0, 1 and 0); vertex 1 and 3: one landmark each; vertex 6: only the zero weight of (1,0,0)
    assert [t[1:] for t in triples[begin[2]: begin[3]]] == [(0, 2), (1, 0), (2, 1), (4, 0)]
    assert begin[6 + 1] - begin[6] == 1 and LC.SHARED_LMK_BARY[3].tolist() == [1.0, 0.0, 0.0]
    # the sums the kernel forms from this table are the composed-torch gradient
    v = torch.randn(LC.SHARED_V, 3, dtype=torch.float64, requires_grad=True)
    from gaussianavatars_amd import unfused as U

    g = torch.randn(L, 3, dtype=torch.float64)
    (U.landmarks(v[None], faces, lf, torch.as_tensor(LC.SHARED_LMK_BARY).double())[0] * g).sum().backward()
    want = torch.zeros_like(v)
    for (vi, l, k) in triples:
        want[vi] += float(LC.SHARED_LMK_BARY[l, k]) * g[l]
    assert torch.allclose(v.grad, want, rtol=1e-13, atol=0)


def test_embedding_is_checked_on_the_host():
    from gaussianavatars_amd import binding as B

    faces = torch.as_tensor(LC.SHARED_FACES)
    idx, bary = B.check_landmark_embedding(faces, LC.SHARED_LMK_FACE[None], LC.SHARED_LMK_BARY[None].astype(np.float64))   # the reference's layout
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (5,) and bary.dtype == torch.float32 and tuple(bary.shape) == (5, 3)
    for bad in (4, -1):   # F = 4: never launched, refused here
        with pytest.raises(ValueError, match=r"\[0, 4\)"):
            B.check_landmark_embedding(faces, np.array([0, bad, 1]), np.ones((3, 3), np.float32) / 3)
    with pytest.raises(ValueError):
        B.check_landmark_embedding(faces, np.array([0, 1]), np.ones((3, 3), np.float32))
    with pytest.raises(ValueError):
        B.check_landmark_embedding(faces, np.array([0.0, 1.0]), np.ones((2, 3), np.float32))


def _call(head, p, **kw):
    t = lambda k: torch.as_tensor(p[k])
    if kw.pop("bare", False):   # nothing but the seven positional arguments
        return head(t("shape"), t("expr"), t("rotation"), t("neck_pose"), t("jaw_pose"), t("eyes_pose"), t("translation"))
    return head(t("shape"), t("expr"), t("rotation"), t("neck_pose"), t("jaw_pose"), t("eyes_pose"), t("translation"), static_offset=t("static_offset"), **kw)


def test_flame_head_default_call_on_the_cpu():
    """FlameHead(rig)(shape, expr, ...) with nothing else passed: a ValueError that names attach_landmarks without an embedding, the reference's
    [vertices, landmarks] with one -- and [vertices, v_shaped, landmarks] with return_verts_cano (flame.py:539-558)."""
    from gaussianavatars_amd.gaussian_model import FlameHead

    rig, p = LC.rig(), LC.pose_inputs("random")
    idx, bary = LC.embedding()
    z = LC.pins()
    head = FlameHead(rig)
    with pytest.raises(ValueError, match="attach_landmarks"):
        _call(head, p, bare=True)
    plain = _call(FlameHead(rig, impl="unfused"), p, return_landmarks=False)   # (the per-frame call of a fused head stays device-only)
    assert isinstance(plain, torch.Tensor)
    head.attach_landmarks(z["full_lmk_faces_idx"], z["full_lmk_bary_coords"])            # the file's (1,L) / (1,L,3) float64 layout
    assert head.full_lmk_faces_idx.dtype == torch.int64 and tuple(head.full_lmk_faces_idx.shape) == (70,)
    assert head.full_lmk_bary_coords.dtype == torch.float32 and tuple(head.full_lmk_bary_coords.shape) == (70, 3)
    assert [tuple(o.shape) for o in _call(head, p, bare=True)] == [(1, 5143, 3), (1, 70, 3)]
    out = _call(head, p)
    assert isinstance(out, list) and len(out) == 2 and tuple(out[0].shape) == (1, 5143, 3) and tuple(out[1].shape) == (1, 70, 3)
    assert torch.equal(out[0], plain)
    assert _rel(out[1][0].numpy(), z["random_landmarks"]) < 1e-5
    out3 = _call(head, p, return_verts_cano=True, zero_centered_at_root_node=True)
    assert [tuple(o.shape) for o in out3] == [(1, 5143, 3), (1, 5143, 3), (1, 70, 3)]
    assert _rel(out3[0][0].numpy()[z["vert_rows"]], z["random_verts_rc"]) < 1e-5 and _rel(out3[2][0].numpy(), z["random_landmarks_rc"]) < 1e-5
    only = _call(head, p, return_landmarks=False, zero_centered_at_root_node=True)
    assert isinstance(only, torch.Tensor) and torch.equal(only, out3[0])
    # a rig dict that carries the embedding attaches it in the constructor; a bad index is refused there
    head2 = FlameHead({**rig, "full_lmk_faces_idx": idx, "full_lmk_bary_coords": bary})
    assert torch.equal(_call(head2, p)[1], out[1])
    with pytest.raises(ValueError):
        FlameHead(rig).attach_landmarks(np.array([rig["faces"].shape[0]]), np.ones((1, 3), np.float32) / 3)


# ---- load_ply(motion_path=..., disable_fid=...) -------------------------------------------------------------------------------------------
N_SPLATS, T0, T1 = 400, 3, 5
PER_SPLAT = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "binding", "max_radii2D", "xyz_gradient_accum", "denom")


def _saved_model(tmp_path):
    from gaussianavatars_amd.gaussian_model import FlameGaussianModel

    rig = BR.small_rig(37, 3, 5)
    F, V = rig["faces"].shape[0], rig["v_template"].shape[0]
    sp = S.bound_splats(N_SPLATS, F, 1, 3)
    g = np.random.default_rng(12)

    def fp(T):
        f = lambda *s: g.normal(0, 0.1, s).astype(np.float32)
        return dict(shape=f(300), expr=f(T, 100), rotation=f(T, 3), neck_pose=f(T, 3), jaw_pose=f(T, 3), eyes_pose=f(T, 6), translation=f(T, 3),
                    static_offset=f(1, V, 3), dynamic_offset=f(T, V, 3))

    m = FlameGaussianModel(1, rig, binding_impl="unfused", device="cpu")
    m.load_arrays(sp, device="cpu")
    m.load_flame_param(fp(T0), device="cpu")
    ply = tmp_path / "point_cloud" / "point_cloud.ply"
    os.makedirs(ply.parent)
    m.save_ply(str(ply))
    motion = fp(T1)
    np.savez(tmp_path / "motion.npz", **motion, not_float=np.arange(3))
    fresh = lambda: FlameGaussianModel(1, rig, binding_impl="unfused", device="cpu")
    return fresh, ply, motion, F


def test_load_ply_motion_path_replaces_the_dynamic_parameters(tmp_path):
    fresh, ply, motion, _ = _saved_model(tmp_path)
    a, b = fresh(), fresh()
    a.load_ply(str(ply), device="cpu")
    b.load_ply(str(ply), device="cpu", has_target=False, motion_path=str(tmp_path / "motion.npz"))
    assert a.num_timesteps == T0 and b.num_timesteps == T1
    dynamic = ("translation", "rotation", "neck_pose", "jaw_pose", "eyes_pose", "expr", "dynamic_offset")
    assert set(b.flame_param) == set(dynamic) | {"shape", "static_offset"}
    for k in dynamic:
        assert np.array_equal(b.flame_param[k].numpy(), motion[k]), k
    for k in ("shape", "static_offset"):
        assert torch.equal(b.flame_param[k], a.flame_param[k]), k
    assert torch.equal(a._xyz, b._xyz)


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_load_ply_disable_fid_drops_the_splats_of_the_listed_faces(tmp_path, spatial_sort):
    fresh, ply, _, F = _saved_model(tmp_path)
    a, b = fresh(), fresh()
    a.load_ply(str(ply), device="cpu", spatial_sort=spatial_sort)
    fid = torch.as_tensor([int(a.binding[0]), int(a.binding[7]), F - 1, 5])
    b.load_ply(str(ply), device="cpu", spatial_sort=spatial_sort, disable_fid=fid)
    gone = (a.binding[:, None] == fid[None, :]).any(-1)
    assert 0 < int(gone.sum()) < N_SPLATS
    for k in PER_SPLAT:
        ta, tb = getattr(a, k), getattr(b, k)
        assert tb.shape[0] == N_SPLATS - int(gone.sum()), k
        assert torch.equal(tb.detach(), ta.detach()[~gone]), k
    assert isinstance(b._xyz, torch.nn.Parameter) and b._xyz.requires_grad
    assert not (b.binding[:, None] == fid[None, :]).any()
    assert torch.equal(b.binding_counter, torch.bincount(b.binding.long(), minlength=a.binding_counter.shape[0]).to(a.binding_counter.dtype))
    if spatial_sort:
        assert torch.equal(b._gaa_order, a._gaa_order[~gone])
    else:
        assert b._gaa_order is None
    c = fresh()
    c.load_ply(str(ply), device="cpu", spatial_sort=spatial_sort, disable_fid=torch.as_tensor([], dtype=torch.long))   # an empty list: nothing happens
    assert torch.equal(c._xyz, a._xyz)
