"""The 3-nearest-neighbour distances without a GPU (include/gdc.h: gdc_knn3_dist2, gaussianavatars_amd/knn.py): the composed-torch statement
against the float64 brute force of tests/knn_ref.py on every case of its table, header / description / library agree on the two additive
entries, the library's argument checks answer before anything touches a device, and `create_from_pcd` on CPU tensors reproduces the
reference's own leaves (tests/golden/pcd_init_pins.npz, tests/golden/make_pcd_golden.py)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib, knn
from tests import knn_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib.GDC_KNN_CHUNK
CASES = KR.cases(C)


@pytest.fixture(scope="module")
def refs():
    return {name: KR.brute_force(cloud) for name, cloud in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_composed_matches_the_float64_brute_force(name, refs):
    cloud = CASES[name]
    got = knn.dist2_knn3_composed(torch.from_numpy(cloud))
    assert got.dtype is torch.float32 and got.shape == (cloud.shape[0],)
    KR.check(got.numpy(), refs[name], name)
    if name == "dup_4":
        assert not got.any()
    if name == "lattice":
        assert (got == 1.0).all()
    if name == "few_1":
        assert got.tolist() == [0.0]


def test_a_cpu_tensor_takes_the_composed_path_and_rows_keep_their_order(refs):
    name = KR.SHUFFLE_OF.format(n=4 * C + 1)
    cloud, perm = KR.shuffled(CASES[name])
    got = knn.dist2_knn3(torch.from_numpy(cloud))
    assert torch.equal(got, knn.dist2_knn3_composed(torch.from_numpy(cloud)))
    KR.check(got.numpy(), refs[name][perm], "shuffled " + name)
    assert knn.dist2_knn3(torch.zeros(0, 3)).shape == (0,)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        knn.dist2_knn3(torch.zeros(4, 2))


def test_types_and_layouts_are_accepted_and_the_input_is_left_alone():
    base = torch.from_numpy(CASES[f"cube_{4 * C + 1}"])
    want = knn.dist2_knn3_composed(base)
    wide = torch.zeros(base.shape[0], 6)
    wide[:, ::2] = base
    view = wide[:, ::2]
    assert not view.is_contiguous()
    kept = wide.clone()
    leaf = base.clone().requires_grad_(True)
    for t in (base.double(), view, leaf):
        got = knn.dist2_knn3(t)
        assert got.dtype is torch.float32 and not got.requires_grad and torch.equal(got, want)
    assert torch.equal(wide, kept)
    assert torch.equal(knn.dist2_knn3(base), knn.dist2_knn3(base))


def test_the_stand_in_keeps_its_cpu_body():
    """shims.simple_knn._C.distCUDA2 on CPU tensors is the |a|^2 + |b|^2 - 2 a.b body it always was: fine at the origin, zeros on a cloud a few
    units away from it (what its docstring now says; device tensors take knn.dist2_knn3, tests/test_knn_gpu.py)."""
    from gaussianavatars_amd.shims.simple_knn import _C

    far = torch.from_numpy(CASES["far_50"])
    assert "cancels" in _C.__doc__ and int((_C.distCUDA2(far) == 0).sum()) > 500
    assert float(knn.dist2_knn3_composed(far).min()) > 0


# ---- header, description, library -------------------------------------------------------------------------------------------------------
def test_header_description_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "gdc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int64_t\s+gdc_knn_workspace_bytes\(int32_t P\);", code)
    assert re.search(r"int\s+gdc_knn3_dist2\(int32_t P, const void\* xyz, void\* dist2_out, void\* workspace, void\* stream\);", code)
    for name in ("gdc_knn_workspace_bytes", "gdc_knn3_dist2"):
        assert name in _lib.GDC_SYMBOLS and hasattr(_lib.gdc(), name)
    assert int(re.search(r"#define\s+GDC_ABI_VERSION\s+(\d+)", txt).group(1)) == 2 == _lib.GDC_ABI_VERSION == _lib.gdc().gdc_abi_version()
    assert int(re.search(r"#define\s+GDC_KNN_CHUNK\s+(\d+)", txt).group(1)) == _lib.GDC_KNN_CHUNK
    mk = open(os.path.join(ROOT, "gaussianavatars_amd", "csrc", "Makefile")).read()
    assert re.search(r"^gdc_kernels\.o:.*\bgdc_knn\.h\b", mk, flags=re.M)


def test_library_argument_checks():
    """Every answer below comes before anything touches a device: this machine has none."""
    lib = _lib.gdc()
    knn3 = lambda P, *ptrs: lib.gdc_knn3_dist2(P, *ptrs, None)
    assert knn3(-1, 16, 16, 16) == -1 and "P = -1" in _lib.gdc_error()
    assert knn3(_lib.GDC_MAX_SPLATS, 16, 16, 16) == -1 and "outside" in _lib.gdc_error()
    for ptrs in ((None, 16, 16), (16, None, 16), (16, 16, None)):
        assert knn3(8, *ptrs) == -1 and "NULL pointer" in _lib.gdc_error()
    assert knn3(8, 18, 16, 16) == -1 and "aligned" in _lib.gdc_error()
    assert knn3(8, 16, 16, 24) == -1 and "16 bytes" in _lib.gdc_error()
    assert knn3(0, None, None, None) == 0                       # P == 0: nothing is launched, nothing is needed
    sizes = [lib.gdc_knn_workspace_bytes(P) for P in (0, 1, 2, C - 1, C, C + 1, 255, 256, 257, 1000, 10 ** 5, 10 ** 6, 10 ** 8, _lib.GDC_MAX_SPLATS - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 4 == 0 for s in sizes)
    assert sizes[-1] > 20 * (_lib.GDC_MAX_SPLATS - 1)            # (no 32-bit arithmetic on the way)
    assert all(lib.gdc_knn_workspace_bytes(P) >= 20 * P + lib.gdc_order_workspace_bytes(P) for P in (1, 1000, 10 ** 6))
    assert lib.gdc_knn_workspace_bytes(-1) == -1 and lib.gdc_knn_workspace_bytes(_lib.GDC_MAX_SPLATS) == -1


# ---- create_from_pcd on CPU tensors -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pins():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pcd_init_pins.npz"))
    return {c: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(c + "/")} for c in ("free", "bound")}


ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=1000, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3,
                             flame_pose_lr=1e-5, flame_trans_lr=1e-6, flame_expr_lr=1e-3)


def test_create_from_pcd_unbound_matches_the_reference(pins):
    from gaussianavatars_amd.gaussian_model import GaussianModel

    p = pins["free"]
    m = GaussianModel(int(p["sh"]))
    m.create_from_pcd(types.SimpleNamespace(points=p["in_points"], colors=p["in_colors"]), float(p["spatial_lr_scale"]), device="cpu")
    KR.check_leaves(m, p)
    assert m.active_sh_degree == 0 and m.binding is None
    m.training_setup(ARGS)
    assert [g["name"] for g in m.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert m.optimizer.param_groups[0]["lr"] == ARGS.position_lr_init * 2.5 and m.xyz_gradient_accum.shape == (300, 1)


def test_create_from_pcd_bound_matches_the_reference(pins):
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.gaussian_model import FlameGaussianModel, GaussianModel

    p = pins["bound"]
    F = int(p["F"])
    m = FlameGaussianModel(int(p["sh"]), S.flame_rig(seed=4), device="cpu")
    m.binding, m.binding_counter = torch.arange(F), torch.ones(F, dtype=torch.int32)
    np.random.seed(int(p["seed"]))
    m.create_from_pcd(None, float(p["spatial_lr_scale"]), device="cpu")
    KR.check_leaves(m, p)
    with pytest.raises(ValueError, match="binding"):
        GaussianModel(3).create_from_pcd(None, 1.0, device="cpu")
