"""Adaptive density control without a GPU (include/gdc.h, gaussianavatars_amd/densify.py): the float64 statement of the contract
(tests/densify_ref.py) reproduces the reference's own end state on every fixture of tests/golden/densify_pins.npz, the composed-torch
statement does too, header / description / library agree, the library's argument checks answer before anything is launched, and a model on
CPU tensors takes the original method."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib, densify
from tests import densify_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["bound_sh3", "bound_sh0", "free_sh3", "free_sh0"]
LEAVES = DR.LEAVES
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def pins():
    z = np.load(os.path.join(ROOT, "tests", "golden", "densify_pins.npz"))
    return {c: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(c + "/")} for c in CASES}


def case_inputs(p):
    leaves = {k: p["in" + k] for k in LEAVES}
    moments = {a + k: p["in_" + a + k] for k in LEAVES for a in "mv"}
    bound = int(p["F"]) > 0
    kw = dict(max_grad=float(p["max_grad"]), min_opacity=float(p["min_opacity"]), extent=float(p["extent"]), percent_dense=float(p["percent_dense"]),
              max_screen_size=float(p["max_screen_size"]), binding=p["in_binding"] if bound else None,
              face_scaling=p["in_face_scaling"] if bound else None, binding_counter=p["in_binding_counter"] if bound else None)
    return leaves, moments, kw


def child_bounds(p, ref):
    """What fp32 rounding may put between the reference's fp32 children and the float64 ones: a few ulp of the largest term of each sum."""
    child = ref["child"]
    w_max = np.abs(ref["_xyz"][child]).max(initial=0.0) + 6.0 * np.exp(p["in_scaling"].astype(np.float64)).max() * (
        p["in_face_scaling"].max() if int(p["F"]) else 1.0)
    return 16 * EPS * w_max, 8 * EPS * max(1.0, np.abs(ref["_scaling"][child]).max(initial=0.0))


@pytest.mark.parametrize("case", CASES)
def test_the_float64_contract_reproduces_the_reference(pins, case):
    p = pins[case]
    leaves, moments, kw = case_inputs(p)
    ref = DR.densify_ref(leaves, p["in_accum"], p["in_denom"], p["noise"], moments=moments, **kw)
    assert ref["margin"] >= 0.01
    N = p["out_xyz"].shape[0]
    assert ref["src"].shape == (N,)
    child = ref["child"]
    assert child.any() and (ref["src"] < 0).sum() > child.sum() and (ref["src"] >= 0).any()   # originals, clones and children are all present
    for k in LEAVES:
        rows = ~child if k in ("_xyz", "_scaling") else slice(None)
        assert np.array_equal(ref[k][rows], p["out" + k][rows]), k
        for a in "mv":
            assert np.array_equal(ref["moments"][a + k], p["out_" + a + k]), (a, k)
            assert not np.signbit(p["out_" + a + k][ref["src"] < 0]).any()
    bx, bs = child_bounds(p, ref)
    assert np.abs(ref["_xyz"][child] - p["out_xyz"][child]).max() <= bx
    assert np.abs(ref["_scaling"][child] - p["out_scaling"][child]).max() <= bs
    for k in ("out_accum", "out_denom", "out_max_radii2D"):
        assert p[k].shape[0] == N and not p[k].any()
    if int(p["F"]):
        assert np.array_equal(ref["binding"], p["out_binding"]) and np.array_equal(ref["binding_counter"], p["out_binding_counter"])
        assert np.array_equal(ref["binding_counter"], np.bincount(ref["binding"], minlength=int(p["F"])))
        b = p["in_binding"]
        on5 = b == 5                                                                    # face 5: nothing but candidates, so all of them stay
        assert ref["cand_row"][on5].all() and np.isin(np.flatnonzero(on5 & ~ref["split"]), ref["src"]).all()
        assert p["out_binding_counter"][5] == on5.sum() + (ref["clone"] | ref["split"])[on5].sum()
        assert (p["out_binding"] == 9).sum() < (b == 9).sum()                           # face 9: its candidates go
    else:
        assert ref["binding"] is None and ref["binding_counter"] is None


def test_the_screen_size_term_is_pinned_by_a_fixture(pins):
    """max_radii2D is 1000 everywhere and max_screen_size 20: were the radius term evaluated, every row would be a candidate."""
    for case in ("bound_sh3", "free_sh0"):
        p = pins[case]
        assert float(p["max_screen_size"]) == 20 and (p["in_max_radii2D"] > 20).all() and p["out_xyz"].shape[0] > int(p["P"]) // 2


@pytest.mark.parametrize("case", CASES)
def test_the_composed_torch_statement_reproduces_the_reference(pins, case):
    p = pins[case]
    leaves, moments, kw = case_inputs(p)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    tl = {k: t(v) for k, v in leaves.items()}
    tm = {k: (t(moments["m" + k]), t(moments["v" + k])) for k in LEAVES}
    out = densify.density_control_composed(tl, tm, t(p["in_accum"]), t(p["in_denom"]), t(p["noise"]), kw["max_grad"], kw["min_opacity"], kw["extent"],
                                           kw["percent_dense"], kw["max_screen_size"], t(kw["binding"]), t(kw["face_scaling"]),
                                           t(kw["binding_counter"]))
    ref = DR.densify_ref(leaves, p["in_accum"], p["in_denom"], p["noise"], **kw)
    assert np.array_equal(out["src"].numpy(), ref["src"])
    child = ref["child"]
    for k in LEAVES:
        rows = ~child if k in ("_xyz", "_scaling") else slice(None)
        assert np.array_equal(out["leaves"][k].numpy()[rows], p["out" + k][rows]), k
        assert np.array_equal(out["moments"][k][0].numpy(), p["out_m" + k]) and np.array_equal(out["moments"][k][1].numpy(), p["out_v" + k])
    bx, bs = child_bounds(p, ref)
    assert np.abs(out["leaves"]["_xyz"].numpy()[child] - ref["_xyz"][child]).max() <= bx
    assert np.abs(out["leaves"]["_scaling"].numpy()[child] - ref["_scaling"][child]).max() <= bs
    if int(p["F"]):
        assert np.array_equal(out["binding"].numpy(), p["out_binding"]) and np.array_equal(out["binding_counter"].numpy(), p["out_binding_counter"])


# ---- header constants and structures (names, ABI and load failures: tests/test_lib_loader_cpu.py) -------------------
def test_header_description_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "gdc.h")).read()
    define = lambda n: int(re.search(r"#define\s+%s\s+\(?(-?[\d <]+)\)?" % n, txt).group(1).replace(" ", "").replace("1<<30", str(1 << 30)))
    assert define("GDC_ABI_VERSION") == _lib.LIBS["gdc"].abi == _lib.GDC_ABI_VERSION
    assert define("GDC_CHUNK") == _lib.GDC_CHUNK and define("GDC_MAX_TENSORS") == _lib.GDC_MAX_TENSORS and define("GDC_MAX_SPLATS") == _lib.GDC_MAX_SPLATS
    for i, n in enumerate(("GDC_COPY", "GDC_MOMENT", "GDC_ZERO", "GDC_XYZ", "GDC_SCALING")):
        assert define(n) == getattr(_lib, n) == i
    assert C.sizeof(_lib.GdcParams) == 20 and C.sizeof(_lib.GdcTensor) == 24
    _lib.profile_enable(("gdc",), True)     # the shims take the tag like any of LIBS
    assert _lib.profile_read(("gdc",)) == {}
    _lib.profile_enable(("gdc",), False)


def test_the_makefile_builds_it_through_the_single_rule():
    mk = open(os.path.join(ROOT, "gaussianavatars_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SINGLE := .*\bgdc\b", mk, flags=re.M) and re.search(r"^gdc_kernels\.o: CONTRACT := -ffp-contract=off$", mk, flags=re.M)


# ---- host argument checks: answered before anything touches a device ------------------------------------------------
def test_library_argument_checks():
    lib = _lib.gdc()
    assert lib.gdc_workspace_bytes(1000, 16) == 4 * (4 + 32 + 16) + 1000 and lib.gdc_workspace_bytes(0, 0) == 16
    assert lib.gdc_workspace_bytes(-1, 0) == -1 and lib.gdc_workspace_bytes(_lib.GDC_MAX_SPLATS, 0) == -1
    totals = (C.c_int32 * 4)(7, 7, 7, 7)
    ok = _lib.GdcParams(2e-4, 5e-3, 5.0, 0.01, 0.0)
    plan = lambda P, F, prm, *ptrs: lib.gdc_plan(P, F, prm, *ptrs, totals, None)
    nul = (None,) * 4 + (None, 0, None, None, None, None)
    assert plan(-1, 0, C.byref(ok), *nul) == -1 and "P = -1" in _lib.gdc_error()
    assert plan(8, 0, None, *nul) == -1 and "NULL params" in _lib.gdc_error()
    assert plan(8, 0, C.byref(_lib.GdcParams(0.0, 5e-3, 5.0, 0.01, 0.0)), *nul) == -1 and "max_grad" in _lib.gdc_error()
    assert plan(8, 0, C.byref(ok), *nul) == -1 and "NULL pointer" in _lib.gdc_error()
    assert plan(8, 4, C.byref(ok), 16, 16, 16, 16, 16, 0, None, None, None, 16) == -1 and "bound model" in _lib.gdc_error()
    assert plan(8, 0, C.byref(ok), 16, 18, 16, 16, None, 0, None, None, None, 16) == -1 and "aligned" in _lib.gdc_error()
    assert list(totals) == [0, 0, 0, 0]
    assert plan(0, 0, C.byref(ok), *nul) == 0 and list(totals) == [0, 0, 0, 0]      # P == 0: nothing is launched, nothing is needed

    emit = lambda P, tot, n, table, *ptrs: lib.gdc_emit(P, 0, (C.c_int32 * 4)(*tot), n, table, *ptrs, None)
    none = (None, None, None, None, None, 0, None, None, None, None)
    assert emit(8, (0, 0, 0, 0), 0, None, *none) == 0                                # N == 0 likewise
    assert emit(8, (9, 0, 0, 0), 0, None, *none) == -1 and "totals[0]" in _lib.gdc_error()
    assert emit(8, (4, 0, 2, 1), 0, None, *none) == -1 and "no plan reports" in _lib.gdc_error()
    assert emit(8, (4, 0, 0, 0), _lib.GDC_MAX_TENSORS + 1, None, *none) == -1 and "ntensors" in _lib.gdc_error()
    assert emit(8, (4, 0, 0, 0), 0, None, *none) == -1 and "NULL pointer" in _lib.gdc_error()
    dev = (16, 16, 16, 16, None, 0, None, 16, None, 16)
    bad_kind = (_lib.GdcTensor * 1)((16, 16, 3, 9))
    assert emit(8, (4, 0, 0, 0), 1, bad_kind, *dev) == -1 and "tensor 0" in _lib.gdc_error()
    two_xyz = (_lib.GdcTensor * 2)((16, 16, 3, _lib.GDC_XYZ), (16, 16, 3, _lib.GDC_XYZ))
    assert emit(8, (4, 0, 0, 0), 2, two_xyz, *dev) == -1 and "one GDC_XYZ" in _lib.gdc_error()
    no_scaling = (_lib.GdcTensor * 1)((16, 16, 3, _lib.GDC_XYZ))
    assert emit(8, (4, 0, 2, 2), 1, no_scaling, *dev) == -1 and "children need" in _lib.gdc_error()


def test_wrapper_argument_checks():
    leaves = {k: torch.zeros((4,) + s) for k, s in zip(LEAVES, ((3,), (1, 3), (0, 3), (1,), (3,), (4,)))}
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        densify.density_control_fused(leaves, None, torch.zeros(4, 1), torch.zeros(4, 1), torch.zeros(2, 4, 3), 2e-4, 5e-3, 5.0, 0.01)
    with pytest.raises(ValueError, match=r"shape \(2, 4, 3\)"):
        densify.density_control_composed(leaves, None, torch.zeros(4, 1), torch.zeros(4, 1), torch.zeros(2, 5, 3), 2e-4, 5e-3, 5.0, 0.01)


# ---- a model on CPU tensors ---------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=1000, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3,
                             flame_pose_lr=1e-5, flame_trans_lr=1e-6, flame_expr_lr=1e-3)


def mirror_model(p, device="cpu"):
    from gaussianavatars_amd.gaussian_model import GaussianModel

    m = GaussianModel(int(p["sh"]))
    arrs = {k: p["in" + k] for k in LEAVES}
    arrs["binding"] = p["in_binding"] if int(p["F"]) else None
    m.load_arrays(arrs, device=device)
    if int(p["F"]):
        m.face_scaling = torch.as_tensor(p["in_face_scaling"], device=device)
    m.training_setup(ARGS)
    for k in LEAVES:    # the fixture's optimizer state, step 1
        m.optimizer.state[getattr(m, k)] = {"step": torch.tensor(1.0), "exp_avg": torch.as_tensor(p["in_m" + k], device=device).clone(),
                                            "exp_avg_sq": torch.as_tensor(p["in_v" + k], device=device).clone()}
    m.xyz_gradient_accum, m.denom = torch.as_tensor(p["in_accum"], device=device).clone(), torch.as_tensor(p["in_denom"], device=device).clone()
    m.max_radii2D = torch.as_tensor(p["in_max_radii2D"], device=device).clone()
    return m


def test_training_setup_builds_the_references_groups():
    from gaussianavatars_amd.gaussian_model import GaussianModel

    m = GaussianModel(0)
    m.load_arrays({k: np.zeros((5,) + s, np.float32) for k, s in zip(LEAVES, ((3,), (1, 3), (0, 3), (1,), (3,), (4,)))}, device="cpu")
    m.training_setup(ARGS)
    assert [g["name"] for g in m.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert [g["lr"] for g in m.optimizer.param_groups] == [1.6e-4, 2.5e-3, 2.5e-3 / 20.0, 5e-2, 5e-3, 1e-3]
    assert m.percent_dense == 0.01 and m.optimizer.defaults["eps"] == 1e-15 and isinstance(m.optimizer, torch.optim.Adam)
    assert m.update_learning_rate(0) == pytest.approx(1.6e-4) and m.update_learning_rate(1000) == pytest.approx(1.6e-6)
    assert m.update_learning_rate(500) == pytest.approx(1.6e-5)


@pytest.mark.parametrize("case", ["bound_sh3", "free_sh0"])
def test_a_cpu_model_takes_the_composed_path_and_matches_the_reference(pins, case):
    p = pins[case]
    m = mirror_model(p)
    P = int(p["P"])
    m._gaa_order = torch.arange(P)
    pose = torch.nn.Parameter(torch.zeros(3))
    m.optimizer.add_param_group({"params": [pose], "lr": 1e-5, "name": "pose"})
    os.environ["GAA_SPATIAL_SORT"] = "0"          # the rows stay in the contract's order
    try:
        m.densify_and_prune(float(p["max_grad"]), float(p["min_opacity"]), float(p["extent"]), float(p["max_screen_size"]) or None,
                            noise=torch.from_numpy(p["noise"]))
    finally:
        del os.environ["GAA_SPATIAL_SORT"]
    ref = DR.densify_ref({k: p["in" + k] for k in LEAVES}, p["in_accum"], p["in_denom"], p["noise"], **case_inputs(p)[2])
    child = ref["child"]
    for k, g in zip(LEAVES, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")):
        param = getattr(m, k)
        group = [x for x in m.optimizer.param_groups if x["name"] == g][0]
        assert group["params"][0] is param and isinstance(param, torch.nn.Parameter) and param.requires_grad
        rows = ~child if k in ("_xyz", "_scaling") else slice(None)
        assert np.array_equal(param.detach().numpy()[rows], p["out" + k][rows])
        s = m.optimizer.state[param]
        assert float(s["step"]) == 1.0 and np.array_equal(s["exp_avg"].numpy(), p["out_m" + k]) and np.array_equal(s["exp_avg_sq"].numpy(), p["out_v" + k])
    assert len(m.optimizer.state) == 6 and m.optimizer.param_groups[-1]["params"][0] is pose
    N = p["out_xyz"].shape[0]
    assert m.xyz_gradient_accum.shape == (N, 1) and m.denom.shape == (N, 1) and m.max_radii2D.shape == (N,)
    assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()
    src = torch.from_numpy(ref["src"]).long()
    assert torch.equal(m._gaa_order, torch.where(src >= 0, src, torch.full_like(src, -1)))
    if int(p["F"]):
        assert np.array_equal(m.binding.numpy(), p["out_binding"]) and np.array_equal(m.binding_counter.numpy(), p["out_binding_counter"])


def test_the_fall_through_returns_the_original_methods_result():
    """A class shaped like the reference's, on CPU tensors: the call IS the original method -- same arguments, same return value."""
    calls = []

    class Model:
        def __init__(self):
            self._xyz = torch.nn.Parameter(torch.zeros(4, 3))
            self.optimizer = None

    def original(self, max_grad, min_opacity, extent, max_screen_size):
        calls.append((self, max_grad, min_opacity, extent, max_screen_size))
        return "the original's result"

    m = Model()
    assert densify.densify_and_prune(m, 2e-4, 5e-3, 5.0, 20, fallback=original) == "the original's result"
    assert calls == [(m, 2e-4, 5e-3, 5.0, 20)]
    with pytest.raises(ValueError, match="noise is only taken by the fused path"):
        densify.densify_and_prune(m, 2e-4, 5e-3, 5.0, 20, noise=torch.zeros(2, 4, 3), fallback=original)


def test_the_patch_hook_passes_the_classes_own_method_as_the_fall_through():
    from gaussianavatars_amd import patch

    class G:
        get_xyz = get_scaling = get_rotation = get_opacity = property(lambda self: None)

        def __init__(self):
            self._xyz = torch.nn.Parameter(torch.zeros(1, 3))
            self.optimizer = None

        def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
            return ("own", max_grad, max_screen_size)

    own = G.__dict__["densify_and_prune"]
    patch.patch_classes(G)
    try:
        assert G.__dict__["densify_and_prune"] is not own and patch._ORIG[(G, "densify_and_prune")] is own
        assert G().densify_and_prune(2e-4, 5e-3, 5.0, None) == ("own", 2e-4, None)
    finally:
        patch.unpatch_classes(G)
    assert G.__dict__["densify_and_prune"] is own


def test_prune_points_and_reset_opacity_on_the_mirror(pins):
    p = pins["bound_sh0"]
    m = mirror_model(p)
    P, F = int(p["P"]), int(p["F"])
    m._gaa_order = torch.arange(P)
    mask = torch.zeros(P, dtype=torch.bool)
    mask[torch.from_numpy(p["in_binding"]) == 3] = True       # all of face 3: protected
    mask[20:40] = True
    want = mask.clone()
    want[torch.from_numpy(p["in_binding"]) == 3] = False
    b = torch.from_numpy(p["in_binding"]).long()
    for f in b[want].unique():                                 # (a face whose every splat lies in 20:40 is protected too)
        if (b[want] == f).sum() == (b == f).sum():
            want[b == f] = False
    m.prune_points(mask)
    assert torch.equal(mask, want)
    keep = ~want
    assert np.array_equal(m._xyz.detach().numpy(), p["in_xyz"][keep.numpy()])
    assert np.array_equal(m.optimizer.state[m._xyz]["exp_avg"].numpy(), p["in_m_xyz"][keep.numpy()])
    assert torch.equal(m.binding_counter, torch.bincount(m.binding.long(), minlength=F).int()) and (m.binding_counter > 0).all()
    assert torch.equal(m._gaa_order, torch.arange(P)[keep])
    m.reset_opacity()
    assert torch.sigmoid(m._opacity).max() <= 0.01 * (1 + 1e-6) and not m.optimizer.state[m._opacity]["exp_avg"].any()
    assert float(m.optimizer.state[m._opacity]["step"]) == 1.0
    assert [g for g in m.optimizer.param_groups if g["name"] == "opacity"][0]["params"][0] is m._opacity
