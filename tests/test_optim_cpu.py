"""CPU tests of the fused Adam step's host side (gaussianavatars_amd.optim, include/gop.h, patch.patch_optimizer): the library's C ABI, the
optimizer class on host tensors (where every step is torch's own, bit for bit), adopt(), state_dict interchange and the zero-edit hook on a
stand-in shaped like the reference's classes -- and, where the reference checkout is present, on the reference's own
FlameGaussianModel.training_setup.  No GPU."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap
import types

import pytest
import torch

from gaussianavatars_amd import optim, patch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "scene")), reason="reference checkout not present on this box")

# arguments/__init__.py: OptimizationParams
LRS = dict(xyz=0.005, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, scaling=0.017, rotation=0.001, pose=1e-5, trans=1e-6, expr=1e-3)


def _tensors(n=37, t=5, seed=0):
    """The reference's twelve tensors at a toy size, in the order of its nine groups."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return [("xyz", [r(n, 3)]), ("f_dc", [r(n, 1, 3)]), ("f_rest", [r(n, 15, 3)]), ("opacity", [r(n, 1)]), ("scaling", [r(n, 3)]),
            ("rotation", [r(n, 4)]), ("pose", [r(t, 3), r(t, 3), r(t, 3), r(t, 6)]), ("trans", [r(t, 3)]), ("expr", [r(t, 100)])]


def _groups(tensors):
    return [{"params": [torch.nn.Parameter(p.clone()) for p in ps], "lr": LRS[name], "name": name} for name, ps in tensors]


def _params(opt):
    return [p for grp in opt.param_groups for p in grp["params"]]


def _set_grads(opt, step, skip=()):
    g = torch.Generator().manual_seed(1000 + step)
    for i, p in enumerate(_params(opt)):
        grad = torch.randn(p.shape, generator=g) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))
        p.grad = None if i in skip else grad


def _same(a, b):
    for p, q in zip(_params(a), _params(b)):
        assert torch.equal(p, q)
        sa, sb = a.state.get(p, {}), b.state.get(q, {})
        assert sa.keys() == sb.keys()
        for k in sa:
            assert torch.equal(sa[k], sb[k]) and sa[k].device == sb[k].device and sa[k].dtype == sb[k].dtype, k


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_gop_library_exports_every_declared_symbol():
    from gaussianavatars_amd import _lib

    txt = open(os.path.join(ROOT, "include", "gop.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    abi = int(re.search(r"#define\s+GOP_ABI_VERSION\s+(\d+)", txt).group(1))
    names = sorted(set(re.findall(r"\b(gop_[a-z0-9_]+)\s*\(", code)))
    assert len(names) == 8 and "gop_adam_step" in names
    lib = _lib.gop()
    for n in names:
        assert hasattr(lib, n) and n in _lib.GOP_SYMBOLS, n
    assert sorted(_lib.GOP_SYMBOLS) == names
    assert lib.gop_abi_version() == _lib.GOP_ABI_VERSION == abi
    assert int(re.search(r"#define\s+GOP_MAX_TENSORS\s+(\d+)", txt).group(1)) == _lib.GOP_MAX_TENSORS >= 16
    assert int(re.search(r"#define\s+GOP_SLAB\s+(\d+)", txt).group(1)) == _lib.GOP_SLAB
    # the descriptor: the header's fields, in order, and the C layout (four pointers, one int64, two floats)
    body = re.search(r"typedef struct \{(.*?)\} GopAdamTensor;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in _lib.GopAdamTensor._fields_]
    assert C.sizeof(_lib.GopAdamTensor) == 48
    # host-side argument checks (nothing is launched)
    one = _lib.GopAdamTensor(16, 16, 16, 16, 4, 1e-3, 1.0)
    assert lib.gop_adam_step(0, None, 0.9, 0.999, 1e-15, None) == 0                       # nothing to do
    assert lib.gop_adam_step(1, None, 0.9, 0.999, 1e-15, None) < 0 and b"bad arguments" in lib.gop_last_error()
    assert lib.gop_adam_step(1, C.byref(one), 1.0, 0.999, 1e-15, None) < 0 and b"betas" in lib.gop_last_error()
    for field, value, msg in (("n", -1, b"n < 0"), ("grad", None, b"NULL"), ("exp_avg", 18, b"aligned"), ("bias_correction2_sqrt", 0.0, b"bias_correction2_sqrt")):
        bad = _lib.GopAdamTensor(16, 16, 16, 16, 4, 1e-3, 1.0)
        setattr(bad, field, value)
        assert lib.gop_adam_step_ex(1, C.byref(bad), 0.9, 0.1, 0.999, 0.001, 1e-15, None) < 0 and msg in lib.gop_last_error(), field
    empty = _lib.GopAdamTensor(None, None, None, None, 0, 1e-3, 1.0)
    assert lib.gop_adam_step(1, C.byref(empty), 0.9, 0.999, 1e-15, None) == 0               # an empty tensor is skipped: no launch
    assert lib.gop_profile_enable(0) == 0 and lib.gop_profile_reset() == 0 and lib.gop_profile_collect() == 0
    assert lib.gop_profile_entry(0, None, None, None) == -1


def test_optim_imports_neither_oracle_nor_tests():
    txt = open(os.path.join(ROOT, "gaussianavatars_amd", "optim.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", txt, flags=re.M)


# ---- the class on host tensors: torch's own step ----------------------------------------------------------------------------------------
def test_fused_adam_on_cpu_is_torch_adam_bit_for_bit():
    tensors = _tensors()
    a = torch.optim.Adam(_groups(tensors), lr=0.0, eps=1e-15)
    b = optim.FusedAdam(_groups(tensors), lr=0.0, eps=1e-15)
    assert isinstance(b, torch.optim.Adam) and [g["name"] for g in b.param_groups] == list(LRS)
    for step in range(8):
        skip = (2, 7) if step in (3, 4) else ()        # None grads in the middle: f_rest and one pose tensor
        for o in (a, b):
            _set_grads(o, step, skip)
            if step == 5:
                o.param_groups[0]["lr"] = 0.0031       # update_learning_rate: read at step time
            assert o.step() is None
        _same(a, b)
    pa, pb = _params(a), _params(b)
    assert float(a.state[pa[2]]["step"]) == float(b.state[pb[2]]["step"]) == 6.0 and float(b.state[pb[0]]["step"]) == 8.0
    assert all(not b.state[p]["step"].is_cuda and b.state[p]["step"].dim() == 0 for p in pb)


def test_fused_adam_without_any_gradient_creates_no_state():
    b = optim.FusedAdam(_groups(_tensors()), lr=0.0, eps=1e-15)
    assert b.step() is None and len(b.state) == 0


def test_fused_adam_closure_and_hooks_run_once():
    p = torch.nn.Parameter(torch.ones(3))
    b = optim.FusedAdam([p], lr=0.1)
    calls = []
    b.register_step_post_hook(lambda *a: calls.append("post"))

    def closure():
        b.zero_grad()
        loss = (p ** 2).sum()
        loss.backward()
        calls.append("closure")
        return loss

    assert float(b.step(closure).detach()) == 3.0 and calls == ["closure", "post"]
    assert float(b.state[p]["step"]) == 1.0


# ---- adopt ---------------------------------------------------------------------------------------------------------------------------------
def test_adopt_keeps_the_object_and_its_state():
    tensors = _tensors()
    a = torch.optim.Adam(_groups(tensors), lr=0.0, eps=1e-15)
    ref = torch.optim.Adam(_groups(tensors), lr=0.0, eps=1e-15)
    for o in (a, ref):
        _set_grads(o, 0)
        o.step()
    state_before, groups_before = a.state, a.param_groups
    out = optim.adopt(a)
    assert out is a and type(a) is optim.FusedAdam and isinstance(a, torch.optim.Adam)
    assert a.state is state_before and a.param_groups is groups_before and len(a.state) == 12
    assert optim.adopt(a) is a and type(a) is optim.FusedAdam            # already adopted: unchanged
    for o in (a, ref):
        _set_grads(o, 1)
        o.step()
    _same(a, ref)
    hooked = []
    a.register_step_pre_hook(lambda *x: hooked.append(1))               # the step wrapper of Optimizer.__init__ is in place on the new class
    _set_grads(a, 2)
    a.step()
    assert hooked == [1]


def test_adopt_refuses_everything_but_plain_adam():
    class MyAdam(torch.optim.Adam):
        pass

    p = [torch.nn.Parameter(torch.ones(2))]
    for o in (MyAdam(p, lr=0.1), torch.optim.AdamW(p, lr=0.1), torch.optim.SGD(p, lr=0.1)):
        cls = type(o)
        assert optim.adopt(o) is o and type(o) is cls
    assert optim.adopt(None) is None


# ---- state_dict interchange ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["torch", "fused"])
def test_state_dict_loads_into_the_other_class(first):
    tensors = _tensors()
    mk = {"torch": torch.optim.Adam, "fused": optim.FusedAdam}
    other = "fused" if first == "torch" else "torch"
    a = mk[first](_groups(tensors), lr=0.0, eps=1e-15)
    for step in range(3):
        _set_grads(a, step)
        a.step()
    groups = _groups(tensors)
    for grp, src in zip(groups, a.param_groups):
        for p, q in zip(grp["params"], src["params"]):
            p.data.copy_(q.data)
    b = mk[other](groups, lr=0.0, eps=1e-15)
    b.load_state_dict(copy.deepcopy(a.state_dict()))     # (load_state_dict keeps the tensors it is given: a checkpoint comes from a file)
    _same(a, b)
    for o in (a, b):
        _set_grads(o, 3)
        o.step()
    _same(a, b)


# ---- the zero-edit hook on a stand-in shaped like the reference's classes ----------------------------------------------------------------------
def _stand_ins():
    class Model:                                          # scene/gaussian_model.py:208-226
        def __init__(self):
            self.t = {name: [torch.nn.Parameter(p) for p in ps] for name, ps in _tensors()}
            self.optimizer = None
            self.setups = 0

        def training_setup(self, args):
            """the stand-in's own docstring"""
            self.setups += 1
            l = [{"params": self.t[n], "lr": LRS[n] * args.scale, "name": n} for n in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")]
            self.optimizer = torch.optim.Adam(l, lr=0.0, eps=1e-15)

    class FlameModel(Model):                              # scene/flame_gaussian_model.py:174-208
        def training_setup(self, args):
            super().training_setup(args)
            for n in ("pose", "trans", "expr"):
                self.optimizer.add_param_group({"params": self.t[n], "lr": LRS[n], "name": n})

    return Model, FlameModel


def test_patch_optimizer_on_a_stand_in():
    Model, FlameModel = _stand_ins()
    orig_m, orig_f = Model.__dict__["training_setup"], FlameModel.__dict__["training_setup"]
    args = types.SimpleNamespace(scale=1.0)
    try:
        assert patch.patch_optimizer(Model, FlameModel) == ["Model.training_setup", "FlameModel.training_setup"]
        wrapped = FlameModel.__dict__["training_setup"]
        assert wrapped is not orig_f and wrapped.__doc__ == orig_f.__doc__
        assert patch.patch_optimizer(Model, FlameModel) == []                                   # twice: wrapped once
        assert FlameModel.__dict__["training_setup"] is wrapped
        m = FlameModel()
        m.training_setup(args)
        assert m.setups == 1 and type(m.optimizer) is optim.FusedAdam
        assert [g["name"] for g in m.optimizer.param_groups] == list(LRS)
        assert [g["lr"] for g in m.optimizer.param_groups] == list(LRS.values())
        assert sum(len(g["params"]) for g in m.optimizer.param_groups) == 12 and m.optimizer.param_groups[0]["eps"] == 1e-15
        assert m.optimizer.param_groups[0]["params"][0] is m.t["xyz"][0]
        base = Model()
        base.training_setup(args)
        assert type(base.optimizer) is optim.FusedAdam and len(base.optimizer.param_groups) == 6
        # it steps like the torch.optim.Adam the unpatched class builds
        plain = _stand_ins()[1]()
        plain.training_setup(args)
        assert type(plain.optimizer) is torch.optim.Adam
        for step in range(3):
            for o in (m.optimizer, plain.optimizer):
                _set_grads(o, step)
                o.step()
        _same(m.optimizer, plain.optimizer)
    finally:
        patch.unpatch_classes(Model, FlameModel)
    assert Model.__dict__["training_setup"] is orig_m and FlameModel.__dict__["training_setup"] is orig_f
    assert "_gaa_patched_optimizer" not in Model.__dict__ and "_gaa_patched_optimizer" not in FlameModel.__dict__
    m = FlameModel()
    m.training_setup(args)
    assert type(m.optimizer) is torch.optim.Adam


def test_patch_optimizer_skips_classes_without_training_setup():
    from gaussianavatars_amd import gaussian_model as GM

    assert "training_setup" not in GM.GaussianModel.__dict__          # the mirror: its users construct optim.FusedAdam themselves
    assert patch.patch_optimizer(GM.GaussianModel, None) == []
    assert "FusedAdam" in patch.patch_optimizer.__doc__ and "mirror" in patch.patch_optimizer.__doc__


# ---- the reference's own classes (build container only) ------------------------------------------------------------------------------------
_REF_BODY = """
    import os, sys, types
    sys.path.insert(0, {root!r})
    from pathlib import Path
    import torch
    from tests import ref_cpu_env
    ref_cpu_env._no_cuda()
    from gaussianavatars_amd import optim, patch
    info = patch.patch_reference(reference_root={farm!r}, pin=False)
    from scene.flame_gaussian_model import FlameGaussianModel
    from scene.gaussian_model import GaussianModel
    print("INFO", info["optimizer"])
    os.environ["GAA_SPATIAL_SORT"] = "0"
    opt = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.005, position_lr_final=0.00005, position_lr_delay_mult=0.01,
                                position_lr_max_steps=600_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.017, rotation_lr=0.001,
                                flame_pose_lr=1e-5, flame_trans_lr=1e-6, flame_expr_lr=1e-3)
    def model():
        g = FlameGaussianModel(3)
        g.load_ply(Path({ply!r}), has_target=False)
        g.spatial_lr_scale = 1.0
        g.training_setup(opt)
        return g
    g = model()
    o = g.optimizer
    print("TYPE", type(o).__module__ + "." + type(o).__name__, isinstance(o, torch.optim.Adam))
    print("GROUPS", ",".join(grp["name"] for grp in o.param_groups), sum(len(grp["params"]) for grp in o.param_groups))
    # the same model under the reference's unwrapped training_setup
    wrapped = (GaussianModel.training_setup, FlameGaussianModel.training_setup)
    GaussianModel.training_setup = patch._ORIG.get((GaussianModel, "training_setup"), wrapped[0])
    FlameGaussianModel.training_setup = patch._ORIG.get((FlameGaussianModel, "training_setup"), wrapped[1])
    h = model()
    GaussianModel.training_setup, FlameGaussianModel.training_setup = wrapped
    print("PLAIN", type(h.optimizer) is torch.optim.Adam)
    same = True
    for step in range(4):
        gen = torch.Generator().manual_seed(step)
        for grp_a, grp_b in zip(o.param_groups, h.optimizer.param_groups):
            for p, q in zip(grp_a["params"], grp_b["params"]):
                grad = torch.randn(p.shape, generator=gen) * 1e-3
                p.grad, q.grad = (None, None) if (step == 2 and grp_a["name"] == "f_rest") else (grad, grad.clone())
        g.update_learning_rate(step + 1), h.update_learning_rate(step + 1)
        o.step(), h.optimizer.step()
        for grp_a, grp_b in zip(o.param_groups, h.optimizer.param_groups):
            for p, q in zip(grp_a["params"], grp_b["params"]):
                same &= torch.equal(p, q) and torch.equal(o.state[p]["exp_avg_sq"], h.optimizer.state[q]["exp_avg_sq"])
    print("SAME", same)
    # the reference's own surgery on the adopted optimizer's state
    n = g._xyz.shape[0]
    keep = torch.ones(n, dtype=torch.bool); keep[::3] = False
    kept = g._prune_optimizer(keep)                       # scene/gaussian_model.py:355-369
    x = kept["xyz"]
    print("PRUNED", x.shape[0] == int(keep.sum()) < n, type(g.optimizer).__name__, g.optimizer.state[x]["exp_avg"].shape[0] == x.shape[0])
"""


def _run_ref(tmp_path, env_extra):
    from gaussianavatars_amd import synthetic as S
    from tests.test_reference_entry_cpu import symlink_farm

    farm = str(tmp_path / "checkout")
    os.makedirs(farm)
    out = S.write_reference_assets(symlink_farm(farm), str(tmp_path / "avatar"),
                                   os.path.join(REF, "flame_model", "assets", "flame", "head_template_mesh.obj"), n_frames=4)
    code = textwrap.dedent(_REF_BODY.format(root=ROOT, farm=farm, ply=out["point_cloud"]))
    env = dict(os.environ, GAA_BINDING_IMPL="unfused", PYTHONPATH=ROOT, MPLBACKEND="Agg", **env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=farm, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in r.stdout.splitlines() if " " in ln and ln.split(" ", 1)[0].isupper()}


@needs_ref
def test_patch_reference_adopts_the_references_optimizer(tmp_path):
    got = _run_ref(tmp_path, {})
    assert got["INFO"] == "['GaussianModel.training_setup', 'FlameGaussianModel.training_setup']"
    assert got["TYPE"] == "gaussianavatars_amd.optim.FusedAdam True"
    assert got["GROUPS"] == "xyz,f_dc,f_rest,opacity,scaling,rotation,pose,trans,expr 12"
    assert got["PLAIN"] == "True" and got["SAME"] == "True"
    assert got["PRUNED"] == "True FusedAdam True"


@needs_ref
def test_gaa_fused_adam_0_leaves_training_setup_alone(tmp_path):
    got = _run_ref(tmp_path, {"GAA_FUSED_ADAM": "0"})
    assert got["INFO"] == "[]"
    assert got["TYPE"] == "torch.optim.adam.Adam True"
    assert got["GROUPS"] == "xyz,f_dc,f_rest,opacity,scaling,rotation,pose,trans,expr 12"
    assert got["SAME"] == "True"


def test_gaa_fused_adam_0_is_read_by_patch_reference():
    """Everywhere (the reference checkout does not travel): patch_reference consults GAA_FUSED_ADAM and reports under the key 'optimizer'."""
    import inspect

    src = inspect.getsource(patch.patch_reference)
    assert re.search(r'patch_optimizer\(gm\.GaussianModel, fgm\.FlameGaussianModel\) if os\.environ\.get\("GAA_FUSED_ADAM", "1"\) != "0" else \[\]', src)
    assert "optimizer=fused_adam" in src
