"""The fused Adam step (gaussianavatars_amd.optim.FusedAdam, include/gop.h) on the GPU, against torch.optim.Adam.

The yardstick is torch.optim.Adam in float64.  The bar, for every tensor and for each of param / exp_avg / exp_avg_sq:

    max|fused - fp64|  <=  2 * max|torch_fp32 - fp64|  +  one fp32 ulp of the tensor's largest magnitude

torch_fp32 being torch.optim.Adam on the same GPU in fp32, i.e. what the step was before this class.  The bar is torch's own fp32 error,
measured here; the factor 2 is there because two correct fp32 evaluation orders of one expression differ from each other by as much as
each differs from exact arithmetic; the ulp term covers a tensor on which torch happens to be exact.  Every check prints the ratio
max|fused - fp64| / max|torch_fp32 - fp64| it measured (run with -s).

Gradients are drawn log-uniformly from 1e-9 to 1 (both signs), about 30 % exact zeros, some rows zero on every step and some whole tensors
without a gradient on some steps.  The smallest, 1e-9, squares to 1e-18, far above fp32's smallest normal number: behaviour on gradients
small enough for g * g to go denormal (|g| < 1e-19) is NOT pinned by these tests.

Nothing here reads the reference checkout."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# arguments/__init__.py: OptimizationParams
LRS = dict(xyz=0.005, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, scaling=0.017, rotation=0.001, pose=1e-5, trans=1e-6, expr=1e-3)
SPLAT = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ZERO_ROW = 11          # rows i % ZERO_ROW == 0 never see a gradient


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _reference_tensors(n=4099, t=7, seed=0):
    """[(group name, lr, [fp32 host tensors])]: the reference's twelve tensors in its nine groups.  With N = 4099 and T = 7 every element count
    that can be odd is (3N, 45N, N, 3T, 6T are not multiples of four); rotation (4N) and expr (100T) always are."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    spec = [("xyz", [r(n, 3)]), ("f_dc", [r(n, 1, 3)]), ("f_rest", [r(n, 15, 3)]), ("opacity", [r(n, 1)]), ("scaling", [r(n, 3)]),
            ("rotation", [r(n, 4)]), ("pose", [r(t, 3), r(t, 3), r(t, 3), r(t, 6)]), ("trans", [r(t, 3)]), ("expr", [r(t, 100)])]
    assert sum(1 for _, ps in spec for p in ps if p.numel() % 4) == 10
    return [(name, LRS[name], ps) for name, ps in spec]


def _grad(shape, gen, zero_rows=True):
    """log-uniform 1e-9..1, both signs, ~30 % exact zeros; rows i % ZERO_ROW == 0 always zero"""
    mag = 10.0 ** (-9.0 * torch.rand(shape, generator=gen))
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    g = (mag * sign * (torch.rand(shape, generator=gen) >= 0.3)).float()
    if zero_rows and len(shape) > 0 and shape[0] > 0:
        g[::ZERO_ROW] = 0.0
    return g


class Run:
    """One optimizer of `kind` ('f64': torch.optim.Adam in float64, 'torch': torch.optim.Adam in fp32, 'fused': FusedAdam) on `spec`."""

    def __init__(self, kind, spec, dev, **adam_kw):
        from gaussianavatars_amd.optim import FusedAdam

        self.kind, self.dev = kind, dev
        self.dtype = torch.float64 if kind == "f64" else torch.float32
        groups = [{"params": [self.leaf(p) for p in ps], "lr": lr, "name": name} for name, lr, ps in spec]
        self.opt = (FusedAdam if kind == "fused" else torch.optim.Adam)(groups, lr=0.0, eps=1e-15, **adam_kw)

    def leaf(self, host):
        return host.to(self.dev, self.dtype, copy=True).requires_grad_(True)

    def params(self):
        return [p for grp in self.opt.param_groups for p in grp["params"]]

    def step(self, grads):
        """grads: one fp32 host tensor or None per parameter, in group order"""
        for p, g in zip(self.params(), grads):
            p.grad = None if g is None else g.to(self.dev, self.dtype).reshape(p.shape)
        self.opt.step()

    def snapshot(self):
        out = []
        for p in self.params():
            st = self.opt.state.get(p, {})
            out.append({"param": p.detach().double().cpu(), "exp_avg": st["exp_avg"].double().cpu() if st else None,
                        "exp_avg_sq": st["exp_avg_sq"].double().cpu() if st else None, "step": float(st["step"]) if st else 0.0})
        return out


def _ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


def _check_bar(runs, what):
    """The bar of the module docstring on the current state of runs = {'f64':, 'torch':, 'fused':}; prints the measured ratios."""
    s64, s32, sf = (runs[k].snapshot() for k in ("f64", "torch", "fused"))
    names = [f"{grp['name']}[{i}]" for grp in runs["f64"].opt.param_groups for i in range(len(grp["params"]))]
    worst, same_bits, compared = 0.0, 0, 0
    for name, a, b, c in zip(names, s64, s32, sf):
        assert a["step"] == b["step"] == c["step"], (what, name)
        for q in ("param", "exp_avg", "exp_avg_sq"):
            if a[q] is None:
                assert b[q] is None and c[q] is None, (what, name, q)
                continue
            assert torch.isfinite(c[q]).all(), (what, name, q)
            if a[q].numel() == 0:
                continue
            e_t, e_f = float((b[q] - a[q]).abs().max()), float((c[q] - a[q]).abs().max())
            ulp = _ulp(float(a[q].abs().max()))
            ratio = e_f / e_t if e_t > 0 else (0.0 if e_f == 0 else float("inf"))
            worst = max(worst, ratio if math.isfinite(ratio) else 0.0)
            same_bits, compared = same_bits + int(torch.equal(b[q], c[q])), compared + 1
            print(f"{what:>12s} {name:>12s} {q:>10s}: torch_fp32 err {e_t:.3e}  fused err {e_f:.3e}  ratio {ratio:.3f}  ulp {ulp:.1e}")
            assert e_f <= 2.0 * e_t + ulp, (what, name, q, e_f, e_t, ulp)
    print(f"{what:>12s} worst ratio fused / torch_fp32: {worst:.3f}; bit-identical to torch_fp32 (reported, not required): {same_bits} of {compared} arrays")


def _three(spec, dev, **kw):
    return {k: Run(k, spec, dev, **kw) for k in ("f64", "torch", "fused")}


def _step_all(runs, step, none_for=(), zero_rows=True):
    gen = torch.Generator().manual_seed(77_000 + step)
    grads = []
    for i, p in enumerate(runs["f64"].params()):
        g = _grad(tuple(p.shape), gen, zero_rows)        # (drawn even when unused: the sequence does not depend on the skips)
        grads.append(None if i in none_for else g)
    for r in runs.values():
        r.step(grads)


def _launches():
    from gaussianavatars_amd import _lib

    return sum(k for _, k in _lib.gop_profile_read().values())


# ---- parity -----------------------------------------------------------------------------------------------------------------------------
def test_parity_with_torch_adam_over_50_steps():
    dev = _dev()
    spec = _reference_tensors()
    runs = _three(spec, dev)
    start = runs["fused"].snapshot()
    for step in range(50):
        none_for = (2, 5) if step % 7 == 3 else ((8,) if step % 5 == 4 else ())     # f_rest + rotation, one pose tensor: whole tensors without a gradient
        _step_all(runs, step, none_for)
    torch.cuda.synchronize()
    _check_bar(runs, "50 steps")
    end = runs["fused"].snapshot()
    for a, b, p in zip(start, end, runs["fused"].params()):
        assert torch.isfinite(b["param"]).all() and torch.isfinite(b["exp_avg"]).all() and torch.isfinite(b["exp_avg_sq"]).all()
        assert torch.equal(a["param"][::ZERO_ROW], b["param"][::ZERO_ROW]), "a row whose gradient was always zero moved"
        assert not b["exp_avg"][::ZERO_ROW].any() and not b["exp_avg_sq"][::ZERO_ROW].any()
        assert not torch.equal(a["param"], b["param"])
    steps = [s["step"] for s in end]
    assert steps[0] == 50.0 and steps[2] == steps[5] == 43.0 and steps[8] == 41.0        # every tensor its own step count


def test_two_runs_give_identical_bits():
    dev = _dev()
    spec = _reference_tensors()
    snaps = []
    for _ in range(2):
        runs = {"f64": Run("fused", spec, dev)}       # (only the fused optimizer; _step_all reads the shapes from 'f64')
        for step in range(12):
            _step_all(runs, step, (3,) if step == 5 else ())
        torch.cuda.synchronize()
        r = runs["f64"]
        snaps.append([(p.detach().clone(), r.opt.state[p]["exp_avg"].clone(), r.opt.state[p]["exp_avg_sq"].clone()) for p in r.params()])
    for a, b in zip(*snaps):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- one launch ---------------------------------------------------------------------------------------------------------------------------
def test_twelve_tensors_are_one_launch_and_more_than_the_table_two():
    from gaussianavatars_amd import _lib

    dev = _dev()
    runs = _three(_reference_tensors(), dev)
    _step_all(runs, 0)                                   # (state creation: torch's zeros_like launches are not this library's)
    torch.cuda.synchronize()
    _lib.gop_profile_enable(True)
    try:
        runs["fused"].step([_grad(tuple(p.shape), torch.Generator().manual_seed(5)) for p in runs["fused"].params()])
        torch.cuda.synchronize()
        prof = _lib.gop_profile_read()
        assert list(prof) == ["gop::k_adam"] and prof["gop::k_adam"][1] == 1, prof
        # GOP_MAX_TENSORS + 3 tensors in one group: two launches, still within the bar
        gen = torch.Generator().manual_seed(9)
        many = [("many", 0.01, [torch.randn(3 + 2 * i, 3, generator=gen) for i in range(_lib.GOP_MAX_TENSORS + 3)])]
        big = _three(many, dev)
        _lib.gop_profile_enable(True)                    # (empties the table)
        for step in range(6):
            _step_all(big, step)
        torch.cuda.synchronize()
        assert _launches() == 2 * 6
    finally:
        _lib.gop_profile_enable(False)
    _check_bar(big, "35 tensors")


# ---- skip semantics -------------------------------------------------------------------------------------------------------------------------
def test_tensors_without_a_gradient_are_skipped_and_keep_their_step():
    dev = _dev()
    runs = _three(_reference_tensors(), dev)
    for step in range(3):
        _step_all(runs, step)
    f = runs["fused"]
    before = [(p.detach().clone(), f.opt.state[p]["exp_avg"].clone(), f.opt.state[p]["exp_avg_sq"].clone()) for p in f.params()]
    _step_all(runs, 3, none_for=range(6))                # a densification iteration: the six splat tensors have no gradient
    torch.cuda.synchronize()
    for i, (p, (p0, m0, v0)) in enumerate(zip(f.params(), before)):
        st = f.opt.state[p]
        untouched = torch.equal(p, p0) and torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0)
        assert untouched == (i < 6), i
        assert float(st["step"]) == (3.0 if i < 6 else 4.0) and not st["step"].is_cuda
    for step in range(4, 8):
        _step_all(runs, step)
    torch.cuda.synchronize()
    _check_bar(runs, "after skip")


# ---- surgery on optimizer.state, as scene/gaussian_model.py:334-424 does it ----------------------------------------------------------------------
def _prune(run, mask):
    """_prune_optimizer: the rows of every splat tensor and of its moments where mask is True; the parameter object is replaced."""
    for grp in run.opt.param_groups:
        if grp["name"] not in SPLAT:
            continue
        old = grp["params"][0]
        st = run.opt.state.get(old, None)
        new = old.detach()[mask].clone().requires_grad_(True)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][mask], st["exp_avg_sq"][mask]
            del run.opt.state[old]
            run.opt.state[new] = st
        grp["params"][0] = new


def _cat(run, extension):
    """cat_tensors_to_optimizer: rows appended to every splat tensor, its moments extended with zeros."""
    for grp in run.opt.param_groups:
        if grp["name"] not in SPLAT:
            continue
        old, ext = grp["params"][0], extension[grp["name"]].to(run.dev, run.dtype)
        st = run.opt.state.get(old, None)
        new = torch.cat((old.detach(), ext), 0).requires_grad_(True)
        if st is not None:
            st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), 0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), 0)
            del run.opt.state[old]
            run.opt.state[new] = st
        grp["params"][0] = new


def _replace(run, name, host):
    """replace_tensor_to_optimizer: a new tensor under `name`, moments zeroed (the opacity reset)."""
    for grp in run.opt.param_groups:
        if grp["name"] != name:
            continue
        old = grp["params"][0]
        st = run.opt.state.get(old, None)
        new = host.to(run.dev, run.dtype).requires_grad_(True)
        st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(new), torch.zeros_like(new)
        del run.opt.state[old]
        run.opt.state[new] = st
        grp["params"][0] = new


def test_state_surgery_prune_cat_replace():
    dev = _dev()
    runs = _three(_reference_tensors(), dev)
    n = runs["f64"].params()[0].shape[0]
    for step in range(4):
        _step_all(runs, step)
    gen = torch.Generator().manual_seed(3)
    mask = torch.rand(n, generator=gen) < 0.7
    for r in runs.values():
        _prune(r, mask.to(dev))
    assert runs["fused"].params()[0].shape[0] == int(mask.sum()) < n
    for step in range(4, 8):
        _step_all(runs, step)
    torch.cuda.synchronize()
    _check_bar(runs, "pruned")
    ext = {name: torch.randn(501, *p.shape[1:], generator=gen) for name, p in zip(SPLAT, runs["f64"].params())}
    for r in runs.values():
        _cat(r, ext)
    for step in range(8, 12):
        _step_all(runs, step, zero_rows=False)
    torch.cuda.synchronize()
    _check_bar(runs, "appended")
    rows = runs["f64"].params()[0].shape[0]
    reset = torch.full((rows, 1), -4.59512)                      # inverse_sigmoid(0.01)
    for r in runs.values():
        _replace(r, "opacity", reset)
    for step in range(12, 16):
        _step_all(runs, step, zero_rows=False)
    torch.cuda.synchronize()
    _check_bar(runs, "reset")
    assert float(runs["fused"].opt.state[runs["fused"].params()[3]]["step"]) == 16.0     # the reference keeps the step count through all three


# ---- edge shapes --------------------------------------------------------------------------------------------------------------------------------
class _OffsetRun(Run):
    """Parameters of the group 'offset' start at element 1 of their storage: contiguous, data pointer only 4-byte aligned."""

    def leaf(self, host):
        if getattr(self, "_offset", False):
            base = torch.zeros(host.numel() + 1, device=self.dev, dtype=self.dtype)
            base[1:] = host.to(self.dev, self.dtype).reshape(-1)
            return base[1:].view(host.shape).detach().requires_grad_(True)
        return super().leaf(host)

    def __init__(self, kind, spec, dev):
        self._offset = True
        super().__init__(kind, spec, dev)


def test_edge_shapes_and_a_4_byte_aligned_tensor():
    from gaussianavatars_amd import _lib

    dev = _dev()
    gen = torch.Generator().manual_seed(4)
    small = [("small", 0.01, [torch.randn(k, generator=gen) for k in (1, 3, 4, 5)] + [torch.zeros(0, 3)] +
              [torch.randn(2048, generator=gen), torch.randn(2049, generator=gen), torch.randn(4097, generator=gen)])]
    runs = _three(small, dev)
    for step in range(6):
        _step_all(runs, step, zero_rows=False)
    torch.cuda.synchronize()
    _check_bar(runs, "small")
    offset = [("offset", 0.01, [torch.randn(5, generator=gen), torch.randn(5000, generator=gen), torch.randn(333, 3, generator=gen)])]
    runs = {k: _OffsetRun(k, offset, dev) for k in ("f64", "torch", "fused")}
    f = runs["fused"]
    assert all(p.is_contiguous() and p.data_ptr() % 16 == 4 for p in f.params())
    _lib.gop_profile_enable(True)
    try:
        for step in range(6):
            _step_all(runs, step, zero_rows=False)
        torch.cuda.synchronize()
        assert _launches() == 6                              # handled by the kernel's element-wise path, not by the fallback
    finally:
        _lib.gop_profile_enable(False)
    _check_bar(runs, "offset")


# ---- fallback ---------------------------------------------------------------------------------------------------------------------------------------
def test_out_of_domain_steps_are_torchs_own_bits_and_launch_nothing():
    from gaussianavatars_amd import _lib

    dev = _dev()
    gen = torch.Generator().manual_seed(6)
    spec = [("a", 0.01, [torch.randn(301, 3, generator=gen)]), ("b", 0.002, [torch.randn(40, 7, generator=gen)])]
    _lib.gop_profile_enable(True)
    try:
        # amsgrad
        t, f = Run("torch", spec, dev, amsgrad=True), Run("fused", spec, dev, amsgrad=True)
        for step in range(3):
            _step_all({"f64": t, "fused": f}, step)
        for p, q in zip(t.params(), f.params()):
            assert torch.equal(p, q) and torch.equal(t.opt.state[p]["max_exp_avg_sq"], f.opt.state[q]["max_exp_avg_sq"])
        # a non-contiguous gradient on one tensor: the whole step is torch's
        t, f = Run("torch", spec, dev), Run("fused", spec, dev)
        for step in range(3):
            g0 = _grad((3, 301), gen).t()                 # (301, 3), strides (1, 301)
            g1 = _grad((40, 7), gen)
            for r in (t, f):
                p0, p1 = r.params()
                p0.grad, p1.grad = g0.to(dev).t().contiguous().t(), g1.to(dev)
                assert not p0.grad.is_contiguous()
                r.opt.step()
        for p, q in zip(t.params(), f.params()):
            assert torch.equal(p, q) and torch.equal(t.opt.state[p]["exp_avg"], f.opt.state[q]["exp_avg"])
            assert torch.equal(t.opt.state[p]["exp_avg_sq"], f.opt.state[q]["exp_avg_sq"])
        torch.cuda.synchronize()
        assert _launches() == 0
        # ... and the same optimizer is back on the kernel as soon as the gradients are in its domain
        _step_all({"f64": f}, 9)
        torch.cuda.synchronize()
        assert _launches() == 1
    finally:
        _lib.gop_profile_enable(False)


# ---- checkpoint ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["fused", "torch"])
def test_checkpoint_continues_in_the_other_class(first):
    """state_dict() after 5 steps of one class, loaded into a fresh optimizer of the other: the continuation stays within the bar."""
    dev = _dev()
    spec = _reference_tensors(n=1027)
    other = "torch" if first == "fused" else "fused"
    runs = {"f64": Run("f64", spec, dev), "torch": Run("torch", spec, dev), "fused": Run(first, spec, dev)}
    for step in range(5):
        _step_all(runs, step)
    a = runs["fused"]
    now = [(name, lr, [p.detach().cpu() for p in grp["params"]]) for (name, lr, _), grp in zip(spec, a.opt.param_groups)]
    b = Run(other, now, dev)
    b.opt.load_state_dict(copy.deepcopy(a.opt.state_dict()))
    assert all(not b.opt.state[p]["step"].is_cuda and float(b.opt.state[p]["step"]) == 5.0 for p in b.params())
    runs["fused"] = b
    for step in range(5, 10):
        _step_all(runs, step)
    torch.cuda.synchronize()
    _check_bar(runs, f"{first}->{other}")


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
class _Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def _train(kind, dev, iters=20):
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.gaussian_model import FlameGaussianModel
    from gaussianavatars_amd.gaussian_renderer import l1_loss, render
    from gaussianavatars_amd.optim import FusedAdam

    frames = 12
    g = FlameGaussianModel(3, S.flame_rig(seed=4), device=dev)
    g.load_arrays(S.bound_splats(20000, S.FLAME_F, 3, seed=2), device=dev, requires_grad=True)
    g.load_flame_param(S.flame_sequence(frames, seed=4), device=dev, requires_grad=True)
    cam = S.orbit_camera(208, 176, r=1.0, fovy_deg=20.0)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, k, torch.as_tensor(getattr(cam, k), device=dev))
    fp = g.flame_param
    groups = [{"params": [getattr(g, "_" + ("features_dc" if n == "f_dc" else "features_rest" if n == "f_rest" else n))], "lr": LRS[n], "name": n}
              for n in SPLAT]
    groups += [{"params": [fp["rotation"], fp["neck_pose"], fp["jaw_pose"], fp["eyes_pose"]], "lr": LRS["pose"], "name": "pose"},
               {"params": [fp["translation"]], "lr": LRS["trans"], "name": "trans"}, {"params": [fp["expr"]], "lr": LRS["expr"], "name": "expr"}]
    opt = (FusedAdam if kind == "fused" else torch.optim.Adam)(groups, lr=0.0, eps=1e-15)
    bg = torch.ones(3, device=dev)
    target = torch.full((3, 176, 208), 0.5, device=dev)
    losses = []
    for it in range(iters + 1):
        g.select_mesh_by_timestep(it % 4)
        loss = l1_loss(render(cam, g, _Pipe, bg)["render"], target)
        losses.append(float(loss))
        if it == iters:
            break
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    return losses, opt


def test_twenty_training_iterations_end_to_end():
    """render -> L1 -> backward -> step on the synthetic bound avatar, the groups carrying the reference's learning rates.  torch.optim.Adam runs
    beside it and both final losses are printed; no bar is put on their difference (the fast blend's threshold pixels make two trajectories
    diverge)."""
    from gaussianavatars_amd import _lib
    from gaussianavatars_amd.optim import FusedAdam

    dev = _dev()
    _lib.gop_profile_enable(True)
    try:
        fused, opt = _train("fused", dev)
        torch.cuda.synchronize()
        assert _launches() == 20                       # every step of the loop went through the kernel, once
    finally:
        _lib.gop_profile_enable(False)
    plain, _ = _train("torch", dev)
    print(f"end to end: loss {fused[0]:.6f} -> FusedAdam {fused[-1]:.6f} | torch.optim.Adam {plain[-1]:.6f}")
    assert type(opt) is FusedAdam and all(float(opt.state[grp["params"][0]]["step"]) == 20.0 for grp in opt.param_groups[:6])
    assert all(math.isfinite(x) for x in fused) and all(math.isfinite(x) for x in plain)
    assert fused[-1] < fused[0] and plain[-1] < plain[0]
