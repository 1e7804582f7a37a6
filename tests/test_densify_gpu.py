"""Adaptive density control on the GPU (include/gdc.h, csrc/gdc_kernels.hip, gaussianavatars_amd/densify.py) against the float64 statement
of the contract (tests/densify_ref.py) and the reference's own end states (tests/golden/densify_pins.npz).

Bit-exact: the row count, `src`, `binding`, `binding_counter`, every copied leaf row, the gathered moments (+0.0 for new rows) and the zeroed
statistics.  The children's xyz and scaling are held to

    max|gpu - f64|  <=  2 * max|composed-torch fp32 on the same GPU - f64|  +  one fp32 ulp of the tensor's largest magnitude

the bar of tests/test_optim_gpu.py; every check prints the measured ratio.  Inputs keep g, S and o at least 1 % away from their thresholds
(asserted), so one ulp of expf cannot flip a decision."""
import math
import os
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib, densify
from tests import densify_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES = DR.LEAVES
PARAMS = dict(max_grad=2e-4, min_opacity=5e-3, extent=5.0, percent_dense=0.01)
CASES = ["bound_sh3", "bound_sh0", "free_sh3", "free_sh0"]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_inputs(P, F, sh, seed, mode="mixed", i64=False):
    """Seeded inputs whose g, S and o sit well away from the thresholds of PARAMS.  mode: mixed | none | clone | split | protected."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    binding = face_scaling = counter = None
    fs = np.ones(P)
    if F:
        binding = rng.integers(0, F, P)
        binding[:min(P, F)] = np.arange(min(P, F))
        binding = binding.astype(np.int64 if i64 else np.int32)
        face_scaling = f32(rng.uniform(0.5, 2.0, (F, 1)))
        fs = face_scaling[binding, 0].astype(np.float64)
        counter = np.bincount(binding, minlength=F).astype(np.int32)
    sizes = {"mixed": [0.015, 0.15, 1.2], "none": [0.015, 0.15], "clone": [0.015], "split": [0.15, 1.2], "protected": [0.015, 0.15]}[mode]
    target = rng.choice(sizes, P) * rng.uniform(0.8, 1.2, P)
    axes = rng.uniform(0.3, 1.0, (P, 3))
    axes[np.arange(P), rng.integers(0, 3, P)] = 1.0
    scaling = np.log(target[:, None] * axes / fs[:, None])
    levels = {"mixed": [0.2, 3.0], "none": [0.2], "clone": [3.0], "split": [3.0], "protected": [0.2, 3.0]}[mode]
    g = PARAMS["max_grad"] * rng.choice(levels, P) * rng.uniform(0.8, 1.2, P)
    denom = rng.integers(1, 40, P).astype(np.float64)
    accum = g * denom
    if mode == "mixed":
        denom[3::17], accum[3::17] = 0, 0
        denom[5::29] = 0
    low = {"mixed": rng.random(P) < 0.25, "protected": np.ones(P, bool)}.get(mode, np.zeros(P, bool))
    o = np.where(low, rng.uniform(0.001, 0.004, P), rng.uniform(0.1, 0.9, P))
    K = (sh + 1) ** 2 - 1
    leaves = {"_xyz": f32(rng.normal(0, 0.3, (P, 3))), "_features_dc": f32(rng.normal(0, 1, (P, 1, 3))),
              "_features_rest": f32(rng.normal(0, 0.1, (P, K, 3))), "_opacity": f32(np.log(o / (1 - o)))[:, None],
              "_scaling": f32(scaling), "_rotation": f32(rng.normal(0, 1, (P, 4)))}
    moments = {a + k: f32(rng.normal(0, 1e-3, v.shape)) ** (2 if a == "v" else 1) for k, v in leaves.items() for a in "mv"}
    return dict(leaves=leaves, moments=moments, accum=f32(accum)[:, None], denom=f32(denom)[:, None], noise=f32(rng.normal(0, 1, (2, P, 3))),
                binding=binding, face_scaling=face_scaling, counter=counter)


def from_pins(p):
    bound = int(p["F"]) > 0
    inp = dict(leaves={k: p["in" + k] for k in LEAVES}, moments={a + k: p["in_" + a + k] for k in LEAVES for a in "mv"}, accum=p["in_accum"],
               denom=p["in_denom"], noise=p["noise"], binding=p["in_binding"] if bound else None,
               face_scaling=p["in_face_scaling"] if bound else None, counter=p["in_binding_counter"] if bound else None)
    prm = dict(max_grad=float(p["max_grad"]), min_opacity=float(p["min_opacity"]), extent=float(p["extent"]), percent_dense=float(p["percent_dense"]))
    return inp, prm, float(p["max_screen_size"])


def to_dev(a, dev, offset=False):
    """The array on the device; offset: a contiguous view that starts 4 bytes into its allocation."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset or t.element_size() != 4:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (t.numel() == 0 or view.data_ptr() % 16 == 4)
    return view


def run(fn, inp, dev, prm=PARAMS, mss=0, offset=False):
    d = lambda a: to_dev(a, dev, offset)
    leaves = {k: d(v) for k, v in inp["leaves"].items()}
    moments = {k: (d(inp["moments"]["m" + k]), d(inp["moments"]["v" + k])) for k in LEAVES}
    out = fn(leaves, moments, d(inp["accum"]), d(inp["denom"]), d(inp["noise"]), prm["max_grad"], prm["min_opacity"], prm["extent"],
             prm["percent_dense"], mss, d(inp["binding"]), d(inp["face_scaling"]), d(inp["counter"]))
    torch.cuda.synchronize()
    return out


def reference(inp, prm=PARAMS, mss=0, min_margin=0.01):
    ref = DR.densify_ref(inp["leaves"], inp["accum"], inp["denom"], inp["noise"], max_screen_size=mss, binding=inp["binding"],
                         face_scaling=inp["face_scaling"], binding_counter=inp["counter"], moments=inp["moments"], **prm)
    assert ref["margin"] >= min_margin, ref["margin"]
    return ref


def _ulp(x):
    return float(np.spacing(np.float32(abs(x)))) if x else float(np.finfo(np.float32).tiny)


def check(out, ref, inp, composed=None, what=""):
    """Everything exact but the children's xyz / scaling, which are held to the bar of the module text when `composed` is given."""
    n = lambda t: t.cpu().numpy()
    N = ref["src"].shape[0]
    assert sum(out["totals"]) == N == out["src"].shape[0]
    assert np.array_equal(n(out["src"]), ref["src"])
    child = ref["child"]
    for k in LEAVES:
        got = n(out["leaves"][k])
        assert got.shape == (N,) + inp["leaves"][k].shape[1:], k
        rows = ~child if k in ("_xyz", "_scaling") else slice(None)
        assert np.array_equal(got[rows].view(np.uint32), np.asarray(ref[k][rows], np.float32).view(np.uint32)), k
        for i, a in enumerate("mv"):
            assert np.array_equal(n(out["moments"][k][i]).view(np.uint32), ref["moments"][a + k].view(np.uint32)), (k, a)
    for k, shape in (("xyz_gradient_accum", (N, 1)), ("denom", (N, 1)), ("max_radii2D", (N,))):
        assert tuple(out[k].shape) == shape and not n(out[k]).view(np.uint32).any(), k
    if inp["binding"] is not None:
        assert out["binding"].dtype == torch.from_numpy(inp["binding"]).dtype
        assert np.array_equal(n(out["binding"]), ref["binding"]) and np.array_equal(n(out["binding_counter"]), ref["binding_counter"])
        assert np.array_equal(n(out["binding_counter"]), np.bincount(n(out["binding"]), minlength=inp["counter"].shape[0]))
    else:
        assert out["binding"] is None and out["binding_counter"] is None
    if composed is not None and child.any():
        assert np.array_equal(n(composed["src"]), ref["src"])
        for k in ("_xyz", "_scaling"):
            want = ref[k][child]
            e_f = np.abs(n(out["leaves"][k])[child].astype(np.float64) - want).max()
            e_t = np.abs(n(composed["leaves"][k])[child].astype(np.float64) - want).max()
            ulp = _ulp(float(np.abs(want).max()))
            print(f"{what:>24s} {k:>9s}: composed fp32 err {e_t:.3e}  fused err {e_f:.3e}  ratio {e_f / e_t if e_t else math.inf:.3f}  ulp {ulp:.1e}")
            assert e_f <= 2.0 * e_t + ulp, (what, k, e_f, e_t, ulp)


SIZES = [(1, 1, 3), (3, 1, 0), (257, 8, 3), (4099, 64, 3), (4099, 64, 0), (257, 0, 3), (4099, 0, 0), (3, 8, 3)]


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("P,F,sh", SIZES)
def test_sizes_against_the_float64_contract(P, F, sh, offset):
    dev = _dev()
    for mss in (0, 20):
        inp = make_inputs(P, F, sh, seed=1000 * P + F + mss, i64=(P == 257))
        ref = reference(inp, mss=mss)
        out = run(densify.density_control_fused, inp, dev, mss=mss, offset=offset)
        comp = run(densify.density_control_composed, inp, dev, mss=mss)
        check(out, ref, inp, comp, what=f"P={P} F={F} sh={sh} mss={mss}")


@pytest.fixture(scope="module")
def pins():
    z = np.load(os.path.join(ROOT, "tests", "golden", "densify_pins.npz"))
    return {c: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(c + "/")} for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_the_references_end_states(pins, case):
    """The fixtures: the reference's own run.  Copied rows, moments, binding and counters are its bits; its fp32 children lie within the bar too
    (they ARE a composed fp32 evaluation, made on the CPU)."""
    p = pins[case]
    inp, prm, mss = from_pins(p)
    dev = _dev()
    out = run(densify.density_control_fused, inp, dev, prm, mss)
    comp = run(densify.density_control_composed, inp, dev, prm, mss)
    ref = reference(inp, prm, mss)
    check(out, ref, inp, comp, what=case)
    child = ref["child"]
    n = lambda t: t.cpu().numpy()
    for k in LEAVES:
        rows = ~child if k in ("_xyz", "_scaling") else slice(None)
        assert np.array_equal(n(out["leaves"][k])[rows], p["out" + k][rows]), k
        assert np.array_equal(n(out["moments"][k][0]), p["out_m" + k]) and np.array_equal(n(out["moments"][k][1]), p["out_v" + k]), k
    if int(p["F"]):
        assert np.array_equal(n(out["binding"]), p["out_binding"]) and np.array_equal(n(out["binding_counter"]), p["out_binding_counter"])


@pytest.mark.parametrize("mode,F", [("none", 8), ("clone", 8), ("split", 8), ("protected", 8), ("none", 0), ("clone", 0), ("split", 0)])
def test_edge_cases(mode, F):
    dev = _dev()
    P = 300
    inp = make_inputs(P, F, 3, seed=7, mode=mode)
    ref = reference(inp)
    out = run(densify.density_control_fused, inp, dev)
    comp = run(densify.density_control_composed, inp, dev)
    check(out, ref, inp, comp, what=f"{mode} F={F}")
    want = {"none": (P, 0, 0, 0), "clone": (P, P, 0, 0), "split": (0, 0, P, P), "protected": None}[mode]
    if want is not None:
        assert out["totals"] == want
    else:       # every row is a candidate on every face: nothing may go
        assert out["totals"][0] + out["totals"][2] == P and sum(out["totals"]) == P + int(ref["clone"].sum()) + int(ref["split"].sum())


def test_no_splats_launch_nothing():
    dev = _dev()
    for F in (0, 4):
        inp = make_inputs(0, F, 3, seed=1)
        if F:
            inp["counter"] = np.zeros(F, np.int32)
        _lib.gdc_profile_enable(True)
        try:
            out = run(densify.density_control_fused, inp, dev)
            launches = sum(k for _, k in _lib.gdc_profile_read().values())
        finally:
            _lib.gdc_profile_enable(False)
        assert launches == 0 and out["totals"] == (0, 0, 0, 0) and out["src"].shape == (0,)
        assert all(out["leaves"][k].shape == (0,) + inp["leaves"][k].shape[1:] for k in LEAVES)
        if F:
            assert out["binding"].shape == (0,) and not out["binding_counter"].cpu().numpy().any()


def test_two_calls_give_the_same_bits_and_five_launches():
    dev = _dev()
    inp = make_inputs(4099, 64, 3, seed=11)
    a = run(densify.density_control_fused, inp, dev, mss=20)
    _lib.gdc_profile_enable(True)
    try:
        b = run(densify.density_control_fused, inp, dev, mss=20)
        prof = _lib.gdc_profile_read()
    finally:
        _lib.gdc_profile_enable(False)
    assert sorted(k for _, k in prof.values()) == [1] * 5, prof
    assert a["totals"] == b["totals"] and torch.equal(a["src"], b["src"]) and torch.equal(a["binding"], b["binding"])
    assert torch.equal(a["binding_counter"], b["binding_counter"])
    for k in LEAVES:
        assert torch.equal(a["leaves"][k].view(torch.int32), b["leaves"][k].view(torch.int32))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a["moments"][k], b["moments"][k]))


# ---- a live model ---------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=1000, feature_lr=2.5e-3, opacity_lr=5e-2, scaling_lr=5e-3, rotation_lr=1e-3,
                             flame_pose_lr=1e-5, flame_trans_lr=1e-6, flame_expr_lr=1e-3)
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def live_model(inp, sh, dev, fused_adam, monkeypatch):
    from gaussianavatars_amd.gaussian_model import GaussianModel

    monkeypatch.setenv("GAA_FUSED_ADAM", "1" if fused_adam else "0")
    monkeypatch.setenv("GAA_SPATIAL_SORT", "0")      # the rows stay in the contract's order
    m = GaussianModel(sh)
    m.load_arrays({**inp["leaves"], "binding": inp["binding"]}, device=dev)
    if inp["binding"] is not None:
        m.face_scaling = torch.as_tensor(inp["face_scaling"], device=dev)
    m.training_setup(ARGS)
    gen = torch.Generator().manual_seed(3)
    for k in LEAVES:     # one real step: the optimizer's own state
        getattr(m, k).grad = (torch.randn(getattr(m, k).shape, generator=gen) * 1e-3).to(dev)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.xyz_gradient_accum, m.denom = torch.as_tensor(inp["accum"], device=dev), torch.as_tensor(inp["denom"], device=dev)
    m.max_radii2D = torch.full((inp["accum"].shape[0],), 1000.0, device=dev)
    m._gaa_order = torch.arange(inp["accum"].shape[0], device=dev).flip(0)
    return m


def test_optimizer_state_order_and_the_next_step(monkeypatch):
    """torch.optim.Adam and an adopted FusedAdam through the same densification: state re-keyed with `step` kept, other groups untouched,
    state_dict round trip, `_gaa_order` by the wrappers' rule, and the step that follows equal to torch's (the bar of tests/test_optim_gpu.py)."""
    from gaussianavatars_amd.optim import FusedAdam

    dev = _dev()
    inp = make_inputs(4099, 64, 3, seed=5)
    noise = torch.as_tensor(inp["noise"], device=dev)
    models = {}
    for kind in ("torch", "fused"):
        m = live_model(inp, 3, dev, kind == "fused", monkeypatch)
        assert type(m.optimizer) is (FusedAdam if kind == "fused" else torch.optim.Adam)
        pose = torch.nn.Parameter(torch.zeros(4, 3, device=dev))
        m.optimizer.add_param_group({"params": [pose], "lr": 1e-5, "name": "pose"})
        before = {k: getattr(m, k).detach().clone() for k in LEAVES}
        mom = {a + k: m.optimizer.state[getattr(m, k)][key].clone() for k in LEAVES for a, key in (("m", "exp_avg"), ("v", "exp_avg_sq"))}
        _lib.gdc_profile_enable(True)
        try:
            assert m.densify_and_prune(PARAMS["max_grad"], PARAMS["min_opacity"], PARAMS["extent"], 20, noise=noise) is None
            torch.cuda.synchronize()
            assert sum(k for _, k in _lib.gdc_profile_read().values()) == 5        # the kernels ran: this was not the composed path
        finally:
            _lib.gdc_profile_enable(False)
        live = dict(inp, leaves={k: v.cpu().numpy() for k, v in before.items()}, moments={k: v.cpu().numpy() for k, v in mom.items()})
        ref = reference(live, mss=20, min_margin=0.005)      # (one Adam step moved the leaves by 1e-3 of their learning rates)
        N, src = ref["src"].shape[0], torch.from_numpy(ref["src"]).long()
        for k, g in zip(LEAVES, GROUPS):
            p = getattr(m, k)
            group = [x for x in m.optimizer.param_groups if x["name"] == g][0]
            assert len(group["params"]) == 1 and group["params"][0] is p
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.shape[0] == N
            s = m.optimizer.state[p]
            assert float(s["step"]) == 1.0 and s["step"].device.type == "cpu"
            assert np.array_equal(s["exp_avg"].cpu().numpy(), ref["moments"]["m" + k]) and np.array_equal(s["exp_avg_sq"].cpu().numpy(), ref["moments"]["v" + k])
        assert len(m.optimizer.state) == 6 and m.optimizer.param_groups[-1]["params"][0] is pose
        assert torch.equal(m._gaa_order.cpu(), torch.where(src >= 0, (4098 - src), torch.full_like(src, -1)))
        assert torch.equal(m.binding_counter, torch.bincount(m.binding.long(), minlength=64).int())
        assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any() and m.max_radii2D.shape == (N,)
        # state_dict round trip through a fresh torch.optim.Adam over the same parameters
        sd = m.optimizer.state_dict()
        fresh = torch.optim.Adam([{k: v for k, v in g.items()} for g in m.optimizer.param_groups], lr=0.0, eps=1e-15)
        fresh.load_state_dict(sd)
        for k in LEAVES:
            a, b = m.optimizer.state[getattr(m, k)], fresh.state[getattr(m, k)]
            assert float(b["step"]) == 1.0 and torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        models[kind] = m
    a, b = models["torch"], models["fused"]
    gen = torch.Generator().manual_seed(9)
    f64 = {}
    for k, g in zip(LEAVES, GROUPS):
        assert torch.equal(getattr(a, k), getattr(b, k))
        grad = (torch.randn(getattr(a, k).shape, generator=gen) * 1e-3).to(dev)
        getattr(a, k).grad, getattr(b, k).grad = grad, grad.clone()
        # the same step in float64: torch.optim.Adam on double copies of parameter, gradient and moments
        p64 = torch.nn.Parameter(getattr(a, k).detach().double())
        p64.grad = grad.double()
        lr = [x for x in a.optimizer.param_groups if x["name"] == g][0]["lr"]
        o64 = torch.optim.Adam([p64], lr=lr, eps=1e-15)
        s = a.optimizer.state[getattr(a, k)]
        o64.state[p64] = {"step": torch.tensor(1.0), "exp_avg": s["exp_avg"].double().clone(), "exp_avg_sq": s["exp_avg_sq"].double().clone()}
        o64.step()
        f64[k] = p64.detach()
    _lib.gop_profile_enable(True)
    try:
        a.optimizer.step()
        b.optimizer.step()
        torch.cuda.synchronize()
        assert sum(k for _, k in _lib.gop_profile_read().values()) == 1            # b's step was the fused kernel
    finally:
        _lib.gop_profile_enable(False)
    for k in LEAVES:
        e_t = float((getattr(a, k).detach().double() - f64[k]).abs().max())
        e_f = float((getattr(b, k).detach().double() - f64[k]).abs().max())
        ulp = _ulp(float(f64[k].abs().max())) if f64[k].numel() else 0.0
        print(f"next step {k:>15s}: torch fp32 err {e_t:.3e}  fused err {e_f:.3e}  ulp {ulp:.1e}")
        assert e_f <= 2.0 * e_t + ulp, (k, e_f, e_t, ulp)
        assert float(b.optimizer.state[getattr(b, k)]["step"]) == 2.0


def test_outside_the_domain_is_the_composed_path(monkeypatch):
    """GAA_FUSED_DENSIFY=0 and a group without optimizer state: no launch of this library, the same end state."""
    dev = _dev()
    inp = make_inputs(257, 8, 0, seed=21)
    noise = torch.as_tensor(inp["noise"], device=dev)
    ends = []
    for env in ("1", "0"):
        m = live_model(inp, 0, dev, True, monkeypatch)
        monkeypatch.setenv("GAA_FUSED_DENSIFY", env)
        _lib.gdc_profile_enable(True)
        try:
            m.densify_and_prune(PARAMS["max_grad"], PARAMS["min_opacity"], PARAMS["extent"], None, noise=noise)
            torch.cuda.synchronize()
            assert sum(k for _, k in _lib.gdc_profile_read().values()) == (5 if env == "1" else 0)
        finally:
            _lib.gdc_profile_enable(False)
        ends.append(m)
    a, b = ends
    assert torch.equal(a.binding, b.binding) and torch.equal(a.binding_counter, b.binding_counter) and torch.equal(a._gaa_order, b._gaa_order)
    for k in ("_features_dc", "_rotation", "_opacity"):
        assert torch.equal(getattr(a, k), getattr(b, k)) and torch.equal(a.optimizer.state[getattr(a, k)]["exp_avg"], b.optimizer.state[getattr(b, k)]["exp_avg"])


# ---- end to end -------------------------------------------------------------------------------------------------------
class _Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def test_sixty_training_iterations_with_densification(monkeypatch):
    """render -> L1 -> backward -> statistics -> (every 20 iterations) densify_and_prune -> step, on the synthetic bound avatar, with nothing but
    this package: runs, the loss stays finite, the splat count changes and binding_counter == bincount(binding) at the end."""
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.gaussian_model import FlameGaussianModel
    from gaussianavatars_amd.gaussian_renderer import l1_loss, render

    dev = _dev()
    monkeypatch.delenv("GAA_SPATIAL_SORT", raising=False)
    monkeypatch.delenv("GAA_FUSED_DENSIFY", raising=False)
    g = FlameGaussianModel(3, S.flame_rig(seed=4), device=dev)
    P0 = S.FLAME_F + 2000
    g.load_arrays(S.bound_splats(P0, S.FLAME_F, 3, seed=2), device=dev, requires_grad=True)
    g.load_flame_param(S.flame_sequence(4, seed=4), device=dev, requires_grad=True)
    g.training_setup(ARGS)
    assert [x["name"] for x in g.optimizer.param_groups] == list(GROUPS) + ["pose", "trans", "expr"]
    cam = S.orbit_camera(64, 64, r=1.0, fovy_deg=20.0)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, k, torch.as_tensor(getattr(cam, k), device=dev))
    bg = torch.ones(3, device=dev)
    target = torch.full((3, 64, 64), 0.5, device=dev)
    losses, counts, fused_calls = [], [P0], 0
    _lib.gdc_profile_enable(True)
    try:
        for it in range(1, 61):
            g.update_learning_rate(it)
            g.select_mesh_by_timestep(it % 4)
            pkg = render(cam, g, _Pipe, bg)
            loss = l1_loss(pkg["render"], target)
            loss.backward()
            losses.append(float(loss))
            with torch.no_grad():
                g.update_densification_stats(pkg["viewspace_points"], pkg["radii"])
                if it % 20 == 0:
                    # thresholds from the run itself, so that both sides of each are populated whatever the scene's units: the median gradient
                    # statistic of the splats seen so far, and the extent that puts the median world scale at percent_dense * extent
                    seen = g.denom.reshape(-1) > 0
                    max_grad = float((g.xyz_gradient_accum.reshape(-1)[seen] / g.denom.reshape(-1)[seen]).median())
                    extent = float(g.get_scaling.max(dim=1).values.median()) / ARGS.percent_dense
                    assert seen.any() and max_grad > 0
                    g.densify_and_prune(max_grad, 5e-3, extent, 20 if it > 20 else None)
                    counts.append(g._xyz.shape[0])
            g.optimizer.step()
            g.optimizer.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        fused_calls = sum(k for _, k in _lib.gdc_profile_read().values())
    finally:
        _lib.gdc_profile_enable(False)
    print(f"densification loop: splats {counts}, loss {losses[0]:.5f} -> {losses[-1]:.5f}, gdc launches {fused_calls}")
    assert all(math.isfinite(x) for x in losses)
    assert fused_calls == 15 and len(set(counts)) > 1
    N = g._xyz.shape[0]
    assert torch.equal(g.binding_counter, torch.bincount(g.binding.long(), minlength=S.FLAME_F).int()) and g.binding.shape == (N,)
    assert all(getattr(g, k).shape[0] == N for k in LEAVES) and g.denom.shape == (N, 1) and g.max_radii2D.shape == (N,)
    assert all(g.optimizer.state[getattr(g, k)]["exp_avg"].shape == getattr(g, k).shape for k in LEAVES)
