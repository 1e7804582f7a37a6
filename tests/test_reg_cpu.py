"""CPU tests of the fused splat regularisers' host side (include/grl.h, gaussianavatars_amd.loss.splat_regularizers / regularization_losses):
the library's C ABI and argument checks, the float64 reference of the contract (tests/reg_ref.py) against torch's float64 autograd of the
reference's composed expressions (train.py:139, :146) and on hand cases, the composed-torch path on host tensors, and the drop-in's keys,
weights and switches.  No GPU."""
import os
import re
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.reg_ref import band_rows, gapped_inputs, generic_inputs, reg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_XYZ, T_S = 1.0, 0.6   # arguments/__init__.py:100-105
T_S32 = float(np.float32(T_S))   # the threshold as the kernel (and torch's fp32 arithmetic) sees it


def _composed(xyz, ls, vis, t_xyz, t_s):
    """train.py:139 and :146 without their lambdas."""
    return F.relu(xyz[vis].norm(dim=1) - t_xyz).mean(), F.relu(torch.exp(ls[vis]) - t_s).norm(dim=1).mean()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_grl_library_exports_every_declared_symbol():
    from gaussianavatars_amd import _lib

    txt = open(os.path.join(ROOT, "include", "grl.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    abi = int(re.search(r"#define\s+GRL_ABI_VERSION\s+(\d+)", txt).group(1))
    names = re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", code)
    assert names == ["grl_abi_version", "grl_last_error", "grl_scratch_bytes", "grl_forward", "grl_backward", "grl_profile_enable",
                     "grl_profile_collect", "grl_profile_entry", "grl_profile_reset"]
    lib = _lib.grl()
    for n in names:
        assert hasattr(lib, n) and n in _lib.GRL_SYMBOLS, n
    assert list(_lib.GRL_SYMBOLS) == names
    assert lib.grl_abi_version() == _lib.GRL_ABI_VERSION == abi == 1
    assert int(re.search(r"#define\s+GRL_SLAB\s+(\d+)", txt).group(1)) == _lib.GRL_SLAB
    assert _lib.GRL_MAX_SPLATS == 1 << 24 and re.search(r"#define\s+GRL_MAX_SPLATS\s+\(1 << 24\)", txt)
    # the loss library's ABI is untouched by this one
    assert _lib.gls().gls_abi_version() == 4


def test_grl_host_side_argument_checks_launch_nothing():
    """Every call here returns before the first launch: there is no GPU in this process."""
    from gaussianavatars_amd import _lib

    lib = _lib.grl()
    ok = 64   # any aligned non-NULL address: never dereferenced on the host
    # scratch size: the arrival block and one 16-byte partial per GRL_SLAB splats
    assert lib.grl_scratch_bytes(0) == lib.grl_scratch_bytes(1) == lib.grl_scratch_bytes(1024) == 32
    assert lib.grl_scratch_bytes(1025) == 48 and lib.grl_scratch_bytes((1 << 24) - 1) == 16 + 16 * (1 << 14)
    assert lib.grl_scratch_bytes(-1) < 0 and b"P < 0" in lib.grl_last_error()
    assert lib.grl_scratch_bytes(1 << 24) < 0 and b"2^24" in lib.grl_last_error()
    fwd = lambda P, xyz=ok, ls=ok, vis=ok, out=ok, scratch=ok: lib.grl_forward(P, xyz, ls, vis, T_XYZ, T_S, out, scratch, None)
    assert fwd(-1) < 0 and b"P < 0" in lib.grl_last_error()
    assert fwd(1 << 24) == -1 and b"2^24" in lib.grl_last_error()
    for kw in ("xyz", "ls", "vis", "scratch"):
        assert fwd(5, **{kw: None}) < 0 and b"NULL" in lib.grl_last_error(), kw
    assert fwd(5, out=None) < 0 and b"NULL out" in lib.grl_last_error()
    assert fwd(0, out=None) < 0 and b"NULL out" in lib.grl_last_error()
    assert fwd(5, xyz=66) < 0 and b"aligned" in lib.grl_last_error()
    assert fwd(5, scratch=68) < 0 and b"aligned" in lib.grl_last_error()

    def bwd(P, xyz=ok, ls=ok, vis=ok, out=ok, gx=ok, gs=ok, dx=ok, ds=ok):
        return lib.grl_backward(P, xyz, ls, vis, T_XYZ, T_S, out, gx, gs, dx, ds, None)

    assert bwd(-1) < 0 and b"P < 0" in lib.grl_last_error()
    assert bwd(1 << 24) < 0 and b"2^24" in lib.grl_last_error()
    assert bwd(0) == 0                                   # P == 0: nothing to write, nothing launched
    assert bwd(0, None, None, None, None, None, None, None, None) == 0
    assert bwd(7, dx=None, ds=None) == 0                 # no output wanted: nothing launched
    assert bwd(7, out=None) < 0 and b"NULL" in lib.grl_last_error()
    assert bwd(7, vis=None) < 0 and b"NULL" in lib.grl_last_error()
    assert bwd(7, xyz=None) < 0 and b"d_xyz wanted" in lib.grl_last_error()
    assert bwd(7, ls=None) < 0 and b"d_log_scaling wanted" in lib.grl_last_error()
    assert bwd(7, dx=66) < 0 and b"aligned" in lib.grl_last_error()
    assert lib.grl_profile_enable(0) == 0 and lib.grl_profile_reset() == 0 and lib.grl_profile_collect() == 0
    assert lib.grl_profile_entry(0, None, None, None) == -1


def test_loss_reg_code_imports_neither_oracle_nor_tests():
    txt = open(os.path.join(ROOT, "gaussianavatars_amd", "loss.py")).read()
    assert "def splat_regularizers" in txt and "def regularization_losses" in txt
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", txt, flags=re.M)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,P", [("generic", 1), ("generic", 257), ("generic", 4099), ("gapped", 4099)])
def test_reg_ref_against_torch_float64_autograd(kind, P):
    xyz, ls, vis = generic_inputs(P, seed=3) if kind == "generic" else gapped_inputs(P, T_XYZ, T_S, seed=3)
    if P == 1:
        vis[:] = True
    gx, gs = 0.37, -1.9
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S, gx, gs)
    tx = torch.from_numpy(xyz).double().requires_grad_(True)
    tl = torch.from_numpy(ls).double().requires_grad_(True)
    a, b = _composed(tx, tl, torch.from_numpy(vis), T_XYZ, T_S32)
    (gx * a + gs * b).backward()
    a, b = a.detach(), b.detach()
    assert ref["count"] == int(vis.sum())
    assert abs(ref["xyz_mean"] - float(a)) <= 1e-12 * abs(float(a))
    assert abs(ref["scale_mean"] - float(b)) <= 1e-12 * abs(float(b))
    assert np.abs(ref["d_xyz"] - tx.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["d_scale"] - tl.grad.numpy()).max() <= 1e-12
    # rows of invisible splats carry no gradient
    assert not ref["d_xyz"][~vis].any() and not ref["d_scale"][~vis].any()


def test_reg_ref_hand_cases():
    t = 1.5
    one = np.ones(1, bool)
    s0 = np.full((1, 3), -5.0)
    r = reg_ref([[t, 0, 0]], s0, one, t, T_S, 2.0, 1.0)                # at the threshold: zero value, zero gradient
    assert r["xyz_mean"] == 0.0 and not r["d_xyz"].any()
    r = reg_ref([[2 * t, 0, 0]], s0, one, t, T_S, 0.75, 1.0)           # the only visible splat, twice the threshold
    assert r["xyz_mean"] == t and r["d_xyz"].tolist() == [[0.75, 0.0, 0.0]]
    r = reg_ref([[0, 0, 0]], s0, one, t, T_S, 1.0, 1.0)                # the origin: zero, not NaN
    assert r["xyz_mean"] == 0.0 and not r["d_xyz"].any() and np.isfinite(r["d_xyz"]).all()
    assert r["scale_mean"] == 0.0 and not r["d_scale"].any()           # exp(-5) is under the threshold on every axis
    r = reg_ref(np.ones((4, 3)) * 3, np.zeros((4, 3)), np.zeros(4, bool), t, T_S)   # nothing visible
    assert np.isnan(r["xyz_mean"]) and np.isnan(r["scale_mean"]) and r["count"] == 0 and not r["d_xyz"].any() and not r["d_scale"].any()
    # all visible, one axis above the scale threshold: b = v_0 and the gradient is g / c * e_0 on that axis alone
    ls = np.log(np.array([[1.0, 0.1, 0.1], [2.0, 0.2, 0.3]]))
    r = reg_ref(np.zeros((2, 3)), ls, np.ones(2, bool), t, 0.5, 1.0, 3.0)
    assert r["count"] == 2 and abs(r["scale_mean"] - (0.5 + 1.5) / 2) < 1e-15
    np.testing.assert_allclose(r["d_scale"], [[1.5 * 1.0, 0, 0], [1.5 * 2.0, 0, 0]], rtol=1e-15, atol=0)


def test_generic_inputs_put_few_rows_in_the_threshold_band():
    """The cap the GPU test applies (<= 2 % of rows excluded from the tight gradient bar) holds for the committed seed by the reference alone."""
    P = 70_001
    xyz, ls, vis = generic_inputs(P, seed=0)
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S)
    share = band_rows(ref, T_XYZ, T_S).mean()
    assert 0 < share <= 0.02, share
    assert 0.45 < vis.mean() < 0.55
    above = (ref["n"] > T_XYZ).mean(), (ref["e"] > T_S32).mean()
    assert 0.2 < above[0] < 0.8 and 0.1 < above[1] < 0.5, above


def test_gapped_inputs_keep_their_gap_in_fp32():
    for P in (1, 3, 257, 4099, 70_001):
        xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=P)
        ref = reg_ref(xyz, ls, vis, T_XYZ, T_S)
        assert ((ref["n"] <= 0.5 * T_XYZ) | (ref["n"] >= 1.5 * T_XYZ)).all()
        assert ((ref["e"] <= 0.5 * T_S) | (ref["e"] >= 1.5 * T_S)).all()
        if P >= 257:
            assert 0.4 < vis.mean() < 0.6 and 0.4 < (ref["n"] > T_XYZ).mean() < 0.6 and 0.4 < (ref["e"] > T_S).mean() < 0.6


# ---- the Python entry on host tensors: composed torch, bit for bit ---------------------------------------------------------------------------
def test_splat_regularizers_on_cpu_is_composed_torch_bit_for_bit():
    from gaussianavatars_amd import loss

    xyz, ls, vis = generic_inputs(513, seed=1)
    tx, tl, tv = torch.from_numpy(xyz).requires_grad_(True), torch.from_numpy(ls).requires_grad_(True), torch.from_numpy(vis)
    a, b = loss.splat_regularizers(tx, tl, tv, T_XYZ, T_S)
    (0.01 * a + b).backward()
    rx, rl = torch.from_numpy(xyz).requires_grad_(True), torch.from_numpy(ls).requires_grad_(True)
    ra, rb = _composed(rx, rl, tv, T_XYZ, T_S)
    (0.01 * ra + rb).backward()
    assert torch.equal(a, ra) and torch.equal(b, rb) and torch.equal(tx.grad, rx.grad) and torch.equal(tl.grad, rl.grad)
    # outside the kernel's domain in other ways: float64 inputs, an index list as the filter
    a64, b64 = loss.splat_regularizers(tx.detach().double(), tl.detach().double(), tv, T_XYZ, T_S)
    assert a64.dtype == torch.float64 and abs(float(a64) - float(ra.detach())) < 1e-6
    idx = torch.nonzero(tv)[:, 0]
    ai, bi = loss.splat_regularizers(tx.detach(), tl.detach(), idx, T_XYZ, T_S)
    assert torch.equal(ai, ra.detach()) and torch.equal(bi, rb.detach())
    # nothing visible: NaN, NaN (the mean of an empty tensor) and zero gradients
    tx.grad = tl.grad = None
    an, bn = loss.splat_regularizers(tx, tl, torch.zeros_like(tv), T_XYZ, T_S)
    assert torch.isnan(an) and torch.isnan(bn)
    (an + bn).backward()
    assert not tx.grad.any() and not tl.grad.any()


# ---- the drop-in for train.py:135-146 ------------------------------------------------------------------------------------------------------------
def _stand_in(P=200, seed=2, bound=True):
    xyz, ls, vis = generic_inputs(P, seed=seed)
    g = types.SimpleNamespace()
    g._xyz = torch.nn.Parameter(torch.from_numpy(xyz))
    g._scaling = torch.nn.Parameter(torch.from_numpy(ls))
    gen = torch.Generator().manual_seed(seed)
    g.binding = torch.randint(0, 7, (P,), generator=gen) if bound else None
    g.face_scaling = torch.rand(7, 1, generator=gen) + 0.5
    g.get_scaling = torch.exp(g._scaling) * g.face_scaling[g.binding] if bound else torch.exp(g._scaling)
    return g, torch.from_numpy(vis)


def _opt(**kw):
    base = dict(lambda_xyz=1e-2, threshold_xyz=T_XYZ, lambda_scale=1.0, threshold_scale=T_S, metric_xyz=False, metric_scale=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _reference_lines(g, vis, opt):
    """train.py:134-146, copied line for line in meaning."""
    losses = {}
    if g.binding is not None:
        if opt.metric_xyz:
            losses["xyz"] = F.relu((g._xyz * g.face_scaling[g.binding])[vis] - opt.threshold_xyz).norm(dim=1).mean() * opt.lambda_xyz
        else:
            losses["xyz"] = F.relu(g._xyz[vis].norm(dim=1) - opt.threshold_xyz).mean() * opt.lambda_xyz
        if opt.lambda_scale != 0:
            if opt.metric_scale:
                losses["scale"] = F.relu(g.get_scaling[vis] - opt.threshold_scale).norm(dim=1).mean() * opt.lambda_scale
            else:
                losses["scale"] = F.relu(torch.exp(g._scaling[vis]) - opt.threshold_scale).norm(dim=1).mean() * opt.lambda_scale
    return losses


@pytest.mark.parametrize("metric_xyz", [False, True])
@pytest.mark.parametrize("metric_scale", [False, True])
@pytest.mark.parametrize("lambda_scale", [0.0, 1.0, 0.25])
def test_regularization_losses_keys_weights_and_metric_flags(metric_xyz, metric_scale, lambda_scale):
    from gaussianavatars_amd import loss

    g, vis = _stand_in()
    opt = _opt(metric_xyz=metric_xyz, metric_scale=metric_scale, lambda_scale=lambda_scale, lambda_xyz=0.03)
    got = loss.regularization_losses(g, vis, opt)
    want = _reference_lines(g, vis, opt)
    assert list(got) == list(want) == (["xyz", "scale"] if lambda_scale != 0 else ["xyz"])
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # the lambdas are applied: the plain means times the weights
    a, b = _composed(g._xyz, g._scaling, vis, T_XYZ, T_S)
    if not metric_xyz:
        assert torch.equal(got["xyz"], a * 0.03)
    if not metric_scale and lambda_scale != 0:
        assert torch.equal(got["scale"], b * lambda_scale)
    if metric_xyz:                              # the metric form is a different number: the flag did reach the composed line
        assert not torch.equal(got["xyz"], a * 0.03)
    sum(got.values()).backward()
    assert g._xyz.grad is not None and (lambda_scale == 0 or g._scaling.grad is not None)


def test_regularization_losses_of_an_unbound_model_is_empty():
    from gaussianavatars_amd import loss

    g, vis = _stand_in(bound=False)
    assert loss.regularization_losses(g, vis, _opt()) == {}
    assert "face_scaling" in loss.regularization_losses.__doc__ and "GAA_FUSED_REG" in loss.regularization_losses.__doc__


def test_fused_path_is_taken_unless_gaa_fused_reg_is_0():
    """A child process counts the calls of splat_regularizers behind regularization_losses, with and without GAA_FUSED_REG=0."""
    body = textwrap.dedent(f"""
        import sys, types
        sys.path.insert(0, {ROOT!r})
        import torch
        from gaussianavatars_amd import loss
        calls = []
        real = loss.splat_regularizers
        loss.splat_regularizers = lambda *a: (calls.append(1), real(*a))[1]
        g = types.SimpleNamespace(_xyz=torch.randn(9, 3), _scaling=torch.randn(9, 3), binding=torch.zeros(9, dtype=torch.long))
        opt = types.SimpleNamespace(lambda_xyz=1e-2, threshold_xyz=1.0, lambda_scale=1.0, threshold_scale=0.6, metric_xyz=False, metric_scale=False)
        out = loss.regularization_losses(g, torch.ones(9, dtype=torch.bool), opt)
        print("CALLS", len(calls), sorted(out))
    """)
    for value, want in ((None, "CALLS 1 ['scale', 'xyz']"), ("1", "CALLS 1 ['scale', 'xyz']"), ("0", "CALLS 0 ['scale', 'xyz']")):
        env = {k: v for k, v in os.environ.items() if k != "GAA_FUSED_REG"}
        if value is not None:
            env["GAA_FUSED_REG"] = value
        r = subprocess.run([sys.executable, "-c", body], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert want in r.stdout, (value, r.stdout)
