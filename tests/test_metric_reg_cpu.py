"""CPU tests of the fused metric-space regularisers' host side (include/gms.h, gaussianavatars_amd.loss.metric_regularizers /
regularization_losses): the library's description and argument checks, the float64 reference of the contract (tests/metric_reg_ref.py)
against torch's float64 autograd of the reference's composed lines (train.py:136, :143), the cases the GPU tests run, the composed-torch path
on host tensors, and which function each flag combination of the drop-in calls.  No GPU."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.metric_reg_ref import CASES, case_id, metric_case, metric_ref, scale_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _composed(xyz, ls, fs, binding, vis, t_xyz, t_s):
    """train.py:136 and :143 without their lambdas; get_scaling is exp(_scaling) * face_scaling[binding] (scene/gaussian_model.py:113-118)."""
    a = F.relu((xyz * fs[binding])[vis] - t_xyz).norm(dim=1).mean()
    b = F.relu((torch.exp(ls) * fs[binding])[vis] - t_s).norm(dim=1).mean()
    return a, b


# ---- the library's description -----------------------------------------------------------------------------------------------------------
def test_description_header_and_library_agree():
    from gaussianavatars_amd import _lib

    txt = open(os.path.join(ROOT, "include", "gms.h")).read()
    # header, description and built file agree name by name, in order: tests/test_lib_loader_cpu.py.  Here, what the names are
    assert list(_lib.LIBS["gms"].symbols) == ["gms_abi_version", "gms_last_error", "gms_scratch_bytes", "gms_forward", "gms_backward",
                                              "gms_profile_enable", "gms_profile_collect", "gms_profile_entry", "gms_profile_reset"]
    assert _lib.gms().gms_abi_version() == _lib.GMS_ABI_VERSION == 1 and isinstance(_lib.gms_error(), str)
    for name in ("GMS_SLAB", "GMS_ROW_BYTES"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1)) == getattr(_lib, name)
    assert _lib.GMS_MAX_SPLATS == 1 << 24 and re.search(r"#define\s+GMS_MAX_SPLATS\s+\(1 << 24\)", txt)
    # the local forms' library and the loss library are untouched by this one
    assert _lib.grl().grl_abi_version() == 1 and _lib.gls().gls_abi_version() == 4
    mk = open(os.path.join(ROOT, "gaussianavatars_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SINGLE := .*\bgms\b", mk, flags=re.M) and re.search(r"^gms_kernels\.o: CONTRACT := -ffp-contract=off$", mk, flags=re.M)


def test_bare_import_maps_no_metric_library():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gaussianavatars_amd\n"
            "from gaussianavatars_amd import _lib\n"
            "import gaussianavatars_amd.loss, gaussianavatars_amd.patch\n"
            "print('MAPPED', 'libgms_hip.so' in open('/proc/self/maps').read())\n"
            "print('LOADED', _lib.gms() is not None and 'libgms_hip.so' in open('/proc/self/maps').read())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "MAPPED False" in r.stdout and "LOADED True" in r.stdout, r.stdout


def test_host_side_argument_checks_launch_nothing():
    """Every call here returns before the first launch: there is no GPU in this process."""
    from gaussianavatars_amd import _lib

    lib = _lib.gms()
    err = lib.gms_last_error
    ok = 64   # any aligned non-NULL address: never dereferenced on the host
    # scratch: the arrival block and one 32-byte partial per GMS_SLAB splats, whatever F
    assert lib.gms_scratch_bytes(0, 1) == lib.gms_scratch_bytes(1, 1) == lib.gms_scratch_bytes(1024, 40) == 48
    assert lib.gms_scratch_bytes(1025, 7) == 80 and lib.gms_scratch_bytes((1 << 24) - 1, 10144) == 16 + 32 * (1 << 14)
    assert lib.gms_scratch_bytes(-1, 1) < 0 and b"P < 0" in err()
    assert lib.gms_scratch_bytes(1 << 24, 1) < 0 and b"2^24" in err()
    assert lib.gms_scratch_bytes(5, 0) < 0 and b"F < 1" in err()

    def fwd(P, F=7, xyz=ok, ls=ok, fs=ok, binding=ok, is64=0, vis=ok, out=ok, scratch=ok):
        return lib.gms_forward(P, F, xyz, ls, fs, binding, is64, vis, 0.1, 0.4, out, scratch, None)

    assert fwd(-1) < 0 and b"P < 0" in err()
    assert fwd(1 << 24) == -1 and b"2^24" in err()
    assert fwd(5, F=0) < 0 and b"F < 1" in err() and fwd(5, F=-3) < 0
    for kw in ("fs", "binding", "vis", "scratch"):
        assert fwd(5, **{kw: None}) < 0 and b"NULL" in err(), kw
    assert fwd(5, xyz=None, ls=None) < 0 and b"no term selected" in err()
    assert fwd(5, out=None) < 0 and b"NULL out" in err()
    assert fwd(0, out=None) < 0 and b"NULL out" in err()
    assert fwd(5, xyz=66) < 0 and b"aligned" in err()
    assert fwd(5, scratch=72) < 0 and b"aligned" in err()
    assert fwd(5, binding=68, is64=1) < 0 and b"aligned" in err()

    def bwd(P, F=7, xyz=ok, ls=ok, fs=ok, binding=ok, vis=ok, out=ok, gx=ok, gs=ok, dx=ok, ds=ok, df=ok, fb=ok, slot=ok, rows=ok):
        return lib.gms_backward(P, F, xyz, ls, fs, binding, 0, vis, 0.1, 0.4, out, gx, gs, dx, ds, df, fb, slot, rows, None)

    assert bwd(-1) < 0 and b"P < 0" in err()
    assert bwd(1 << 24) < 0 and b"2^24" in err()
    assert bwd(7, F=0) < 0 and b"F < 1" in err()
    assert bwd(0, df=None) == 0                                   # P == 0 and no face gradient: nothing to write, nothing enqueued
    assert bwd(7, dx=None, ds=None, df=None) == 0                 # no output wanted: nothing launched
    for kw in ("out", "vis", "fs", "binding"):
        assert bwd(7, **{kw: None}) < 0 and b"NULL" in err(), kw
    assert bwd(7, xyz=None) < 0 and b"g_xyz given" in err()
    assert bwd(7, ls=None) < 0 and b"g_scale given" in err()
    for kw in ("fb", "slot", "rows"):
        assert bwd(7, **{kw: None}) < 0 and b"d_face_scaling wanted" in err(), kw
    assert bwd(7, dx=66) < 0 and b"aligned" in err()
    assert bwd(7, rows=68) < 0 and b"aligned" in err()
    assert lib.gms_profile_enable(0) == 0 and lib.gms_profile_reset() == 0 and lib.gms_profile_collect() == 0
    assert lib.gms_profile_entry(0, None, None, None) == -1


# ---- the float64 reference and the cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,F,opt", [(1, 1, {}), (255, 7, {}), (1025, 40, {}), (3000, 40, dict(one_face=True))])
def test_metric_ref_against_torch_float64_autograd(P, F, opt):
    c = metric_case(P, F, seed=3, **opt)
    gx, gs = 0.37, 1.9
    ref = metric_ref(c["xyz"], c["ls"], c["fs"], c["binding"], c["vis"], c["t_xyz"], c["t_s"], gx, gs)
    clean = lambda a: torch.from_numpy(np.nan_to_num(a)).double()   # (NaN sits in invisible rows only; 0 * NaN would poison torch's backward)
    tx, tl = clean(c["xyz"]).requires_grad_(True), clean(c["ls"]).requires_grad_(True)
    tf = torch.from_numpy(c["fs"]).double()[:, None].requires_grad_(True)
    a, b = _composed(tx, tl, tf, torch.from_numpy(c["binding"]).long(), torch.from_numpy(c["vis"]), float(np.float32(c["t_xyz"])), float(np.float32(c["t_s"])))
    (gx * a + gs * b).backward()
    a, b = a.detach(), b.detach()
    assert ref["count"] == int(c["vis"].sum()) > 0
    assert abs(ref["xyz_mean"] - float(a)) <= 1e-12 * abs(float(a)) and abs(ref["scale_mean"] - float(b)) <= 1e-12 * abs(float(b))
    assert np.abs(ref["d_xyz"] - tx.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["d_scale"] - tl.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["d_face"] - tf.grad.numpy()[:, 0]).max() <= 1e-12 * max(1.0, np.abs(ref["d_face"]).max())
    assert not ref["d_xyz"][~c["vis"]].any() and not ref["d_scale"][~c["vis"]].any()
    # one term alone: the other's gradient vanishes and the face gradient is that term's share
    rx = metric_ref(c["xyz"], c["ls"], c["fs"], c["binding"], c["vis"], c["t_xyz"], c["t_s"], gx, None)
    rs = metric_ref(c["xyz"], c["ls"], c["fs"], c["binding"], c["vis"], c["t_xyz"], c["t_s"], None, gs)
    assert not rx["d_scale"].any() and not rs["d_xyz"].any()
    np.testing.assert_allclose(rx["d_face"] + rs["d_face"], ref["d_face"], rtol=1e-12, atol=1e-15)


def test_metric_ref_hand_cases():
    one = np.ones(1, bool)
    low = np.full((1, 3), -9.0)
    # f = 2: x f = (3, 0.5, -1) against t = 1 -> u = (2, 0, 0), m = 2; d_xyz = g * (1, 0, 0) * f; d_face = g * x_0
    r = metric_ref([[1.5, 0.25, -0.5]], low, [2.0], [0], one, 1.0, 0.5, 0.75, 1.0)
    assert r["xyz_mean"] == 2.0 and r["d_xyz"].tolist() == [[1.5, 0.0, 0.0]] and r["d_face"].tolist() == [0.75 * 1.5]
    assert r["scale_mean"] == 0.0 and not r["d_scale"].any()
    # every component at or under the threshold: m = 0, zero value and zero gradients, not NaN
    r = metric_ref([[0.5, 0.1, -3.0]], low, [2.0], [0], one, 1.0, 0.5)
    assert r["xyz_mean"] == 0.0 and not r["d_xyz"].any() and not r["d_face"].any()
    # nothing visible
    r = metric_ref(np.ones((4, 3)), np.zeros((4, 3)), [1.0, 2.0], [0, 1, 1, 0], np.zeros(4, bool), 0.1, 0.1)
    assert np.isnan(r["xyz_mean"]) and np.isnan(r["scale_mean"]) and r["count"] == 0
    assert not r["d_xyz"].any() and not r["d_scale"].any() and not r["d_face"].any()
    # scale term, two splats on two faces, one axis above the threshold each: b = v_0, d_face = g / c * e_0
    ls = np.log(np.array([[1.0, 0.1, 0.1], [2.0, 0.2, 0.3]]))
    r = metric_ref(np.zeros((2, 3)), ls, [1.0, 0.5], [0, 1], np.ones(2, bool), 9.0, 0.5, 1.0, 3.0)
    assert abs(r["scale_mean"] - (0.5 + 0.5) / 2) < 1e-15
    np.testing.assert_allclose(r["d_face"], [1.5 * 1.0, 1.5 * 2.0], rtol=1e-15)
    np.testing.assert_allclose(r["d_scale"], [[1.5 * 1.0 * 1.0, 0, 0], [1.5 * 0.5 * 2.0, 0, 0]], rtol=1e-15)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cases_hold_what_the_gpu_tests_rely_on(case):
    """By the reference alone: about half the relus fire, exact ties and all-under rows exist where the shape has room for them, faces without
    splats exist, invisible rows carry NaN, and at most 1 % of the entries lie within 2 ulp of the scale threshold."""
    P, nf, opt = case
    c = metric_case(P, nf, **opt)
    assert c["fs"].min() >= 0.5 and c["fs"].max() < 1.5 and c["binding"].dtype == opt.get("index_dtype", np.int64)
    assert c["binding"].min() >= 0 and c["binding"].max() < nf
    ref = metric_ref(c["xyz"], c["ls"], c["fs"], c["binding"], c["vis"], c["t_xyz"], c["t_s"])
    assert scale_band(c, ref).sum() <= 0.01 * 3 * P
    counts = np.bincount(c["binding"], minlength=nf)
    if nf >= 3:
        assert (counts == 0).any()
    if opt.get("one_face"):
        assert counts.max() == P
    mode = opt.get("visible", "some")
    assert ref["count"] == {"all": P, "none": 0}.get(mode, ref["count"])
    if mode == "some" and P >= 255:
        assert 0.5 < c["vis"].mean() < 0.7
        assert np.isnan(c["xyz"][~c["vis"]]).any() and np.isnan(c["ls"][~c["vis"]]).any()
    if mode != "none" and P >= 255:
        px = (c["xyz"] * c["fs"][c["binding"]][:, None]).astype(np.float32)
        fire_x = (px[c["vis"]] > np.float32(c["t_xyz"])).mean()
        fire_s = (ref["q"][c["vis"]] > c["t_s"]).mean()
        assert 0.4 < fire_x < 0.6 and 0.4 < fire_s < 0.6, (fire_x, fire_s)
        assert ((px == np.float32(c["t_xyz"])) & c["vis"][:, None]).sum() >= 6           # exact ties of the fp32 product
        assert ((px < np.float32(c["t_xyz"])).all(1) & c["vis"]).sum() >= 6              # rows with m_i = 0


# ---- the Python entry on host tensors: composed torch, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("flat", [False, True])
def test_metric_regularizers_on_cpu_is_composed_torch_bit_for_bit(flat):
    from gaussianavatars_amd import loss

    c = metric_case(513, 7, seed=1, visible="all")
    leaf = lambda a: torch.from_numpy(a.copy()).requires_grad_(True)
    tb, tv = torch.from_numpy(c["binding"]), torch.from_numpy(c["vis"])
    tx, tl, tf = leaf(c["xyz"]), leaf(c["ls"]), leaf(c["fs"] if flat else c["fs"][:, None])
    a, b = loss.metric_regularizers(tx, tl, tf, tb, tv, c["t_xyz"], c["t_s"])
    (0.01 * a + b).backward()
    rx, rl, rf = leaf(c["xyz"]), leaf(c["ls"]), leaf(c["fs"][:, None])
    ra, rb = _composed(rx, rl, rf, tb, tv, c["t_xyz"], c["t_s"])
    (0.01 * ra + rb).backward()
    assert torch.equal(a, ra) and torch.equal(b, rb) and torch.equal(tx.grad, rx.grad) and torch.equal(tl.grad, rl.grad)
    assert tf.grad.shape == tf.shape and torch.equal(tf.grad.reshape(-1), rf.grad.reshape(-1))
    # one term alone: the other is None, the wanted one is the same number
    only_x = loss.metric_regularizers(tx.detach(), tl.detach(), tf.detach(), tb, tv, c["t_xyz"], c["t_s"], want_scale=False)
    only_s = loss.metric_regularizers(tx.detach(), tl.detach(), tf.detach(), tb, tv, c["t_xyz"], c["t_s"], want_xyz=False)
    assert only_x[1] is None and only_s[0] is None and torch.equal(only_x[0], ra.detach()) and torch.equal(only_s[1], rb.detach())
    assert loss.metric_regularizers(tx, tl, tf, tb, tv, c["t_xyz"], c["t_s"], want_xyz=False, want_scale=False) == (None, None)
    # nothing visible: NaN, NaN and zero gradients
    tx.grad = tl.grad = tf.grad = None
    an, bn = loss.metric_regularizers(tx, tl, tf, tb, torch.zeros_like(tv), c["t_xyz"], c["t_s"])
    assert torch.isnan(an) and torch.isnan(bn)
    (an + bn).backward()
    assert not tx.grad.any() and not tl.grad.any() and not tf.grad.any()


def test_loss_metric_code_imports_neither_oracle_nor_tests():
    txt = open(os.path.join(ROOT, "gaussianavatars_amd", "loss.py")).read()
    assert "def metric_regularizers" in txt and "_lib.gms()" in txt
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", txt, flags=re.M)


# ---- the drop-in: which function a flag combination calls ------------------------------------------------------------------------------------
def test_each_flag_combination_calls_the_function_it_should():
    """A child process counts the calls of splat_regularizers and metric_regularizers behind regularization_losses, and which terms each
    metric call asked for; get_scaling is a property that counts its reads."""
    body = textwrap.dedent(f"""
        import sys, types
        sys.path.insert(0, {ROOT!r})
        import torch
        from gaussianavatars_amd import loss
        local, metric, reads = [], [], []
        real_l, real_m = loss.splat_regularizers, loss.metric_regularizers
        loss.splat_regularizers = lambda *a: (local.append(1), real_l(*a))[1]
        def counted(*a, **kw):
            metric.append((kw["want_xyz"], kw["want_scale"]))
            return real_m(*a, **kw)
        loss.metric_regularizers = counted
        class Model:
            def __init__(self):
                g = torch.Generator().manual_seed(0)
                self._xyz, self._scaling = torch.randn(9, 3, generator=g), torch.randn(9, 3, generator=g)
                self.binding = torch.randint(0, 4, (9,), generator=g)
                self.face_scaling = torch.rand(4, 1, generator=g) + 0.5
            @property
            def get_scaling(self):
                reads.append(1)
                return torch.exp(self._scaling) * self.face_scaling[self.binding]
        for mx in (False, True):
            for ms in (False, True):
                for lam in (1.0, 0.0):
                    del local[:], metric[:], reads[:]
                    opt = types.SimpleNamespace(lambda_xyz=1e-2, threshold_xyz=0.1, lambda_scale=lam, threshold_scale=0.6, metric_xyz=mx, metric_scale=ms)
                    out = loss.regularization_losses(Model(), torch.ones(9, dtype=torch.bool), opt)
                    print("CASE", int(mx), int(ms), lam, "local", len(local), "metric", metric, "reads", len(reads), sorted(out))
    """)
    fused = {(0, 0, 1.0): "local 1 metric [] reads 0 ['scale', 'xyz']",
             (0, 0, 0.0): "local 1 metric [] reads 0 ['xyz']",
             (0, 1, 1.0): "local 1 metric [(False, True)] reads 0 ['scale', 'xyz']",
             (0, 1, 0.0): "local 1 metric [] reads 0 ['xyz']",
             (1, 0, 1.0): "local 1 metric [(True, False)] reads 0 ['scale', 'xyz']",
             (1, 0, 0.0): "local 0 metric [(True, False)] reads 0 ['xyz']",
             (1, 1, 1.0): "local 0 metric [(True, True)] reads 0 ['scale', 'xyz']",
             (1, 1, 0.0): "local 0 metric [(True, False)] reads 0 ['xyz']"}
    for value in (None, "0"):
        env = {k: v for k, v in os.environ.items() if k != "GAA_FUSED_REG"}
        if value is not None:
            env["GAA_FUSED_REG"] = value
        r = subprocess.run([sys.executable, "-c", body], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        for (mx, ms, lam), want in fused.items():
            if value == "0":   # composed torch for everything: neither function is called, the metric scale line reads get_scaling
                want = f"local 0 metric [] reads {int(bool(ms and lam))} " + want.split("reads 0 ")[1]
            assert f"CASE {mx} {ms} {lam} {want}" in r.stdout, (value, mx, ms, lam, r.stdout)


def test_docstrings_name_what_they_should():
    from gaussianavatars_amd import loss

    doc = loss.regularization_losses.__doc__
    assert "face_scaling" in doc and "GAA_FUSED_REG" in doc and "metric_regularizers" in doc
    assert "binding_csr" in loss.metric_regularizers.__doc__
