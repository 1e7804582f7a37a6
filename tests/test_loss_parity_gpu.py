"""GPU parity of libgls (include/gls.h) against the fp64 references of tests/loss_cases.py: the fused L1 + SSIM pair at tile-edge shapes through
every entry of loss.py and both host sides, the C ABI inside NaN guard bands, the plain L1 at the sizes where its grid changes, the L1 inputs
outside [0,1) the one-launch form was never shown (and the state it leaves on the stream), and the two statistics kernels.

Bars: tests/loss_cases.py.  `pytest -s` prints the kernel's distance, ref32's and the bar of every assertion.  No test reads the reference."""
import contextlib
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _host, _lib
from gaussianavatars_amd import loss as L
from oracle import loss_oracle as LO

import loss_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(x, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def _host_side(native):
    prev = _host.set_enabled(native)
    try:
        yield
    finally:
        _host.set_enabled(prev)


def _model(figure, shape, kind, config, swapped=False):
    return LC.model(shape, kind, config, swapped) if (figure, kind) in LC.MODEL_BARS else None


# ---- SSIM and the fused pair ----------------------------------------------------------------------------------------------------------------
def _loss_of(config, ta, tb):
    """One configuration through the entry of loss.py that serves it."""
    if config == "ssim":
        return L.ssim(ta, tb)
    if config in ("weights", "mean"):
        per = L.ssim(ta, tb, size_average=False)
        return LC.combine(config, {"ssim_i": per}, per.detach())
    if config in ("l1", "mix"):
        l1, ss = L.l1_ssim(ta, tb)
        return LC.combine(config, {"l1": l1, "ssim": ss, "ssim_i": ss.detach().reshape(-1)}, l1.detach())
    l1_i, ss_i = L._L1Ssim.apply(ta, tb)   # per-image L1 with weights that differ: the node itself
    return LC.combine(config, {"l1_i": l1_i.reshape(-1), "ssim_i": ss_i.reshape(-1)}, l1_i.detach())


def _check_values(dev, shape, kind, a, b, tag):
    vals = LC.values(shape, kind)
    ta, tb = _t(a, dev), _t(b, dev)
    m = _model("ssim_value", shape, kind, "ssim")
    per = _np(L.ssim(ta, tb, size_average=False)).astype(np.float64)
    LC.assert_scalar(per, *vals["ssim_i"], f"{tag} ssim per image", None if m is None else m[0])
    assert np.all(np.abs(per - vals["ssim_i"][1]) < LC.SSIM_BAR)
    avg = L.ssim(ta, tb)
    LC.assert_scalar(float(avg), *vals["ssim"], f"{tag} ssim", None if m is None else m[0].mean())
    l1, ss = L.l1_ssim(ta, tb)
    assert float(ss) == float(avg)                                   # the same kernel: the same bits
    LC.assert_scalar(float(l1), *vals["l1"], f"{tag} l1 of the pair")
    assert abs(float(l1) - float(vals["l1"][1])) < LC.L1_BAR and abs(float(ss) - float(vals["ssim"][1])) < LC.SSIM_BAR
    a4, b4 = (ta, tb) if ta.dim() == 4 else (ta[None], tb[None])
    l1_i, ss_i = L._L1Ssim.apply(a4, b4)
    LC.assert_scalar(_np(l1_i), *vals["l1_i"], f"{tag} l1 per image")
    assert np.array_equal(_np(ss_i).reshape(-1).astype(np.float64), per)
    if kind == "same":
        assert float(l1) == 0.0 and not _np(l1_i).any()
    # the zero-edit pair: stand-alone kernels on the first iteration, the fused pass from the second on
    saved = dict(L._PAIR)
    L._PAIR.update(fused=False, last=None, parked=None, unclaimed=0)
    try:
        for it in range(2):
            pa = ta.detach().clone().requires_grad_(True)
            pl1 = L.l1_loss_paired(pa, tb)
            assert L._PAIR["fused"] is (it == 1)
            pss = L.ssim_paired(pa, tb)
            LC.assert_scalar(float(pl1), *vals["l1"], f"{tag} paired l1 (iteration {it})")
            assert float(pss) == float(avg)
            (0.8 * pl1 - 0.2 * pss).backward()
            g32, g64 = LC.gradients(shape, kind, "mix", "a")
            mg = _model("ssim_grad", shape, kind, "mix")
            LC.assert_tensor(_np(pa.grad).reshape(shape), g32[0], g64[0], f"{tag} paired mix gradient (iteration {it})", kind == "same",
                             None if mg is None else mg[1])
    finally:
        L._PAIR.update(saved)


def _check_gradients(dev, shape, kind, a, b, tag):
    B = shape[0]
    configs = LC.CONFIGS_ANY + (LC.CONFIGS_BATCH if B > 1 else ())
    for wrt in ("a", "b", "ab"):
        for config in configs:
            ta, tb = _t(a, dev, "a" in wrt), _t(b, dev, "b" in wrt)
            _loss_of(config, ta, tb).backward()
            g32, g64 = LC.gradients(shape, kind, config, wrt)
            got = [t.grad for t, n in ((ta, "a"), (tb, "b")) if n in wrt]
            for i, n in enumerate(wrt):
                mg = _model("ssim_grad", shape, kind, config, n == "b")
                absolute = kind == "same"   # (the L1 part of an identical pair is exactly zero on both sides)
                LC.assert_tensor(_np(got[i]).reshape(shape), g32[i], g64[i], f"{tag} d {config} / d {n} (of {wrt})", absolute, None if mg is None else mg[1])
                if kind == "same" and config == "l1":
                    assert not _np(got[i]).any()


@pytest.mark.parametrize("kind", LC.VALUE_SETS)
@pytest.mark.parametrize("shape", LC.SSIM_SHAPES, ids=LC.shape_id)
def test_ssim_and_fused_pair_against_fp64(dev, shape, kind):
    """Every entry of loss.py on one shape and value set, values and gradients, against fp64 at the bars of tests/loss_cases.py.
    [1x1x1x1-same] asks for a gradient of exactly 0 (ref32 and fp64 give 0): what k_l1_ssim_fwd's quotients and the uncontracted last sum of
    k_l1_ssim_bwd are there for."""
    a, b = LC.pair(shape, kind)
    if shape[0] == 1:   # one image: (C,H,W) inputs, through the compiled host's node and through the Python twin
        for native in (True, False):
            with _host_side(native):
                tag = f"{LC.shape_id(shape)} {kind} {'native' if native else 'python'}"
                _check_values(dev, shape, kind, a[0], b[0], tag)
                _check_gradients(dev, shape, kind, a[0], b[0], tag)
    else:
        tag = f"{LC.shape_id(shape)} {kind}"
        _check_values(dev, shape, kind, a, b, tag)
        _check_gradients(dev, shape, kind, a, b, tag)


# ---- the C ABI directly ---------------------------------------------------------------------------------------------------------------------
def _banded(n, dev, lead=4, tail=8):
    """n floats inside a larger NaN-filled buffer -> (buffer, the slice)."""
    buf = torch.full((lead + n + tail,), float("nan"), device=dev)
    return buf, buf[lead:lead + n]


def _bands_intact(buf, n, lead=4):
    return bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all())


def test_c_abi_both_backward_forms_inside_nan_guard_bands(dev):
    shape = (2, 4, 17, 33)
    B, Cc, H, W = shape
    n = B * Cc * H * W
    a, b = LC.pair(shape, "wide")
    ta, tb = _t(a, dev), _t(b, dev)
    lib, stream = _lib.gls(), _lib.raw_stream(dev)
    scale = 1.0 / (Cc * H * W)
    nparts = int(lib.gls_partial_floats(B, Cc, H, W))
    sums_buf, sums = _banded(2 * B, dev)
    maps_buf, maps = _banded(3 * n, dev)
    part_buf, part = _banded(nparts, dev)
    rc = lib.gls_l1_ssim_forward(B, Cc, H, W, ta.data_ptr(), tb.data_ptr(), scale, sums.data_ptr(), maps.data_ptr(), part.data_ptr(), stream)
    assert rc == 0, _lib.gls_error()
    assert _bands_intact(sums_buf, 2 * B) and _bands_intact(maps_buf, 3 * n) and _bands_intact(part_buf, nparts)
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(maps).all())
    vals = LC.values(shape, "wide")
    got = _np(sums).reshape(B, 2).astype(np.float64)
    LC.assert_scalar(got[:, 0], *vals["l1_i"], "C ABI l1 per image")
    m = _model("ssim_value", shape, "wide", "ssim")
    LC.assert_scalar(got[:, 1], *vals["ssim_i"], "C ABI ssim per image", None if m is None else m[0])
    # an evaluation-only call (maps = NULL): the same sums, bit for bit
    sums2_buf, sums2 = _banded(2 * B, dev)
    rc = lib.gls_l1_ssim_forward(B, Cc, H, W, ta.data_ptr(), tb.data_ptr(), scale, sums2.data_ptr(), None, part.data_ptr(), stream)
    assert rc == 0, _lib.gls_error()
    assert torch.equal(sums2, sums) and _bands_intact(sums2_buf, 2 * B) and _bands_intact(part_buf, nparts)
    # the (B,2) backward and the split one with g_stride = 2
    g = torch.stack([_t(LC.weights(B), dev), _t(LC.weights2(B), dev)], dim=1).contiguous()
    d1_buf, d1 = _banded(n, dev)
    d2_buf, d2 = _banded(n, dev)
    rc = lib.gls_l1_ssim_backward(B, Cc, H, W, ta.data_ptr(), tb.data_ptr(), maps.data_ptr(), g.data_ptr(), scale, d1.data_ptr(), stream)
    assert rc == 0, _lib.gls_error()
    rc = lib.gls_l1_ssim_backward_split(B, Cc, H, W, ta.data_ptr(), tb.data_ptr(), maps.data_ptr(), g.data_ptr(), g.data_ptr() + 4, 2, scale,
                                        d2.data_ptr(), stream)
    assert rc == 0, _lib.gls_error()
    assert _bands_intact(d1_buf, n) and _bands_intact(d2_buf, n) and _bands_intact(maps_buf, 3 * n)
    assert bool(torch.isfinite(d1).all()) and torch.equal(d1, d2)
    g32, g64 = LC.gradients(shape, "wide", "weights_both", "a")
    mg = _model("ssim_grad", shape, "wide", "weights_both")
    LC.assert_tensor(_np(d1).reshape(shape), g32[0], g64[0], "C ABI d weights_both / d a", False, None if mg is None else mg[1])


# ---- plain L1 -------------------------------------------------------------------------------------------------------------------------------
def _l1_value_ok(v, r32, r64, what):
    LC.assert_scalar(v, r32, r64, what)
    assert abs(v - r64) < LC.L1_BAR * max(1.0, abs(r64)), (what, v, r64)


@pytest.mark.parametrize("n", LC.L1_SIZES)
def test_l1_value_and_gradient_at_every_size(dev, n):
    a, b = LC.l1_pair(n)
    r32, r64, grad = LC.l1_reference(n)
    tb = _t(b, dev)
    for native in (True, False):
        with _host_side(native):
            for seeded in (False, True):
                L.install_backward_seed(seeded)
                try:
                    ta = _t(a, dev, True)
                    v = L.l1_loss(ta, tb)
                    v.backward()
                    _l1_value_ok(float(v), r32, r64, f"l1 n={n} {'native' if native else 'python'} seeded={seeded}")
                    assert np.array_equal(_np(ta.grad), grad)
                finally:
                    L.install_backward_seed(False)
            # a buffer that is 16-byte aligned but not at the start of its allocation
            ba, bb = torch.empty(n + 8, device=dev), torch.empty(n + 8, device=dev)
            oa, ob = ba[4:4 + n].copy_(_t(a, dev)).requires_grad_(True), bb[4:4 + n].copy_(tb)
            v = L.l1_loss(oa, ob)
            (g,) = torch.autograd.grad(v, oa)
            _l1_value_ok(float(v), r32, r64, f"l1 n={n} offset buffer")
            assert np.array_equal(_np(g), grad)


@pytest.mark.parametrize("n", LC.L1_SWITCH)
def test_l1_at_the_switch_to_the_two_launch_form(dev, n):
    """n = 2^26 - 1 is the last size of the one-launch form, 2^26 the first of the two-launch one: generated and referenced on the device."""
    gen = torch.Generator(device=dev).manual_seed(n % 1000)
    a, b = torch.rand(n, device=dev, generator=gen), torch.rand(n, device=dev, generator=gen)
    r32 = float((a - b).abs().mean())
    r64 = float((a.double() - b.double()).abs_().mean())
    v = float(L.l1_loss(a, b))
    again = float(L.l1_loss(a, b))
    del a, b
    torch.cuda.empty_cache()
    _l1_value_ok(v, r32, r64, f"l1 n={n}")
    assert again == v


# ---- L1 values the kernel was never shown ---------------------------------------------------------------------------------------------------
def _ordinary(dev):
    g = np.random.default_rng(41)
    a, b = g.random(LC.ORDINARY_SHAPE, dtype=np.float32), g.random(LC.ORDINARY_SHAPE, dtype=np.float32)
    return _t(a, dev), _t(b, dev), LO.l1(a, b)


def _abnormal_call(dev, name, seeded):
    a, b = LC.abnormal_pair(name)
    r32, r64, grad = LC.abnormal_reference(name)
    L.install_backward_seed(seeded)
    try:
        ta = _t(a, dev, True)
        v = L.l1_loss(ta, _t(b, dev))
        v.backward()
    finally:
        L.install_backward_seed(False)
    what = f"l1 {name} seeded={seeded}"
    print(what, "kernel:", float(v), "torch:", r32, "fp64:", r64)
    assert LC.value_class(float(v)) == LC.value_class(r32), (what, float(v), r32)
    if np.isfinite(r32):
        LC.assert_scalar(float(v), r32, r64, what)
    assert np.array_equal(_np(ta.grad), grad), what


@pytest.mark.parametrize("name", LC.ABNORMAL)
def test_l1_outside_unit_range_has_torchs_class_and_leaves_the_stream_clean(dev, name):
    """NaN, +-inf, a sum past the fixed-point field: the loss has the class torch gives and a finite one is inside the bar; an ordinary [0,1) call
    afterwards returns the bits it returned before, on the same stream and on a side stream that saw the same abnormal calls."""
    oa, ob, ref = _ordinary(dev)
    for native in (True, False):
        with _host_side(native):
            first = float(L.l1_loss(oa, ob))
            assert abs(first - ref) < LC.L1_BAR
            for seeded in (False, True):
                _abnormal_call(dev, name, seeded)
                assert float(L.l1_loss(oa, ob)) == first
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                assert float(L.l1_loss(oa, ob)) == first
                for seeded in (False, True):
                    _abnormal_call(dev, name, seeded)
                    assert float(L.l1_loss(oa, ob)) == first
            side.synchronize()
            torch.cuda.current_stream(dev).wait_stream(side)
            assert float(L.l1_loss(oa, ob)) == first


# ---- statistics kernels ---------------------------------------------------------------------------------------------------------------------
def _two_ulp(got, want64):
    return np.all(np.abs(got.astype(np.float64) - want64) <= 2.0 * np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64))


@pytest.mark.parametrize("P", LC.STATS_P)
def test_add_densification_stats_against_fp64(dev, P):
    grad4, acc0, den0 = LC.stats_inputs(P)
    g4 = _t(grad4, dev)
    grads = {"(P,3)": g4[:, :3].contiguous(), "(P,2)": g4[:, :2].contiguous(), "(P,4)": g4, "t[:, :3] of (P,4)": g4[:, :3]}
    assert grads["t[:, :3] of (P,4)"].stride(0) == 4
    rnd = np.random.default_rng(P).random(P) < 0.5
    for fname, filt in (("none", np.zeros(P, bool)), ("all", np.ones(P, bool)), ("random", rnd)):
        want, dn = LC.add_stats_reference(grad4, filt, acc0, den0)
        for gname, g in grads.items():
            model = types.SimpleNamespace(xyz_gradient_accum=_t(acc0, dev), denom=_t(den0, dev))
            L.add_densification_stats(model, types.SimpleNamespace(grad=g), _t(filt, dev))
            acc, den = _np(model.xyz_gradient_accum), _np(model.denom)
            what = (P, fname, gname)
            assert np.array_equal(den, dn), what
            assert np.array_equal(acc[~filt], acc0[~filt]) and np.array_equal(den[~filt], den0[~filt]), what   # untouched rows keep their bits
            assert _two_ulp(acc, want), what
        # an index list as the filter: the reference's own lines
        model = types.SimpleNamespace(xyz_gradient_accum=_t(acc0, dev), denom=_t(den0, dev))
        L.add_densification_stats(model, types.SimpleNamespace(grad=grads["(P,3)"]), torch.nonzero(_t(filt, dev)).reshape(-1))
        assert np.array_equal(_np(model.denom), dn) and _two_ulp(_np(model.xyz_gradient_accum), want), (P, fname, "index list")


@pytest.mark.parametrize("P", LC.STATS_P)
def test_densification_stats_against_fp64(dev, P):
    grad4, acc0, den0 = LC.stats_inputs(P, seed=1)
    g = np.random.default_rng(P + 9)
    radii = g.integers(-3, 40, P).astype(np.int32)
    radii[::5] = 0
    mx0 = g.integers(0, 60, P).astype(np.float32)        # some stored maxima above the new radius
    assert P < 5 or ((mx0 > radii) & (radii > 0)).any()
    vg = np.ascontiguousarray(grad4[:, :3])
    mx, acc, den = _t(mx0, dev), _t(acc0, dev), _t(den0, dev)
    L.densification_stats(_t(radii, dev), _t(vg, dev), mx, acc, den)
    vis = radii > 0
    want, dn = LC.add_stats_reference(grad4, vis, acc0, den0)
    assert np.array_equal(_np(mx), np.where(vis, np.maximum(mx0, radii.astype(np.float32)), mx0))
    assert np.array_equal(_np(den), dn)
    assert np.array_equal(_np(acc)[~vis], acc0[~vis]) and _two_ulp(_np(acc), want)


def test_statistics_of_no_splats(dev):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    model = types.SimpleNamespace(xyz_gradient_accum=z(0, 1), denom=z(0, 1))
    L.add_densification_stats(model, types.SimpleNamespace(grad=z(0, 3)), z(0, dt=torch.bool))
    L.densification_stats(z(0, dt=torch.int32), z(0, 3), z(0), z(0, 1), z(0, 1))
    torch.cuda.synchronize()
    assert model.denom.shape == (0, 1)
