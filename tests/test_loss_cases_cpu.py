"""CPU tests that hold the references of tests/loss_cases.py themselves: the fp64 composition against the numpy oracle and the reference's pins,
ref32's distance from it on every shape of the GPU parity tests, the float32 model of the kernels' summation order, and torch's own answers
for the L1 inputs outside [0,1)."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_oracle as LO

import loss_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = np.load(os.path.join(HERE, "golden", "loss_pins.npz"))


def _fp64(a, b):
    a4, b4 = (torch.from_numpy(np.ascontiguousarray(x if x.ndim == 4 else x[None])).double() for x in (a, b))
    a4.requires_grad_(True)
    f = LC.figures(a4, b4)
    (g_l1,) = torch.autograd.grad(f["l1"], a4, retain_graph=True)
    (g_ss,) = torch.autograd.grad(f["ssim"], a4)
    return f, g_l1.numpy().reshape(a.shape), g_ss.numpy().reshape(a.shape)


@pytest.mark.parametrize("case", ["chw", "bchw", "tiny"])
def test_fp64_reference_agrees_with_the_oracle_and_the_pins(case):
    a, b = PINS[f"{case}_a"], PINS[f"{case}_b"]
    f, g_l1, g_ss = _fp64(a, b)
    l1, ss = float(f["l1"].detach()), float(f["ssim"].detach())
    # the numpy oracle is the same fp64 arithmetic in another order
    assert abs(l1 - LO.l1(a, b)) < 1e-15 and abs(ss - LO.ssim(a, b)) < 1e-13
    assert np.abs(g_ss - LO.ssim_grad(a, b)).max() < 1e-12 * np.abs(g_ss).max()
    np.testing.assert_array_equal(g_l1, LO.l1_grad(a, b))
    # the pins, at the bars of tests/test_loss_cpu.py
    assert abs(l1 - float(PINS[f"{case}_l1"])) < 2e-6
    assert abs(ss - float(PINS[f"{case}_ssim"])) < 2e-5
    np.testing.assert_allclose(g_l1, PINS[f"{case}_g_l1"], rtol=1e-5, atol=1e-9)
    ref = PINS[f"{case}_g_ssim"]
    assert np.abs(g_ss - ref).max() < 2e-4 * np.abs(ref).max()
    if a.ndim == 4:
        np.testing.assert_allclose(f["ssim_i"].detach().numpy(), PINS[f"{case}_ssim_per_image"], rtol=0, atol=2e-5)


@pytest.mark.parametrize("shape", LC.SSIM_SHAPES, ids=LC.shape_id)
def test_ref32_distance_is_nonzero_and_four_times_it_is_far_below_the_old_bar(shape):
    """The bar of the GPU parity tests on every shape: 4 x ref32's distance is not zero and is below 3e-5 of the gradient's maximum, an order of
    magnitude under the 3e-4 of tests/test_loss_gpu.py."""
    for kind in ("uniform", "wide"):
        g32, g64 = LC.gradients(shape, kind, "ssim", "a")
        own, top = np.abs(g32[0] - g64[0]).max(), np.abs(g64[0]).max()
        print(LC.shape_id(shape), kind, "ref32 distance / max:", own / top)
        assert own > 0.0
        assert 4.0 * own < 3e-5 * top
        assert LC.tensor_bar(g32[0], g64[0]) < 3e-5 * top


@pytest.mark.parametrize("shape", [(1, 3, 17, 33), (2, 4, 17, 33), (1, 2, 5, 7)], ids=LC.shape_id)
def test_kernel_model_is_the_same_function(shape):
    """The float32 model of the kernels' summation order computes the reference's SSIM and gradient: within 1e-5 of the maximum of fp64."""
    a, b = LC.pair(shape, "wide")
    B = shape[0]
    ss, d = LC.kernel_model(a, b, LC.weights(B), LC.weights2(B))
    np.testing.assert_allclose(ss, LC.values(shape, "wide")["ssim_i"][1], rtol=0, atol=2e-6)
    if B > 1:
        _, g64 = LC.gradients(shape, "wide", "weights_both", "a")
        assert np.abs(d - g64[0]).max() < 1e-5 * np.abs(g64[0]).max()


def test_identical_pair_reference():
    for shape in LC.SSIM_SHAPES:
        v = LC.values(shape, "same")
        assert np.all(v["l1_i"][1] == 0.0) and np.all(np.abs(v["ssim_i"][1] - 1.0) < 1e-12)
        g32, g64 = LC.gradients(shape, "same", "l1", "a")
        assert not g32[0].any() and not g64[0].any()


def test_seam_mask():
    m = LC.seam_mask((1, 1, 33, 65))[0, 0]
    assert m[:, :5].all() and m[:5].all() and m[:, 27:37].all() and m[11:21].all() and m[:, 60:].all() and m[28:].all()
    assert not m[5:11, 5:27].any() and not m[21:27, 37:59].any()


@pytest.mark.parametrize("name", LC.ABNORMAL)
def test_abnormal_l1_expectations_are_torchs_own(name):
    v, v64, g = LC.abnormal_reference(name)
    a, b = LC.abnormal_pair(name)
    want = {"nan_first": "nan", "nan_tail": "nan", "nan_last_group": "nan", "pos_inf": "+inf", "neg_inf": "+inf", "inf_minus_inf": "nan",
            "overflow_3e38": "+inf"}.get(name, "finite")
    assert LC.value_class(v) == want, (name, v)
    d = a - b
    assert g.shape == a.shape and np.array_equal(g[np.isnan(d)], np.zeros(int(np.isnan(d).sum()), np.float32))   # torch: sign(nan) = 0
    ok = ~np.isnan(d)
    assert np.array_equal(g[ok], (np.sign(d[ok]) * np.float32(1.0 / a.size)).astype(np.float32))
    if name == "sum_4e8":
        assert v64 * a.size > 2.0 ** 26 * 4
    if name == "near_100":
        assert v64 * a.size > 2.0 ** 26
    if name == "overflow_3e38":
        assert np.isfinite(v64) and np.isfinite(a).all()


def test_l1_references_and_sizes():
    assert 4 * 1024 * 255 in LC.L1_SIZES and LC.L1_SWITCH == (2 ** 26 - 1, 2 ** 26)
    for n in LC.L1_SIZES[:11]:
        r32, r64, g = LC.l1_reference(n)
        a, b = LC.l1_pair(n)
        assert abs(r64 - LO.l1(a, b)) < 1e-15 and abs(r32 - r64) < 2e-6
        np.testing.assert_array_equal(g, LO.l1_grad(a, b).astype(np.float32))


def test_add_stats_reference_equals_the_oracle_for_radii_filter():
    grad4, acc, den = LC.stats_inputs(257)
    radii = np.random.default_rng(5).integers(-2, 3, 257).astype(np.int32)
    want, dn = LC.add_stats_reference(grad4, radii > 0, acc, den)
    _, acc_o, den_o = LO.densification_stats(radii, grad4[:, :3], np.zeros(257, np.float32), acc.ravel(), den.ravel())
    np.testing.assert_array_equal(den_o, dn.ravel())
    np.testing.assert_allclose(acc_o, want.ravel(), rtol=1.2e-7, atol=0)
