"""GPU tests of the evaluation and export kernels (include/gev.h) through gaussianavatars_amd/evaluate.py: the 8-bit frame against torch's bytes,
the pair statistics against tests/golden/eval_pins.npz at the fixture's shapes and at shapes chosen for the tiles, both PSNR conventions, the
device-resident accumulator, and the composed path behind GAA_FUSED_EVAL=0.  Bars: tests/eval_cases.py."""
import numpy as np
import pytest
import torch

import eval_cases as EC
from gaussianavatars_amd import _lib
from gaussianavatars_amd import evaluate as E

pytestmark = pytest.mark.gpu
ALL_CASES = list(EC.CASES) + list(EC.EXTRA)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.gev()
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
def test_to_u8_is_torchs_bytes_on_the_images(case):
    dev = _dev()
    a, b = EC.pair(case)
    ua, ub = E.to_u8(_t(a, dev)), E.to_u8(_t(b, dev))
    assert ua.dtype == torch.uint8 and ua.is_cuda and tuple(ua.shape) == EC.torch_bytes(a).shape
    assert np.array_equal(ua.cpu().numpy(), EC.torch_bytes(a)) and np.array_equal(ub.cpu().numpy(), EC.torch_bytes(b))
    if case in EC.CASES:
        assert np.array_equal(ua.cpu().numpy(), EC.PINS[case + "_a_u8"]) and np.array_equal(ub.cpu().numpy(), EC.PINS[case + "_b_u8"])
    two = E.to_u8(_t(a, dev), also=_t(b, dev))   # the second image of the same launch
    assert torch.equal(two[0], ua) and torch.equal(two[1], ub)


@pytest.mark.parametrize("shape", [(3, 25, 31), (3, 24, 36), (2, 3, 10, 20), (1, 5, 31), (4, 25, 31)])
def test_to_u8_boundary_sweep(shape):
    """Every value at which the byte changes, +-4 ulp: (3,25,31) holds the sweep exactly once with a width that is no multiple of 4 (one pixel per
    thread); (3,24,36) and the batch take the 16-byte path; one and four channels take the general one."""
    dev = _dev()
    v = EC.boundary_sweep()
    n = int(np.prod(shape))
    img = np.resize(v if n >= v.size else v[::-(-v.size // n)], n).reshape(shape)   # (a smaller image holds every second / fifteenth value)
    got = E.to_u8(_t(img, dev))
    want = EC.torch_bytes(img)
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:8]
    rev = np.ascontiguousarray(img.reshape(-1)[::-1].reshape(shape))
    both = E.to_u8(_t(img, dev), also=_t(rev, dev))
    assert np.array_equal(both[0].cpu().numpy(), want) and np.array_equal(both[1].cpu().numpy(), EC.torch_bytes(rev))


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", EC.TRANSFORMS)
@pytest.mark.parametrize("case", ALL_CASES)
def test_pair_statistics_against_the_reference(case, transform):
    dev = _dev()
    a, b = EC.pair(case)
    ta, tb = _t(a, dev), _t(b, dev)
    ref = EC.reference(case, transform)
    B = a.shape[0] if a.ndim == 4 else 1
    Cc, hw = a.shape[-3], float(a.shape[-2] * a.shape[-1])
    sums = E.plane_sums(ta, tb, transform)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (B * Cc, 3)
    s = sums.cpu().numpy().reshape(B, Cc, 3)
    assert abs(s[:, :, 0].sum() / (B * Cc * hw) - float(ref["l1"])) < EC.L1_BAR
    assert abs(s[:, :, 2].sum() / (B * Cc * hw) - float(ref["ssim"])) < EC.SSIM_BAR
    if case in EC.CASES:
        s64 = EC.PINS[f"{case}_{transform}_sums64"].reshape(B, Cc, 3)
        assert np.abs(s[:, :, 0] - s64[:, :, 0]).max() / hw < EC.L1_BAR and np.abs(s[:, :, 2] - s64[:, :, 2]).max() / hw < EC.SSIM_BAR
    EC.assert_new((s[:, :, 1] / hw).reshape(ref["mse3_64"].shape), ref["mse3"], ref["mse3_64"], (case, transform, "mse per channel"))
    EC.assert_new((s[:, :, 1].sum(1) / (Cc * hw)).reshape(ref["mse4_64"].shape), ref["mse4"], ref["mse4_64"], (case, transform, "mse per image"))
    # both PSNR conventions on the same pair, through the reducing launch
    for per_channel, key in ((True, "psnr3"), (False, "psnr4")):
        l1, ps, ss = E.frame_metrics(ta, tb, transform=transform, per_channel_psnr=per_channel)
        assert l1.is_cuda and l1.dtype == ps.dtype == ss.dtype == torch.float32 and l1.dim() == 0
        assert abs(float(l1) - float(ref["l1"])) < EC.L1_BAR and abs(float(ss) - float(ref["ssim"])) < EC.SSIM_BAR
        r32, r64 = ref[key], ref[key + "_64"]
        r32, r64 = (r32.reshape(B, -1).mean(1).mean(), r64.reshape(B, -1).mean(1).mean())
        EC.assert_new(float(ps), r32, r64, (case, transform, key))
    native = E.frame_metrics(ta, tb, transform=transform)   # None follows the reference: per channel for 3-D, per image for 4-D
    same = E.frame_metrics(ta, tb, transform=transform, per_channel_psnr=a.ndim == 3)
    assert all(x.equal(y) for x, y in zip(native, same))


@pytest.mark.parametrize("case", ALL_CASES)
def test_drop_in_psnr_has_the_references_rows(case):
    dev = _dev()
    a, b = EC.pair(case)
    ref = EC.reference(case, "raw")
    key = "psnr3" if a.ndim == 3 else "psnr4"
    out = E.psnr(_t(a, dev), _t(b, dev))
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (a.shape[0], 1)
    EC.assert_new(out.cpu().numpy(), ref[key], ref[key + "_64"], (case, "psnr()"))
    # and behind the zero-edit boundary: a device pair takes the kernels, through the rebound name
    import types

    from gaussianavatars_amd import patch

    mod = types.ModuleType("stand_in_image_utils")
    mod.psnr = lambda img1, img2: "original"
    patch.adopt_evaluation(mod)
    try:
        assert torch.equal(mod.psnr(_t(a, dev), _t(b, dev)), out) and mod.psnr(torch.from_numpy(a), torch.from_numpy(b)) == "original"
    finally:
        patch.unpatch_classes(mod)


@pytest.mark.parametrize("case", ALL_CASES)
def test_uint8_input_is_the_png8_transform_bit_for_bit(case):
    dev = _dev()
    a, b = EC.pair(case)
    ta, tb = _t(a, dev), _t(b, dev)
    ua, ub = E.to_u8(ta, also=tb)
    from_floats = E.plane_sums(ta, tb, "png8")
    assert torch.equal(E.plane_sums(ua, ub, "raw"), from_floats) and torch.equal(E.plane_sums(ua, ub, "clamp"), from_floats)
    assert torch.equal(E.plane_sums(ta, ub, "png8"), from_floats) and torch.equal(E.plane_sums(ua, tb, "png8"), from_floats)
    x, y = E.frame_metrics(ua, ub), E.frame_metrics(ta, tb, transform="png8")
    assert all(p.equal(q) for p, q in zip(x, y))


def test_identical_pair():
    dev = _dev()
    for case in ("chw", "bchw", "four_tiles"):
        ta = _t(EC.pair(case)[0], dev)
        for per_channel in (True, False):
            l1, ps, ss = E.frame_metrics(ta, ta.clone(), per_channel_psnr=per_channel)
            assert float(l1) == 0.0 and float(ps) == float("inf") and abs(float(ss) - 1.0) < EC.SSIM_BAR
        assert torch.isinf(E.psnr(ta, ta.clone())).all()


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------------
def _five(dev):
    pairs = [EC.pair(c) for c in ("chw", "small", "pixel", "one_tile", "four_tiles")]
    return [(_t(a, dev), _t(b, dev)) for a, b in pairs]


def test_accumulator_is_the_fp64_mean_of_the_single_calls_and_repeats_its_bits():
    dev = _dev()
    pairs = _five(dev)
    singles = torch.stack([torch.stack(E.frame_metrics(a, b)) for a, b in pairs])
    runs = []
    for _ in range(2):
        acc = E.MetricAccumulator(5, dev)
        for a, b in pairs:
            acc.update(a, b)
        runs.append((acc.per_view().clone(), acc.acc.clone(), acc.result()))
    table, sums, r = runs[0]
    assert torch.equal(table, singles)                                   # the rows are the single calls, bit for bit
    assert torch.equal(runs[1][0], table) and torch.equal(runs[1][1], sums)   # and a second run has the same bits
    assert r["n"] == 5 and float(sums[3]) == 5.0
    want = singles.double().mean(0).cpu()
    assert torch.isinf(want[1]) and r["psnr"] == float("inf")        # ("pixel" clamps one channel to an identical plane, as in the pins)
    for i, key in ((0, "l1"), (2, "ssim")):
        assert abs(r[key] - float(want[i])) <= 1e-12 * abs(float(want[i])), key
    # the PSNR mean over the finite views
    acc = E.MetricAccumulator(4, dev)
    for a, b in pairs[:2] + pairs[3:]:
        acc.update(a, b)
    keep = singles[[0, 1, 3, 4]].double().mean(0).cpu()
    r = acc.result()
    for i, key in enumerate(("l1", "psnr", "ssim")):
        assert np.isfinite(r[key]) and abs(r[key] - float(keep[i])) <= 1e-12 * abs(float(keep[i])), key
    with pytest.raises(IndexError):
        acc.update(*pairs[0])


def test_a_batch_fills_one_row_per_image():
    dev = _dev()
    a, b = (_t(x, dev) for x in EC.pair("bchw"))
    acc = E.MetricAccumulator(3, dev)
    acc.update(a[1], b[1], per_channel_psnr=False)
    acc.update(a, b)
    rows = torch.stack([torch.stack(E.frame_metrics(a[i][None], b[i][None])) for i in (1, 0, 1)])
    assert acc.n == 3 and torch.equal(acc.per_view(), rows)
    r = acc.result()
    assert r["n"] == 3 and abs(r["psnr"] - float(rows[:, 1].double().mean())) <= 1e-12 * r["psnr"]


def test_update_never_waits_for_the_device():
    """torch's sync debug mode raises on every synchronising call torch makes (a scalar read, a blocking copy); the library itself has no
    synchronising call to make (include/gev.h).  result() is the one read: it is what raises under the mode."""
    dev = _dev()
    pairs = _five(dev)
    acc = E.MetricAccumulator(5, dev)
    acc.update(*pairs[0])   # (first use: the library is mapped and the scratch pool warm before the mode is on)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for a, b in pairs[1:]:
            acc.update(a, b)
        E.frame_metrics(*pairs[0])
        E.psnr(*pairs[0])
        E.to_u8(*pairs[0][:1])
        acc.per_view()
        with pytest.raises(RuntimeError):
            acc.result()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert acc.result()["n"] == 5


def test_two_launches_per_pair_and_one_per_frame():
    dev = _dev()
    a, b = (_t(x, dev) for x in EC.pair("four_tiles"))
    _lib.gev_profile_enable(True)
    try:
        acc = E.MetricAccumulator(2, dev)
        acc.update(a, b)
        acc.update(a, b, transform="png8")
        E.to_u8(a, also=b)
        prof = _lib.gev_profile_read()
    finally:
        _lib.gev_profile_enable(False)
    assert {k: v[1] for k, v in prof.items()} == {"gev::k_pair_stats": 2, "gev::k_reduce_accumulate": 2, "gev::k_to_u8_any": 1}


# ---- the opt-out --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EC.CASES))
def test_gaa_fused_eval_0_takes_the_composed_path_and_agrees(case, monkeypatch):
    dev = _dev()
    a, b = EC.pair(case)
    ta, tb = _t(a, dev), _t(b, dev)
    ref = EC.reference(case, "clamp")
    fused = E.frame_metrics(ta, tb)
    fused_bytes = E.to_u8(ta)
    monkeypatch.setenv("GAA_FUSED_EVAL", "0")

    def refuse(*a, **k):
        raise AssertionError("the kernels were called with GAA_FUSED_EVAL=0")

    monkeypatch.setattr(E, "_accumulate", refuse)
    monkeypatch.setattr(_lib, "gev", refuse)
    l1, ps, ss = E.frame_metrics(ta, tb)
    assert l1.is_cuda and abs(float(l1) - float(ref["l1"])) < EC.L1_BAR and abs(float(ss) - float(ref["ssim"])) < EC.SSIM_BAR
    assert abs(float(l1) - float(fused[0])) < EC.L1_BAR and abs(float(ss) - float(fused[2])) < EC.SSIM_BAR
    key = "psnr3" if a.ndim == 3 else "psnr4"
    r32, r64 = ref[key].mean(), ref[key + "_64"].mean()
    EC.assert_new(float(ps), r32, r64, (case, "composed on the device", key))
    EC.assert_new(float(fused[1]), r32, r64, (case, "fused", key))
    assert torch.equal(E.to_u8(ta), fused_bytes)
    out = E.psnr(ta, tb)
    assert tuple(out.shape) == (a.shape[0], 1)
    acc = E.MetricAccumulator(1 if a.ndim == 3 else a.shape[0], dev)
    acc.update(ta, tb)
    assert abs(acc.result()["l1"] - float(l1)) < 1e-7
