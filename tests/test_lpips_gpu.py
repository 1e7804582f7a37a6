"""GPU tests of the LPIPS kernels (include/glp.h, gaussianavatars_amd/lpips.py), bottom-up: the convolution alone against fp64 F.conv2d, the max
pool bit for bit, the head against fp64 with all-zero positions, the two nets against the reference's pins (tests/golden/lpips_pins.npz), and
the adoption in evaluate.py.  Every shape is tiny; cases, weights, the fp64 restatement and the bars: tests/lpips_cases.py.

Bars: CONV_BAR and SCALAR_BAR are 4 x the error torch's fp32 path has on the host against fp64 on the same cases (measured, not chosen).
Every test prints its figure before it asserts; the figures observed on an MI355X are tabulated in DESIGN.md section 20."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from gaussianavatars_amd import lpips

    return lpips


@pytest.fixture(scope="module")
def pins():
    return np.load(LC.PINS_PATH)


def _conv_err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


# ---- the convolution alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.CONV_CASES, ids=LC.conv_id)
def test_conv2d_with_bias_and_relu_against_fp64(case, dev, L):
    x, w, b = LC.make_conv_case(case)
    ref = LC.conv_ref(x, w, b, case[3], case[4], True)
    got = L.conv2d(torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev), case[3], case[4], relu=True)
    assert got.shape == ref.shape and got.dtype is torch.float32
    err = _conv_err(got, ref)
    print(LC.conv_id(case), "max|err| / max|out| =", err, "bar", LC.CONV_BAR)
    assert (ref == 0).any() and (ref > 0).any()                      # the ReLU cuts something and passes something
    assert err <= LC.CONV_BAR


def test_conv2d_epilogue_relu_off_and_bias_off(dev, L):
    case = LC.CONV_CASES[0]
    x, w, b = LC.make_conv_case(case)
    tx, tw, tb = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    raw = LC.conv_ref(x, w, b, case[3], case[4], False)
    assert (raw < -0.1).any()                                        # negative outputs are present
    got = L.conv2d(tx, tw, tb, case[3], case[4], relu=False)
    err = _conv_err(got, raw)
    print("relu off:", err)
    assert err <= LC.CONV_BAR and bool((got < -0.1).any())
    on = L.conv2d(tx, tw, tb, case[3], case[4], relu=True)
    assert torch.equal(on, torch.clamp_min(got, 0.0))               # the epilogue's ReLU is max(., 0) of the very same sums
    nob = L.conv2d(tx, tw, None, case[3], case[4], relu=False)
    err = _conv_err(nob, LC.conv_ref(x, w, np.zeros_like(b), case[3], case[4], False))
    print("bias off:", err)
    assert err <= LC.CONV_BAR and not torch.equal(nob, got)


def test_conv2d_1x1_and_a_packed_weight_is_reused(dev, L):
    g = np.random.default_rng(77)
    x = g.standard_normal((1, 5, 9, 7)).astype(np.float32)
    w = (g.standard_normal((64, 5, 1, 1)) * np.sqrt(2.0 / 5)).astype(np.float32)
    b = (0.05 * g.standard_normal(64)).astype(np.float32)
    tx, tw, tb = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    packed = L.pack_weights(tw)
    assert packed.numel() == 16 * 64 and bool((packed.reshape(16, 64)[5:] == 0).all()) and torch.equal(packed.reshape(16, 64)[:5], tw.reshape(64, 5).t())
    got = L.conv2d(tx, tw, tb, 1, 0, relu=True, packed=packed)
    err = _conv_err(got, LC.conv_ref(x, w, b, 1, 0, True))
    print("1x1:", err)
    assert err <= LC.CONV_BAR
    assert torch.equal(got, L.conv2d(tx, tw, tb, 1, 0, relu=True))   # same bits run to run


# ---- the max pool ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,H,W,Ho,Wo", LC.POOL_CASES)
def test_maxpool_is_torchs_bit_for_bit(k, s, H, W, Ho, Wo, dev, L):
    x = torch.from_numpy(np.random.default_rng(H * W).standard_normal((2, 5, H, W)).astype(np.float32)).to(dev)
    got = L.maxpool(x, k, s)
    assert tuple(got.shape) == (2, 5, Ho, Wo)
    assert torch.equal(got, F.max_pool2d(x, k, s)) and torch.equal(got.cpu(), F.max_pool2d(x.cpu(), k, s))


def test_zscore_puts_both_images_into_one_batch(dev, L):
    x, y = (torch.from_numpy(a).to(dev) for a in LC.make_inputs(2, 7, 5, 3))
    got = L.zscore(x, y)
    mean, std = (torch.tensor(v, device=dev)[None, :, None, None] for v in (LC.MEAN, LC.STD))
    ref = torch.cat([(x - mean) / std, (y - mean) / std], 0)
    assert got.shape == (4, 3, 7, 5)
    assert float((got - ref).abs().max()) <= 2.5e-7 * float(ref.abs().max())   # two fp32 roundings of either side


# ---- the head ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", LC.HEAD_CASES)
def test_head_against_fp64_with_all_zero_positions(C, dev, L):
    feat, lin = LC.make_head_case(C)
    assert not feat[0, :, 0, 0].any() and feat[2, :, 0, 0].any() and not feat[1, :, 4, 2].any() and not feat[3, :, 4, 2].any()
    ref = float(LC.head_ref(feat, lin))
    tf, tl = torch.from_numpy(feat).to(dev), torch.from_numpy(lin).to(dev)
    part = L.head(tf, tl)
    assert part.dtype is torch.float64 and part.numel() == 1      # 2 x 15 positions: one workgroup
    got = float(part.sum())
    print("head C =", C, "rel err", abs(got - ref) / ref, "bar", LC.SCALAR_BAR)
    assert np.isfinite(got) and abs(got - ref) <= LC.SCALAR_BAR * ref
    assert torch.equal(L.head(tf, tl), part)                       # identical bits on a second run
    same = torch.cat([tf[:2], tf[:2]], 0)
    assert float(L.head(same, tl).sum()) == 0.0                    # an identical pair, zero positions included: exactly 0, no NaN


# ---- the whole network against the reference's pins ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(L):
    return {name: L.Weights(net, *LC.make_weights(net, seed)) for name, (net, B, H, W, seed) in LC.NET_CASES.items()}


@pytest.mark.parametrize("name", list(LC.NET_CASES))
def test_network_reproduces_the_reference_pins(name, dev, L, nets, pins):
    net, B, H, W, seed = LC.NET_CASES[name]
    x, y = (torch.from_numpy(a).to(dev) for a in LC.make_inputs(B, H, W, seed))
    got = L.terms(x, y, net, nets[name])
    assert got.is_cuda and got.dtype is torch.float32 and got.shape == (6,)
    g = got.double().cpu().numpy()
    errs = np.abs(g[:5] - pins[name + "_terms"]) / pins[name + "_terms"]
    total = abs(g[5] - float(pins[name + "_total"])) / float(pins[name + "_total"])
    print(name, "rel err: terms", " ".join("%.1e" % e for e in errs), "total %.3e" % total, "bar", LC.SCALAR_BAR)
    assert errs.max() <= LC.SCALAR_BAR and total <= LC.SCALAR_BAR
    m = L.LPIPS(net, weights=nets[name])
    out = m(x, y)
    assert tuple(out.shape) == (1, 1, 1, 1) and float(out) == float(got[5])     # the module, and the same bits on a second run
    if B == 1:
        assert float(m(x[0], y[0])) == float(got[5])                             # (3,H,W) is accepted
    else:   # the batch-sum quirk: the result of a batch is the SUM of its pairs' results
        singles = sum(float(m(x[i:i + 1], y[i:i + 1])) for i in range(B))
        assert abs(singles - float(got[5])) <= 4e-7 * singles
    assert float(m(x, x.clone())) == 0.0                                          # x == y gives exactly 0.0
    composed = float(L.lpips_composed(x, y, net, nets[name]))                     # torch's convolution on the same GPU: inside the same bar
    assert abs(composed - float(pins[name + "_total"])) <= LC.SCALAR_BAR * float(pins[name + "_total"])


def test_result_is_forward_only_and_the_switch_takes_the_composed_path(dev, L, nets, monkeypatch):
    name = "alex_35x31_b2"
    net, B, H, W, seed = LC.NET_CASES[name]
    x, y = (torch.from_numpy(a).to(dev) for a in LC.make_inputs(B, H, W, seed))
    xg = x.clone().requires_grad_(True)
    out = L.terms(xg, y, net, nets[name])[5]
    assert out.requires_grad
    with pytest.raises(NotImplementedError, match="forward-only"):
        out.backward()
    fused = float(L.terms(x, y, net, nets[name])[5])
    from gaussianavatars_amd import _lib

    _lib.glp_profile_enable(True)
    try:
        monkeypatch.setenv("GAA_FUSED_LPIPS", "0")
        off = float(L.terms(x, y, net, nets[name])[5])
        assert _lib.glp_profile_read() == {}                                      # no kernel of ours ran
        monkeypatch.delenv("GAA_FUSED_LPIPS")
        L.terms(x, y, net, nets[name])
        ran = _lib.glp_profile_read()
    finally:
        _lib.glp_profile_enable(False)
    assert abs(off - fused) <= 2 * LC.SCALAR_BAR * fused
    assert sum(k for _, k in ran.values()) == 14 and ran["glp::k_head"][1] == 5 and ran["glp::k_finish"][1] == 1   # alex: 1 + 5 + 2 + 5 + 1 launches


# ---- evaluate with weights -------------------------------------------------------------------------------------------------------------------------
def test_evaluate_reports_lpips_and_leaves_the_other_figures_alone(dev, L):
    from gaussianavatars_amd import evaluate as E

    net, seed = "alex", 12
    views = [tuple(torch.from_numpy(a[0]).to(dev) for a in LC.make_inputs(1, 35, 31, s)) for s in (21, 22)]

    class View:
        def __init__(self, gt):
            self.original_image, self.timestep = gt, 0

    render = lambda view, gaussians, pipe, bg: {"render": view.render}
    cams = []
    for a, b in views:
        v = View(b)
        v.render = a * 1.2 - 0.1          # leaves [0,1]: the clamp of train.py:277 matters
        cams.append(v)

    def run():
        acc = E.MetricAccumulator(2, dev, lpips_net=net)
        for v in cams:
            acc.update(v.render, v.original_image)
        return acc, E.evaluate_views(object(), cams, None, None, render=render)

    L.clear_weights()
    assert not L.weights_available(net)
    acc0, ev0 = run()
    assert "lpips" not in acc0.result() and len(ev0) == 3 and acc0.per_view_lpips() is None
    try:
        L.load_weights(net, *LC.make_weights(net, seed))
        acc1, ev1 = run()
        singles = [float(L.lpips(torch.clamp(v.render, 0, 1), torch.clamp(v.original_image, 0, 1), net)) for v in cams]
    finally:
        L.clear_weights()
    r0, r1 = acc0.result(), acc1.result()
    assert all(r0[k] == r1[k] for k in ("l1", "psnr", "ssim", "n")) and torch.equal(acc0.per_view(), acc1.per_view())   # bit for bit
    assert ev1[:3] == ev0 and len(ev1) == 4
    want = (np.float64(np.float32(singles[0])) + np.float64(np.float32(singles[1]))) / 2
    assert singles[0] != singles[1] and r1["lpips"] == want and ev1[3] == want
    assert acc1.per_view_lpips().tolist() == singles
