"""GPU tests of the fused splat regularisers (include/grl.h, loss.splat_regularizers / regularization_losses) against the float64 reference
of their contract (tests/reg_ref.py).

Bars.  Gapped inputs (every norm and every exp at least 50 % away from its threshold): values within (log2(max(P, 2)) + 16) 2^-24 relative --
all terms are non-negative, each is a few ulp off, the pairwise sums add log2 P half-ulps; gradient elements within
64 2^-24 |g| / c max(1, max_j e_j) -- exp <= 2 ulp, amplified <= 3x by the subtraction under the gap, sqrt, one division and two products are
about 20 ulp.  Generic inputs (no gap): values within 1e-5 relative; gradient rows outside the band of 1e-3 relative around a threshold within
2e-3 |g| / c max(1, max_j e_j) (conditioning there <= 1e3), rows inside it bounded by |g| / c max(1, max_j e_j) (1 + 1e-5); the band holds <= 2 %
of the rows.  Measured on the MI355X over every gapped case of this file: values at most 5.8e-8 relative (0.04 of
their bar), gradient elements at most 0.064 of theirs; generic out-of-band rows at most 2.0e-6 of |g| / c max(1, max_j e_j), band share 0.47 %."""
import math
import types

import numpy as np
import pytest
import torch

from tests.reg_ref import band_rows, gapped_inputs, generic_inputs, reg_ref

pytestmark = pytest.mark.gpu
T_XYZ, T_S = 1.0, 0.6   # arguments/__init__.py:100-105
U = 2.0 ** -24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad)


def _raw(xyz, ls, vis, gx=1.0, gs=1.0, t_xyz=T_XYZ, t_s=T_S, scratch=None, want=(True, True)):
    """One grl_forward and one grl_backward on device tensors -> (out[4] on the host, d_xyz, d_scale).  gx / gs None: a NULL upstream."""
    from gaussianavatars_amd import _lib

    lib = _lib.grl()
    dev = xyz.device
    P = xyz.shape[0]
    stream = _lib.raw_stream(dev)
    if scratch is None:
        scratch = torch.zeros(int(lib.grl_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    out = torch.full((4,), 7.0, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.grl_forward(P, p(xyz), p(ls), p(vis), t_xyz, t_s, p(out), p(scratch), stream)
    assert rc == 0, lib.grl_last_error()
    tgx = None if gx is None else torch.tensor(float(gx), device=dev)
    tgs = None if gs is None else torch.tensor(float(gs), device=dev)
    dx = torch.full_like(xyz, float("nan")) if want[0] else None     # (every row of a requested output has to be written)
    ds = torch.full_like(ls, float("nan")) if want[1] else None
    rc = lib.grl_backward(P, p(xyz), p(ls), p(vis), t_xyz, t_s, p(out), p(tgx), p(tgs), p(dx), p(ds), stream)
    assert rc == 0, lib.grl_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), dx, ds


def _check_values(out, ref, P):
    bar = (math.log2(max(P, 2)) + 16) * U
    assert out[2] == ref["count"] and out[3] == 0.0
    rel = lambda got, want: abs(got - want) / want if want != 0 else (0.0 if got == 0 else float("inf"))   # (a one-splat case can be all zero)
    worst = max(rel(out[0], ref["xyz_mean"]), rel(out[1], ref["scale_mean"]))
    print(f"P={P}: values worst rel {worst:.2e} (bar {bar:.2e})")
    assert worst <= bar


def _row_scale(ref, g):
    return abs(g) / max(ref["count"], 1) * np.maximum(1.0, ref["e"].max(1))[:, None]


def _check_gapped_grads(dx, ds, ref, vis, gx, gs, P):
    ex = np.abs(dx.cpu().numpy().astype(np.float64) - ref["d_xyz"]) / (64 * U * _row_scale(ref, gx))
    es = np.abs(ds.cpu().numpy().astype(np.float64) - ref["d_scale"]) / (64 * U * _row_scale(ref, gs))
    print(f"P={P}: gradient worst / bar: xyz {ex.max():.3f} scale {es.max():.3f}")
    assert ex.max() <= 1.0 and es.max() <= 1.0
    # invisible rows and rows (elements) under the threshold: exactly zero
    tv = torch.from_numpy(vis)
    below = torch.from_numpy(ref["n"] <= T_XYZ)
    assert torch.equal(dx.cpu()[~tv | below], torch.zeros(int((~tv | below).sum()), 3))
    off = (~tv)[:, None] | torch.from_numpy(ref["e"] <= np.float32(T_S))
    assert torch.equal(ds.cpu()[off], torch.zeros(int(off.sum())))


# ---- gapped inputs, every shape ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 257, 4099, 70_001])
def test_gapped_inputs_against_the_reference(P):
    from gaussianavatars_amd import loss

    dev = _dev()
    xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=P)
    gx, gs = 0.37, -1.9
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S, gx, gs)
    txyz, tls, tvis = _t(xyz, dev), _t(ls, dev), _t(vis, dev)
    out, dx, ds = _raw(txyz, tls, tvis, gx, gs)
    _check_values(out, ref, P)
    _check_gapped_grads(dx, ds, ref, vis, gx, gs, P)
    # the Python entry: the same launches, the same bits
    a, b = txyz.clone().requires_grad_(True), tls.clone().requires_grad_(True)
    m_x, m_s = loss.splat_regularizers(a, b, tvis, T_XYZ, T_S)
    assert m_x.dim() == 0 and m_s.dim() == 0 and m_x.grad_fn is not None
    torch.autograd.backward([m_x, m_s], [torch.tensor(gx, device=dev), torch.tensor(gs, device=dev)])
    assert float(m_x.detach()) == out[0] and float(m_s.detach()) == out[1]
    assert torch.equal(a.grad, dx) and torch.equal(b.grad, ds)


def test_bases_that_are_only_4_byte_aligned():
    """buf[1:] of a (P + 1, 3) tensor (12 bytes past an aligned base) and a filter one byte past its base: the element-wise path."""
    dev = _dev()
    P = 4099
    xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=11)
    gx, gs = 1.0, 0.5
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S, gx, gs)
    bx, bl, bv = torch.zeros(P + 1, 3, device=dev), torch.zeros(P + 1, 3, device=dev), torch.zeros(P + 1, dtype=torch.bool, device=dev)
    bx[1:], bl[1:], bv[1:] = _t(xyz, dev), _t(ls, dev), _t(vis, dev)
    vx, vl, vv = bx[1:], bl[1:], bv[1:]
    assert vx.data_ptr() % 16 == 12 and vv.data_ptr() % 4 == 1 and vx.is_contiguous()
    out, dx, ds = _raw(vx, vl, vv, gx, gs)
    _check_values(out, ref, P)
    _check_gapped_grads(dx, ds, ref, vis, gx, gs, P)
    out2, dx2, ds2 = _raw(_t(xyz, dev), _t(ls, dev), _t(vis, dev), gx, gs)      # the 16-byte path: same arithmetic, same order
    assert np.array_equal(out, out2) and torch.equal(dx, dx2) and torch.equal(ds, ds2)
    # a mixed case: aligned inputs, unaligned filter only
    out3, dx3, _ = _raw(_t(xyz, dev), _t(ls, dev), vv, gx, gs)
    assert np.array_equal(out, out3) and torch.equal(dx, dx3)


def test_generic_inputs_mask_and_indexing():
    dev = _dev()
    P = 70_001
    xyz, ls, vis = generic_inputs(P, seed=0)
    gx, gs = 0.01, 1.0
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S, gx, gs)
    out, dx, ds = _raw(_t(xyz, dev), _t(ls, dev), _t(vis, dev), gx, gs)
    assert out[2] == ref["count"]
    assert abs(out[0] - ref["xyz_mean"]) <= 1e-5 * ref["xyz_mean"] and abs(out[1] - ref["scale_mean"]) <= 1e-5 * ref["scale_mean"]
    band = band_rows(ref, T_XYZ, T_S)
    assert band.mean() <= 0.02
    dx, ds = dx.cpu().numpy().astype(np.float64), ds.cpu().numpy().astype(np.float64)
    sx, ss = _row_scale(ref, gx), _row_scale(ref, gs)
    ex, es = np.abs(dx - ref["d_xyz"]) / sx, np.abs(ds - ref["d_scale"]) / ss
    print(f"generic: out-of-band worst / (|g|/c max(1,e)): xyz {ex[~band].max():.2e} scale {es[~band].max():.2e}; band share {band.mean():.4f}")
    assert ex[~band].max() <= 2e-3 and es[~band].max() <= 2e-3
    assert (np.abs(dx[band]) <= sx[band] * (1 + 1e-5)).all() and (np.abs(ds[band]) <= ss[band] * (1 + 1e-5)).all()
    assert not dx[~vis].any() and not ds[~vis].any()


# ---- hand cases, exact ----------------------------------------------------------------------------------------------------------------------
def test_hand_cases_are_exact():
    from gaussianavatars_amd import loss

    dev = _dev()
    t = 1.5
    low = torch.full((1, 3), -5.0, device=dev)
    for xyz, g, want_value, want_grad in (([[t, 0, 0]], 2.0, 0.0, [[0.0, 0.0, 0.0]]),           # at the threshold
                                          ([[2 * t, 0, 0]], 0.75, t, [[0.75, 0.0, 0.0]]),       # the only visible splat, twice the threshold
                                          ([[0, 0, 0]], 1.0, 0.0, [[0.0, 0.0, 0.0]])):          # the origin: zero, not NaN
        x = torch.tensor(xyz, dtype=torch.float32, device=dev, requires_grad=True)
        s = low.clone().requires_grad_(True)
        a, b = loss.splat_regularizers(x, s, torch.ones(1, dtype=torch.bool, device=dev), t, T_S)
        (g * a + b).backward()
        assert float(a) == want_value and float(b) == 0.0
        assert torch.equal(x.grad.cpu(), torch.tensor(want_grad)) and torch.equal(s.grad.cpu(), torch.zeros(1, 3))
    # all visible, several workgroups
    P = 2500
    xyz, ls, _ = gapped_inputs(P, T_XYZ, T_S, seed=5)
    vis = np.ones(P, bool)
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S)
    out, dx, ds = _raw(_t(xyz, dev), _t(ls, dev), _t(vis, dev))
    _check_values(out, ref, P)
    _check_gapped_grads(dx, ds, ref, vis, 1.0, 1.0, P)


def test_forward_of_an_empty_model_launches_nothing_and_writes_nan():
    from gaussianavatars_amd import _lib, loss

    dev = _dev()
    lib = _lib.grl()
    out = torch.full((4,), 7.0, device=dev)
    _lib.grl_profile_enable(True)
    assert lib.grl_forward(0, None, None, None, T_XYZ, T_S, out.data_ptr(), None, _lib.raw_stream(dev)) == 0
    torch.cuda.synchronize()
    assert _lib.grl_profile_read() == {}
    _lib.grl_profile_enable(False)
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[1]) and o[2] == 0.0 and o[3] == 0.0
    x, s = torch.zeros(0, 3, device=dev, requires_grad=True), torch.zeros(0, 3, device=dev, requires_grad=True)
    a, b = loss.splat_regularizers(x, s, torch.zeros(0, dtype=torch.bool, device=dev), T_XYZ, T_S)
    (a + b).backward()
    assert torch.isnan(a) and torch.isnan(b) and x.grad.shape == (0, 3) and s.grad.shape == (0, 3)


def test_nothing_visible_then_a_clean_call_on_the_same_scratch():
    from gaussianavatars_amd import _lib

    dev = _dev()
    P = 4099
    xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=7)
    txyz, tls = _t(xyz, dev), _t(ls, dev)
    scratch = torch.zeros(int(_lib.grl().grl_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    out, dx, ds = _raw(txyz, tls, torch.zeros(P, dtype=torch.bool, device=dev), scratch=scratch)
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 0.0
    assert torch.equal(dx, torch.zeros_like(dx)) and torch.equal(ds, torch.zeros_like(ds))
    assert int(scratch[:4].view(torch.int32)[0]) == 0          # the arrival word was reset
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S)
    out, dx, ds = _raw(txyz, tls, _t(vis, dev), scratch=scratch)
    _check_values(out, ref, P)
    _check_gapped_grads(dx, ds, ref, vis, 1.0, 1.0, P)


def test_non_finite_inputs_are_not_hidden():
    from gaussianavatars_amd import _lib

    dev = _dev()
    P = 4099
    xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=8)
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S)
    seen, hidden = int(np.nonzero(vis)[0][1500]), int(np.nonzero(~vis)[0][10])
    scratch = torch.zeros(int(_lib.grl().grl_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    tvis = _t(vis, dev)
    # +inf log-scale in a visible row: the scale mean is non-finite, the xyz mean is untouched
    bad = ls.copy()
    bad[seen, 1] = np.inf
    out, _, _ = _raw(_t(xyz, dev), _t(bad, dev), tvis, scratch=scratch)
    assert not np.isfinite(out[1]) and abs(out[0] - ref["xyz_mean"]) <= 1e-6 * ref["xyz_mean"] and out[2] == ref["count"]
    # NaN in a visible xyz row: the xyz mean is NaN
    badx = xyz.copy()
    badx[seen, 2] = np.nan
    out, _, _ = _raw(_t(badx, dev), _t(ls, dev), tvis, scratch=scratch)
    assert np.isnan(out[0]) and abs(out[1] - ref["scale_mean"]) <= 1e-6 * ref["scale_mean"]
    # the same in INVISIBLE rows: never read into a sum, gradients stay zero there
    badx, bad = xyz.copy(), ls.copy()
    badx[hidden], bad[hidden] = np.nan, np.inf
    out, dx, ds = _raw(_t(badx, dev), _t(bad, dev), tvis, scratch=scratch)
    _check_values(out, ref, P)
    assert not dx[hidden].any() and not ds[hidden].any()
    # and the following clean call on the same scratch is correct
    out, dx, ds = _raw(_t(xyz, dev), _t(ls, dev), tvis, scratch=scratch)
    _check_values(out, ref, P)
    _check_gapped_grads(dx, ds, ref, vis, 1.0, 1.0, P)


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_null_upstreams_and_unwanted_outputs():
    dev = _dev()
    P = 1500
    xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=9)
    args = (_t(xyz, dev), _t(ls, dev), _t(vis, dev))
    _, dx, ds = _raw(*args, 0.5, 2.0)
    _, dx0, ds1 = _raw(*args, None, 2.0)                       # a requested output whose upstream is NULL: zeros
    assert torch.equal(dx0, torch.zeros_like(dx0)) and torch.equal(ds1, ds)
    _, dx1, ds0 = _raw(*args, 0.5, None)
    assert torch.equal(ds0, torch.zeros_like(ds0)) and torch.equal(dx1, dx)
    _, dxo, none = _raw(*args, 0.5, 2.0, want=(True, False))   # an output that is not wanted
    assert none is None and torch.equal(dxo, dx)
    _, none, dso = _raw(*args, 0.5, 2.0, want=(False, True))
    assert none is None and torch.equal(dso, ds)


def _api(xyz, ls, vis, dev, wx=1.0, ws=1.0):
    from gaussianavatars_amd import loss

    a, b = _t(xyz, dev, True), _t(ls, dev, True)
    m_x, m_s = loss.splat_regularizers(a, b, _t(vis, dev), T_XYZ, T_S)
    (wx * m_x + ws * m_s).backward()
    return m_x.detach(), m_s.detach(), a.grad, b.grad


def test_two_identical_calls_give_identical_bits():
    dev = _dev()
    xyz, ls, vis = generic_inputs(70_001, seed=4)
    r1, r2 = _api(xyz, ls, vis, dev), _api(xyz, ls, vis, dev)
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)


def test_two_streams_in_one_process():
    from gaussianavatars_amd import loss

    dev = _dev()
    xyz, ls, vis = gapped_inputs(4099, T_XYZ, T_S, seed=12)
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S)
    base = _api(xyz, ls, vis, dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    got = []
    torch.cuda.synchronize()
    for s in streams:
        with torch.cuda.stream(s):
            got.append(_api(xyz, ls, vis, dev))
    torch.cuda.synchronize()
    keys = [k for k in loss._REG_SCRATCH if k[0] == dev.index]
    assert len({k[1] for k in keys}) >= 3                       # one scratch per stream, none shared
    assert len({loss._REG_SCRATCH[k].data_ptr() for k in keys}) == len(keys)
    for r in got:
        _check_values(np.array([float(r[0]), float(r[1]), ref["count"], 0.0]), ref, 4099)
        for u, v in zip(r, base):
            assert torch.equal(u, v)


def test_one_output_alone_and_lambda_scaling():
    from gaussianavatars_amd import loss

    dev = _dev()
    P = 1500
    xyz, ls, vis = gapped_inputs(P, T_XYZ, T_S, seed=13)
    ref = reg_ref(xyz, ls, vis, T_XYZ, T_S, 1e-2, 0.25)
    _, _, fx, fs = _api(xyz, ls, vis, dev, 1e-2, 0.25)          # lambdas through autograd
    _check_gapped_grads(fx, fs, ref, vis, 1e-2, 0.25, P)
    for which in (0, 1):
        a, b = _t(xyz, dev, True), _t(ls, dev, True)
        m = loss.splat_regularizers(a, b, _t(vis, dev), T_XYZ, T_S)
        ((1e-2, 0.25)[which] * m[which]).backward()
        mine, other = (a, b) if which == 0 else (b, a)
        assert torch.equal(mine.grad, fx if which == 0 else fs)
        assert other.grad is None or not other.grad.any()
    # a leaf that does not require a gradient gets none, the other is unchanged
    a, b = _t(xyz, dev, False), _t(ls, dev, True)
    m_x, m_s = loss.splat_regularizers(a, b, _t(vis, dev), T_XYZ, T_S)
    (1e-2 * m_x + 0.25 * m_s).backward()
    assert a.grad is None and torch.equal(b.grad, fs)
    # non-contiguous inputs are made contiguous
    wide = torch.zeros(P, 6, device=dev)
    wide[:, :3] = _t(xyz, dev)
    a = wide[:, :3].detach().requires_grad_(True)
    assert not a.is_contiguous()
    m_x, _ = loss.splat_regularizers(a, _t(ls, dev), _t(vis, dev), T_XYZ, T_S)
    (1e-2 * m_x).backward()
    assert torch.equal(a.grad, fx)


def test_in_place_edit_between_the_passes_raises():
    from gaussianavatars_amd import loss

    dev = _dev()
    xyz, ls, vis = gapped_inputs(257, T_XYZ, T_S, seed=14)
    a, b = _t(xyz, dev, True), _t(ls, dev, True)
    m_x, m_s = loss.splat_regularizers(a, b, _t(vis, dev), T_XYZ, T_S)
    with torch.no_grad():
        a.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (m_x + m_s).backward()


def test_graph_replay_gives_the_eager_bits():
    """Forward + backward recorded on one stream after an eager warm-up there: neither pass waits on the host or allocates outside torch."""
    from gaussianavatars_amd import loss

    dev = _dev()
    P = 4099
    xyz, ls, vis = generic_inputs(P, seed=15)
    eager = _api(xyz, ls, vis, dev, 1e-2, 1.0)
    a, b, v = _t(xyz, dev, True), _t(ls, dev, True), _t(vis, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        m_x, m_s = loss.splat_regularizers(a, b, v, T_XYZ, T_S)        # the warm-up: this stream's scratch is made here
        torch.autograd.grad(1e-2 * m_x + m_s, [a, b])
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        m_x, m_s = loss.splat_regularizers(a, b, v, T_XYZ, T_S)
        ga, gb = torch.autograd.grad(1e-2 * m_x + m_s, [a, b])
    for t in (m_x, m_s, ga, gb):
        t.detach().zero_()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip((m_x.detach(), m_s.detach(), ga, gb), eager):
        assert torch.equal(got, want)


def test_regularization_losses_on_a_rendered_mirror_model():
    """train.py:118-164 at a toy size: the gradients of sum(losses) are the render-only gradients plus the reference's regulariser gradients.
    Thresholds are the model's own medians (the synthetic head's local coordinates sit far below the reference's defaults), so there is no
    gap: the generic bars apply, plus 2^-23 (|render-only| + |total|) per element for autograd's fp32 accumulation of the two gradients."""
    import bench
    from gaussianavatars_amd import loss
    from gaussianavatars_amd.gaussian_renderer import render
    from gaussianavatars_amd.rasterizer import set_deterministic

    dev = _dev()
    g, cam = bench.build_scene(dev, 12_000, 3, 96, 64, 2, "fused", True)   # (the synthetic head wants a splat on each of its 10 144 faces)
    P = g._xyz.shape[0]
    xyz, ls = g._xyz.detach().cpu().numpy(), g._scaling.detach().cpu().numpy()
    opt = types.SimpleNamespace(lambda_xyz=0.5, threshold_xyz=float(np.median(np.linalg.norm(xyz, axis=1))), lambda_scale=2.0,
                                threshold_scale=float(np.median(np.exp(ls))), metric_xyz=False, metric_scale=False)
    bg = torch.ones(3, device=dev)
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(1)).to(dev)
    prev = set_deterministic(True)
    try:
        grads = {}
        for with_reg in (False, True):
            bench.zero_grads(g)
            g.select_mesh_by_timestep(0)
            pkg = render(cam, g, bench.Pipe, bg)
            vis = pkg["visibility_filter"]
            losses = {"l1": loss.l1_loss(pkg["render"], gt)}
            if with_reg:
                losses.update(loss.regularization_losses(g, vis, opt))
                assert list(losses) == ["l1", "xyz", "scale"]
            sum(losses.values()).backward()
            grads[with_reg] = (g._xyz.grad.double().cpu().numpy(), g._scaling.grad.double().cpu().numpy())
    finally:
        set_deterministic(prev)
    vis = vis.cpu().numpy()
    assert 100 < vis.sum() < P or vis.sum() == P
    rx = reg_ref(xyz, ls, vis, opt.threshold_xyz, opt.threshold_scale, opt.lambda_xyz, opt.lambda_scale)
    assert abs(float(losses["xyz"]) - opt.lambda_xyz * rx["xyz_mean"]) <= 1e-5 * opt.lambda_xyz * rx["xyz_mean"]
    assert abs(float(losses["scale"]) - opt.lambda_scale * rx["scale_mean"]) <= 1e-5 * opt.lambda_scale * rx["scale_mean"]
    band = band_rows(rx, opt.threshold_xyz, opt.threshold_scale)
    for (plain, total), want, lam in zip(zip(*grads.values()), (rx["d_xyz"], rx["d_scale"]), (opt.lambda_xyz, opt.lambda_scale)):
        scale = _row_scale(rx, lam)
        acc = 2.0 ** -23 * (np.abs(plain) + np.abs(total))
        err = np.abs((total - plain) - want)
        assert np.abs(want).max() > 0
        assert (err[~band] <= 2e-3 * scale[~band] + acc[~band]).all()
        assert (np.abs(total - plain)[band] <= scale[band] * (1 + 1e-5) + acc[band]).all()
