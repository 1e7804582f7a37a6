"""GPU tests of the fused metric-space regularisers (include/gms.h, loss.metric_regularizers / regularization_losses) against the float64
reference of their contract (tests/metric_reg_ref.py).

The bar, for the two means, for every row of d_xyz and d_log_scaling (relative to the row's largest reference magnitude) and for every face
of d_face_scaling: the error against float64 is no larger than max(2 x the error of the reference's composed fp32 torch lines on the same
device and inputs against the same float64, 4 ulp of the value).  The yardstick is the composed path, never the kernel under test.  The
composed lines run with torch's deterministic algorithms (their index_put is then a fixed-order sum, so the yardstick does not move between
runs) and see the invisible rows' NaN replaced by 0: torch's backward multiplies the masked-out zero gradient by the row, and 0 * NaN would
poison face_scaling's gradient; the fused call gets the NaN."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.metric_reg_ref import CASES, case_id, metric_case, metric_ref, scale_band

pytestmark = pytest.mark.gpu
GX, GS = 0.37, 1.9   # upstream gradients of the two means (same sign: a face's two shares do not cancel)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(x, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(grad)


def _composed(xyz, ls, fs, binding, vis, t_xyz, t_s):
    """train.py:136 and :143 without their lambdas; get_scaling is exp(_scaling) * face_scaling[binding]."""
    a = F.relu((xyz * fs[binding])[vis] - t_xyz).norm(dim=1).mean()
    b = F.relu((torch.exp(ls) * fs[binding])[vis] - t_s).norm(dim=1).mean()
    return a, b


def _run_composed(c, dev, gx=GX, gs=GS):
    clean = lambda a: np.where(c["vis"][:, None], a, np.float32(0)).astype(np.float32)
    x, l, f = _t(clean(c["xyz"]), dev, True), _t(clean(c["ls"]), dev, True), _t(c["fs"][:, None], dev, True)
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        a, b = _composed(x, l, f, _t(c["binding"], dev).long(), _t(c["vis"], dev), c["t_xyz"], c["t_s"])
        if c["vis"].any():
            (gx * a + gs * b).backward()
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return [v.detach().double().cpu().numpy() for v in (a, b, z(x), z(l), z(f).reshape(-1))]


def _run_fused(c, dev, gx=GX, gs=GS, want=(True, True), face_grad=True, tensors=None):
    from gaussianavatars_amd import loss

    x, l, f, b, v = tensors or (_t(c["xyz"], dev), _t(c["ls"], dev), _t(c["fs"][:, None], dev), _t(c["binding"], dev), _t(c["vis"], dev))
    x, l, f = x.detach().requires_grad_(True), l.detach().requires_grad_(True), f.detach().requires_grad_(face_grad)
    mx, ms = loss.metric_regularizers(x, l, f, b, v, c["t_xyz"], c["t_s"], want_xyz=want[0], want_scale=want[1])
    outs = [(m, g) for m, g in ((mx, gx), (ms, gs)) if m is not None]
    assert all(m.dim() == 0 and m.grad_fn is not None for m, _ in outs)
    torch.autograd.backward([m for m, _ in outs], [torch.tensor(g, device=dev) for _, g in outs])
    torch.cuda.synchronize()
    return mx, ms, x.grad, l.grad, f.grad


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _check(name, mine, comp, ref, scale=None):
    """err(mine) <= max(2 err(composed), 4 ulp of `scale` (default: the value)), elementwise; prints the worst ratio first."""
    scale = np.abs(ref) if scale is None else scale
    em, ec = np.abs(mine - ref), np.abs(comp - ref)
    bar = np.maximum(2 * ec, 4 * _ulp(scale))
    ratio = np.max(em / bar) if em.size else 0.0
    print(f"{name}: worst error / bar {ratio:.3f}; worst error in ulp of the scale: fused {np.max(em / _ulp(scale), initial=0):.2f} composed {np.max(ec / _ulp(scale), initial=0):.2f}")
    assert (em <= bar).all(), name


# ---- every shape against float64 and the composed yardstick ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_means_and_gradients_against_float64(case):
    dev = _dev()
    P, nf, opt = case
    c = metric_case(P, nf, **opt)
    ref = metric_ref(c["xyz"], c["ls"], c["fs"], c["binding"], c["vis"], c["t_xyz"], c["t_s"], GX, GS)
    ca, cb, cdx, cds, cdf = _run_composed(c, dev)
    mx, ms, dx, ds, df = _run_fused(c, dev)
    again = _run_fused(c, dev)
    for u, v in zip((mx, ms, dx, ds, df), again):                       # two calls: identical bits, d_face_scaling included
        assert torch.equal(u.detach(), v.detach()) or (torch.isnan(u).all() and torch.isnan(v).all())
    assert df.shape == (nf, 1)
    a, b = float(mx.detach()), float(ms.detach())
    dx, ds, df = (t.double().cpu().numpy() for t in (dx, ds, df.reshape(-1)))
    empty = np.bincount(c["binding"], minlength=nf) == 0
    if ref["count"] == 0:
        assert np.isnan(a) and np.isnan(b) and np.isnan(ca) and np.isnan(cb)
        assert not dx.any() and not ds.any() and not df.any() and not np.signbit(dx).any() and not np.signbit(ds).any() and not np.signbit(df).any()
        return
    _check("xyz_mean", np.array(a), ca, np.array(ref["xyz_mean"]))
    _check("scale_mean", np.array(b), cb, np.array(ref["scale_mean"]))
    _check("d_xyz", dx, cdx, ref["d_xyz"], np.abs(ref["d_xyz"]).max(1, keepdims=True))
    _check("d_log_scaling", ds, cds, ref["d_scale"], np.abs(ref["d_scale"]).max(1, keepdims=True))
    _check("d_face_scaling", df, cdf, ref["d_face"])
    # zeros: +0.0, where composed torch has its zeros (d_log_scaling: outside the 2-ulp band of the threshold, which holds <= 1 % of the entries)
    assert np.array_equal(dx == 0, cdx == 0) and not np.signbit(dx[dx == 0]).any()
    band = scale_band(c, ref)
    assert band.sum() <= 0.01 * 3 * P
    assert np.array_equal((ds == 0)[~band], (cds == 0)[~band]) and not np.signbit(ds[ds == 0]).any()
    assert not dx[~c["vis"]].any() and not ds[~c["vis"]].any()           # the NaN of invisible rows reached nothing
    assert np.isfinite(a) and np.isfinite(b) and np.isfinite(df).all()
    assert not df[empty].any() and not np.signbit(df[empty]).any()      # faces without splats: exactly +0.0
    if nf >= 3:
        assert empty.any()


def test_bases_that_are_only_4_byte_aligned():
    """Row 1 onwards of buffers one row longer: xyz and log-scales 12 bytes, an int32 binding 4 bytes and the filter 1 byte past an aligned
    base -- the element-wise path, with the bits of the 16-byte path."""
    dev = _dev()
    P, nf = 1025, 7
    c = metric_case(P, nf, index_dtype=np.int32)
    base = _run_fused(c, dev)
    bx, bl = torch.zeros(P + 1, 3, device=dev), torch.zeros(P + 1, 3, device=dev)
    bb, bv = torch.zeros(P + 1, dtype=torch.int32, device=dev), torch.zeros(P + 1, dtype=torch.bool, device=dev)
    bx[1:], bl[1:], bb[1:], bv[1:] = _t(c["xyz"], dev), _t(c["ls"], dev), _t(c["binding"], dev), _t(c["vis"], dev)
    views = (bx[1:], bl[1:], _t(c["fs"][:, None], dev), bb[1:], bv[1:])
    assert views[0].data_ptr() % 16 == 12 and views[3].data_ptr() % 16 == 4 and views[4].data_ptr() % 4 == 1 and views[0].is_contiguous()
    got = _run_fused(c, dev, tensors=views)
    for u, v in zip(got, base):
        assert torch.equal(u.detach(), v.detach())
    # int64 binding, 8 bytes past an aligned base, and only the filter unaligned
    b64 = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    b64[1:] = _t(c["binding"], dev).long()
    for views in ((_t(c["xyz"], dev), _t(c["ls"], dev), _t(c["fs"][:, None], dev), b64[1:], _t(c["vis"], dev)),
                  (_t(c["xyz"], dev), _t(c["ls"], dev), _t(c["fs"][:, None], dev), _t(c["binding"], dev), bv[1:])):
        for u, v in zip(_run_fused(c, dev, tensors=views), base):
            assert torch.equal(u.detach(), v.detach())


def _profiled(fn):
    from gaussianavatars_amd import _lib

    _lib.gms_profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, _lib.gms_profile_read()
    finally:
        _lib.gms_profile_enable(False)


def test_terms_alone_and_launch_counts():
    """Each term alone has the bits it has in the joint call and costs one forward launch; the face sum is launched only when face_scaling
    wants a gradient; the library has three kernels in all."""
    dev = _dev()
    c = metric_case(3000, 40)
    (mx, ms, dx, ds, df), prof = _profiled(lambda: _run_fused(c, dev))
    assert len(prof) <= 3 and sorted(k.split("::")[-1] for k in prof) == ["k_metric_bwd", "k_metric_faces", "k_metric_fwd"], prof
    assert all(n == 1 for _, n in prof.values())
    (ax, none, adx, ads, adf), prof = _profiled(lambda: _run_fused(c, dev, want=(True, False)))
    assert none is None and torch.equal(ax, mx) and torch.equal(adx, dx) and ads is None
    assert sorted((k.split("::")[-1], n) for k, (_, n) in prof.items()) == [("k_metric_bwd", 1), ("k_metric_faces", 1), ("k_metric_fwd", 1)]
    (none, bs, bdx, bds, bdf), prof = _profiled(lambda: _run_fused(c, dev, want=(False, True)))
    assert none is None and torch.equal(bs, ms) and torch.equal(bds, ds) and bdx is None
    # the two shares of the face gradient: each rounded once from a double, their sum is the joint one to an ulp of the larger share
    both = adf.double() + bdf.double()
    assert ((both - df.double()).abs() <= 2.0 ** -22 * torch.maximum(adf.abs(), bdf.abs()).double()).all()
    # face_scaling without a gradient: no CSR, no second launch, the same per-splat gradients
    (_, _, ndx, nds, ndf), prof = _profiled(lambda: _run_fused(c, dev, face_grad=False))
    assert ndf is None and torch.equal(ndx, dx) and torch.equal(nds, ds)
    assert sorted(k.split("::")[-1] for k in prof) == ["k_metric_bwd", "k_metric_fwd"], prof


def test_csr_is_reused_and_rebuilt_after_the_binding_changed():
    from gaussianavatars_amd import binding as gbinding
    from gaussianavatars_amd import loss

    dev = _dev()
    c = metric_case(1025, 7, index_dtype=np.int64)
    t = (_t(c["xyz"], dev), _t(c["ls"], dev), _t(c["fs"][:, None], dev), _t(c["binding"], dev), _t(c["vis"], dev))
    base = _run_fused(c, dev, tensors=t)
    held = loss._METRIC_CSR[dev.index]
    assert held[1].data_ptr() == t[3].data_ptr()
    _run_fused(c, dev, tensors=t)
    assert loss._METRIC_CSR[dev.index] is held                            # the same binding: the same CSR object
    # a caller's own CSR gives the same bits
    x, l, f = (u.detach().requires_grad_(True) for u in t[:3])
    mx, ms = loss.metric_regularizers(x, l, f, t[3], t[4], c["t_xyz"], c["t_s"], csr=gbinding.binding_csr(t[3], 7))
    torch.autograd.backward([mx, ms], [torch.tensor(GX, device=dev), torch.tensor(GS, device=dev)])
    assert torch.equal(f.grad, base[4])
    with pytest.raises(RuntimeError, match="binding CSR does not match"):
        loss.metric_regularizers(x, l, f, t[3], t[4], c["t_xyz"], c["t_s"], csr=gbinding.binding_csr(t[3][:100], 7))
    # an in-place change of the binding (what a densification's prune leaves behind): rebuilt, and right
    with torch.no_grad():
        t[3].copy_(torch.roll(t[3], 1))
    c2 = dict(c, binding=np.roll(c["binding"], 1))
    got = _run_fused(c2, dev, tensors=t)
    assert loss._METRIC_CSR[dev.index] is not held
    x, l, f = (u.detach().requires_grad_(True) for u in t[:3])
    mx, ms = loss.metric_regularizers(x, l, f, t[3], t[4], c2["t_xyz"], c2["t_s"], csr=gbinding.binding_csr(t[3], 7))   # a fresh CSR: the same bits
    torch.autograd.backward([mx, ms], [torch.tensor(GX, device=dev), torch.tensor(GS, device=dev)])
    assert torch.equal(f.grad, got[4]) and not torch.equal(got[4], base[4])
    # a strided binding is keyed as the caller holds it: the second call finds the first one's CSR
    wide = torch.stack([t[3], t[3]], 1)[:, 0]
    assert not wide.is_contiguous()
    first = _run_fused(c2, dev, tensors=(t[0], t[1], t[2], wide, t[4]))
    held = loss._METRIC_CSR[dev.index]
    again = _run_fused(c2, dev, tensors=(t[0], t[1], t[2], wide, t[4]))
    assert loss._METRIC_CSR[dev.index] is held and torch.equal(first[4], got[4]) and torch.equal(again[4], got[4])


def test_no_host_wait():
    dev = _dev()
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available")
    from gaussianavatars_amd import loss

    c = metric_case(3000, 40)
    t = (_t(c["xyz"], dev), _t(c["ls"], dev), _t(c["fs"][:, None], dev), _t(c["binding"], dev), _t(c["vis"], dev))
    base = _run_fused(c, dev, tensors=t)                                  # warm-up: library, scratch and the binding's CSR are made here
    x, l, f = (u.detach().requires_grad_(True) for u in t[:3])
    ups = [torch.tensor(GX, device=dev), torch.tensor(GS, device=dev)]
    torch.cuda.synchronize()
    was = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mx, ms = loss.metric_regularizers(x, l, f, t[3], t[4], c["t_xyz"], c["t_s"])
        torch.autograd.backward([mx, ms], ups)
    finally:
        torch.cuda.set_sync_debug_mode(was)
    torch.cuda.synchronize()
    for u, v in zip((mx, ms, x.grad, l.grad, f.grad), base):
        assert torch.equal(u.detach(), v.detach())


def test_graph_replay_gives_the_eager_bits():
    """Forward + backward recorded on one stream after an eager warm-up there, replayed twice."""
    from gaussianavatars_amd import loss

    dev = _dev()
    c = metric_case(3000, 40)
    t = (_t(c["xyz"], dev), _t(c["ls"], dev), _t(c["fs"][:, None], dev), _t(c["binding"], dev), _t(c["vis"], dev))
    eager = _run_fused(c, dev, tensors=t)
    x, l, f = (u.detach().requires_grad_(True) for u in t[:3])
    ups = [torch.tensor(GX, device=dev), torch.tensor(GS, device=dev)]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        mx, ms = loss.metric_regularizers(x, l, f, t[3], t[4], c["t_xyz"], c["t_s"])   # the warm-up: this stream's scratch is made here
        torch.autograd.grad([mx, ms], [x, l, f], ups)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mx, ms = loss.metric_regularizers(x, l, f, t[3], t[4], c["t_xyz"], c["t_s"])
        gx, gl, gf = torch.autograd.grad([mx, ms], [x, l, f], ups)
    for u in (mx, ms, gx, gl, gf):
        u.detach().zero_()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip((mx, ms, gx, gl, gf), eager):
        assert torch.equal(got.detach(), want.detach())


def test_in_place_edit_between_the_passes_raises():
    from gaussianavatars_amd import loss

    dev = _dev()
    c = metric_case(255, 7)
    x, l, f = _t(c["xyz"], dev, True), _t(c["ls"], dev, True), _t(c["fs"][:, None], dev, True)
    mx, ms = loss.metric_regularizers(x, l, f, _t(c["binding"], dev), _t(c["vis"], dev), c["t_xyz"], c["t_s"])
    with torch.no_grad():
        f.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (mx + ms).backward()


def test_empty_model():
    from gaussianavatars_amd import loss

    dev = _dev()
    x, l = torch.zeros(0, 3, device=dev, requires_grad=True), torch.zeros(0, 3, device=dev, requires_grad=True)
    f = torch.full((5, 1), 0.7, device=dev, requires_grad=True)
    (mx, ms), prof = _profiled(lambda: loss.metric_regularizers(x, l, f, torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.bool, device=dev), 0.1, 0.4))
    (mx + ms).backward()
    assert prof == {} and torch.isnan(mx) and torch.isnan(ms)
    assert x.grad.shape == (0, 3) and l.grad.shape == (0, 3) and torch.equal(f.grad, torch.zeros_like(f))


# ---- the drop-in and a real model --------------------------------------------------------------------------------------------------------------
def test_regularization_losses_mixes_metric_and_local_terms():
    from gaussianavatars_amd import loss

    dev = _dev()
    c = metric_case(3000, 40)
    mk = lambda: types.SimpleNamespace(_xyz=_t(c["xyz"], dev, True), _scaling=_t(c["ls"], dev, True), face_scaling=_t(c["fs"][:, None], dev, True),
                                       binding=_t(c["binding"], dev))
    vis = _t(c["vis"], dev)
    for mx, ms in ((True, True), (True, False), (False, True)):
        opt = types.SimpleNamespace(lambda_xyz=0.5, threshold_xyz=c["t_xyz"], lambda_scale=2.0, threshold_scale=c["t_s"], metric_xyz=mx, metric_scale=ms)
        g, h = mk(), mk()
        got = loss.regularization_losses(g, vis, opt)
        assert list(got) == ["xyz", "scale"]
        sum(got.values()).backward()
        m = loss.metric_regularizers(h._xyz, h._scaling, h.face_scaling, h.binding, vis, c["t_xyz"], c["t_s"], want_xyz=mx, want_scale=ms)
        s = loss.splat_regularizers(h._xyz, h._scaling, vis, c["t_xyz"], c["t_s"])
        want = {"xyz": (m[0] if mx else s[0]) * 0.5, "scale": (m[1] if ms else s[1]) * 2.0}
        sum(want.values()).backward()
        for k in want:
            assert torch.equal(got[k], want[k]), (mx, ms, k)
        for name in ("_xyz", "_scaling", "face_scaling"):
            assert torch.equal(getattr(g, name).grad, getattr(h, name).grad), (mx, ms, name)
        assert g._gaa_csr[3][1].numel() == 41                              # the CSR is the one kept on the model


def _expr_gradient_float64(g, d_face):
    """(d_expr of timestep 0, face_scaling) in float64 on the CPU: the composed-torch twin of the mesh update (unfused.flame_forward and
    unfused.face_frames, the math the kernels are tested against) evaluated in double on the model's rig and FLAME parameters, and
    `d_face` (float64, per face) sent back through it by torch's float64 autograd."""
    from gaussianavatars_amd import unfused

    fm = g.flame_model
    rig = {k: getattr(fm, k).detach().double().cpu() for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")}
    rig["parents"] = fm.parents.cpu()
    fp = {k: v.detach().double().cpu() for k, v in g.flame_param.items()}
    expr = fp["expr"][[0]].requires_grad_(True)
    verts, _ = unfused.flame_forward(rig, fp["shape"][None, ...], expr, fp["rotation"][[0]], fp["neck_pose"][[0]], fp["jaw_pose"][[0]],
                                     fp["eyes_pose"][[0]], fp["translation"][[0]], fp.get("static_offset"))
    scale = unfused.face_frames(verts[0], fm.faces.cpu())[2]
    scale.backward(torch.from_numpy(np.asarray(d_face, np.float64)).reshape(scale.shape))
    return expr.grad[0].numpy(), scale.detach().numpy().reshape(-1)


def test_gradient_reaches_the_flame_parameters_of_a_bound_model(monkeypatch):
    """face_scaling of the mirror's select_mesh_by_timestep takes the metric terms' gradient back into flame_param['expr'].  The float64
    statement of that gradient: the float64 d_face_scaling of tests/metric_reg_ref.py sent through a float64 evaluation of the mesh update
    (_expr_gradient_float64); the fused and the composed path are held to the bar of this file on expr's row, relative to the row's maximum.

    This test FAILS on the MI355X, and its bar is the issue's, unchanged.  Measured in three runs, in ulp of the row maximum: the fused path is
    8.08-9.23 from float64 at worst, the composed path 7.87-8.58; the worst element misses max(2 x composed, 4 ulp) by a factor of 1.25-2.07
    (an element where the composed path happens to land within 2 ulp).  Of the fused path's distance 0.59 ulp is owed to its d_face_scaling
    (that gradient sent through the float64 chain), of the composed path's 0.56; the other 8 ulp are the fp32 mesh backward both paths go
    through, whose rounding differs between the two runs of it (the two paths differ by 4.50 ulp at worst) and from one process to the next.
    d_face_scaling itself: 32.47 ulp of the value at worst for both paths (the fp32 relu arguments they share), medians 0.14 fused, 0.18
    composed."""
    import bench
    from gaussianavatars_amd import loss

    dev = _dev()
    g, _cam = bench.build_scene(dev, 12_000, 3, 96, 64, 2, "fused", True)   # (the synthetic head wants a splat on each of its 10 144 faces)
    P = g._xyz.shape[0]
    g.select_mesh_by_timestep(0)
    nf = g.face_scaling.shape[0]
    xyz, ls = g._xyz.detach().cpu().numpy(), g._scaling.detach().cpu().numpy()
    fs, binding = g.face_scaling.detach().cpu().numpy().reshape(-1), g.binding.cpu().numpy()
    vis = np.random.default_rng(5).random(P) < 0.6
    t_xyz = float(np.median(xyz * fs[binding][:, None])) + 1e-4             # (off the exact median: no element sits at it)
    t_s = float(np.median(np.exp(ls) * fs[binding][:, None])) * (1 + 1e-4)
    opt = types.SimpleNamespace(lambda_xyz=GX, threshold_xyz=t_xyz, lambda_scale=GS, threshold_scale=t_s, metric_xyz=True, metric_scale=True)
    tvis = _t(vis, dev)
    ref = metric_ref(xyz, ls, fs, binding, vis, t_xyz, t_s, GX, GS)
    grads = {}
    for mode in ("fused", "composed"):
        monkeypatch.setenv("GAA_FUSED_REG", "1" if mode == "fused" else "0")
        bench.zero_grads(g)
        g.select_mesh_by_timestep(0)
        assert g.face_scaling.requires_grad and g.face_scaling.shape == (nf, 1)
        g.face_scaling.retain_grad()
        losses = loss.regularization_losses(g, tvis, opt)
        sum(losses.values()).backward()
        grads[mode] = (g.face_scaling.grad.double().cpu().numpy().reshape(-1), g.flame_param["expr"].grad.double().cpu().numpy())
    want_expr = np.zeros_like(grads["fused"][1])
    want_expr[0], fs64 = _expr_gradient_float64(g, ref["d_face"])
    assert np.abs(fs64 - fs).max() <= 1e-4 * np.abs(fs).max()               # (sanity: the float64 twin is the function the kernels evaluate)
    assert np.abs(want_expr[0]).max() > 0 and not grads["fused"][1][1:].any()
    # (the per-face bar on d_face_scaling is test_means_and_gradients_against_float64's business; here its figures are printed only)
    ef, ec = (np.abs(grads[m][0] - ref["d_face"]) / _ulp(ref["d_face"]) for m in ("fused", "composed"))
    print(f"d_face_scaling on {nf} faces: worst error in ulp of the value: fused {ef.max():.2f} composed {ec.max():.2f}; median fused {np.median(ef):.2f} composed {np.median(ec):.2f}")
    assert not grads["fused"][0][np.bincount(binding[vis], minlength=nf) == 0].any()
    # where each path's distance on expr comes from: its own d_face_scaling sent through the float64 chain (what its face gradient costs), and
    # the rest, which is the fp32 mesh backward both paths share
    row_ulp = _ulp(np.abs(want_expr[0]).max())
    for m in ("fused", "composed"):
        own = np.abs(_expr_gradient_float64(g, grads[m][0])[0] - want_expr[0]).max() / row_ulp
        total = np.abs(grads[m][1][0] - want_expr[0]).max() / row_ulp
        print(f"d_expr, {m}: {total:.2f} ulp of the row maximum from float64 at worst, {own:.2f} of them owed to its d_face_scaling")
    print(f"d_expr: fused and composed differ by {np.abs(grads['fused'][1][0] - grads['composed'][1][0]).max() / row_ulp:.2f} ulp of the row maximum at worst")
    _check("d_expr", grads["fused"][1], grads["composed"][1], want_expr, np.abs(want_expr).max(1, keepdims=True))
    assert np.abs(grads["fused"][1][0]).max() > 0
