"""GPU parity tests proper: the HIP rasterizer (through the C ABI, via the autograd Function that
render() uses) against the CPU oracle on the same seeded inputs.

Bars: integer outputs (radii, tile rects, tiles_touched, sorted keys, point list, tile ranges,
n_contrib, clamp flags) BIT-EXACT; forward floats bit-exact too (the forward TUs are built with
-ffp-contract=off and share the oracle's exp polynomial) -- asserted as max-abs == 0 with a fallback
tolerance of 0 documented here; backward gradients within rel 2e-4 of the oracle (float atomics
reorder the sums) measured against the per-tensor max magnitude.
"""
import math

import numpy as np
import pytest
import torch

from tests.scenes import scene, settings_args

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run_both(oracle, name, use_precomp_color=False, use_precomp_cov=False, exact_scale_grad=False):
    from gaussianavatars_amd.debug import forward_state
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    cam, sp, bg, deg, mod = scene(name)
    a = settings_args(cam, bg, deg, mod)
    s = oracle.make_settings(**a, exact_scale_grad=exact_scale_grad)
    shs = None if use_precomp_color else sp["shs"]
    colors = np.ascontiguousarray(np.abs(sp["shs"][:, 0, :])) if use_precomp_color else None
    st0 = None
    cov = None
    if use_precomp_cov:
        st0 = oracle.forward(s, sp["means3D"], sp["shs"], None, sp["opacities"], sp["scales"], sp["rotations"], None)
        cov = np.ascontiguousarray(st0.cov3D.copy())
        # culled splats have zeroed cov3D in the oracle state: give them something valid
        cov[(st0.radii == 0)] = np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32)
    sc = None if use_precomp_cov else sp["scales"]
    ro = None if use_precomp_cov else sp["rotations"]
    st = oracle.forward(s, sp["means3D"], shs, colors, sp["opacities"], sc, ro, cov)
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]),
                                       t(a["projmatrix"]), deg, t(a["campos"]), False, False)
    hs = forward_state(rs, t(sp["means3D"]), t(shs), t(colors), t(sp["opacities"]), t(sc), t(ro), t(cov))
    return s, st, hs, rs, dict(means3D=sp["means3D"], shs=shs, colors=colors, opacities=sp["opacities"], scales=sc,
                               rotations=ro, cov=cov)


def _np(x):
    return x.detach().cpu().numpy()


def _check_forward(st, hs):
    I = st.num_rendered
    assert hs["num_rendered"] == I
    np.testing.assert_array_equal(_np(hs["radii"]), st.radii)
    np.testing.assert_array_equal(_np(hs["tiles_touched"]).astype(np.uint32), st.tiles_touched)
    vis = st.radii > 0
    np.testing.assert_array_equal(_np(hs["rect"]).astype(np.int32)[vis], st.rect[vis])
    cl = _np(hs["clamped"])
    for c in range(3):
        np.testing.assert_array_equal((cl >> c) & 1, st.clamped[:, c])
    # sorted keys / values / ranges: bit-exact
    np.testing.assert_array_equal(_np(hs["keys"]).view(np.uint64), st.keys)
    np.testing.assert_array_equal(_np(hs["point_list"]).astype(np.uint32), st.point_list)
    np.testing.assert_array_equal(_np(hs["ranges"]).astype(np.uint32), st.ranges)
    # per-splat floats: bit-exact
    for name in ("depths", "xy", "conic_opacity", "rgb", "cov3D"):
        a, b = _np(hs[name])[vis], getattr(st, name)[vis]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: max abs diff {np.abs(a - b).max()}"
    np.testing.assert_array_equal(_np(hs["n_contrib"]).astype(np.uint32), st.n_contrib)
    assert np.array_equal(_np(hs["final_T"]).view(np.uint32), st.final_T.view(np.uint32))
    img = _np(hs["color"])
    assert np.array_equal(img.view(np.uint32), st.color.view(np.uint32)), f"image max abs diff {np.abs(img - st.color).max()}"
    # quadrant streams: ordered sub-sequences of the tile's sorted list -- splat indices in qpos, their positions in the
    # tile list in the twin stream qlist (parity modes)
    qpos, qlist, qcnt, rng = (_np(hs["qpos"]).astype(np.int64), _np(hs["qlist"]).astype(np.int64), _np(hs["qcount"]).astype(np.int64),
                              st.ranges.astype(np.int64))
    assert (qcnt <= (rng[:, 1] - rng[:, 0])[:, None]).all()
    checked = 0
    for t in np.argsort(-(rng[:, 1] - rng[:, 0]))[:6]:
        n, start = rng[t, 1] - rng[t, 0], rng[t, 0]
        if n == 0:
            continue
        for q in range(4):
            sl = slice(4 * start + q * n, 4 * start + q * n + qcnt[t, q])
            pos = qlist[sl]
            assert (np.diff(pos) > 0).all() and (pos < n).all() and (pos >= 0).all()
            np.testing.assert_array_equal(qpos[sl], st.point_list[start + pos].astype(np.int64))
            checked += 1
    assert checked or I == 0


@pytest.mark.parametrize("name", ["cfg1", "sh3_small", "sh2_mod", "culls", "dense_tile", "dense_tile_xl", "depth_ties", "deep_stack", "empty_view", "huge_grid"])
def test_forward_bit_exact(oracle, name):
    s, st, hs, rs, _ = _run_both(oracle, name)
    _check_forward(st, hs)


def test_forward_precomputed_inputs(oracle):
    s, st, hs, rs, _ = _run_both(oracle, "sh3_small", use_precomp_color=True, use_precomp_cov=True)
    _check_forward(st, hs)


def _grad_check(oracle, name, use_precomp_color=False, use_precomp_cov=False, rtol=2e-4, exact_scale_grad=False):
    from gaussianavatars_amd.rasterizer import GaussianRasterizer

    dev = _dev()
    s, st, hs, rs, inp = _run_both(oracle, name, use_precomp_color, use_precomp_cov, exact_scale_grad)
    H, W = rs.image_height, rs.image_width
    gpix = np.random.default_rng(5).normal(0, 1, (3, H, W)).astype(np.float32)
    ref = oracle.backward(s, st, gpix)
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(True)
    m3, sh, col, op, sc, ro, cov = (tt(inp["means3D"]), tt(inp["shs"]), tt(inp["colors"]), tt(inp["opacities"]),
                                    tt(inp["scales"]), tt(inp["rotations"]), tt(inp["cov"]))
    m2 = torch.zeros_like(m3, requires_grad=True)
    color, radii = GaussianRasterizer(rs)(means3D=m3, means2D=m2, shs=sh, colors_precomp=col, opacities=op, scales=sc,
                                           rotations=ro, cov3D_precomp=cov)
    assert radii.dtype == torch.int32 and not radii.requires_grad
    (color * torch.from_numpy(gpix).to(dev)).sum().backward()
    got = dict(means3D=m3.grad, means2D=m2.grad, shs=None if sh is None else sh.grad,
               colors_precomp=None if col is None else col.grad, opacities=op.grad,
               scales=None if sc is None else sc.grad, rotations=None if ro is None else ro.grad,
               cov3D_precomp=None if cov is None else cov.grad)
    for k, g in got.items():
        r = ref[k]
        if r is None:
            assert g is None, k
            continue
        g = _np(g).reshape(r.shape)
        scale = np.abs(r).max() + 1e-20
        err = np.abs(g - r).max() / scale
        assert err < rtol, f"{name}/{k}: rel err {err:.3e} (max |ref| {scale:.3e})"
    assert float(m2.grad[:, 2].abs().max()) == 0.0
    return got


@pytest.mark.parametrize("name", ["cfg1", "sh3_small", "sh2_mod", "culls", "deep_stack", "huge_grid"])
def test_backward_matches_oracle(oracle, name):
    # huge_grid: screen-filling splats sum ~10^7 per-pixel terms through fp32 atomics; the run-to-run spread of the most
    # cancellation-prone gradient (rotations) reaches 3e-4 of its max, so that scene gets 1e-3
    _grad_check(oracle, name, rtol=1e-3 if name == "huge_grid" else 2e-4)


def test_scale_gradient_conventions(oracle):
    """scale_modifier = 1.4 (sh2_mod).  Default: dL/dscales is upstream's -- the gradient w.r.t. (modifier * scale), no
    factor for the modifier.  set_exact_scale_grad(True): the exact chain rule, = default x modifier.  Both against the
    oracle in the same mode (oracle exact mode is pinned to fp64 autograd, tests/test_oracle_pins.py)."""
    from gaussianavatars_amd import rasterizer as R

    up = _grad_check(oracle, "sh2_mod")
    prev = R.set_exact_scale_grad(True)
    try:
        ex = _grad_check(oracle, "sh2_mod", exact_scale_grad=True)
    finally:
        R.set_exact_scale_grad(prev)
    assert prev is False
    a, b = _np(up["scales"]) * np.float32(1.4), _np(ex["scales"])
    assert np.abs(a - b).max() <= 2e-4 * np.abs(b).max()


def test_backward_precomputed_inputs(oracle):
    _grad_check(oracle, "sh3_small", use_precomp_color=True, use_precomp_cov=True)


def test_split_sh_equals_concatenated(oracle):
    """gsr_forward_ex / gsr_backward_ex read the model's two SH leaf tensors in place: same image bit for bit,
    same gradients as the concatenated (reference) path."""
    from gaussianavatars_amd.rasterizer import GaussianRasterizer

    dev = _dev()
    s, st, hs, rs, inp = _run_both(oracle, "sh3_small")
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(True)
    outs = []
    for split in (False, True):
        m3, op, sc, ro = tt(inp["means3D"]), tt(inp["opacities"]), tt(inp["scales"]), tt(inp["rotations"])
        m2 = torch.zeros_like(m3, requires_grad=True)
        if split:
            dc, rest = tt(inp["shs"][:, :1]), tt(inp["shs"][:, 1:])
            color, radii = GaussianRasterizer(rs)(means3D=m3, means2D=m2, shs=dc, shs_rest=rest, opacities=op, scales=sc, rotations=ro)
        else:
            sh = tt(inp["shs"])
            color, radii = GaussianRasterizer(rs)(means3D=m3, means2D=m2, shs=sh, opacities=op, scales=sc, rotations=ro)
        (color * color).sum().backward()
        gsh = torch.cat([dc.grad, rest.grad], 1) if split else sh.grad
        outs.append((color.detach(), radii, gsh, m3.grad, op.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][2:], outs[1][2:]):
        assert float((a - b).abs().max()) <= 2e-4 * float(a.abs().max())


def test_argument_contract():
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)
    rs = GaussianRasterizationSettings(32, 32, 0.5, 0.5, z(3), 1.0, torch.eye(4, device=dev), torch.eye(4, device=dev), 0,
                                       z(3), False, False)
    r = GaussianRasterizer(rs)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), scales=z(4, 3), rotations=z(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair"):
        r(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), shs=z(4, 1, 3), scales=z(4, 3))
    vis = r.markVisible(torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 0.1]], device=dev))
    assert vis.tolist() == [True, False]


def test_zero_splats_renders_background():
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)
    bg = torch.tensor([0.25, 0.5, 0.75], device=dev)
    rs = GaussianRasterizationSettings(37, 53, 0.5, 0.5, bg, 1.0, torch.eye(4, device=dev), torch.eye(4, device=dev), 0, z(3), False, False)
    color, radii = GaussianRasterizer(rs)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 1, 3), scales=z(0, 3), rotations=z(0, 4))
    assert radii.numel() == 0
    assert torch.equal(color, bg[:, None, None].expand(3, 37, 53))


@pytest.mark.parametrize("fast", [True, False])
def test_zero_splats_forward_and_backward_in_both_blend_modes(fast):
    """P == 0 is the one frame whose state the host zeroes itself (no k_preprocess workgroup runs): the image is the background bit for bit in
    both blend modes, radii is empty, and a backward through it returns."""
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, set_fast_blend

    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    bg = torch.tensor([0.25, 0.5, 0.75], device=dev)
    eye = torch.eye(4, device=dev)
    rs = GaussianRasterizationSettings(32, 48, 0.5, 0.5, bg, 1.0, eye, eye, 0, torch.zeros(3, device=dev), False, False)
    prev = set_fast_blend(fast)
    try:
        color, radii = GaussianRasterizer(rs)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 1, 3), scales=z(0, 3), rotations=z(0, 4))
        color.sum().backward()
        torch.cuda.synchronize()
    finally:
        set_fast_blend(prev)
    assert radii.numel() == 0
    assert torch.equal(color.detach(), bg[:, None, None].expand(3, 32, 48))


def test_replay_on_capacity_overflow(oracle):
    """A frame needing more instances than the current capacity hint is replayed, not truncated."""
    from gaussianavatars_amd import rasterizer as R

    R._capacity_hint.clear()
    s, st, hs, rs, _ = _run_both(oracle, "cfg1")
    key = (0, rs.image_height, rs.image_width, False)    # (device, H, W, production path?)
    R._capacity_hint[key] = R._CAP_QUANTUM  # far below the 73k instances cfg1 needs? keep it honest:
    if st.num_rendered <= R._CAP_QUANTUM:
        pytest.skip("scene fits the minimum capacity")
    s, st, hs, rs, _ = _run_both(oracle, "cfg1")
    assert R.last_forward_info()["replays"] >= 1
    _check_forward(st, hs)


def test_replay_on_capacity_overflow_production(oracle):
    """The same on the production path, whose capacity counts quadrant-stream entries: an under-sized buffer is detected on the
    device (k_qscatter and the blend do nothing), the host grows it and replays; the image is the oracle's."""
    from gaussianavatars_amd import debug as D
    from gaussianavatars_amd import rasterizer as R
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    cam, sp, bg, deg, mod = scene("cfg1")
    a = settings_args(cam, bg, deg, mod)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]),
                                       t(a["projmatrix"]), deg, t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    st = oracle.forward(oracle.make_settings(**a), sp["means3D"], sp["shs"], None, sp["opacities"], sp["scales"], sp["rotations"], None)
    prev = R.set_tile_culling(4)
    try:
        R._capacity_hint[(0, a["H"], a["W"], True)] = R._CAP_QUANTUM
        pro = D._forward_state(rs, *args)
        info = R.last_forward_info()
    finally:
        R.set_tile_culling(prev)
    if pro["num_rendered"] <= R._CAP_QUANTUM:
        pytest.skip("scene fits the minimum capacity")
    assert info["replays"] >= 1 and info["production_binning"]
    assert np.array_equal(_np(pro["color"]).view(np.uint32), st.color.view(np.uint32))


@pytest.mark.parametrize("name", ["cfg1", "sh3_small", "sh2_mod", "culls", "dense_tile", "empty_view"])
def test_tile_culling_changes_only_the_binning_state(oracle, name):
    """GsrSettings.tile_culling: instances whose {alpha >= 1/255} ellipse cannot reach a tile are not binned.  The image,
    final_T and radii must be the same BITS as without culling (and as the oracle's); the culled lists must be ordered
    subsequences of the reference-exact ones that still contain every instance the exact mode streams to a quadrant."""
    from gaussianavatars_amd.debug import forward_state
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    cam, sp, bg, deg, mod = scene(name)
    a = settings_args(cam, bg, deg, mod)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]),
                                       t(a["projmatrix"]), deg, t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    ex = forward_state(rs, *args, tile_culling=False)
    cu = forward_state(rs, *args, tile_culling=True)
    st = oracle.forward(oracle.make_settings(**a), sp["means3D"], sp["shs"], None, sp["opacities"], sp["scales"], sp["rotations"], None)
    assert ex["num_rendered"] == st.num_rendered == ex["rect_instances"] == cu["rect_instances"]
    assert cu["num_rendered"] <= ex["num_rendered"]
    for k in ("color", "final_T"):
        assert np.array_equal(_np(cu[k]).view(np.uint32), _np(ex[k]).view(np.uint32)), k
    assert np.array_equal(_np(cu["color"]).view(np.uint32), st.color.view(np.uint32))
    np.testing.assert_array_equal(_np(cu["radii"]), _np(ex["radii"]))
    rex, rcu = _np(ex["ranges"]).astype(np.int64), _np(cu["ranges"]).astype(np.int64)
    kex, kcu = _np(ex["keys"]).view(np.uint64), _np(cu["keys"]).view(np.uint64)
    pex, pcu = _np(ex["point_list"]).astype(np.int64), _np(cu["point_list"]).astype(np.int64)
    qex, cex = _np(ex["qlist"]).astype(np.int64), _np(ex["qcount"]).astype(np.int64)
    dropped = 0
    for tile in range(rex.shape[0]):
        e0, e1, c0, c1 = rex[tile, 0], rex[tile, 1], rcu[tile, 0], rcu[tile, 1]
        assert (kex[e0:e1] >> np.uint64(32) == tile).all() and (kcu[c0:c1] >> np.uint64(32) == tile).all()
        # (depth bits, splat index) is unique inside a tile and is the order both lists are sorted in
        ke = ((kex[e0:e1] & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | pex[e0:e1].astype(np.uint64)
        kc = ((kcu[c0:c1] & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | pcu[c0:c1].astype(np.uint64)
        assert (np.diff(ke.astype(np.int64)) > 0).all() and (np.diff(kc.astype(np.int64)) > 0).all()
        # subsequence: every culled-mode entry appears in the exact list
        pos = np.searchsorted(ke, kc)
        assert (pos < len(ke)).all() and np.array_equal(ke[pos], kc), f"tile {tile}: culled list is not a subsequence"
        # nothing that reaches a quadrant in exact mode was dropped
        n = e1 - e0
        if n:
            reach = np.zeros(n, bool)
            for q in range(4):
                reach[qex[4 * e0 + q * n: 4 * e0 + q * n + cex[tile, q]]] = True
            kept = np.zeros(n, bool)
            kept[pos] = True
            assert not (reach & ~kept).any(), f"tile {tile}: a reachable instance was culled"
        dropped += n - (c1 - c0)
    assert dropped == ex["num_rendered"] - cu["num_rendered"]
    if name in ("sh3_small", "dense_tile"):
        assert dropped > 0


def test_production_mode_state(oracle):
    """tile_culling = 1 (what render() runs): same image / final_T / radii bits as the parity modes; the reference-format
    lists are not written and n_contrib holds the quadrant-stream position (include/gsr.h)."""
    from gaussianavatars_amd import debug as D
    from gaussianavatars_amd import rasterizer as R
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    cam, sp, bg, deg, mod = scene("sh3_small")
    a = settings_args(cam, bg, deg, mod)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]),
                                       t(a["projmatrix"]), deg, t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    par = D.forward_state(rs, *args, tile_culling=True)
    for mode in (1, 3, 4):  # 1: what render() runs (rank path at this size), 3 / 4: rank path, depth-ordered scatter forced
        prev = R.set_tile_culling(mode)
        try:
            pro = D._forward_state(rs, *args)
        finally:
            R.set_tile_culling(prev)
        for k in ("color", "final_T"):
            assert np.array_equal(_np(pro[k]).view(np.uint32), _np(par[k]).view(np.uint32)), k
        np.testing.assert_array_equal(_np(pro["radii"]), _np(par["radii"]))
        np.testing.assert_array_equal(_np(pro["n_contrib_q"]), _np(par["n_contrib_q"]))
        np.testing.assert_array_equal(_np(pro["n_contrib"]), _np(pro["n_contrib_q"]))
        _same_streams(pro, par, packed=mode == 4)
        assert pro["production_binning"] == (mode == 4) and not par["production_binning"]
        if mode == 4:
            assert pro["num_rendered"] == int(_np(pro["qcount"]).astype(np.int64).sum())    # the scatter path counts stream entries
        else:
            assert pro["num_rendered"] == par["num_rendered"]
        assert pro["rect_instances"] == par["rect_instances"]
    # tile_culling 5 (the retired per-tile sort) is the library's error, not another path under the old number; the smallest scene
    cam, sp, bg, deg, mod = scene("cfg1")
    a = settings_args(cam, bg, deg, mod)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]),
                                       t(a["projmatrix"]), deg, t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    prev = R.set_tile_culling(5)
    try:
        with pytest.raises(RuntimeError, match="per-tile sort was removed"):
            D._forward_state(rs, *args)
    finally:
        R.set_tile_culling(prev)
    assert D._forward_state(rs, *args)["num_rendered"] > 0


def _same_streams(pro, par, packed=True):
    """The production binning (depth-ordered scatter, csrc/gsr_binning.hip) must produce the quadrant streams of the per-tile sort
    path entry for entry: same membership, same (depth, index) order."""
    np.testing.assert_array_equal(_np(pro["qcount"]), _np(par["qcount"]))
    qc = _np(pro["qcount"]).astype(np.int64).reshape(-1)
    a0, b0 = _np(pro["qstart"]).astype(np.int64).reshape(-1), _np(par["qstart"]).astype(np.int64).reshape(-1)
    qa, qb = _np(pro["qpos"]).astype(np.int64), _np(par["qpos"]).astype(np.int64)
    nz = np.nonzero(qc)[0]
    if packed:
        assert np.array_equal(a0[nz], np.concatenate([[0], np.cumsum(qc)[:-1]])[nz])          # the scatter path packs the streams back to back
    ia = np.concatenate([np.arange(a0[q], a0[q] + qc[q]) for q in nz]) if len(nz) else np.zeros(0, np.int64)
    ib = np.concatenate([np.arange(b0[q], b0[q] + qc[q]) for q in nz]) if len(nz) else np.zeros(0, np.int64)
    np.testing.assert_array_equal(qa[ia], qb[ib])


def _streams_in_depth_order(st):
    """Every quadrant stream lists its splats in strictly increasing (depth bits, index) order -- checked from the state's own depths,
    whatever binning wrote the streams."""
    qc, q0 = _np(st["qcount"]).astype(np.int64).reshape(-1), _np(st["qstart"]).astype(np.int64).reshape(-1)
    nz = np.nonzero(qc)[0]
    if not len(nz):
        return
    at = np.concatenate([np.arange(q0[q], q0[q] + qc[q]) for q in nz])
    idx = _np(st["qpos"]).astype(np.int64)[at]
    key = (_np(st["depths"]).view(np.uint32).astype(np.int64)[idx] << 32) | idx
    inside = np.ones(len(at), bool)
    inside[np.concatenate([[0], np.cumsum(qc[nz])[:-1]])] = False      # the first entry of a stream has no predecessor
    assert (np.diff(key)[inside[1:]] > 0).all()


@pytest.mark.parametrize("name", ["cfg1", "sh2_mod", "culls", "dense_tile", "dense_tile_xl", "depth_ties", "deep_stack", "empty_view"])
def test_production_binning_streams_equal_the_sort_path(oracle, name):
    """Every scene of the parity set through the production binning: streams identical to the per-tile sort path's, image /
    final_T / radii the oracle's bits."""
    from gaussianavatars_amd import debug as D
    from gaussianavatars_amd import rasterizer as R
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    cam, sp, bg, deg, mod = scene(name)
    a = settings_args(cam, bg, deg, mod)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]),
                                       t(a["projmatrix"]), deg, t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    par = D.forward_state(rs, *args, tile_culling=True)
    prev = R.set_tile_culling(4)   # the depth-ordered scatter whatever the splat count (mode 1 takes it beyond 262144 splats)
    try:
        pro = D._forward_state(rs, *args)
    finally:
        R.set_tile_culling(prev)
    assert pro["production_binning"]
    _same_streams(pro, par)
    st = oracle.forward(oracle.make_settings(**a), sp["means3D"], sp["shs"], None, sp["opacities"], sp["scales"], sp["rotations"], None)
    assert np.array_equal(_np(pro["color"]).view(np.uint32), st.color.view(np.uint32))
    assert np.array_equal(_np(pro["final_T"]).view(np.uint32), st.final_T.view(np.uint32))
    np.testing.assert_array_equal(_np(pro["radii"]), st.radii)


def test_tile_culling_gradients_equal_exact_mode(oracle):
    from gaussianavatars_amd import rasterizer as R

    prev = R.set_tile_culling(False)
    try:
        _grad_check(oracle, "sh3_small")
    finally:
        R.set_tile_culling(prev)
    assert R.get_tile_culling() == prev
    prev = R.set_tile_culling(True)
    try:
        _grad_check(oracle, "sh3_small")
        _grad_check(oracle, "culls")
    finally:
        R.set_tile_culling(prev)


@pytest.mark.parametrize("name", ["sh3_small", "culls", "deep_stack", "huge_grid"])
def test_deterministic_backward_is_bit_reproducible(oracle, name):
    """GsrSettings.deterministic: the blend backward accumulates in 64-bit fixed point (integer adds commute), so two runs give the
    same bits -- the default fp32 atomics do not -- and the values still match the oracle (the 3300x3300 scene, whose sums run over
    10^7 pixels, at 5e-4: what is left there is the fp32 rounding of each 64-pixel partial and of the oracle's own running sums)."""
    from gaussianavatars_amd import rasterizer as R

    prev = R.set_deterministic(True)
    try:
        rtol = 5e-4 if name == "huge_grid" else 2e-4
        a = _grad_check(oracle, name, rtol=rtol)
        b = _grad_check(oracle, name, rtol=rtol)
    finally:
        R.set_deterministic(prev)
    assert prev is False
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), f"{name}/{k}: two deterministic backward passes differ"


@pytest.mark.parametrize("seed", range(10))
def test_rank_path_equals_the_per_tile_sort_on_random_scenes(seed):
    """The rank path (tile lists ordered through bitmaps of global depth ranks, csrc/gsr_rank.hip), one band and forced bands, against the depth-ordered
    scatter (csrc/gsr_binning.hip; the per-tile bitonic sort this test is named after was retired) on scenes drawn at random: odd image sizes, splat counts around the wave / workgroup / chunk boundaries, tiny to
    screen-filling splats, everything behind the camera.  Same quadrant streams entry for entry, same image / final_T / radii /
    n_contrib bits, same instance counts."""
    from gaussianavatars_amd import debug as D
    from gaussianavatars_amd import rasterizer as R
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    rng = np.random.default_rng(1000 + seed)
    P = int(rng.choice([1, 2, 63, 64, 65, 255, 257, 1023, 4097, 20011]))
    W, H = int(rng.integers(17, 400)), int(rng.integers(17, 300))
    deg = int(rng.integers(0, 4))
    sp = S.random_splats(P, deg, 500 + seed, xyz_sigma=float(rng.choice([0.01, 0.05, 0.3])),
                         log_scale_mean=math.log(float(rng.choice([0.0005, 0.004, 0.03, 0.2]))), log_scale_sigma=float(rng.choice([0.1, 0.6, 1.2])))
    if seed == 7:
        sp["means3D"][:, 2] += 5.0      # everything behind the near plane
    cam = S.orbit_camera(W, H, yaw_deg=float(rng.uniform(-40, 40)), pitch_deg=float(rng.uniform(-20, 20)))
    a = settings_args(cam, [0.2, 0.5, 0.1], deg, 1.0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), 1.0, t(a["viewmatrix"]), t(a["projmatrix"]), deg,
                                       t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    out = {}
    for mode in (3, 6, 4):     # 6: the rank path with a rank per band of tile rows (what frames beyond 262144 splats use)
        prev = R.set_tile_culling(mode)
        try:
            out[mode] = D._forward_state(rs, *args)
        finally:
            R.set_tile_culling(prev)
    # the yardstick: the depth-ordered scatter (4), the binning that shares no kernel with the rank path.  (It counts stream entries, not
    # tile instances: the two rank forms are held to each other there, and to the sum of the tile counters.)
    old = out[4]
    assert old["binning_path"] == 1
    assert out[3]["num_rendered"] == out[6]["num_rendered"]
    for mode in (3, 6):
        new = out[mode]
        assert new["binning_path"] == 0
        assert new["num_rendered"] == int(_np(new["tile_count"]).astype(np.int64).sum()) and new["rect_instances"] == old["rect_instances"]
        for k in ("color", "final_T"):
            assert np.array_equal(_np(new[k]).view(np.uint32), _np(old[k]).view(np.uint32)), (mode, k)
        for k in ("radii", "n_contrib", "n_contrib_q", "tiles_touched"):
            np.testing.assert_array_equal(_np(new[k]), _np(old[k]), err_msg=f"{mode}/{k}")
        _same_streams(old, new, packed=True)


@pytest.mark.parametrize("W,H", [(2560, 2400), (1100, 1600)])
def test_rank_scatter_forms_on_tile_grids_around_the_staging_limit(oracle, W, H):
    """k_rscatter / k_rsort_rscatter deal the tile instances evenly to the lanes from staging rows in LDS when those fit beside the tile
    histogram (1100 x 1600: 6900 tiles) and fall back to the lockstep expansion when they do not (2560 x 2400: 24000 tiles = 96 KB of
    histogram), one band and forced bands: the oracle's image bits and counters, and the same depth-ordered streams either way.  (These
    grids are beyond what the depth-ordered scatter takes, so the yardstick is the CPU oracle.  Grids beyond the LDS histogram altogether --
    per-instance L2 atomics -- are the 3300 x 3300 scene of the oracle tests.)"""
    from gaussianavatars_amd import debug as D
    from gaussianavatars_amd import rasterizer as R
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    P, deg = 6000, 1
    sp = S.random_splats(P, deg, 91, xyz_sigma=0.12, log_scale_mean=math.log(0.006), log_scale_sigma=1.0)   # a few tiles to hundreds of tiles per splat
    cam = S.orbit_camera(W, H, yaw_deg=12.0, pitch_deg=-5.0)
    a = settings_args(cam, [0.1, 0.2, 0.3], deg, 1.0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), 1.0, t(a["viewmatrix"]), t(a["projmatrix"]), deg,
                                       t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    out = {}
    for mode in (3, 6):
        prev = R.set_tile_culling(mode)
        try:
            out[mode] = D._forward_state(rs, *args)
        finally:
            R.set_tile_culling(prev)
    st = oracle.forward(oracle.make_settings(**a), sp["means3D"], sp["shs"], None, sp["opacities"], sp["scales"], sp["rotations"], None)
    assert out[3]["num_rendered"] == out[6]["num_rendered"] > 20 * P
    for mode in (3, 6):
        new = out[mode]
        assert new["binning_path"] == 0 and new["num_rendered"] == int(_np(new["tile_count"]).astype(np.int64).sum())
        assert new["rect_instances"] == st.num_rendered
        for k in ("color", "final_T"):
            assert np.array_equal(_np(new[k]).view(np.uint32), getattr(st, k).view(np.uint32)), (mode, k)
        np.testing.assert_array_equal(_np(new["radii"]), st.radii, err_msg=f"{mode}/radii")
        np.testing.assert_array_equal(_np(new["tiles_touched"]).astype(np.uint32), st.tiles_touched, err_msg=f"{mode}/tiles_touched")
        for k in ("n_contrib", "n_contrib_q"):
            np.testing.assert_array_equal(_np(new[k]), _np(out[3][k]), err_msg=f"{mode}/{k}")
        _streams_in_depth_order(new)
    _same_streams(out[6], out[3], packed=False)


@pytest.mark.parametrize("W,H,nbands", [(96, 80, 5), (96, 16, 1)])
def test_rank_bands_with_more_splats_than_one_bitmap_holds(W, H, nbands):
    """300 000 splats crowded into the middle of a small image: past 262144 splats the rank path ranks per band of tile rows, and here
    one band (or, 16 pixels high, the only one) holds more splats than a tile bitmap has bits, so the tile kernel takes several
    passes over its rank space.  Same streams, image bits and counters as the depth-ordered scatter (the binning that shares no kernel with
    the rank path; it counts stream entries, so the instance count is held to the sum of the tile counters)."""
    from gaussianavatars_amd import debug as D
    from gaussianavatars_amd import rasterizer as R
    from gaussianavatars_amd import synthetic as S
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    dev = _dev()
    P, deg = 300_000, 0
    sp = S.random_splats(P, deg, 77, xyz_sigma=0.004, log_scale_mean=math.log(0.002), log_scale_sigma=0.3)
    cam = S.orbit_camera(W, H)
    a = settings_args(cam, [0.0, 0.0, 0.0], deg, 1.0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), 1.0, t(a["viewmatrix"]), t(a["projmatrix"]), deg,
                                       t(a["campos"]), False, False)
    args = (t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None)
    out = {}
    for mode in (3, 4):
        prev = R.set_tile_culling(mode)
        try:
            out[mode] = D._forward_state(rs, *args)
        finally:
            R.set_tile_culling(prev)
    new, old = out[3], out[4]
    assert new["binning_path"] == 0 and old["binning_path"] == 1
    assert new["nbands"] == nbands and new["band_rows"] == 1
    if nbands > 1:
        assert int(_np(new["band_total"]).max()) > 262144, "the scene is meant to overflow one band's bitmap"
    assert new["num_rendered"] == int(_np(new["tile_count"]).astype(np.int64).sum()) > 262144 and new["rect_instances"] == old["rect_instances"]
    for k in ("color", "final_T"):
        assert np.array_equal(_np(new[k]).view(np.uint32), _np(old[k]).view(np.uint32)), k
    for k in ("radii", "n_contrib", "n_contrib_q"):
        np.testing.assert_array_equal(_np(new[k]), _np(old[k]), err_msg=k)
    _same_streams(old, new, packed=True)


def test_debug_mode_dumps_the_failing_calls_arguments(tmp_path, monkeypatch):
    """Upstream's `debug=True`: a native call that fails writes its arguments to snapshot_fw.dump in the working directory before the error
    is raised (gaussian_renderer/__init__.py:50 passes pipe.debug)."""
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

    dev = _dev()
    monkeypatch.chdir(tmp_path)
    cam, sp, bg, deg, mod = scene("cfg1")
    a = settings_args(cam, bg, deg, mod)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for debug in (False, True):
        rs = GaussianRasterizationSettings(a["H"], a["W"], a["tanfovx"], a["tanfovy"], t(a["bg"]), mod, t(a["viewmatrix"]), t(a["projmatrix"]),
                                           3, t(a["campos"]), False, debug)     # degree 3 asked of one coefficient per splat: the library refuses
        with pytest.raises(RuntimeError, match="sh_degree 3 needs 16"):
            GaussianRasterizer(rs)(means3D=t(sp["means3D"]), means2D=torch.zeros(len(sp["means3D"]), 3, device=dev), shs=t(sp["shs"]),
                                   opacities=t(sp["opacities"]), scales=t(sp["scales"]), rotations=t(sp["rotations"]))
        assert (tmp_path / "snapshot_fw.dump").exists() == debug
    saved = torch.load(tmp_path / "snapshot_fw.dump")
    assert len(saved) == 18 and torch.equal(saved[1], torch.from_numpy(sp["means3D"])) and saved[15] == 3
