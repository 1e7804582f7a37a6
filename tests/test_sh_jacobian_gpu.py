"""The SH colour's derivative with respect to the view direction travels from k_preprocess to k_preprocess_bwd through the geom state
(include/gsr.h: GsrGeomLayout.shjac, nine floats per visible splat) instead of being rebuilt in the backward from the 192-byte coefficient rows.

Every case compares dL/dmeans3D and dL/dsh of one frame with the CPU oracle (oracle/gsr_oracle, forward plus backward) at the bar of
tests/test_gsr_gpu.py: max |difference| below 2e-4 of the tensor's largest magnitude.  The shapes are the smallest at which the stash can go wrong:
P on both sides of the backward's 208 rows per workgroup (a last workgroup of one row included), a 64 x 48 image, stored degree 3 at every active
degree, and stored degree 0 (M = 1, the matrix is zero).  All four ways into the two kernels: the world-space entry with one SH tensor and with the
two leaf tensors, the leaves entry and the bound entry (on identity face frames, under which the gradient of `_xyz` is dL/dmeans3D).  The scenes clamp
some colours at zero and cull some splats; the state buffers are poisoned (rasterizer.set_poison_state: NaN wherever the forward did not write), so a
row of a culled splat that the backward read would show."""
import functools
import math

import numpy as np
import pytest
import torch

from gaussianavatars_amd import synthetic as S

pytestmark = pytest.mark.gpu

W, H = 64, 48
RTOL = 2e-4                     # tests/test_gsr_gpu.py: gradients against the oracle, relative to the tensor's largest magnitude
SIZES = (1, 207, 208, 209, 417)
ENTRIES = ("single", "split", "leaves", "bound")
FACES = 7
# (P, stored degree, active degree, entry)
CASES = ([(P, 3, 3, e) for P in SIZES for e in ENTRIES] + [(209, 3, d, e) for d in (0, 1, 2) for e in ENTRIES] +
         [(209, 0, 0, e) for e in ENTRIES] + [(1, 0, 0, "single")])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _leaves(P, maxdeg):
    """The model's leaves of a seeded scene: positions, log scales, raw quaternions, opacity logits, SH (P, M, 3)."""
    sp = S.random_splats(P, maxdeg, 100 + P, xyz_sigma=0.05, log_scale_mean=math.log(0.012))
    g = np.random.default_rng(200 + P)
    xyz, sh = sp["means3D"].copy(), sp["shs"].copy()
    sh[:, 1:] *= 6.0                         # a view-dependent colour strong enough for its share of dL/dmean to stand above the bar
    opacity = g.normal(0.5, 1.5, (P, 1)).astype(np.float32)
    if P == 1:
        xyz[:], opacity[:] = 0.01, 1.0       # the one splat is on screen and contributes
    else:
        xyz[5::13, 2] += 1.5                 # behind the camera (it sits at z = +1): culled
        xyz[6::29, 0] += 0.9                 # outside the frustum: culled
        sh[3::7, 0, 0] = -3.0                # red clamps at zero
        sh[4::11, 0, :] = -3.0               # every channel clamps at zero
    return dict(_xyz=xyz, _scaling=np.log(sp["scales"]), _rotation=sp["rotations"].copy(),
                _opacity=opacity, sh=sh)


def _settings(deg, dev):
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings

    cam = S.orbit_camera(W, H)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device=dev)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), t([0.2, 0.7, 0.4]), 1.0, t(cam.world_view_transform),
                                       t(cam.full_proj_transform), deg, t(cam.camera_center), False, False)
    return cam, rs


def _frames(F, dev):
    eye = torch.eye(3, device=dev).repeat(F, 1, 1).contiguous()
    quat = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(F, 1).contiguous()
    return eye, torch.ones(F, 1, device=dev), torch.zeros(F, 3, device=dev), quat


@functools.lru_cache(maxsize=None)
def _reference(P, maxdeg, deg):
    """Computed once per scene and left unchanged: the leaves, the world-space values the kernels see (gab_bind_forward on identity frames: the
    activations, bit for bit what the leaves entries evaluate in-kernel), the pixel cotangent, and the oracle's state and gradients."""
    from gaussianavatars_amd import binding as B
    from oracle import gsr_oracle as O

    O.build()
    dev = _dev()
    L = _leaves(P, maxdeg)
    t = lambda a: torch.as_tensor(a, device=dev)
    binding = torch.zeros(P, dtype=torch.int64, device=dev)
    with torch.no_grad():
        world = B.bind_splats(t(L["_xyz"]), t(L["_scaling"]), t(L["_rotation"]), binding, *_frames(1, dev), csr=B.binding_csr(binding, 1),
                              opacity_logit=t(L["_opacity"]))
    wx, ws, wr, wo = (w.cpu().numpy() for w in world)
    cam, _ = _settings(deg, dev)
    s = O.make_settings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), np.array([0.2, 0.7, 0.4], np.float32), 1.0, cam.world_view_transform,
                        cam.full_proj_transform, deg, cam.camera_center)
    st = O.forward(s, wx, L["sh"], None, wo, ws, wr, None)
    gpix = np.random.default_rng(5).normal(0, 1, (3, H, W)).astype(np.float32)
    ref = O.backward(s, st, gpix)
    return dict(leaves=L, world=(wx, ws, wr, wo), gpix=gpix, st=st, means3D=ref["means3D"], shs=ref["shs"], settings=s)


def _frame(R, entry, ref, rs, dev, grad=True, colors=None):
    """One forward of `entry` on fresh tensors -> (image, {name: leaf tensor})."""
    from gaussianavatars_amd import binding as B

    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).requires_grad_(grad)
    L, sh = ref["leaves"], ref["leaves"]["sh"]
    P = sh.shape[0]
    if entry in ("single", "split", "precomp"):
        wx, ws, wr, wo = ref["world"]
        xyz, sc, ro, op = t(wx), t(ws), t(wr), t(wo)
        m2 = torch.zeros_like(xyz, requires_grad=grad)
        rast = R.GaussianRasterizer(rs)
        if entry == "precomp":
            col = t(colors)
            img, _ = rast(means3D=xyz, means2D=m2, opacities=op, colors_precomp=col, scales=sc, rotations=ro)
            return img, dict(xyz=xyz, col=col)
        if entry == "split":
            dc, rest = t(sh[:, :1]), t(sh[:, 1:])
            img, _ = rast(means3D=xyz, means2D=m2, opacities=op, shs=dc, shs_rest=rest, scales=sc, rotations=ro)
            return img, dict(xyz=xyz, dc=dc, rest=rest)
        shs = t(sh)
        img, _ = rast(means3D=xyz, means2D=m2, opacities=op, shs=shs, scales=sc, rotations=ro)
        return img, dict(xyz=xyz, shs=shs)
    xyz, ls, ro, op = t(L["_xyz"]), t(L["_scaling"]), t(L["_rotation"]), t(L["_opacity"])
    dc, rest = t(sh[:, :1]), t(sh[:, 1:])
    m2 = torch.zeros_like(xyz, requires_grad=grad)
    if entry == "leaves":
        img, _, _ = R.rasterize_leaves(xyz, m2, dc, rest, op, ls, ro, rs)
    else:
        binding = (torch.arange(P, device=dev) % FACES).to(torch.int64)
        img, _, _ = R.rasterize_bound(xyz, m2, dc, rest, op, ls, ro, *_frames(FACES, dev), binding, B.binding_csr(binding, FACES), rs)
    return img, dict(xyz=xyz, dc=dc, rest=rest)


def _grads(leaves):
    """-> (dL/dmeans3D, dL/dsh (P, M, 3)) as numpy."""
    gx = leaves["xyz"].grad.cpu().numpy()
    if "shs" in leaves:
        return gx, leaves["shs"].grad.cpu().numpy()
    if "dc" not in leaves:
        return gx, None
    rest = leaves["rest"].grad
    dc = leaves["dc"].grad.cpu().numpy()
    return gx, dc if rest is None or rest.shape[1] == 0 else np.concatenate([dc, rest.cpu().numpy()], 1)


class _modes:
    """Poisoned state buffers, the Python host side (the one that poisons) unless `host`, and optionally the bit-reproducible backward."""

    def __init__(self, deterministic=False, host=False, poison=True):
        self.want = (deterministic, host, poison)

    def __enter__(self):
        from gaussianavatars_amd import _host
        from gaussianavatars_amd import rasterizer as R

        det, host, poison = self.want
        self.prev = (R.set_deterministic(det), R.set_poison_state(poison), _host.set_enabled(host))
        return R

    def __exit__(self, *exc):
        from gaussianavatars_amd import _host
        from gaussianavatars_amd import rasterizer as R

        R.set_deterministic(self.prev[0]), R.set_poison_state(self.prev[1]), _host.set_enabled(self.prev[2])


def _check_against_oracle(what, ref, gx, gsh):
    st = ref["st"]
    culled = st.radii == 0
    for name, g, r in (("dL/dmeans3D", gx, ref["means3D"]), ("dL/dsh", gsh, ref["shs"])):
        assert g.shape == r.shape and np.isfinite(g).all(), f"{what}: {name} is not finite"
        scale = np.abs(r).max() + 1e-20
        err = np.abs(g - r).max() / scale
        print(f"{what}: {name} rel err {err:.3e} (max |ref| {scale:.3e})")
        assert err < RTOL, f"{what}: {name} rel err {err:.3e} (max |ref| {scale:.3e})"
        if culled.any():
            assert np.abs(g[culled]).max() == 0.0, f"{what}: {name} of a culled splat is not exactly zero"


def _case_id(c):
    return f"P{c[0]}-sh{c[1]}-deg{c[2]}-{c[3]}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gradients_match_the_oracle(case):
    P, maxdeg, deg, entry = case
    dev = _dev()
    ref = _reference(P, maxdeg, deg)
    st = ref["st"]
    if P >= 207:   # the scene does what the case is about
        vis = st.radii > 0
        assert 0 < (~vis).sum() < P // 4, "culled splats"
        assert (st.clamped[vis].sum(1) == 1).any() and (st.clamped[vis].sum(1) == 3).any() and (st.clamped[vis].sum(1) == 0).any(), "clamped colours"
    else:
        assert st.radii[0] > 0 and st.clamped.sum() < 3 and st.num_rendered > 0
    _, rs = _settings(deg, dev)
    with _modes() as R:
        img, leaves = _frame(R, entry, ref, rs, dev)
        info = dict(R.last_forward_info())
        img.backward(torch.as_tensor(ref["gpix"], device=dev))
        torch.cuda.synchronize()
    assert not info["forward_only"]
    assert np.array_equal(img.detach().cpu().numpy().view(np.uint32), st.color.view(np.uint32)), "the image is not the oracle's bits"
    _check_against_oracle(_case_id(case), ref, *_grads(leaves))


@pytest.mark.parametrize("entry", ["leaves", "bound"])
def test_gradients_match_the_oracle_through_the_compiled_host(entry):
    """The same frame launched by csrc/gaa_host.cpp: its one allocation of geom, image and binning state takes the new field from gsr_geom_layout."""
    from gaussianavatars_amd import _host

    dev = _dev()
    ref = _reference(417, 3, 3)
    _, rs = _settings(3, dev)
    with _modes(host=True, poison=False) as R:
        if _host.get() is None:
            pytest.skip("gaa_host.so is not built")
        img, leaves = _frame(R, entry, ref, rs, dev)
        assert R.last_forward_info()["native_host"] is True
        img.backward(torch.as_tensor(ref["gpix"], device=dev))
        torch.cuda.synchronize()
    _check_against_oracle(f"compiled host, {entry}", ref, *_grads(leaves))


@pytest.mark.parametrize("entry", ENTRIES)
def test_second_backward_on_one_forward_gives_the_same_bits(entry):
    """retain_graph: the stash is read-only in the backward, so nothing has to be restored between two of them.  (Deterministic mode: the blend's
    sums are then order-free, and every bit of the two gradients can be compared.)"""
    dev = _dev()
    ref = _reference(417, 3, 3)
    _, rs = _settings(3, dev)
    gpix = torch.as_tensor(ref["gpix"], device=dev)
    with _modes(deterministic=True) as R:
        img, leaves = _frame(R, entry, ref, rs, dev)
        img.backward(gpix, retain_graph=True)
        first = _grads(leaves)
        for t in leaves.values():
            t.grad = None
        img.backward(gpix)
        second = _grads(leaves)
        torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _check_against_oracle(f"second backward, {entry}", ref, *second)


@pytest.mark.parametrize("entry", ENTRIES)
def test_forward_without_grad_then_a_training_frame(entry):
    """A torch.no_grad() forward (forward_only: the stash is neither computed nor written) followed by a normal forward and backward on the same
    tensors gives the bits of a fresh run."""
    dev = _dev()
    ref = _reference(209, 3, 3)
    _, rs = _settings(3, dev)
    gpix = torch.as_tensor(ref["gpix"], device=dev)
    with _modes(deterministic=True) as R:
        img, leaves = _frame(R, entry, ref, rs, dev)
        img.backward(gpix)
        fresh = _grads(leaves)
        with torch.no_grad():
            img0, _ = _frame(R, entry, ref, rs, dev, grad=False)
            assert R.last_forward_info()["forward_only"]
        img1, leaves1 = _frame(R, entry, ref, rs, dev)
        assert not R.last_forward_info()["forward_only"]
        img1.backward(gpix)
        again = _grads(leaves1)
        torch.cuda.synchronize()
    assert torch.equal(img0, img.detach()) and torch.equal(img1.detach(), img.detach())
    for a, b in zip(fresh, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_position_gradient_carries_the_view_direction_term():
    """With the same colours passed precomputed the view direction is frozen: dL/dmeans3D loses exactly the term the stash feeds, and must differ
    from the SH run's by more than the bar -- an all-zero stash would make the two runs agree (and is what stored degree 0 legitimately gives)."""
    dev = _dev()
    for maxdeg, differs in ((3, True), (0, False)):
        ref = _reference(209, maxdeg, maxdeg)
        _, rs = _settings(maxdeg, dev)
        gpix = torch.as_tensor(ref["gpix"], device=dev)
        with _modes(deterministic=True) as R:
            img, leaves = _frame(R, "single", ref, rs, dev)
            img.backward(gpix)
            img_p, leaves_p = _frame(R, "precomp", ref, rs, dev, colors=ref["st"].rgb)
            img_p.backward(gpix)
            torch.cuda.synchronize()
        assert torch.equal(img.detach(), img_p.detach())
        a, b = _grads(leaves)[0], _grads(leaves_p)[0]
        gap = np.abs(a - b).max() / (np.abs(a).max() + 1e-20)
        print(f"stored degree {maxdeg}: dL/dmeans3D with and without the view-direction term differ by {gap:.3e} of the largest magnitude")
        if differs:
            assert gap > RTOL
        else:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
