"""The rasterizer's two leaves entries (rasterizer.rasterize_bound / rasterize_leaves: what render() calls) against float64, row by row.

The activations and the mesh-local -> world transform run inside k_preprocess; their chain rule (bindm::bind_backward and
bindm::unit_rotation_backward of csrc/bind_math.h, as compiled into libgsr_hip.so) runs at the tail of k_preprocess_bwd, which also parks the
20-float row per splat that gab_bind_backward_faces reduces per face.  Nothing here differentiates the blend in float64 (a threshold flip
would make any reference disagree).  Instead, for one case of tests/binding_ref.py (raster_case):

  1. W = binding.bind_splats(leaves, frames, opacity_logit): the world values (gab_bind_forward, held to float64 by test_binding_parity_gpu.py);
  2. the world-space entry on W, deterministic backward -> G_w = (d xyz, d scaling, d rotation, d opacity), d means2D, d sh;
  3. the bound (or leaves) entry on the leaves, same settings and grad_out_color: image, radii and visibility must be the bits of 2;
  4. d means2D and the SH gradients pass through no bind chain rule: the same bits in both entries -- the witness that both summed the same
     per-splat cotangent;
  5. binding_ref.bind_eval(leaves, binding, w=G_w) in float64 and in fp32 on the CPU is the VJP wanted: the entry's d _xyz, _scaling, _rotation,
     _opacity and the four face gradients are held to it with binding_ref.check (row_err, bar = max(FLOOR, FACTOR x the CPU-fp32 deviation)).

The unbound entry runs the same scheme on identity frames (every splat on face 0), under which gab_bind_forward returns exp, normalize, sigmoid
and the position as the bits the entry computes in-kernel.  Exact blend and fast blend; the Python host side, the compiled one, and the Python one
once more on poisoned buffers (rasterizer.set_poison_state), which must give the same bits.  Exact zeros: the gradient rows of culled splats,
the face rows of empty and of all-culled faces, d _opacity of the saturated logits.  The cases' conditions: tests/test_bound_entry_cases_cpu.py."""
import math

import numpy as np
import pytest
import torch

from tests import binding_ref as BR

pytestmark = pytest.mark.gpu

LEAF_GRADS = ("_xyz", "_scaling", "_rotation", "_opacity")
FACE_GRADS = ("face_R", "face_scale", "face_center", "face_quat")
# (N, scaled_quat, binding dtype, active SH degree, _rotation normalised first)
CASES = [(N, sq, torch.int64, 3, False) for N in BR.RASTER_NS for sq in (False, True)] + [
    (257, True, torch.int32, 3, False),      # int32 binding
    (63, True, torch.int64, 1, False),       # active degree below the stored one
    (257, True, torch.int64, 3, True),       # |_rotation| = 1: the one case in which the 1 / |_rotation| factors of the chain rule are 1
]
BLENDS = [pytest.param(False, id="exact"), pytest.param(True, id="fast", marks=pytest.mark.fast_blend)]


def _case_id(c):
    N, sq, dt, deg, unit = c
    return f"N{N}-{'scaled' if sq else 'unit'}quat-{str(dt)[6:]}-deg{deg}" + ("-unitrot" if unit else "")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _settings(R, entry, cam, deg, dev):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device=dev)
    return R.GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), t(BR.RASTER_BG),
                                           BR.RASTER_SCALE_MODIFIER[entry], t(cam.world_view_transform), t(cam.full_proj_transform), deg,
                                           t(cam.camera_center), False, False)


def _inputs(entry, case):
    N, sq, _, _, unit = case
    leaves, binding, sh, gpix, cam = BR.raster_case(N, sq, entry)
    if unit:
        leaves = dict(leaves)
        q = leaves["_rotation"].astype(np.float64)
        leaves["_rotation"] = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), np.float32)
    return leaves, binding, sh, gpix, cam


def _world_run(R, B, dev, entry, case, leaves, binding_t, sh, gpix, rs):
    """Steps 1 and 2 -> image, radii, visible, G_w (numpy fp32, bind_eval's weight names), d means2D, d sh_dc, d sh_rest."""
    L = {k: torch.as_tensor(leaves[k], device=dev) for k in BR.BIND_LEAVES}
    with torch.no_grad():
        W = B.bind_splats(L["_xyz"], L["_scaling"], L["_rotation"], binding_t, L["face_R"], L["face_scale"], L["face_center"], L["face_quat"],
                          csr=B.binding_csr(binding_t, BR.BIND_F), opacity_logit=L["_opacity"])
    xyz, scaling, rotation, opacity = (w.detach().clone().requires_grad_(True) for w in W)
    m2 = torch.zeros_like(xyz, requires_grad=True)
    dc, rest = (torch.as_tensor(np.ascontiguousarray(a), device=dev).requires_grad_(True) for a in (sh[:, :1], sh[:, 1:]))
    rast = R.GaussianRasterizer(rs)
    img, radii = rast(means3D=xyz, means2D=m2, opacities=opacity, shs=dc, scales=scaling, rotations=rotation, shs_rest=rest)
    vis = rast.visibility_filter.clone()
    img.backward(torch.as_tensor(gpix, device=dev))
    G = {k: t.grad.cpu().numpy() for k, t in zip(BR.BIND_OUTS, (xyz, scaling, rotation, opacity))}
    return img.detach(), radii, vis, G, m2.grad, dc.grad, rest.grad


def _entry_run(R, B, dev, entry, leaves, binding_t, sh, gpix, rs):
    """Step 3 -> image, radii, visible, {leaf or face tensor name: gradient}, d means2D, d sh_dc, d sh_rest."""
    bound = entry == "bound"
    L = {k: torch.as_tensor(leaves[k], device=dev).requires_grad_(bound or k in LEAF_GRADS) for k in BR.BIND_LEAVES}
    m2 = torch.zeros_like(L["_xyz"], requires_grad=True)
    dc, rest = (torch.as_tensor(np.ascontiguousarray(a), device=dev).requires_grad_(True) for a in (sh[:, :1], sh[:, 1:]))
    if bound:
        img, radii, vis = R.rasterize_bound(L["_xyz"], m2, dc, rest, L["_opacity"], L["_scaling"], L["_rotation"], L["face_R"], L["face_scale"],
                                            L["face_center"], L["face_quat"], binding_t, B.binding_csr(binding_t, BR.BIND_F), rs)
    else:
        img, radii, vis = R.rasterize_leaves(L["_xyz"], m2, dc, rest, L["_opacity"], L["_scaling"], L["_rotation"], rs)
    info = dict(R.last_forward_info())
    vis = vis.clone()
    img.backward(torch.as_tensor(gpix, device=dev))
    torch.cuda.synchronize()
    grads = {k: L[k].grad for k in (LEAF_GRADS + FACE_GRADS if bound else LEAF_GRADS)}
    return img.detach(), radii, vis, grads, m2.grad, dc.grad, rest.grad, info


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run_case(entry, case, fast):
    from gaussianavatars_amd import _host
    from gaussianavatars_amd import binding as B
    from gaussianavatars_amd import rasterizer as R

    dev = _dev()
    N, sq, idx_dtype, deg, _ = case
    leaves, binding, sh, gpix, cam = _inputs(entry, case)
    binding_t = torch.as_tensor(binding, device=dev).to(idx_dtype)
    rs = _settings(R, entry, cam, deg, dev)
    what = f"{entry} {_case_id(case)} {'fast' if fast else 'exact'}"
    prev = (R.set_fast_blend(fast), R.set_deterministic(True), R.set_poison_state(False), _host.set_enabled(False))
    try:
        img_w, radii_w, vis_w, G, m2_w, dc_w, rest_w = _world_run(R, B, dev, entry, case, leaves, binding_t, sh, gpix, rs)
        runs = {"python": _entry_run(R, B, dev, entry, leaves, binding_t, sh, gpix, rs)}
        assert runs["python"][7]["native_host"] is False and runs["python"][7]["bound"] is True
        R.set_poison_state(True)
        runs["poisoned"] = _entry_run(R, B, dev, entry, leaves, binding_t, sh, gpix, rs)
        R.set_poison_state(False)
        _host.set_enabled(True)
        if _host.get() is not None:
            runs["compiled"] = _entry_run(R, B, dev, entry, leaves, binding_t, sh, gpix, rs)
            assert runs["compiled"][7]["native_host"] is True, f"{what}: the compiled host did not take the call"
    finally:
        R.set_fast_blend(prev[0]), R.set_deterministic(prev[1]), R.set_poison_state(prev[2]), _host.set_enabled(prev[3])

    r64, r32 = BR.bind_eval(leaves, binding, G, torch.float64), BR.bind_eval(leaves, binding, G, torch.float32)
    radii = radii_w.cpu().numpy()
    culled = torch.as_tensor(radii == 0, device=dev)
    counts, seen = np.bincount(binding, minlength=BR.BIND_F), np.bincount(binding[radii > 0], minlength=BR.BIND_F)
    dead = torch.as_tensor(np.nonzero(seen == 0)[0], device=dev)      # faces that own no splat, or none that is visible
    if entry == "bound" and N == 1000:
        assert ((counts > 0) & (seen == 0)).any(), f"{what}: no face with every splat culled"
        assert 0.40 <= (radii > 0).mean() <= 0.95
    for host, (img, rad, vis, grads, m2, dc, rest, _info) in runs.items():
        w = f"{what} {host}"
        # step 3: the same frame
        assert _bits(img, img_w), f"{w}: image differs from the world-space entry's, max |diff| {float((img - img_w).abs().max()):.2e}"
        assert torch.equal(rad, radii_w) and torch.equal(vis, vis_w) and torch.equal(vis, rad > 0), f"{w}: radii / visibility"
        # step 4: the same per-splat cotangent
        for name, a, b in (("d means2D", m2, m2_w), ("d sh_dc", dc, dc_w), ("d sh_rest", rest, rest_w)):
            assert _bits(a, b), f"{w}: {name} is not the world-space entry's bits, max |diff| {float((a - b).abs().max()):.2e}"
        # step 5
        for k, g in grads.items():
            assert g is not None and bool(torch.isfinite(g).all()), f"{w} d{k} is not finite"
            BR.check(f"{w} d{k}", g, r64["d_" + k], r32["d_" + k])
        # exact zeros
        for name, g in list(grads.items())[:4] + [("means2D", m2), ("sh_dc", dc), ("sh_rest", rest)]:
            if bool(culled.any()):
                assert float(g[culled].abs().max()) == 0.0, f"{w}: d{name} of a culled splat is not exactly zero"
        if entry == "bound":
            for k in FACE_GRADS:
                assert float(grads[k][dead].abs().max()) == 0.0, f"{w}: d{k} of a face without a visible splat is not exactly zero"
        if N >= 63:
            sat = grads["_opacity"][N - 4:, 0].tolist()
            assert all(x == 0.0 for x in sat), f"{w}: d_opacity of the saturated logits {BR.SATURATED} = {sat}"
    # the poisoned run: the same bits as the clean one, every output
    a, b = runs["python"], runs["poisoned"]
    assert _bits(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), f"{what}: poisoning changes the frame"
    for name, x, y in [(k, a[3][k], b[3][k]) for k in a[3]] + [("means2D", a[4], b[4]), ("sh_dc", a[5], b[5]), ("sh_rest", a[6], b[6])]:
        assert _bits(x, y), f"{what}: d{name} changes when the backward's buffers are poisoned"


@pytest.mark.parametrize("fast", BLENDS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_bound_entry_gradients_against_float64(case, fast):
    _run_case("bound", case, fast)


@pytest.mark.parametrize("fast", BLENDS)
@pytest.mark.parametrize("case", [c for c in CASES if c[2] is torch.int64], ids=_case_id)
def test_leaves_entry_gradients_against_float64(case, fast):
    _run_case("leaves", case, fast)
