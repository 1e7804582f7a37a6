"""The binding kernels (csrc/gab_kernels.hip, csrc/bind_math.h) against the float64 reference of tests/binding_ref.py, at the sizes, poses and
faces tests/test_binding_gpu.py (one full-size rig, fp32 composed torch on the same GPU, whole-tensor relative errors) does not reach:

  rigs of 37 .. 1000 vertices with 0 .. 30 shape and 1 .. 100 expression coefficients; all-zero, partly zero, large and 1e-4 rad poses;
  the sequence table at T around the 32-frame tile and at expression counts on both sides of its staged path; 1 .. 257 faces, int32 and int64,
  hand-built degenerate faces; splats whose _rotation and face quaternion are not unit length, faces that own no splat and one that owns
  hundreds, the fused sigmoid out to +-100.

Every comparison is binding_ref.check: row by row against float64, the bar FLAME_ROW_FACTOR x the CPU-fp32 deviation of unfused.py on the same
inputs (floor FLAME_ROW_FLOOR); name, err, fp32_dev and bar are printed.  The inputs' conditioning is asserted by tests/test_binding_ref_cpu.py."""
import numpy as np
import pytest
import torch

from tests import binding_ref as BR
from tests.test_binding_gpu import _dev, _Head

pytestmark = pytest.mark.gpu

RIGS = [(37, 3, 5), (64, 0, 1), (257, 10, 100), (1000, 30, 33)]
# classic: the three-kernel forward and backward; prepared: the one-launch forward (its backward is the classic one here: a gradient arrives at
# v_shaped); prepared+shape: shape and static_offset optimised (gab_flame_backward with d_shape, d_static_offset); prepared/verts: the loss on
# the posed vertices only, which is what reaches gab_flame_backward_prepared
PATHS = ["classic", "prepared", "prepared+shape", "prepared/verts"]


def _t(a, dev, grad=False):
    return torch.as_tensor(a, device=dev).clone().requires_grad_(grad)


def _run_flame(dev, V, n_shape, n_expr, pose, path):
    from gaussianavatars_amd import binding as B

    rig, p, w = BR.flame_case(V, n_shape, n_expr, pose)
    r64, r32 = BR.flame_refs(V, n_shape, n_expr, pose)
    head = _Head(rig, dev, n_shape)
    if path == "classic":
        head.flame_impl = "classic"
    static = ("shape", "static_offset") if path != "prepared+shape" else ()
    L = {k: _t(p[k], dev, k not in static) for k in BR.FLAME_LEAVES}
    verts, vs = B.flame_forward(head, L["shape"], L["expr"], L["rotation"], L["neck_pose"], L["jaw_pose"], L["eyes_pose"], L["translation"],
                                L["static_offset"])
    assert (getattr(head, "_gab_prepared", None) is not None) == (path in ("prepared", "prepared/verts")), path
    loss = (verts * _t(w["verts"], dev)).sum()
    pre = "dv_" if path == "prepared/verts" else "d_"
    if pre == "d_":
        loss = loss + (vs * _t(w["v_shaped"], dev)).sum()
    loss.backward()
    what = f"flame V={V} ns={n_shape} ne={n_expr} {pose} {path}"
    assert bool(torch.isfinite(verts).all()) and bool(torch.isfinite(vs).all()), what
    BR.check(f"{what} verts", verts, r64["verts"], r32["verts"])
    BR.check(f"{what} v_shaped", vs, r64["v_shaped"], r32["v_shaped"])
    for k in BR.FLAME_LEAVES:
        if k in static:
            assert L[k].grad is None
            continue
        assert bool(torch.isfinite(L[k].grad).all()), f"{what} d_{k} is not finite"
        BR.check(f"{what} d_{k}", L[k].grad, r64[pre + k], r32[pre + k])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("V,n_shape,n_expr", RIGS)
def test_flame_forward_backward_on_small_rigs(V, n_shape, n_expr, path):
    """V below, at and just above one wave and one 256-thread block; 1, an odd number and the product's 100 expression coefficients; no shape block."""
    _run_flame(_dev(), V, n_shape, n_expr, "random", path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pose", ["zero", "eyes_neck_zero", "large", "tiny"])
def test_flame_pose_edges(pose, path):
    """zero: rodrigues / rodrigues_bwd at r == 0 live on the 1e-8-before-the-norm convention (angle 1.7e-8, divisions by its square); the float64
    reference follows the same convention.  Outputs and gradients finite (asserted in _run_flame) and within the bar."""
    _run_flame(_dev(), 257, 10, 100, pose, path)


@pytest.mark.parametrize("mode", ["merged", "split"])
@pytest.mark.parametrize("V,F", list(BR.MESH_CASES))
def test_mesh_frames_timestep(monkeypatch, V, F, mode):
    from gaussianavatars_amd import binding as B

    dev = _dev()
    monkeypatch.setenv("GAA_MESH_BWD", mode)
    rig, fp_np, faces_np, w, r64, r32 = BR.mesh_case(V, F)
    head = _Head(rig, dev, rig["n_shape"])
    faces = torch.as_tensor(faces_np, device=dev)
    fp = {k: _t(v, dev, k in BR.FLAME_ROWS) for k, v in fp_np.items()}
    verts, cano, center, R, scale, quat = B.mesh_frames_timestep(head, fp, BR.MESH_ROW, faces)
    outs = dict(verts=verts, v_shaped=cano, center=center, R=R, scale=scale, quat=quat)
    loss = sum((outs[k] * _t(w[k], dev)).sum() for k in ("center", "R", "scale", "quat", "verts"))
    loss.backward()
    what = f"mesh V={V} F={F} {mode}"
    for k, o in outs.items():
        BR.check(f"{what} {k}", o, r64[k], r32[k])
    for k in BR.FLAME_ROWS:
        g = fp[k].grad
        assert tuple(g.shape) == tuple(fp[k].shape)
        assert float(g[0].abs().max()) == 0.0 and float(g[2].abs().max()) == 0.0, f"{what} d_{k}: gradient outside row {BR.MESH_ROW}"
        BR.check(f"{what} d_{k}", g[[BR.MESH_ROW]], r64["d_" + k], r32["d_" + k])


# n_shape = 8: (257, 8, 100) and the two K < 100 multiples of four take the LDS-staged product (the latter its zero-padded columns, which the
# product's K = 100 never touches); 1, 33, 99 take the direct one
SEQUENCES = [(100, T) for T in (2, 31, 32, 33, 64, 65)] + [(K, 33) for K in (1, 33, 99, 36, 96)]


@pytest.mark.parametrize("n_expr,T", SEQUENCES)
def test_sequence_table(monkeypatch, n_expr, T):
    from gaussianavatars_amd import binding as B

    dev = _dev()
    monkeypatch.setenv("GAA_MESH_SEQUENCE", "eager")
    V = 257
    rig, fp_np, vs64, vs32 = BR.sequence_case(V, 8, n_expr, T)
    head = _Head(rig, dev, 8)
    fp = {k: _t(v, dev) for k, v in fp_np.items()}
    t = T - 1
    with torch.no_grad():
        verts, vs = B.flame_forward_timestep(head, fp, t)
    table = head._gab_sequence[1]
    assert table is not None and tuple(table.shape) == (T, 3 * V)
    what = f"sequence ne={n_expr} T={T}"
    BR.check(f"{what} table", table, vs64, vs32)
    assert torch.equal(vs.view(-1), table[t])
    v64, v32 = (BR.flame_row_eval(rig, fp_np, t, d)[0].double().numpy() for d in (torch.float64, torch.float32))
    BR.check(f"{what} verts of frame {t}", verts, v64, v32)


def _run_faces(dev, verts_np, faces_np, w, idx_dtype):
    from gaussianavatars_amd import binding as B

    v = _t(verts_np, dev, True)
    outs = B.face_frames(v, torch.as_tensor(faces_np, device=dev).to(idx_dtype))
    loss = sum((o * _t(w[k], dev)).sum() for k, o in zip(("center", "R", "scale", "quat"), outs))
    loss.backward()
    return dict(zip(("center", "R", "scale", "quat"), outs)), v.grad


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("F", [1, 255, 256, 257])
def test_face_frames_forward_backward(F, idx_dtype):
    verts, faces, w, r64, r32 = BR.face_case(F)
    outs, d_verts = _run_faces(_dev(), verts, faces, w, idx_dtype)
    what = f"faces F={F} {str(idx_dtype)[6:]}"
    for k, o in outs.items():
        BR.check(f"{what} {k}", o, r64[k], r32[k])
    BR.check(f"{what} d_verts", d_verts, r64["d_verts"], r32["d_verts"])


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_degenerate_faces_equal_the_float64_reference_exactly(idx_dtype):
    """A repeated vertex (e1 == 0), collinear points (n == 0), e2 parallel to e1 (reversed, and equal): make_frame's clamps.  The coordinates are
    small integers, so every value of the forward is exact in both precisions: the kernel's outputs EQUAL the float64 reference rounded to fp32.
    Gradients: finite, and within the bar of unfused.face_frames' float64 autograd -- its clamp(min=eps) has the constant-length derivative of
    unit_bwd's clamped branch, and |.| has derivative 0 at 0 in both (the reference project's compute_face_orientation is the same composition)."""
    verts, faces, w, r64, r32 = BR.degenerate_case()
    outs, d_verts = _run_faces(_dev(), verts, faces, w, idx_dtype)
    for k, o in outs.items():
        got, want = o.detach().cpu().numpy(), r64[k].astype(np.float32)
        print(f"degenerate {k}: max |kernel - fp32(float64)| = {np.abs(got.astype(np.float64) - want).max():.1e}")
        assert np.array_equal(got, want), f"degenerate faces, {k}:\n{got}\nwant\n{want}"
    assert bool(torch.isfinite(d_verts).all())
    BR.check(f"degenerate {str(idx_dtype)[6:]} d_verts", d_verts, r64["d_verts"], r32["d_verts"])


FORMS = ["atomics", "two-pass", "one-pass"]


def _poison(dev, sizes):
    """NaN-filled blocks of the sizes the bind backward is about to allocate, handed back to the caching allocator: a row the kernels are
    trusted to write ("d_face needs no zero-fill") and do not then most likely reads as NaN instead of as a fresh allocation's zeros."""
    blocks = [torch.full((max(1, n),), float("nan"), dtype=torch.float32, device=dev) for n in sizes]
    torch.cuda.synchronize()
    del blocks


@pytest.mark.parametrize("scaled_quat", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_bind_splats_forward_backward(N, form, scaled_quat):
    from gaussianavatars_amd import binding as B

    dev = _dev()
    leaves, binding_np, w = BR.bind_case(N, scaled_quat)
    r64, r32 = BR.bind_refs(N, scaled_quat)
    L = {k: _t(leaves[k], dev, True) for k in BR.BIND_LEAVES}
    binding = torch.as_tensor(binding_np, device=dev).to(torch.int64 if form == "atomics" else torch.int32)
    csr = None if form == "atomics" else B.binding_csr(binding, BR.BIND_F)
    if form == "one-pass":
        csr = csr[:2]
    outs = B.bind_splats(L["_xyz"], L["_scaling"], L["_rotation"], binding, L["face_R"], L["face_scale"], L["face_center"], L["face_quat"], csr=csr,
                         opacity_logit=L["_opacity"])
    outs = dict(zip(BR.BIND_OUTS, outs))
    loss = sum((outs[k] * _t(w[k], dev)).sum() for k in BR.BIND_OUTS)
    _poison(dev, [3 * N, 3 * N, 4 * N, 17 * BR.BIND_F, N, 20 * N])
    loss.backward()
    what = f"bind N={N} {form} {'scaled' if scaled_quat else 'unit'} quat"
    n = N - 4 if N >= 63 else N          # the saturated logits at the end are held to saturation, not to a relative error
    for k in BR.BIND_OUTS:
        cut = n if k == "opacity" else N
        BR.check(f"{what} {k}", outs[k][:cut], r64[k][:cut], r32[k][:cut])
    for k in BR.BIND_LEAVES:
        g = L[k].grad
        assert g is not None and bool(torch.isfinite(g).all()), f"{what} d{k}"
        cut = n if k == "_opacity" else g.shape[0]
        BR.check(f"{what} d{k}", g[:cut], r64["d_" + k][:cut], r32["d_" + k][:cut])
    if n < N:
        o, g = outs["opacity"][n:, 0].tolist(), L["_opacity"].grad[n:, 0].tolist()
        for x, oi, gi, o64, g64 in zip(BR.SATURATED, o, g, r64["opacity"][n:, 0], r64["d__opacity"][n:, 0]):
            print(f"{what} sigmoid({x:+.0f}) = {oi!r} (float64 {o64:.3e}), gradient {gi!r} (float64 {g64:.3e})")
            assert np.isfinite(oi) and np.isfinite(gi)
            assert (oi == 1.0) if x > 0 else (0.0 <= oi <= 1e-37), f"{what}: sigmoid({x}) = {oi}"
            assert abs(gi) <= 1e-36
            assert abs(oi - o64) <= 1e-37 and abs(gi - g64) <= 1e-36
    # faces that own no splat: every form writes their rows, as zeros
    counts = np.bincount(binding_np, minlength=BR.BIND_F)
    empty = torch.as_tensor(np.nonzero(counts == 0)[0], device=dev)
    assert len(empty) >= len(BR.BIND_EMPTY)
    for k in ("face_center", "face_R", "face_scale", "face_quat"):
        assert float(L[k].grad[empty].abs().max()) == 0.0, f"{what}: d_{k} of an empty face is not exactly zero"
