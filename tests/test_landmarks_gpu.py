"""Landmarks and the root-centred output of FlameHead.forward on the kernels (include/gab_landmarks.h: gab_landmarks_forward / _backward,
gab_root_joint, gab_root_center / _backward; gaussianavatars_amd/binding.py: landmarks, root_center, flame_head_outputs).

Two kinds of bars, none taken from a kernel's output:
  * derived: a kernel against the float64 value of ITS OWN formula on ITS OWN fp32 inputs, bounded by the roundings the formula has
    (stated at each assertion, in units of u = 2^-24);
  * the reference's recorded float64 outputs (tests/golden/landmark_pins.npz) and float64 autograd of unfused.py, at the bar of
    tests/test_binding_parity_gpu.py:9-10,51 -- binding_ref.check: row by row, FLAME_ROW_FACTOR x what unfused.py loses in fp32 on the CPU
    on the same inputs, floor FLAME_ROW_FLOOR.
No test launches an embedding the host check refuses (tests/test_landmarks_cpu.py covers the check itself)."""
import functools

import numpy as np
import pytest
import torch

from tests import binding_ref as BR
from tests import landmark_cases as LC
from tests.test_binding_gpu import _dev, _Head

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24


def _t(a, dev, grad=False):
    return torch.as_tensor(a, device=dev).clone().requires_grad_(grad)


class _Mesh:
    """The least the two landmark entries read from a head: a vertex count, faces and the embedding."""

    def __init__(self, V, faces, idx, bary, dev, idx_dtype=torch.int64):
        self.v_template = torch.zeros((V, 3), dtype=torch.float32, device=dev)
        self.faces = torch.as_tensor(faces, device=dev).to(idx_dtype)
        self.full_lmk_faces_idx = torch.as_tensor(idx, dtype=torch.long, device=dev)
        self.full_lmk_bary_coords = torch.as_tensor(bary, dtype=torch.float32, device=dev).reshape(-1, 3)


def _full_head(dev):
    rig = LC.rig()
    head = _Head(rig, dev, 300)
    idx, bary = LC.embedding()
    head.faces = torch.as_tensor(rig["faces"], device=dev)
    head.full_lmk_faces_idx, head.full_lmk_bary_coords = torch.as_tensor(idx, device=dev), torch.as_tensor(bary, device=dev)
    return head


def _formula64(verts, faces, idx, bary):
    """(landmarks, sum_k |bary_k v_k|) of lbs.py:86-97 in float64 numpy, on whatever vertices it is given."""
    v, b = np.asarray(verts, np.float64), np.asarray(bary, np.float64).reshape(-1, 3)
    terms = v[np.asarray(faces)[np.asarray(idx).reshape(-1)]] * b[:, :, None]      # (L, 3 corners, 3)
    return terms.sum(1), np.abs(terms).sum(1)


def _check_forward_bound(what, got, verts, faces, idx, bary):
    """three rounded products and two rounded adds (the fmaf chain has fewer): |err| <= 4 u sum_k |bary_k v_k| per coordinate."""
    want, mag = _formula64(verts, faces, idx, bary)
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want)
    worst = float((err / np.maximum(mag, 1e-300)).max()) / U24 if want.size else 0.0
    print(f"{what}: worst |err| / (u sum|terms|) = {worst:.3f} (bound 4)")
    assert np.isfinite(got).all() and (err <= 4 * U24 * mag).all(), what


def _backward64(V, faces, idx, bary, g):
    """(d_verts, sum |terms|, row length) per vertex, float64."""
    f, idx, b, g = np.asarray(faces), np.asarray(idx).reshape(-1), np.asarray(bary, np.float64).reshape(-1, 3), np.asarray(g, np.float64).reshape(-1, 3)
    d, mag, n = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    for l in range(idx.shape[0]):
        for k in range(3):
            v = f[idx[l], k]
            d[v] += b[l, k] * g[l]
            mag[v] += np.abs(b[l, k] * g[l])
            n[v] += 1
    return d, mag, n


def _check_backward_bound(what, got, V, faces, idx, bary, g):
    """a row of n fused multiply-adds: |err| <= (n + 1) u sum |terms| per vertex and coordinate; vertices no landmark touches are exactly zero."""
    want, mag, n = _backward64(V, faces, idx, bary, g)
    got = got.detach().double().cpu().numpy().reshape(V, 3)
    err = np.abs(got - want)
    bound = (n[:, None] + 1) * U24 * mag
    touched = n > 0
    worst = float((err[touched] / np.maximum(bound[touched], 1e-300)).max()) if touched.any() else 0.0
    print(f"{what}: {int(touched.sum())} touched vertices, longest row {int(n.max()) if n.size else 0}, worst |err| / bound = {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), what
    assert (got[~touched] == 0.0).all(), f"{what}: a vertex no landmark touches has a gradient"


# ---- the pins' poses on the full-size rig -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu32(pose, rc):
    """unfused.py in fp32 on the CPU (the yardstick of binding_ref.check) -> (verts rows, landmarks) as float64 numpy; computed once, shared."""
    rig, p = LC.rig(), LC.pose_inputs(pose)
    idx, bary = LC.embedding()
    verts, _, lm, _ = LC.unfused_eval(rig, p, rig["faces"], idx, bary, torch.float32, zero_centered=rc)
    return verts[0].double().numpy()[LC.pins()["vert_rows"]], lm[0].double().numpy()


def _run_pose(dev, head, pose, rc):
    from gaussianavatars_amd import binding as B

    p = LC.pose_inputs(pose)
    L = {k: _t(p[k], dev) for k in LC.LEAVES}
    return B.flame_head_outputs(head, *[L[k] for k in LC.LEAVES[:-1]], L["static_offset"], zero_centered_at_root_node=rc, return_landmarks=True,
                                return_verts_cano=True)


@pytest.mark.parametrize("pose", LC.POSES)
def test_forward_parity_on_the_pinned_poses(pose):
    dev = _dev()
    head, z, rig = _full_head(dev), LC.pins(), LC.rig()
    idx, bary = LC.embedding()
    verts, vs, lm = _run_pose(dev, head, pose, False)
    assert tuple(lm.shape) == (1, 70, 3) and tuple(verts.shape) == (1, 5143, 3)
    _check_forward_bound(f"landmarks {pose}", lm, verts[0].cpu().numpy(), rig["faces"], idx, bary)
    v32, lm32 = _cpu32(pose, False)
    BR.check(f"landmarks {pose} vs pins", lm, z[pose + "_landmarks"][None], lm32[None])
    BR.check(f"verts {pose} vs pins", verts[0, torch.as_tensor(z["vert_rows"], device=dev)], z[pose + "_verts"], v32)


@pytest.mark.parametrize("pose", LC.POSES)
def test_root_centring_on_the_pinned_poses(pose):
    from gaussianavatars_amd import binding as B

    dev = _dev()
    head, z, rig = _full_head(dev), LC.pins(), LC.rig()
    idx, bary = LC.embedding()
    verts, vs, lm = _run_pose(dev, head, pose, True)
    # the root joint against the float64 dot on the kernel's own inputs: V fused multiply-adds in some fixed order, |err| <= V u sum_v |J[0][v] v_shaped[v][c]|
    root = B.root_joint(head, vs)
    terms = rig["J_regressor"][0].astype(np.float64)[:, None] * vs[0].double().cpu().numpy()
    err = np.abs(root.double().cpu().numpy() - terms.sum(0))
    bound = terms.shape[0] * U24 * np.abs(terms).sum(0)
    print(f"root {pose}: |err| {err.max():.2e}, bound {bound.min():.2e}, |root - pinned root| {np.abs(root.double().cpu().numpy() - z[pose + '_root']).max():.2e}")
    assert (err <= bound).all()
    v32, lm32 = _cpu32(pose, True)
    rows = torch.as_tensor(z["vert_rows"], device=dev)
    BR.check(f"root-centred verts {pose} vs pins", verts[0, rows], z[pose + "_verts_rc"], v32)
    BR.check(f"root-centred landmarks {pose} vs pins", lm, z[pose + "_landmarks_rc"][None], lm32[None])
    _check_forward_bound(f"root-centred landmarks {pose}", lm, verts[0].cpu().numpy(), rig["faces"], idx, bary)
    # the same bits run after run
    verts2, vs2, lm2 = _run_pose(dev, head, pose, True)
    assert torch.equal(B.root_joint(head, vs2), root) and torch.equal(verts2, verts) and torch.equal(lm2, lm)


# ---- edge embeddings ------------------------------------------------------------------------------------------------------------------
def _edge_mesh():
    rig = BR.small_rig(257, 3, 5, 1)
    g = np.random.default_rng(77)
    return (rig["v_template"] + g.normal(0, 2e-3, rig["v_template"].shape)).astype(np.float32), rig["faces"]   # 257 vertices (two blocks), 514 faces


def _edge_embeddings(F):
    g = np.random.default_rng(78)

    def bary(n):
        b = g.uniform(0.05, 1.0, (n, 3))
        return (b / b.sum(1, keepdims=True)).astype(np.float32)

    return {
        "L=1": (np.array([F // 2]), bary(1)),
        "L=0": (np.zeros((0,), np.int64), np.zeros((0, 3), np.float32)),
        "first and last face": (np.array([0, F - 1, F - 1, 0]), bary(4)),
        "bary (1,0,0)": (np.array([3, 4, 5]), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)),
        "100 landmarks on one face": (np.full((100,), 17), bary(100)),            # 300 lanes: two blocks of the forward, one row of 100 per corner
    }


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("case", ["L=1", "L=0", "first and last face", "bary (1,0,0)", "100 landmarks on one face"])
def test_edge_embeddings(case, idx_dtype):
    from gaussianavatars_amd import binding as B

    dev = _dev()
    verts_np, faces = _edge_mesh()
    idx, bary = _edge_embeddings(faces.shape[0])[case]
    head = _Mesh(verts_np.shape[0], faces, idx, bary, dev, idx_dtype)
    v = _t(verts_np, dev, True)
    lm = B.landmarks(head, v)
    assert tuple(lm.shape) == (len(idx), 3) and lm.dtype == torch.float32
    what = f"{case} {str(idx_dtype)[6:]}"
    _check_forward_bound(what, lm, verts_np, faces, idx, bary)
    if case == "bary (1,0,0)":   # a landmark ON a vertex is that vertex, bit for bit
        assert torch.equal(lm.detach(), v.detach()[torch.as_tensor(faces[[3, 4, 5], [0, 1, 2]], device=dev)])
    g = np.random.default_rng(79).normal(0, 1.0, (len(idx), 3)).astype(np.float32)
    (lm * _t(g, dev)).sum().backward()
    assert tuple(v.grad.shape) == tuple(v.shape)
    _check_backward_bound(f"{what} d_verts", v.grad, verts_np.shape[0], faces, idx, bary, g)
    lm_b = B.landmarks(head, v.detach()[None])        # the (1,V,3) layout of FlameHead's vertices
    assert tuple(lm_b.shape) == (1, len(idx), 3) and torch.equal(lm_b[0], lm.detach())


# ---- the backward on its own ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shared", "real"])
def test_landmark_backward(which):
    from gaussianavatars_amd import binding as B

    dev = _dev()
    if which == "shared":
        V, faces, idx, bary = LC.SHARED_V, LC.SHARED_FACES, LC.SHARED_LMK_FACE, LC.SHARED_LMK_BARY
    else:
        rig = LC.rig()
        V, faces = rig["v_template"].shape[0], rig["faces"]
        idx, bary = LC.embedding()
    head = _Mesh(V, faces, idx, bary, dev)
    rng = np.random.default_rng(80)
    g = rng.normal(0, 1.0, (len(idx), 3)).astype(np.float32)
    base = rng.normal(0, 1.0, (V, 3)).astype(np.float32)
    blocks = [torch.full((3 * V,), float("nan"), device=dev) for _ in range(2)]   # what a fresh allocation may hold: accumulate = 0 must write every row
    torch.cuda.synchronize()
    del blocks
    d0 = B.landmarks_backward(head, _t(g, dev))
    _check_backward_bound(f"{which} embedding d_verts", d0, V, faces, idx, bary, g)
    # against float64 autograd of the restated formula (the issue's reference), same bound
    from gaussianavatars_amd import unfused as U

    v64 = torch.zeros((1, V, 3), dtype=torch.float64, requires_grad=True)
    (U.landmarks(v64, torch.as_tensor(faces), torch.as_tensor(idx), torch.as_tensor(bary).double())[0] * torch.as_tensor(g).double()).sum().backward()
    want, mag, n = _backward64(V, faces, idx, bary, g)
    assert np.abs(v64.grad[0].numpy() - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
    assert (np.abs(d0.double().cpu().numpy() - v64.grad[0].numpy()) <= (n[:, None] + 1) * U24 * mag + 1e-15).all()
    # accumulate = 1 onto a non-zero buffer: the row sums are formed first and added once, so the result IS base + d0 in fp32
    into = _t(base, dev)
    out = B.landmarks_backward(head, _t(g, dev), into=into)
    assert out is into and torch.equal(into, _t(base, dev) + d0)
    # twice: the same bits
    assert torch.equal(B.landmarks_backward(head, _t(g, dev)), d0)
    into2 = _t(base, dev)
    B.landmarks_backward(head, _t(g, dev), into=into2)
    assert torch.equal(into2, into)


# ---- end to end through FlameHead.forward -------------------------------------------------------------------------------------------------
PER_FRAME = ("expr", "rotation", "neck_pose", "jaw_pose", "eyes_pose", "translation")


def _loss(verts, lm, rc, w):
    if rc:   # root centring: a weighted sum, so that the sum over the vertices (what reaches the root joint) does not vanish by symmetry
        return (verts * w).sum() + lm.square().sum()
    return lm.square().sum() + verts.sum()


@functools.lru_cache(maxsize=None)
def _e2e_refs(with_shape, rc):
    """float64 and CPU-fp32 autograd of the unfused path on the small case -> two dicts (verts, landmarks, d_<leaf>); computed once, shared."""
    rig, p, idx, bary = LC.small_case()
    wanted = LC.LEAVES if with_shape else PER_FRAME
    out = []
    for dtype in (torch.float64, torch.float32):
        leaves = {k: torch.as_tensor(p[k]).to(dtype).requires_grad_(k in wanted) for k in LC.LEAVES}
        verts, vs, lm, _ = LC.unfused_eval(rig, p, rig["faces"], idx, bary, dtype, zero_centered=rc, leaves=leaves)
        w = torch.as_tensor(BR.flame_case(257, 10, 100, "random")[2]["verts"]).to(dtype)
        gs = torch.autograd.grad(_loss(verts, lm, rc, w), [leaves[k] for k in wanted])
        r = dict(verts=verts.detach().double().numpy(), landmarks=lm.detach().double().numpy())
        r.update({"d_" + k: g.double().numpy() for k, g in zip(wanted, gs)})
        out.append(r)
    return tuple(out)


def _small_head(dev, attach=True):
    from gaussianavatars_amd.gaussian_model import FlameHead

    rig, p, idx, bary = LC.small_case()
    head = FlameHead(rig).to(dev)
    head.n_shape_params = 10          # (the mirror's constructor assumes FLAME's 300)
    if attach:
        head.attach_landmarks(idx[None], bary[None])
    return head, p


def _forward(head, L, **kw):
    return head(L["shape"], L["expr"], L["rotation"], L["neck_pose"], L["jaw_pose"], L["eyes_pose"], L["translation"], static_offset=L["static_offset"], **kw)


@pytest.mark.parametrize("rc", [False, True], ids=["face-centred", "root-centred"])
@pytest.mark.parametrize("with_shape", [False, True], ids=["per-frame leaves", "shape and static_offset too"])
def test_end_to_end_gradients(with_shape, rc):
    """loss = landmarks.square().sum() + vertices.sum() through FlameHead.forward(return_landmarks=True) (root-centred: a weighted sum of the vertices):
    gradients of expr, rotation, neck, jaw, eyes and translation -- and of shape and static_offset in the second case -- against float64
    autograd of the unfused path, at the bar of tests/test_binding_parity_gpu.py:58 (binding_ref.check)."""
    dev = _dev()
    head, p = _small_head(dev)
    wanted = LC.LEAVES if with_shape else PER_FRAME
    L = {k: _t(p[k], dev, k in wanted) for k in LC.LEAVES}
    verts, lm = _forward(head, L, zero_centered_at_root_node=rc)
    assert lm.grad_fn is not None and type(lm.grad_fn).__name__.startswith("_Landmarks"), "the landmarks did not come from the kernels"
    w = _t(BR.flame_case(257, 10, 100, "random")[2]["verts"], dev)
    _loss(verts, lm, rc, w).backward()
    r64, r32 = _e2e_refs(with_shape, rc)
    what = f"e2e {'root' if rc else 'face'}-centred {'+shape' if with_shape else 'per-frame'}"
    BR.check(f"{what} verts", verts, r64["verts"], r32["verts"])
    BR.check(f"{what} landmarks", lm, r64["landmarks"], r32["landmarks"])
    for k in LC.LEAVES:
        if k not in wanted:
            assert L[k].grad is None
            continue
        assert L[k].grad is not None and bool(torch.isfinite(L[k].grad).all()), f"{what} d_{k}"
        BR.check(f"{what} d_{k}", L[k].grad, r64["d_" + k], r32["d_" + k])
    # the same bits run after run
    L2 = {k: _t(p[k], dev, k in wanted) for k in LC.LEAVES}
    verts2, lm2 = _forward(head, L2, zero_centered_at_root_node=rc)
    _loss(verts2, lm2, rc, w).backward()
    assert torch.equal(verts2, verts) and torch.equal(lm2, lm)
    if rc:   # (the face-centred FLAME backward accumulates with atomics: its bits are the existing tests' business)
        for k in ("translation",):
            assert torch.equal(L2[k].grad, L[k].grad), k


def test_default_call_needs_an_embedding_and_returns_the_reference_list():
    dev = _dev()
    head, p = _small_head(dev, attach=False)
    L = {k: _t(p[k], dev) for k in LC.LEAVES}
    with pytest.raises(ValueError, match="attach_landmarks"):
        _forward(head, L)
    _, _, idx, bary = LC.small_case()
    head.attach_landmarks(idx, bary)
    out = _forward(head, L, return_verts_cano=True)
    assert [tuple(o.shape) for o in out] == [(1, 257, 3), (1, 257, 3), (1, 70, 3)]
    assert isinstance(_forward(head, L, return_landmarks=False, zero_centered_at_root_node=True), torch.Tensor)


def test_the_per_frame_path_is_unchanged_by_an_attached_embedding():
    """FlameHead.forward(return_landmarks=False) before and after attach_landmarks: torch.equal vertices, v_shaped and gradients.  On the
    37-vertex rig: the existing FLAME backward accumulates with float atomics, and at this size every accumulator receives at most two
    non-zero addends (one workgroup per kernel, one wave with vertices), whose order cannot change the sum -- so equal bits are what an
    unchanged path gives, run after run."""
    from gaussianavatars_amd.gaussian_model import FlameHead

    dev = _dev()
    rig, p, wts = BR.flame_case(37, 3, 5, "random")
    head = FlameHead(rig).to(dev)
    head.n_shape_params = 3
    idx, bary = LC.embedding()
    w = _t(wts["verts"], dev)

    def run():
        L = {k: _t(p[k], dev, k in PER_FRAME) for k in LC.LEAVES}
        verts, cano = _forward(head, L, return_landmarks=False, return_verts_cano=True)
        (verts * w).sum().backward()
        return verts.detach(), cano.detach(), {k: L[k].grad for k in PER_FRAME}

    v0, c0, g0 = run()
    head.attach_landmarks(idx % rig["faces"].shape[0], bary)
    v1, c1, g1 = run()
    assert torch.equal(v0, v1) and torch.equal(c0, c1)
    for k in PER_FRAME:
        assert g0[k] is not None and torch.equal(g0[k], g1[k]), k
    lm = _forward(head, {k: _t(p[k], dev) for k in LC.LEAVES})[1]       # and the embedding is live
    assert tuple(lm.shape) == (1, 70, 3)
