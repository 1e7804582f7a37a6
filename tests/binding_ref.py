"""The binding half (include/gab.h) in float64: gaussianavatars_amd/unfused.py -- the project's statement of the reference semantics, pinned to
the reference's own classes by tests/golden/binding_pins.npz -- run on CPU float64 tensors, gradients by torch autograd in float64, plus sigmoid
for the opacity path.  TEST INFRASTRUCTURE: no mathematics of its own.  Inputs are the fp32 arrays the kernels get, widened exactly.

Also the input sets shared by tests/test_binding_ref_cpu.py (which checks their conditioning) and tests/test_binding_parity_gpu.py (which runs
them through the kernels): rigs of any size (small_rig), pose edge cases, face sets, splat sets with empty and crowded faces.

The yardstick (row_err, bar): a kernel's output is compared row by row with the float64 value; the bar of a comparison is FLAME_ROW_FACTOR times
what unfused.py itself loses when it is run in fp32 ON THE CPU on the same inputs, never below FLAME_ROW_FLOOR (the rule of
tests/test_fullsize_gpu.py::_flame_row_bars, its two numbers imported, not re-chosen).  No bar is derived from a kernel's output."""
import functools
import math

import numpy as np
import torch

from gaussianavatars_amd import unfused as U
from tests.test_fullsize_gpu import FLAME_ROW_FACTOR as FACTOR
from tests.test_fullsize_gpu import FLAME_ROW_FLOOR as FLOOR

RIG_BUFFERS = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")
FLAME_LEAVES = ("shape", "expr", "rotation", "neck_pose", "jaw_pose", "eyes_pose", "translation", "static_offset")
FLAME_ROWS = ("expr", "rotation", "neck_pose", "jaw_pose", "eyes_pose", "translation")
PARENTS = (-1, 0, 1, 1, 1)

# ------------------------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------------------------------------------------
TABLE = []   # (name, err, fp32_dev, bar) of every comparison made in this process, in order


def rows_of(a):
    """A (1, V, 3) batch-1 tensor is compared vertex by vertex; everything else by its own first axis."""
    a = np.asarray(a)
    return a[0] if a.ndim == 3 and a.shape[0] == 1 and a.shape[2] == 3 else a


def row_err(got, ref):
    """Worst row i (first axis) of max|got_i - ref_i| / (max|ref_i| + 1e-3 max|ref|).  The 1e-3 is a condition, not a measurement: a thousand
    times finer per row than a whole-tensor relative error, while a row that is pure cancellation noise does not divide by zero."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    g, r = got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    num = np.abs(g - r).max(1)
    den = np.abs(r).max(1) + 1e-3 * np.abs(r).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(num == 0.0, 0.0, num / den)
    return float(e.max())


def bar(name, fp32_dev):
    return max(FLOOR, FACTOR * fp32_dev)


def check(name, got, ref64, ref32):
    """`got` (the kernel's) against `ref64`, held to bar(row_err(ref32, ref64)); prints name, err, fp32_dev, bar before it asserts."""
    if isinstance(got, torch.Tensor):
        got = got.detach().cpu().numpy()
    got, ref64, ref32 = rows_of(got), rows_of(ref64), rows_of(ref32)
    err, dev = row_err(got.reshape(ref64.shape), ref64), row_err(ref32, ref64)
    b = bar(name, dev)
    TABLE.append((name, err, dev, b))
    print(f"{name}: err {err:.2e}  fp32_dev {dev:.2e}  bar {b:.2e}")
    assert err < b, f"{name}: row err {err:.2e} (bar {b:.2e} = max({FLOOR:g}, {FACTOR:g} x {dev:.2e}))"


def _np64(t):
    return t.detach().double().cpu().numpy()


def _grads(loss, leaves):
    gs = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
    return {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(leaves.items(), gs)}


# ------------------------------------------------------------------------------------------------------------------------------------------
# rigs
# ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_rig(V, n_shape, n_expr, seed=0):
    """A rig with the schema of synthetic.flame_rig at any V: random points on the ellipsoid, smooth blend directions, Gaussian J_regressor and
    lbs_weights, the FLAME tree; and 2V triangles on it (each vertex with two pairs of its nearest neighbours, random winding)."""
    g = np.random.default_rng(1000 * seed + V)
    d = g.normal(size=(V, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    vt = d * np.array([0.8, 1.0, 0.9]) * 0.12
    NB = n_shape + n_expr
    u = vt / 0.12
    basis = np.concatenate([u, np.sin(3.0 * u), np.cos(2.0 * u)], 1)
    shapedirs = (basis @ g.normal(0.0, 1.0, (9, 3 * NB))).reshape(V, 3, NB) * (2e-3 / 3.0) + g.normal(0.0, 2e-4, (V, 3, NB))
    posedirs = g.normal(0.0, 1e-3, (36, 3 * V))
    joints = np.array([[0, -0.10, 0], [0, -0.05, 0], [0, -0.02, 0.03], [0.03, 0.04, 0.08], [-0.03, 0.04, 0.08]], np.float64)
    J_regressor, lbs_weights = np.zeros((5, V)), np.zeros((V, 5))
    for j in range(5):
        d2 = ((vt - joints[j]) ** 2).sum(1)
        near = np.argsort(d2)[: min(50, V)]
        w = np.exp(-d2[near] / (2 * 0.02 ** 2))
        J_regressor[j, near] = w / w.sum()
        lbs_weights[:, j] = np.exp(-d2 / (2 * (0.06 if j < 3 else 0.015) ** 2))
    lbs_weights[:, 0] += 1e-3
    lbs_weights /= lbs_weights.sum(1, keepdims=True)
    faces = []
    for f in range(2 * V):
        i = f % V
        nb = np.argsort(((vt - vt[i]) ** 2).sum(1))[1:5]
        a, b = (nb[0], nb[1]) if f < V else (nb[2], nb[3])
        faces.append((i, a, b) if g.random() < 0.5 else (i, b, a))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(v_template=f32(vt), shapedirs=f32(shapedirs), posedirs=f32(posedirs), J_regressor=f32(J_regressor), lbs_weights=f32(lbs_weights),
                parents=np.asarray(PARENTS, np.int64), faces=np.asarray(faces, np.int64), n_shape=n_shape, n_expr=n_expr)


def _torch_rig(rig, dtype):
    r = {k: torch.as_tensor(rig[k]).to(dtype) for k in RIG_BUFFERS}
    r["parents"] = torch.as_tensor(rig["parents"])
    return r


# ------------------------------------------------------------------------------------------------------------------------------------------
# FLAME forward / backward
# ------------------------------------------------------------------------------------------------------------------------------------------
POSE_SETS = ("random", "zero", "eyes_neck_zero", "large", "tiny")


@functools.lru_cache(maxsize=None)
def flame_case(V, n_shape, n_expr, pose="random", seed=0):
    """(rig, params, weights): batch-1 FLAME inputs in the reference's shapes and the two loss weights (on verts; 0.1 x on v_shaped).
    pose: random -- five rotations of ~0.3 rad; zero -- all five exactly zero; eyes_neck_zero -- eyes and neck exactly zero, the others of norm
    0.3; large -- a global rotation of norm 2.5 about a generic axis, a jaw of norm 0.6 with three non-zero components; tiny -- one component
    of each rotation 1e-4, the others zero (the small-angle regime)."""
    rig = small_rig(V, n_shape, n_expr, seed)
    g = np.random.default_rng(7000 + 10 * V + POSE_SETS.index(pose))
    unit = lambda n: (lambda x: x / np.linalg.norm(x))(g.normal(size=n))
    p = dict(shape=g.normal(0, 1.0, (1, n_shape)), expr=g.normal(0, 0.7, (1, n_expr)), rotation=0.3 * unit(3)[None], neck_pose=0.3 * unit(3)[None],
             jaw_pose=0.3 * unit(3)[None], eyes_pose=np.concatenate([0.3 * unit(3), 0.3 * unit(3)])[None], translation=g.normal(0, 0.01, (1, 3)),
             static_offset=g.normal(0, 2e-4, (1, V, 3)))
    if pose == "zero":
        for k in ("rotation", "neck_pose", "jaw_pose", "eyes_pose"):
            p[k] = np.zeros_like(p[k])
    elif pose == "eyes_neck_zero":
        p["eyes_pose"], p["neck_pose"] = np.zeros((1, 6)), np.zeros((1, 3))
    elif pose == "large":
        p["rotation"] = 2.5 * (np.array([0.48, -0.62, 0.62]) / np.linalg.norm([0.48, -0.62, 0.62]))[None]
        p["jaw_pose"] = 0.6 * (np.array([0.7, 0.5, -0.51]) / np.linalg.norm([0.7, 0.5, -0.51]))[None]
    elif pose == "tiny":
        for i, k in enumerate(("rotation", "neck_pose", "jaw_pose")):
            p[k] = np.zeros((1, 3))
            p[k][0, i] = 1e-4
        p["eyes_pose"] = np.zeros((1, 6))
        p["eyes_pose"][0, 1] = p["eyes_pose"][0, 5] = 1e-4
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    w = dict(verts=g.normal(0, 1.0, (1, V, 3)).astype(np.float32), v_shaped=(0.1 * g.normal(0, 1.0, (1, V, 3))).astype(np.float32))
    return rig, p, w


def flame_eval(rig, p, w, dtype):
    """unfused.flame_forward in `dtype` on the CPU -> verts, v_shaped, d_<leaf> (loss: w.verts . verts + w.v_shaped . v_shaped) and dv_<leaf>
    (loss on verts only), as float64 numpy."""
    leaves = {k: torch.as_tensor(p[k]).to(dtype).requires_grad_(True) for k in FLAME_LEAVES}
    verts, vs = U.flame_forward(_torch_rig(rig, dtype), leaves["shape"], leaves["expr"], leaves["rotation"], leaves["neck_pose"], leaves["jaw_pose"],
                                leaves["eyes_pose"], leaves["translation"], leaves["static_offset"])
    lv = (verts * torch.as_tensor(w["verts"]).to(dtype)).sum()
    ls = (vs * torch.as_tensor(w["v_shaped"]).to(dtype)).sum()
    gv, gs = _grads(lv, leaves), _grads(ls, leaves)
    out = dict(verts=_np64(verts), v_shaped=_np64(vs))
    for k in FLAME_LEAVES:
        out["dv_" + k] = _np64(gv[k])
        out["d_" + k] = _np64(gv[k] + gs[k])
    return out


@functools.lru_cache(maxsize=None)
def flame_refs(V, n_shape, n_expr, pose="random", seed=0):
    """(float64 result, fp32-on-the-CPU result) of a flame_case: computed once, shared, not modified."""
    rig, p, w = flame_case(V, n_shape, n_expr, pose, seed)
    return flame_eval(rig, p, w, torch.float64), flame_eval(rig, p, w, torch.float32)


@functools.lru_cache(maxsize=None)
def sequence_case(V, n_shape, n_expr, T, seed=0):
    """A rig, a flame_param dict (npz schema) of T frames, and the float64 / CPU-fp32 v_shaped of every frame, (T, 3V)."""
    rig = small_rig(V, n_shape, n_expr, seed)
    fp = flame_tables(V, n_shape, n_expr, T, seed=300 + T)
    both = []
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.as_tensor(a).to(dtype)
        z = torch.zeros((T, 3), dtype=dtype)
        _, vs = U.flame_forward(_torch_rig(rig, dtype), t(fp["shape"])[None].expand(T, -1), t(fp["expr"]), z, z, z, torch.zeros((T, 6), dtype=dtype), z,
                                t(fp["static_offset"]))
        both.append(_np64(vs).reshape(T, 3 * V))
    return rig, fp, both[0], both[1]


def flame_tables(V, n_shape, n_expr, T, seed=0):
    g = np.random.default_rng(9000 + seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(shape=f32(g.normal(0, 1.0, (n_shape,))), expr=f32(g.normal(0, 0.7, (T, n_expr))), rotation=f32(g.normal(0, 0.2, (T, 3))),
                neck_pose=f32(g.normal(0, 0.15, (T, 3))), jaw_pose=f32(g.normal(0, 0.15, (T, 3))), eyes_pose=f32(g.normal(0, 0.15, (T, 6))),
                translation=f32(g.normal(0, 0.01, (T, 3))), static_offset=f32(g.normal(0, 2e-4, (1, V, 3))))


def flame_row_eval(rig, fp, t, dtype):
    """Frame t of a flame_param table through unfused.flame_forward -> (verts (1,V,3), v_shaped), `dtype` torch tensors (no gradients)."""
    c = lambda a: torch.as_tensor(a).to(dtype)
    return U.flame_forward(_torch_rig(rig, dtype), c(fp["shape"])[None], *[c(fp[k][[t]]) for k in FLAME_ROWS], c(fp["static_offset"]))


# ------------------------------------------------------------------------------------------------------------------------------------------
# face frames
# ------------------------------------------------------------------------------------------------------------------------------------------
def quat_branches(R):
    """(branch (F,), margin (F,)) of rotmat_to_unitquat's argmax(R00, R11, R22, trace): margin = largest - second largest."""
    R = np.asarray(R, np.float64)
    dec = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]], 1)
    s = np.sort(dec, 1)
    return dec.argmax(1), s[:, 3] - s[:, 2]


def degenerate(verts, faces):
    """Faces on which one of make_frame's three clamps is active (|e1|^2, |a0 x e2|^2 or |a1 x a0|^2 below 1e-20), in float64."""
    v = np.asarray(verts, np.float64)
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    q1 = (e1 * e1).sum(1)
    a0 = e1 / np.sqrt(np.maximum(q1, 1e-20))[:, None]
    n = np.cross(a0, e2)
    qn = (n * n).sum(1)
    m = np.cross(n / np.sqrt(np.maximum(qn, 1e-20))[:, None], a0)
    return (q1 < 1e-20) | (qn < 1e-20) | ((m * m).sum(1) < 1e-20)


def face_eval(verts, faces, w, dtype):
    """unfused.face_frames in `dtype` -> center, R, scale, quat, d_verts (loss: sum of w[k] . output k)."""
    v = torch.as_tensor(verts).to(dtype).requires_grad_(True)
    outs = U.face_frames(v, torch.as_tensor(faces).long())
    loss = sum((o * torch.as_tensor(w[k]).to(dtype)).sum() for k, o in zip(("center", "R", "scale", "quat"), outs))
    (g,) = torch.autograd.grad(loss, [v])
    out = {k: _np64(o) for k, o in zip(("center", "R", "scale", "quat"), outs)}
    out["d_verts"] = _np64(g)
    return out


def face_weights(F, seed):
    g = np.random.default_rng(4000 + seed)
    return {k: g.normal(0, 1.0, s).astype(np.float32) for k, s in (("center", (F, 3)), ("R", (F, 3, 3)), ("scale", (F, 1)), ("quat", (F, 4)))}


FACE_SEED = 1   # (changed until condition (a) of tests/test_binding_ref_cpu.py held on the 257 faces; the check itself is not loosened)


@functools.lru_cache(maxsize=None)
def face_case(F):
    """The first F of the 2 x 257 small_rig triangles on perturbed vertices -> (verts, faces int64, weights, float64 result, CPU fp32 result)."""
    rig = small_rig(257, 3, 5, FACE_SEED)
    g = np.random.default_rng(50 + FACE_SEED)
    verts = (rig["v_template"] + g.normal(0, 2e-3, rig["v_template"].shape)).astype(np.float32)
    faces = rig["faces"][:F]
    w = face_weights(F, F)
    return verts, faces, w, face_eval(verts, faces, w, torch.float64), face_eval(verts, faces, w, torch.float32)


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """Hand-built faces on small-integer / power-of-two vertices (fp32 and fp64 take the same clamps, bit for bit): a repeated vertex index
    (e1 == 0), three collinear points (n == 0), e2 parallel to e1 and reversed; and two faces whose frames are exact in fp32."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [1, 0, -2], [1, 0, 2]], np.float32)
    faces = np.array([[3, 3, 1], [0, 1, 2], [0, 1, 4], [0, 2, 2], [0, 2, 5], [0, 2, 6]], np.int64)
    #                  e1 == 0    collinear  reversed   e2 == e1   R = I      R = diag(1, -1, -1)
    w = face_weights(len(faces), 99)
    return verts, faces, w, face_eval(verts, faces, w, torch.float64), face_eval(verts, faces, w, torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------------------
# mesh_frames_timestep (FLAME forward + face frames as one node)
# ------------------------------------------------------------------------------------------------------------------------------------------
MESH_CASES = {(37, 60): (3, 5, 0), (257, 500): (10, 100, 0)}   # (V, F) -> (n_shape, n_expr, seed); seeds changed until condition (a) held
MESH_T, MESH_ROW = 3, 1


def mesh_eval(rig, fp, faces, w, dtype):
    c = lambda a: torch.as_tensor(a).to(dtype)
    rows = {k: c(fp[k][[MESH_ROW]]).requires_grad_(True) for k in FLAME_ROWS}
    verts, vs = U.flame_forward(_torch_rig(rig, dtype), c(fp["shape"])[None], *[rows[k] for k in FLAME_ROWS], c(fp["static_offset"]))
    outs = U.face_frames(verts[0], torch.as_tensor(faces).long())
    loss = sum((o * c(w[k])).sum() for k, o in zip(("center", "R", "scale", "quat"), outs)) + (verts * c(w["verts"])).sum()
    g = _grads(loss, rows)
    out = {k: _np64(o) for k, o in zip(("center", "R", "scale", "quat"), outs)}
    out.update(verts=_np64(verts), v_shaped=_np64(vs))
    out.update({"d_" + k: _np64(g[k]) for k in FLAME_ROWS})
    return out


@functools.lru_cache(maxsize=None)
def mesh_case(V, F):
    n_shape, n_expr, seed = MESH_CASES[(V, F)]
    rig = small_rig(V, n_shape, n_expr, seed)
    fp = flame_tables(V, n_shape, n_expr, MESH_T, seed=seed + V)
    faces = rig["faces"][:F]
    w = face_weights(F, V)
    w["verts"] = np.random.default_rng(V).normal(0, 1.0, (1, V, 3)).astype(np.float32)
    return rig, fp, faces, w, mesh_eval(rig, fp, faces, w, torch.float64), mesh_eval(rig, fp, faces, w, torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------------------
# bind_splats
# ------------------------------------------------------------------------------------------------------------------------------------------
BIND_F, BIND_HEAVY, BIND_EMPTY = 40, 7, (0, 3, 17, 26, 39)
BIND_LEAVES = ("_xyz", "_scaling", "_rotation", "_opacity", "face_R", "face_scale", "face_center", "face_quat")
BIND_OUTS = ("xyz", "scaling", "rotation", "opacity")
SATURATED = (90.0, -90.0, 100.0, -100.0)   # the last four opacity logits of a set with N >= 63: finiteness and saturation only
BIND_SEED = 2


@functools.lru_cache(maxsize=None)
def bind_faces():
    """The 40 faces under the splats: (verts, faces) and their frames by unfused.face_frames in float64, rounded to fp32 -- the kernels' inputs."""
    rig = small_rig(37, 3, 5, BIND_SEED)
    verts, faces = rig["v_template"], rig["faces"][:BIND_F]
    c, R, s, q = U.face_frames(torch.as_tensor(verts).double(), torch.as_tensor(faces))
    return verts, faces, {k: np.ascontiguousarray(v.numpy().astype(np.float32)) for k, v in (("face_center", c), ("face_R", R), ("face_scale", s), ("face_quat", q))}


@functools.lru_cache(maxsize=None)
def bind_case(N, scaled_quat):
    """Leaves, binding and loss weights of N splats on the 40 faces: faces BIND_EMPTY own nothing, face BIND_HEAVY about 35 % of the splats
    (> 300 of 1000); |_rotation| log-uniform in [0.2, 5]; _scaling in [-8, 2]; opacity logits in [-12, 12] (+ SATURATED); face_quat unit, or
    scaled per face by a factor in [0.5, 2] when `scaled_quat` (the only case in which the 1 / |face_quat| path matters)."""
    g = np.random.default_rng(100 + N)
    frames = dict(bind_faces()[2])
    allowed = np.array([f for f in range(BIND_F) if f not in BIND_EMPTY and f != BIND_HEAVY])
    binding = np.where(g.random(N) < 0.35, BIND_HEAVY, allowed[g.integers(0, len(allowed), N)]).astype(np.int64)
    rot = g.normal(size=(N, 4))
    rot *= (np.exp(g.uniform(math.log(0.2), math.log(5.0), N)) / np.linalg.norm(rot, axis=1))[:, None]
    opacity = g.uniform(-12.0, 12.0, (N, 1))
    if N >= 63:
        opacity[-4:, 0] = SATURATED
    if scaled_quat:
        frames["face_quat"] = frames["face_quat"] * g.uniform(0.5, 2.0, (BIND_F, 1)).astype(np.float32)
    leaves = dict(_xyz=g.normal(0, 0.35, (N, 3)), _scaling=g.uniform(-8.0, 2.0, (N, 3)), _rotation=rot, _opacity=opacity, **frames)
    leaves = {k: np.ascontiguousarray(v, np.float32) for k, v in leaves.items()}
    w = {k: g.normal(0, 1.0, s).astype(np.float32) for k, s in (("xyz", (N, 3)), ("scaling", (N, 3)), ("rotation", (N, 4)), ("opacity", (N, 1)))}
    return leaves, binding, w


def bind_eval(leaves, binding, w, dtype):
    """unfused.bind_xyz / bind_scaling / bind_rotation and sigmoid in `dtype` -> the four outputs and d_<leaf> of all eight leaves."""
    L = {k: torch.as_tensor(leaves[k]).to(dtype).requires_grad_(True) for k in BIND_LEAVES}
    b = torch.as_tensor(binding)
    outs = (U.bind_xyz(L["_xyz"], b, L["face_R"], L["face_scale"], L["face_center"]), U.bind_scaling(L["_scaling"], b, L["face_scale"]),
            U.bind_rotation(L["_rotation"], b, L["face_quat"]), torch.sigmoid(L["_opacity"]))
    loss = sum((o * torch.as_tensor(w[k]).to(dtype)).sum() for k, o in zip(BIND_OUTS, outs))
    g = _grads(loss, L)
    out = {k: _np64(o) for k, o in zip(BIND_OUTS, outs)}
    out.update({"d_" + k: _np64(g[k]) for k in BIND_LEAVES})
    return out


@functools.lru_cache(maxsize=None)
def bind_refs(N, scaled_quat):
    leaves, binding, w = bind_case(N, scaled_quat)
    return bind_eval(leaves, binding, w, torch.float64), bind_eval(leaves, binding, w, torch.float32)


# ------------------------------------------------------------------------------------------------------------------------------------------
# every face set the GPU tests run, for the conditioning checks of tests/test_binding_ref_cpu.py
# ------------------------------------------------------------------------------------------------------------------------------------------
def face_sets():
    """name -> (verts float64 (V,3), faces (F,3)): the vertices are the ones the face-frame kernels see (posed ones for the mesh node)."""
    out = {}
    for F in (1, 255, 256, 257):
        v, f = face_case(F)[:2]
        out[f"face_frames F={F}"] = (v.astype(np.float64), f)
    v, f = degenerate_case()[:2]
    out["degenerate set"] = (v.astype(np.float64), f)
    for (V, F) in MESH_CASES:
        c = mesh_case(V, F)
        out[f"mesh V={V} F={F}"] = (c[4]["verts"][0], c[2])
    v, f, _ = bind_faces()
    out["bind F=40"] = (v.astype(np.float64), f)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# the rasterizer's bound and leaves entries (tests/test_bound_entry_parity_gpu.py; conditions: tests/test_bound_entry_cases_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------------
RASTER_NS = (1, 63, 257, 1000)
RASTER_W, RASTER_H, RASTER_M = 96, 80, 16        # 6 x 5 tiles of 16 x 16; SH stored up to degree 3
RASTER_BG = (0.2, 0.1, 0.3)
# orbit_camera arguments of the two entries' cases: the camera sits inside the cloud, so splats and whole faces lie behind it (changed until the conditions of
# tests/test_bound_entry_cases_cpu.py held for every case, as FACE_SEED was; the checks themselves are not loosened)
RASTER_CAMERA = dict(bound=dict(r=0.25, fovy_deg=70.0, yaw_deg=20.0, pitch_deg=-10.0), leaves=dict(r=0.7, fovy_deg=100.0, yaw_deg=20.0, pitch_deg=-10.0))
# GaussianRasterizationSettings.scale_modifier: identity frames leave exp(_scaling) up to e^2 world units, every pixel saturated by the first few
RASTER_SCALE_MODIFIER = dict(bound=1.0, leaves=0.05)


def identity_frames(F=BIND_F):
    """Frames under which gab_bind_forward is the unbound model's activations, bit for bit (every fma of bind_math.h has an exact 0 or 1 operand)."""
    return dict(face_R=np.tile(np.eye(3, dtype=np.float32), (F, 1, 1)), face_scale=np.ones((F, 1), np.float32), face_center=np.zeros((F, 3), np.float32),
                face_quat=np.tile(np.array([1, 0, 0, 0], np.float32), (F, 1)))


def raster_camera(entry):
    from gaussianavatars_amd import synthetic as S

    return S.orbit_camera(RASTER_W, RASTER_H, **RASTER_CAMERA[entry])


@functools.lru_cache(maxsize=None)
def raster_case(N, scaled_quat, entry="bound"):
    """bind_case(N, scaled_quat) in front of a camera -> (leaves, binding, sh (N, 16, 3), grad_out_color (3, H, W), camera).
    leaves: identity frames, every splat on face 0."""
    leaves, binding, _ = bind_case(N, scaled_quat)
    leaves = dict(leaves)
    if entry == "leaves":
        leaves.update(identity_frames())
        binding = np.zeros_like(binding)
    g = np.random.default_rng(600 + N)
    sh = np.zeros((N, RASTER_M, 3), np.float32)
    sh[:, 0] = g.normal(0.5, 0.5, (N, 3))
    sh[:, 1:] = g.normal(0.0, 0.08, (N, RASTER_M - 1, 3))
    gpix = g.normal(0.0, 1.0, (3, RASTER_H, RASTER_W)).astype(np.float32)
    return leaves, binding, sh, gpix, raster_camera(entry)


def world_values(leaves, binding):
    """The four world-space tensors of a case: bind_eval in float64, rounded to fp32."""
    zero = {k: np.zeros((1, n), np.float32) for k, n in (("xyz", 3), ("scaling", 3), ("rotation", 4), ("opacity", 1))}
    r = bind_eval(leaves, binding, zero, torch.float64)
    return {k: np.ascontiguousarray(r[k], np.float32) for k in BIND_OUTS}


def raster_settings_args(cam, sh_degree, entry):
    return dict(H=cam.image_height, W=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=np.asarray(RASTER_BG, np.float32),
                scale_modifier=RASTER_SCALE_MODIFIER[entry], viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center)


def oracle_figures(oracle, N, scaled_quat, entry, sh_degree=3):
    """The oracle's forward and backward on the fp32-rounded float64 world values of a case -> (radii (N,), binding, which rows of
    G_w = (d xyz, d scaling, d rotation, d opacity) are not all zero)."""
    leaves, binding, sh, gpix, cam = raster_case(N, scaled_quat, entry)
    w = world_values(leaves, binding)
    s = oracle.make_settings(**raster_settings_args(cam, sh_degree, entry))
    st = oracle.forward(s, w["xyz"], sh, None, w["opacity"], w["scaling"], w["rotation"], None)
    g = oracle.backward(s, st, gpix)
    nz = np.zeros(N, bool)
    for k in ("means3D", "scales", "rotations", "opacities"):
        nz |= (g[k].reshape(N, -1) != 0).any(1)
    return st.radii, binding, nz
