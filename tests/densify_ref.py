"""The contract of include/gdc.h in float64 numpy: the end state of the reference's densify_and_prune (clone -> split -> prune) as one
pass over the splats.  TEST INFRASTRUCTURE: what the fixtures of tests/golden/densify_pins.npz (the reference's own run) and the kernels of
csrc/gdc_kernels.hip are both held to.  Inputs are taken as they are (fp32 leaves) and raised to float64 before any arithmetic."""
import numpy as np

LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def rotation_matrices(q):
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def quantities(leaves, accum, denom, binding=None, face_scaling=None):
    """(g, world scaling (P,3), S, o, face scale per splat (P,1)) in float64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.asarray(accum, np.float64).reshape(-1) / np.asarray(denom, np.float64).reshape(-1)
    g = np.where(np.isnan(g), 0.0, g)
    P = g.shape[0]
    fs = np.ones((P, 1)) if binding is None else np.asarray(face_scaling, np.float64).reshape(-1)[np.asarray(binding, np.int64)][:, None]
    w = np.exp(np.asarray(leaves["_scaling"], np.float64)) * fs
    o = 1.0 / (1.0 + np.exp(-np.asarray(leaves["_opacity"], np.float64).reshape(-1)))
    return g, w, w.max(1) if P else np.zeros(0), o, fs


def densify_ref(leaves, accum, denom, noise, max_grad, min_opacity, extent, percent_dense, max_screen_size=0, binding=None, face_scaling=None,
                binding_counter=None, moments=None):
    """Returns a dict: src, child (bool per row), the six leaves (rows copied from the input keep its values exactly; the children's _xyz and
    _scaling are float64), binding / binding_counter (None when unbound), `moments` gathered the same way (zero for new rows) and the
    intermediate masks (clone, split, cand_row, cand_child, margin: the smallest relative distance of g, S, o to a threshold)."""
    P = np.asarray(leaves["_xyz"]).shape[0]
    g, w, S, o, fs = quantities(leaves, accum, denom, binding, face_scaling)
    dense, big = percent_dense * extent, 0.1 * extent
    clone = (np.abs(g) >= max_grad) & (S <= dense)
    split = (g >= max_grad) & (S > dense)
    c_scaling = np.log(w / fs / 1.6)
    S_child = (np.exp(c_scaling) * fs).max(1) if P else np.zeros(0)
    low = o < min_opacity
    cand_row = low | ((S > big) if max_screen_size else False)
    cand_child = low | ((S_child > big) if max_screen_size else False)
    idx = np.arange(P)
    if binding is not None:
        b = np.asarray(binding, np.int64)
        F = np.asarray(binding_counter).shape[0]
        cnt = np.asarray(binding_counter, np.int64) + np.bincount(b[clone | split], minlength=F)
        n_cand = np.where(split, 2 * cand_child, cand_row * (1 + clone))
        cand = np.bincount(b, weights=n_cand, minlength=F).astype(np.int64)
        remove_f = cnt - cand > 0
        remove = remove_f[b]
        counter = (cnt - np.where(remove_f, cand, 0)).astype(np.int32)
    else:
        remove = np.ones(P, bool)
        counter = None
    keep_row = ~(cand_row & remove)
    keep_child = ~(cand_child & remove)
    seg = [idx[~split & keep_row], idx[clone & keep_row], idx[split & keep_child], idx[split & keep_child]]
    source = np.concatenate(seg).astype(np.int64)
    n0, n1, n2 = len(seg[0]), len(seg[1]), len(seg[2])
    N = source.shape[0]
    src = np.where(np.arange(N) < n0, source, -1 - source).astype(np.int32)
    child = np.arange(N) >= n0 + n1
    out = {"src": src, "child": child, "clone": clone, "split": split, "cand_row": cand_row, "cand_child": cand_child}
    for k in LEAVES:
        out[k] = np.asarray(leaves[k])[source]
    if n2:
        c = (np.arange(N)[child] >= n0 + n1 + n2).astype(np.int64)
        s = source[child]
        smp = np.asarray(noise, np.float64)[c, s] * w[s]
        R = rotation_matrices(np.asarray(leaves["_rotation"], np.float64)[s])
        xyz = out["_xyz"].astype(np.float64)
        xyz[child] = np.einsum("nij,nj->ni", R, smp) + np.asarray(leaves["_xyz"], np.float64)[s]
        sc = out["_scaling"].astype(np.float64)
        sc[child] = c_scaling[s]
        out["_xyz"], out["_scaling"] = xyz, sc
    out["binding"] = None if binding is None else np.asarray(binding)[source]
    out["binding_counter"] = counter
    if moments is not None:
        out["moments"] = {k: np.where((src >= 0).reshape((-1,) + (1,) * (np.asarray(v).ndim - 1)), np.asarray(v)[source], 0).astype(np.asarray(v).dtype)
                          for k, v in moments.items()}

    def rel(a, t):
        a = a[np.isfinite(a)]
        return np.inf if a.size == 0 or t == 0 else float(np.min(np.abs(a - t)) / abs(t))

    m = [rel(np.abs(g[g != 0]), max_grad), rel(S, dense), rel(o, min_opacity)]
    if max_screen_size:
        m += [rel(S, big), rel(S_child[split], big)]
    out["margin"] = min(m)
    return out
