"""float64 numpy statement of the splat regularisers' contract (include/grl.h), written from its formulas:

    n_i = ||xyz_i||,              a_i = max(n_i - t_xyz, 0)
    e_ij = exp(s_ij),             v_ij = max(e_ij - t_s, 0),        b_i = ||v_i||
    c = number of visible splats, xyz_mean = sum_vis a_i / c,       scale_mean = sum_vis b_i / c     (c == 0: NaN, NaN)
    d_xyz[i]   = g_xyz / c * xyz_i / n_i                 where visible[i] and n_i > t_xyz,  else 0
    d_scale[i][j] = g_scale / c * v_ij / b_i * e_ij      where visible[i] and v_ij > 0,     else 0

Shared by tests/test_reg_cpu.py and tests/test_reg_gpu.py; also the input generators both use."""
import numpy as np


def reg_ref(xyz, log_scaling, visible, t_xyz, t_s, g_xyz=1.0, g_scale=1.0):
    """-> dict(xyz_mean, scale_mean, count, d_xyz, d_scale, n, e): float64 throughout."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    s = np.asarray(log_scaling, np.float64).reshape(-1, 3)
    vis = np.asarray(visible).astype(bool).reshape(-1)
    t_xyz, t_s = float(np.float32(t_xyz)), float(np.float32(t_s))   # the kernel receives the thresholds as fp32
    c = int(vis.sum())
    n = np.sqrt((x * x).sum(1))
    a = np.maximum(n - t_xyz, 0.0)
    with np.errstate(over="ignore"):
        e = np.exp(s)
    v = np.maximum(e - t_s, 0.0)
    b = np.sqrt((v * v).sum(1))
    d_xyz, d_scale = np.zeros_like(x), np.zeros_like(s)
    if c > 0:
        on = vis & (n > t_xyz)
        d_xyz[on] = float(g_xyz) / c * x[on] / n[on, None]
        on = vis[:, None] & (v > 0)
        rows = np.nonzero(on.any(1))[0]
        full = np.zeros_like(s)
        full[rows] = float(g_scale) / c * v[rows] / b[rows, None] * e[rows]
        d_scale[on] = full[on]
        xyz_mean, scale_mean = a[vis].sum() / c, b[vis].sum() / c
    else:
        xyz_mean = scale_mean = float("nan")
    return dict(xyz_mean=xyz_mean, scale_mean=scale_mean, count=c, d_xyz=d_xyz, d_scale=d_scale, n=n, e=e)


def generic_inputs(P, seed=0):
    """The timing tool's distributions: xyz ~ N(0, 0.8) per axis, log-scales ~ N(log 0.4, 0.5), about half the splats visible (fp32, bool)."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0.0, 0.8, (P, 3)).astype(np.float32)
    ls = rng.normal(np.log(0.4), 0.5, (P, 3)).astype(np.float32)
    vis = rng.random(P) < 0.5
    return xyz, ls, vis


def gapped_inputs(P, t_xyz, t_s, seed=0):
    """The well-conditioned set: every ||xyz_i|| is <= 0.5 t_xyz or >= 1.5 t_xyz, every exp(s_ij) is <= 0.5 t_s or >= 1.5 t_s (about half of each
    above), about half the splats visible.  The margins are drawn strictly inside the two ranges so that fp32 rounding cannot cross them."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    r = np.where(rng.random(P) < 0.5, rng.uniform(0.05, 0.49, P), rng.uniform(1.51, 3.0, P)) * t_xyz
    xyz = (d * r[:, None]).astype(np.float32)
    e = np.where(rng.random((P, 3)) < 0.5, rng.uniform(0.05, 0.49, (P, 3)), rng.uniform(1.51, 4.0, (P, 3))) * t_s
    ls = np.log(e).astype(np.float32)
    vis = rng.random(P) < 0.5
    if P <= 3:
        vis[:] = True   # (a one-splat case with nothing visible is the hand case's business)
    return xyz, ls, vis


def band_rows(ref, t_xyz, t_s, rel=1e-3):
    """Rows within `rel` of a threshold, in fp64: | ||xyz|| - t_xyz | <= rel t_xyz, or any | e_j - t_s | <= rel t_s."""
    t_xyz, t_s = float(np.float32(t_xyz)), float(np.float32(t_s))
    return (np.abs(ref["n"] - t_xyz) <= rel * t_xyz) | (np.abs(ref["e"] - t_s) <= rel * t_s).any(1)
