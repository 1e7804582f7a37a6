"""float64 numpy statement of the metric-space splat regularisers' contract (include/gms.h), written from its formulas:

    f_i = face_scaling[binding_i]
    u_ij = max(x_ij f_i - t_xyz, 0),            m_i = ||u_i||
    e_ij = exp(s_ij),  v_ij = max(e_ij f_i - t_s, 0),  b_i = ||v_i||
    c = number of visible splats,  xyz_mean = sum_vis m_i / c,  scale_mean = sum_vis b_i / c        (c == 0: NaN, NaN)
    d_xyz[i][j]   = g_xyz / c * u_ij / m_i * f_i               where visible[i] and u_ij > 0, else 0
    d_scale[i][j] = g_scale / c * v_ij / b_i * f_i * e_ij      where visible[i] and v_ij > 0, else 0
    d_face[k]     = sum over visible i bound to k of  g_xyz / c * sum_j u_ij / m_i * x_ij  +  g_scale / c * sum_j v_ij / b_i * e_ij

and the case generator of tests/test_metric_reg_cpu.py and tests/test_metric_reg_gpu.py.  A term whose g is None is off."""
import numpy as np


def metric_ref(xyz, log_scaling, face_scaling, binding, visible, t_xyz, t_s, g_xyz=1.0, g_scale=1.0):
    """-> dict(xyz_mean, scale_mean, count, d_xyz, d_scale, d_face, p, q): float64 throughout; p = x f and q = e f are the relu arguments
    before the thresholds.  Rows of invisible splats may hold anything: they are masked before any arithmetic."""
    vis = np.asarray(visible).astype(bool).reshape(-1)
    x = np.where(vis[:, None], np.asarray(xyz, np.float64).reshape(-1, 3), 0.0)
    s = np.where(vis[:, None], np.asarray(log_scaling, np.float64).reshape(-1, 3), 0.0)
    fs = np.asarray(face_scaling, np.float64).reshape(-1)
    b_idx = np.asarray(binding).astype(np.int64).reshape(-1)
    t_xyz, t_s = float(np.float32(t_xyz)), float(np.float32(t_s))   # the kernel receives the thresholds as fp32
    f = fs[b_idx][:, None]
    c = int(vis.sum())
    p = x * f
    u = np.maximum(p - t_xyz, 0.0)
    m = np.sqrt((u * u).sum(1))
    e = np.exp(s)
    q = e * f
    v = np.maximum(q - t_s, 0.0)
    b = np.sqrt((v * v).sum(1))
    d_xyz, d_scale, d_face = np.zeros_like(x), np.zeros_like(s), np.zeros_like(fs)
    if c > 0:
        gx = 0.0 if g_xyz is None else float(g_xyz) / c
        gs = 0.0 if g_scale is None else float(g_scale) / c
        rx = np.divide(u, m[:, None], out=np.zeros_like(u), where=(m > 0)[:, None]) * vis[:, None]
        rs = np.divide(v, b[:, None], out=np.zeros_like(v), where=(b > 0)[:, None]) * vis[:, None]
        d_xyz = gx * rx * f
        d_scale = gs * rs * f * e
        w = gx * (rx * x).sum(1) + gs * (rs * e).sum(1)
        np.add.at(d_face, b_idx[vis], w[vis])
        xyz_mean, scale_mean = m[vis].sum() / c, b[vis].sum() / c
    else:
        xyz_mean = scale_mean = float("nan")
    return dict(xyz_mean=xyz_mean, scale_mean=scale_mean, count=c, d_xyz=d_xyz, d_scale=d_scale, d_face=d_face, p=p, q=q)


def _f32_products(a, f):
    return (a.astype(np.float32) * f.astype(np.float32)[:, None]).astype(np.float32)


def metric_case(P, F, seed=0, index_dtype=np.int64, one_face=False, visible="some"):
    """One input set -> dict(xyz, ls, fs, binding, vis, t_xyz, t_s), fp32 / bool / `index_dtype`.

    face_scaling in [0.5, 1.5); xyz ~ N(0, 0.8), log-scales ~ N(log 0.4, 1); about 60 % of the splats visible (`visible`: "some", "all",
    "none").  F >= 3 leaves every third face without a splat; `one_face` binds everything to one face.  The thresholds sit at the medians of
    the fp32 products x f and e f, so about half the relus fire: t_xyz IS the fp32 product of one element, and (P >= 255) a few more rows are
    given that element's x and face, so their product ties the threshold exactly; t_s lies halfway between the two middle products, so
    that no e f is at it.  P >= 255: some visible rows have all three components under t_xyz (m_i = 0).  Invisible rows hold NaN in places."""
    rng = np.random.default_rng(1000 * seed + 7 * P + F)
    fs = rng.uniform(0.5, 1.5, F).astype(np.float32)
    used = np.array([k for k in range(F) if F < 3 or k % 3 != 1])
    binding = np.full(P, used[len(used) // 2]) if one_face else used[rng.integers(0, len(used), P)]
    xyz = rng.normal(0.0, 0.8, (P, 3)).astype(np.float32)
    ls = rng.normal(np.log(0.4), 1.0, (P, 3)).astype(np.float32)
    vis = {"some": rng.random(P) < 0.6, "all": np.ones(P, bool), "none": np.zeros(P, bool)}[visible]
    if P <= 3 and visible == "some":
        vis[:] = True
    # t_xyz: the fp32 product of the middle element
    px = _f32_products(xyz, fs[binding])
    flat = np.argsort(px, axis=None)[px.size // 2]
    i_star, j_star = np.unravel_index(flat, px.shape)
    t_xyz = np.float32(px[i_star, j_star])
    if P >= 255:
        rows = rng.choice(np.setdiff1d(np.arange(P), [i_star]), 12, replace=False)
        ties, under = rows[:6], rows[6:]
        binding[ties] = binding[i_star]
        xyz[ties, np.arange(6) % 3] = xyz[i_star, j_star]        # the same fp32 factors: the same fp32 product, exactly the threshold
        xyz[under] = -np.abs(xyz[under]) - abs(float(t_xyz)) - 1.0  # x f < t on all three axes
        vis[rows] = visible != "none"
    # t_s: halfway between the two middle products
    ps = np.sort(_f32_products(np.exp(ls.astype(np.float64)).astype(np.float32), fs[binding]), axis=None)
    k = (ps.size - 1) // 2
    t_s = np.float32(0.5 * (float(ps[k]) + float(ps[k + 1])))
    hidden = np.nonzero(~vis)[0]
    if hidden.size:
        xyz[hidden[::2], 0] = np.nan
        ls[hidden[::3], 2] = np.nan
    return dict(xyz=xyz, ls=ls, fs=fs, binding=binding.astype(index_dtype), vis=vis, t_xyz=float(t_xyz), t_s=float(t_s))


def scale_band(case, ref, ulps=2):
    """(P,3) bool: visible entries whose fp64 |e f - t_s| is within `ulps` ulp of the fp32 t_s -- where two fp32 exponentials that differ in the
    last place may put e f on different sides of the threshold."""
    t = np.float32(case["t_s"])
    return (np.abs(ref["q"] - float(t)) <= ulps * float(np.spacing(t))) & case["vis"][:, None]


#: (P, F, options): every shape of tests/test_metric_reg_gpu.py.  P: one splat, under one wave-quad, exactly one slab, one slab and a splat,
#: three slabs with a partial one; F: one face, a few, more than FACE_LANES.
CASES = ([(P, F, dict(index_dtype=(np.int32, np.int64)[(n + k) % 2])) for n, P in enumerate((1, 255, 1024, 1025, 3000)) for k, F in enumerate((1, 7, 40))]
         + [(3000, 40, dict(one_face=True, index_dtype=np.int32)), (1025, 7, dict(index_dtype=np.int64)),   # (the table has 1025 / 7 as int32)
            (1025, 7, dict(visible="none")), (1025, 7, dict(visible="all"))])


def case_id(c):
    P, F, opt = c
    return f"P{P}-F{F}-" + "-".join(f"{k}={getattr(v, '__name__', v)}" for k, v in sorted(opt.items()))
