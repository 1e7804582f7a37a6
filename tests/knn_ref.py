"""The contract of include/gdc.h's gdc_knn3_dist2 in float64 numpy, and the clouds the nearest-neighbour tests run on.

brute_force(points) takes fp32 positions and returns, in fp64, the mean of the 3 smallest squared distances to the OTHER rows (the row itself
is masked by index, so a duplicate is a neighbour at 0); with N - 1 < 3 neighbours the mean over those there are, 0 for N == 1.

The bar (derived, not measured), u = 2^-24: one rounded subtraction per axis, three squarings, two additions, then two more additions and a
division give at most about 8 u of relative error on the value; the k-th smallest of perturbed values is within the perturbation of the k-th
smallest of the true ones, so a different neighbour at a near-tie costs nothing more.  RTOL = 16 u, ATOL = 0: exact zeros and lattice values
must compare equal.
"""
import numpy as np

RTOL = 16 * 2.0 ** -24
ATOL = 0.0


def brute_force(points, chunk=512):
    p = np.ascontiguousarray(points, np.float32).astype(np.float64)
    n = p.shape[0]
    out = np.zeros(n, np.float64)
    k = min(3, n - 1)
    if k <= 0:
        return out
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        d2 = ((p[s:e, None, :] - p[None, :, :]) ** 2).sum(-1)
        d2[np.arange(e - s), np.arange(s, e)] = np.inf
        out[s:e] = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1).sum(1) / k
    return out


def cases(C, tile=256):
    """{name: (N, 3) fp32 cloud}; C = the search's chunk size (_lib.GDC_KNN_CHUNK), tile = its boxes per LDS tile."""
    rng = np.random.default_rng(20)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    out = {}
    for n in (1, 2, 3, 4, 5):                                   # 1: the few-point rule, the seed window at both ends of the sequence
        out[f"few_{n}"] = f32(rng.normal(0, 1, (n, 3)))
    for n in (C - 1, C, C + 1, 4 * C + 1):                      # 2: chunk edges, a ragged last chunk
        out[f"cube_{n}"] = f32(rng.random((n, 3)))
    out[f"cube_{tile * C + C + 1}"] = f32(rng.random((tile * C + C + 1, 3)))   # more boxes than one tile holds, a ragged second tile
    out["far_50"] = f32(rng.normal(0, 1, (600, 3))) * np.float32(1e-3) + np.float32(50)   # 3: where |a|^2 + |b|^2 - 2 a.b returns zeros
    out["far_4"] = f32(rng.normal(0, 1, (600, 3))) * np.float32(1e-2) + np.float32(4)
    base = f32(rng.normal(0, 1, (300, 3)))
    out["dup_4"] = np.repeat(base, 4, axis=0)[rng.permutation(1200)]             # 4: every value exactly 0
    out["dup_2"] = np.repeat(base, 2, axis=0)[rng.permutation(600)]              #    (0 + d + d) / 3
    g = np.arange(10, dtype=np.float32)
    out["lattice"] = f32(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))   # 5: ties everywhere, every value exactly 1
    plane = f32(rng.random((1000, 3)))
    plane[:, 2] = 0.25
    out["plane"] = plane                                         # 6: a zero-span axis in the quantiser, degenerate boxes
    t = f32(rng.random((1000, 1)))
    out["line"] = f32(np.float32([0.3, -1.0, 2.0]) + t * np.float32([1.0, 2.0, -0.5]))
    blobs = np.concatenate([f32(rng.normal(0, 1, (1000, 3))), f32(rng.normal(0, 1, (1000, 3))) + np.float32([100, 0, 0]),
                            np.float32([[50, 1000, 0]])])
    out["blobs"] = f32(blobs)                                    # 7: each blob prunes the other; the lone query prunes nothing
    return out


SHUFFLE_OF = "cube_{n}"   # 8: case 2's largest cloud (n = 4 C + 1) with its rows shuffled


def shuffled(cloud):
    perm = np.random.default_rng(21).permutation(cloud.shape[0])
    return np.ascontiguousarray(cloud[perm]), perm


def check(got, want, what):
    got = np.asarray(got, np.float64)
    err = np.abs(got - want) / np.maximum(want, np.finfo(np.float64).tiny)
    print(f"{what}: n = {want.shape[0]}, max rel. error {float(np.where(want > 0, err, 0).max()) if want.size else 0.0:.3e} (bar {RTOL:.3e})")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
U = 2.0 ** -24
# `_scaling` = log sqrt dist2 = log(dist2) / 2: RTOL on dist2 is RTOL / 2 absolute on the leaf; the square root (correctly rounded) adds u / 2
# and the logarithm 2 ulp of the leaf's magnitude at most, on either side (the fixture's fp32 roundings and ours): 10 u absolute, 8 u relative
SCALING_ATOL, SCALING_RTOL = RTOL / 2 + 2 * U, 8 * U



def check_leaves(m, p, device="cpu"):
    """The leaves create_from_pcd left in `m` against a case of tests/golden/pcd_init_pins.npz: `_scaling` of an unbound model at the bar above, everything else exact."""
    import torch

    for k in LEAVES:
        t = getattr(m, k)
        assert isinstance(t, torch.nn.Parameter) and t.requires_grad and t.dtype is torch.float32 and t.is_contiguous() and t.device.type == device
        got, want = t.detach().cpu().numpy(), p["out" + k]
        assert got.shape == want.shape, k
        if k == "_scaling" and m.binding is None:
            print(f"_scaling: max abs. error {np.abs(got - want).max():.3e} (bar {SCALING_ATOL:.3e} + {SCALING_RTOL:.3e} |v|)")
            np.testing.assert_allclose(got, want, rtol=SCALING_RTOL, atol=SCALING_ATOL)
        else:
            assert np.array_equal(got, want), k
    assert np.array_equal(m.max_radii2D.cpu().numpy(), p["out_max_radii2D"]) and m.spatial_lr_scale == float(p["spatial_lr_scale"])
