"""k_render_bwd_rp's lane mapping (two records per lane, the two half-waves on columns 0..3 and 4..7 of a row) on the
smallest scenes at which it can go wrong, every leaf gradient and means2D.grad against oracle.backward with the bar of
tests/test_fast_blend_gpu.py::test_fast_backward_vs_oracle (REL_GRAD of each tensor's largest magnitude).

The scenes are built here: small splats (footprints of three pixels' radius) placed by pixel and by depth, so that a quadrant's stream has a chosen
length and a pixel a chosen set of contributors.  Stream entry e of a chunk [lo, hi) is record hi - 1 - e: an "even" record (the .x half of
a lane's pairs) when hi - 1 - e is even, so odd stream lengths leave a lane one valid and one invalid record, and lengths around 60 and 120
put the stream's end on either side of a segment's.  Every scene is first checked on the CPU, with the oracle's state alone, to have no
(pixel, splat) alpha within 1e-4 (relative) of 1/255 -- the fp32 evaluations of alpha, hardware 2^x included, differ from the oracle's by
a few 1e-6, so that is a factor of ten and more -- and no pixel whose transmittance comes near 1e-4: the two evaluations then take the
same records everywhere and the bar needs no exemption list."""
import numpy as np
import pytest
import torch

from gaussianavatars_amd import synthetic as S
from tests.scenes import settings_args
from tests.test_fast_blend_gpu import REL_GRAD
from tests.test_gsr_gpu import _dev, _np

pytestmark = [pytest.mark.gpu, pytest.mark.fast_blend]

SEG = 60          # GSR_BWD_SEGMENT (include/gsr.h)
SIGMA_PX = 0.3    # world-space sigma in pixels (the 0.3 low-pass is added to its square): a footprint of 3 pixels' radius


def _place(cam, px, py, z):
    """World x, y of the points that project to pixel centres (px, py) (continuous pixel coordinates, the rasterizer's
    pix = ((ndc + 1) * size - 1) / 2: integer values are pixel centres) at world depth coordinate z."""
    M = np.asarray(cam.full_proj_transform, np.float64)
    W, H = cam.image_width, cam.image_height
    px, py, z = (np.asarray(v, np.float64) for v in (px, py, z))
    nx, ny = (2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0
    # (x, y, z, 1) @ M = (cx, cy, ., w); cx = nx w and cy = ny w are two linear equations in x, y
    a11, a12 = M[0, 0] - nx * M[0, 3], M[1, 0] - nx * M[1, 3]
    a21, a22 = M[0, 1] - ny * M[0, 3], M[1, 1] - ny * M[1, 3]
    b1 = -(z * (M[2, 0] - nx * M[2, 3]) + (M[3, 0] - nx * M[3, 3]))
    b2 = -(z * (M[2, 1] - ny * M[2, 3]) + (M[3, 1] - ny * M[3, 3]))
    det = a11 * a22 - a12 * a21
    return (b1 * a22 - a12 * b2) / det, (a11 * b2 - b1 * a21) / det


def _splats(cam, px, py, opac, seed, sigma_px=SIGMA_PX):
    """Splat i at pixel (px[i], py[i]); entry i of its quadrant's stream (front to back: depth grows with i)."""
    n = len(px)
    g = np.random.default_rng(seed)
    z = -1e-3 * np.arange(n)                                   # the camera sits at z = +1 and looks down -z
    x, y = _place(cam, px, py, z)
    focal = cam.image_height / (2.0 * np.tan(cam.FoVy * 0.5))
    sc = sigma_px * (1.0 - z) / focal
    sc = sc[:, None] * g.uniform(0.8, 1.2, (n, 3))             # (anisotropic, turned at random: an isotropic splat's rotation gradient is exactly 0)
    rot = g.normal(0.0, 1.0, (n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)   # (unit: the kernel takes the quaternion as it comes)
    shs = g.uniform(-0.5, 1.5, (n, 1, 3)).astype(np.float32)
    return dict(means3D=np.stack([x, y, z], 1).astype(np.float32), scales=sc.astype(np.float32), rotations=rot,
                opacities=np.asarray(opac, np.float32).reshape(n, 1), shs=shs)


def _stream(n, seed, x0=3.0, x1=4.5, y0=3.0, y1=4.5, opac=(0.15, 0.6)):
    """n splats inside the quadrant at pixels [0, 8)^2 (centres in [x0, x1] x [y0, y1]; the footprint's radius is 3 pixels, so with the defaults no other quadrant is touched)."""
    g = np.random.default_rng(seed)
    return g.uniform(x0, x1, n), g.uniform(y0, y1, n), g.uniform(opac[0], opac[1], n)


def _scene(name):
    """-> (camera, splats, {(tile, quadrant): stream length} of every stream | the length of tile 0's quadrant 0 | None)"""
    if name.startswith("n"):            # a stream of exactly n entries over quadrant 0 of the only tile that has any
        n = int(name[1:])
        cam = S.orbit_camera(24, 24)
        px, py, op = _stream(n, 100 + n, opac=(0.15, 0.6) if n <= 2 else (0.02, 0.12))
        return cam, _splats(cam, px, py, op, n), {(0, 0): n}
    if name.startswith("ragged"):       # 27 x 29 / 30 x 27: the image ends inside the last tile's right-hand and lower quadrants -- after column 2 of the
        W, H = (27, 29) if name == "ragged27" else (30, 27)   # quadrant (inside the low half-wave's columns) / after column 5 (inside the high one's)
        cam = S.orbit_camera(W, H)
        g = np.random.default_rng(7)
        n = 90
        px, py = g.uniform(17.0, W - 1.0, n), g.uniform(17.0, H - 1.0, n)
        return cam, _splats(cam, px, py, g.uniform(0.03, 0.2, n), 8), None
    if name == "deep":                  # ~700 faint splats over one quadrant: all ten segments, the open-ended last one carrying across several chunks
        cam = S.orbit_camera(24, 24)
        n = 700
        px, py, _ = _stream(n, 31)
        op = np.random.default_rng(32).uniform(0.008, 0.012, n)
        return cam, _splats(cam, px, py, op, 61), {(0, 0): n}   # (seed: one whose alphas keep the margin below)
    if name in ("left", "right"):       # contributions in columns 0..3 / 4..7 of the quadrant only: one half-wave has nothing to add
        cam = S.orbit_camera(24, 24)
        n = 75
        x = 1.25 if name == "left" else 5.75
        px, py, op = _stream(n, 41, x, x + 0.5, 1.5, 6.0, opac=(0.03, 0.2))
        return cam, _splats(cam, px, py, op, 42), n     # (the right-hand footprints reach into the next quadrant's rectangle)
    if name == "four_tiles":            # 40 x 40 = 3 x 3 tiles, four of them with work; the last two entries of a stream on different pixels
        cam = S.orbit_camera(40, 40)
        g = np.random.default_rng(51)
        px, py, op = [], [], []
        for tx, ty, n in ((0, 0, 61), (1, 0, 64), (0, 1, 33), (1, 1, 122)):
            px.append(16 * tx + 8 + g.uniform(3.0, 4.5, n)); py.append(16 * ty + 8 + g.uniform(3.0, 4.5, n)); op.append(g.uniform(0.02, 0.12, n))
        px, py, op = (np.concatenate(v) for v in (px, py, op))
        order = g.permutation(len(px))  # depth order across the tiles
        return cam, _splats(cam, px[order], py[order], op[order], 52), {(0, 3): 61, (1, 3): 64, (3, 3): 33, (4, 3): 122}
    raise KeyError(name)


def _check_margins(st, H, W):
    """No alpha within 1e-4 (relative) of 1/255 at any pixel, no transmittance near 1e-4: from the oracle's state, in fp64."""
    co, xy = st.conic_opacity.astype(np.float64), st.xy.astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    worst = np.inf
    for i in np.nonzero(st.radii > 0)[0]:
        dx, dy = xy[i, 0] - xx, xy[i, 1] - yy
        power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
        alpha = co[i, 3] * np.exp(power)
        worst = min(worst, np.abs(alpha * 255.0 - 1.0).min())
        assert alpha.max() < 0.98, "no record at the 0.99 clamp"
    assert worst > 1e-4, f"an alpha sits within {worst:.1e} of 1/255"
    assert st.final_T.min() > 3e-4, f"a pixel's transmittance reaches {st.final_T.min():.1e}: near the 1e-4 cut"


NAMES = ["n1", "n2", "n59", "n60", "n61", "n119", "n120", "n121", "ragged27", "ragged30", "deep", "left", "right", "four_tiles"]


@pytest.mark.parametrize("name", NAMES)
def test_pairs_backward_vs_oracle(oracle, name):
    from gaussianavatars_amd.debug import forward_state
    from gaussianavatars_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, set_fast_blend

    assert set_fast_blend(True) == 1, "the product default is the fast blend"
    dev = _dev()
    cam, sp, want_q = _scene(name)
    a = settings_args(cam, [0.3, 0.6, 0.1], 0, 1.0)
    H, W = a["H"], a["W"]
    s = oracle.make_settings(**a)
    st = oracle.forward(s, sp["means3D"], sp["shs"], None, sp["opacities"], sp["scales"], sp["rotations"], None)
    _check_margins(st, H, W)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rs = GaussianRasterizationSettings(H, W, a["tanfovx"], a["tanfovy"], t(a["bg"]), 1.0, t(a["viewmatrix"]), t(a["projmatrix"]), 0,
                                       t(a["campos"]), False, False)
    hs = forward_state(rs, t(sp["means3D"]), t(sp["shs"]), None, t(sp["opacities"]), t(sp["scales"]), t(sp["rotations"]), None, fast_blend=True)
    qc, last = _np(hs["qcount"]).astype(np.int64), _np(hs["n_contrib_q"]).astype(np.int64)
    print(f"{name}: quadrant streams {[(int(i), int(j), int(qc[i, j])) for i, j in zip(*np.nonzero(qc))]}")
    # ---- the scene is what its name says (a culling change must not hollow the case out)
    if isinstance(want_q, int):
        assert int(qc[0, 0]) == want_q
    elif want_q is not None:
        assert {(int(i), int(j)): int(qc[i, j]) for i, j in zip(*np.nonzero(qc))} == want_q
    if name.startswith("ragged"):
        assert W % 8 and H % 8 and (qc[3] > 0).all(), "all four quadrants of the cut tile have a stream"
        assert (last[:, 24:] > 0).any() and (last[24:, :] > 0).any(), "contributors in the cut quadrants"
    if name == "deep":
        assert last.max() > SEG * 9 + 2 * SEG, "the open-ended tenth segment carries across at least two chunks"
    if name == "left":
        assert (last[:8, :4] > 0).any() and not (last[:8, 4:8] > 0).any()
    if name == "right":
        assert (last[:8, 4:8] > 0).any() and not (last[:8, :4] > 0).any()
    if name in ("n59", "n60", "n61", "n119", "n120", "n121", "four_tiles"):
        # a pixel's last contributor is entry last - 1 = record hi - last of its chunk: both parities occur, so one pixel's walk ends on the
        # even record of a lane and another's on the odd one
        l = last[last > 0]
        hi = ((l - 1) // SEG + 1) * SEG
        assert set(np.unique((hi - l) % 2)) == {0, 1}

    gpix = np.random.default_rng(5).normal(0, 1, (3, H, W)).astype(np.float32)
    ref = oracle.backward(s, st, gpix)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(True)
    m3, sh, op, sc, ro = tt(sp["means3D"]), tt(sp["shs"]), tt(sp["opacities"]), tt(sp["scales"]), tt(sp["rotations"])
    m2 = torch.zeros_like(m3, requires_grad=True)
    color, radii = GaussianRasterizer(rs)(means3D=m3, means2D=m2, shs=sh, opacities=op, scales=sc, rotations=ro)
    (color * torch.from_numpy(gpix).to(dev)).sum().backward()
    np.testing.assert_array_equal(_np(radii), st.radii)
    for k, g in dict(means3D=m3.grad, means2D=m2.grad, shs=sh.grad, opacities=op.grad, scales=sc.grad, rotations=ro.grad).items():
        r = ref[k]
        scale = np.abs(r).max() + 1e-20
        err = np.abs(_np(g).reshape(r.shape) - r).max() / scale
        print(f"{name}/{k}: rel err {err:.3e} (max |ref| {scale:.3e})")
        assert err < REL_GRAD, f"{name}/{k}: rel err {err:.3e} (max |ref| {scale:.3e})"
