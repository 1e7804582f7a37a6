"""What tests/test_eval_cpu.py and tests/test_eval_gpu.py share: the pins of tests/golden/eval_pins.npz, the bar of the figures that are new with
the evaluation path, the extra shapes chosen for the kernel's tiles, and the boundary sweep of the 8-bit transform.

The bar of a NEW figure (MSE, PSNR): the reference's own fp32 result sits some distance from the fp64 value; a figure under test may sit at most
4 x that distance from the fp64 value (a tiled fixed-order sum against torch's pairwise one), and never less than 2 fp32 units in the last place
of the value is demanded.  L1 and SSIM keep the bars of tests/test_loss_gpu.py: 2e-6 and 2e-5 absolute."""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = np.load(os.path.join(ROOT, "tests", "golden", "eval_pins.npz"))
CASES = {"chw": (3, 37, 45), "bchw": (2, 3, 16, 32), "small": (3, 5, 7), "pixel": (3, 1, 1)}
TRANSFORMS = ("raw", "clamp", "png8")
L1_BAR, SSIM_BAR = 2e-6, 2e-5
#: shapes beyond the fixture's, for the 32x16 tiles, their 5-pixel halo and the 16-byte loads: exactly one tile; four partial tiles
EXTRA = {"one_tile": (3, 16, 32), "four_tiles": (3, 17, 33)}


def new_bar(ref32, ref64):
    """|value - ref64| allowed for a new figure: 4 x the reference's own distance, at least 2 fp32 ulp of the value."""
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    with np.errstate(invalid="ignore"):
        dist = np.where(np.isfinite(ref64), np.abs(ref32 - ref64), 0.0)
        return np.maximum(4.0 * dist, 2.0 * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64))


def assert_new(value, ref32, ref64, what):
    value, ref64 = np.asarray(value, np.float64), np.asarray(ref64, np.float64)
    assert value.shape == ref64.shape, (what, value.shape, ref64.shape)
    inf = np.isinf(ref64)
    assert np.array_equal(value[inf], ref64[inf]), what   # an identical plane: +inf on both sides
    err, bar = np.abs(value[~inf] - ref64[~inf]), new_bar(ref32, ref64)[~inf]
    with np.errstate(invalid="ignore"):
        own = np.abs(np.asarray(ref32, np.float64) - ref64)[~inf]
    if err.size:   # (pytest -s shows them: the distances DESIGN.md section 17 quotes)
        print(what, "distance from fp64:", err.max(), "the reference's:", own.max(), "bar:", bar.min())
    assert np.all(err <= bar), (what, err.tolist(), bar.tolist())


@functools.lru_cache(maxsize=None)
def extra_pair(name):
    """A pair of an EXTRA shape, values in [-0.2, 1.3] like the fixture's."""
    g = np.random.default_rng(sum(map(ord, name)))
    a = g.uniform(-0.2, 1.3, EXTRA[name]).astype(np.float32)
    b = (0.7 * a + 0.3 * g.uniform(-0.2, 1.3, EXTRA[name])).astype(np.float32)
    b[..., ::4, ::3] = a[..., ::4, ::3]
    return a, b


@functools.lru_cache(maxsize=None)
def extra_reference(name, transform):
    """For an EXTRA pair what the fixture holds for its own: the composed-torch figures on the CPU in fp32 (tests/test_eval_cpu.py holds that path to
    the reference's pins) and the same expressions in fp64 from the same fp32 transformed inputs.  Computed once."""
    from gaussianavatars_amd import evaluate as E

    a, b = (E._planar(torch.from_numpy(x), transform).contiguous() for x in extra_pair(name))
    out = {}
    for tag, (x, y) in (("", (a, b)), ("_64", (a.double(), b.double()))):
        out["l1" + tag] = float(E._figures_composed(x, y, True)[0, 0])
        out["ssim" + tag] = float(E._figures_composed(x, y, True)[0, 2])
        sq = (x - y) ** 2
        out["mse3" + tag] = sq.reshape(3, -1).mean(1, keepdim=True).numpy()
        out["mse4" + tag] = sq.reshape(1, -1).mean(1, keepdim=True).numpy()
        out["psnr3" + tag] = (20 * torch.log10(1.0 / torch.sqrt(sq.reshape(3, -1).mean(1, keepdim=True)))).numpy()
        out["psnr4" + tag] = (20 * torch.log10(1.0 / torch.sqrt(sq.reshape(1, -1).mean(1, keepdim=True)))).numpy()
    return out


def reference(case, transform):
    """The figures of a fixture case or an EXTRA shape under one name each: l1, ssim, mse3, mse4, psnr3, psnr4 and their *_64 twins."""
    if case in EXTRA:
        return extra_reference(case, transform)
    k = f"{case}_{transform}_"
    return {n: PINS[k + n] for n in ("l1", "ssim", "mse3", "mse4", "psnr3", "psnr4", "l1_64", "ssim_64", "mse3_64", "mse4_64", "psnr3_64", "psnr4_64")}


def pair(case):
    return extra_pair(case) if case in EXTRA else (PINS[case + "_a"], PINS[case + "_b"])


def boundary_sweep():
    """The fp32 values at which render.py:41's byte changes: for every k in 0..255 the nine values within +-4 ulp of fp32((k + 0.5) / 255), then
    -0.0, negatives and values above 1: 2325 values."""
    v = []
    for k in range(256):
        x = np.float32((k + 0.5) / 255.0)
        lo = x
        for _ in range(4):
            lo = np.nextafter(lo, np.float32(-np.inf))
        for _ in range(9):
            v.append(lo)
            lo = np.nextafter(lo, np.float32(np.inf))
    v += [np.float32(x) for x in (-0.0, 0.0, -1e-30, -1e-3, -0.2, -1.0, -255.0, -3e38, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0019, 1.002,
                                  1.3, 2.0, 255.0, 256.0, 3e38, 1e-45, 1e-38, 0.5, 0.25)]
    v = np.asarray(v, np.float32)
    assert v.size == 2325
    return v


def torch_bytes(x):
    """render.py:41 in torch on the CPU, for a planar image or batch (numpy in, numpy out)."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    perm = (1, 2, 0) if t.dim() == 3 else (0, 2, 3, 1)
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(*perm).to("cpu", torch.uint8).contiguous().numpy()
