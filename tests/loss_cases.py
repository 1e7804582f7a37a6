"""What tests/test_loss_cases_cpu.py and tests/test_loss_parity_gpu.py share: the shapes and value sets chosen for the 32 x 16 tiles of the fused
L1 + SSIM kernels and their 5-pixel halo, the sizes of the plain L1 kernel, the inputs the one-launch L1 was never shown, and the references.

References.  `fp64`: the reference's own expressions (utils/loss_utils.py:17-18 and :36-63) composed in torch on the CPU in float64, from the fp32
inputs and the fp32 2-D window values (oracle.loss_oracle.window_2d); gradients from autograd.  `ref32`: the same expressions in float32.

Bars.  A figure under test may sit at most 4 x ref32's own distance from fp64 (tests/eval_cases.py: new_bar).  For a tensor the largest absolute
error over the tensor is held to 4 x ref32's largest absolute error, and never less than 2 fp32 units in the last place of the tensor's largest
fp64 magnitude is demanded.  The existing absolute bars (2e-6 for L1, 2e-5 for the SSIM value) hold beside them.

`kernel_model` is a float32 numpy model of the summation order of k_l1_ssim_fwd / k_l1_ssim_bwd (eleven taps added in the order k = 0 .. 10,
horizontal then vertical).  It is a reference: twice its distance from fp64 is the bar of a figure listed in MODEL_BARS (DESIGN.md section 19
states why a figure is listed).  The kernel's own output never sets a bar."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_oracle as LO

L1_BAR, SSIM_BAR = 2e-6, 2e-5
TX, TY, RAD = 32, 16, 5

#: (B,C,H,W): one pixel; one row; under the window; the window; exactly one tile; one short of a tile; one past (four partial tiles);
#: two tiles and a pixel each way; a batch with C != 3; a batch of single planes one short of two tiles
SSIM_SHAPES = ((1, 1, 1, 1), (1, 3, 1, 40), (1, 2, 5, 7), (1, 3, 11, 11), (1, 3, 16, 32), (1, 1, 15, 31), (1, 3, 17, 33), (1, 3, 33, 65),
               (2, 4, 17, 33), (3, 1, 31, 63))
VALUE_SETS = ("uniform", "wide", "const", "same", "zero")
#: the loss a gradient is taken of, from the per-image figures (l1_i, ssim_i) and the averaged ones (l1, ssim)
CONFIGS_ANY = ("l1", "ssim", "mix")
CONFIGS_BATCH = ("weights", "mean", "weights_both", "mixed_strides")
#: (figure, value set) held to twice the model's distance where that is above 4 x ref32's (see the module docstring and DESIGN.md section 19).
#: The SSIM value of a constant plane: sigma12 = E[xy] - mu1 * mu2 is zero there and what float32 leaves of it is measured against C2 = 9e-4;
#: at 1x1x15x31 ref32 happens to land 6e-9 from fp64, the model 1.5e-7 and the kernel 1.6e-7.
MODEL_BARS = frozenset({("ssim_value", "const")})


def shape_id(shape):
    return "x".join(map(str, shape))


def weights(B):
    """Per-image upstream gradients that differ: 0.3, -1.7, 0.9, ..."""
    return np.asarray([0.3, -1.7, 0.9, 2.1, -0.4][:B], np.float32)


def weights2(B):
    return np.asarray([-1.1, 0.6, 0.25, -2.0, 1.4][:B], np.float32)


@functools.lru_cache(maxsize=None)
def pair(shape, kind):
    """A float32 pair of one shape and value set; built once, never written again."""
    g = np.random.default_rng(sum(shape) * 131 + VALUE_SETS.index(kind))
    tex = g.uniform(0.0, 1.0, shape).astype(np.float32)
    if kind == "uniform":
        a, b = tex, np.clip(tex + g.normal(0.0, 0.1, shape), 0.0, 1.0).astype(np.float32)
    elif kind == "wide":   # as eval_cases.extra_pair
        a = g.uniform(-0.2, 1.3, shape).astype(np.float32)
        b = (0.7 * a + 0.3 * g.uniform(-0.2, 1.3, shape)).astype(np.float32)
        if shape[-2] * shape[-1] > 1:   # (a single pixel stays a differing pair)
            b[..., ::4, ::3] = a[..., ::4, ::3]
    elif kind == "const":
        a, b = np.full(shape, 0.4375, np.float32), tex
    elif kind == "same":
        a, b = tex, tex.copy()
    else:
        a, b = np.zeros(shape, np.float32), tex
    return a, b


def figures(x, y):
    """utils/loss_utils.py:17-18 and :43-63 on (B,C,H,W) tensors of one dtype -> per-image and averaged L1 and SSIM."""
    C = x.shape[1]
    win = torch.from_numpy(LO.window_2d()).to(x.dtype).expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, win, padding=5, groups=C)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    m = ((2 * mu1_mu2 + LO.C1) * (2 * s12 + LO.C2)) / ((mu1_sq + mu2_sq + LO.C1) * (s1 + s2 + LO.C2))
    d = torch.abs(x - y)
    return {"l1_i": d.flatten(1).mean(1), "ssim_i": m.mean(1).mean(1).mean(1), "l1": d.mean(), "ssim": m.mean()}


def combine(config, f, like):
    """The scalar of one configuration from the four figures `f` (reference tensors or the kernels' outputs alike)."""
    B = f["ssim_i"].reshape(-1).shape[0]
    w, v = (torch.from_numpy(x(B)).to(like) for x in (weights, weights2))
    if config == "l1":
        return f["l1"]
    if config == "ssim":
        return f["ssim"]
    if config == "mix":
        return 0.8 * f["l1"] - 0.2 * f["ssim"]
    if config == "weights":
        return (w * f["ssim_i"]).sum()
    if config == "mean":
        return f["ssim_i"].mean()
    if config == "weights_both":
        return (w * f["l1_i"]).sum() + (v * f["ssim_i"]).sum()
    if config == "mixed_strides":
        return (w * f["l1_i"]).sum() + f["ssim_i"].mean()
    raise KeyError(config)


def config_weights(config, B):
    """(g_l1, g_ssim): the per-image upstream gradients of the per-image means that one configuration amounts to (what kernel_model takes)."""
    z, e, w, v = np.zeros(B, np.float32), np.full(B, 1.0 / B, np.float32), weights(B), weights2(B)
    return {"l1": (e, z), "ssim": (z, e), "mix": (np.float32(0.8) * e, np.float32(-0.2) * e), "weights": (z, w), "mean": (z, e),
            "weights_both": (w, v), "mixed_strides": (w, e)}[config]


@functools.lru_cache(maxsize=None)
def model(shape, kind, config, swapped=False):
    """kernel_model for one case: (per-image ssim, gradient w.r.t. the first image -- of the swapped pair for the second)."""
    a, b = pair(shape, kind)
    return kernel_model(*((b, a) if swapped else (a, b)), *config_weights(config, shape[0]))


@functools.lru_cache(maxsize=None)
def values(shape, kind):
    """{figure: (ref32, fp64)} as float64 numpy."""
    a, b = (torch.from_numpy(x) for x in pair(shape, kind))
    with torch.no_grad():
        f32, f64 = figures(a, b), figures(a.double(), b.double())
    return {k: (f32[k].double().numpy(), f64[k].numpy()) for k in f32}


@functools.lru_cache(maxsize=None)
def gradients(shape, kind, config, wrt):
    """(ref32, fp64) gradients of one configuration w.r.t. image "a", "b" or "ab" (both requiring one: a tuple each)."""
    out = []
    for dt in (torch.float32, torch.float64):
        a, b = (torch.from_numpy(x).to(dt) for x in pair(shape, kind))
        leaves = [t.requires_grad_(True) for t, n in ((a, "a"), (b, "b")) if n in wrt]
        g = torch.autograd.grad(combine(config, figures(a, b), a.detach()), leaves)
        out.append(tuple(x.double().numpy() for x in g))
    return out[0], out[1]


def tensor_bar(ref32, ref64, absolute=False):
    """Largest |error| allowed over a tensor: 4 x ref32's largest, at least 2 fp32 ulp of the largest fp64 magnitude.
    absolute: the identical pair, whose true gradient is zero -- 4 x ref32's largest magnitude."""
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    if absolute:
        return 4.0 * float(np.abs(ref32).max())
    own = float(np.abs(ref32 - ref64).max())
    return max(4.0 * own, 2.0 * float(np.spacing(np.float32(np.abs(ref64).max()))))


def seam_mask(shape):
    """True for pixels within 5 of a 32 x 16 tile seam or of the image border."""
    H, W = shape[-2:]
    y, x = np.arange(H), np.arange(W)
    ny = (y % TY < RAD) | (y % TY >= TY - RAD) | (y >= H - RAD)
    nx = (x % TX < RAD) | (x % TX >= TX - RAD) | (x >= W - RAD)
    return np.broadcast_to(ny[:, None] | nx[None, :], shape)


def assert_tensor(value, ref32, ref64, what, absolute=False, model=None):
    """Holds `value` to the bar over the whole tensor, reporting the seam / border pixels and the interior separately (pytest -s shows the
    distances DESIGN.md section 19 quotes).  model: the float32 model's tensor, for a figure of MODEL_BARS."""
    value, ref32, ref64 = (np.asarray(x, np.float64) for x in (value, ref32, ref64))
    assert value.shape == ref64.shape, (what, value.shape, ref64.shape)
    assert np.isfinite(value).all(), what
    bar = tensor_bar(ref32, ref64, absolute)
    if model is not None:
        bar = max(bar, 2.0 * float(np.abs(np.asarray(model, np.float64) - ref64).max()))
    err, own = np.abs(value - ref64), np.abs(ref32 - ref64)
    seam = seam_mask(value.shape) if value.ndim >= 2 else np.ones(value.shape, bool)
    for name, m in (("seam", seam), ("interior", ~seam)):
        if m.any():
            print(what, name, "distance from fp64:", err[m].max(), "the reference's:", own[m].max(), "bar:", bar)
            assert err[m].max() <= bar, (what, name, float(err[m].max()), bar)


def assert_scalar(value, ref32, ref64, what, model=None):
    """eval_cases.new_bar's rule for one or a few scalars, elementwise, printed as eval_cases.assert_new prints."""
    from eval_cases import new_bar

    value, ref32, ref64 = (np.asarray(x, np.float64).reshape(-1) for x in (value, ref32, ref64))
    assert value.shape == ref64.shape and np.isfinite(value).all(), (what, value)
    bar = new_bar(ref32, ref64)
    if model is not None:
        bar = np.maximum(bar, 2.0 * np.abs(np.asarray(model, np.float64).reshape(-1) - ref64))
    err = np.abs(value - ref64)
    print(what, "distance from fp64:", err.max(), "the reference's:", np.abs(ref32 - ref64).max(), "bar:", bar.min())
    assert np.all(err <= bar), (what, err.tolist(), bar.tolist())


# ---- the float32 model of the kernels' summation order -------------------------------------------------------------------------------------
def _fma(w, x, acc):
    """acc + w * x with one rounding (the product of two float32 is exact in float64), as -ffp-contract=fast compiles `acc += w * x`."""
    return (w.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _window_pass(planes, axis):
    """Eleven taps in the order k = 0 .. 10 along one axis of (..., H, W) float32 planes, zero outside."""
    w = LO.window_1d()
    pad = [(0, 0)] * planes.ndim
    pad[axis] = (RAD, RAD)
    p = np.pad(planes, pad)
    n = planes.shape[axis]
    acc = np.zeros_like(planes)
    for k in range(11):
        acc = _fma(np.broadcast_to(w[k], acc.shape), np.take(p, range(k, k + n), axis=axis), acc)
    return acc


def _separable(planes):
    return _window_pass(_window_pass(planes, -1), -2)


def kernel_model(a, b, g_l1, g_ssim):
    """float32 model of gls_l1_ssim_forward / _backward_split on (B,C,H,W): -> (per-image ssim, d_img1) for per-image upstream gradients
    g_l1, g_ssim of the per-image means ((B,) arrays).  Moments as in k_l1_ssim_fwd; sums of the map in float64 (the order of a sum over
    a plane is not what this models)."""
    f = np.float32
    x, y = a.astype(f), b.astype(f)
    mu1, mu2, e11, e22, e12 = (_separable(p) for p in (x, y, x * x, y * y, x * y))
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    A, Bv = f(2) * mu12 + f(1e-4), f(2) * s12 + f(9e-4)
    Cv, D = mu1_sq + mu2_sq + f(1e-4), s1 + s2 + f(9e-4)
    inv = f(1) / (Cv * D)
    qa, rD = A / Cv, f(1) / D
    m = qa * (Bv / D)
    maps = ((f(2) * mu2 * (Bv - A) - m * f(2) * mu1 * (D - Cv)) * inv, -(m * rD), (f(2) * qa) * rD)
    ca, cb, cc = (_separable(p) for p in maps)
    scale = f(1.0 / (x.shape[1] * x.shape[2] * x.shape[3]))
    gl = (np.asarray(g_l1, f) * scale)[:, None, None, None]
    gs = (np.asarray(g_ssim, f) * scale)[:, None, None, None]
    d = gs * (ca + f(2) * x * cb + y * cc) + gl * np.sign(x - y)
    return m.astype(np.float64).mean(axis=(1, 2, 3)), d.astype(f)


# ---- plain L1 ------------------------------------------------------------------------------------------------------------------------------
#: 4 * 1024 * 255 is where the one-launch grid saturates at 255 workgroups and the grid-stride loop takes its second trip
L1_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 4 * 1024 * 255 - 1, 4 * 1024 * 255, 4 * 1024 * 255 + 1)
L1_SWITCH = (2 ** 26 - 1, 2 ** 26)   # the switch to the two-launch form: generated and referenced on the device


@functools.lru_cache(maxsize=None)
def l1_pair(n):
    g = np.random.default_rng(n)
    a, b = g.random(n, dtype=np.float32), g.random(n, dtype=np.float32)
    a[3::7] = b[3::7]   # exact ties: gradient 0
    return a, b


@functools.lru_cache(maxsize=None)
def l1_reference(n):
    """(ref32, fp64, gradient): the gradient is sign(a - b) / n rounded to float32, the bits the kernels must give."""
    a, b = l1_pair(n)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    return float((ta - tb).abs().mean()), float((ta.double() - tb.double()).abs().mean()), (np.sign(a - b) * np.float32(1.0 / n)).astype(np.float32)


ABNORMAL_N = 4 * 1024 * 3 + 3   # three workgroups of the one-launch form and a tail of three
ABNORMAL = ("nan_first", "nan_tail", "nan_last_group", "pos_inf", "neg_inf", "inf_minus_inf", "sum_4e8", "overflow_3e38", "near_100")
ORDINARY_SHAPE = (3, 37, 41)


@functools.lru_cache(maxsize=None)
def abnormal_pair(name):
    """Inputs outside [0,1): what an unclamped render of a diverging run hands the loss."""
    g = np.random.default_rng(ABNORMAL.index(name) + 77)
    n = {"sum_4e8": 4096, "overflow_3e38": 4096, "near_100": 3 * 802 * 550}.get(name, ABNORMAL_N)
    a, b = g.random(n, dtype=np.float32), g.random(n, dtype=np.float32)
    if name == "nan_first":
        a[0] = np.nan
    elif name == "nan_tail":
        a[n - 1] = np.nan
    elif name == "nan_last_group":
        b[4 * (2 * 1024 + 5) + 1] = np.nan
    elif name == "pos_inf":
        a[4321] = np.inf
    elif name == "neg_inf":
        a[4321] = -np.inf
    elif name == "inf_minus_inf":
        a[4321] = b[4321] = np.inf
    elif name == "sum_4e8":
        a = (1e5 + 100.0 * g.standard_normal(n)).astype(np.float32)
    elif name == "overflow_3e38":
        a, b = (3e38 * (0.9 + 0.1 * a)).astype(np.float32), -b
    elif name == "near_100":
        a = (100.0 + g.standard_normal(n)).astype(np.float32)
    return a, b


@functools.lru_cache(maxsize=None)
def abnormal_reference(name):
    """torch's own (a - b).abs().mean() and autograd gradient on the CPU in float32, and the float64 value: evaluated, never typed in."""
    a, b = abnormal_pair(name)
    ta, tb = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b)
    v = (ta - tb).abs().mean()
    (g,) = torch.autograd.grad(v, ta)
    with torch.no_grad():
        v64 = (ta.double() - tb.double()).abs().mean()
    return float(v.detach()), float(v64), g.numpy()


def value_class(v):
    v = float(v)
    return "nan" if np.isnan(v) else ("+inf" if v == np.inf else ("-inf" if v == -np.inf else "finite"))


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------
STATS_P = (1, 255, 256, 257, 1000)


def stats_inputs(P, seed=0):
    g = np.random.default_rng(1000 * P + seed)
    grad4 = g.normal(0.0, 1e-3, (P, 4)).astype(np.float32)
    acc = g.uniform(0.0, 0.05, (P, 1)).astype(np.float32)
    den = g.integers(0, 40, (P, 1)).astype(np.float32)
    return grad4, acc, den


def add_stats_reference(grad, filt, acc, den):
    """scene/gaussian_model.py:517-519 in float64 for a bool filter -> (accumulator fp64, denom)."""
    out, dn = acc.astype(np.float64).copy(), den.copy()
    g = grad[:, :2].astype(np.float64)
    out[filt, 0] += np.sqrt((g[filt] ** 2).sum(-1))
    dn[filt] += 1.0
    return out, dn
