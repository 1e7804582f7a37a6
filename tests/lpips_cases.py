"""What tests/test_lpips_cpu.py, tests/test_lpips_gpu.py and tests/golden/make_lpips_pins.py share: the two layer tables restated from the
issue's facts (NOT imported from the package), test weights and inputs from numpy's generator, an fp64 restatement of the metric, the cases,
and the bars.

What is restated (lpipsPyTorch/__init__.py, modules/{lpips,networks,utils}.py):
 1. x, y (B,3,H,W) in [0,1] go in as they are (no rescale to [-1,1]);
 2. z-score (x - mean) / std with mean (-.030,-.088,-.188), std (.458,.448,.450);
 3. torchvision's `features` layer by layer, tapped after the ReLU at the 1-based positions TAPS, stopping at the last tap;
 4. every tap is f / (sqrt(sum_c f^2) + 1e-10), eps outside the root;
 5. d = (fx - fy)^2 through a bias-free 1x1 convolution to one channel, then the mean over H and W;
 6. the five (B,1,1,1) results are concatenated along the BATCH axis and summed: one number, over taps and batch.

Bars.  Nobody can say in advance how far an fp32 evaluation of a 13-layer network sits from fp64, so the yardstick is measured: torch's own fp32
convolution and the package's composed fp32 path, on the host, against fp64 on the same fp32 inputs, over every case of this file --

    python tests/lpips_cases.py          (prints every case's figure and the two maxima below)

CONV_ERR_FP32 is the largest |fp32 - fp64| of a convolution output relative to that output's max|.|, SCALAR_ERR_FP32 the largest relative error of
a final scalar (a head's sum, a per-tap term, a net's total).  The HIP path may sit 4 x as far from fp64 (GPU_FACTOR): its K-blocking and MFMA
accumulation order differ from the host's, and fp32 summation error scales with the order; a wrong tap, stride or padding shows at 1e-2."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS_PATH = os.path.join(ROOT, "tests", "golden", "lpips_pins.npz")

MEAN, STD, EPS = (-.030, -.088, -.188), (.458, .448, .450), 1e-10

# measured on the host by `python tests/lpips_cases.py` (torch 2.x CPU, fp32 against fp64; the printout is quoted in DESIGN.md section 20)
CONV_ERR_FP32 = 5.578e-07     # its largest: the 11x11 stride-4 convolution (K = 363); the others 1.3e-7 .. 3.7e-7
SCALAR_ERR_FP32 = 3.937e-06   # its largest: the fifth term of vgg_32x24_b1; the four totals 1.1e-7 .. 3.7e-7, the heads 1.2e-7 and 5e-9
GPU_FACTOR = 4.0
CONV_BAR, SCALAR_BAR = GPU_FACTOR * CONV_ERR_FP32, GPU_FACTOR * SCALAR_ERR_FP32


def _features(net):
    """torchvision's `features` of a net as a list whose entry i is the layer at 1-based position i + 1:
    ("conv", Cin, Cout, k, stride, pad) | ("relu",) | ("pool", k, stride)."""
    if net == "alex":
        return [("conv", 3, 64, 11, 4, 2), ("relu",), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2), ("relu",), ("pool", 3, 2),
                ("conv", 192, 384, 3, 1, 1), ("relu",), ("conv", 384, 256, 3, 1, 1), ("relu",), ("conv", 256, 256, 3, 1, 1), ("relu",), ("pool", 3, 2)]
    assert net == "vgg"
    layers, cin = [], 3
    for block in ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512)):
        for cout in block:
            layers += [("conv", cin, cout, 3, 1, 1), ("relu",)]
            cin = cout
        layers.append(("pool", 2, 2))
    return layers


FEATURES = {"alex": _features("alex"), "vgg": _features("vgg")}
TAPS = {"alex": (2, 5, 8, 10, 12), "vgg": (4, 9, 16, 23, 30)}
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
assert len(FEATURES["alex"]) == 13 and len(FEATURES["vgg"]) == 31

#: whole-network cases: name -> (net, B, H, W, seed)
NET_CASES = {
    "alex_64x48_b1": ("alex", 1, 64, 48, 11),
    "alex_35x31_b2": ("alex", 2, 35, 31, 12),   # the last three convolutions run on 1x1; the batch-sum quirk is visible
    "vgg_32x24_b1": ("vgg", 1, 32, 24, 13),
    "vgg_35x21_b2": ("vgg", 2, 35, 21, 14),     # odd sizes through four floor pools, ending at 2x1
}
#: one convolution alone: (Cin, Cout, k, stride, pad, H, W, N)
CONV_CASES = [
    (3, 64, 11, 4, 2, 35, 31, 2),     # K = 363 tail, stride 4, output 8x7
    (64, 192, 5, 1, 2, 7, 5, 2),      # image smaller than any tile, padding on every side of every pixel
    (3, 64, 3, 1, 1, 17, 19, 1),      # K = 27
    (192, 384, 3, 1, 1, 3, 3, 2),     # Cout = 6 x 64
    (512, 512, 3, 1, 1, 2, 1, 2),     # deepest K = 4608, on two pixels
    (256, 256, 3, 1, 1, 1, 1, 2),     # only the centre tap is inside the image
]
HEAD_CASES = [64, 512]   # channels, on B = 2 pairs of 5x3 positions
POOL_CASES = [(3, 2, 15, 13, 7, 6), (2, 2, 7, 5, 3, 2)]   # (k, stride, H, W, Ho, Wo)


def conv_id(c):
    return "c%dto%d_k%ds%dp%d_%dx%d_n%d" % c


# ---- weights and inputs: numpy's generator only ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_weights(net, seed):
    """-> (backbone, lin): {`features.N.weight` / `.bias`: fp32} with torchvision's 0-based N, He-scaled weights and a small bias (activations stay
    O(1) through 13 layers), and {`lin{k}.model.1.weight`: fp32 (1,C,1,1)}, non-negative as the real ones are."""
    g = np.random.default_rng(seed)
    backbone, lin = {}, {}
    for i, layer in enumerate(FEATURES[net]):
        if layer[0] == "conv":
            _, cin, cout, k = layer[:4]
            backbone[f"features.{i}.weight"] = (g.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
            backbone[f"features.{i}.bias"] = (0.05 * g.standard_normal(cout)).astype(np.float32)
    for t, c in enumerate(CHANNELS[net]):
        lin[f"lin{t}.model.1.weight"] = g.uniform(0.0, 1.0, (1, c, 1, 1)).astype(np.float32)
    return backbone, lin


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, seed):
    """A pair in [0,1]: y is x with a third of something else mixed in, as a render is its ground truth."""
    g = np.random.default_rng(1000 + seed)
    x = g.uniform(0.0, 1.0, (B, 3, H, W)).astype(np.float32)
    y = (0.7 * x + 0.3 * g.uniform(0.0, 1.0, (B, 3, H, W))).astype(np.float32)
    return x, np.clip(y, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def make_conv_case(case):
    cin, cout, k, s, p, H, W, N = case
    g = np.random.default_rng(2000 + 7 * cin + cout + k + H)
    x = g.standard_normal((N, cin, H, W)).astype(np.float32)
    w = (g.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    b = (0.05 * g.standard_normal(cout)).astype(np.float32)
    return x, w, b


@functools.lru_cache(maxsize=None)
def make_head_case(C):
    """feat (4,C,5,3): x's features of two pairs, then y's, non-negative as after a ReLU; position (0,0) of pair 0 is all zero in x only,
    position (4,2) of pair 1 in both.  lin (C,), non-negative."""
    g = np.random.default_rng(3000 + C)
    feat = np.maximum(g.standard_normal((4, C, 5, 3)), 0.0).astype(np.float32)
    feat[2:] = (0.8 * feat[:2] + 0.2 * np.maximum(g.standard_normal((2, C, 5, 3)), 0.0)).astype(np.float32)
    feat[0, :, 0, 0] = 0.0
    feat[1, :, 4, 2] = 0.0
    feat[3, :, 4, 2] = 0.0
    return feat, g.uniform(0.0, 1.0, C).astype(np.float32)


# ---- the restatement, in whatever dtype it is asked for -------------------------------------------------------------------------------------
def conv_ref(x, w, b, stride, pad, relu, dtype=torch.float64):
    out = F.conv2d(torch.from_numpy(x).to(dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype), stride=stride, padding=pad)
    return F.relu(out) if relu else out


def head_ref(feat, lin, dtype=torch.float64):
    """-> the tap's term before the division by H*W: sum over pairs and positions."""
    f, l = torch.from_numpy(feat).to(dtype), torch.from_numpy(lin).to(dtype)
    n = f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + EPS)
    b = f.shape[0] // 2
    return (((n[:b] - n[b:]) ** 2) * l[None, :, None, None]).sum()


def restatement(net, backbone, lin, x, y, dtype=torch.float64):
    """The six points above -> (6,) tensor of `dtype`: the five per-tap terms, each summed over the batch, and their sum."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    # (the reference's buffers are fp32 tensors: in .double() they are the fp32-rounded constants)
    mean, std = (torch.tensor(v, dtype=torch.float32).to(dtype)[None, :, None, None] for v in (MEAN, STD))
    terms = []
    fx, fy = (t(x) - mean) / std, (t(y) - mean) / std
    for pos, layer in enumerate(FEATURES[net], 1):
        if layer[0] == "conv":
            w, b = t(backbone[f"features.{pos - 1}.weight"]), t(backbone[f"features.{pos - 1}.bias"])
            fx, fy = (F.conv2d(f, w, b, stride=layer[4], padding=layer[5]) for f in (fx, fy))
        elif layer[0] == "relu":
            fx, fy = F.relu(fx), F.relu(fy)
        else:
            fx, fy = (F.max_pool2d(f, layer[1], layer[2]) for f in (fx, fy))
        if pos in TAPS[net]:
            nx, ny = (f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + EPS) for f in (fx, fy))
            d = (nx - ny) ** 2
            res = F.conv2d(d, t(lin[f"lin{len(terms)}.model.1.weight"])).mean((2, 3), True)   # (B,1,1,1)
            terms.append(torch.sum(res, 0, True).reshape(()))
            if len(terms) == len(TAPS[net]):
                break
    return torch.stack(terms + [torch.stack(terms).sum()])


@functools.lru_cache(maxsize=None)
def net_reference(name):
    """The fp64 restatement of a whole-network case, computed once: (6,) numpy."""
    net, B, H, W, seed = NET_CASES[name]
    return restatement(net, *make_weights(net, seed), *make_inputs(B, H, W, seed)).numpy()


def rel(value, ref):
    return float(np.max(np.abs(np.asarray(value, np.float64) - np.asarray(ref, np.float64)) / np.abs(np.asarray(ref, np.float64))))


def measure():
    """The fp32 host figures the bars come from; prints every case."""
    import sys

    sys.path.insert(0, ROOT)
    from gaussianavatars_amd import lpips as L

    conv_worst = scalar_worst = 0.0
    for case in CONV_CASES:
        x, w, b = make_conv_case(case)
        ref, got = conv_ref(x, w, b, case[3], case[4], True), conv_ref(x, w, b, case[3], case[4], True, torch.float32)
        e = float((got.double() - ref).abs().max() / ref.abs().max())
        conv_worst = max(conv_worst, e)
        print("conv   %-34s max|err| / max|out| = %.3e" % (conv_id(case), e))
    for C in HEAD_CASES:
        feat, lin = make_head_case(C)
        e = rel(head_ref(feat, lin, torch.float32), head_ref(feat, lin))
        scalar_worst = max(scalar_worst, e)
        print("head   C = %-28d rel err of the sum  = %.3e" % (C, e))
    for name, (net, B, H, W, seed) in NET_CASES.items():
        weights = L.Weights(net, *make_weights(net, seed))
        x, y = (torch.from_numpy(a) for a in make_inputs(B, H, W, seed))
        got = L._terms_composed(x, y, weights).double().numpy()
        assert float(L.lpips_composed(x, y, net, weights)) == np.float32(got[5])
        ref = net_reference(name)
        e = rel(got, ref)
        scalar_worst = max(scalar_worst, e)
        print("net    %-34s rel err: terms %s total %.3e" % (name, " ".join("%.1e" % rel(got[i], ref[i]) for i in range(5)), rel(got[5], ref[5])))
    print("CONV_ERR_FP32 = %.3e   SCALAR_ERR_FP32 = %.3e" % (conv_worst, scalar_worst))


if __name__ == "__main__":
    measure()
