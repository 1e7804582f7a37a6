#!/usr/bin/env python3
"""Generates tests/golden/eval_pins.npz by IMPORTING THE REFERENCE (read-only checkout beside this repository) on the CPU -- it does not
travel to the GPU box, so the vectors it produces are committed, as make_golden.py's are.

    python tests/golden/make_eval_golden.py

Pins of the evaluation path (include/gev.h, gaussianavatars_amd/evaluate.py): for four image pairs whose values span [-0.2, 1.3]

    chw (3,37,45)   bchw (2,3,16,32)   small (3,5,7)   pixel (3,1,1)

and each of the three load transforms -- raw, clamp (train.py:277-278), png8 (render.py:41's bytes, then / 255: what metrics.py decodes) --

    <case>_<t>_l1, _ssim      utils/loss_utils.l1_loss / ssim of the transformed pair (fp32 torch-CPU scalars)
    <case>_<t>_psnr3, _mse3   utils/image_utils.psnr / mse in the 3-D convention: one row per channel ((C,1); (B,C) for the batched case, image
                              by image) -- what training_report takes the mean of
    <case>_<t>_psnr4, _mse4   the same in the 4-D convention: one row per image ((B,1); the 3-D cases as a batch of one) -- metrics.py
    <case>_<t>_sums64         (B*C,3) per plane: sum |a-b|, sum (a-b)^2, sum of the SSIM map, from the same fp32 transformed inputs in fp64
    <case>_<t>_l1_64, _ssim_64, _psnr3_64, _mse3_64, _psnr4_64, _mse4_64     the figures above formed from those fp64 sums
    <case>_a, _b              the pair;  <case>_a_u8, _b_u8: render.py:41 of each on the CPU, (H,W,C) / (B,H,W,C) bytes

The distance of a reference fp32 figure from its fp64 twin is the yardstick tests/test_eval_gpu.py scales the new bars (MSE, PSNR) with.
Numeric arrays only.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from unittest import mock  # noqa: E402

with mock.patch.dict(sys.modules, {k: mock.MagicMock() for k in ("matplotlib", "matplotlib.cm") if k not in sys.modules}):
    from utils import image_utils, loss_utils  # noqa: E402  (reference modules; image_utils imports matplotlib for error_map only)

CASES = {"chw": (3, 37, 45), "bchw": (2, 3, 16, 32), "small": (3, 5, 7), "pixel": (3, 1, 1)}


def to_bytes(x):
    """render.py:41 on a planar image or batch, bytes interleaved."""
    perm = (1, 2, 0) if x.dim() == 3 else (0, 2, 3, 1)
    return x.mul(255).add_(0.5).clamp_(0, 255).permute(*perm).to("cpu", torch.uint8).contiguous()


def transformed(x, t):
    if t == "raw":
        return x.clone()
    if t == "clamp":
        return torch.clamp(x, 0.0, 1.0)
    u8 = to_bytes(x)
    perm = (2, 0, 1) if x.dim() == 3 else (0, 3, 1, 2)
    return u8.permute(*perm).to(torch.float32).div(255).contiguous()   # torchvision's to_tensor


def sums64(a, b):
    """(B*C,3) fp64 plane sums of a planar pair (3-D or 4-D)."""
    a4, b4 = (a[None], b[None]) if a.dim() == 3 else (a, b)
    a4, b4 = a4.double(), b4.double()
    C = a4.shape[1]
    w = loss_utils.create_window(11, C).double()   # the reference's fp32 window, exactly, in double
    conv = lambda z: F.conv2d(z, w, padding=5, groups=C)
    mu1, mu2 = conv(a4), conv(b4)
    s1, s2, s12 = conv(a4 * a4) - mu1 * mu1, conv(b4 * b4) - mu2 * mu2, conv(a4 * b4) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    d = a4 - b4
    out = torch.stack([d.abs().sum((2, 3)), (d * d).sum((2, 3)), m.sum((2, 3))], dim=-1)   # (B,C,3)
    return out.reshape(-1, 3).numpy()


def main():
    g = np.random.default_rng(404)
    out = {}
    for name, shape in CASES.items():
        a = g.uniform(-0.2, 1.3, shape).astype(np.float32)
        b = (0.7 * a + 0.3 * g.uniform(-0.2, 1.3, shape)).astype(np.float32)
        if a[0].size > 12:
            b[..., ::4, ::3] = a[..., ::4, ::3]   # exact ties
        a.flat[0], a.flat[-1] = -0.2, 1.3         # the ends of the range are present
        ta, tb = torch.tensor(a), torch.tensor(b)
        out[f"{name}_a"], out[f"{name}_b"] = a, b
        out[f"{name}_a_u8"], out[f"{name}_b_u8"] = to_bytes(ta.clone()).numpy(), to_bytes(tb.clone()).numpy()
        for t in ("raw", "clamp", "png8"):
            xa, xb = transformed(ta, t), transformed(tb, t)
            k = f"{name}_{t}_"
            out[k + "l1"] = loss_utils.l1_loss(xa, xb).numpy()
            out[k + "ssim"] = loss_utils.ssim(xa, xb).numpy()
            if xa.dim() == 3:
                out[k + "psnr3"], out[k + "mse3"] = image_utils.psnr(xa, xb).numpy(), image_utils.mse(xa, xb).numpy()
                out[k + "psnr4"], out[k + "mse4"] = image_utils.psnr(xa[None], xb[None]).numpy(), image_utils.mse(xa[None], xb[None]).numpy()
            else:
                out[k + "psnr3"] = np.stack([image_utils.psnr(p, q).numpy()[:, 0] for p, q in zip(xa, xb)])
                out[k + "mse3"] = np.stack([image_utils.mse(p, q).numpy()[:, 0] for p, q in zip(xa, xb)])
                out[k + "psnr4"], out[k + "mse4"] = image_utils.psnr(xa, xb).numpy(), image_utils.mse(xa, xb).numpy()
            s = sums64(xa, xb)
            B = 1 if xa.dim() == 3 else xa.shape[0]
            C, hw = xa.shape[-3], float(xa.shape[-2] * xa.shape[-1])
            sb = s.reshape(B, C, 3)
            out[k + "sums64"] = s
            out[k + "l1_64"] = np.float64(s[:, 0].sum() / (B * C * hw))
            out[k + "ssim_64"] = np.float64(s[:, 2].sum() / (B * C * hw))
            mse3, mse4 = sb[:, :, 1] / hw, sb[:, :, 1].sum(1) / (C * hw)
            with np.errstate(divide="ignore"):
                p3, p4 = -10.0 * np.log10(mse3), -10.0 * np.log10(mse4)
            shape3 = (C, 1) if xa.dim() == 3 else (B, C)
            out[k + "mse3_64"], out[k + "psnr3_64"] = mse3.reshape(shape3), p3.reshape(shape3)
            out[k + "mse4_64"], out[k + "psnr4_64"] = mse4.reshape(B, 1), p4.reshape(B, 1)
    path = os.path.join(HERE, "eval_pins.npz")
    np.savez_compressed(path, **out)
    print("eval_pins.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
