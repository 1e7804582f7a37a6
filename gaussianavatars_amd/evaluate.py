"""Evaluation and export on the kernels of include/gev.h: what the reference does with a rendered image outside the training step.

    frame_metrics(image, gt)        (l1, psnr, ssim) of one pair from ONE pass: training_report's per-image body (train.py:277-288)
    psnr(img1, img2)                drop-in for utils.image_utils.psnr, the reference's (shape[0], 1) result
    to_u8(image, also=None)         the bytes render.py:41 writes, interleaved, on the device (one launch, optionally for a second image)
    MetricAccumulator               running L1 / PSNR / SSIM of N views that stay on the device: update() launches and never waits,
                                    result() is the one host read
    evaluate_views(...)             the loop of train.py:274-303 without tensorboard
    score_directories / evaluate    metrics.py's scoring of the written PNGs, `python -m gaussianavatars_amd.evaluate -m MODEL_PATH ...`

LPIPS (lpips.py, include/glp.h) joins each of the last three when its weights are configured -- lpips.weights_available(): `alex` in
evaluate_views (train.py:296), `vgg` in the metrics.py paths (metrics.py:74) -- and only then: without weights every result is exactly what it
was, with no "LPIPS" key anywhere.

An image of a pair is fp32 planar, (C,H,W) or (B,C,H,W), or uint8 interleaved, (H,W,C) or (B,H,W,C) -- what a decoded PNG is, read as
byte / 255.  `transform` applies to the fp32 ones: "raw", "clamp" (train.py:277-278) or "png8" (the byte to_u8 would write, / 255: the image
metrics.py decodes, without writing it).  PSNR follows the reference's `view(shape[0], -1)`: per channel, then averaged, for 3-D input; per
image for 4-D input; `per_channel_psnr` overrides.  A batch of several images yields the mean of its images' figures.

Device pairs of those two kinds run on the kernels.  Anything else -- host tensors, other dtypes, GAA_FUSED_EVAL=0 -- evaluates the composed
torch expressions below, which restate the reference's and are what the CPU tests hold to the pins.  A missing library is an error, never a
reason to take the composed path.
"""
from __future__ import annotations

import json
import math
import os

import torch
import torch.nn.functional as F

from . import _lib

TRANSFORMS = {"raw": _lib.GEV_RAW, "clamp": _lib.GEV_CLAMP, "png8": _lib.GEV_PNG8}


def fused_default() -> bool:
    """GAA_FUSED_EVAL=0: every call takes the composed-torch path (A/B runs)."""
    return os.environ.get("GAA_FUSED_EVAL", "1") != "0"


# ---- what an argument is -----------------------------------------------------------------------------------------------------------------
def _describe(t):
    """-> (layout, (B,C,H,W)) of an image the kernels read, or None."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
        return None
    s = tuple(t.shape) if t.dim() == 4 else (1, *t.shape)
    if t.dtype is torch.float32:
        return _lib.GEV_F32_PLANAR, s
    if t.dtype is torch.uint8:
        return _lib.GEV_U8_INTERLEAVED, (s[0], s[3], s[1], s[2])
    return None


def _pair(image, gt):
    """-> (layout_a, layout_b, (B,C,H,W)) when the pair runs on the kernels, else None."""
    da, db = _describe(image), _describe(gt)
    if da is None or db is None or not (image.is_cuda and gt.is_cuda and image.device == gt.device) or not fused_default():
        return None
    if da[1] != db[1] or image.dim() != gt.dim() or min(da[1]) < 1:
        return None
    return da[0], db[0], da[1]


def _per_channel(image, per_channel_psnr) -> bool:
    return image.dim() == 3 if per_channel_psnr is None else bool(per_channel_psnr)


def _transform_code(transform) -> int:
    try:
        return TRANSFORMS[transform]
    except KeyError:
        raise ValueError(f"transform must be one of {sorted(TRANSFORMS)}, got {transform!r}") from None


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {_lib.gev_error()}")


def _buffers(image, gt, shape):
    """The contiguous pair, and the two buffers every statistics call writes: (B*C,3) fp64 plane sums and the per-tile scratch."""
    B, Cc, H, W = shape
    dev = image.device
    sums = torch.empty((B * Cc, 3), dtype=torch.float64, device=dev)
    partial = torch.empty(int(_lib.gev().gev_partial_floats(B, Cc, H, W)), dtype=torch.float32, device=dev)
    return image.contiguous(), gt.contiguous(), sums, partial


def _accumulate(image, gt, la, lb, shape, transform, per_channel, per_view, row, acc):
    """gev_accumulate on one pair: two launches, nothing read back.  -> the (B*C,3) fp64 plane sums."""
    a, b, sums, partial = _buffers(image, gt, shape)
    dev = image.device
    with _lib.on_device(dev):
        _check(_lib.gev().gev_accumulate(*shape, a.data_ptr(), la, b.data_ptr(), lb, transform,
                                         _lib.GEV_PSNR_PER_CHANNEL if per_channel else _lib.GEV_PSNR_PER_IMAGE, sums.data_ptr(), partial.data_ptr(),
                                         None if per_view is None else per_view.data_ptr(), row, None if acc is None else acc.data_ptr(),
                                         _lib.raw_stream(dev)), "gev_accumulate")
    return sums


def plane_sums(image, gt, transform="clamp"):
    """(B*C, 3) fp64 device tensor: sum |a-b|, sum (a-b)^2 and the sum of the SSIM map of every plane of a device pair (gev_pair_stats): what
    both PSNR conventions and the two means are composed from."""
    p = _pair(image, gt)
    if p is None:
        raise ValueError("plane_sums needs a device pair of fp32 planar or uint8 interleaved images of one shape")
    la, lb, shape = p
    a, b, sums, partial = _buffers(image, gt, shape)
    dev = image.device
    with _lib.on_device(dev):
        _check(_lib.gev().gev_pair_stats(*shape, a.data_ptr(), la, b.data_ptr(), lb, _transform_code(transform), sums.data_ptr(), partial.data_ptr(),
                                         _lib.raw_stream(dev)), "gev_pair_stats")
    return sums


# ---- the composed-torch restatement (the reference's expressions; host tensors, other dtypes, GAA_FUSED_EVAL=0) ------------------------------
def _to_u8_composed(image):
    perm = (1, 2, 0) if image.dim() == 3 else (0, 2, 3, 1)
    return image.mul(255).add_(0.5).clamp_(0, 255).permute(*perm).to(torch.uint8).contiguous()   # render.py:41


def _planar(x, transform):
    """-> the (B,C,H,W) floating-point image the statistics are taken over."""
    if x.dtype is torch.uint8:
        x = x if x.dim() == 4 else x[None]
        return x.permute(0, 3, 1, 2).to(torch.float32).div(255)   # torchvision's to_tensor
    if not x.is_floating_point():
        raise TypeError(f"images are floating-point planar or uint8 interleaved, got {x.dtype}")
    x = x if x.dim() == 4 else x[None]
    if transform == "clamp":
        return torch.clamp(x, 0.0, 1.0)
    if transform == "png8":
        return _to_u8_composed(x).permute(0, 3, 1, 2).to(x.dtype).div(255)
    return x


_WINDOWS = {}


def _window(channels, like):
    key = (channels, like.device, like.dtype)
    w = _WINDOWS.get(key)
    if w is None:   # utils/loss_utils.py:23-31: the fp32 Gaussian, normalised, as an outer product, one copy per channel
        g = torch.tensor([math.exp(-((x - 5) ** 2) / (2 * 1.5 ** 2)) for x in range(11)])
        g = (g / g.sum()).unsqueeze(1)
        w = _WINDOWS[key] = g.mm(g.t()).float()[None, None].expand(channels, 1, 11, 11).contiguous().to(like)
    return w


def _figures_composed(a, b, per_channel):
    """(B,3) rows of [l1, psnr, ssim] of a planar pair: utils/loss_utils.py:17-18,43-63 and utils/image_utils.py:18-20 written out."""
    B, Cc = a.shape[:2]
    d = a - b
    l1 = d.abs().reshape(B, -1).mean(1)
    sq = d ** 2
    if per_channel:
        ps = (20 * torch.log10(1.0 / torch.sqrt(sq.reshape(B * Cc, -1).mean(1)))).reshape(B, Cc).mean(1)
    else:
        ps = 20 * torch.log10(1.0 / torch.sqrt(sq.reshape(B, -1).mean(1)))
    w = _window(Cc, a)
    conv = lambda z: F.conv2d(z, w, padding=5, groups=Cc)
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu12
    m = ((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return torch.stack([l1, ps, m.reshape(B, -1).mean(1)], dim=1)


def _rows_composed(image, gt, transform, per_channel):
    _transform_code(transform)
    a, b = _planar(image, transform), _planar(gt, transform)
    if a.shape != b.shape:
        raise ValueError(f"image shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    if b.device != a.device or b.dtype != a.dtype:
        b = b.to(a)
    return _figures_composed(a, b, per_channel).to(torch.float32)


# ---- the public interface ------------------------------------------------------------------------------------------------------------------
def _rows(image, gt, transform, per_channel_psnr):
    """(B,3) fp32 rows of [l1, psnr, ssim], on the kernels where the pair allows."""
    per_channel = _per_channel(image, per_channel_psnr)
    p = _pair(image, gt)
    if p is None:
        return _rows_composed(image, gt, transform, per_channel)
    la, lb, shape = p
    table = torch.empty((shape[0], 3), dtype=torch.float32, device=image.device)
    _accumulate(image, gt, la, lb, shape, _transform_code(transform), per_channel, table, 0, None)
    return table


def frame_metrics(image, gt, transform="clamp", per_channel_psnr=None):
    """(l1, psnr, ssim) of one image pair as device scalars: `l1_loss(a, b).mean()`, `psnr(a, b).mean()` and `ssim(a, b).mean()` of
    train.py:286-288 over the transformed pair, from one pass.  An identical pair has PSNR +inf, as in the reference."""
    rows = _rows(image, gt, transform, per_channel_psnr)
    r = rows[0] if rows.shape[0] == 1 else rows.mean(0)
    return r[0], r[1], r[2]


def psnr(img1, img2):
    """utils/image_utils.py:18-20: `20 * log10(1 / sqrt(mse))` with the mse over `view(shape[0], -1)`, shape (shape[0], 1) -- one row per channel
    of a (C,H,W) pair, one per image of a (B,C,H,W) pair.  No transform: the caller's values, as the reference."""
    if (isinstance(img1, torch.Tensor) and isinstance(img2, torch.Tensor) and img1.dtype is torch.float32 and img2.dtype is torch.float32
            and img1.dim() in (3, 4) and img1.shape == img2.shape and img1.numel() > 0 and img1.is_cuda and img2.device == img1.device
            and fused_default()):
        # rows of shape[0]: a (C,H,W) pair is C one-plane images
        shape = (img1.shape[0], 1, *img1.shape[1:]) if img1.dim() == 3 else tuple(img1.shape)
        table = torch.empty((shape[0], 3), dtype=torch.float32, device=img1.device)
        _accumulate(img1, img2, _lib.GEV_F32_PLANAR, _lib.GEV_F32_PLANAR, shape, _lib.GEV_RAW, False, table, 0, None)
        return table[:, 1:2]
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def to_u8(image, also=None):
    """The uint8 (H,W,C) -- (B,H,W,C) for a batch -- image render.py:41 hands to PIL, bit for bit (one fp32 multiply by 255, one add of 0.5, clamp,
    truncation), still on the device.  `also`: a second image of the same shape converted by the same launch (the ground truth render.py:85
    writes beside every render); the result is then the pair."""
    if also is not None and (not isinstance(also, torch.Tensor) or also.shape != image.shape):
        raise ValueError("`also` must be an image of the same shape")
    if image.dim() not in (3, 4):
        raise ValueError("images must be (C,H,W) or (B,C,H,W)")
    fused = (image.is_cuda and image.dtype is torch.float32 and image.numel() > 0 and fused_default()
             and (also is None or (also.dtype is torch.float32 and also.device == image.device)))
    if not fused:
        out = _to_u8_composed(image)
        return out if also is None else (out, _to_u8_composed(also))
    lib = _lib.gev()
    B, Cc, H, W = tuple(image.shape) if image.dim() == 4 else (1, *image.shape)
    dev = image.device
    oshape = (B, H, W, Cc) if image.dim() == 4 else (H, W, Cc)
    src, dst = image.contiguous(), torch.empty(oshape, dtype=torch.uint8, device=dev)
    src2 = dst2 = None
    if also is not None:
        src2, dst2 = also.contiguous(), torch.empty(oshape, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _check(lib.gev_to_u8(B, Cc, H, W, src.data_ptr(), dst.data_ptr(), None if src2 is None else src2.data_ptr(),
                             None if dst2 is None else dst2.data_ptr(), _lib.raw_stream(dev)), "gev_to_u8")
    return dst if also is None else (dst, dst2)


class MetricAccumulator:
    """Running L1 / PSNR / SSIM of up to `n_views` images, resident on `device`: a (n_views, 3) fp32 table of the per-view figures and four
    doubles [l1, psnr, ssim, count].  The sums are fp64 sums of fp32 figures, as the reference's `.double()` followed by `+=` makes them
    (train.py:286-288).  `update` enqueues two launches and returns; `result` reads the 32 bytes.
    `lpips_net` ("alex" / "vgg"): when that net's weights are configured (lpips.weights_available), every view's LPIPS over the same transformed
    pair is kept in a table of its own and `result` gains "lpips", their mean (one more read); otherwise nothing changes."""

    def __init__(self, n_views: int, device, lpips_net=None):
        self.device = torch.device(device)
        self.table = torch.zeros((int(n_views), 3), dtype=torch.float32, device=self.device)
        self.acc = torch.zeros(4, dtype=torch.float64, device=self.device)
        self.n = 0   # rows handed out (host-side: known without reading the device)
        self.lpips_net = self.lpips_table = None
        if lpips_net is not None:
            from . import lpips as L

            if L.weights_available(lpips_net):
                self.lpips_net = lpips_net
                self.lpips_table = torch.zeros(int(n_views), dtype=torch.float32, device=self.device)

    def update(self, image, gt, transform="clamp", per_channel_psnr=None) -> None:
        per_channel = _per_channel(image, per_channel_psnr)
        p = _pair(image, gt) if self.device.type == "cuda" and isinstance(image, torch.Tensor) and image.device == self.device else None
        B = p[2][0] if p is not None else (image.shape[0] if image.dim() == 4 else 1)
        if self.n + B > self.table.shape[0]:
            raise IndexError(f"MetricAccumulator of {self.table.shape[0]} views is full")
        if p is not None:
            _accumulate(image, gt, p[0], p[1], p[2], _transform_code(transform), per_channel, self.table, self.n, self.acc)
        else:
            rows = _rows_composed(image, gt, transform, per_channel).to(self.device)
            self.table[self.n:self.n + B] = rows
            self.acc[:3] += rows.double().sum(0)
            self.acc[3] += B
        if self.lpips_net is not None:
            from . import lpips as L

            with torch.no_grad():   # one image at a time: the reference's sum over a batch (train.py:296) is the sum of these
                a, b = _planar(image, transform), _planar(gt, transform)
                for i in range(B):
                    self.lpips_table[self.n + i] = L.lpips(a[i:i + 1], b[i:i + 1].to(a), self.lpips_net).reshape(()).to(self.device)
        self.n += B

    def result(self) -> dict:
        """dict(l1, psnr, ssim, n): the means over the views so far (Python floats), after one host read; with LPIPS on, also `lpips`."""
        l1, ps, ss, n = self.acc.tolist()
        more = {} if self.lpips_net is None else dict(lpips=float(self.lpips_table[:self.n].double().mean()) if self.n else float("nan"))
        if n == 0:
            return dict(l1=float("nan"), psnr=float("nan"), ssim=float("nan"), n=0, **more)
        return dict(l1=l1 / n, psnr=ps / n, ssim=ss / n, n=int(n), **more)

    def per_view(self):
        """(n, 3) fp32 device tensor: [l1, psnr, ssim] of every view so far, in the order of the updates."""
        return self.table[:self.n]

    def per_view_lpips(self):
        """(n,) fp32 device tensor: the LPIPS of every view so far, or None when LPIPS is off."""
        return None if self.lpips_net is None else self.lpips_table[:self.n]


def evaluate_views(gaussians, views, pipe, bg, render=None):
    """The loop body of train.py:274-303 over `views`, without tensorboard: select the mesh by the view's timestep when the model has
    more than one, render, clamp both images and accumulate.  -> (l1, psnr, ssim) means as Python floats.  One host read, at the end.
    With the `alex` LPIPS weights configured (lpips.weights_available("alex"); train.py:296's net) -> (l1, psnr, ssim, lpips): the mean over
    the views of their LPIPS, which is what train.py:302 forms from its sums over batches of 16."""
    if render is None:
        from .gaussian_renderer import render
    views = list(views)
    acc = None
    with torch.no_grad():
        for view in views:
            if getattr(gaussians, "num_timesteps", 1) > 1:
                gaussians.select_mesh_by_timestep(view.timestep)
            image = render(view, gaussians, pipe, bg)["render"]
            if acc is None:
                acc = MetricAccumulator(len(views), image.device, lpips_net="alex")
            acc.update(image, view.original_image.to(image.device), transform="clamp")
    if acc is None:
        raise ValueError("no views to evaluate")
    r = acc.result()
    return (r["l1"], r["psnr"], r["ssim"]) + ((r["lpips"],) if "lpips" in r else ())


def _decode(path):
    """The first three channels of an 8-bit image file as a uint8 (H,W,C) host tensor (metrics.py:29-32 keeps `[:, :3]` of to_tensor)."""
    import numpy as np
    from PIL import Image

    arr = np.array(Image.open(path))
    if arr.dtype != np.uint8:
        raise ValueError(f"{path}: only 8-bit images are scored (got {arr.dtype})")
    if arr.ndim == 2:
        arr = arr[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(arr[:, :, :3]))


def score_directories(renders_dir, gt_dir, device=None):
    """metrics.py:62-86 for one method: SSIM and PSNR of every file of `renders_dir` against the file of the same name in `gt_dir`.  PIL decodes
    on the host, the bytes are uploaded as they are (uint8 interleaved; the kernels divide by 255 as to_tensor does), and the running sums stay
    on the device.  -> (full, per_view) with the reference's key layout: {"SSIM": mean, "PSNR": mean} and {"SSIM": {name: value}, "PSNR": {...}}.
    "LPIPS" (net `vgg`, metrics.py:74) joins both dicts when, and only when, its weights are configured (lpips.weights_available("vgg")): a
    made-up value would be worse than none."""
    dev = torch.device(device) if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    names = sorted(os.listdir(renders_dir))
    acc = MetricAccumulator(max(len(names), 1), dev, lpips_net="vgg")
    for name in names:
        a, b = _decode(os.path.join(renders_dir, name)), _decode(os.path.join(gt_dir, name))
        acc.update(a[None].to(dev), b[None].to(dev), transform="raw", per_channel_psnr=False)
    r, rows = acc.result(), acc.per_view().tolist()
    full = {"SSIM": r["ssim"], "PSNR": r["psnr"]}
    per_view = {"SSIM": {n: row[2] for n, row in zip(names, rows)}, "PSNR": {n: row[1] for n, row in zip(names, rows)}}
    if "lpips" in r:
        full["LPIPS"] = r["lpips"]
        per_view["LPIPS"] = dict(zip(names, acc.per_view_lpips().tolist()))
    return full, per_view


def evaluate(model_paths, device=None) -> dict:
    """metrics.py:36-93: for every model path, every method under <path>/test is scored (its `renders` against its `gt`) and
    <path>/results.json and <path>/per_view.json are written.  -> {model path: {method: {"SSIM": ..., "PSNR": ...}}}, with "LPIPS" beside them
    when the `vgg` weights are configured."""
    out = {}
    for scene_dir in model_paths:
        print("Scene:", scene_dir)
        full, per_view = {}, {}
        test_dir = os.path.join(scene_dir, "test")
        for method in sorted(os.listdir(test_dir)):
            method_dir = os.path.join(test_dir, method)
            full[method], per_view[method] = score_directories(os.path.join(method_dir, "renders"), os.path.join(method_dir, "gt"), device)
            print("Method:", method)
            print("  SSIM : {:>12.7f}".format(full[method]["SSIM"]))
            print("  PSNR : {:>12.7f}".format(full[method]["PSNR"]))
            if "LPIPS" in full[method]:
                print("  LPIPS: {:>12.7f}".format(full[method]["LPIPS"]))
        with open(os.path.join(scene_dir, "results.json"), "w") as fp:
            json.dump(full, fp, indent=True)
        with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
            json.dump(per_view, fp, indent=True)
        out[scene_dir] = full
    return out


def main(argv=None) -> None:
    from argparse import ArgumentParser

    parser = ArgumentParser(description="SSIM and PSNR of the rendered test views of trained models (metrics.py), and LPIPS when GAA_LPIPS_DIR "
                                        "holds vgg16.pth and vgg.pth")
    parser.add_argument("--model_paths", "-m", required=True, nargs="+", type=str, default=[])
    evaluate(parser.parse_args(argv).model_paths)


if __name__ == "__main__":
    main()
