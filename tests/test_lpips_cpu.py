"""CPU tests of the LPIPS path (include/glp.h, gaussianavatars_amd/lpips.py): the fp64 restatement of tests/lpips_cases.py against the reference's
own figures (tests/golden/lpips_pins.npz), the composed-torch path on host tensors against the same pins at the measured fp32 constants, the
library's description and every argument check, the weight loader, and the adoption in evaluate.py and patch_reference().  Nothing here launches."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib
from gaussianavatars_amd import lpips as L

import lpips_cases as LC

ROOT = LC.ROOT
PINS = np.load(LC.PINS_PATH)


@pytest.fixture(autouse=True)
def _no_configured_weights(monkeypatch):
    monkeypatch.delenv("GAA_LPIPS_DIR", raising=False)
    monkeypatch.delenv("GAA_FUSED_LPIPS", raising=False)
    L.clear_weights()
    yield
    L.clear_weights()


# ---- the pins ------------------------------------------------------------------------------------------------------------------------------
def test_pins_file_is_small_and_holds_results_and_seeds_only():
    assert os.path.getsize(LC.PINS_PATH) < 16 * 1024
    assert sorted(PINS.files) == sorted(f"{n}_{k}" for n in LC.NET_CASES for k in ("total", "terms", "seed"))
    for name, case in LC.NET_CASES.items():
        assert int(PINS[name + "_seed"]) == case[4] and PINS[name + "_terms"].shape == (5,) and PINS[name + "_total"].dtype == np.float64


@pytest.mark.parametrize("name", list(LC.NET_CASES))
def test_fp64_restatement_reproduces_the_reference(name):
    """Tap positions, eps outside the root, the fp32-rounded z-score constants and the sum over the batch: all of it is the reference's code's."""
    ref = LC.net_reference(name)
    assert LC.rel(ref[:5], PINS[name + "_terms"]) <= 1e-12 and LC.rel(ref[5], PINS[name + "_total"]) <= 1e-12
    assert abs(ref[:5].sum() - ref[5]) <= 1e-15


def test_batch_sum_quirk_is_in_the_pins():
    net, B, H, W, seed = LC.NET_CASES["alex_35x31_b2"]
    x, y = LC.make_inputs(B, H, W, seed)
    singles = [LC.restatement(net, *LC.make_weights(net, seed), x[i:i + 1], y[i:i + 1])[5] for i in range(B)]
    assert abs(float(singles[0] + singles[1]) - float(PINS["alex_35x31_b2_total"])) <= 1e-14 and float(singles[0]) != float(singles[1])


@pytest.mark.parametrize("name", list(LC.NET_CASES))
def test_composed_path_on_host_tensors_against_the_pins(name):
    net, B, H, W, seed = LC.NET_CASES[name]
    weights = L.Weights(net, *LC.make_weights(net, seed))
    x, y = (torch.from_numpy(a) for a in LC.make_inputs(B, H, W, seed))
    got = L.terms(x, y, net, weights)                     # host tensors: the composed path, fp32
    assert got.dtype is torch.float32 and got.shape == (6,)
    assert LC.rel(got.double().numpy(), np.append(PINS[name + "_terms"], PINS[name + "_total"])) <= LC.SCALAR_ERR_FP32 * 1.0000001
    out = L.LPIPS(net, weights=weights)(x, y)
    assert tuple(out.shape) == (1, 1, 1, 1) and float(out) == float(got[5]) == float(L.lpips_composed(x, y, net, weights))
    d = L.lpips_composed(x.double(), y.double(), net, weights)   # other dtypes run in their own precision
    assert d.dtype is torch.float64 and LC.rel(float(d), PINS[name + "_total"]) <= 1e-12
    if B == 1:
        assert float(L.LPIPS(net, weights=weights)(x[0], y[0])) == float(got[5])
    assert float(L.lpips_composed(x, x.clone(), net, weights)) == 0.0


def test_measured_constants_are_the_bars():
    assert LC.GPU_FACTOR == 4.0 and LC.CONV_BAR == 4 * LC.CONV_ERR_FP32 and LC.SCALAR_BAR == 4 * LC.SCALAR_ERR_FP32
    assert 1e-8 < LC.CONV_ERR_FP32 < 1e-5 and 1e-8 < LC.SCALAR_ERR_FP32 < 1e-4     # a wrong tap, stride or padding shows at 1e-2
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%.3e" % LC.CONV_ERR_FP32 in design and "%.3e" % LC.SCALAR_ERR_FP32 in design


# ---- the constants _lib.py mirrors (names in header order, ABI and load failures: tests/test_lib_loader_cpu.py) -----------------------------
def test_description_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "glp.h")).read()
    lib = _lib.glp()
    for name, value in re.findall(r"#define\s+(GLP_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", txt):
        if name not in ("GLP_OK", "GLP_E_ARG", "GLP_E_HIP"):
            assert getattr(_lib, name) == int(value), name
    assert lib.glp_net_convs(_lib.GLP_NET_ALEX) == 5 and lib.glp_net_convs(_lib.GLP_NET_VGG) == _lib.GLP_MAX_CONVS
    mk = open(os.path.join(ROOT, "gaussianavatars_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SINGLE := .*\bglp\b", mk, flags=re.M) and re.search(r"^glp_kernels\.o: CONTRACT := -ffp-contract=fast$", mk, flags=re.M)


def test_layer_tables_of_package_library_and_helper_agree():
    for net, code in (("alex", _lib.GLP_NET_ALEX), ("vgg", _lib.GLP_NET_VGG)):
        convs = [op for op in L.NETS[net]["ops"] if op[0] == "conv"]
        helper = [(i, l) for i, l in enumerate(LC.FEATURES[net]) if l[0] == "conv"]
        assert [(op[1],) + op[2:7] for op in convs] == [(i,) + l[1:] for i, l in helper]
        assert tuple(op[1] + 2 for op in convs if op[7]) == LC.TAPS[net]            # 1-based position of the ReLU after a tapped convolution
        assert tuple(op[3] for op in convs if op[7]) == LC.CHANNELS[net] == L.NETS[net]["channels"]
        assert len(convs) == _lib.glp().glp_net_convs(code) and all(op[3] % _lib.GLP_TILE == 0 for op in convs)
    # the workspace: two buffers of the largest layer for 2B images, and the head partials
    ws = _lib.glp().glp_workspace_bytes
    assert ws(_lib.GLP_NET_VGG, 1, 32, 24) == 2 * (2 * 64 * 32 * 24 * 4) + 5 * 256 * 8
    assert ws(_lib.GLP_NET_ALEX, 2, 35, 31) == 2 * (4 * 64 * 8 * 7 * 4) + 5 * 256 * 8      # the first convolution's 64 x 8 x 7 is alex's largest layer here


def test_bare_import_maps_no_lpips_library():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gaussianavatars_amd\n"
            "from gaussianavatars_amd import _lib\n"
            "import gaussianavatars_amd.lpips, gaussianavatars_amd.evaluate, gaussianavatars_amd.patch\n"
            "print('MAPPED', 'libglp_hip.so' in open('/proc/self/maps').read())\n"
            "print('LOADED', _lib.glp() is not None and 'libglp_hip.so' in open('/proc/self/maps').read())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "MAPPED False" in r.stdout and "LOADED True" in r.stdout, r.stdout


def test_argument_checks_need_no_gpu():
    lib = _lib.glp()
    one, two = C.c_void_p(64), C.c_void_p(128)   # (never dereferenced: every call below is refused before it launches)
    err = lib.glp_last_error
    assert lib.glp_net_convs(2) < 0 and b"unknown net" in err()
    # packing
    assert lib.glp_packed_floats(3, 64, 11) == 368 * 64 and lib.glp_packed_floats(3, 64, 3) == 32 * 64 and lib.glp_packed_floats(512, 512, 3) == 4608 * 512
    assert lib.glp_packed_floats(3, 64, 7) < 0 and b"bad kernel shape" in err()
    assert lib.glp_packed_floats(0, 64, 3) < 0 and lib.glp_packed_floats(1 << 24, 64, 3) < 0 and b"too large" in err()
    assert lib.glp_pack_weights(3, 64, 4, one, two, None) < 0 and b"bad kernel shape" in err()
    assert lib.glp_pack_weights(3, 64, 3, None, two, None) < 0 and b"null pointer" in err()
    # convolution
    conv = lambda N=1, Cin=3, H=8, W=8, Cout=64, k=3, s=1, p=1, x=one, w=one, b=one, out=two: lib.glp_conv2d(N, Cin, H, W, Cout, k, s, p, x, w, b, 1, out, None)
    assert conv(N=0) < 0 and b"bad image shape" in err()
    assert conv(k=7) < 0 and b"bad kernel shape" in err()
    assert conv(Cout=96) < 0 and b"not a multiple of 64" in err()
    assert conv(s=0) < 0 and b"bad stride" in err() and conv(p=3) < 0 and conv(p=-1) < 0
    assert conv(H=2, W=9, k=5, p=1) < 0 and b"smaller than the 5x5 kernel" in err()
    for kw in ("x", "w", "out"):
        assert conv(**{kw: None}) < 0 and b"null pointer" in err(), kw
    assert conv(out=one) < 0 and b"alias" in err()
    assert conv(b=C.c_void_p(66)) < 0 and b"4-byte aligned" in err()
    assert conv(N=1 << 20, H=64, W=64) < 0 and b"too large" in err()
    # pool
    pool = lambda planes=6, H=7, W=5, k=2, s=2, x=one, out=two: lib.glp_maxpool(planes, H, W, k, s, x, out, None)
    assert pool(planes=0) < 0 and b"bad plane shape" in err()
    assert pool(k=3, s=1) < 0 and b"k3 s2 or k2 s2" in err() and pool(k=4) < 0
    assert pool(H=2, k=3) < 0 and b"smaller than the 3x3 window" in err()
    assert pool(x=None) < 0 and b"null pointer" in err() and pool(out=one) < 0 and b"alias" in err()
    # z-score
    assert lib.glp_zscore(0, 4, 4, one, one, two, None) < 0 and b"bad image shape" in err()
    assert lib.glp_zscore(1, 4, 4, one, None, two, None) < 0 and b"null pointer" in err()
    # head and finish
    assert lib.glp_head_blocks(2, 5, 3) == 1 and lib.glp_head_blocks(1, 550, 802) == 256 and lib.glp_head_blocks(1, 16, 17) == 2
    assert lib.glp_head_blocks(0, 5, 3) < 0 and b"bad feature shape" in err()
    assert lib.glp_head(1, 0, 5, 3, one, one, two, None) < 0 and b"bad feature shape" in err()
    assert lib.glp_head(1, 64, 5, 3, one, None, two, None) < 0 and b"null pointer" in err()
    assert lib.glp_head(1, 64, 5, 3, one, one, C.c_void_p(68), None) < 0 and b"8-byte aligned" in err()
    five = lambda *v: (C.c_int32 * 5)(*v)
    assert lib.glp_finish(one, five(1, 1, 1, 1, 1), None, two, None) < 0 and b"null pointer" in err()
    assert lib.glp_finish(C.c_void_p(68), five(1, 1, 1, 1, 1), five(1, 1, 1, 1, 1), two, None) < 0 and b"8-byte aligned" in err()
    assert lib.glp_finish(one, five(1, 1, 257, 1, 1), five(1, 1, 1, 1, 1), two, None) < 0 and b"tap 2: bad block count 257" in err()
    assert lib.glp_finish(one, five(1, 1, 1, 1, 1), five(1, 1, 1, 1, 0), two, None) < 0 and b"tap 4" in err()
    # workspace and the whole chain
    assert lib.glp_workspace_bytes(2, 1, 64, 64) < 0 and b"unknown net" in err()
    assert lib.glp_workspace_bytes(0, 0, 64, 64) < 0 and b"bad image shape" in err()
    assert lib.glp_workspace_bytes(0, 1, 30, 64) < 0 and b"too small for this net" in err()      # alex needs 31: 7 -> pool 3 -> pool 1
    assert lib.glp_workspace_bytes(0, 1, 31, 31) > 0
    assert lib.glp_workspace_bytes(1, 1, 15, 64) < 0 and b"too small" in err() and lib.glp_workspace_bytes(1, 1, 16, 16) > 0
    ptrs = lambda n, hole=None: (C.c_void_p * n)(*[None if i == hole else 64 for i in range(n)])
    fwd = lambda net=0, H=35, x=one, w=ptrs(13), b=ptrs(13), lin=ptrs(5), ws=two: lib.glp_forward(net, 1, H, 35, x, one, w, b, lin, ws, two, None)
    assert fwd(net=5) < 0 and b"unknown net" in err() and fwd(H=20) < 0 and b"too small" in err()
    assert fwd(x=None) < 0 and b"null pointer" in err() and fwd(w=None) < 0 and b"null pointer" in err()
    assert fwd(ws=C.c_void_p(72)) < 0 and b"16-byte aligned" in err()
    assert fwd(w=ptrs(13, 4)) < 0 and b"convolution 4: null" in err() and fwd(net=1, b=ptrs(13, 12)) < 0 and b"convolution 12: null" in err()
    assert fwd(lin=ptrs(5, 3)) < 0 and b"tap 3: null" in err()


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------
def test_load_weights_accepts_both_spellings_pth_and_npz_and_names_a_wrong_shape(tmp_path):
    backbone, lin = LC.make_weights("alex", 11)
    a = L.load_weights("alex", backbone, lin)
    assert L.weights_available("alex") and not L.weights_available("vgg")
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}
    assert sorted(renamed) == [f"{k}.1.weight" for k in range(5)]
    torch.save({k: torch.from_numpy(v) for k, v in backbone.items()}, tmp_path / "alexnet.pth")
    torch.save({k: torch.from_numpy(v) for k, v in renamed.items()}, tmp_path / "alex.pth")
    np.savez(tmp_path / "backbone.npz", **backbone)
    np.savez(tmp_path / "lin.npz", **lin)
    for w in (L.Weights("alex", str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")), L.Weights("alex", str(tmp_path / "backbone.npz"), tmp_path / "lin.npz"),
              L.Weights("alex", {k: torch.from_numpy(v).double() for k, v in backbone.items()}, renamed)):
        assert all(torch.equal(p, q) for p, q in zip(w.conv_w + w.conv_b + w.lin, a.conv_w + a.conv_b + a.lin))
    assert [tuple(w.shape) for w in a.conv_w] == [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3)]
    assert [v.shape[0] for v in a.lin] == [64, 192, 384, 256, 256]
    bad = dict(backbone)
    bad["features.3.weight"] = backbone["features.3.weight"][:, :, :3, :3]
    with pytest.raises(ValueError, match=r"features\.3\.weight: shape \(192, 64, 3, 3\), expected \(192, 64, 5, 5\)"):
        L.load_weights("alex", bad, lin)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight: shape \(1, 64, 1, 1\), expected \(1, 384, 1, 1\)"):
        L.load_weights("alex", backbone, {**lin, "lin2.model.1.weight": lin["lin0.model.1.weight"]})
    with pytest.raises(KeyError, match="features.10.bias is missing"):
        L.load_weights("alex", {k: v for k, v in backbone.items() if k != "features.10.bias"}, lin)
    with pytest.raises(KeyError, match="lin4.model.1.weight or 4.1.weight is missing"):
        L.load_weights("alex", backbone, {k: v for k, v in lin.items() if not k.startswith("lin4")})
    with pytest.raises(ValueError):
        L.load_weights("vgg", backbone, lin)             # alex's shapes are not vgg's
    with pytest.raises(TypeError):
        L.load_weights("alex", 3, lin)


def test_squeeze_and_unknown_nets_raise_and_missing_weights_say_what_is_expected(tmp_path, monkeypatch):
    x = torch.zeros(1, 3, 40, 40)
    with pytest.raises(NotImplementedError, match="squeeze"):
        L.lpips(x, x, net_type="squeeze")
    with pytest.raises(NotImplementedError, match=r"choose net_type from \[alex, squeeze, vgg\]"):
        L.LPIPS("resnet")
    with pytest.raises(NotImplementedError):
        L.load_weights("squeeze", {}, {})
    with pytest.raises(AssertionError):
        L.lpips(x, x, version="0.0")
    assert not L.weights_available("alex") and not L.weights_available("vgg")
    with pytest.raises(FileNotFoundError) as e:
        L.lpips(x, x)
    assert all(s in str(e.value) for s in ("alexnet.pth", "alex.pth", "GAA_LPIPS_DIR is unset", "load_weights", "Nothing is downloaded"))
    monkeypatch.setenv("GAA_LPIPS_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError) as e:
        L.lpips(x, x, net_type="vgg")
    assert "vgg16.pth" in str(e.value) and "vgg.pth" in str(e.value) and repr(str(tmp_path)) in str(e.value)
    with pytest.raises(ValueError):
        L.lpips(x, x[:, :, :5], net_type="vgg")
    # the directory, read lazily at the first call
    backbone, lin = LC.make_weights("alex", 11)
    torch.save({k: torch.from_numpy(v) for k, v in backbone.items()}, tmp_path / "alexnet.pth")
    assert not L.weights_available("alex")               # one of the two files is not enough
    torch.save({k: torch.from_numpy(v) for k, v in lin.items()}, tmp_path / "alex.pth")
    assert L.weights_available("alex") and not L.weights_available("vgg") and "alex" not in L._CONFIGURED
    a, b = (torch.from_numpy(v) for v in LC.make_inputs(1, 64, 48, 11))
    got = float(L.lpips(a, b))
    assert "alex" in L._CONFIGURED and abs(got - float(PINS["alex_64x48_b1_total"])) <= LC.SCALAR_ERR_FP32 * got


# ---- adoption ----------------------------------------------------------------------------------------------------------------------------------
def _png_model(tmp_path):
    from PIL import Image

    g = np.random.default_rng(9)
    method = tmp_path / "model" / "test" / "ours_7"
    (method / "renders").mkdir(parents=True)
    (method / "gt").mkdir()
    for i in range(2):
        gt = g.integers(0, 256, (35, 21, 3), dtype=np.uint8)
        rd = np.clip(gt.astype(np.int32) + g.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
        Image.fromarray(rd).save(method / "renders" / f"{i:05d}.png")
        Image.fromarray(gt).save(method / "gt" / f"{i:05d}.png")
    return tmp_path / "model", method


def test_evaluate_without_weights_is_todays_and_with_vgg_weights_gains_lpips(tmp_path):
    import json

    from gaussianavatars_amd import evaluate as E

    model, method = _png_model(tmp_path)
    out0 = E.evaluate([str(model)], device="cpu")[str(model)]["ours_7"]
    assert set(out0) == {"SSIM", "PSNR"} and "LPIPS" not in open(model / "results.json").read() + open(model / "per_view.json").read()
    acc = E.MetricAccumulator(2, "cpu", lpips_net="vgg")
    assert acc.lpips_net is None and acc.per_view_lpips() is None and set(acc.result()) == {"l1", "psnr", "ssim", "n"}
    L.load_weights("alex", *LC.make_weights("alex", 12))        # alex alone does not switch the metrics.py paths on: their net is vgg
    assert set(E.evaluate([str(model)], device="cpu")[str(model)]["ours_7"]) == {"SSIM", "PSNR"}
    w = L.load_weights("vgg", *LC.make_weights("vgg", 14))
    out1 = E.evaluate([str(model)], device="cpu")[str(model)]["ours_7"]
    assert set(out1) == {"SSIM", "PSNR", "LPIPS"} and out1["SSIM"] == out0["SSIM"] and out1["PSNR"] == out0["PSNR"]
    views = json.load(open(model / "per_view.json"))["ours_7"]
    assert set(views) == {"SSIM", "PSNR", "LPIPS"} and sorted(views["LPIPS"]) == ["00000.png", "00001.png"]
    singles = []
    for name in sorted(views["LPIPS"]):
        a, b = (E._planar(E._decode(str(method / d / name)), "raw") for d in ("renders", "gt"))
        singles.append(float(L.lpips(a, b, net_type="vgg")))
        assert views["LPIPS"][name] == singles[-1] == float(L.lpips_composed(a, b, "vgg", w))
    assert out1["LPIPS"] == (singles[0] + singles[1]) / 2 and singles[0] != singles[1]


def test_evaluate_views_on_the_host_gains_a_fourth_figure_with_alex_weights():
    from gaussianavatars_amd import evaluate as E

    class View:
        timestep = 0

    cams = []
    for s in (21, 22):
        a, b = (torch.from_numpy(v[0]) for v in LC.make_inputs(1, 35, 31, s))
        v = View()
        v.original_image, v.render = b, a * 1.2 - 0.1
        cams.append(v)
    render = lambda view, gaussians, pipe, bg: {"render": view.render}
    ev0 = E.evaluate_views(object(), cams, None, None, render=render)
    L.load_weights("alex", *LC.make_weights("alex", 12))
    ev1 = E.evaluate_views(object(), cams, None, None, render=render)
    assert len(ev0) == 3 and len(ev1) == 4 and ev1[:3] == ev0
    singles = [float(L.lpips(torch.clamp(v.render, 0, 1), torch.clamp(v.original_image, 0, 1))) for v in cams]
    assert ev1[3] == (singles[0] + singles[1]) / 2


def test_adopt_lpips_touches_nothing_without_weights_and_rebinds_with_them(monkeypatch):
    from gaussianavatars_amd import patch

    def ref_lpips(x, y, net_type="alex", version="0.1"):
        return "original"

    mod = types.ModuleType("stand_in_lpipsPyTorch")
    mod.lpips = ref_lpips
    assert patch.adopt_lpips(mod) == [] and mod.lpips is ref_lpips and not hasattr(mod, "_gaa_patched_lpips")      # no weights
    L.load_weights("alex", *LC.make_weights("alex", 12))
    monkeypatch.setenv("GAA_FUSED_LPIPS", "0")
    assert patch.adopt_lpips(mod) == [] and mod.lpips is ref_lpips                                                   # opted out
    monkeypatch.delenv("GAA_FUSED_LPIPS")
    assert patch.adopt_lpips(mod) == ["stand_in_lpipsPyTorch.lpips"] and mod.lpips is L.lpips and patch._ORIG[(mod, "lpips")] is ref_lpips
    assert patch.adopt_lpips(mod) == []                                                                              # idempotent
    a, b = (torch.from_numpy(v) for v in LC.make_inputs(2, 35, 31, 12))
    out = mod.lpips(a, b)
    assert tuple(out.shape) == (1, 1, 1, 1) and abs(float(out) - float(PINS["alex_35x31_b2_total"])) <= LC.SCALAR_ERR_FP32 * float(out)
    patch.unpatch_classes(mod)
    assert mod.lpips is ref_lpips and not hasattr(mod, "_gaa_patched_lpips") and (mod, "lpips") not in patch._ORIG
    import inspect

    src = inspect.getsource(patch.patch_reference)
    assert 'adopt_lpips() if os.environ.get("GAA_FUSED_LPIPS", "1") != "0" else []' in src and "lpips=fused_lpips" in src


REFERENCE = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "lpipsPyTorch")), reason="needs the reference checkout beside this repository")
def test_adopt_lpips_on_the_reference_package_in_a_fresh_process(tmp_path):
    """The reference's own lpipsPyTorch, imported with the package's torchvision stand-in: left alone without weights, rebound with them."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from gaussianavatars_amd import shims, patch, lpips as L\n"
            "import lpips_cases as LC\n"
            "shims.install(stub_torchvision=True)\n"
            "import lpipsPyTorch\n"
            "orig = lpipsPyTorch.lpips\n"
            "print('NONE', patch.adopt_lpips(), lpipsPyTorch.lpips is orig)\n"
            "L.load_weights('vgg', *LC.make_weights('vgg', 14))\n"
            "print('SOME', patch.adopt_lpips(), lpipsPyTorch.lpips is L.lpips)\n" % (ROOT, os.path.join(ROOT, "tests"), REFERENCE))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "NONE [] True" in r.stdout and "SOME ['lpipsPyTorch.lpips'] True" in r.stdout, r.stdout
