"""CPU tests of the evaluation path (include/gev.h, gaussianavatars_amd/evaluate.py): the eighth library's description against its header
and the built file, the composed-torch restatement against tests/golden/eval_pins.npz (the reference's own figures, every transform, both PSNR
conventions), the zero-edit adoption on a stand-in module, and the metrics.py stand-in on two tiny PNG directories.  Nothing here launches.

Bars: tests/eval_cases.py."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib
from gaussianavatars_amd import evaluate as E

from eval_cases import CASES, PINS, ROOT, TRANSFORMS, assert_new


def test_pins_file_holds_the_four_pairs_in_range():
    assert PINS["chw_a"].nbytes and os.path.getsize(os.path.join(ROOT, "tests", "golden", "eval_pins.npz")) < 256 * 1024
    for case, shape in CASES.items():
        a, b = PINS[case + "_a"], PINS[case + "_b"]
        assert a.shape == b.shape == shape and a.dtype == np.float32
        assert a.min() == np.float32(-0.2) and a.max() == np.float32(1.3) and b.min() >= -0.2 and b.max() <= 1.3
        assert PINS[case + "_a_u8"].dtype == np.uint8 and PINS[case + "_a_u8"].shape == (shape[1:] + shape[:1] if len(shape) == 3 else (shape[0], *shape[2:], shape[1]))
    assert all(PINS[k].dtype.kind in "fu" for k in PINS.files)


# ---- the constants _lib.py mirrors (names, ABI and load failures: tests/test_lib_loader_cpu.py) --------------------------------------------
def test_description_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "gev.h")).read()
    for name, value in re.findall(r"#define\s+(GEV_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", txt):   # the constants _lib.py mirrors
        if hasattr(_lib, name):
            assert getattr(_lib, name) == int(value), name
    for name in ("GEV_F32_PLANAR", "GEV_U8_INTERLEAVED", "GEV_RAW", "GEV_CLAMP", "GEV_PNG8", "GEV_PSNR_PER_CHANNEL", "GEV_PSNR_PER_IMAGE"):
        assert hasattr(_lib, name) and re.search(r"#define\s+%s\s" % name, txt), name


def test_argument_checks_need_no_gpu():
    lib = _lib.gev()
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused before it launches)
    err = lambda: lib.gev_last_error()
    assert lib.gev_partial_floats(1, 3, 550, 802) == 4 * 3 * 26 * 35 and lib.gev_partial_floats(0, 3, 5, 5) == 0
    assert lib.gev_pair_stats(0, 3, 4, 4, one, 0, one, 0, 0, one, one, None) < 0 and b"bad image shape" in err()
    assert lib.gev_pair_stats(1, 3, 4, 4, None, 0, one, 0, 0, one, one, None) < 0 and b"null pointer" in err()
    assert lib.gev_pair_stats(1, 3, 4, 4, one, 2, one, 0, 0, one, one, None) < 0 and b"unknown layout" in err()
    assert lib.gev_pair_stats(1, 3, 4, 4, one, 0, one, 0, 3, one, one, None) < 0 and b"unknown transform" in err()
    assert lib.gev_accumulate(1, 3, 4, 4, one, 0, one, 0, 0, 2, one, one, None, 0, None, None) < 0 and b"unknown psnr mode" in err()
    assert lib.gev_accumulate(1, 3, 4, 4, one, 0, one, 0, 0, 0, one, one, None, -1, None, None) < 0 and b"row < 0" in err()
    assert lib.gev_pair_stats(1, 3, 4, 4, one, 0, one, 0, 0, C.c_void_p(12), one, None) < 0 and b"8-byte aligned" in err()
    assert lib.gev_to_u8(1, 3, 0, 4, one, one, None, None, None) < 0 and b"bad image shape" in err()
    assert lib.gev_to_u8(1, 3, 4, 4, one, one, one, None, None) < 0 and b"null pointer" in err()


def test_bare_import_maps_no_evaluation_library():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gaussianavatars_amd\n"
            "from gaussianavatars_amd import _lib\n"
            "import gaussianavatars_amd.evaluate, gaussianavatars_amd.patch\n"
            "print('MAPPED', 'libgev_hip.so' in open('/proc/self/maps').read())\n"
            "print('LOADED', _lib.gev() is not None and 'libgev_hip.so' in open('/proc/self/maps').read())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "MAPPED False" in r.stdout and "LOADED True" in r.stdout, r.stdout


# ---- the composed-torch path against the pins -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("case", list(CASES))
def test_composed_path_reproduces_the_pins(case, transform):
    a, b = torch.from_numpy(PINS[case + "_a"]), torch.from_numpy(PINS[case + "_b"])
    k = f"{case}_{transform}_"
    native, other = ("psnr3", "psnr4") if a.dim() == 3 else ("psnr4", "psnr3")
    for per_channel, key in ((None, native), (a.dim() != 3, other)):
        l1, ps, ss = E.frame_metrics(a, b, transform=transform, per_channel_psnr=per_channel)
        assert l1.dtype == ps.dtype == ss.dtype == torch.float32 and l1.dim() == 0
        assert abs(float(l1) - float(PINS[k + "l1"])) < 2e-6 and abs(float(ss) - float(PINS[k + "ssim"])) < 2e-5
        ref32, ref64 = PINS[k + key], PINS[k + key + "_64"]
        if key == "psnr3":   # per channel, then averaged (over the channels, then over the images)
            ref32, ref64 = ref32.reshape(-1, 3).mean(1).mean(), ref64.reshape(-1, 3).mean(1).mean()
        else:
            ref32, ref64 = ref32.mean(), ref64.mean()
        assert_new(float(ps), ref32, ref64, (k, key))
    # the drop-in psnr: the caller's values (the transform applied outside), the reference's shape
    xa, xb = E._planar(a, transform), E._planar(b, transform)
    if a.dim() == 3:
        xa, xb = xa[0], xb[0]
    out = E.psnr(xa, xb)
    assert tuple(out.shape) == (a.shape[0], 1)
    assert_new(out.numpy(), PINS[k + native], PINS[k + native + "_64"], (k, "psnr"))


@pytest.mark.parametrize("case", list(CASES))
def test_composed_bytes_are_the_pinned_bytes_and_score_like_png8(case):
    a, b = torch.from_numpy(PINS[case + "_a"]), torch.from_numpy(PINS[case + "_b"])
    ua, ub = E.to_u8(a), E.to_u8(b)
    assert ua.dtype == torch.uint8 and np.array_equal(ua.numpy(), PINS[case + "_a_u8"]) and np.array_equal(ub.numpy(), PINS[case + "_b_u8"])
    two = E.to_u8(a, also=b)
    assert torch.equal(two[0], ua) and torch.equal(two[1], ub)
    # uint8 interleaved input is the png8 transform of the fp32 image it was made from
    per_channel = a.dim() == 3
    from_bytes = E.frame_metrics(ua, ub, per_channel_psnr=per_channel)
    from_floats = E.frame_metrics(a, b, transform="png8", per_channel_psnr=per_channel)
    mixed = E.frame_metrics(a, ub, transform="png8", per_channel_psnr=per_channel)
    for x, y, z in zip(from_bytes, from_floats, mixed):
        assert float(x) == float(y) == float(z) or (np.isinf(float(x)) and np.isinf(float(y)))


def test_accumulator_on_the_host_and_argument_errors():
    acc = E.MetricAccumulator(5, "cpu")
    singles = []
    for case in ("chw", "small", "bchw"):
        a, b = torch.from_numpy(PINS[case + "_a"]), torch.from_numpy(PINS[case + "_b"])
        acc.update(a, b)
        rows = E._rows(a, b, "clamp", None)
        singles += [r for r in rows]
    r = acc.result()
    assert r["n"] == 4 and acc.per_view().shape == (4, 3) and torch.equal(acc.per_view(), torch.stack(singles))
    want = torch.stack(singles).double().mean(0)
    for i, key in enumerate(("l1", "psnr", "ssim")):
        assert abs(r[key] - float(want[i])) <= 1e-12 * abs(float(want[i]))
    acc.update(a[0], b[0])
    with pytest.raises(IndexError):
        acc.update(a[0], b[0])
    with pytest.raises(ValueError):
        E.frame_metrics(a, b, transform="gamma")
    with pytest.raises(ValueError):
        E.frame_metrics(a, b[:, :, :5])
    with pytest.raises(ValueError):
        E.to_u8(a, also=a[0])
    assert E.MetricAccumulator(2, "cpu").result()["n"] == 0
    l1, ps, ss = E.frame_metrics(a, a.clone())
    assert float(l1) == 0.0 and float(ps) == float("inf") and abs(float(ss) - 1.0) < 2e-5


# ---- adoption ---------------------------------------------------------------------------------------------------------------------------------
def test_adopt_evaluation_rebinds_is_idempotent_and_is_undone():
    from gaussianavatars_amd import patch

    def ref_psnr(img1, img2):
        return "original"

    mod = types.ModuleType("stand_in_image_utils")
    mod.psnr = ref_psnr
    assert patch.adopt_evaluation(mod) == ["stand_in_image_utils.psnr"]
    assert mod.psnr is not ref_psnr and mod._gaa_orig_psnr is ref_psnr and patch._ORIG[(mod, "psnr")] is ref_psnr
    assert patch.adopt_evaluation(mod) == [] and mod._gaa_orig_psnr is ref_psnr      # idempotent
    a = torch.from_numpy(PINS["small_a"])
    assert mod.psnr(a, a) == "original"                      # host tensors: the module's own function
    assert mod.psnr(a.double(), a.double()) == "original" and mod.psnr(a[0], a[0]) == "original" and mod.psnr(1.0, 2.0) == "original"
    patch.unpatch_classes(mod)
    assert mod.psnr is ref_psnr and (mod, "psnr") not in patch._ORIG
    assert not hasattr(mod, "_gaa_patched_eval") and not hasattr(mod, "_gaa_orig_psnr")
    assert patch.adopt_evaluation(mod) == ["stand_in_image_utils.psnr"]             # and can be adopted again
    patch.unpatch_classes(mod)
    assert patch.adopt_evaluation(types.ModuleType("no_psnr_here")) == []


def test_patch_reference_reports_evaluation_and_gaa_fused_eval_0_opts_out():
    import inspect

    from gaussianavatars_amd import patch

    src = inspect.getsource(patch.patch_reference)
    assert 'adopt_evaluation() if os.environ.get("GAA_FUSED_EVAL", "1") != "0" else []' in src and "evaluation=evaluation" in src


# ---- the metrics.py stand-in --------------------------------------------------------------------------------------------------------------------
def test_score_directories_writes_the_reference_layout_without_lpips(tmp_path):
    from PIL import Image

    g = np.random.default_rng(5)
    method = tmp_path / "model" / "test" / "ours_100"
    (method / "renders").mkdir(parents=True)
    (method / "gt").mkdir()
    pairs = {}
    for i in range(3):
        gt = g.integers(0, 256, (9, 13, 3), dtype=np.uint8)
        rd = np.clip(gt.astype(np.int32) + g.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8) if i else gt.copy()
        name = f"{i:05d}.png"
        Image.fromarray(rd).save(method / "renders" / name)
        Image.fromarray(np.dstack([gt, np.full(gt.shape[:2], 255, np.uint8)])).save(method / "gt" / name)   # RGBA: the first three channels count
        pairs[name] = (rd, gt)
    full, per_view = E.score_directories(str(method / "renders"), str(method / "gt"), device="cpu")
    assert set(full) == {"SSIM", "PSNR"} and set(per_view) == {"SSIM", "PSNR"}
    assert list(per_view["PSNR"]) == sorted(pairs) == list(per_view["SSIM"])
    for name, (rd, gt) in pairs.items():   # metrics.py:31-32,72-73 written out: to_tensor, a batch of one, psnr over the whole image
        ta, tb = (torch.from_numpy(x).permute(2, 0, 1).float().div(255)[None] for x in (rd, gt))
        ref = 20 * torch.log10(1.0 / torch.sqrt(((ta - tb) ** 2).reshape(1, -1).mean(1)))
        got = per_view["PSNR"][name]
        assert got == float("inf") if name == "00000.png" else abs(got - float(ref)) <= 4e-6 * float(ref)
        assert abs(per_view["SSIM"][name] - float(E._figures_composed(ta, tb, False)[0, 2])) < 1e-6
    assert per_view["SSIM"]["00000.png"] == pytest.approx(1.0, abs=2e-5) and full["PSNR"] == float("inf")
    out = E.evaluate([str(tmp_path / "model")], device="cpu")
    results = json.load(open(tmp_path / "model" / "results.json"))
    views = json.load(open(tmp_path / "model" / "per_view.json"))
    assert set(results) == {"ours_100"} == set(views) and set(results["ours_100"]) == {"SSIM", "PSNR"}
    assert "LPIPS" not in json.dumps(results) + json.dumps(views)
    assert set(views["ours_100"]["SSIM"]) == set(pairs) and out[str(tmp_path / "model")]["ours_100"]["SSIM"] == results["ours_100"]["SSIM"]
    assert "LPIPS" in E.score_directories.__doc__
