"""The spatial re-sort of include/gdc.h (ABI 2) without a GPU: header, description and library export the new entries, their argument checks
answer before anything touches a device, the workspace size is monotonic, and a model on CPU tensors -- or any model with
GAA_FUSED_RESORT=0 -- takes the host statement of gaussian_model.spatial_resort with the results it always had."""
import ctypes as C
import os
import re

import pytest
import torch

from gaussianavatars_amd import _lib, densify
from tests import resort_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gdc_order_workspace_bytes", "gdc_morton_order", "gdc_permute")


def test_header_description_and_library_export_the_new_entries():
    txt = open(os.path.join(ROOT, "include", "gdc.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    declared = set(re.findall(r"\b(gdc_[a-z0-9_]+)\s*\(", code))
    assert int(re.search(r"#define\s+GDC_ABI_VERSION\s+(\d+)", txt).group(1)) == 2 == _lib.GDC_ABI_VERSION == _lib.LIBS["gdc"].abi
    lib = _lib.gdc()
    assert lib.gdc_abi_version() == 2
    for name in NEW:
        assert name in declared and name in _lib.GDC_SYMBOLS and getattr(lib, name) is not None
    src = open(os.path.join(ROOT, "gaussianavatars_amd", "csrc", "gdc_kernels.hip")).read()
    assert "GDC_ABI_VERSION" in src and "k_dc_permute" in src and '#include "gdc_order.h"' in src


def test_order_workspace_bytes_is_monotonic_and_bounded():
    lib = _lib.gdc()
    assert lib.gdc_order_workspace_bytes(-1) == -1 and lib.gdc_order_workspace_bytes(_lib.GDC_MAX_SPLATS) == -1
    sizes = [lib.gdc_order_workspace_bytes(P) for P in (0, 1, 2, 255, 256, 257, 4099, 70001, 1_000_000, _lib.GDC_MAX_SPLATS - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[4] < sizes[5]
    assert all(s % 4 == 0 for s in sizes)
    # two key and two row buffers of P words, a 256-entry table row per chunk of 256, and the head
    assert sizes[5] - sizes[4] == 4 * (4 * 1 + 256)


def test_morton_order_argument_checks():
    lib = _lib.gdc()
    order = lambda P, F, xyz, b, i64, c, out, ws: lib.gdc_morton_order(P, F, xyz, b, i64, c, out, ws, None)
    assert order(-1, 0, 16, None, 0, None, 16, 16) == -1 and "P = -1" in _lib.gdc_error()
    assert order(_lib.GDC_MAX_SPLATS, 0, 16, None, 0, None, 16, 16) == -1 and "outside" in _lib.gdc_error()
    assert order(8, -1, 16, None, 0, None, 16, 16) == -1 and "F = -1" in _lib.gdc_error()
    assert order(8, 0, None, None, 0, None, 16, 16) == -1 and "NULL pointer" in _lib.gdc_error()
    assert order(8, 0, 16, None, 0, None, None, 16) == -1 and "NULL pointer" in _lib.gdc_error()
    assert order(8, 0, 16, None, 0, None, 16, None) == -1 and "NULL pointer" in _lib.gdc_error()
    assert order(8, 4, 16, 16, 0, None, 16, 16) == -1 and "bound model" in _lib.gdc_error()          # bound without a centre table
    assert order(8, 4, 16, None, 0, 16, 16, 16) == -1 and "bound model" in _lib.gdc_error()          # a table without a binding
    assert order(8, 0, 16, 16, 0, 16, 16, 16) == -1 and "bound model" in _lib.gdc_error()            # bound with F == 0
    assert order(8, 0, 18, None, 0, None, 16, 16) == -1 and "aligned" in _lib.gdc_error()
    assert order(8, 4, 16, 20, 1, 16, 16, 16) == -1 and "aligned" in _lib.gdc_error()                # an int64 binding on a 4-byte boundary
    assert order(8, 0, 16, None, 0, None, 17, 16) == -1 and "aligned" in _lib.gdc_error()
    assert order(0, 0, None, None, 0, None, None, None) == 0                                         # P == 0: nothing is launched, nothing is needed


def test_permute_argument_checks():
    lib = _lib.gdc()
    one = (_lib.GdcTensor * 1)((16, 32, 3, _lib.GDC_COPY))
    assert lib.gdc_permute(-1, 16, 1, one, None) == -1 and "P = -1" in _lib.gdc_error()
    assert lib.gdc_permute(_lib.GDC_MAX_SPLATS, 16, 1, one, None) == -1 and "outside" in _lib.gdc_error()
    assert lib.gdc_permute(8, 16, _lib.GDC_MAX_TENSORS + 1, one, None) == -1 and "ntensors" in _lib.gdc_error()
    assert lib.gdc_permute(8, 16, 1, None, None) == -1 and "ntensors" in _lib.gdc_error()
    assert lib.gdc_permute(8, None, 1, one, None) == -1 and "NULL pointer" in _lib.gdc_error()
    assert lib.gdc_permute(8, 18, 1, one, None) == -1 and "aligned" in _lib.gdc_error()
    assert lib.gdc_permute(8, 16, 1, (_lib.GdcTensor * 1)((16, None, 3, _lib.GDC_COPY)), None) == -1 and "tensor 0: NULL" in _lib.gdc_error()
    assert lib.gdc_permute(8, 16, 1, (_lib.GdcTensor * 1)((18, 32, 3, _lib.GDC_COPY)), None) == -1 and "tensor 0" in _lib.gdc_error()
    assert lib.gdc_permute(8, 16, 1, (_lib.GdcTensor * 1)((16, 32, -1, _lib.GDC_COPY)), None) == -1 and "tensor 0" in _lib.gdc_error()
    assert lib.gdc_permute(8, 16, 1, (_lib.GdcTensor * 1)((16, 32, 3, _lib.GDC_MOMENT)), None) == -1 and "GDC_COPY" in _lib.gdc_error()
    assert lib.gdc_permute(0, None, 1, one, None) == 0 and lib.gdc_permute(8, 16, 0, None, None) == 0    # nothing to move: nothing is launched


def test_wrapper_argument_checks():
    with pytest.raises(RuntimeError, match="io.morton_order"):
        densify.morton_permutation(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="dtype must be"):
        densify.morton_permutation(torch.zeros(4, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="device vector"):
        densify.permute_rows([torch.zeros(4, 3)], torch.arange(4))


def _expected(before, perm):
    return {k: (None if v is None else v[perm]) for k, v in before.items()}


@pytest.mark.parametrize("env", [None, "0"])
@pytest.mark.parametrize("bound", [True, False])
def test_a_cpu_model_takes_the_host_path_with_the_same_tensors(monkeypatch, env, bound):
    """CPU tensors are outside the kernels' domain whatever GAA_FUSED_RESORT says: no entry of the library is reached, and the model ends
    as the host statement always left it."""
    from gaussianavatars_amd.gaussian_model import spatial_resort, template_face_centers

    if env is None:
        monkeypatch.delenv("GAA_FUSED_RESORT", raising=False)
    else:
        monkeypatch.setenv("GAA_FUSED_RESORT", env)
    monkeypatch.setenv("GAA_FUSED_ADAM", "0")

    def never(*a, **k):
        raise AssertionError("the device path was taken")

    monkeypatch.setattr(densify, "_morton_i32", never)
    monkeypatch.setattr(densify, "permute_rows", never)
    P, F = 517, 16 if bound else 0
    m = U.make_model(P, F, 1, "cpu", seed=3)
    before = U.snapshot(m)
    step = m.optimizer.state[m._xyz]["step"]
    pose = m.optimizer.param_groups[-1]["params"][0]
    want = U.host_order(before["_xyz"].numpy(), None if not bound else before["binding"].numpy(), template_face_centers(m) if bound else None)
    perm = spatial_resort(m)
    assert perm.dtype is torch.long and torch.equal(perm, want) and not torch.equal(perm, torch.arange(P))
    after, exp = U.snapshot(m), _expected(before, want)
    assert set(after) == set(exp) and all(U.same_bits(after[k], exp[k]) for k in exp), [k for k in exp if not U.same_bits(after[k], exp[k])]
    for k, g in zip(U.LEAVES, U.GROUPS):
        group = [x for x in m.optimizer.param_groups if x["name"] == g][0]
        assert group["params"][0] is getattr(m, k) and getattr(m, k).requires_grad
    assert m.optimizer.state[m._xyz]["step"] is step and m.optimizer.param_groups[-1]["params"][0] is pose and len(m.optimizer.state) == 6
    assert torch.equal(spatial_resort(m), torch.arange(P))
    assert torch.equal(spatial_resort(m, fused=False), torch.arange(P))
