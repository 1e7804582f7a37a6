"""The 3-nearest-neighbour distances on the GPU (include/gdc.h: gdc_knn3_dist2 through gaussianavatars_amd/knn.py): the exact search against the
float64 brute force of tests/knn_ref.py on every case of its table at the derived bar (16 u relative, 0 absolute), the distCUDA2 stand-in on
the clouds its old body returned zeros on, the opt-out, `create_from_pcd` against the reference's own leaves, and a recorded call."""
import os
import types

import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib, knn
from tests import knn_ref as KR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib.GDC_KNN_CHUNK
CASES = KR.cases(C)
BIG = f"cube_{4 * C + 1}"
KNN_KERNELS = {"gdc::k_ord_clear": 1, "gdc::k_ord_bounds": 1, "gdc::k_ord_codes": 1, "gdc::k_ord_hist": 4, "gdc::k_ord_scan": 4, "gdc::k_ord_scatter": 4,
               "gdc::k_knn_gather": 1, "gdc::k_knn_search": 1}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def refs():
    return {name: KR.brute_force(cloud) for name, cloud in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_matches_the_float64_brute_force(name, refs):
    cloud = CASES[name]
    got = knn.dist2_knn3(torch.from_numpy(cloud).to(_dev()))
    assert got.dtype is torch.float32 and got.shape == (cloud.shape[0],) and got.device.type == "cuda"
    got = got.cpu()
    KR.check(got.numpy(), refs[name], name)
    if name == "dup_4":
        assert not got.any()
    if name == "lattice":
        assert (got == 1.0).all()
    if name == "few_1":
        assert got.tolist() == [0.0]


def test_fused_equals_the_fp32_brute_force_bit_for_bit():
    """The search is exact: on clouds with no tie-breaking freedom in the VALUE (any tie for the third place has the same value) the result is
    the composed difference form's, which evaluates the same fp32 expression over every j."""
    dev = _dev()
    for name in ("far_4", "blobs", "lattice", "dup_2", f"cube_{256 * C + C + 1}"):
        x = torch.from_numpy(CASES[name]).to(dev)
        assert torch.equal(knn.dist2_knn3(x), knn.dist2_knn3_composed(x)), name


def test_results_land_in_input_row_order(refs):
    cloud, perm = KR.shuffled(CASES[BIG])
    dev = _dev()
    got = knn.dist2_knn3(torch.from_numpy(cloud).to(dev))
    KR.check(got.cpu().numpy(), refs[BIG][perm], "shuffled " + BIG)
    assert torch.equal(got.cpu(), knn.dist2_knn3(torch.from_numpy(CASES[BIG]).to(dev)).cpu()[torch.from_numpy(perm)])


def test_types_and_layouts_are_accepted_and_the_input_is_left_alone():
    dev = _dev()
    base = torch.from_numpy(CASES[BIG]).to(dev)
    want = knn.dist2_knn3(base)
    wide = torch.zeros(base.shape[0], 6, device=dev)
    wide[:, ::2] = base
    view = wide[:, ::2]
    assert not view.is_contiguous()
    kept, kept_base = wide.clone(), base.clone()
    leaf = base.clone().requires_grad_(True)
    for t in (base.double(), view, leaf):
        got = knn.dist2_knn3(t)
        assert got.dtype is torch.float32 and not got.requires_grad and torch.equal(got, want)
    assert torch.equal(wide, kept) and torch.equal(base, kept_base)
    assert torch.equal(knn.dist2_knn3(base), want)               # two calls, the same bits
    assert knn.dist2_knn3(torch.zeros(0, 3, device=dev)).shape == (0,)


def test_launches_and_profile_entries():
    dev = _dev()
    x = torch.from_numpy(CASES[BIG]).to(dev)
    knn.dist2_knn3(x)
    _lib.gdc_profile_enable(True)
    try:
        knn.dist2_knn3(x)
        torch.cuda.synchronize()
        prof = _lib.gdc_profile_read()
    finally:
        _lib.gdc_profile_enable(False)
    assert {k: n for k, (_, n) in prof.items()} == KNN_KERNELS


@pytest.mark.parametrize("name", ["far_50", "far_4"])
def test_the_stand_in_is_right_on_clouds_away_from_the_origin(name, refs):
    """Fails on the parent commit: its |a|^2 + |b|^2 - 2 a.b body returns zeros here."""
    from gaussianavatars_amd.shims.simple_knn import _C

    got = _C.distCUDA2(torch.from_numpy(CASES[name]).to(_dev()))
    KR.check(got.cpu().numpy(), refs[name], "distCUDA2 " + name)


def test_the_opt_out_is_the_composed_path(monkeypatch, refs):
    dev = _dev()
    x = torch.from_numpy(CASES["far_4"]).to(dev)
    monkeypatch.setenv("GAA_FUSED_KNN", "0")
    _lib.gdc_profile_enable(True)
    try:
        got = knn.dist2_knn3(x)
        torch.cuda.synchronize()
        assert _lib.gdc_profile_read() == {}
    finally:
        _lib.gdc_profile_enable(False)
    KR.check(got.cpu().numpy(), refs["far_4"], "GAA_FUSED_KNN=0")
    assert torch.equal(got, knn.dist2_knn3(x, fused=False))


def test_create_from_pcd_unbound_matches_the_reference():
    from gaussianavatars_amd.gaussian_model import GaussianModel

    z = np.load(os.path.join(ROOT, "tests", "golden", "pcd_init_pins.npz"))
    p = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("free/")}
    m = GaussianModel(int(p["sh"]))
    m.create_from_pcd(types.SimpleNamespace(points=p["in_points"], colors=p["in_colors"]), float(p["spatial_lr_scale"]), device=_dev())
    KR.check_leaves(m, p, device="cuda")   # _scaling at KR.SCALING_ATOL / KR.SCALING_RTOL, the other leaves exact


def test_graph_replay_gives_the_eager_bits():
    """One call recorded on one stream after an eager warm-up there, replayed twice on changed inputs: the library reads nothing back, waits
    on nothing and allocates nothing."""
    dev = _dev()
    first = CASES[BIG]
    second = np.ascontiguousarray(first[::-1] * np.float32(0.5) + np.float32(3))
    x = torch.from_numpy(first).to(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        knn.dist2_knn3(x)                                        # the warm-up: this stream's workspace
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = knn.dist2_knn3(x)
    for data in (second, first):
        x.copy_(torch.from_numpy(data))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = knn.dist2_knn3(x)
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        KR.check(out.cpu().numpy(), KR.brute_force(data), "replayed")
