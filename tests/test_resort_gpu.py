"""The spatial re-sort on the GPU (include/gdc.h ABI 2, csrc/gdc_order.h, densify.morton_permutation / permute_rows and the device path of
gaussian_model.spatial_resort) against its host statement, io.morton_order on the fp32 positions numpy computes.

Every comparison is exact: the arithmetic that decides a code is fp64 on both sides, the positions are the same two fp32 roundings, and
everything else is a copy.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from gaussianavatars_amd import _lib, densify
from tests import resort_util as U

pytestmark = pytest.mark.gpu
ORDER_KERNELS = {"gdc::k_ord_clear": 1, "gdc::k_ord_bounds": 1, "gdc::k_ord_codes": 1, "gdc::k_ord_hist": 4, "gdc::k_ord_scan": 4, "gdc::k_ord_scatter": 4}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(xyz, binding=None, centers=None, what=""):
    """morton_permutation of the arrays on the device == io.morton_order of the host's fp32 positions; returns the permutation."""
    dev = _dev()
    got = densify.morton_permutation(_d(xyz, dev), _d(binding, dev), _d(centers, dev))
    want = U.host_order(xyz, binding, centers)
    assert got.dtype is torch.long and got.device.type == "cuda" and got.shape == want.shape
    bad = (got.cpu() != want).nonzero().reshape(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {want.numel()} rows differ, first at {int(bad[0])}"
    return got


# ---- permutation equality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 255, 256, 257, 4099, 70001])
def test_the_permutation_is_numpys(P):
    """Unbound, and bound with F = 16 and F = 10 144, binding int32 and int64.  70 001 rows are 274 chunks of 256: the scan of a digit's table
    row gives every thread more than one entry."""
    rng = np.random.default_rng(P)
    xyz = rng.normal(0, 0.3, (P, 3)).astype(np.float32)
    _check(xyz, what="unbound")
    _check((xyz * 1e3).astype(np.float32), what="unbound, large")
    for F in (16, 10144):
        centers = rng.normal(0, 0.2, (F, 3)).astype(np.float32)
        for dt in (np.int32, np.int64):
            binding = rng.integers(0, F, P).astype(dt)
            _check(xyz, binding, centers, what=f"bound F={F} {np.dtype(dt).name}")


# ---- ties and edges -----------------------------------------------------------------------------------------------------------
def test_ties_and_edges():
    P = 4099
    dev = _dev()
    rng = np.random.default_rng(7)
    base = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    same = np.tile(np.array([[0.25, -3.0, 7.5]], np.float32), (P, 1))
    assert torch.equal(_check(same, what="all rows identical").cpu(), torch.arange(P))      # hi == lo on every axis: one code, ties by row
    flat = base.copy()
    flat[:, 1] = -0.125
    _check(flat, what="one degenerate axis")
    twins = np.where((np.arange(P) % 3 == 0)[:, None], np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[-0.4, 0.9, 0.05]], np.float32))
    got = _check(twins.astype(np.float32), what="two clusters of duplicates").cpu()
    first = int((np.arange(P) % 3 != 0).sum())
    assert torch.equal(got[:first], torch.arange(P)[torch.arange(P) % 3 != 0]) and torch.equal(got[first:], torch.arange(P)[torch.arange(P) % 3 == 0])
    corners = base.copy()
    corners[5], corners[4000] = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)                          # rows exactly at lo and hi: codes 0 and 2^30 - 1
    got = _check(corners, what="rows at lo and hi").cpu()
    assert int(got[0]) == 5 and int(got[-1]) == 4000
    # a bound model with 600 splats on one face: one cell, long runs of equal codes
    F = 16
    centers = rng.normal(0, 0.2, (F, 3)).astype(np.float32)
    binding = rng.integers(0, F, P).astype(np.int32)
    binding[1000:1600] = 3
    _check(base, binding, centers, what="600 splats on one face")
    small = (base * 1e-3).astype(np.float32)
    _check(small, binding, centers, what="600 splats on one face, offsets below the cell size")
    # xyz as the [1:] view of a (P + 1, 3) buffer: contiguous, its base on a 4-byte boundary only
    buf = torch.empty(P + 1, 3, device=dev)
    view = buf[1:]
    view.copy_(torch.from_numpy(base))
    assert view.is_contiguous() and view.data_ptr() % 16 == 12
    assert torch.equal(densify.morton_permutation(view).cpu(), U.host_order(base))
    # a binding outside [0, F) is outside the contract (the host path raises): no centre is read and (0, 0, 0) is used -- also for an int64
    # value whose low 32 bits name a face
    wild = binding.astype(np.int64)
    wild[7], wild[9], wild[11], wild[13] = -1, F, 2 ** 32 + 3, -(2 ** 32) + 3
    valid = (wild >= 0) & (wild < F)
    want = U.host_order(base, np.where(valid, wild, F), np.vstack([centers, np.zeros((1, 3), np.float32)]))
    assert torch.equal(densify.morton_permutation(_d(base, dev), _d(wild, dev), _d(centers, dev)).cpu(), want)
    w32 = np.where(valid, wild, -5).astype(np.int32)
    assert torch.equal(densify.morton_permutation(_d(base, dev), _d(w32, dev), _d(centers, dev)).cpu(), want)
    # the library's own int32 tensor through the public entry: the same rows, no conversion
    p32 = densify.morton_permutation(_d(base, dev), dtype=torch.int32)
    assert p32.dtype is torch.int32 and torch.equal(p32.long().cpu(), U.host_order(base))


def test_two_calls_and_a_second_stream_give_the_same_bits():
    dev = _dev()
    rng = np.random.default_rng(11)
    P, F = 70001, 64
    xyz, centers, binding = _d(rng.normal(0, 0.3, (P, 3)).astype(np.float32), dev), _d(rng.normal(0, 0.2, (F, 3)).astype(np.float32), dev), \
        _d(rng.integers(0, F, P).astype(np.int32), dev)
    a = densify.morton_permutation(xyz, binding, centers)
    b = densify.morton_permutation(xyz, binding, centers)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        c = densify.morton_permutation(xyz, binding, centers)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_non_finite_positions_still_give_a_permutation():
    dev = _dev()
    P = 257
    xyz = np.random.default_rng(13).normal(0, 0.3, (P, 3)).astype(np.float32)
    xyz[17, 1], xyz[200, 2] = np.nan, np.inf
    a = densify.morton_permutation(_d(xyz, dev))
    b = densify.morton_permutation(_d(xyz, dev))
    assert torch.equal(a.sort().values.cpu(), torch.arange(P)) and torch.equal(a, b)


# ---- permute_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [257, 4099])
def test_permute_rows_moves_every_bit(P):
    """Rows of 1, 3, 4, 45 and 0 floats, an int64 column and a tensor on a 4-byte-aligned base, filled with random bit patterns (NaN
    payloads among them): the result is t[perm], compared as integers."""
    dev = _dev()
    gen = torch.Generator().manual_seed(P)
    bits = lambda *shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32).to(dev)
    off = torch.empty(P * 45 + 1, device=dev)[1:].view(P, 15, 3)
    off.copy_(bits(P, 15, 3))
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    tensors = [bits(P, 1), bits(P), bits(P, 3), bits(P, 4), bits(P, 15, 3), bits(P, 0, 3), off,
               torch.randint(-2 ** 62, 2 ** 62, (P,), generator=gen, dtype=torch.int64).to(dev),
               torch.randint(-2 ** 31, 2 ** 31 - 1, (P,), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)]
    assert any(t.isnan().any() for t in tensors if t.dtype is torch.float32)
    perm = torch.randperm(P, generator=gen).to(dev)
    for index in (perm, perm.to(torch.int32)):
        out = densify.permute_rows(tensors, index)
        assert len(out) == len(tensors)
        for t, o in zip(tensors, out):
            assert o.shape == t.shape and o.dtype is t.dtype and o.data_ptr() != t.data_ptr() or t.numel() == 0
            assert U.same_bits(o.cpu(), t[perm].cpu())
    # more tensors than one table holds: a second launch, nothing else
    many = [bits(P, 3) for _ in range(_lib.GDC_MAX_TENSORS + 2)]
    _lib.gdc_profile_enable(True)
    try:
        out = densify.permute_rows(many, perm)
        torch.cuda.synchronize()
        assert {k: n for k, (_, n) in _lib.gdc_profile_read().items()} == {"gdc::k_dc_permute": 2}
    finally:
        _lib.gdc_profile_enable(False)
    assert all(U.same_bits(o.cpu(), t[perm].cpu()) for t, o in zip(many, out))
    # an index outside [0, P) reads nothing and writes +0.0
    wild = perm.clone()
    wild[3], wild[P - 1] = -1, P
    o = densify.permute_rows([tensors[4]], wild)[0].view(torch.int32)
    assert not o[3].any() and not o[P - 1].any() and U.same_bits(o[4:P - 1].view(torch.float32).cpu(), tensors[4][perm][4:P - 1].cpu())


# ---- profiling ------------------------------------------------------------------------------------------------------------------
def _profiled_resort(m):
    from gaussianavatars_amd.gaussian_model import spatial_resort

    _lib.gdc_profile_enable(True)
    try:
        perm = spatial_resort(m)
        torch.cuda.synchronize()
        return perm, {k: n for k, (_, n) in _lib.gdc_profile_read().items()}
    finally:
        _lib.gdc_profile_enable(False)


def test_the_device_path_shows_in_the_profile_and_the_host_path_does_not(monkeypatch):
    dev = _dev()
    monkeypatch.delenv("GAA_FUSED_RESORT", raising=False)
    perm, prof = _profiled_resort(U.make_model(4099, 64, 3, dev, seed=1))
    assert prof == {**ORDER_KERNELS, "gdc::k_dc_permute": 1}, prof
    monkeypatch.setenv("GAA_FUSED_RESORT", "0")
    perm0, prof0 = _profiled_resort(U.make_model(4099, 64, 3, dev, seed=1))
    assert prof0 == {} and torch.equal(perm, perm0)


# ---- a live model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_adam", [False, True], ids=["torch_adam", "fused_adam"])
@pytest.mark.parametrize("sh", [3, 0])
def test_a_live_model_ends_as_the_host_path_leaves_it(monkeypatch, sh, fused_adam):
    from gaussianavatars_amd.gaussian_model import spatial_resort
    from gaussianavatars_amd.optim import FusedAdam

    dev = _dev()
    P, F = 4099, 64
    monkeypatch.setenv("GAA_FUSED_ADAM", "1" if fused_adam else "0")
    monkeypatch.delenv("GAA_FUSED_RESORT", raising=False)
    a = U.make_model(P, F, sh, dev, seed=5)
    assert type(a.optimizer) is (FusedAdam if fused_adam else torch.optim.Adam) and a._features_rest.shape[1] == (15 if sh else 0)
    monkeypatch.setenv("GAA_FUSED_ADAM", "0")
    host = U.cpu_twin(a)
    monkeypatch.setenv("GAA_FUSED_ADAM", "1" if fused_adam else "0")
    b = U.make_model(P, F, sh, dev, seed=5)                                   # the same model again, for the host path on the GPU
    steps = {k: a.optimizer.state[getattr(a, k)]["step"] for k in U.LEAVES}
    pose = a.optimizer.param_groups[-1]["params"][0]
    perm, prof = _profiled_resort(a)
    assert prof == {**ORDER_KERNELS, "gdc::k_dc_permute": 1}, prof
    want = spatial_resort(host)
    assert perm.dtype is torch.long and perm.device.type == "cuda" and torch.equal(perm.cpu(), want) and not torch.equal(want, torch.arange(P))
    got, exp = U.snapshot(a), U.snapshot(host)
    assert set(got) == set(exp) and len(got) == 23
    assert all(U.same_bits(got[k], exp[k]) for k in exp), [k for k in exp if not U.same_bits(got[k], exp[k])]
    assert a._gaa_order.device.type == "cuda" and a.binding.dtype is torch.int32
    for k, g in zip(U.LEAVES, U.GROUPS):
        p = getattr(a, k)
        group = [x for x in a.optimizer.param_groups if x["name"] == g][0]
        assert len(group["params"]) == 1 and group["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        assert a.optimizer.state[p]["step"] is steps[k] and float(steps[k]) == 1.0
    assert len(a.optimizer.state) == 6 and a.optimizer.param_groups[-1]["params"][0] is pose and not pose.any()
    again, prof = _profiled_resort(a)
    assert torch.equal(again.cpu(), torch.arange(P)) and sum(prof.values()) == 16
    # the step that follows: the same bits as on the model the host path sorted on the GPU
    monkeypatch.setenv("GAA_FUSED_RESORT", "0")
    perm_b, prof = _profiled_resort(b)
    assert prof == {} and torch.equal(perm_b, perm)
    gen = torch.Generator().manual_seed(9)
    for k in U.LEAVES:
        assert U.same_bits(getattr(a, k).detach().cpu(), getattr(b, k).detach().cpu())
        grad = (torch.randn(getattr(a, k).shape, generator=gen) * 1e-3).to(dev)
        getattr(a, k).grad, getattr(b, k).grad = grad, grad.clone()
    a.optimizer.step()
    b.optimizer.step()
    torch.cuda.synchronize()
    got, exp = U.snapshot(a), U.snapshot(b)
    assert all(U.same_bits(got[k], exp[k]) for k in exp), [k for k in exp if not U.same_bits(got[k], exp[k])]
    assert all(float(a.optimizer.state[getattr(a, k)]["step"]) == 2.0 for k in U.LEAVES)


def test_the_three_cases_of_the_order_bookkeeping(monkeypatch):
    from gaussianavatars_amd.gaussian_model import spatial_resort

    dev = _dev()
    monkeypatch.delenv("GAA_FUSED_RESORT", raising=False)
    m = U.make_model(257, 8, 0, dev, seed=2, optimizer=False, tracked=False)
    perm = spatial_resort(m)                                   # first sort of a freshly loaded model: the order it had until now
    assert torch.equal(m._gaa_order, perm) and m._gaa_order.data_ptr() != perm.data_ptr()
    m._gaa_order = torch.arange(5, device=dev)                 # a row count that was not followed: lost, and it stays lost
    spatial_resort(m)
    assert m._gaa_order is None and m._gaa_order_lost is True
    spatial_resort(m)
    assert m._gaa_order is None
    m = U.make_model(257, 8, 0, dev, seed=2, optimizer=False, tracked=False)
    m._gaa_order = torch.arange(257).flip(0)                   # tracked on the host (what load_ply leaves): composed, and on the device afterwards
    perm = spatial_resort(m)
    assert torch.equal(m._gaa_order.cpu(), (256 - perm).cpu()) and m._gaa_order.device.type == "cuda"


@pytest.mark.parametrize("with_optimizer", [False, True], ids=["no_optimizer", "no_state_yet"])
def test_models_without_optimizer_state(monkeypatch, with_optimizer):
    from gaussianavatars_amd.gaussian_model import spatial_resort

    dev = _dev()
    monkeypatch.delenv("GAA_FUSED_RESORT", raising=False)
    monkeypatch.setenv("GAA_FUSED_ADAM", "0")
    P = 257
    m = U.make_model(P, 8, 3, dev, seed=4, optimizer=with_optimizer, step=False)
    m._opacity.requires_grad_(False)
    host = U.cpu_twin(m)
    assert host._opacity.requires_grad is False
    perm, prof = _profiled_resort(m)
    assert prof == {**ORDER_KERNELS, "gdc::k_dc_permute": 1}, prof
    assert torch.equal(perm.cpu(), spatial_resort(host))
    got, exp = U.snapshot(m), U.snapshot(host)
    assert set(got) == set(exp) and len(got) == 11 and all(U.same_bits(got[k], exp[k]) for k in exp)
    for k, g in zip(U.LEAVES, U.GROUPS):
        p = getattr(m, k)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad is (k != "_opacity")
        if with_optimizer:
            group = [x for x in m.optimizer.param_groups if x["name"] == g][0]
            assert group["params"][0] is p
    if with_optimizer:
        assert len(m.optimizer.state) == 0


def test_optimizer_state_that_is_not_adams_stays_on_the_host_path(monkeypatch):
    """A leaf whose state lacks the two moments, or holds another per-row tensor, is outside the domain: nothing of this library is launched."""
    from gaussianavatars_amd.gaussian_model import _spatial_resort_fused

    dev = _dev()
    monkeypatch.delenv("GAA_FUSED_RESORT", raising=False)
    monkeypatch.setenv("GAA_FUSED_ADAM", "0")
    P = 257
    for extra in ("momentum_only", "amsgrad"):
        m = U.make_model(P, 8, 0, dev, seed=6)
        state = m.optimizer.state[m._scaling]
        if extra == "momentum_only":
            m.optimizer.state[m._scaling] = {"momentum_buffer": torch.zeros(P, 3, device=dev)}
        else:
            state["max_exp_avg_sq"] = torch.zeros(P, 3, device=dev)
        before = m._xyz
        _lib.gdc_profile_enable(True)
        try:
            assert _spatial_resort_fused(m) is None
            torch.cuda.synchronize()
            assert _lib.gdc_profile_read() == {} and m._xyz is before
        finally:
            _lib.gdc_profile_enable(False)


# ---- no hidden synchronisation ------------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_eager_bits():
    """morton_permutation + permute_rows recorded on one stream after an eager warm-up there, replayed on changed inputs: neither call waits
    on the host, reads anything back or allocates outside torch."""
    dev = _dev()
    P, F = 4099, 64
    rng = np.random.default_rng(21)
    first, second = (rng.normal(0, 0.3, (P, 3)).astype(np.float32) for _ in range(2))
    centers, binding = _d(rng.normal(0, 0.2, (F, 3)).astype(np.float32), dev), _d(rng.integers(0, F, P).astype(np.int64), dev)
    rest = _d(rng.normal(0, 1, (P, 15, 3)).astype(np.float32), dev)
    xyz = _d(first, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        densify.permute_rows([xyz, rest, binding], densify.morton_permutation(xyz, binding, centers))     # the warm-up: this stream's workspace
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        perm = densify.morton_permutation(xyz, binding, centers)
        out = densify.permute_rows([xyz, rest, binding], perm)
    for data in (second, first):
        xyz.copy_(torch.from_numpy(data))
        perm.zero_()
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = densify.morton_permutation(xyz, binding, centers)
        torch.cuda.synchronize()
        assert torch.equal(perm, eager) and torch.equal(perm.cpu(), U.host_order(data, binding.cpu().numpy(), centers.cpu().numpy()))
        for t, o in zip((xyz, rest, binding), out):
            assert U.same_bits(o.cpu(), t[eager].cpu())
