"""The launch profile of libgab / libgls (csrc/launch_prof.h behind _lib.launch_profile_enable / launch_profile_read): the table bench.py builds
roofline.all_kernels from.  It counts every launch of the two libraries and of nothing else, starts empty at every enable, stands still when
disabled, and leaves the tables of libgop and libgrl alone."""
import math

import pytest
import torch

from gaussianavatars_amd import _lib, binding, loss

pytestmark = pytest.mark.gpu

N = 3


def _l1_step(a, b):
    a.grad = None
    loss.l1_loss(a, b).backward()


def test_launch_profile_counts_gab_and_gls_launches_only():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    a = torch.rand(3, 16, 16, generator=g).to(dev).requires_grad_(True)
    b = torch.rand(3, 16, 16, generator=g).to(dev)
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], device=dev)
    faces = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32, device=dev)
    others = (_lib.gop_profile_read(), _lib.grl_profile_read())
    try:
        _lib.launch_profile_enable(True)
        for _ in range(N):
            _l1_step(a, b)
        for _ in range(N):
            binding.face_frames(verts, faces)
        torch.cuda.synchronize()
        table = _lib.launch_profile_read()
        print(table)
        assert table and all(k.startswith(("gls::", "gab::")) for k in table), sorted(table)
        assert any(k.startswith("gls::") for k in table) and any(k.startswith("gab::") for k in table), sorted(table)
        for name, (ms, launches) in table.items():
            assert launches > 0 and launches % N == 0, (name, launches)
            assert math.isfinite(ms) and ms > 0, (name, ms)

        # enabling starts from an empty table
        _lib.launch_profile_enable(True)
        assert _lib.launch_profile_read() == {}

        # a disabled profile stands still: the launches of one enabled step stay as they are through a disabled one
        _l1_step(a, b)
        torch.cuda.synchronize()
        one = _lib.launch_profile_read()
        assert one and all(k.startswith("gls::") for k in one)
        _lib.launch_profile_enable(False)
        _l1_step(a, b)
        torch.cuda.synchronize()
        assert _lib.launch_profile_read() == one

        assert (_lib.gop_profile_read(), _lib.grl_profile_read()) == others
    finally:
        _lib.launch_profile_enable(False)
