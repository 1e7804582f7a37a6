"""Conditions of the cases tests/test_bound_entry_parity_gpu.py runs (tests/binding_ref.py: raster_case), checked on the CPU with the oracle's
forward and backward on the fp32-rounded float64 world values; no GPU needed.  They are what makes the GPU file's checks bite -- visible and
culled splats side by side, a face whose splats are all culled, gradients that are not all zero -- not tolerances: the camera is changed until
they hold."""
import numpy as np
import pytest

from tests import binding_ref as BR


@pytest.mark.parametrize("scaled_quat", [False, True])
@pytest.mark.parametrize("entry", ["bound", "leaves"])
def test_camera_conditions_at_1000_splats(oracle, entry, scaled_quat):
    radii, binding, nz = BR.oracle_figures(oracle, 1000, scaled_quat, entry)
    vis = radii > 0
    counts, seen = np.bincount(binding, minlength=BR.BIND_F), np.bincount(binding[vis], minlength=BR.BIND_F)
    all_culled = np.nonzero((counts > 0) & (seen == 0))[0]
    print(f"{entry} scaled_quat={scaled_quat}: visible {vis.mean():.3f}, culled {1 - vis.mean():.3f}, all-culled faces {all_culled.tolist()}, "
          f"visible with a non-zero G_w row {nz[vis].mean():.3f}, crowded face: {seen[BR.BIND_HEAVY]} of {counts[BR.BIND_HEAVY]} visible")
    assert vis.mean() >= 0.40
    assert (~vis).mean() >= 0.05
    assert nz[vis].mean() >= 0.25
    assert not nz[~vis].any()
    if entry == "bound":   # (the leaves entry has one face: it cannot be culled as a whole while 40 % of its splats are visible)
        assert len(all_culled) >= 1
        assert seen[BR.BIND_HEAVY] > 300                              # the crowded face's sum is one of visible splats


def test_every_size_keeps_its_odd_shapes():
    """257 and 63 are no multiples of four (the backward's CSR rows start at the next multiple of four floats behind 9 P); the saturated
    logits are the last four rows of every set that has them; the leaves cases sit on face 0 of identity frames."""
    assert BR.RASTER_NS == (1, 63, 257, 1000) and (9 * 63) % 4 and (9 * 257) % 4
    for N in BR.RASTER_NS:
        leaves, binding, sh, gpix, cam = BR.raster_case(N, True, "leaves")
        assert not binding.any() and sh.shape == (N, 16, 3) and gpix.shape == (3, cam.image_height, cam.image_width)
        assert (cam.image_width, cam.image_height) == (96, 80)
        w = BR.world_values(leaves, binding)
        assert np.array_equal(w["xyz"], leaves["_xyz"])
        if N >= 63:
            assert leaves["_opacity"][-4:, 0].tolist() == list(BR.SATURATED)
            assert w["opacity"][-4:, 0].tolist()[::2] == [1.0, 1.0]
