"""The scenes of tests/gs2d_edge_fixtures.py are what they claim to be - checked in float64 alone, without a GPU.

Every scene: the selection's conditions hold (exact replay length at the anchor block, no 1 / 255, T = 0.5 or T = 1e-4
decision on a knife edge), the float64 and the fp32 oracle run, every gradient tensor of the float64 oracle is non-zero,
and relL1(oracle32, f64) - the yardstick tests.util.assert_no_further_from_f64 holds the HIP kernel to in
tests/test_gs2d_backward_edges_gpu.py - is printed per tensor."""
import numpy as np
import pytest

from tests import gs2d_edge_fixtures as F
from tests.util import grad_errors


def _oracles_run(scene):
    wc, wa = F.upstream(scene.size, 7)
    g32, g64 = F.oracle_grads(scene, "all", wc, wa)
    worst = 0.0
    for name in F.GRADS:
        assert np.isfinite(g64[name]).all() and np.isfinite(g32[name]).all(), name
        assert np.abs(g64[name]).sum() > 0, f"{scene.name}: {name} has nothing to compare"
        e = grad_errors(g32[name], g64[name])[1]
        worst = max(worst, e)
        print(f"{scene.name} {name}: relL1(oracle32, f64) {e:.2e}")
    return worst


@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_yields_every_length(size):
    _, cands, rows = F.edge_pool(size)
    print(f"{size[0]}x{size[1]}: pool {F.POOL[size]}, {cands.rows.size} surfels pass (a) and (b), "
          f"the {rows.size} taken end at candidate {int(np.nonzero(cands.rows == rows[-1])[0][0]) + 1}")
    assert rows.size == max(F.LENGTHS) and np.unique(rows).size == rows.size


@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", F.LENGTHS)
def test_edge_scene_replays_exactly_n(n, size):
    scene = F.edge_scene(n, size)
    t = scene.check()
    count = t.blend()[0]
    assert count[F.ANCHOR[1], F.ANCHOR[0]] == n == count.max()
    _oracles_run(scene)


def test_saturating_scene_stops_pixels_at_different_depths():
    scene = F.saturating_scene()
    t = scene.check()
    count, T_final, _, _ = t.blend()
    stopped = count < t.hit.sum(0)
    print(f"saturating: hits blended per pixel {count.min()} .. {count.max()}, {int(stopped.sum())} of {count.size} pixels stop early")
    assert np.unique(count[:8, :8]).size >= 2 and stopped[:8, :8].sum() >= 32
    _oracles_run(scene)


def test_lowpass_scene_has_both_branches():
    scene = F.lowpass_scene()
    n3d, n2d = F.check_lowpass(scene)
    print(f"lowpass: {n3d} hits of the anchor block on the 3-D branch, {n2d} on the low-pass branch")
    _oracles_run(scene)


def test_horizon_scene_has_unsteady_hits():
    scene = F.horizon_scene()
    print(f"horizon: {F.check_horizon(scene)} (block, surfel) hits with p.z a factor 2 off its block-centre value")
    _oracles_run(scene)


def test_uncovered_scene_leaves_a_block_and_scattered_pixels():
    scene = F.uncovered_scene()
    none = F.uncovered_mask(scene)
    print(f"{scene.name}: {scene.kw['means3D'].shape[0]} surfels, {int(none.sum())} of {none.size} pixels without a contributor")
    assert not none[F.ANCHOR[1], F.ANCHOR[0]]
    _oracles_run(scene)
