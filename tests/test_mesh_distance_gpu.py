"""csrc/mesh_distance.hip on the GPU against tests/mesh_distance_reference.py: the bodies of tests/mesh_distance_checks.py
that tests/test_mesh_distance_cpu.py runs on the numpy form, here on CUDA tensors, plus what only the kernels have: the
grid's header (the pair count under its cap, the cell grown for two scene-sized triangles) and the agreement of the two
forms.  The tolerance is the one measured on the CPU (fixtures.TOL_REL = 16 x 4e-17 = 6.4e-16 D^2).

Measured in one MI355X run (printed by the tests): the kernel's largest |d^2 - yardstick d^2| / D^2 per fixture equals the
numpy form's to the printed digits - collinear 3.82e-17 (the largest), scene_sized 3.55e-17, faces1 2.34e-17, sliver 1.87e-17,
faces2 1.68e-17, sphere_random 1.64e-17, mixed_degenerate 1.37e-17, flat 1.14e-17, max_distance 1.1e-18, the others below
1e-18 - and on the four fixtures compared bit for bit the two forms were equal.  scene_sized: 4902 pairs under the cap of
8176 in 13^3 cells after one growth step; the sphere fixtures: 11 778 pairs (cap 17 536) in 20^3 cells, no growth."""
import numpy as np
import pytest
import torch

from tests import mesh_distance_checks as checks
from tests import mesh_distance_fixtures as fx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fx.FIXTURES)
def test_kernel_matches_the_yardstick(name):
    checks.check_fixture(name, "cuda")


@pytest.mark.parametrize("name", ["sphere_random", "sliver", "scene_sized", "mixed_degenerate"])
def test_kernel_and_numpy_form_give_the_same_bits(name):
    """the two run the same float64 statements with fp contraction off, and the grid never decides a value"""
    gpu, cpu = checks.run(name, "cuda"), checks.run(name, "cpu")
    for a, b, what in zip(gpu, cpu, ("squared_distance", "face", "closest")):
        assert np.array_equal(a, b, equal_nan=True), what


@pytest.mark.parametrize("count", fx.BLOCK_EDGE_COUNTS)
def test_query_counts_at_the_block_edges(count):
    checks.check_block_edges(count, "cuda")


def test_results_do_not_depend_on_order_or_split():
    checks.check_determinism("cuda")


def test_limits():
    checks.check_limits("cuda")


def test_sampler():
    s = checks.check_sampler("cuda")
    cpu = checks.cpu_samples()
    assert torch.equal(s.faces.cpu(), cpu.faces)
    for a, b in ((s.points.cpu(), cpu.points), (s.barycentric.cpu(), cpu.barycentric)):
        assert (np.abs(a.numpy() - b.numpy()) <= np.spacing(np.abs(b.numpy()))).all()


@pytest.mark.parametrize("name", ["cube", "two_clusters"])
def test_nearest_point_distance(name):
    checks.check_nearest(name, "cuda")


def test_nearest_point_ties_and_limits():
    checks.check_nearest_ties("cuda")


def test_metrics():
    checks.check_metrics("cuda")


def test_surface_nets_against_marching_cubes():
    checks.check_nets_against_cubes("cuda")
