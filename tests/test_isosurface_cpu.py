"""The surface-nets yardstick (tests/isosurface_reference.py) on analytic fields over a 24 x 20 x 28 lattice with unequal
spacing - closed, consistently wound, of the right genus and volume - and the CPU path of
scorp_amd.mesh.extract_surface against it."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import isosurface_reference as ref


@functools.lru_cache(maxsize=None)
def reference(name):
    coords = ref.lattice()
    return ref.surface_nets(ref.field(name), coords)


def test_sphere_is_closed_oriented_genus_zero_and_of_the_right_volume():
    v, f = reference("sphere")
    assert len(v) > 0 and ref.is_closed_and_oriented(f)
    assert ref.euler_characteristic(v, f) == 2
    vol, h, r = ref.signed_volume(v, f), ref.max_edge(ref.lattice()), 0.7
    # every vertex lies in a cell the surface crosses: within a cell diagonal, sqrt(3) h, of the sphere
    assert 4 / 3 * math.pi * (r - math.sqrt(3) * h) ** 3 < vol < 4 / 3 * math.pi * (r + math.sqrt(3) * h) ** 3
    assert np.all(np.abs(np.linalg.norm(v - np.array([0.03, -0.02, 0.05]), axis=1) - r) <= math.sqrt(3) * h)


def test_torus_has_genus_one():
    v, f = reference("torus")
    assert ref.is_closed_and_oriented(f)
    assert ref.euler_characteristic(v, f) == 0
    assert ref.signed_volume(v, f) > 0


def test_open_surface_and_degenerate_grids():
    v, f = reference("plane")
    assert len(v) > 0 and len(f) > 0 and not ref.is_closed_and_oriented(f)   # it leaves the grid: a boundary
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.all(n @ np.array([0.3, 0.5, 0.8]) > 0)                          # normals from inside (f < 0) to outside
    v, f = reference("none")
    assert v.shape == (0, 3) and f.shape == (0, 3)
    one = np.zeros((2, 2, 2), np.float32) + 1
    one[0, 0, 0] = -1
    v, f = ref.surface_nets(one, [np.array([0.0, 1.0], np.float32)] * 3)
    assert v.shape == (1, 3) and f.shape == (0, 3)
    assert np.allclose(v[0], [1 / 6, 1 / 6, 1 / 6])    # three crossings at t = 0.5, each on one axis


@pytest.mark.parametrize("name", ("sphere", "torus", "plane", "none"))
def test_cpu_path_matches_the_reference(name):
    from scorp_amd.mesh import extract_surface
    coords = ref.lattice()
    v, f = extract_surface(torch.from_numpy(ref.field(name)), [torch.from_numpy(c) for c in coords])
    rv, rf = reference(name)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.shape == rv.shape and np.array_equal(f.numpy(), rf)
    if len(rv):
        assert np.abs(v.numpy().astype(np.float64) - rv).max() <= 1e-5 * ref.max_edge(coords)


def test_extract_surface_argument_errors():
    from scorp_amd.mesh import extract_surface
    c = [torch.linspace(0, 1, 4)] * 3
    with pytest.raises(ValueError, match="grid must be"):
        extract_surface(torch.zeros(4, 4), c)
    with pytest.raises(ValueError, match="coords"):
        extract_surface(torch.zeros(4, 4, 5), c)
    with pytest.raises(ValueError, match="at least 2"):
        extract_surface(torch.zeros(4, 4, 1), [c[0], c[1], torch.zeros(1)])


def test_scan_counts_totals_scans_and_limits():
    """_scan_counts, the step between every count and emit call of the four GPU drivers, on CPU tensors."""
    from scorp_amd.mesh import _scan_counts
    assert _scan_counts(torch.zeros(37, dtype=torch.uint8), 2 ** 31, "vertices") == (0, None)
    counts = torch.from_numpy(np.random.default_rng(5).integers(0, 6, 1000).astype(np.uint8))   # sums far above 255
    total = int(counts.numpy().astype(np.int64).sum())
    assert total > 255
    n, scan = _scan_counts(counts, 2 ** 31, "triangles")
    assert n == total and scan.dtype == torch.int32
    assert np.array_equal(scan.numpy(), np.cumsum(counts.numpy(), dtype=np.int64))
    assert _scan_counts(counts, total + 1, "vertices")[0] == total
    for what in ("vertices", "triangles"):
        for limit in (total, total - 1):
            with pytest.raises(ValueError, match=rf"^the surface has more than 2\^31 - 1 {what}$"):
                _scan_counts(counts, limit, what)
