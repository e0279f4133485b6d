"""The dense marching-cubes kernels (csrc/marching_cubes.hip) against the numpy float64 yardstick
(tests/marching_cubes_reference.py): identical vertex count and face indices, vertex positions within 1e-5 h (h the largest
cell edge; the bound of the surface-nets tests for the same t = (level - f0) / (f1 - f0) - one crossing per vertex here: a
division and a multiply-add, under 10 fp32 epsilons of h), and a second run bit-equal to the first."""
import functools

import numpy as np
import pytest
import torch

from tests import marching_cubes_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(name):
    return ref.random_field() if name == "random" else (ref.field(name), ref.lattice())


@functools.lru_cache(maxsize=None)
def reference(name, level=0.0):
    g, coords = _inputs(name)
    return ref.marching_cubes(g, coords, level=np.float32(level))


def _extract(dev, g, coords, level=0.0):
    from scorp_amd.mesh import extract_surface
    return extract_surface(torch.from_numpy(g).to(dev), [torch.from_numpy(np.asarray(c)).to(dev) for c in coords], level=level,
                           method="marching_cubes")


@pytest.mark.parametrize("name, level", [("sphere", 0.0), ("torus", 0.0), ("plane", 0.0), ("random", 0.0), ("sphere", 0.1)])
def test_kernels_match_the_reference(dev, name, level):
    g, coords = _inputs(name)
    v, f = _extract(dev, g, coords, level)
    rv, rf = reference(name, level)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.shape == rv.shape
    assert np.array_equal(f.cpu().numpy(), rf)
    err = float(np.abs(v.cpu().numpy().astype(np.float64) - rv).max())
    print(f"{name} at {level}: {len(rv)} vertices, {len(rf)} faces, max vertex error {err / ref.max_edge(coords):.3e} h")
    assert err <= 1e-5 * ref.max_edge(coords)
    v2, f2 = _extract(dev, g, coords, level)
    assert torch.equal(v2, v) and torch.equal(f2, f)


def test_random_field_mesh_is_closed_and_uses_every_vertex(dev):
    g, coords = ref.random_field()
    v, f = _extract(dev, g, coords)
    f = f.cpu().numpy()
    assert len(v) == 16700 and len(np.unique(f)) == len(v)
    assert ref.is_closed_and_oriented(f)


def test_no_crossing_gives_an_empty_mesh(dev):
    v, f = _extract(dev, ref.field("none"), ref.lattice())
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    torch.cuda.synchronize()


def test_single_cell(dev):
    g = np.ones((2, 2, 2), np.float32)
    g[0, 0, 0] = -1.0
    c = np.array([0.0, 1.0], np.float32)
    v, f = _extract(dev, g, (c, c, c))
    assert torch.equal(v.cpu(), 0.5 * torch.eye(3)) and f.cpu().tolist() == [[0, 1, 2]]


def test_floater_removal_on_the_three_spheres(dev):
    """The three-sphere field of the clustering tests: marching cubes gives three clusters - the two large spheres and the
    octahedron (8 triangles) round the one lattice point of the small one - where no mesh edge carries more than two
    triangles; post_process_mesh drops the floater (below the floor of 50 triangles) and leaves two closed spheres."""
    from scorp_amd.mesh import Mesh, cluster_connected_triangles, post_process_mesh
    from tests.mesh_cluster_reference import three_spheres
    g, coords = three_spheres()
    v, f = _extract(dev, g, coords)
    _, n, _ = cluster_connected_triangles(f)
    n = n.cpu().tolist()
    assert len(n) == 3 and sorted(n)[0] == 8 and sum(n) == f.shape[0]
    out = post_process_mesh(Mesh(v, f, torch.zeros_like(v)), cluster_to_keep=50)
    kept = out.faces.cpu().numpy()
    assert len(kept) == sum(n) - 8 and ref.is_closed_and_oriented(kept)
    assert len(np.unique(kept)) == out.vertices.shape[0] == v.shape[0] - 6
    _, n2, _ = cluster_connected_triangles(out.faces)
    assert sorted(n2.cpu().tolist()) == sorted(n)[1:]


def test_errors(dev):
    from scorp_amd import _C
    L = _C.lib()
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    s = _C.current_stream_ptr()
    assert L.scorp_marching_cubes_count_edges(None, 2, 2, 2, 0.0, out.data_ptr(), out.data_ptr(), s) != 0
    assert L.scorp_marching_cubes_count_edges(buf.data_ptr(), 1, 2, 2, 0.0, out.data_ptr(), out.data_ptr(), s) != 0
    assert L.scorp_marching_cubes_count_faces(buf.data_ptr(), 2, 2, 2, 0.0, None, s) != 0
    assert L.scorp_marching_cubes_emit_vertices(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 2, 2, 2, 0.0, out.data_ptr(),
                                                buf.data_ptr(), 2 ** 31, buf.data_ptr(), s) != 0
    assert L.scorp_marching_cubes_emit_faces(buf.data_ptr(), 2, 2, 2, 0.0, out.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0,
                                             buf.data_ptr(), s) != 0
    torch.cuda.synchronize()
