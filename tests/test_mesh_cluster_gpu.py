"""The triangle-clustering kernels (csrc/mesh_cluster.hip) against the breadth-first search of
tests/mesh_cluster_reference.py.  triangle_clusters and cluster_n_triangles must be EQUAL: a root is only hooked under a
smaller index, so the numbering does not depend on the order the lanes run in.  cluster_area must lie within
F 2^-52 (total area) per cluster, the bound for F float64 additions in any order (the per-triangle areas are formed
without contraction and are the yardstick's bits).  post_process_mesh on the three-sphere surface-nets mesh must equal the
numpy restatement of mesh_utils.py:35-40 exactly."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_cluster_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def spheres_mesh():
    """the real producer, with its 4-triangle edges: extract_surface on the GPU, (vertices, faces) kept on the device"""
    from scorp_amd.mesh import extract_surface
    grid, coords = ref.three_spheres()
    d = torch.device("cuda:0")
    return extract_surface(torch.from_numpy(grid).to(d), [torch.from_numpy(c).to(d) for c in coords])


def _mesh(name):
    if name == "spheres":
        v, f = spheres_mesh()
        return f.cpu().numpy(), v.cpu().numpy(), 3
    return ref.mesh(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    f, v, _ = _mesh(name)
    return ref.cluster(f, v)


def _run(dev, name):
    from scorp_amd.mesh import cluster_connected_triangles
    f, v, _ = _mesh(name)
    out = cluster_connected_triangles(torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev) if v is not None else None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ref.MESHES + ("spheres",))
def test_kernels_match_the_search(dev, name):
    f, v, clusters = _mesh(name)
    tc, n, area = _run(dev, name)
    rtc, rn, rarea = expected(name)
    assert tc.is_cuda and n.is_cuda and tc.dtype == torch.int32 and n.dtype == torch.int32
    assert len(rn) == clusters
    assert tuple(n.shape) == (clusters,) and np.array_equal(n.cpu().numpy(), rn)
    assert np.array_equal(tc.cpu().numpy(), rtc)
    if v is None:
        assert area is None
        return
    assert area.is_cuda and area.dtype == torch.float64 and tuple(area.shape) == (clusters,)
    err, bound = float(np.abs(area.cpu().numpy() - rarea).max()), len(f) * 2.0 ** -52 * float(rarea.sum())
    print(f"{name}: F = {len(f)}, {clusters} clusters, worst area error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_spheres_mesh_has_a_floater(dev):
    _, n, _ = expected("spheres")
    assert len(n) == 3 and n[1] < ref.MIN_TRIANGLES <= min(n[0], n[2])   # numbered by first triangle: the small one is second


def test_without_vertices(dev):
    from scorp_amd.mesh import cluster_connected_triangles
    f, _, _ = ref.mesh("three_strips")
    tc, n, area = cluster_connected_triangles(torch.from_numpy(f).to(dev))
    rtc, rn, _ = expected("three_strips")
    assert area is None and np.array_equal(tc.cpu().numpy(), rtc) and np.array_equal(n.cpu().numpy(), rn)


def test_empty_does_not_call_the_library(dev, monkeypatch):
    from scorp_amd import _C
    from scorp_amd.mesh import cluster_connected_triangles

    def no_library():
        raise AssertionError("the library was called for an empty mesh")
    monkeypatch.setattr(_C, "lib", no_library)
    tc, n, area = cluster_connected_triangles(torch.empty(0, 3, dtype=torch.int32, device=dev), torch.empty(0, 3, device=dev))
    assert tc.is_cuda and tuple(tc.shape) == (0,) and tuple(n.shape) == (0,) and tuple(area.shape) == (0,)
    assert tc.dtype == torch.int32 and n.dtype == torch.int32 and area.dtype == torch.float64


@pytest.mark.parametrize("name", ("chain", "spheres"))
def test_integer_outputs_are_deterministic(dev, name):
    a, b = _run(dev, name), _run(dev, name)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("keep", (1, 2, 3, 1000))
def test_post_process_spheres(dev, keep):
    from scorp_amd.mesh import Mesh, post_process_mesh
    v, f = spheres_mesh()
    col = ref.vertex_colors(v.shape[0])
    out = post_process_mesh(Mesh(v, f, torch.from_numpy(col).to(dev)), cluster_to_keep=keep)
    rv, rf, rc = ref.post_process(v.cpu().numpy(), f.cpu().numpy(), col, keep)
    assert out.vertices.is_cuda and out.faces.is_cuda and out.colors.is_cuda
    assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32
    assert np.array_equal(out.vertices.cpu().numpy(), rv)
    assert np.array_equal(out.faces.cpu().numpy(), rf)
    assert np.array_equal(out.colors.cpu().numpy(), rc)
    _, n, _ = expected("spheres")
    kept = sorted(int(x) for x in n if x >= ref.MIN_TRIANGLES)[-min(keep, 2):]
    assert out.faces.shape[0] == sum(kept)                            # the small sphere is gone at every setting
    assert torch.unique(out.faces).numel() == out.vertices.shape[0]   # every vertex is referenced


def test_entry_points_refuse_bad_arguments(dev):
    from scorp_amd import _C
    L = _C.lib()
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    d = buf.data_ptr()
    for args, text in (((d, 100, d, d, 1000, d, None), b"power of two"), ((d, 171, d, d, 1024, d, None), b"at least 6 num_faces"),
                       ((d, 2 ** 28 + 1, d, d, 2 ** 31, d, None), b"2^28"), ((None, 100, d, d, 1024, d, None), b"NULL"),
                       ((d, 100, None, d, 1024, d, None), b"NULL"), ((d, 100, d, None, 1024, d, None), b"NULL"),
                       ((d, 100, d, d, 1024, None, None), b"NULL")):
        assert L.scorp_mesh_cluster_link(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    for args, text in (((None, 10, d, d, None), b"NULL"), ((d, 10, None, d, None), b"NULL"), ((d, 10, d, None, None), b"NULL"),
                       ((d, 2 ** 28 + 1, d, d, None), b"2^28")):
        assert L.scorp_mesh_cluster_roots(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    for args, text in (((None, d, 9, d, d, 10, 2, d, d, d, None), b"NULL"), ((d, d, 9, None, d, 10, 2, d, d, d, None), b"NULL"),
                       ((d, d, 9, d, None, 10, 2, d, d, d, None), b"NULL"), ((d, d, 9, d, d, 10, 2, None, d, d, None), b"NULL"),
                       ((d, d, 9, d, d, 10, 2, d, None, d, None), b"NULL"), ((d, d, 9, d, d, 2 ** 28 + 1, 2, d, d, d, None), b"2^28")):
        assert L.scorp_mesh_cluster_stats(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0   # nothing was launched
