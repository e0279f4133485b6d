"""The vertex-clustering kernels (csrc/mesh_simplify.hip) through scorp_amd.mesh on CUDA tensors against the plain-Python
yardstick of tests/mesh_simplify_reference.py, on every mesh there and in both placements.  vertex_cell, the cell count and
the faces must be EQUAL: both hash tables resolve their slots by atomic min on an index, so the integers do not depend on the
order the lanes run in.  Positions and colours must lie within one float32 ulp, 2^-23 max(|ref|, |out|) per component: the
float64 sums differ only in their order (count x 2^-52 relative), the solve amplifies that by at most 1 / 1e-3, and the
results then round to the same or the adjacent float32.  Cells with a decision of rule 4 near its threshold (at most 1 % of
a mesh's) are left out of the position comparison only."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_cluster_reference as cluster_ref
from tests import mesh_simplify_reference as ref

pytestmark = pytest.mark.gpu

NAMES = ref.MESHES + tuple(ref.SPHERES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(vertices, colours, faces, h) as numpy arrays; `spheres` comes from extract_surface on the GPU"""
    if name in ref.SPHERES:
        from scorp_amd.mesh import extract_surface
        grid, coords = cluster_ref.three_spheres()
        d = torch.device("cuda:0")
        v, f = extract_surface(torch.from_numpy(grid).to(d), [torch.from_numpy(c).to(d) for c in coords])
        return v.cpu().numpy(), ref.vertex_colors(v.shape[0]), f.cpu().numpy(), ref.spheres_voxel_size(name)
    return ref.mesh(name)


@functools.lru_cache(maxsize=None)
def expected(name, contraction):
    return ref.simplify(*_mesh(name), contraction)


def _run(dev, name, contraction):
    from scorp_amd.mesh import Mesh, cluster_vertices
    v, c, f, h = _mesh(name)
    vertex_cell, out = cluster_vertices(Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(c).to(dev)), h, contraction)
    torch.cuda.synchronize()
    return vertex_cell, out


@pytest.mark.parametrize("contraction", ref.CONTRACTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_kernels_match_the_yardstick(dev, name, contraction):
    vertex_cell, out = _run(dev, name, contraction)
    r = expected(name, contraction)
    C = len(r["positions"])
    assert vertex_cell.is_cuda and vertex_cell.dtype == torch.int32
    assert np.array_equal(vertex_cell.cpu().numpy(), r["vertex_cell"])
    assert tuple(out.vertices.shape) == (C, 3) and tuple(out.colors.shape) == (C, 3)
    assert np.array_equal(out.faces.cpu().numpy(), r["faces"])
    compared = ~r["near"]
    assert r["near"].sum() <= ref.MAX_NEAR_FRACTION * C
    err_c = ref.ulp_error(out.colors.cpu().numpy(), r["colors"])
    got = out.vertices.cpu().numpy()
    err_p = ref.ulp_error(got[compared], r["positions"][compared])
    print(f"{name} {contraction}: {len(r['vertex_cell'])} / {len(_mesh(name)[2])} -> {C} / {len(r['faces'])}, {int(r['near'].sum())} cells "
          f"left out, {int(r['clamped'].sum())} clamped, worst position error {err_p:.3f} ulp, worst colour error {err_c:.3f} ulp")
    for c, k in ref.misses(got, r["positions"], compared)[:8]:
        print(f"    cell {c} axis {k}: {got[c, k]!r} against {r['positions'][c, k]!r} ({int((r['vertex_cell'] == c).sum())} members, rank {r['rank'][c]})")
    assert err_c <= 1.0
    assert err_p <= 1.0


def test_counts_of_the_real_producers_mesh(dev):
    v, _, f, _ = _mesh("spheres_2.5")
    assert (len(v), len(f)) == (2372, 4732)


@pytest.mark.parametrize("name", ("scattered", "spheres_2.5", "one_cell"))
def test_integer_outputs_are_deterministic(dev, name):
    (ca, a), (cb, b) = _run(dev, name, "quadric"), _run(dev, name, "quadric")
    assert torch.equal(ca, cb) and torch.equal(a.faces, b.faces) and a.vertices.shape == b.vertices.shape


@pytest.mark.parametrize("drop", (True, False))
def test_simplify_returns_a_mesh_on_the_device(dev, drop):
    from scorp_amd.mesh import Mesh, simplify_vertex_clustering
    v, c, f, h = _mesh("cube16")
    out = simplify_vertex_clustering(Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(c).to(dev)), h, "quadric",
                                     drop_unreferenced=drop)
    assert out.vertices.device == dev and out.faces.device == dev and out.colors.device == dev
    assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32
    r = expected("cube16", "quadric")
    rv, rc, rf = ref.drop_unreferenced(r["positions"], r["colors"], r["faces"]) if drop else (r["positions"], r["colors"], r["faces"])
    assert np.array_equal(out.faces.cpu().numpy(), rf) and out.vertices.shape[0] == len(rv)
    assert ref.ulp_error(out.vertices.cpu().numpy(), rv) <= 1.0 and ref.ulp_error(out.colors.cpu().numpy(), rc) <= 1.0


def test_unreferenced_cells_are_dropped(dev):
    from scorp_amd.mesh import Mesh, simplify_vertex_clustering
    v, c, f, h = _mesh("zero_area")   # the cell of the three collinear vertices loses all its faces
    mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(c).to(dev))
    full, cut = simplify_vertex_clustering(mesh, h, drop_unreferenced=False), simplify_vertex_clustering(mesh, h)
    r = expected("zero_area", "average")
    rv, rc, rf = ref.drop_unreferenced(r["positions"], r["colors"], r["faces"])
    assert full.vertices.shape[0] == len(r["positions"]) == len(rv) + 1
    assert np.array_equal(cut.faces.cpu().numpy(), rf) and ref.ulp_error(cut.vertices.cpu().numpy(), rv) <= 1.0
    assert torch.unique(cut.faces).numel() == cut.vertices.shape[0]


def test_empty_does_not_call_the_library(dev, monkeypatch):
    from scorp_amd import _C
    from scorp_amd.mesh import Mesh, simplify_vertex_clustering

    def no_library():
        raise AssertionError("the library was called for an empty mesh")
    monkeypatch.setattr(_C, "lib", no_library)
    for nv in (0, 5):
        out = simplify_vertex_clustering(Mesh(torch.rand(nv, 3, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                                              torch.rand(nv, 3, device=dev)), 0.1)
        assert out.vertices.is_cuda and tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3)
        assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32


def test_entry_points_refuse_bad_arguments(dev):
    from scorp_amd import _C
    L = _C.lib()
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    d = buf.data_ptr()
    for args, text in (((d, 100, d, 0.1, d, d, 100, d, d, None), b"power of two"), ((d, 513, d, 0.1, d, d, 1024, d, d, None), b"at least 2 num_vertices"),
                       ((d, 100, d, 0.0, d, d, 256, d, d, None), b"voxel_size"), ((None, 100, d, 0.1, d, d, 256, d, d, None), b"NULL")):
        assert L.scorp_mesh_simplify_cells(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    assert L.scorp_mesh_simplify_faces(d, 513, d, 100, d, 1024, d, d, None) == _C.ERR_INVALID and b"at least 2 num_faces" in L.scorp_last_error()
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0   # nothing was launched
