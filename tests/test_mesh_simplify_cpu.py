"""The numpy form of the vertex clustering (scorp_amd.mesh.simplify_vertex_clustering / cluster_vertices on CPU tensors)
against the plain-Python yardstick of tests/mesh_simplify_reference.py on every mesh there, in both placements: vertex_cell,
the cell count and the faces equal, positions and colours within one float32 ulp (the GPU test's bound) outside the cells a
decision of rule 4 leaves near its threshold.  Then the properties the rules promise, the argument checks and the empty
mesh.  No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_cluster_reference as cluster_ref
from tests import mesh_simplify_reference as ref

NAMES = ref.MESHES + tuple(ref.SPHERES)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name in ref.SPHERES:
        from scorp_amd.mesh import extract_surface
        grid, coords = cluster_ref.three_spheres()
        v, f = extract_surface(torch.from_numpy(grid), [torch.from_numpy(c) for c in coords])
        return v.numpy(), ref.vertex_colors(v.shape[0]), f.numpy(), ref.spheres_voxel_size(name)
    return ref.mesh(name)


@functools.lru_cache(maxsize=None)
def expected(name, contraction):
    return ref.simplify(*_mesh(name), contraction)


def _as_mesh(v, c, f):
    from scorp_amd.mesh import Mesh
    return Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))


@functools.lru_cache(maxsize=None)
def _run(name, contraction):
    from scorp_amd.mesh import cluster_vertices
    v, c, f, h = _mesh(name)
    return cluster_vertices(_as_mesh(v, c, f), h, contraction)


@pytest.mark.parametrize("contraction", ref.CONTRACTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_cpu_form_matches_the_yardstick(name, contraction):
    vertex_cell, out = _run(name, contraction)
    r = expected(name, contraction)
    C = len(r["positions"])
    assert vertex_cell.dtype == torch.int32 and np.array_equal(vertex_cell.numpy(), r["vertex_cell"])
    assert tuple(out.vertices.shape) == (C, 3) and tuple(out.colors.shape) == (C, 3)
    assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32
    assert np.array_equal(out.faces.numpy(), r["faces"])
    compared = ~r["near"]
    assert r["near"].sum() <= ref.MAX_NEAR_FRACTION * C
    err_c = ref.ulp_error(out.colors.numpy(), r["colors"])
    err_p = ref.ulp_error(out.vertices.numpy()[compared], r["positions"][compared])
    print(f"{name} {contraction}: {len(r['vertex_cell'])} / {len(_mesh(name)[2])} -> {C} / {len(r['faces'])}, {int(r['near'].sum())} cells "
          f"left out, {int(r['clamped'].sum())} clamped, worst position error {err_p:.3f} ulp, worst colour error {err_c:.3f} ulp")
    assert err_c <= 1.0
    assert err_p <= 1.0


def test_the_counts_the_rules_give():
    """what a numpy prototype of the rules gave before anything here was written"""
    got = {name: (len(expected(name, "quadric")["positions"]), len(expected(name, "quadric")["faces"]))
           for name in ("cube16", "cube32", "spheres_2.5", "spheres_4")}
    assert got == {"cube16": (98, 192), "cube32": (218, 432), "spheres_2.5": (327, 650), "spheres_4": (133, 263)}
    assert np.bincount(expected("cube16", "quadric")["rank"], minlength=4).tolist() == [0, 54, 36, 8]   # faces, edges, corners
    assert (len(_mesh("spheres_4")[0]), len(_mesh("spheres_4")[2])) == (2372, 4732)
    for name in ("uv_sphere", "cube16", "cube32", "spheres_2.5", "spheres_4"):
        r = expected(name, "quadric")
        assert not r["near"].any() and not r["clamped"].any(), name
    r = expected("one_cell", "quadric")
    assert len(r["positions"]) == 1 and len(r["faces"]) == 0


@pytest.mark.parametrize("name", ("cube16", "cube32"))
def test_quadric_keeps_the_cube(name):
    q = float(ref.cube_distance(_run(name, "quadric")[1].vertices.numpy()).max())
    a = float(ref.cube_distance(_run(name, "average")[1].vertices.numpy()).max())
    print(f"{name}: worst distance to the cube's surface {q:.3e} (quadric), {a:.3e} (average)")
    assert q <= 1e-6     # creases and corners stay where they are, up to the float32 rounding of the inputs
    assert a > 1e-2      # the mean of an edge or corner cell lies inside the cube


@pytest.mark.parametrize("contraction", ref.CONTRACTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_faces_are_distinct_rotated_and_unique(name, contraction):
    f = _run(name, contraction)[1].faces.numpy()
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])).all()
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()
    assert len(np.unique(f, axis=0)) == len(f)
    assert (f >= 0).all() and (f.size == 0 or f.max() < _run(name, contraction)[1].vertices.shape[0])


def test_own_cells_come_back_unchanged():
    v, c, f, h = _mesh("own_cells")
    for contraction in ref.CONTRACTIONS:
        vertex_cell, out = _run("own_cells", contraction)
        assert np.array_equal(vertex_cell.numpy(), np.arange(len(v)))
        assert np.array_equal(out.vertices.numpy(), v) and np.array_equal(out.colors.numpy(), c)
        kept = expected("own_cells", contraction)["kept"]
        assert len(kept) == len(f) - 5                       # two copies, one rotated copy and two degenerate faces go
        assert len(f) - 3 in kept                            # the face of the opposite orientation stays
        rotated = np.sort(out.faces.numpy(), 1)
        assert np.array_equal(rotated, np.sort(f[kept], 1))  # the survivors are the input faces, rotated


def test_two_sheets_clamp_to_the_mean():
    r = expected("two_sheets", "quadric")
    assert r["clamped"].any() and not r["near"].any()
    out = _run("two_sheets", "quadric")[1].vertices.numpy()
    mean = _run("two_sheets", "average")[1].vertices.numpy()
    assert np.array_equal(out[r["clamped"]], mean[r["clamped"]])


def test_zero_area_cell_takes_the_mean():
    r = expected("zero_area", "quadric")
    cell = int(r["vertex_cell"][0])
    assert r["rank"][cell] == 0 and (r["vertex_cell"][:3] == cell).all()
    assert np.array_equal(_run("zero_area", "quadric")[1].vertices.numpy()[cell], _run("zero_area", "average")[1].vertices.numpy()[cell])


def test_on_faces_belong_to_the_upper_cell():
    v, _, _, h = _mesh("on_faces")
    r = expected("on_faces", "average")
    origin = v.min(0).astype(np.float64) - 0.5 * h
    q = (v.astype(np.float64) - origin) / h
    on = (q == np.round(q)).all(1)
    assert on.sum() >= 100
    below = np.nextafter(v[on], np.float32(-np.inf))
    lattice = {tuple(p): int(c) for p, c in zip(v.tolist(), r["vertex_cell"])}
    shared = [lattice[tuple(b)] != lattice[tuple(p)] for p, b in zip(v[on].tolist(), below.tolist()) if tuple(b) in lattice]
    assert len(shared) >= 50 and all(shared)   # the last float32 below a cell face lies in another cell than the face itself


@pytest.mark.parametrize("name", ("cube16", "zero_area", "one_cell"))
def test_drop_unreferenced(name):
    from scorp_amd.mesh import simplify_vertex_clustering
    v, c, f, h = _mesh(name)
    r = expected(name, "average")
    full = simplify_vertex_clustering(_as_mesh(v, c, f), h, drop_unreferenced=False)
    cut = simplify_vertex_clustering(_as_mesh(v, c, f), h)
    assert np.array_equal(full.vertices.numpy(), r["positions"]) and np.array_equal(full.faces.numpy(), r["faces"])
    rv, rc, rf = ref.drop_unreferenced(r["positions"], r["colors"], r["faces"])
    assert np.array_equal(cut.vertices.numpy(), rv) and np.array_equal(cut.colors.numpy(), rc) and np.array_equal(cut.faces.numpy(), rf)
    assert cut.faces.dtype == torch.int32 and torch.unique(cut.faces).numel() == cut.vertices.shape[0]
    if name == "zero_area":
        assert len(rv) == len(r["positions"]) - 1
    if name == "one_cell":
        assert cut.vertices.shape == (0, 3) and cut.faces.shape == (0, 3) and full.vertices.shape == (1, 3)


def test_bad_arguments():
    from scorp_amd.mesh import Mesh, simplify_vertex_clustering
    v, c, f, h = _mesh("zero_area")
    v, c, f = torch.from_numpy(v), torch.from_numpy(c), torch.from_numpy(f)
    for bad in (float("nan"), float("inf")):
        w = v.clone()
        w[5, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            simplify_vertex_clustering(Mesh(w, f, c), h)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            simplify_vertex_clustering(Mesh(v, f, c), bad)
    with pytest.raises(ValueError, match="contraction"):
        simplify_vertex_clustering(Mesh(v, f, c), h, contraction="median")
    with pytest.raises(ValueError, match="colours"):
        simplify_vertex_clustering(Mesh(v, f, c[:-1]), h)
    for bad in (-1, len(v)):
        g = f.clone()
        g[2, 1] = bad
        with pytest.raises(ValueError, match="vertex index"):
            simplify_vertex_clustering(Mesh(v, g, c), h)
    with pytest.raises(ValueError, match=r"extent.*voxel_size 1e-06.*2\^21"):
        simplify_vertex_clustering(Mesh(v, f, c), 1e-6)   # an extent of 2.3 at 1e-6: 2.3 million cells
    ok = simplify_vertex_clustering(Mesh(v, f, c), 2.3 / (2 ** 21 - 2))   # just inside
    assert ok.vertices.shape[0] > 0


def test_empty_does_not_load_the_library(monkeypatch):
    from scorp_amd import _C
    from scorp_amd.mesh import Mesh, cluster_vertices, simplify_vertex_clustering

    def no_library():
        raise AssertionError("the library was loaded for an empty mesh")
    monkeypatch.setattr(_C, "lib", no_library)
    for nv in (0, 5):
        mesh = Mesh(torch.rand(nv, 3), torch.empty(0, 3, dtype=torch.int32), torch.rand(nv, 3))
        out = simplify_vertex_clustering(mesh, 0.1)
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.colors.shape) == (0, 3)
        assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32
        assert cluster_vertices(mesh, 0.1)[0].shape == (0,)


def test_entry_points_refuse_bad_arguments():
    """Validation runs before any HIP call: the dummy pointers are never dereferenced and no GPU is needed."""
    from scorp_amd import _C
    L = _C.lib()
    d = 0x10000
    for args, text in (((d, 100, d, 0.1, d, d, 100, d, d, None), b"power of two"), ((d, 513, d, 0.1, d, d, 1024, d, d, None), b"at least 2 num_vertices"),
                       ((d, 100, d, 0.1, d, d, 2 ** 32, d, d, None), b"2^31"), ((d, 2 ** 30 + 1, d, 0.1, d, d, 2 ** 31, d, d, None), b"2^30"),
                       ((d, 0, d, 0.1, d, d, 256, d, d, None), b"2^30"), ((d, 100, d, 0.0, d, d, 256, d, d, None), b"voxel_size"),
                       ((d, 100, d, float("nan"), d, d, 256, d, d, None), b"voxel_size"), ((d, 100, d, float("inf"), d, d, 256, d, d, None), b"voxel_size"),
                       ((None, 100, d, 0.1, d, d, 256, d, d, None), b"NULL"), ((d, 100, None, 0.1, d, d, 256, d, d, None), b"NULL"),
                       ((d, 100, d, 0.1, None, d, 256, d, d, None), b"NULL"), ((d, 100, d, 0.1, d, None, 256, d, d, None), b"NULL"),
                       ((d, 100, d, 0.1, d, d, 256, None, d, None), b"NULL"), ((d, 100, d, 0.1, d, d, 256, d, None, None), b"NULL")):
        assert L.scorp_mesh_simplify_cells(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    for args, text in (((None, 256, d, 100, d, d, None), b"NULL"), ((d, 256, None, 100, d, d, None), b"NULL"), ((d, 256, d, 100, None, d, None), b"NULL"),
                       ((d, 256, d, 100, d, None, None), b"NULL"), ((d, 128, d, 100, d, d, None), b"at least 2 num_vertices"),
                       ((d, 256, d, 2 ** 30 + 1, d, d, None), b"2^30")):
        assert L.scorp_mesh_simplify_roots(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    good = [d, d, 100, d, 50, d, 0.1, d, d, 10, 1, d, d, d, None]
    for at, value, text in ((0, None, b"NULL"), (1, None, b"NULL"), (3, None, b"NULL"), (5, None, b"NULL"), (7, None, b"NULL"), (8, None, b"NULL"),
                            (11, None, b"NULL"), (12, None, b"NULL"), (13, None, b"NULL"), (2, 0, b"2^30"), (4, 2 ** 28 + 1, b"2^28"),
                            (4, 0, b"2^28"), (6, -0.5, b"voxel_size"), (9, 0, b"num_cells"), (9, 101, b"num_cells")):
        args = list(good)
        args[at] = value
        assert L.scorp_mesh_simplify_accumulate(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), (at, value)
    for args, text in (((None, d, 10, d, 0.1, 1, d, d, None), b"NULL"), ((d, None, 10, d, 0.1, 1, d, d, None), b"NULL"),
                       ((d, d, 10, None, 0.1, 1, d, d, None), b"NULL"), ((d, d, 10, d, 0.1, 1, None, d, None), b"NULL"),
                       ((d, d, 10, d, 0.1, 1, d, None, None), b"NULL"), ((d, d, 0, d, 0.1, 1, d, d, None), b"num_cells"),
                       ((d, d, 10, d, 0.0, 1, d, d, None), b"voxel_size")):
        assert L.scorp_mesh_simplify_place(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
    for args, text in (((None, 100, d, 50, d, 256, d, d, None), b"NULL"), ((d, 100, None, 50, d, 256, d, d, None), b"NULL"),
                       ((d, 100, d, 50, None, 256, d, d, None), b"NULL"), ((d, 100, d, 50, d, 256, None, d, None), b"NULL"),
                       ((d, 100, d, 50, d, 256, d, None, None), b"NULL"), ((d, 2 ** 28 + 1, d, 50, d, 2 ** 30, d, d, None), b"2^28"),
                       ((d, 0, d, 50, d, 256, d, d, None), b"2^28"), ((d, 100, d, 0, d, 256, d, d, None), b"2^30"),
                       ((d, 100, d, 50, d, 200, d, d, None), b"power of two"), ((d, 513, d, 50, d, 1024, d, d, None), b"at least 2 num_faces")):
        assert L.scorp_mesh_simplify_faces(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), args
