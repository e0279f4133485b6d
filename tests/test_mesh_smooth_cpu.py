"""scorp_amd/mesh/smooth.py without a GPU: the numpy form against the yardstick (tests/mesh_smooth_reference.py) bit for bit on
every fixture, the facts that are exact on the planar grid, a derived bound on the vertex normals of a sphere, what the two
filters do to a noisy sphere relative to each other, the arguments that are refused, normals in the mesh PLY, and the
package's re-exports.

Measured here (printed by the tests): icosphere(3), area weighting - the vertex normals lie 0.68 degrees from the radial
direction at most, and at least 4.4 degrees inside the bound (the largest angle between the radial direction and an
incident face normal).  Noisy sphere, ten iterations, uniform weights: radius mean / std 0.9996 / 0.0299 of the input,
0.9445 / 0.0065 after Laplacian, 1.0026 / 0.0118 after Taubin."""
import importlib

import numpy as np
import pytest
import torch

from tests import mesh_smooth_checks as checks
from tests import mesh_smooth_fixtures as fx


@pytest.mark.parametrize("name", fx.FIXTURES)
def test_numpy_form_equals_the_yardstick_bit_for_bit(name):
    adj = checks.check_adjacency(name, "cpu")
    checks.check_normals(name, "cpu")
    checks.check_normals(name, "cpu", adjacency=adj)
    checks.check_filters(name, "cpu", adjacency=adj)


def test_a_filter_builds_the_adjacency_it_is_not_given():
    for kind, n in (("laplacian", 2), ("taubin", 1)):
        got = checks.smooth("grid_non_manifold", "cpu", kind, n, "inverse_distance", True)
        assert np.array_equal(fx.bits(got), fx.bits(fx.expected_smooth("grid_non_manifold", kind, n, "inverse_distance", True)))


def test_the_planar_grid_is_exact():
    """coordinates in eighths: six neighbours that sum to 6 p, so s / W = p and an interior vertex does not move; n =
    (0, 0, 1 / 64) for every face, so every vertex normal is (0, 0, 1) exactly"""
    from scorp_amd.mesh import filter_smooth_laplacian, mesh_adjacency, vertex_normals
    mesh = fx.mesh_of("grid", "cpu")
    adj = mesh_adjacency(mesh)
    n = fx.GRID_SIDE
    interior = np.array([0 < i < n - 1 and 0 < j < n - 1 for j in range(n) for i in range(n)])
    assert np.array_equal(adj.boundary.numpy(), ~interior)
    assert set(np.diff(adj.neighbor_offsets.numpy())[interior].tolist()) == {6}
    moved = filter_smooth_laplacian(mesh, 1, 0.5, adjacency=adj).vertices
    assert np.array_equal(fx.bits(moved)[interior], fx.bits(mesh.vertices)[interior])
    assert not np.array_equal(fx.bits(moved)[~interior], fx.bits(mesh.vertices)[~interior]), "the rim shrinks"
    for weights in fx.WEIGHTS:
        kept = filter_smooth_laplacian(mesh, 3, 0.5, weights=weights, fix_boundary=True, adjacency=adj).vertices
        assert np.array_equal(fx.bits(kept), fx.bits(mesh.vertices)), weights
    want = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (n * n, 1))
    for weighting in fx.WEIGHTINGS:
        assert np.array_equal(fx.bits(vertex_normals(mesh, weighting, adjacency=adj)), fx.bits(want)), weighting


def test_sphere_vertex_normals_lie_within_their_faces_normals():
    """An area-weighted vertex normal is a positive combination of the incident face normals.  Each of those lies within
    theta_v < 90 degrees of the radial direction r_v (theta_v: the largest of their angles to r_v), and the directions within
    theta_v of r_v form a convex cone, so the vertex normal lies within theta_v of r_v too.  The rounding of the normal to
    float32 moves it by 1e-5 degrees at most, far below the 4.4 degrees the bound has to spare."""
    from scorp_amd.mesh import face_normals, mesh_adjacency, vertex_normals
    mesh = fx.mesh_of("icosphere3", "cpu")
    adj = mesh_adjacency(mesh)
    v = mesh.vertices.numpy().astype(np.float64)
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    angle = lambda a, b: np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))
    fn = face_normals(mesh).numpy().astype(np.float64)
    co, cf = adj.corner_offsets.numpy(), adj.corner_faces.numpy()
    bound = np.array([angle(fn[cf[co[k]:co[k + 1]]], radial[k]).max() for k in range(len(v))])
    assert bound.max() < 90.0
    got = angle(vertex_normals(mesh, "area", adjacency=adj).numpy().astype(np.float64), radial)
    print(f"icosphere(3): vertex normals {got.max():.3g} degrees from the radial direction at most, bound {bound.min():.3g} .. {bound.max():.3g}, "
          f"at least {(bound - got).min():.3g} inside it")
    assert (got <= bound).all()


def _radius(vertices):
    r = np.linalg.norm(vertices.numpy().astype(np.float64), axis=1)
    return r.mean(), r.std()


@pytest.mark.parametrize("weights", fx.WEIGHTS)
def test_both_filters_smooth_a_noisy_sphere_and_taubin_keeps_its_size(weights):
    from scorp_amd.mesh import filter_smooth_laplacian, filter_smooth_taubin, mesh_adjacency
    mesh = fx.mesh_of("noisy_sphere", "cpu")
    adj = mesh_adjacency(mesh)
    mean0, std0 = _radius(mesh.vertices)
    mean_l, std_l = _radius(filter_smooth_laplacian(mesh, 10, weights=weights, adjacency=adj).vertices)
    mean_t, std_t = _radius(filter_smooth_taubin(mesh, 10, weights=weights, adjacency=adj).vertices)
    print(f"{weights}: radius mean / std {mean0:.4f} / {std0:.4f} of the input, {mean_l:.4f} / {std_l:.4f} after Laplacian x 10, "
          f"{mean_t:.4f} / {std_t:.4f} after Taubin x 10")
    assert std_l < std0 and std_t < std0
    assert abs(mean_t - mean0) < abs(mean_l - mean0)


def test_zero_iterations_return_the_inputs_bits():
    checks.check_zero_iterations("cpu")


def test_meshes_without_faces_or_vertices():
    from scorp_amd.mesh import Mesh, empty_mesh, face_normals, filter_smooth_taubin, mesh_adjacency, vertex_normals
    points = Mesh(torch.rand(5, 3), torch.empty(0, 3, dtype=torch.int32), torch.zeros(5, 3))
    adj = mesh_adjacency(points)
    assert adj.neighbor_offsets.tolist() == [0] * 6 == adj.corner_offsets.tolist() and adj.neighbors.numel() == 0 == adj.corner_faces.numel()
    assert not adj.boundary.any()
    assert torch.equal(filter_smooth_taubin(points, 3).vertices, points.vertices)
    assert vertex_normals(points).tolist() == [[0.0] * 3] * 5 and tuple(face_normals(points).shape) == (0, 3)
    none = empty_mesh(torch.device("cpu"))
    assert tuple(filter_smooth_taubin(none, 3).vertices.shape) == (0, 3) == tuple(vertex_normals(none).shape)


def test_arguments_that_are_refused():
    from scorp_amd.mesh import (Mesh, MeshRender, filter_smooth_laplacian, filter_smooth_taubin, mesh_adjacency, normal_difference,
                                normal_map, vertex_normals)
    mesh = fx.mesh_of("tetrahedron", "cpu")
    with pytest.raises(ValueError, match="number_of_iterations"):
        filter_smooth_laplacian(mesh, -1)
    with pytest.raises(ValueError, match="number_of_iterations"):
        filter_smooth_taubin(mesh, 1.5)
    with pytest.raises(ValueError, match="lambda_filter must be finite"):
        filter_smooth_laplacian(mesh, 1, float("nan"))
    with pytest.raises(ValueError, match="mu must be finite"):
        filter_smooth_taubin(mesh, 1, 0.5, float("inf"))
    with pytest.raises(ValueError, match="weights must be one of"):
        filter_smooth_laplacian(mesh, 1, weights="cotangent")
    with pytest.raises(ValueError, match="weighting must be one of"):
        vertex_normals(mesh, "angle")
    other = mesh_adjacency(fx.mesh_of("triangle", "cpu"))
    for call in (lambda: filter_smooth_laplacian(mesh, 1, adjacency=other), lambda: filter_smooth_taubin(mesh, 1, adjacency=other),
                 lambda: vertex_normals(mesh, adjacency=other)):
        with pytest.raises(ValueError, match="the adjacency is of a mesh with 3 vertices and 1 faces"):
            call()
    bad = mesh.vertices.clone()
    bad[2, 1] = float("nan")
    for call in (lambda m: filter_smooth_laplacian(m), lambda m: filter_smooth_taubin(m, 0), mesh_adjacency, vertex_normals):
        with pytest.raises(ValueError, match="not all finite"):
            call(Mesh(bad, mesh.faces, mesh.colors))
    with pytest.raises(ValueError, match="vertex index 4 with 4 vertices"):
        filter_smooth_laplacian(Mesh(mesh.vertices, torch.tensor([[0, 1, 4]], dtype=torch.int32), mesh.colors))
    render = MeshRender(torch.zeros(1, 4, 5), torch.zeros(1, 4, 5, dtype=torch.int32), None, None)
    with pytest.raises(ValueError, match="render.barycentric"):
        normal_map(render, mesh, normals=vertex_normals(mesh))
    with pytest.raises(ValueError, match=r"normals must be \[4, 3\]"):
        normal_map(render, mesh, normals=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="of another mesh"):
        normal_map(MeshRender(render.depth, render.face + 4, None, None), mesh)
    with pytest.raises(ValueError, match="two normal stacks"):
        normal_difference(torch.zeros(1, 3, 4, 5), torch.zeros(1, 3, 5, 4))


def test_normal_map_of_a_hand_made_render():
    """face and barycentric maps written by hand: the flat and the interpolated value of each pixel against the yardstick"""
    from scorp_amd.mesh import MeshRender, normal_map, vertex_normals
    from tests import mesh_smooth_reference as ref
    verts, faces = fx.fixture("icosphere2")
    mesh = fx.mesh_of("icosphere2", "cpu")
    rng = np.random.default_rng(9)
    face = rng.integers(0, len(faces), (2, 7, 5)).astype(np.int32)
    face[0, 0, 0] = face[1, 3, 2] = face[1, 6, 4] = -1
    bary = rng.dirichlet((1.0, 1.0, 1.0), (2, 7, 5)).astype(np.float32).transpose(0, 3, 1, 2).copy()
    render = MeshRender(torch.zeros(2, 7, 5), torch.from_numpy(face), None, torch.from_numpy(bary))
    normals = vertex_normals(mesh)
    flat, smooth = normal_map(render, mesh), normal_map(render, mesh, normals)
    assert np.array_equal(fx.bits(flat), fx.bits(ref.normal_map(verts, faces, None, face, bary)))
    assert np.array_equal(fx.bits(smooth), fx.bits(ref.normal_map(verts, faces, normals.numpy(), face, bary)))
    empty = torch.from_numpy(face < 0)[:, None].expand(2, 3, 7, 5)
    assert empty.any() and not fx.bits(flat)[empty.numpy()].any() and not fx.bits(smooth)[empty.numpy()].any(), "+0 where there is no face"


def test_normal_map_of_the_planar_grid_is_exact():
    checks.check_planar_normal_map("cpu")


def test_normal_difference_of_known_angles():
    from scorp_amd.mesh import normal_difference
    z = torch.zeros(2, 3, 2, 3)
    m, r = z.clone(), z.clone()
    m[:, 2] = 1.0                                   # the mesh: +z everywhere ...
    m[1, :, 1, 2] = 0.0                             # ... but one pixel of view 1
    r[0, 2] = 0.25                                  # view 0: the reference parallel (and short: alpha-weighted) -> 0 degrees
    r[0, :, 0, 0] = 0.0                             # (one pixel without a reference)
    r[1, 0] = 0.5                                   # view 1: the reference along +x -> 90 degrees
    r[1, :, 0, 0] = torch.tensor([0.0, 0.3, 0.3])   # one pixel at 45 degrees
    d = normal_difference(m, r)
    assert d.mean_deg.dtype == torch.float64 and d.median_deg.dtype == torch.float64
    assert d.mean_deg.tolist() == pytest.approx([0.0, (4 * 90.0 + 45.0) / 5], abs=1e-9)
    assert d.median_deg.tolist() == pytest.approx([0.0, 90.0], abs=1e-9)
    assert d.reference_covered.tolist() == pytest.approx([1.0, 5 / 6]) and d.mesh_covered.tolist() == pytest.approx([5 / 6, 1.0])
    assert d.overall["mean_deg"] == pytest.approx((4 * 90.0 + 45.0) / 10, abs=1e-9) and d.overall["median_deg"] == pytest.approx(0.0, abs=1e-9)
    assert d.overall["reference_covered"] == pytest.approx(10 / 11) and d.overall["mesh_covered"] == pytest.approx(10 / 11)
    nothing = normal_difference(z, z)
    assert np.isnan(nothing.overall["mean_deg"]) and torch.isnan(nothing.mean_deg).all() and torch.isnan(nothing.median_deg).all()


def test_mesh_ply_with_and_without_normals(tmp_path):
    from scorp_amd.mesh import vertex_normals
    from scorp_amd.ply import read_mesh_ply, read_ply_vertices, write_mesh_ply
    mesh = fx.mesh_of("tetrahedron", "cpu")
    mesh.colors[:] = torch.tensor([[0.0, 0.5, 1.0], [0.2, 0.4, 0.6], [1.0, 1.0, 1.0], [0.1, 0.9, 0.3]])
    normals = vertex_normals(mesh)
    old, none, with_normals = (str(tmp_path / n) for n in ("old.ply", "none.ply", "normals.ply"))
    write_mesh_ply(old, mesh)
    write_mesh_ply(none, mesh, normals=None)
    write_mesh_ply(with_normals, mesh, normals=normals)
    v = np.empty(4, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, nm in enumerate("xyz"):
        v[nm] = mesh.vertices.numpy()[:, k]
    for k, nm in enumerate(("red", "green", "blue")):
        v[nm] = np.rint(mesh.colors.numpy().astype(np.float64)[:, k] * 255.0)
    f = np.empty(4, dtype=[("n", "u1"), ("i", "<i4", (3,))])
    f["n"], f["i"] = 3, mesh.faces.numpy()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n")
    layout_before_normals = header.encode("ascii") + v.tobytes() + f.tobytes()
    assert open(old, "rb").read() == layout_before_normals == open(none, "rb").read()
    a, b = read_mesh_ply(old), read_mesh_ply(with_normals)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(a[0], mesh.vertices.numpy()) and np.array_equal(a[1], mesh.faces.numpy())
    stored = read_ply_vertices(with_normals)
    assert stored.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([stored["nx"], stored["ny"], stored["nz"]], 1), normals.numpy())
    with pytest.raises(ValueError, match=r"normals must be \[4, 3\]"):
        write_mesh_ply(str(tmp_path / "bad.ply"), mesh, normals=normals[:3])


NAMES = ["MeshAdjacency", "NormalDifference", "mesh_adjacency", "face_normals", "vertex_normals", "filter_smooth_laplacian",
         "filter_smooth_taubin", "normal_map", "normal_difference", "WEIGHTINGS", "SMOOTH_WEIGHTS", "DISTANCE_EPS", "MAX_SMOOTH_STEPS"]


def test_the_package_re_exports_the_new_names_from_their_home():
    package, module = importlib.import_module("scorp_amd.mesh"), importlib.import_module("scorp_amd.mesh.smooth")
    for name in NAMES:
        assert getattr(package, name) is getattr(module, name), name
        if callable(getattr(module, name)):
            assert getattr(module, name).__module__ == module.__name__, name
    from scorp_amd.mesh import GaussianExtractor
    import inspect
    assert inspect.signature(GaussianExtractor.reconstruction).parameters["keep_normals"].default is False
    assert hasattr(GaussianExtractor, "normal_difference")
    from scorp_amd.ply import write_mesh_ply
    assert inspect.signature(write_mesh_ply).parameters["normals"].default is None
