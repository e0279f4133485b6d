"""The bodies of the mesh-smooth tests that run on either device: tests/test_mesh_smooth_cpu.py runs them on the numpy form,
tests/test_mesh_smooth_gpu.py on csrc/mesh_smooth.hip.  Every comparison with the yardstick (tests/mesh_smooth_reference.py)
is of float32 BITS: nothing is left out and there is no tolerance."""
import numpy as np
import torch

from tests import mesh_smooth_fixtures as fx


def _same_bits(got, want, what):
    g, w = fx.bits(got), fx.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    differ = g != w
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values differ, the first at {np.argwhere(differ)[0].tolist()}"


def check_adjacency(name, dev):
    from scorp_amd.mesh import mesh_adjacency
    verts, faces = fx.fixture(name)
    near, corners, boundary = fx.expected_adjacency(name)
    adj = mesh_adjacency(fx.mesh_of(name, dev))
    assert (adj.num_vertices, adj.num_faces) == (len(verts), len(faces))
    for t in (adj.neighbor_offsets, adj.neighbors, adj.corner_offsets, adj.corner_faces):
        assert t.dtype == torch.int32 and t.device.type == dev and t.is_contiguous()
    no, nb, co, cf = (t.cpu().numpy() for t in (adj.neighbor_offsets, adj.neighbors, adj.corner_offsets, adj.corner_faces))
    assert len(no) == len(co) == len(verts) + 1 and len(cf) == 3 * len(faces) and no[0] == 0 == co[0]
    assert [nb[no[v]:no[v + 1]].tolist() for v in range(len(verts))] == near
    assert [cf[co[v]:co[v + 1]].tolist() for v in range(len(verts))] == corners
    assert adj.boundary.dtype == torch.bool and adj.boundary.cpu().tolist() == boundary
    return adj


def check_normals(name, dev, adjacency=None):
    from scorp_amd.mesh import face_normals, vertex_normals
    mesh = fx.mesh_of(name, dev)
    for normalized in (True, False):
        _same_bits(face_normals(mesh, normalized), fx.expected_face_normals(name, normalized), f"{name}: face_normals({normalized})")
    for weighting in fx.WEIGHTINGS:
        got = vertex_normals(mesh, weighting, adjacency=adjacency)
        assert got.device.type == dev
        _same_bits(got, fx.expected_normals(name, weighting), f"{name}: vertex_normals({weighting})")


def smooth(name, dev, kind, iterations, weights, fix_boundary, adjacency=None):
    from scorp_amd.mesh import filter_smooth_laplacian, filter_smooth_taubin
    mesh = fx.mesh_of(name, dev)
    if kind == "laplacian":
        out = filter_smooth_laplacian(mesh, iterations, fx.LAMBDA, weights=weights, fix_boundary=fix_boundary, adjacency=adjacency)
    else:
        out = filter_smooth_taubin(mesh, iterations, fx.LAMBDA, fx.MU, weights=weights, fix_boundary=fix_boundary, adjacency=adjacency)
    assert out.faces is mesh.faces and out.colors is mesh.colors and out.vertices is not mesh.vertices
    assert out.vertices.device.type == dev and out.vertices.dtype == torch.float32
    return out.vertices


def filter_cases():
    for weights in fx.WEIGHTS:
        for fix_boundary in (False, True):
            for kind, counts in (("laplacian", fx.LAPLACIAN_ITERATIONS), ("taubin", fx.TAUBIN_ITERATIONS)):
                for n in counts:
                    yield kind, n, weights, fix_boundary


def check_filters(name, dev, adjacency=None, against=None):
    """every filter case against the yardstick and, with `against` (another device), against that device's form too"""
    for kind, n, weights, fix_boundary in filter_cases():
        what = f"{name}: {kind} x {n}, {weights}, fix_boundary={fix_boundary}"
        got = smooth(name, dev, kind, n, weights, fix_boundary, adjacency)
        _same_bits(got, fx.expected_smooth(name, kind, n, weights, fix_boundary), what + " against the yardstick")
        if against is not None:
            _same_bits(got, smooth(name, against, kind, n, weights, fix_boundary), what + f" against the {against} form")


def check_planar_normal_map(dev):
    """The grid fixture put where pixel_camera sees it: vertex (i, j) on pixel (4 i, 4 j) at depth 1, so n = (0, 0, 16) for
    every face and the corners' normals mix to (0, 0, b_0 + b_1 + b_2), whose unit form is 1 exactly.  Every covered pixel is
    (0, 0, 1) as a VALUE - rule 5 divides the cross product by its length, and the upper triangle of each cell has
    n_y = 0 (-4) - 0 0 = -0, which stays -0 in the flat map - and every empty pixel is +0 in its bits."""
    from scorp_amd.mesh import Mesh, normal_map, render_mesh, vertex_normals
    from tests.mesh_render_fixtures import SMALL, pixel_camera
    H, W = SMALL
    verts, faces = fx.fixture("grid")
    v = torch.from_numpy(verts * np.array([32.0, 32.0, 0.0], np.float32) + np.array([0.0, 0.0, 1.0], np.float32)).to(dev)
    mesh = Mesh(v.contiguous(), torch.from_numpy(faces.copy()).to(dev), torch.zeros(len(verts), 3, device=dev))
    out = render_mesh(mesh, torch.from_numpy(pixel_camera(H, W)).to(dev), H, W, colors=False, barycentric=True)
    covered = (out.face >= 0)[:, None].expand(1, 3, H, W).cpu().numpy()
    assert int((out.face >= 0).sum()) == 32 * 32
    want = np.zeros((1, 3, H, W), np.float32)
    want[:, 2] = 1.0
    want[~covered] = 0.0
    for normals in (None, vertex_normals(mesh)):
        what = "flat" if normals is None else "interpolated"
        got = normal_map(out, mesh, normals).cpu().numpy()
        assert np.array_equal(got, want), what
        assert not fx.bits(got)[~covered].any(), what + ": +0 where there is no face"


def check_zero_iterations(dev):
    from scorp_amd.mesh import filter_smooth_laplacian, filter_smooth_taubin
    mesh = fx.mesh_of("noisy_sphere", dev)
    for out in (filter_smooth_laplacian(mesh, 0), filter_smooth_taubin(mesh, 0, fix_boundary=True, weights="inverse_distance")):
        assert out.vertices is not mesh.vertices and out.faces is mesh.faces and out.colors is mesh.colors
        _same_bits(out.vertices, mesh.vertices, "zero iterations")
