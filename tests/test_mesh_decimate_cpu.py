"""Edge-collapse decimation without a GPU: the properties the rules of include/scorp_gs.h promise, checked on the plain-Python
yardstick of tests/mesh_decimate_reference.py AND on scorp_amd.mesh.simplify_quadric_decimation with CPU tensors (its numpy
form of the same rules), and the two held to each other exactly: equal faces, positions and colours equal bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_decimate_reference as ref
from tests import mesh_simplify_reference as sref

# Worst | |p - centre| - 1 | over the output of uv_sphere(24) -> 300, measured on the yardstick; the cap of the test is twice
# this, against gross regressions only (the chord of a 300-triangle sphere alone sags by about 0.01)
SPHERE_DEVIATION = 0.014272


def _mesh(name, device="cpu"):
    from scorp_amd.mesh import Mesh
    v, c, f = ref.mesh(name)
    return Mesh(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device))


@functools.lru_cache(maxsize=None)
def cpu_path(case):
    from scorp_amd.mesh import simplify_quadric_decimation
    name, target, max_err, bw = ref.CASES[case]
    out = simplify_quadric_decimation(_mesh(name), target, max_err, bw)
    return {"positions": out.vertices.numpy(), "colors": out.colors.numpy(), "faces": out.faces.numpy()}


BOTH = pytest.mark.parametrize("result", (ref.expected, cpu_path), ids=("yardstick", "cpu_path"))


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_cpu_path_equals_the_yardstick(case):
    r, out = ref.expected(case), cpu_path(case)
    assert out["faces"].dtype == np.int32 and np.array_equal(out["faces"], r["faces"])
    assert ref.exact(out["positions"], r["positions"])
    assert ref.exact(out["colors"], r["colors"])


def _at_cube_corners(positions):
    off = np.abs(positions.astype(np.float64) - np.asarray(sref.CUBE_CENTRE))
    assert np.abs(off - 0.5).max() <= 1e-6
    assert len({tuple(s) for s in np.sign(positions.astype(np.float64) - np.asarray(sref.CUBE_CENTRE))}) == 8


@BOTH
def test_cube_goes_to_its_twelve_triangles(result):
    r = result("cube8")
    assert r["faces"].shape == (12, 3) and r["positions"].shape == (8, 3)
    _at_cube_corners(r["positions"])
    assert ref.is_closed_manifold(r["faces"]) and ref.euler_characteristic(r["faces"]) == 2


@BOTH
def test_maximum_error_stops_the_cube_at_its_twelve_triangles(result):
    r = result("cube8_error_cap")          # target 0, but every further collapse would cost far more than 1e-12
    assert r["faces"].shape == (12, 3) and r["positions"].shape == (8, 3)
    _at_cube_corners(r["positions"])


@BOTH
def test_scattered_cube_stays_a_closed_cube(result):
    r = result("cube16_scattered")
    assert len(r["faces"]) == 200
    assert ref.is_closed_manifold(r["faces"]) and ref.euler_characteristic(r["faces"]) == 2
    assert np.abs(sref.cube_distance(r["positions"])).max() <= 1e-6


@BOTH
def test_sphere_stays_a_closed_sphere(result):
    r = result("uv_sphere24")
    assert len(r["faces"]) == 300
    assert ref.is_closed_manifold(r["faces"]) and ref.euler_characteristic(r["faces"]) == 2
    radius = np.linalg.norm(r["positions"].astype(np.float64) - np.asarray(sref.CUBE_CENTRE), axis=1)
    worst = np.abs(radius - 1.0).max()
    print(f"worst radial deviation {worst:.6f}")
    assert worst <= 2.0 * SPHERE_DEVIATION


@BOTH
def test_flat_sheet_keeps_its_corners(result):
    r = result("flat_sheet")
    v, _, _ = ref.mesh("flat_sheet")
    assert len(r["faces"]) == 2 and len(r["positions"]) == 4
    corners = {(x, y, v[0, 2]) for x in (v[:, 0].min(), v[:, 0].max()) for y in (v[:, 1].min(), v[:, 1].max())}
    assert {tuple(p) for p in r["positions"]} == corners
    assert np.array_equal(r["positions"].min(0), v.min(0)) and np.array_equal(r["positions"].max(0), v.max(0))


@BOTH
def test_wavy_sheet_keeps_its_boundary(result):
    r = result("wavy_sheet")
    v, _, f = ref.mesh("wavy_sheet")
    assert len(r["faces"]) in (71, 72)
    rim = ref.boundary_vertices(r["faces"])
    assert rim
    worst = ref.polyline_distance(r["positions"][rim], v, f).max()
    print(f"{len(rim)} boundary vertices, worst distance to the input's boundary {worst:.3e}")
    assert worst <= 1e-6


def test_fin_has_three_face_edges():
    _, _, f = ref.mesh("fin")
    counts = ref.edge_face_counts(f)
    assert set(counts.values()) == {1, 2, 3} and sum(c == 3 for c in counts.values()) == 8


@BOTH
@pytest.mark.parametrize("case", ("fin", "fin_weight"))
def test_fin_keeps_its_locked_vertices_and_edges(result, case):
    r = result(case)
    v, _, f = ref.mesh("fin")
    assert len(r["faces"]) in (ref.CASES[case][1] - 1, ref.CASES[case][1])
    locked = sorted({i for e, c in ref.edge_face_counts(f).items() if c == 3 for i in e})
    assert len(locked) == 9
    where = {tuple(p): i for i, p in enumerate(r["positions"])}
    assert all(tuple(v[i]) in where for i in locked)                     # they never move (and never merge)
    out = ref.edge_face_counts(r["faces"])
    for (a, b), c in ref.edge_face_counts(f).items():
        if c == 3:
            ia, ib = where[tuple(v[a])], where[tuple(v[b])]
            assert out[(min(ia, ib), max(ia, ib))] == 3
    assert sum(c == 3 for c in out.values()) == 8


@BOTH
def test_target_above_the_face_count_returns_the_cleaned_input(result):
    r = result("target_above")
    v, c, f = ref.mesh("degenerate")
    clean = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    assert len(clean) == len(f) - 3
    rv, rc, rf = sref.drop_unreferenced(v, c, clean)
    assert len(rv) == len(v) - 1
    assert np.array_equal(r["faces"], rf) and ref.exact(r["positions"], rv) and ref.exact(r["colors"], rc)


@BOTH
def test_open_mesh_may_end_one_below_the_target(result):
    r = result("open_within_one")          # the round's last collapse is an inner edge: two faces for a budget of one
    assert len(r["faces"]) == ref.CASES["open_within_one"][1] - 1


def test_yardstick_rounds_apply_an_independent_set():
    r = ref.expected("cube16_scattered")
    assert r["rounds"] == len(r["applied"]) and all(a >= 1 for a in r["applied"])
    assert all(a <= w for a, w in zip(r["applied"], r["window"]))


def test_argument_errors():
    from scorp_amd.mesh import Mesh, simplify_quadric_decimation
    m = _mesh("cube8")
    inf = float("inf")
    bad_face = m.faces.clone()
    bad_face[3, 1] = m.vertices.shape[0]
    negative = m.faces.clone()
    negative[0, 0] = -1
    nan_vertex = m.vertices.clone()
    nan_vertex[5, 2] = float("nan")
    inf_vertex = m.vertices.clone()
    inf_vertex[7, 0] = inf
    for mesh, args in ((m, (-1,)), (m, (10, -1e-9)), (m, (10, float("nan"))), (m, (10, inf, -1.0)), (m, (10, inf, inf)),
                       (m, (10, inf, float("nan"))), (Mesh(m.vertices, bad_face, m.colors), (10,)),
                       (Mesh(m.vertices, negative, m.colors), (10,)), (Mesh(nan_vertex, m.faces, m.colors), (10,)),
                       (Mesh(inf_vertex, m.faces, m.colors), (10,)), (Mesh(m.vertices[:, :2], m.faces, m.colors), (10,)),
                       (Mesh(m.vertices, m.faces[:, :2], m.colors), (10,)), (Mesh(m.vertices, m.faces.float(), m.colors), (10,)),
                       (Mesh(m.vertices, m.faces, m.colors[:-1]), (10,))):
        with pytest.raises(ValueError):
            simplify_quadric_decimation(mesh, *args)


def test_empty_mesh_comes_back_empty():
    from scorp_amd.mesh import Mesh, simplify_quadric_decimation
    for nv in (0, 5):
        out = simplify_quadric_decimation(Mesh(torch.rand(nv, 3), torch.empty(0, 3, dtype=torch.int32), torch.rand(nv, 3)), 10)
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.colors.shape) == (0, 3)
        assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32
