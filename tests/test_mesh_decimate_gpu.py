"""The decimation kernels (csrc/mesh_decimate.hip) through scorp_amd.mesh.simplify_quadric_decimation on CUDA tensors against
the plain-Python yardstick of tests/mesh_decimate_reference.py, on every case there and on the surface-nets mesh of the
three spheres.  Faces must be EQUAL and positions and colours equal BIT FOR BIT: the rules sum no float in an order that
could vary, so nothing is left out of the comparison and there is no tolerance - with one, a decision would fall the
other way somewhere and every later round would differ."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_cluster_reference as cluster_ref
from tests import mesh_decimate_reference as ref
from tests import mesh_simplify_reference as sref

pytestmark = pytest.mark.gpu

SPHERES_TARGET = 2400
CASES = tuple(sorted(ref.CASES)) + ("spheres",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(case):
    """(vertices, colours, faces, target, maximum_error, boundary_weight); `spheres` comes from extract_surface on the GPU"""
    if case == "spheres":
        from scorp_amd.mesh import extract_surface
        grid, coords = cluster_ref.three_spheres()
        d = torch.device("cuda:0")
        v, f = extract_surface(torch.from_numpy(grid).to(d), [torch.from_numpy(c).to(d) for c in coords])
        return v.cpu().numpy(), sref.vertex_colors(v.shape[0]), f.cpu().numpy(), SPHERES_TARGET, ref.INF, 1.0
    name, target, max_err, bw = ref.CASES[case]
    return ref.mesh(name) + (target, max_err, bw)


@functools.lru_cache(maxsize=None)
def expected(case):
    return ref.expected(case) if case != "spheres" else ref.decimate(*_case(case))


def _run(dev, case, rounds=None):
    from scorp_amd.mesh import Mesh, simplify_quadric_decimation
    v, c, f, target, max_err, bw = _case(case)
    out = simplify_quadric_decimation(Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(c).to(dev)), target,
                                      max_err, bw, rounds=rounds)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES)
def test_kernels_match_the_yardstick(dev, case):
    rounds = []
    out, r = _run(dev, case, rounds), expected(case)
    got_v, got_c, got_f = out.vertices.cpu().numpy(), out.colors.cpu().numpy(), out.faces.cpu().numpy()
    differ = lambda a, b: int((a.view(np.uint32) != b.view(np.uint32)).sum()) if a.shape == b.shape else -1
    print(f"{case}: {len(_case(case)[2])} -> {len(got_f)} faces ({len(r['faces'])}), {len(rounds)} rounds ({r['rounds']}), "
          f"{differ(got_v, r['positions'])} position and {differ(got_c, r['colors'])} colour components differ")
    assert len(rounds) == r["rounds"]
    assert np.array_equal(got_f, r["faces"])
    assert ref.exact(got_v, r["positions"])
    assert ref.exact(got_c, r["colors"])


def test_counts_of_the_real_producers_mesh(dev):
    v, _, f = _case("spheres")[:3]
    assert (len(v), len(f)) == (2372, 4732)
    assert len(expected("spheres")["faces"]) in (SPHERES_TARGET - 1, SPHERES_TARGET)


@pytest.mark.parametrize("case", ("cube16_scattered", "spheres", "fin"))
def test_two_runs_give_equal_tensors(dev, case):
    a, b = _run(dev, case), _run(dev, case)
    assert torch.equal(a.faces, b.faces) and torch.equal(a.vertices, b.vertices) and torch.equal(a.colors, b.colors)


def test_result_is_on_the_device(dev):
    out = _run(dev, "wavy_sheet")
    assert out.vertices.device == dev and out.faces.device == dev and out.colors.device == dev
    assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32
    assert out.vertices.shape[1] == 3 and out.colors.shape == out.vertices.shape and out.faces.shape[1] == 3


def test_empty_does_not_call_the_library(dev, monkeypatch):
    from scorp_amd import _C
    from scorp_amd.mesh import Mesh, simplify_quadric_decimation

    def no_library():
        raise AssertionError("the library was called for an empty mesh")
    monkeypatch.setattr(_C, "lib", no_library)
    for nv in (0, 5):
        out = simplify_quadric_decimation(Mesh(torch.rand(nv, 3, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                                               torch.rand(nv, 3, device=dev)), 10)
        assert out.vertices.is_cuda and tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3)
        assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.float32


def test_entry_points_refuse_bad_arguments(dev):
    from scorp_amd import _C
    L = _C.lib()
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    d, inf, nan = buf.data_ptr(), float("inf"), float("nan")
    calls = (
        (L.scorp_mesh_decimate_quadrics, (None, 10, d, 10, d, d, 20, d, d, 1.0, d, None), b"NULL"),
        (L.scorp_mesh_decimate_quadrics, (d, 0, d, 10, d, d, 20, d, d, 1.0, d, None), b"num_vertices"),
        (L.scorp_mesh_decimate_quadrics, (d, 10, d, (1 << 28) + 1, d, d, 20, d, d, 1.0, d, None), b"num_faces"),
        (L.scorp_mesh_decimate_quadrics, (d, 10, d, 10, d, d, 31, d, d, 1.0, d, None), b"num_edges"),
        (L.scorp_mesh_decimate_quadrics, (d, 10, d, 10, d, d, 20, d, d, -1.0, d, None), b"boundary_weight"),
        (L.scorp_mesh_decimate_quadrics, (d, 10, d, 10, d, d, 20, d, d, inf, d, None), b"boundary_weight"),
        (L.scorp_mesh_decimate_flags, (d, d, 20, (1 << 30) + 1, d, None), b"num_vertices"),
        (L.scorp_mesh_decimate_flags, (d, None, 20, 10, d, None), b"NULL"),
        (L.scorp_mesh_decimate_candidates, (d, d, 10, d, 10, d, d, 20, d, d, d, -1.0, d, d, None), b"maximum_error"),
        (L.scorp_mesh_decimate_candidates, (d, d, 10, d, 10, d, d, 20, d, d, d, nan, d, d, None), b"maximum_error"),
        (L.scorp_mesh_decimate_candidates, (d, d, 10, d, 10, d, d, 0, d, d, d, inf, d, d, None), b"num_edges"),
        (L.scorp_mesh_decimate_candidates, (d, d, 10, d, 10, d, d, 20, d, d, d, inf, None, d, None), b"NULL"),
        (L.scorp_mesh_decimate_hash, (d, 20, d, 21, 1, d, None), b"num_window"),
        (L.scorp_mesh_decimate_hash, (d, 20, d, 5, 0, d, None), b"round"),
        (L.scorp_mesh_decimate_select, (d, 20, d, 0, 10, d, d, d, None), b"num_window"),
        (L.scorp_mesh_decimate_select, (d, 20, d, 5, 10, d, None, d, None), b"NULL"),
        (L.scorp_mesh_decimate_apply, (d, 20, d, d, 21, d, 10, d, d, d, d, d, None), b"num_window"),
        (L.scorp_mesh_decimate_apply, (d, 20, d, d, 5, d, 0, d, d, d, d, d, None), b"num_vertices"),
        (L.scorp_mesh_decimate_faces, (d, 0, d, 10, d, d, None), b"num_faces"),
        (L.scorp_mesh_decimate_faces, (d, 10, None, 10, d, d, None), b"NULL"),
    )
    for fn, args, text in calls:
        assert fn(*args) == _C.ERR_INVALID and text in L.scorp_last_error(), (fn.__name__, args, L.scorp_last_error())
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0   # nothing was launched
