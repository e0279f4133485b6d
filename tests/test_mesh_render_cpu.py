"""scorp_amd/mesh/render.py without a GPU: the numpy form of the mesh-render rules (include/scorp_gs.h) against the exact
yardstick of tests/mesh_render_reference.py on the fixtures of tests/mesh_render_fixtures.py, the argument checks, the
package's re-exports, and the C ABI's own checks (which run before any HIP call).  tests/test_mesh_render_gpu.py runs the
same bodies on the kernels."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import mesh_render_checks as checks
from tests import mesh_render_fixtures as fx

HOMES = {"render": ["WORKSPACE_CAP", "MAX_RENDER_VIEWS", "MAX_RENDER_SIDE", "MeshRender", "DepthDifference", "render_mesh", "face_visibility",
                    "cull_unseen_faces", "depth_difference", "_render_mesh_numpy"]}


@pytest.mark.parametrize("home", sorted(HOMES))
def test_the_package_re_exports_the_modules_names(home):
    package = importlib.import_module("scorp_amd.mesh")
    module = importlib.import_module(f"scorp_amd.mesh.{home}")
    for name in HOMES[home]:
        assert getattr(package, name) is getattr(module, name), name
        if callable(getattr(module, name)):
            assert getattr(module, name).__module__ == module.__name__, name


@pytest.mark.parametrize("name", fx.CHECKED_IN_PYTHON)
def test_numpy_form_matches_the_yardstick(name):
    checks.check_fixture(name, "cpu")


def test_winding_and_backface_culling():
    checks.check_winding_and_culling("cpu")


@pytest.mark.parametrize("count", fx.COUNT_EDGES)
def test_face_counts_at_the_block_edges(count):
    checks.check_counts(count, "cpu")


def test_coplanar_duplicates_go_to_the_lower_index():
    checks.check_coplanar("cpu")


def test_an_index_out_of_range_is_never_followed():
    """check_mesh refuses such a mesh, so this calls the numpy form itself"""
    from scorp_amd.mesh import _render_mesh_numpy
    f = fx.fixture("bad_indices")
    depth, face, _, _, visible = _render_mesh_numpy(f["verts"], f["faces"], None, f["full_proj"], f["H"], f["W"], f["near"], False, False)
    want_face, want_depth, want_visible = fx.expected("bad_indices")
    assert np.array_equal(face, want_face) and set(np.unique(face)) == {-1, 1}
    assert np.array_equal(visible, want_visible) and visible.tolist() == [0, 1, 0, 0]


def test_arguments_python_refuses_and_the_empty_mesh():
    checks.check_python_refuses("cpu")


def test_a_list_of_cameras():
    checks.check_cameras_argument("cpu")


def test_views_split_over_calls_give_the_same_bits():
    checks.check_view_splits("cpu")


def test_sphere_depth_within_the_chord_bound():
    checks.check_sphere_depth("cpu")


def test_sphere_colour_and_barycentrics():
    checks.check_sphere_colour("cpu")


def test_cull_unseen_faces_of_a_cube():
    checks.check_cube_culling("cpu")


def test_support_depth():
    checks.check_support_depth("cpu")


def test_depth_difference():
    checks.check_depth_difference("cpu")


def test_extractor_methods_need_the_maps():
    from scorp_amd.mesh import GaussianExtractor, empty_mesh

    class _Points:
        get_xyz = torch.zeros(4, 3)
    ex = GaussianExtractor(_Points(), lambda *a, **k: None, pipe=None)
    for call in (lambda: ex.render_mesh(empty_mesh("cpu")), lambda: ex.cull_unseen_faces(empty_mesh("cpu"))):
        with pytest.raises(RuntimeError, match="reconstruction"):
            call()


def test_extractor_methods_on_given_maps():
    """the two methods only hand the kept views on: with depthmaps set to the mesh's own render, a depth tolerance of 0
    keeps what plain culling keeps"""
    from scorp_amd.mesh import GaussianExtractor, cull_unseen_faces

    class _Points:
        get_xyz = torch.zeros(4, 3)
    f = fx.fixture("cube")
    mesh = checks.mesh_of(f, "cpu")
    ex = GaussianExtractor(_Points(), lambda *a, **k: None, pipe=None)
    ex.full_proj = torch.from_numpy(f["full_proj"]).reshape(-1, 4, 4)
    ex.depthmaps = torch.zeros(2, f["H"], f["W"])
    out = ex.render_mesh(mesh, colors=False)
    assert torch.equal(out.depth, checks.render("cube", "cpu").depth) and out.color is None
    ex.depthmaps = out.depth
    plain = cull_unseen_faces(mesh, ex.full_proj, f["H"], f["W"])
    for got in (ex.cull_unseen_faces(mesh), ex.cull_unseen_faces(mesh, depth_tolerance=0.0)):
        assert torch.equal(got.faces, plain.faces) and torch.equal(got.vertices, plain.vertices)
    assert ex.cull_unseen_faces(mesh, min_views=2).faces.shape[0] == 4


DUMMY = 0x10000   # non-zero and 256-byte aligned; validation runs before any HIP call, so it is never dereferenced

BAD_CALLS = {
    "no vertices": (dict(vertices=None), b"NULL"),
    "no faces": (dict(faces=None), b"NULL"),
    "no full_proj": (dict(full_proj=None), b"NULL"),
    "no out_depth": (dict(out_depth=None), b"NULL"),
    "no out_face": (dict(out_face=None), b"NULL"),
    "colour without colours": (dict(out_color=DUMMY), b"out_color without colors"),
    "Nv 0": (dict(Nv=0), b"num_vertices"),
    "Nv above 2^30": (dict(Nv=(1 << 30) + 1), b"num_vertices"),
    "F -1": (dict(F=-1), b"num_faces"),
    "F above 2^28": (dict(F=(1 << 28) + 1), b"num_faces"),
    "V 0": (dict(V=0), b"num_views"),
    "H 0": (dict(H=0), b"height and width"),
    "W 16385": (dict(W=16385), b"height and width"),
    "near 0": (dict(near=0.0), b"near"),
    "near inf": (dict(near=float("inf")), b"near"),
    "near NaN": (dict(near=float("nan")), b"near"),
    "unknown flag": (dict(flags=2), b"unknown flags"),
    "negative tolerance": (dict(support=DUMMY, tol=-1.0), b"support_tolerance"),
    "NaN tolerance": (dict(support=DUMMY, tol=float("nan")), b"support_tolerance"),
    "no workspace": (dict(workspace=None), b"workspace"),
    "misaligned workspace": (dict(workspace=DUMMY + 64), b"workspace"),
    "small workspace": (dict(size_less=1), b"workspace"),
}


@pytest.fixture(scope="module")
def built_lib():
    from scorp_amd import build
    return build.build()


@pytest.mark.parametrize("what", sorted(BAD_CALLS))
def test_the_c_abi_refuses(built_lib, what):
    from scorp_amd import _C
    L = _C.lib()
    a = dict(vertices=DUMMY, Nv=8, faces=DUMMY, F=12, colors=None, full_proj=DUMMY, V=2, H=37, W=53, near=0.01, flags=0, support=None, tol=0.0,
             out_depth=DUMMY, out_face=DUMMY, out_bary=None, out_color=None, out_visible=None, workspace=DUMMY, size_less=0)
    edit, reason = BAD_CALLS[what]
    a.update(edit)
    size = L.scorp_mesh_render_workspace_bytes(8, 12, 2, 37, 53)
    assert size >= 2 * (8 * 16 + 37 * 53 * 8 + 12 * 5) and size % 256 == 0
    rc = L.scorp_mesh_render(a["vertices"], a["Nv"], a["faces"], a["F"], a["colors"], a["full_proj"], a["V"], a["H"], a["W"], a["near"], a["flags"],
                             a["support"], a["tol"], a["out_depth"], a["out_face"], a["out_bary"], a["out_color"], a["out_visible"],
                             a["workspace"], size - a["size_less"], None)
    assert rc == _C.ERR_INVALID
    assert reason in L.scorp_last_error()


def test_workspace_bytes_is_zero_outside_the_limits(built_lib):
    from scorp_amd import _C
    L = _C.lib()
    assert L.scorp_mesh_render_workspace_bytes(1, 0, 1, 1, 1) > 0
    for args in ((0, 1, 1, 1, 1), ((1 << 30) + 1, 1, 1, 1, 1), (1, (1 << 28) + 1, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 65536, 1, 1), (1, 1, 1, 0, 1),
                 (1, 1, 1, 1, 16385)):
        assert L.scorp_mesh_render_workspace_bytes(*args) == 0, args
