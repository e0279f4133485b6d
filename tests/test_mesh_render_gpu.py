"""csrc/mesh_render.hip on the GPU against tests/mesh_render_reference.py: the bodies of tests/mesh_render_checks.py that
tests/test_mesh_render_cpu.py runs on the numpy form, here on CUDA tensors, plus what only the kernels have: the large list
at the edges of its stride, the raw C call with indices that are out of range, the agreement of the two forms bit for bit,
two runs, a permutation of the faces, the chunking of the views under a small workspace cap, and the extractor's methods
on the surfel scene of tests/test_mesh_gpu.py.

Measured in one MI355X run (printed by the tests): on every fixture the kernel's depth equals the correctly rounded exact
value at EVERY owned pixel - 0 pixels differ, where the acceptance allows an fp32 neighbour - triangle 449 pixels, quad 256,
grid 1 961, overlap 779, coplanar 613, interpenetrating 1 033, covering and large_mix 4 096, counts 187, large_list 3 107,
near 430, snap_bound 1 961, degenerate 449, sphere 5 022 over three views, cube 1 775 over two; the numpy form gives the same
zeros, and the two forms the same bits in depth, face, barycentric, colour and visible_views on the seven fixtures
compared.  Sphere: 5 000 pixels inside the chord bound (largest circumradius 0.0951, inner radius 0.995472), largest colour
error 5.6e-8 against the bound 2^-23 = 1.19e-7.  Extractor (15 880 faces, 8 views of 96 x 80): mean |mesh - surfel depth|
0.0219, largest 0.472, the mesh covers 87.4 % of the surfel render's pixels; cull_unseen_faces keeps 8 508 faces, 2 814 with
min_views=2, 8 438 with depth_tolerance=0.1.  DESIGN.md 4.12 ("Looking at a mesh") quotes the same run."""
import numpy as np
import pytest
import torch

from tests import mesh_render_checks as checks
from tests import mesh_render_fixtures as fx

pytestmark = pytest.mark.gpu

BIT_EQUAL = ("grid", "large_mix", "sphere", "cube", "coplanar", "interpenetrating", "snap_bound")


@pytest.mark.parametrize("name", fx.CHECKED_IN_PYTHON)
def test_kernel_matches_the_yardstick(name):
    checks.check_fixture(name, "cuda")


def test_winding_and_backface_culling():
    checks.check_winding_and_culling("cuda")


@pytest.mark.parametrize("count", fx.COUNT_EDGES)
def test_face_counts_at_the_block_edges(count):
    checks.check_counts(count, "cuda")


@pytest.mark.parametrize("count", fx.LARGE_EDGES)
def test_large_list_lengths_at_the_edges_of_its_stride(count):
    checks.check_large_list(count, "cuda")


def test_coplanar_duplicates_go_to_the_lower_index():
    checks.check_coplanar("cuda")


def _colors_of(name):
    n = len(fx.fixture(name)["verts"])
    return checks.sphere_colors() if name == "sphere" else np.random.default_rng(3).uniform(0, 1, (n, 3)).astype(np.float32)


@pytest.mark.parametrize("name", BIT_EQUAL)
def test_kernel_and_numpy_form_give_the_same_bits(name):
    """the two run the same int64 and float64 statements with fp contraction off; the box a thread walks decides no value"""
    colors = _colors_of(name)
    gpu, cpu = (checks.render(name, dev, colors=colors, barycentric=True) for dev in ("cuda", "cpu"))
    for a, b, what in zip(gpu, cpu, checks.MeshRenderFields):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.numpy().view(np.uint32)), what
    assert np.array_equal(checks.visibility(name, "cuda"), checks.visibility(name, "cpu")), "visible_views"


def test_two_runs_give_the_same_bits():
    colors = _colors_of("large_mix")
    a, b = (checks.render("large_mix", "cuda", colors=colors, barycentric=True) for _ in range(2))
    for x, y, what in zip(a, b, checks.MeshRenderFields):
        assert torch.equal(x, y), what
    assert np.array_equal(checks.visibility("large_mix", "cuda"), checks.visibility("large_mix", "cuda"))


def test_a_permutation_of_the_faces_only_renames_them():
    """(not claimed for coplanar duplicates: there the LOWER of the two indices wins, whichever face carries it)"""
    from scorp_amd.mesh import Mesh, face_visibility, render_mesh
    for name in ("large_mix", "sphere"):
        f = fx.fixture(name)
        mesh = checks.mesh_of(f, "cuda", colors=_colors_of(name))
        fp = torch.from_numpy(f["full_proj"]).cuda()
        perm = torch.from_numpy(np.random.default_rng(7).permutation(len(f["faces"]))).cuda()
        shuffled = Mesh(mesh.vertices, mesh.faces[perm].contiguous(), mesh.colors)
        a = render_mesh(mesh, fp, f["H"], f["W"], barycentric=True)
        b = render_mesh(shuffled, fp, f["H"], f["W"], barycentric=True)
        assert torch.equal(a.depth, b.depth) and torch.equal(a.color, b.color) and torch.equal(a.barycentric, b.barycentric)
        named = torch.where(b.face >= 0, perm[b.face.clamp(min=0).long()].to(torch.int32), b.face)
        assert torch.equal(a.face, named)
        assert torch.equal(face_visibility(mesh, fp, f["H"], f["W"])[perm], face_visibility(shuffled, fp, f["H"], f["W"]))


def test_raw_call_never_follows_an_index_out_of_range():
    """faces that name vertex 3 of 3, -1 and 2^31 - 1: the kernels compare before they load, so the faces are dropped"""
    from scorp_amd import _C
    f = fx.fixture("bad_indices")
    dev = torch.device("cuda")
    verts, faces, fp = (torch.from_numpy(np.array(f[k])).to(dev) for k in ("verts", "faces", "full_proj"))
    H, W, F = f["H"], f["W"], len(f["faces"])
    depth = torch.empty(1, H, W, device=dev)
    face = torch.empty(1, H, W, dtype=torch.int32, device=dev)
    visible = torch.zeros(F, dtype=torch.int32, device=dev)
    size = _C.lib().scorp_mesh_render_workspace_bytes(3, F, 1, H, W)
    workspace = torch.empty(size, dtype=torch.uint8, device=dev)
    _C.call("scorp_mesh_render", verts, 3, faces, F, None, fp, 1, H, W, 0.01, 0, None, 0.0, depth, face, None, None, visible, workspace, size)
    want_face, want_depth, want_visible = fx.expected("bad_indices")
    checks.judge("bad_indices through the C ABI", checks.MeshRenderOut(depth, face), want_face, want_depth)
    assert visible.tolist() == want_visible.tolist() == [0, 1, 0, 0]
    _C.call("scorp_mesh_render", verts, 3, faces, F, None, fp, 1, H, W, 0.01, 0, None, 0.0, depth, face, None, None, visible, workspace, size)
    assert visible.tolist() == [0, 2, 0, 0], "out_visible_views is added to"


@pytest.mark.parametrize("name, large", [("counts", 0), ("covering", 1), ("large_mix", 1), ("large_list", fx.LARGE_GROUPS + 1)])
def test_header_counts_the_triangles_a_workgroup_walked(name, large):
    from scorp_amd.mesh import render_mesh
    f = fx.fixture(name)
    header = []
    render_mesh(checks.mesh_of(f, "cuda"), torch.from_numpy(f["full_proj"]).cuda(), f["H"], f["W"], header=header)
    assert [h.tolist() for h in header] == [[large]]


def test_arguments_python_refuses_and_the_empty_mesh():
    checks.check_python_refuses("cuda")


def test_a_list_of_cameras():
    checks.check_cameras_argument("cuda")


def test_views_split_over_calls_and_chunks_give_the_same_bits(monkeypatch):
    checks.check_view_splits("cuda", monkeypatch)


def test_sphere_depth_within_the_chord_bound():
    checks.check_sphere_depth("cuda")


def test_sphere_colour_and_barycentrics():
    checks.check_sphere_colour("cuda")


def test_cull_unseen_faces_of_a_cube():
    checks.check_cube_culling("cuda")


def test_support_depth():
    checks.check_support_depth("cuda")


def test_depth_difference():
    checks.check_depth_difference("cuda")


def test_extractor_renders_and_culls_its_own_mesh():
    """Structure only: nobody has measured how far a mesh of a blurred surfel render lies from that render, so the figures of
    depth_difference are printed (and recorded in DESIGN.md 4.12), not asserted."""
    from scorp_amd.mesh import GaussianExtractor, check_mesh, depth_difference
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    from tests.test_mesh_gpu import sphere_surfels
    dev = torch.device("cuda:0")
    model = GaussianModel2D.from_raw(sphere_surfels(), 0, device=dev)
    model.active_sh_degree = 0
    pipe = PipelineParams()
    pipe.depth_ratio = 0.0
    ex = GaussianExtractor(model, render, pipe)
    ex.reconstruction(ring_cameras(8, 96, 80, 3, radius=4.0, device=dev))
    mesh = ex.extract_mesh_bounded(voxel_size=0.05, sdf_trunc=0.2, depth_trunc=6)
    F = mesh.faces.shape[0]
    out = ex.render_mesh(mesh, barycentric=True)
    assert tuple(out.depth.shape) == (8, 80, 96) == tuple(out.face.shape) and out.face.dtype == torch.int32
    assert tuple(out.color.shape) == (8, 3, 80, 96) == tuple(out.barycentric.shape)
    assert bool((out.face >= 0).flatten(1).any(1).all()), "a view in which the mesh covers no pixel"
    assert int(out.face.max()) < F and bool(((out.depth > 0) == (out.face >= 0)).all())
    d = depth_difference(out.depth, ex.depthmaps)
    print(f"extractor: {F} faces; mesh depth against the surfel depth over 8 views of 96 x 80: {d.overall}")
    for kw in (dict(), dict(min_views=2), dict(depth_tolerance=0.1)):
        culled = ex.cull_unseen_faces(mesh, **kw)
        print(f"cull_unseen_faces({kw}): {culled.faces.shape[0]} of {F} faces, {culled.vertices.shape[0]} of {mesh.vertices.shape[0]} vertices")
        assert culled.faces.shape[0] <= F and culled.faces.dtype == torch.int32
        assert culled.faces.shape[0] == 0 or check_mesh(culled) is not None
