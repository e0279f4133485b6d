"""The bodies the CPU and GPU test files of scorp_amd/mesh/render.py share: each takes the device to run on ("cpu": the numpy
form, "cuda": csrc/mesh_render.hip) and asserts against tests/mesh_render_reference.py."""
import collections
import functools

import numpy as np
import pytest
import torch

from tests import mesh_render_fixtures as fx


def mesh_of(f, dev, num_faces=None, colors=None):
    from scorp_amd.mesh import Mesh
    v = torch.from_numpy(np.array(f["verts"])).to(dev)
    c = torch.zeros(v.shape[0], 3, device=dev) if colors is None else torch.from_numpy(np.array(colors, np.float32)).to(dev)
    return Mesh(v, torch.from_numpy(np.array(f["faces"][:num_faces])).to(dev), c)


def render(name, dev, cull=False, num_faces=None, colors=None, barycentric=False):
    from scorp_amd.mesh import render_mesh
    f = fx.fixture(name)
    out = render_mesh(mesh_of(f, dev, num_faces, colors), torch.from_numpy(f["full_proj"]).to(dev), f["H"], f["W"], near=f["near"],
                      cull_backfaces=cull, colors=colors is not None, barycentric=barycentric)
    assert all(t is None or t.device.type == dev for t in out)
    return out


def visibility(name, dev, cull=False, num_faces=None, **kw):
    from scorp_amd.mesh import face_visibility
    f = fx.fixture(name)
    return face_visibility(mesh_of(f, dev, num_faces), torch.from_numpy(f["full_proj"]).to(dev), f["H"], f["W"], near=f["near"],
                           cull_backfaces=cull, **kw).cpu().numpy()


def judge(what, out, want_face, want_depth):
    """face equal everywhere; depth the correctly rounded exact value or one of its fp32 neighbours; prints how many differ"""
    face, depth = out.face.cpu().numpy(), out.depth.cpu().numpy()
    assert face.dtype == np.int32 and depth.dtype == np.float32 and face.shape == want_face.shape
    assert np.array_equal(face, want_face), f"{what}: {int((face != want_face).sum())} pixels name another face"
    off = depth != want_depth
    print(f"{what}: {int((want_face >= 0).sum())} pixels owned, depth differs from the correctly rounded value at {int(off.sum())}")
    lo, hi = np.nextafter(want_depth, np.float32(-np.inf)), np.nextafter(want_depth, np.float32(np.inf))
    assert ((depth == want_depth) | (((depth == lo) | (depth == hi)) & (want_face >= 0))).all(), f"{what}: a depth is off by more than one ulp"
    return int(off.sum())


def check_fixture(name, dev, cull=False):
    f = fx.fixture(name)
    want_face, want_depth, want_visible = fx.expected(name, cull)
    judge(f"{name} on {dev}" + (" (culled)" if cull else ""), render(name, dev, cull), want_face, want_depth)
    assert np.array_equal(visibility(name, dev, cull), want_visible), "visible_views"
    if "owned" in f and not cull:
        assert int((want_face >= 0).sum()) == f["owned"]
        if f.get("once"):
            assert all(len(lst) == 1 for o in fx.owners(name) for lst in o.values()), "a centre is owned twice"
    if "only_face" in f:
        assert set(np.unique(want_face)) - {-1} == {f["only_face"]}


def check_winding_and_culling(dev):
    """the reversed triangle covers the same pixels (rule 3 exchanges two corners); culling keeps exactly one of the two;
    the barycentrics of the reversed one come back in ITS corner order"""
    a, b = render("triangle", dev, barycentric=True), render("triangle_reversed", dev, barycentric=True)
    assert torch.equal(a.face, b.face) and int((a.face >= 0).sum()) > 100
    assert torch.equal(a.barycentric[:, 0], b.barycentric[:, 0])
    assert (a.barycentric[:, 1] - b.barycentric[:, 2]).abs().max() <= 2.0 ** -22 and (a.barycentric[:, 2] - b.barycentric[:, 1]).abs().max() <= 2.0 ** -22
    ca, cb = render("triangle", dev, cull=True), render("triangle_reversed", dev, cull=True)
    kept = [int((t.face >= 0).sum()) for t in (ca, cb)]
    assert sorted(kept) == [0, int((a.face >= 0).sum())], kept
    for name in ("triangle", "triangle_reversed"):
        check_fixture(name, dev, cull=True)
    # the sphere is wound counter-clockwise seen from outside: culling its back faces changes no pixel
    s, sc = render("sphere", dev), render("sphere", dev, cull=True)
    assert torch.equal(s.face, sc.face) and torch.equal(s.depth, sc.depth)


def check_counts(n, dev):
    want_face, want_depth, want_visible = fx.expected("counts", False, n)
    judge(f"counts[{n}] on {dev}", render("counts", dev, num_faces=n), want_face, want_depth)
    assert np.array_equal(visibility("counts", dev, num_faces=n), want_visible)


def check_large_list(n, dev):
    want_face, want_depth, want_visible = fx.expected("large_list", False, n)
    judge(f"large_list[{n}] on {dev}", render("large_list", dev, num_faces=n), want_face, want_depth)
    assert np.array_equal(visibility("large_list", dev, num_faces=n), want_visible)


def check_coplanar(dev):
    out = render("coplanar", dev)
    want_face, want_depth, _ = fx.expected("coplanar")
    judge(f"coplanar on {dev}", out, want_face, want_depth)
    faces = set(np.unique(out.face.cpu().numpy()))
    assert 1 in faces and 2 not in faces, "of two coplanar duplicates the lower index wins"


def check_python_refuses(dev):
    from scorp_amd.mesh import Mesh, cull_unseen_faces, empty_mesh, face_visibility, render_mesh
    f = fx.fixture("bad_indices")
    fp = torch.from_numpy(f["full_proj"]).to(dev)
    with pytest.raises(ValueError, match="vertex index -1 with 3 vertices"):
        render_mesh(mesh_of(f, dev), fp, f["H"], f["W"])
    good = mesh_of(fx.fixture("triangle"), dev)
    for kw, msg in ((dict(near=0.0), "near"), (dict(near=float("inf")), "near"), (dict(near=float("nan")), "near")):
        with pytest.raises(ValueError, match=msg):
            render_mesh(good, fp, 8, 8, **kw)
    with pytest.raises(ValueError, match="height and width"):
        render_mesh(good, fp)
    with pytest.raises(ValueError, match=r"\[1, 16384\]"):
        render_mesh(good, fp, 0, 8)
    with pytest.raises(ValueError, match="full_proj"):
        render_mesh(good, fp.reshape(-1)[:12].reshape(1, 12), 8, 8)
    with pytest.raises(ValueError, match="min_views"):
        cull_unseen_faces(good, fp, 8, 8, min_views=0)
    with pytest.raises(ValueError, match="support_tolerance"):
        face_visibility(good, fp, 8, 8, support_depth=torch.zeros(1, 8, 8, device=dev))
    with pytest.raises(ValueError, match="support_tolerance"):
        face_visibility(good, fp, 8, 8, support_depth=torch.zeros(1, 8, 8, device=dev), support_tolerance=-1.0)
    with pytest.raises(ValueError, match="support_depth must be"):
        face_visibility(good, fp, 8, 8, support_depth=torch.zeros(1, 8, 9, device=dev), support_tolerance=0.1)
    out = render_mesh(empty_mesh(torch.device(dev)), fp.repeat(2, 1), 5, 7, barycentric=True)   # an empty mesh: empty maps
    assert tuple(out.depth.shape) == (2, 5, 7) and float(out.depth.abs().max()) == 0.0 and int(out.face.max()) == -1
    assert tuple(out.color.shape) == (2, 3, 5, 7) and tuple(out.barycentric.shape) == (2, 3, 5, 7)
    assert face_visibility(empty_mesh(torch.device(dev)), fp, 5, 7).shape == (0,)
    assert cull_unseen_faces(empty_mesh(torch.device(dev)), fp, 5, 7).faces.shape == (0, 3)


def check_cameras_argument(dev):
    """a list of cameras gives full_proj and the resolution; two resolutions raise"""
    from scorp_amd.camera import look_at_camera
    from scorp_amd.mesh import render_mesh
    f = fx.fixture("sphere")
    cams = [look_at_camera(e, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0) if abs(e[2]) < 2 else (0.0, 1.0, 0.0), fx.SPHERE_FOV, (f["W"], f["H"]), device=dev)
            for e in fx.SPHERE_EYES]
    a, b = render_mesh(mesh_of(f, dev), cams), render("sphere", dev)
    assert torch.equal(a.face, b.face) and torch.equal(a.depth, b.depth)
    cams[1] = look_at_camera(fx.SPHERE_EYES[1], (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), fx.SPHERE_FOV, (48, 32), device=dev)
    with pytest.raises(ValueError, match="different resolutions"):
        render_mesh(mesh_of(f, dev), cams)


def check_view_splits(dev, monkeypatch=None):
    """V = 3 in one call equals three single-view calls bit for bit, and (on the GPU) any chunking forced by a small cap"""
    from scorp_amd.mesh import face_visibility, render, render_mesh
    f = fx.fixture("sphere")
    colors = sphere_colors()
    mesh = mesh_of(f, dev, colors=colors)
    fp = torch.from_numpy(f["full_proj"]).to(dev)
    whole = render_mesh(mesh, fp, f["H"], f["W"], barycentric=True)
    vis = face_visibility(mesh, fp, f["H"], f["W"])
    parts = [render_mesh(mesh, fp[v:v + 1], f["H"], f["W"], barycentric=True) for v in range(3)]
    for k, what in enumerate(MeshRenderFields):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), what
    assert torch.equal(vis, sum(face_visibility(mesh, fp[v:v + 1], f["H"], f["W"]) for v in range(3)))
    if monkeypatch is not None:   # two views per call, then one
        from scorp_amd import _C
        one = _C.lib().scorp_mesh_render_workspace_bytes(len(f["verts"]), len(f["faces"]), 1, f["H"], f["W"])
        for cap in (2 * one + 1024, 1):
            monkeypatch.setattr(render, "WORKSPACE_CAP", cap)
            again = render_mesh(mesh, fp, f["H"], f["W"], barycentric=True)
            for k, what in enumerate(MeshRenderFields):
                assert torch.equal(whole[k], again[k]), (what, cap)
            assert torch.equal(vis, face_visibility(mesh, fp, f["H"], f["W"]))


MeshRenderFields = ("depth", "face", "color", "barycentric")
MeshRenderOut = collections.namedtuple("MeshRenderOut", "depth face")   # what judge() reads, for a raw C call's outputs


# ---- the sphere: analytic depth, colour, barycentrics ----

COLOR_A = np.array([[0.11, -0.07, 0.05], [0.02, 0.13, -0.04], [-0.06, 0.03, 0.12]])   # colour = A p + C0, inside [0, 1] on the unit ball
COLOR_C0 = np.array([0.5, 0.45, 0.55])


@functools.lru_cache(maxsize=None)
def sphere_colors():
    v = fx.fixture("sphere")["verts"].astype(np.float64)
    return (v @ COLOR_A.T + COLOR_C0).astype(np.float32)


def _rays(cam, H, W, du=0.0, dv=0.0):
    """(origin [3], unit directions [H, W, 3], forward [3]) of the pixel centres moved by (du, dv) pixels, float64"""
    w2c = cam.world_view_transform.numpy().astype(np.float64).T        # stored transposed
    R, t = w2c[:3, :3], w2c[:3, 3]
    proj = cam.projection_matrix.numpy().astype(np.float64).T
    i, j = np.meshgrid(np.arange(W) + du, np.arange(H) + dv)
    ndc_x, ndc_y = (2 * i + 1) / W - 1, (2 * j + 1) / H - 1            # sx = ((ndc + 1) W - 1) / 2
    d_cam = np.stack([(ndc_x - proj[0, 2]) / proj[0, 0], (ndc_y - proj[1, 2]) / proj[1, 1], np.ones_like(ndc_x)], -1)
    d = d_cam @ R                                                      # R^T d_cam, row-vector form
    return -R.T @ t, d / np.linalg.norm(d, axis=-1, keepdims=True), R[2]


def _sphere_depth(o, d, fwd, radius):
    """view-space depth of the first hit of the rays with the sphere of `radius` about the origin; NaN for a miss"""
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return t * (d @ fwd)


def check_sphere_depth(dev):
    """The chord bound.  The vertices lie on the unit sphere, so a triangle with circumradius rc lies between the spheres of
    radius sqrt(1 - rc^2) and 1, and the closed mesh encloses the inner one: along a ray that meets the inner sphere the
    mesh's first hit has a depth between the two spheres' first hits, z_outer <= z <= z_inner.  Snapping moves each vertex
    by at most 1/512 pixel per axis, and the depth rule evaluates 1 / z, which is affine over the true triangle, with the
    snapped triangle's weights: the depth at centre P is the true mesh's depth at a point within 1/512 pixel of P per
    axis.  The bounds are therefore taken as the extremes over the four points P + (+-1/256, +-1/256) (twice the shift;
    the depth of a sphere has no interior extremum in that box except at the image of its centre, where the second-order
    term (1/256 pixel x 0.015 rad)^2 is below 1e-8) and widened by 4 fp32 ulps for the roundings of the projection."""
    f = fx.fixture("sphere")
    v = f["verts"].astype(np.float64)
    a, b, c = (v[f["faces"][:, k]] for k in range(3))
    la, lb, lc = np.linalg.norm(b - c, axis=1), np.linalg.norm(c - a, axis=1), np.linalg.norm(a - b, axis=1)
    rc = (la * lb * lc / (2 * np.linalg.norm(np.cross(b - a, c - a), axis=1))).max()   # a b c / (4 area)
    inner = float(np.sqrt(1 - rc * rc))
    out = render("sphere", dev)
    depth = out.depth.cpu().numpy().astype(np.float64)
    _, cams = fx.look_at_proj(fx.SPHERE_EYES, (0.0, 0.0, 0.0), fx.SPHERE_FOV, f["H"], f["W"])
    checked = 0
    for k, cam in enumerate(cams):
        lows, highs = [], []
        for du in (-1 / 256, 1 / 256):
            for dv in (-1 / 256, 1 / 256):
                o, d, fwd = _rays(cam, f["H"], f["W"], du, dv)
                lows.append(_sphere_depth(o, d, fwd, 1.0))
                highs.append(_sphere_depth(o, d, fwd, inner))
        lo, hi = np.min(lows, 0), np.max(highs, 0)
        inside = np.isfinite(np.sum(highs, 0))
        assert (depth[k][inside] > 0).all(), "a ray through the inner sphere misses the mesh"
        slack = 4 * 2.0 ** -23 * hi
        ok = (depth[k] >= lo - slack) & (depth[k] <= hi + slack)
        assert ok[inside].all(), f"view {k}: depth outside the chord bound by {np.abs(depth[k] - np.clip(depth[k], lo, hi))[inside].max():.3g}"
        checked += int(inside.sum())
    print(f"sphere on {dev}: {checked} pixels inside the chord bound (largest circumradius {rc:.4f}, inner radius {inner:.6f})")
    assert checked > 1000


def check_sphere_colour(dev):
    """Colours that are a linear function of the position, c = A p + c0.  The exact rule-6 colour at a pixel is that function
    at the point sum_k b_k v_k of the (float32) vertices, because the b_k sum to 1.  The test rebuilds that point from the
    OUTPUT barycentrics, each off by at most half an fp32 ulp of a weight <= 1 (2^-25) plus a few float64 roundings, against
    vertices of norm 1: the point is off by at most 3 x 2^-25 per axis, the colour by at most 3 x 2^-25 x 0.25 (the largest
    absolute row sum of A is 0.23).  The vertex colours themselves were rounded to fp32 (2^-25 each, values below 1) and
    the output once more (2^-25): 3 x 2^-25 x 0.25 + 2 x 2^-25 < 2^-23.  The weights sum to 1 within 2^-22 (three
    roundings of 2^-25 and the float64 noise)."""
    f = fx.fixture("sphere")
    out = render("sphere", dev, colors=sphere_colors(), barycentric=True)
    face, bary, color = out.face.cpu().numpy(), out.barycentric.cpu().numpy().astype(np.float64), out.color.cpu().numpy().astype(np.float64)
    hit = face >= 0
    total = bary.sum(1)
    assert np.abs(total[hit] - 1).max() <= 2.0 ** -22 and (bary >= 0).all()
    assert (bary.transpose(0, 2, 3, 1)[~hit] == 0).all() and (color.transpose(0, 2, 3, 1)[~hit] == 0).all()
    corners = f["verts"].astype(np.float64)[f["faces"][face[hit]]]                     # [n, 3 corners, 3]
    point = (bary.transpose(0, 2, 3, 1)[hit][:, :, None] * corners).sum(1)
    want = point @ COLOR_A.T + COLOR_C0
    err = np.abs(color.transpose(0, 2, 3, 1)[hit] - want).max()
    print(f"sphere colour on {dev}: largest error {err:.3g} (bound {2.0 ** -23:.3g})")
    assert err <= 2.0 ** -23
    # and the rebuilt point projects back onto its pixel: the weights are the perspective-correct ones, not the screen's
    for k in range(3):
        m = f["full_proj"][k].astype(np.float64).reshape(4, 4)
        jj, ii = np.nonzero(hit[k])
        p = np.concatenate([point[(np.nonzero(hit)[0] == k)], np.ones((len(ii), 1))], 1) @ m
        sx, sy = ((p[:, 0] / p[:, 3] + 1) * f["W"] - 1) / 2, ((p[:, 1] / p[:, 3] + 1) * f["H"] - 1) / 2
        assert np.abs(sx - ii).max() < 0.01 and np.abs(sy - jj).max() < 0.01   # (snapping: 1/512 pixel; rounding far below)


# ---- the cube: culling and support ----

def check_cube_culling(dev):
    from scorp_amd.mesh import check_mesh, cull_unseen_faces
    f = fx.fixture("cube")
    want_visible = fx.expected("cube")[2]
    sides = list(f["views_per_side"].values())
    assert want_visible.tolist() == [n for n in sides for _ in range(2)], "the yardstick sees the cube as the cameras were placed"
    mesh = mesh_of(f, dev, colors=np.linspace(0, 1, 24).reshape(8, 3))
    fp = torch.from_numpy(f["full_proj"]).to(dev)
    for min_views, keep in ((1, want_visible >= 1), (2, want_visible >= 2)):
        out = cull_unseen_faces(mesh, fp, f["H"], f["W"], min_views=min_views)
        assert check_mesh(out) is not None
        got = out.vertices[out.faces.long()].cpu().numpy()
        assert np.array_equal(got, f["verts"][f["faces"][keep]]), f"min_views={min_views}: not exactly the faces seen that often"
        used = np.unique(f["faces"][keep])
        assert out.vertices.shape[0] == len(used) and torch.equal(out.colors, mesh.colors[torch.from_numpy(used).to(dev)])
    assert cull_unseen_faces(mesh, fp, f["H"], f["W"], min_views=3).faces.shape[0] == 0


def check_support_depth(dev):
    """a support map equal to the mesh's own depth keeps every count; view 1 moved by more than the tolerance takes one
    off every face seen there; a support of 0 counts nothing"""
    own = render("cube", dev).depth
    plain = visibility("cube", dev)
    assert np.array_equal(visibility("cube", dev, support_depth=own, support_tolerance=0.0), plain)
    moved = own.clone()
    moved[1] += 0.02
    seen_in_1 = fx.expected("cube")[0][1]
    drop = np.zeros_like(plain)
    drop[np.unique(seen_in_1[seen_in_1 >= 0])] = 1
    assert np.array_equal(visibility("cube", dev, support_depth=moved, support_tolerance=0.01), plain - drop)
    assert np.array_equal(visibility("cube", dev, support_depth=moved, support_tolerance=0.03), plain)
    assert not visibility("cube", dev, support_depth=torch.zeros_like(own), support_tolerance=1e9).any()


def check_depth_difference(dev):
    from scorp_amd.mesh import depth_difference
    m = torch.tensor([[[1.0, 2.0, 0.0, 0.0]], [[0.0, 0.0, 3.0, 1.0]]], device=dev)
    r = torch.tensor([[[1.5, 0.0, 2.0, 0.0]], [[0.0, 0.0, 2.0, 2.0]]], device=dev)
    d = depth_difference(m, r)
    assert d.mean_abs.tolist() == [0.5, 1.0] and d.max_abs.tolist() == [0.5, 1.0]
    assert d.reference_covered.tolist() == [0.5, 1.0] and d.mesh_covered.tolist() == [0.5, 1.0]
    assert d.overall == dict(mean_abs=2.5 / 3, max_abs=1.0, reference_covered=0.75, mesh_covered=0.75)
    with pytest.raises(ValueError):
        depth_difference(m, r[:1])
