"""The bodies the CPU and GPU test files of scorp_amd/mesh/distance.py share: each takes the device to run on
("cpu": the numpy form, "cuda": csrc/mesh_distance.hip) and asserts against tests/mesh_distance_reference.py."""
import functools

import numpy as np
import pytest
import torch

from tests import icp_probe_fixtures as icp_fx
from tests import mesh_distance_fixtures as fx
from tests import mesh_distance_reference as ref


def mesh_of(verts, faces, dev):
    from scorp_amd.mesh import Mesh
    v = torch.from_numpy(np.array(verts)).to(dev)
    return Mesh(v, torch.from_numpy(np.array(faces)).to(dev), torch.zeros(v.shape[0], 3, device=dev))


def run(name, dev, rows=slice(None), header=None):
    from scorp_amd.mesh import point_mesh_distance
    verts, faces, q, r = fx.fixture(name)
    out = point_mesh_distance(torch.from_numpy(np.array(q[rows])).to(dev), mesh_of(verts, faces, dev), r, header=header)
    assert all(t.device.type == dev for t in out)
    return tuple(t.cpu().numpy() for t in out)


def check_fixture(name, dev):
    header = []
    worst = fx.judge(name, *run(name, dev, header=header))
    print(f"{name} on {dev}: largest |d^2 - yardstick| = {worst:.3g} D^2 (tolerance {fx.TOL_REL:.3g} D^2)" +
          (f", grid {header[0]}" if header else ""))
    if header:
        h = header[0]
        F = len(fx.fixture(name)[1])
        from scorp_amd.mesh import PAIR_CAP_FACTOR, PAIR_CAP_FLOOR
        assert h["pair_cap"] == PAIR_CAP_FACTOR * F + PAIR_CAP_FLOOR == 8 * F + 4096 and h["pairs"] <= h["pair_cap"] and h["cells"] <= h["cell_cap"]
        assert h["cells"] == h["dim_x"] * h["dim_y"] * h["dim_z"]
        if name == "scene_sized":
            assert h["grow"] > 0, "two scene-sized triangles over a fine grid: the cap must have grown the cell"
    return worst


def check_block_edges(count, dev):
    rows = slice(0, count)
    fx.judge("flat", *run("flat", dev, rows), rows=rows)


def check_determinism(dev):
    """the same call twice, the queries shuffled, the queries split over two calls: bit-equal"""
    name = "scene_sized"
    a = run(name, dev)
    b = run(name, dev)
    Q = len(a[0])
    perm = np.random.default_rng(5).permutation(Q)
    from scorp_amd.mesh import point_mesh_distance
    verts, faces, q, r = fx.fixture(name)
    mesh = mesh_of(verts, faces, dev)
    shuffled = tuple(t.cpu().numpy() for t in point_mesh_distance(torch.from_numpy(q[perm].copy()).to(dev), mesh, r))
    half = Q // 2 - 7
    parts = [tuple(t.cpu().numpy() for t in point_mesh_distance(torch.from_numpy(np.array(part)).to(dev), mesh, r))
             for part in (q[:half], q[half:])]
    for k, what in enumerate(("squared_distance", "face", "closest")):
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: two calls differ"
        un = np.empty_like(shuffled[k])
        un[perm] = shuffled[k]
        assert np.array_equal(a[k], un, equal_nan=True), f"{what}: depends on the queries' order"
        assert np.array_equal(a[k], np.concatenate([parts[0][k], parts[1][k]]), equal_nan=True), f"{what}: depends on the split"


def check_limits(dev):
    from scorp_amd.mesh import Mesh, empty_mesh, point_mesh_distance
    verts, faces, q, _ = fx.fixture("faces2")
    mesh = mesh_of(verts, faces, dev)
    pts = np.array(q[:8])
    pts[1, 0], pts[3, 2], pts[5, 1] = np.nan, np.inf, -np.inf
    out = point_mesh_distance(torch.from_numpy(pts).to(dev), mesh)
    bad = np.array([0, 1, 0, 1, 0, 1, 0, 0], bool)
    assert np.array_equal(out.face.cpu().numpy() < 0, bad)
    assert torch.isinf(out.squared_distance[torch.from_numpy(bad).to(dev)]).all()
    good = fx.ref.brute_force(pts[~bad], verts, faces)
    assert np.array_equal(out.face.cpu().numpy()[~bad], good[1])
    assert torch.equal(out.distance, out.squared_distance.sqrt())
    none = point_mesh_distance(torch.from_numpy(pts).to(dev), empty_mesh(torch.device(dev)))      # an empty mesh: all misses
    assert (none.face == -1).all() and torch.isinf(none.squared_distance).all() and torch.isnan(none.closest).all()
    empty = point_mesh_distance(torch.empty(0, 3, device=dev), mesh)                              # Q = 0: empty outputs
    assert empty.squared_distance.shape == (0,) and empty.face.shape == (0,) and empty.closest.shape == (0, 3)
    assert empty.squared_distance.dtype == torch.float64 and empty.face.dtype == torch.int32
    with pytest.raises(ValueError, match="max_distance"):
        point_mesh_distance(torch.from_numpy(pts).to(dev), mesh, -1.0)
    with pytest.raises(ValueError, match="max_distance"):
        point_mesh_distance(torch.from_numpy(pts).to(dev), mesh, float("nan"))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        point_mesh_distance(torch.zeros(4, 2, device=dev), mesh)
    broken = mesh.vertices.clone()
    broken[2, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        point_mesh_distance(torch.from_numpy(pts).to(dev), Mesh(broken, mesh.faces, mesh.colors))
    with pytest.raises(ValueError, match="vertex index"):
        point_mesh_distance(torch.from_numpy(pts).to(dev), Mesh(mesh.vertices, mesh.faces + 5, mesh.colors))


# ---- the sampler ----

def unequal_mesh():
    """the flat mesh with its y coordinates squared: areas from 0.1 to 6, plus one face of zero area"""
    verts, faces = fx._flat_mesh(31)
    v = np.array(verts)
    v[:, 1] = v[:, 1] ** 2 * 0.4
    v[:, 2] += 0.1 * v[:, 0]
    f = np.concatenate([faces[:7], [[3, 3, 9]], faces[7:]]).astype(np.int32)
    return v.astype(np.float32), f


def check_sampler(dev):
    from scorp_amd.mesh import point_mesh_distance, sample_points_uniformly, triangle_area_prefix
    verts, faces = unequal_mesh()
    mesh = mesh_of(verts, faces, dev)
    F = len(faces)
    n = 64 * F
    prefix = triangle_area_prefix(mesh)
    assert prefix.dtype == torch.float64 and prefix.shape == (F,)
    s = sample_points_uniformly(mesh, n, seed=3, area_prefix=prefix)
    pts, chosen, bary = s.points.cpu().numpy(), s.faces.cpu().numpy(), s.barycentric.cpu().numpy()
    assert pts.dtype == np.float32 and chosen.dtype == np.int32 and bary.dtype == np.float32
    want_p, want_f, want_w = ref.sample(verts, faces, prefix.cpu().numpy(), n, 3)
    assert np.array_equal(chosen, want_f)
    assert (np.abs(pts - want_p) <= np.spacing(np.abs(want_p).astype(np.float32))).all()
    assert (np.abs(bary - want_w) <= np.spacing(np.abs(want_w).astype(np.float32))).all()
    assert (np.diff(chosen) >= 0).all()                       # stratified: the face index never falls
    assert not (chosen == 7).any()                            # the face of zero area
    # Stratification: sample i's area coordinate lies in slice i of n equal slices of the total area, so N(y), the number
    # of samples below the area coordinate y, is floor or ceil of n y / A: within one of it.  The samples of a face are
    # N(prefix[f]) - N(prefix[f - 1]), hence between floor(n a / A) - 1 and ceil(n a / A) + 1: within one of the expected
    # count rounded outward (independent draws would scatter like its square root).
    p = prefix.cpu().numpy()
    area = np.diff(p, prepend=0.0)
    expect = n * area / p[-1]
    count = np.bincount(chosen, minlength=F)
    assert (count >= np.floor(expect) - 1).all() and (count <= np.ceil(expect) + 1).all(), (count - expect)
    # every point lies on its face: its distance to that single-face mesh is below 4 ulp of the extent
    extent = float(np.ptp(verts, axis=0).max())
    lim = 4.0 * float(np.spacing(np.float32(extent)))
    for f in (0, 5, 20, F - 1):
        mine = torch.from_numpy(pts[chosen == f]).to(dev)
        assert len(mine) > 0
        d = point_mesh_distance(mine, mesh_of(verts, faces[f:f + 1], dev)).distance
        assert float(d.max()) <= lim, (f, float(d.max()), lim)
    _, d_on = ref.on_faces(pts, verts, faces, chosen)
    assert np.sqrt(d_on.max()) <= lim
    again = sample_points_uniformly(mesh, n, seed=3)          # (the default prefix is triangle_area_prefix)
    assert torch.equal(again.points, s.points) and torch.equal(again.faces, s.faces) and torch.equal(again.barycentric, s.barycentric)
    other = sample_points_uniformly(mesh, n, seed=4)
    assert not torch.equal(other.points, s.points)
    assert sample_points_uniformly(mesh, 0).points.shape == (0, 3)
    with pytest.raises(ValueError, match="no area"):
        sample_points_uniformly(mesh_of(*fx.fixture("collinear")[:2], dev), 10)
    return s


# ---- nearest point of a cloud ----

def check_nearest(name, dev):
    """the slack rule and the 5 % cap of tests/test_icp_search_gpu.py on one of tests/icp_probe_fixtures.py's shapes"""
    from scorp_amd.mesh import nearest_point_distance
    tgt, q, r, (i1, d1, d2, _) = icp_fx.fixture(name)
    out = nearest_point_distance(torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(tgt)).to(dev), r)
    idx, got = out.index.cpu().numpy(), out.squared_distance.cpu().numpy()
    assert idx.dtype == np.int32 and got.dtype == np.float64
    E, delta = icp_fx.slack(tgt, q)
    t64, q64 = tgt.astype(np.float64), q.astype(np.float64)
    hit = idx >= 0
    d_chosen = np.linalg.norm(q64[hit] - t64[idx[hit]], axis=1)
    assert np.allclose(np.sqrt(got[hit]), d_chosen, rtol=1e-12, atol=0.0) and np.isinf(got[~hit]).all()
    assert (d_chosen <= r * (1.0 + 1e-12)).all() and (d_chosen <= d1[hit] + delta).all()
    assert (d1[~hit] > r - delta).all()
    margin = icp_fx.has_margin(d1, d2, r, delta)
    assert np.mean(~margin) <= icp_fx.MARGIN_CAP
    _, lowest = icp_fx.positions_of(tgt)
    want = np.where(d1 <= r, lowest[i1], -1)
    assert np.array_equal(idx[margin], want[margin])


def check_nearest_ties(dev):
    """duplicated points: the lowest original index among the tied ones, for every query"""
    from scorp_amd.mesh import nearest_point_distance
    for shuffle in (0, 1):
        tgt, q, r, (i1, d1, _, _), _ = icp_fx.ties_fixture(shuffle)
        out = nearest_point_distance(torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(tgt)).to(dev), r)
        assert np.array_equal(out.index.cpu().numpy(), i1)
    pts = torch.tensor([[0.0, 0, 0], [float("nan"), 0, 0], [9.0, 0, 0]], device=dev)
    out = nearest_point_distance(pts, torch.tensor([[0.0, 0, 1]], device=dev), 2.0)
    assert out.index.tolist() == [0, -1, -1] and out.squared_distance[0] == 1.0
    assert nearest_point_distance(torch.empty(0, 3, device=dev), pts[:1]).index.shape == (0,)
    with pytest.raises(ValueError, match="finite"):
        nearest_point_distance(pts, pts)


# ---- the metrics ----

def square(side, z, dev, n=5, offset=0.0):
    c = np.linspace(0.0, side, n) + offset
    x, y = np.meshgrid(c, c, indexing="ij")
    v = np.stack([x, y, np.full(x.shape, z)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, cc, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return mesh_of(v, np.concatenate([np.stack([a, b, cc], 1), np.stack([a, cc, d], 1)]).astype(np.int32), dev)


def check_metrics(dev):
    from scorp_amd.mesh import mesh_cloud_distance, mesh_distance, sample_points_uniformly
    a, b = square(1.0, 0.0, dev), square(1.0, 0.25, dev)
    m = mesh_distance(a, b, samples=2000, thresholds=(0.2, 0.3))
    for v in (m.accuracy, m.completeness, m.chamfer, m.hausdorff_ab, m.hausdorff_ba):
        assert v == pytest.approx(0.25, abs=1e-7)             # (0.25 and the fp32 samples' z are exact; the sqrt is not)
    assert m.f_score == (0.0, 1.0) and m.precision == (0.0, 1.0) and m.recall == (0.0, 1.0)
    assert m.samples_a == 2000 and m.samples_b == 2000 and m.thresholds == (0.2, 0.3)
    # a unit square inside a 2 x 2 square of the same plane: every sample of the small one is on the large one, not the reverse
    small, large = square(1.0, 0.0, dev, offset=0.5), square(2.0, 0.0, dev)
    m = mesh_distance(small, large, samples=3000, seed=7)
    assert m.accuracy <= 1e-7 and m.hausdorff_ab <= 1e-6
    sb = sample_points_uniformly(large, 3000, 8).points.cpu().numpy()
    want = np.sqrt(ref.brute_force(sb, small.vertices.cpu().numpy(), small.faces.cpu().numpy())[0])
    assert m.completeness > 0.05
    assert m.completeness == pytest.approx(want.mean(), rel=1e-9) and m.hausdorff_ba == pytest.approx(want.max(), rel=1e-9)
    assert m.chamfer == pytest.approx(0.5 * (m.accuracy + m.completeness), rel=1e-15)
    # a mesh against itself
    verts, faces = fx.sphere_mesh()
    sphere = mesh_of(verts, faces, dev)
    extent = float(np.ptp(verts, axis=0).max())
    m = mesh_distance(sphere, sphere, samples=1500, thresholds=(1e-5 * extent,))
    assert m.chamfer <= 1e-6 * extent and m.f_score == (1.0,)
    # a mesh against a scan of it
    cloud = sample_points_uniformly(sphere, 3000, 9).points
    m = mesh_cloud_distance(sphere, cloud, samples=1500, thresholds=(0.1,))
    assert m.completeness <= 1e-6 * extent and 0.0 < m.accuracy < 0.1 and m.samples_b == 3000 and m.f_score == (1.0,)


def check_nets_against_cubes(dev):
    """Surface nets against marching cubes of one sphere grid: a surface-nets vertex lies in a cell the marching-cubes
    surface crosses, and every marching-cubes triangle in a cell that holds a surface-nets vertex whose faces reach it, so no
    point of either surface is farther than two cell diagonals, 2 sqrt(3) h, from the other."""
    from scorp_amd.mesh import mesh_distance
    n = 14
    h = 2.6 / (n - 1)
    nets, cubes = mesh_of(*fx.sphere_mesh("surface_nets", n), dev), mesh_of(*fx.sphere_mesh("marching_cubes", n), dev)
    m = mesh_distance(nets, cubes, samples=2000)
    print(f"surface nets against marching cubes on {dev}: chamfer {m.chamfer / h:.4f} h, Hausdorff {m.hausdorff_ab / h:.4f} / "
          f"{m.hausdorff_ba / h:.4f} h")
    assert 0.0 < m.hausdorff_ab <= 2.0 * np.sqrt(3.0) * h and 0.0 < m.hausdorff_ba <= 2.0 * np.sqrt(3.0) * h
    return m


@functools.lru_cache(maxsize=None)
def cpu_samples():
    """the CPU form's samples of unequal_mesh(), for the GPU file's comparison"""
    from scorp_amd.mesh import sample_points_uniformly
    verts, faces = unequal_mesh()
    return sample_points_uniformly(mesh_of(verts, faces, "cpu"), 64 * len(faces), seed=3)
