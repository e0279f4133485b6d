"""GaussianExtractor.extract_mesh_bounded end to end on the scene of tests/test_mesh_gpu.py: about 2 000 opaque surfels on a unit
sphere, 8 ring cameras at 96 x 80, reconstruction -> extract_mesh_bounded(voxel_size=0.05, sdf_trunc=0.2, depth_trunc=6) ->
post_process_mesh -> write_mesh_ply -> read back.  What a blurred render should give is fixed by nothing here, so the geometry
is held only to what the rules promise: a vertex lies between voxels that some view wrote near its depth.  The median
vertex radius of the first run is recorded in DESIGN.md 4.12."""
import numpy as np
import pytest
import torch

from tests.test_mesh_gpu import sphere_surfels

pytestmark = pytest.mark.gpu

VOXEL, TRUNC, DEPTH_TRUNC = 0.05, 0.2, 6


@pytest.fixture(scope="module")
def extractor():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from scorp_amd.mesh import GaussianExtractor
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    model = GaussianModel2D.from_raw(sphere_surfels(), 0, device=dev)
    model.active_sh_degree = 0
    pipe = PipelineParams()
    pipe.depth_ratio = 0.0
    ex = GaussianExtractor(model, render, pipe)
    ex.reconstruction(ring_cameras(8, 96, 80, 3, radius=4.0, device=dev))
    return ex


def _depth_points(depth, world_to_cam, intrinsics):
    """The world points of every pixel with a measurement, [n, 3]."""
    V, H, W = depth.shape
    v, u = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32),
                          torch.arange(W, device=depth.device, dtype=torch.float32), indexing="ij")
    pts = []
    for i in range(V):
        fx, fy, cx, cy = (float(x) for x in intrinsics[i])
        d = depth[i]
        p_cam = torch.stack([(u - cx) * d / fx, (v - cy) * d / fy, d], -1)[d > 0]
        R, t = world_to_cam[i, :, :3], world_to_cam[i, :, 3]
        pts.append((p_cam - t) @ R)      # R^T (p_cam - t), row-vector form
    return torch.cat(pts)


def test_surfel_sphere_to_bounded_mesh_and_ply(extractor, tmp_path):
    from scorp_amd.mesh import Mesh, post_process_mesh
    from scorp_amd.ply import read_mesh_ply, write_mesh_ply
    mesh = extractor.extract_mesh_bounded(voxel_size=VOXEL, sdf_trunc=TRUNC, depth_trunc=DEPTH_TRUNC)
    assert isinstance(mesh, Mesh)
    v, f, c = mesh.vertices, mesh.faces, mesh.colors
    assert v.shape[0] > 0 and f.shape[0] > 0 and c.shape == v.shape
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(c).all())
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0
    pts = _depth_points(*[t for i, t in enumerate(extractor.bounded_views(DEPTH_TRUNC)) if i != 1])
    nearest = torch.cat([torch.cdist(v[i:i + 1024], pts).min(1).values for i in range(0, v.shape[0], 1024)])
    print(f"bounded mesh: {v.shape[0]} vertices, {f.shape[0]} faces, median vertex radius {float(v.norm(dim=1).median()):.4f}, "
          f"largest distance to a depth point {float(nearest.max()):.4f}")
    assert float(nearest.max()) <= TRUNC
    cleaned = post_process_mesh(mesh, cluster_to_keep=1)
    assert 0 < cleaned.faces.shape[0] <= f.shape[0] and int(cleaned.faces.max()) < cleaned.vertices.shape[0]
    path = str(tmp_path / "bounded.ply")
    write_mesh_ply(path, mesh)
    rv, rf, rc = read_mesh_ply(path)
    assert np.array_equal(rv, v.cpu().numpy()) and np.array_equal(rf, f.cpu().numpy())
    assert np.array_equal(rc, np.rint(c.cpu().numpy().astype(np.float64) * 255).astype(np.uint8))
    # the reference's defaults are accepted as keywords, its spelling included
    assert isinstance(extractor.extract_mesh_bounded(voxel_size=VOXEL, sdf_trunc=TRUNC, depth_trunc=DEPTH_TRUNC, mask_backgrond=False), Mesh)


def test_depth_trunc_and_quantised_colours(extractor):
    depth, rgb, world_to_cam, intrinsics = extractor.bounded_views(3.5)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (8, 80, 96, 3)
    assert torch.equal(rgb, (extractor.rgbmaps.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1))
    assert float(depth.max()) <= 3.5 and bool(((extractor.depthmaps > 3.5) == ((depth == 0) & (extractor.depthmaps != 0))).all())
    cam = extractor.viewpoint_stack[0]
    assert torch.allclose(world_to_cam[0].cpu(), cam.world_view_transform.T[:3].cpu())
    fx = 96 / (2 * np.tan(cam.FoVx / 2))
    assert abs(float(intrinsics[0, 0]) - fx) < 1e-3 * fx and abs(float(intrinsics[0, 2]) - 47.5) < 1e-3 and abs(float(intrinsics[0, 3]) - 39.5) < 1e-3


def test_masked_pixels_touch_no_block(extractor):
    """With gt_alpha_mask zero on the left half of every view the volume is the one fused from depth maps whose left halves
    were cleared by hand: no block exists through a masked pixel."""
    from scorp_amd.mesh import tsdf_blocks_fuse
    depth, rgb, world_to_cam, intrinsics = extractor.bounded_views(DEPTH_TRUNC)
    full = tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, VOXEL, TRUNC)
    alpha = torch.ones(1, 80, 96, device=depth.device)
    alpha[..., :48] = 0.0
    try:
        for cam in extractor.viewpoint_stack:
            cam.gt_alpha_mask = alpha
        masked_depth = extractor.bounded_views(DEPTH_TRUNC)[0]
        assert not bool(masked_depth[..., :48].any()) and torch.equal(masked_depth[..., 48:], depth[..., 48:])
        assert torch.equal(extractor.bounded_views(DEPTH_TRUNC, mask_backgrond=False)[0], depth)
        mesh = extractor.extract_mesh_bounded(voxel_size=VOXEL, sdf_trunc=TRUNC, depth_trunc=DEPTH_TRUNC)
    finally:
        for cam in extractor.viewpoint_stack:
            del cam.gt_alpha_mask
    by_hand = depth.clone()
    by_hand[..., :48] = 0
    want = tsdf_blocks_fuse(by_hand, rgb, world_to_cam, intrinsics, VOXEL, TRUNC)
    got = tsdf_blocks_fuse(masked_depth, rgb, world_to_cam, intrinsics, VOXEL, TRUNC)
    assert torch.equal(got.keys, want.keys) and torch.equal(got.view_mask, want.view_mask) and torch.equal(got.tsdf, want.tsdf)
    bits = lambda vol: int(sum(((vol.view_mask[:, 0] >> i) & 1).sum() for i in range(8)))
    assert 0 < got.keys.numel() <= full.keys.numel() and 0 < bits(got) < bits(full)   # fewer (block, view) pairs than unmasked
    # every block of the masked volume is reached from an unmasked pixel: within sdf_trunc (per axis) of its point
    pts = _depth_points(by_hand, world_to_cam, intrinsics)
    lo, hi = got.coords.float() * (16 * VOXEL) - TRUNC - 1e-4, (got.coords.float() + 1) * (16 * VOXEL) + TRUNC + 1e-4
    reached = ((pts[None] >= lo[:, None]) & (pts[None] <= hi[:, None])).all(-1).any(1)
    assert bool(reached.all())
    from scorp_amd.mesh import extract_surface_blocks
    assert torch.equal(mesh.vertices, extract_surface_blocks(want).vertices)
