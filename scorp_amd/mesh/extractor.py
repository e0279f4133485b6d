"""GaussianExtractor: render the views of a trained surfel model, fuse them and mesh the result by either route."""
import os
from functools import partial

import numpy as np
import torch

from ._common import Mesh, _check_method, empty_mesh
from .blocks import extract_surface_blocks, tsdf_blocks_fuse
from .render import cull_unseen_faces, render_mesh
from .smooth import normal_difference, normal_map
from .surface import extract_surface
from .tsdf import MAX_RANGE, tsdf_fuse, uncontract


def focus_point(origins, directions):
    """The point with the least summed squared distance to the rays (origins [n, 3], directions [n, 3], any length or sign):
    with the projectors P_i = I - d_i d_i^T onto each ray's normal plane it solves (sum P_i) x = sum P_i o_i.  What the
    reference's bounding-sphere estimate takes as the scene centre (focus_point_fn, render_utils.py:68-74)."""
    d = directions / np.linalg.norm(directions, axis=1, keepdims=True)
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    return np.linalg.solve(P.sum(0), np.einsum("nij,nj->i", P, origins))


class GaussianExtractor:
    """mesh_utils.py:72-295 GaussianExtractor on this package's 2DGS render():

        ex = GaussianExtractor(gaussians, render, pipe)
        ex.reconstruction(cameras)
        mesh = ex.extract_mesh_unbounded(resolution=1024)
    """

    def __init__(self, gaussians, render, pipe, bg_color=None):
        if bg_color is None:
            bg_color = [0, 0, 0]
        self.gaussians = gaussians
        self.device = gaussians.get_xyz.device
        self.render = partial(render, pipe=pipe, bg_color=torch.tensor(bg_color, dtype=torch.float32, device=self.device))
        self.clean()

    @torch.no_grad()
    def clean(self):
        self.depthmaps = None    # [V, H, W] on the device
        self.rgbmaps = None      # [V, 3, H, W]
        self.full_proj = None    # [V, 4, 4]
        self.normalmaps = None   # [V, 3, H, W], world space, alpha-weighted: only after reconstruction(keep_normals=True)
        self.viewpoint_stack = []

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack, keep_normals=False):
        """Render every camera and keep its colour and surface-depth maps (the 'render' and 'render_depth' keys); with
        keep_normals also its normal map ('render_normal': world space, alpha-weighted) as self.normalmaps, for
        normal_difference."""
        self.clean()
        self.viewpoint_stack = list(viewpoint_stack)
        if not self.viewpoint_stack:
            raise ValueError("reconstruction needs at least one camera")
        depths, rgbs, normals = [], [], []
        for cam in self.viewpoint_stack:
            pkg = self.render(cam, self.gaussians)
            rgb, depth = pkg["render"], pkg["render_depth"]
            if depths and depth.shape != depths[0].shape:
                raise ValueError(f"all views must share one resolution: {tuple(depth.shape)} after {tuple(depths[0].shape)}")
            rgbs.append(rgb)
            depths.append(depth)
            if keep_normals:
                normals.append(pkg["render_normal"])
        self.depthmaps = torch.stack(depths, 0).reshape(len(depths), *depths[0].shape[-2:]).contiguous()
        self.rgbmaps = torch.stack(rgbs, 0).contiguous()
        if keep_normals:
            self.normalmaps = torch.stack(normals, 0).contiguous()
        self.full_proj = torch.stack([cam.full_proj_transform.to(self.device) for cam in self.viewpoint_stack], 0).contiguous()
        self.estimate_bounding_sphere()

    def estimate_bounding_sphere(self):
        """centre = the focus point of the cameras' optical axes, radius = the nearest camera's distance to it
        (mesh_utils.py:124-136).  world_view_transform is stored transposed, so its upper 3x3 holds the camera axes in world
        coordinates as columns: column 2 is the optical axis."""
        axes = np.stack([cam.world_view_transform[:3, 2].detach().cpu().numpy() for cam in self.viewpoint_stack]).astype(np.float64)
        eyes = np.stack([cam.camera_center.detach().cpu().numpy() for cam in self.viewpoint_stack]).astype(np.float64)
        center = focus_point(eyes, axes)
        self.radius = float(np.sqrt(((eyes - center) ** 2).sum(1)).min())
        self.center_host = tuple(float(np.float32(c)) for c in center)   # what the fusion calls take: no device read per call
        self.center = torch.tensor(self.center_host, dtype=torch.float32, device=self.device)

    def _need_maps(self):
        if self.depthmaps is None:
            raise RuntimeError("call reconstruction(viewpoint_stack) first")

    @torch.no_grad()
    def compute_unbounded_tsdf(self, samples, contracted, voxel_size, return_rgb=False):
        """mesh_utils.py:209-247 over the kept views; `contracted`: the samples lie in the contracted unit space of the
        bounding sphere (the reference's inv_contraction is not None).  samples: [M, 3] or a lattice (x, y, z)."""
        self._need_maps()
        return tsdf_fuse(self.depthmaps, self.rgbmaps if return_rgb else None, self.full_proj, samples, voxel_size,
                         contracted=bool(contracted), center=self.center_host, radius=self.radius)

    @torch.no_grad()
    def tsdf_volume(self, resolution, bounds=None):
        """(grid [N, N, N], (x, y, z)): the TSDF over the lattice linspace(-R, R, N)^3 of the contracted space, one dense
        grid.  R defaults to the reference's bound (mesh_utils.py:259-261): the 0.95 quantile of the contracted surfel
        radii plus 0.01, at most 1.9."""
        self._need_maps()
        N = int(resolution)
        if N < 2:
            raise ValueError(f"resolution must be at least 2; got {resolution}")
        if bounds is None:
            n = torch.linalg.vector_norm((self.gaussians.get_xyz.detach() - self.center) / self.radius, dim=-1)
            contracted_n = torch.where(n < 1, n, 2 - 1 / n)   # the norm of the contracted point
            R = min(float(np.quantile(contracted_n.cpu().numpy(), 0.95)) + 0.01, 1.9)
            lo, hi = (-R, -R, -R), (R, R, R)
        else:
            lo, hi = bounds
        coords = tuple(torch.linspace(float(a), float(b), N).to(self.device) for a, b in zip(lo, hi))
        voxel_size = self.radius * 2 / N
        return self.compute_unbounded_tsdf(coords, True, voxel_size), coords

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=1024, method="surface_nets"):
        """mesh_utils.py:182-278: the TSDF volume of the contracted space, its zero surface (`method`: "surface_nets" or
        "marching_cubes", as in extract_surface), the vertices un-contracted and clipped to +-32, coloured by a second fusion
        pass over the vertices."""
        _check_method(method)
        grid, coords = self.tsdf_volume(resolution)
        verts, faces = extract_surface(grid, coords, level=0.0, method=method)
        voxel_size = self.radius * 2 / int(resolution)
        if verts.shape[0] == 0:
            return empty_mesh(verts.device)
        verts = (uncontract(verts) * float(self.radius) + self.center).clamp(-MAX_RANGE, MAX_RANGE)
        _, colors = self.compute_unbounded_tsdf(verts, False, voxel_size, return_rgb=True)
        return Mesh(verts, faces, colors)

    def bounded_views(self, depth_trunc=3, mask_backgrond=True):
        """What extract_mesh_bounded hands to the volume (mesh_utils.py:45-69, 161-175): (depth [V, H, W] with 0 where the
        camera's gt_alpha_mask is below 0.5 - when it has one and masking is asked for - and where it exceeds depth_trunc,
        rgb uint8 [V, H, W, 3] = clip(rgb, 0, 1) * 255 truncated, world_to_cam [V, 3, 4], intrinsics [V, 4]), the last two
        taken as to_cam_open3d takes them from world_view_transform and projection_matrix."""
        self._need_maps()
        depth = self.depthmaps
        V, H, W = depth.shape
        dev = self.device
        alphas = [getattr(cam, "gt_alpha_mask", None) for cam in self.viewpoint_stack]
        drop = depth > float(depth_trunc)
        if mask_backgrond and any(a is not None for a in alphas):   # one stacked mask, no per-view indexing
            ones = torch.ones(H, W, device=dev)
            alpha = torch.stack([a.to(dev).reshape(H, W) if a is not None else ones for a in alphas])
            drop = drop | (alpha < 0.5)
        depth = torch.where(drop, torch.zeros((), dtype=depth.dtype, device=dev), depth)
        ndc2pix = torch.tensor([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]], dtype=torch.float32, device=dev).T
        proj = torch.stack([cam.projection_matrix.to(dev) for cam in self.viewpoint_stack]).float()
        intrins = (proj @ ndc2pix)[:, :3, :3].transpose(1, 2)
        K = torch.stack([intrins[:, 0, 0], intrins[:, 1, 1], intrins[:, 0, 2], intrins[:, 1, 2]], 1)
        E = torch.stack([cam.world_view_transform.to(dev) for cam in self.viewpoint_stack]).float().transpose(1, 2)[:, :3]
        rgb = (self.rgbmaps.clamp(0.0, 1.0) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return depth, rgb, E.contiguous(), K

    @torch.no_grad()
    def extract_mesh_bounded(self, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3, mask_backgrond=True, stride=4,
                             method="surface_nets"):
        """mesh_utils.py:138-180 (the keyword spelling is the reference's): fuse the kept views into a sparse volume of 16^3
        blocks of `voxel_size` voxels, truncation sdf_trunc, depths above depth_trunc dropped, and mesh its zero surface.
        The volume follows the rules written down in include/scorp_gs.h, not Open3D's ScalableTSDFVolume, whose output was
        never available to compare with; the surface is extracted by surface nets unless method="marching_cubes" asks for
        this project's marching cubes (scorp_amd/mc_table.py; its table was not compared with Open3D's either)."""
        _check_method(method)
        depth, rgb, world_to_cam, intrinsics = self.bounded_views(depth_trunc, mask_backgrond)
        return extract_surface_blocks(tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, voxel_size, sdf_trunc, stride=stride),
                                      method=method)

    @torch.no_grad()
    def render_mesh(self, mesh, **kw):
        """render_mesh (render.py) from the views kept by reconstruction(), on their pixel grid: the depth of the result
        compares with self.depthmaps pixel for pixel (depth_difference)."""
        self._need_maps()
        _, H, W = self.depthmaps.shape
        return render_mesh(mesh, self.full_proj, H, W, **kw)

    @torch.no_grad()
    def cull_unseen_faces(self, mesh, min_views=1, depth_tolerance=None):
        """The faces of `mesh` that own a pixel in at least `min_views` of the kept views (cull_unseen_faces, render.py);
        with depth_tolerance only the pixels where the surfel depth map has a value within that distance of the mesh's."""
        self._need_maps()
        _, H, W = self.depthmaps.shape
        return cull_unseen_faces(mesh, self.full_proj, H, W, support_depth=None if depth_tolerance is None else self.depthmaps,
                                 support_tolerance=depth_tolerance, min_views=min_views)

    @torch.no_grad()
    def normal_difference(self, mesh, normals=None):
        """How the orientation of `mesh` differs from the surfel model's own normals in the kept views
        (reconstruction(..., keep_normals=True)): normal_difference (smooth.py) of the mesh's normal map - flat, or
        interpolated from `normals` [Nv, 3] - against self.normalmaps."""
        self._need_maps()
        if self.normalmaps is None:
            raise RuntimeError("call reconstruction(viewpoint_stack, keep_normals=True) first")
        out = self.render_mesh(mesh, colors=False, barycentric=normals is not None)
        return normal_difference(normal_map(out, mesh, normals), self.normalmaps)

    @torch.no_grad()
    def export_image(self, path):
        """mesh_utils.py:280-294: renders/NNNNN.png, vis/depth_NNNNN.tiff and (where the camera has one) gt/NNNNN.png."""
        from PIL import Image
        self._need_maps()
        dirs = {k: os.path.join(path, k) for k in ("renders", "gt", "vis")}
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)
        u8 = lambda img: Image.fromarray((np.clip(np.nan_to_num(img.permute(1, 2, 0).cpu().numpy()), 0.0, 1.0) * 255).astype(np.uint8))
        for idx, cam in enumerate(self.viewpoint_stack):
            gt = getattr(cam, "original_image", None)
            if gt is not None:
                u8(gt[0:3]).save(os.path.join(dirs["gt"], f"{idx:05d}.png"))
            u8(self.rgbmaps[idx]).save(os.path.join(dirs["renders"], f"{idx:05d}.png"))
            Image.fromarray(self.depthmaps[idx].cpu().numpy().astype(np.float32)).save(os.path.join(dirs["vis"], f"depth_{idx:05d}.tiff"))
