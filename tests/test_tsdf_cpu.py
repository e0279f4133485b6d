"""TSDF fusion without a GPU: the yardstick's float32 run against its float64 run on the inputs the GPU tests use (no
decision flips among the kept samples, at most 1 % left out), the CPU path of scorp_amd.mesh.tsdf_fuse against the
yardstick, closed forms, and the argument errors."""
import math

import numpy as np
import pytest
import torch

from tests import tsdf_reference as ref

CASES = ("points", "lattice_contracted", "lattice_plain", "colour")


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("views", (5, 1))
def test_float32_restatement_flips_no_decision_among_the_kept_samples(name, views):
    c = ref.case(name, views)
    keep = c["keep"]
    left_out = 1.0 - float(keep.float().mean())
    print(f"{name} V={views}: left out {left_out:.4%}, e_ref {c['e_ref']:.3e}, e_ref_rgb {c['e_ref_rgb']:.3e}")
    assert left_out <= 0.01
    assert torch.equal(c["hits32"][:, keep], c["hits64"][:, keep])
    # the sets are worth fusing: every kind of sample is there
    hit_any = c["hits64"].any(0)
    assert bool(hit_any.any()) and (name == "colour" or not bool(hit_any.all()))
    assert float(c["ref64"].min()) < 0.5   # (with one view: (1 + s) / 2 < 0.5 needs a negative sdf)


def test_scene_has_samples_behind_a_camera_and_outside_a_frustum():
    depth, rgb, fp = ref.scene()
    pts = ref.uncontract(ref.point_samples().double()) * ref.RADIUS + torch.tensor(ref.CENTER, dtype=torch.float64)
    p = torch.cat([pts, torch.ones_like(pts[:, :1])], -1) @ fp[3].double()
    assert 0.1 < float((p[:, 3] <= 0).float().mean()) < 0.9
    p = torch.cat([pts, torch.ones_like(pts[:, :1])], -1) @ fp[4].double()
    pix = p[:, :2] / p[:, 3:]
    assert float(((pix.abs() >= 1).any(-1) & (p[:, 3] > 0)).float().mean()) > 0.1


@pytest.mark.parametrize("name", CASES)
def test_cpu_path_matches_the_yardstick(name):
    from scorp_amd.mesh import tsdf_fuse
    c = ref.case(name)
    depth, rgb, fp = ref.scene()
    samples = c["coords"] if c["coords"] is not None else c["samples"]
    tsdf, col = tsdf_fuse(depth, rgb, fp, samples, ref.VOXEL, contracted=c["contracted"], **c["kw"])
    keep = c["keep"]
    err = float((tsdf.reshape(-1).double() - c["ref64"])[keep].abs().max())
    err_rgb = float((col.reshape(-1, 3).double() - c["rgb64"])[keep].abs().max())
    print(f"{name}: cpu path {err:.3e} (e_ref {c['e_ref']:.3e}), rgb {err_rgb:.3e} (e_ref_rgb {c['e_ref_rgb']:.3e})")
    assert err <= 4 * c["e_ref"]
    assert err_rgb <= 4 * c["e_ref_rgb"]
    if c["coords"] is not None:
        assert tsdf.shape == tuple(x.numel() for x in c["coords"]) and col.shape == tsdf.shape + (3,)
        only = tsdf_fuse(depth, None, fp, samples, ref.VOXEL, contracted=c["contracted"], **c["kw"])
        assert torch.equal(only, tsdf)


def _axis_camera(distance):
    from scorp_amd.camera import look_at_camera
    return look_at_camera((-distance, 0.0, 0.0), (0, 0, 0), (0, 0, 1), math.radians(50.0), (8, 6))


def test_one_view_one_sample_at_known_depth():
    from scorp_amd.mesh import tsdf_fuse
    cam = _axis_camera(5.0)
    voxel = 0.1   # trunc 0.5
    for offset, s in ((0.25, 0.5), (-0.2, -0.4), (2.0, 1.0)):
        depth = torch.full((1, 6, 8), 5.0 + offset)    # the sample at the origin has zc = 5
        rgb = torch.full((1, 3, 6, 8), 0.6)
        tsdf, col = tsdf_fuse(depth, rgb, cam.full_proj_transform[None], torch.zeros(1, 3), voxel)
        assert abs(float(tsdf) - (1 + s) / 2) < 1e-6
        assert torch.allclose(col, torch.full((1, 3), 0.3), atol=1e-6)   # (0 * 1 + 0.6) / 2
    # behind the surface by more than trunc: no update
    tsdf = tsdf_fuse(torch.full((1, 6, 8), 4.0), None, cam.full_proj_transform[None], torch.zeros(1, 3), voxel)
    assert float(tsdf) == 1.0


def test_sample_seen_by_no_view_keeps_its_initial_state():
    from scorp_amd.mesh import tsdf_fuse
    cam = _axis_camera(5.0)
    samples = torch.tensor([[-9.0, 0.0, 0.0], [0.0, 40.0, 0.0], [-5.0, 0.0, 0.0]])   # behind, outside the frustum, zc = 0
    tsdf, col = tsdf_fuse(torch.full((2, 6, 8), 5.0), torch.rand(2, 3, 6, 8), cam.full_proj_transform[None].repeat(2, 1, 1),
                          samples, 0.1)
    assert torch.equal(tsdf, torch.ones(3)) and torch.equal(col, torch.zeros(3, 3))


@pytest.mark.parametrize("norm, factor", [(0.5, 1.0), (1.5, 2.0), (1.95, 10.0)])
def test_trunc_scales_with_the_contracted_norm(norm, factor):
    """trunc = 5 voxel / (2 - min(n, 1.9)) beyond n = 1 (clamped at 1.9): a surface half a trunc behind the sample gives 0.75."""
    from scorp_amd.mesh import tsdf_fuse
    cam = _axis_camera(60.0)
    voxel, radius = 0.02, 2.0
    world_x = (norm if norm < 1 else 1.0 / (2.0 - norm)) * radius
    trunc = 5 * voxel * factor
    depth = torch.full((1, 6, 8), float(60.0 + world_x + 0.5 * trunc))
    tsdf = tsdf_fuse(depth, None, cam.full_proj_transform[None], torch.tensor([[norm, 0.0, 0.0]]), voxel, contracted=True,
                     center=(0.0, 0.0, 0.0), radius=radius)
    # zc and the depth are ~100: a few ulp(128) = 7.6e-6 each, over trunc >= 0.1 and halved - under 1e-3; a wrong factor
    # (no scaling, or 1 / (2 - 1.95) = 20 without the clamp) moves the value by 0.1 or more
    assert abs(float(tsdf) - 0.75) < 1e-3


def test_argument_errors():
    from scorp_amd.mesh import tsdf_fuse
    depth, rgb, fp = ref.scene()
    pts = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="voxel_size"):
        tsdf_fuse(depth, None, fp, pts, 0.0)
    with pytest.raises(ValueError, match="center and radius"):
        tsdf_fuse(depth, None, fp, pts, 0.1, contracted=True)
    with pytest.raises(ValueError, match="radius"):
        tsdf_fuse(depth, None, fp, pts, 0.1, contracted=True, center=(0, 0, 0), radius=0.0)
    with pytest.raises(ValueError, match="rgb must be"):
        tsdf_fuse(depth, rgb[:, :, :-1], fp, pts, 0.1)
    with pytest.raises(ValueError, match="full_proj"):
        tsdf_fuse(depth, None, fp[:-1], pts, 0.1)
    with pytest.raises(ValueError, match="at least 2 x 2"):
        tsdf_fuse(depth[:, :1], None, fp, pts, 0.1)
    with pytest.raises(ValueError, match="no samples"):
        tsdf_fuse(depth, None, fp, torch.zeros(0, 3), 0.1)
    with pytest.raises(ValueError, match="samples must be"):
        tsdf_fuse(depth, None, fp, torch.zeros(4, 2), 0.1)
    with pytest.raises(ValueError, match="lattice"):
        tsdf_fuse(depth, None, fp, (torch.zeros(3), torch.zeros(3)), 0.1)


def test_c_abi_refuses_bad_arguments():
    """scorp_tsdf_fuse validates before any HIP call: the dummy pointers are never dereferenced, no GPU is needed."""
    import ctypes
    from scorp_amd import _C
    L = _C.lib()
    d = 0x10000

    def call(views=None, samples=None, params=None, out=d, out_rgb=None):
        v = _C.ScorpTsdfViews(depth=d, rgb=None, full_proj=d, num_views=2, width=8, height=6)
        s = _C.ScorpTsdfSamples(xyz=d, first=0, count=10)
        p = _C.ScorpTsdfParams(voxel_size=0.1, contracted=0, radius=0.0)
        for obj, kw in ((v, views), (s, samples), (p, params)):
            for k, val in (kw or {}).items():
                setattr(obj, k, val)
        return L.scorp_tsdf_fuse(ctypes.byref(v), ctypes.byref(s), ctypes.byref(p), out, out_rgb, None)
    for kw, text in ((dict(views=dict(num_views=0)), b"num_views"), (dict(views=dict(width=1)), b"width"),
                     (dict(views=dict(depth=None)), b"NULL"), (dict(samples=dict(count=0)), b"count"),
                     (dict(samples=dict(xyz=None)), b"neither points nor a lattice"),
                     (dict(samples=dict(xyz=None, x=d, y=d, z=d, nx=2, ny=2, nz=2, count=9)), b"past the end"),
                     (dict(params=dict(voxel_size=0.0)), b"voxel_size"), (dict(params=dict(contracted=1)), b"radius"),
                     (dict(out=None), b"NULL"), (dict(out_rgb=d), b"out_rgb without")):
        assert call(**kw) == _C.ERR_INVALID, kw
        assert text in L.scorp_last_error(), (kw, L.scorp_last_error())
