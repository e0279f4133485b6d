"""The bounded TSDF route without a GPU: the yardstick's float32 run against its float64 run on the scene the GPU tests fuse
(no decision flips among the kept voxels, at most 1 % left out), the numpy form of scorp_amd.mesh.tsdf_blocks_fuse /
extract_surface_blocks against the yardstick, the yardstick's surface against the dense extractor on a full box, and the
argument errors.

Scene (tests/tsdf_blocks_reference.py): a unit sphere over the plane z = -0.6, five cameras at distance 3 looking at the
origin, 48 x 40 pixels, voxel_length 0.05, sdf_trunc 0.2, stride 4.  Two things about it are decided here and written down:
  * the analytic depth has a range of 6; beyond it a ray measures nothing.  The rays near the horizon meet the plane up to
    1 300 units away, where a float32 coordinate resolves 6e-5 and no float32 statement holds a margin of 1e-5;
  * the plane's points put the lower face of their touch boxes, z = -0.6 - 0.2, ON the block face z = -16 * 0.05: whether the
    36 blocks below it exist hangs on the last bits of p_w.z, in float64 as in float32.  So the touch decisions get the
    same treatment as the voxels': the yardstick brackets them (boxes widened / narrowed by 1e-5 max(1, d)), block keys and
    view masks must be EQUAL in every bit outside the bracket, a voxel that an undecided bit would write is left out (none
    is, in this scene), and a block that was free not to exist must hold no written kept voxel.
Measured here: 134 blocks may exist, 81 must (the float32 forms give 98); 23.2 % of the voxels observed, 0.113 % left out,
e_ref 3.4e-6 (tsdf) and 5.1e-6 (colour, of 255), no weight differing among the kept voxels."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tsdf_blocks_reference as ref


def _fuse(depth, rgb, cam, voxel_length=ref.VOXEL, sdf_trunc=ref.TRUNC, stride=ref.STRIDE, device="cpu", **kw):
    from scorp_amd.mesh import tsdf_blocks_fuse
    t = lambda a: torch.from_numpy(a).to(device)
    return tsdf_blocks_fuse(t(depth), t(rgb) if rgb is not None else None, t(cam[:, :12].reshape(-1, 3, 4)), t(cam[:, 12:]),
                            voxel_length, sdf_trunc, stride, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(num_views=1), dict(shift=(-7.0, -7.0, -7.0)), dict(blank_view=2)], ids=str)
def test_float32_restatement_flips_no_decision_among_the_kept_voxels(kw):
    c = ref.case(**kw)
    left_out = 1.0 - float(c["keep"].mean())
    undecided = int(np.unpackbits((c["mask"] & ~c["sure"]).view(np.uint8)).sum())
    print(f"{kw}: {c['keys'].size} blocks may exist, {int(c['sure'].any(1).sum())} must, {undecided} view bits undecided, float32 touch "
          f"{c['keys32'].size}; observed {float((c['w64'] > 0).mean()):.3%}, left out {left_out:.4%}, e_ref {c['e_ref']:.3e}, "
          f"e_ref_colour {c['e_ref_colour']:.3e}")
    assert left_out <= 0.01
    assert np.array_equal(c["w32"][c["keep"]], c["w64"][c["keep"]])
    ref.match_blocks(c, c["keys32"], c["mask32"])
    assert 0.05 < float((c["w64"] > 0).mean()) < 0.9 and float(c["tsdf64"].min()) < -0.5 and float(c["tsdf64"].max()) == 1.0


def test_scene_covers_the_rules_edges():
    c = ref.case()
    depth, _, _ = ref.inputs()
    assert (depth == 0).any() and (depth > 0).any()                       # pixels without a measurement
    coords = np.array([ref.coords_of(int(k)) for k in c["keys"]])
    assert coords.min() < 0 <= coords.max()                                # blocks on both sides of the origin
    assert len({int(m) for m in c["mask"][:, 0]}) > 5                       # blocks seen by different sets of views
    assert float(c["w64"].max()) >= 3.0                                     # voxels several views write
    shifted = np.array([ref.coords_of(int(k)) for k in ref.case(shift=(-7.0, -7.0, -7.0))["keys"]])
    assert shifted.max() < 0                                                # every block at negative coordinates


@pytest.mark.parametrize("kw", [dict(), dict(num_views=1), dict(shift=(-7.0, -7.0, -7.0)), dict(blank_view=2)], ids=str)
def test_numpy_form_matches_the_yardstick(kw):
    c = ref.case(**kw)
    vol = _fuse(*ref.inputs(**kw))
    err, err_colour = ref.compare_volume(c, vol.keys.numpy(), vol.view_mask.numpy(), vol.tsdf.numpy(), vol.weight.numpy(), vol.colour.numpy())
    print(f"{kw}: numpy form {err:.3e} (e_ref {c['e_ref']:.3e}), colour {err_colour:.3e} (e_ref_colour {c['e_ref_colour']:.3e})")
    assert vol.coords.dtype == torch.int32 and np.array_equal(vol.coords.numpy(), [ref.coords_of(int(k)) for k in vol.keys])
    if not kw:
        only = _fuse(ref.inputs()[0], None, ref.inputs()[2])
        assert only.colour is None and torch.equal(only.tsdf, vol.tsdf) and torch.equal(only.weight, vol.weight)


def test_one_block_and_closed_forms():
    depth, rgb, cam, vl, trunc, stride = ref.one_block_inputs()
    vol = _fuse(depth, rgb, cam, vl, trunc, stride)
    assert vol.keys.tolist() == [ref.key_of((0, 0, 0))] and vol.view_mask.tolist() == [[1]]
    c = ref.fuse_case(depth, rgb, cam, vl, trunc, stride)
    ref.compare_volume(c, vol.keys.numpy(), vol.view_mask.numpy(), vol.tsdf.numpy(), vol.weight.numpy(), vol.colour.numpy())
    # the voxel (8, 8, gz) lies on the optical axis: sdf = 8 - (gz + 0.5) over a truncation of 0.5
    t, w = vol.tsdf.reshape(16, 16, 16)[8, 8], vol.weight.reshape(16, 16, 16)[8, 8]
    assert t[:7].tolist() == [1.0] * 7 and w[:8].tolist() == [1.0] * 8     # in front of the plane: free space
    assert abs(float(t[7]) - 1.0) < 1e-6                                    # sdf = +0.5: min(1, 1)
    assert w[8:].tolist() == [0.0] * 8 and t[8:].tolist() == [0.0] * 8     # sdf = -0.5 is not > -sdf_trunc: never written


def test_surface_yardstick_matches_the_dense_extractor_and_the_numpy_form():
    """On a full box with every weight positive the block rules ARE the dense rules: the yardstick's loops give the mesh of
    scorp_amd.mesh._surface_nets_numpy over the gathered grid (vertex for vertex through their cells, the faces as a set).  The numpy form of
    extract_surface_blocks is held to the yardstick index for index on every hand-made volume."""
    from scorp_amd.mesh import BlockVolume, _surface_nets_numpy, block_coords, extract_surface_blocks
    for name, (blocks, vl) in ref.surface_cases().items():
        rv, rf, rc = ref.surface_blocks(blocks, vl)
        keys, tsdf, w, col = ref.volume_arrays(blocks)
        k = torch.from_numpy(keys)
        m = extract_surface_blocks(BlockVolume(k, block_coords(k), None, torch.from_numpy(tsdf), torch.from_numpy(w), torch.from_numpy(col), vl))
        assert np.array_equal(m.faces.numpy(), rf) and m.vertices.shape[0] == rv.shape[0] > 0, name
        assert np.abs(m.vertices.numpy() - rv).max() <= 1e-5 * vl + 2 * 2.0 ** -23 * np.abs(rv).max(), name
        assert np.abs(m.colors.numpy() - rc).max() <= 2.0 ** -20, name
        if all(wt.all() for _, wt, _ in blocks.values()) and len(blocks) == np.prod(np.ptp(np.array(sorted(blocks)), 0) + 1):
            T, g0 = ref.gather_dense(blocks)
            coords = [(vl * (np.arange(n) + g0[d] + 0.5)).astype(np.float32) for d, n in enumerate(T.shape)]
            dv, df = _surface_nets_numpy(T, coords, 0.0)
            assert len(dv) == len(rv) and len(df) == len(rf), name
            cells = ref.surface_blocks(blocks, vl, return_cells=True)[3]
            to_dense = np.empty(len(rv), np.int64)   # the dense extractor numbers its vertices by ascending (i, j, k)
            to_dense[np.lexsort(cells[:, ::-1].T)] = np.arange(len(rv))
            assert np.abs(dv[to_dense] - rv).max() <= 1e-5 * vl + 2 * 2.0 ** -23 * np.abs(rv).max(), name
            rows = lambda f: f[np.lexsort(f[:, ::-1].T)]
            assert np.array_equal(rows(df.astype(np.int64)), rows(to_dense[rf])), name
    hole, full = ref.surface_cases()["sphere_hole"][0], ref.surface_cases()["sphere_8_blocks"][0]
    assert len(ref.surface_blocks(hole, ref.SURFACE_VOXEL)[0]) < len(ref.surface_blocks(full, ref.SURFACE_VOXEL)[0])


def test_empty_views_give_an_empty_volume_and_mesh():
    from scorp_amd.mesh import extract_surface_blocks
    depth, rgb, cam = ref.inputs()
    vol = _fuse(np.zeros_like(depth), rgb, cam)
    assert vol.keys.numel() == 0 and tuple(vol.tsdf.shape) == (0, 4096)
    m = extract_surface_blocks(vol)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.colors.shape == (0, 3)


def test_argument_errors():
    depth, rgb, cam = ref.inputs()
    with pytest.raises(ValueError, match="voxel_length"):
        _fuse(depth, rgb, cam, voxel_length=0.0)
    with pytest.raises(ValueError, match="sdf_trunc"):
        _fuse(depth, rgb, cam, sdf_trunc=0.0)
    with pytest.raises(ValueError, match="sdf_trunc"):
        _fuse(depth, rgb, cam, voxel_length=0.01, sdf_trunc=0.17)   # > 16 voxel_length
    with pytest.raises(ValueError, match="stride"):
        _fuse(depth, rgb, cam, stride=0)
    with pytest.raises(ValueError, match="rgb must be"):
        _fuse(depth, rgb[:, :, :-1], cam)
    with pytest.raises(ValueError, match="world_to_cam"):
        _fuse(depth, rgb, cam[:-1])
    far = depth.copy()
    far[0, 0, 0] = 3e38
    with pytest.raises(ValueError, match="outside the volume's range"):
        _fuse(far, rgb, cam)


def test_c_abi_refuses_bad_arguments():
    """Every call validates before any HIP call: the dummy pointers are never dereferenced, no GPU is needed."""
    from scorp_amd import _C
    L = _C.lib()
    d = 0x10000

    def views(**kw):
        v = _C.ScorpTsdfBlockViews(depth=d, rgb=None, cam=d, num_views=2, width=8, height=6)
        for k, val in kw.items():
            setattr(v, k, val)
        return ctypes.byref(v)
    touch = lambda v=None, vl=0.1, tr=0.2, stride=4, keys=d, mask=d, slots=64, over=d: \
        L.scorp_tsdf_blocks_touch(v or views(), vl, tr, stride, keys, mask, slots, over, None)
    integ = lambda v=None, vl=0.1, tr=0.2, keys=d, mask=d, B=3, t=d, w=d, c=None: \
        L.scorp_tsdf_blocks_integrate(v or views(), vl, tr, keys, mask, B, t, w, c, None)
    calls = [
        (lambda: touch(v=views(num_views=0)), b"num_views"), (lambda: touch(v=views(depth=None)), b"NULL"),
        (lambda: touch(stride=0), b"stride"), (lambda: touch(vl=0.0), b"voxel_length"), (lambda: touch(tr=0.0), b"sdf_trunc"),
        (lambda: touch(tr=1.7), b"sdf_trunc"), (lambda: touch(slots=48), b"power of two"), (lambda: touch(slots=0), b"power of two"),
        (lambda: touch(keys=None), b"NULL"), (lambda: touch(over=None), b"NULL"),
        (lambda: integ(v=views(num_views=0)), b"num_views"), (lambda: integ(B=0), b"num_blocks"), (lambda: integ(t=None), b"NULL"),
        (lambda: integ(c=d), b"out_colour without"), (lambda: integ(vl=-1.0), b"voxel_length"), (lambda: integ(tr=2.0), b"sdf_trunc"),
        (lambda: L.scorp_tsdf_blocks_neighbors(None, 3, d, None), b"NULL"), (lambda: L.scorp_tsdf_blocks_neighbors(d, 0, d, None), b"num_blocks"),
        (lambda: L.scorp_isosurface_blocks_count_cells(d, d, None, 3, d, None), b"NULL"),
        (lambda: L.scorp_isosurface_blocks_count_cells(d, d, d, 0, d, None), b"num_blocks"),
        (lambda: L.scorp_isosurface_blocks_emit_vertices(d, d, None, d, d, 3, 0.1, d, 2 ** 31, d, None, None), b"num_vertices"),
        (lambda: L.scorp_isosurface_blocks_emit_vertices(d, d, None, d, d, 3, 0.1, d, 5, d, d, None), b"out_colours without"),
        (lambda: L.scorp_isosurface_blocks_emit_vertices(d, d, None, d, d, 3, 0.0, d, 5, d, None, None), b"voxel_length"),
        (lambda: L.scorp_isosurface_blocks_count_faces(d, None, d, 3, d, None), b"NULL"),
        (lambda: L.scorp_isosurface_blocks_emit_faces(d, d, d, 3, d, d, 0, d, None), b"num_quads"),
        (lambda: L.scorp_isosurface_blocks_emit_faces(d, d, d, 3, d, d, 2 ** 31, d, None), b"num_quads"),
        (lambda: L.scorp_isosurface_blocks_emit_faces(d, d, d, 3, None, d, 5, d, None), b"NULL"),
    ]
    for i, (call, text) in enumerate(calls):
        assert call() == _C.ERR_INVALID, i
        assert text in L.scorp_last_error(), (i, L.scorp_last_error())
