"""`blend_forward_wave_kernel` (gs3d_forward.hip, exp_mfma.hpp) against a float64 blend, per pixel, hit lists included.

Each scene of tests/blend_forward_fixtures.py runs once through the C ABI (`scorp_gs3d_preprocess` + `scorp_gs3d_render`),
and `scorp_gs3d_debug_geom`, `scorp_gs3d_debug_tiles` and `scorp_gs3d_debug_blend` hand out the kernel's own records, its
sorted tile lists and what it left behind: final_T, n_contrib, the per-block hit lists and iteration counts.  The float64
blend of tests/blend_forward_reference.py starts from those very records, so every difference is the blend kernel's.
What is asserted (the check functions are the ones tests/test_blend_forward_edges_cpu.py shows to flag twelve planted
defects):
  - the scene shows on the kernel's geometry what it is there for, and at most 5 % of its pixels are ambiguous;
  - colour, depth, alpha and final_T on every kept pixel within 4 x the first-order bound; out_alpha == 1 - final_T bit for
    bit; nothing written outside the three images (guard words round them);
  - n_contrib: 0 exactly where float64 finds no contributor, otherwise hits[n_contrib - 1] is float64's last contributor;
  - each block's hit list up to max n_contrib: only certain or either hits, the certain ones complete and in order, no
    splat twice, block_hits between that length and the tile's;
  - `scorp_gs3d_render_image` gives the three images bit for bit; a second run repeats every bit of all of the above.

The kernel passes as it stands: no fixture found a defect, and no correction to the bound was needed.

Measured on an MI355X, for the record, not bars (worst case of each family; error and bound are the colour image's,
ratio = the largest |error| / bound over colour, depth, alpha and final_T on kept pixels - the bar is 4; e_ref = the
float32 run of the reference against float64; left out = ambiguous pixels):
| family | worst case | colour error | bound | worst ratio | e_ref | most left out |
|---|---|---|---|---|---|---|
| lengths (63 cases) | len1-13x11 | 4.46e-08 | 1.78e-07 | 0.50 | 6.85e-08 | 0 of 64 (len1-8x8) |
| stops (24) | stop16-37x21 | 2.28e-07 | 1.42e-06 | 0.48 | 2.20e-07 | 0 of 64 (stop8-8x8) |
| stops, spread of scales (3) | stops_spread-37x21 | 4.57e-07 | 7.91e-06 | 0.46 | 4.57e-07 | 1 of 64 (stops_spread-8x8) |
| sparse takers (1) | sparse-37x21 | 4.93e-07 | 4.75e-05 | 0.44 | 4.69e-07 | 1 of 777 (sparse-37x21) |
| clamp switch (16) | clamp64-all-37x21 | 3.56e-07 | 6.20e-06 | 0.37 | 3.51e-07 | 0 of 143 (clamp0-all-13x11) |
| indefinite conic (3 of its 4) | indefinite0-37x21 | 3.47e-07 | 6.07e-06 | 0.10 | 3.56e-07 | 1 of 777 (indefinite0-37x21) |
| empty (1) | empty-37x21 | 1.95e-07 | 1.93e-05 | 0.45 | 6.82e-08 | 0 of 777 (empty-37x21) |
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import blend_forward_fixtures as F
from tests import blend_forward_reference as R

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.05
GUARD = 64            # floats in front of and behind each output image (keeps the images 256-byte aligned)
GUARD_VALUE = -12345.0
_runs = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def forward(kw, dev, entry="scorp_gs3d_render", debug=True):
    """preprocess + `entry` through the C ABI into guarded images; with `debug` also the kernel's records, tile lists and
    what the blend left behind, as numpy arrays."""
    from scorp_amd import _C, rasterizer3d as Rz
    L = _C.lib()
    T = lambda a: None if a is None else torch.tensor(np.asarray(a), device=dev)
    N, W, H = kw["means3D"].shape[0], kw["W"], kw["H"]
    s = Rz.GaussianRasterizationSettings(H, W, kw["tanfovx"], kw["tanfovy"], T(kw["bg"]), kw.get("scale_modifier", 1.0),
                                         T(kw["view"]), T(kw["proj"]), kw.get("sh_degree", 0), T(kw["campos"]), False, True)
    ten = {k: T(kw.get(k)) for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")}
    keep = []
    args = Rz._inputs_struct(s, ten["means3D"], ten["shs"], ten["colors_precomp"], ten["opacities"], ten["scales"],
                             ten["rotations"], ten["cov3D_precomp"], keep)
    sb = L.scorp_gs3d_state_bytes(N, W, H)
    state = torch.zeros(sb, dtype=torch.uint8, device=dev)
    radii = torch.empty(N, dtype=torch.int32, device=dev)
    stream = Rz._stream()
    _C.check(L.scorp_gs3d_preprocess(ctypes.byref(args), Rz._ptr(radii), Rz._ptr(state), sb, stream), "preprocess")
    n = ctypes.c_uint64()
    _C.check(L.scorp_gs3d_num_pairs(Rz._ptr(state), stream, ctypes.byref(n)), "num_pairs")
    cap = max(n.value, 1)
    pairs = torch.zeros(L.scorp_gs3d_pairs_bytes(cap), dtype=torch.uint8, device=dev)
    img = {k: torch.full((c * H * W + 2 * GUARD,), GUARD_VALUE, device=dev) for k, c in (("color", 3), ("depth", 1), ("alpha", 1))}
    ptr = {k: v.data_ptr() + 4 * GUARD for k, v in img.items()}
    _C.check(getattr(L, entry)(ctypes.byref(args), Rz._ptr(state), Rz._ptr(pairs), cap, ptr["color"], ptr["depth"], ptr["alpha"],
                               stream), entry)
    torch.cuda.synchronize()
    out = dict(N=N, W=W, H=H, n=n.value)
    for k, v in img.items():
        h = v.cpu().numpy()
        out[k] = h[GUARD:-GUARD].reshape((3, H, W) if k == "color" else (H, W)).copy()
        out[k + "_guard"] = np.concatenate([h[:GUARD], h[-GUARD:]])
    if debug:
        xy = np.zeros((N, 2), np.float32); depth = np.zeros(N, np.float32); conic = np.zeros((N, 4), np.float32)
        rgb = np.zeros((N, 3), np.float32)
        _C.check(L.scorp_gs3d_debug_geom(state.data_ptr(), N, W, H, _p(xy), _p(depth), _p(conic), _p(rgb), None, stream), "debug_geom")
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        ts = np.zeros(tiles + 1, np.uint32); pl = np.zeros(max(n.value, 1), np.uint32)
        _C.check(L.scorp_gs3d_debug_tiles(state.data_ptr(), pairs.data_ptr(), cap, N, W, H, _p(ts), _p(pl), stream), "debug_tiles")
        fT = np.full(H * W, np.nan, np.float32); nc = np.zeros(H * W, np.uint32); bh = np.zeros(tiles * 4, np.uint32)
        hits = np.full(4 * max(n.value, 1), 0xFFFFFFFF, np.uint32)
        _C.check(L.scorp_gs3d_debug_blend(state.data_ptr(), pairs.data_ptr(), cap, N, W, H, _p(fT), _p(nc), _p(bh), _p(hits), stream), "debug_blend")
        assert int(ts[-1]) == n.value
        out.update(geom=dict(xy=xy, depth=depth, conic_o=conic, rgb=rgb), tile_start=ts.astype(np.int64), point_list=pl,
                   final_T=fT.reshape(H, W), n_contrib=nc.reshape(H, W), block_hits=bh, hits=hits)
    return out


def run(name, dev):
    """(kernel outputs, float64 blend, float32 blend, scene conditions) of a fixture: one render, one reference."""
    if name not in _runs:
        kw, want = F.build(name)
        got = forward(kw, dev)
        r64 = R.blend(got["geom"], got["tile_start"], got["point_list"], kw["W"], kw["H"], kw["bg"])
        r32 = R.blend(got["geom"], got["tile_start"], got["point_list"], kw["W"], kw["H"], kw["bg"], dtype=np.float32, with_bound=False)
        _runs[name] = (got, r64, r32, want)
    return _runs[name]


def defined_hits(got):
    """Per block, the prefix of its hit list up to max n_contrib (what the backward replays; the rest is undefined)."""
    W, H, ts = got["W"], got["H"], got["tile_start"]
    tiles_x, num_pairs = (W + 15) // 16, int(ts[-1])
    out = {}
    for t in range(len(ts) - 1):
        for quad in range(4):
            x0, y0 = (t % tiles_x) * 16 + (quad & 1) * 8, (t // tiles_x) * 16 + (quad >> 1) * 8
            blk = got["n_contrib"][y0:y0 + 8, x0:x0 + 8]
            ln = int(blk.max()) if blk.size else 0
            b = quad * num_pairs + int(ts[t])
            out[t, quad] = got["hits"][b:b + ln].copy()
    return out


@pytest.mark.parametrize("name", list(F.FIXTURES))
def test_blend_forward_against_f64(name, dev):
    got, r64, r32, want = run(name, dev)
    ts = got["tile_start"]
    assert F.conditions(name, want, r64, ts) == []
    left_out = int(r64.ambiguous.sum())
    assert left_out <= AMBIGUOUS_CAP * r64.ambiguous.size, f"{name}: {left_out} of {r64.ambiguous.size} pixels ambiguous"
    stats = {}
    found = R.check_images(got, r64, stats=stats)
    keep = ~r64.ambiguous
    e_ref = float(np.where(keep, np.abs(r32.color.astype(np.float64) - r64.color), 0).max())
    print(f"{name}: colour error {stats['color'][0]:.2e}, bound {stats['color'][1]:.2e}, worst ratio "
          f"{max(v[2] for v in stats.values()):.3f} (" + ", ".join(f"{k} {v[2]:.2f}" for k, v in stats.items()) + f"), e_ref {e_ref:.2e}, "
          f"left out {left_out} of {r64.ambiguous.size}")
    assert found == []
    # the epilogue: out_alpha = 1.0f - T, and nothing outside the images
    assert np.array_equal(got["alpha"], np.float32(1.0) - got["final_T"]), "out_alpha is not 1 - final_T bit for bit"
    for k in ("color", "depth", "alpha"):
        assert (got[k + "_guard"] == np.float32(GUARD_VALUE)).all(), f"{k}: written outside the image"
    assert R.check_n_contrib(got, r64, ts) == []
    assert R.check_hit_lists(got, r64, ts) == []


@pytest.mark.parametrize("name", list(F.FIXTURES))
def test_render_image_and_a_second_run_give_the_same_bits(name, dev):
    got = run(name, dev)[0]
    kw, _ = F.build(name)
    img = forward(kw, dev, entry="scorp_gs3d_render_image", debug=False)
    again = forward(kw, dev)
    for k in ("color", "depth", "alpha"):
        assert np.array_equal(img[k].view(np.uint32), got[k].view(np.uint32)), f"scorp_gs3d_render_image: {k} differs from scorp_gs3d_render"
        assert (img[k + "_guard"] == np.float32(GUARD_VALUE)).all(), f"scorp_gs3d_render_image: {k} written outside the image"
        assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), f"second run: {k} differs"
    assert np.array_equal(again["final_T"].view(np.uint32), got["final_T"].view(np.uint32)), "second run: final_T differs"
    for k in ("n_contrib", "block_hits", "tile_start", "point_list"):
        assert np.array_equal(again[k], got[k]), f"second run: {k} differs"
    a, b = defined_hits(again), defined_hits(got)
    assert all(np.array_equal(a[key], b[key]) for key in b), "second run: a hit list differs"
