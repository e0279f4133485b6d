"""The mask vote (scorp_gs3d_mask_vote / scorp_gs2d_mask_vote, scorp_amd.segment) on the GPU: S_in / S_out against the CPU
oracle's colour gradients, its invariants, the reference's get_mask3d loop restated through autograd, determinism, the
read-only contract and the edges of the public API."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_oracle2d_cpu import make_case2d
from tests.util import assert_no_further_from_f64, make_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


CASES_3D = {
    "sh3_bg_mod": dict(N=3000, W=160, H=120, deg=3, seed=1, bg=(0.2, 0.5, 0.7), scale_modifier=1.3),
    "tiny_splats": dict(N=20000, W=256, H=192, deg=3, seed=5, log_scale=math.log(0.006)),
    "huge_splats": dict(N=6000, W=64, H=64, deg=0, seed=6, log_scale=math.log(0.6)),
    "precomp_cov": dict(N=3000, W=96, H=96, deg=0, seed=4, precomp_cov=True),
    "odd_size": dict(N=4000, W=137, H=91, deg=2, seed=2),
}
CASES_2D = {
    "sh3_bg": dict(N=3000, W=160, H=120, deg=3, seed=1, bg=(0.2, 0.5, 0.7)),
    "tiny_surfels": dict(N=20000, W=256, H=192, deg=1, seed=5, log_scale=math.log(0.006)),
    "scale_mod": dict(N=2000, W=96, H=96, deg=1, seed=8, scale_modifier=1.4),
    "odd_size": dict(N=4000, W=137, H=91, deg=2, seed=2, log_scale=math.log(0.06)),
}


def seeded_masks(H, W, seed, blobs=3):
    """[blobs + 3, H, W] bool: random discs, one all-ones mask, one empty mask, one with a ragged (random-walk) border."""
    rng = np.random.default_rng(seed + 555)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(blobs):
        m = np.zeros((H, W), bool)
        for _ in range(3):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.1, 0.35) * min(H, W)
            m |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
        out.append(m)
    out.append(np.ones((H, W), bool))
    out.append(np.zeros((H, W), bool))
    edge = np.clip(W // 2 + np.cumsum(rng.integers(-3, 4, H)), 0, W)
    out.append(xx < edge[:, None])
    return np.stack(out)


def ones_colour(kw):
    kw = dict(kw)
    kw.pop("shs", None)
    kw.pop("sh_degree", None)
    kw["colors_precomp"] = np.ones((kw["means3D"].shape[0], 3), np.float32)
    return kw


def kw_case(kind, name):
    kw, _ = make_case(**CASES_3D[name]) if kind == "3d" else make_case2d(**CASES_2D[name])
    return ones_colour(kw)


def hip_votes(kind, kw, masks, method="sums", dev=None, out=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from scorp_amd.rasterizer3d import _GS2D, _GS3D
    from scorp_amd.refcall import _settings
    from scorp_amd.segment import view_votes
    T = lambda a: None if a is None else torch.tensor(a, device=dev)
    cov = kw.get("cov3D_precomp")
    return view_votes(_GS3D if kind == "3d" else _GS2D, _settings(GaussianRasterizationSettings, kw, T, False),
                      T(kw["means3D"]), T(kw["opacities"].reshape(-1, 1)), torch.as_tensor(masks), method,
                      scales=T(kw.get("scales")), rotations=T(kw.get("rotations")), cov3D_precomp=T(cov), out=out)


def oracle_sums(kind, kw, masks, dtype):
    """(S_in, S_out) [K, N] from the oracle's colour gradient under dL/dcolor = mask (resp. 1 - mask) in channel 0."""
    from oracle.gs_oracle import OracleRender, OracleRender2D
    o = (OracleRender if kind == "3d" else OracleRender2D)(dtype, **kw)
    res = []
    for m in masks:
        row = []
        for mm in (m, ~m):
            dc = np.zeros((3,) + m.shape, dtype)
            dc[0] = mm
            row.append(o.backward(dL_dcolor=dc)["colors_precomp"][:, 0])
        res.append(row)
    return np.asarray(res, np.float64)   # [K, 2, N]


@pytest.mark.parametrize("kind,name", [("3d", n) for n in CASES_3D] + [("2d", n) for n in CASES_2D])
def test_vote_sums_match_oracle(kind, name, dev):
    kw = kw_case(kind, name)
    masks = seeded_masks(kw["H"], kw["W"], 7)
    got = hip_votes(kind, kw, masks, "sums", dev).cpu().numpy().astype(np.float64)
    r32, r64 = oracle_sums(kind, kw, masks, np.float32), oracle_sums(kind, kw, masks, np.float64)
    for k in range(len(masks)):
        for s, side in enumerate(("in", "out")):
            assert_no_further_from_f64(f"{kind}/{name} mask {k} S_{side}", got[k, s], r32[k, s], r64[k, s])


@pytest.mark.parametrize("kind", ["3d", "2d"])
def test_vote_invariants(kind, dev):
    name = "sh3_bg_mod" if kind == "3d" else "sh3_bg"
    kw = kw_case(kind, name)
    H, W = kw["H"], kw["W"]
    masks = seeded_masks(H, W, 3)
    sums = hip_votes(kind, kw, masks, "sums", dev)
    ones_k, empty_k = len(masks) - 3, len(masks) - 2
    assert (sums[ones_k, 1] == 0).all() and (sums[empty_k, 0] == 0).all()
    # sum_i S_in of the all-ones mask = sum_p alpha(p) of the same render
    from scorp_amd.refcall import render2d_reference_call, render3d_reference_call
    with torch.no_grad():
        if kind == "3d":
            alpha = render3d_reference_call(kw, dev, requires_grad=False)[0][3]
        else:
            alpha = render2d_reference_call(kw, dev, requires_grad=False)[0][2][1]
    a = float(alpha.double().sum())
    assert abs(float(sums[ones_k, 0].double().sum()) - a) <= 1e-5 * a
    # binary votes are integers in [-V, V] after V views
    out = None
    for v in range(3):
        out = hip_votes(kind, kw, masks, "binary", dev, out=out)
    b = out.cpu().numpy()
    assert (b == np.round(b)).all() and np.abs(b).max() <= 3


class _Pipe:   # the reference's PipelineParams defaults (no python-side branches)
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def _model(kind, N, seed, dev, deg=3):
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.renderer2d import GaussianModel2D
    from scorp_amd.synthetic import make_gaussians
    cls = GaussianModel if kind == "3d" else GaussianModel2D
    raw = make_gaussians(N, deg, seed, log_scale_mean=math.log(0.04), scale_dims=3 if kind == "3d" else 2)
    g = cls.from_raw(raw, deg, device=dev)
    g.active_sh_degree = deg
    return g


def reference_get_mask3d_votes(kind, g, cams, masks, method):
    """This repository's restatement of utils/mask.py:42-100: a render with override_color = ones, then per object two
    backward passes (mask, inverted mask) through autograd with retain_graph, voting on |colors.grad|."""
    from scorp_amd import renderer, renderer2d
    from scorp_amd.rasterizer3d import backward_precision
    render = renderer.render if kind == "3d" else renderer2d.render
    N, dev = g.get_xyz.shape[0], g.get_xyz.device
    bg = torch.zeros(3, device=dev)
    votes = torch.zeros((len(masks[0]), N), device=dev)
    with backward_precision("deterministic"):
        for cam, ms in zip(cams, masks):
            colors = torch.ones((N, 3), requires_grad=True, device=dev)
            img = render(cam, g, _Pipe(), bg, override_color=colors)["render"]
            img.permute(1, 2, 0).mean().backward(retain_graph=True)
            for k, m in enumerate(torch.as_tensor(ms, device=dev)):
                for sign, mm in ((1.0, m), (-1.0, ~m)):
                    colors.grad.zero_()
                    (img.permute(1, 2, 0) * mm[..., None]).mean().backward(retain_graph=True)
                    n = colors.grad.norm(dim=1)
                    votes[k] += sign * (n if method == "gradient" else (n > 0).float())
    return votes


@pytest.mark.parametrize("kind", ["3d", "2d"])
def test_reference_semantics(kind, dev):
    from scorp_amd.segment import get_mask3d, mask_votes
    from scorp_amd.synthetic import ring_cameras
    W, H = 128, 96
    g = _model(kind, 4000, 11, dev)
    cams = ring_cameras(5, W, H, 11, device=dev)
    masks = [seeded_masks(H, W, 20 + i, blobs=3)[:3] for i in range(5)]
    for method in ("gradient", "binary"):
        got = mask_votes(g, cams, masks, method)
        ref = reference_get_mask3d_votes(kind, g, cams, masks, method)
        if method == "binary":
            assert torch.equal(got, ref)
        else:
            assert float((got - ref).abs().sum() / ref.abs().sum()) < 1e-4
            margin = 1e-5 * float(ref.abs().max())
            decided = ref.abs() > margin
            assert torch.equal((got > 0)[decided], (ref > 0)[decided])
    assert torch.equal(get_mask3d(g, cams, masks, "binary"), ref > 0)


@pytest.mark.parametrize("kind", ["3d", "2d"])
def test_determinism_and_chunking(kind, dev):
    kw = kw_case(kind, "sh3_bg_mod" if kind == "3d" else "sh3_bg")
    H, W = kw["H"], kw["W"]
    masks = np.concatenate([seeded_masks(H, W, 40), seeded_masks(H, W, 41)[:5]])   # K = 11: two passes of eight
    assert len(masks) == 11
    a = hip_votes(kind, kw, masks, "gradient", dev)
    b = hip_votes(kind, kw, masks, "gradient", dev)
    assert torch.equal(a, b)
    for k in range(11):
        one = hip_votes(kind, kw, masks[k:k + 1], "gradient", dev)[0]
        den = float(one.abs().sum())
        assert float((a[k] - one).abs().sum()) <= 1e-6 * max(den, 1e-30)
        decided = one.abs() > 1e-5 * float(one.abs().max() if den > 0 else 0.0)
        assert torch.equal((a[k] > 0)[decided], (one > 0)[decided])


def _c_render(kind, kw, dev):
    """preprocess + render (the form that leaves hit lists) through the C ABI; -> (args, state, pairs, capacity, keep)."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import _GS2D, _GS3D, _inputs_struct, _preprocess, _ptr, _stream
    from scorp_amd.refcall import _settings
    K = _GS3D if kind == "3d" else _GS2D
    T = lambda a: None if a is None else torch.tensor(a, device=dev)
    keep = [T(kw["means3D"]), T(kw["colors_precomp"]), T(kw["opacities"].reshape(-1, 1)), T(kw.get("scales")),
            T(kw.get("rotations")), T(kw.get("cov3D_precomp"))]
    args = _inputs_struct(_settings(GaussianRasterizationSettings, kw, T, False), keep[0], None, *keep[1:], keep)
    N, H, W = kw["means3D"].shape[0], kw["H"], kw["W"]
    _, state, pairs, cap, _ = _preprocess(K, args, N, H, W, dev, _stream(), True)
    maps = [torch.empty((c, H, W), device=dev) for c in K.maps]
    color = torch.empty((3, H, W), device=dev)
    _C.check(getattr(_C.lib(), K.render)(ctypes.byref(args), _ptr(state), _ptr(pairs), cap, _ptr(color), *map(_ptr, maps),
                                         _stream()), K.render)
    return K, args, state, pairs, cap, keep + [color] + maps


@pytest.mark.parametrize("kind", ["3d", "2d"])
def test_vote_leaves_state_and_pairs_unchanged(kind, dev):
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import _ptr, _stream
    kw = kw_case(kind, "sh3_bg_mod" if kind == "3d" else "sh3_bg")
    K, args, state, pairs, cap, keep = _c_render(kind, kw, dev)
    N, H, W = kw["means3D"].shape[0], kw["H"], kw["W"]
    L = _C.lib()
    rng = np.random.default_rng(3)
    gc = torch.tensor(rng.normal(0, 1, (3, H, W)).astype(np.float32), device=dev)
    flags = _C.BACKWARD_DETERMINISTIC

    def backward():
        g = {"colors_precomp": torch.empty((N, 3), device=dev), "opacities": torch.empty((N, 1), device=dev),
             "means3D": torch.empty((N, 3), device=dev)}
        grads = _C.ScorpGs3dGrads()
        for f, t in g.items():
            setattr(grads, f, _ptr(t))
        nb = getattr(L, K.backward_scratch_bytes_ex)(N, W, H, cap, flags)
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        maps = [None] * len(K.maps)
        _C.check(getattr(L, K.backward_ex)(ctypes.byref(args), _ptr(state), _ptr(pairs), cap, _ptr(gc), *maps,
                                           ctypes.byref(grads), _ptr(scratch), nb, flags, _stream()), K.backward_ex)
        return g

    before = backward()
    st0, pr0 = state.clone(), pairs.clone()
    masks = torch.tensor(seeded_masks(H, W, 9), device=dev, dtype=torch.uint8)
    out = torch.zeros((len(masks), N), device=dev)
    nb = L.scorp_mask_vote_scratch_bytes(N, W, H, cap)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    fn = "scorp_gs3d_mask_vote" if kind == "3d" else "scorp_gs2d_mask_vote"
    _C.check(getattr(L, fn)(ctypes.byref(args), _ptr(state), _ptr(pairs), cap, _ptr(masks), len(masks), _C.VOTE_GRADIENT,
                            ctypes.c_float(1.0), _ptr(out), _ptr(scratch), nb, _stream()), fn)
    assert torch.equal(state, st0) and torch.equal(pairs, pr0)
    after = backward()
    for f in before:
        assert torch.equal(before[f], after[f]), f
    # the C-level checks
    bad = lambda **o: getattr(L, fn)(ctypes.byref(args), _ptr(state), _ptr(pairs), cap, o.get("masks", _ptr(masks)),
                                     o.get("k", len(masks)), o.get("method", 0), ctypes.c_float(1.0), _ptr(out),
                                     _ptr(scratch), o.get("nb", nb), _stream())
    assert bad(k=0) == -1   # SCORP_ERR_INVALID
    assert bad(method=3) == -1 and bad(nb=nb - 256) == -1 and bad(masks=None) == -1


def test_edges(dev, tmp_path):
    from scorp_amd.rasterizer3d import _GS3D
    from scorp_amd.segment import mask_votes, view_votes
    from scorp_amd.synthetic import ring_cameras
    kw = kw_case("3d", "sh3_bg_mod")
    H, W = kw["H"], kw["W"]
    masks = seeded_masks(H, W, 1)
    # N = 0
    kw0 = dict(kw, means3D=kw["means3D"][:0], opacities=kw["opacities"][:0], scales=kw["scales"][:0],
               rotations=kw["rotations"][:0], colors_precomp=kw["colors_precomp"][:0])
    z = hip_votes("3d", kw0, masks, "gradient", dev)
    assert z.shape == (len(masks), 0)
    # a camera that sees nothing: every Gaussian behind it
    campos = kw["campos"].astype(np.float64)
    behind = dict(kw, means3D=(kw["means3D"] * 0.01 + 3.0 * campos).astype(np.float32))
    assert (hip_votes("3d", behind, masks, "sums", dev) == 0).all()
    with pytest.raises(ValueError):
        hip_votes("3d", kw, masks[:, :-1], "gradient", dev)
    with pytest.raises(ValueError, match="projection"):
        hip_votes("3d", kw, masks, "projection", dev)
    g = _model("3d", 500, 2, dev)
    cams = ring_cameras(2, W, H, 2, device=dev)
    with pytest.raises(ValueError):
        mask_votes(g, cams, [masks], "gradient")            # one mask set for two cameras
    with pytest.raises(ValueError, match="projection"):
        mask_votes(g, cams, [masks, masks], "projection")


# SH degree 0 as well: post_refine_gs.py reuses apply_mask3d on SH-0 objects, whose _features_rest is [N, 0, 3]
@pytest.mark.parametrize("deg", [3, 0])
@pytest.mark.parametrize("kind", ["3d", "2d"])
def test_segment_writes_object_and_remainder_plys(kind, deg, dev, tmp_path):
    from scorp_amd.ply import read_gaussian_ply, read_ply_vertices
    from scorp_amd.segment import apply_mask3d, segment
    from scorp_amd.synthetic import ring_cameras
    W, H = 96, 80
    g = _model(kind, 3000, 5, dev, deg)
    cams = ring_cameras(3, W, H, 5, device=dev)
    masks = lambda cam: seeded_masks(H, W, 100 + cam.uid, blobs=2)[:2]
    out_dir = tmp_path / "seg"
    m3d = segment(g, cams, masks, ["cup", "plate"], str(out_dir))
    assert m3d.shape == (2, 3000) and m3d.any()
    files = sorted(os.listdir(out_dir))
    assert files == ["cup.ply", "plate.ply", "remained.ply"]
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ply_attributes.json")))
    key = {("3d", 3): "sh3_3d", ("3d", 0): "sh0_3d", ("2d", 3): "sh3_2d"}.get((kind, deg))
    if key is not None:
        attributes = gold[key]["attributes"]
    else:   # (no golden list for this kind and degree: the attributes the model's own save_ply writes)
        g.save_ply(str(tmp_path / "full.ply"))
        attributes = list(read_ply_vertices(str(tmp_path / "full.ply")).dtype.names)
    rows = {"xyz": g._xyz, "opacity": g._opacity, "scaling": g._scaling, "rotation": g._rotation,
            "features_dc": g._features_dc, "features_rest": g._features_rest}
    for f, sel in (("cup.ply", m3d[0]), ("plate.ply", m3d[1]), ("remained.ply", ~m3d.any(0))):
        p = str(out_dir / f)
        assert list(read_ply_vertices(p).dtype.names) == attributes
        raw = read_gaussian_ply(p, deg)
        assert raw["xyz"].shape[0] == int(sel.sum())
        for k, t in rows.items():
            np.testing.assert_array_equal(raw[k], t.detach()[sel].cpu().numpy().reshape(raw[k].shape), err_msg=f"{f} {k}")
    # the clone apply_mask3d returns: the selected rows, max_radii2D zeroed
    clone = apply_mask3d(g, m3d[0], str(tmp_path / "clone.ply"), return_clone_gs=True)
    assert type(clone) is type(g) and clone.active_sh_degree == deg
    assert torch.equal(clone.max_radii2D, torch.zeros(int(m3d[0].sum()), device=dev))
    for k, t in rows.items():
        assert torch.equal(getattr(clone, "_" + k), t.detach()[m3d[0]]), k
    # an empty selection (an object nobody claimed) writes a PLY with no rows
    apply_mask3d(g, torch.zeros(3000, dtype=torch.bool, device=dev), str(tmp_path / "none.ply"))
    raw = read_gaussian_ply(str(tmp_path / "none.ply"), deg)
    assert raw["xyz"].shape == (0, 3) and raw["features_rest"].shape == (0, (deg + 1) ** 2 - 1, 3)
