"""tests/aux_reference.py held against independent formulations where there is no GPU (torch on the CPU, the golden
Wigner-D table, sort-based restatements), and the argument refusals of the helper entry points, which return before any
HIP call.

Measured here (torch CPU, float32, 6 steps, eps 1e-15 and 1e-8, an lr change mid-run): `adam_step32` is NOT bit-equal to
torch.optim.Adam - torch's lerp_ / addcmul_ fuse a multiply-add - but within one ulp in every element (132 / 67 / 2 of 1890
elements of exp_avg / exp_avg_sq / param differ); the test asserts that distance."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import aux_reference as ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "wigner_d.npz")


# ---- Adam -------------------------------------------------------------------------------------------------------------
_ADAM_SHAPES = ((33,), (7, 3), (1,), (260,))
_ADAM_LR = (1.6e-4, 2.5e-3, 0.05, 0.001)


def _torch_adam_run(dtype, eps, steps=6):
    """torch.optim.Adam (single-tensor path) and the yardstick side by side; yields per step and parameter
    (torch p, m, v), (state handed to the yardstick: p, g, m, v), lr, step."""
    rng = np.random.default_rng(11)
    ps = [torch.nn.Parameter(torch.tensor(rng.normal(0, 1, s), dtype=dtype)) for s in _ADAM_SHAPES]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, _ADAM_LR)], lr=0.0, betas=(0.9, 0.999), eps=eps,
                           foreach=False)
    for it in range(1, steps + 1):
        before = []
        for p in ps:
            g = rng.normal(0, 1, p.shape) * 10.0 ** rng.uniform(-8, 2, p.shape)
            g.reshape(-1)[::3] = 0.0
            p.grad = torch.tensor(g, dtype=dtype)
            st = opt.state[p]
            m0 = st["exp_avg"].numpy().copy() if st else np.zeros(p.shape)
            v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(p.shape)
            before.append((p.detach().numpy().copy(), p.grad.numpy().copy(), m0, v0))
        lrs = [grp["lr"] for grp in opt.param_groups]
        opt.step()
        for p, b, lr in zip(ps, before, lrs):
            st = opt.state[p]
            assert int(st["step"]) == it
            yield (p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()), b, lr, it
        if it == 3:
            opt.param_groups[0]["lr"] = 3e-5          # update_learning_rate mid-run
            opt.param_groups[2]["lr"] = 0.2


@pytest.mark.parametrize("eps", (1e-15, 1e-8))
def test_adam_step64_is_torch_adam_in_float64(eps):
    worst = 0.0
    for (tp, tm, tv), (p, g, m, v), lr, step in _torch_adam_run(torch.float64, eps):
        rp, rm, rv = ref.adam_step64(p, g, m, v, lr, 0.9, 0.999, eps, step)
        for a, b in ((rp, tp), (rm, tm), (rv, tv)):
            np.testing.assert_allclose(a, b, rtol=1e-14, atol=0)
            worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
    print(f"adam_step64 vs torch float64, eps {eps}: worst relative difference {worst:.3g}")


@pytest.mark.parametrize("eps", (1e-15, 1e-8))
def test_adam_step32_against_torch_adam_in_float32(eps):
    """Bit-equality was the expectation and does not hold: torch's CPU lerp_ and addcmul_ round once where the
    operation order rounds twice (a fused multiply-add), so exp_avg and exp_avg_sq sit within one ulp (of the larger
    operand of the sum) of `adam_step32`, and the parameter follows: linear in exp_avg's difference, 8 ulp of the update for
    the root, the two host constants torch forms differently (a quotient by sqrt(bc2) against a product with the rounded
    reciprocal, lr / bc1 rounded once against twice) and the quotient, one ulp for the parameter's own rounding.
    Measured: 132 / 67 / 2 of 1890 elements of m / v / p not bit-equal, none further than 1 ulp."""
    unequal, total, worst = [0, 0, 0], 0, [0.0, 0.0, 0.0]
    w = np.float32(1.0 - 0.9)
    for (tp, tm, tv), (p, g, m, v), lr, step in _torch_adam_run(torch.float32, eps):
        rp, rm, rv = ref.adam_step32(p, g, m, v, np.float32(lr), 0.9, 0.999, eps, step)
        f = lambda a: a.astype(np.float64)
        dm, dv, dp = np.abs(f(rm) - f(tm)), np.abs(f(rv) - f(tv)), np.abs(f(rp) - f(tp))
        m_unit = ref.ulp32(np.maximum(np.maximum(np.abs(m), np.abs(tm)), np.abs((g - m) * w)))
        assert np.all(dm <= m_unit), f"exp_avg, step {step}"
        assert np.all(dv <= ref.ulp32(tv)), f"exp_avg_sq, step {step}"
        update = np.abs(f(rp) - f(p))
        carried = np.where(rm != 0, update * dm / np.maximum(np.abs(f(rm)), 1e-300), 0.0)
        assert np.all(dp <= ref.ulp32(tp) + 8 * ref.ulp32(update) + carried), f"param, step {step}"
        for i, (a, b, d, unit) in enumerate(((rm, tm, dm, m_unit), (rv, tv, dv, ref.ulp32(tv)), (rp, tp, dp, ref.ulp32(tp)))):
            unequal[i] += int((a.view(np.int32) != b.view(np.int32)).sum())
            worst[i] = max(worst[i], float((d / unit).max()))
        total += rp.size
    print(f"adam_step32 vs torch float32, eps {eps}: {unequal} of {total} elements of m / v / p not bit-equal, worst {worst} ulp")


def test_adam_step32_stays_next_to_adam_step64_on_the_gpu_inputs():
    """The float32 yardstick on the inputs of the GPU sweep: within a few ulp of the float64 one (it is a bar, so it must
    not be loose itself), subnormal squares included."""
    for tiny in (False, True):
        p, g = ref.adam_inputs(4097, 4097, tiny)
        m, v = np.zeros_like(p), np.zeros_like(p)
        for step in (1, 2, 3):
            m_in = m
            p64, m64, v64 = ref.adam_step64(p, g, m, v, float(np.float32(1e-3)), 0.9, 0.999, 1e-15, step)
            p, m, v = ref.adam_step32(p, g, m, v, np.float32(1e-3), 0.9, 0.999, 1e-15, step)
            # (four: the float constants (float)beta2, (float)(1 - beta2), ... are half an ulp off each, three roundings)
            assert np.all(np.abs(m - m64) <= 4 * ref.ulp32(np.maximum(np.abs(m64), np.abs(m_in))))
            assert np.all(np.abs(p - p64) <= 4 * ref.ulp32(p64))
            assert np.all(np.abs(v - v64) <= 4 * ref.ulp32(v64) + (1.5e-45 if tiny else 0.0))
    assert tiny and 0 < float(v[v > 0].max()) < 1.2e-38            # the squares really are subnormal


# ---- transform --------------------------------------------------------------------------------------------------------
class _CpuModel:
    """What scorp_amd.transforms touches of a model: four leaves and the SH degree."""

    def __init__(self, xyz, rot, scaling, rest, degree):
        mk = lambda a: torch.nn.Parameter(torch.tensor(np.asarray(a, dtype=np.float64)))
        self._xyz, self._rotation, self._scaling, self._features_rest = mk(xyz), mk(rot), mk(scaling), mk(rest)
        self.max_sh_degree = degree


@pytest.mark.parametrize("degree", (0, 1, 2, 3))
def test_transform64_is_rotate_then_scale_then_translate(degree):
    from scorp_amd import transforms as TR
    g = np.load(GOLDEN)
    k_rest = (degree + 1) ** 2 - 1
    xyz, rot, scaling, rest = ref.transform_inputs(257, k_rest, 3, degree)
    R = torch.tensor(g["rotations"][5])
    s, t = torch.tensor(ref.TRANSFORM_SCALE, dtype=torch.float64), torch.tensor(ref.TRANSFORM_SHIFT, dtype=torch.float64)
    m = _CpuModel(xyz, rot, scaling, rest, degree)
    c = m._xyz.data.mean(0).numpy().copy()
    TR.gaussians_rotate(m, R, fix_center=True)
    TR.gaussians_scale(m, s, fix_center=True)          # (the centre is a fixed point of the rotation about it)
    TR.gaussians_translate(m, t)
    blocks = [b.double().numpy() for b in TR.sh_rotation_blocks(R, degree)] if degree else []
    D = [np.eye(n) for n in (3, 5, 7)]
    D[:len(blocks)] = blocks
    q = TR.matrix_to_quat(R).double().numpy()
    out = ref.transform64(xyz, rot, scaling, rest, R.numpy(), c, t.numpy(), s.numpy(), q, D[0], D[1], D[2], 3)
    for got, want, name in zip(out, (m._xyz, m._rotation, m._scaling, m._features_rest), ("xyz", "rotation", "scaling", "rest")):
        want = want.detach().numpy()
        assert got.shape == want.shape
        if not want.size:
            continue
        # xyz carries the cancellation of (x - c) + c at |c| = 100: 1e-13 absolute is 1e-15 relative there
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), name
    # a part that is not passed is not transformed; a surfel model has two log-scales
    xyz2, rot2, sc2, rest2 = ref.transform64(xyz, None, scaling[:, :2], None, R.numpy(), c, t.numpy(), s.numpy(), q, D[0], D[1], D[2], 2)
    assert rot2 is None and rest2 is None and np.array_equal(xyz2, out[0])
    np.testing.assert_allclose(sc2, scaling[:, :2].astype(np.float64) + np.log(np.array(ref.TRANSFORM_SCALE[:2])), rtol=0, atol=1e-15)


@pytest.mark.parametrize("k_rest", ref.TRANSFORM_K_REST)
def test_transform64_rotates_the_complete_bands_by_the_golden_table(k_rest):
    g = np.load(GOLDEN)
    for k in (0, 3, 7):
        P = ref.transform_params(g, k)
        xyz, rot, scaling, rest = ref.transform_inputs(64, k_rest, 3, k_rest)
        for fn, tol in ((ref.transform64, 1e-14), (ref.transform32, 4e-6)):
            out = fn(xyz, rot, scaling, rest, dims=3, **P)[3]
            want = rest.astype(np.float64)
            done = 0
            for l, name in ((1, "D1"), (2, "D2"), (3, "D3")):
                lo, hi = l * l - 1, (l + 1) ** 2 - 1
                if k_rest >= hi:
                    want[:, lo:hi] = np.einsum("ij,njc->nic", P[name].astype(np.float64).reshape(hi - lo, hi - lo), want[:, lo:hi])
                    done = hi
            assert np.abs(out - want).max() <= tol if k_rest else out.shape == (64, 0, 3)
            assert np.array_equal(out[:, done:], rest[:, done:].astype(out.dtype))       # an incomplete band: as it came
        # the float32 blocks handed over are the table's, and the quaternion is the rotation's
        assert np.abs(P["D3"].reshape(7, 7) - g["D3"][k]).max() < 1e-7
        q = P["q"].astype(np.float64)
        w, x, y, z = q / np.linalg.norm(q)
        Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert np.abs(Rq - g["rotations"][k]).max() < 1e-6
    assert ref.transform_block(P).size == 105


def test_transform_parameter_block_is_what_the_header_says():
    """The three descriptions of scorp_gaussians_transform's `params` name the 105 floats the kernel's struct holds."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "scorp_gs.h")).read()
    kernel = open(os.path.join(root, "scorp_amd", "csrc", "aux_kernels.hip")).read()
    host = open(os.path.join(root, "scorp_amd", "transforms.py")).read()
    fields = re.search(r"struct TransformParams \{ float ([^;]*); \};", kernel).group(1)
    assert sum(int(n) for n in re.findall(r"\[(\d+)\]", fields)) == 105
    assert "params: 105 device floats" in header and "105 floats" in kernel and "105 floats" in host
    for txt in (header, kernel, host):
        assert "113" not in txt.split("scorp_gaussians_transform")[1][:1500] and "flags[8]" not in txt


# ---- the other yardsticks ---------------------------------------------------------------------------------------------
def test_render_tail64_is_nan_to_num_and_its_autograd_on_the_live_pixels():
    depth, alpha, g, radii = ref.tail_inputs(2257, 1000, 0)
    out, vis = ref.render_tail64(depth, alpha, radii)
    d = torch.tensor(depth, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(alpha, dtype=torch.float64, requires_grad=True)
    want32 = torch.nan_to_num(torch.tensor(depth) / torch.tensor(alpha), 0, 0).numpy()
    assert np.array_equal(out.astype(np.float32).view(np.int32), want32.view(np.int32))
    assert np.array_equal(vis, radii > 0) and (radii < 0).any() and (radii == 0).any()
    with np.errstate(over="ignore"):
        live = (alpha != 0) & np.isfinite(depth / np.where(alpha == 0, 1, alpha))
        live &= np.isfinite((depth.astype(np.float64) / np.where(alpha == 0, 1, alpha)).astype(np.float32))
    want = torch.nan_to_num(d / a, 0, 0)
    assert np.array_equal(out[live], want.detach().numpy()[live])
    (want * torch.tensor(g, dtype=torch.float64)).sum().backward()
    gd, ga = ref.render_tail_backward64(g, depth, alpha)
    np.testing.assert_allclose(gd[live], d.grad.numpy()[live], rtol=1e-15, atol=0)
    np.testing.assert_allclose(ga[live], a.grad.numpy()[live], rtol=1e-15, atol=0)
    assert (~live).sum() > 400 and not gd[~live].any() and not ga[~live].any()      # torch leaves NaN at 0 / 0
    assert out[1] == 0 and out[3] == 0 and 9e29 < out[2] < 1.1e30 and live[2] and not live[3]


@pytest.mark.parametrize("hw, n", ref.TAIL_SHAPES)
def test_render_tail_inputs_have_no_double_rounding_case(hw, n):
    depth, alpha, _, _ = ref.tail_inputs(hw, n, hw + n)
    assert ref.double_rounding_cases(depth, alpha) == 0


def _knn_by_sorting(pts):
    p = pts.astype(np.float64)
    out = np.zeros(len(p))
    for i in range(len(p)):
        d = ((p - p[i]) ** 2).sum(1)
        d = np.sort(np.delete(d, i))
        out[i] = d[:3].sum() / 3.0
    return out


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 255, 1025))
def test_knn_yardstick_equals_a_sort_based_restatement(n):
    pts = ref.knn_points(n)
    got, want = ref.knn_mean_dist2_64(pts), _knn_by_sorting(pts)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    if n >= 255:
        assert not got[3:8].any() and got[20] > 0 and got[21] > 0           # five identical points: exactly 0; a pair: not
        half = (n + 1) // 2
        assert not got[half + 3:half + 8].any()                               # the moved copy of the cluster
        order = np.argsort(((pts.astype(np.float64) - pts[10].astype(np.float64)) ** 2).sum(1))
        tail = n - ref.KNN_TILE * ((n - 1) // ref.KNN_TILE)
        assert set(order[1:1 + min(3, tail)]) == set(range(n - min(3, tail), n))     # row 10's neighbours: the last tile
    if n == 1:
        assert got[0] == 0.0
    got32 = ref.knn_mean_dist2_32(pts)
    ok = want > 0
    assert np.all(got32[~ok] == 0) and (not ok.any() or np.max(np.abs(got32[ok] - want[ok]) / want[ok]) < 1e-3)


def test_gather_reference_and_its_row_plans():
    src = [np.arange(12, dtype=np.float32).reshape(4, 3) + 1, -np.arange(4, dtype=np.float32).reshape(4, 1) - 1]
    idx = np.array([2, 0x80000001, 2, 3 | 0x80000000], dtype=np.uint32).view(np.int32)
    a, b = ref.gather_rows(src, (3, 1), (0, 1), idx)
    assert a.tolist() == [[7, 8, 9], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    assert b.reshape(-1).tolist() == [-3, 0, -3, 0] and not np.signbit(b).reshape(-1)[[1, 3]].any()
    for n_out in ref.GATHER_N_OUT:
        idx = ref.gather_index(n_out, ref.GATHER_SRC_ROWS, n_out).view(np.uint32)
        assert idx.shape == (n_out,) and ((idx & 0x7FFFFFFF) < ref.GATHER_SRC_ROWS).all()
        if n_out >= 255:
            fresh = (idx >> 31).astype(bool)
            assert 0.1 < fresh.mean() < 0.3 and len(np.unique(idx & 0x7FFFFFFF)) < n_out
    assert np.array_equal(ref.gather_index(5003, 4000, 5003).view(np.uint32)[:100] & 0x7FFFFFFF, np.arange(100))


def test_densification_stats64_both_norms_and_the_skip_word():
    (mx, ac, de), views = ref.stats_inputs(257, 4, 1)
    radii, vis, grad = views[0]
    for comps in (2, 3):
        m2, a2, d2 = ref.densification_stats64(radii, vis, grad, comps, mx, ac, de)
        on = vis != 0
        want = np.linalg.norm(grad[:, :comps].astype(np.float64), axis=1)
        np.testing.assert_allclose(a2[on] - ac[on], want[on], rtol=0, atol=1e-15)
        assert np.array_equal(a2[~on], ac[~on]) and np.array_equal(m2[~on], mx[~on]) and np.array_equal(d2[~on], de[~on])
        assert np.array_equal(d2[on], de[on] + 1) and np.array_equal(m2[on], np.maximum(mx[on], radii[on]))
        assert (radii[on] < 0).any() and (radii[on] > mx[on]).any()
    m3, a3, d3 = ref.densification_stats64(radii, vis, grad, 2, mx, ac, de, skip=1)
    assert np.array_equal(m3, mx) and np.array_equal(a3, ac) and np.array_equal(d3, de)


@pytest.mark.parametrize("hw", ref.POSE_HW)
def test_pose_score_probes_are_exact_in_any_order_by_the_reference_alone(hw):
    """The planted maps' terms are zero except at the probes (distinct powers of two), and with the power-of-two scale
    every partial result 0.25 + scale * (a subset's sum) is a float32: whatever the order of the additions, and whichever
    workgroup scales which partial sum, nothing is ever rounded, so the GPU test's equality is a condition."""
    d, a, td, ta, probes = ref.pose_planted(hw, hw)
    terms = ref.pose_score_terms64(d, a, td, ta)
    hit = np.flatnonzero(terms)
    assert sorted(hit.tolist()) == sorted(probes) and all(terms[p] == v for p, v in probes.items())
    assert abs((a == 0).mean() - 0.2) < 0.02 or hw < 1000
    q4, trip = 4 * (hw // 4), 1024 * ref.POSE_GRID_BLOCKS
    for must in (0, q4 - 1, q4, hw - 1, trip, trip + 1023):
        assert must in probes or not 0 <= must < hw
    assert len(set(probes.values())) == len(probes) <= 9
    scale = ref.pose_planted_scale(hw)
    assert scale == 2.0 ** round(np.log2(scale)) and scale <= 1.0 / hw < 2 * scale
    quantum = scale                                           # every term is a whole multiple of 2^0
    total = 0.25 + scale * sum(probes.values())
    assert float(np.float32(total)) == total and (0.25 / quantum) == int(0.25 / quantum) or quantum == 1.0
    assert (0.25 + scale * 511) / min(quantum, 0.25) < 2 ** 24          # all partial sums fit 24 bits of one quantum
    # float32 additions in three shuffled orders give that same number
    rng = np.random.default_rng(hw)
    vals = np.array([np.float32(scale) * np.float32(v) for v in probes.values()], dtype=np.float32)
    for _ in range(3):
        acc = np.float32(0.25)
        for v in rng.permutation(vals):
            acc = np.float32(acc + v)
        assert float(acc) == total


@pytest.mark.parametrize("hw", ref.POSE_HW[:7])
def test_pose_score_bound_holds_for_a_float32_evaluation(hw):
    """gamma is the derived worst case of the kernel's tree.  Another float32 tree of about that depth (numpy's pairwise
    sum per 1024 pixels, the partial sums scaled and added one after the other) must sit inside it too, or the bound would
    ask more than float32 gives."""
    d, a, td, ta = ref.pose_maps(hw, hw)
    terms = ref.pose_score_terms64(d, a, td, ta)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = d / a
    q = np.where(np.isfinite(q), q, np.float32(0))
    t32 = (np.abs(a - ta) + np.abs(q - td)).astype(np.float32)
    scale = np.float32(1.0 / hw)
    acc = np.float32(0.25)
    for lo in range(0, hw, 1024):
        acc = np.float32(acc + scale * t32[lo:lo + 1024].sum(dtype=np.float32))
    want = 0.25 + float(scale) * terms.sum()
    assert abs(float(acc) - want) <= ref.pose_gamma(hw) * float(scale) * np.abs(terms).sum()
    assert ref.pose_grid(ref.POSE_HW[-1]) == (2048, 13) and ref.pose_grid(1025) == (2, 5)


def test_edge_sizes_straddle_every_block_and_tile():
    e = ref.edge_sizes()
    for n in (4095, 4096, 4097, 8193, 3 * 4096 + 1):
        assert n in e["adam"]
    assert {255, 256, 257} <= set(e["gather"]) and {255, 256, 257} <= set(e["transform"]) and {255, 256, 257} <= set(e["stats"])
    assert {1023, 1024, 1025} <= set(e["knn"]) and {1023, 1024, 1025} <= set(e["pose_score"])
    assert max(e["pose_score"]) > 2 * 2048 * 1024 and (1000, 2257) in e["render_tail"]
    assert sorted(e["adam_pack"]).count(0) == 2 and len(e["adam_pack"]) == 8


# ---- argument refusals: before any HIP call, so the dummy pointers are never read ---------------------------------------
@pytest.fixture(scope="module")
def L():
    from scorp_amd import _C, build
    build.build()
    return _C.lib()


_DUMMY = 0x10000       # non-zero, 256-byte aligned, never dereferenced


def _refused(L, rc):
    assert rc == -1                                   # SCORP_ERR_INVALID
    msg = L.scorp_last_error()
    assert msg and len(msg) > 8
    return msg


def _adam_tensors(n, numel=16):
    from scorp_amd import _C
    arr = (_C.ScorpAdamTensor * n)()
    for k in range(n):
        arr[k].param = arr[k].grad = arr[k].exp_avg = arr[k].exp_avg_sq = ctypes.cast(_DUMMY, ctypes.c_void_p)
        arr[k].numel, arr[k].lr = numel, 1e-3
    return arr


def test_adam_refuses_too_many_tensors_step_zero_and_a_null_moment(L):
    from scorp_amd import _C
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scorp_gs.h")).read()
    assert "#define SCORP_ADAM_MAX_TENSORS 8" in header and "#define SCORP_ROWS_MAX_TENSORS 24" in header
    many = _adam_tensors(9)
    assert b"n=9" in _refused(L, L.scorp_adam_step_guarded_ex(many, 9, 0.9, 0.999, 1e-15, 1, None, None, None))
    assert b"step=0" in _refused(L, L.scorp_adam_step_guarded_ex(_adam_tensors(2), 2, 0.9, 0.999, 1e-15, 0, None, None, None))
    assert b"step=0" in _refused(L, L.scorp_adam_step(_adam_tensors(2), 2, 0.9, 0.999, 1e-15, 0, None))
    for field in ("exp_avg", "exp_avg_sq"):
        arr = _adam_tensors(3)
        setattr(arr[1], field, ctypes.cast(None, ctypes.c_void_p))
        assert b"tensor 1" in _refused(L, L.scorp_adam_step_guarded(arr, 3, 0.9, 0.999, 1e-15, 1, None, None))


def test_gather_rows_refuses_too_many_tensors_and_an_empty_row(L):
    from scorp_amd import _C

    def tensors(n):
        arr = (_C.ScorpRowTensor * n)()
        for k in range(n):
            arr[k].src = arr[k].dst = ctypes.cast(_DUMMY, ctypes.c_void_p)
            arr[k].row_floats = 3
        return arr
    assert b"n=25" in _refused(L, L.scorp_gather_rows(tensors(25), 25, _DUMMY, 10, None))
    arr = tensors(4)
    arr[2].row_floats = 0
    assert b"tensor 2" in _refused(L, L.scorp_gather_rows(arr, 4, _DUMMY, 10, None))


def test_transform_refuses_an_unaligned_rotation_and_four_scale_dims(L):
    args = lambda rot, dims: (_DUMMY, rot, _DUMMY, _DUMMY, 10, 15, dims, _DUMMY, None)
    assert b"scorp_gaussians_transform" in _refused(L, L.scorp_gaussians_transform(*args(_DUMMY + 4, 3)))
    assert b"scorp_gaussians_transform" in _refused(L, L.scorp_gaussians_transform(*args(_DUMMY, 4)))


def test_view_statistics_refuse_a_row_shorter_than_the_norm(L):
    for stride, comps in ((1, 2), (2, 3)):
        msg = _refused(L, L.scorp_densification_stats_ex(10, _DUMMY, _DUMMY, _DUMMY, stride, comps, None, _DUMMY, _DUMMY, _DUMMY, None))
        assert f"grad_stride={stride}".encode() in msg
    _refused(L, L.scorp_densification_stats(10, _DUMMY, _DUMMY, _DUMMY, 1, None, _DUMMY, _DUMMY, _DUMMY, None))


def test_pose_score_refuses_a_null_accumulator(L):
    rc = L.scorp_gs3d_pose_score_accumulate(_DUMMY, _DUMMY, _DUMMY, _DUMMY, 100, 0.01, None, None)
    assert b"pose_score" in _refused(L, rc)
