"""Float64 yardsticks for the per-iteration helper kernels of scorp_amd/csrc/aux_kernels.hip (numpy only, no GPU).

Written from the contracts in include/scorp_gs.h and the Python the project was modelled on, not from the kernels:
multi-tensor Adam (torch.optim.Adam's single-tensor order), the densify / prune row gather, the model transform
(utils/gaussians.py: translate, scale, rotate incl. the SH bands), the per-view densification statistics, the pose score,
the render tail (nan_to_num(depth / alpha, 0, 0), radii > 0) and the 3-NN initialisation (simple_knn's distCUDA2).

The float32 restatements (`adam_step32`, `transform32`, `knn_mean_dist2_32`) are what the precision of the number format
gives for the same operation in its natural order: they are where the bars of tests/test_aux_edges_gpu.py come from.
The case lists and the seeded inputs live here too, so that tests/test_aux_reference_cpu.py (which makes this file
trusted where there is no GPU) and the GPU tests see the same data.
"""
import math

import numpy as np

F32_MAX = float(np.finfo(np.float32).max)

# ---- case lists -------------------------------------------------------------------------------------------------------
ADAM_BLOCK = 4096                      # elements one workgroup of the Adam kernel owns
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 1)
ADAM_OFFSET = (None, "param", "grad", "exp_avg", "exp_avg_sq")     # which pointer sits 4 bytes off a 16-byte boundary
ADAM_LATE_STEPS = (1000, 30000)
ADAM_LATE_CONFIGS = ((0.9, 0.999, 1e-15), (0.9, 0.999, 1e-8))
ADAM_PACK_SIZES = (4097, 0, 1, 4096, 0, 8193, 3, 12289)
ADAM_PACK_LR = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 0.005, 0.001, 0.01, 0.02)
GATHER_SRC_ROWS = 4000
GATHER_N_OUT = (1, 255, 256, 257, 5003)
GATHER_ROW_FLOATS = (1, 3, 4, 45, 48, 3, 1, 4)
TRANSFORM_N = (1, 255, 256, 257, 1001)
TRANSFORM_K_REST = (0, 1, 3, 5, 8, 12, 15)
TRANSFORM_DIMS = (2, 3)
TRANSFORM_SCALE = (1.5, 0.75, 2.0)
TRANSFORM_CENTRE = (100.0, -50.0, 30.0)
TRANSFORM_SHIFT = (0.3, -0.2, 0.7)
STATS_N = (1, 255, 256, 257)
STATS_FORMS = ((2, 2), (3, 2), (4, 2), (3, 3), (4, 3))        # (grad_stride, norm_components)
POSE_GRID_BLOCKS = 2048                # the pose score's grid is capped here, 1024 pixels per block and trip
POSE_HW = (1, 3, 4, 5, 1023, 1024, 1025, 2048 * 1024 + 5, 2 * 2048 * 1024 + 7)
POSE_OFFSET = (None, "depth", "alpha", "tgt_depth", "tgt_alpha")
TAIL_SHAPES = ((2257, 1000), (1000, 2257), (0, 300), (300, 0), (256, 256), (257, 255))    # (HW, N)
KNN_N = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)
KNN_TILE = 1024


def edge_sizes():
    """Every size list of the edge sweep by kernel, for the tests that walk all of them."""
    return {"adam": ADAM_SIZES, "adam_pack": ADAM_PACK_SIZES, "gather": GATHER_N_OUT, "transform": TRANSFORM_N,
            "stats": STATS_N, "pose_score": POSE_HW, "render_tail": TAIL_SHAPES, "knn": KNN_N}


def ulp32(x):
    """Spacing of float32 at |x| (elementwise, as float64)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- Adam -------------------------------------------------------------------------------------------------------------
def adam_step64(p, g, m, v, lr, beta1, beta2, eps, step):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) in its single-tensor operation order, float64:
    exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2);
    denom = (exp_avg_sq.sqrt() / sqrt(bias_correction2)).add_(eps); param.addcdiv_(exp_avg, denom, value=-lr / bias_correction1).
    -> (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    p = p + (-(lr / bc1)) * (m / denom)
    return p, m, v


def adam_step32(p, g, m, v, lr, beta1, beta2, eps, step):
    """The same order in float32, every product, sum, root and quotient rounded on its own, with the host constants the
    way scorp_adam_step_guarded_ex hands them over: (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps,
    (float)bc1 and (float)(1 / sqrt(bc2)) formed in double; the step size is the float lr over the float bc1.  -> (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    omb1, b2, omb2, eps32 = f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps)
    bc1 = f(1.0 - beta1 ** step)
    inv_sqrt_bc2 = f(1.0 / math.sqrt(1.0 - beta2 ** step))
    step_size = f(lr) / bc1
    with np.errstate(under="ignore"):
        m = m + (g - m) * omb1
        v = v * b2 + (omb2 * g) * g
        denom = np.sqrt(v) * inv_sqrt_bc2 + eps32
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adam_inputs(numel, seed, tiny=False):
    """Parameters and a gradient of `numel` floats: magnitudes 1e-12 .. 1e3, every third gradient exactly zero (an
    invisible splat: eps decides the quotient).  tiny: |g| in 1e-22 .. 3e-20, so that g * g is subnormal in float32."""
    rng = np.random.default_rng(1000 + seed)
    p = rng.normal(0.0, 1.0, numel).astype(np.float32)
    lo, hi = (-22.0, -19.5) if tiny else (-12.0, 3.0)
    g = (10.0 ** rng.uniform(lo, hi, numel) * rng.choice([-1.0, 1.0], numel)).astype(np.float32)
    g[::3] = 0.0
    return p, g


def adam_moments(numel, seed):
    """Random non-zero moments of a run that has been going for a while (exp_avg_sq >= 0)."""
    rng = np.random.default_rng(2000 + seed)
    m = (rng.normal(0.0, 1.0, numel) * 10.0 ** rng.uniform(-6, 1, numel)).astype(np.float32)
    v = (10.0 ** rng.uniform(-12, 2, numel)).astype(np.float32)
    return m, v


# ---- row gather -------------------------------------------------------------------------------------------------------
def gather_rows(srcs, row_floats, zero_if_fresh, src_index):
    """dst row j of every tensor = src row (src_index[j] & 0x7fffffff); a fresh row (bit 31) of a tensor with
    zero_if_fresh is +0.0.  srcs: float32 [rows, row_floats[k]] -> list of [n_out, row_floats[k]]."""
    idx = np.asarray(src_index).astype(np.int64) & 0xFFFFFFFF
    fresh = (idx >> 31) != 0
    rows = idx & 0x7FFFFFFF
    out = []
    for s, w, z in zip(srcs, row_floats, zero_if_fresh):
        d = np.asarray(s, dtype=np.float32).reshape(-1, w)[rows].copy()
        if z:
            d[fresh] = 0.0
        out.append(d)
    return out


def gather_index(n_out, n_src, seed):
    """A row plan as densify_and_prune writes them: an identity stretch, a reversed stretch, duplicates, rows dropped,
    and about a fifth of the entries fresh (bit 31 set, the low bits a valid row).  int32 [n_out]."""
    rng = np.random.default_rng(3000 + seed)
    parts = [np.arange(0, 100), np.arange(900, 800, -1) - 1, rng.integers(0, n_src, 20).repeat(3),
             rng.integers(0, n_src // 2, max(n_out, 8)) * 2]         # (behind the stretches every odd row is dropped)
    idx = np.resize(np.concatenate(parts).astype(np.int64), n_out)
    fresh = rng.random(n_out) < 0.2
    idx = np.where(fresh, idx | 0x80000000, idx)
    return idx.astype(np.uint32).view(np.int32)


# ---- model transform --------------------------------------------------------------------------------------------------
def _bands(k_rest):
    """(first coefficient, width) of the SH bands 1..3 that are complete inside k_rest coefficients of features_rest."""
    return [(l * l - 1, 2 * l + 1) for l in (1, 2, 3) if k_rest >= (l + 1) * (l + 1) - 1]


def _transform(dt, xyz, rot, scaling, rest, R, c, t, s, q, D1, D2, D3, dims):
    a = lambda x: None if x is None else np.array(x, dtype=dt)
    xyz, rot, scaling, rest = a(xyz), a(rot), a(scaling), a(rest)
    R, c, t, s, q = a(R).reshape(3, 3), a(c), a(t), a(s), a(q)
    xyz = ((xyz - c) @ R.T) * s + c + t
    if rot is not None:
        b = rot / np.sqrt((rot * rot).sum(1, keepdims=True))
        aw, ax, ay, az = q
        bw, bx, by, bz = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        rot = np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1)
    if scaling is not None:
        scaling = scaling + np.log(s[:dims])[None]
    if rest is not None and rest.shape[1] > 0:
        out = rest.copy()
        for (first, width), D in zip(_bands(rest.shape[1]), (D1, D2, D3)):
            out[:, first:first + width] = np.einsum("ij,njc->nic", a(D).reshape(width, width), rest[:, first:first + width])
        rest = out
    return xyz, rot, scaling, rest


def transform64(xyz, rot, scaling, rest, R, c, t, s, q, D1, D2, D3, dims):
    """xyz <- ((xyz - c) R^T) * s + c + t; rot <- q (x) normalize(rot) (Hamilton, w x y z); scaling <- scaling + log(s)
    (`dims` log-scales); rest[N, k_rest, 3]: band l = 1..3 multiplied by D_l where the whole band (coefficients
    l^2 - 1 .. (l+1)^2 - 2) is there, i.e. k_rest >= 3, >= 8, >= 15; any other coefficient is returned as it came.
    rot / scaling / rest may be None (that part is not transformed).  float64."""
    return _transform(np.float64, xyz, rot, scaling, rest, R, c, t, s, q, D1, D2, D3, dims)


def transform32(xyz, rot, scaling, rest, R, c, t, s, q, D1, D2, D3, dims):
    """The same in numpy float32, in the order the formula is written."""
    out = _transform(np.float32, xyz, rot, scaling, rest, R, c, t, s, q, D1, D2, D3, dims)
    assert all(o is None or o.dtype == np.float32 for o in out)
    return out


def quat_of(R):
    """(w, x, y, z) of a proper rotation matrix (float64), the branch with the largest pivot."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    return np.array(q)


def transform_inputs(n, k_rest, dims, seed):
    """A model of n Gaussians around TRANSFORM_CENTRE: quaternions NOT normalised (norms 0.1 .. 10), float32."""
    rng = np.random.default_rng(4000 + seed)
    xyz = (rng.normal(0.0, 2.0, (n, 3)) + np.array(TRANSFORM_CENTRE)).astype(np.float32)
    rot = rng.normal(0.0, 1.0, (n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True) * 10.0 ** rng.uniform(-1, 1, (n, 1))).astype(np.float32)
    scaling = rng.normal(-3.0, 1.0, (n, dims)).astype(np.float32)
    rest = rng.normal(0.0, 0.5, (n, k_rest, 3)).astype(np.float32)
    return xyz, rot, scaling, rest


def transform_params(golden, k):
    """Rotation k of tests/golden/wigner_d.npz with its blocks, as the float32 values the kernel is handed (the
    yardsticks then read the same numbers): dict R, c, t, s, q, D1, D2, D3."""
    f = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32)
    R = golden["rotations"][k]
    return dict(R=f(R).reshape(-1), c=f(TRANSFORM_CENTRE), t=f(TRANSFORM_SHIFT), s=f(TRANSFORM_SCALE), q=f(quat_of(R)),
                D1=f(golden["D1"][k]).reshape(-1), D2=f(golden["D2"][k]).reshape(-1), D3=f(golden["D3"][k]).reshape(-1))


def transform_block(P):
    """The 105 floats scorp_gaussians_transform reads, in its order."""
    flat = np.concatenate([P[n].reshape(-1) for n in ("R", "c", "t", "s", "q", "D1", "D2", "D3")]).astype(np.float32)
    assert flat.size == 105
    return flat


# ---- view statistics --------------------------------------------------------------------------------------------------
def densification_stats64(radii, visible, grad, norm_components, max_radii2D, accum, denom, skip=0):
    """For every visible Gaussian: max_radii2D = max(max_radii2D, radii), accum += |grad row's first norm_components
    floats| (2: x, y, the 3DGS model; 3: the whole row, the 2DGS model), denom += 1.  Nothing changes when the skip word
    is non-zero.  grad: [N, stride].  -> three float64 arrays."""
    mx, ac, de = (np.array(a, dtype=np.float64) for a in (max_radii2D, accum, denom))
    if skip:
        return mx, ac, de
    vis = np.asarray(visible) != 0
    g = np.asarray(grad, dtype=np.float64)[:, :norm_components]
    mx[vis] = np.maximum(mx[vis], np.asarray(radii, dtype=np.float64)[vis])
    ac[vis] += np.sqrt((g[vis] * g[vis]).sum(1))
    de[vis] += 1.0
    return mx, ac, de


def stats_inputs(n, stride, seed):
    """State with a distinctive value in every row, and two views (radii, visible, grad [n, stride]).  The gradients stay
    below the accumulator's magnitude, so that the sum's rounding is the accumulator's."""
    rng = np.random.default_rng(5000 + seed)
    i = np.arange(n)
    state = ((3.0 + (i % 37)).astype(np.float32), (0.5 + 1e-3 * i).astype(np.float32), (7.0 + (i % 5)).astype(np.float32))
    views = []
    for _ in range(2):
        radii = rng.integers(-3, 60, n).astype(np.int32)
        visible = (rng.random(n) > 0.3).astype(np.uint8)
        if n > 2:
            visible[n - 1], visible[0] = 1, 0
        grad = (rng.normal(0.0, 1.0, (n, stride)) * 10.0 ** rng.uniform(-4, -2, (n, 1))).astype(np.float32)
        views.append((radii, visible, grad))
    return state, views


# ---- pose score -------------------------------------------------------------------------------------------------------
def normalised_depth64(depth, alpha):
    """nan_to_num(depth / alpha, nan=0, posinf=0) of float32 maps as float64: the quotient is judged finite or not as a
    float32 (1 / 1e-40 is infinite there), -inf becomes the most negative float32 as torch.nan_to_num does."""
    d, a = np.asarray(depth, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = d / a
        q32 = q.astype(np.float32)
    out = np.where(np.isfinite(q32), q, 0.0)
    return np.where(q32 == -np.inf, -F32_MAX, out)


def pose_score_terms64(depth, alpha, tgt_depth, tgt_alpha):
    """Per pixel |alpha - tgt_alpha| + |nan_to_num(depth / alpha, 0, 0) - tgt_depth| in float64 (the caller sums)."""
    a, ta, td = (np.asarray(x, dtype=np.float64) for x in (alpha, tgt_alpha, tgt_depth))
    return np.abs(a - ta) + np.abs(normalised_depth64(depth, alpha) - td)


def pose_grid(hw):
    """(workgroups, most terms one thread adds in a row) of the pose score at hw pixels: 1024 pixels per workgroup and
    trip, at most POSE_GRID_BLOCKS workgroups, plus one term of the tail behind the last whole quad."""
    blocks = min((hw + 1023) // 1024, POSE_GRID_BLOCKS)
    return blocks, 4 * -(-hw // (1024 * blocks)) + 1


def pose_gamma(hw):
    """Worst case of the pose score's summation tree in units of sum |term|: k terms in a row in one thread, 6 shuffle
    levels, 3 adds across the waves, B atomics in any order, 2 for the scaling and the term's own roundings."""
    blocks, k = pose_grid(hw)
    return (k + 6 + 3 + blocks + 2) * 2.0 ** -24


def pose_maps(hw, seed):
    """Random maps: alpha in (0, 1], depth = z * alpha with z in 2 .. 3, a fifth of the pixels empty (alpha = depth = 0);
    targets of the same kind, independent.  float32 x 4."""
    rng = np.random.default_rng(6000 + seed)

    def pair():
        a = (1.0 - rng.random(hw)).astype(np.float32)
        d = ((2.0 + rng.random(hw)).astype(np.float32) * a).astype(np.float32)
        e = rng.random(hw) < 0.2
        a[e], d[e] = 0.0, 0.0
        return d, a
    d, a = pair()
    td_raw, ta = pair()
    td = normalised_depth64(td_raw, ta).astype(np.float32)
    return d, a, td, ta


def pose_probes(hw, seed):
    """The pixels a wrong loop bound would drop or count twice: 0, the last pixel of the last whole quad, the first pixel
    behind it, the last pixel, the first and last pixel of workgroup 0's second trip, and three seeded ones."""
    rng = np.random.default_rng(7000 + seed)
    q4 = 4 * (hw // 4)
    trip = 1024 * POSE_GRID_BLOCKS
    cand = [0, q4 - 1, q4, hw - 1, trip, trip + 1023] + [int(x) for x in rng.integers(0, hw, 3)]
    out = []
    for c in cand:
        if 0 <= c < hw and c not in out:
            out.append(c)
    return out


def pose_planted_scale(hw):
    """The power of two at or just below 1 / hw (1 / hw itself where hw is one).  Only a power of two commutes with the
    rounding of every workgroup's `scale * partial sum`, which is what makes the planted result a condition."""
    return 2.0 ** -math.ceil(math.log2(hw))


def pose_planted(hw, seed):
    """Maps whose every term is exactly zero (alpha == tgt_alpha, depth / alpha == tgt_depth with an exact quotient; a
    fifth empty) except at pose_probes, where tgt_depth is off by a distinct power of two 2^0 .. 2^8.
    -> (depth, alpha, tgt_depth, tgt_alpha, {pixel: term})."""
    rng = np.random.default_rng(8000 + seed)
    a = (2.0 ** -rng.integers(0, 3, hw)).astype(np.float32)                 # 1, 1/2, 1/4
    z = (2.0 + rng.integers(0, 256, hw) / 128.0).astype(np.float32)         # 2 .. 4 in steps of 1/128
    e = rng.random(hw) < 0.2
    a[e], z[e] = 0.0, 0.0
    d = (z * a).astype(np.float32)
    td, ta = z.copy(), a.copy()
    probes = {}
    for j, px in enumerate(pose_probes(hw, seed)):
        probes[px] = 2.0 ** j
        td[px] = np.float32(z[px] + 2.0 ** j)
    return d, a, td, ta, probes


# ---- render tail ------------------------------------------------------------------------------------------------------
def render_tail64(depth, alpha, radii):
    """(nan_to_num(depth / alpha, nan=0, posinf=0) as float64, radii > 0)."""
    return normalised_depth64(depth, alpha), np.asarray(radii) > 0


def render_tail_backward64(g_out, depth, alpha):
    """Gradients of the normalised depth with the empty-pixel convention of render_tail_backward_kernel: where the
    quotient is not finite (alpha = 0, or depth / alpha beyond float32) both gradients are plain zeros, elsewhere
    g / alpha and -g * depth / alpha^2.  float64 (values beyond float32 stay what they are: the caller rounds)."""
    g, d, a = (np.asarray(x, dtype=np.float64) for x in (g_out, depth, alpha))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q32 = (d / a).astype(np.float32)
        ok = (a != 0.0) & np.isfinite(q32)
        gd = np.where(ok, g / a, 0.0)
        ga = np.where(ok, -g * d / (a * a), 0.0)
    return gd, ga


def tail_inputs(hw, n, seed):
    """depth, alpha, upstream gradient (float32 [hw]) and radii (int32 [n], negative ones included).  Pixels 0 / 0,
    1 / 1e-30 (finite, huge) and 1 / 1e-40 (infinite in float32) are planted where there is room."""
    rng = np.random.default_rng(9000 + seed)
    alpha = (1.0 - rng.random(hw)).astype(np.float32)
    depth = ((2.0 + rng.random(hw)).astype(np.float32) * alpha).astype(np.float32)
    e = rng.random(hw) < 0.2
    alpha[e], depth[e] = 0.0, 0.0
    for first, (dv, av) in zip((1, 2, 3), ((0.0, 0.0), (1.0, 1e-30), (1.0, 1e-40))):
        with np.errstate(under="ignore"):
            depth[first::97], alpha[first::97] = np.float32(dv), np.float32(av)
    g = rng.normal(0.0, 1.0, hw).astype(np.float32)
    g[g == 0] = 1.0
    radii = rng.integers(-4, 5, n).astype(np.int32)
    return depth, alpha, g, radii


def double_rounding_cases(depth, alpha):
    """Number of pixels at which the correctly rounded float32 quotient differs from the float64 quotient rounded once."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q32 = np.asarray(depth, dtype=np.float32) / np.asarray(alpha, dtype=np.float32)
        q64 = (np.asarray(depth, dtype=np.float64) / np.asarray(alpha, dtype=np.float64)).astype(np.float32)
    same = (q32 == q64) | (np.isnan(q32) & np.isnan(q64))
    return int((~same).sum())


# ---- 3-NN -------------------------------------------------------------------------------------------------------------
def _knn(dt, xyz, chunk=512):
    p = np.asarray(xyz, dtype=np.float32).astype(dt)
    n = p.shape[0]
    out = np.zeros(n, dtype=dt)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        diff = p[None, :, :] - p[lo:hi, None, :]
        d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        d2[np.arange(hi - lo), np.arange(lo, hi)] = np.inf          # its own neighbour BY INDEX: duplicates stay
        k = min(3, n - 1)
        if k == 0:
            continue
        near = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
        s = near[:, 0].copy()
        for j in range(1, k):
            s = s + near[:, j]
        out[lo:hi] = s / dt(3.0)
    return out


def knn_mean_dist2_64(xyz):
    """Mean squared distance of every point to its 3 nearest OTHER points (other by index: a duplicate is a neighbour at
    distance 0), brute force over all pairs in float64.  With fewer than four points: the sum of what exists, over 3."""
    return _knn(np.float64, xyz)


def knn_mean_dist2_32(xyz):
    """The same from float32 differences, float32 throughout."""
    out = _knn(np.float32, xyz)
    assert out.dtype == np.float32
    return out


def knn_points(n, seed=0):
    """Exactly n points.  From 255 up: normal points in the first half with a cluster of five identical points (rows
    3 .. 7) and an identical pair (rows 20, 21), the second half a copy of the first moved to (1000, 1000, 1000) - nearest
    neighbours then sit in other 1024-point tiles and the coordinates are large - and the last rows (those of the last,
    partly filled tile, three at the most) put right next to row 10, whose nearest neighbours are then in that tile."""
    rng = np.random.default_rng(10000 + n + seed)
    if n < 255:
        return rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    half = (n + 1) // 2
    base = rng.normal(0.0, 1.0, (half, 3)).astype(np.float32)
    base[3:8] = base[3]
    base[21] = base[20]
    pts = np.concatenate([base, base[:n - half] + np.float32(1000.0)]).astype(np.float32)
    tail = n - KNN_TILE * ((n - 1) // KNN_TILE)
    for j in range(min(3, tail)):
        pts[n - 1 - j] = base[10] + np.float32(1e-3) * np.array([j + 1, -(j + 1), 2 * j + 1], dtype=np.float32)
    return pts
