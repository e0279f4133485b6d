"""Fixtures of the pose-fit edge tests (tests/test_pose_fit_edges_cpu.py, tests/test_pose_fit_edges_gpu.py): seeded
builders of RANSAC and Adam cases and their float64 yardstick results (tests/pose_fit_reference.py), computed once per
process.  No GPU.

A RANSAC case is a planted similarity (rotation 20 degrees, scale 1.2 for Umeyama and 1 for Kabsch), Gaussian noise on
the inliers, about 30 % gross outliers, triples by rng.choice(n, 3, replace=False).  The seeds are fixed here; the CPU
test checks from the yardstick alone that each case has the margin, the conditioning and the structure (block edges,
ties, early exits, degenerate fits) that its name claims, so a seed that stops qualifying fails there, not on the GPU."""
import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

from tests import pose_fit_reference as ref

CHUNK = 1024                 # kPoseChunk of csrc/pose_fit.hip: pairs per block (256 threads x 4)
WAVE = 64
MIN_MARGIN = 1e-9            # smallest |residual - threshold| / threshold an exact comparison needs
MIN_COND = 1e-6              # second over first singular value of every ordinary triple
BOUND = 1e-9                 # the project's float64-to-float64 bound, scaled by the data

R0 = ref.rotation_about((0.2, 0.5, -0.8), 20.0)
T0 = np.array([0.3, -0.11, 0.2])
SPREAD, NOISE, THRESHOLD = 0.3, 1e-3, 5e-3

EDGE_SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
NH_EDGES = (1, 63, 64, 65, 128, 129)
METHODS = ("umeyama", "kabsch")
TIES = {"lanes": (201, (130, 67, 200)), "strides": (201, (5, 69, 133)), "slot0": (201, (0, 64, 100)), "late": (201, (137, 200)),
        "last": (201, (200,)), "small": (50, (49, 20, 33))}          # name: (nh, slots holding the best triple)


def blocks_of(n):
    """(nblk, pairs in the last block) of the kernels' decomposition."""
    nblk = (n + CHUNK - 1) // CHUNK
    return nblk, n - (nblk - 1) * CHUNK


@dataclass
class Ransac:
    name: str
    p: np.ndarray
    q: np.ndarray
    tri: np.ndarray
    thr: float = THRESHOLD
    ratio: float = -1.0
    method: str = "umeyama"
    note: dict = field(default_factory=dict)     # what the builder planted (slots, intended hypotheses)

    @property
    def extent(self):
        """max(1, largest finite |coordinate|): the factor on the 1e-9 bound for t."""
        a = np.concatenate([self.p.ravel(), self.q.ravel()])
        return max(1.0, float(np.abs(a[np.isfinite(a)]).max()))


def cloud(n, seed, method="umeyama", outlier_share=0.3, noise=NOISE):
    """(p, q, rng): q = s0 R0 p + T0 + noise, int(outlier_share * n) pairs with q replaced by an unrelated point."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)) * SPREAD
    q = (1.2 if method == "umeyama" else 1.0) * p @ R0.T + T0 + rng.normal(size=(n, 3)) * noise
    k = int(outlier_share * n)
    out = rng.choice(n, k, replace=False)
    q[out] = rng.normal(size=(k, 3)) * SPREAD + T0
    return p, q, rng


def draw(rng, n, nh):
    return np.stack([rng.choice(n, 3, replace=False) for _ in range(nh)]).astype(np.int32)


def _counts(p, q, tri, thr, method):
    return ref.ransac_counts(p, q, tri, thr, method)


def edge_case(n, method, nh=130):
    p, q, rng = cloud(n, 1000 + n, method)
    if n == 3:                                   # one triple: its six orders, cycled
        tri = np.array(list(itertools.islice(itertools.cycle(itertools.permutations(range(3))), nh)), dtype=np.int32)
    else:
        tri = draw(rng, n, nh)
    return Ransac(f"edge-{n}-{method}", p, q, tri, method=method)


def nh_case(nh):
    """The first nh of 129 triples on 257 pairs, a triple with at least 3 inliers moved to slot 0 (nh = 1 must fit)."""
    p, q, rng = cloud(257, 77)
    tri = draw(rng, 257, 129)
    good = int(np.nonzero(_counts(p, q, tri, THRESHOLD, "umeyama") >= 3)[0][0])
    tri[[0, good]] = tri[[good, 0]]
    return Ransac(f"nh-{nh}", p, q, tri[:nh].copy())


def nh_limit_case():
    """65 535 hypotheses over 8 pairs: the grid's y limit, and every ordered triple many times over (ties at scale)."""
    p, q, rng = cloud(8, 8)
    u = rng.random((65535, 8))
    return Ransac("nh-65535", p, q, np.argsort(u, axis=1)[:, :3].astype(np.int32))


def tie_case(name):
    """The best triple of a base fixture copied into the given slots, its own slot overwritten with the worst one."""
    nh, slots = TIES[name]
    p, q, rng = cloud(257, 31)
    tri = draw(rng, 257, nh)
    c = _counts(p, q, tri, THRESHOLD, "umeyama")
    best, worst = tri[int(np.argmax(c))].copy(), tri[int(np.argmin(c))].copy()
    tri[c == c.max()] = worst
    tri[list(slots)] = best
    return Ransac(f"tie-{name}", p, q, tri, note={"slots": slots})


def _early_base():
    """257 pairs, 130 triples rolled so that a global maximum sits at slot 70, and the maxima that the roll put before it
    overwritten with the worst triple: slot 70 is the first maximum."""
    p, q, rng = cloud(257, 41)
    tri = draw(rng, 257, 130)
    c = _counts(p, q, tri, THRESHOLD, "umeyama")
    roll = 70 - int(np.argmax(c))
    tri, c = np.roll(tri, roll, axis=0), np.roll(c, roll)
    early = np.nonzero(c[:70] == c.max())[0]
    tri[early], c[early] = tri[int(np.argmin(c))], c.min()
    return p, q, tri, c


def early_case(kind):
    """before: the first count above the ratio lies before the global maximum; at: it is the global maximum; none: nothing
    exceeds the ratio (the first maximum wins); tiny: ratio 1e-12, the first hypothesis with any inlier.  (A first
    exceeding hypothesis AFTER the first global maximum cannot exist: the maximum exceeds whatever a later count does.)"""
    p, q, tri, c = _early_base()
    n, g = len(p), 70
    f = int(np.argmax(c[:g]))
    ratio = {"before": (c[f] - 0.5) / n, "at": (c[g] - 0.5) / n, "none": (c[g] + 0.5) / n, "tiny": 1e-12}[kind]
    if kind == "tiny":                            # a hypothesis with no inlier first, then one with at least 3
        zero, fit = int(np.nonzero(c == 0)[0][0]), int(np.nonzero(c >= 3)[0][0])
        tri = np.concatenate([tri[[zero, fit]], tri])
    return Ransac(f"early-{kind}", p, q, tri, ratio=float(ratio), note={"g": g, "f": f})


def early_tiny_error_case():
    """Ratio 1e-12 where the first hypothesis with any inlier has 1 or 2: the reference stops there and raises."""
    p, q, tri, c = _early_base()
    zero, few = int(np.nonzero(c == 0)[0][0]), int(np.nonzero((c == 1) | (c == 2))[0][0])
    return Ransac("early-tiny-error", p, q, np.concatenate([tri[[zero, few]], tri]), ratio=1e-12)


def early_equal_case(kind):
    """n = 1000, ratio 0.5 (500.0 exactly): pairs that no triple samples are turned into outliers until the intended
    hypothesis counts exactly 500, which does not exceed.  more: it sits at slot 3, before every hypothesis that counts
    more (a >= test would stop at slot 3); max: it is the global maximum, nothing exceeds, the first maximum wins."""
    p, q, rng = cloud(1000, 51)
    tri = draw(rng, 1000, 130)
    t = ref.ransac_table(p, q, tri, THRESHOLD, "umeyama")
    c = t["counts"]
    if kind == "max":
        h = int(np.argmax(c))
    else:
        above = np.nonzero(c > 520)[0]
        h = int(above[np.argmin(c[above])])
    inl = ref.residuals(p, q, t["R"][h], t["t"][h], t["s"][h]) < THRESHOLD
    free = np.nonzero(inl & ~np.isin(np.arange(1000), tri))[0][:int(c[h]) - 500]
    q[free] = T0 + 50.0 + rng.normal(size=(len(free), 3))
    c = _counts(p, q, tri, THRESHOLD, "umeyama")
    if kind == "more":                            # the hypotheses that count less first, h at slot 3, then the rest
        low = np.nonzero(c < 500)[0][:3]
        rest = np.setdiff1d(np.arange(130), np.concatenate([low, [h]]))
        tri, h = tri[np.concatenate([low, [h], rest])], 3
    return Ransac(f"early-equal-{kind}", p, q, tri, ratio=0.5, note={"h": h})


NO_INLIER_SEED = 0


def no_inlier_cases(seed=NO_INLIER_SEED):
    """Two fixtures that differ in one pair: three exactly consistent pairs among unrelated ones (the best count is 3), and
    the same with the target of pair 2 moved by 2.5 thresholds: the fit on (0, 1, 2) then passes pairs 0 and 1 within the
    threshold and pair 2 outside it (the three residual vectors of a centred fit sum to zero), the best count is 2."""
    rng = np.random.default_rng(900 + seed)
    n = 12
    p = rng.normal(size=(n, 3)) * SPREAD
    q = rng.normal(size=(n, 3)) * SPREAD + T0 + 3.0
    q[:3] = 1.2 * p[:3] @ R0.T + T0
    tri = np.concatenate([np.array([[5, 6, 7], [0, 1, 2], [2, 0, 1]], dtype=np.int32), draw(rng, n, 37)])
    qb, d = q.copy(), rng.normal(size=3)
    qb[2] += 2.5 * THRESHOLD * d / np.linalg.norm(d)
    return Ransac("count-3", p, q, tri), Ransac("count-2", p, qb, tri)


def reflection_case(method):
    """target = similarity(mirror(source)) on a non-planar cloud; the threshold takes every pair as an inlier of the winner,
    so the final covariance has full rank and det(U) det(V) < 0."""
    rng = np.random.default_rng(61)
    p = rng.normal(size=(300, 3)) * SPREAD * np.array([1.0, 0.7, 0.4])
    q = (1.2 if method == "umeyama" else 1.0) * (p * np.array([1.0, 1.0, -1.0])) @ R0.T + T0
    return Ransac(f"reflection-{method}", p, q, draw(rng, 300, 65), thr=2.0, method=method)


def planar_case(kind):
    """Rank 2 in the final fit.  plane: the inliers' third coordinate is exactly 0 before the planted map; slab: it is
    1e-14 of the extent (below svd3's 1e-13 rank threshold); three: exactly three inliers."""
    rng = np.random.default_rng(71)
    n = 300 if kind != "three" else 40
    p = rng.normal(size=(n, 3)) * SPREAD
    p[:, 2] = 0.0 if kind != "slab" else rng.uniform(-1, 1, n) * 1e-14 * SPREAD
    q = 1.2 * p @ R0.T + T0
    if kind == "three":
        q[3:] = rng.normal(size=(n - 3, 3)) * SPREAD + T0 + 5.0
        tri = np.concatenate([draw(rng, n, 20), [[0, 1, 2]], draw(rng, n, 20)]).astype(np.int32)
        return Ransac("rank2-three", p, q, tri, thr=1e-6)
    out = rng.choice(n, 90, replace=False)
    q[out] = rng.normal(size=(90, 3)) * SPREAD + T0
    return Ransac(f"rank2-{kind}", p, q, draw(rng, n, 65), thr=1e-6)


def scaled_case(kind):
    """The n = 1025 fixture with its coordinates times 1e-6 / 1e6 (threshold alike) or shifted by 1e5 on every axis."""
    c = edge_case(1025, "umeyama")
    if kind == "shift":
        return Ransac("scale-shift", c.p + 1e5, c.q + 1e5, c.tri)
    f = {"small": 1e-6, "large": 1e6}[kind]
    return Ransac(f"scale-{kind}", c.p * f, c.q * f, c.tri, thr=c.thr * f)


def nonfinite_case(method="umeyama"):
    """257 pairs; pair 10 has a NaN source coordinate, pair 20 an infinite target coordinate; triples 3, 64 and 100 sample
    them."""
    c = edge_case(257, method)
    p, q, tri = c.p.copy(), c.q.copy(), c.tri.copy()
    p[10, 1], q[20, 2] = np.nan, np.inf
    tri[3], tri[64], tri[100] = (10, 1, 2), (4, 20, 5), (20, 7, 10)
    return Ransac(f"nonfinite-{method}", p, q, tri, method=method, note={"pairs": (10, 20), "hyps": (3, 64, 100)})


def degenerate_case(method):
    """Ordinary triples with degenerate ones among them: (i, i, j) at slot 5, three collinear pairs at slot 64, (i, i, i)
    at slot 70.  Pairs 250..252 lie on a line in source and target (an image under the planted map, so either method fits
    them); pair 42 has short mantissas, so its triple centres to exactly zero and Umeyama's scale is 0 / 0 there."""
    c = edge_case(257, method)
    p, q, tri = c.p.copy(), c.q.copy(), c.tri.copy()
    s0 = 1.2 if method == "umeyama" else 1.0
    a, d = p[250].copy(), np.array([0.6, -0.3, 0.2])
    for k, u in enumerate((0.0, 0.35, 1.0)):
        p[250 + k] = a + u * d
        q[250 + k] = s0 * p[250 + k] @ R0.T + T0
    keep = ~np.isin(tri, (250, 251, 252)).any(axis=1)
    tri[~keep] = tri[np.nonzero(keep)[0][0]]       # no ordinary triple samples the line
    p[42], q[42] = np.round(p[42] * 1024) / 1024, np.round(q[42] * 1024) / 1024   # few bits: (x + x + x) / 3 == x exactly
    inl = np.nonzero(ransac_yardstick(f"edge-257-{method}")["mask"][:240])[0]
    i, j = [int(v) for v in inl[inl != 42][:2]]    # two inlier pairs: the line through them is mapped within the threshold
    tri[5], tri[64], tri[70] = (i, i, j), (250, 251, 252), (42, 42, 42)
    return Ransac(f"degenerate-{method}", p, q, tri, method=method, note={"hyps": (5, 64, 70)})


def line_inliers(c, h):
    """How many of the distinct pairs of the degenerate sample h the map of the line through the sample's sources onto
    the line through its targets (centroid to centroid, direction to direction, rigid for Kabsch and with the least-squares
    scale for Umeyama: what either fits at rank 1, whatever the completion) puts within the threshold, and the relative
    margin of that count."""
    idx = c.tri[h]
    p, q = c.p[idx], c.q[idx]
    pc, qc = p - p.mean(axis=0), q - q.mean(axis=0)
    if not pc.any() and not qc.any():
        return 1, 1.0                                                         # one pair, mapped onto its target
    u = np.linalg.svd(pc)[2][0]
    a = pc @ u
    v = (a[:, None] * qc).sum(axis=0)
    scale = np.linalg.norm(v) / (a @ a) if c.method == "umeyama" else 1.0
    res = np.linalg.norm(scale * a[:, None] * (v / np.linalg.norm(v)) - qc, axis=1)
    first = np.unique(idx, return_index=True)[1]
    return int((res[first] < c.thr).sum()), float(np.abs(res[first] - c.thr).min() / c.thr)


def collinear_winner_case(method):
    """40 pairs on a line (a rigid or similar image of it) plus 60 outliers: the winner's inliers are collinear, the
    final covariance has rank 1."""
    rng = np.random.default_rng(81)
    n, s0 = 100, (1.2 if method == "umeyama" else 1.0)
    p = rng.normal(size=(n, 3)) * SPREAD
    p[:40] = np.array([0.1, -0.2, 0.05]) + rng.uniform(-1, 1, (40, 1)) * np.array([0.5, 0.4, -0.3])
    q = rng.normal(size=(n, 3)) * SPREAD + T0 + 3.0
    q[:40] = s0 * p[:40] @ R0.T + T0
    tri = draw(rng, n, 30)
    tri[7] = (3, 20, 33)
    return Ransac(f"collinear-winner-{method}", p, q, tri, thr=1e-6, method=method)


def _builders():
    b = {}
    for n in EDGE_SIZES:
        for m in METHODS:
            b[f"edge-{n}-{m}"] = functools.partial(edge_case, n, m)
    for nh in NH_EDGES:
        b[f"nh-{nh}"] = functools.partial(nh_case, nh)
    b["nh-65535"] = nh_limit_case
    for k in TIES:
        b[f"tie-{k}"] = functools.partial(tie_case, k)
    for k in ("before", "at", "none", "tiny"):
        b[f"early-{k}"] = functools.partial(early_case, k)
    b["early-tiny-error"] = early_tiny_error_case
    for k in ("more", "max"):
        b[f"early-equal-{k}"] = functools.partial(early_equal_case, k)
    b["count-3"] = lambda: no_inlier_cases()[0]
    b["count-2"] = lambda: no_inlier_cases()[1]
    for m in METHODS:
        b[f"reflection-{m}"] = functools.partial(reflection_case, m)
        b[f"nonfinite-{m}"] = functools.partial(nonfinite_case, m)
        b[f"degenerate-{m}"] = functools.partial(degenerate_case, m)
        b[f"collinear-winner-{m}"] = functools.partial(collinear_winner_case, m)
    for k in ("plane", "slab", "three"):
        b[f"rank2-{k}"] = functools.partial(planar_case, k)
    for k in ("small", "large", "shift"):
        b[f"scale-{k}"] = functools.partial(scaled_case, k)
    return b


BUILDERS = _builders()
EDGE_CASES = [f"edge-{n}-{m}" for n in EDGE_SIZES for m in METHODS]
NH_CASES = [f"nh-{nh}" for nh in NH_EDGES] + ["nh-65535"]
TIE_CASES = [f"tie-{k}" for k in TIES]
EARLY_CASES = ["early-before", "early-at", "early-none", "early-tiny", "early-equal-more", "early-equal-max"]
RANK2_CASES = ["rank2-plane", "rank2-slab", "rank2-three"]
SCALE_CASES = ["scale-small", "scale-large", "scale-shift"]
REFLECTION_CASES = [f"reflection-{m}" for m in METHODS]
NONFINITE_CASES = [f"nonfinite-{m}" for m in METHODS]
# every case compared exactly (all counts, winner, mask, R, t, s): each needs the margin and the conditioning
EXACT_CASES = (EDGE_CASES + NH_CASES + TIE_CASES + EARLY_CASES + RANK2_CASES + SCALE_CASES + REFLECTION_CASES + NONFINITE_CASES +
               ["count-3", "count-2", "early-tiny-error"])
PROPERTY_CASES = [f"degenerate-{m}" for m in METHODS] + [f"collinear-winner-{m}" for m in METHODS]


@functools.lru_cache(maxsize=None)
def ransac_case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def ransac_yardstick(name):
    """ref.ransac_fit_batched of the case: counts, margin, cond, winner, count, mask and (count >= 3) R, t, s."""
    c = ransac_case(name)
    return ref.ransac_fit_batched(c.p, c.q, c.tri, c.thr, c.ratio, c.method)


# ---- Adam ----

@dataclass
class Adam:
    name: str
    p: np.ndarray
    q: np.ndarray
    kw: dict
    holds_ro: bool          # distinct start scales: rotation_orthogonal is determined and compared itself

    @property
    def extent(self):
        return max(1.0, float(np.abs(self.p).max()), float(np.abs(self.q).max()))


RO0 = ref.rotation_about((0.7, 0.1, 0.4), 30.0)
M0 = R0 @ RO0.T @ np.diag([1.1, 0.9, 1.25]) @ RO0
DISTINCT = (0.9, 1.0, 1.2)
ADAM_SIZES = (3, 4, 1023, 1024, 1025, 2049)
REG_CASES = [(ls, lr_, lr) for (ls, lr_) in ((0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.3, 0.3)) for lr in (1e-3, 1e-2)]


def adam_points(n, seed=7, shift=0.0, isotropic=False):
    """fp32-representable pairs (the wrapper rounds to fp32 first): q = M0 p + T0 + noise, or 1.1 R0 p + T0 + noise."""
    rng = np.random.default_rng(seed + n)
    p = (rng.normal(size=(n, 3)) * SPREAD + shift).astype(np.float32).astype(np.float64)
    M = 1.1 * R0 if isotropic else M0
    q = ((p - shift) @ M.T + T0 + shift + rng.normal(size=(n, 3)) * NOISE).astype(np.float32).astype(np.float64)
    return p, q


def _adam_builders():
    b = {}
    for n in ADAM_SIZES:
        b[f"n-{n}-equal"] = lambda n=n: Adam(f"n-{n}-equal", *adam_points(n, isotropic=True), dict(iterations=100, init_scale=1.0), False)
        b[f"n-{n}-distinct"] = lambda n=n: Adam(f"n-{n}-distinct", *adam_points(n), dict(iterations=100, init_scale=DISTINCT), True)
    b["outside"] = lambda: Adam("outside", *adam_points(257), dict(iterations=100, init_scale=(0.5, 1.0, 1.0)), False)
    b["midpoint"] = lambda: Adam("midpoint", *adam_points(257), dict(iterations=100, init_scale=(1.125, 1.125, 1.125)), False)
    b["bounds-wide"] = lambda: Adam("bounds-wide", *adam_points(257), dict(iterations=100, init_scale=DISTINCT, scale_min=0.5,
                                                                              scale_max=2.0), True)
    b["bounds-narrow"] = lambda: Adam("bounds-narrow", *adam_points(257), dict(iterations=100, init_scale=(0.95, 1.0, 1.05),
                                                                                  scale_min=0.9, scale_max=1.1), True)
    for ls, lrot, lr in REG_CASES:
        name = f"reg-{ls}-{lrot}-{lr}"
        b[name] = lambda name=name, ls=ls, lrot=lrot, lr=lr: Adam(name, *adam_points(257), dict(
            iterations=200, init_scale=DISTINCT, lambda_reg_scale=ls, lambda_reg_rot=lrot, lr=lr, loss_every=10), True)
    for shift in (100.0, 1e4):
        name = f"far-{shift:g}"
        b[name] = lambda name=name, shift=shift: Adam(name, *adam_points(1025, shift=shift), dict(iterations=100, init_scale=DISTINCT), True)
    b["one-step"] = lambda: Adam("one-step", *adam_points(257), dict(iterations=1, init_scale=DISTINCT, lambda_reg_scale=0.3,
                                                                       lambda_reg_rot=0.3), True)
    return b


ADAM_BUILDERS = _adam_builders()
ADAM_SIZE_CASES = [f"n-{n}-{k}" for n in ADAM_SIZES for k in ("equal", "distinct")]
ADAM_SCALE_CASES = ["outside", "midpoint", "bounds-wide", "bounds-narrow"]
ADAM_REG_CASES = [f"reg-{ls}-{lrot}-{lr}" for ls, lrot, lr in REG_CASES]
ADAM_FAR_CASES = [f"far-{shift:g}" for shift in (100.0, 1e4)]
ADAM_CASES = ADAM_SIZE_CASES + ADAM_SCALE_CASES + ADAM_REG_CASES + ADAM_FAR_CASES + ["one-step"]
ADAM_ARRAYS = ("rotation", "translation", "scale", "rotation_orthogonal", "M")


@functools.lru_cache(maxsize=None)
def adam_case(name):
    return ADAM_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def adam_yardstick(name):
    """(y, bound): the yardstick's run and, per array, (10 x spread, floor, spread) with spread the largest distance from
    y among the yardstick's other runs (the pairs permuted; the loss written about the centroids) and floor =
    1e-9 max(1, largest |coordinate|)."""
    c = adam_case(name)
    y = ref.adam_9dof(c.p, c.q, **c.kw)
    order = np.random.default_rng(3).permutation(len(c.p))
    others = [ref.adam_9dof(c.p[order], c.q[order], **c.kw), ref.adam_9dof(c.p, c.q, centred=True, **c.kw)]
    bound = {}
    for k in ADAM_ARRAYS:
        spread = max(float(np.abs(o[k] - y[k]).max()) for o in others)
        spread = max(spread, float(np.abs(others[0][k] - others[1][k]).max()))
        bound[k] = (10 * spread, BOUND * c.extent, spread)
    return y, bound
