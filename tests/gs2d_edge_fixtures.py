"""Surfel scenes whose 2DGS blend backward replays an EXACT number of hits, for the chunk / pair edge tests.

`make_case2d` draws surfels at random; many are seen edge-on or miss the image, so the number drawn says nothing about
the length of a block's hit list.  The scenes here are built by SELECTION instead: a pool is drawn, every surfel's alpha
is evaluated at every pixel in float64 (the oracle's transforms, the reference's formula: alpha = o exp(-min(rho3d,
rho2d) / 2)), and surfels are kept that
  (a) contribute at the anchor pixel (3, 3) with alpha > 1.5 / 255, and
  (b) have no pixel whose alpha lies in [0.8, 1.25] / 255 - no 1 / 255 decision that fp32 and float64 could take
      differently (nor, an addition of the same kind, a pixel whose depth is within 1 % of the near plane).
All n surfels of the scene then blend into the anchor pixel, so its 8x8 block replays exactly n hits; `Scene.check()`
asserts that from the float64 alphas (count == n at the anchor, <= n elsewhere), and along each pixel's running
transmittance T that
  (c) no T is within 1e-3 relative of 0.5 (the median-depth switch), and
  (d) every final T is above 1e-3 (the early stop at 1e-4 stays out; the saturating variant replaces this by "no
      T (1 - alpha) within 1e-3 relative of 1e-4").
(c) does not hold by chance: with every alpha near 0.03 a pixel's T passes 0.5 in steps of 0.015, so one pixel in fifteen
lands inside the band of 0.001, and an image has 64 to 777 pixels.  It is therefore part of the selection: the
candidates that pass (a) and (b) are walked front to back, and one is taken (`Blend.offer`) only if, blended BEHIND those
already taken, it leaves no pixel's T in the band.  The scene of n surfels is the nearest n taken, so every length's
running T is a prefix of the longest scene's.  The float64 table is itself checked against the float64 oracle's alpha map;
nothing here looks at what the kernel under test produces.

Pools (POOL): 600 surfels drawn for 8x8 give 212 candidates; 13x11 takes 6 000 (1 082 candidates, the 97 taken end at the
141st), 37x21 - 777 pixels for (b) and (c) - 48 000 (1 122 candidates, the 97 end at the 498th).  Condition (a) is
evaluated first, at the anchor alone, and the full table only for the few per cent that pass it: about a second in all.
"""
import math

import numpy as np

from tests.test_oracle2d_cpu import make_case2d

ANCHOR = (3, 3)                    # (x, y): inside block (0, 0) of every image size
LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97)
SIZES = ((8, 8), (13, 11), (37, 21))
# surfels drawn per image size so that 97 pass the whole selection (tests/test_gs2d_backward_edges_cpu.py prints the yield)
POOL = {(8, 8): 600, (13, 11): 6000, (37, 21): 48000}
BG = (0.3, 0.1, 0.6)
FAINT = 0.03
A_MIN, A_ANCHOR, A_BAND = 1.0 / 255.0, 1.5 / 255.0, (0.8 / 255.0, 1.25 / 255.0)
NEAR_Z, FILTER_INV_SQ, ALPHA_MAX, T_MIN = 0.2, 2.0, 0.99, 1e-4
SURFEL_KEYS = ("means3D", "opacities", "shs", "scales", "rotations")
GRADS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")


def take(kw, rows):
    q = dict(kw)
    for key in SURFEL_KEYS:
        q[key] = np.ascontiguousarray(kw[key][rows])
    return q


def join(a, b):
    q = dict(a)
    for key in SURFEL_KEYS:
        q[key] = np.ascontiguousarray(np.concatenate([a[key], b[key]], 0))
    return q


def evaluate(g, visible, px, py):
    """The reference's ray-surfel evaluation in float64 at pixels (px, py) (broadcast against a leading surfel axis), from
    the oracle's geometry `g` -> (alpha, 0 where the reference would not evaluate or blend it; use3d; depth)."""
    Tu, Tv, Tw = (g["T"][:, None, None, 3 * r:3 * r + 3] for r in range(3))
    p = np.cross(px[..., None] * Tw - Tu, py[..., None] * Tw - Tv)
    ok = p[..., 2] != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s0, s1 = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
        rho3d = s0 * s0 + s1 * s1
        rho2d = FILTER_INV_SQ * ((g["xy"][:, 0, None, None] - px) ** 2 + (g["xy"][:, 1, None, None] - py) ** 2)
        use3d = rho3d <= rho2d
        depth = np.where(use3d, s0 * Tw[..., 0] + s1 * Tw[..., 1] + Tw[..., 2], Tw[..., 2])
        alpha = np.minimum(ALPHA_MAX, g["nrm_o"][:, 3, None, None] * np.exp(-0.5 * np.minimum(rho3d, rho2d)))
    ok &= np.isfinite(alpha) & np.isfinite(depth) & (depth >= NEAR_Z) & visible[:, None, None]
    return np.where(ok, alpha, 0.0), use3d, depth


class Table:
    """float64, per (surfel, pixel): alpha as the reference evaluates it, whether it is a hit, which branch, p.z."""

    def __init__(self, kw):
        from oracle.gs_oracle import OracleRender2D
        self.oracle = o = OracleRender2D(np.float64, **kw)
        g = o.geom()
        W, H = kw["W"], kw["H"]
        self.W, self.H, self.N = W, H, o.N
        self.T = T = g["T"]
        self.visible = o.radii > 0
        self.depth_key = g["depth"]
        px, py = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
        self.alpha, self.use3d, self.depth = evaluate(g, self.visible, px, py)
        # the reference hands a surfel only to the 16x16 tiles of its rectangle
        x0, y0, x1, y1 = (g["rect"][:, c, None, None] for c in range(4))
        in_rect = (px >= 16 * x0) & (px < 16 * x1) & (py >= 16 * y0) & (py < 16 * y1)
        self.hit = in_rect & (self.alpha >= A_MIN)
        self.order = np.lexsort((np.arange(self.N), self.depth_key))   # front to back: (depth, index)

    def pz_at(self, x, y):
        """Third component of cross(x Tw - Tu, y Tw - Tv): linear in (x, y)."""
        Tu, Tv, Tw = (self.T[:, 3 * r:3 * r + 3].reshape((self.N,) + (1,) * (np.ndim(x) - 1) + (3,)) for r in range(3))
        k, l = np.asarray(x, np.float64)[..., None] * Tw - Tu, np.asarray(y, np.float64)[..., None] * Tw - Tv
        return k[..., 0] * l[..., 1] - k[..., 1] * l[..., 0]

    def qualifies(self):
        """Conditions (a) and (b) per surfel."""
        ax, ay = ANCHOR
        a = self.hit[:, ay, ax] & (self.alpha[:, ay, ax] > A_ANCHOR)
        knife = (self.alpha >= A_BAND[0]) & (self.alpha <= A_BAND[1])
        near = (self.alpha >= A_BAND[0]) & (np.abs(self.depth / NEAR_Z - 1.0) < 0.01)
        return a & ~knife.any((1, 2)) & ~near.any((1, 2))

    def blend(self):
        """The reference's front-to-back loop per pixel -> (hits blended [H, W], final T [H, W], every running T and every
        tested T (1 - alpha) as two flat arrays)."""
        T = np.ones((self.H, self.W))
        going = np.ones((self.H, self.W), bool)
        count = np.zeros((self.H, self.W), int)
        running, tested = [], []
        for i in self.order:
            h = self.hit[i] & going
            test = T * (1.0 - self.alpha[i])
            tested.append(test[h])
            going &= ~(h & (test < T_MIN))
            h &= going
            T = np.where(h, test, T)
            count += h
            running.append(T[h])
        return count, T, np.concatenate(running) if running else np.zeros(0), np.concatenate(tested) if tested else np.zeros(0)


class Scene:
    def __init__(self, name, kw, n=None, saturating=False):
        self.name, self.kw, self.n, self.saturating = name, kw, n, saturating
        self._table = None

    @property
    def size(self):
        return self.kw["W"], self.kw["H"]

    def table(self):
        if self._table is None:
            self._table = Table(self.kw)
        return self._table

    def check(self):
        """The conditions of the module docstring, from float64 alone.  -> the table."""
        t = self.table()
        ax, ay = ANCHOR
        assert t.visible.all() and t.qualifies().all(), f"{self.name}: a surfel misses (a) or (b)"
        count, T_final, running, tested = t.blend()
        assert np.abs((1.0 - T_final) - t.oracle.allmap[1]).max() < 1e-12, f"{self.name}: the table is not the oracle's blend"
        assert (count <= t.N).all()
        if self.saturating:
            assert (np.abs(tested / T_MIN - 1.0) > 1e-3).all(), f"{self.name}: a pixel stops on a knife edge"
        else:
            assert count[ay, ax] == t.N, f"{self.name}: the anchor block replays {count[ay, ax]} hits, not {t.N}"
            assert T_final.min() > 1e-3, f"{self.name}: (d) final T {T_final.min():.3e}"
        assert self.n is None or t.N == self.n
        assert (np.abs(running / 0.5 - 1.0) > 1e-3).all(), f"{self.name}: (c) a running T within 1e-3 of 0.5"
        return t


def pool_case(size, n_pool, seed, log_scale=math.log(8.0), opacity=FAINT):
    W, H = size
    kw, _ = make_case2d(N=n_pool, W=W, H=H, deg=2, seed=seed, log_scale=log_scale, bg=BG)
    if opacity is not None:
        kw["opacities"] = np.full_like(kw["opacities"], opacity)
    return kw


class Candidates:
    """The surfels of a pool that pass (a) and (b), front to back, with their float64 alpha maps (0 where a surfel is no
    hit)."""

    def __init__(self, kw, chunk=1200):
        from oracle.gs_oracle import OracleRender2D
        o = OracleRender2D(np.float64, **kw)       # (a) first, at the anchor alone: the full table only for those that pass it
        at_anchor = evaluate(o.geom(), o.radii > 0, np.full((1, 1, 1), float(ANCHOR[0])), np.full((1, 1, 1), float(ANCHOR[1])))[0]
        first = np.nonzero(at_anchor[:, 0, 0] > A_ANCHOR)[0]
        rows, alphas, depths = [], [], []
        for lo in range(0, first.size, chunk):
            t = Table(take(kw, first[lo:lo + chunk]))
            idx = np.nonzero(t.qualifies())[0]
            rows.append(first[lo:lo + chunk][idx])
            alphas.append(np.where(t.hit[idx], t.alpha[idx], 0.0))
            depths.append(t.depth_key[idx])
        rows, alphas, depths = np.concatenate(rows), np.concatenate(alphas), np.concatenate(depths)
        order = np.lexsort((rows, depths))
        self.kw, self.rows, self.alpha, self.depth = kw, rows[order], alphas[order], depths[order]

    def subset(self, mask):
        sub = Candidates.__new__(Candidates)
        sub.kw, sub.rows, sub.alpha, sub.depth = self.kw, self.rows[mask], self.alpha[mask], self.depth[mask]
        return sub


class Blend:
    """The reference's front-to-back loop over the image, one surfel at a time.  `offer` adds a surfel BEHIND those taken so
    far unless a pixel's transmittance would then sit on a switch: (c) a running T within 1e-3 relative of 0.5, (d) a final
    T down to 1e-3 - saturating scenes: a tested T (1 - alpha) within 1e-3 relative of the early stop at 1e-4 instead."""

    def __init__(self, size, saturating=False):
        self.T = np.ones((size[1], size[0]))
        self.going = np.ones((size[1], size[0]), bool)
        self.saturating = saturating

    def offer(self, alpha):
        h = (alpha > 0) & self.going
        test = self.T * (1.0 - alpha)
        stop = h & (test < T_MIN)
        blended = h & ~stop
        bad = (np.abs(test[blended] / 0.5 - 1.0) <= 1e-3).any()
        if self.saturating:
            bad |= (np.abs(test[h] / T_MIN - 1.0) <= 1e-3).any()
        else:
            bad |= stop.any() or test[blended].min(initial=1.0) <= 1e-3
        if bad:
            return False
        self.T = np.where(blended, test, self.T)
        self.going &= ~stop
        return True


def pick(cands, n, blend, behind=-np.inf, at_least=None):
    """The first n candidates (front to back, farther than `behind`) that `blend` takes -> their rows in the pool."""
    rows = []
    for row, alpha, depth in zip(cands.rows, cands.alpha, cands.depth):
        if len(rows) < n and depth > behind and blend.offer(alpha):
            rows.append(row)
    assert len(rows) >= (n if at_least is None else at_least), f"only {len(rows)} of {n} surfels found among {cands.rows.size} candidates"
    return np.asarray(rows)


_scenes = {}


def _cached(key, build):
    if key not in _scenes:
        _scenes[key] = build()
    return _scenes[key]


def edge_pool(size):
    """(the pool, its candidates, the max(LENGTHS) rows taken front to back): the scene of n surfels is the nearest n."""
    def build():
        kw = pool_case(size, POOL[size], 50 + size[0])
        cands = Candidates(kw)
        return kw, cands, pick(cands, max(LENGTHS), Blend(size))
    return _cached(("pool", size), build)


def edge_scene(n, size):
    """n surfels on a size = (W, H) image, all n of them hits of the anchor pixel's block."""
    def build():
        kw, _, rows = edge_pool(size)
        return Scene(f"n{n}_{size[0]}x{size[1]}", take(kw, rows[:n]), n=n)
    return _cached(("edge", n, size), build)


VARIANT_SIZE = (13, 11)


def saturating_scene():
    """Variant 1: opacities 0.6 .. 0.95 - pixels stop at different depths (`last` differs, `pos1 <= last` masks lanes)."""
    def build():
        kw = pool_case(VARIANT_SIZE, 600, 71, opacity=None)
        kw["opacities"] = np.random.default_rng(71).uniform(0.6, 0.95, kw["opacities"].shape).astype(np.float32)
        rows = pick(Candidates(kw), 40, Blend(VARIANT_SIZE, saturating=True))
        return Scene("saturating", take(kw, rows), saturating=True)
    return _cached("saturating", build)


def lowpass_scene():
    """Variant 2: tiny surfels (0.006 world units: a hundredth of a pixel, the screen-space low-pass rho2d decides) in front
    of large ones.  Both branches occur in the anchor block's list, 12 and 24 hits."""
    def build():
        big_kw, big, _ = edge_pool(VARIANT_SIZE)
        tiny_kw = pool_case(VARIANT_SIZE, 2400, 72, log_scale=math.log(0.006))
        for key in ("view", "proj", "campos", "tanfovx", "tanfovy"):      # (one camera for both pools)
            tiny_kw[key] = big_kw[key]
        tiny = Candidates(tiny_kw)
        blend = Blend(VARIANT_SIZE)
        tiny_rows = pick(tiny, 12, blend)
        big_rows = pick(big, 24, blend, behind=tiny.depth[np.isin(tiny.rows, tiny_rows)].max())
        return Scene("lowpass", join(take(tiny_kw, tiny_rows), take(big_kw, big_rows)))
    return _cached("lowpass", build)


def check_lowpass(scene):
    t = scene.check()
    blk = (slice(None), slice(0, 8), slice(0, 8))
    n3d = int((t.hit[blk] & t.use3d[blk]).any((1, 2)).sum())
    n2d = int((t.hit[blk] & ~t.use3d[blk]).any((1, 2)).sum())
    assert n3d >= 8 and n2d >= 8, f"lowpass: {n3d} hits on the 3-D branch, {n2d} on the low-pass branch in the anchor block"
    return n3d, n2d


def _turned(kw, lo_deg, hi_deg, seed):
    """Every surfel's normal turned to lo .. hi degrees from its viewing direction."""
    rng = np.random.default_rng(seed)
    N = kw["means3D"].shape[0]
    d = kw["means3D"].astype(np.float64) - kw["campos"].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = np.cross(d, rng.normal(0, 1, (N, 3)))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    th = np.radians(rng.uniform(lo_deg, hi_deg, N))[:, None]
    n = np.cos(th) * d + np.sin(th) * e
    u = np.cross(n, rng.normal(0, 1, (N, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n, u)
    R = np.stack([u, v, n], 2)                         # columns: the two tangents, the normal
    w = 0.5 * np.sqrt(np.maximum(1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1e-12))
    w = np.maximum(w, 1e-3)
    q = np.stack([w, (R[:, 2, 1] - R[:, 1, 2]) / (4 * w), (R[:, 0, 2] - R[:, 2, 0]) / (4 * w), (R[:, 1, 0] - R[:, 0, 1]) / (4 * w)], 1)
    keep = 1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] > 0.1       # (away from w ~ 0, where this form of the conversion is poor)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    out = dict(kw)
    out["rotations"] = q.astype(np.float32)
    return take(out, np.nonzero(keep)[0])


def unsteady_hits(t):
    """(block, surfel) hits whose float64 p.z varies over the block's 64 pixels by more than a factor 2 from its value at
    the block centre: the split form cannot take the 1 / p.z scale from the centre there (`Sh == 0`)."""
    n = 0
    for by in range(0, t.H, 8):
        for bx in range(0, t.W, 8):
            if not t.hit[:, by:by + 8, bx:bx + 8].any():
                continue
            pz = t.pz_at((bx + np.arange(8))[None, None, :], (by + np.arange(8))[None, :, None])      # all 64, in the image or not
            pzc = t.pz_at(np.full((1, 1, 1), bx + 3.5), np.full((1, 1, 1), by + 3.5))
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.abs(pz / pzc).reshape(t.N, -1)
            off = (ratio.max(1) > 2.0) | (ratio.min(1) < 0.5)
            n += int((off & t.hit[:, by:by + 8, bx:bx + 8].any((1, 2))).sum())
    return n


def horizon_scene():
    """Variant 3: large surfels turned 80 .. 88 degrees from the view direction; their horizon (p.z = 0) passes near or
    through the blocks."""
    def build():
        kw = _turned(pool_case(VARIANT_SIZE, 2400, 73), 80.0, 88.0, 73)
        return Scene("horizon", take(kw, pick(Candidates(kw), 40, Blend(VARIANT_SIZE))))
    return _cached("horizon", build)


def check_horizon(scene):
    t = scene.check()
    n = unsteady_hits(t)
    assert n >= 8, f"horizon: only {n} (block, surfel) hits with p.z off its centre value by a factor 2"
    return n


def uncovered_scene():
    """Variant 4: the 37x21 selection restricted to surfels that leave one whole 8x8 block without a contributor - and
    scattered pixels of other blocks with it.  -> the scene; `uncovered_mask` gives the pixels."""
    def build():
        size = (37, 21)
        kw, cands, _ = edge_pool(size)
        best = None
        for by in (0, 8):                  # (the blocks that lie wholly inside 37x21)
            for bx in (0, 8, 16, 24):
                free = ~(cands.alpha[:, by:by + 8, bx:bx + 8] > 0).any((1, 2))
                if (bx, by) != (0, 0) and (best is None or free.sum() > best[0].sum()):
                    best = (free, bx, by)
        free, bx, by = best
        return Scene(f"uncovered_block_{bx}_{by}", take(kw, pick(cands.subset(free), 48, Blend(size), at_least=24)))
    return _cached("uncovered", build)


def uncovered_mask(scene):
    """[H, W] bool: pixels no surfel is blended into.  Asserts one whole block and >= 20 pixels in other blocks."""
    t = scene.check()
    none = ~t.hit.any(0)
    whole = [(bx, by) for by in (0, 8) for bx in (0, 8, 16, 24) if none[by:by + 8, bx:bx + 8].all()]
    assert whole, "uncovered: no whole block without a contributor"
    scattered = none.copy()
    for bx, by in whole:
        scattered[by:by + 8, bx:bx + 8] = False
    for by in range(0, t.H, 8):            # count only pixels of blocks that do have contributors
        for bx in range(0, t.W, 8):
            if none[by:by + 8, bx:bx + 8].all():
                scattered[by:by + 8, bx:bx + 8] = False
    assert scattered.sum() >= 20, f"uncovered: {scattered.sum()} scattered pixels without a contributor"
    return none


def upstream(size, seed, maps=True):
    """Seeded upstream gradients (dL/dcolor [3, H, W], dL/dallmap [7, H, W] or None)."""
    W, H = size
    rng = np.random.default_rng(seed + 99)
    wc = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    wa = rng.normal(0, 1, (7, H, W)).astype(np.float32)
    wa[5] *= 0.1                                       # median depth: a selection, keep its weight modest
    return wc, (wa if maps else None)


_oracles = {}


def oracle_grads(scene, key, wc, wa):
    """(float32, float64) oracle gradients for the upstream gradients registered under `key`; computed once, read-only."""
    k = (scene.name, key)
    if k not in _oracles:
        from oracle.gs_oracle import OracleRender2D
        wa_ = np.zeros((7,) + wc.shape[1:], np.float32) if wa is None else wa
        both = []
        for dt in (np.float32, np.float64):
            g = OracleRender2D(dt, **scene.kw).backward(wc, wa_)
            g = {name: np.asarray(g[name]) for name in GRADS}
            for a in g.values():
                a.setflags(write=False)
            both.append(g)
        _oracles[k] = tuple(both)
    return _oracles[k]
