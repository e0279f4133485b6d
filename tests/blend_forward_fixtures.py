"""Scenes at the edges of `blend_forward_wave_kernel`: a 64-entry chunk, a 16-hit group, the 80-slot ring and its second
lap, the half-group saturation test, the latch in the sign of T, the clamp-free groups on either side of `hot_end`, the
`power > 0` guard and the kept-hit compaction.  Everything is tests.util.make_case plus overrides, seeded; nothing is
read from disk.  FIXTURES maps a name to (builder, what the scene must show); `build(name)` returns (kw, want).

`want` holds the conditions both test modules assert on the geometry they run with:
  n       every block's hit list has exactly n entries, every pixel takes all of them
  s       every pixel takes exactly s - 1 hits: hit s is the one that would take T below 1e-4
  spread  the pixels of some block stop at different hits
  holes   some block's tile list holds hits that pass both selects on a pixel of the block and are taken by none
  clamp   "all": the 0.99 clamp binds on every pixel; "some": on some pixels of a block and not on others
  power   some pixel skips a hit for power > 0 and some pixel takes that splat
  empty   some tile's list is empty and another tile's is not
"""
import math

import numpy as np

from tests.util import make_case

SIZES = [(8, 8), (13, 11), (37, 21)]
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 80, 81, 95, 96, 97, 128, 129, 145, 161]
STOPS = [8, 9, 16, 17, 32, 33, 64, 65, 80, 81]
HOT_RANKS = [0, 15, 16, 63, 64, 79, 80]
BG = (0.3, 0.1, 0.6)


def _depth_order(kw):
    """Splat indices front to back by view-space z (the sort key; ties by index), in float32 as the projection has it."""
    m = np.concatenate([kw["means3D"].astype(np.float32), np.ones((len(kw["means3D"]), 1), np.float32)], 1)
    z = (m @ kw["view"].astype(np.float32))[:, 2]
    return np.argsort(z, kind="stable"), z


def faint(n, size, seed=None, precomp_cov=False):
    """The scene of test_backward_chunk_tail_gpu: n large faint splats (scale ~3, every opacity 0.03) in front of a small
    image - every splat a hit of every pixel and no pixel saturated (0.97^161 = 7e-3)."""
    W, H = size
    kw, _ = make_case(N=n, W=W, H=H, deg=2, seed=30 + n if seed is None else seed, log_scale=math.log(3.0), log_scale_std=0.1,
                      bg=BG, precomp_cov=precomp_cov)
    kw["opacities"] = np.full_like(kw["opacities"], 0.03)
    return kw


# seeds at which one splat falls short of 1/255 on some pixel of one of the three images: the next seed in steps of 1000
_LENGTH_SEED = {63: 1093, 128: 1158, 145: 1175}


def lengths(n, size):
    return faint(n, size, seed=_LENGTH_SEED.get(n)), dict(n=n)


def stops(s, size, n=200):
    """n huge splats (scale ~60: G = 1 to 1e-4 over the image) of ONE opacity a with (1 - a)^(s - 1/2) = 1e-4: after s - 1
    hits T = (1 - a)^(s - 1) is half a hit above 1e-4, and hit s would take it half a hit below."""
    W, H = size
    kw, _ = make_case(N=n, W=W, H=H, deg=1, seed=500 + s, log_scale=math.log(60.0), log_scale_std=0.05, bg=BG)
    a = 1.0 - math.exp(math.log(1e-4) / (s - 0.5))
    kw["opacities"] = np.full_like(kw["opacities"], a)
    return kw, dict(s=s)


def stops_spread(size, n=200):
    """The same kind with a spread of scales: the pixels of one block stop at different hits (the latch, waves that are
    partly finished)."""
    W, H = size
    kw, _ = make_case(N=n, W=W, H=H, deg=1, seed=77, log_scale=math.log(1.0), log_scale_std=0.6, bg=BG)
    kw["opacities"] = np.full_like(kw["opacities"], 0.3)
    return kw, dict(spread=True)


def sparse(size=(37, 21), N=3000):
    """Small splats: many hits pass the exact block test and no pixel takes them (holes in the kept-hit compaction)."""
    W, H = size
    kw, _ = make_case(N=N, W=W, H=H, deg=1, seed=41, log_scale=math.log(0.05), bg=BG)
    return kw, dict(holes=True)


def clamp_switch(rank, size, large):
    """The faint n = 81 list with ONE splat of opacity 0.995 at depth rank `rank`: `hot_end` and the clamp-free groups on
    either side.  The splat is moved onto the optical axis.  large: it is huge (G = 1 everywhere: the clamp binds on
    every pixel); otherwise 0.995 G > 0.99 holds near the image centre only."""
    W, H = size
    kw = faint(81, size)
    order, z = _depth_order(kw)
    i = int(order[rank])
    for k in ("opacities", "scales", "means3D"):
        kw[k] = kw[k].copy()
    kw["opacities"][i] = 0.995
    # onto the optical axis at its own depth (its rank stays: asserted with the scene's conditions)
    view = kw["view"].astype(np.float64)
    kw["means3D"][i] = ((np.array([0.0, 0.0, float(z[i])]) - view[3, :3]) @ np.linalg.inv(view[:3, :3])).astype(np.float32)
    kw["scales"][i] = 60.0 if large else 65.0 / W      # (65 / W: 0.995 G > 0.99 within about two pixels of the centre)
    return kw, dict(clamp="all" if large else "some", hot=i, rank=rank)


def indefinite(rank, size):
    """One cov3D_precomp that is not positive semi-definite (largest eigenvalue negated, as in test_gs3d_gpu's
    _indefinite_case) at depth rank `rank` of a faint 81-list: the `power > 0` guard and kcut = +inf."""
    kw = faint(81, size, seed=900 + rank, precomp_cov=True)
    order, _ = _depth_order(kw)
    i = int(order[rank])
    c = kw["cov3D_precomp"].astype(np.float64)
    S = np.array([[c[i, 0], c[i, 1], c[i, 2]], [c[i, 1], c[i, 3], c[i, 4]], [c[i, 2], c[i, 4], c[i, 5]]])
    w, V = np.linalg.eigh(S)
    w[2] *= -1.0
    S = (V * w) @ V.T
    kw["cov3D_precomp"] = kw["cov3D_precomp"].copy()
    kw["cov3D_precomp"][i] = np.array([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]], np.float32)
    kw["opacities"] = kw["opacities"].copy()
    kw["opacities"][i] = 0.5      # visible: a skipped or wrongly drawn pixel moves the image by far more than the bound
    return kw, dict(power=True, hot=i, rank=rank)


def empty_beside_full(size=(37, 21)):
    """A few small splats: tiles (and blocks) with an empty list beside tiles that have one."""
    W, H = size
    kw, _ = make_case(N=6, W=W, H=H, deg=1, seed=3, log_scale=math.log(0.08), log_scale_std=0.2, bg=BG)
    kw["opacities"] = np.full_like(kw["opacities"], 0.6)
    return kw, dict(empty=True)


FIXTURES = {}
for _n in LENGTHS:
    for _s in SIZES:
        FIXTURES[f"len{_n}-{_s[0]}x{_s[1]}"] = (lengths, (_n, _s))
for _k in STOPS:
    for _s in SIZES[:2] if _k not in (16, 17, 80, 81) else SIZES:
        FIXTURES[f"stop{_k}-{_s[0]}x{_s[1]}"] = (stops, (_k, _s))
for _s in SIZES:
    FIXTURES[f"stops_spread-{_s[0]}x{_s[1]}"] = (stops_spread, (_s,))
FIXTURES["sparse-37x21"] = (sparse, ())
for _r in HOT_RANKS:
    FIXTURES[f"clamp{_r}-all-13x11"] = (clamp_switch, (_r, (13, 11), True))
    FIXTURES[f"clamp{_r}-some-13x11"] = (clamp_switch, (_r, (13, 11), False))
FIXTURES["clamp64-all-37x21"] = (clamp_switch, (64, (37, 21), True))
FIXTURES["clamp64-some-37x21"] = (clamp_switch, (64, (37, 21), False))
for _r in (0, 64):
    for _s in ((13, 11), (37, 21)):
        FIXTURES[f"indefinite{_r}-{_s[0]}x{_s[1]}"] = (indefinite, (_r, _s))
FIXTURES["empty-37x21"] = (empty_beside_full, ())

_built = {}


def build(name):
    if name not in _built:
        fn, args = FIXTURES[name]
        kw, want = fn(*args)
        for v in kw.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _built[name] = (kw, want)
    return _built[name]


def conditions(name, want, r, tile_start):
    """The findings (empty = the scene shows what it is there for) on a float64 blend `r` of the scene."""
    from tests.blend_forward_reference import block_pixels
    bad = []
    nblocks = [(t, q) for t, tile in enumerate(r.tiles) for q in range(4) if block_pixels(tile, q).size]
    if "n" in want:
        n = want["n"]
        if not (r.n_taken == n).all():
            bad.append(f"{name}: pixels take {r.n_taken.min()} .. {r.n_taken.max()} hits, not all {n}")
        if not all(int(tile_start[t + 1] - tile_start[t]) == n for t, _ in nblocks):
            bad.append(f"{name}: a tile's list is not {n} long")
    if "s" in want:
        s = want["s"]
        if not (r.n_taken == s - 1).all():
            bad.append(f"{name}: pixels take {r.n_taken.min()} .. {r.n_taken.max()} hits, not all {s - 1}")
        if min(int(tile_start[t + 1] - tile_start[t]) for t, _ in nblocks) < 2 * s:
            bad.append(f"{name}: a list is shorter than {2 * s}")
    if "rank" in want:
        at = [int(np.nonzero(tile.ids == want["hot"])[0][0]) if (tile.ids == want["hot"]).any() else -1 for tile in r.tiles]
        if not any(a == want["rank"] for a in at):      # (the exact tile cull may shorten other tiles' lists in front of it)
            bad.append(f"{name}: the marked splat sits at list positions {at}, nowhere at {want['rank']}")
    if want.get("spread"):
        if not any(len(set(r.n_taken[tile.py[block_pixels(tile, q)], tile.px[block_pixels(tile, q)]].tolist())) > 3
                   for t, tile in enumerate(r.tiles) for q in range(4) if block_pixels(tile, q).size):
            bad.append(f"{name}: no block whose pixels stop at different hits")
        if not (r.final_T < 0.01).mean() > 0.5:
            bad.append(f"{name}: fewer than half of the pixels come near saturation")
    if want.get("holes"):
        holes = sum(int((tile.live[:, block_pixels(tile, q)].any(1) & ~tile.took[:, block_pixels(tile, q)].any(1)).sum())
                    for t, tile in enumerate(r.tiles) for q in range(4) if block_pixels(tile, q).size and len(tile.ids))
        if holes < 10:
            bad.append(f"{name}: only {holes} hits that pass the selects and have no taker")
    if want.get("clamp") == "all" and not (r.n_clamped == 1).all():
        bad.append(f"{name}: the clamp binds on {int((r.n_clamped == 1).sum())} of {r.n_clamped.size} pixels")
    if want.get("clamp") == "some":
        mixed = [1 for t, tile in enumerate(r.tiles) for q in range(4) if block_pixels(tile, q).size
                 and 0 < r.n_clamped[tile.py[block_pixels(tile, q)], tile.px[block_pixels(tile, q)]].sum() < block_pixels(tile, q).size]
        if not mixed:
            bad.append(f"{name}: no block with the clamp on some pixels only ({int(r.n_clamped.sum())} clamped pixels)")
    if want.get("power"):
        took_hot = any((tile.took[tile.ids == want["hot"]]).any() for tile in r.tiles)
        if not ((r.power_skips > 0).any() and took_hot):
            bad.append(f"{name}: power > 0 on {int((r.power_skips > 0).sum())} pixels, indefinite splat taken: {took_hot}")
    if want.get("empty"):
        lens = [int(tile_start[t + 1] - tile_start[t]) for t in range(len(r.tiles))]
        if not (min(lens) == 0 and max(lens) > 0):
            bad.append(f"{name}: tile list lengths {lens}: no empty one beside a full one")
    return bad
