"""A plain blend of the 3DGS forward in numpy, the checks that hold `blend_forward_wave_kernel` to it, and the planted
defects that show the checks bite.  No GPU is needed to import or run anything in here.

INPUTS are the records the kernel itself starts from - `xy`, `depth`, `conic_o`, `rgb` as `scorp_gs3d_debug_geom` hands
them out and the sorted tile lists of `scorp_gs3d_debug_tiles` (on the CPU: the fp32 oracle's `geom()` / `tiles()`) - so
that projection and sorting are common to both sides and every difference belongs to the blend.

THE BLEND (`blend`) walks, per pixel, the WHOLE list of the pixel's tile in order, as oracle/gs3d_oracle.c blend_tile
does: `power > 0` skips, alpha = min(0.99, o exp(power)), alpha < 1/255 skips, T (1 - alpha) < 1e-4 stops the pixel
before that hit.  It applies no 8x8 block cull: the kernel's cull is documented to change no output bit.  Vectorised
over the pixels of a tile, a Python loop over the tile's list; float64, or float32 for the record.

DECISIONS.  Each (pixel, hit) the pixel reaches makes up to three decisions, and each has a margin:
    |255 alpha - 1|,   |T (1 - alpha) / 1e-4 - 1|,   and for a conic that is not positive-definite |power|.
A decision closer than DELTA = 1e-4 is AMBIGUOUS and a pixel with one is an ambiguous pixel: left out of every per-pixel
comparison (it must still be finite and within 2e-2).  DELTA is a condition, not a measurement: it lies ten to a hundred
times above the kernel's relative error in alpha (2^-24 times the block-frame term sum M below, M of order 10 to 100).
The third margin is there because the kernel's `power > 0` guard is exp2(e) <= o (1 + 4e-5) by design (exp_mfma.hpp,
guard_limit_pack): a power within 1e-4 of zero is decided either way.

THE BOUND (first order, float64).  The kernel forms the exponent e = log2(o G) of a hit at a pixel as six block-frame
terms, e = c0 + c1 xl + c2 yl + c3 xl^2 + c4 xl yl + c5 yl^2 (exp_mfma.hpp), and
    M = |L| + |A| X^2 + |B X Y| + |C| Y^2 + (|2 A X| + |B Y|) |xl| + (|2 C Y| + |B X|) |yl| + |A| xl^2 + |B xl yl| + |C| yl^2
is the sum of their magnitudes ((X, Y) = splat centre - block centre, (xl, yl) = pixel - block centre, A, B, C the conic
scaled by log2(e)/2, L = log2(o)).  Every rounding on the way to e is relative to a partial sum of those terms, so
|delta e| <= K_E u M with u = 2^-24 and K_E counted from the code:
     3  the conic's scaling: the record holds fl(-k conic) (one rounding; k = log2(e)/2 is itself a rounded constant: a
        second), and debug_geom hands the conic back as fl(record * fl(-1/k)) (a third), which is what this blend reads
     2  L = v_log_f32(o) in the record: assumed accurate to 1 ulp = two roundings (nobody has measured it here)
     2  X = x - cx and Y = y - cy, one rounding each, and a term holds at most two of those factors
     3  forming c0 (splat_exponent: B Y, the inner fma, the outer fma; likewise C Y, its fma, the outer fma), c1, c2 (two)
    18  the accumulation of the 3 x 6 non-zero products on the matrix core in fp32, one rounding each (the three bf16
        terms of a coefficient are exact and so are the products)
    --
    28
v_exp_f32 is assumed accurate to 1 ulp too (again unmeasured) and counted as two roundings, relative to alpha itself:
    delta raw = raw (ln 2 K_E u M + 2 u),   raw = o G,    delta alpha = delta raw, or 0 where raw - delta raw >= 0.99.
That is propagated through dX / dalpha_i = T_i c_i - S_i / (1 - alpha_i) (S_i = what is blended behind hit i, background
included) to X = colour, depth, and through -T / (1 - alpha_i) to the final T.  The fp32 accumulations add
(2 n + 2) u sum |c_i| w_i, n = hits the pixel took: n for the running sum, n for the rounding of T in
the T chain that every weight w_i = alpha_i T_i inherits, 2 for the products alpha_i T_i and c_i w_i; T itself n u T;
the epilogue's C + T bg and 1 - T one more u each.  THE BAR IS 4 x THIS BOUND (the factor of the TSDF and surfel-map
suites).  No constant here was tuned to what the kernel does.
"""
import math
from types import SimpleNamespace

import numpy as np

DELTA = 1e-4
K_E = 28
U = 2.0 ** -24
FACTOR = 4.0
ALPHA_MAX, ALPHA_MIN, T_MIN = 0.99, 1.0 / 255.0, 1e-4
K_CONIC = 0.5 * math.log2(math.e)
GROSS = 2e-2          # compare_forward's bar: what even an ambiguous pixel has to meet


def _tile_pixels(t, tiles_x, W, H):
    x0, y0 = (t % tiles_x) * 16, (t // tiles_x) * 16
    ys, xs = np.mgrid[y0:min(y0 + 16, H), x0:min(x0 + 16, W)]
    return xs.reshape(-1), ys.reshape(-1)


def _kernel_exponent(g, gid, px, py, truncate_bits16):
    """log2(o G) the way exp_mfma.hpp forms it (block-frame coefficients), in float64; `truncate_bits16` cuts every
    coefficient to its first two bf16 terms (the planted defect)."""
    ca, cb, cc, o = (float(v) for v in g["conic_o"][gid])
    A, B, C, L = -K_CONIC * ca, -2.0 * K_CONIC * cb, -K_CONIC * cc, math.log2(o)
    cx, cy = (px // 8) * 8 + 3.5, (py // 8) * 8 + 3.5
    X, Y, xl, yl = float(g["xy"][gid, 0]) - cx, float(g["xy"][gid, 1]) - cy, px - cx, py - cy
    c = [L + A * X * X + B * X * Y + C * Y * Y, -(2 * A * X + B * Y), -(2 * C * Y + B * X),
         np.full_like(X, A), np.full_like(X, B), np.full_like(X, C)]
    if truncate_bits16:
        cut = []
        for v in c:
            v32 = v.astype(np.float32)
            t0 = (v32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
            r1 = v32 - t0
            t1 = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
            cut.append(t0.astype(np.float64) + t1.astype(np.float64))
        c = cut
    return c[0] + c[1] * xl + c[2] * yl + c[3] * xl * xl + c[4] * xl * yl + c[5] * yl * yl


def _term_sum(g, gid, px, py):
    ca, cb, cc, o = (abs(float(v)) for v in g["conic_o"][gid])
    A, B, C, L = K_CONIC * ca, 2.0 * K_CONIC * cb, K_CONIC * cc, abs(math.log2(o)) if o > 0 else 0.0
    cx, cy = (px // 8) * 8 + 3.5, (py // 8) * 8 + 3.5
    X, Y = np.abs(float(g["xy"][gid, 0]) - cx), np.abs(float(g["xy"][gid, 1]) - cy)
    xl, yl = np.abs(px - cx), np.abs(py - cy)
    return (L + A * X * X + B * X * Y + C * Y * Y + (2 * A * X + B * Y) * xl + (2 * C * Y + B * X) * yl
            + A * xl * xl + B * xl * yl + C * yl * yl)


def blend(geom, tile_start, point_list, W, H, bg, dtype=np.float64, defect=None, delta=DELTA, with_bound=True):
    """The blend described in the module docstring.  `defect` plants one error (see DEFECTS).  Returns a namespace:
      color[3,H,W], depth[H,W], alpha[H,W] (= 1 - T), final_T[H,W], last_id[H,W] (splat, -1 = none), n_taken[H,W],
      ambiguous[H,W], n_clamped[H,W] (hits taken at raw alpha > 0.99), power_skips[H,W],
      b_color[3,H,W], b_depth[H,W], b_T[H,W]  (the bound, float64 runs only),
      tiles: per tile a namespace (ids, px, py, took[n,P], maybe[n,P], live[n,P], amb[P]), and tile_start / W / H / tiles_x."""
    dt = np.dtype(dtype)
    f = dt.type
    defect = defect or {}
    g = {k: np.asarray(geom[k]) for k in ("xy", "depth", "conic_o", "rgb")}
    xy, dep, co, rgb = (g[k].astype(dt) for k in ("xy", "depth", "conic_o", "rgb"))
    bg = np.asarray(bg, dt).reshape(3)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    r = SimpleNamespace(W=W, H=H, tiles_x=tiles_x, tile_start=np.asarray(tile_start, np.int64), dtype=dt, delta=delta,
                        color=np.zeros((3, H, W), dt), depth=np.zeros((H, W), dt), alpha=np.zeros((H, W), dt),
                        final_T=np.ones((H, W), dt), last_id=np.full((H, W), -1, np.int64), n_taken=np.zeros((H, W), np.int64),
                        ambiguous=np.zeros((H, W), bool), n_clamped=np.zeros((H, W), np.int64),
                        power_skips=np.zeros((H, W), np.int64), b_color=np.zeros((3, H, W)), b_depth=np.zeros((H, W)),
                        b_T=np.zeros((H, W)), tiles=[])
    half, amax, amin, tmin, one = f(0.5), f(ALPHA_MAX), f(ALPHA_MIN), f(T_MIN), f(1.0)
    for t in range(tiles_x * tiles_y):
        px, py = _tile_pixels(t, tiles_x, W, H)
        ids = np.asarray(point_list[r.tile_start[t]:r.tile_start[t + 1]], np.int64)
        if "drop" in defect:
            ids_run = np.delete(ids, defect["drop"]) if defect["drop"] < len(ids) else ids
        elif "twice" in defect and defect["twice"] < len(ids):
            ids_run = np.insert(ids, defect["twice"], ids[defect["twice"]])
        elif "swap" in defect and defect["swap"] + 1 < len(ids):
            ids_run = ids.copy()
            k = defect["swap"]
            ids_run[k], ids_run[k + 1] = ids[k + 1], ids[k]
        else:
            ids_run = ids
        n, P = len(ids_run), len(px)
        fx, fy = px.astype(dt), py.astype(dt)
        T = np.ones(P, dt)
        alive = np.ones(P, bool)
        acc = np.zeros((4, P), dt)
        last = np.full(P, -1, np.int64)
        amb = np.zeros(P, bool)
        first_amb = np.full(P, n, np.int64)
        took = np.zeros((n, P), bool)
        maybe = np.zeros((n, P), bool)
        live_k = np.zeros((n, P), bool)   # passes the two selects, whatever T is
        al_k = np.zeros((n, P), dt)       # the alpha a pixel blended (0 = not taken)
        raw_k = np.zeros((n, P), dt)
        Tb_k = np.zeros((n, P), dt)       # T in front of the hit
        for k, gid in enumerate(ids_run):
            ca, cb, cc, o = co[gid]
            if defect.get("bf16x2"):
                e2 = _kernel_exponent(g, gid, px.astype(np.float64), py.astype(np.float64), True)
                power = ((e2 - math.log2(float(o))) / math.log2(math.e)).astype(dt)
                raw = np.exp2(e2).astype(dt)
            else:
                dx, dy = xy[gid, 0] - fx, xy[gid, 1] - fy
                power = -half * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
                raw = o * np.exp(power)
            alpha = raw if defect.get("no_clamp") else np.minimum(amax, raw)
            guard = np.ones(P, bool) if defect.get("no_power_guard") else power <= 0
            live = guard if defect.get("no_select") else guard & (alpha >= amin)
            test_T = T * (one - alpha)
            stop = alive & live & (test_T < tmin)
            take = alive & live & ~stop
            if defect.get("blend_saturating"):
                take = alive & live
            # margins of the decisions the pixel makes here
            near = np.abs(255.0 * alpha.astype(np.float64) - 1.0) < delta
            near |= live & (np.abs(test_T.astype(np.float64) / T_MIN - 1.0) < delta)
            if not (ca > 0 and cc > 0 and float(ca) * float(cc) - float(cb) * float(cb) > 0):
                near |= np.abs(power.astype(np.float64)) < delta
            near &= alive
            first_amb = np.where(near & ~amb, k, first_amb)
            amb |= near
            # what a pixel whose decisions are open from `first_amb` on may still take
            maybe[k] = (255.0 * alpha.astype(np.float64) >= 1.0 - delta) & (power.astype(np.float64) <= delta)
            w = np.where(take, alpha * T, f(0.0))
            acc[0] += rgb[gid, 0] * w; acc[1] += rgb[gid, 1] * w; acc[2] += rgb[gid, 2] * w; acc[3] += dep[gid] * w
            took[k], raw_k[k], Tb_k[k], live_k[k] = take, raw, T, live
            al_k[k] = np.where(take, alpha, f(0.0))
            T = np.where(take, test_T, T)
            last = np.where(take, gid, last)
            r.n_clamped[py, px] += take & (raw > amax)
            r.power_skips[py, px] += alive & ~guard
            alive &= ~stop
        r.color[:, py, px] = acc[:3] + T[None, :] * bg[:, None]
        r.depth[py, px], r.final_T[py, px], r.alpha[py, px] = acc[3], T, one - T
        r.last_id[py, px], r.n_taken[py, px], r.ambiguous[py, px] = last, took.sum(0), amb
        maybe = took | (maybe & (np.arange(n)[:, None] >= first_amb[None, :]))
        r.tiles.append(SimpleNamespace(ids=ids_run, px=px, py=py, took=took, maybe=maybe, live=live_k, amb=amb))
        if with_bound and dt == np.float64 and n:
            M = np.stack([_term_sum(g, gid, px.astype(np.float64), py.astype(np.float64)) for gid in ids_run])
            d_raw = raw_k * (math.log(2.0) * K_E * U * M + 2.0 * U)
            d_al = np.where(took & (raw_k - d_raw < ALPHA_MAX), d_raw, 0.0)
            inv = 1.0 / (1.0 - al_k)
            w = al_k * Tb_k
            nt = took.sum(0)
            chans = [(rgb[ids_run, c].astype(np.float64), float(bg[c])) for c in range(3)] + [(dep[ids_run].astype(np.float64), 0.0)]
            for ci, (cv, bgc) in enumerate(chans):
                cw = cv[:, None] * w
                behind = np.cumsum(cw[::-1], 0)[::-1] - cw + T[None, :] * bgc     # S_i: everything behind hit i
                b = (d_al * np.abs(Tb_k * cv[:, None] - behind * inv)).sum(0) + (2 * nt + 2) * U * np.abs(cw).sum(0)
                if ci < 3:
                    r.b_color[ci, py, px] = b + 2 * U * (np.abs(acc[ci]) + np.abs(T * bgc))
                else:
                    r.b_depth[py, px] = b
            r.b_T[py, px] = T * ((d_al * inv).sum(0) + (nt + 1) * U) + U
    return r


# ---------------------------------------------------------------------------------------------------------------------
# What the kernel leaves, formed from a blend: the shape of the data the checks take
# ---------------------------------------------------------------------------------------------------------------------
def block_pixels(tile, quad):
    """Index (into the tile's pixel vectors) of the pixels of block `quad` = 2 (lower half) + (right half)."""
    return np.nonzero((((tile.py % 16) >= 8) * 2 + ((tile.px % 16) >= 8)) == quad)[0]


def expected_lists(r):
    """{(t, quad): (certain ids in list order, set of either ids)} for every block that has pixels."""
    out = {}
    for t, tile in enumerate(r.tiles):
        for quad in range(4):
            sel = block_pixels(tile, quad)
            if sel.size == 0:
                continue
            kept = sel[~tile.amb[sel]]
            certain = tile.took[:, kept].any(1) if kept.size else np.zeros(len(tile.ids), bool)
            either = tile.maybe[:, sel[tile.amb[sel]]].any(1) & ~certain if (tile.amb[sel]).any() else np.zeros(len(tile.ids), bool)
            out[t, quad] = (tile.ids[certain], set(tile.ids[either].tolist()))
    return out


def as_kernel_outputs(r, defect=None):
    """A blend in the form `scorp_gs3d_render` + `scorp_gs3d_debug_blend` give it: images, final_T, n_contrib (1-based
    position in the block's compacted hit list), hits[4 * num_pairs] in raster tile order, block_hits[tiles * 4].
    `defect` plants an error of the bookkeeping (see DEFECTS)."""
    defect = defect or {}
    H, W = r.H, r.W
    num_pairs = int(r.tile_start[-1])
    hits = np.full(4 * max(num_pairs, 1), 0xFFFFFFFF, np.uint32)
    block_hits = np.zeros(len(r.tiles) * 4, np.uint32)
    n_contrib = np.zeros((H, W), np.uint32)
    for t, tile in enumerate(r.tiles):
        n = len(tile.ids)
        for quad in range(4):
            sel = block_pixels(tile, quad)
            if sel.size == 0 or n == 0:
                continue
            taken = tile.took[:, sel].any(1)
            listed = taken.copy()
            if defect.get("keep_no_taker") and taken.any():
                free = np.nonzero(~tile.maybe[:np.nonzero(taken)[0][-1], sel].any(1))[0]
                if free.size:
                    listed[free[free.size // 2]] = True
            counted = tile.live[:, sel].any(1) | taken if defect.get("uncompacted") else listed
            pos_all = np.cumsum(counted)                                  # 1-based position of entry k where counted
            any_took = tile.took[:, sel].any(0)
            lastk = n - 1 - np.argmax(tile.took[::-1][:, sel], 0)
            nc = np.where(any_took, pos_all[lastk], 0)
            lst = tile.ids[listed]
            if defect.get("drop_taken") and len(lst) > 1:
                lst = np.delete(lst, len(lst) // 2)
            if defect.get("off_by_one"):
                nc = np.where(nc > 0, nc + 1, 0)
            room = int(r.tile_start[t + 1] - r.tile_start[t])
            lst = lst[:room]
            n_contrib[tile.py[sel], tile.px[sel]] = nc
            b = quad * num_pairs + int(r.tile_start[t])
            hits[b:b + len(lst)] = lst
            block_hits[t * 4 + quad] = max(len(lst), int(nc.max()))
    f32 = lambda a: np.asarray(a, np.float32)
    return dict(color=f32(r.color), depth=f32(r.depth), alpha=f32(r.alpha), final_T=f32(r.final_T), n_contrib=n_contrib,
                hits=hits, block_hits=block_hits)


# ---------------------------------------------------------------------------------------------------------------------
# The checks (the GPU test and the planted-defect test call the same three): each returns a list of findings, empty = pass
# ---------------------------------------------------------------------------------------------------------------------
def check_images(got, r, factor=FACTOR, stats=None):
    """Colour, depth, alpha and final_T on every kept pixel within factor x the bound of the float64 blend; every pixel
    finite and within 2e-2 (colour, alpha, T) of it."""
    bad = []
    keep = ~r.ambiguous
    worst = {}
    for name, ref, bound in (("color", r.color, r.b_color), ("depth", r.depth, r.b_depth), ("alpha", r.alpha, r.b_T),
                             ("final_T", r.final_T, r.b_T)):
        g = np.asarray(got[name], np.float64).reshape(ref.shape)
        if not np.isfinite(g).all():
            bad.append(f"{name}: non-finite values")
            continue
        err = np.abs(g - ref)
        k = np.broadcast_to(keep, err.shape)
        ratio = np.where(k, err / np.maximum(bound, 1e-300), 0.0)
        worst[name] = (float(np.where(k, err, 0).max()), float(np.where(k, bound, 0).max()), float(ratio.max()))
        if (ratio > factor).any():
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            bad.append(f"{name}: {int((ratio > factor).sum())} kept values beyond {factor:g} x the bound; worst at {i}: "
                       f"|err| {err[i]:.3e}, bound {bound[i]:.3e}")
        if name != "depth" and (err > GROSS).any():
            bad.append(f"{name}: {int((err > GROSS).sum())} values (ambiguous ones included) off by more than {GROSS:g}")
    if stats is not None:
        stats.update(worst)
    return bad


def check_n_contrib(got, r, tile_start):
    """For every kept pixel: n_contrib is 0 exactly when the float64 blend finds no contributor; otherwise entry
    n_contrib - 1 of its block's hit list is the splat float64 names as its last contributor."""
    bad = []
    num_pairs = int(tile_start[-1])
    nc = np.asarray(got["n_contrib"]).reshape(r.H, r.W).astype(np.int64)
    hits = np.asarray(got["hits"])
    for t, tile in enumerate(r.tiles):
        n = int(tile_start[t + 1] - tile_start[t])
        for j in np.nonzero(~tile.amb)[0]:
            x, y = int(tile.px[j]), int(tile.py[j])
            want, c = int(r.last_id[y, x]), int(nc[y, x])
            if (c == 0) != (want < 0):
                bad.append(f"pixel ({x}, {y}): n_contrib {c}, float64's last contributor {want}")
            elif c > n:
                bad.append(f"pixel ({x}, {y}): n_contrib {c} beyond its tile's {n} entries")
            elif c > 0:
                quad = ((y % 16) >= 8) * 2 + ((x % 16) >= 8)
                have = int(hits[quad * num_pairs + int(tile_start[t]) + c - 1])
                if have != want:
                    bad.append(f"pixel ({x}, {y}): hits[n_contrib - 1] = {have}, float64's last contributor {want}")
    return bad[:20]


def check_hit_lists(got, r, tile_start):
    """For every block, the prefix of its hit list up to max n_contrib: every entry a certain or an either hit; without
    the either hits it IS the certain list, in order; no splat twice; block_hits between that length and the tile's."""
    bad = []
    num_pairs = int(tile_start[-1])
    nc = np.asarray(got["n_contrib"]).reshape(r.H, r.W).astype(np.int64)
    hits, bh = np.asarray(got["hits"]), np.asarray(got["block_hits"])
    for (t, quad), (certain, either) in expected_lists(r).items():
        tile = r.tiles[t]
        sel = block_pixels(tile, quad)
        n = int(tile_start[t + 1] - tile_start[t])
        ln = int(nc[tile.py[sel], tile.px[sel]].max())
        tag = f"block ({t}, {quad})"
        if ln > n:
            bad.append(f"{tag}: max n_contrib {ln} beyond the tile's {n} entries")
            continue
        b = quad * num_pairs + int(tile_start[t])
        lst = hits[b:b + ln].astype(np.int64)
        if len(np.unique(lst)) != len(lst):
            bad.append(f"{tag}: a splat appears twice in the hit list")
        cset = set(certain.tolist())
        strangers = [int(v) for v in lst if int(v) not in cset and int(v) not in either]
        if strangers:
            bad.append(f"{tag}: entries no pixel can have taken: {strangers[:8]}")
        core = np.array([v for v in lst if int(v) not in either or int(v) in cset], np.int64)
        # (certain hits behind the deepest n_contrib cannot exist: a kept pixel that took one has a deeper n_contrib)
        if not np.array_equal(core, certain):
            bad.append(f"{tag}: list without the either hits has {len(core)} entries, the certain list {len(certain)}"
                       + ("" if len(core) != len(certain) else f"; first difference at {int(np.argmax(core != certain))}"))
        if not ln <= int(bh[t * 4 + quad]) <= n:
            bad.append(f"{tag}: block_hits {int(bh[t * 4 + quad])} outside [{ln}, {n}]")
    return bad[:20]


def check_all(got, r, tile_start, stats=None):
    return check_images(got, r, stats=stats) + check_n_contrib(got, r, tile_start) + check_hit_lists(got, r, tile_start)


# Planted defects: name -> (where it is planted, its arguments).  "blend" defects change the arithmetic of `blend`,
# "outputs" defects the bookkeeping of `as_kernel_outputs`.
DEFECTS = {
    "hit 80 dropped": ("blend", dict(drop=80)),
    "last hit of a chunk blended twice": ("blend", dict(twice=63)),
    "two adjacent hits swapped": ("blend", dict(swap=15)),
    "the saturating hit blended": ("blend", dict(blend_saturating=True)),
    "0.99 clamp omitted": ("blend", dict(no_clamp=True)),
    "1/255 select omitted": ("blend", dict(no_select=True)),
    "power > 0 guard omitted": ("blend", dict(no_power_guard=True)),
    "coefficients cut to two bf16 terms": ("blend", dict(bf16x2=True)),
    "n_contrib in the uncompacted list": ("outputs", dict(uncompacted=True)),
    "n_contrib off by one": ("outputs", dict(off_by_one=True)),
    "a hit with no taker kept": ("outputs", dict(keep_no_taker=True)),
    "a taken hit dropped from the list": ("outputs", dict(drop_taken=True)),
}
