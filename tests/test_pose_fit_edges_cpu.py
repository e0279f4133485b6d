"""The conditions under which tests/test_pose_fit_edges_gpu.py may compare exactly, checked on the float64 yardstick alone
(tests/pose_fit_reference.py on the seeded cases of tests/pose_fit_fixtures.py); no GPU.

  margin        every exactly compared case keeps |residual - threshold| / threshold >= 1e-9 over ALL (hypothesis, pair)
  conditioning  every ordinary triple of such a case has s2 / s1 >= 1e-6
  block edges   the sizes reach the edges of the 1 024-pair blocks (256 threads x 4) they are named for
  structure     the ties, early exits, count-2 / count-3 pair, reflections, planar and collinear inlier sets and non-finite
                pairs are what the case names say, on the yardstick's counts and singular values
  Adam          the two statements of the loss agree; every regulariser case moves M or the scales, under a 1 % change of
                each regulariser term it uses, by at least 100x the bound the GPU test holds the kernel to

The 1e-9 and 1e-6 are the recorded fixture's own conditions (tests/test_pose_fit_cpu.py), an order stricter in the margin.

What the yardstick gives on the fixed seeds (the smallest of each family; printed by the tests):
  family                      margin (>= 1e-9)   s2 / s1 (>= 1e-6)
  block edges (30)            6.5e-7             2.1e-4
  hypothesis counts (7)       1.1e-4             1.3e-3
  ties (6)                    7.0e-6             1.4e-2
  early exits (7)             3.5e-5             4.0e-4
  count 3 / count 2           7.8e-2             7.3e-3
  reflection (2)              1.6e-3             3.0e-4
  rank 2 (3)                  1.0                1.0e-5
  scaled, shifted (3)         2.5e-5             5.7e-3
  non-finite pairs (2)        1.3e-4             2.1e-4
The kernel's distances to the yardstick on an MI355X, with their bounds, are in tests/test_pose_fit_edges_gpu.py: RANSAC
R and s within 2.9e-15 (bound 1e-9) with every count, winner and mask equal; Adam within 3.5e-13 in M (bound 1.2e-9 or more)."""
import numpy as np
import pytest

from tests import pose_fit_fixtures as fx
from tests import pose_fit_reference as ref


def test_sizes_reach_the_block_edges():
    want = {3: (1, 3), 4: (1, 4), 63: (1, 63), 64: (1, 64), 65: (1, 65), 255: (1, 255), 256: (1, 256), 257: (1, 257),
            1023: (1, 1023), 1024: (1, 1024), 1025: (2, 1), 2047: (2, 1023), 2048: (2, 1024), 2049: (3, 1), 3073: (4, 1)}
    assert set(want) == set(fx.EDGE_SIZES)
    for n, (nblk, last) in want.items():
        assert fx.blocks_of(n) == (nblk, last), n
        for m in fx.METHODS:
            c = fx.ransac_case(f"edge-{n}-{m}")
            assert len(c.p) == len(c.q) == n and c.tri.shape == (130, 3) and c.tri.max() < n
    lasts = {fx.blocks_of(n)[1] for n in fx.EDGE_SIZES}
    assert 3 in lasts and 1 in lasts and fx.CHUNK in lasts                    # the minimum, one pair, a full block
    assert any(l < fx.WAVE for l in lasts) and any(fx.WAVE < l < 256 for l in lasts)   # shorter than a wave; than one pass of the block
    assert max(fx.blocks_of(n)[0] for n in fx.EDGE_SIZES) >= 3
    assert {fx.blocks_of(n) for n in fx.ADAM_SIZES} == {(1, 3), (1, 4), (1, 1023), (1, 1024), (2, 1), (3, 1)}
    for name in fx.NH_CASES:                                                   # the one-wave selection: lanes x strides
        assert len(fx.ransac_case(name).tri) == int(name.split("-")[1])
    assert len(fx.ransac_case("nh-65535").tri) == 65535 and len(fx.ransac_case("nh-65535").p) == 8


@pytest.mark.parametrize("name", fx.EXACT_CASES)
def test_exact_cases_have_the_margin_and_the_conditioning(name):
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    print(f"{name}: margin {y['margin']:.3g}, s2/s1 {y['cond']:.3g}, winner {y['winner']} with {y['count']} of {len(c.p)}")
    assert y["margin"] >= fx.MIN_MARGIN
    assert y["cond"] >= fx.MIN_COND
    assert y["mask"].sum() == y["count"]
    if name not in ("count-2", "early-tiny-error"):
        assert y["count"] >= 3 and np.isfinite(y["R"]).all() and np.isfinite(y["t"]).all() and np.isfinite(y["s"])


@pytest.mark.parametrize("name", ["edge-3-kabsch", "edge-65-umeyama", "edge-1025-kabsch", "tie-lanes", "early-equal-more",
                                  "degenerate-umeyama", "count-2"])
def test_batched_counts_are_the_loop_counts(name):
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    try:
        r = ref.ransac_fit(c.p, c.q, c.tri, c.thr, c.ratio, c.method)
    except ValueError:
        assert y["count"] < 3
        return
    assert np.array_equal(r["counts"], y["counts"]) and r["winner"] == y["winner"] and np.array_equal(r["mask"], y["mask"])
    assert np.array_equal(r["R"], y["R"]) and np.array_equal(r["t"], y["t"]) and r["s"] == y["s"]


def test_the_limit_case_repeats_every_triple():
    c, y = fx.ransac_case("nh-65535"), fx.ransac_yardstick("nh-65535")
    keys, inverse = np.unique(c.tri, axis=0, return_inverse=True)
    assert len(keys) == 8 * 7 * 6 and np.bincount(inverse.reshape(-1)).min() > 64
    top = np.nonzero(y["counts"] == y["counts"].max())[0]
    assert len(top) > 1000 and y["winner"] == top[0]                           # the tie rule at scale
    assert len({int(h) % fx.WAVE for h in top}) == fx.WAVE                      # maxima in every lane


@pytest.mark.parametrize("kind", list(fx.TIES))
def test_ties_sit_where_the_names_say(kind):
    nh, slots = fx.TIES[kind]
    y = fx.ransac_yardstick(f"tie-{kind}")
    assert len(y["counts"]) == nh
    assert set(np.nonzero(y["counts"] == y["counts"].max())[0]) == set(slots)   # the copies hold the maximum, nothing else does
    assert y["winner"] == min(slots)
    lanes = [s % fx.WAVE for s in slots]
    if kind == "lanes":
        assert len(set(lanes)) == 3 and min(slots) != slots[0]
    if kind == "strides":
        assert len(set(lanes)) == 1 and len({s // fx.WAVE for s in slots}) == 3
    if kind in ("late", "last"):
        assert nh % fx.WAVE != 0 and max(slots) == nh - 1
    if kind == "small":
        assert nh < fx.WAVE


def test_early_exits_are_where_the_names_say():
    base = fx.ransac_yardstick("early-none")
    c, g = base["counts"], 70
    assert int(np.argmax(c)) == g and (c == c.max()).sum() > 1                  # the first of several maxima
    assert base["winner"] == g and base["iterations"] == len(c)                 # nothing exceeds: the first maximum
    assert not (c > fx.ransac_case("early-none").ratio * 257).any()
    y = fx.ransac_yardstick("early-at")
    assert y["winner"] == g and y["iterations"] == g + 1
    y, f = fx.ransac_yardstick("early-before"), fx.ransac_case("early-before").note["f"]
    assert y["winner"] == f < g and 3 <= c[f] < c[g] and (c[:f] < c[f]).all()
    y = fx.ransac_yardstick("early-tiny")
    assert y["counts"][0] == 0 and y["winner"] == 1 and 3 <= y["count"] < y["counts"].max()
    y = fx.ransac_yardstick("early-tiny-error")
    assert y["counts"][0] == 0 and y["winner"] == 1 and y["count"] in (1, 2) and y["R"] is None
    c = fx.ransac_case("early-tiny-error")
    with pytest.raises(ValueError, match="No inliers found in RANSAC."):
        ref.ransac_fit(c.p, c.q, c.tri, c.thr, c.ratio)


def test_a_count_equal_to_the_ratio_does_not_exceed_it():
    for kind in ("more", "max"):
        c, y = fx.ransac_case(f"early-equal-{kind}"), fx.ransac_yardstick(f"early-equal-{kind}")
        assert len(c.p) == 1000 and c.ratio * len(c.p) == 500.0
        h = c.note["h"]
        assert y["counts"][h] == 500
        if kind == "more":
            assert h == 3 and (y["counts"][:3] < 500).all() and y["winner"] > 3 and y["count"] > 500
            assert y["winner"] == np.nonzero(y["counts"] > 500)[0][0]
        else:
            assert y["counts"].max() == 500 and y["winner"] == h == np.argmax(y["counts"]) and y["iterations"] == 130


def test_the_no_inlier_boundary_is_one_pair_wide():
    a, b = fx.ransac_case("count-3"), fx.ransac_case("count-2")
    assert np.array_equal(a.p, b.p) and np.array_equal(a.tri, b.tri) and (a.q != b.q).any(axis=1).sum() == 1
    ya, yb = fx.ransac_yardstick("count-3"), fx.ransac_yardstick("count-2")
    assert ya["counts"].max() == 3 and ya["count"] == 3 and ya["R"] is not None
    assert yb["counts"].max() == 2 and yb["count"] == 2 and yb["R"] is None
    assert ya["counts"][0] == 0 and ya["winner"] == yb["winner"] == 1


def _final_covariance(c, y):
    p, q = c.p[y["mask"]], c.q[y["mask"]]
    U, S, Vt = np.linalg.svd((p - p.mean(axis=0)).T @ (q - q.mean(axis=0)))
    return U, S, Vt


@pytest.mark.parametrize("name", fx.REFLECTION_CASES)
def test_reflections_take_the_determinant_branch_at_full_rank(name):
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    assert y["count"] == len(c.p)                                             # every pair is an inlier of the winner
    U, S, Vt = _final_covariance(c, y)
    assert S[2] / S[0] > 1e-3 and np.linalg.det(U) * np.linalg.det(Vt) < 0
    assert abs(np.linalg.det(y["R"]) - 1) < 1e-12
    if c.method == "umeyama":                                                 # the rule reaches the scale: (S0 + S1 - S2) / spp
        spp = ((c.p - c.p.mean(axis=0)) ** 2).sum()
        assert abs(y["s"] - (S[0] + S[1] - S[2]) / spp) < 1e-12 and y["s"] < (S.sum() / spp) * 0.99


def test_planar_inliers_give_rank_two_in_the_final_fit():
    for name, rel in (("rank2-plane", 1e-15), ("rank2-slab", 1e-13), ("rank2-three", 1e-15)):
        c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
        U, S, Vt = _final_covariance(c, y)
        print(f"{name}: {y['count']} inliers, singular values {S}")
        assert S[1] / S[0] >= 1e-3 and S[2] / S[0] < rel, name               # below svd3's 1e-13 rank threshold
        assert (y["count"] == 3) == (name == "rank2-three")
    assert (fx.ransac_case("rank2-plane").p[:, 2] == 0).all()
    z = fx.ransac_case("rank2-slab").p[:, 2]
    assert 0 < np.abs(z).max() <= 1e-14 * fx.SPREAD


def test_the_thin_slab_answer_under_a_permutation_of_the_pairs():
    """Which bound the GPU test uses for rank2-slab: 1e-9 unless the yardstick itself moves by more under a permutation."""
    print("rank2-slab: the yardstick's permutation spread", slab_spread())
    assert slab_spread() <= fx.BOUND                                          # so the plain exact bound applies


def slab_spread():
    c, y = fx.ransac_case("rank2-slab"), fx.ransac_yardstick("rank2-slab")
    order = np.random.default_rng(5).permutation(int(y["count"]))
    R, t, s = ref.similarity_fit(c.p[y["mask"]][order], c.q[y["mask"]][order])
    return max(np.abs(R - y["R"]).max(), np.abs(t - y["t"]).max(), abs(s - y["s"]))


@pytest.mark.parametrize("kind", ["small", "large", "shift"])
def test_scaled_and_shifted_variants_count_what_the_base_counts(kind):
    base, y = fx.ransac_yardstick("edge-1025-umeyama"), fx.ransac_yardstick(f"scale-{kind}")
    c = fx.ransac_case(f"scale-{kind}")
    assert np.array_equal(y["counts"], base["counts"]) and np.array_equal(y["mask"], base["mask"])
    assert {"small": c.extent == 1.0, "large": c.extent > 1e5, "shift": c.extent > 1e5}[kind]


@pytest.mark.parametrize("name", fx.NONFINITE_CASES)
def test_non_finite_pairs_are_sampled_and_count_nothing(name):
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    bad = ~(np.isfinite(c.p).all(axis=1) & np.isfinite(c.q).all(axis=1))
    assert set(np.nonzero(bad)[0]) == set(c.note["pairs"])
    hit = bad[c.tri].any(axis=1)
    assert set(np.nonzero(hit)[0]) >= set(c.note["hyps"])                     # the planted ones, and whatever the draw hit
    assert (y["counts"][hit] == 0).all() and not y["mask"][bad].any() and not hit[y["winner"]]
    clean = fx.ransac_yardstick(name.replace("nonfinite", "edge-257"))
    assert (clean["counts"][~hit] - y["counts"][~hit]).max() <= 2 and (y["counts"][~hit] <= clean["counts"][~hit]).all()


@pytest.mark.parametrize("method", fx.METHODS)
def test_degenerate_triples_sit_among_ordinary_ones(method):
    c = fx.ransac_case(f"degenerate-{method}")
    rep, col, same = c.note["hyps"]
    assert len(set(c.tri[rep])) == 2 and len(set(c.tri[same])) == 1 and len(set(c.tri[col])) == 3
    for h, rank in ((rep, 1), (col, 1), (same, 0)):
        pc = c.p[c.tri[h]] - c.p[c.tri[h]].mean(axis=0)
        S = np.linalg.svd(pc.T @ (c.q[c.tri[h]] - c.q[c.tri[h]].mean(axis=0)), compute_uv=False)
        assert (S > 1e-13 * max(S[0], 1e-300)).sum() == rank, (h, S)
    one = np.concatenate([c.p[c.tri[same][0]], c.q[c.tri[same][0]]])
    assert ((one + one + one) / 3.0 == one).all()                             # (i, i, i) centres to exactly 0: Umeyama's s is 0 / 0
    ordinary = np.setdiff1d(np.arange(len(c.tri)), c.note["hyps"])
    t = ref.ransac_table(c.p, c.q, c.tri[ordinary], c.thr, method)
    assert t["margin"] >= fx.MIN_MARGIN and t["cond"] >= fx.MIN_COND
    assert t["counts"].max() >= 3 and not np.isin(c.tri[ordinary], (250, 251, 252)).any()
    for h in (rep, col, same):
        k, margin = fx.line_inliers(c, h)
        print(f"{method} hypothesis {h} {c.tri[h]}: the line map holds {k} of its pairs, margin {margin:.3g}")
        assert margin >= fx.MIN_MARGIN
    assert fx.line_inliers(c, col)[0] == 3 and fx.line_inliers(c, rep)[0] == 2   # an image of a line; two inlier pairs


@pytest.mark.parametrize("method", fx.METHODS)
def test_the_collinear_winner_has_a_rank_one_inlier_set(method):
    c, y = fx.ransac_case(f"collinear-winner-{method}"), fx.ransac_yardstick(f"collinear-winner-{method}")
    assert y["winner"] == 7 and y["count"] == 40 and y["mask"][:40].all() and (y["counts"] == 40).sum() == 1
    S = _final_covariance(c, y)[1]
    assert S[1] / S[0] < 1e-13


# ---- Adam ----

def test_the_two_statements_of_the_loss_agree_at_the_start():
    c = fx.adam_case("one-step")
    a = ref.adam_9dof(c.p, c.q, **c.kw)
    b = ref.adam_9dof(c.p, c.q, centred=True, **c.kw)
    assert abs(a["loss"] - b["loss"]) <= 1e-14 * abs(a["loss"]) and np.abs(a["grad0"] - b["grad0"]).max() <= 1e-14
    # one step is a sign check of the gradients: 13 of the 14 are far from 0; the component of qo's along qo = (1, 0, 0, 0)
    # is identically 0 (R(qo) does not depend on |qo|), in the yardstick exactly
    assert np.abs(np.delete(a["grad0"], 7)).min() > 1e-6 and a["grad0"][7] == 0.0
    start = np.concatenate([np.float64(np.float32([0.01] * 3 + [0.9, 0.01, 0.01, 0.01] + [1, 0, 0, 0]))])
    y0 = ref.adam_9dof(c.p, c.q, **{**c.kw, "iterations": 0})
    lr = 1e-3
    assert np.allclose(a["translation"], start[:3] - lr * np.sign(a["grad0"][:3]), rtol=0, atol=1e-9)
    assert np.array_equal(y0["translation"], start[:3]) and y0["loss"] == 0.0 and np.array_equal(y0["scale"], fx.DISTINCT)


@pytest.mark.parametrize("name", fx.ADAM_REG_CASES)
def test_regulariser_cases_can_see_one_per_cent(name):
    """A case is kept only if a 1 % error in each regulariser term it uses moves M or the scales by 100x its bound."""
    c = fx.adam_case(name)
    y, bound = fx.adam_yardstick(name)
    ls, lrot = c.kw["lambda_reg_scale"], c.kw["lambda_reg_rot"]
    used = [i for i, lam in enumerate((ls, ls, lrot)) if lam > 0]
    for i in range(3):
        f = [1.0, 1.0, 1.0]
        f[i] = 1.01
        z = ref.adam_9dof(c.p, c.q, reg_factors=tuple(f), **c.kw)
        moved = {k: float(np.abs(z[k] - y[k]).max()) for k in ("M", "scale")}
        need = {k: 100 * max(bound[k][:2]) for k in moved}
        print(f"{name}: term {('logit', 'spread', 'rotation')[i]} x 1.01 moves M {moved['M']:.3g} (100x bound {need['M']:.3g}), "
              f"scale {moved['scale']:.3g} ({need['scale']:.3g})")
        if i in used:
            assert moved["M"] >= need["M"] or moved["scale"] >= need["scale"]
        else:
            assert moved["M"] == 0.0 and moved["scale"] == 0.0
    if not used:                                                              # (0, 0): the data term alone, the base of the others
        other = fx.adam_yardstick(name.replace("reg-0.0-0.0", "reg-0.3-0.3"))[0]
        assert np.abs(other["M"] - y["M"]).max() > 1e-4


def test_adam_cases_cover_what_the_names_say():
    for name in fx.ADAM_CASES:
        c = fx.adam_case(name)
        assert c.kw["iterations"] <= 200
        assert np.array_equal(c.p, c.p.astype(np.float32)) and np.array_equal(c.q, c.q.astype(np.float32))
        s0 = ref.start_scale(c.kw["init_scale"], c.kw.get("scale_min", 0.75), c.kw.get("scale_max", 1.5))
        assert (len(set(s0)) == 3) == c.holds_ro, name
    assert np.array_equal(ref.start_scale(fx.adam_case("outside").kw["init_scale"], 0.75, 1.5), fx.adam_case("midpoint").kw["init_scale"])
    assert fx.adam_case("far-100").extent > 100 and fx.adam_case("far-10000").extent > 1e4
