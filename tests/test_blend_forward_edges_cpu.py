"""The fixtures and the bound of the 3DGS blend-forward edge suite, checked without a GPU.

tests/test_blend_forward_edges_gpu.py holds `blend_forward_wave_kernel` to the float64 blend of
tests/blend_forward_reference.py on the scenes of tests/blend_forward_fixtures.py.  Here the same reference runs on the
fp32 oracle's geometry and tile lists, and shows
  - that every scene is what it claims to be (lengths, stops, clamp, power > 0, holes, an empty list), with few
    ambiguous pixels even at ten times the ambiguity threshold;
  - that the bound is not too tight: the oracle's own fp32 image and the float32 run of the reference stay within 1 x the
    bound of float64 on every kept pixel (the GPU test allows 4 x);
  - that it is not too loose: each of twelve planted defects, applied to the reference and put through the very check
    functions the GPU test calls, is flagged on the fixture aimed at it.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import blend_forward_fixtures as F
from tests import blend_forward_reference as R

AMBIGUOUS_CAP = 0.05
_cache = {}


def reference(name):
    """(kw, want, oracle images, tile_start, point_list, geom, float64 blend, float32 blend), once per scene, read-only."""
    if name not in _cache:
        from oracle.gs_oracle import OracleRender
        kw, want = F.build(name)
        o = OracleRender(np.float32, **kw)
        g = o.geom()
        ts, pl = o.tiles()
        r64 = R.blend(g, ts, pl, kw["W"], kw["H"], kw["bg"])
        r32 = R.blend(g, ts, pl, kw["W"], kw["H"], kw["bg"], dtype=np.float32)
        _cache[name] = SimpleNamespace(kw=kw, want=want, o=dict(color=o.color.copy(), depth=o.depth[0].copy(), alpha=o.alpha[0].copy()),
                                       ts=ts, pl=pl.copy(), g=g, r64=r64, r32=r32)
        o.close()
    return _cache[name]



@pytest.mark.parametrize("name", list(F.FIXTURES))
def test_fixture_holds_its_conditions(name):
    c = reference(name)
    assert F.conditions(name, c.want, c.r64, c.ts) == []
    kw = c.kw
    share = c.r64.ambiguous.mean()
    share10 = R.blend(c.g, c.ts, c.pl, kw["W"], kw["H"], kw["bg"], delta=10 * R.DELTA, with_bound=False).ambiguous.mean()
    print(f"{name}: ambiguous pixels {100 * share:.2f} % at delta, {100 * share10:.2f} % at 10 x delta")
    assert share10 <= AMBIGUOUS_CAP, f"{name}: {100 * share10:.2f} % ambiguous pixels at 10 x delta"
    # the reference in the form the kernel leaves it passes its own checks
    assert R.check_all(R.as_kernel_outputs(c.r64), c.r64, c.ts) == []


@pytest.mark.parametrize("name", list(F.FIXTURES))
def test_bound_is_not_too_tight(name):
    """Two fp32 evaluations of the same blend - the oracle's C loop and the float32 run of the reference - lie within 1 x
    the bound of float64 on every kept pixel, and so within 2 x the bound of each other."""
    c = reference(name)
    r32 = dict(color=c.r32.color, depth=c.r32.depth, alpha=c.r32.alpha, final_T=c.r32.final_T)
    st = {}
    assert R.check_images(r32, c.r64, factor=1.0, stats=st) == []
    keep = ~c.r64.ambiguous
    e_ref = max(float(np.where(keep, np.abs(c.r32.color - c.r64.color), 0).max()), float(np.where(keep, np.abs(c.r32.alpha - c.r64.alpha), 0).max()))
    for key, bound in (("color", c.r64.b_color), ("depth", c.r64.b_depth)):
        d = np.abs(c.o[key].astype(np.float64) - getattr(c.r32, key))
        assert (np.where(keep, d - 2.0 * bound, 0.0) <= 0).all(), f"{name}: oracle {key} further than 2 x the bound from the float32 run"
    print(f"{name}: e_ref {e_ref:.2e}, bound (colour) up to {st['color'][1]:.2e}, float32 run at {max(v[2] for v in st.values()):.2f} x the bound, "
          f"oracle vs float32 run {np.abs(c.o['color'] - c.r32.color).max():.2e}")


# planted defect -> the fixtures aimed at it
AIMED = {
    "hit 80 dropped": ["len81-13x11", "len161-37x21"],
    "last hit of a chunk blended twice": ["len64-8x8", "len81-13x11"],
    "two adjacent hits swapped": ["len17-13x11", "stops_spread-13x11"],
    "the saturating hit blended": ["stop8-8x8", "stop17-13x11", "stop81-37x21", "stops_spread-37x21"],
    "0.99 clamp omitted": ["clamp0-all-13x11", "clamp64-some-13x11", "clamp80-all-13x11"],
    "1/255 select omitted": ["sparse-37x21", "empty-37x21"],
    "power > 0 guard omitted": ["indefinite0-13x11", "indefinite64-37x21"],
    "coefficients cut to two bf16 terms": ["sparse-37x21", "len161-37x21"],
    "n_contrib in the uncompacted list": ["sparse-37x21", "stops_spread-37x21"],
    "n_contrib off by one": ["len81-13x11", "sparse-37x21"],
    "a hit with no taker kept": ["sparse-37x21"],
    "a taken hit dropped from the list": ["len81-13x11", "sparse-37x21"],
}


def test_every_defect_is_aimed_at():
    assert set(AIMED) == set(R.DEFECTS)


@pytest.mark.parametrize("defect,name", [(d, n) for d, names in AIMED.items() for n in names])
def test_planted_defect_is_flagged(defect, name):
    c = reference(name)
    kw = c.kw
    where, args = R.DEFECTS[defect]
    if where == "blend":
        wrong = R.as_kernel_outputs(R.blend(c.g, c.ts, c.pl, kw["W"], kw["H"], kw["bg"], defect=args, with_bound=False))
    else:
        wrong = R.as_kernel_outputs(c.r64, defect=args)
    found = R.check_all(wrong, c.r64, c.ts)
    print(f"{defect} on {name}: {len(found)} findings; first: {found[0] if found else '-'}")
    assert found, f"'{defect}' passes every check on {name}"
