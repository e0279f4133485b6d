"""The marching-cubes case table of csrc/marching_cubes.hip and csrc/marching_cubes_blocks.hip, generated from a written
rule - not copied from any library, and never compared with skimage's (Lewiner) or Open3D's table.

    python -m scorp_amd.mc_table          # rewrites scorp_amd/csrc/mc_table.hpp

Numbering (include/scorp_gs.h): corner n = 4 di + 2 dj + dk; edges 0 .. 11 = the x-edges, the y-edges, the z-edges, each by
ascending first corner; bit n of a case is set when corner n is inside (f < level).

Rule.  Each of the six cube faces has 0, 2 or 4 crossed edges.  Two crossings are joined.  With four (two inside corners on
a face diagonal) the two edges at each INSIDE corner are joined: the inside corners are cut off separately.  The choice
depends on the face's four signs alone, so the two cells that share a face agree and the surface is closed.  Every crossed
edge then has exactly two partners; the loops are the cycles of that graph, opened at the lowest unused edge id, oriented so
that the Newell normal over the edge midpoints agrees with the sum over the loop's edges of (outside end - inside end), and
rotated to start at their lowest edge id.

Triangulation of a loop p[0 .. k - 1]: the first triangulation, in the order below, none of whose diagonals joins two
crossings that lie on one cube face (such a diagonal lies IN that face, and the neighbouring cell may produce it too: an edge
with four triangles).  Order: tri(p) takes the triangle (p[0], p[m], p[-1]) on the closing edge with the apex m DESCENDING
from k - 2 to 1, and for each apex every tri(p[0 .. m]) (outer loop) with every tri(p[m .. k - 1]) (inner loop); the
triangles are listed left part, apex triangle, right part.  The first candidate is therefore the fan (p0, p1, p2), (p0, p2,
p3), ... from the lowest edge; 18 cases need a later one.  Every triangle keeps the loop's orientation.

A row is 16 bytes: five triangles x three edge ids, 0xFF padding, and the triangle count in the last byte."""
import os

import numpy as np

CORNER = np.array([[n >> 2, (n >> 1) & 1, n & 1] for n in range(8)], np.int64)
# edge e: (first corner n0, axis); the second corner is n0 + (4 >> axis)
EDGES = [(n0, axis) for axis in range(3) for n0 in range(8) if not n0 & (4 >> axis)]
EDGE_N0 = np.array([e[0] for e in EDGES], np.int64)
EDGE_AXIS = np.array([e[1] for e in EDGES], np.int64)
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.hpp")


def _edge_faces(e):
    """The two cube faces (axis, side) that edge e lies in."""
    n0, axis = EDGES[e]
    return {(a, int(CORNER[n0][a])) for a in range(3) if a != axis}


def _edge_id(n, m):
    lo, hi = min(n, m), max(n, m)
    return EDGES.index((lo, {4: 0, 2: 1, 1: 2}[hi - lo]))


def crossed_edges(case):
    return [e for e, (n0, axis) in enumerate(EDGES) if ((case >> n0) & 1) != ((case >> (n0 + (4 >> axis))) & 1)]


def loops(case):
    """The oriented loops of a case, each a list of edge ids starting at its lowest."""
    inside = [(case >> n) & 1 for n in range(8)]
    partner = {e: [] for e in crossed_edges(case)}
    for axis in range(3):
        for side in (0, 1):
            on = [n for n in range(8) if CORNER[n][axis] == side]
            edges = [e for e in partner if (axis, side) in _edge_faces(e)]
            if len(edges) == 2:
                pairs = [tuple(edges)]
            elif len(edges) == 4:   # the two edges of the face at each inside corner
                pairs = [tuple(_edge_id(n, m) for m in on if bin(n ^ m).count("1") == 1) for n in on if inside[n]]
            else:
                assert not edges
                pairs = []
            for a, b in pairs:
                partner[a].append(b)
                partner[b].append(a)
    assert all(len(p) == 2 for p in partner.values()), case
    out, used = [], set()
    for first in sorted(partner):
        if first in used:
            continue
        loop, prev, cur = [first], None, first
        used.add(first)
        while True:
            nxt = [p for p in partner[cur] if p != prev]
            nxt = nxt[0] if nxt else partner[cur][0]   # (a two-edge cycle cannot occur; kept total)
            if nxt == first:
                break
            loop.append(nxt)
            used.add(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3, case
        mid = np.array([CORNER[EDGES[e][0]] + 0.5 * np.eye(3)[EDGES[e][1]] for e in loop])
        newell = sum(np.cross(mid[i], mid[(i + 1) % len(loop)]) for i in range(len(loop)))
        outward = np.zeros(3)
        for e in loop:
            n0, axis = EDGES[e]
            outward[axis] += 1.0 if inside[n0] else -1.0   # outside end - inside end
        d = float(newell @ outward)
        assert d != 0.0, case
        if d < 0:
            loop = [loop[0]] + loop[:0:-1]
        out.append(loop)
    return out


def _triangulations(p):
    """Every triangulation of the polygon p (a tuple of edge ids) as a list of triangles, in the order of the module text."""
    if len(p) < 3:
        yield []
        return
    for m in range(len(p) - 2, 0, -1):
        for left in _triangulations(p[:m + 1]):
            for right in _triangulations(p[m:]):
                yield left + [(p[0], p[m], p[-1])] + right


def _admissible(loop, tris):
    k = len(loop)
    at = {e: i for i, e in enumerate(loop)}
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            if (at[a] - at[b]) % k in (1, k - 1):
                continue   # an edge of the loop itself
            if _edge_faces(a) & _edge_faces(b):
                return False
    return True


def triangles(case):
    """The triangles of a case as (e0, e1, e2) edge-id triples, loop by loop."""
    out = []
    for loop in loops(case):
        tris = next((t for t in _triangulations(tuple(loop)) if _admissible(loop, t)), None)
        assert tris is not None, case
        out += tris
    return out


def table():
    """[256, 16] uint8: the rows as the kernels read them."""
    t = np.full((256, 16), 0xFF, np.uint8)
    for case in range(256):
        tris = triangles(case)
        assert len(tris) <= 5, case
        t[case, :3 * len(tris)] = np.array(tris, np.uint8).reshape(-1)
        t[case, 15] = len(tris)
    return t


_cache = None


def cached_table():
    global _cache
    if _cache is None:
        _cache = table()
    return _cache


def header_text():
    rows = ",\n".join("    " + ", ".join(f"0x{b:02X}" for b in row) for row in table())
    return ("// mc_table.hpp - GENERATED by `python -m scorp_amd.mc_table`; do not edit.  The marching-cubes case table: row = case (bit n\n"
            "// set when corner n = 4 di + 2 dj + dk is inside), 16 bytes = five triangles x three edge ids (0xFF padding) and the\n"
            "// triangle count.  The rule it follows is written down in scorp_amd/mc_table.py and include/scorp_gs.h.\n"
            "#pragma once\n\n"
            "namespace scorp {\n\n"
            "static __device__ __attribute__((aligned(16))) const unsigned char kMcTable[256 * 16] = {\n"
            f"{rows}}};\n\n"
            "}  // namespace scorp\n")


if __name__ == "__main__":
    with open(HEADER, "w") as f:
        f.write(header_text())
    print(HEADER)
