"""Every output of the public functions of scorp_amd.mesh that run csrc/mesh_cluster.hip, mesh_simplify.hip,
mesh_decimate.hip, mesh_distance.hip, mesh_render.hip and mesh_smooth.hip, on the fixtures of their GPU tests, dumped by one
library and compared with another's (profiles/mesh_common_bitequal.json).

    SCORP_GS_LIB=<library A> python scripts/dev/mesh_common_dump.py dump a.npz      (a fresh process per library)
    SCORP_GS_LIB=<library B> python scripts/dev/mesh_common_dump.py dump b.npz
    python scripts/dev/mesh_common_dump.py compare a.npz b.npz out.json [a2.npz]

Everything is compared in dtype, shape and bytes but the two families include/scorp_gs.h gives to float64 atomic sums in
arrival order: cluster_area (tensors named .../area) and the positions and colours of cluster_vertices (.../positions,
.../colors under simplify/).  Those are held to the bound the GPU test of the function uses - F 2^-52 (total area) per
cluster, one float32 ulp per component - and, with a second dump a2.npz of library A, A is compared with itself first."""
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def dump(path):
    import torch
    from scorp_amd import _C, mesh as M
    from tests import mesh_cluster_reference as cref
    from tests import mesh_distance_fixtures as dfx
    from tests import mesh_render_checks as rchecks
    from tests import mesh_render_fixtures as rfx
    from tests import mesh_simplify_reference as sref
    from tests import mesh_smooth_fixtures as sfx
    from tests.mesh_distance_checks import mesh_of
    from tests.test_mesh_cluster_gpu import _mesh as cluster_mesh
    from tests.test_mesh_decimate_gpu import CASES, _case
    from tests.test_mesh_render_gpu import _colors_of
    from tests.test_mesh_simplify_gpu import NAMES, _mesh as simplify_mesh
    dev = torch.device("cuda:0")
    cuda = lambda a: torch.from_numpy(np.array(a)).to(dev)
    out = {"library_source_sha": np.array(_C.lib().scorp_source_sha().decode())}

    def put(case, **tensors):
        for k, t in tensors.items():
            if t is not None:
                out[f"{case}/{k}"] = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    for name in cref.MESHES + ("spheres",):
        f, v, _ = cluster_mesh(name)
        tc, n, area = M.cluster_connected_triangles(cuda(f), cuda(v) if v is not None else None)
        put(f"cluster/{name}", triangle_clusters=tc, cluster_n_triangles=n, area=area, num_faces=len(f))
    f, v, _ = cluster_mesh("spheres")
    for keep in (1, 2, 1000):
        m = M.post_process_mesh(M.Mesh(cuda(v), cuda(f), torch.zeros(len(v), 3, device=dev)), keep)
        put(f"post_process/spheres_{keep}", vertices=m.vertices, faces=m.faces)

    for name in NAMES:
        v, c, f, h = simplify_mesh(name)
        for contraction in sref.CONTRACTIONS:
            cell, m = M.cluster_vertices(M.Mesh(cuda(v), cuda(f), cuda(c)), h, contraction)
            put(f"simplify/{name}_{contraction}", vertex_cell=cell, faces=m.faces, positions=m.vertices, colors=m.colors)

    for case in CASES:
        v, c, f, target, max_err, bw = _case(case)
        rounds = []
        m = M.simplify_quadric_decimation(M.Mesh(cuda(v), cuda(f), cuda(c)), target, max_err, bw, rounds=rounds)
        put(f"decimate/{case}", vertices=m.vertices, faces=m.faces, colors=m.colors, rounds=np.array(rounds, np.int64).reshape(-1, 4))

    def distance_case(case, verts, faces, q, r):
        mesh = mesh_of(verts, faces, "cuda")
        d2, face, closest = M.point_mesh_distance(cuda(q), mesh, r)[:3]
        put(f"distance/{case}", squared_distance=d2, face=face, closest=closest)

    for name in dfx.FIXTURES:
        verts, faces, q, r = dfx.fixture(name)
        distance_case(name, verts, faces, q, r)
        for n in (1, 255, 256, 257, 1025):
            try:
                s = M.sample_points_uniformly(mesh_of(verts, faces, "cuda"), n, seed=5)
            except ValueError:   # (a mesh of no area has nothing to sample)
                break
            put(f"sample/{name}_{n}", **{k: getattr(s, k) for k in s.__dataclass_fields__})
    verts, faces, q, r = dfx.fixture("flat")
    for count in dfx.BLOCK_EDGE_COUNTS:
        distance_case(f"flat_first{count}", verts, faces, q[:count], r)

    for name in rfx.CHECKED_IN_PYTHON:
        colors = _colors_of(name)
        for cull in (False, True):
            r = rchecks.render(name, "cuda", cull=cull, colors=colors, barycentric=True)
            put(f"render/{name}_cull{int(cull)}", **dict(zip(rchecks.MeshRenderFields, r)), visible_views=rchecks.visibility(name, "cuda", cull=cull))
    for count in rfx.COUNT_EDGES:
        r = rchecks.render("counts", "cuda", num_faces=count, barycentric=True)
        put(f"render/counts_first{count}", **dict(zip(rchecks.MeshRenderFields, r)), visible_views=rchecks.visibility("counts", "cuda", num_faces=count))

    for name in sfx.FIXTURES:
        mesh = sfx.mesh_of(name, dev)
        adj = M.mesh_adjacency(mesh)
        put(f"smooth/{name}/adjacency", neighbor_offsets=adj.neighbor_offsets, neighbors=adj.neighbors, corner_offsets=adj.corner_offsets,
            corner_faces=adj.corner_faces, boundary=adj.boundary)
        put(f"smooth/{name}/normals", face=M.face_normals(mesh), face_raw=M.face_normals(mesh, normalized=False),
            **{w: M.vertex_normals(mesh, w, adj) for w in sfx.WEIGHTINGS})
        for w in sfx.WEIGHTS:
            for fixed in (False, True):
                put(f"smooth/{name}/{w}_fixed{int(fixed)}",
                    **{f"laplacian{n}": M.filter_smooth_laplacian(mesh, n, weights=w, fix_boundary=fixed, adjacency=adj).vertices for n in sfx.LAPLACIAN_ITERATIONS},
                    **{f"taubin{n}": M.filter_smooth_taubin(mesh, n, weights=w, fix_boundary=fixed, adjacency=adj).vertices for n in sfx.TAUBIN_ITERATIONS})
    for name in ("sphere", "cube", "large_mix"):
        f = rfx.fixture(name)
        mesh = rchecks.mesh_of(f, "cuda")
        render = M.render_mesh(mesh, cuda(f["full_proj"]), f["H"], f["W"], near=f["near"], colors=False, barycentric=True)
        put(f"normal_map/{name}", flat=M.normal_map(render, mesh), smooth=M.normal_map(render, mesh, M.vertex_normals(mesh)))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} tensors, {sum(a.nbytes for a in out.values())} bytes -> {path}")


def _ulp(a, b):
    """the worst |a - b| in units of 2^-23 max(|a|, |b|), as tests/mesh_simplify_reference.py's ulp_error"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    scale = 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(scale > 0, np.abs(a - b) / np.where(scale > 0, scale, 1.0), 0.0), initial=0.0))


def _judge(k, a, b):
    """(same, note): bytes for everything but the two families of float64 atomic sums"""
    if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
        return False, "missing, or another dtype or shape"
    if a[k].tobytes() == b[k].tobytes():
        return True, None
    case, field = k.rsplit("/", 1)
    if case.startswith("cluster/") and field == "area":
        err, bound = float(np.abs(a[k] - b[k]).max()), int(a[f"{case}/num_faces"]) * 2.0 ** -52 * float(a[k].sum())
        return err <= bound, f"worst difference {err:.3e}, bound {bound:.3e}"
    if case.startswith("simplify/") and field in ("positions", "colors"):
        err = _ulp(a[k], b[k])
        return err <= 1.0, f"worst difference {err:.3f} float32 ulp, bound 1"
    return False, "bytes differ"


def _compare(a, b):
    """per family (the first part of a tensor's name: cluster, simplify, ...) the counts, and every case that is not equal in bytes"""
    families, cases, not_equal = {}, set(), []
    for k in sorted((set(a.files) | set(b.files)) - {"library_source_sha"}):
        case = k.rsplit("/", 1)[0]
        fam = families.setdefault(k.split("/", 1)[0], {"cases": set(), "tensors": 0, "bytes": 0, "different": 0, "within_bound_not_equal": 0})
        fam["cases"].add(case)
        cases.add(case)
        fam["tensors"] += 1
        fam["bytes"] += a[k].nbytes if k in a.files else 0
        same, note = _judge(k, a, b)
        if note:
            fam["within_bound_not_equal" if same else "different"] += 1
            not_equal.append(f"{k}: {note}")
    for fam in families.values():
        fam["cases"] = len(fam["cases"])
    return {"library_source_sha": [str(a["library_source_sha"]), str(b["library_source_sha"])], "cases": len(cases),
            "tensors": sum(f["tensors"] for f in families.values()), "tensors_different": sum(f["different"] for f in families.values()),
            "tensors_within_bound_not_equal": sum(f["within_bound_not_equal"] for f in families.values()),
            "per_family": families, "not_equal_in_bytes": not_equal}


def compare(a_path, b_path, out_path, a2_path=None):
    a, b = np.load(a_path), np.load(b_path)
    res = {"what": "every public function of scorp_amd.mesh over the six mesh_*.hip files on the fixtures of their GPU tests, the parent "
                   "commit's library against this tree's, one fresh process each; every output compared in dtype, shape and bytes, but "
                   "cluster_area and the positions and colours of cluster_vertices (float64 atomic sums in arrival order), held to their "
                   "GPU tests' bounds",
           "parent_against_this": _compare(a, b)}
    if a2_path:
        res["parent_against_parent"] = _compare(a, np.load(a2_path))
    text = re.sub(r"([\[{])\s+([^\[\]{}]*?)\s+([\]}])", lambda m: m.group(1) + " ".join(m.group(2).split()) + m.group(3), json.dumps(res, indent=1))
    with open(out_path, "w") as f:   # (a family's counts on one line)
        f.write(text + "\n")
    r = res["parent_against_this"]
    print(f"{r['cases']} cases, {r['tensors']} tensors, {r['tensors_different']} different, {r['tensors_within_bound_not_equal']} within their bound")
    return 1 if r["tensors_different"] else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) in (5, 6) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
