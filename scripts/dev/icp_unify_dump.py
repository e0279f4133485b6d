"""Every output of the ICP, normal-estimation, mesh-distance and nearest-point calls on the test fixtures, dumped by one
library and compared with another's in dtype, shape and bytes (profiles/icp_unify_bitequal.json).

    SCORP_GS_LIB=<library A> python scripts/dev/icp_unify_dump.py dump a.npz      (a fresh process per library)
    SCORP_GS_LIB=<library B> python scripts/dev/icp_unify_dump.py dump b.npz
    python scripts/dev/icp_unify_dump.py compare a.npz b.npz out.json

Cases: every estimator on the aggregate fixtures at every AGGREGATE_NS (max_iteration 0 and 1), the two margin fixtures
at max_iteration 0, 1 and 5, the realistic fixture, the four rank-deficient systems, the no-pair and zero-normal cases and
a 3-init batch next to each init alone; estimate_normals with its neighbours on every NORMALS fixture; the mesh-distance
query and nearest_point_distance on every mesh fixture and on the block-edge query counts."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

FIELDS = ("transformation", "fitness", "inlier_rmse", "iterations")


def dump(path):
    import torch
    from scorp_amd import icp
    from scorp_amd.mesh import nearest_point_distance, point_mesh_distance
    from tests import icp_color_fixtures as cfx
    from tests import icp_plane_fixtures as pfx
    from tests import icp_probe_fixtures as fx
    from tests import icp_reference as ref
    from tests import mesh_distance_fixtures as mfx
    from tests.mesh_distance_checks import mesh_of
    from tests.test_icp_gpu import ROT64, _margin_fixture, _realistic
    from scorp_amd import _C
    out = {"library_source_sha": np.array(_C.lib().scorp_source_sha().decode())}

    def both(case, src, tgt, nrm, r, inits, **kw):
        for est in icp.ESTIMATIONS:
            # the coloured estimator's colours: a smooth texture of position, the source's taken where it lies
            colors = {"source_colors": cfx.smooth_texture(src), "target_colors": cfx.smooth_texture(tgt)} if est == "colored" else {}
            res = icp.registration_icp(np.array(src), np.array(tgt), r, inits, estimation=est,
                                       target_normals=None if nrm is None or est == "point_to_point" else np.array(nrm), **colors, **kw)
            for f in FIELDS:
                out[f"icp/{case}/{est}/{f}"] = getattr(res, f)

    for ns in fx.AGGREGATE_NS:
        src, tgt, r, inits, _ = fx.aggregate_fixture(ns)
        for it in (0, 1):
            both(f"aggregate_{ns}_it{it}", src, tgt, pfx.aggregate_normals(), r, inits, max_iteration=it, relative_fitness=0.0,
                 relative_rmse=0.0)
    src, tgt, r, inits, _ = _margin_fixture()
    psrc, ptgt, pnrm, pr, pinits, _ = pfx.margin_fixture()
    for it in (0, 1, 5):
        both(f"margin_it{it}", src, tgt, None, r, inits, max_iteration=it, relative_fitness=0.0, relative_rmse=0.0)
        both(f"plane_margin_it{it}", psrc, ptgt, pnrm, pr, pinits, max_iteration=it, relative_fitness=0.0, relative_rmse=0.0)
    both("plane_margin_batch", psrc, ptgt, pnrm, pr, pinits, max_iteration=30)
    for j in range(len(pinits)):
        both(f"plane_margin_alone{j}", psrc, ptgt, pnrm, pr, pinits[j], max_iteration=30)
    far = np.array(pinits[2])
    far[:3, 3] += (5.0, 0.0, 0.0)
    both("no_pairs", psrc, ptgt, pnrm, 1e-3, far, max_iteration=30)
    both("zero_normals", psrc, ptgt, np.zeros_like(pnrm), pr, pinits, max_iteration=7)
    for name in sorted(pfx.RANK_DEFICIENT):
        s, t, n, r, _ = pfx.rank_deficient(name)
        both(f"rank_{name}", s, t, n, r, np.eye(4), max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    src, tgt, _, _ = _realistic()
    rots = np.load(ROT64)["rotations"][:13]
    both("realistic", src, tgt, None, float(np.ptp(tgt, axis=0).mean() / 10 * 1.6), ref.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0)),
         max_iteration=400)

    for name in pfx.NORMALS:
        build, knn, _ = pfx.NORMALS[name]
        nrm, nb = icp.estimate_normals(build().astype(np.float32), knn=knn, return_neighbors=True)
        out[f"normals/{name}/normals"], out[f"normals/{name}/neighbors"] = nrm.cpu().numpy(), nb.cpu().numpy()

    def mesh_case(case, verts, faces, q, r):
        qt = torch.from_numpy(np.array(q)).cuda()
        for f, t in zip(("squared_distance", "face", "closest"), point_mesh_distance(qt, mesh_of(verts, faces, "cuda"), r)):
            out[f"mesh/{case}/{f}"] = t.cpu().numpy()
        near = nearest_point_distance(qt, torch.from_numpy(np.array(verts)).cuda(), r)
        out[f"nearest/{case}/squared_distance"], out[f"nearest/{case}/index"] = near.squared_distance.cpu().numpy(), near.index.cpu().numpy()

    for name in mfx.FIXTURES:
        mesh_case(name, *mfx.fixture(name))
    verts, faces, q, r = mfx.fixture("flat")
    for count in mfx.BLOCK_EDGE_COUNTS:
        mesh_case(f"flat_first{count}", verts, faces, q[:count], r)
    np.savez(path, **out)
    print(f"{len(out)} tensors, {sum(a.nbytes for a in out.values())} bytes -> {path}")


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    cases = {}
    # an estimator that only one of the two libraries has (a new one) is named and left out; everything else must match
    ests = [{k.split("/")[2] for k in f.files if k.startswith("icp/")} for f in (a, b)]
    lone = sorted(ests[0] ^ ests[1])
    for k in sorted((set(a.files) | set(b.files)) - {"library_source_sha"}):
        if k.startswith("icp/") and k.split("/")[2] in lone:
            continue
        c = cases.setdefault(k.rsplit("/", 1)[0], {"tensors": 0, "bytes": 0, "different": []})
        c["tensors"] += 1
        same = k in a.files and k in b.files and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        c["bytes"] += a[k].nbytes if k in a.files else 0
        if not same:
            c["different"].append(k.rsplit("/", 1)[1])
    res = {"what": "ICP (every estimator both libraries have), estimate_normals, mesh-distance query and nearest_point_distance on the test fixtures, parent "
                   "commit's library against this tree's, one fresh process each; every output compared in dtype, shape and bytes",
           "library_source_sha": [str(a["library_source_sha"]), str(b["library_source_sha"])], "estimators_compared": sorted(ests[0] & ests[1]),
           "estimators_in_one_library_only": lone, "cases": len(cases), "tensors": sum(c["tensors"] for c in cases.values()),
           "tensors_different": sum(len(c["different"]) for c in cases.values()),
           "per_case": [dict(case=k, **c) for k, c in cases.items()]}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{res['cases']} cases, {res['tensors']} tensors, {res['tensors_different']} different")
    return 1 if res["tensors_different"] else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
