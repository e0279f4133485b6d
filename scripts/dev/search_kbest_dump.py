"""Every output of the grid-search kernels on the test fixtures, dumped by one library and compared with another's in dtype,
shape and bytes (profiles/search_kbest_bitequal.json).

    SCORP_GS_LIB=<library A> python scripts/dev/search_kbest_dump.py dump a.npz      (a fresh process per library)
    SCORP_GS_LIB=<library B> python scripts/dev/search_kbest_dump.py dump b.npz
    python scripts/dev/search_kbest_dump.py compare a.npz b.npz out.json

Cases: everything scripts/dev/icp_unify_dump.py dumps (the three ICP estimators, estimate_normals with its neighbours, the
mesh-distance query and nearest_point_distance); knn_mean_distance with its neighbours at k = 1, 20, 32 (k > n on the
small clouds), radius_neighbor_count and cluster_dbscan with its core flags on every fixture of tests/cloud_fixtures.py, each
at its test's radius; compute_fpfh_feature(return_neighbors=True) on every case of tests/fpfh_fixtures.py."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

KNNS = (1, 20, 32)


def cloud_cases():
    """{name: (key of tests/cloud_fixtures.py, radius, min_points)}"""
    from tests import cloud_fixtures as fx
    out = {}
    for offset in (100.0, 4096.0):
        out[f"blobs_{offset:g}"] = (("blobs", offset), fx.EPS, fx.MIN_POINTS)
        out[f"exact_{offset:g}"] = (("exact", offset), fx.EXACT_RADIUS, 2)
    out["traps"] = (("traps",), fx.EPS, fx.MIN_POINTS)
    for n in fx.SIZES:
        out[f"sized_{n}"] = (("sized", n), fx.sized(n)[1], fx.SIZED_MIN_POINTS)
    out["lattice"] = (("lattice",), float(np.sqrt(2.0)), 19)
    for name in fx.DEGENERATE:
        out[f"degenerate_{name}"] = (("degenerate", name), fx.DEGENERATE_RADIUS[name], fx.SIZED_MIN_POINTS)
    out["uniform"] = (("degenerate", "uniform"), 0.05, fx.SIZED_MIN_POINTS)
    out["chain"] = (("chain",),) + fx.chain()[1:]
    out["bridge"] = (("bridge",),) + fx.bridge()[1:]
    for order in ("ab", "ba"):
        out[f"tie_{order}"] = (("tie", order),) + fx.tie(order)[1:]
    for seed in (1, 2):
        out[f"shuffled_blobs_{seed}"] = (("shuffled", ("blobs", 100.0), seed), fx.EPS, fx.MIN_POINTS)
    return out


def dump(path):
    import icp_unify_dump
    icp_unify_dump.dump(path)
    out = dict(np.load(path))

    from scorp_amd import cloud
    from scorp_amd import global_registration as gr
    from tests import cloud_fixtures as fx
    from tests import fpfh_fixtures as ffx
    for name, (key, radius, min_points) in cloud_cases().items():
        P = np.array(fx.cloud(key))
        for k in KNNS:
            mean, nb = cloud.knn_mean_distance(P, k, return_neighbors=True)
            out[f"knn/{name}_k{k}/mean"], out[f"knn/{name}_k{k}/neighbors"] = mean.cpu().numpy(), nb.cpu().numpy()
        out[f"count/{name}/count"] = cloud.radius_neighbor_count(P, radius).cpu().numpy()
        labels, core = cloud.cluster_dbscan(P, radius, min_points, return_core=True)
        out[f"dbscan/{name}/labels"], out[f"dbscan/{name}/core"] = labels.cpu().numpy(), core.cpu().numpy()
    for name, (P, N, radius, max_nn) in ffx.cases().items():
        res = gr.compute_fpfh_feature(np.array(P), np.array(N), radius, max_nn, return_neighbors=True)
        for f, t in zip(("feature", "neighbors", "degree", "spfh_count"), res):
            out[f"fpfh/{name}/{f}"] = t.cpu().numpy()
    np.savez(path, **out)
    print(f"{len(out)} tensors, {sum(a.nbytes for a in out.values())} bytes -> {path}")


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    cases = {}
    for k in sorted((set(a.files) | set(b.files)) - {"library_source_sha"}):
        c = cases.setdefault(k.split("/", 1)[0], {"cases": set(), "tensors": 0, "bytes": 0, "different": []})
        c["cases"].add(k.rsplit("/", 1)[0])
        c["tensors"] += 1
        same = k in a.files and k in b.files and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        c["bytes"] += a[k].nbytes if k in a.files else 0
        if not same:
            c["different"].append(k)
    res = {"what": "the three ICP estimators, estimate_normals, the mesh-distance query, nearest_point_distance, knn_mean_distance "
                   f"(k = {', '.join(map(str, KNNS))}), radius_neighbor_count, cluster_dbscan and compute_fpfh_feature on the test fixtures, "
                   "parent commit's library against this tree's, one fresh process each; every output compared in dtype, shape and "
                   "bytes; counted per family of calls, the tensors that differ named",
           "library_source_sha": [str(a["library_source_sha"]), str(b["library_source_sha"])],
           "cases": sum(len(c["cases"]) for c in cases.values()), "tensors": sum(c["tensors"] for c in cases.values()),
           "tensors_different": sum(len(c["different"]) for c in cases.values()),
           "per_family": [dict(family=k, cases=len(c["cases"]), tensors=c["tensors"], bytes=c["bytes"], different=c["different"])
                          for k, c in cases.items()]}
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
