"""The scorp_amd.mesh package without a GPU: every name the tree imports from it is the object of its home module, _C.call
marshals its arguments as the C ABI takes them, the one helper that drops unreferenced vertices does so on the smallest mesh
that has some, and the argument checks cluster_vertices and simplify_quadric_decimation share raise what each raised when it
carried its own copy."""
import ctypes
import importlib

import pytest
import torch

HOMES = {
    "_common": ["Mesh", "METHODS", "MAX_CLUSTER_FACES", "MAX_SIMPLIFY_VERTICES"],
    "tsdf": ["MAX_RANGE", "LAUNCH_SAMPLES", "uncontract", "tsdf_fuse"],
    "surface": ["extract_surface", "_surface_nets_numpy", "_scan_counts"],
    "blocks": ["BLOCK_SIDE", "BLOCK_VOXELS", "KEY_BIAS", "MAX_TABLE_SLOTS", "BlockVolume", "tsdf_blocks_fuse", "block_coords",
               "block_neighbors", "extract_surface_blocks"],
    "cluster": ["MIN_CLUSTER_TRIANGLES", "cluster_connected_triangles", "post_process_mesh", "_cluster_numpy"],
    "simplify": ["CONTRACTIONS", "CELL_SIDE", "QUADRIC_TRUNCATE", "cluster_vertices", "simplify_vertex_clustering"],
    "decimate": ["DECIMATE_DET_FLOOR", "DECIMATE_REACH", "simplify_quadric_decimation", "_decimate", "_DecimateHip"],
    "extractor": ["focus_point", "GaussianExtractor"],
}


@pytest.mark.parametrize("home", sorted(HOMES))
def test_the_package_re_exports_its_modules_names(home):
    package = importlib.import_module("scorp_amd.mesh")
    module = importlib.import_module(f"scorp_amd.mesh.{home}")
    for name in HOMES[home]:
        assert getattr(package, name) is getattr(module, name), name
        if callable(getattr(module, name)):
            assert getattr(module, name).__module__ == module.__name__, name   # (its home, not a copy there)


class _FakeLib:
    def __init__(self, code):
        self.code, self.got = code, None

    def scorp_fake(self, *args):
        self.got = args
        return self.code

    def scorp_last_error(self):
        return b"why"


def test_call_marshals_tensors_structs_and_the_stream(monkeypatch):
    from scorp_amd import _C
    fake = _FakeLib(0)
    monkeypatch.setattr(_C, "lib", lambda: fake)
    monkeypatch.setattr(_C, "current_stream_ptr", lambda: 0x5EED)
    t, params = torch.arange(4.0), _C.ScorpTsdfParams()
    assert _C.call("scorp_fake", t, None, 7, 0.25, params) is None
    ptr, none, i, f, ref, stream = fake.got
    assert ptr == t.data_ptr() and none is None
    assert type(i) is int and i == 7 and type(f) is float and f == 0.25
    assert type(ref) is type(ctypes.byref(params)) and ref._obj is params
    assert stream == 0x5EED


def test_call_raises_under_the_functions_name(monkeypatch):
    from scorp_amd import _C
    fake = _FakeLib(-1)
    monkeypatch.setattr(_C, "lib", lambda: fake)
    monkeypatch.setattr(_C, "current_stream_ptr", lambda: 0)
    with pytest.raises(RuntimeError, match=r"scorp_fake failed \(-1\): why"):
        _C.call("scorp_fake", 1)
    assert fake.got == (1, 0)


def test_drop_unreferenced_keeps_order_and_re_indexes():
    from scorp_amd.mesh import drop_unreferenced
    verts = torch.arange(18.0).reshape(6, 3)
    colors = 0.01 * torch.arange(18.0, dtype=torch.float64).reshape(6, 3)
    faces = torch.tensor([[5, 1, 3], [3, 1, 0]], dtype=torch.int64)
    v, f, c = drop_unreferenced(verts, faces, colors)
    kept = [0, 1, 3, 5]
    assert torch.equal(v, verts[kept]) and v.dtype == torch.float32
    assert torch.equal(c, colors[kept]) and c.dtype == torch.float64
    assert f.dtype == torch.int32 and f.is_contiguous() and f.tolist() == [[3, 1, 2], [2, 1, 0]]
    f_t = drop_unreferenced(verts, faces.to(torch.int32).T.contiguous().T, colors)[1]   # (a strided int32 input)
    assert f_t.dtype == torch.int32 and f_t.is_contiguous() and torch.equal(f_t, f)


def test_drop_unreferenced_of_no_faces_is_empty():
    from scorp_amd.mesh import drop_unreferenced
    v, f, c = drop_unreferenced(torch.zeros(6, 3), torch.empty(0, 3, dtype=torch.int32), torch.zeros(6, 3))
    assert tuple(v.shape) == (0, 3) and v.dtype == torch.float32
    assert tuple(f.shape) == (0, 3) and f.dtype == torch.int32 and f.is_contiguous()
    assert tuple(c.shape) == (0, 3) and c.dtype == torch.float32


def _edited(t, at, value):
    t = t.clone()
    t[at] = value
    return t


SHAPES = "vertices must be [Nv, 3] and faces an integer tensor [F, 3]"
BAD = {   # what to replace in a tetrahedron, and the message of the parent commit, where each function had its own checks
    "vertices [4, 2]": ("vertices", lambda v: torch.zeros(4, 2), SHAPES),
    "float faces": ("faces", lambda f: f.float(), SHAPES),
    "3 colours": ("colors", lambda c: c[:3], "3 colours for 4 vertices"),
    "NaN vertex": ("vertices", lambda v: _edited(v, (2, 1), float("nan")), "the vertices are not all finite"),
    "index -1": ("faces", lambda f: _edited(f, (1, 2), -1), "vertex index -1 with 4 vertices"),
    "index Nv": ("faces", lambda f: _edited(f, (3, 0), 4), "vertex index 4 with 4 vertices"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_both_simplifiers_refuse_a_bad_mesh_alike(what):
    from scorp_amd.mesh import Mesh, cluster_vertices, simplify_quadric_decimation
    parts = dict(vertices=torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
                 faces=torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32), colors=torch.zeros(4, 3))
    field, spoil, message = BAD[what]
    parts[field] = spoil(parts[field])
    for run in (lambda m: cluster_vertices(m, 0.5), lambda m: simplify_quadric_decimation(m, 2)):
        with pytest.raises(ValueError) as err:
            run(Mesh(**parts))
        assert str(err.value) == message
