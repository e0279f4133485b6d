"""The surface-extraction kernels (csrc/isosurface.hip) against the numpy float64 yardstick: identical vertex count and
face indices, vertex positions within 1e-5 h (h the largest cell edge: t divides two numbers of opposite sign, about 3
roundings per crossing, a mean of at most 12 crossings stays under 40 fp32 epsilons)."""
import functools

import numpy as np
import pytest
import torch

from tests import isosurface_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(name):
    return ref.surface_nets(ref.field(name), ref.lattice())


@pytest.mark.parametrize("name", ("sphere", "torus", "plane"))
def test_kernels_match_the_reference(dev, name):
    from scorp_amd.mesh import extract_surface
    coords = ref.lattice()
    v, f = extract_surface(torch.from_numpy(ref.field(name)).to(dev), [torch.from_numpy(c).to(dev) for c in coords])
    rv, rf = reference(name)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.shape == rv.shape
    assert np.array_equal(f.cpu().numpy(), rf)
    err = float(np.abs(v.cpu().numpy().astype(np.float64) - rv).max())
    print(f"{name}: {len(rv)} vertices, {len(rf)} faces, max vertex error {err / ref.max_edge(coords):.3e} h")
    assert err <= 1e-5 * ref.max_edge(coords)


def test_nonzero_level(dev):
    from scorp_amd.mesh import extract_surface
    coords = ref.lattice()
    g = ref.field("sphere")
    v, f = extract_surface(torch.from_numpy(g).to(dev), [torch.from_numpy(c).to(dev) for c in coords], level=0.1)
    rv, rf = ref.surface_nets(g, coords, level=np.float32(0.1))
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.abs(v.cpu().numpy().astype(np.float64) - rv).max() <= 1e-5 * ref.max_edge(coords)


def test_no_crossing_gives_an_empty_mesh(dev):
    from scorp_amd.mesh import extract_surface
    v, f = extract_surface(torch.from_numpy(ref.field("none")).to(dev), [torch.from_numpy(c).to(dev) for c in ref.lattice()])
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    torch.cuda.synchronize()


def test_single_cell(dev):
    from scorp_amd.mesh import extract_surface
    g = torch.ones(2, 2, 2)
    g[0, 0, 0] = -1.0
    c = torch.tensor([0.0, 1.0])
    v, f = extract_surface(g.to(dev), [c.to(dev)] * 3)
    assert tuple(v.shape) == (1, 3) and tuple(f.shape) == (0, 3)
    assert torch.allclose(v.cpu(), torch.full((1, 3), 1 / 6), atol=1e-6)
