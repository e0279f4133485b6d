"""scorp_amd.segment without a GPU: argument validation, the voting methods' bookkeeping and the reference's mask files."""
import math

import numpy as np
import pytest
import torch

from scorp_amd import _C
from scorp_amd import segment as S


def test_method_codes_match_the_c_abi():
    assert S.method_code("sums") == _C.VOTE_SUMS == 0
    assert S.method_code("gradient") == _C.VOTE_GRADIENT == 1
    assert S.method_code("binary") == _C.VOTE_BINARY == 2
    with pytest.raises(ValueError, match="projection"):
        S.method_code("projection")
    with pytest.raises(ValueError, match="unknown"):
        S.method_code("votes")


def test_gradient_scale_is_the_channel_norm_of_the_mean_loss():
    # mean(render * mask) over 3 H W elements: dL/dcolor[i, c] = S_in / (3 H W), its norm over 3 channels S_in / (sqrt(3) H W)
    H, W = 1200, 1600
    s_in = 123.25
    per_channel = s_in / (3 * H * W)
    assert math.isclose(S.vote_scale("gradient", H, W) * s_in, math.sqrt(3 * per_channel ** 2), rel_tol=1e-12)
    assert S.vote_scale("binary", H, W) == 1.0 and S.vote_scale("sums", H, W) == 1.0


def test_prepare_masks_checks_the_shape_and_makes_bytes():
    m = np.zeros((2, 4, 5), bool)
    m[1, 2, 3] = True
    out = S.prepare_masks(m, 4, 5, "cpu")
    assert out.dtype == torch.uint8 and out.shape == (2, 4, 5) and int(out.sum()) == 1
    assert S.prepare_masks(torch.tensor(m).float() * 0.5, 4, 5, "cpu").sum() == 1   # nonzero = inside
    for bad in (m[0], m[:, :3], np.zeros((0, 4, 5), bool)):
        with pytest.raises(ValueError, match="masks must be"):
            S.prepare_masks(bad, 4, 5, "cpu")


def test_api_rejects_what_it_cannot_vote_on():
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    with pytest.raises(TypeError):
        S.mask_votes(object(), [], [])
    g = GaussianModel.from_raw(make_gaussians(10, 0, 1), 0, device="cpu")
    cams = ring_cameras(2, 32, 16, 1)
    m = np.zeros((1, 16, 32), bool)
    with pytest.raises(ValueError, match="projection"):
        S.get_mask3d(g, cams, [m, m], "projection")
    with pytest.raises(ValueError, match="2 cameras"):
        S.mask_votes(g, cams, [m])
    with pytest.raises(RuntimeError, match="GPU"):
        S.mask_votes(g, cams, [m, m])
    with pytest.raises(ValueError, match="mask3d"):
        S.apply_mask3d(g, torch.ones(9, dtype=torch.bool), "x.ply")
    with pytest.raises(ValueError, match="mask3d"):
        S.apply_mask3d(g, torch.ones(10, dtype=torch.int32), "x.ply")


def _write_rgba(path, alpha, rgb_only=False):
    from PIL import Image
    h, w = alpha.shape
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = 200
    img[..., 3] = alpha
    path.parent.mkdir(parents=True, exist_ok=True)
    (Image.fromarray(img[..., :3], "RGB") if rgb_only else Image.fromarray(img, "RGBA")).save(path)


def test_load_prompt_masks_reads_the_alpha_channel(tmp_path):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(0)
    a0 = (rng.uniform(size=(12, 20)) > 0.5).astype(np.uint8) * rng.integers(1, 256, (12, 20)).astype(np.uint8)
    a1 = np.zeros((12, 20), np.uint8)
    a1[3:7, 5:9] = 255
    _write_rgba(tmp_path / "masked_image_rgba" / "cup" / "img_0.png", a0)
    _write_rgba(tmp_path / "masked_image_rgba" / "plate" / "img_0.png", a1)
    m = S.load_prompt_masks(str(tmp_path), ["cup", "plate"], "img_0", (20, 12))
    assert m.dtype == torch.bool and m.shape == (2, 12, 20)
    assert np.array_equal(m[0].numpy(), a0 > 0) and np.array_equal(m[1].numpy(), a1 > 0)
    # another resolution: nearest-neighbour resize (a 2x upscale repeats every pixel)
    m2 = S.load_prompt_masks(str(tmp_path), ["plate"], "img_0", (40, 24))
    assert m2.shape == (1, 24, 40) and np.array_equal(m2[0].numpy(), np.repeat(np.repeat(a1 > 0, 2, 0), 2, 1))
    src = S.prompt_mask_source(str(tmp_path), ["cup"])
    cam = type("Cam", (), {"image_name": "img_0", "resolution": (20, 12)})()
    assert torch.equal(src(cam), m[:1])
    with pytest.raises(FileNotFoundError):
        S.load_prompt_masks(str(tmp_path), ["bowl"], "img_0", (20, 12))
    _write_rgba(tmp_path / "masked_image_rgba" / "rgb" / "img_0.png", a1, rgb_only=True)
    with pytest.raises(ValueError, match="alpha"):
        S.load_prompt_masks(str(tmp_path), ["rgb"], "img_0", (20, 12))


@pytest.mark.parametrize("deg,dims", [(0, 3), (3, 3), (0, 2)])
def test_ply_round_trip_of_an_empty_selection(tmp_path, deg, dims):
    """apply_mask3d writes the rows a mask selects, possibly none (an object no Gaussian was voted into): the PLY writer and
    reader handle zero rows, also with the zero-width _features_rest of an SH-0 model."""
    from scorp_amd.ply import read_gaussian_ply, write_ply
    from scorp_amd.synthetic import make_gaussians
    raw = make_gaussians(5, deg, 1, scale_dims=dims)
    for n in (5, 0):
        p = str(tmp_path / f"m{n}.ply")
        write_ply(p, raw["xyz"][:n], raw["features_dc"][:n], raw["features_rest"][:n], raw["opacity"][:n],
                  raw["scaling"][:n], raw["rotation"][:n])
        back = read_gaussian_ply(p, deg)
        for k, v in back.items():
            assert v.shape == raw[k][:n].shape, k
            np.testing.assert_array_equal(v, raw[k][:n])
