"""Resolutions that are multiples of 8 but not of 64, the CPU side: the crop-equals-nearest rule the engine's upsample
conv relies on, and the sized fp32 UNet (tests/sized_unet_ref.py) the GPU tests compare against."""
import pytest
import torch
import torch.nn.functional as F

import sized_unet_ref


@pytest.mark.parametrize("n", range(1, 65))
def test_nearest_to_odd_size_is_x2_then_crop(n):
    x = torch.arange(2 * n * (n + 1), dtype=torch.float32).reshape(1, 2, n, n + 1)
    to = F.interpolate(x, size=(2 * n - 1, 2 * n + 1), mode="nearest")
    x2 = F.interpolate(x, scale_factor=2.0, mode="nearest")
    assert torch.equal(to, x2[..., : 2 * n - 1, : 2 * n + 1])


def test_level_sizes_are_ceil_halvings():
    assert sized_unet_ref.level_sizes(45) == [45, 23, 12, 6]
    assert sized_unet_ref.level_sizes(25) == [25, 13, 7, 4]
    assert sized_unet_ref.level_sizes(9) == [9, 5, 3, 2]
    assert sized_unet_ref.level_sizes(48) == [48, 24, 12, 6]


@pytest.fixture(scope="module")
def unet_sd():
    from diffusiontexturepainting_amd import weights as W
    from oracle import nets
    return nets.merge_lora(W.synthetic_unet(3), W.synthetic_lora(3))


def _inputs(h, n=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 9, h, h, generator=g), torch.tensor(501.0), torch.randn(n, 14, 768, generator=g)


def test_sized_unet_equals_the_oracle_at_h_8(unet_sd):
    from oracle import nets
    s, t, c = _inputs(8)
    with torch.no_grad():
        assert torch.equal(sized_unet_ref.unet_forward(unet_sd, s, t, c), nets.unet_forward(unet_sd, s, t, c))


@pytest.mark.parametrize("h", [9, 17])
def test_sized_unet_runs_odd_levels(unet_sd, h):
    s, t, c = _inputs(h, seed=h)
    with torch.no_grad():
        out, trace = sized_unet_ref.unet_forward(unet_sd, s, t, c, return_trace=True)
    assert out.shape == (1, 4, h, h) and torch.isfinite(out).all()
    lv = sized_unet_ref.level_sizes(h)
    assert tuple(trace["down"].shape[-2:]) == (lv[3], lv[3])
    assert [tuple(trace[f"up{i}"].shape[-2:]) for i in range(3)] == [(lv[2], lv[2]), (lv[1], lv[1]), (lv[0], lv[0])]
