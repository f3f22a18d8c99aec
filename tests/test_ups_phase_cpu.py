"""The identity behind the phase tiles of the weight-streaming conv: a 3x3 conv over the nearest-2x upsample equals
four 2x2 convs over the stored map, one per output parity.  fp64, CPU only; borders and a 1 x 1 map included."""
import pytest
import torch
import torch.nn.functional as F

from ups_phase_ref import collapse, pack_ups4, phase_conv


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (8, 16)])
def test_four_phase_convs_equal_the_conv_over_the_upsample(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(2, 6, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(5, 6, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(5, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, bias, padding=1)
    got = phase_conv(x, collapse(wt), bias)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12


def test_collapsed_kernels_keep_the_total_weight_and_the_tap_sets_partition_the_taps():
    wt = torch.randn(3, 4, 3, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    w4 = collapse(wt)
    assert w4.shape == (4, 3, 4, 2, 2)
    assert torch.allclose(w4.sum(dim=(3, 4)), wt.sum(dim=(2, 3)).expand(4, -1, -1), atol=1e-12)
    assert torch.equal(w4[0, :, :, 0, 0], wt[:, :, 0, 0]) and torch.equal(w4[3, :, :, 1, 1], wt[:, :, 2, 2])


def test_packing_layout_of_the_restatement():
    cout, cin = 40, 128  # two n-tiles (the second holds 8 channels), two channel blocks
    wt = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(2))
    flat = pack_ups4(wt)
    nts, ncb = 2, 2
    assert flat.dtype == torch.float16 and flat.numel() == 4 * nts * ncb * 16 * 512
    w4 = collapse(wt).half()
    for phase, nt, cb, q, tap, lane, e in [(0, 0, 0, 0, 0, 0, 0), (3, 1, 1, 3, 3, 39, 7), (2, 0, 1, 2, 1, 63, 5), (1, 1, 0, 1, 2, 8, 3)]:
        f = (((phase * nts + nt) * ncb + cb) * 4 + q) * 4 + tap
        n, ch = 32 * nt + (lane & 31), 64 * cb + 16 * q + 8 * (lane >> 5) + e
        want = w4[phase, n, ch, tap >> 1, tap & 1] if n < cout else torch.tensor(0.0).half()
        assert flat[f * 512 + lane * 8 + e] == want, (phase, nt, cb, q, tap, lane, e)
