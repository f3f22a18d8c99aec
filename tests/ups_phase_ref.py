"""Torch restatement of the phase form of the 3x3 conv over a nearest-2x upsample (conv_ws.hip tiles 56 / 57).

An output pixel of parity (py, px) sees a 2 x 2 block of distinct source pixels, so its nine taps collapse to four: the conv is four
2 x 2 convs over the STORED map, one per parity, whose kernels are sums of the original taps.  Output row 2i + py reads upsampled
rows 2i + py - 1 .. 2i + py + 1, i.e. source rows

    py = 0:  i - 1, i, i      -> tap sets {0}, {1, 2}
    py = 1:  i, i, i + 1      -> tap sets {0, 1}, {2}

and phase tap r of parity py reads source row i - 1 + py + r; columns alike.  Zero padding carries over: a source row / column
outside the map is a padding row / column of the upsampled map.
"""
import torch
import torch.nn.functional as F

TAP_SETS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}  # parity -> the original taps summed into phase tap 0 and 1


def collapse(w):
    """w [Cout, Cin, 3, 3] -> [4, Cout, Cin, 2, 2], phase = 2 py + px.  Sums in w's dtype, one add after the other with ky ascending
    and kx ascending inside a ky: the order pack_conv_ws_ups4_kernel uses in fp32."""
    cout, cin = w.shape[:2]
    out = w.new_zeros(4, cout, cin, 2, 2)
    for py in range(2):
        for px in range(2):
            for ry in range(2):
                for rx in range(2):
                    acc = None
                    for ky in TAP_SETS[py][ry]:
                        for kx in TAP_SETS[px][rx]:
                            acc = w[:, :, ky, kx].clone() if acc is None else acc + w[:, :, ky, kx]
                    out[2 * py + px, :, :, ry, rx] = acc
    return out


def phase_conv(x, w4, bias=None):
    """x [B, Cin, H, W], w4 = collapse(w) -> [B, Cout, 2H, 2W]: phase (py, px) is a 2 x 2 conv over the stored map padded by one pixel,
    its output pixel (y, x) lands at (2y + py, 2x + px)."""
    b, _, h, w = x.shape
    out = x.new_zeros(b, w4.shape[1], 2 * h, 2 * w)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], w4[2 * py + px], bias)
    return out


def pack_ups4(w):
    """CPU restatement of the device packing (dtp_op_pack_conv_ws_ups4): w f32 [Cout, Cin, 3, 3] (Cin % 64 == 0) -> f16, flat.  Collapsed
    weights are summed in fp32 and rounded to fp16 ONCE.  1 KB fragment f = (((phase * nts + nt) * ncb + cb) * 4 + q) * 4 + tap
    (nts = ceil(Cout / 32) n-tiles, ncb = Cin / 64 channel blocks, q = channel quarter, tap = 2 ry + rx); element e of lane l is
    W4[phase][n = 32 nt + (l & 31)][ch = 64 cb + 16 q + 8 (l >> 5) + e][tap], zero for n >= Cout."""
    cout, cin = w.shape[:2]
    assert cin % 64 == 0
    nts, ncb = (cout + 31) // 32, cin // 64
    w4 = collapse(w.float()).half()
    full = torch.zeros(4, nts * 32, cin, 4, dtype=torch.float16)
    full[:, :cout] = w4.reshape(4, cout, cin, 4)
    t = full.reshape(4, nts, 32, ncb, 4, 2, 8, 4)      # phase, nt, l & 31, cb, q, l >> 5, e, tap
    return t.permute(0, 1, 3, 4, 7, 5, 2, 6).contiguous().reshape(-1)
