"""sha256 of the outputs of the op wrappers that reach the staged-tile epilogue (csrc/tile_epilogue.h: gemm_kernel, gemm_wide_kernel,
gemm_fp8_kernel, gemm_f8f8_kernel, conv_halo_kernel, the split-K reduce kernels, xattn_kernel), for a byte-for-byte A/B of two builds of the
library (a change of the epilogue text that leaves the arithmetic and its order alone must leave every line alone):

    python tools/epilogue_digest.py  >  new.txt
    DTP_LIB=tools/ab/libdtp_head.so python tools/epilogue_digest.py  >  ref.txt       (separate processes; then diff)

The shapes are the smallest of the op tests in tests/test_gpu_ops.py / tests/test_gpu_fp8_operands.py that still cross a tile edge (M = 130,
300 on the 256-row tiles; N = 256 / 320; K = 192); a combination the tile's predicate refuses prints `refused`.  Run the reference twice
first: a line it does not reproduce against itself says nothing about the other build."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diffusiontexturepainting_amd import _lib, ops  # noqa: E402
from diffusiontexturepainting_amd._lib import GF_BIAS, GF_BIAS_M, GF_GEGLU, GF_GELU, GF_OUT_F32, GF_QUICKGELU, GF_SILU, GF_SOFTMAX16, DtpError  # noqa: E402

# gemm_kernel: 4-wave tiles of each shape and ring depth, a 256-wide one of each orientation, 8-wave (k-split) twins, loader-wave variants
DENSE = [0, 1, 2, 3, 5, 6, 8, 11, 16, 17, 32, 34, 37, 39, 40, 42, 45, 47]
WIDE = [20, 21]                  # gemm_wide_kernel: 256 x 256, 256 x 320
FP8 = [24, 25, 26, 27, 28]       # gemm_fp8_kernel
F8F8 = [0, 1]                    # gemm_f8f8_kernel: 128 / 64 rows
HALO = [(2, 24, 40, 128, 128, 12, 1), (2, 16, 16, 128, 256, 13, 1), (2, 12, 20, 64, 64, 14, 1), (3, 8, 8, 128, 128, 15, 1), (3, 8, 8, 128, 128, 48, 1),
        (3, 12, 20, 64, 192, 49, 1), (2, 16, 16, 128, 128, 13, 2), (3, 8, 8, 256, 128, 48, 3), (3, 8, 8, 1280, 1280, 15, 5), (3, 8, 8, 1280, 1280, 48, 5)]  # B, H, W, Cin, Cout, variant, splits
ACTS = [("gelu", GF_GELU), ("quickgelu", GF_QUICKGELU), ("silu", GF_SILU)]


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is not None:
            h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:24]


def line(name, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        out = out if isinstance(out, (tuple, list)) else (out,)
        print(f"{name}: {sha(*out)}", flush=True)
    except DtpError as err:
        if "(code 1)" not in str(err):  # DTP_ERR_ARG = the tile's predicate refused the combination; anything else is a failure, not a line
            raise
        print(f"{name}: refused", flush=True)


def main():
    g = torch.Generator().manual_seed(1)

    def f16(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, generator=g) * scale + shift).half().cuda()

    def f32(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda()

    def e4(t, scale):
        return (t.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)

    print(f"# library: {os.environ.get('DTP_LIB') or 'working build'}")
    k = 192
    for tiles, m in ((DENSE, 130), (WIDE, 300)):
        a, r = f16(m, k, scale=1.3, shift=0.3), f16(m, 320)
        w = f32(320, k, scale=k ** -0.5)
        wp, wg = ops.pack_linear(w), ops.pack_linear(w[:256].contiguous(), geglu=True)
        bias, bm, lns, lnsg = f32(320), f32(m), ops.rowsum(wp, k), ops.rowsum(wg, k)
        for t in tiles:
            for n in (256, 320):
                line(f"gemm tile {t} {(m, n, k)} bias", lambda: ops.gemm(a, wp, n, k, bias=bias, tile=t))
                line(f"gemm tile {t} {(m, n, k)} bias + residual", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r[:, :n], tile=t))
                line(f"gemm tile {t} {(m, n, k)} bias + residual + row statistics", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r[:, :n], tile=t, row_stats=True))
                line(f"gemm tile {t} {(m, n, k)} layernorm fold + bias", lambda: ops.gemm(a, wp, n, k, bias=bias, lns=lns, tile=t))
            n = 256
            for name, fl in ACTS:
                line(f"gemm tile {t} {(m, n, k)} bias + {name}", lambda: ops.gemm(a, wp, n, k, bias=bias, flags=fl, tile=t))
            line(f"gemm tile {t} {(m, n, k)} geglu", lambda: ops.gemm(a, wg, n, k, bias=bias, flags=GF_GEGLU | GF_BIAS, tile=t))
            line(f"gemm tile {t} {(m, n, k)} geglu + layernorm fold", lambda: ops.gemm(a, wg, n, k, bias=bias, lns=lnsg, flags=GF_GEGLU | GF_BIAS, tile=t))
            line(f"gemm tile {t} {(m, n, k)} per-row bias", lambda: ops.gemm(a, wp, n, k, bias=bm, flags=GF_BIAS_M, tile=t))
            line(f"gemm tile {t} {(m, n, k)} fp32 output", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r[:, :n], flags=GF_OUT_F32, tile=t))
            line(f"gemm tile {t} {(m, 200, k)} ragged N", lambda: ops.gemm(a, wp, 200, k, bias=bias, resid=r[:, :200], tile=t))
            line(f"gemm tile {t} {(m, 100, k)} ragged N, unaligned rows", lambda: ops.gemm(a, wp, 100, k, bias=bias, resid=r[:, :100].contiguous(), tile=t, row_stats=True))
            line(f"gemm tile {t} {(m, 200, k)} ragged N + row statistics + gelu", lambda: ops.gemm(a, wp, 200, k, bias=bias, flags=GF_GELU, tile=t, row_stats=True))
            # the three reduce kernels: four columns per thread, one column per thread (fp32 output), one wave per row (row statistics)
            line(f"gemm tile {t} {(m, n, k)} 3 K-slices bias + residual + silu", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r[:, :n], flags=GF_SILU, tile=t, splits=3))
            line(f"gemm tile {t} {(m, n, k)} 3 K-slices fp32 output + gelu", lambda: ops.gemm(a, wp, n, k, bias=bias, flags=GF_OUT_F32 | GF_GELU, tile=t, splits=3))
            line(f"gemm tile {t} {(m, n, k)} 2 K-slices row statistics", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r[:, :n], tile=t, splits=2, row_stats=True))
    # grouped problems: LayerNorm fold + 16-wide softmax (shared weights per entry), per-sample biases without a fold, shared bias + residual
    nb, m, c = 3, 130, 320
    x = f16(nb * m, c, scale=1.3, shift=0.2)
    wb = torch.cat([ops.pack_linear(f32(128, c, scale=2.0 * c ** -0.5)) for _ in range(nb)], dim=0).contiguous()
    bb, lb = f32(nb * 128, scale=0.3), ops.rowsum(wb, c)
    pm = f16(nb * m, 128, scale=0.3)
    w2 = torch.cat([ops.pack_linear(f32(c, 128, scale=0.1)) for _ in range(nb)], dim=0).contiguous()
    b2 = f32(c)
    for t in DENSE:
        line(f"gemm tile {t} grouped {(nb, m, 128, c)} layernorm fold + bias + softmax16", lambda: ops.gemm(x, wb, 128, c, bias=bb, lns=lb, tile=t, flags=GF_BIAS | GF_SOFTMAX16, batch=nb, sm_valid=14))
        line(f"gemm tile {t} grouped {(nb, m, 128, c)} per-sample bias", lambda: ops.gemm(x, wb, 128, c, bias=bb, tile=t, batch=nb))
        line(f"gemm tile {t} grouped {(nb, m, c, 128)} shared bias + residual + row statistics", lambda: ops.gemm(pm, w2, c, 128, bias=b2, resid=x, tile=t, batch=nb, bias_shared=True, row_stats=True))
    # e4m3 weights, fp16 activations
    m, n, k = 130, 320, 256
    a, r, bias = f16(m, k), f16(m, n), f32(n)
    wp, wg = ops.pack_linear(f32(n, k, scale=k ** -0.5)), ops.pack_linear(f32(256, k, scale=k ** -0.5), geglu=True)
    (w8, ws), (wg8, wgs) = ops.quantize_w8(wp, k), ops.quantize_w8(wg, k)
    for t in FP8:
        line(f"gemm fp8 tile {t} {(m, n, k)} bias + residual", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r, tile=t, w8=w8, w_scale=ws))
        line(f"gemm fp8 tile {t} {(m, n, k)} bias + residual + row statistics", lambda: ops.gemm(a, wp, n, k, bias=bias, resid=r, tile=t, w8=w8, w_scale=ws, row_stats=True))
        line(f"gemm fp8 tile {t} {(m, 256, k)} geglu", lambda: ops.gemm(a, wg, 256, k, bias=bias, flags=GF_GEGLU | GF_BIAS, tile=t, w8=wg8, w_scale=wgs))
        line(f"gemm fp8 tile {t} {(m, 256, k)} geglu + layernorm", lambda: ops.gemm(a, wg, 256, k, bias=bias, flags=GF_GEGLU | GF_BIAS, tile=t, w8=wg8, w_scale=wgs, layernorm=True))
    # e4m3 weights and activations
    sa, cs = 2.0 ** -6, 2.0 ** -4
    a8 = e4(a, sa)
    for t in F8F8:
        line(f"gemm f8f8 tile {t} {(m, n, k)} bias + residual + row statistics, both outputs", lambda: ops.gemm_f8f8(a8, w8, n, sa, ws, bias=bias, resid=r, tile=t, row_stats=True, out8_scale=cs))
        line(f"gemm f8f8 tile {t} {(m, n, k)} bias, e4m3 output alone", lambda: ops.gemm_f8f8(a8, w8, n, sa, ws, bias=bias, tile=t, out8_scale=cs, out16=False))
        line(f"gemm f8f8 tile {t} {(m, n, k)} bias, fp16 output alone", lambda: ops.gemm_f8f8(a8, w8, n, sa, ws, bias=bias, tile=t))
        line(f"gemm f8f8 tile {t} {(m, 256, k)} geglu, both outputs", lambda: ops.gemm_f8f8(a8, wg8, 256, sa, wgs, bias=bias, flags=GF_GEGLU, tile=t, out8_scale=cs))
        line(f"gemm f8f8 tile {t} {(m, 256, k)} geglu, e4m3 output alone", lambda: ops.gemm_f8f8(a8, wg8, 256, sa, wgs, bias=bias, flags=GF_GEGLU, tile=t, out8_scale=cs, out16=False))
    for b, h, w, cin, cout, variant, splits in HALO:
        xh, wt = f16(b, h, w, cin), f32(cout, cin, 3, 3, scale=(9 * cin) ** -0.5)
        bias, res = f32(cout), f16(b, h, w, cout)
        line(f"conv3x3 halo {(b, h, w, cin, cout)} variant {variant} K-slices {splits} bias + residual",
             lambda: ops.conv3x3(xh, ops.pack_conv(wt), cout, bias=bias, resid=res, wcb=ops.pack_conv_cb(wt), tile=variant, splits=splits))
    for nb, s, c in ((2, 130, 320), (1, 64, 640)):  # xattn_kernel: only its staging store is the shared text
        x = f16(nb * s, c, scale=1.3, shift=0.2)
        xf = x.float()
        st_in = torch.stack([torch.stack([xf.sum(1), (xf * xf).sum(1)], dim=1)]).contiguous()
        w1 = torch.cat([ops.pack_linear(f32(128, c, scale=2.0 * c ** -0.5)) for _ in range(nb)], dim=0).contiguous()
        w2 = torch.cat([ops.pack_linear(f32(c, 128, scale=0.1)) for _ in range(nb)], dim=0).contiguous()
        b1, b2 = f32(nb * 128, scale=0.3), f32(c)
        line(f"xattn {(nb, s, c)}", lambda: ops.xattn(x, w1, b1, ops.rowsum(w1, c), st_in, w2, b2, nb, row_stats=True))


if __name__ == "__main__":
    main()
