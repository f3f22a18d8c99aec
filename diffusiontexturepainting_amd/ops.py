"""Thin torch-tensor wrappers over the kernel-level C-ABI entry points (dtp_op_*).

torch is only the owner of device memory here: every function hands raw pointers to
libdtp.so and returns the output tensor.  Activations are NHWC fp16.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import (GF_BIAS, GF_BIAS_M, GF_GEGLU, GF_GELU, GF_LNFOLD, GF_OUT_F32, GF_QUICKGELU, GF_RESID, GemmDesc, check,
                   ptr)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(x, m):
    return (x + m - 1) // m * m


def pack_linear(w, geglu=False):
    """w f32 [N,K] (device) -> f16 [roundup(N,128), roundup(K,64)] in the kernel layout."""
    lib = _lib.load()
    n, k = w.shape
    out = torch.zeros(_up(n, 128), _up(k, 64), dtype=torch.float16, device=w.device)
    w = w.contiguous().float()
    check(lib.dtp_op_pack_linear(ptr(w), ptr(out), n, k, out.shape[1], int(geglu), _stream()), "pack_linear")
    return out


def pack_conv(w, cin_pad=None):
    """w f32 [Cout,Cin,kh,kw] -> f16 [roundup(Cout,128), roundup(taps*cin_pad,64)], k = tap*cin_pad + ci."""
    lib = _lib.load()
    cout, cin, kh, kw = w.shape
    cin_pad = cin_pad or _up(cin, 8)
    out = torch.zeros(_up(cout, 128), _up(kh * kw * cin_pad, 64), dtype=torch.float16, device=w.device)
    w = w.contiguous().float()
    check(lib.dtp_op_pack_conv(ptr(w), ptr(out), cout, cin, cin_pad, kh * kw, out.shape[1], _stream()), "pack_conv")
    return out


def pack_conv_cb(w):
    """w f32 [Cout,Cin,3,3] (Cin % 64 == 0) -> channel-block-major packing for the halo-tiled conv kernel."""
    lib = _lib.load()
    cout, cin = w.shape[:2]
    out = torch.zeros(_up(cout, 128), 9 * cin, dtype=torch.float16, device=w.device)
    w = w.contiguous().float()
    check(lib.dtp_op_pack_conv_cb(ptr(w), ptr(out), cout, cin, out.shape[1], _stream()), "pack_conv_cb")
    return out


def pack_conv_ws(w, w1=None):
    """w f32 [Cout,Cin,3,3] (Cin % 64 == 0) -> the MFMA-fragment-order packing convws_kernel streams (tile ids 51 / 52); w1 f32
    [Cout,Cin2(,1,1)]: the 1x1 weights of a fused shortcut, packed behind the 3x3 fragments."""
    lib = _lib.load()
    cout, cin = w.shape[:2]
    cin2 = w1.shape[1] if w1 is not None else 0
    out = torch.zeros(lib.dtp_op_pack_conv_ws_elems(cout, cin, cin2), dtype=torch.float16, device=w.device)
    w = w.contiguous().float()
    w1 = w1.reshape(cout, cin2).contiguous().float() if w1 is not None else None
    check(lib.dtp_op_pack_conv_ws(ptr(w), ptr(w1), ptr(out), cout, cin, cin2, _stream()), "pack_conv_ws")
    return out


def pack_conv_ws_ups4(w):
    """w f32 [Cout,Cin,3,3] (Cin % 64 == 0) -> the four phase sets of collapsed 2x2 weights, in MFMA fragment order, that the phase
    build of convws_kernel streams for a conv over the nearest-2x upsample (tile ids 56 / 57; conv3x3(..., upsample=True, wfr4=))."""
    lib = _lib.load()
    cout, cin = w.shape[:2]
    out = torch.zeros(lib.dtp_op_pack_conv_ws_ups4_elems(cout, cin), dtype=torch.float16, device=w.device)
    w = w.contiguous().float()
    check(lib.dtp_op_pack_conv_ws_ups4(ptr(w), ptr(out), cout, cin, _stream()), "pack_conv_ws_ups4")
    return out


def pack_linear_ws(wp, n, k):
    """wp: packed f16 rows of pack_linear (k % 64 == 0) -> the MFMA-fragment-order copy gemmws_kernel streams (tile id 55)."""
    lib = _lib.load()
    out = torch.zeros(lib.dtp_op_pack_linear_ws_elems(n, k), dtype=torch.float16, device=wp.device)
    check(lib.dtp_op_pack_linear_ws(ptr(wp), wp.stride(0), ptr(out), n, k, _stream()), "pack_linear_ws")
    return out


def lora_refit(w0, up, down, scale=1.0, gamma=None, out=None, row0=0):
    """One matrix through the refit kernel: rows row0 .. row0 + N - 1 of `out` = f16((w0 + scale * up @ down) * gamma) in the packed
    layout.  w0 f32 [N,K], up f32 [N,rank], down f32 [rank,K] (up = down = None: no LoRA), gamma f32 [K] or None; out f16
    [>= roundup(row0 + N, 128), ldw] (default: a zeroed [roundup(row0 + N, 128), roundup(K, 64)]); rows outside and columns >= K are not
    written.  Returns out."""
    lib = _lib.load()
    n, k = w0.shape
    if out is None:
        out = torch.zeros(_up(row0 + n, 128), _up(k, 64), dtype=torch.float16, device=w0.device)
    if out.dim() != 2 or out.dtype != torch.float16 or out.stride(1) != 1 or out.shape[0] < row0 + n:
        raise ValueError(f"lora_refit: out must be f16 [>= {row0 + n}, ldw] with unit column stride, got {tuple(out.shape)}")
    w0 = w0.contiguous().float()
    rank = 0 if up is None else up.shape[1]
    up = up.contiguous().float() if up is not None else None
    down = down.contiguous().float() if down is not None else None
    gamma = gamma.contiguous().float() if gamma is not None else None
    check(lib.dtp_op_lora_refit(ptr(w0), ptr(up), ptr(down), rank, float(scale), ptr(gamma), ptr(out), int(row0), n, k, out.stride(0),
                                _stream()), "lora_refit")
    return out


def rowsum(wp, k):
    """fp32 row sums of packed fp16 weights over the first k columns (the `lns` vector of a LayerNorm-folded GEMM)."""
    lib = _lib.load()
    out = torch.empty(wp.shape[0], dtype=torch.float32, device=wp.device)
    check(lib.dtp_op_rowsum(ptr(wp), wp.stride(0), k, ptr(out), wp.shape[0], _stream()), "rowsum")
    return out


def quantize_w8(wp, k):
    """packed f16 weights [rows, ldw] -> (e4m3 bytes [rows, roundup(k,128)], per-tensor scale) for the fp8 GEMM tiles 24..27."""
    lib = _lib.load()
    out = torch.zeros(wp.shape[0], _up(k, 128), dtype=torch.uint8, device=wp.device)
    sc = C.c_float()
    check(lib.dtp_op_quantize_w8(ptr(wp), wp.stride(0), k, wp.shape[0], ptr(out), out.shape[1], C.byref(sc), _stream()), "quantize_w8")
    return out, sc.value


def quant_e4m3(x, scale, ln=False, stats_in=None, eps=1e-5, k=None, x2=None, scale2=1.0, ln2=False, k2=None):
    """fp16 rows x [M, >=k] -> e4m3 bytes (torch.uint8) [M, k] = e4m3(x / scale), saturating at +-448; ln=True first applies the
    LayerNorm (x - mean) * rstd (no gamma / beta) with the producer's per-row partials stats_in f32 [parts, M, 2] (None: computed
    in-kernel).  x2 (or None): a second job over the same rows in the same launch; then returns both outputs."""
    lib = _lib.load()
    m = x.shape[0]
    k = k or x.shape[1]
    y = torch.empty(m, k, dtype=torch.uint8, device=x.device)
    y2 = None
    if x2 is not None:
        k2 = k2 or x2.shape[1]
        y2 = torch.empty(m, k2, dtype=torch.uint8, device=x.device)
    st = stats_in.contiguous() if stats_in is not None else None
    check(lib.dtp_op_quant_e4m3(ptr(x), x.stride(0), ptr(y), y.stride(0), k, float(scale), int(ln),
                                ptr(x2), x2.stride(0) if x2 is not None else 0, ptr(y2), y2.stride(0) if y2 is not None else 0,
                                k2 or 0, float(scale2), int(ln2), m, ptr(st), st.shape[0] if st is not None else 0, eps, _stream()),
          "quant_e4m3")
    return (y, y2) if x2 is not None else y


def gemm_f8f8(a8, w8, n, a_scale, w_scale, k=None, bias=None, resid=None, flags=0, tile=-1, tail8=None, row_stats=False,
              out8_scale=None, out16=True, tail_scale=None):
    """Both operands e4m3 (torch.uint8): a8 [M, >=k] = e4m3(A / a_scale), w8 [rows, ldw8] from quantize_w8 (scale w_scale);
    tail8 (or None): e4m3 [M, K2] supplying the last K2 columns (scale tail_scale, default a_scale).  Returns the f16 output [M, N] (or [M, N/2] with
    GEGLU; None with out16=False), the e4m3 output (out8_scale given: e4m3(out / out8_scale)) and, with row_stats, the partials."""
    lib = _lib.load()
    m = a8.shape[0]
    k = k or a8.shape[1]
    n_out = n // 2 if flags & GF_GEGLU else n
    d = GemmDesc()
    out = torch.empty(m, n_out, dtype=torch.float16, device=a8.device) if out16 else None
    out8 = torch.empty(m, n_out, dtype=torch.uint8, device=a8.device) if out8_scale is not None else None
    d.A8, d.lda8 = a8.data_ptr(), a8.stride(0)
    d.W8, d.ldw8, d.a_scale, d.w_scale = w8.data_ptr(), w8.stride(0), a_scale, w_scale
    d.C, d.ldc = (out.data_ptr(), out.stride(0)) if out is not None else (None, 0)
    if out8 is not None:
        d.C8, d.ldc8, d.c_scale = out8.data_ptr(), out8.stride(0), out8_scale
    d.bias = bias.data_ptr() if bias is not None else None
    d.R = resid.data_ptr() if resid is not None else None
    d.ldr = resid.stride(0) if resid is not None else 0
    d.M, d.N, d.K = m, n, k
    d.flags = flags | (GF_BIAS if bias is not None else 0) | (GF_RESID if resid is not None else 0)
    d.tile = tile
    if tail8 is not None:
        d.A2_8, d.lda2_8, d.Cin2 = tail8.data_ptr(), tail8.stride(0), tail8.shape[1]
        d.a2_scale = tail_scale or 0.0
        d.K = k + tail8.shape[1]
    st = None
    if row_stats:
        st = torch.zeros((n + 127) // 128, m, 2, dtype=torch.float32, device=a8.device)
        d.st_out = st.data_ptr()
        d.flags |= _lib.GF_ROWSTATS
    check(lib.dtp_op_gemm_f8f8(C.byref(d), _stream()), "gemm_f8f8")
    if row_stats:
        st = st[:d.st_parts_out]
    return out, out8, st


def gemm(a, wp, n, k=None, bias=None, resid=None, flags=0, tile=-1, splits=0, out=None, lda=None, lns=None, ln_eps=1e-5, batch=0,
         sm_valid=0, bias_shared=False, tail=None, row_stats=False, stats_in=None, w8=None, w_scale=1.0, a_scale=1.0, layernorm=False,
         wfr=None):
    """a f16 [M, >=K] row-major; wp packed weights; returns f16 [M, N] (or [M, N/2] with GEGLU).
    batch > 1: a is [batch*M, K] (problem b = rows b*M..), wp is [batch*Npad, Kpad], bias / lns are [batch*Npad]."""
    lib = _lib.load()
    m = a.shape[0] // batch if batch > 1 else a.shape[0]
    k = k or a.shape[1]
    n_out = n // 2 if flags & GF_GEGLU else n
    if out is None:
        out = torch.empty(a.shape[0], n_out, dtype=torch.float32 if flags & GF_OUT_F32 else torch.float16, device=a.device)
    d = GemmDesc()
    d.A, d.W, d.C = a.data_ptr(), wp.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.R = resid.data_ptr() if resid is not None else None
    d.M, d.N, d.K = m, n, k
    d.lda, d.ldw, d.ldc = lda or a.stride(0), wp.stride(0), out.stride(0)
    d.ldr = resid.stride(0) if resid is not None else 0
    d.flags = flags | (GF_BIAS if bias is not None and not flags & GF_BIAS_M else 0) | (GF_RESID if resid is not None else 0)
    d.tile, d.splits = tile, splits
    if lns is not None:
        d.lns, d.ln_eps = lns.data_ptr(), ln_eps
        d.flags |= GF_LNFOLD
    if batch > 1:
        npad = wp.shape[0] // batch
        d.batch, d.a_bs, d.w_bs, d.c_bs = batch, m * d.lda, npad * d.ldw, m * d.ldc
        d.r_bs, d.bias_bs, d.lns_bs = m * d.ldr, 0 if bias_shared else npad, npad
    d.sm_valid = sm_valid
    if tail is not None:  # second activation matrix: supplies the last tail.shape[1] columns of the contraction
        d.A2, d.lda2, d.Cin2 = tail.data_ptr(), tail.stride(0), tail.shape[1]
        d.K = k + tail.shape[1]
    if w8 is not None:  # fp8 tiles: the e4m3 weight copy + scales; layernorm=True applies (x - mean) * rstd while staging A
        d.W8, d.ldw8, d.w_scale, d.a_scale = w8.data_ptr(), w8.stride(0), w_scale, a_scale
        if layernorm:
            d.flags |= GF_LNFOLD
            d.ln_eps = ln_eps
    if wfr is not None:  # tile 55: the fragment-order copy of wp (pack_linear_ws)
        d.Wfr = wfr.data_ptr()
    st = None
    if row_stats:  # also return the per-row (sum, sumsq) partials of the fp16 output: f32 [parts, M, 2]
        st = torch.zeros((n + 63) // 64, a.shape[0], 2, dtype=torch.float32, device=a.device)
        d.st_out = st.data_ptr()
        d.flags |= _lib.GF_ROWSTATS
    if stats_in is not None:  # LayerNorm fold with the producer's partials instead of in-kernel statistics
        d.st_in, d.st_parts = stats_in.data_ptr(), stats_in.shape[0]
    check(lib.dtp_op_gemm(C.byref(d), _stream()), "gemm")
    if row_stats:
        return out, st[: d.st_parts_out]
    return out


def _conv3x3_desc(x, wp, cout, stride=1, pad=1, upsample=False, bias=None, resid=None, tile=-1, splits=0, out_hw=None, flags=0,
                  tail=None, wcb=None, wfr=None, gn_groups=0, wfr4=None):
    """the descriptor of conv3x3 with its output (and, with gn_groups, statistics) tensors"""
    b, h, w, cin = x.shape
    hv, wv = (2 * h, 2 * w) if upsample else (h, w)
    ho, wo = out_hw or ((hv + 2 * pad - 3) // stride + 1, (wv + 2 * pad - 3) // stride + 1)
    out = torch.empty(b, ho, wo, cout, dtype=torch.float32 if flags & GF_OUT_F32 else torch.float16, device=x.device)
    d = GemmDesc()
    d.A, d.W, d.C = x.data_ptr(), wp.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.R = resid.data_ptr() if resid is not None else None
    d.M, d.N, d.K = b * ho * wo, cout, 9 * cin + (tail.shape[-1] if tail is not None else 0)
    if tail is not None:  # fused 1x1 shortcut: NHWC tensor with the output's spatial size
        d.A2, d.lda2, d.Cin2 = tail.data_ptr(), tail.stride(2), tail.shape[-1]
    d.lda, d.ldw, d.ldc = x.stride(2), wp.stride(0), cout
    d.ldr = resid.stride(2) if resid is not None else 0
    d.conv, d.Hi, d.Wi, d.Ho, d.Wo, d.Cin, d.stride, d.pad, d.upsample2x = 1, h, w, ho, wo, cin, stride, pad, int(upsample)
    d.flags = flags | (GF_BIAS if bias is not None else 0) | (GF_RESID if resid is not None else 0)
    d.tile, d.splits = tile, splits
    if wcb is not None:
        d.Wcb = wcb.data_ptr()
    if wfr is not None:
        d.Wfr = wfr.data_ptr()
    st = None
    if gn_groups:  # tiles 53 / 54 / 56 / 57, unsplit: also return the GroupNorm partial sums f32 [B, 2 * tiles, groups, 2] of the output
        st = torch.full((b, 2 * ((ho + 7) // 8) * ((wo + 15) // 16), gn_groups, 2), float("nan"), dtype=torch.float32, device=x.device)
        d.st_out, d.gn_cpg = st.data_ptr(), cout // gn_groups
        d.flags |= _lib.GF_GNSTATS
    return d, out, st


def conv3x3(x, wp, cout, *args, **kw):
    """x f16 NHWC [B,H,W,C] -> f16 NHWC [B,Ho,Wo,cout].  pad is the top/left zero padding; bottom/right
    padding is implied by out_hw (default: the symmetric-padding output size).  Arguments: _conv3x3_desc; wfr4 (keyword, with
    upsample=True): the phase sets of pack_conv_ws_ups4 that tiles 56 / 57 read -- the launch then goes through dtp_op_conv_ups4."""
    d, out, st = _conv3x3_desc(x, wp, cout, *args, **kw)
    if kw.get("wfr4") is not None:
        check(_lib.load().dtp_op_conv_ups4(C.byref(d), ptr(kw["wfr4"]), _stream()), "conv3x3")
    else:
        check(_lib.load().dtp_op_gemm(C.byref(d), _stream()), "conv3x3")
    return (out, st) if st is not None else out


def conv_ws_supported(x, wp, cout, tile, splits=1, **kw):
    """Does convws_kernel tile `tile` (51 .. 54, 56 / 57) take the conv conv3x3(x, wp, cout, **kw) would launch?"""
    d, _, _ = _conv3x3_desc(x, wp, cout, tile=tile, splits=splits, **kw)
    return bool(_lib.load().dtp_op_conv_ws_supported(C.byref(d), ptr(kw.get("wfr4")), tile, splits))


def groupnorm(x, gamma, beta, groups=32, eps=1e-5, silu=False):
    """x f16 NHWC [B,H,W,C] (or [B,HW,C])."""
    lib = _lib.load()
    b, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * c)
    y = torch.empty_like(x)
    check(lib.dtp_op_groupnorm(ptr(x), c, ptr(y), c, ptr(gamma), ptr(beta), b, hw, c, groups, eps, int(silu), _stream()),
          "groupnorm")
    return y


def groupnorm_apply(x, gamma, beta, partial, groups=32, eps=1e-5, silu=False):
    """GroupNorm of x f16 [B,H,W,C] from producer-emitted partial sums f32 [B, nchunk, groups, 2] (no statistics pass)."""
    lib = _lib.load()
    b, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * c)
    y = torch.empty_like(x)
    check(lib.dtp_op_groupnorm_apply(ptr(x), c, ptr(y), c, ptr(gamma), ptr(beta), ptr(partial), partial.shape[1], b, hw, c, groups, eps, int(silu),
                                     _stream()), "groupnorm_apply")
    return y


def reduce_groupnorm(part, gamma, beta, bias=None, resid=None, groups=32, eps=1e-5, silu=False, skip=None):
    """part f32 [splits, B, HW, Cx] split-K slabs of a conv -> (conv output f16 [B,HW,C], GroupNorm(+SiLU) of it).
    skip f16 [B, HW, C - Cx] (optional): the tensor is the zero-copy concatenation [conv output | skip]; the slabs (bias, residual) cover its
    first Cx channels only and the GroupNorm runs over all C = Cx + skip channels."""
    lib = _lib.load()
    sp, b, hw, cx = part.shape
    c = cx + (skip.shape[-1] if skip is not None else 0)
    out, y = torch.empty(b, hw, c, dtype=torch.float16, device=part.device), torch.empty(b, hw, c, dtype=torch.float16, device=part.device)
    if skip is not None:
        out[..., cx:] = skip
    check(lib.dtp_op_reduce_groupnorm_cx(ptr(part), sp, ptr(bias), ptr(resid), ptr(out), ptr(y), ptr(gamma), ptr(beta), b, hw, c, groups, eps, int(silu), cx,
                                         _stream()), "reduce_groupnorm")
    return out, y


def groupnorm_stats_apply(gamma, beta, x=None, part=None, bias=None, resid=None, groups=32, eps=1e-5, silu=False):
    """The statistics pass, then the apply pass from its partial sums.  part f32 [splits, B, HW, C] split-K slabs of a conv (+ bias, + resid):
    the statistics pass sums them -> (conv output f16 [B,HW,C], GroupNorm(+SiLU) of it); part None: GroupNorm of x f16 [B,HW,C] -> (x, y)."""
    lib = _lib.load()
    sp, (b, hw, c) = (part.shape[0], part.shape[1:]) if part is not None else (0, x.shape)
    out = x if part is None else torch.empty(b, hw, c, dtype=torch.float16, device=part.device)
    y = torch.empty_like(out)
    check(lib.dtp_op_groupnorm_stats_apply(ptr(part), sp, ptr(bias), ptr(resid), ptr(out), ptr(y), ptr(gamma), ptr(beta), b, hw, c, groups, eps, int(silu),
                                           _stream()), "groupnorm_stats_apply")
    return out, y


def xattn(x, w1, b1, lns1, st_in, w2, b2, n_samples, sm_valid=14, ln_eps=1e-5, row_stats=False, ct=0):
    """Fused cross-attention GEMM pair (xattn.hip): x f16 [N*S, C]; w1 f16 [N*128, C]; b1 / lns1 f32 [N*128]; st_in f32 [parts, N*S, 2];
    w2 f16 [N*roundup(C,128), 128]; b2 f32 [C] -> y f16 [N*S, C] (and the [ceil(C/128), N*S, 2] row-statistics partials).
    ct: 128-column tiles per workgroup (0 = the launcher's rule)."""
    lib = _lib.load()
    rows, c = x.shape
    s = rows // n_samples
    y = torch.empty_like(x)
    st = torch.zeros((c + 127) // 128, rows, 2, dtype=torch.float32, device=x.device) if row_stats else None
    check(lib.dtp_op_xattn_ct(ptr(x), ptr(w1), ptr(b1), ptr(lns1), ptr(st_in), st_in.shape[0], ptr(w2), ptr(b2), ptr(x), ptr(y), ptr(st), s, c, n_samples,
                              sm_valid, ln_eps, int(ct), _stream()), "xattn")
    return (y, st) if row_stats else y


def xchain(a, wo, bo, y, w1, b1, lns1, w2, b2, n_samples, sm_valid=14, ln_eps=1e-5, row_stats=False):
    """Register-chained out-projection + cross-attention (xchain.hip): a / y f16 [N*S, C = 320]; wo packed f16 [rows, ldw]; w1 / b1 / lns1 / w2 /
    b2 as for xattn() -> y3 f16 [N*S, C] (and the [N*S, 2] row statistics of y3)."""
    lib = _lib.load()
    rows, c = a.shape
    s = rows // n_samples
    y3 = torch.empty_like(a)
    st = torch.zeros(rows, 2, dtype=torch.float32, device=a.device) if row_stats else None
    check(lib.dtp_op_xchain(ptr(a), ptr(wo), wo.shape[1], ptr(bo), ptr(y), ptr(w1), ptr(b1), ptr(lns1), ptr(w2), ptr(b2), ptr(y3), ptr(st), s, c,
                            n_samples, sm_valid, ln_eps, _stream()), "xchain")
    return (y3, st) if row_stats else y3


def ffchain(x, w1, lns1, b1, wm, bm, resid=None, ln_eps=1e-5):
    """Register-chained feed-forward (ffchain.hip): x f16 [M, 320]; w1 packed (geglu) f16 [2560, ldw] with lns1 / b1 f32 [2560] by packed row; wm
    packed f16 [rows, 1600] = the merged [ff.net.2 | proj_out] weights -> out f16 [M, 320] = [GEGLU(LN(x) w1^T + b1) | x] wm^T + bm + resid."""
    lib = _lib.load()
    m, c = x.shape
    out = torch.empty_like(x)
    check(lib.dtp_op_ffchain(ptr(x), ptr(w1), w1.shape[1], ptr(lns1), ptr(b1), ptr(wm), wm.shape[1], ptr(bm), ptr(resid), ptr(out), m, c, ln_eps,
                             _stream()), "ffchain")
    return out


def gn_fold_weights(x, wp, n_out, bias, gamma, beta, groups=32, eps=1e-6):
    """x f16 [B,HW,C], wp packed f16 [rows, ldw] -> (per-sample packed weights f16 [B, rows, ldw], biases f32 [B, rows]) such that
    proj(GroupNorm(x_b)) == x_b @ W_b^T + b_b (GroupNorm without activation folded into its consumer)."""
    lib = _lib.load()
    b, hw, c = x.shape
    rows = _up(n_out, 128)
    wout = torch.zeros(b, rows, wp.shape[1], dtype=torch.float16, device=x.device)
    bout = torch.zeros(b, rows, dtype=torch.float32, device=x.device)
    check(lib.dtp_op_gn_fold_weights(ptr(x), ptr(wp), wp.shape[1], ptr(bias), ptr(gamma), ptr(beta), b, hw, c, n_out, groups, eps, ptr(wout), ptr(bout),
                                     _stream()), "gn_fold_weights")
    return wout, bout


def gn_linear(x, wp, n_out, bias, gamma, beta, groups=32, eps=1e-6, col_ranges=4, row_stats=False):
    """x f16 [B,HW,C] (C in {320, 640}, HW % 128 == 0), wp packed f16 [rows, ldw] -> y f16 [B,HW,n_out] = proj(GroupNorm(x)) in one launch
    behind the statistics pass: the GroupNorm is applied to the resident activation fragments of lnlin_kernel (no fold, no apply pass)."""
    lib = _lib.load()
    b, hw, c = x.shape
    y = torch.empty(b, hw, n_out, dtype=torch.float16, device=x.device)
    st = torch.zeros(col_ranges, b * hw, 2, dtype=torch.float32, device=x.device) if row_stats else None
    check(lib.dtp_op_gn_linear(ptr(x), ptr(wp), wp.shape[1], ptr(bias), ptr(gamma), ptr(beta), b, hw, c, n_out, groups, eps, ptr(y), ptr(st),
                               col_ranges, _stream()), "gn_linear")
    return (y, st) if row_stats else y


def layernorm(x, gamma, beta, eps=1e-5):
    """x f16 [..., C] contiguous, or a 2-D row view [rows, C] of a wider / longer buffer (unit column stride, any row pitch)."""
    lib = _lib.load()
    c = x.shape[-1]
    rows = x.numel() // c
    ldx = c
    if not x.is_contiguous():
        if x.dim() != 2 or x.stride(1) != 1:
            raise ValueError(f"layernorm: a non-contiguous input must be a 2-D row view with unit column stride, got strides {x.stride()}")
        ldx = x.stride(0)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    check(lib.dtp_op_layernorm(ptr(x), ldx, ptr(y), c, ptr(gamma), ptr(beta), rows, c, eps, _stream()), "layernorm")
    return y


def attention(q, k, v, heads, scale=None):
    """q [B,Sq,C], k/v [B,Skv,C] f16 (last dim contiguous; may be column slices of a fused buffer)."""
    lib = _lib.load()
    b, sq, c = q.shape
    skv = k.shape[1]
    d = c // heads
    o = torch.empty(b, sq, c, dtype=torch.float16, device=q.device)
    scale = scale if scale is not None else d ** -0.5
    check(lib.dtp_op_attention(ptr(q), ptr(k), ptr(v), ptr(o), q.stride(1), k.stride(1), v.stride(1), o.stride(1), b, heads,
                               sq, skv, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, _stream()), "attention")
    return o


def attention_dma_supported(sq, skv, heads, d):
    """Would attn_dma_kernel take a contiguous [B, S, heads * d] problem?  (d in {40, 80} in the product build.)"""
    lib = _lib.load()
    c = heads * d
    return lib.dtp_op_attention_dma(None, None, None, None, c, c, c, c, 1, heads, sq, skv, d, sq * c, skv * c, skv * c, sq * c, 1.0, 0, None) == 0


def attention_dma(q, k, v, heads, scale=None, nw=0):
    """attention() forced onto the LDS-DMA kernel (attn_dma.hip) whatever the sequence length; nw = waves per workgroup (0 = rule, 4, 8)."""
    lib = _lib.load()
    b, sq, c = q.shape
    skv = k.shape[1]
    d = c // heads
    o = torch.empty(b, sq, c, dtype=torch.float16, device=q.device)
    scale = scale if scale is not None else d ** -0.5
    check(lib.dtp_op_attention_dma(ptr(q), ptr(k), ptr(v), ptr(o), q.stride(1), k.stride(1), v.stride(1), o.stride(1), b, heads,
                                   sq, skv, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, int(nw), _stream()), "attention_dma")
    return o


def attention_fp8(q, k, v, heads, scale=None, q_scale=1.0, v_scale=1.0):
    """attention() with both contractions on the fp8 (e4m3) MX MFMA; tensors stay f16 in memory."""
    lib = _lib.load()
    b, sq, c = q.shape
    skv = k.shape[1]
    d = c // heads
    o = torch.empty(b, sq, c, dtype=torch.float16, device=q.device)
    scale = scale if scale is not None else d ** -0.5
    check(lib.dtp_op_attention_fp8(ptr(q), ptr(k), ptr(v), ptr(o), q.stride(1), k.stride(1), v.stride(1), o.stride(1), b, heads,
                                   sq, skv, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, q_scale, v_scale, _stream()),
          "attention_fp8")
    return o


def softmax_rows(x, scale=1.0):
    lib = _lib.load()
    rows, cols = x.shape
    y = torch.empty_like(x)
    check(lib.dtp_op_softmax_rows(ptr(x), x.stride(0), ptr(y), y.stride(0), rows, cols, scale, _stream()), "softmax_rows")
    return y


def dilate_alpha(canvas, pad):
    """canvas f32 [B,4,R,R] -> f32 [B,1,R,R]: flat pad x pad dilation of the alpha plane (handler.py:28-29)."""
    lib = _lib.load()
    b, _, r, _ = canvas.shape
    canvas = canvas.contiguous().float()
    tmp = torch.empty(b, r, r, dtype=torch.float32, device=canvas.device)
    out = torch.empty(b, 1, r, r, dtype=torch.float32, device=canvas.device)
    check(lib.dtp_op_dilate(ptr(canvas), ptr(tmp), ptr(out), b, r, int(pad), _stream()), "dilate")
    return out


def dilate_alpha_pads(canvas, pads):
    """dilate_alpha with one pad per image (pads: B ints), in one launch pair as a mixed-settings stamp runs it."""
    lib = _lib.load()
    b, _, r, _ = canvas.shape
    if len(pads) != b:
        raise ValueError(f"{len(pads)} pads for {b} images")
    canvas = canvas.contiguous().float()
    tmp = torch.empty(b, r, r, dtype=torch.float32, device=canvas.device)
    out = torch.empty(b, 1, r, r, dtype=torch.float32, device=canvas.device)
    arr = (C.c_int * b)(*[int(p) for p in pads])
    check(lib.dtp_op_dilate_pads(ptr(canvas), ptr(tmp), ptr(out), b, r, arr, _stream()), "dilate")
    return out


def scheduler_tables(scheduler, steps):
    """Host-only schedule tables of a sampler ("DDIM" | "DPM" | "LMSD" or its id) for `steps` steps, as the stamp uploads them:
    dict(evals=E, init_sigma, timesteps f32 [E], in_scale f32 [E + 1], coefs f32 [E, 8]) -- row layouts in include/dtp.h."""
    import numpy as np
    lib = _lib.load()
    sid = _lib.scheduler_id(scheduler) if isinstance(scheduler, str) else int(scheduler)
    n = max(int(steps), 1)
    ev, sig = C.c_int(), C.c_float()
    ts, sc, cf = (C.c_float * n)(), (C.c_float * (n + 1))(), (C.c_float * (n * _lib.SCHED_ROW))()
    check(lib.dtp_scheduler_tables(sid, int(steps), C.byref(ev), C.byref(sig), ts, sc, cf), "dtp_scheduler_tables")
    e = ev.value
    return dict(evals=e, init_sigma=sig.value, timesteps=np.array(ts[:e], dtype=np.float32),
                in_scale=np.array(sc[:e + 1], dtype=np.float32),
                coefs=np.array(cf[:e * _lib.SCHED_ROW], dtype=np.float32).reshape(e, _lib.SCHED_ROW))


def sched_step(scheduler, row, next_scale, eps_out, x, hist, cfg, tg, rank, k, step_index):
    """One sampler update with the stamp's own step kernel (dtp_op_sched_step), in place on the caller's device tensors.
    eps_out f32 [2B + k, 4, h, w] UNet outputs in the stamp's row order; x f32 [B, 4, h, w] (updated); hist f32 [3, B, h*w*4]
    (NHWC history, persists across calls); row: one coefficient row (8 floats); cfg / tg / rank: B per-stamp values.
    Returns the fp16 UNet input rows the kernel wrote, latent channels only: f16 [2B + k, 4, h, w]."""
    lib = _lib.load()
    sid = _lib.scheduler_id(scheduler) if isinstance(scheduler, str) else int(scheduler)
    b, _, h, w = x.shape
    dev = x.device
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().float()  # noqa: E731
    e = nhwc(eps_out)
    xs = nhwc(x)
    in16 = torch.zeros(2 * b + int(k), h, w, 16, dtype=torch.float16, device=dev)
    row_t = torch.as_tensor(row, dtype=torch.float32).reshape(-1)[: _lib.SCHED_ROW].to(dev).contiguous()
    sc = torch.tensor([float(next_scale)], dtype=torch.float32, device=dev)
    cfg_t = torch.tensor([float(v) for v in cfg], dtype=torch.float32, device=dev)
    tg_t = torch.tensor([float(v) for v in tg], dtype=torch.float32, device=dev)
    rank_t = torch.tensor([int(v) for v in rank], dtype=torch.int32, device=dev)
    if hist.numel() < 3 * b * h * w * 4 or not hist.is_contiguous() or hist.dtype != torch.float32:
        raise ValueError("hist must be a contiguous f32 tensor of 3 * B * h * w * 4 elements")
    check(lib.dtp_op_sched_step(sid, ptr(e), ptr(xs), ptr(hist), ptr(in16), ptr(row_t), ptr(sc), ptr(cfg_t), ptr(tg_t), ptr(rank_t),
                                int(step_index), b, h * w, int(k), _stream()), "sched_step")
    x.copy_(xs.permute(0, 3, 1, 2))
    return in16[..., :4].permute(0, 3, 1, 2)


def strength_schedule(scheduler, steps, strength):
    """Host-only initialize_timesteps of a sampler ("DDIM" | "DPM" | "LMSD" or its id) at `strength` (dtp_strength_schedule):
    dict(t_start, evals, noise_coefs=(a, b)) -- the stamp's start point is a * z0 + b * latents and its loop runs table rows
    t_start - steps_offset .. + evals - 1."""
    lib = _lib.load()
    sid = _lib.scheduler_id(scheduler) if isinstance(scheduler, str) else int(scheduler)
    ts, ev, nc = C.c_int(), C.c_int(), (C.c_float * 2)()
    check(lib.dtp_strength_schedule(sid, int(steps), C.c_double(float(strength)), C.byref(ts), C.byref(ev), nc), "dtp_strength_schedule")
    return dict(t_start=ts.value, evals=ev.value, noise_coefs=(nc[0], nc[1]))


def strength_init(z0, eps, a, b):
    """The stamp's strength < 1 start point a * z0 + b * eps (dtp_op_strength_init) of two f32 device tensors of one shape."""
    if z0.shape != eps.shape:
        raise ValueError(f"z0 {tuple(z0.shape)} and eps {tuple(eps.shape)} differ")
    lib = _lib.load()
    z = z0.float().contiguous()
    e = eps.float().contiguous()
    out = torch.empty_like(z)
    check(lib.dtp_op_strength_init(ptr(z), ptr(e), C.c_float(float(a)), C.c_float(float(b)), ptr(out), C.c_longlong(z.numel()), _stream()),
          "strength_init")
    return out


def philox4x32(counter, key):
    """Host-only: Philox4x32-10 of one (counter: 4 uint32, key: 2 uint32) -> 4 uint32, the bit generator of the seeded stamps
    (dtp_philox4x32: the function the noise kernel runs)."""
    lib = _lib.load()
    ctr, k, out = (C.c_uint32 * 4)(*[int(v) for v in counter]), (C.c_uint32 * 2)(*[int(v) for v in key]), (C.c_uint32 * 4)()
    check(lib.dtp_philox4x32(ctr, k, out), "dtp_philox4x32")
    return tuple(out)


def stamp_noise(seed, draw, n, device=None):
    """The n = 4 h w normals of draw `draw` (0 latents, 1 / 2 the VAE draws of the masked / context image, 3 init_eps) of a stamp
    seeded `seed` (0 .. 2^64 - 1), as dtp_stamp_seeded draws them (dtp_op_stamp_noise: the same device function): f32 [n]."""
    lib = _lib.load()
    out = torch.empty(max(int(n), 0), dtype=torch.float32, device=device if device is not None else torch.cuda.current_device())
    check(lib.dtp_op_stamp_noise(C.c_uint64(int(seed)), int(draw), ptr(out), C.c_longlong(int(n)), _stream()), "stamp_noise")
    return out


def _windows(xs, ys, modes):
    B = len(xs)
    arr = C.c_int * B
    return B, arr(*[int(v) for v in xs]), arr(*[int(v) for v in ys]), (arr(*[int(v) for v in modes]) if modes is not None else None)


def stroke_gather(texture, xs, ys, R, modes=None, wrap=False, over_y=0, over_x=0):
    """dtp_op_stroke_gather, the gather kernel of dtp_stroke on its own: texture u8 [H,W,4] (device) and B windows with top-left texel
    (row ys[b], column xs[b]) and DTP_STROKE_* modes[b] -> canvas f32 [B,4,R,R] = texel / 255; 0 outside a non-wrapping texture and in
    the inner rectangle of an Overpaint window."""
    lib = _lib.load()
    B, ax, ay, am = _windows(xs, ys, modes)
    canvas = torch.empty(B, 4, R, R, dtype=torch.float32, device=texture.device)
    check(lib.dtp_op_stroke_gather(ptr(texture), texture.shape[0], texture.shape[1], ptr(canvas), int(R), B, ax, ay, am, int(bool(wrap)),
                                   int(over_y), int(over_x), _stream()), "stroke_gather")
    return canvas


def stroke_paste(dec, mask, texture, xs, ys, modes=None, wrap=False):
    """dtp_op_stroke_paste, the paste kernel of dtp_stroke on its own: dec f32 [B,R,R,4] (the VAE decoder's working layout; None when
    every window is an Erase window), mask u8 [R,R], texture u8 [H,W,4] written in place where the mask is > 0.  Returns texture."""
    lib = _lib.load()
    B, ax, ay, am = _windows(xs, ys, modes)
    check(lib.dtp_op_stroke_paste(ptr(dec), ptr(mask), ptr(texture), texture.shape[0], texture.shape[1], mask.shape[0], B, ax, ay, am,
                                  int(bool(wrap)), _stream()), "stroke_paste")
    return texture


def mesh_render(mesh, camera, fov, texture, R, flip_normals=False, mode=0, over_y=0, over_x=0):
    """dtp_op_mesh_render, the render half of a dtp_mesh_stroke stamp on its own: mesh a mesh.Mesh, camera the [3, 4] matrix of
    mesh_camera, texture u8 [H,W,4] (device) -> (canvas f32 [1,4,R,R], face_idx i32 [R,R]).  The mesh keeps the projection for
    mesh_backproject."""
    lib = _lib.load()
    cam = (C.c_float * 12)(*[float(v) for v in torch.as_tensor(camera).reshape(-1).tolist()])
    canvas = torch.empty(1, 4, R, R, dtype=torch.float32, device=texture.device)
    face_idx = torch.empty(R, R, dtype=torch.int32, device=texture.device)
    check(lib.dtp_op_mesh_render(mesh.handle, C.byref(cam), C.c_float(float(fov)), int(bool(flip_normals)), ptr(texture), texture.shape[0],
                                 texture.shape[1], int(R), int(mode), int(over_y), int(over_x), ptr(canvas), ptr(face_idx), _stream()),
          "mesh_render")
    return canvas, face_idx


def mesh_backproject(mesh, dec, mask, face_idx, texture, painted=None, face_mask=None, fov=None, occlude=None):
    """dtp_op_mesh_backproject, the other half: through the faces the LAST mesh_render of `mesh` showed (face_idx: that render's), the
    stamp image is carried into texture u8 [H,W,4] in place where the sampled mask u8 [R,R] * (face_idx != -1) is > 0.  The stamp image
    is dec f32 [R,R,4] (the VAE decoder's working layout, values around -1..1), or `painted` f32 [3,R,R] / [1,3,R,R] in 0..1 (what
    generate_raw returns, used as it is); neither: erase.  face_mask: a face set (int32 [(F + 31) // 32] on the texture's device,
    contiguous; dtp_op_mesh_backproject_masked): a face whose bit is 0 is not backprojected.  occlude: the per-texel occlusion test
    (dtp_op_mesh_backproject_occluded; True: 1.0, a float >= 0: the tolerance in stamp pixels, None or False: off); it needs fov, the fov
    of that render.  Returns texture."""
    lib = _lib.load()
    from . import mesh as _mesh
    occlude = _mesh.occlude_arg(occlude)
    if occlude is not None and fov is None:
        raise ValueError("occlude needs fov, the fov of the render whose face_idx this is")
    if face_mask is not None:
        _mesh.faceset_check(face_mask, mesh.num_faces, texture.device)
    finished = painted is not None
    if finished:
        if dec is not None:
            raise ValueError("dec and painted are exclusive")
        R = face_idx.shape[0]
        dec = torch.zeros(R, R, 4, dtype=torch.float32, device=texture.device)
        dec[..., :3] = painted.reshape(3, R, R).permute(1, 2, 0)
    if occlude is not None:
        check(lib.dtp_op_mesh_backproject_occluded(mesh.handle, ptr(dec), int(finished), ptr(mask), ptr(face_idx), face_idx.shape[0], ptr(texture),
                                                   texture.shape[0], texture.shape[1], ptr(face_mask),
                                                   0 if face_mask is None else face_mask.shape[0], C.c_float(float(fov)), C.c_float(occlude),
                                                   _stream()), "mesh_backproject_occluded")
        return texture
    if face_mask is not None:
        check(lib.dtp_op_mesh_backproject_masked(mesh.handle, ptr(dec), int(finished), ptr(mask), ptr(face_idx), face_idx.shape[0], ptr(texture),
                                                 texture.shape[0], texture.shape[1], ptr(face_mask), face_mask.shape[0], _stream()),
              "mesh_backproject_masked")
        return texture
    check(lib.dtp_op_mesh_backproject(mesh.handle, ptr(dec), int(finished), ptr(mask), ptr(face_idx), face_idx.shape[0], ptr(texture),
                                      texture.shape[0], texture.shape[1], _stream()), "mesh_backproject")
    return texture


def mesh_coverage(mesh, H, W):
    """dtp_op_mesh_coverage: the texels of an H x W texture whose centre at least one of all faces of `mesh` (a mesh.Mesh) covers in
    texture space, by the backprojection's integer rule -> bool [H, W] on the mesh's device.  The first call for a size builds the mask the
    bleed pass uses."""
    lib = _lib.load()
    out = torch.empty(int(H), int(W), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
    check(lib.dtp_op_mesh_coverage(mesh.handle, int(H), int(W), ptr(out), _stream()), "mesh_coverage")
    return out.bool()


def mesh_pick(mesh, origins, directions):
    """dtp_op_mesh_pick: the closest hit of n rays on `mesh` (a mesh.Mesh) with the records left on the device -> the dict of
    MI355ConditionalInpainter.pick, as tensors on the current device.  On the current stream, which it waits for."""
    from . import mesh as _mesh
    lib = _lib.load()
    rays, n = _mesh.rays(origins, directions)
    rec = torch.zeros(n, _mesh.HIT_WORDS, dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
    check(lib.dtp_op_mesh_pick(mesh.handle, C.cast(rays.data_ptr(), C.POINTER(_lib.Ray)), n, ptr(rec), _stream()), "mesh_pick")
    return _mesh.hits_dict(rec)


def faceset_extend(mesh, sel, how, rings=1, out=None):
    """dtp_mesh_select_extend, the bare call on the current stream: the face set `sel` of `mesh` (a mesh.Mesh) grown by how = "rings",
    "shrink", "linked" or "charts" (MI355ConditionalInpainter.extend_selection has the rules) -> out, default a fresh set; out=sel works in
    place.  Only the mesh's first use waits (it builds the topology)."""
    from . import mesh as _mesh
    if how not in _lib.EXTEND_HOWS:
        raise ValueError(f"how {how!r}: choose one of {', '.join(_lib.EXTEND_HOWS)}")
    _mesh.faceset_check(sel, mesh.num_faces, sel.device if isinstance(sel, torch.Tensor) else "cpu", what="sel")
    if out is None:
        out = torch.empty_like(sel)
    else:
        _mesh.faceset_check(out, mesh.num_faces, sel.device, what="out")
    check(_lib.load().dtp_mesh_select_extend(mesh.handle, ptr(sel), ptr(out), sel.shape[0], _lib.EXTEND_HOWS[how], int(rings), _stream()),
          "dtp_mesh_select_extend")
    return out


def mesh_view(mesh, texture, camera, size=None, binned=True, want_face_idx=True, want_depth=True, clip_near=False, filter="bilinear", mips=None,
              want_lod=False, samples=1, want_coverage=False, anisotropy=None, want_taps=False, **opts):
    """dtp_op_mesh_view: the frame of MI355ConditionalInpainter.render_view on the current stream -> (image u8 [H,W,4], face_idx i32
    [H,W] or None, depth f32 [H,W] or None).  binned=False puts every drawn face on the list that every tile streams (the arm a
    measurement compares the bins with); the frame is the same bytes.  opts: cull, flip_normals, shade, ambient, unpainted, background.
    clip_near=True (dtp_op_mesh_view_clip): the faces across the camera's near plane are drawn too, down to the plane; binned=False
    then also gives each of them the whole frame as its pixel range.  With it, filter="trilinear" takes mips (the pyramid of
    build_mips / ops.texture_mips) and want_lod appends lod f32 [H,W] to the tuple.
    samples in (2, 4) (dtp_op_mesh_view_aa): samples x samples centres per pixel, averaged (render_view has the rule); filter="trilinear"
    then needs no clip_near.  want_coverage (any samples) appends coverage u8 [H,W], the number of the pixel's samples a face covers, last.
    samples=1 without want_coverage is the call it always was.
    anisotropy in 1..16 (dtp_op_mesh_view_aniso; needs filter="trilinear" and mips): up to that many trilinear taps along the longer axis
    of the footprint, the level from the shorter one (render_view has the rule), with clip_near, samples and binned as above; 1 runs that
    entry too and gives the trilinear frame.  want_taps appends taps u8 [H,W], the number of taps per pixel, after lod and before
    coverage.  None is today's routing."""
    from . import mesh as _mesh
    lib = _lib.load()
    H, W = (int(v) for v in (camera.size if size is None else size))
    if not (1 <= H <= _lib.VIEW_MAX and 1 <= W <= _lib.VIEW_MAX):
        raise ValueError(f"size = ({H}, {W}): each side 1..{_lib.VIEW_MAX}")
    if filter not in ("bilinear", "trilinear"):
        raise ValueError(f"filter {filter!r}: choose 'bilinear' or 'trilinear'")
    samples = _lib.view_samples_check(samples, H, W)
    if anisotropy is None and want_taps:
        raise ValueError("want_taps needs anisotropy (an integer in 1..16)")
    if anisotropy is not None:
        anisotropy = _lib.view_anisotropy_check(anisotropy, filter, want_taps, least=1)
    aa = samples > 1 or bool(want_coverage)
    if not clip_near and not aa and anisotropy is None and (filter != "bilinear" or mips is not None or want_lod):
        raise ValueError("filter, mips and want_lod need clip_near=True or samples > 1 here (render_view(filter='trilinear') is the unclipped "
                         "filtered frame)")
    if aa and filter == "bilinear" and (mips is not None or want_lod):
        raise ValueError("mips and want_lod need filter='trilinear'")
    o, cam = _mesh.view_opts(**opts), camera.struct()
    image = torch.empty(H, W, 4, dtype=torch.uint8, device=texture.device)
    face_idx = torch.empty(H, W, dtype=torch.int32, device=texture.device) if want_face_idx else None
    depth = torch.empty(H, W, dtype=torch.float32, device=texture.device) if want_depth else None
    if anisotropy is not None:
        lod = torch.empty(H, W, dtype=torch.float32, device=texture.device) if want_lod else None
        taps = torch.empty(H, W, dtype=torch.uint8, device=texture.device) if want_taps else None
        coverage = torch.empty(H, W, dtype=torch.uint8, device=texture.device) if want_coverage else None
        check(lib.dtp_op_mesh_view_aniso(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips), C.byref(cam), H, W, C.byref(o),
                                         int(bool(clip_near)), samples, anisotropy, ptr(image), ptr(face_idx), ptr(depth), ptr(lod), ptr(taps),
                                         ptr(coverage), int(bool(binned)), _stream()), "mesh_view_aniso")
        return (image, face_idx, depth) + ((lod,) if want_lod else ()) + ((taps,) if want_taps else ()) + ((coverage,) if want_coverage else ())
    if aa:
        lod = torch.empty(H, W, dtype=torch.float32, device=texture.device) if want_lod else None
        coverage = torch.empty(H, W, dtype=torch.uint8, device=texture.device) if want_coverage else None
        check(lib.dtp_op_mesh_view_aa(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips), C.byref(cam), H, W, C.byref(o),
                                      int(filter == "trilinear"), int(bool(clip_near)), samples, ptr(image), ptr(face_idx), ptr(depth), ptr(lod),
                                      ptr(coverage), int(bool(binned)), _stream()), "mesh_view_aa")
        return (image, face_idx, depth) + ((lod,) if want_lod else ()) + ((coverage,) if want_coverage else ())
    if not clip_near:
        check(lib.dtp_op_mesh_view(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], C.byref(cam), H, W, C.byref(o), ptr(image),
                                   ptr(face_idx), ptr(depth), int(bool(binned)), _stream()), "mesh_view")
        return image, face_idx, depth
    lod = torch.empty(H, W, dtype=torch.float32, device=texture.device) if want_lod else None
    check(lib.dtp_op_mesh_view_clip(mesh.handle, ptr(texture), texture.shape[0], texture.shape[1], ptr(mips), C.byref(cam), H, W, C.byref(o),
                                    int(filter == "trilinear"), ptr(image), ptr(face_idx), ptr(depth), ptr(lod), int(bool(binned)), _stream()),
          "mesh_view_clip")
    return (image, face_idx, depth, lod) if want_lod else (image, face_idx, depth)


def mip_layout(TH, TW):
    """dtp_mip_layout (host only, needs no GPU): where the levels of the mip pyramid of a TH x TW texture lie -> dict(levels, h, w,
    offset, bytes): h, w, offset lists of `levels` entries (level 0 is the texture itself, offset[0] = 0 and unused; offset[1] = 0),
    bytes the size of the buffer of levels 1 .. levels - 1 (MI355ConditionalInpainter.build_mips)."""
    lay = _lib.MipLevels()
    check(_lib.load().dtp_mip_layout(int(TH), int(TW), C.byref(lay)), "dtp_mip_layout")
    n = lay.levels
    return dict(levels=n, h=list(lay.h)[:n], w=list(lay.w)[:n], offset=list(lay.offset)[:n], bytes=int(lay.bytes))


def mesh_bleed_offsets(k):
    """dtp_mesh_bleed_offsets (host only, needs no GPU): the candidate offsets (di, dj) of a gutter texel's source at radius k in 1..16,
    sorted by (di^2 + dj^2, di, dj) -> int8 [n, 2].  The table of a smaller radius is a prefix of it."""
    lib = _lib.load()
    n = C.c_int(0)
    check(lib.dtp_mesh_bleed_offsets(int(k), C.byref(n), None), "mesh_bleed_offsets")
    buf = (C.c_byte * (2 * n.value))()
    check(lib.dtp_mesh_bleed_offsets(int(k), C.byref(n), buf), "mesh_bleed_offsets")
    return torch.tensor(list(buf), dtype=torch.int8).reshape(n.value, 2)


def journal_window_tiles(H, W, R, x, y, wrap=False):
    """dtp_journal_window_tiles (host only, needs no GPU): the ascending indices of the 16 x 16-texel tiles that an open journal record
    saves for ONE 2D stroke window at (x, y) of an H x W texture: every tile that meets the R x R window clipped to the texture, or with
    wrap a wrapped piece of it.  -> list of int, tile t = (row / 16) * ceil(W / 16) + col / 16."""
    from . import journal
    return journal.window_tiles(H, W, R, x, y, wrap=wrap)


def delta_layout(H, W, capacity_tiles=None):
    """dtp_delta_layout (host only, needs no GPU): what a changed-tile tracker of an H x W image with `capacity_tiles` (default: its tile
    count) owns -> dict(tiles_x, tiles_y, n_tiles, n_groups, capacity, and the byte sizes shadow_bytes, stale_bytes, flag_bytes,
    group_bytes, ids_bytes, tiles_bytes, counts_bytes, host_ids_offset, host_tiles_offset, host_bytes)."""
    from . import journal
    if capacity_tiles is None:
        capacity_tiles = journal.tile_count(H, W)
    lay = _lib.DeltaSizes()
    check(_lib.load().dtp_delta_layout(int(H), int(W), int(capacity_tiles), C.byref(lay)), "dtp_delta_layout")
    return {name: int(getattr(lay, name)) for name, _ in _lib.DeltaSizes._fields_}


def delta_scan(tracker, image):
    """dtp_delta_scan of `image` (u8 [H,W,4]) with a delta.DeltaTracker on the current stream, and the tracker's state afterwards, for the
    kernel tests -> (ids i32 [emitted], tiles u8 [emitted,16,16,4], counts [emitted, remaining], shadow u8 [H,W,4], stale u8 [n_tiles]),
    CPU tensors; ids and tiles are copies of the first `emitted` device slots."""
    from . import journal
    lib = _lib.load()
    m = tracker._model
    check(lib.dtp_delta_scan(m._h, tracker.handle, ptr(image), image.shape[0], image.shape[1], _stream()), "dtp_delta_scan")
    ids, tiles, counts = tracker._device_views()
    counts = counts.cpu().tolist()
    shadow = torch.empty(tracker.H, tracker.W, 4, dtype=torch.uint8)
    stale = torch.empty(journal.tile_count(tracker.H, tracker.W), dtype=torch.uint8)
    check(lib.dtp_op_delta_state(tracker.handle, ptr(shadow), ptr(stale), _stream()), "dtp_op_delta_state")
    return ids[:counts[0]].cpu(), tiles[:counts[0]].cpu(), counts, shadow, stale

