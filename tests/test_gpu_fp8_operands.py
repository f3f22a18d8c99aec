"""Option fp8_operands: e4m3 activations in memory for the K = 1280 transformer Linears (q/k/v, to_out, FF1 of the C = 1280 blocks).

(1) the quantise pass (dtp_op_quant_e4m3) against torch.float8_e4m3fn (round to nearest even; the kernel saturates at +-448, so the
    reference is clamped first); (2) the two-operand e4m3 GEMM (dtp_op_gemm_f8f8) against fp32 on the e4m3-rounded operands and against
    exact fp32, with every epilogue; (3) the option routes q/k/v, to_out and FF1 at K = 1280 and only when asked; (4) whole stamps against
    the fp32 CPU oracle (64^2) and against the fp16 path (256^2).
"""
import csv
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PIXEL_TOL = 1e-2  # the fp8 stamp gate of tests/test_gpu_fullsize.py (FP8_FULL_PIXEL_TOL), restated


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def e4_bytes(t, scale):
    """what the kernels write: e4m3(t / scale), saturated at +-448, as bytes"""
    return (t.double() / scale).clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)


def dq(b, scale=1.0):
    return b.view(torch.float8_e4m3fn).float() * scale


def ordinal(b):
    """e4m3 codes on one integer line (neighbouring values differ by 1; +0 and -0 are both 0)"""
    b = b.to(torch.int32)
    mag = b & 0x7F
    return torch.where(b & 0x80 != 0, -mag, mag)


def pow2_scale(t):
    return 2.0 ** math.ceil(math.log2(t.float().abs().max().item() * 2.0 / 448.0))


def close(got, ref, tol):
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    lim = tol * ref.abs().max().item() + tol
    assert err <= lim, f"max err {err} > {lim}"


# ---------------------------------------------------------------- (1) quantise pass
@pytest.mark.parametrize("m,k", [(96, 1280), (1001, 640), (37, 5120)])
def test_quant_raw_bit_exact(ops, m, k):
    x = rnd(m, k, seed=1, scale=3.0)
    x[0, :8] = torch.tensor([1e4, -1e4, 500.0, -449.0, 1e-4, -3e-3, 0.0, 2.0 ** -12]).half()  # saturation, subnormals, zero
    s = 0.5
    got = ops.quant_e4m3(x.cuda(), s)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), e4_bytes(x, s))


def _stats_parts(x, parts):
    """per-row (sum, sumsq) partials the way a GF_ROWSTATS producer leaves them: [parts][M][2], column ranges summed in fp32"""
    chunks = x.float().chunk(parts, dim=1)
    return torch.stack([torch.stack([c.sum(1), (c * c).sum(1)], dim=1) for c in chunks])


@pytest.mark.parametrize("with_stats", [True, False])
def test_quant_layernorm_and_dual_copy(ops, with_stats):
    m, k = 777, 1280
    x = rnd(m, k, seed=2).float()
    x[::3] = x[::3] * 0.5 + 8.0 * 0.5  # |mean| = 8 sigma on every third row
    x[1::3] = x[1::3] * 2.0 - 5.0
    x = x.half()
    st = _stats_parts(x, 10) if with_stats else None
    s_ln, s_raw = 0.125, pow2_scale(x)
    raw, ln = ops.quant_e4m3(x.cuda(), s_raw, x2=x.cuda(), scale2=s_ln, ln2=True, stats_in=st.cuda() if st is not None else None)
    torch.cuda.synchronize()
    assert torch.equal(raw.cpu(), e4_bytes(x, s_raw))  # the raw copy of the dual launch: bit-exact
    xd = x.double()
    xn = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
    d = (ordinal(ln.cpu()) - ordinal(e4_bytes(xn, s_ln))).abs()
    assert d.max().item() <= 1, d.max().item()  # within one e4m3 ulp of the fp64 normalised value
    assert (d > 0).float().mean().item() < 0.01  # ... and almost always the same code


# ---------------------------------------------------------------- (2) two-operand GEMM
GEMM_SHAPES = [(96, 1280, 1280, 0, -1), (96, 1280, 1280, 0, 0), (6144, 1280, 1280, 0, -1), (1536, 1280, 5120, 1280, -1),
               (24576, 640, 2560, 640, -1), (300, 640, 2560, 640, 1),
               (200, 320, 320, 0, 0), (130, 320, 208, 112, 1)]  # N % 128 == 64 (half-empty last tile); K and the A2 boundary off the k-block grid


@pytest.mark.parametrize("m,n,k1,k2,tile", GEMM_SHAPES)
def test_gemm_f8f8_bias_resid_stats_e4m3_out(ops, m, n, k1, k2, tile):
    dev = "cuda"
    k = k1 + k2
    a = rnd(m, k, seed=10, scale=2.0)
    w = rnd(n, k, seed=11, scale=k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(12))
    r = rnd(m, n, seed=13)
    sa = pow2_scale(a)
    a8 = e4_bytes(a.to(dev), sa)
    wp = ops.pack_linear(w.float().to(dev))
    w8, ws = ops.quantize_w8(wp, k)
    cs = 2.0 ** -4
    tail = a8[:, k1:] if k2 else None
    got, got8, st = ops.gemm_f8f8(a8[:, :k1] if k2 else a8, w8, n, sa, ws, k=k1, bias=bias.to(dev), resid=r.to(dev), tail8=tail,
                                  tile=tile, row_stats=True, out8_scale=cs)
    torch.cuda.synchronize()
    # the same contraction on the e4m3-rounded operands (products exact in fp32: only the summation order differs)
    ref8 = F.linear(dq(a8, sa), dq(w8[:n, :k].contiguous(), ws), bias.to(dev)) + r.to(dev).float()
    close(got, ref8, 2e-3)
    ref = F.linear(a.float().to(dev), w.float().to(dev), bias.to(dev)) + r.to(dev).float()
    assert (got.float() - ref).abs().max().item() <= 6e-2 * ref.abs().max().item()
    assert torch.equal(got8, e4_bytes(got, cs))  # e4m3 output = the quantised fp16 output
    if tile >= 0:  # (the small cases) ... and the same bytes when it is the only output
        only8 = ops.gemm_f8f8(a8[:, :k1] if k2 else a8, w8, n, sa, ws, k=k1, bias=bias.to(dev), resid=r.to(dev), tail8=tail, tile=tile,
                              out8_scale=cs, out16=False)[1]
        assert torch.equal(only8, got8)
    tot = st.sum(dim=0)
    g = got.float()
    assert torch.allclose(tot[:, 0], g.sum(1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[:, 1], (g * g).sum(1), rtol=1e-4, atol=1e-2)


def _geglu_pack(c, w, bias):
    f = torch.arange(4 * c)
    perm = torch.empty(8 * c, dtype=torch.long)
    perm[f] = (f // 64) * 128 + f % 64
    perm[4 * c + f] = (f // 64) * 128 + 64 + f % 64
    bp = torch.empty_like(bias)
    bp[perm] = bias
    return bp


@pytest.mark.parametrize("m,tile", [(6144, -1), (96, 0), (333, 1)])
def test_gemm_f8f8_geglu_e4m3_out(ops, m, tile):
    from diffusiontexturepainting_amd._lib import GF_GEGLU
    dev = "cuda"
    c = 1280
    a = rnd(m, c, seed=20)
    w = rnd(8 * c, c, seed=21, scale=c ** -0.5)
    bias = 0.1 * torch.randn(8 * c, generator=torch.Generator().manual_seed(22))
    sa = 0.125
    a8 = e4_bytes(a.to(dev), sa)
    wp = ops.pack_linear(w.float().to(dev), geglu=True)
    w8, ws = ops.quantize_w8(wp, c)
    cs = 2.0 ** -6
    got, got8, _ = ops.gemm_f8f8(a8, w8, 8 * c, sa, ws, bias=_geglu_pack(c, w, bias).to(dev), flags=GF_GEGLU, tile=tile, out8_scale=cs)
    only8 = ops.gemm_f8f8(a8, w8, 8 * c, sa, ws, bias=_geglu_pack(c, w, bias).to(dev), flags=GF_GEGLU, tile=tile, out8_scale=cs, out16=False)[1]
    torch.cuda.synchronize()
    h8 = F.linear(dq(a8, sa), dq(e4_bytes(w, ws), ws).to(dev), bias.to(dev))  # per-tensor scale: the packing does not change it
    a_, g_ = h8.chunk(2, dim=-1)
    close(got, a_ * F.gelu(g_), 2e-3)
    h = F.linear(a.float().to(dev), w.float().to(dev), bias.to(dev))
    ref = h[:, :4 * c] * F.gelu(h[:, 4 * c:])
    assert (got.float() - ref).abs().max().item() <= 6e-2 * ref.abs().max().item()
    assert torch.equal(got8, e4_bytes(got, cs))
    assert torch.equal(only8, got8)  # the e4m3-only output (FF1 in the engine) is the same bytes


def test_gemm_f8f8_rejects_what_it_cannot_do(ops):
    from diffusiontexturepainting_amd import _lib
    a8 = torch.zeros(64, 1280, dtype=torch.uint8, device="cuda")
    w8 = torch.zeros(128, 1280, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.DtpError):
        ops.gemm_f8f8(a8, w8, 96, 1.0, 1.0)  # N % 64 != 0
    with pytest.raises(_lib.DtpError):
        ops.gemm_f8f8(a8, w8, 128, 1.0, 1.0, tile=2)


def test_quant_keeps_nan_and_rejects_non_power_of_two_scales(ops):
    from diffusiontexturepainting_amd import _lib
    x = rnd(4, 64, seed=3)
    x[1, 5] = float("nan")
    got = ops.quant_e4m3(x.cuda(), 1.0)
    torch.cuda.synchronize()
    assert torch.isnan(dq(got.cpu()))[1, 5] and torch.isfinite(dq(got.cpu())).sum() == 4 * 64 - 1  # NaN stays NaN, not -448
    with pytest.raises(_lib.DtpError):
        ops.quant_e4m3(x.cuda(), 0.3)


@pytest.mark.parametrize("mfast", [False, True])
def test_gemm_f8f8_tail_with_its_own_scale(ops, mfast):
    """[f | y3] with different calibrated scales: the A2 columns' scale enters as the MFMA's E8M0 block scale (ratio 2^7 here: a
    GEGLU-sized part next to a residual-stream-sized one); GF_MFAST (tile_m fastest) gives the same bytes"""
    from diffusiontexturepainting_amd import _lib
    dev = "cuda"
    m, n, k1, k2 = 300, 640, 2560, 640
    f = rnd(m, k1, seed=30, scale=0.05).to(dev)
    y3 = rnd(m, k2, seed=31, scale=30.0).to(dev)
    w = rnd(n, k1 + k2, seed=32, scale=(k1 + k2) ** -0.5)
    sf, sy = pow2_scale(f), pow2_scale(y3)
    assert sy / sf >= 2 ** 7
    f8, y8 = e4_bytes(f, sf), e4_bytes(y3, sy)
    wp = ops.pack_linear(w.float().to(dev))
    w8, ws = ops.quantize_w8(wp, k1 + k2)
    got = ops.gemm_f8f8(f8, w8, n, sf, ws, tail8=y8, tail_scale=sy, flags=(1 << 20) if mfast else 0)[0]
    torch.cuda.synchronize()
    ref8 = F.linear(torch.cat([dq(f8, sf), dq(y8, sy)], dim=1), dq(w8[:n, :k1 + k2].contiguous(), ws))
    close(got, ref8, 2e-3)
    ref = F.linear(torch.cat([f.float(), y3.float()], dim=1), w.float().to(dev))
    assert (got.float() - ref).abs().max().item() <= 6e-2 * ref.abs().max().item()
    with pytest.raises(_lib.DtpError):  # a ratio needs whole k-blocks of A2
        ops.gemm_f8f8(f8[:, :2496], w8, n, sf, ws, tail8=y8, tail_scale=sy)
    with pytest.raises(_lib.DtpError):
        ops.gemm_f8f8(f8, w8, n, 0.3, ws)


# ---------------------------------------------------------------- (3) + (4) the engine option
def _inputs(b, res, seed):
    from diffusiontexturepainting_amd import synthetic
    canvas, brush, lat, eps = synthetic.make_stamp_batch(b, res, seed)
    cond, uncond = synthetic.make_conditioning(seed + 1)
    return canvas, brush, cond, uncond, lat, eps


@pytest.fixture(scope="module")
def w64():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    from oracle import nets
    sd = dict(unet=W.synthetic_unet(2), lora=W.synthetic_lora(2), vae=W.synthetic_vae(2))
    return sd, dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"])


ST64 = dict(steps=8, context_pad=5, tg_steps=4, cfg_weight=2.0, tg_weight=1.0)  # tg cut-off mid-loop: both programs are built and calibrated


@pytest.fixture(scope="module")
def stamp64(w64):
    """batch 8, 64^2, 8 steps: fp8_operands (and fp8_operands + fp8_attention) against the fp32 oracle"""
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from oracle import pipeline
    canvas, brush, cond, uncond, lat, eps = _inputs(8, 64, 31)
    ref = pipeline.generate_raw(w64[1], brush, cond, uncond, canvas, lat, eps, **ST64)
    out, models = {}, {}
    for name, kw in (("operands", dict(fp8_operands=True)), ("attention+operands", dict(fp8_operands=True, fp8_attention=True))):
        m = MI355ConditionalInpainter(64, device=0, weights=w64[0], max_batch=8, **kw)
        m.set_conditioning(cond, uncond, brush)
        out[name] = m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST64).cpu()
        torch.cuda.synchronize()
        models[name] = m
    return dict(ref=ref, out=out, models=models, inputs=(canvas, brush, cond, uncond, lat, eps))


def test_stamp64_batch8_matches_oracle(stamp64):
    ref = stamp64["ref"]
    for name, got in stamp64["out"].items():
        per_stamp = [(got[i] - ref[i]).abs().max().item() for i in range(got.shape[0])]
        print(f"64^2 x 8, 8 steps, fp8 {name}: max abs pixel error per stamp {['%.2e' % e for e in per_stamp]}")
        assert torch.isfinite(got).all()
        assert max(per_stamp) <= PIXEL_TOL, (name, max(per_stamp))


def _profile_one_stamp(m, inputs, tmp_path, tag):
    canvas, brush, cond, uncond, lat, eps = inputs
    m.profile(1)
    try:
        m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST64)
        torch.cuda.synchronize()
        rows = {r["kernel"]: r["launches"] for r in m.profile_rows()}
        path = tmp_path / f"prof_{tag}.csv"
        m.profile_dump(path)
    finally:
        m.profile(0)
    with open(path) as fh:
        labels = [r[-1] for r in csv.reader(fh) if r and r[0].isdigit()]
    return rows, labels, m.stamp_info()["unet_evals"]


def test_option_routes_the_k1280_linears(stamp64, tmp_path):
    from diffusiontexturepainting_amd import _lib
    m = stamp64["models"]["operands"]
    rows, labels, evals = _profile_one_stamp(m, stamp64["inputs"], tmp_path, "on")
    f8 = [lb for lb in labels if lb.startswith("f8f8 ")]
    q8 = [lb for lb in labels if lb.startswith("quant8 ")]
    assert rows.get(_lib.PROF_KINDS[53], 0) == len(f8) > 0 and rows.get(_lib.PROF_KINDS[54], 0) == len(q8) > 0
    # per evaluation: q/k/v (LN1), to_out and FF1 (LN3, GEGLU) of the six C = 1280 blocks, each behind one quantise pass.  Every other
    # Linear stays fp16: K < 1280, proj_in (GroupNorm'd input), and the merged FF2 | proj_out, whose A2 operand is the residual stream
    assert len(f8) == 6 * 3 * evals, (len(f8), evals)
    assert len(q8) == 6 * 3 * evals
    assert {int(lb.split("K=")[1].split()[0]) for lb in f8} == {1280}
    assert rows.get("gemm_fp8_kernel", 0) == 0 and not any(" fp8" in lb for lb in labels if lb.startswith("gemm "))
    lib = _lib.load()  # the option is fixed once a UNet program exists
    assert lib.dtp_set_option(m._h, b"fp8_operands", 0) == 3  # DTP_ERR_STATE
    assert lib.dtp_set_option(m._h, b"fp8_operands", 1) == 0  # (the value it has: accepted)


def test_option_off_never_launches_the_new_kernels(w64, stamp64, tmp_path):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    m = MI355ConditionalInpainter(64, device=0, weights=w64[0], max_batch=8, fp8_operands=False)
    canvas, brush, cond, uncond, lat, eps = stamp64["inputs"]
    m.set_conditioning(cond, uncond, brush)
    rows, labels, evals = _profile_one_stamp(m, stamp64["inputs"], tmp_path, "off")
    assert evals > 0
    assert rows.get(_lib.PROF_KINDS[53], 0) == 0 and rows.get(_lib.PROF_KINDS[54], 0) == 0
    assert not any(lb.startswith(("f8f8 ", "quant8 ")) for lb in labels)


def test_stamp256_batch8_operands_vs_fp16():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    sd = dict(unet=W.synthetic_unet(7), lora=W.synthetic_lora(7), vae=W.synthetic_vae(7))
    canvas, brush, cond, uncond, lat, eps = _inputs(8, 256, 410)
    st = dict(steps=8, context_pad=150, tg_steps=8, cfg_weight=2.0, tg_weight=1.0)
    out = {}
    for on in (False, True):
        m = MI355ConditionalInpainter(256, device=0, weights=sd, max_batch=8, fp8_operands=on)
        m.set_conditioning(cond, uncond, brush)
        out[on] = m.generate_raw(canvas, latents=lat, vae_eps=eps, **st).cpu()
        torch.cuda.synchronize()
        del m
    err = (out[True] - out[False]).abs().max().item()
    print(f"256^2 x 8, 8 steps: max |fp8_operands - fp16| = {err:.2e}")
    assert torch.isfinite(out[True]).all() and 0 < err <= PIXEL_TOL
