"""Kernel-level parity: every HIP kernel shape class vs a plain torch fp32
CPU reference of the same op, called through the C ABI (dtp_op_*).  Inputs are fp16-rounded
so the only differences are fp32-accumulation order and the fp16 rounding of the output.

Tolerance: |err| <= 2e-3 * max|ref| + 2e-3 (fp16 has 2^-11 relative precision; K up to 11520)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def needs_experimental_build(ops):
    """skip unless libdtp.so was built with DTP_EXPERIMENTAL=1 (the default build answers 0 packed elements for the tile-55 packing)"""
    from diffusiontexturepainting_amd import _lib
    if _lib.load().dtp_op_pack_linear_ws_elems(64, 64) == 0:
        pytest.skip("experiment not in this build (DTP_EXPERIMENTAL=1 python -m diffusiontexturepainting_amd.build)")


def close(got, ref, tol=2e-3):
    got = got.float().cpu()
    ref = ref.float()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    lim = tol * ref.abs().max().item() + tol
    assert err <= lim, f"max err {err} > {lim}"


GEMM_SHAPES = [(300, 320, 320), (4096, 640, 1280), (192, 1280, 2560), (77, 768, 768), (14, 1280, 768)]
GEMM_TILES = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47]  # shape + 4 * (stages - 2); 16.. = 256-wide tiles; 20 / 21 = 8-wave wide tiles; 32.. = 8-wave (k-split) twins of 0..7; 40.. = loader-wave variants (4 / 8 DMA-only waves)
# round 6: every tile id still runs, the heuristic (-1) on all five shapes, an explicit tile on THREE of them -- always the large one (every
# pipeline stage in steady state) and two of the four ragged ones, rotating with the tile's position (the full 35 x 5 cross-product was a
# minute of the driver's GPU leg re-checking the same code paths)
GEMM_CASES = [(m, n, k, t) for i, t in enumerate(GEMM_TILES) for j, (m, n, k) in enumerate(GEMM_SHAPES)
              if t == -1 or j == 1 or j == (0, 2, 3, 4)[i % 4] or j == (2, 3, 4, 0)[(i // 4) % 4]]


@pytest.mark.parametrize("m,n,k,tile", GEMM_CASES)
def test_gemm_dense(ops, m, n, k, tile):
    a, w = rnd(m, k, seed=1), rnd(n, k, seed=2, scale=k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(3))
    r = rnd(m, n, seed=4)
    ref = F.linear(a.float(), w.float(), bias) + r.float()
    wp = ops.pack_linear(w.float().cuda())
    got = ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), resid=r.cuda(), tile=tile)
    close(got, ref)


@pytest.mark.parametrize("tile", [-1, 34, 36, 42, 47])
@pytest.mark.parametrize("splits", [2, 5, 16])
def test_gemm_splitk(ops, splits, tile):
    m, n, k = 192, 1280, 11520
    a, w = rnd(m, k, seed=5), rnd(n, k, seed=6, scale=k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(7))
    ref = F.linear(a.float(), w.float(), bias)
    wp = ops.pack_linear(w.float().cuda())
    got = ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), splits=splits, tile=tile)
    close(got, ref)
    got2 = ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda())  # heuristic split
    close(got2, ref)


def test_gemm_asymmetric_identity(ops):
    """A = I against an asymmetric W catches operand / output transposes."""
    n = k = 128
    a = torch.eye(k).half()
    w = (torch.arange(n * k).reshape(n, k).float() % 251 - 125).half() / 64
    wp = ops.pack_linear(w.float().cuda())
    got = ops.gemm(a.cuda(), wp, n, k)
    close(got, w.float().t(), tol=1e-6)


@pytest.mark.parametrize("m,c,tile", [(512, 320, -1), (100, 1280, -1), (700, 320, 20), (300, 640, 20), (512, 320, 32), (100, 1280, 39), (300, 640, 36), (512, 320, 40), (100, 1280, 47)])
def test_gemm_geglu(ops, m, c, tile):
    a, w = rnd(m, c, seed=8), rnd(8 * c, c, seed=9, scale=c ** -0.5)
    bias = torch.randn(8 * c, generator=torch.Generator().manual_seed(10)) * 0.1
    h = F.linear(a.float(), w.float(), bias)
    x, gate = h.chunk(2, dim=-1)
    ref = x * F.gelu(gate)
    wp = ops.pack_linear(w.float().cuda(), geglu=True)
    # the bias follows the same [a|gate] row packing as the weights
    f = torch.arange(4 * c)
    perm = torch.empty(8 * c, dtype=torch.long)
    perm[f] = (f // 64) * 128 + f % 64
    perm[4 * c + f] = (f // 64) * 128 + 64 + f % 64
    bp = torch.empty_like(bias)
    bp[perm] = bias
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    got = ops.gemm(a.cuda(), wp, 8 * c, c, bias=bp.cuda(), flags=GF_GEGLU | GF_BIAS, tile=tile)
    close(got, ref)


@pytest.mark.parametrize("m,c,n,tile,geglu", [(300, 320, 960, -1, False), (100, 1280, 1280, 6, False), (513, 640, 5120, -1, True),
                                             (64, 768, 768, 3, False), (513, 640, 5120, 17, True), (300, 320, 960, 18, False),
                                             (513, 640, 5120, 20, True), (300, 320, 960, 21, False), (700, 320, 960, 20, False),
                                             (300, 320, 960, 34, False), (513, 640, 5120, 32, True), (64, 768, 768, 39, False), (100, 1280, 1280, 37, False),
                                             (300, 320, 960, 42, False), (513, 640, 5120, 44, True), (100, 1280, 1280, 41, False)])
def test_gemm_layernorm_fold(ops, m, c, n, tile, geglu):
    """LN(x) W^T + b computed from the RAW x: W carries gamma, bias carries W.beta, statistics in-kernel."""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    x = rnd(m, c, seed=90) * 1.7 + 0.4
    w = rnd(n, c, seed=91, scale=c ** -0.5).float()
    g = torch.Generator().manual_seed(92)
    gamma, beta, bias = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(n, generator=g)
    ref = F.linear(F.layer_norm(x.float(), (c,), gamma, beta, 1e-5), w, bias)
    b2 = bias + w @ beta
    if geglu:
        a, gate = ref.chunk(2, dim=-1)
        ref = a * F.gelu(gate)
        f = torch.arange(n // 2)
        perm = torch.empty(n, dtype=torch.long)
        perm[f] = (f // 64) * 128 + f % 64
        perm[n // 2 + f] = (f // 64) * 128 + 64 + f % 64
        bp = torch.empty_like(b2)
        bp[perm] = b2
        b2 = bp
    wp = ops.pack_linear((w * gamma[None]).cuda(), geglu=geglu)
    lns = ops.rowsum(wp, c)
    got = ops.gemm(x.cuda(), wp, n, c, bias=b2.cuda(), lns=lns, tile=tile, flags=(GF_GEGLU | GF_BIAS) if geglu else 0)
    close(got, ref, tol=3e-3)


@pytest.mark.parametrize("m,c,n,ranges,geglu,with_bias", [(300, 320, 960, 2, False, True), (12288, 320, 960, 5, False, True), (513, 640, 1920, 4, False, True),
                                                          (129, 320, 320, 10, False, False), (513, 320, 2560, 3, True, True), (12288, 320, 2560, 5, True, True),
                                                          (1000, 640, 5120, 8, True, True), (3072, 640, 5120, 5, True, False), (128, 320, 2560, 20, True, True)])
def test_lnlin_activation_stationary_kernel(ops, m, c, n, ranges, geglu, with_bias):
    """lnlin_kernel (tile id 50: activations resident in registers, weights streamed, statistics from the registers) against torch and
    against gemm_kernel's LayerNorm fold of the same operands; `ranges` = column ranges per 128-row block (ragged last range)."""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    x = rnd(m, c, seed=190) * 1.7 + 0.4
    w = rnd(n, c, seed=191, scale=c ** -0.5).float()
    g = torch.Generator().manual_seed(192)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    bias = 0.1 * torch.randn(n, generator=g) if with_bias else torch.zeros(n)
    b2 = bias + w @ beta
    ref = F.linear(F.layer_norm(x.float(), (c,), gamma, beta, 1e-5), w, bias)
    if geglu:
        a, gate = ref.chunk(2, dim=-1)
        ref = a * F.gelu(gate)
        f = torch.arange(n // 2)
        perm = torch.empty(n, dtype=torch.long)
        perm[f] = (f // 64) * 128 + f % 64
        perm[n // 2 + f] = (f // 64) * 128 + 64 + f % 64
        bp = torch.empty_like(b2)
        bp[perm] = b2
        b2 = bp
    wp = ops.pack_linear((w * gamma[None]).cuda(), geglu=geglu)
    lns = ops.rowsum(wp, c)
    fl = (GF_GEGLU if geglu else 0) | GF_BIAS
    got = ops.gemm(x.cuda(), wp, n, c, bias=b2.cuda(), lns=lns, tile=50, splits=ranges, flags=fl)
    close(got, ref, tol=3e-3)
    other = ops.gemm(x.cuda(), wp, n, c, bias=b2.cuda(), lns=lns, tile=0, flags=fl)
    assert (got.float() - other.float()).abs().max().item() <= 2e-2 * max(1.0, other.float().abs().max().item())


@pytest.mark.parametrize("m,c,n,ranges,batch", [(12288, 320, 320, 4, 0), (3072, 640, 640, 5, 0), (300, 320, 640, 10, 0), (4096, 320, 320, 2, 3), (1024, 640, 640, 10, 3),
                                                 (129, 640, 32, 1, 0)])
def test_lnlin_plain_variant_bias_residual_rowstats_grouped(ops, m, c, n, ranges, batch):
    """lnlin_kernel without the LayerNorm (tile id 50 on a plain problem): out = A W^T + bias + R with the row statistics of the stored
    values (one partial per column range), and as a grouped problem (per-sample weights and biases, rows of all samples in one launch)."""
    nb = max(batch, 1)
    x = rnd(nb * m, c, seed=195)
    res = rnd(nb * m, n, seed=196)
    g = torch.Generator().manual_seed(197)
    ws = [rnd(n, c, seed=198 + b, scale=c ** -0.5).float() for b in range(nb)]
    bs = [0.1 * torch.randn(n, generator=g) for _ in range(nb)]
    ref = torch.cat([F.linear(x[b * m:(b + 1) * m].float(), ws[b], bs[b]) for b in range(nb)]) + res.float()
    wp = torch.cat([ops.pack_linear(w.cuda()) for w in ws]).contiguous()
    npad = wp.shape[0] // nb
    bias = torch.zeros(nb, npad)
    for b in range(nb):
        bias[b, :n] = bs[b]
    got, st = ops.gemm(x.cuda(), wp, n, c, bias=bias.reshape(-1).cuda(), resid=res.cuda(), tile=50, splits=ranges, batch=batch, row_stats=True)
    close(got, ref, tol=3e-3)
    assert st.shape[0] == ranges
    gf = got.float().cpu()
    want = torch.stack([gf.sum(dim=1), (gf * gf).sum(dim=1)], dim=-1)
    assert torch.allclose(st.sum(dim=0).cpu(), want, rtol=1e-3, atol=5e-2)
    other = ops.gemm(x.cuda(), wp, n, c, bias=bias.reshape(-1).cuda(), resid=res.cuda(), tile=2, batch=batch)
    assert (got.float() - other.float()).abs().max().item() <= 1e-2 * max(1.0, other.float().abs().max().item())


@pytest.mark.parametrize("ranges", [6, 8, 9])
def test_lnlin_rejects_column_range_counts_that_leave_a_range_empty(ops, ranges):
    """N = 640 is 20 chunks of 32 columns: 6 ranges of ceil(20 / 6) = 4 chunks leave the sixth range empty (8 and 9 ranges of 3
    chunks: the last one / two).  Such a workgroup used to return before it wrote its row-statistics partial while the consumer summed all
    `ranges` partials (round-4 advisor finding): the launcher now refuses these counts (the tuner only tries what it accepts).  The
    counts that divide evenly keep working with a NaN-poisoned statistics table."""
    from diffusiontexturepainting_amd._lib import DtpError
    m, c, n = 300, 320, 640
    x, res = rnd(m, c, seed=295), rnd(m, n, seed=296)
    w = rnd(n, c, seed=297, scale=c ** -0.5).float()
    wp = ops.pack_linear(w.cuda())
    with pytest.raises(DtpError):
        ops.gemm(x.cuda(), wp, n, c, resid=res.cuda(), tile=50, splits=ranges, row_stats=True)
    got, st = ops.gemm(x.cuda(), wp, n, c, resid=res.cuda(), tile=50, splits=10, row_stats=True)
    gf = got.float().cpu()
    want = torch.stack([gf.sum(dim=1), (gf * gf).sum(dim=1)], dim=-1)
    assert st.shape[0] == 10 and torch.allclose(st.sum(dim=0).cpu(), want, rtol=1e-3, atol=5e-2)


@pytest.mark.experimental
@pytest.mark.parametrize("m,k,n,splits,tail", [(768, 1280, 1280, 1, 0), (768, 1280, 3840, 1, 0), (3072, 2560, 640, 1, 640), (192, 1280, 1280, 4, 0),
                                                (100, 128, 96, 1, 0), (333, 704, 320, 3, 64), (64, 6400, 64, 5, 1280), (12288, 1280, 320, 1, 320)])
def test_gemm_weight_streaming_kernel(ops, m, k, n, splits, tail):
    needs_experimental_build(ops)
    """gemmws_kernel (tile id 55: weights in fragment order straight into registers, the four waves split the contraction by k-blocks,
    wave-private activation rings): out = [A | A2] W^T + bias + R with the row statistics of the stored values; ragged row tiles, an
    odd n-tile count (N = 96), waves without a k-block (K = 128), K-slices with fp32 slabs, the two-operand contraction."""
    ka = k - tail
    x = rnd(m, ka, seed=230)
    x2 = rnd(m, tail, seed=231) if tail else None
    res = rnd(m, n, seed=232)
    w = rnd(n, k, seed=233, scale=k ** -0.5).float()
    bias = 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(234))
    xa = torch.cat([x, x2], dim=1) if tail else x
    ref = F.linear(xa.float(), w, bias) + res.float()
    wp = ops.pack_linear(w.cuda())
    wfr = ops.pack_linear_ws(wp, n, k)
    bp = torch.zeros(wp.shape[0])
    bp[:n] = bias
    kw = dict(bias=bp.cuda(), resid=res.cuda(), tail=x2.cuda() if tail else None)
    got, st = ops.gemm(x.cuda(), wp, n, ka, tile=55, splits=splits, wfr=wfr, row_stats=True, **kw)
    close(got, ref, tol=3e-3)
    gf = got.float().cpu()
    want = torch.stack([gf.sum(dim=1), (gf * gf).sum(dim=1)], dim=-1)
    assert st.shape[0] == (1 if splits > 1 else (n + 63) // 64)
    assert torch.allclose(st.sum(dim=0).cpu(), want, rtol=1e-3, atol=5e-2)
    other = ops.gemm(x.cuda(), wp, n, ka, tile=2, **kw)
    assert (got.float() - other.float()).abs().max().item() <= 1e-2 * max(1.0, other.float().abs().max().item())
    again, _ = ops.gemm(x.cuda(), wp, n, ka, tile=55, splits=splits, wfr=wfr, row_stats=True, **kw)
    assert torch.equal(got, again)  # fixed summation order


@pytest.mark.experimental
@pytest.mark.parametrize("m,c,n", [(768, 1280, 3840), (192, 1280, 1280), (500, 640, 320)])
def test_gemm_weight_streaming_layernorm_fold(ops, m, c, n):
    needs_experimental_build(ops)
    """gemmws_kernel with GF_LNFOLD: the raw pre-LayerNorm rows, gamma folded into W, statistics from the producer's per-range
    partials (here: three synthetic partials per row that add up to the row sums)."""
    x = rnd(m, c, seed=240) * 1.5 + 0.3
    w = rnd(n, c, seed=241, scale=c ** -0.5).float()
    g = torch.Generator().manual_seed(242)
    gamma, beta, bias = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(n, generator=g)
    ref = F.linear(F.layer_norm(x.float(), (c,), gamma, beta, 1e-5), w, bias)
    wp = ops.pack_linear((w * gamma[None]).cuda())
    wfr = ops.pack_linear_ws(wp, n, c)
    lns = ops.rowsum(wp, c)
    b2 = torch.zeros(wp.shape[0])
    b2[:n] = bias + w @ beta
    xf = x.float()
    tot = torch.stack([xf.sum(dim=1), (xf * xf).sum(dim=1)], dim=-1)
    parts = torch.stack([0.5 * tot, 0.3 * tot, 0.2 * tot]).contiguous().cuda()
    got = ops.gemm(x.cuda(), wp, n, c, bias=b2.cuda(), lns=lns, stats_in=parts, tile=55, wfr=wfr)
    close(got, ref, tol=3e-3)
    other = ops.gemm(x.cuda(), wp, n, c, bias=b2.cuda(), lns=lns, stats_in=parts, tile=2)
    assert (got.float() - other.float()).abs().max().item() <= 1e-2 * max(1.0, other.float().abs().max().item())


@pytest.mark.parametrize("tile", [-1, 2, 5, 8, 33, 34, 39, 41, 46])
def test_gemm_batched_group_softmax(ops, tile):
    """Grouped GEMM (one weight matrix per batch entry) + LayerNorm fold + softmax over groups of 16 columns (14 valid):
    the first half of the algebraically fused cross-attention (scores against 14 context tokens, 8 heads)."""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_SOFTMAX16
    nb, m, c = 3, 200, 320
    x = rnd(nb * m, c, seed=70) * 1.3 + 0.2
    w = rnd(nb, 128, c, seed=71, scale=2.0 * c ** -0.5).float()
    g = torch.Generator().manual_seed(72)
    gamma, beta, bias = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(nb, 128, generator=g)
    xn = F.layer_norm(x.float(), (c,), gamma, beta, 1e-5).view(nb, m, c)
    sc = torch.einsum("bmc,bnc->bmn", xn, w) + bias[:, None]
    sc = sc.view(nb, m, 8, 16)
    ref = torch.zeros_like(sc)
    ref[..., :14] = torch.softmax(sc[..., :14], dim=-1)
    wp = torch.cat([ops.pack_linear((w[b] * gamma[None]).cuda()) for b in range(nb)], dim=0).contiguous()
    b2 = (bias + torch.einsum("bnc,c->bn", w, beta)).reshape(-1)
    lns = ops.rowsum(wp, c)
    got = ops.gemm(x.cuda(), wp, 128, c, bias=b2.cuda(), lns=lns, tile=tile, flags=GF_BIAS | GF_SOFTMAX16, batch=nb, sm_valid=14)
    close(got, ref.view(nb * m, 128), tol=3e-3)


@pytest.mark.parametrize("nb,s,c", [(3, 4096, 320), (3, 1024, 640), (3, 256, 1280), (2, 64, 1280), (3, 200, 320), (1, 16, 1280), (6, 4, 640)])
def test_fused_cross_attention_pair_matches_the_two_gemms(ops, nb, s, c):
    """xattn_kernel = scores GEMM (LayerNorm fold from the producer's row statistics, group softmax) + value-output GEMM (bias,
    residual, row statistics for the next fold) in one launch.  Same MFMA order and the same fp16 rounding points as the unfused pair
    (only the fp32 epilogue expressions may be contracted differently by the compiler): outputs within one fp16 step of it, the
    statistics partials consistent with the stored rows, and both against torch."""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_SOFTMAX16
    g = torch.Generator().manual_seed(77)
    x = (rnd(nb * s, c, seed=78) * 1.3 + 0.2).cuda()
    w1 = rnd(nb, 128, c, seed=79, scale=2.0 * c ** -0.5).float()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    b1 = 0.3 * torch.randn(nb, 128, generator=g)
    w2 = rnd(nb, c, 128, seed=80, scale=0.1).float()
    b2 = torch.randn(c, generator=g)
    # the producer's row statistics: (sum, sumsq) of x in two arbitrary column parts
    xf = x.float().cpu()
    h = c // 2
    st_in = torch.stack([torch.stack([xf[:, :h].sum(1), (xf[:, :h] ** 2).sum(1)], dim=1),
                         torch.stack([xf[:, h:].sum(1), (xf[:, h:] ** 2).sum(1)], dim=1)]).cuda()
    w1p = torch.cat([ops.pack_linear((w1[b] * gamma[None]).cuda()) for b in range(nb)], dim=0).contiguous()
    b1f = (b1 + torch.einsum("bnc,c->bn", w1, beta)).reshape(-1).cuda()
    lns = ops.rowsum(w1p, c)
    w2p = torch.cat([ops.pack_linear(w2[b].cuda()) for b in range(nb)], dim=0).contiguous()
    # unfused pair on tile 3 (64 x 128, two stages, 4 waves)
    pm = ops.gemm(x, w1p, 128, c, bias=b1f, lns=lns, tile=3, flags=GF_BIAS | GF_SOFTMAX16, batch=nb, sm_valid=14, stats_in=st_in)
    ref_y, ref_st = ops.gemm(pm, w2p, c, 128, bias=b2.cuda(), resid=x, tile=3, batch=nb, bias_shared=True, row_stats=True)
    got_y, got_st = ops.xattn(x, w1p, b1f, lns, st_in, w2p, b2.cuda(), nb, row_stats=True)
    d = (got_y.float() - ref_y.float()).abs()
    assert d.max().item() <= 2.0 ** -7 * max(1.0, ref_y.float().abs().max().item()) and (d > 0).float().mean().item() < 0.05
    # the partials are the (sum, sumsq) of the STORED fp16 rows, per 128-column tile
    yf = got_y.float()
    for t in range(got_st.shape[0]):
        blk = yf[:, 128 * t:128 * (t + 1)]
        assert torch.allclose(got_st[t, :, 0], blk.sum(1), rtol=1e-4, atol=1e-2) and torch.allclose(got_st[t, :, 1], (blk * blk).sum(1), rtol=1e-4, atol=1e-2)
    xn = F.layer_norm(xf, (c,), gamma, beta, 1e-5).view(nb, s, c)
    sc = (torch.einsum("bmc,bnc->bmn", xn, w1) + b1[:, None]).view(nb, s, 8, 16)
    pr = torch.zeros_like(sc)
    pr[..., :14] = torch.softmax(sc[..., :14], dim=-1)
    ref = torch.einsum("bmk,bnk->bmn", pr.view(nb, s, 128), w2).reshape(nb * s, c) + b2 + xf
    close(got_y, ref, tol=4e-3)


@pytest.mark.parametrize("nb,s,c,ct", [(3, 4096, 320, 2), (2, 300, 640, 5), (1, 130, 1280, 3), (3, 256, 1280, 10), (2, 64, 320, 3)])
def test_fused_cross_attention_several_column_tiles_per_workgroup(ops, nb, s, c, ct, monkeypatch):
    """xattn_kernel with `ct` consecutive 128-column tiles per workgroup (round 5: the probability tile is computed once, the W2 tiles
    alternate between two LDS buffers, bias / residual operands of the next tile are prefetched): bit-identical to one tile per
    workgroup -- same MFMA order per output element -- for full and ragged tile groups (3 tiles in groups of 2, 10 in groups of 3)."""
    g = torch.Generator().manual_seed(177)
    x = (rnd(nb * s, c, seed=178) * 1.3 + 0.2).cuda()
    w1 = rnd(nb, 128, c, seed=179, scale=2.0 * c ** -0.5).float()
    b1 = 0.3 * torch.randn(nb, 128, generator=g)
    w2 = rnd(nb, c, 128, seed=180, scale=0.1).float()
    b2 = torch.randn(c, generator=g)
    xf = x.float().cpu()
    st_in = torch.stack([torch.stack([xf.sum(1), (xf ** 2).sum(1)], dim=1)]).cuda()
    w1p = torch.cat([ops.pack_linear(w1[b].cuda()) for b in range(nb)], dim=0).contiguous()
    lns = ops.rowsum(w1p, c)
    w2p = torch.cat([ops.pack_linear(w2[b].cuda()) for b in range(nb)], dim=0).contiguous()
    ref_y, ref_st = ops.xattn(x, w1p, b1.reshape(-1).cuda(), lns, st_in, w2p, b2.cuda(), nb, row_stats=True, ct=1)
    got_y, got_st = ops.xattn(x, w1p, b1.reshape(-1).cuda(), lns, st_in, w2p, b2.cuda(), nb, row_stats=True, ct=ct)
    assert torch.equal(got_y, ref_y) and torch.equal(got_st, ref_st)


@pytest.mark.parametrize("nb,s", [(3, 4096), (1, 128), (2, 1024), (24, 256)])
def test_register_chained_out_projection_and_cross_attention(ops, nb, s):
    """xchain_kernel: y2 = a Wo^T + bo + y, P = softmax_14of16(LN(y2) W1^T + b1) per head group, y3 = P W2^T + b2 + y2 in ONE launch with y2,
    its LayerNorm statistics and P held in registers (the accumulator of one MFMA contraction is the B operand of the next, the weight
    fragments of the chained contractions are read in the permuted k order).  Against torch in fp32, and against the two launches it replaces
    (plain Linear with residual + row statistics, then the fused cross-attention pair) within fp16 rounding; the row statistics it emits for
    the LayerNorm-folded FF1 must be those of the stored y3."""
    c = 320
    g = torch.Generator().manual_seed(377)
    a = (rnd(nb * s, c, seed=378) * 1.2).cuda()
    y = (rnd(nb * s, c, seed=379) * 1.3 + 0.2).cuda()
    wo = rnd(c, c, seed=380, scale=c ** -0.5).float()
    bo = 0.2 * torch.randn(c, generator=g)
    w1 = rnd(nb, 128, c, seed=381, scale=2.0 * c ** -0.5).float()
    b1 = 0.3 * torch.randn(nb, 128, generator=g)
    w2 = rnd(nb, c, 128, seed=382, scale=0.1).float()
    b2 = torch.randn(c, generator=g)
    # fp32 reference
    y2 = (a.float().cpu() @ wo.t() + bo + y.float().cpu()).half().float()
    ln = F.layer_norm(y2, (c,), eps=1e-5).view(nb, s, c)
    sc = torch.einsum("bsc,bnc->bsn", ln, w1) + b1[:, None, :]
    pm = torch.zeros_like(sc).view(nb, s, 8, 16)
    pm[..., :14] = torch.softmax(sc.view(nb, s, 8, 16)[..., :14], dim=-1)
    ref = torch.einsum("bsn,bcn->bsc", pm.view(nb, s, 128).half().float(), w2).reshape(nb * s, c) + b2 + y2
    wop = ops.pack_linear(wo.cuda())
    w1p = torch.cat([ops.pack_linear(w1[b].cuda()) for b in range(nb)], dim=0).contiguous()
    lns = ops.rowsum(w1p, c)
    w2p = torch.cat([ops.pack_linear(w2[b].cuda()) for b in range(nb)], dim=0).contiguous()
    got, st = ops.xchain(a, wop, bo.cuda(), y, w1p, b1.reshape(-1).cuda(), lns, w2p, b2.cuda(), nb, row_stats=True)
    close(got, ref, tol=3e-3)
    gf = got.float().cpu()
    assert torch.allclose(st[:, 0].cpu(), gf.sum(dim=1), rtol=1e-4, atol=1e-2) and torch.allclose(st[:, 1].cpu(), (gf * gf).sum(dim=1), rtol=1e-4, atol=1e-2)
    # the two launches it replaces
    y2g, st2 = ops.gemm(a, wop, c, c, bias=bo.cuda(), resid=y, tile=50, splits=5, row_stats=True)
    two = ops.xattn(y2g, w1p, b1.reshape(-1).cuda(), lns, st2[:5].contiguous(), w2p, b2.cuda(), nb)
    close(got, two.float().cpu(), tol=3e-3)


@pytest.mark.parametrize("m", [12288, 128, 300, 1000])
def test_register_chained_feed_forward(ops, m):
    """ffchain_kernel: out = [GEGLU(LN(x) W1^T + b1) | x] Wm^T + bm + r with the [M, 1280] hidden tensor held in registers (FF1's
    accumulators become FF2's B operand, pair of 32-column chunks by pair).  Against torch in fp32 (hidden rounded to fp16 where the kernel
    rounds it), and against the two launches it replaces (lnlin GEGLU, then the K = 1600 GEMM over [h | x]); ragged last row block."""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    c, hdim = 320, 1280
    g = torch.Generator().manual_seed(477)
    x = rnd(m, c, seed=478) * 1.7 + 0.4
    r = rnd(m, c, seed=479)
    w1 = rnd(2 * hdim, c, seed=480, scale=c ** -0.5).float()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    b1 = 0.1 * torch.randn(2 * hdim, generator=g)
    wm = rnd(c, hdim + c, seed=481, scale=(hdim + c) ** -0.5).float()
    bm = 0.1 * torch.randn(c, generator=g)
    pre = F.linear(F.layer_norm(x.float(), (c,), gamma, beta, 1e-5), w1, b1)
    a, gate = pre.chunk(2, dim=-1)
    h = (a * F.gelu(gate)).half().float()
    ref = F.linear(torch.cat([h, x.float()], dim=-1), wm, bm) + r.float()
    # packed operands: GEGLU row packing for W1 (and its bias), LayerNorm gamma folded into W1, beta into the bias
    b1f = b1 + w1 @ beta
    f = torch.arange(hdim)
    perm = torch.empty(2 * hdim, dtype=torch.long)
    perm[f] = (f // 64) * 128 + f % 64
    perm[hdim + f] = (f // 64) * 128 + 64 + f % 64
    b1p = torch.empty_like(b1f)
    b1p[perm] = b1f
    w1p = ops.pack_linear((w1 * gamma[None]).cuda(), geglu=True)
    lns = ops.rowsum(w1p, c)
    wmp = ops.pack_linear(wm.cuda())
    got = ops.ffchain(x.cuda(), w1p, lns, b1p.cuda(), wmp, bm.cuda(), resid=r.cuda())
    close(got, ref, tol=4e-3)
    hg = ops.gemm(x.cuda(), w1p, 2 * hdim, c, bias=b1p.cuda(), lns=lns, tile=50, splits=5, flags=GF_GEGLU | GF_BIAS)
    two = ops.gemm(hg, wmp, c, hdim, bias=bm.cuda(), resid=r.cuda(), tail=x.cuda())
    close(got, two.float().cpu(), tol=4e-3)


def test_gemm_batched_residual(ops):
    """Second half: P [b*M, 128] times a per-entry [N, 128] matrix, + bias + residual."""
    nb, m, n = 3, 130, 320
    pm = torch.rand(nb * m, 128, generator=torch.Generator().manual_seed(73)).half()
    w = rnd(nb, n, 128, seed=74, scale=0.1).float()
    bias = torch.randn(n, generator=torch.Generator().manual_seed(75))
    r = rnd(nb * m, n, seed=76)
    ref = torch.einsum("bmk,bnk->bmn", pm.float().view(nb, m, 128), w).reshape(nb * m, n) + bias + r.float()
    wp = torch.cat([ops.pack_linear(w[b].cuda()) for b in range(nb)], dim=0).contiguous()
    from diffusiontexturepainting_amd._lib import GemmDesc
    got = ops.gemm(pm.cuda(), wp, n, 128, bias=bias.cuda().repeat(1), resid=r.cuda(), batch=nb, bias_shared=True)
    close(got, ref)


@pytest.mark.parametrize("m,k1,k2,n,tile,splits", [(300, 1280, 320, 320, -1, 0), (130, 256, 64, 192, 2, 3), (768, 640, 128, 640, 17, 1), (64, 128, 128, 128, 5, 2),
                                                   (768, 640, 128, 640, 21, 1), (600, 1280, 320, 320, 20, 1), (300, 1280, 320, 320, 32, 1), (130, 256, 64, 192, 38, 3),
                                                   (768, 640, 128, 640, 35, 2), (300, 1280, 320, 320, 43, 1), (130, 256, 64, 192, 46, 3)])
def test_gemm_two_activation_matrices(ops, m, k1, k2, n, tile, splits):
    """[f | r] . [W1 | W2]^T with f and r in separate buffers: how ff.net.2 (+residual) and proj_out run as one GEMM."""
    f, r = rnd(m, k1, seed=30), rnd(m, k2, seed=31)
    w = rnd(n, k1 + k2, seed=32, scale=(k1 + k2) ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(33))
    res = rnd(m, n, seed=34)
    ref = F.linear(torch.cat([f, r], dim=1).float(), w.float(), bias) + res.float()
    got = ops.gemm(f.cuda(), ops.pack_linear(w.float().cuda()), n, k1, bias=bias.cuda(), resid=res.cuda(), tail=r.cuda(), tile=tile, splits=splits)
    close(got, ref)


@pytest.mark.parametrize("tile", [-1, 20, 21])
def test_gemm_epilogues(ops, tile):
    from diffusiontexturepainting_amd._lib import GF_BIAS_M, GF_GELU, GF_OUT_F32, GF_QUICKGELU, GF_SILU
    m, n, k = 130, 256, 192
    a, w = rnd(m, k, seed=11), rnd(n, k, seed=12, scale=k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(13))
    wp = ops.pack_linear(w.float().cuda())
    lin = F.linear(a.float(), w.float(), bias)
    close(ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), flags=GF_GELU, tile=tile), F.gelu(lin))
    close(ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), flags=GF_QUICKGELU, tile=tile), lin * torch.sigmoid(1.702 * lin))
    close(ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), flags=GF_SILU, tile=tile), F.silu(lin))
    if tile >= 20:
        from diffusiontexturepainting_amd._lib import DtpError
        with pytest.raises(DtpError):  # per-row bias is not an epilogue of the wide tiles: loud, not silent
            ops.gemm(a.cuda(), wp, n, k, bias=torch.zeros(m).cuda(), flags=GF_BIAS_M, tile=tile)
        return
    # operand-swapped call: out[n'][m'] = W x^T + bias[n'] (how V^T is produced for the VAE attention)
    bm = torch.randn(m, generator=torch.Generator().manual_seed(14))
    got = ops.gemm(a.cuda(), wp, n, k, bias=bm.cuda(), flags=GF_BIAS_M)
    close(got, F.linear(a.float(), w.float()) + bm[:, None])
    # the same activations behind a split contraction: the slabs are summed, biased and activated by the reduce kernel (four columns per
    # thread with an fp16 output, one per thread with an fp32 one); reached once, by the tile = -1 case (the wide tiles returned above)
    for f32 in (0, GF_OUT_F32):
        close(ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), flags=GF_GELU | f32, tile=2, splits=3), F.gelu(lin))
        close(ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), flags=GF_QUICKGELU | f32, tile=2, splits=3), lin * torch.sigmoid(1.702 * lin))
        close(ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), flags=GF_SILU | f32, tile=2, splits=3), F.silu(lin))
    close(ops.gemm(a.cuda(), wp, n, k, bias=bm.cuda(), flags=GF_BIAS_M | GF_SILU, tile=2, splits=3), F.silu(F.linear(a.float(), w.float()) + bm[:, None]))


CONV_CASES = [
    # B, H, W, Cin, Cout, stride, pad, upsample, out_hw
    (2, 16, 16, 64, 128, 1, 1, False, None),
    (3, 8, 8, 320, 320, 1, 1, False, None),
    (1, 12, 20, 128, 64, 1, 1, False, None),       # non-square, Cout < tile
    (2, 16, 16, 64, 64, 2, 1, False, None),        # UNet downsampler
    (2, 16, 16, 128, 128, 2, 0, False, (8, 8)),    # VAE downsampler: pad (0,1,0,1)
    (2, 8, 8, 64, 64, 1, 1, True, None),           # nearest-2x upsample fused into the gather
    (3, 16, 16, 16, 320, 1, 1, False, None),       # conv_in (9 -> 16 padded channels): taps straddle k-blocks
    (1, 16, 16, 8, 128, 1, 1, False, None),        # VAE conv_in (3 -> 8)
    (2, 16, 16, 320, 4, 1, 1, False, None),        # conv_out: tiny N
    (1, 4, 4, 1280, 1280, 1, 1, False, None),      # deep level, split-K heuristic
]


CONV_TILES = [-1, 5, 8, 10, 16, 19, 20, 21, 32, 34, 37, 39, 40, 42, 45, 47]
# (round 6, as for test_gemm_dense: the heuristic on every case, an explicit tile on four of the seven, rotating)
CONV_TILE_CASES = [(c, t) for i, t in enumerate(CONV_TILES) for j, c in enumerate(CONV_CASES) if t == -1 or (j + i) % 7 in (0, 2, 3, 5)]


@pytest.mark.parametrize("case,tile", CONV_TILE_CASES)
def test_conv3x3(ops, case, tile):
    b, h, w, cin, cout, stride, pad, ups, out_hw = case
    if tile in (20, 21) and cout % 8:
        pytest.skip("the wide tiles need N % 8 == 0")
    x = rnd(b, h, w, cin, seed=20)
    wt = rnd(cout, cin, 3, 3, seed=21, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(22))
    xin = x.float().permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if out_hw is not None and pad == 0:
        xin = F.pad(xin, (0, 1, 0, 1))
        ref = F.conv2d(xin, wt.float(), bias, stride=stride, padding=0)
    else:
        ref = F.conv2d(xin, wt.float(), bias, stride=stride, padding=pad)
    res = rnd(*ref.permute(0, 2, 3, 1).shape, seed=23)
    ref = ref.permute(0, 2, 3, 1) + res.float()
    wp = ops.pack_conv(wt.float().cuda())
    got = ops.conv3x3(x.cuda(), wp, cout, stride=stride, pad=pad, upsample=ups, bias=bias.cuda(), resid=res.cuda(),
                      out_hw=out_hw, tile=tile)
    close(got, ref)


@pytest.mark.parametrize("b,h,cin,cin2,cout,tile,splits", [(2, 16, 64, 128, 64, -1, 0), (3, 8, 320, 640, 320, 5, 0), (1, 8, 128, 64, 256, 8, 3),
                                                           (3, 16, 320, 640, 320, 17, 2), (1, 16, 128, 64, 256, 18, 0),
                                                           (3, 16, 320, 640, 320, 21, 1), (1, 16, 128, 64, 256, 20, 1),
                                                           (3, 8, 320, 640, 320, 33, 0), (1, 8, 128, 64, 256, 36, 3), (2, 16, 64, 128, 64, 38, 2),
                                                           (3, 8, 320, 640, 320, 41, 0), (1, 8, 128, 64, 256, 46, 3), (3, 16, 320, 640, 320, 44, 2)])
def test_conv3x3_fused_shortcut(ops, b, h, cin, cin2, cout, tile, splits):
    """ResBlock tail as ONE contraction: conv3x3(t) + conv1x1(x) + biases = [im2col(t) | x] . [W3 | W1]^T."""
    t, x = rnd(b, h, h, cin, seed=24), rnd(b, h, h, cin2, seed=25)
    w3 = rnd(cout, cin, 3, 3, seed=26, scale=(9 * cin) ** -0.5)
    w1 = rnd(cout, cin2, 1, 1, seed=27, scale=cin2 ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(28))
    ref = F.conv2d(t.float().permute(0, 3, 1, 2), w3.float(), bias, padding=1) + F.conv2d(x.float().permute(0, 3, 1, 2), w1.float())
    wp = torch.cat([ops.pack_conv(w3.float().cuda())[:, : 9 * cin], ops.pack_conv(w1.float().cuda())[:, :cin2]], dim=1).contiguous()
    got = ops.conv3x3(t.cuda(), wp, cout, bias=bias.cuda(), tail=x.cuda(), tile=tile, splits=splits)
    close(got, ref.permute(0, 2, 3, 1))


HALO_CASES = [
    # B, H, W, Cin, Cout, variant(12..15), splits
    (3, 64, 64, 320, 320, 12, 1), (3, 64, 64, 320, 320, 13, 1), (2, 32, 32, 640, 640, 13, 2), (3, 16, 16, 1280, 1280, 14, 4),
    (3, 8, 8, 1280, 1280, 15, 5), (1, 24, 40, 128, 128, 12, 1), (2, 12, 20, 64, 64, 14, 1), (1, 128, 128, 128, 256, 13, 1),
    # 48 / 49: three images per workgroup
    (3, 8, 8, 1280, 1280, 48, 5), (3, 8, 8, 1280, 1280, 49, 1), (6, 16, 16, 1280, 1280, 49, 4), (3, 16, 16, 640, 1280, 48, 2), (3, 12, 20, 64, 192, 49, 1),
]


@pytest.mark.parametrize("case", HALO_CASES)
def test_conv3x3_halo_kernel(ops, case):
    """The halo-tiled kernel (input patch staged once per 64-channel block, reused by all 9 taps) vs torch conv2d."""
    b, h, w, cin, cout, variant, splits = case
    x = rnd(b, h, w, cin, seed=33)
    wt = rnd(cout, cin, 3, 3, seed=34, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(35))
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    res = rnd(*ref.shape, seed=36)
    ref = ref + res.float()
    wf = wt.float().cuda()
    got = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), resid=res.cuda(), wcb=ops.pack_conv_cb(wf), tile=variant,
                      splits=splits)
    close(got, ref)


WS_CASES = [
    # B, H(=W), Cin, Cout, tile (51: 8x8 images in groups of three, 52: 16x16 images), K-slices
    (3, 8, 1280, 1280, 51, 5), (3, 8, 128, 64, 51, 1), (3, 8, 192, 96, 51, 2), (6, 8, 640, 320, 51, 3), (3, 8, 2560, 1280, 51, 8),
    (3, 16, 1280, 1280, 52, 2), (1, 16, 64, 32, 52, 1), (2, 16, 320, 100, 52, 5), (3, 16, 640, 1280, 52, 1),
    # tile 53: 8 x 16 pixel tiles (any H % 8 == 0, W % 16 == 0; here W = H or (H, W) given as a pair), two n-tiles per workgroup
    (3, 16, 1280, 1280, 53, 2), (1, 64, 320, 320, 53, 1), (2, 32, 640, 640, 53, 2), (1, (24, 32), 128, 96, 53, 1), (3, (8, 48), 192, 160, 53, 3),
    # tile 54: the same kernel built for two co-resident workgroups per CU (two fragment sets, the partial tiles combined one n-tile at a time)
    (3, 16, 1280, 1280, 54, 2), (1, 64, 320, 320, 54, 1), (2, 32, 640, 640, 54, 2), (1, (24, 32), 128, 96, 54, 1), (3, (8, 48), 192, 160, 54, 3),
]


@pytest.mark.parametrize("case", WS_CASES)
def test_conv3x3_weight_streaming_kernel(ops, case):
    """convws_kernel (weights in MFMA fragment order straight into registers, contraction split over the four waves) vs torch conv2d:
    split launches through the slab reduce, unsplit ones through the kernel's own bias / residual epilogue."""
    b, h, cin, cout, tile, splits = case
    h, w_ = h if isinstance(h, tuple) else (h, h)
    x = rnd(b, h, w_, cin, seed=53)
    wt = rnd(cout, cin, 3, 3, seed=54, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(55))
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    res = rnd(*ref.shape, seed=56)
    ref = ref + res.float()
    wf = wt.float().cuda()
    got = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), resid=res.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile, splits=splits)
    close(got, ref)


@pytest.mark.parametrize("b,h,cin,cout,tile,resid", [(3, 64, 320, 320, 54, False), (2, 32, 640, 640, 53, True), (1, (16, 32), 128, 1280, 54, True),
                                                     (2, 16, 64, 640, 53, False)])
def test_conv3x3_weight_streaming_emits_groupnorm_statistics(ops, b, h, cin, cout, tile, resid):
    """DTP_GF_GNSTATS: the conv's epilogue also emits per-(pixel tile, group) sums of its rounded outputs (32 groups of 10 / 20 / 40
    channels: groups straddle the 64-channel n-ranges); summed over the chunks they are the statistics of the stored tensor, and the
    apply pass fed with them equals torch's group_norm."""
    h, w_ = h if isinstance(h, tuple) else (h, h)
    x = rnd(b, h, w_, cin, seed=83)
    wt = rnd(cout, cin, 3, 3, seed=84, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(85))
    res = rnd(b, h, w_, cout, seed=86) if resid else None
    wf = wt.float().cuda()
    y, st = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), resid=res.cuda() if resid else None, wfr=ops.pack_conv_ws(wf), tile=tile,
                        splits=1, gn_groups=32)
    assert torch.isfinite(st).all()  # every (chunk, group) slot was written
    yf = y.float().reshape(b, h * w_, 32, cout // 32)
    want = torch.stack([yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))], dim=-1)
    got = st.sum(dim=1)
    assert torch.allclose(got, want, rtol=2e-4, atol=2e-2), (got - want).abs().max().item()
    gamma, beta = torch.randn(cout, generator=torch.Generator().manual_seed(87)).cuda(), torch.randn(cout, generator=torch.Generator().manual_seed(88)).cuda()
    z = ops.groupnorm_apply(y, gamma, beta, st, eps=1e-5, silu=True)
    ref = F.silu(F.group_norm(y.float().permute(0, 3, 1, 2), 32, gamma, beta, eps=1e-5)).permute(0, 2, 3, 1)
    close(z, ref.cpu())


@pytest.mark.parametrize("b,h,cin,cout,tile,splits", [(3, 8, 1280, 1280, 52, 2), (3, 4, 128, 64, 51, 1), (3, 16, 1280, 1280, 54, 1), (1, 32, 640, 640, 53, 1), (2, 8, 192, 96, 54, 3)])
def test_conv3x3_weight_streaming_upsample(ops, b, h, cin, cout, tile, splits):
    """convws_kernel over the nearest-2x upsample of the stored input (the Upsample2D conv): only the patch DMA's addresses change."""
    x = rnd(b, h, h, cin, seed=73)
    wt = rnd(cout, cin, 3, 3, seed=74, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(75))
    xin = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    wf = wt.float().cuda()
    got = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, upsample=True, bias=bias.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile, splits=splits)
    close(got, ref)


@pytest.mark.parametrize("b,h,cin,cin2,cout,tile,splits", [(3, 8, 1280, 2560, 1280, 51, 5), (3, 8, 128, 64, 96, 51, 1), (6, 8, 320, 448, 320, 51, 2),
                                                           (3, 16, 1280, 1920, 1280, 52, 2), (1, 16, 64, 320, 64, 52, 1), (2, 16, 640, 640, 100, 52, 3),
                                                           (3, 16, 1280, 2560, 1280, 53, 2), (1, 64, 320, 960, 320, 53, 1), (2, 32, 128, 192, 96, 53, 1),
                                                           (3, 16, 1280, 2560, 1280, 54, 2), (1, 64, 320, 960, 320, 54, 1), (2, 32, 128, 192, 96, 54, 1)])
def test_conv3x3_weight_streaming_fused_shortcut(ops, b, h, cin, cin2, cout, tile, splits):
    """convws_kernel with the ResBlock's 1x1 shortcut: its dense blocks go from memory straight into the B-operand registers, their
    weight fragments follow the 3x3 fragments; every K-slice takes its share of both ranges (block counts that 3 does not divide)."""
    t, x = rnd(b, h, h, cin, seed=64), rnd(b, h, h, cin2, seed=65)
    w3 = rnd(cout, cin, 3, 3, seed=66, scale=(9 * cin) ** -0.5)
    w1 = rnd(cout, cin2, 1, 1, seed=67, scale=cin2 ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(68))
    ref = F.conv2d(t.float().permute(0, 3, 1, 2), w3.float(), bias, padding=1) + F.conv2d(x.float().permute(0, 3, 1, 2), w1.float())
    wp = torch.cat([ops.pack_conv(w3.float().cuda())[:, : 9 * cin], ops.pack_conv(w1.float().cuda())[:, :cin2]], dim=1).contiguous()
    got = ops.conv3x3(t.cuda(), wp, cout, bias=bias.cuda(), tail=x.cuda(), wfr=ops.pack_conv_ws(w3.float().cuda(), w1.float().cuda()), tile=tile, splits=splits)
    close(got, ref.permute(0, 2, 3, 1))


@pytest.mark.parametrize("b,h,cin,cin2,cout,variant,splits", [(2, 16, 64, 128, 64, 12, 1), (3, 8, 320, 640, 320, 14, 1), (1, 16, 128, 64, 256, 13, 3),
                                                              (3, 8, 1280, 2560, 1280, 15, 7), (2, 32, 320, 960, 320, 12, 2),
                                                              (3, 8, 320, 640, 320, 48, 1), (3, 8, 1280, 2560, 1280, 49, 7), (6, 16, 320, 640, 640, 49, 3)])
def test_conv3x3_halo_fused_shortcut(ops, b, h, cin, cin2, cout, variant, splits):
    """Halo kernel with the ResBlock's 1x1 shortcut appended as dense k-blocks; split-K cuts the k-block sequence anywhere."""
    t, x = rnd(b, h, h, cin, seed=44), rnd(b, h, h, cin2, seed=45)
    w3 = rnd(cout, cin, 3, 3, seed=46, scale=(9 * cin) ** -0.5)
    w1 = rnd(cout, cin2, 1, 1, seed=47, scale=cin2 ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(48))
    ref = F.conv2d(t.float().permute(0, 3, 1, 2), w3.float(), bias, padding=1) + F.conv2d(x.float().permute(0, 3, 1, 2), w1.float())
    w1p = ops.pack_conv(w1.float().cuda())[:, :cin2]
    wp = torch.cat([ops.pack_conv(w3.float().cuda())[:, : 9 * cin], w1p], dim=1).contiguous()
    wcb = torch.cat([ops.pack_conv_cb(w3.float().cuda()), w1p], dim=1).contiguous()
    got = ops.conv3x3(t.cuda(), wp, cout, bias=bias.cuda(), tail=x.cuda(), wcb=wcb, tile=variant, splits=splits)
    close(got, ref.permute(0, 2, 3, 1))


def test_conv3x3_strided_view_and_f32_out(ops):
    """Input is a channel slice of a wider NHWC buffer (lda > Cin); output fp32."""
    from diffusiontexturepainting_amd._lib import GF_OUT_F32
    b, h, w, cin, cout = 2, 8, 8, 64, 4
    big = rnd(b, h, w, 192, seed=30).cuda()
    x = big[..., 64:128]
    wt = rnd(cout, cin, 3, 3, seed=31, scale=(9 * cin) ** -0.5)
    ref = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), wt.float(), None, padding=1).permute(0, 2, 3, 1)
    got = ops.conv3x3(x, ops.pack_conv(wt.float().cuda()), cout, flags=GF_OUT_F32)
    assert got.dtype == torch.float32
    close(got, ref, tol=1e-3)


@pytest.mark.parametrize("tile", [53, 54])
def test_conv_epilogue_statistics_with_a_large_output_mean(ops, tile):
    """GF_GNSTATS with conv outputs whose group means are ~150 standard deviations away from zero (a large bias): the statistics the
    epilogue emits -- fp64 from the lane butterflies on since round 6 -- must still give the GroupNorm of the STORED tensor (fp64 reference
    on the fp16 conv output)."""
    b, h, cin, cout = 2, 32, 128, 320
    x = rnd(b, h, h, cin, seed=183)
    wt = rnd(cout, cin, 3, 3, seed=184, scale=(9 * cin) ** -0.5)
    g = torch.Generator().manual_seed(185)
    bias = 150.0 * (1 + 0.1 * torch.rand(32, generator=g)).repeat_interleave(cout // 32)
    wf = wt.float().cuda()
    y, st = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile, splits=1, gn_groups=32)
    gamma, beta = (1 + 0.2 * torch.randn(cout, generator=g)).cuda(), (0.2 * torch.randn(cout, generator=g)).cuda()
    z = ops.groupnorm_apply(y, gamma, beta, st, eps=1e-5, silu=False)
    yd = y.double().cpu()
    assert 50 < (yd.mean() / yd.reshape(b, -1, 32, cout // 32).std(dim=(1, 3)).mean()).item()  # the case is what it says
    ref = F.group_norm(yd.permute(0, 3, 1, 2), 32, gamma.double().cpu(), beta.double().cpu(), eps=1e-5).permute(0, 2, 3, 1)
    err = (z.double().cpu() - ref).abs().max().item()
    print("conv-epilogue statistics, large mean: max abs err", err)
    assert err <= 6e-3


@pytest.mark.parametrize("b,hw,c,silu,eps", [(3, 64, 320, True, 1e-5), (2, 256, 640, False, 1e-6), (1, 1024, 128, True, 1e-6),
                                             (2, 16, 1920, True, 1e-5), (1, 100, 2560, True, 1e-5), (2, 64, 256, True, 1e-6),
                                             (1, 64, 512, False, 1e-6), (3, 4, 960, True, 1e-5), (1, 4096, 320, True, 1e-5),
                                             (2, 2048, 128, True, 1e-6), (1, 1600, 640, False, 1e-5)])
def test_groupnorm(ops, b, hw, c, silu, eps):
    x = rnd(b, hw, c, seed=40) * 2 + 0.5
    g = torch.Generator().manual_seed(41)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, gamma, beta, eps).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    got = ops.groupnorm(x.cuda(), gamma.cuda(), beta.cuda(), eps=eps, silu=silu)
    close(got, ref)


# |group mean| / group sigma -> allowed max abs error of the normalised output (|y| <= ~4; one fp16 step there is 2e-3..4e-3)
GN_LARGE_MEAN_BOUNDS = {0: 3e-3, 50: 3e-3, 300: 1.5e-2}


@pytest.mark.parametrize("k", [0, 50, 300])
@pytest.mark.parametrize("b,hw,c", [(3, 4096, 320), (3, 1024, 640), (3, 256, 1280), (3, 64, 1280), (1, 16384, 128)])
def test_groupnorm_large_group_means(ops, b, hw, c, k):
    """Round-5 verdict: every GroupNorm variance in norm.hip was E[x^2] - mean^2 from fp32 sums and no test fed |mean| >> sigma.  Inputs
    whose 32 group means are k sigma (k = 0 / 50 / 300, one sign) through the two-launch GroupNorm (statistics pass + apply), the
    single-launch form of the small maps and the reduce-in-GroupNorm forms, against an fp64 reference on the same fp16 tensor.
    Measured with the fp32 sums of rounds 1-5 (profiles/r06_gn_large_mean_before.log): 3.7e-3 at 50 sigma, 7e-2 .. 1.1e-1 at 300 sigma, O(1) at
    1000 sigma.  Round 6: every sum above a thread's own few elements, the totals over the chunks and E[x^2] - mean^2 itself run in fp64 (and the
    element count is exact, not a rounded reciprocal): 2.1e-3 at 50 sigma (one fp16 step of the output), <= 9.3e-3 at 300 sigma, 1.2e-1 at 1000
    sigma (profiles/r06_gn_large_mean_after.log).  What is left at 300 sigma is the fp32 STORAGE of the per-chunk partial sums between the
    statistics and the apply launch (2^-24 of a sum of squares that is 9e4 x the variance); carrying those in two floats would remove it --
    not done: no GroupNorm input of these networks is expected to sit hundreds of group standard deviations away from zero."""
    sigma = 0.05
    g = torch.Generator().manual_seed(7 + k)
    grp_mean = k * sigma * (1 + 0.2 * torch.rand(32, generator=g))
    x = (grp_mean.repeat_interleave(c // 32) + sigma * torch.randn(b, hw, c, generator=g)).half()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    ref = F.group_norm(x.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1)
    got = ops.groupnorm(x.cuda(), gamma.cuda(), beta.cuda(), eps=1e-5, silu=False).double().cpu()
    part = torch.stack([x.float() * 0.5, x.float() * 0.5]).contiguous()  # the same tensor as two fp32 split-K slabs (exact halves)
    out, y = ops.reduce_groupnorm(part.cuda(), gamma.cuda(), beta.cuda(), silu=False)
    assert torch.equal(out.cpu(), x)
    e1, e2 = (got - ref).abs().max().item(), (y.double().cpu() - ref).abs().max().item()
    print(f"k={k} B={b} HW={hw} C={c}: groupnorm {e1:.2e}, reduce+groupnorm {e2:.2e}")
    assert e1 <= GN_LARGE_MEAN_BOUNDS[k] and e2 <= GN_LARGE_MEAN_BOUNDS[k]


@pytest.mark.parametrize("hw,c", [(4096, 320), (4096, 640), (1024, 1280), (4096, 960), (256, 1280), (16384, 128)])
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm_result_does_not_depend_on_the_batch(ops, hw, c, silu):
    """A sample must come out of the GroupNorm with the same BITS whatever the batch it sits in: the de-duplicated UNet prefix evaluates two
    of three branches and copies the third (test_deduplicated_prefix_is_bit_identical).  Round 5: gn_apply_kernel's grid -- and with it
    which inlined copy of its item code handled a pixel -- depends on the batch, and hipcc had fused the final multiply with the fp16
    conversion (v_fma_mixlo_f16: one rounding) in one copy and not in the others."""
    x1 = (rnd(1, hw, c, seed=47) * 2 + 0.5).cuda()
    g = torch.Generator().manual_seed(48)
    gamma, beta = (1 + 0.2 * torch.randn(c, generator=g)).cuda(), (0.2 * torch.randn(c, generator=g)).cuda()
    one = ops.groupnorm(x1, gamma, beta, eps=1e-5, silu=silu)
    for nb in (2, 3, 6, 24):
        y = ops.groupnorm(x1.repeat(nb, 1, 1).contiguous(), gamma, beta, eps=1e-5, silu=silu)
        for i in range(nb):
            assert torch.equal(y[i], one[0]), (nb, i, (y[i].float() - one[0].float()).abs().max().item())


@pytest.mark.parametrize("b,hw,c,splits,silu,bias,resid", [(3, 64, 1280, 8, True, True, False), (3, 256, 1280, 4, True, True, True),   # one launch (HW <= 256)
                                                           (3, 1024, 640, 2, True, True, False), (2, 1024, 640, 3, False, False, True),  # reduce rides in the
                                                           (1, 4096, 320, 2, True, True, True), (2, 1600, 960, 2, True, False, False)])  # statistics pass
def test_reduce_groupnorm(ops, b, hw, c, splits, silu, bias, resid):
    """The split-K reduce of a conv folded into the GroupNorm that consumes it: conv output = fp16(sum of slabs + bias + residual)
    BIT-exactly (the same fp32 additions in the same order), normalised tensor against torch on that rounded tensor."""
    g = torch.Generator().manual_seed(45)
    part = torch.randn(splits, b, hw, c, generator=g) * 0.7
    bv = torch.randn(c, generator=g) if bias else None
    rv = rnd(b, hw, c, seed=46) if resid else None
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    acc = part[0].clone()
    for z in range(1, splits):
        acc += part[z]
    if bias:
        acc += bv
    if resid:
        acc += rv.float()
    conv = acc.half()
    ref = F.group_norm(conv.float().permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    out, y = ops.reduce_groupnorm(part.cuda(), gamma.cuda(), beta.cuda(), bias=bv.cuda() if bias else None, resid=rv.cuda() if resid else None, silu=silu)
    assert torch.equal(out.cpu(), conv)
    close(y, ref)


@pytest.mark.parametrize("b,hw,cx,cskip,splits,bias,resid", [(3, 64, 1280, 1280, 5, True, True), (3, 256, 1280, 640, 4, True, False), (2, 256, 1280, 1280, 2, False, True),
                                                             (3, 16, 1280, 1280, 12, True, True), (1, 64, 640, 320, 3, True, False)])
def test_reduce_groupnorm_over_a_concatenation(ops, b, hw, cx, cskip, splits, bias, resid):
    """Round 5: the GroupNorm that opens an up-block ResBlock runs over the zero-copy concatenation [x | skip]; when x's producer was a
    split conv / Linear its reduce now rides in that GroupNorm (it used to be a launch of its own): the first Cx channels are summed from
    the slabs (+ bias, + residual) and written back BIT-exactly, the skip half is read in place, groups may straddle the seam
    (1280 + 640 channels: 60 per group)."""
    g = torch.Generator().manual_seed(145)
    c = cx + cskip
    part = torch.randn(splits, b, hw, cx, generator=g) * 0.7
    bv = torch.randn(cx, generator=g) if bias else None
    rv = rnd(b, hw, cx, seed=146) if resid else None
    skip = (rnd(b, hw, cskip, seed=147).float() * 1.3 + 0.2).half()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    acc = part[0].clone()
    for z in range(1, splits):
        acc += part[z]
    if bias:
        acc += bv
    if resid:
        acc += rv.float()
    cat = torch.cat([acc.half(), skip], dim=-1)
    ref = F.silu(F.group_norm(cat.float().permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1))
    out, y = ops.reduce_groupnorm(part.cuda(), gamma.cuda(), beta.cuda(), bias=bv.cuda() if bias else None, resid=rv.cuda() if resid else None, silu=True,
                                  skip=skip.cuda())
    assert torch.equal(out.cpu(), cat)
    close(y, ref)


@pytest.mark.parametrize("b,hw,c,n", [(3, 4096, 320, 320), (2, 1024, 640, 640), (1, 1024, 1280, 1280), (2, 1600, 960, 320)])
def test_groupnorm_folded_into_linear(ops, b, hw, c, n):
    """proj_in(GroupNorm(x)) as a grouped GEMM on the RAW x with per-sample weights W diag(gamma rstd_b) and biases b + W (beta - mean_b
    rstd_b gamma): statistics pass + fold kernel + the grouped GEMM against torch (x carries a per-channel offset: the fold has to
    cancel the group means through the bias term)."""
    from diffusiontexturepainting_amd._lib import GF_BIAS
    g = torch.Generator().manual_seed(47)
    x = (rnd(b, hw, c, seed=48).float() * 1.5 + 0.8 * torch.randn(c, generator=g)).half()
    w = rnd(n, c, seed=49, scale=c ** -0.5).float()
    bias = 0.1 * torch.randn(n, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    ref = F.linear(F.group_norm(x.float().permute(0, 2, 1), 32, gamma, beta, 1e-6).permute(0, 2, 1), w, bias)
    wp = ops.pack_linear(w.cuda())
    wf, bf = ops.gn_fold_weights(x.cuda(), wp, n, bias.cuda(), gamma.cuda(), beta.cuda())
    got = ops.gemm(x.cuda().view(b * hw, c), wf.view(-1, wf.shape[-1]), n, c, bias=bf.view(-1), flags=GF_BIAS, batch=b)
    close(got.view(b, hw, n), ref, tol=4e-3)


@pytest.mark.parametrize("b,hw,c,n,ranges", [(3, 4096, 320, 320, 5), (3, 1024, 640, 640, 4), (2, 1024, 320, 320, 1), (1, 256, 640, 640, 10),
                                              (8, 128, 320, 320, 3), (3, 1024, 640, 320, 2)])
def test_groupnorm_applied_on_the_resident_fragments_of_the_linear(ops, b, hw, c, n, ranges):
    """Round 6: proj_in(GroupNorm(x)) WITHOUT per-sample folded weights -- lnlin_kernel<.., GNA> normalises its resident activation fragments
    from the statistics partials (fp32 fma per element, as gn_apply_kernel) and streams the shared weight matrix: statistics pass + one
    launch.  Against torch in fp32 (x carries per-channel offsets and a group mean of several sigma), against the two-step path
    GroupNorm launch -> plain Linear (bit-identical: same statistics, same per-element arithmetic, same MFMA order), and the row
    statistics it emits for the LayerNorm-folded q / k / v projection."""
    g = torch.Generator().manual_seed(147)
    x = (rnd(b, hw, c, seed=148).float() * 1.5 + 0.8 * torch.randn(c, generator=g) + 3.0).half()
    w = rnd(n, c, seed=149, scale=c ** -0.5).float()
    bias = 0.1 * torch.randn(n, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    ref = F.linear(F.group_norm(x.float().permute(0, 2, 1), 32, gamma, beta, 1e-6).permute(0, 2, 1), w, bias)
    wp = ops.pack_linear(w.cuda())
    got, st = ops.gn_linear(x.cuda(), wp, n, bias.cuda(), gamma.cuda(), beta.cuda(), col_ranges=ranges, row_stats=True)
    close(got, ref, tol=4e-3)
    if hw >= 1024:  # (below, GroupNorm alone is the single-launch kernel, whose per-element arithmetic is (x - mean) rstd gamma + beta)
        from diffusiontexturepainting_amd._lib import GF_BIAS
        xn = ops.groupnorm(x.cuda(), gamma.cuda(), beta.cuda(), eps=1e-6, silu=False)
        two = ops.gemm(xn.view(b * hw, c), wp, n, c, bias=bias.cuda(), flags=GF_BIAS, tile=50, splits=ranges)
        assert torch.equal(got.view(b * hw, n), two)
    gf = got.float().view(b * hw, n).cpu()
    tot = st.sum(dim=0).cpu()
    assert torch.allclose(tot[:, 0], gf.sum(dim=1), rtol=1e-4, atol=1e-2) and torch.allclose(tot[:, 1], (gf * gf).sum(dim=1), rtol=1e-4, atol=1e-2)


def _slabs_sum(b, hw, c, splits, bias, resid, seed):
    """split-K slabs (+ bias, + residual) of a conv output and fp16(their sum), the fp32 additions in the kernels' order"""
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(splits, b, hw, c, generator=g) * 0.7
    bv = torch.randn(c, generator=g) if bias else None
    rv = rnd(b, hw, c, seed=seed + 1) if resid else None
    acc = part[0].clone()
    for z in range(1, splits):
        acc += part[z]
    if bias:
        acc += bv
    if resid:
        acc += rv.float()
    return part, bv, rv, acc.half()


def _gn_ref(x, gamma, beta, eps=1e-5, groups=32):
    return F.group_norm(x.float().permute(0, 2, 1), groups, gamma, beta, eps).permute(0, 2, 1)


@pytest.mark.parametrize("b,hw,c,splits,bias,resid", [(2, 1024, 320, 2, True, True),    # base
                                                      (1, 1000, 640, 3, False, True),   # 15 chunks of 67 pixels, the last one short
                                                      (3, 16, 1280, 4, True, False),    # one chunk, the thread-row clamp
                                                      (2, 64, 128, 0, False, False)])   # no slabs, 4 channels per group
def test_groupnorm_stats_with_reduce_then_apply(ops, b, hw, c, splits, bias, resid):
    """What gn_linear / gn_conv3 run on a claimed reduce: the statistics pass alone with the producer's split-K slabs as its source (it
    writes the conv output, BIT-exactly fp16(sum of slabs + bias + residual), and partial sums that outlive the launch), then the apply
    pass from those partials.  No slabs: the plain statistics pass."""
    g = torch.Generator().manual_seed(245)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    if splits:
        part, bv, rv, conv = _slabs_sum(b, hw, c, splits, bias, resid, seed=246)
        out, y = ops.groupnorm_stats_apply(gamma.cuda(), beta.cuda(), part=part.cuda(), bias=bv.cuda() if bias else None, resid=rv.cuda() if resid else None)
    else:
        conv = rnd(b, hw, c, seed=246) * 2 + 0.5
        out, y = ops.groupnorm_stats_apply(gamma.cuda(), beta.cuda(), x=conv.cuda())
    assert torch.equal(out.cpu(), conv)
    close(y, _gn_ref(conv, gamma, beta))


def test_groupnorm_launchers_refuse_what_they_do_not_take(ops):
    """The acceptance set of every GroupNorm launcher, pinned from both sides: a shape just outside it raises (DTP_ERR_ARG before any launch),
    its neighbour inside -- a shape of the tests above, 32 groups -- still runs.  (A residual pitch that is no multiple of 8 cannot be
    expressed through reduce_groupnorm(): the wrapper's residual has the pitch of the slabs.)"""
    from diffusiontexturepainting_amd._lib import DtpError
    g = torch.Generator().manual_seed(345)

    def affine(c):
        return (1 + 0.2 * torch.randn(c, generator=g)).cuda(), (0.2 * torch.randn(c, generator=g)).cuda()

    def x16(b, hw, c):
        return (rnd(b, hw, c, seed=346) * 2 + 0.5).cuda()

    for c, groups in [(48, 8), (36, 9), (520, 65), (320, 7)]:  # 6 channels per group; C % 8; more than 64 groups; C % groups
        with pytest.raises(DtpError):
            ops.groupnorm(x16(1, 64, c), *affine(c), groups=groups)
    x, (gamma, beta) = x16(1, 1024, 128), affine(128)  # 4 channels per group
    close(ops.groupnorm(x, gamma, beta), _gn_ref(x.cpu(), gamma.cpu(), beta.cpu()))

    x, (gamma, beta) = x16(2, 256, 640), affine(640)
    xf = x.float().view(2, 256, 32, 20)
    partial = torch.stack([xf.sum(dim=(1, 3)), (xf * xf).sum(dim=(1, 3))], dim=-1).view(2, 1, 32, 2).contiguous()
    with pytest.raises(DtpError):  # the apply pass keeps the statistics of at most 32 groups
        ops.groupnorm_apply(x16(1, 64, 512), *affine(512), torch.zeros(1, 1, 64, 2, device="cuda"), groups=64)
    with pytest.raises(DtpError):  # no partials
        ops.groupnorm_apply(x, gamma, beta, partial[:, :0])
    close(ops.groupnorm_apply(x, gamma, beta, partial), _gn_ref(x.cpu(), gamma.cpu(), beta.cpu()))

    part, _, _, front = _slabs_sum(1, 1024, 640, 2, False, False, seed=347)
    with pytest.raises(DtpError):  # a concatenation outside the single-launch shapes
        ops.reduce_groupnorm(part.cuda(), *affine(960), skip=x16(1, 1024, 320))
    part, _, _, front = _slabs_sum(1, 64, 640, 3, False, False, seed=347)
    skip, (gamma, beta) = x16(1, 64, 320), affine(960)
    out, y = ops.reduce_groupnorm(part.cuda(), gamma, beta, skip=skip)
    cat = torch.cat([front, skip.cpu()], dim=-1)
    assert torch.equal(out.cpu(), cat)
    close(y, _gn_ref(cat, gamma.cpu(), beta.cpu()))

    # the fold holds at most 2048 channels.  C = 2056 never reaches it through the wrapper: the statistics pass in front refuses 2056 % 32;
    # C = 2112 (66 per group) does: that statistics pass runs, then the fold launcher refuses
    for c in (2056, 2112):
        with pytest.raises(DtpError, match="groupnorm stats" if c == 2056 else "gn fold"):
            ops.gn_fold_weights(x16(1, 64, c), torch.zeros(128, c, dtype=torch.float16, device="cuda"), 128, None, *affine(c))
    x, (gamma, beta) = x16(2, 1024, 640), affine(640)
    w = rnd(640, 640, seed=348, scale=640 ** -0.5).float()
    wf, bf = ops.gn_fold_weights(x, ops.pack_linear(w.cuda()), 640, torch.zeros(640, device="cuda"), gamma, beta, eps=1e-5)
    from diffusiontexturepainting_amd._lib import GF_BIAS
    got = ops.gemm(x.view(2 * 1024, 640), wf.view(-1, wf.shape[-1]), 640, 640, bias=bf.view(-1), flags=GF_BIAS, batch=2)
    close(got.view(2, 1024, 640), F.linear(_gn_ref(x.cpu(), gamma.cpu(), beta.cpu()), w), tol=4e-3)

    with pytest.raises(DtpError):  # 6 channels per group (its accepted neighbours: test_groupnorm_stats_with_reduce_then_apply)
        ops.groupnorm_stats_apply(*affine(48), x=x16(1, 64, 48), groups=8)


@pytest.mark.parametrize("rows,c", [(1000, 320), (333, 640), (64, 1280), (14, 768), (5, 2048)])
def test_layernorm(ops, rows, c):
    x = rnd(rows, c, seed=50) * 1.5 + 0.3
    g = torch.Generator().manual_seed(51)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    ref = F.layer_norm(x.float(), (c,), gamma, beta, 1e-5)
    close(ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda()), ref)


def _attn_ref(q, k, v, heads):
    b, sq, c = q.shape
    d = c // heads
    qh, kh, vh = (t.float().view(b, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    a = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, dim=-1)
    return (a @ vh).transpose(1, 2).reshape(b, sq, c)


@pytest.mark.parametrize("b,sq,skv,heads,d", [(3, 256, 256, 8, 40), (2, 1024, 1024, 8, 80), (3, 64, 64, 8, 160),
                                              (3, 256, 14, 8, 40), (2, 100, 14, 8, 160), (2, 50, 50, 12, 64),
                                              (1, 9, 9, 4, 192), (3, 16, 16, 8, 160), (1, 4, 4, 8, 160), (1, 200, 130, 8, 80)])
def test_attention(ops, b, sq, skv, heads, d):
    c = heads * d
    q, k, v = rnd(b, sq, c, seed=60), rnd(b, skv, c, seed=61), rnd(b, skv, c, seed=62)
    ref = _attn_ref(q, k, v, heads)
    got = ops.attention(q.cuda(), k.cuda(), v.cuda(), heads)
    close(got, ref, tol=3e-3)


def test_attention_fused_qkv_views_and_peaked_softmax(ops):
    """q/k/v are column slices of one [B,S,3C] buffer; one key dominates each row (forces the
    online-softmax rescale path on a later tile)."""
    b, s, heads, d = 2, 192, 8, 40
    c = heads * d
    qkv = rnd(b, s, 3 * c, seed=70)
    qkv[:, 150, c:2 * c] *= 6.0  # a spike in tile 2 (keys 128..191)
    ref = _attn_ref(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], heads)
    g = qkv.cuda()
    got = ops.attention(g[..., :c], g[..., c:2 * c], g[..., 2 * c:], heads)
    close(got, ref, tol=3e-3)


def test_attention_eight_wave_workgroups_on_a_batched_launch(ops):
    """A launch with >= 8 x CUs 256-query blocks (here 130 samples x 8 heads x 2 blocks) takes the eight-wave build of the d = 40 kernel
    (one K / V^T tile staged for 256 queries); ragged last query block and last key tile, fused-buffer views, a dominant late key."""
    b, s, heads, d = 130, 500, 8, 40
    c = heads * d
    qkv = rnd(b, s, 3 * c, seed=75)
    qkv[:, 470, c:2 * c] *= 5.0
    ref = _attn_ref(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], heads)
    g = qkv.cuda()
    got = ops.attention(g[..., :c], g[..., c:2 * c], g[..., 2 * c:], heads)
    close(got, ref, tol=3e-3)


@pytest.mark.parametrize("b,sq,skv,heads,d", [(3, 4096, 4096, 8, 40), (3, 1024, 1024, 8, 80), (1, 200, 256, 8, 40), (2, 40, 128, 4, 80),
                                              (1, 1024, 1024, 5, 40), (2, 300, 640, 8, 80), (24, 256, 256, 8, 40), (130, 500, 512, 8, 40),
                                              (3, 256, 256, 8, 160), (3, 64, 64, 8, 160), (1, 200, 320, 8, 160), (2, 64, 128, 3, 160)])
def test_attention_dma_kernel(ops, b, sq, skv, heads, d):
    """attn_dma_kernel (round 5: K / V tiles by LDS-DMA, V^T fragments by ds_read_b64_tr_b16, the softmax shift in the MFMA's C operand):
    the UNet's level-0 / level-1 launches at batch 1, ragged query blocks, Sq != Skv, a (batch x heads) count that is not a multiple
    of 8 (the plain block -> (head, query block) map), short sequences (2 tiles: shorter than the DMA ring), many small problems, and a
    launch with >= 8 x CUs 256-query blocks (130 samples x 8 heads x 2: the eight-wave build, one K / V tile staged for 256 queries).
    The d = 160 cases exist only in a DTP_EXPERIMENTAL=1 build (the kernel brought nothing at levels 2-3) and skip otherwise.  The kernel is
    called through dtp_op_attention_dma: the stamp's dispatcher hands it sequences of >= 512 keys only (where it wins)."""
    if not ops.attention_dma_supported(sq, skv, heads, d):
        assert d == 160, "the product build takes d = 40 / 80 with whole 64-key tiles"
        pytest.skip("d = 160 on attn_dma_kernel: DTP_EXPERIMENTAL builds only")
    c = heads * d
    q, k, v = rnd(b, sq, c, seed=260), rnd(b, skv, c, seed=261), rnd(b, skv, c, seed=262)
    ref = _attn_ref(q, k, v, heads)
    got = ops.attention_dma(q.cuda(), k.cuda(), v.cuda(), heads)
    close(got, ref, tol=3e-3)


@pytest.mark.parametrize("nw", [4, 8])
@pytest.mark.parametrize("sq,skv", [(200, 128), (300, 192), (130, 192), (257, 128), (64, 192)])
def test_attention_dma_ragged_query_blocks_and_short_key_ranges_on_both_builds(ops, sq, skv, nw):
    """Round-5 advisor: Sq that is not a multiple of 128 / 256 (the last query block of the four- and of the eight-wave build is ragged:
    rows >= Sq are computed on clamped addresses and never stored) with Skv = 128 / 192 (2-3 key tiles: shorter than the DMA ring of four
    slots), d = 40 through BOTH builds.  At d = 40 the kernel over-reads the third K k-step / V columns 48..63 into the next key's
    row: the reference must still match (the over-read meets zero Q' columns), including for the LAST key (whose over-read leaves the tensor)."""
    b, heads, d = 2, 8, 40
    c = heads * d
    q, k, v = rnd(b, sq, c, seed=290), rnd(b, skv, c, seed=291), rnd(b, skv, c, seed=292)
    ref = _attn_ref(q, k, v, heads)
    got = ops.attention_dma(q.cuda(), k.cuda(), v.cuda(), heads, nw=nw)
    close(got, ref, tol=3e-3)


@pytest.mark.parametrize("d,s,spike_at,gain", [(40, 1024, 900, 6.0), (80, 512, 70, 5.0), (40, 256, 255, 8.0), (80, 1024, 0, 6.0), (160, 256, 200, 4.0),
                                               (160, 128, 40, 4.0)])
def test_attention_dma_reference_moves_late_and_peaked_rows(ops, d, s, spike_at, gain):
    """The rare branch of attn_dma_kernel: one key dominates every row from a LATER tile on (the reference moves there, O^T and the row
    sums are rescaled, the pending scores re-based), q / k / v as column slices of one fused buffer, queries scaled up so that the
    softmax is peaked (several moves per row).  Full-tensor fp32 reference; spike_at = 0: the dominant key sits in the first tile."""
    b, heads = 2, 8
    c = heads * d
    qkv = rnd(b, s, 3 * c, seed=270 + d)
    qkv[..., :c] *= 2.0
    qkv[:, spike_at, c:2 * c] *= gain
    ref = _attn_ref(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], heads)
    g = qkv.cuda()
    if not ops.attention_dma_supported(s, s, heads, d):
        assert d == 160
        pytest.skip("d = 160 on attn_dma_kernel: DTP_EXPERIMENTAL builds only")
    got = ops.attention_dma(g[..., :c], g[..., c:2 * c], g[..., 2 * c:], heads)
    close(got, ref, tol=3e-3)


def test_attention_dma_very_negative_and_very_positive_scores(ops):
    """Rows whose scores are all far below zero (the first tile must pull the reference DOWN onto the row maximum, or every P underflows)
    and rows whose scores are far above (no fp16 overflow of P): q is a multiple of one direction, k carries a large component along it."""
    b, s, heads, d = 1, 256, 8, 40
    c = heads * d
    g = torch.Generator().manual_seed(281)
    u = torch.randn(heads, d, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    q = (0.3 * torch.randn(b, s, heads, d, generator=g) + 6.0 * u)            # every query has a +6 component along u
    sign = torch.where(torch.arange(s) % 2 == 0, -1.0, 1.0).view(1, s, 1, 1)   # even QUERIES see strongly negative scores, odd ones positive
    q = q * sign
    k = (0.3 * torch.randn(b, s, heads, d, generator=g) + 8.0 * u)
    v = torch.randn(b, s, heads, d, generator=g)
    q, k, v = (t.reshape(b, s, c).half() for t in (q, k, v))
    ref = _attn_ref(q, k, v, heads)
    got = ops.attention_dma(q.cuda(), k.cuda(), v.cuda(), heads)
    close(got, ref, tol=3e-3)


def test_softmax_rows(ops):
    x = rnd(300, 4096, seed=80) * 3
    ref = torch.softmax(x.float() * 0.21, dim=-1)
    close(ops.softmax_rows(x.cuda(), 0.21), ref, tol=1e-3)


@pytest.mark.parametrize("m,n,k,tile", [(300, 320, 320, -1), (700, 640, 640, 0), (700, 640, 640, 20), (130, 1280, 320, 2), (513, 320, 1280, 20),
                                        (700, 640, 640, 32), (130, 1280, 320, 38), (513, 320, 1280, 35), (700, 640, 640, 40), (130, 1280, 320, 46)])
def test_gemm_row_statistics_feed_the_layernorm_fold(ops, m, n, k, tile):
    """Producer GEMM emits per-row (sum, sumsq) partials of its fp16 output (one per N tile); a LayerNorm-folded consumer
    that takes them must equal the consumer that computes the statistics itself -- and the fp32 LayerNorm reference."""
    a, w = rnd(m, k, seed=100), rnd(n, k, seed=101, scale=k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(102))
    r = rnd(m, n, seed=103)
    y, st = ops.gemm(a.cuda(), ops.pack_linear(w.float().cuda()), n, k, bias=bias.cuda(), resid=r.cuda(), tile=tile, row_stats=True)
    yf = y.float().cpu()
    tot = st.sum(dim=0).cpu()
    assert torch.allclose(tot[:, 0], yf.sum(dim=1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[:, 1], (yf * yf).sum(dim=1), rtol=1e-4, atol=1e-2)
    n2 = 384
    w2 = rnd(n2, n, seed=104, scale=n ** -0.5).float()
    g = torch.Generator().manual_seed(105)
    gamma, beta = 1 + 0.2 * torch.randn(n, generator=g), 0.2 * torch.randn(n, generator=g)
    ref = F.linear(F.layer_norm(yf, (n,), gamma, beta, 1e-5), w2)
    wp2 = ops.pack_linear((w2 * gamma[None]).cuda())
    lns = ops.rowsum(wp2, n)
    b2 = (w2 @ beta).cuda()
    for t2 in (-1, 20):
        own = ops.gemm(y, wp2, n2, n, bias=b2, lns=lns, tile=t2)
        fed = ops.gemm(y, wp2, n2, n, bias=b2, lns=lns, tile=t2, stats_in=st)
        close(own, ref, tol=3e-3)
        close(fed, ref, tol=3e-3)


def test_gemm_wide_large_asymmetric(ops):
    """Several 256-row tiles, ragged M and N tails, non-square: catches tile / wave-grid index mix-ups of the 8-wave kernels."""
    for tile, (m, n, k) in ((20, (1000, 776, 448)), (21, (1000, 968, 448)), (21, (2304, 320, 2880))):
        a, w = rnd(m, k, seed=110), rnd(n, k, seed=111, scale=k ** -0.5)
        bias = torch.randn(n, generator=torch.Generator().manual_seed(112))
        ref = F.linear(a.float(), w.float(), bias)
        got = ops.gemm(a.cuda(), ops.pack_linear(w.float().cuda()), n, k, bias=bias.cuda(), tile=tile)
        close(got, ref)


@pytest.mark.parametrize("b,s,skv,heads,d,q_scale,v_scale", [(2, 256, 256, 8, 40, 1.0, 1.0), (1, 1024, 1024, 8, 40, 2.0, 0.5), (2, 256, 256, 8, 80, 1.0, 1.0),
                                                          (1, 128, 64, 8, 160, 1.0, 2.0), (1, 200, 130, 4, 40, 1.0, 1.0), (1, 4096, 4096, 2, 40, 1.0, 1.0)])
def test_attention_fp8(ops, b, s, skv, heads, d, q_scale, v_scale):
    """fp8 (e4m3) MX-MFMA attention (BASELINE configs[4]).  Two references: the exact fp32 attention of the same f16 tensors
    (tolerance = what e4m3 operands cost on N(0,1) tensors -- 3 mantissa bits: the same contraction in fp32 on e4m3-rounded
    inputs is already 8.6e-2 of the output range away, mean 4.7e-2 -- so 1.2e-1) and the fp32 attention of the e4m3-ROUNDED q' / k' / v'
    (isolates the kernel from the input quantisation: what remains is the fp8 rounding of P, <= 4e-2 of the range)."""
    c = heads * d
    q, k, v = rnd(b, s, c, seed=160), rnd(b, skv, c, seed=161), rnd(b, skv, c, seed=162)
    ref = _attn_ref(q, k, v, heads)
    got = ops.attention_fp8(q.cuda(), k.cuda(), v.cuda(), heads, q_scale=q_scale, v_scale=v_scale).float().cpu()
    assert torch.isfinite(got).all()
    rng = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= 1.2e-1 * rng, (got - ref).abs().max().item() / rng
    e4 = torch.float8_e4m3fn
    log2e = 1.4426950408889634
    qq = (q.float() * (d ** -0.5 * log2e * q_scale)).to(e4).float() / (log2e * q_scale)  # what the kernel feeds the MFMA, rescaled
    kk = (k.float() / q_scale).to(e4).float() * q_scale
    vv = (v.float() / v_scale).to(e4).float() * v_scale
    qh, kh, vh = (t.view(b, -1, heads, d).transpose(1, 2) for t in (qq, kk, vv))
    ref8 = (torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh).transpose(1, 2).reshape(b, s, c)
    assert (got - ref8).abs().max().item() <= 4e-2 * rng + 2e-3, (got - ref8).abs().max().item() / rng


def _attn_ref_e4m3_inputs(q, k, v, heads):
    """fp32 attention of the e4m3-rounded operands the fp8 kernel feeds its MFMAs (unit scales)."""
    b, s, c = q.shape
    d = c // heads
    e4, log2e = torch.float8_e4m3fn, 1.4426950408889634
    qq = (q.float() * (d ** -0.5 * log2e)).to(e4).float() / log2e
    qh, kh, vh = (t.view(b, -1, heads, d).transpose(1, 2) for t in (qq, k.float().to(e4).float(), v.float().to(e4).float()))
    return (torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh).transpose(1, 2).reshape(b, s, c)


def test_attention_fp8_peaked_rows_and_views(ops):
    """q/k/v as column slices of one buffer; a dominant key late in the sequence forces the reference move (rescale path)."""
    b, s, heads, d = 2, 320, 8, 40
    c = heads * d
    qkv = rnd(b, s, 3 * c, seed=170)
    qkv[:, 300, c:2 * c] *= 5.0
    ref = _attn_ref(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], heads)
    g = qkv.cuda()
    got = ops.attention_fp8(g[..., :c], g[..., c:2 * c], g[..., 2 * c:], heads).float().cpu()
    # against exact fp32 a dominant score magnifies the e4m3 rounding of q and k (5 % of a score of ~15 in the exp2 domain):
    # only a sanity bound; the sharp check is against the same contraction on the e4m3-rounded operands
    assert torch.isfinite(got).all() and (got - ref).abs().max().item() <= 2.5e-1 * ref.abs().max().item()
    ref8 = _attn_ref_e4m3_inputs(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], heads)
    assert (got - ref8).abs().max().item() <= 5e-2 * ref8.abs().max().item()
    from diffusiontexturepainting_amd._lib import DtpError
    with pytest.raises(DtpError):  # d = 64 has no spare contraction column for the shift: loud, not silent
        ops.attention_fp8(rnd(1, 64, 512, seed=1).cuda(), rnd(1, 64, 512, seed=2).cuda(), rnd(1, 64, 512, seed=3).cuda(), 8)


def _e4(t, scale=1.0):
    """what the kernels feed the fp8 MFMA: e4m3(t / scale), dequantised back to fp32"""
    return (t.float() / scale).to(torch.float8_e4m3fn).float() * scale


@pytest.mark.parametrize("m,n,k,tile", [(300, 320, 320, 24), (700, 640, 1280, 24), (130, 1280, 320, 26), (64, 768, 768, 27), (513, 320, 1280, 25),
                                        (200, 320, 400, 26), (700, 640, 1280, 28), (300, 320, 320, 28)])
def test_gemm_fp8(ops, m, n, k, tile):
    """fp8 (e4m3) GEMM on the MX MFMA (configs[4]): the products of e4m3 operands are exact in the fp32 accumulator, so against the
    same contraction on the e4m3-rounded operands only the summation order differs (2e-3); against exact fp32 it is the
    operand rounding (3 mantissa bits each: a few percent of the output range)."""
    a, w = rnd(m, k, seed=201), rnd(n, k, seed=202, scale=k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(203))
    r = rnd(m, n, seed=204)
    wp = ops.pack_linear(w.float().cuda())
    w8, ws = ops.quantize_w8(wp, k)
    assert ws > 0 and abs(math.log2(ws) - round(math.log2(ws))) < 1e-6  # a power of two
    assert (w.float().abs().max() / ws) <= 448 and (w.float().abs().max() / ws) > 112  # the tensor uses the top of the range
    got = ops.gemm(a.cuda(), wp, n, k, bias=bias.cuda(), resid=r.cuda(), tile=tile, w8=w8, w_scale=ws)
    ref8 = F.linear(_e4(a), _e4(w, ws), bias) + r.float()
    close(got, ref8, tol=2e-3)
    ref = F.linear(a.float(), w.float(), bias) + r.float()
    assert (got.float().cpu() - ref).abs().max().item() <= 6e-2 * ref.abs().max().item()


def test_gemm_fp8_layernorm_geglu_and_two_operands(ops):
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    # (1) LayerNorm applied while A is staged (consumer of a residual stream with a large mean), GEGLU epilogue
    m, c = 300, 320
    x = rnd(m, c, seed=210) * 1.5 + 6.0
    w = rnd(8 * c, c, seed=211, scale=c ** -0.5).float()
    g = torch.Generator().manual_seed(212)
    gamma, beta, bias = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(8 * c, generator=g)
    wg = w * gamma[None]
    b2 = bias + w @ beta
    f = torch.arange(4 * c)
    perm = torch.empty(8 * c, dtype=torch.long)
    perm[f] = (f // 64) * 128 + f % 64
    perm[4 * c + f] = (f // 64) * 128 + 64 + f % 64
    bp = torch.empty_like(b2)
    bp[perm] = b2
    wp = ops.pack_linear(wg.cuda(), geglu=True)
    w8, ws = ops.quantize_w8(wp, c)
    got = ops.gemm(x.cuda(), wp, 8 * c, c, bias=bp.cuda(), flags=GF_GEGLU | GF_BIAS, tile=24, w8=w8, w_scale=ws, layernorm=True)
    wide = ops.gemm(x.cuda(), wp, 8 * c, c, bias=bp.cuda(), flags=GF_GEGLU | GF_BIAS, tile=28, w8=w8, w_scale=ws, layernorm=True)
    assert (wide.float() - got.float()).abs().max().item() <= 2e-3 * got.float().abs().max().item() + 2e-3  # 8-wave tile: same operands
    xn = F.layer_norm(x.float(), (c,), None, None, 1e-5)
    h8 = F.linear(_e4(xn), _e4(wg, ws), b2)
    a8, g8 = h8.chunk(2, dim=-1)
    # the kernel's fp32 (x - mean) * rstd and torch's layer_norm differ in the last bits, and a value that sits on an e4m3
    # rounding boundary then lands on the neighbouring code (6 % of that element): not bit-comparable like the plain case
    close(got, a8 * F.gelu(g8), tol=2.5e-2)
    h = F.linear(F.layer_norm(x.float(), (c,), gamma, beta, 1e-5), w, bias)
    ref = h[:, : 4 * c] * F.gelu(h[:, 4 * c:])
    assert (got.float().cpu() - ref).abs().max().item() <= 8e-2 * ref.abs().max().item()
    # (2) [f | r] . [W1 | W2]^T with f and r in separate buffers (ff.net.2 + proj_out), + row statistics of the output
    m, k1, k2, n = 260, 1280, 320, 320
    fa, rb = rnd(m, k1, seed=213), rnd(m, k2, seed=214)
    w = rnd(n, k1 + k2, seed=215, scale=(k1 + k2) ** -0.5)
    res = rnd(m, n, seed=216)
    wp = ops.pack_linear(w.float().cuda())
    w8, ws = ops.quantize_w8(wp, k1 + k2)
    got28 = ops.gemm(fa.cuda(), wp, n, k1, resid=res.cuda(), tail=rb.cuda(), tile=28, w8=w8, w_scale=ws)
    got, st = ops.gemm(fa.cuda(), wp, n, k1, resid=res.cuda(), tail=rb.cuda(), tile=26, w8=w8, w_scale=ws, row_stats=True)
    assert (got28.float() - got.float()).abs().max().item() <= 2e-3 * got.float().abs().max().item() + 2e-3
    ref8 = F.linear(torch.cat([_e4(fa), _e4(rb)], dim=1), _e4(w, ws)) + res.float()
    close(got, ref8, tol=2e-3)
    tot = st.sum(dim=0).cpu()
    assert torch.allclose(tot[:, 0], got.float().cpu().sum(dim=1), rtol=1e-4, atol=1e-2)
