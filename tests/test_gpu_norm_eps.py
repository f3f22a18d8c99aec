"""eps and the low-variance edge of every normalisation kernel.

About sixteen sites compute rsqrt(max(var, 0) + eps): norm.hip (the GroupNorm launchers, layernorm_kernel) and the finalise helper of common.h,
the LayerNorm folds of gemm_conv / gemm_wide / gemm_ws / gemm_fp8 / gemm_f8f8 (the quantiser) / lnlin, xattn / xchain / ffchain, the
GroupNorm folded into a Linear (gn_fold_weights, gn_linear) and the GroupNorm applied from conv-emitted statistics.  Every other op test feeds
rows or groups with a variance between 2.5e-3 and 4: there eps moves the output by less than one fp16 step, so a launcher that drops its eps
argument, hard-codes the other constant or reads it from the wrong field passes all of them -- and no test reaches the max(var, 0) clamp.

Inputs here: grid() = round(N(0, 1) * 16) * 2^-12 as fp16.  Every value is 0 or a NORMAL fp16 number (nothing depends on how a kernel
treats fp16 subnormals), the mean is ~0 (nothing for E[x^2] - mean^2 to cancel: this is not a large-mean test) and the row / group variance
is ~1.5e-5, between the two eps values the networks use (1e-5, 1e-6).  A float64 reference with the other eps is then 0.8 .. 1.2 away, one
with eps = 0 in place of 1e-6 0.15 .. 0.19, while the fp32 restatement of the kernels' own formula stays within 2e-3
(test_grid_inputs_see_the_eps_that_gaussian_inputs_hide, which needs no device).  Tolerances are the ones each path has in test_gpu_ops.py;
only the inputs are new.  Every case runs eps = 1e-5, then 1e-6, on the same tensors in one test body (a launcher that caches or ignores
eps fails one of the two), and before it runs it asserts that its own float64 references for the two eps are at least 3x its limit apart.

Degenerate rows / groups ride in the same launches: an all-zero row, constant rows 0.5 and -3, a row with a single 2^-12, a row of ordinary
N(0, 1) data between grid rows (a row's statistics must not depend on its neighbours in the tile); for GroupNorm one sample with an all-zero
group, a constant group 0.5 and an ordinary group.  Constant rows / groups must come out as beta (for the folds: bias + W beta).

NOT covered: the eps CONSTANTS the launch builder hard-codes per site -- 1e-5 in the UNet ResNet GroupNorms and in every LayerNorm
(unet.hip, builder.hip: Builder::layernorm and the ln_eps of the folded q/k/v, FF1, cross-attention and chain launches), 1e-6 in the
transformer's GroupNorm (gn_linear / gn_fold_weights in unet.hip) and in all of the VAE (vae.hip).  Seeing those needs a weight set with a
small residual stream and an oracle with a switchable eps.  Also out of scope: large row or group means, attention.

ops.gemm(..., layernorm=True) on the fp8 tiles, ops.quant_e4m3, ops.xattn / xchain / ffchain all take their eps at the op level; lnlin_kernel
(tile 50) with GF_LNFOLD ignores stats_in by design (statistics from its resident fragments), so it has the in-kernel form only.

Run time on one MI355X: see RUN_TIME below.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_fp8_operands import e4_bytes, ordinal
from test_gpu_ops import close, needs_experimental_build, ops, rnd  # noqa: F401  (ops: the module-scoped fixture)

RUN_TIME = ("this file on one MI355X: 39 GPU cases plus the three CPU tests in 3.0 s (2.8 .. 3.2 s over five runs); the weight-streaming fold case "
            "(tile 55) skips outside DTP_EXPERIMENTAL builds and has NOT been run on a device: unverified (gemm_ws.hip keeps its epilogue in fp32); the GPU suite was last recorded at 1 084 s of its 1 200 s limit (VERDICT.md), so the file adds "
            "0.3 % -- under the 1 % at which its tile lists would have to be thinned")

gpu = pytest.mark.gpu

EPS = (1e-5, 1e-6)  # in this order, on the same tensors
LN_SHAPES = [(64, 320), (14, 768), (5, 2048)]
GN_SHAPES = [(2, 64, 320), (1, 1024, 128), (3, 4, 960)]  # single launch (HW <= 256), two launches, 30 channels per group in slabs of four groups
ZERO_ROW, HALF_ROW, MINUS3_ROW, SINGLE_ROW, NORMAL_ROW = 1, 3, 5, 7, 9
CONST_ROWS = [ZERO_ROW, HALF_ROW, MINUS3_ROW]
ZERO_GROUP, HALF_GROUP, NORMAL_GROUP = 1, 3, 5  # of sample 0


# ---------------------------------------------------------------- inputs
def grid(shape, seed, steps=16):
    """round(N(0, 1) * steps) * 2^-12 as fp16: multiples of 2^-12 (zero or normal fp16), mean ~0, variance ~steps^2 * 2^-24 = 1.5e-5"""
    g = torch.Generator().manual_seed(seed)
    return (torch.round(torch.randn(*shape, generator=g) * steps) * 2.0 ** -12).half()


def rows_mix(m, c, seed):
    """grid rows with the degenerate rows between them (m >= 10)"""
    x = grid((m, c), seed)
    x[ZERO_ROW] = 0
    x[HALF_ROW] = 0.5
    x[MINUS3_ROW] = -3.0
    x[SINGLE_ROW] = 0
    x[SINGLE_ROW, c // 3] = 2.0 ** -12
    x[NORMAL_ROW] = rnd(c, seed=seed + 1000)
    return x


def gn_mix(b, hw, c, seed, groups=32):
    """grid samples [B, HW, C]; sample 0 has an all-zero group, a constant group and an ordinary one"""
    x = grid((b, hw, c), seed)
    cpg = c // groups
    x[0, :, ZERO_GROUP * cpg:(ZERO_GROUP + 1) * cpg] = 0
    x[0, :, HALF_GROUP * cpg:(HALF_GROUP + 1) * cpg] = 0.5
    x[0, :, NORMAL_GROUP * cpg:(NORMAL_GROUP + 1) * cpg] = rnd(hw, cpg, seed=seed + 1000)
    return x


def affine(c, seed, n=0):
    """gamma, beta (and a bias of n entries) as the op tests draw them, fp32"""
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    return (gamma, beta, 0.1 * torch.randn(n, generator=g)) if n else (gamma, beta)


# ---------------------------------------------------------------- references (float64) and the comparison
def ln64(x, gamma, beta, eps):
    c = x.shape[-1]
    return F.layer_norm(x.double(), (c,), None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)


def gn64(x, gamma, beta, eps, silu=False, groups=32):
    y = F.group_norm(x.double().transpose(1, 2), groups, gamma.double(), beta.double(), eps).transpose(1, 2)
    return F.silu(y) if silu else y


def geglu(h):
    a, gate = h.chunk(2, dim=-1)
    return a * F.gelu(gate)


def geglu_pack(v):
    """a per-output-row vector in the [a | gate] row packing of pack_linear(geglu=True)"""
    n = v.numel()
    f = torch.arange(n // 2)
    perm = torch.empty(n, dtype=torch.long)
    perm[f] = (f // 64) * 128 + f % 64
    perm[n // 2 + f] = (f // 64) * 128 + 64 + f % 64
    out = torch.empty_like(v)
    out[perm] = v
    return out


def limit(ref, tol):
    """the bound close() applies"""
    return tol * ref.abs().max().item() + tol


def two_refs(ref, tol, factor=3.0):
    """{eps: float64 reference}; the premise of every case: the two are further apart than `factor` limits, so a kernel that used the other
    eps (or none: that is further still) cannot pass"""
    refs = {e: ref(e) for e in EPS}
    gap = (refs[EPS[0]] - refs[EPS[1]]).abs().max().item()
    lim = max(limit(r, tol) for r in refs.values())
    assert gap >= factor * lim, f"the case cannot tell its two eps apart: references {gap} apart, limit {lim}"
    return refs


def both_eps(run, ref, tol=2e-3, const=None):
    """run(eps) against ref(eps) for eps = 1e-5, then 1e-6; const = (index, want): that part of the output against `want` on its own limit"""
    refs = two_refs(ref, tol)
    for eps in EPS:
        got = run(eps)
        close(got, refs[eps], tol)
        if const is not None:
            index, want = const
            close(got[index], want.expand_as(refs[eps][index]), tol)


def kernel_formula_ln(x, gamma, beta, eps):
    """the kernels' own arithmetic in fp32: s1, s2 -> mean, var = max(s2 / K - mean^2, 0), rsqrt(var + eps); stored as fp16"""
    xf = x.float()
    k = xf.shape[-1]
    mean = xf.sum(-1, keepdim=True) / k
    var = ((xf * xf).sum(-1, keepdim=True) / k - mean * mean).clamp_min(0.0)
    return ((xf - mean) * torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32)) * gamma + beta).half()


def kernel_formula_gn(x, gamma, beta, eps, groups=32):
    b, hw, c = x.shape
    xf = x.float().view(b, hw, groups, c // groups)
    cnt = hw * (c // groups)
    mean = xf.sum(dim=(1, 3), keepdim=True) / cnt
    var = ((xf * xf).sum(dim=(1, 3), keepdim=True) / cnt - mean * mean).clamp_min(0.0)
    y = ((xf - mean) * torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))).view(b, hw, c)
    return (y * gamma + beta).half()


# ---------------------------------------------------------------- the cases: CPU data and float64 references (no device needed)
class Case:
    def __init__(self, ref, tol, **kw):
        self.ref, self.tol = ref, tol
        self.__dict__.update(kw)


def ln_case(rows, c):
    x = rows_mix(rows, c, seed=500) if rows >= 10 else grid((rows, c), seed=500)
    gamma, beta = affine(c, 501)
    return Case(lambda eps: ln64(x, gamma, beta, eps), 2e-3, x=x, gamma=gamma, beta=beta)


def gn_case(b, hw, c, silu=False, seed=510):
    x = gn_mix(b, hw, c, seed=seed)
    gamma, beta = affine(c, seed + 1)
    return Case(lambda eps: gn64(x, gamma, beta, eps, silu), 2e-3, x=x, gamma=gamma, beta=beta, silu=silu)


def gn_const(case):
    """(index, want) of the constant groups of sample 0: beta (through SiLU)"""
    cpg = case.x.shape[-1] // 32
    ch = torch.cat([torch.arange(g * cpg, (g + 1) * cpg) for g in (ZERO_GROUP, HALF_GROUP)])
    want = case.beta.double()[ch]
    return (0, slice(None), ch), (F.silu(want) if case.silu else want)


def gn_linear_case(b, hw, c, n):
    x = gn_mix(b, hw, c, seed=520)
    w = rnd(n, c, seed=521, scale=c ** -0.5).float()
    gamma, beta, bias = affine(c, 522, n)
    return Case(lambda eps: F.linear(gn64(x, gamma, beta, eps), w.double(), bias.double()), 4e-3, x=x, w=w, gamma=gamma, beta=beta, bias=bias)


def fold_case(m, c, n, is_geglu):
    """LN(x) W^T + b from the raw x: W carries gamma, the bias W.beta"""
    x = rows_mix(m, c, seed=530)
    w = rnd(n, c, seed=531, scale=c ** -0.5).float()
    gamma, beta, bias = affine(c, 532, n)
    act = geglu if is_geglu else (lambda h: h)
    b2 = bias + w @ beta
    return Case(lambda eps: act(F.linear(ln64(x, gamma, beta, eps), w.double(), bias.double())), 3e-3, x=x, w=w, gamma=gamma, beta=beta, bias=bias,
                b2=geglu_pack(b2) if is_geglu else b2, const=(CONST_ROWS, act(bias.double() + w.double() @ beta.double())))


def _e4(t, scale=1.0):
    """what the fp8 kernels feed the MFMA: e4m3(t / scale), dequantised"""
    return ((t.float() / scale).to(torch.float8_e4m3fn).float() * scale).double()


def fp8_case(m, c):
    """test_gemm_fp8_layernorm_geglu_and_two_operands (1): LayerNorm applied while A is staged, e4m3 operands, GEGLU epilogue; the reference
    contracts the e4m3-rounded operands (w_scale: the power of two quantize_w8 reports)"""
    n = 8 * c
    x = rows_mix(m, c, seed=540)
    w = rnd(n, c, seed=541, scale=c ** -0.5).float()
    gamma, beta, bias = affine(c, 542, n)
    wg = (w * gamma[None]).half().float()  # the packed fp16 weights
    b2 = bias + w @ beta
    guess = 2.0 ** math.ceil(math.log2(wg.abs().max().item() / 448.0))

    def ref(eps, w_scale=guess):
        return geglu(F.linear(_e4(ln64(x, None, None, eps)), _e4(wg, w_scale), b2.double()))

    return Case(ref, 2.5e-2, x=x, w=w, gamma=gamma, beta=beta, bias=bias, b2=geglu_pack(b2), const=(CONST_ROWS, geglu(b2.double())),
                exact=lambda eps: geglu(F.linear(ln64(x, gamma, beta, eps), w.double(), bias.double())))


def quant_case(m, k):
    x = rows_mix(m, k, seed=550)
    return Case(lambda eps: ln64(x, None, None, eps), None, x=x, scale=0.125)


def xattn_case(nb, s, c):
    """test_fused_cross_attention_pair_matches_the_two_gemms: scores GEMM (LayerNorm fold from the producer's statistics, softmax over 14 of 16
    columns per head) + value-output GEMM (bias, residual)"""
    g = torch.Generator().manual_seed(560)
    x = rows_mix(nb * s, c, seed=561)
    w1 = rnd(nb, 128, c, seed=562, scale=2.0 * c ** -0.5).float()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    b1 = 0.3 * torch.randn(nb, 128, generator=g)
    w2 = rnd(nb, c, 128, seed=563, scale=0.5).float()
    b2 = 0.2 * torch.randn(c, generator=g)
    xf = x.float()
    h = c // 2
    st_in = torch.stack([torch.stack([xf[:, :h].sum(1), (xf[:, :h] ** 2).sum(1)], dim=1), torch.stack([xf[:, h:].sum(1), (xf[:, h:] ** 2).sum(1)], dim=1)])

    def ref(eps):
        xn = ln64(x, gamma, beta, eps).view(nb, s, c)
        sc = (torch.einsum("bmc,bnc->bmn", xn, w1.double()) + b1.double()[:, None]).view(nb, s, 8, 16)
        pr = torch.zeros_like(sc)
        pr[..., :14] = torch.softmax(sc[..., :14], dim=-1)
        return torch.einsum("bmk,bnk->bmn", pr.view(nb, s, 128), w2.double()).reshape(nb * s, c) + b2.double() + x.double()

    return Case(ref, 4e-3, x=x, w1=w1, gamma=gamma, beta=beta, b1=b1, w2=w2, b2=b2, st_in=st_in, nb=nb)


def xchain_case(nb, s):
    """test_register_chained_out_projection_and_cross_attention: y2 = a Wo^T + bo + y, P = softmax(LN(y2) W1^T + b1), y3 = P W2^T + b2 + y2.  The
    LayerNorm acts on y2, which has to be ON the grid: a is zero except on the ordinary rows, bo is zero, so y2 = y on every grid and degenerate
    row and an ordinary Linear output on the N(0, 1) rows"""
    c = 320
    g = torch.Generator().manual_seed(570)
    y = rows_mix(nb * s, c, seed=571)
    a = torch.zeros(nb * s, c, dtype=torch.float16)
    a[NORMAL_ROW] = rnd(c, seed=572)
    wo = rnd(c, c, seed=573, scale=c ** -0.5).float()
    bo = torch.zeros(c)
    w1 = rnd(nb, 128, c, seed=574, scale=2.0 * c ** -0.5).float()
    b1 = 0.3 * torch.randn(nb, 128, generator=g)
    w2 = rnd(nb, c, 128, seed=575, scale=0.5).float()
    b2 = 0.2 * torch.randn(c, generator=g)

    def ref(eps):
        y2 = (a.double() @ wo.double().t() + bo.double() + y.double()).half().double()
        ln = ln64(y2, None, None, eps).view(nb, s, c)
        sc = torch.einsum("bsc,bnc->bsn", ln, w1.double()) + b1.double()[:, None, :]
        pm = torch.zeros_like(sc).view(nb, s, 8, 16)
        pm[..., :14] = torch.softmax(sc.view(nb, s, 8, 16)[..., :14], dim=-1)
        return torch.einsum("bsn,bcn->bsc", pm.view(nb, s, 128).half().double(), w2.double()).reshape(nb * s, c) + b2.double() + y2

    return Case(ref, 3e-3, a=a, y=y, wo=wo, bo=bo, w1=w1, b1=b1, w2=w2, b2=b2, nb=nb)


def ffchain_case(m):
    """test_register_chained_feed_forward: out = [GEGLU(LN(x) W1^T + b1) | x] Wm^T + bm + r, the hidden tensor rounded to fp16 where the kernel
    rounds it"""
    c, hdim = 320, 1280
    x = rows_mix(m, c, seed=580)
    r = rnd(m, c, seed=581)
    w1 = rnd(2 * hdim, c, seed=582, scale=c ** -0.5).float()
    gamma, beta, b1 = affine(c, 583, 2 * hdim)
    wm = rnd(c, hdim + c, seed=584, scale=(hdim + c) ** -0.5).float()
    bm = 0.1 * torch.randn(c, generator=torch.Generator().manual_seed(585))

    def ref(eps):
        h = geglu(F.linear(ln64(x, gamma, beta, eps), w1.double(), b1.double())).half().double()
        return F.linear(torch.cat([h, x.double()], dim=-1), wm.double(), bm.double()) + r.double()

    return Case(ref, 4e-3, x=x, r=r, w1=w1, gamma=gamma, b1f=geglu_pack(b1 + w1 @ beta), wm=wm, bm=bm)


FOLD_CASES = [  # m, c, n, tile, column ranges (lnlin), GEGLU
    (300, 320, 960, -1, 0, False),   # gemm_kernel, the heuristic
    (300, 320, 960, 34, 0, False),   # ... an 8-wave (k-split) id
    (300, 320, 960, 42, 0, False),   # ... a loader-wave id
    (300, 320, 960, 20, 0, False),   # gemm_wide
    (300, 320, 960, 21, 0, False),
    (300, 320, 2560, 0, 0, True),    # gemm_kernel and gemm_wide, the GEGLU epilogue
    (300, 320, 2560, 20, 0, True),
    (300, 320, 960, 50, 2, False),   # lnlin
    (128, 320, 2560, 50, 20, True),  # lnlin with GEGLU
]
XATTN_CASES = [(1, 16, 1280), (2, 64, 320)]
FFCHAIN_CASES = [128, 300]
GN_LINEAR_CASES = [(2, 128, 320, 320, 5), (2, 128, 640, 640, 10)]  # b, hw, c, n, column ranges of gn_linear


# ---------------------------------------------------------------- without a device: the file is not vacuous
def test_grid_inputs_see_the_eps_that_gaussian_inputs_hide():
    """On the Gaussian inputs of test_layernorm / test_groupnorm a float64 reference with the WRONG eps (the other constant, or none) passes
    close() against the right one; on grid() inputs it fails by at least ten limits while the fp32 restatement of the kernels' formula passes.
    And the premises of the generator: no nonzero |x| below 2^-12, every row / group variance in [5e-6, 5e-5]."""
    for rows, c in LN_SHAPES:
        gamma, beta = affine(c, 51)
        xg = rnd(rows, c, seed=50) * 1.5 + 0.3
        for right, wrong in ((1e-5, 1e-6), (1e-6, 1e-5), (1e-6, 0.0), (1e-5, 0.0)):
            close(ln64(xg, gamma, beta, wrong), ln64(xg, gamma, beta, right))  # accepted: the gap
        x = grid((rows, c), seed=500)
        nz = x[x != 0].float().abs()
        assert nz.min().item() >= 2.0 ** -12 and torch.equal(x.float() * 4096, torch.round(x.float() * 4096))
        var = x.double().var(dim=-1, unbiased=False)
        assert 5e-6 <= var.min().item() and var.max().item() <= 5e-5 and x.double().mean(dim=-1).abs().max().item() < 1e-3
        for right, wrong in ((1e-5, 1e-6), (1e-6, 1e-5)):
            ref = ln64(x, gamma, beta, right)
            assert (ln64(x, gamma, beta, wrong) - ref).abs().max().item() >= 10 * limit(ref, 2e-3)
            close(kernel_formula_ln(x, gamma, beta, right), ref)
        ref = ln64(x, gamma, beta, 1e-6)
        assert (ln64(x, gamma, beta, 0.0) - ref).abs().max().item() >= 10 * limit(ref, 2e-3)  # a dropped eps
    for b, hw, c in GN_SHAPES:
        gamma, beta = affine(c, 41)
        xg = rnd(b, hw, c, seed=40) * 2 + 0.5
        for right, wrong in ((1e-5, 1e-6), (1e-6, 1e-5), (1e-6, 0.0), (1e-5, 0.0)):
            close(gn64(xg, gamma, beta, wrong), gn64(xg, gamma, beta, right))
        x = grid((b, hw, c), seed=510)
        assert x[x != 0].float().abs().min().item() >= 2.0 ** -12
        var = x.double().view(b, hw, 32, c // 32).var(dim=(1, 3), unbiased=False)
        assert 5e-6 <= var.min().item() and var.max().item() <= 5e-5
        for right, wrong in ((1e-5, 1e-6), (1e-6, 1e-5)):
            ref = gn64(x, gamma, beta, right)
            assert (gn64(x, gamma, beta, wrong) - ref).abs().max().item() >= 10 * limit(ref, 2e-3)
            close(kernel_formula_gn(x, gamma, beta, right), ref)
        ref = gn64(x, gamma, beta, 1e-6)
        assert (gn64(x, gamma, beta, 0.0) - ref).abs().max().item() >= 10 * limit(ref, 2e-3)


def test_degenerate_rows_and_groups_through_the_kernel_formula():
    """The mix of rows / groups the GPU cases carry, through the fp32 restatement of the kernels' formula: finite, constant rows and groups
    come out as beta, every row within the tolerance of its float64 reference (also a constant 100.0 row)."""
    for eps in EPS:
        for rows, c in ((64, 320), (14, 768)):
            x = rows_mix(rows, c, seed=500)
            x[11] = 100.0
            gamma, beta = affine(c, 501)
            got = kernel_formula_ln(x, gamma, beta, eps)
            close(got, ln64(x, gamma, beta, eps))
            close(got[CONST_ROWS + [11]], beta.expand(4, c))
        for b, hw, c in GN_SHAPES:
            case = gn_case(b, hw, c)
            got = kernel_formula_gn(case.x, case.gamma, case.beta, eps)
            close(got, case.ref(eps))
            index, want = gn_const(case)
            close(got[index], want.expand(hw, -1))


def test_every_case_separates_its_two_eps():
    """The premise both_eps() asserts in front of every GPU case, here without a device: the float64 references for eps = 1e-5 and 1e-6 are more
    than three limits apart on every path (the e4m3 quantiser: more than half of the codes differ)."""
    for rows, c in LN_SHAPES:
        two_refs(ln_case(rows, c).ref, 2e-3)
    for b, hw, c in GN_SHAPES + [(1, 64, 960)]:
        for silu in (False, True):
            two_refs(gn_case(b, hw, c, silu).ref, 2e-3)
    for b, hw, c, n, _ in GN_LINEAR_CASES:
        case = gn_linear_case(b, hw, c, n)
        two_refs(case.ref, case.tol)
    for m, c, n, is_geglu in sorted({(m, c, n, gg) for m, c, n, _, _, gg in FOLD_CASES}):
        case = fold_case(m, c, n, is_geglu)
        two_refs(case.ref, case.tol)
    case = fp8_case(300, 320)
    two_refs(case.ref, case.tol)
    case = quant_case(37, 640)
    codes = [ordinal(e4_bytes(case.ref(eps), case.scale)) for eps in EPS]
    assert (codes[0] != codes[1]).float().mean().item() > 0.5
    for nb, s, c in XATTN_CASES:
        case = xattn_case(nb, s, c)
        two_refs(case.ref, case.tol)
    case = xchain_case(1, 128)
    two_refs(case.ref, case.tol)
    for m in FFCHAIN_CASES:
        case = ffchain_case(m)
        two_refs(case.ref, case.tol)


# ---------------------------------------------------------------- (1) LayerNorm
@gpu
@pytest.mark.parametrize("rows,c", LN_SHAPES)
def test_layernorm_eps(ops, rows, c):
    case = ln_case(rows, c)
    x, gamma, beta = case.x.cuda(), case.gamma.cuda(), case.beta.cuda()
    both_eps(lambda eps: ops.layernorm(x, gamma, beta, eps=eps), case.ref, const=(CONST_ROWS, case.beta.double()) if rows >= 10 else None)


@gpu
def test_layernorm_eps_on_a_strided_row_view(ops):
    """rows 0, 50, 100, ... of a [14 * 50, 768] buffer (the class-token rows of the brush encoder's 14 images); the rows between hold ordinary
    data that must not reach the statistics"""
    case = ln_case(14, 768)
    buf = rnd(14 * 50, 768, seed=502)
    buf[::50] = case.x
    view = buf.cuda()[::50]
    assert not view.is_contiguous() and view.stride() == (50 * 768, 1)
    gamma, beta = case.gamma.cuda(), case.beta.cuda()
    both_eps(lambda eps: ops.layernorm(view, gamma, beta, eps=eps), case.ref, const=(CONST_ROWS, case.beta.double()))


# ---------------------------------------------------------------- (2) GroupNorm
@gpu
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("b,hw,c", GN_SHAPES)
def test_groupnorm_eps(ops, b, hw, c, silu):
    case = gn_case(b, hw, c, silu)
    x, gamma, beta = case.x.cuda(), case.gamma.cuda(), case.beta.cuda()
    both_eps(lambda eps: ops.groupnorm(x, gamma, beta, eps=eps, silu=silu), case.ref, const=gn_const(case))


# ---------------------------------------------------------------- (3) GroupNorm applied from conv-emitted statistics
@gpu
@pytest.mark.parametrize("tile", [53, 54])
def test_groupnorm_apply_from_conv_statistics_eps(ops, tile):
    """conv3x3(..., gn_groups=32) on a grid input with THINNED weights (two of the 576 taps of an output channel are +-1, the rest 0): the
    stored output is a sum of a few grid values -- on the grid itself, group variance below 1e-4 (asserted).  Output groups 1 / 3 / 5 of
    every sample: no taps and bias 0 (all-zero), no taps and bias 0.5 (constant), dense weights (ordinary)."""
    b, h, cin, cout = 2, 16, 64, 640
    cpg = cout // 32
    g = torch.Generator().manual_seed(590)
    x = grid((b, h, h, cin), seed=591)
    wt = torch.sign(torch.randn(cout, cin, 3, 3, generator=g)) * (torch.rand(cout, cin, 3, 3, generator=g) < 2.0 / (9 * cin)).float()
    bias = torch.zeros(cout)
    for grp, val in ((ZERO_GROUP, 0.0), (HALF_GROUP, 0.5)):
        wt[grp * cpg:(grp + 1) * cpg] = 0
        bias[grp * cpg:(grp + 1) * cpg] = val
    wt[NORMAL_GROUP * cpg:(NORMAL_GROUP + 1) * cpg] = rnd(cpg, cin, 3, 3, seed=592, scale=256.0 * (9 * cin) ** -0.5).float()
    wf = wt.cuda()
    y, st = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile, splits=1, gn_groups=32)
    yc = y.cpu().view(b, h * h, cout)
    var = yc.double().view(b, h * h, 32, cpg).var(dim=(1, 3), unbiased=False)
    on_grid = [i for i in range(32) if i not in (ZERO_GROUP, HALF_GROUP, NORMAL_GROUP)]
    assert 1e-6 < var[:, on_grid].min().item() and var[:, on_grid].max().item() < 1e-4  # the case is what it says
    assert var[:, ZERO_GROUP].max().item() == 0 and var[:, HALF_GROUP].max().item() == 0 and var[:, NORMAL_GROUP].min().item() > 0.1
    assert torch.equal(yc[..., ZERO_GROUP * cpg:(ZERO_GROUP + 1) * cpg], torch.zeros(b, h * h, cpg, dtype=torch.float16))
    gamma, beta = affine(cout, 593)
    for silu in (True, False):
        index, want = gn_const(Case(None, 2e-3, x=yc, beta=beta, silu=silu))
        both_eps(lambda eps: ops.groupnorm_apply(y, gamma.cuda(), beta.cuda(), st, eps=eps, silu=silu).view(b, h * h, cout),
                 lambda eps: gn64(yc, gamma, beta, eps, silu), const=(index, want))


# ---------------------------------------------------------------- (4) the split-K reduce folded into the GroupNorm
@gpu
@pytest.mark.parametrize("b,hw,c,cskip,silu", [(2, 64, 320, 0, True), (1, 1024, 128, 0, False),  # one launch / reduce in the statistics pass
                                               (1, 64, 960, 320, True)])                       # over the concatenation [x | skip], groups straddle the seam
def test_reduce_groupnorm_eps(ops, b, hw, c, cskip, silu):
    """the two fp32 slabs are exact halves of a grid tensor: the conv output the launch writes is that tensor, bit for bit"""
    case = gn_case(b, hw, c, silu, seed=600)
    front = case.x[..., :c - cskip].contiguous()
    part = torch.stack([front.float() * 0.5, front.float() * 0.5]).contiguous().cuda()
    skip = case.x[..., c - cskip:].contiguous().cuda() if cskip else None
    gamma, beta = case.gamma.cuda(), case.beta.cuda()

    def run(eps):
        out, y = ops.reduce_groupnorm(part, gamma, beta, eps=eps, silu=silu, skip=skip)
        assert torch.equal(out.cpu(), case.x)
        return y

    both_eps(run, case.ref, const=gn_const(case))


# ---------------------------------------------------------------- (5) statistics pass, then the apply pass
@gpu
@pytest.mark.parametrize("slabs", [False, True])
def test_groupnorm_stats_apply_eps(ops, slabs):
    case = gn_case(2, 64, 320, seed=610)
    gamma, beta = case.gamma.cuda(), case.beta.cuda()
    part = torch.stack([case.x.float() * 0.5, case.x.float() * 0.5]).contiguous().cuda()
    xg = case.x.cuda()

    def run(eps):
        out, y = ops.groupnorm_stats_apply(gamma, beta, part=part, eps=eps) if slabs else ops.groupnorm_stats_apply(gamma, beta, x=xg, eps=eps)
        assert torch.equal(out.cpu(), case.x)
        return y

    both_eps(run, case.ref, const=gn_const(case))


# ---------------------------------------------------------------- (6) GroupNorm folded into / applied inside a Linear
@gpu
@pytest.mark.parametrize("b,hw,c,n,ranges", GN_LINEAR_CASES)
def test_groupnorm_folded_into_linear_weights_eps(ops, b, hw, c, n, ranges):
    """gn_fold_weights + the grouped GEMM.  With a zero-variance group the folded weights carry rstd = eps^-1/2 (up to 1000) and the constant
    0.5 group puts |x W'^T| at ~100 (eps = 1e-5) / ~300 (1e-6), which the folded per-sample bias has to cancel: that works only if the bias
    joins the accumulator before gemm_kernel rounds it to fp16 (3.2e-2 / 1.3e-1 against a limit of 2e-2 when it was added behind)."""
    from diffusiontexturepainting_amd._lib import GF_BIAS
    case = gn_linear_case(b, hw, c, n)
    x, gamma, beta, bias = case.x.cuda(), case.gamma.cuda(), case.beta.cuda(), case.bias.cuda()
    wp = ops.pack_linear(case.w.cuda())

    def folded(eps):
        wf, bf = ops.gn_fold_weights(x, wp, n, bias, gamma, beta, eps=eps)
        return ops.gemm(x.view(b * hw, c), wf.view(-1, wf.shape[-1]), n, c, bias=bf.view(-1), flags=GF_BIAS, batch=b).view(b, hw, n)

    both_eps(folded, case.ref, case.tol)


@gpu
@pytest.mark.parametrize("b,hw,c,n,ranges", GN_LINEAR_CASES)
def test_groupnorm_applied_inside_the_linear_eps(ops, b, hw, c, n, ranges):
    """gn_linear: the GroupNorm applied to the resident activation fragments of lnlin_kernel, on the operands of the fold above"""
    case = gn_linear_case(b, hw, c, n)
    x, gamma, beta, bias = case.x.cuda(), case.gamma.cuda(), case.beta.cuda(), case.bias.cuda()
    wp = ops.pack_linear(case.w.cuda())
    both_eps(lambda eps: ops.gn_linear(x, wp, n, bias, gamma, beta, eps=eps, col_ranges=ranges), case.ref, case.tol)


# ---------------------------------------------------------------- (7) the LayerNorm fold of the GEMM kernels
def _producer_stats(ops, x):
    """x through an identity Linear with row_stats=True: the output is x, bit for bit, and the partials are a producer's own"""
    c = x.shape[1]
    y, st = ops.gemm(x, ops.pack_linear(torch.eye(c).cuda()), c, c, row_stats=True)
    assert torch.equal(y, x)
    return st.contiguous()


@gpu
@pytest.mark.parametrize("m,c,n,tile,ranges,is_geglu", FOLD_CASES)
def test_gemm_layernorm_fold_eps(ops, m, c, n, tile, ranges, is_geglu):
    """in-kernel statistics and (gemm_kernel, gemm_wide) the stats_in= form fed from a producer's row_stats partials; constant rows come out
    as bias + W beta"""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    case = fold_case(m, c, n, is_geglu)
    x, b2 = case.x.cuda(), case.b2.cuda()
    wp = ops.pack_linear((case.w * case.gamma[None]).cuda(), geglu=is_geglu)
    lns = ops.rowsum(wp, c)
    fl = (GF_GEGLU | GF_BIAS) if is_geglu else 0
    both_eps(lambda eps: ops.gemm(x, wp, n, c, bias=b2, lns=lns, ln_eps=eps, tile=tile, splits=ranges, flags=fl), case.ref, case.tol, const=case.const)
    if tile != 50:
        st = _producer_stats(ops, x)
        both_eps(lambda eps: ops.gemm(x, wp, n, c, bias=b2, lns=lns, ln_eps=eps, tile=tile, flags=fl, stats_in=st), case.ref, case.tol, const=case.const)


@gpu
@pytest.mark.experimental
def test_gemm_weight_streaming_layernorm_fold_eps(ops):
    """gemmws_kernel (tile 55, DTP_EXPERIMENTAL builds) with GF_LNFOLD: statistics from the producer's partials only"""
    needs_experimental_build(ops)
    m, c, n = 192, 1280, 1280
    case = fold_case(m, c, n, False)
    x = case.x.cuda()
    wp = ops.pack_linear((case.w * case.gamma[None]).cuda())
    wfr = ops.pack_linear_ws(wp, n, c)
    lns = ops.rowsum(wp, c)
    b2 = torch.zeros(wp.shape[0])
    b2[:n] = case.b2
    b2 = b2.cuda()
    st = _producer_stats(ops, x)
    both_eps(lambda eps: ops.gemm(x, wp, n, c, bias=b2, lns=lns, ln_eps=eps, stats_in=st, tile=55, wfr=wfr), case.ref, case.tol, const=case.const)


# ---------------------------------------------------------------- (8) the fp8 paths
@gpu
@pytest.mark.parametrize("tile", [24, 28])
def test_gemm_fp8_layernorm_eps(ops, tile):
    """against the same contraction on the e4m3-rounded operands (2.5e-2, as test_gemm_fp8_layernorm_geglu_and_two_operands: a normalised value
    on an e4m3 rounding boundary may land on the neighbouring code) and against exact float64 (8e-2 of the range: the operand rounding)"""
    from diffusiontexturepainting_amd._lib import GF_BIAS, GF_GEGLU
    m, c = 300, 320
    case = fp8_case(m, c)
    x, bp = case.x.cuda(), case.b2.cuda()
    wp = ops.pack_linear((case.w * case.gamma[None]).cuda(), geglu=True)
    w8, ws = ops.quantize_w8(wp, c)
    outs = {}

    def run(eps):
        outs[eps] = ops.gemm(x, wp, 8 * c, c, bias=bp, flags=GF_GEGLU | GF_BIAS, tile=tile, w8=w8, w_scale=ws, layernorm=True, ln_eps=eps)
        return outs[eps]

    both_eps(run, lambda eps: case.ref(eps, ws), case.tol, const=case.const)
    for eps in EPS:
        ref = case.exact(eps)
        assert (outs[eps].double().cpu() - ref).abs().max().item() <= 8e-2 * ref.abs().max().item()


@gpu
@pytest.mark.parametrize("with_stats", [True, False])
def test_quant_layernorm_eps(ops, with_stats):
    """quant_e4m3(ln=True, eps=...) as test_quant_layernorm_and_dual_copy compares it: within one e4m3 code of the float64 normalised value,
    almost always the same code; constant rows are code 0 exactly"""
    m, k = 37, 640
    case = quant_case(m, k)
    xf = case.x.float()
    st = None
    if with_stats:
        st = torch.stack([torch.stack([ch.sum(1), (ch * ch).sum(1)], dim=1) for ch in xf.chunk(10, dim=1)]).cuda()
    x = case.x.cuda()
    want = {eps: ordinal(e4_bytes(case.ref(eps), case.scale)) for eps in EPS}
    assert (want[EPS[0]] != want[EPS[1]]).float().mean().item() > 0.5  # the two eps give different codes
    for eps in EPS:
        got = ops.quant_e4m3(x, case.scale, ln=True, stats_in=st, eps=eps)
        torch.cuda.synchronize()
        d = (ordinal(got.cpu()) - want[eps]).abs()
        assert d.max().item() <= 1, (eps, d.max().item())
        assert (d > 0).float().mean().item() < 0.01
        assert int(ordinal(got.cpu())[CONST_ROWS].abs().max()) == 0


# ---------------------------------------------------------------- (9) the fused transformer launches
@gpu
@pytest.mark.parametrize("nb,s,c", XATTN_CASES)
def test_xattn_eps(ops, nb, s, c):
    case = xattn_case(nb, s, c)
    x = case.x.cuda()
    w1p = torch.cat([ops.pack_linear((case.w1[b] * case.gamma[None]).cuda()) for b in range(nb)], dim=0).contiguous()
    b1f = (case.b1 + torch.einsum("bnc,c->bn", case.w1, case.beta)).reshape(-1).cuda()
    lns = ops.rowsum(w1p, c)
    w2p = torch.cat([ops.pack_linear(case.w2[b].cuda()) for b in range(nb)], dim=0).contiguous()
    st_in, b2 = case.st_in.cuda(), case.b2.cuda()
    both_eps(lambda eps: ops.xattn(x, w1p, b1f, lns, st_in, w2p, b2, nb, ln_eps=eps), case.ref, case.tol)


@gpu
def test_xchain_eps(ops):
    nb, s, c = 1, 128, 320
    case = xchain_case(nb, s)
    a, y = case.a.cuda(), case.y.cuda()
    wop = ops.pack_linear(case.wo.cuda())
    w1p = torch.cat([ops.pack_linear(case.w1[b].cuda()) for b in range(nb)], dim=0).contiguous()
    lns = ops.rowsum(w1p, c)
    w2p = torch.cat([ops.pack_linear(case.w2[b].cuda()) for b in range(nb)], dim=0).contiguous()
    bo, b1, b2 = case.bo.cuda(), case.b1.reshape(-1).cuda(), case.b2.cuda()
    both_eps(lambda eps: ops.xchain(a, wop, bo, y, w1p, b1, lns, w2p, b2, nb, ln_eps=eps), case.ref, case.tol)


@gpu
@pytest.mark.parametrize("m", FFCHAIN_CASES)
def test_ffchain_eps(ops, m):
    case = ffchain_case(m)
    x, r = case.x.cuda(), case.r.cuda()
    w1p = ops.pack_linear((case.w1 * case.gamma[None]).cuda(), geglu=True)
    lns = ops.rowsum(w1p, 320)
    wmp = ops.pack_linear(case.wm.cuda())
    b1p, bm = case.b1f.cuda(), case.bm.cuda()
    both_eps(lambda eps: ops.ffchain(x, w1p, lns, b1p, wmp, bm, resid=r, ln_eps=eps), case.ref, case.tol)
