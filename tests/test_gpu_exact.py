"""Bit-exact checks of every contraction kernel and every LINEAR epilogue on small-integer operands.

tests/test_gpu_ops.py compares against fp32 torch within 2e-3 * max|ref| + 2e-3 on Gaussian data: about 0.011 for outputs of order 1,
while ONE wrong term of the contraction moves an element by |x| K^-0.5 (0.028 at K = 1280, 0.009 at K = 11520).  A border pixel that reads
its neighbour's row instead of the zero padding, an element dropped at a split-K cut, a partial sum rounded to fp16 before a combine or a
wait that returns one load early all fit under that limit.  With small integer operands every product and every fp32 partial sum is exact
in ANY order, so the kernel has to equal the float64 CPU reference bit for bit and torch.equal replaces the tolerance:

  fp16 out : activations in {-2..2}, weights in {-1, 0, 1}, bias and residual in {-8..8}; the reference must satisfy max|ref| <= 2048
             (every such integer is an fp16 number, so the stored output is exact too);
  fp32 out : GF_OUT_F32 on the launchers that take it (dtp_launch_gemm, i.e. gemm_kernel in its dense and conv modes; gemm_wide, lnlin,
             gemm_ws, conv_halo, conv_ws, gemm_fp8 and gemm_f8f8 refuse the flag in their *_supported checks and have no fp32-out case);
             activations in {-32..32}, weights in {-8..8}; max sum|a||w| < 2^24 (every fp32 partial exact) and max|ref| > 2048 (a partial
             that went through fp16 on the way would show).  This holds for the SPLIT launches only (fp32 slabs + the slab reduce):
             an unsplit gemm_kernel launch stages its accumulators through LDS as fp16 on purpose (gemm_conv.hip), so its fp32-out
             cases ("staged") keep the fp16-out ranges and |accumulator| <= 2048 and check the fp32 store path, not a wider range;
  GF_ROWSTATS / GF_GNSTATS : the emitted partials, summed in fp32 as their consumer sums them, equal the sums of the exact output; weights
             thinned (1 in 4, then halved) until every sum of squares is < 2^24;
  fp8      : operands in {-2..2} (exact in e4m3), unit scales; the e4m3 output with |ref| <= 16 (K = 64, thinned weights).

These are conditions on the INPUTS, asserted on the CPU reference alone (test_exact_case_inputs_satisfy_their_bounds, no device, and again
in front of every GPU call).  Tile ids, conv cases and the halo / weight-streaming variant ids come from test_gpu_ops.py.

Out of scope, because their arithmetic is not exact by design: the LayerNorm and GroupNorm folds (rsqrt), the GEGLU / GELU / QuickGELU /
SiLU epilogues (erf / exp), GF_SOFTMAX16, every attention kernel, and xchain / ffchain (which contain the former).

Run time on one MI355X: see RUN_TIME below.
"""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as T
from diffusiontexturepainting_amd._lib import GF_BIAS_M, GF_OUT_F32, GF_RAGGED
from test_gpu_ops import CONV_CASES, CONV_TILES, GEMM_SHAPES, GEMM_TILES, HALO_CASES, WS_CASES, close, needs_experimental_build

RUN_TIME = ("this file on one MI355X: 417 GPU cases in 5.8 s (8 s wall with start-up); the GPU suite was last recorded at 1 084 s of its 1 200 s "
            "limit (VERDICT.md), so the file adds about 0.5 % -- far below the tenth of the suite that would call for thinning the case lists")

gpu = pytest.mark.gpu


# dtp_gemm_wide_supported() refuses GF_OUT_F32: the two gemm_wide ids among GEMM_TILES / CONV_TILES have fp16-out cases only
NO_F32_TILES = (20, 21)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import ops as o
    return o


def _params(fn):
    """the argvalues of a test_gpu_ops test's (single) parametrize mark: its case list, not a copy of it"""
    marks = [m for m in fn.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1
    return list(marks[0].args[1])


# ---------------------------------------------------------------- the helper
def exact(got, ref, kind="gemm"):
    """got == ref bit for bit (identical shapes, all finite, torch.equal).  On failure: the number of differing elements, the first five
    (index, got, want), and where they sit -- (row % 64, col % 64) for a GEMM, (y % 8, x % 16, channel % 64) for an NHWC conv output."""
    g = got.float().cpu()
    assert g.shape == ref.shape, (tuple(g.shape), tuple(ref.shape))
    assert ref.dtype == torch.float32
    assert torch.isfinite(g).all(), f"{(~torch.isfinite(g)).sum().item()} non-finite outputs"
    if torch.equal(g, ref):
        return
    bad = (g != ref).nonzero()
    first = [(tuple(i.tolist()), g[tuple(i.tolist())].item(), ref[tuple(i.tolist())].item()) for i in bad[:5]]
    if kind == "conv" and g.dim() == 4:
        names, coords = ("y % 8", "x % 16", "channel % 64"), (bad[:, 1] % 8, bad[:, 2] % 16, bad[:, 3] % 64)
    else:
        names, coords = ("row % 64", "col % 64"), (bad[:, -2] % 64 if g.dim() > 1 else bad[:, 0] * 0, bad[:, -1] % 64)
    joint = collections.Counter(zip(*[c.tolist() for c in coords])).most_common(12)
    axes = "; ".join(f"{n}: {dict(sorted(collections.Counter(c.tolist()).items()))}" for n, c in zip(names, coords))
    raise AssertionError(f"{bad.shape[0]} of {g.numel()} elements differ; first (index, got, want): {first}; "
                         f"positions over ({', '.join(names)}), most frequent first: {joint}; per axis -- {axes}")


# ---------------------------------------------------------------- integer inputs and their conditions
LIM24 = float(2 ** 24)


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).double()


def thin(w, keep, seed):
    """keep about `keep` of the weights, zero the rest"""
    if keep >= 1.0:
        return w
    return w * (torch.rand(w.shape, generator=torch.Generator().manual_seed(seed)) < keep).double()


class Data(dict):
    __getattr__ = dict.__getitem__


def cached(fn):
    """one result per set of keyword arguments, whatever their order; the tests share it and leave it unchanged"""
    store = {}

    @functools.wraps(fn)
    def wrapper(**k):
        key = tuple(sorted(k.items()))
        if key not in store:
            store[key] = fn(**k)
        return store[key]
    return wrapper


def _finish(d, ref, absum, f32, stats_sq=None, out_lim=2048.0, acc=None):
    """cast the float64 reference down and record what the conditions need"""
    d.update(ref=ref.float(), f32=f32, max_ref=ref.abs().max().item(), max_absum=absum.max().item(), stats_sq=stats_sq, out_lim=out_lim,
             max_acc=acc.abs().max().item())
    assert torch.equal(d.ref.double(), ref)  # integers below 2^24: the cast is exact
    return d


def check(d):
    """the conditions that make `exact` true, on the CPU reference alone"""
    if d.f32 is True:
        assert d.max_absum < LIM24, f"sum|a||w| = {d.max_absum} >= 2^24: an fp32 partial could round"
        assert d.max_ref > 2048, f"max|ref| = {d.max_ref} <= 2048: an fp16 round of a partial would not show"
    elif d.get("fp16_values"):  # the all-ones conv: not bounded by 2048, but every output (and every unsplit accumulator) is an fp16 number
        assert torch.equal(d.ref.half().float(), d.ref)
    else:
        assert d.max_ref <= d.out_lim, f"max|ref| = {d.max_ref} > {d.out_lim}: the stored output would round"
        assert d.max_acc <= 2048, f"max|accumulator| = {d.max_acc} > 2048: the fp16 staging tile of an unsplit launch would round"
    if d.stats_sq is not None:
        assert d.stats_sq < LIM24, f"largest sum of squares {d.stats_sq} >= 2^24"


def _ranges(f32):
    """f32: False = fp16 out, True = fp32 out of a split launch, "staged" = fp32 out of a launch that may be unsplit (fp16-out ranges)"""
    assert f32 in (False, True, "staged")
    return ((-32, 32), (-8, 8)) if f32 is True else ((-2, 2), (-1, 1))


@cached
def gemm_data(m, n, k, f32=False, nb=1, bias="n", resid=True, stats=False, keep=1.0, seed=0, act=None, out_lim=2048.0, bres=8, k2=0, k2_scale=1.0):
    """[nb * m, k] x nb weight matrices [n, k] (+ bias per column ("n": one vector per problem, "shared": one for all) or per row ("m"),
    + residual); with stats the weights are thinned until the row sums of squares of the output are < 2^24.  k2: the last k2 columns of
    the activations count k2_scale times (the fp8 tail with its own scale)."""
    (alo, ahi), (wlo, whi) = _ranges(f32)
    if act is not None:
        alo, ahi = act
    a = ints((nb * m, k), alo, ahi, 1000 + seed)
    w0 = ints((nb, n, k), wlo, whi, 2000 + seed)
    bv = ints((nb, n) if bias == "n" else (m,) if bias == "m" else (n,), -bres, bres, 3000 + seed) if bias else None
    r = ints((nb * m, n), -bres, bres, 4000 + seed) if resid else None
    av = a.clone()
    if k2:
        av[:, k - k2:] *= k2_scale
    if stats and keep >= 1.0:
        keep = 0.25
    while True:
        w = thin(w0, keep, 5000 + seed)
        ref = torch.einsum("bmk,bnk->bmn", av.view(nb, m, k), w)
        absum = torch.einsum("bmk,bnk->bmn", av.abs().view(nb, m, k), w.abs())
        acc = ref
        if bias == "m":
            ref, absum = ref + bv[None, :, None], absum + bv.abs()[None, :, None]
        elif bias == "n":
            ref, absum = ref + bv[:, None, :], absum + bv.abs()[:, None, :]
        elif bias == "shared":
            ref, absum = ref + bv, absum + bv.abs()
        ref, absum = ref.reshape(nb * m, n), absum.reshape(nb * m, n)
        if resid:
            ref, absum = ref + r, absum + r.abs()
        sq = (ref * ref).sum(dim=1).max().item() if stats else None
        if (not stats or sq < LIM24) and (out_lim >= 2048.0 or ref.abs().max().item() <= out_lim) or keep < 1e-3:
            break
        keep /= 2
    return _finish(Data(a=a, w=w, bias=bv, resid=r, keep=keep), ref, absum, f32, sq, out_lim, acc=acc)


def row_stats_of(ref):
    return torch.stack([ref.sum(dim=1), (ref * ref).sum(dim=1)], dim=-1)


def fp32_sum(parts):
    """sum over the leading dimension one partial after the other in fp32, as the consumers of the statistics tables do"""
    tot = parts[0].float().cpu().clone()
    for z in range(1, parts.shape[0]):
        tot += parts[z].float().cpu()
    return tot


@cached
def conv_data(b, h, w, cin, cout, stride=1, pad=1, ups=False, out_hw=None, f32=False, cin2=0, bias=True, resid=True, ones=False, gn_groups=0,
              seed=0):
    """NHWC input [b, h, w, cin] through a 3x3 conv (as test_conv3x3 builds its reference), optionally + a 1x1 shortcut over a second
    tensor of cin2 channels; ones: x = 1, W = 1, no bias / residual (every output = in-image taps * cin); gn_groups: weights thinned
    until the per-(image, group) sums of squares of the output are < 2^24."""
    (alo, ahi), (wlo, whi) = _ranges(f32)
    x = torch.ones(b, h, w, cin, dtype=torch.float64) if ones else ints((b, h, w, cin), alo, ahi, 6000 + seed)
    w0 = torch.ones(cout, cin, 3, 3, dtype=torch.float64) if ones else ints((cout, cin, 3, 3), wlo, whi, 7000 + seed)
    xin = x.permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, size=(2 * h - 1, 2 * w - 1) if out_hw is not None else (2 * h, 2 * w), mode="nearest")
    p = pad
    if out_hw is not None and pad == 0:
        xin, p = F.pad(xin, (0, 1, 0, 1)), 0
    keep = 0.25 if gn_groups else 1.0
    x2 = ints((b, *((out_hw or (h, w))), cin2), alo, ahi, 8000 + seed) if cin2 else None
    w1 = ints((cout, cin2, 1, 1), wlo, whi, 9000 + seed) if cin2 else None
    while True:
        wt = thin(w0, keep, 9500 + seed)
        ref = F.conv2d(xin, wt, None, stride=stride, padding=p)
        absum = F.conv2d(xin.abs(), wt.abs(), None, stride=stride, padding=p)
        if cin2:
            ref, absum = ref + F.conv2d(x2.permute(0, 3, 1, 2), w1), absum + F.conv2d(x2.abs().permute(0, 3, 1, 2), w1.abs())
        ref, absum = ref.permute(0, 2, 3, 1).contiguous(), absum.permute(0, 2, 3, 1)
        acc = ref
        bv = ints((cout,), -8, 8, 9600 + seed) if bias and not ones else None
        r = ints(ref.shape, -8, 8, 9700 + seed) if resid and not ones else None
        if bv is not None:
            ref, absum = ref + bv, absum + bv.abs()
        if r is not None:
            ref, absum = ref + r, absum + r.abs()
        sq = None
        if gn_groups:
            yf = ref.reshape(b, -1, gn_groups, cout // gn_groups)
            sq = (yf * yf).sum(dim=(1, 3)).max().item()
        if not gn_groups or sq < LIM24 or keep < 1e-3:
            break
        keep /= 2
    return _finish(Data(x=x, w=wt, bias=bv, resid=r, x2=x2, w1=w1, keep=keep, fp16_values=ones), ref, absum, f32, sq, acc=acc)


REGISTRY = []  # (data function, list of argument tuples / dicts): what test_exact_case_inputs_satisfy_their_bounds walks


def register(fn, keys):
    REGISTRY.append((fn, list(dict.fromkeys(keys))))


def kw(**k):
    """hashable keyword arguments of a data function"""
    return tuple(sorted(k.items()))


def data(fn, key):
    return fn(**dict(key))


def dev16(t):
    return t.half().cuda()


def dev32(t):
    return t.float().cuda()


def f32flag(f32):
    return GF_OUT_F32 if f32 else 0


# ---------------------------------------------------------------- 1. dense GEMM, every tile id
DENSE_EDGE_SHAPES = [(77, 768, 768), (520, 640, 1280)]  # ragged M, N and K no multiples of 128 / 256; > 1 M tile of the 256-row tiles + 20 k-blocks
DENSE_CASES = [(m, n, k, t, f32) for t in GEMM_TILES for (m, n, k) in (GEMM_SHAPES if t == -1 else DENSE_EDGE_SHAPES)
               for f32 in (False, "staged") if not (f32 and t in NO_F32_TILES)]
register(gemm_data, [kw(m=m, n=n, k=k, f32=f32) for m, n, k, t, f32 in DENSE_CASES])


@gpu
@pytest.mark.parametrize("m,n,k,tile,f32", DENSE_CASES)
def test_exact_gemm_dense(ops, m, n, k, tile, f32):
    """an explicit tile runs unsplit (its own staged epilogue; the K slices are test_exact_gemm_splitk's), the heuristic as the launcher likes"""
    d = gemm_data(m=m, n=n, k=k, f32=f32)
    check(d)
    got = ops.gemm(dev16(d.a), ops.pack_linear(dev32(d.w[0])), n, k, bias=dev32(d.bias[0]), resid=dev16(d.resid), tile=tile, splits=0 if tile == -1 else 1,
                   flags=f32flag(f32))
    exact(got, d.ref)


# ---------------------------------------------------------------- 2. split-K
SPLITK_SHAPE = (192, 1280, 11520)  # 180 k-blocks: 5 slices do not divide them
SPLITK_CASES = [(s, t, f32) for t in (-1, 34, 36, 42, 47) for s in (2, 5, 16) for f32 in (False, True)] + [(0, -1, False), (0, -1, "staged")]
register(gemm_data, [kw(m=SPLITK_SHAPE[0], n=SPLITK_SHAPE[1], k=SPLITK_SHAPE[2], f32=f32, seed=2) for f32 in (False, True, "staged")])


@gpu
@pytest.mark.parametrize("splits,tile,f32", SPLITK_CASES)
def test_exact_gemm_splitk(ops, splits, tile, f32):
    """fp32 slabs + the slab reduce (bias, residual); splits = 0: the launcher's own slice count"""
    m, n, k = SPLITK_SHAPE
    d = gemm_data(m=m, n=n, k=k, f32=f32, seed=2)
    check(d)
    got = ops.gemm(dev16(d.a), ops.pack_linear(dev32(d.w[0])), n, k, bias=dev32(d.bias[0]), resid=dev16(d.resid), splits=splits, tile=tile,
                   flags=f32flag(f32))
    exact(got, d.ref)


# ---------------------------------------------------------------- 3. per-row bias, batched, strided A
FORM_SHAPE = (130, 192, 256)
FORM_CASES = [(form, t, f32) for form in ("bias_m", "batch_own_bias", "batch_shared_bias", "strided_lda") for t in (-1, 5, 34, 41) for f32 in (False, "staged")]


def form_key(form, f32):
    m, n, k = FORM_SHAPE
    nb = 3 if form.startswith("batch") else 1
    bias = {"bias_m": "m", "batch_shared_bias": "shared"}.get(form, "n")
    return kw(m=m, n=n, k=k, f32=f32, nb=nb, bias=bias, resid=form != "bias_m", seed=3)


register(gemm_data, [form_key(form, f32) for form, t, f32 in FORM_CASES])


@gpu
@pytest.mark.parametrize("form,tile,f32", FORM_CASES)
def test_exact_gemm_bias_per_row_batched_and_strided(ops, form, tile, f32):
    m, n, k = FORM_SHAPE
    d = data(gemm_data, form_key(form, f32))
    check(d)
    fl = f32flag(f32)
    if form == "bias_m":  # the operand-swapped call: out[m'][n'] += bias[m']
        got = ops.gemm(dev16(d.a), ops.pack_linear(dev32(d.w[0])), n, k, bias=dev32(d.bias), flags=fl | GF_BIAS_M, tile=tile)
    elif form == "strided_lda":  # A is a column slice of a wider buffer
        big = torch.full((m, 2 * k), 7.0, dtype=torch.float16).cuda()
        big[:, k // 2: k // 2 + k] = dev16(d.a)
        got = ops.gemm(big[:, k // 2: k // 2 + k], ops.pack_linear(dev32(d.w[0])), n, k, bias=dev32(d.bias[0]), resid=dev16(d.resid), flags=fl, tile=tile)
    else:
        wp = torch.cat([ops.pack_linear(dev32(d.w[b])) for b in range(3)]).contiguous()
        npad = wp.shape[0] // 3
        if form == "batch_shared_bias":
            bias = dev32(d.bias)
        else:
            bias = torch.zeros(3, npad)
            bias[:, :n] = d.bias.float()
            bias = bias.reshape(-1).cuda()
        got = ops.gemm(dev16(d.a), wp, n, k, bias=bias, resid=dev16(d.resid), batch=3, bias_shared=form == "batch_shared_bias", flags=fl, tile=tile)
    exact(got, d.ref)


# ---------------------------------------------------------------- 4. two activation matrices
# the shapes of test_gemm_two_activation_matrices (k2 = 64 / 128 / 320) + K = 128 | 320 in two slices of four k-blocks: the cut lands inside the tail
TAIL_CASES = _params(T.test_gemm_two_activation_matrices) + [(130, 128, 320, 192, 2, 2), (130, 128, 320, 192, 38, 2)]
TAIL_CASES = [c + (f32,) for c in TAIL_CASES for f32 in (False, True if c[5] >= 2 else "staged") if not (f32 and c[4] in NO_F32_TILES)]
register(gemm_data, [kw(m=m, n=n, k=k1 + k2, f32=f32, seed=4) for m, k1, k2, n, t, s, f32 in TAIL_CASES])


@gpu
@pytest.mark.parametrize("m,k1,k2,n,tile,splits,f32", TAIL_CASES)
def test_exact_gemm_two_activation_matrices(ops, m, k1, k2, n, tile, splits, f32):
    assert {c[2] for c in TAIL_CASES} >= {64, 128, 320}
    d = gemm_data(m=m, n=n, k=k1 + k2, f32=f32, seed=4)
    check(d)
    got = ops.gemm(dev16(d.a[:, :k1].contiguous()), ops.pack_linear(dev32(d.w[0])), n, k1, bias=dev32(d.bias[0]), resid=dev16(d.resid),
                   tail=dev16(d.a[:, k1:].contiguous()), tile=tile, splits=splits, flags=f32flag(f32))
    exact(got, d.ref)


# ---------------------------------------------------------------- 5. gemm_wide, plain lnlin, gemm_ws
# (tile, m, n, k1, k2, row statistics): ragged M and a two-operand problem for each wide tile; 21 emits no statistics
WIDE_CASES = [(20, 700, 640, 640, 0, True), (21, 300, 960, 320, 0, False), (20, 600, 320, 1280, 320, True), (21, 768, 640, 640, 128, False)]
register(gemm_data, [kw(m=m, n=n, k=k1 + k2, stats=st, seed=5) for t, m, n, k1, k2, st in WIDE_CASES])


@gpu
@pytest.mark.parametrize("tile,m,n,k1,k2,stats", WIDE_CASES)
def test_exact_gemm_wide(ops, tile, m, n, k1, k2, stats):
    d = gemm_data(m=m, n=n, k=k1 + k2, stats=stats, seed=5)
    check(d)
    tail = dev16(d.a[:, k1:].contiguous()) if k2 else None
    out = ops.gemm(dev16(d.a[:, :k1].contiguous()), ops.pack_linear(dev32(d.w[0])), n, k1, bias=dev32(d.bias[0]), resid=dev16(d.resid), tail=tail, tile=tile,
                   row_stats=stats)
    if stats:
        exact(out[0], d.ref)
        exact(fp32_sum(out[1]), row_stats_of(d.ref))
    else:
        exact(out, d.ref)


# m, c, n, ranges, batch from test_lnlin_plain_variant_bias_residual_rowstats_grouped: ragged M, 10 ranges, and the grouped forms with 2 and 10
LNLIN_CASES = [c for c in _params(T.test_lnlin_plain_variant_bias_residual_rowstats_grouped) if c in ((129, 640, 32, 1, 0), (300, 320, 640, 10, 0),
                                                                                                      (4096, 320, 320, 2, 3), (1024, 640, 640, 10, 3))]
assert len(LNLIN_CASES) == 4
register(gemm_data, [kw(m=m, n=n, k=c, nb=max(b, 1), stats=True, seed=6) for m, c, n, rg, b in LNLIN_CASES])


@gpu
@pytest.mark.parametrize("m,c,n,ranges,batch", LNLIN_CASES)
def test_exact_lnlin_plain_variant(ops, m, c, n, ranges, batch):
    nb = max(batch, 1)
    d = gemm_data(m=m, n=n, k=c, nb=nb, stats=True, seed=6)
    check(d)
    wp = torch.cat([ops.pack_linear(dev32(d.w[b])) for b in range(nb)]).contiguous()
    npad = wp.shape[0] // nb
    bias = torch.zeros(nb, npad)
    bias[:, :n] = d.bias.float()
    got, st = ops.gemm(dev16(d.a), wp, n, c, bias=bias.reshape(-1).cuda(), resid=dev16(d.resid), tile=50, splits=ranges, batch=batch, row_stats=True)
    assert st.shape[0] == ranges
    exact(got, d.ref)
    exact(fp32_sum(st), row_stats_of(d.ref))


WS_GEMM_CASES = [c for c in _params(T.test_gemm_weight_streaming_kernel) if c in ((100, 128, 96, 1, 0), (333, 704, 320, 3, 64))]  # ragged M; tail + 3 slices
assert len(WS_GEMM_CASES) == 2
register(gemm_data, [kw(m=m, n=n, k=k, stats=True, seed=7) for m, k, n, s, tl in WS_GEMM_CASES])


@gpu
@pytest.mark.experimental
@pytest.mark.parametrize("m,k,n,splits,tail", WS_GEMM_CASES)
def test_exact_gemm_weight_streaming(ops, m, k, n, splits, tail):
    needs_experimental_build(ops)
    d = gemm_data(m=m, n=n, k=k, stats=True, seed=7)
    check(d)
    ka = k - tail
    wp = ops.pack_linear(dev32(d.w[0]))
    bp = torch.zeros(wp.shape[0])
    bp[:n] = d.bias[0].float()
    got, st = ops.gemm(dev16(d.a[:, :ka].contiguous()), wp, n, ka, tile=55, splits=splits, wfr=ops.pack_linear_ws(wp, n, k), row_stats=True, bias=bp.cuda(),
                       resid=dev16(d.resid), tail=dev16(d.a[:, ka:].contiguous()) if tail else None)
    exact(got, d.ref)
    exact(fp32_sum(st), row_stats_of(d.ref))


# ---------------------------------------------------------------- 6. implicit-GEMM conv
def conv_key(case, f32=False, ones=False):
    b, h, w, cin, cout, stride, pad, ups, out_hw = case
    return kw(b=b, h=h, w=w, cin=cin, cout=cout, stride=stride, pad=pad, ups=ups, out_hw=out_hw, f32=f32, ones=ones, seed=10)


# every explicit tile runs the three cases whose gather is not the plain one: stride 2 with pad (0, 1, 0, 1), the 2x upsample, 16 channels
# (taps straddle k-blocks)
CONV_ALWAYS = [c for c in CONV_CASES if (c[5] == 2 and c[6] == 0) or c[7] or c[3] == 16]
assert len(CONV_ALWAYS) == 3
CONV_EXACT = [(c, t, f32) for t in CONV_TILES for c in (CONV_CASES if t == -1 else CONV_ALWAYS) for f32 in (False, "staged") if not (f32 and t in NO_F32_TILES)]
register(conv_data, [conv_key(c, f32) for c, t, f32 in CONV_EXACT])


def run_conv(ops, case, d, tile, f32, **more):
    b, h, w, cin, cout, stride, pad, ups, out_hw = case
    return ops.conv3x3(dev16(d.x), ops.pack_conv(dev32(d.w)), cout, stride=stride, pad=pad, upsample=ups, bias=dev32(d.bias) if d.bias is not None else None,
                       resid=dev16(d.resid) if d.resid is not None else None, out_hw=out_hw, tile=tile, flags=f32flag(f32), **more)


@gpu
@pytest.mark.parametrize("case,tile,f32", CONV_EXACT)
def test_exact_conv3x3(ops, case, tile, f32):
    d = data(conv_data, conv_key(case, f32))
    check(d)
    exact(run_conv(ops, case, d, tile, f32), d.ref, kind="conv")


# x = 1 and W = 1: every output is (taps inside the image) * Cin, whatever the draw; fp16 and fp32 out
ONES_CASES = [(c, f32) for c in CONV_CASES for f32 in (False, "staged")]
register(conv_data, [conv_key(c, f32, ones=True) for c, f32 in ONES_CASES])


@gpu
@pytest.mark.parametrize("case,f32", ONES_CASES)
def test_exact_conv3x3_all_ones_counts_the_taps_inside_the_image(ops, case, f32):
    d = data(conv_data, conv_key(case, f32, ones=True))
    check(d)
    assert d.max_ref == 9 * case[3] or case[1] < 3
    exact(run_conv(ops, case, d, -1, f32), d.ref, kind="conv")


# ---------------------------------------------------------------- 7. fused 1x1 shortcut: implicit, halo, weight-streaming
def smallest(cases, work, count, need_splits=()):
    """the `count` cheapest cases + the cheapest one for every split count in need_splits that is not among them"""
    order = sorted(cases, key=work)
    pick = order[:count]
    for s in need_splits:
        if not any(c[-1] == s for c in pick):
            pick += [c for c in order if c[-1] == s][:1]
    return pick


def _sc_work(c):  # b, h, cin, cin2, cout, tile, splits
    return c[0] * c[1] * c[1] * (9 * c[2] + c[3]) * c[4]


SC_IMPLICIT = smallest(_params(T.test_conv3x3_fused_shortcut), _sc_work, 3, (3,))
SC_HALO = smallest(_params(T.test_conv3x3_halo_fused_shortcut), _sc_work, 3, (3, 7))
SC_WS = smallest(_params(T.test_conv3x3_weight_streaming_fused_shortcut), _sc_work, 3, (3,))
SC_CASES = [("implicit", c, f32) for c in SC_IMPLICIT for f32 in (False, True if c[6] >= 2 else "staged") if not (f32 and c[5] in NO_F32_TILES)] + \
           [("halo", c, False) for c in SC_HALO] + [("ws", c, False) for c in SC_WS]


def sc_key(c, f32):
    b, h, cin, cin2, cout, tile, splits = c
    return kw(b=b, h=h, w=h, cin=cin, cout=cout, cin2=cin2, resid=False, f32=f32, seed=11)


register(conv_data, [sc_key(c, f32) for form, c, f32 in SC_CASES])


@gpu
@pytest.mark.parametrize("form,case,f32", SC_CASES)
def test_exact_conv3x3_fused_shortcut(ops, form, case, f32):
    """[im2col(t) | x] . [W3 | W1]^T; the K slices cut the k-block sequence anywhere (3 and 7 do not divide the block counts)"""
    b, h, cin, cin2, cout, tile, splits = case
    d = data(conv_data, sc_key(case, f32))
    check(d)
    w3, w1 = dev32(d.w), dev32(d.w1)
    w1p = ops.pack_conv(w1)[:, :cin2]
    wp = torch.cat([ops.pack_conv(w3)[:, : 9 * cin], w1p], dim=1).contiguous()
    more = {}
    if form == "halo":
        more["wcb"] = torch.cat([ops.pack_conv_cb(w3), w1p], dim=1).contiguous()
    if form == "ws":
        more["wfr"] = ops.pack_conv_ws(w3, w1)
    got = ops.conv3x3(dev16(d.x), wp, cout, bias=dev32(d.bias), tail=dev16(d.x2), tile=tile, splits=splits, flags=f32flag(f32), **more)
    exact(got, d.ref, kind="conv")


# ---------------------------------------------------------------- 8. conv_halo
def _halo_work(c):  # b, h, w, cin, cout, variant, splits
    return c[0] * c[1] * c[2] * c[3] * c[4]


HALO_VARIANTS = sorted({c[5] for c in HALO_CASES})
HALO_EXACT = [min((c for c in HALO_CASES if c[5] == v), key=_halo_work) for v in HALO_VARIANTS]
HALO_EXACT += [c for c in HALO_CASES if c[:5] == (1, 24, 40, 128, 128) and c not in HALO_EXACT]  # the non-square map
assert (1, 24, 40, 128, 128) in [c[:5] for c in HALO_EXACT]
register(conv_data, [kw(b=b, h=h, w=w, cin=cin, cout=cout, seed=12) for b, h, w, cin, cout, v, s in HALO_EXACT])


@gpu
@pytest.mark.parametrize("case", HALO_EXACT)
def test_exact_conv3x3_halo_kernel(ops, case):
    b, h, w, cin, cout, variant, splits = case
    d = conv_data(b=b, h=h, w=w, cin=cin, cout=cout, seed=12)
    check(d)
    wf = dev32(d.w)
    got = ops.conv3x3(dev16(d.x), ops.pack_conv(wf), cout, bias=dev32(d.bias), resid=dev16(d.resid), wcb=ops.pack_conv_cb(wf), tile=variant, splits=splits)
    exact(got, d.ref, kind="conv")


# ---------------------------------------------------------------- 9. convws
def _ws_hw(h):
    return h if isinstance(h, tuple) else (h, h)


def _ws_work(c):  # b, h, cin, cout, tile, splits
    return c[0] * _ws_hw(c[1])[0] * _ws_hw(c[1])[1] * c[2] * c[3]


WS_TILES = sorted({c[4] for c in WS_CASES})
WS_EXACT = [c for t in WS_TILES for c in sorted((c for c in WS_CASES if c[4] == t), key=_ws_work)[:2]]  # on 53 / 54 these are the non-square maps
assert {c[1] for c in WS_EXACT} >= {(24, 32), (8, 48)}
WS_RAGGED_TILES = [t for t in WS_TILES if t >= 53]  # the builds that take GF_RAGGED (conv_ws.hip: variants 2 / 3)
WS_RAGGED = [(2, hw, 128, 192, t, 1) for t in WS_RAGGED_TILES for hw in ((17, 17), (13, 7))]
register(conv_data, [kw(b=b, h=_ws_hw(h)[0], w=_ws_hw(h)[1], cin=cin, cout=cout, seed=13) for b, h, cin, cout, t, s in WS_EXACT + WS_RAGGED])


@gpu
@pytest.mark.parametrize("case", WS_EXACT + WS_RAGGED)
def test_exact_conv3x3_weight_streaming_kernel(ops, case):
    """split launches through the slab reduce, unsplit ones through the kernel's own combine and epilogue; whole and ragged maps"""
    b, hw, cin, cout, tile, splits = case
    h, w = _ws_hw(hw)
    d = conv_data(b=b, h=h, w=w, cin=cin, cout=cout, seed=13)
    check(d)
    wf = dev32(d.w)
    ragged = GF_RAGGED if (h % 8 or w % 16) and tile >= 53 else 0
    got = ops.conv3x3(dev16(d.x), ops.pack_conv(wf), cout, bias=dev32(d.bias), resid=dev16(d.resid), wfr=ops.pack_conv_ws(wf), tile=tile, splits=splits,
                      flags=ragged)
    exact(got, d.ref, kind="conv")


WS_UPS = [(1, 5, 256, 128, t) for t in WS_RAGGED_TILES]  # 5 x 5 -> 9 x 9: the upsample cropped by one row / column
register(conv_data, [kw(b=b, h=hi, w=hi, cin=cin, cout=cout, ups=True, out_hw=(2 * hi - 1, 2 * hi - 1), resid=False, seed=14) for b, hi, cin, cout, t in WS_UPS])


@gpu
@pytest.mark.parametrize("b,hi,cin,cout,tile", WS_UPS)
def test_exact_conv3x3_weight_streaming_upsample_to_odd_size(ops, b, hi, cin, cout, tile):
    ho = 2 * hi - 1
    d = conv_data(b=b, h=hi, w=hi, cin=cin, cout=cout, ups=True, out_hw=(ho, ho), resid=False, seed=14)
    check(d)
    wf = dev32(d.w)
    got = ops.conv3x3(dev16(d.x), ops.pack_conv(wf), cout, upsample=True, out_hw=(ho, ho), bias=dev32(d.bias), wfr=ops.pack_conv_ws(wf), tile=tile, splits=1,
                      flags=GF_RAGGED)
    exact(got, d.ref, kind="conv")


# 32 groups of 10 and of 40 channels: groups straddle the 64-channel n-ranges
WS_GN = [(2, (16, 16), 64, 320, 53), (2, (16, 16), 64, 320, 54), (1, (16, 32), 128, 1280, 53), (1, (16, 32), 128, 1280, 54)]
register(conv_data, [kw(b=b, h=hw[0], w=hw[1], cin=cin, cout=cout, gn_groups=32, seed=15) for b, hw, cin, cout, t in WS_GN])


@gpu
@pytest.mark.parametrize("b,hw,cin,cout,tile", WS_GN)
def test_exact_conv3x3_weight_streaming_groupnorm_statistics(ops, b, hw, cin, cout, tile):
    h, w = hw
    d = conv_data(b=b, h=h, w=w, cin=cin, cout=cout, gn_groups=32, seed=15)
    check(d)
    wf = dev32(d.w)
    y, st = ops.conv3x3(dev16(d.x), ops.pack_conv(wf), cout, bias=dev32(d.bias), resid=dev16(d.resid), wfr=ops.pack_conv_ws(wf), tile=tile, splits=1, gn_groups=32)
    exact(y, d.ref, kind="conv")
    yf = d.ref.double().reshape(b, h * w, 32, cout // 32)
    want = torch.stack([yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))], dim=-1).float()
    exact(fp32_sum(st.transpose(0, 1)), want)


# ---------------------------------------------------------------- 10. fp8 GEMMs
def e4_bytes(t):
    """integers that e4m3 holds exactly -> their e4m3 codes"""
    b = t.float().to(torch.float8_e4m3fn)
    assert torch.equal(b.float().double(), t.double())
    return b.view(torch.uint8)


def w8_unit_scale(w, dev="cuda"):
    """the e4m3 weight copy in quantize_w8's layout ([roundup(N, 128), roundup(K, 128)] bytes), with scale 1.0"""
    n, k = w.shape
    out = torch.zeros((n + 127) // 128 * 128, (k + 127) // 128 * 128, dtype=torch.uint8)
    out[:n, :k] = e4_bytes(w)
    return out.to(dev)


FP8_CASES = [(m, n, k, 0, t) for m, n, k, t in _params(T.test_gemm_fp8) if (m, n, k) != (700, 640, 1280)] + [(260, 320, 1280, 320, 26), (260, 320, 1280, 320, 28)]
assert {c[4] for c in FP8_CASES} == {24, 25, 26, 27, 28}
register(gemm_data, [kw(m=m, n=n, k=k + k2, act=(-2, 2), stats=t == 26 and k2 > 0, seed=16) for m, n, k, k2, t in FP8_CASES])


@gpu
@pytest.mark.parametrize("m,n,k1,k2,tile", FP8_CASES)
def test_exact_gemm_fp8_weights(ops, m, n, k1, k2, tile):
    """gemm_fp8_kernel (fp16 activations converted while staged, e4m3 weights): bias, residual, the two-operand form, row statistics"""
    stats = tile == 26 and k2 > 0
    d = gemm_data(m=m, n=n, k=k1 + k2, act=(-2, 2), stats=stats, seed=16)
    check(d)
    wp = ops.pack_linear(dev32(d.w[0]))
    q8, qs = ops.quantize_w8(wp, k1 + k2)  # the project's own quantiser keeps these weights exactly as well
    assert torch.equal(q8[:n, :k1 + k2].cpu().view(torch.float8_e4m3fn).float() * qs, d.w[0].float())
    out = ops.gemm(dev16(d.a[:, :k1].contiguous()), wp, n, k1, bias=dev32(d.bias[0]), resid=dev16(d.resid), tail=dev16(d.a[:, k1:].contiguous()) if k2 else None,
                   tile=tile, w8=w8_unit_scale(d.w[0]), w_scale=1.0, a_scale=1.0, row_stats=stats)
    if stats:
        exact(out[0], d.ref)
        exact(fp32_sum(out[1]), row_stats_of(d.ref))
    else:
        exact(out, d.ref)


# m, n, k1, k2, tile, tail scale, e4m3 out
F8F8_CASES = [(96, 1280, 1280, 0, 0, 1.0, False), (200, 320, 320, 0, 0, 1.0, False), (130, 320, 208, 112, 1, 1.0, False), (300, 640, 256, 128, 1, 4.0, False),
              (300, 640, 256, 128, 0, 2.0, False), (130, 192, 64, 0, 1, 1.0, True), (130, 192, 64, 0, 0, 1.0, True)]


def f8f8_key(m, n, k1, k2, tile, ts, out8):
    if out8:  # outputs within e4m3's exact integers: K = 64, thinned weights, bias and residual in {-2..2}
        return kw(m=m, n=n, k=k1, act=(-2, 2), keep=0.125, out_lim=16.0, bres=2, seed=17)
    return kw(m=m, n=n, k=k1 + k2, act=(-2, 2), stats=True, k2=k2 if ts != 1.0 else 0, k2_scale=ts, seed=17)


register(gemm_data, [f8f8_key(*c) for c in F8F8_CASES])


@gpu
@pytest.mark.parametrize("m,n,k1,k2,tile,tail_scale,out8", F8F8_CASES)
def test_exact_gemm_f8f8(ops, m, n, k1, k2, tile, tail_scale, out8):
    """gemm_f8f8_kernel (both operands e4m3): bias, residual, row statistics, the tail at its own power-of-two scale (its integers count
    tail_scale times), and the e4m3 output"""
    d = data(gemm_data, f8f8_key(m, n, k1, k2, tile, tail_scale, out8))
    check(d)
    a8 = e4_bytes(d.a).cuda()
    got, got8, st = ops.gemm_f8f8(a8[:, :k1] if k2 else a8, w8_unit_scale(d.w[0]), n, 1.0, 1.0, k=k1, bias=dev32(d.bias[0]), resid=dev16(d.resid),
                                  tail8=a8[:, k1:] if k2 else None, tail_scale=tail_scale if k2 else None, tile=tile, row_stats=not out8,
                                  out8_scale=1.0 if out8 else None)
    exact(got, d.ref)
    if out8:
        exact(got8.cpu().view(torch.float8_e4m3fn).float(), d.ref)
    else:
        exact(fp32_sum(st), row_stats_of(d.ref))


# ---------------------------------------------------------------- no device needed
def test_exact_case_inputs_satisfy_their_bounds():
    """Every case generator of this file against its conditions (<= 2048, < 2^24, > 2048), on the CPU: an ill-chosen range fails here,
    before any GPU time is spent."""
    n = 0
    for fn, keys in REGISTRY:
        for key in keys:
            d = data(fn, key)
            check(d)
            assert d.keep > 1e-3, (key, d.keep)  # the thinning loops ended because the condition held
            n += 1
    assert n > 0
    every = lambda cases, pos: {c[pos] for c in cases}  # noqa: E731
    assert every(DENSE_CASES, 3) == set(GEMM_TILES) and every(CONV_EXACT, 1) == set(CONV_TILES)
    assert every(HALO_EXACT, 5) == set(HALO_VARIANTS) and every(WS_EXACT, 4) == set(WS_TILES)


def test_exact_sees_what_the_tolerance_accepts():
    """The gap this file closes, without a device, on the split-K case (192 x 1280, K = 11520).  (a) one output element off by ONE product
    of the contraction; (b) in the fp32-out variant, one element of one of two K-slabs rounded to fp16 before the reduce.  close() of
    test_gpu_ops accepts (a) on Gaussian data of the same shape -- there the same slip, one product of typical size, is ~ K^-0.5 = 0.009
    of an output of order 1, under the limit of ~ 0.011 -- and exact() rejects both and names the element."""
    m, n, k = SPLITK_SHAPE
    d = gemm_data(m=m, n=n, k=k, f32=False, seed=2)
    i, j = 100, 700
    # (a) on the Gaussian data of test_gemm_splitk: the element loses the term of typical size, |a| |w| = 1 * K^-0.5
    a, w = T.rnd(m, k, seed=5), T.rnd(n, k, seed=6, scale=k ** -0.5)
    ref_g = F.linear(a.float(), w.float(), torch.randn(n, generator=torch.Generator().manual_seed(7)))
    off_g = ref_g.clone()
    off_g[i, j] += k ** -0.5
    close(off_g, ref_g)  # accepted
    off = d.ref.clone()
    off[i, j] += 1.0  # the same slip on the integer data: one product of size 1
    with pytest.raises(AssertionError, match=r"1 of 245760 elements differ.*\(100, 700\)"):
        exact(off, d.ref)
    # (b) two slabs of the fp32-out variant, one element of the first through fp16
    d32 = gemm_data(m=m, n=n, k=k, f32=True, seed=2)
    half = k // 2
    s0 = d32.a[:, :half] @ d32.w[0][:, :half].t()
    s1 = d32.a[:, half:] @ d32.w[0][:, half:].t()
    cand = (s0.float().half().double() != s0).nonzero()  # partials that fp16 cannot hold
    assert cand.shape[0] > 0
    i2, j2 = cand[0].tolist()
    s0r = s0.clone()
    s0r[i2, j2] = s0[i2, j2].float().half().double()
    got = (s0r + s1 + d32.bias[0] + d32.resid).float()
    rel = (got - d32.ref).abs().max().item() / d32.ref.abs().max().item()
    assert 0 < rel < 2e-3  # far inside what a relative tolerance of 2e-3 lets through
    with pytest.raises(AssertionError, match=rf"1 of 245760 elements differ.*\({i2}, {j2}\)"):
        exact(got, d32.ref)
    exact((s0 + s1 + d32.bias[0] + d32.resid).float(), d32.ref)  # and the unrounded slabs are the reference
