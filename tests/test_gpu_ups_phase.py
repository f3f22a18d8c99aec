"""The phase build of the weight-streaming conv (tile ids 56 / 57): a 3x3 conv over the nearest-2x upsample run as four
2x2 convs over the stored map.  Through the op entry (dtp_op_conv_ups4) with the tile forced:

  * the device packing of the collapsed weights equals its CPU restatement (tests/ups_phase_ref.py) bit for bit;
  * the output against fp32 torch, with test_conv3x3's helper and tolerance;
  * integer operands (tests/test_gpu_exact.py): weights in {-1, 0, 1}, so every sum of up to four of them is an integer of magnitude
    <= 4 <= 2048, exact in fp16 -- the collapsed weights are exact and the output has to equal the float64 reference bit for bit;
  * the GroupNorm partial sums, totalled over the chunks, are the statistics of the stored tensor;
  * what the predicate refuses, and that such a problem still runs right on the nine-tap path;
  * one 64^2 stamp with the tile forced wherever it applies, inside the project's pixel gate.

Shapes (B, Hi, Wi, Cin, Cout): one source tile and one channel block (the loop's last-block form alone); two blocks and an odd n-tile
count (the zero n-tile); four tiles and three blocks (all three forms of the block loop); 32 groups of 10 channels straddling the
64-channel n-ranges."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_exact import LIM24, Data, _finish, _ranges, check, exact, fp32_sum, ints, thin
from test_gpu_ops import close, rnd
from ups_phase_ref import pack_ups4

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 16, 64, 64, 0), (3, 8, 16, 128, 96, 0), (2, 16, 32, 192, 64, 0), (1, 16, 32, 64, 320, 32)]  # ..., gn_groups
TILES = [56, 57]
CASES = [(s, t) for s in SHAPES for t in TILES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def gauss(b, h, w, cin, cout):
    """Gaussian operands and the fp32 torch reference of conv(upsample(x)) + bias + residual, NHWC; shared by the tests, left unchanged"""
    x = rnd(b, h, w, cin, seed=91)
    wt = rnd(cout, cin, 3, 3, seed=92, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(93))
    xin = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    res = rnd(*ref.shape, seed=94)
    return Data(x=x, w=wt, bias=bias, resid=res, ref=ref + res.float())


@functools.lru_cache(maxsize=None)
def integers(b, h, w, cin, cout, gn_groups):
    """Integer operands (the fp16-out ranges of test_gpu_exact) and the float64 reference; with gn_groups the weights are thinned until
    the per-(image, group) sums of squares of the output are < 2^24, as conv_data does"""
    (alo, ahi), (wlo, whi) = _ranges(False)
    assert 4 * max(abs(wlo), abs(whi)) <= 2048  # every sum of up to four weights is exact in fp16
    x = ints((b, h, w, cin), alo, ahi, 6100)
    w0 = ints((cout, cin, 3, 3), wlo, whi, 7100)
    bv = ints((cout,), -8, 8, 9610)
    r = ints((b, 2 * h, 2 * w, cout), -8, 8, 9710)
    xin = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    keep = 0.25 if gn_groups else 1.0
    while True:
        wt = thin(w0, keep, 9510)
        acc = F.conv2d(xin, wt, None, padding=1).permute(0, 2, 3, 1).contiguous()
        absum = F.conv2d(xin.abs(), wt.abs(), None, padding=1).permute(0, 2, 3, 1) + bv.abs() + r.abs()
        ref = acc + bv + r
        sq = None
        if gn_groups:
            yf = ref.reshape(b, -1, gn_groups, cout // gn_groups)
            sq = (yf * yf).sum(dim=(1, 3)).max().item()
        if not gn_groups or sq < LIM24 or keep < 1e-3:
            break
        keep /= 2
    return _finish(Data(x=x, w=wt, bias=bv, resid=r, keep=keep), ref, absum, False, sq, acc=acc)


@pytest.mark.parametrize("shape", SHAPES)
def test_device_packing_equals_the_cpu_restatement(ops, shape):
    _, _, _, cin, cout, _ = shape
    wt = gauss(*shape[:5]).w.float()
    got = ops.pack_conv_ws_ups4(wt.cuda()).cpu()
    want = pack_ups4(wt)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))  # bit for bit (also the sign of a zero)


def _run(ops, d, cout, tile, gn_groups, **kw):
    wf = d.w.float().cuda()
    return ops.conv3x3(d.x.half().cuda(), ops.pack_conv(wf), cout, upsample=True, bias=d.bias.float().cuda(), resid=d.resid.half().cuda(),
                       wfr=ops.pack_conv_ws(wf), wfr4=ops.pack_conv_ws_ups4(wf), tile=tile, splits=1, gn_groups=gn_groups, **kw)


@pytest.mark.parametrize("shape,tile", CASES)
def test_phase_conv_against_fp32_torch(ops, shape, tile):
    b, h, w, cin, cout, gn = shape
    d = gauss(b, h, w, cin, cout)
    assert ops.conv_ws_supported(d.x.cuda(), ops.pack_conv(d.w.float().cuda()), cout, tile, upsample=True, wfr4=ops.pack_conv_ws_ups4(d.w.float().cuda()))
    out = _run(ops, d, cout, tile, gn)
    y, st = out if gn else (out, None)
    close(y, d.ref)
    if gn:  # the statistics of the STORED tensor, as test_conv3x3_weight_streaming_emits_groupnorm_statistics checks for the nine-tap build
        assert torch.isfinite(st).all()  # every (chunk, group) slot was written
        yf = y.float().reshape(b, 4 * h * w, gn, cout // gn)
        want = torch.stack([yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))], dim=-1)
        got = st.sum(dim=1)
        assert torch.allclose(got, want, rtol=2e-4, atol=2e-2), (got - want).abs().max().item()
        gamma, beta = torch.randn(cout, generator=torch.Generator().manual_seed(95)).cuda(), torch.randn(cout, generator=torch.Generator().manual_seed(96)).cuda()
        z = ops.groupnorm_apply(y, gamma, beta, st, eps=1e-5, silu=True)
        ref = F.silu(F.group_norm(y.float().permute(0, 3, 1, 2), gn, gamma, beta, eps=1e-5)).permute(0, 2, 3, 1)
        close(z, ref.cpu())


@pytest.mark.parametrize("shape,tile", CASES)
def test_phase_conv_is_exact_on_integer_operands(ops, shape, tile):
    b, h, w, cin, cout, gn = shape
    d = integers(b, h, w, cin, cout, gn)
    check(d)
    out = _run(ops, d, cout, tile, gn)
    y, st = out if gn else (out, None)
    exact(y, d.ref, kind="conv")
    if gn:
        yf = d.ref.double().reshape(b, 4 * h * w, gn, cout // gn)
        want = torch.stack([yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))], dim=-1).float()
        exact(fp32_sum(st.transpose(0, 1)), want)


@pytest.mark.parametrize("tile", TILES)
def test_predicate_refuses_the_cropped_upsample_and_the_fused_shortcut(ops, tile):
    b, h, w, cin, cout = 1, 8, 16, 64, 64
    from diffusiontexturepainting_amd._lib import GF_RAGGED
    x = rnd(b, h, w, cin, seed=97)
    wt = rnd(cout, cin, 3, 3, seed=98, scale=(9 * cin) ** -0.5)
    wf = wt.float().cuda()
    wp, wfr, wfr4 = ops.pack_conv(wf), ops.pack_conv_ws(wf), ops.pack_conv_ws_ups4(wf)
    assert ops.conv_ws_supported(x.cuda(), wp, cout, tile, upsample=True, wfr=wfr, wfr4=wfr4)
    assert not ops.conv_ws_supported(x.cuda(), wp, cout, tile, upsample=True, wfr=wfr)          # no phase weights
    assert not ops.conv_ws_supported(x.cuda(), wp, cout, tile, splits=2, upsample=True, wfr=wfr, wfr4=wfr4)  # unsplit only
    assert not ops.conv_ws_supported(x.cuda(), wp, cout, tile, wfr=wfr, wfr4=wfr4)               # not a conv over the upsample
    # the upsample cropped by one row / column: the row behind the crop is padding, not data
    crop = (2 * h - 1, 2 * w - 1)
    assert not ops.conv_ws_supported(x.cuda(), wp, cout, tile, upsample=True, out_hw=crop, flags=GF_RAGGED, wfr=wfr, wfr4=wfr4)
    assert ops.conv_ws_supported(x.cuda(), wp, cout, tile - 3, upsample=True, out_hw=crop, flags=GF_RAGGED, wfr=wfr, wfr4=wfr4)  # 53 / 54 take it
    xin = F.interpolate(x.float().permute(0, 3, 1, 2), size=crop, mode="nearest")
    ref = F.conv2d(xin, wt.float(), None, padding=1).permute(0, 2, 3, 1)
    close(ops.conv3x3(x.cuda(), wp, cout, upsample=True, out_hw=crop, flags=GF_RAGGED, wfr=wfr, wfr4=wfr4), ref)  # heuristic tile
    # a fused 1x1 shortcut over a second tensor
    cin2 = 64
    tail = rnd(b, 2 * h, 2 * w, cin2, seed=99)
    w1 = rnd(cout, cin2, 1, 1, seed=100, scale=cin2 ** -0.5)
    wp2 = torch.cat([wp[:, : 9 * cin], ops.pack_conv(w1.float().cuda())[:, :cin2]], dim=1).contiguous()  # as test_conv3x3_fused_shortcut
    wfr2 = ops.pack_conv_ws(wf, w1.float().cuda())
    assert not ops.conv_ws_supported(x.cuda(), wp2, cout, tile, upsample=True, tail=tail.cuda(), wfr=wfr2, wfr4=wfr4)
    xin = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ref = (F.conv2d(xin, wt.float(), None, padding=1) + F.conv2d(tail.float().permute(0, 3, 1, 2), w1.float())).permute(0, 2, 3, 1)
    close(ops.conv3x3(x.cuda(), wp2, cout, upsample=True, tail=tail.cuda(), wfr=wfr2, wfr4=wfr4), ref)  # heuristic tile, nine-tap path


R = 64


@pytest.mark.parametrize("force", [2, 3])
def test_stamp_with_the_phase_tiles_forced_against_the_oracle(force, tmp_path):
    """One 64^2 stamp, autotuner off, tile 56 (force = 2) / 57 (3) wherever the predicate takes the launch -- at this size the VAE decoder's
    16^2 -> 32^2 and 32^2 -> 64^2 upsamplers -- within the 1e-2 pixel gate of test_gpu_engine.py."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    sd = dict(unet=W.synthetic_unet(1), lora=W.synthetic_lora(1), vae=W.synthetic_vae(1))
    g = torch.Generator().manual_seed(21)
    canvas = torch.rand(1, 4, R, R, generator=g)
    canvas[:, 3:] = 0
    canvas[0, 3, : R // 2, : R // 2] = 1
    brush = torch.rand(1, 3, R, R, generator=g)
    cond, uncond = torch.randn(1, 14, 768, generator=g), torch.randn(1, 14, 768, generator=g)
    lat, eps = torch.randn(1, 4, R // 8, R // 8, generator=g), torch.randn(2, 1, 4, R // 8, R // 8, generator=g)
    st = dict(steps=4, context_pad=10, tg_steps=4, width=R, cfg_weight=2.0, tg_weight=1.0)
    ref = _oracle_stamp(sd, brush, cond, uncond, canvas, lat, eps, st)
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    m.set_option("autotune", 0)
    m.set_option("ups_phase", force)
    m.set_conditioning(cond, uncond, brush)
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, **st)
    torch.cuda.synchronize()
    err = (got.cpu() - ref).abs().max().item()
    print("stamp max abs err", err)
    assert err <= 1e-2
    m.profile(True)
    m.generate_raw(canvas, latents=lat, vae_eps=eps, **st)
    dump = tmp_path / "launches.csv"
    m.profile_dump(dump)
    m.profile(False)
    labels = [ln for ln in open(dump) if " ups" in ln]
    assert sum(f"tile={54 + force} " in ln and " ups4" in ln for ln in labels) == 2, labels  # the two aligned VAE upsamplers ran on the forced tile


_ORACLE = {}


def _oracle_stamp(sd, brush, cond, uncond, canvas, lat, eps, st):
    """the CPU pipeline's stamp, computed once for both forced tiles"""
    from oracle import nets, pipeline
    if "ref" not in _ORACLE:
        merged = nets.merge_lora(sd["unet"], sd["lora"])
        _ORACLE["ref"] = pipeline.generate_raw(dict(unet=merged, vae=sd["vae"]), brush, cond, uncond, canvas, lat, eps, **st)
    return _ORACLE["ref"]
