"""Resolutions that are multiples of 8 but not of 64: dtp_create takes them, the ragged builds of convws_kernel and
attn_dma_kernel match fp32 torch, and whole stamps match the fp32 oracle with the sized UNet (tests/sized_unet_ref.py: every non-final
up block upsamples to its skip's size).  R = 72 (latent 9: levels 9, 5, 3, 2) and 136 (17, 9, 5, 3), 4 steps, autotuner off."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import sized_unet_ref

pytestmark = pytest.mark.gpu

TOL = 1e-2
ST = dict(steps=4, context_pad=5, tg_steps=3, cfg_weight=2.0, tg_weight=1.0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def close(got, ref, tol=2e-3):  # the tolerance of the existing convws / attention op tests (tests/test_gpu_ops.py)
    got = got.float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err <= tol * ref.abs().max().item() + tol, err


# ---------------------------------------------------------------- dtp_create
def test_create_accepts_multiples_of_8_and_refuses_the_rest(ops):
    from diffusiontexturepainting_amd import _lib
    lib = _lib.load()
    for r in (72, 136, 200, 360):
        h = C.c_void_p()
        assert lib.dtp_create(0, r, 1, C.byref(h)) == 0, lib.dtp_last_error()
        lib.dtp_destroy(h)
    for r in (60, 100, 0):
        h = C.c_void_p()
        assert lib.dtp_create(0, r, 1, C.byref(h)) != 0
        assert b"multiple of 8" in lib.dtp_last_error()


# ---------------------------------------------------------------- convws_kernel, ragged build
MAPS = [(9, 9), (17, 17), (45, 45), (13, 7)]


@pytest.mark.parametrize("tile", [53, 54])
@pytest.mark.parametrize("hw", MAPS)
def test_convws_ragged_maps(ops, hw, tile):
    from diffusiontexturepainting_amd._lib import GF_RAGGED
    (h, w), b, cin, cout = hw, 2, 128, 192
    x = rnd(b, h, w, cin, seed=201)
    wt = rnd(cout, cin, 3, 3, seed=202, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(203))
    res = rnd(b, h, w, cout, seed=204)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, padding=1).permute(0, 2, 3, 1) + res.float()
    wf = wt.float().cuda()
    got = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), resid=res.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile, splits=1,
                      flags=GF_RAGGED)
    close(got, ref)


@pytest.mark.parametrize("tile,splits", [(53, 1), (54, 2)])
@pytest.mark.parametrize("hw", MAPS)
def test_convws_ragged_fused_shortcut(ops, hw, tile, splits):
    from diffusiontexturepainting_amd._lib import GF_RAGGED
    (h, w), b, cin, cin2, cout = hw, 1, 128, 192, 128
    t, x = rnd(b, h, w, cin, seed=211), rnd(b, h, w, cin2, seed=212)
    w3 = rnd(cout, cin, 3, 3, seed=213, scale=(9 * cin) ** -0.5)
    w1 = rnd(cout, cin2, 1, 1, seed=214, scale=cin2 ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(215))
    ref = F.conv2d(t.float().permute(0, 3, 1, 2), w3.float(), bias, padding=1) + F.conv2d(x.float().permute(0, 3, 1, 2), w1.float())
    wp = torch.cat([ops.pack_conv(w3.float().cuda())[:, : 9 * cin], ops.pack_conv(w1.float().cuda())[:, :cin2]], dim=1).contiguous()
    got = ops.conv3x3(t.cuda(), wp, cout, bias=bias.cuda(), tail=x.cuda(), wfr=ops.pack_conv_ws(w3.float().cuda(), w1.float().cuda()), tile=tile,
                      splits=splits, flags=GF_RAGGED)
    close(got, ref.permute(0, 2, 3, 1))


@pytest.mark.parametrize("tile", [53, 54])
@pytest.mark.parametrize("hi", [23, 5])
def test_convws_ragged_upsample_to_odd_size(ops, tile, hi):
    """The up-block conv at an odd level: nearest to 2 Hi - 1 (= x2 then crop), then the 3x3 conv with zero padding."""
    from diffusiontexturepainting_amd._lib import GF_RAGGED
    b, cin, cout, ho = 1, 256, 128, 2 * hi - 1
    x = rnd(b, hi, hi, cin, seed=221)
    wt = rnd(cout, cin, 3, 3, seed=222, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(223))
    xin = F.interpolate(x.float().permute(0, 3, 1, 2), size=(ho, ho), mode="nearest")
    ref = F.conv2d(xin, wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    wf = wt.float().cuda()
    got = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, upsample=True, out_hw=(ho, ho), bias=bias.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile,
                      splits=1, flags=GF_RAGGED)
    close(got, ref)
    generic = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, upsample=True, out_hw=(ho, ho), bias=bias.cuda(), tile=0, splits=1)
    close(generic, ref)  # the tiled kernel bounds the window by the output size as well


@pytest.mark.parametrize("tile", [53, 54])
@pytest.mark.parametrize("hw", [(17, 17), (45, 45), (13, 7)])
def test_convws_ragged_groupnorm_statistics(ops, hw, tile):
    """GF_GNSTATS on a ragged map: the partial tiles' out-of-map pixels add nothing; summed over the chunks the partials are the group
    sums of the stored tensor, and the apply pass fed with them equals torch's group_norm."""
    from diffusiontexturepainting_amd._lib import GF_RAGGED
    (h, w), b, cin, cout = hw, 2, 128, 320
    x = rnd(b, h, w, cin, seed=231)
    wt = rnd(cout, cin, 3, 3, seed=232, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(233))
    wf = wt.float().cuda()
    y, st = ops.conv3x3(x.cuda(), ops.pack_conv(wf), cout, bias=bias.cuda(), wfr=ops.pack_conv_ws(wf), tile=tile, splits=1, gn_groups=32,
                        flags=GF_RAGGED)
    assert torch.isfinite(st).all()
    yf = y.float().reshape(b, h * w, 32, cout // 32)
    want = torch.stack([yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))], dim=-1)
    got = st.sum(dim=1)
    assert torch.allclose(got, want, rtol=2e-4, atol=2e-2), (got - want).abs().max().item()
    gamma, beta = torch.randn(cout, generator=torch.Generator().manual_seed(234)).cuda(), torch.randn(cout, generator=torch.Generator().manual_seed(235)).cuda()
    z = ops.groupnorm_apply(y, gamma, beta, st, eps=1e-5, silu=True)
    close(z, F.silu(F.group_norm(y.float().permute(0, 3, 1, 2), 32, gamma, beta, eps=1e-5)).permute(0, 2, 3, 1).cpu())


# ---------------------------------------------------------------- attn_dma_kernel, ragged last key tile
@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("s", [81, 289, 2025])
def test_attn_dma_ragged_sequences(ops, d, s):
    heads, b = 8, 2
    assert ops.attention_dma_supported(s, s, heads, d)
    q, k, v = (rnd(b, s, heads * d, seed=241 + i) for i in range(3))
    got = ops.attention_dma(q.cuda(), k.cuda(), v.cuda(), heads)
    qf, kf, vf = (t.float().reshape(b, s, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = torch.softmax(qf @ kf.transpose(-1, -2) * d ** -0.5, dim=-1) @ vf
    close(got, ref.transpose(1, 2).reshape(b, s, heads * d))


# ---------------------------------------------------------------- whole stamps against the oracle with the sized UNet
@pytest.fixture(scope="module")
def sd():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    return dict(unet=W.synthetic_unet(7), lora=W.synthetic_lora(7), vae=W.synthetic_vae(7), clip=W.synthetic_clip(7),
                penc=W.synthetic_patch_encoder(7))


@pytest.fixture(scope="module")
def nets(sd):
    from oracle import nets as N
    return dict(unet=N.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"])


_MODELS = {}


def _model(sd, r):
    if r not in _MODELS:
        from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
        m = MI355ConditionalInpainter(r, device=0, weights=sd, max_batch=2)
        m.set_option("autotune", 0)
        _MODELS[r] = m
    return _MODELS[r]


def _inputs(b, r, seed):
    from diffusiontexturepainting_amd import synthetic
    canvas, brush, lat, eps = synthetic.make_stamp_batch(b, r, seed)
    cond, uncond = synthetic.make_conditioning(seed + 1)
    return canvas, brush, cond, uncond, lat, eps


@pytest.fixture
def sized_oracle(monkeypatch):
    from oracle import nets as N
    monkeypatch.setattr(N, "unet_forward", sized_unet_ref.unet_forward)


@pytest.mark.parametrize("r", [72, 136])
def test_stamp_matches_the_sized_oracle(sd, nets, sized_oracle, r):
    from oracle import pipeline
    m = _model(sd, r)
    canvas, brush, cond, uncond, lat, eps = _inputs(1, r, 300 + r)
    m.set_conditioning(cond, uncond, brush)
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST).cpu()
    ref = pipeline.generate_raw(nets, brush, cond, uncond, canvas, lat, eps, **ST)
    err = (got - ref).abs().max().item()
    print(f"R={r}: max|hip - oracle| = {err:.2e}")
    assert torch.isfinite(got).all() and err <= TOL


@pytest.mark.parametrize("r", [72, 136])
def test_mixed_batch_matches_the_sized_oracle(sd, nets, sized_oracle, r):
    from oracle import pipeline
    m = _model(sd, r)
    per = [dict(cfg_weight=1.5, tg_weight=0.5, tg_steps=1, context_pad=3), dict(cfg_weight=4.0, tg_weight=2.0, tg_steps=3, context_pad=11)]
    ins = [_inputs(1, r, 400 + 10 * r + i) for i in range(2)]
    for slot, (_, brush, cond, uncond, _, _) in enumerate(ins):
        m.set_conditioning(cond, uncond, brush, slot=slot)
    canvas, lat = torch.cat([i[0] for i in ins]), torch.cat([i[4] for i in ins])
    eps = torch.cat([i[5] for i in ins], dim=1)
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1], per_stamp=per, steps=4).cpu()
    for b, st in enumerate(per):
        _, brush, cond, uncond, _, _ = ins[b]
        ref = pipeline.generate_raw(nets, brush, cond, uncond, canvas[b:b + 1], lat[b:b + 1], eps[:, b:b + 1], steps=4, **st)
        err = (got[b:b + 1] - ref).abs().max().item()
        print(f"R={r} stamp {b}: max|hip - oracle| = {err:.2e}")
        assert err <= TOL


def test_dpm_stamp_matches_the_sized_oracle(sd, nets, sized_oracle):
    import sched_ref
    r = 136
    m = _model(sd, r)
    canvas, brush, cond, uncond, lat, eps = _inputs(1, r, 555)
    m.set_conditioning(cond, uncond, brush)
    try:
        m.set_scheduler("DPM")
        got = m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST).cpu()
    finally:
        m.set_scheduler("DDIM")
    ref = sched_ref.generate_raw(nets, brush, cond, uncond, canvas, lat, eps, scheduler="DPM", **ST)
    err = (got - ref).abs().max().item()
    print(f"R={r} DPM: max|hip - oracle| = {err:.2e}")
    assert err <= TOL


def test_graph_replay_equals_eager_at_136(sd):
    m = _model(sd, 136)
    canvas, brush, cond, uncond, lat, eps = _inputs(1, 136, 777)
    m.set_conditioning(cond, uncond, brush)
    graph = m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST).cpu()
    try:
        m.set_option("use_graph", 0)
        eager = m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST).cpu()
    finally:
        m.set_option("use_graph", 1)
    assert torch.equal(graph, eager)


def test_fp8_options_are_refused_at_ragged_resolutions(sd):
    from diffusiontexturepainting_amd import _lib
    m = _model(sd, 72)
    for name in ("fp8_attention", "fp8_linear", "fp8_operands"):
        with pytest.raises(_lib.DtpError, match="not offered at resolution 72"):
            m.set_option(name, 1)
        m.set_option(name, 0)  # switching one off is always fine


def test_profile_shows_the_ragged_fast_paths(sd, tmp_path, monkeypatch):
    """R = 200 (latent 25: levels 25, 13, 7, 4; self-attention S = 625 at d = 40) with the autotuner on: convws_kernel takes ragged maps and
    the level-0 self-attention runs on attn_dma_kernel (S % 64 = 49)."""
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    monkeypatch.setenv("DTP_TUNE_CACHE", str(tmp_path / "tune.txt"))
    m = MI355ConditionalInpainter(200, device=0, weights=sd, max_batch=1)
    canvas, brush, cond, uncond, lat, eps = _inputs(1, 200, 888)
    m.set_conditioning(cond, uncond, brush)
    m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST)  # builds (and tunes) the programs
    m.profile(1)
    m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST)
    m.profile_dump(tmp_path / "prof.csv")
    rows = m.profile_rows()
    m.profile(0)
    kinds = {r["kernel"] for r in rows if r["launches"] > 0}
    lines = (tmp_path / "prof.csv").read_text().splitlines()[1:]
    print(sorted(kinds))
    assert any(k.startswith("convws_kernel<8, 16") for k in kinds), sorted(kinds)
    ragged_hw = {25 * 25, 13 * 13, 7 * 7, 4 * 4}
    ws = [ln for ln in lines if " tile=53 " in ln or " tile=54 " in ln]
    assert any(int(ln.split(" M=")[1].split()[0]) % hw == 0 and int(ln.split(" M=")[1].split()[0]) // hw <= 3 for ln in ws for hw in ragged_hw), ws[:8]
    assert any("Sq=625 Skv=625 D=40 dma" in ln for ln in lines)
