"""Strength < 1 stamps (dtp_stamp_strength, `generate*(strength=...)`): strength 1 against today's entry points byte for byte, the
start-point combine and the step kernel from t_start against torch and the reference's captured chains, whole stamps of every sampler
against the fp32 restatement on the oracle networks (tests/strength_ref.py), the shortened loop's bookkeeping, a mixed two-slot batch,
graph replay across alternating strengths, and the fp8 refusal.  One 64^2 context (+ one 72^2 stamp); oracle stamps run at most 4
evaluations."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import strength_ref

pytestmark = pytest.mark.gpu

R = 64
TOL = 1e-2


@pytest.fixture(scope="module")
def sd():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    return dict(unet=W.synthetic_unet(5), lora=W.synthetic_lora(5), vae=W.synthetic_vae(5), clip=W.synthetic_clip(5),
                penc=W.synthetic_patch_encoder(5))


@pytest.fixture(scope="module")
def env(sd):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from oracle import nets
    model = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=2)
    # fp8 + strength < 1 before any UNet program exists (the fp8 options can only be chosen then), then back to fp16
    canvas, brush, cond, uncond, lat, eps, ieps = _inputs(1, 4000)
    model.set_conditioning(cond, uncond, brush)
    model.set_option("fp8_attention", 1)
    fp8_error = None
    try:
        model.generate_raw(canvas, latents=lat, vae_eps=eps, init_eps=ieps, strength=0.5, steps=4)
    except _lib.DtpError as e:
        fp8_error = str(e)
    model.set_option("fp8_attention", 0)
    return dict(model=model, nets=dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"]), fp8_error=fp8_error)


def _inputs(b, seed, res=R):
    from diffusiontexturepainting_amd import synthetic
    canvas, brush, lat, eps = synthetic.make_stamp_batch(b, res, seed)
    cond, uncond = synthetic.make_conditioning(seed + 1)
    ieps = torch.randn(b, 4, res // 8, res // 8, generator=torch.Generator().manual_seed(seed + 2))
    return canvas, brush, cond, uncond, lat, eps, ieps


def _settings(n, **st):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd.inpainter import DEFAULT_SETTINGS
    s = {**DEFAULT_SETTINGS, **st}
    return _lib.Settings(int(n), int(s["context_pad"]), int(s["tg_steps"]), float(s["cfg_weight"]), float(s["tg_weight"]), 0, 0)


def _call(m, entry, canvas, n, lat, eps, ieps=None, strength=None, **st):
    """One stamp through a named C entry point on the model's handle, B = canvas.shape[0], all slot 0."""
    from diffusiontexturepainting_amd._lib import check, ptr
    dev = torch.device("cuda", 0)
    B = canvas.shape[0]
    c, l, e = canvas.to(dev).contiguous(), lat.to(dev).contiguous(), eps.to(dev).contiguous()
    i = ieps.to(dev).contiguous() if ieps is not None else None
    out = torch.empty(B, 3, R, R, device=dev)
    arr = (type(_settings(n)) * B)(*[_settings(n, **st)] * B)
    torch.cuda.synchronize()
    if entry == "dtp_stamp":
        check(m._lib.dtp_stamp(m._h, ptr(c), arr, ptr(l), ptr(e), ptr(out), B, None), entry)
    elif entry == "dtp_stamp_mixed":
        check(m._lib.dtp_stamp_mixed(m._h, ptr(c), arr, ptr(l), ptr(e), ptr(out), B, None, None), entry)
    else:
        check(m._lib.dtp_stamp_strength(m._h, ptr(c), arr, ptr(l), ptr(e), ptr(i), C.c_double(strength), ptr(out), B, None, None), entry)
    torch.cuda.synchronize()
    return out.cpu()


def test_fp8_options_refuse_strength(env):
    assert env["fp8_error"] is not None and "code 3" in env["fp8_error"] and "fp8" in env["fp8_error"]  # DTP_ERR_STATE


@pytest.mark.parametrize("name", ["DDIM", "DPM", "LMSD"])
def test_strength_one_is_today_byte_for_byte(env, name):
    m = env["model"]
    canvas, brush, cond, uncond, lat, eps, _ = _inputs(1, 4100)
    m.set_conditioning(cond, uncond, brush)
    m.set_scheduler(name)
    st = dict(tg_steps=2, cfg_weight=2.5)
    a = _call(m, "dtp_stamp", canvas, 3, lat, eps, **st)
    b = _call(m, "dtp_stamp_mixed", canvas, 3, lat, eps, **st)
    nan = torch.full_like(lat, float("nan"))  # init_eps is ignored at strength 1
    c = _call(m, "dtp_stamp_strength", canvas, 3, lat, eps, ieps=nan, strength=1.0, **st)
    d = m.generate_raw(canvas, latents=lat, vae_eps=eps, strength=1.0, steps=3, **st).cpu()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), name


def test_strength_init_op_against_torch():
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = torch.Generator().manual_seed(7)
    z0, e = torch.randn(3, 4, 9, 11, generator=g), torch.randn(3, 4, 9, 11, generator=g)
    dev = torch.device("cuda", 0)
    for name, steps, st in (("DDIM", 8, 0.5), ("DPM", 20, 0.35), ("LMSD", 6, 0.5)):
        a, b = ops.strength_schedule(name, steps, st)["noise_coefs"]
        got = ops.strength_init(z0.to(dev), e.to(dev), a, b).cpu()
        want = torch.tensor(a, dtype=torch.float32) * z0 + torch.tensor(b, dtype=torch.float32) * e  # two rounded products, one sum
        assert torch.equal(got, want), name


def test_step_kernel_from_t_start_follows_the_reference(golden_dir):
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = np.load(os.path.join(golden_dir, "strength_chains.npz"))
    dev = torch.device("cuda", 0)
    for k in range(int(g["count"])):
        p = f"{k}_"
        name, n, st = str(g[p + "name"]), int(g[p + "steps"]), float(g[p + "strength"])
        d = ops.strength_schedule(name, n, st)
        assert d["t_start"] == int(g[p + "t_start"])
        row0 = d["t_start"] - (1 if name == "DDIM" else 0)
        t = ops.scheduler_tables(name, n)
        # the start point with the library's pair, then the loop's rows from row0 with the loop index as step_index
        x = ops.strength_init(torch.from_numpy(g[p + "z0"]).to(dev), torch.from_numpy(g[p + "eps"]).to(dev), *d["noise_coefs"])
        ref = g[p + "x_init"]
        assert np.max(np.abs(x.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-5, (name, n, st)
        e = torch.from_numpy(g[p + "e"]).to(dev)
        b = x.shape[0]
        hist = torch.full((3 * x.numel(),), float("nan"), dtype=torch.float32, device=dev)  # nothing may read a previous x0
        for i in range(d["evals"]):
            ops.sched_step(name, t["coefs"][row0 + i], t["in_scale"][row0 + i + 1], torch.cat([e[i], e[i]]), x, hist, [1.0] * b, [0.0] * b,
                           [0] * b, 0, i)
            torch.cuda.synchronize()
            ref = g[p + "chain"][i]
            err = np.max(np.abs(x.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref)))
            assert err <= 1e-5, (name, n, st, i, err)
        if name == "DPM" and n == 20:
            assert t["coefs"][row0][2] == 2.0  # the first evaluated row says second order: the kernel ran it first order


def _stamp_vs_oracle(env, name, n, strength, seed, evals, **st):
    m = env["model"]
    canvas, brush, cond, uncond, lat, eps, ieps = _inputs(1, seed)
    m.set_conditioning(cond, uncond, brush)
    m.set_scheduler(name)
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, init_eps=ieps, strength=strength, steps=n, **st).cpu()
    assert m.stamp_info()["unet_evals"] == evals
    ref = strength_ref.generate_raw(env["nets"], brush, cond, uncond, canvas, lat, eps, ieps, scheduler=name, steps=n, strength=strength,
                                    **st)
    err = (got - ref).abs().max().item()
    print(f"{name} {n} @ {strength}: vs oracle {err:.2e}")
    assert torch.isfinite(got).all() and err <= TOL
    return got, (canvas, lat, eps)


def test_ddim_stamp(env):
    _stamp_vs_oracle(env, "DDIM", 8, 0.5, 4200, 4, tg_steps=2)
    m = env["model"]
    # 4 evaluations, texture guidance for the first 2 counted from t_start: 2 x 3 + 2 x 2 rows
    assert m.stamp_unet_rows() == 3 + 3 + 2 + 2


def test_dpm_stamp(env):
    _stamp_vs_oracle(env, "DPM", 6, 0.7, 4300, 4, tg_steps=6)
    assert env["model"].stamp_unet_rows() == 4 * 3  # tg_steps 6 cut to the 4 evaluations


def test_lmsd_stamp(env):
    _stamp_vs_oracle(env, "LMSD", 6, 0.5, 4400, 3, tg_steps=1, cfg_weight=3.0)


def test_ddim_from_the_canvas_at_the_full_length(env):
    """DDIM 4 steps at 0.8: t_start 1 and 3 evaluations like strength 1, but the start is the canvas noised to timesteps[1]."""
    got, (canvas, lat, eps) = _stamp_vs_oracle(env, "DDIM", 4, 0.8, 4500, 3, tg_steps=2)
    full = env["model"].generate_raw(canvas, latents=lat, vae_eps=eps, steps=4, tg_steps=2).cpu()
    assert (got - full).abs().max().item() > 1e-2


def test_ragged_resolution_stamp(sd, monkeypatch):
    import sized_unet_ref
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from oracle import nets
    monkeypatch.setattr(nets, "unet_forward", sized_unet_ref.unet_forward)  # 9 x 9 latents: the UNet levels are ceil halvings
    r = 72
    m = MI355ConditionalInpainter(r, device=0, weights=dict(unet=sd["unet"], lora=sd["lora"], vae=sd["vae"]), max_batch=1)
    canvas, brush, cond, uncond, lat, eps, ieps = _inputs(1, 4600, res=r)
    m.set_conditioning(cond, uncond, brush)
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, init_eps=ieps, strength=0.5, steps=6, tg_steps=2).cpu()
    assert m.stamp_info()["unet_evals"] == 3
    ref = strength_ref.generate_raw(dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"]), brush, cond, uncond, canvas, lat,
                                    eps, ieps, scheduler="DDIM", steps=6, strength=0.5, tg_steps=2)
    err = (got - ref).abs().max().item()
    print(f"72^2 DDIM 6 @ 0.5: vs oracle {err:.2e}")
    assert torch.isfinite(got).all() and err <= TOL


MIXED = [dict(cfg_weight=1.5, tg_weight=0.0, tg_steps=3, context_pad=5), dict(cfg_weight=4.0, tg_weight=1.5, tg_steps=1, context_pad=17)]


def test_mixed_two_slot_batch(env):
    m = env["model"]
    ins = [_inputs(1, 4700 + i) for i in range(2)]
    for slot, (_, brush, cond, uncond, _, _, _) in enumerate(ins):
        m.set_conditioning(cond, uncond, brush, slot=slot)
    canvas, lat, ieps = torch.cat([i[0] for i in ins]), torch.cat([i[4] for i in ins]), torch.cat([i[6] for i in ins])
    eps = torch.cat([i[5] for i in ins], dim=1)
    m.set_scheduler("DDIM")
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, init_eps=ieps, strength=0.5, slots=[0, 1], per_stamp=MIXED, steps=6).cpu()
    # t_start 3, 3 evaluations; tg_evals (0, 1): rows 4 + 1, 4, 4
    assert m.stamp_info()["unet_evals"] == 3 and m.stamp_unet_rows() == 5 + 4 + 4
    for b, st in enumerate(MIXED):
        _, brush, cond, uncond, _, _, _ = ins[b]
        ref = strength_ref.generate_raw(env["nets"], brush, cond, uncond, canvas[b:b + 1], lat[b:b + 1], eps[:, b:b + 1], ieps[b:b + 1],
                                        scheduler="DDIM", steps=6, strength=0.5, **st)
        err = (got[b:b + 1] - ref).abs().max().item()
        print(f"stamp {b} {st}: vs oracle {err:.2e}")
        assert err <= TOL


def test_alternating_strengths_replay_without_waiting(env):
    m = env["model"]
    canvas, brush, cond, uncond, lat, eps, ieps = _inputs(2, 4800)
    m.set_conditioning(cond, uncond, brush)
    m.set_scheduler("DPM")
    dev = torch.device("cuda", 0)
    kw = dict(latents=lat.to(dev), vae_eps=eps.to(dev), init_eps=ieps.to(dev), steps=8, tg_steps=2)
    canvas = canvas.to(dev)
    for s in (0.5, 0.3):  # programs, graphs and the 3B encoder exist from here on
        m.generate_raw(canvas, strength=s, **kw)
    torch.cuda.synchronize()
    # the stream is held busy for well over a host enqueue; a table rebuild (or any wait) inside the calls would outlast it
    ms_per_1e6 = None
    if hasattr(torch.cuda, "_sleep"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(m.stream):
            e0.record()
            torch.cuda._sleep(1_000_000)
            e1.record()
        e1.synchronize()
        ms_per_1e6 = max(e0.elapsed_time(e1), 1e-3)
    outs = []
    m.stream.wait_stream(torch.cuda.current_stream())
    if ms_per_1e6 is not None:
        with torch.cuda.stream(m.stream):
            torch.cuda._sleep(int(1_000_000 * 400.0 / ms_per_1e6))  # ~400 ms
    t0 = time.perf_counter()
    for s in (0.5, 0.3, 0.5):
        outs.append(m.generate_raw(canvas, strength=s, **kw))
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    print(f"3 stamps enqueued in {host_ms:.1f} ms behind a ~400 ms busy stream")
    if ms_per_1e6 is not None:
        assert host_ms < 200.0
    assert m.stamp_info()["unet_evals"] == 4
    outs = [o.cpu() for o in outs]
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    try:
        m.set_option("use_graph", 0)
        for s, o in zip((0.5, 0.3), outs):
            assert torch.equal(m.generate_raw(canvas, strength=s, **kw).cpu(), o), s
    finally:
        m.set_option("use_graph", 1)


def test_python_arguments(env):
    m = env["model"]
    canvas, brush, cond, uncond, lat, eps, ieps = _inputs(1, 4900)
    m.set_conditioning(cond, uncond, brush)
    for s in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            m.generate(canvas, strength=s)
    with pytest.raises(ValueError, match="init_eps"):
        m.generate(canvas, strength=0.5, init_eps=torch.zeros(2, 4, 8, 8))
    from diffusiontexturepainting_amd import _lib
    m.set_scheduler("DDIM")
    with pytest.raises(_lib.DtpError, match="strength"):
        m.generate(canvas, strength=0.1, steps=8)  # int(0.8) = 0: no evaluation
    u8 = m.generate_u8(canvas, strength=0.5, steps=4)  # every generate entry takes it; init_eps drawn internally
    assert u8.dtype == torch.uint8 and u8.shape == (1, R, R, 3)
    # the draws at strength 1 are today's: latents and vae_eps from the generator, no third draw
    m.generator.manual_seed(11)
    a = m.generate_raw(canvas, steps=3).cpu()
    m.generator.manual_seed(11)
    b = m.generate_raw(canvas, steps=3, strength=1.0, init_eps=torch.zeros(5)).cpu()
    assert torch.equal(a, b)
