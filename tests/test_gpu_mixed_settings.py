"""Stamps with different guidance settings in one call (dtp_stamp_mixed, `per_stamp=`): every stamp gets what it would get alone,
the texture-guided UNet rows of finished stamps leave the batch, uniform batches keep today's path, and the serving core batches
clients whose sliders differ.  One 64^2 context, steps <= 4, B <= 4."""
import numpy as np
import pytest
import torch

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
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from oracle import nets
    model = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=8)
    return dict(model=model, nets=dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"]))


def _inputs(b, seed):
    from diffusiontexturepainting_amd import synthetic
    canvas, brush, lat, eps = synthetic.make_stamp_batch(b, R, seed)
    cond, uncond = synthetic.make_conditioning(seed + 1)
    return canvas, brush, cond, uncond, lat, eps


def _solo(m, canvas, lat, eps, b, slot, st):
    return m.generate_raw(canvas[b:b + 1], latents=lat[b:b + 1], vae_eps=eps[:, b:b + 1], slots=[slot], **st).cpu()


# stamps spanning the Kit sliders: cfg 1..6, texture guidance 0..4, tg_steps 0..20 and several dilation pads
MIXED = [dict(cfg_weight=1.0, tg_weight=0.0, tg_steps=0, context_pad=5),
         dict(cfg_weight=2.0, tg_weight=1.0, tg_steps=1, context_pad=9),
         dict(cfg_weight=4.5, tg_weight=4.0, tg_steps=3, context_pad=17),
         dict(cfg_weight=6.0, tg_weight=2.5, tg_steps=20, context_pad=150)]


@pytest.fixture(scope="module")
def four_slots(env):
    m = env["model"]
    ins = [_inputs(1, 2000 + i) for i in range(4)]
    for slot, (_, brush, cond, uncond, _, _) in enumerate(ins):
        m.set_conditioning(cond, uncond, brush, slot=slot)
    canvas, lat = torch.cat([i[0] for i in ins]), torch.cat([i[4] for i in ins])
    eps = torch.cat([i[5] for i in ins], dim=1)
    return ins, canvas, lat, eps


def test_mixed_batch_matches_the_oracle_and_the_solo_stamps(env, four_slots):
    from oracle import pipeline
    m = env["model"]
    ins, canvas, lat, eps = four_slots
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], per_stamp=MIXED, steps=4).cpu()
    assert torch.isfinite(got).all()
    for b, st in enumerate(MIXED):
        _, brush, cond, uncond, _, _ = ins[b]
        ref = pipeline.generate_raw(env["nets"], brush, cond, uncond, canvas[b:b + 1], lat[b:b + 1], eps[:, b:b + 1], steps=4, **st)
        solo = _solo(m, canvas, lat, eps, b, b, dict(steps=4, **st))
        e_ref, e_solo = (got[b:b + 1] - ref).abs().max().item(), (got[b:b + 1] - solo).abs().max().item()
        print(f"stamp {b} {st}: vs oracle {e_ref:.2e}, vs solo {e_solo:.2e}")
        assert e_ref <= TOL and e_solo <= TOL


def test_row_independent_coefficients_are_bit_exact(env, four_slots):
    """Same tg_evals, different cfg / tg / context_pad: the programs of a uniform batch, so stamp b equals stamp b of a uniform call
    with stamp b's settings bit for bit."""
    m = env["model"]
    _, canvas, lat, eps = four_slots
    per = [dict(cfg_weight=1.5, tg_weight=0.5, tg_steps=2, context_pad=3), dict(cfg_weight=3.0, tg_weight=2.0, tg_steps=5, context_pad=11),
           dict(cfg_weight=5.5, tg_weight=4.0, tg_steps=20, context_pad=150), dict(cfg_weight=2.0, tg_weight=1.0, tg_steps=3, context_pad=1)]
    got = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], per_stamp=per, steps=3).cpu()
    for b, st in enumerate(per):
        uni = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], steps=3, **st).cpu()
        assert torch.equal(got[b], uni[b]), b


def test_uniform_per_stamp_takes_todays_path(env, four_slots):
    m = env["model"]
    _, canvas, lat, eps = four_slots
    st = dict(steps=4, context_pad=9, tg_steps=2, cfg_weight=2.5, tg_weight=1.5)
    base = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], **st).cpu()
    info = m.stamp_info()
    same = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], per_stamp=[dict(st)] * 4, **st).cpu()
    assert torch.equal(same, base) and m.stamp_info()["graph_nodes"] == info["graph_nodes"]
    assert m.stamp_unet_rows() == 2 * 12 + 8  # two evaluations on 3B rows, one on 2B


def test_finished_stamps_leave_the_unet_batch(env, four_slots):
    m = env["model"]
    _, canvas, lat, eps = four_slots
    per = [dict(tg_steps=0), dict(tg_steps=3), dict(tg_steps=1), dict(tg_steps=0)]  # tg_evals (0, 3, 1, 0): k = 2, 1, 1
    m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2, 3], per_stamp=per, steps=4, tg_weight=1.0)
    torch.cuda.synchronize()
    assert m.stamp_unet_rows() == 10 + 9 + 9


def test_graph_replay_equals_eager(env, four_slots):
    m = env["model"]
    _, canvas, lat, eps = four_slots
    kw = dict(latents=lat, vae_eps=eps, slots=[3, 2, 1, 0], per_stamp=MIXED, steps=4)
    graph = m.generate_raw(canvas, **kw).cpu()
    try:
        m.set_option("use_graph", 0)
        eager = m.generate_raw(canvas, **kw).cpu()
    finally:
        m.set_option("use_graph", 1)
    assert torch.equal(graph, eager)


def test_more_profiles_than_the_graph_cache_holds(env, four_slots):
    """B = 3, steps = 4: 20 sorted tg_evals profiles, more than the loop-graph cache keeps; each stamp still equals its solo run."""
    import itertools
    m = env["model"]
    _, canvas, lat, eps = four_slots
    canvas, lat, eps = canvas[:3], lat[:3], eps[:, :3]
    st = dict(steps=4, cfg_weight=2.0, tg_weight=1.0, context_pad=9)
    solo = {(b, t): _solo(m, canvas, lat, eps, b, b, dict(st, tg_steps=t)) for b in range(3) for t in range(4)}
    profiles = sorted({tuple(sorted(p, reverse=True)) for p in itertools.product(range(4), repeat=3)})
    assert len(profiles) == 20
    first = None
    for p in profiles + profiles[:1]:
        ts = p[::-1]  # the stamps arrive in ascending order: the engine sorts them
        got = m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=[0, 1, 2], per_stamp=[dict(tg_steps=t) for t in ts], **st).cpu()
        for b, t in enumerate(ts):
            assert (got[b:b + 1] - solo[(b, t)]).abs().max().item() <= TOL, (p, b)
        if first is None:
            first = got
    assert torch.equal(got, first)  # the first profile, evicted and captured again


def _every_stamp_path(m, canvas, lat, eps, init_eps):
    """One stamp through each kind of call (B = 2, 4 steps): [(output, graph nodes)].  Ends on the DDIM sampler it starts with."""
    kw = dict(latents=lat, vae_eps=eps, slots=[0, 1], steps=4)
    seeded = dict(slots=[0, 1], steps=4, seeds=7)
    calls = [lambda: m.generate_raw(canvas, **kw),
             lambda: m.generate_raw(canvas, per_stamp=[dict(tg_steps=1), dict(tg_steps=3)], **kw),
             lambda: m.generate_raw(canvas, strength=0.5, init_eps=init_eps, **kw),
             lambda: m.generate_raw(canvas, strength=0.5, init_eps=False, **dict(kw, vae_eps=False)),
             lambda: m.generate_raw(canvas, **seeded),
             lambda: m.generate_raw(canvas, strength=0.5, **seeded)]
    got = []
    try:
        for i in range(8):
            if i >= 6:
                m.set_scheduler("DPM" if i == 6 else "DDIM")
            out = calls[i if i < 6 else 0]().cpu()
            got.append((out, m.stamp_info()["graph_nodes"]))
    finally:
        m.set_scheduler("DDIM")
    return got


def test_call_kinds_on_one_handle_do_not_share_captured_stages(env, four_slots):
    """Plain, per_stamp, strength < 1 with and without its draws, seeded, seeded below strength 1 and a sampler switch, twice through on
    one handle: a captured encode or loop stage replayed for a call of another kind would give other numbers than the first pass and
    than the same calls without graphs."""
    m = env["model"]
    _, canvas, lat, eps = four_slots
    canvas, lat, eps = canvas[:2], lat[:2], eps[:, :2]
    init_eps = torch.randn(2, 4, R // 8, R // 8, generator=torch.Generator().manual_seed(11))
    first = _every_stamp_path(m, canvas, lat, eps, init_eps)
    second = _every_stamp_path(m, canvas, lat, eps, init_eps)
    try:
        m.set_option("use_graph", 0)
        eager = _every_stamp_path(m, canvas, lat, eps, init_eps)
    finally:
        m.set_option("use_graph", 1)
    for i, ((a, na), (b, nb), (e, _)) in enumerate(zip(first, second, eager)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(b, a), f"call {i}: the second pass differs from the first"
        assert torch.equal(e, a), f"call {i}: graph replay differs from eager"
        assert nb == na and na > 0, (i, na, nb)


def test_dilation_with_one_pad_per_image(env):
    from diffusiontexturepainting_amd import ops
    from oracle import pipeline
    canvas = _inputs(5, 77)[0].cuda()
    pads = [1, 2, 9, 150, R + 11]
    got = ops.dilate_alpha_pads(canvas, pads).cpu()
    for b, pad in enumerate(pads):
        ref = pipeline.dilate_flat(canvas[b:b + 1, 3:].cpu(), pad)
        assert torch.equal(got[b:b + 1], ref), pad


def test_argument_errors_name_the_problem(env, sd, four_slots):
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    m = env["model"]
    _, canvas, lat, eps = four_slots
    kw = dict(latents=lat[:2], vae_eps=eps[:, :2], slots=[0, 1])
    with pytest.raises(DtpError, match="per call"):
        m.generate_raw(canvas[:2], per_stamp=[dict(steps=3), dict(steps=4)], **kw)
    with pytest.raises(DtpError, match="context_pad=0 of stamp 1"):
        m.generate_raw(canvas[:2], per_stamp=[dict(), dict(context_pad=0)], steps=3, **kw)
    with pytest.raises(DtpError, match="steps=1 of stamp 0"):
        m.generate_raw(canvas[:2], per_stamp=[dict(steps=1), dict(steps=1)], **kw)
    with pytest.raises(DtpError, match="no brush set in slot 9"):
        m.generate_raw(canvas[:2], latents=lat[:2], vae_eps=eps[:, :2], slots=[0, 9], per_stamp=[dict(), dict(cfg_weight=3.0)], steps=3)
    nine = canvas[[0, 1, 2, 3, 0, 1, 2, 3, 0]]
    with pytest.raises(DtpError, match="B=9, max 8"):
        m.generate_raw(nine, latents=lat[[0] * 9], vae_eps=eps[:, [0] * 9], per_stamp=[dict()] * 9, steps=3)
    # the library checks composite / output_u8 too (the Python API sets them per call)
    import ctypes as C
    from diffusiontexturepainting_amd._lib import Settings, check, ptr
    st = (Settings * 2)(Settings(3, 9, 3, 2.0, 1.0, 0, 0), Settings(3, 9, 3, 2.0, 1.0, 1, 0))
    out = torch.empty(2, 3, R, R, device="cuda")
    c, la, ep = canvas[:2].cuda(), lat[:2].cuda(), eps[:, :2].contiguous().cuda()
    with pytest.raises(DtpError, match="stamp 1 has steps=3 composite=1"):
        check(m._lib.dtp_stamp_mixed(m._h, ptr(c), st, ptr(la), ptr(ep), ptr(out), 2, None, C.c_void_p(0)), "dtp_stamp_mixed")
    st[1].composite, st[1].output_u8 = 0, 1
    with pytest.raises(DtpError, match="output_u8=1"):
        check(m._lib.dtp_stamp_mixed(m._h, ptr(c), st, ptr(la), ptr(ep), ptr(out), 2, None, C.c_void_p(0)), "dtp_stamp_mixed")
    # fp8 options: stamps of one batch must share tg_evals (uniform batches still run); checked before any program is built
    f8 = MI355ConditionalInpainter(R, device=0, weights=dict(unet=sd["unet"], lora=sd["lora"], vae=sd["vae"]), max_batch=2, fp8_operands=True)
    ins = four_slots[0]
    f8.set_conditioning(ins[0][2], ins[0][3], ins[0][1])
    with pytest.raises(DtpError, match="fp8"):
        f8.generate_raw(canvas[:2], latents=lat[:2], vae_eps=eps[:, :2], per_stamp=[dict(tg_steps=0), dict(tg_steps=2)], steps=3)
    f8._lib.dtp_destroy(f8._h)
    f8._h = None


class _FixedNoise:
    """The operator with per-slot noise, so a batched reply can be compared with the same client's solo stamp."""

    def __init__(self, m, noise):
        self.m, self.noise = m, noise

    def resolution(self):
        return self.m.resolution()

    def device(self):
        return self.m.device()

    def set_brush(self, image, slot=0):
        self.m.set_brush(image, slot=slot)

    def slot_image(self, slot):
        return self.m.slot_image(slot)

    def generate(self, canvas, slots=None, per_stamp=None, **settings):
        lat = torch.cat([self.noise[s][0] for s in slots])
        eps = torch.cat([self.noise[s][1] for s in slots], dim=1)
        return self.m.generate(canvas, latents=lat, vae_eps=eps, slots=slots, per_stamp=per_stamp, **settings)


def test_server_batches_clients_with_different_sliders(env):
    from diffusiontexturepainting_amd import server as S, server_io as sio
    m = env["model"]
    ins = [_inputs(1, 3000 + i) for i in range(2)]
    model = _FixedNoise(m, {s: (ins[s][4], ins[s][5]) for s in range(2)})
    srv = S.StampServer([model], max_batch=8, error_replies=True, gather_window_s=0.3, mixed_settings=True)
    rng = np.random.default_rng(5)
    hdrs = {"a": dict(steps=3, width=R, context_pad=9, cfg_weight=2.0, tg_weight=1.0, tg_steps=3),
            "b": dict(steps=3, width=R, context_pad=21, cfg_weight=5.0, tg_weight=2.0, tg_steps=1)}
    out = {"a": [], "b": []}
    for cid in out:
        brush = rng.integers(0, 256, size=(R, R + 7, 4), dtype=np.uint8)
        hdr = sio.encode_inference_settings(**hdrs[cid])
        job = srv.on_message(cid, sio.encode_request_type(sio.RequestType.NEW_BRUSH_IMAGE) + hdr + sio.encode_new_brush_image_request(brush),
                             out[cid].append)
        assert job.done.wait(60) and job.error is None
    canv = {cid: rng.integers(0, 256, size=(R, R, 4), dtype=np.uint8) for cid in out}
    for c in canv.values():
        c[..., 3] = np.where(rng.random((R, R)) > 0.5, 255, 0)
    jobs = [srv.on_message(cid, sio.encode_request_type(sio.RequestType.NEW_STAMP) + sio.encode_inference_settings(**hdrs[cid])
                           + sio.image_to_binary(canv[cid]), out[cid].append) for cid in out]
    assert all(j.done.wait(60) and j.error is None for j in jobs)
    q = srv.queues[0]
    assert q.batch_sizes[-1] == 2
    for cid in out:
        rep = sio.decode_response(out[cid][1])
        assert rep["type"] == sio.RequestType.RETURN_STAMP.value
        known = canv[cid][..., 3] == 255
        assert np.array_equal(rep["image"][known], canv[cid][..., :3][known])  # painted pixels come back bit-exact
        slot = q.clients[cid]
        st = {k: v for k, v in hdrs[cid].items() if k != "width"}
        solo = model.generate(S.np_to_torch(canv[cid]).unsqueeze(0).to(m.device()), slots=[slot], **st).cpu()
        diff = np.abs(rep["image"].astype(np.int32) - S.torch_to_np(solo[0]).astype(np.int32)).max()
        print(f"client {cid}: max u8 difference to its solo stamp {diff}")
        assert diff <= 4  # 1e-2 of the 0..255 range + one level of truncation
    srv.close()
