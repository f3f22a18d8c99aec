"""Seeded stamps (dtp_stamp_seeded, `generate*(seeds=...)`): the device draws against the numpy restatement (tests/noise_ref.py) and
their moments, a seeded stamp against the same stamp fed the same numbers through the caller-tensor entry points byte for byte, its
independence of batch order and size, the untouched generator, enqueue without a host wait or a re-capture, and one oracle stamp.
One 64^2 context, max_batch 4, DDIM, 4 steps."""
import time

import numpy as np
import pytest
import torch

import noise_ref

pytestmark = pytest.mark.gpu

R, H = 64, 8
N = 4 * H * H
TOL = 1e-2       # the project's pixel gate (test_gpu_engine.py)
TOL_SOLO = 1e-2  # a stamp against its own solo run: the margin tests/test_gpu_mixed_settings.py uses (its TOL; that file has no 2e-3)
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
TOP = (1 << 64) - 1


@pytest.fixture(scope="module")
def sd():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import weights as W
    return dict(unet=W.synthetic_unet(5), lora=W.synthetic_lora(5), vae=W.synthetic_vae(5), clip=W.synthetic_clip(5),
                penc=W.synthetic_patch_encoder(5))


@pytest.fixture(scope="module")
def env(sd):
    from diffusiontexturepainting_amd import synthetic
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from oracle import nets
    model = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=4)
    ins = []
    for slot in range(4):  # four clients: a canvas and a brush each
        canvas, brush, _, _ = synthetic.make_stamp_batch(1, R, 6000 + slot)
        cond, uncond = synthetic.make_conditioning(6100 + slot)
        model.set_conditioning(cond, uncond, brush, slot=slot)
        ins.append((canvas, brush, cond, uncond))
    return dict(model=model, ins=ins, canvas=torch.cat([i[0] for i in ins]),
                nets=dict(unet=nets.merge_lora(sd["unet"], sd["lora"]), vae=sd["vae"]))


def _draws(seeds):
    """(latents [B,4,h,h], vae_eps [2,B,4,h,h], init_eps [B,4,h,h]) of the stamps seeded `seeds`, from the device op."""
    from diffusiontexturepainting_amd import ops
    d = [[ops.stamp_noise(s, k, N).view(4, H, H) for s in seeds] for k in range(4)]
    return torch.stack(d[0]), torch.stack([torch.stack(d[1]), torch.stack(d[2])]), torch.stack(d[3])


def test_device_draws_match_the_restatement():
    """<= 1e-5: fp32 spacing at |z| ~ 6 is 4.8e-7 and a few ulp each of logf, sqrtf and sincosf stay below it; fast intrinsics do not."""
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    worst = 0.0
    for n in (N, 4 * 64 * 64):  # one workgroup; several
        for seed in (0, 12345, TOP):
            for draw in range(4):
                got = ops.stamp_noise(seed, draw, n).cpu().numpy()
                err = float(np.abs(got.astype(np.float64) - noise_ref.normals(seed, draw, n, np.float64)).max())
                worst = max(worst, err)
                assert err <= 1e-5, (seed, draw, n, err)
    print(f"max |device - float64 restatement| over 24 draws: {worst:.2e}")


def test_moments_and_independence_of_draws_and_seeds():
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    n, s = 1 << 20, 987654321
    a, b, c = (ops.stamp_noise(sd_, d, n).cpu().numpy() for sd_, d in ((s, 0), (s, 1), (s + 1, 0)))
    for z, what in ((a, "draw 0"), (b, "draw 1"), (c, "seed + 1")):
        noise_ref.check_moments(z, what)  # n = 2^20: |mean| <= 5e-3, |var - 1| <= 1e-2, finite, max |z| <= 5.9
    r_draw, r_seed = noise_ref.correlation(a, b), noise_ref.correlation(a, c)
    print(f"mean {a.mean():+.2e} var {a.var():.5f} max {np.abs(a).max():.3f}; rho(draw 0, 1) {r_draw:+.2e}, rho(s, s + 1) {r_seed:+.2e}")
    assert not np.array_equal(a, b) and abs(r_draw) <= 1e-2
    assert not np.array_equal(a, c) and abs(r_seed) <= 1e-2


@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_seeded_equals_the_same_numbers_through_the_caller_tensors(env, strength):
    m = env["model"]
    seeds = [31, TOP - 5]
    canvas = env["canvas"][:2]
    lat, eps, ieps = _draws(seeds)
    got = m.generate_raw(canvas, seeds=seeds, strength=strength, slots=[0, 1], **ST).cpu()
    want = m.generate_raw(canvas, latents=lat, vae_eps=eps, init_eps=ieps, strength=strength, slots=[0, 1], **ST).cpu()
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert m.stamp_info()["unet_evals"] == (3 if strength == 1.0 else 2)
    # an int seed is seed + b per stamp
    again = m.generate_raw(env["canvas"][:2], seeds=31, strength=strength, slots=[0, 1], **ST).cpu()
    lat2, eps2, ieps2 = _draws([31, 32])
    want2 = m.generate_raw(canvas, latents=lat2, vae_eps=eps2, init_eps=ieps2, strength=strength, slots=[0, 1], **ST).cpu()
    assert torch.equal(again, want2) and torch.equal(again[0], got[0]) and not torch.equal(again[1], got[1])


def test_means_instead_of_vae_draws(env):
    m = env["model"]
    seeds = [8, 9]
    canvas = env["canvas"][:2]
    lat, eps, _ = _draws(seeds)
    got = m.generate_raw(canvas, seeds=seeds, vae_eps=False, **ST).cpu()
    want = m.generate_raw(canvas, latents=lat, vae_eps=False, **ST).cpu()
    sampled = m.generate_raw(canvas, latents=lat, vae_eps=eps, **ST).cpu()
    assert torch.equal(got, want) and not torch.equal(got, sampled)
    got5 = m.generate_raw(canvas, seeds=seeds, vae_eps=False, init_eps=False, strength=0.5, **ST).cpu()
    want5 = m.generate_raw(canvas, latents=lat, vae_eps=False, init_eps=False, strength=0.5, **ST).cpu()
    assert torch.equal(got5, want5)


def test_batch_order_and_batch_size_do_not_reach_the_draws(env):
    m = env["model"]
    seeds, slots = [100, 5, TOP, 77], [0, 1, 2, 3]
    canvas = env["canvas"]
    base = m.generate_raw(canvas, seeds=seeds, slots=slots, **ST).cpu()
    perm = [2, 0, 3, 1]
    got = m.generate_raw(canvas[perm], seeds=[seeds[p] for p in perm], slots=[slots[p] for p in perm], **ST).cpu()
    assert torch.equal(got, base[perm])  # same B: the stamps move with their (canvas, seed, slot), bit for bit
    solo = m.generate_raw(canvas[2:3], seeds=[seeds[2]], slots=[2], **ST).cpu()
    err = (base[2:3] - solo).abs().max().item()
    print(f"member 2 of B = 4 against its solo stamp {err:.2e}")
    assert err <= TOL_SOLO  # (the tile choice may differ per batch size; the draws do not)


def test_the_generator_of_unseeded_stamps_is_left_alone(env):
    m = env["model"]
    canvas = env["canvas"][:1]
    m.generator.manual_seed(11)
    first = m.generate(canvas, **ST).cpu()
    second = m.generate(canvas, strength=0.5, **ST).cpu()
    m.generator.manual_seed(11)
    assert torch.equal(m.generate(canvas, **ST).cpu(), first)
    m.generate(canvas, seeds=3, **ST)
    m.generate_u8(canvas, seeds=[4], strength=0.5, **ST)
    assert torch.equal(m.generate(canvas, strength=0.5, **ST).cpu(), second)  # the stream did not move
    for kw in (dict(latents=torch.zeros(1, 4, H, H)), dict(vae_eps=torch.zeros(2, 1, 4, H, H)), dict(init_eps=torch.zeros(1, 4, H, H))):
        with pytest.raises(ValueError, match="exclusive"):
            m.generate(canvas, seeds=1, **kw, **ST)
    with pytest.raises(ValueError, match="seeds"):
        m.generate(canvas, seeds=[1, 2], **ST)


def test_seeded_stamps_enqueue_without_a_wait_or_a_recapture(env):
    m = env["model"]
    dev = torch.device("cuda", 0)
    canvas = env["canvas"][:2].to(dev)
    lat, eps, _ = _draws([1, 2])
    kw = dict(slots=[0, 1], **ST)
    m.generate_raw(canvas, latents=lat, vae_eps=eps, **kw)
    nodes_unseeded = m.stamp_info()["graph_nodes"]
    m.generate_raw(canvas, seeds=[1, 2], **kw)  # programs and graphs exist from here on
    torch.cuda.synchronize()
    assert m.stamp_info()["graph_nodes"] == nodes_unseeded > 0  # the three captured stages of the unseeded stamp, replayed
    # the stream is held busy for well over a host enqueue; a wait or a capture inside the calls would outlast it
    ms_per_1e6 = None
    if hasattr(torch.cuda, "_sleep"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(m.stream):
            e0.record()
            torch.cuda._sleep(1_000_000)
            e1.record()
        e1.synchronize()
        ms_per_1e6 = max(e0.elapsed_time(e1), 1e-3)
    m.stream.wait_stream(torch.cuda.current_stream())
    if ms_per_1e6 is not None:
        with torch.cuda.stream(m.stream):
            torch.cuda._sleep(int(1_000_000 * 400.0 / ms_per_1e6))  # ~400 ms
    outs, nodes = [], []
    t0 = time.perf_counter()
    for seeds in ([1, 2], [TOP, 7], [1, 2]):
        outs.append(m.generate_raw(canvas, seeds=seeds, **kw))
        nodes.append(m.stamp_info()["graph_nodes"])
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    print(f"3 seeded stamps enqueued in {host_ms:.1f} ms behind a ~400 ms busy stream; graph nodes {nodes}")
    if ms_per_1e6 is not None:
        assert host_ms < 200.0
    assert nodes == [nodes_unseeded] * 3
    outs = [o.cpu() for o in outs]
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    try:
        m.set_option("use_graph", 0)  # eager launches: the same stamp
        assert torch.equal(m.generate_raw(canvas, seeds=[TOP, 7], **kw).cpu(), outs[1])
    finally:
        m.set_option("use_graph", 1)


def test_seeded_stamp_against_the_oracle(env):
    from oracle import pipeline
    m = env["model"]
    canvas, brush, cond, uncond = env["ins"][3]
    seed = 0xC0FFEE1234567890
    got = m.generate_raw(canvas, seeds=[seed], slots=[3], **ST).cpu()
    lat, eps, _ = _draws([seed])
    ref = pipeline.generate_raw(env["nets"], brush, cond, uncond, canvas, lat.cpu(), eps.cpu(), **ST)
    err = (got - ref).abs().max().item()
    print(f"seeded 64^2 stamp, 4 DDIM steps: vs oracle {err:.2e}")
    assert torch.isfinite(got).all() and err <= TOL
