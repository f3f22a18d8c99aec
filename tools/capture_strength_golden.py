"""Generate the strength fixtures under tests/golden/strength_*.npz by running the REFERENCE's own code:
StableDiffusionPipeline.initialize_timesteps (stable_diffusion_pipeline.py:348-355), the add_noise and step() of its three ported
schedulers (utilities.py:267-367 LMSDiscreteScheduler, :370-529 DDIMScheduler, :649-1008 DPMScheduler) and InpaintPipeline.infer
(inpaint_pipeline.py:52-153) with a `strength`.

TEST INFRASTRUCTURE, like tools/capture_scheduler_golden.py, whose pattern it follows: oracle/capture_reference.py's `install_stubs` and
the fake engines of oracle/fakes.py.  Runs only where the reference tree exists; nothing from the reference is copied -- the outputs are
data (inputs + expected outputs).

The reference's infer() has the strength parameter and shortens its loop with it (t_start, step_offset), but the lines that would
start from an init image are commented out (inpaint_pipeline.py:120,127,131-134): it always starts from pure noise.  The orchestration
fixtures therefore replace `initialize_latents` by the scheduler's own add_noise of the init image's latents at t_start,
`scheduler.add_noise(encode_image(init_image), noise, t_start, timesteps[t_start])` -- diffusers' inpainting rule.  That composes only
reference functions (initialize_timesteps, encode_image, add_noise); everything after it is the reference's infer() unchanged.

    python tools/capture_strength_golden.py     # rewrites tests/golden/strength_*.npz

Written:
  strength_schedule.npz   per scheduler and N in NS, for every strength in STRENGTHS: t_start, the number of evaluated timesteps and
                          the add_noise pair (a, b) = (add_noise(1, 0), add_noise(0, 1)) at t_start (NaN where nothing is evaluated)
  strength_chains.npz     per CHAINS entry: add_noise(z0, eps) at t_start and the step() chain from a fresh set_timesteps over fixed
                          random model outputs, step_offset = t_start
  strength_orch_<sampler>.npz   per ORCH entry: InpaintPipeline(scheduler=...).infer(strength=...) with the fake engines at R = 32
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import capture_reference as cr  # noqa: E402

NS = (2, 6, 8, 10, 20, 50)
# 0.58 at 50 steps: the float32 product 50 * 0.58 truncates to 29, the double one (Python's) to 28; 0.35, 0.45, 0.7, 0.9, 0.95 at
# 10 / 20 / 50 steps: a float32-held strength truncates one lower than the double one
STRENGTHS = (0.05, 0.1, 0.15, 0.3, 0.35, 0.45, 0.5, 0.55, 0.58, 0.7, 0.75, 0.8, 0.9, 0.95, 0.99, 1.0)
SCHEDS = ("DDIM", "DPM", "LMSD")
CHAINS = [("DDIM", 8, 0.5), ("DDIM", 20, 0.75), ("DDIM", 20, 0.95), ("DPM", 6, 0.7), ("DPM", 20, 0.5), ("DPM", 20, 0.35),
          ("LMSD", 6, 0.5), ("LMSD", 20, 0.3)]
ORCH = [("DDIM", 8, 0.5, 2.0, 1.0, 2, 21), ("DPM", 6, 0.7, 2.0, 1.0, 6, 22), ("LMSD", 6, 0.5, 3.0, 1.0, 1, 23)]


def _scheduler(name, n):
    """A fresh scheduler configured for n steps, as the pipeline constructs it (stable_diffusion_pipeline.py:109-127) and
    update_infer_settings configures it (inpaint_pipeline.py:44-50).  Fresh per n: DDIM's configure() gathers its table in place and
    DPM's appends to its lists."""
    import utilities
    kw = dict(device="cpu", num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, prediction_type="epsilon")
    s = dict(DDIM=utilities.DDIMScheduler, DPM=utilities.DPMScheduler, LMSD=utilities.LMSDiscreteScheduler)[name](**kw)
    s.set_timesteps(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s.configure()
    return s


def _init_timesteps(s, n, strength):
    """The reference's own initialize_timesteps, on a stand-in `self` that holds only what it reads."""
    import stable_diffusion_pipeline as sdp
    me = types.SimpleNamespace(scheduler=s, device="cpu")
    return sdp.StableDiffusionPipeline.initialize_timesteps(me, n, strength)


def capture_schedule():
    out = {}
    one, zero = torch.ones(1), torch.zeros(1)
    for name in SCHEDS:
        rows = []
        for n in NS:
            for st in STRENGTHS:
                s = _scheduler(name, n)
                ts, t_start = _init_timesteps(s, n, st)
                e = len(ts)
                a = b = float("nan")
                if e > 0:
                    a = float(s.add_noise(one, zero, t_start, ts[0])[0])
                    b = float(s.add_noise(zero, one, t_start, ts[0])[0])
                rows.append((n, st, t_start, e, a, b))
        arr = np.array(rows, dtype=np.float64)
        out[f"{name}_steps"] = arr[:, 0].astype(np.int64)
        out[f"{name}_strength"] = arr[:, 1]
        out[f"{name}_t_start"] = arr[:, 2].astype(np.int64)
        out[f"{name}_evals"] = arr[:, 3].astype(np.int64)
        out[f"{name}_a"] = arr[:, 4].astype(np.float32)
        out[f"{name}_b"] = arr[:, 5].astype(np.float32)
    return out


def capture_chains():
    out = {}
    for k, (name, n, st) in enumerate(CHAINS):
        s = _scheduler(name, n)
        ts, t_start = _init_timesteps(s, n, st)  # set_timesteps again: fresh history (sdp:349)
        g = torch.Generator().manual_seed(300 + k)
        z0 = torch.randn(2, 4, 3, 3, generator=g)
        eps = torch.randn(2, 4, 3, 3, generator=g)
        e = torch.randn(len(ts), 2, 4, 3, 3, generator=g)
        x = s.add_noise(z0, eps, t_start, ts[0])
        x_init, chain = x.clone(), []
        for i, t in enumerate(ts):
            x = s.step(e[i], x, t_start + i, t)  # denoise_latent with step_offset = t_start (sdp:455)
            chain.append(x.clone())
        p = f"{k}_"
        out[p + "name"], out[p + "steps"], out[p + "strength"], out[p + "t_start"] = name, np.int64(n), np.float64(st), np.int64(t_start)
        out[p + "z0"], out[p + "eps"], out[p + "e"] = z0.numpy(), eps.numpy(), e.numpy()
        out[p + "x_init"], out[p + "chain"] = x_init.numpy(), torch.stack(chain).numpy()
    out["count"] = np.int64(len(CHAINS))
    return out


def capture_orch(k, sched, steps, strength, cfg, tg, tg_steps, seed, R=32):
    import inpaint_pipeline
    import stable_diffusion_pipeline as sdp
    from oracle import fakes

    sdp.device_view = lambda t: t
    torch.cuda.synchronize = lambda *a, **kw: None
    pipe = inpaint_pipeline.InpaintPipeline(scheduler=sched, guidance_scale=cfg, denoising_steps=steps,
                                            texture_guidance_steps=tg_steps, version="1.5", hf_token="",
                                            max_batch_size=16, device="cpu")
    pipe.generator = torch.Generator().manual_seed(42)
    pipe.scheduler.set_timesteps(steps)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pipe.scheduler.configure()
    pipe.events = {f"{s}-{m}": None for s in ("clip", "denoise", "vae", "vae_encoder") for m in ("start", "stop")}
    calls = []

    def fake(model_name, feed):
        calls.append(model_name)
        if model_name == "unet":
            return {"latent": fakes.fake_unet(feed["sample"], feed["timestep"], feed["encoder_hidden_states"])}
        if model_name == "vae_encoder":
            return {"latent": fakes.fake_vae_encoder(feed["images"])}
        return {"images": fakes.fake_vae_decoder(feed["latent"])}

    pipe.runEngine = fake
    g = torch.Generator().manual_seed(seed)
    h = R // 8
    # conditioning in 96 repeats of 8 random columns: the fake UNet reads only its mean, and the fixture stays small
    cond = torch.randn(1, 14, 8, generator=g).repeat(1, 1, 96)
    uncond = torch.randn(1, 14, 8, generator=g).repeat(1, 1, 96)
    masked = torch.rand(1, 3, R, R, generator=g) * 2 - 1
    mask = (torch.rand(1, 1, R, R, generator=g) > 0.5).float()
    ctx_img = torch.rand(1, 3, R, R, generator=g) * 2 - 1
    ctx_mask = torch.rand(1, 1, R, R, generator=g)
    init_image = torch.rand(1, 3, R, R, generator=g) * 2 - 1
    lat = torch.randn((1, 4, h, h), generator=torch.Generator().manual_seed(42), dtype=torch.float32)
    pipe.scheduler.beta_start, pipe.scheduler.beta_end = 0.00085, 0.012
    pipe.update_infer_settings(denoising_steps=steps, guidance_scale=cfg, texture_guidance_scale=tg,
                               texture_guidance_steps=tg_steps)
    start = {}

    def initialize_latents(batch_size, unet_channels, latent_height, latent_width):
        # the noise is `lat`, the N(0, 1) draw the reference's initialize_latents takes from pipe.generator (seed 42) before it
        # scales it by init_noise_sigma; the start point is add_noise of the init image's latents at t_start
        noise = lat.clone()
        ts, t_start = pipe.initialize_timesteps(pipe.denoising_steps, strength)
        x = pipe.scheduler.add_noise(pipe.encode_image(init_image), noise, t_start, ts[0])
        start.update(t_start=t_start, evals=len(ts), x_init=x.clone())
        return x

    pipe.initialize_latents = initialize_latents
    trace = []
    orig_step = pipe.scheduler.step

    def step(*a, **kw):
        r = orig_step(*a, **kw)
        trace.append(r.clone())
        return r

    pipe.scheduler.step = step
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = pipe.infer(prompt=cond, negative_prompt=uncond, input_image=masked, mask_image=mask,
                         context_masked_image=ctx_img, context_mask=ctx_mask, image_height=R, image_width=R, strength=strength)
    p = f"{k}_"
    return {p + "cond": cond.numpy(), p + "uncond": uncond.numpy(), p + "masked": masked.numpy(), p + "mask": mask.numpy(),
            p + "ctx_img": ctx_img.numpy(), p + "ctx_mask": ctx_mask.numpy(), p + "init_image": init_image.numpy(),
            p + "latents": lat.numpy(), p + "x_init": start["x_init"].numpy(), p + "out": out.numpy(),
            p + "trace": torch.stack(trace).numpy(), p + "n_unet": np.int64(calls.count("unet")), p + "scheduler": sched,
            p + "t_start": np.int64(start["t_start"]), p + "evals": np.int64(start["evals"]),
            p + "settings": np.array([R, steps, strength, cfg, tg, tg_steps], dtype=np.float64)}


def main():
    cr.install_stubs()
    np.savez_compressed(os.path.join(cr.GOLD, "strength_schedule.npz"), **capture_schedule())
    np.savez_compressed(os.path.join(cr.GOLD, "strength_chains.npz"), **capture_chains())
    names = ["strength_schedule.npz", "strength_chains.npz"]
    for c in ORCH:
        d = {k[2:]: v for k, v in capture_orch(0, *c).items()}
        names.append(f"strength_orch_{c[0].lower()}.npz")
        np.savez_compressed(os.path.join(cr.GOLD, names[-1]), **d)
        print(names[-1], c, "unet calls", int(d["n_unet"]), "t_start", int(d["t_start"]))
    for f in names:
        print(f, os.path.getsize(os.path.join(cr.GOLD, f)), "bytes")


if __name__ == "__main__":
    main()
