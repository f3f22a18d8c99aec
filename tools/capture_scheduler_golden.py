"""Generate the DPM-Solver++ and LMS fixtures under tests/golden/ by running the REFERENCE's own
schedulers and pipeline (utilities.py:267-367 LMSDiscreteScheduler, :649-1008 DPMScheduler,
inpaint_pipeline.py:52-153).

TEST INFRASTRUCTURE, like oracle/capture_reference.py, whose `install_stubs` and whose fake
engines (oracle/fakes.py) it reuses.  Runs only where the reference tree exists; nothing from the
reference is copied -- the outputs are data (inputs + expected outputs).

    python tools/capture_scheduler_golden.py     # rewrites tests/golden/sched_*.npz

Written:
  sched_dpm.npz, sched_lmsd.npz   per N: timesteps, coefficient lists, latent scales, init sigma and a
                                  step() chain over fixed random model outputs
  sched_orch_*.npz                InpaintPipeline(scheduler=...).infer() with the fake engines at R = 32
(deliberately not named orchestration_*.npz: tests/test_oracle_golden.py runs those through DDIM).
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import capture_reference as cr  # noqa: E402

NS = (2, 4, 6, 8, 10, 12, 16, 20, 25, 50)
ORCH = [("DPM", 6, 2.0, 1.0, 6, 11), ("DPM", 16, 2.0, 1.0, 5, 12), ("LMSD", 6, 2.0, 1.0, 3, 13), ("LMSD", 12, 3.0, 0.0, 0, 14)]


def _chain(s, n, seed):
    """x_{i+1} = step(e_i, x_i, i, t_i) over fixed random e_i, from a fresh set_timesteps (no history)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 4, 3, 3, generator=g) * float(s.init_noise_sigma)
    e = torch.randn(n, 2, 4, 3, 3, generator=g)
    x0, out = x.clone(), []
    for i in range(n):
        x = s.step(e[i], x, i, s.timesteps[i])
        out.append(x.clone())
    return x0.numpy(), e.numpy(), torch.stack(out).numpy()


def capture_dpm():
    import utilities
    out = {}
    for n in NS:
        s = utilities.DPMScheduler(device="cpu", num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                   prediction_type="epsilon")
        s.set_timesteps(n)
        s.configure()  # on a fresh instance: the lists hold exactly this schedule's n entries
        ts = s.timesteps.numpy().astype(np.int64)
        out[f"timesteps_{n}"] = ts
        f32 = lambda lst: np.array([float(v) for v in lst], dtype=np.float32)  # noqa: E731
        out[f"first_coef_{n}"] = f32(s.first_order_first_coef)
        out[f"second_coef_{n}"] = f32(s.first_order_second_coef)
        out[f"mid_coef_{n}"] = f32(s.second_order_third_coef)
        out[f"alpha_s_{n}"] = s.alpha_t[ts].numpy()
        out[f"sigma_s_{n}"] = s.sigma_t[ts].numpy()
        # 1 / r0 of the second-order update at every evaluation >= 1 (utilities.py:907-912), from the reference's lambda table
        lam = s.lambda_t
        inv_r0 = [0.0]
        for i in range(1, n):
            t = 0 if i == n - 1 else int(ts[i + 1])
            h, h0 = lam[t] - lam[int(ts[i])], lam[int(ts[i])] - lam[int(ts[i - 1])]
            inv_r0.append(float(1.0 / (h0 / h)))
        out[f"inv_r0_{n}"] = np.array(inv_r0, dtype=np.float32)
        out[f"init_sigma_{n}"] = np.float32(s.init_noise_sigma)
        out[f"x_{n}"], out[f"e_{n}"], out[f"chain_{n}"] = _chain(s, n, 100 + n)
    return out


def capture_lmsd():
    import utilities
    out = {}
    for n in NS:
        s = utilities.LMSDiscreteScheduler(device="cpu", num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                           prediction_type="epsilon")
        s.set_timesteps(n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            s.configure()
        out[f"timesteps_{n}"] = s.timesteps.numpy().astype(np.float32)
        out[f"sigmas_{n}"] = s.sigmas.numpy().astype(np.float32)
        out[f"latent_scales_{n}"] = np.array([float(v) for v in s.latent_scales], dtype=np.float32)
        coefs = np.zeros((n, 4), dtype=np.float64)
        orders = np.zeros(n, dtype=np.int64)
        for i, row in enumerate(s.lms_coeffs):
            orders[i] = len(row)
            coefs[i, :len(row)] = [float(v) for v in row]
        out[f"coefs_{n}"], out[f"orders_{n}"] = coefs, orders
        out[f"init_sigma_{n}"] = np.float32(s.init_noise_sigma)
        out[f"x_{n}"], out[f"e_{n}"], out[f"chain_{n}"] = _chain(s, n, 200 + n)
    return out


def capture_orch(sched, steps, cfg, tg, tg_steps, seed, R=32):
    import inpaint_pipeline
    import stable_diffusion_pipeline as sdp
    from oracle import fakes

    sdp.device_view = lambda t: t
    torch.cuda.synchronize = lambda *a, **k: None
    # constructed with denoising_steps = N: DPMScheduler.configure() appends to its lists and step() indexes them from 0, so a
    # later step-count change would keep the constructor's coefficients (the behaviour the port fixes)
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
    cond = torch.randn(1, 14, 768, generator=g)
    uncond = torch.randn(1, 14, 768, generator=g)
    masked = torch.rand(1, 3, R, R, generator=g) * 2 - 1
    mask = (torch.rand(1, 1, R, R, generator=g) > 0.5).float()
    ctx_img = torch.rand(1, 3, R, R, generator=g) * 2 - 1
    ctx_mask = torch.rand(1, 1, R, R, generator=g)
    lat = torch.randn((1, 4, h, h), generator=torch.Generator().manual_seed(42), dtype=torch.float32)
    # update_infer_settings reads scheduler.beta_start / beta_end (inpaint_pipeline.py:45), which DPMScheduler does not store
    pipe.scheduler.beta_start, pipe.scheduler.beta_end = 0.00085, 0.012
    pipe.update_infer_settings(denoising_steps=steps, guidance_scale=cfg, texture_guidance_scale=tg,
                               texture_guidance_steps=tg_steps)
    trace = []
    orig_step = pipe.scheduler.step

    def step(*a, **k):
        r = orig_step(*a, **k)
        trace.append(r.clone())
        return r

    pipe.scheduler.step = step
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = pipe.infer(prompt=cond, negative_prompt=uncond, input_image=masked, mask_image=mask,
                         context_masked_image=ctx_img, context_mask=ctx_mask, image_height=R, image_width=R)
    return dict(
        cond=cond.numpy(), uncond=uncond.numpy(), masked=masked.numpy(), mask=mask.numpy(), ctx_img=ctx_img.numpy(),
        ctx_mask=ctx_mask.numpy(), latents=lat.numpy(), out=out.numpy(), trace=torch.stack(trace).numpy(),
        n_unet=np.int64(calls.count("unet")), scheduler=sched,
        settings=np.array([R, steps, cfg, tg, tg_steps], dtype=np.float64),
    )


def main():
    cr.install_stubs()
    np.savez_compressed(os.path.join(cr.GOLD, "sched_dpm.npz"), **capture_dpm())
    np.savez_compressed(os.path.join(cr.GOLD, "sched_lmsd.npz"), **capture_lmsd())
    for c in ORCH:
        d = capture_orch(*c)
        name = f"sched_orch_{c[0].lower()}_{c[1]}.npz"
        np.savez_compressed(os.path.join(cr.GOLD, name), **d)
        print(name, c, "unet calls", int(d["n_unet"]))


if __name__ == "__main__":
    main()
