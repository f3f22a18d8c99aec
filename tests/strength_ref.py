"""fp32 CPU restatement of a strength < 1 stamp (not a test module: a helper the strength tests import).  Each piece cites the reference
lines it follows; paths are relative to the reference's trt_inference/.  Pinned on the CPU by tests/test_strength_cpu.py against fixtures
captured from the reference's own initialize_timesteps, add_noise, step() and InpaintPipeline.infer (tools/capture_strength_golden.py),
and used as the oracle of tests/test_gpu_strength.py.

The samplers are those of oracle.pipeline (DDIM) and tests/sched_ref.py (DPM, LMSD) with what strength adds: steps_offset, the
shortened timestep list, add_noise at t_start, and DPM's first-order first evaluation from a fresh history.  The orchestration
differs from sched_ref.infer only at the start point: x = add_noise(z0, latents) with z0 the init image's latents.
"""
import torch
import torch.nn.functional as F

import sched_ref
from oracle import pipeline as P


def initialize_timesteps(steps, strength, offset):
    """stable_diffusion_pipeline.py:348-355 (Python: steps * strength in double).  Returns (t_start, evals)."""
    init = min(int(steps * strength) + offset, steps)
    t_start = max(steps - init + offset, 0)
    return t_start, steps - t_start


class DDIM(P.DDIM):
    steps_offset = 1  # utilities.py:379

    def add_noise(self, z0, noise, idx):
        """utilities.py:524-529 on the gathered table (configure(), :416)."""
        a = self.alphas[idx]
        return a ** 0.5 * z0 + (1 - a) ** 0.5 * noise

    def scale(self, i):
        return 1.0


class DPM(sched_ref.DPM):
    steps_offset = 0  # utilities.py:664

    def add_noise(self, z0, noise, idx):
        """utilities.py:1000-1008: the full alphas_cumprod table at timesteps[idx]."""
        ac = sched_ref._alphas_cumprod()[int(self.timesteps[idx])]
        return ac ** 0.5 * z0 + (1 - ac) ** 0.5 * noise

    def step(self, e, x, i):
        """sched_ref.DPM.step with lower_order_nums counted from this infer's first evaluation (set_timesteps resets it, :805;
        :979 first order while it is 0), not from index 0 of the table."""
        n = self.n
        s0 = int(self.timesteps[i])
        t = 0 if i == n - 1 else int(self.timesteps[i + 1])
        x0 = (x - self.sigma[s0] * e) / self.alpha[s0]
        h = self.lam[t] - self.lam[s0]
        c1 = self.sigma[t] / self.sigma[s0]
        c2 = self.alpha[t] * (torch.exp(-h) - 1.0)
        first = self.prev_x0 is None or (i == n - 1 and n < 15)  # lower_order_final refers to the full list (:971-973)
        if first:
            out = c1 * x - c2 * x0
        else:
            s1 = int(self.timesteps[i - 1])  # the timestep evaluated before (:982)
            r0 = (self.lam[s0] - self.lam[s1]) / h
            d1 = (1.0 / r0) * (x0 - self.prev_x0)
            out = c1 * x - c2 * x0 - (0.5 * c2) * d1
        self.prev_x0 = x0
        return out


class LMSD(sched_ref.LMSD):
    steps_offset = 0  # utilities.py:274

    def add_noise(self, z0, noise, idx):
        """utilities.py:363-366."""
        return z0 + noise * self.sigmas[idx]


SCHEDULERS = {"DDIM": DDIM, "DPM": DPM, "LMSD": LMSD}


def make(name, steps):
    return SCHEDULERS[name](steps)


def infer(unet_fn, vae_enc_fn, vae_dec_fn, cond, uncond, masked_image, mask, ctx_masked_image, ctx_mask, latents, init_image,
          scheduler="DDIM", steps=20, strength=0.5, cfg=2.0, tg=1.0, tg_steps=20, trace=None, start=None):
    """sched_ref.infer (oracle.pipeline.infer for DDIM) with `strength`: the loop runs timesteps[t_start:] with step_offset t_start
    (inpaint_pipeline.py:119,144) from x = add_noise(z0, latents, t_start), z0 = 0.18215 * VAE_enc(init_image) (vae_enc_fn call index
    2).  At strength 1 the start is latents * init_noise_sigma, as in sched_ref.infer."""
    b = latents.shape[0]
    h, w = latents.shape[-2:]
    sched = make(scheduler, steps)  # a fresh set_timesteps per infer: no history carries over (sdp:349)
    m = F.interpolate(mask, size=(h, w))
    cm = F.interpolate(ctx_mask, size=(h, w))
    mask3 = torch.cat([m, m, cm])
    t_start, evals = initialize_timesteps(int(steps), float(strength), sched.steps_offset)
    timesteps = sched.timesteps[t_start:]
    ml = P.VAE_SCALE * vae_enc_fn(masked_image.contiguous(), 0)
    cml = P.VAE_SCALE * vae_enc_fn(ctx_masked_image.contiguous(), 1)
    ml3 = torch.cat([ml, ml, cml])
    ctx = torch.cat([uncond.expand(b, -1, -1), cond.expand(b, -1, -1), cond.expand(b, -1, -1)])
    ctx = ctx.to(torch.float16).float()
    if strength < 1.0:
        z0 = P.VAE_SCALE * vae_enc_fn(init_image.contiguous(), 2)
        x = sched.add_noise(z0, latents, t_start)
    else:
        x = latents * float(getattr(sched, "init_noise_sigma", 1.0))
    if start is not None:
        start.update(t_start=t_start, evals=evals, x_init=x.clone())
    tg_scale = tg
    for i, t in enumerate(timesteps):
        if i > tg_steps - 1:  # sdp:419-420: counted from t_start
            tg_scale = 0.0
        x3 = torch.cat([x] * 3) * sched.scale(t_start + i)
        sample = torch.cat([x3, mask3, ml3], dim=1)
        pred = unet_fn(sample, t.float(), ctx)
        u, c, g = pred.chunk(3)
        eps = u + cfg * (c - u) + tg_scale * (g - c)
        x = sched.step(eps, x, t_start + i)
        if trace is not None:
            trace.append(x.clone())
    x = x / P.VAE_SCALE
    images = vae_dec_fn(x)
    return (images / 2 + 0.5).clamp(0, 1)


def generate_raw(nets, brush_image, cond, uncond, canvas, latents, vae_eps, init_eps, scheduler="DDIM", steps=20, strength=0.5,
                 context_pad=150, tg_steps=20, cfg_weight=2.0, tg_weight=1.0, trace=None):
    """sched_ref.generate_raw with `strength`: the init image is the FULL canvas RGB * 2 - 1 (not the alpha-masked image), encoded with
    its own draw init_eps [B,4,h,w] (None = the distribution mean)."""
    from oracle import nets as N
    masked, masks, ctx_img, ctx_mask = P.prepare_stamp(canvas, brush_image, int(context_pad))
    draws = [vae_eps[0], vae_eps[1], torch.zeros_like(latents) if init_eps is None else init_eps]
    return infer(
        lambda s, t, c: N.unet_forward(nets["unet"], s, t, c),
        lambda img, k: N.vae_encode(nets["vae"], img, draws[k]),
        lambda z: N.vae_decode(nets["vae"], z),
        cond, uncond, masked, masks, ctx_img, ctx_mask, latents, canvas[:, :3] * 2 - 1, scheduler=scheduler,
        steps=int(steps), strength=float(strength), cfg=float(cfg_weight), tg=float(tg_weight), tg_steps=int(tg_steps), trace=trace)
