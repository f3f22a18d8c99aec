"""fp32 CPU restatement of the DPM-Solver++ and LMS samplers of the stamp loop (not a test module: a helper the scheduler tests
import).  Each piece cites the reference lines it follows; paths are relative to the reference's trt_inference/.  Restated from the
formulas -- pinned on the CPU by tests/test_schedulers_cpu.py against fixtures captured from the reference's own DPMScheduler,
LMSDiscreteScheduler and InpaintPipeline (tools/capture_scheduler_golden.py), and used as the oracle of the GPU scheduler tests.

The orchestration around the sampler (masks, VAE scaling, guidance combine, branch order) is oracle.pipeline's; `infer` differs from
oracle.pipeline.infer only where the sampler enters: init_noise_sigma, scale_model_input, the evaluated timesteps and step().
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import pipeline as P


def _alphas_cumprod():
    """utilities.py:283-285 / :684-688: scaled-linear betas 0.00085..0.012 over 1000 training steps, fp32."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class DPM:
    """DPMScheduler (utilities.py:649-1008) as the pipeline constructs it: DPM-Solver++, solver_order 2, midpoint, epsilon
    prediction, no thresholding, lower_order_final, steps_offset 0.  The coefficients are those of the CURRENT step count (the
    reference appends to its lists on every configure() and indexes from 0 -- not reproduced)."""

    def __init__(self, n):
        ac = _alphas_cumprod()
        self.alpha = torch.sqrt(ac)  # :692-694
        self.sigma = torch.sqrt(1 - ac)
        self.lam = torch.log(self.alpha) - torch.log(self.sigma)
        self.n = int(n)
        # set_timesteps (:797-805): numpy rounds half to even
        self.timesteps = torch.from_numpy(np.linspace(0, 999, self.n + 1).round()[::-1][:-1].copy().astype(np.int64))
        self.init_noise_sigma = 1.0  # :699
        self.prev_x0 = None

    def eval_timesteps(self):
        """steps_offset 0 and strength 1: t_start = 0, all n timesteps are evaluated (stable_diffusion_pipeline.py:348-355)."""
        return self.timesteps, 0

    def scale(self, i):
        return 1.0  # scale_model_input (:746-747)

    def step(self, e, x, i):
        n = self.n
        s0 = int(self.timesteps[i])
        t = 0 if i == n - 1 else int(self.timesteps[i + 1])  # :970
        x0 = (x - self.sigma[s0] * e) / self.alpha[s0]  # convert_model_output (:817-822)
        h = self.lam[t] - self.lam[s0]
        c1 = self.sigma[t] / self.sigma[s0]  # :758-760 (== :775-777)
        c2 = self.alpha[t] * (torch.exp(-h) - 1.0)
        first = i == 0 or (i == n - 1 and n < 15)  # lower_order_nums < 1 or lower_order_final (:971-987)
        if first:
            out = c1 * x - c2 * x0  # :838-852
        else:
            s1 = int(self.timesteps[i - 1])
            r0 = (self.lam[s0] - self.lam[s1]) / h  # :907-912
            d1 = (1.0 / r0) * (x0 - self.prev_x0)
            out = c1 * x - c2 * x0 - (0.5 * c2) * d1  # midpoint (:917-923)
        self.prev_x0 = x0
        return out


def _lagrange_integral(s, j, a, b):
    """Exact integral over [a, b] of the Lagrange basis polynomial of node s[j] on the nodes s (lms_derivative, utilities.py:330-339)."""
    poly = np.polynomial.Polynomial([1.0])
    for m, sm in enumerate(s):
        if m != j:
            poly = poly * np.polynomial.Polynomial([-sm, 1.0]) / (s[j] - sm)
    prim = poly.integ()
    return float(prim(b) - prim(a))


class LMSD:
    """LMSDiscreteScheduler (utilities.py:267-367), epsilon prediction, steps_offset 0."""

    def __init__(self, n):
        ac = _alphas_cumprod()
        full = ((1 - ac) / ac) ** 0.5  # :286
        self.init_noise_sigma = full.max()  # :292 (sigma_max = 14.6146)
        self.n = int(n)
        ts = np.linspace(0, 999, self.n, dtype=float)[::-1].copy()  # set_timesteps (:299)
        sig = np.interp(ts, np.arange(0, 1000), full.numpy())  # :301
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts).float()
        self.latent_scales = [1.0 / ((s ** 2 + 1) ** 0.5) for s in self.sigmas]  # configure (:318)
        # configure() (:341-343) rebinds its `order` to min(step_index + 1, order) each pass: 1 from the first evaluation on
        self.coeffs, order = [], 4
        sg = self.sigmas.double().numpy()
        for i in range(self.n):
            order = min(i + 1, order)
            nodes = [sg[i - m] for m in range(order)]
            self.coeffs.append([_lagrange_integral(nodes, j, sg[i], sg[i + 1]) for j in range(order)])
        self.derivatives = []

    def eval_timesteps(self):
        return self.timesteps, 0

    def scale(self, i):
        return self.latent_scales[i]

    def step(self, e, x, i):
        sigma = self.sigmas[i]  # :347-349
        x0 = x - sigma * e
        d = (x - x0) / sigma  # :358
        self.derivatives.append(d)
        if len(self.derivatives) > 4:
            self.derivatives.pop(0)
        # :362-364; the coefficients are fp32 like a python float times an fp32 tensor
        return x + sum(np.float32(c) * dd for c, dd in zip(self.coeffs[i], reversed(self.derivatives)))


SCHEDULERS = {"DPM": DPM, "LMSD": LMSD}


def infer(unet_fn, vae_enc_fn, vae_dec_fn, cond, uncond, masked_image, mask, ctx_masked_image, ctx_mask, latents, scheduler="DPM",
          steps=20, cfg=2.0, tg=1.0, tg_steps=20, trace=None):
    """oracle.pipeline.infer with the sampler `scheduler` ("DPM" | "LMSD"); same arguments and batch order."""
    b = latents.shape[0]
    h, w = latents.shape[-2:]
    sched = SCHEDULERS[scheduler](steps)  # a fresh set_timesteps per infer: no history carries over (sdp:349)
    m = F.interpolate(mask, size=(h, w))
    cm = F.interpolate(ctx_mask, size=(h, w))
    mask3 = torch.cat([m, m, cm])
    timesteps, t_start = sched.eval_timesteps()
    ml = P.VAE_SCALE * vae_enc_fn(masked_image.contiguous(), 0)
    cml = P.VAE_SCALE * vae_enc_fn(ctx_masked_image.contiguous(), 1)
    ml3 = torch.cat([ml, ml, cml])
    ctx = torch.cat([uncond.expand(b, -1, -1), cond.expand(b, -1, -1), cond.expand(b, -1, -1)])
    ctx = ctx.to(torch.float16).float()
    x = latents * sched.init_noise_sigma  # initialize_latents (sdp:345)
    tg_scale = tg
    for i, t in enumerate(timesteps):
        if i > tg_steps - 1:  # sdp:419-420
            tg_scale = 0.0
        x3 = torch.cat([x] * 3) * sched.scale(t_start + i)  # scale_model_input before the concat (sdp:423-427)
        sample = torch.cat([x3, mask3, ml3], dim=1)
        pred = unet_fn(sample, t.float(), ctx)
        u, c, g = pred.chunk(3)
        eps = u + cfg * (c - u) + tg_scale * (g - c)  # sdp:449-451
        x = sched.step(eps, x, t_start + i)
        if trace is not None:
            trace.append(x.clone())
    x = x / P.VAE_SCALE
    images = vae_dec_fn(x)
    return (images / 2 + 0.5).clamp(0, 1)


def generate_raw(nets, brush_image, cond, uncond, canvas, latents, vae_eps, scheduler="DPM", steps=20, context_pad=150, tg_steps=20,
                 cfg_weight=2.0, tg_weight=1.0, trace=None):
    """oracle.pipeline.generate_raw with the sampler `scheduler`, on the oracle networks (oracle.nets)."""
    from oracle import nets as N
    masked, masks, ctx_img, ctx_mask = P.prepare_stamp(canvas, brush_image, int(context_pad))
    return infer(
        lambda s, t, c: N.unet_forward(nets["unet"], s, t, c),
        lambda img, k: N.vae_encode(nets["vae"], img, vae_eps[k]),
        lambda z: N.vae_decode(nets["vae"], z),
        cond, uncond, masked, masks, ctx_img, ctx_mask, latents, scheduler=scheduler,
        steps=int(steps), cfg=float(cfg_weight), tg=float(tg_weight), tg_steps=int(tg_steps), trace=trace)
