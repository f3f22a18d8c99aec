#!/usr/bin/env python3
"""Eight stamps with Kit-like slider spreads at 512^2 / 20 steps, three ways (one context, max_batch 8):
  (a) what the server does without mixed settings: eight B = 1 calls, each with its stamp's own settings;
  (b) one mixed B = 8 call, every tg_steps = 20 (the same tg_evals: the 3B program throughout);
  (c) one mixed B = 8 call with spread tg_steps 0, 3, 5, 8, 12, 15, 20, 20 (finished stamps leave the UNet batch).
plus, for scale, the uniform B = 8 call with the default settings.  Warm rates in stamps/s; the first call of every variant (program
builds, GEMM tuning of new row counts, graph captures) is reported separately, and so is the first call of a NEW profile whose
programs all exist already (capture only).  Device memory after each step.

    python tools/mixed_batch_ab.py [--reps 5] [--out FILE]   (the report goes to stdout, and also to FILE when given)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CFG = [1.5, 2.0, 2.5, 3.0, 3.5, 4.5, 5.0, 6.0]
TG = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
PAD = [150, 150, 120, 150, 100, 150, 150, 80]
SPREAD = [0, 3, 5, 8, 12, 15, 20, 20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    from diffusiontexturepainting_amd import synthetic
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def used_mib():
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2**20

    R, B = a.res, 8
    base_mem = used_mib()
    m = MI355ConditionalInpainter(R, device=0, max_batch=B)
    canvas, brush, lat, eps = synthetic.make_stamp_batch(B, R, 7)
    for s in range(B):
        cond, uncond = synthetic.make_conditioning(100 + s)
        m.set_conditioning(cond, uncond, brush[s:s + 1] if brush.shape[0] == B else brush, slot=s)
    canvas, lat, eps = canvas.cuda(), lat.cuda(), eps.cuda()
    slots = list(range(B))
    say(f"mixed-settings stamp batches, {R}^2 / {a.steps} steps, {B} stamps, {a.reps} warm reps each; context {used_mib() - base_mem:.0f} MiB "
        f"after load")

    def per(tg_steps):
        return [dict(cfg_weight=CFG[b], tg_weight=TG[b], tg_steps=tg_steps[b], context_pad=PAD[b]) for b in range(B)]

    def call(kind, settings):
        if kind == "solo":  # (a): one B = 1 call per stamp
            for b in range(B):
                m.generate_raw(canvas[b:b + 1], latents=lat[b:b + 1], vae_eps=eps[:, b:b + 1], slots=[b], steps=a.steps, **settings[b])
        elif kind == "uniform":
            m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=slots, steps=a.steps)
        else:
            m.generate_raw(canvas, latents=lat, vae_eps=eps, slots=slots, per_stamp=settings, steps=a.steps)

    def measure(name, kind, settings):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(kind, settings)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        call(kind, settings)  # second call: everything built and captured
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            call(kind, settings)
        torch.cuda.synchronize()
        warm = (time.perf_counter() - t0) / a.reps
        rows = m.stamp_unet_rows() if kind != "solo" else None
        say(f"{name:58s} {B / warm:6.2f} stamps/s  {warm * 1e3:8.1f} ms per 8 stamps  first call {first * 1e3:8.1f} ms "
            f"(host {host * 1e3:7.1f} ms)" + (f"  unet rows {rows}" if rows is not None else "") + f"  device {used_mib() - base_mem:.0f} MiB")
        return warm

    t_uni = measure("uniform B=8 (default settings)", "uniform", None)
    t_a = measure("(a) 8 x B=1, spread tg_steps", "solo", per(SPREAD))
    t_a20 = measure("(a') 8 x B=1, tg_steps 20", "solo", per([20] * B))
    t_b = measure("(b) mixed B=8, tg_steps 20", "mixed", per([20] * B))
    t_c = measure("(c) mixed B=8, tg_steps " + ",".join(map(str, SPREAD)), "mixed", per(SPREAD))
    # a new profile whose UNet programs all exist (the same set of tg row counts as (c)): its first call costs the capture only
    t_c2 = measure("(c2) new profile, programs built: tg_steps 0,3,5,8,12,16,20,20", "mixed", per([0, 3, 5, 8, 12, 16, 20, 20]))
    E = a.steps - 1
    evals = sorted((min(E, t) for t in SPREAD), reverse=True)
    rows_c = sum(2 * B + sum(1 for t in evals if t > i) for i in range(E))
    say(f"ratios: (b)/(a') {t_a20 / t_b:.2f}x, (c)/(a) {t_a / t_c:.2f}x, (b) vs uniform {t_uni / t_b:.3f}; "
        f"(c) rows {rows_c} of {3 * B * E} (3B) / {2 * B * E} (2B): rows predict {rows_c / (3 * B * E):.3f} of (b), measured {t_c / t_b:.3f}; "
        f"(c2) {t_c2 / t_c:.3f} of (c)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
