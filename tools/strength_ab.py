#!/usr/bin/env python3
"""Milliseconds per stamp at strength 1 / 0.75 / 0.5 / 0.3 (`generate(strength=...)`, dtp_stamp_strength) at 512^2, DDIM 20 steps,
batch 1 and batch 8, one context per batch size.  Every variant is warmed up first (program builds incl. the 3B-row VAE-encoder program,
GEMM tuning, graph captures); the timed rounds then run the variants in alternating order, one stamp each, so that a drift of the clock
or the thermals spreads over all of them.  Reports the median, the spread and the per-stage times of the last stamp: stage 0 holds the
one batched VAE encode (2B rows at strength 1, 3B rows below), stage 1 the shortened loop.

    python tools/strength_ab.py [--rounds 7] [--batches 1,8] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

VARIANTS = [1.0, 0.75, 0.5, 0.3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from diffusiontexturepainting_amd import synthetic
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    R, n = a.res, a.steps
    say(f"strength of the stamp, {R}^2, DDIM {n} steps, Kit defaults otherwise (cfg 2, tg 1, tg_steps = steps); {a.rounds} timed rounds, "
        f"alternating order; ms per stamp call (median [min..max]), stages of the last call")
    for B in [int(b) for b in a.batches.split(",")]:
        m = MI355ConditionalInpainter(R, device=0, max_batch=B)
        canvas, brush, lat, eps = synthetic.make_stamp_batch(B, R, 7)
        cond, uncond = synthetic.make_conditioning(8)
        m.set_conditioning(cond, uncond, brush[:1])
        canvas, lat, eps = canvas.cuda(), lat.cuda(), eps.cuda()
        ieps = torch.randn_like(lat)

        def run(s):
            m.generate(canvas, latents=lat, vae_eps=eps, init_eps=ieps, strength=s, steps=n, tg_steps=n)

        for s in VARIANTS:  # warm-up: builds, tuning, captures
            run(s)
            run(s)
        torch.cuda.synchronize()
        times = {v: [] for v in VARIANTS}
        stages, evals = {}, {}
        for r in range(a.rounds):
            order = VARIANTS if r % 2 == 0 else VARIANTS[::-1]
            for v in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(v)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e3)
                stages[v] = m.stage_times_ms()
                evals[v] = m.stamp_info()["unet_evals"]
        base = statistics.median(times[VARIANTS[0]])
        for v in VARIANTS:
            t = times[v]
            med = statistics.median(t)
            st = stages[v]
            say(f"B={B} strength {v:<4}: {evals[v]:>2} UNet evals  {med:8.2f} ms [{min(t):.2f}..{max(t):.2f}]  x{med / base:.3f} of strength 1"
                f"  | pre+enc {st[0]:.2f}  loop {st[1]:.2f} ({st[1] / evals[v]:.2f}/eval)  dec+post {st[2]:.2f}")
        del m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
