#!/usr/bin/env python3
"""ms per stamp at a resolution that is a multiple of 8 but not of 64 against its multiple-of-64 neighbour.

Each resolution gets its own context (synthetic weights, 20 DDIM steps, Kit default settings).  The first call of a context at a new
resolution builds -- and, with the autotuner on, tunes -- its programs: that cost is printed as first_call_s.  Then the resolutions
alternate, round by round, and the median ms per stamp call of each is printed.

    python tools/resolution_ab.py --pairs 360:384 600:640 --batch 1 8 --rounds 5 --reps 3
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", nargs="+", default=["360:384", "600:640"], help="ragged:aligned resolution pairs")
    ap.add_argument("--batch", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds after the warm-up")
    ap.add_argument("--reps", type=int, default=3, help="stamp calls per resolution and round")
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--autotune", type=int, default=1)
    ap.add_argument("--profile", action="store_true", help="also print the dtp_profile per-kind table of one stamp call per resolution")
    a = ap.parse_args()

    import torch
    from diffusiontexturepainting_amd import synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter

    sd = dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae(), clip=W.synthetic_clip(), penc=W.synthetic_patch_encoder())
    st = dict(steps=a.ddim_steps)  # everything else: the Kit defaults of the inpainter
    print(f"# resolution A/B: {a.ddim_steps} DDIM steps, autotune={a.autotune}, {a.rounds} alternating rounds x {a.reps} calls; "
          f"device {torch.cuda.get_device_name(0)}", flush=True)
    for pair in a.pairs:
        rs = [int(x) for x in pair.split(":")]
        for b in a.batch:
            models, inputs = {}, {}
            for r in rs:
                m = MI355ConditionalInpainter(r, device=0, weights=sd, max_batch=b)
                m.set_option("autotune", a.autotune)
                canvas, brush, lat, eps = synthetic.make_stamp_batch(b, r, seed=11)
                cond, uncond = synthetic.make_conditioning(12)
                m.set_conditioning(cond, uncond, brush)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.generate(canvas, **st)
                torch.cuda.synchronize()
                print(f"R={r} B={b}: first_call_s={time.perf_counter() - t0:.1f}", flush=True)
                models[r], inputs[r] = m, canvas
            times = {r: [] for r in rs}
            for _ in range(a.rounds):
                for r in rs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        models[r].generate(inputs[r], **st)
                    torch.cuda.synchronize()
                    times[r].append((time.perf_counter() - t0) * 1e3 / a.reps)
            med = {r: statistics.median(times[r]) for r in rs}
            line = "  ".join(f"R={r}: {med[r]:.2f} ms/call (rounds {' '.join(f'{t:.1f}' for t in times[r])})" for r in rs)
            print(f"B={b}: {line}  ratio {rs[0]}/{rs[1]} = {med[rs[0]] / med[rs[1]]:.3f}", flush=True)
            if a.profile:  # per kernel kind: launches and device ms of one (eager, event-bracketed) stamp call
                prof = {}
                for r in rs:
                    models[r].profile(1)
                    models[r].generate(inputs[r], **st)
                    torch.cuda.synchronize()
                    prof[r] = {x["kernel"]: (x["launches"], x["ms"]) for x in models[r].profile_rows() if x["launches"]}
                    models[r].profile(0)
                kinds = sorted(set(prof[rs[0]]) | set(prof[rs[1]]), key=lambda k: -max(prof[r].get(k, (0, 0.0))[1] for r in rs))
                print(f"  {'kernel kind':<70} " + "  ".join(f"R={r} launches / ms" for r in rs))
                for k in kinds:
                    print(f"  {k:<70} " + "  ".join(f"{prof[r].get(k, (0, 0.0))[0]:>8} {prof[r].get(k, (0, 0.0))[1]:>9.2f}" for r in rs))
                print("  " + " " * 70 + " " + "  ".join(f"{'total':>8} {sum(v[1] for v in prof[r].values()):>9.2f}" for r in rs), flush=True)
            del models
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
