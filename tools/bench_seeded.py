#!/usr/bin/env python3
"""Seeded against caller-tensor stamps, same process: ms per stamp of bench.py's flagship call (composite, u8 out, Kit default
settings) with the noise handed over as device tensors ("tensors") and drawn by the library from per-stamp seeds ("seeded"), the two
arms alternating, `--repeats` timed groups of `--stamps` back-to-back stamps each.  Under DTP_LIB=<an older libdtp.so> only the
"tensors" arm runs (the older build lacks dtp_stamp_seeded): that is the parent's figure and its run-to-run spread, to be taken in
the same session as the new build's.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--stamps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from diffusiontexturepainting_amd import _lib, synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    dev = torch.device("cuda", 0)
    sd = dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae())
    st = dict(steps=a.ddim_steps, context_pad=150, tg_steps=a.ddim_steps, cfg_weight=2.0, tg_weight=1.0)
    canvas, brush, lat, eps = synthetic.make_stamp_batch(a.batch, a.res, seed=1000)
    cond, uncond = synthetic.make_conditioning(7)
    m = MI355ConditionalInpainter(a.res, device=0, weights=sd, max_batch=max(a.batch, 8))
    m.set_conditioning(cond, uncond, brush)
    canvas, lat, eps = canvas.to(dev), lat.to(dev), eps.to(dev)
    arms = {"tensors": dict(latents=lat, vae_eps=eps)}
    if hasattr(_lib.load(), "dtp_stamp_seeded"):
        arms["seeded"] = dict(seeds=list(range(500, 500 + a.batch)))
    for kw in arms.values():  # build, capture, warm
        for _ in range(2):
            m._stamp(canvas, st, composite=True, output_u8=True, **kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, kw in arms.items():
            t0 = time.perf_counter()
            for _ in range(a.stamps):
                m._stamp(canvas, st, composite=True, output_u8=True, **kw)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.stamps)
    out = dict(lib=os.path.basename(_lib.LIB_PATH), batch=a.batch, res=a.res, ddim_steps=a.ddim_steps, stamps=a.stamps)
    for name, v in ms.items():
        out[name] = dict(ms_per_stamp=[round(x, 3) for x in v], median=round(statistics.median(v), 3), spread=round(max(v) - min(v), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
