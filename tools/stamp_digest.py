"""sha256 of one stamp's output through every kind of stamp call, for a byte-for-byte A/B of two builds of the library:

    python tools/stamp_digest.py [--res 64 256]  >  new.txt
    DTP_LIB=tools/ab/libdtp_head.so python tools/stamp_digest.py [--res 64 256]  >  ref.txt       (separate processes; then diff)

The calls are those of tests/test_gpu_mixed_settings.py::test_call_kinds_on_one_handle_do_not_share_captured_stages (B = 2, 4 steps,
synthetic weights, one handle per resolution, graphs on): plain, per_stamp, strength 0.5 with and without its draws, seeded, seeded at
strength 0.5, the plain stamp under DPM and under DDIM again.  `--flagship N`: also the 512^2 / 20-step B = 1 stamp, its digest, graph
nodes, stage times and the host time of N warm un-synchronised calls (the enqueue cost of a stamp)."""
import argparse
import hashlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diffusiontexturepainting_amd import synthetic, weights as W  # noqa: E402
from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter  # noqa: E402


def sha(t):
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def handle(res, max_batch):
    return MI355ConditionalInpainter(res, device=0, max_batch=max_batch,
                                     weights=dict(unet=W.synthetic_unet(5), lora=W.synthetic_lora(5), vae=W.synthetic_vae(5)))


def matrix(res):
    m = handle(res, 2)
    canvas, lat, eps = [], [], []
    for slot in range(2):
        c, brush, la, ep = synthetic.make_stamp_batch(1, res, 2000 + slot)
        m.set_conditioning(*synthetic.make_conditioning(2001 + slot), brush, slot=slot)
        canvas.append(c), lat.append(la), eps.append(ep)
    canvas, lat, eps = torch.cat(canvas), torch.cat(lat), torch.cat(eps, dim=1)
    init_eps = torch.randn(2, 4, res // 8, res // 8, generator=torch.Generator().manual_seed(11))
    kw = dict(latents=lat, vae_eps=eps, slots=[0, 1], steps=4)
    seeded = dict(slots=[0, 1], steps=4, seeds=7)
    calls = [("plain", lambda: m.generate_raw(canvas, **kw)),
             ("per_stamp tg_steps 1, 3", lambda: m.generate_raw(canvas, per_stamp=[dict(tg_steps=1), dict(tg_steps=3)], **kw)),
             ("strength 0.5 + init_eps", lambda: m.generate_raw(canvas, strength=0.5, init_eps=init_eps, **kw)),
             ("strength 0.5, means", lambda: m.generate_raw(canvas, strength=0.5, init_eps=False, **dict(kw, vae_eps=False))),
             ("seeds 7", lambda: m.generate_raw(canvas, **seeded)),
             ("seeds 7, strength 0.5", lambda: m.generate_raw(canvas, strength=0.5, **seeded))]
    calls += [("plain, DPM", calls[0][1]), ("plain, DDIM again", calls[0][1])]
    for p in range(2):
        for i, (name, fn) in enumerate(calls):
            if i >= 6:
                m.set_scheduler("DPM" if i == 6 else "DDIM")
            out = fn()
            print(f"res {res} pass {p} {name:26s} sha256 {sha(out)}  graph_nodes {m.stamp_info()['graph_nodes']}", flush=True)


def flagship(n):
    m = handle(512, 1)
    canvas, brush, lat, eps = synthetic.make_stamp_batch(1, 512, 1000)
    m.set_conditioning(*synthetic.make_conditioning(7), brush)
    canvas, lat, eps = canvas.cuda(), lat.cuda(), eps.cuda()
    for _ in range(3):  # capture + warm
        out = m.generate_raw(canvas, latents=lat, vae_eps=eps)
    torch.cuda.synchronize()
    host = []
    for _ in range(n):
        t0 = time.perf_counter()
        m.generate_raw(canvas, latents=lat, vae_eps=eps)
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    print(f"flagship 512^2 B=1 20 steps: sha256 {sha(out)}  graph_nodes {m.stamp_info()['graph_nodes']}  "
          f"stage_times_ms {' '.join('%.2f' % v for v in m.stage_times_ms())}")
    print(f"flagship host ms per un-synchronised warm call, {n} calls: median {statistics.median(host):.3f}  min {min(host):.3f}  "
          f"max {max(host):.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--flagship", type=int, default=0, metavar="N")
    a = ap.parse_args()
    print(f"# library: {os.environ.get('DTP_LIB') or 'working build'}")
    for r in a.res:
        matrix(r)
    if a.flagship:
        flagship(a.flagship)
