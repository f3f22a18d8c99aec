#!/usr/bin/env python3
"""What face sets cost, on the GPU, in one process:
1. the lasso: a 1024-vertex polygon over a 1280 x 720 frame of the height field refined to 100 352 faces (`select_faces`), between
   device events on the view's stream with the launches enqueued behind a blocker (a few milliseconds of queued matrix products, so
   that the interval holds the device's work and not the host's enqueue), warmed up, the median of --lasso-repeats calls; beside it a
   4-vertex rectangle of the same box, the frame's own render, and the tint of the selected faces;
2. a 16-stamp stroke at 512^2 / 20 steps on a 2048^2 texture (`paint_mesh_stroke`, the stroke of tools/mesh_stroke_timing.py) with
   face_mask= one UV chart against the same stroke without the keyword, alternating, warmed up, --repeats each: wall time from the call
   to the end of the device work; and the valid + backproject launches on their own between events behind the blocker, masked and
   unmasked, alternating.
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lasso-repeats", type=int, default=50)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--frame", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--no-stroke", action="store_true", help="skip the two whole strokes (for a kernel trace of the rest)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_timing.py measures on the GPU: no device found")
    from diffusiontexturepainting_amd import mesh as M, ops, synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from diffusiontexturepainting_amd.mesh import mesh_camera, view_camera
    dev = torch.device("cuda", 0)
    R, T = a.res, a.texture
    sd = dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae())
    st = dict(steps=a.ddim_steps, context_pad=150, tg_steps=a.ddim_steps, cfg_weight=2.0, tg_weight=1.0)
    _, brush, _, _ = synthetic.make_stamp_batch(1, R, seed=1000)
    cond, uncond = synthetic.make_conditioning(7)
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    m.set_conditioning(cond, uncond, brush)
    verts, faces, uvs = synthetic.make_height_field(a.grid, a.grid, seed=3)
    F = int(faces.shape[0])
    mesh = m.load_mesh(verts, faces, uvs)
    tex0 = torch.randint(0, 256, (T, T, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    out = dict(res=R, texture=T, faces=F, frame=list(a.frame), stamps=16, ddim_steps=a.ddim_steps, repeats=a.repeats, lasso_repeats=a.lasso_repeats)

    # ---- 1. the lasso
    H, Wf = a.frame
    cam = view_camera((0.3, -0.5, 2.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, (H, Wf), 0.05)
    frame, face_idx = m.render_view(mesh, tex0, cam, want_face_idx=True)
    circle = [((0.5 + 0.33 * math.cos(2 * math.pi * k / 1024)) * Wf, (0.5 + 0.45 * math.sin(2 * math.pi * k / 1024)) * H) for k in range(1024)]
    box = [(0.17 * Wf, 0.05 * H), (0.83 * Wf, 0.05 * H), (0.83 * Wf, 0.95 * H), (0.17 * Wf, 0.95 * H)]
    sel = M.faceset_empty(F, dev)
    vs = m.view_stream
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device=dev)
    cur = torch.cuda.current_stream(dev)

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(4):  # a few milliseconds of queued work: the call's launches are all enqueued before the first one starts
                blocker @ blocker
            vs.wait_stream(cur)
            ev[0].record(vs)
            fn()
            ev[1].record(vs)
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    lasso = {}
    for name, poly in (("polygon_1024", circle), ("rectangle_4", box)):
        lasso[name] = timed(lambda: m.select_faces(mesh, face_idx, poly, out=sel), a.lasso_repeats)
        lasso[name]["faces_selected"] = int(M.faceset_to_bool(sel, F).sum())
    m.select_faces(mesh, face_idx, circle, out=sel)
    lasso["tint"] = timed(lambda: m.tint_selection(frame, face_idx, sel, num_faces=F), a.lasso_repeats)
    lasso["render_view_of_the_frame"] = timed(lambda: m.render_view(mesh, tex0, cam, out=frame), 10)
    lasso["pixels_with_a_face"] = int((face_idx >= 0).sum())
    out["lasso"] = lasso

    # ---- 2. the masked stroke against the unmasked one (the stroke of tools/mesh_stroke_timing.py)
    positions = [(-0.6 + 0.4 * (i % 4), -0.45 + 0.3 * (i // 4), 0.1) for i in range(16)]
    normals = [(0.1 * ((i % 3) - 1), 0.1 * ((i % 2) - 0.5), 1.0) for i in range(16)]
    prevs = [(x, y + 0.1, z) for x, y, z in positions]
    fov = 0.25
    seeds = list(range(500, 516))
    squares = a.grid - 1
    chart = (torch.arange(F) % (2 * squares)) < 2 * (squares // 2)  # the faces left of the middle column: the first UV chart
    face_mask = M.faceset_from_bool(chart).to(dev)
    arms = {
        "unmasked": lambda tex: m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, fov, seeds=seeds, **st),
        "masked": lambda tex: m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, fov, seeds=seeds, face_mask=face_mask, **st),
    }
    if not a.no_stroke:
        for fn in arms.values():  # build, capture, warm
            fn(tex0.clone())
    torch.cuda.synchronize()
    wall = {k: [] for k in arms}
    texels = {}
    for _ in range(0 if a.no_stroke else a.repeats):
        for name, fn in arms.items():
            tex = tex0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(tex)
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            texels[name] = int((tex != tex0).any(dim=-1).sum())
    stroke = {}
    for name in ([] if a.no_stroke else arms):
        med = statistics.median(wall[name])
        stroke[name] = dict(wall_ms=[round(v, 1) for v in wall[name]], median_wall_ms=round(med, 1), per_stamp_ms=round(med / 16, 2),
                            texels_changed=texels[name])
    if not a.no_stroke:
        diff = (stroke["masked"]["median_wall_ms"] - stroke["unmasked"]["median_wall_ms"]) / 16
        stroke["per_stamp_difference_ms"] = round(diff, 3)
        stroke["per_stamp_difference_percent_of_a_stamp"] = round(100 * diff / stroke["unmasked"]["per_stamp_ms"], 2)
    # the valid + backproject launches on their own, per stamp
    tex = tex0.clone()
    dec = torch.randn(R, R, 4, device=dev)
    mask = torch.ones(R, R, dtype=torch.uint8, device=dev)
    cams = [mesh_camera(p, n, q, fov) for p, n, q in zip(positions, normals, prevs)]
    back = {"unmasked": [], "masked": []}
    for rep in range(2):  # (the first round warms up)
        back = {"unmasked": [], "masked": []}
        for i, c in enumerate(cams):
            _, fidx = ops.mesh_render(mesh, c, fov, tex, R)
            pair = (("unmasked", None), ("masked", face_mask))
            for name, fm in (pair if (i // 4) % 2 == 0 else pair[::-1]):  # the second backprojection of a pair is the slower one: take turns
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                for _ in range(4):
                    blocker @ blocker
                ev[0].record()
                ops.mesh_backproject(mesh, dec, mask, fidx, tex, face_mask=fm)
                ev[1].record()
                torch.cuda.synchronize()
                back[name].append(ev[0].elapsed_time(ev[1]))
    stroke["backproject_alone"] = {k: dict(median_ms=round(statistics.median(v), 4), max_ms=round(max(v), 4)) for k, v in back.items()}
    out["stroke"] = stroke
    print(json.dumps(out))


if __name__ == "__main__":
    main()
