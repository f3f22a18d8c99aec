#!/usr/bin/env python3
"""What the bleed pass of a mesh stroke costs: the 16-stamp 512^2 / 20-step stroke of tools/mesh_stroke_timing.py on the
2048^2 atlas of the height field refined to about 100 k faces, `paint_mesh_stroke(bleed=0)` against `paint_mesh_stroke(bleed=4)` in one
process, alternating, warmed up, three repeats each: wall time from the call to the end of the device work.  The bleed launches on
their own between events: per stamp over the stamp's rectangle, and once over the whole texture.  The one-time coverage build (first
use: allocation, kernels, the wait) for the two extreme meshes, 2 faces and 100 352 faces over 2048^2.

--parent-lib PATH: a libdtp.so built from the parent commit.  The bleed=0 arm then runs once more in a fresh child process bound to
that library ($DTP_LIB), before this process touches the GPU; the child's texture must be byte-identical to this build's and its
per-stroke time is recorded next to it.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(a):
    from diffusiontexturepainting_amd import synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    R, T = a.res, a.texture
    sd = dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae())
    st = dict(steps=a.ddim_steps, context_pad=150, tg_steps=a.ddim_steps, cfg_weight=2.0, tg_weight=1.0)
    _, brush, _, _ = synthetic.make_stamp_batch(1, R, seed=1000)
    cond, uncond = synthetic.make_conditioning(7)
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    m.set_conditioning(cond, uncond, brush)
    data = synthetic.make_height_field(a.grid, a.grid, seed=3)
    mesh = m.load_mesh(*data)
    # the stroke of tools/mesh_stroke_timing.py
    positions = [(-0.6 + 0.4 * (i % 4), -0.45 + 0.3 * (i // 4), 0.1) for i in range(16)]
    normals = [(0.1 * ((i % 3) - 1), 0.1 * ((i % 2) - 0.5), 1.0) for i in range(16)]
    prevs = [(x, y + 0.1, z) for x, y, z in positions]
    tex0 = torch.randint(0, 256, (T, T, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to("cuda:0")

    def stroke(tex, bleed):
        return m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, 0.25, seeds=list(range(500, 516)), bleed=bleed, **st)
    return m, mesh, data, (positions, normals, prevs), tex0, stroke


def timed(stroke, tex0, bleeds, repeats):
    """Alternating arms -> {bleed: [wall ms]}, and the last texture of every arm."""
    for b in bleeds:  # build, capture, warm (and the coverage mask)
        stroke(tex0.clone(), b)
    torch.cuda.synchronize()
    wall, last = {b: [] for b in bleeds}, {}
    for _ in range(repeats):
        for b in bleeds:
            tex = tex0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stroke(tex, b)
            torch.cuda.synchronize()
            wall[b].append((time.perf_counter() - t0) * 1e3)
            last[b] = tex
    return wall, last


def digest(tex):
    return hashlib.sha256(tex.cpu().numpy().tobytes()).hexdigest()


def summary(ms):
    med = statistics.median(ms)
    return dict(wall_ms=[round(v, 1) for v in ms], median_wall_ms=round(med, 1), per_stamp_ms=round(med / 16, 2),
                spread_ms=round(max(ms) - min(ms), 1))


def child(a):
    _, _, _, _, tex0, stroke = setup(a)
    wall, last = timed(stroke, tex0, [0], a.repeats)
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), sha256=digest(last[0]), **summary(wall[0]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--bleed", type=int, default=4)
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the bleed=0 comparison")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(res=a.res, texture=a.texture, stamps=16, ddim_steps=a.ddim_steps, repeats=a.repeats, bleed=a.bleed)
    parent = None
    if a.parent_lib:  # first, and in a process of its own: this one has not opened the GPU yet
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--res", str(a.res), "--texture", str(a.texture), "--ddim-steps",
               str(a.ddim_steps), "--repeats", str(a.repeats), "--grid", str(a.grid)]
        r = subprocess.run(cmd, env={**os.environ, "DTP_LIB": os.path.abspath(a.parent_lib)}, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"the parent-library run failed with status {r.returncode}")
        parent = json.loads(r.stdout.strip().splitlines()[-1])

    from diffusiontexturepainting_amd import _lib, ops, synthetic
    from diffusiontexturepainting_amd.mesh import mesh_camera
    m, mesh, data, (positions, normals, prevs), tex0, stroke = setup(a)
    R, T, k = a.res, a.texture, a.bleed
    out["faces"] = int(data[1].shape[0])
    wall, last = timed(stroke, tex0, [0, k], a.repeats)
    out["bleed_0"], out[f"bleed_{k}"] = summary(wall[0]), summary(wall[k])
    diff = (out[f"bleed_{k}"]["median_wall_ms"] - out["bleed_0"]["median_wall_ms"]) / 16
    out["per_stamp_difference_ms"] = round(diff, 3)
    out["per_stamp_difference_percent_of_a_stamp"] = round(100 * diff / out["bleed_0"]["per_stamp_ms"], 2)
    # (stamp i + 1 renders what stamp i bled, so the arms differ in covered texels too: no byte comparison between them)
    cov = ops.mesh_coverage(mesh, T, T)
    out["uncovered_texels_the_stroke_changed"] = {f"bleed_{b}": int(((last[b] != tex0).any(dim=-1) & ~cov).sum()) for b in (0, k)}
    if parent is not None:
        mine = digest(last[0])
        out["bleed_0_against_the_parent_build"] = dict(
            parent=parent, this_build_sha256=mine, texture_byte_identical=parent["sha256"] == mine,
            median_difference_ms_per_stroke=round(out["bleed_0"]["median_wall_ms"] - parent["median_wall_ms"], 1),
            within_the_spread_of_the_repeats=abs(out["bleed_0"]["median_wall_ms"] - parent["median_wall_ms"])
            <= max(out["bleed_0"]["spread_ms"], parent["spread_ms"]))

    # the bleed launches alone, per stamp: render -> backproject as the stroke's, then the pass over the written texels' box grown by k
    lib = _lib.load()
    tex = tex0.clone()
    dec = torch.randn(R, R, 4, device="cuda:0")
    mask = torch.ones(R, R, dtype=torch.uint8, device="cuda:0")
    mask[0], mask[-1], mask[:, 0], mask[:, -1] = 0, 0, 0, 0
    cams = [mesh_camera(p, n, q, 0.25) for p, n, q in zip(positions, normals, prevs)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rep in range(2):  # (the first round warms up)
        back_ms, bleed_ms, texels = [], [], []
        for cam in cams:
            before = tex.clone()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            _, face_idx = ops.mesh_render(mesh, cam, 0.25, tex, R)
            ev[0].record()
            ops.mesh_backproject(mesh, dec, mask, face_idx, tex)
            ev[1].record()
            torch.cuda.synchronize()
            ys, xs = torch.nonzero((tex != before).any(dim=-1), as_tuple=True)
            rect = (C.c_int * 4)(int(xs.min()) - k, int(ys.min()) - k, int(xs.max()) + k, int(ys.max()) + k)
            ev[2].record()
            _lib.check(lib.dtp_mesh_bleed(mesh.handle, _lib.ptr(tex), T, T, k, C.byref(rect), stream), "dtp_mesh_bleed")
            ev[3].record()
            torch.cuda.synchronize()
            back_ms.append(ev[0].elapsed_time(ev[1]))
            bleed_ms.append(ev[2].elapsed_time(ev[3]))
            texels.append((rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1))
    whole_ms = []
    for _ in range(4):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t = tex0.clone()
        ev[0].record()
        _lib.check(lib.dtp_mesh_bleed(mesh.handle, _lib.ptr(t), T, T, k, None, stream), "dtp_mesh_bleed")
        ev[1].record()
        torch.cuda.synchronize()
        whole_ms.append(ev[0].elapsed_time(ev[1]))
    out["kernels_alone"] = dict(bleed_ms_median=round(statistics.median(bleed_ms), 4), bleed_ms_max=round(max(bleed_ms), 4),
                                backproject_ms_median=round(statistics.median(back_ms), 4),
                                rectangle_texels_median=int(statistics.median(texels)),
                                whole_texture_bleed_ms_median=round(statistics.median(whole_ms[1:]), 4))

    # the one-time coverage build, first use of a fresh mesh: wall ms including the allocation and the wait
    build = {}
    for name, d in (("2_faces", synthetic.make_quad()), (f"{out['faces']}_faces", data)):
        ms = []
        for _ in range(3):
            fresh = m.load_mesh(*d)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = ops.mesh_coverage(fresh, T, T)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            fresh.close()
        build[name] = dict(first_use_wall_ms=[round(v, 3) for v in ms], texels_covered=int(c.sum()))
    out["coverage_build_2048"] = build
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
