#!/usr/bin/env python3
"""What picking costs, in one process on one MI355X, warmed up, three repeats:
  - the wall time of `model.pick` for 1, 64 and 1024 rays on the 100 352-face height field and on a 2^20-face one, and the device time
    of the pick's work (frames in, slots zeroed, the two kernels) between events, enqueued behind a blocker so that no host gap is
    counted;
  - `paint_mesh_path` against `paint_mesh_stroke` fed the same stamps, alternating: the 512^2 / 20-step settings of
    tools/mesh_stroke_timing.py on the 2048^2 atlas, a pointer path that plans about 16 stamps;
  - with --parent-lib PATH (a libdtp.so built from the parent commit): the 16-stamp `bleed=0` stroke of tools/mesh_bleed_timing.py in
    fresh child processes, bound in turn to that library ($DTP_LIB) and to this build's, before this process touches the GPU: the
    texture digests must be identical and the medians within the spread (between processes of one library, and of the repeats).
Prints one JSON line; --out writes it to a file as well."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grid_field(nx, ny):
    """synthetic.make_height_field's surface (without its noise) and atlas, vectorised: 2 (nx - 1)(ny - 1) faces."""
    xs, ys = torch.linspace(-1.0, 1.0, nx, dtype=torch.float64), torch.linspace(-0.75, 0.75, ny, dtype=torch.float64)
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    zz = 0.35 * (torch.sin(3.1 * xx + 0.4) * torch.cos(2.3 * yy - 0.2) + 0.25 * torch.sin(9.0 * xx * yy))
    verts = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).to(torch.float32)
    j, i = torch.meshgrid(torch.arange(ny - 1), torch.arange(nx - 1), indexing="ij")
    a = (j * nx + i).reshape(-1)
    faces = torch.stack([torch.stack([a, a + 1, a + nx + 1], 1), torch.stack([a, a + nx + 1, a + nx], 1)], 1).reshape(-1, 3).to(torch.int32)
    uv = torch.stack([(verts[:, 0] + 1) / 2 * 0.94 + 0.03, (verts[:, 1] + 0.75) / 1.5 * 0.9 + 0.05], 1)
    return verts, faces, uv[faces.long()].contiguous()


def pick_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([0.95, 0.7, 0.0]) + torch.tensor([0.0, 0.0, 2.0])
    d = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([0.2, 0.2, 0.0]) + torch.tensor([0.0, 0.0, -1.0])
    return o, d


def stroke_setup(a):
    """The model, mesh and 16-stamp stroke of tools/mesh_bleed_timing.py."""
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
    positions = [(-0.6 + 0.4 * (i % 4), -0.45 + 0.3 * (i // 4), 0.1) for i in range(16)]
    normals = [(0.1 * ((i % 3) - 1), 0.1 * ((i % 2) - 0.5), 1.0) for i in range(16)]
    prevs = [(x, y + 0.1, z) for x, y, z in positions]
    tex0 = torch.randint(0, 256, (T, T, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to("cuda:0")

    def stroke(tex):
        return m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, 0.25, seeds=list(range(500, 516)), bleed=0, **st)
    return m, mesh, data, st, tex0, stroke


def timed(arms, tex0, repeats):
    """arms: {name: f(tex)} run alternating -> {name: [wall ms]}, and the last texture of every arm."""
    for f in arms.values():
        f(tex0.clone())
    torch.cuda.synchronize()
    wall, last = {k: [] for k in arms}, {}
    for _ in range(repeats):
        for k, f in arms.items():
            tex = tex0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(tex)
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            last[k] = tex
    return wall, last


def digest(tex):
    return hashlib.sha256(tex.cpu().numpy().tobytes()).hexdigest()


def summary(ms, stamps):
    med = statistics.median(ms)
    return dict(wall_ms=[round(v, 1) for v in ms], median_wall_ms=round(med, 1), per_stamp_ms=round(med / stamps, 2),
                spread_ms=round(max(ms) - min(ms), 1))


def child(a):
    _, _, _, _, tex0, stroke = stroke_setup(a)
    wall, last = timed(dict(stroke=stroke), tex0, a.repeats)
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), sha256=digest(last["stroke"]), **summary(wall["stroke"], 16))))


def pick_times(m, data, repeats):
    from diffusiontexturepainting_amd import ops
    mesh = m.load_mesh(*data)
    out = dict(faces=int(data[1].shape[0]))
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    for n in (1, 64, 1024):
        o, d = pick_rays(n, 40 + n)
        for _ in range(2):
            hits = m.pick(mesh, o, d)
            ops.mesh_pick(mesh, o, d)
        wall, dev = [], []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.pick(mesh, o, d)
            wall.append((time.perf_counter() - t0) * 1e3)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(4):  # a few milliseconds of queued work: the pick's launches are all enqueued before the first one starts
                blocker @ blocker
            ev[0].record()
            ops.mesh_pick(mesh, o, d)
            ev[1].record()
            torch.cuda.synchronize()
            dev.append(ev[0].elapsed_time(ev[1]))
        out[f"rays_{n}"] = dict(hits=int((hits["face"] >= 0).sum()), pick_wall_ms=[round(v, 3) for v in wall],
                                pick_wall_ms_median=round(statistics.median(wall), 3), device_ms=[round(v, 4) for v in dev],
                                device_ms_median=round(statistics.median(dev), 4))
    mesh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the bleed=0 stroke comparison")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library of the --parent-lib comparison, alternating")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(res=a.res, texture=a.texture, ddim_steps=a.ddim_steps, repeats=a.repeats)
    ab = None
    if a.parent_lib:  # first, each in a process of its own, the two libraries alternating: this process has not opened the GPU yet
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--res", str(a.res), "--texture", str(a.texture), "--ddim-steps",
               str(a.ddim_steps), "--repeats", str(a.repeats), "--grid", str(a.grid)]
        ab = dict(parent=[], this_build=[])
        for _ in range(a.processes):
            for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", "")):
                env = {k: v for k, v in os.environ.items() if k != "DTP_LIB"}
                if lib:
                    env["DTP_LIB"] = lib
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"the {arm} run failed with status {r.returncode}")
                ab[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))

    m, mesh, data, st, tex0, stroke = stroke_setup(a)
    # ---- the pick alone
    out["pick"] = {"height_field_225": pick_times(m, data, a.repeats), "height_field_2_to_20": pick_times(m, grid_field(1025, 513), a.repeats)}

    # ---- the pointer-to-paint call against the stroke fed the same stamps
    n_rays = 17
    origins = [(-0.8 + 1.6 * i / (n_rays - 1), -0.5 + 1.0 * i / (n_rays - 1), 2.0) for i in range(n_rays)]
    directions = [(0.03, 0.02, -1.0)] * n_rays
    radius, spr = 0.25, 2
    hits = m.pick(mesh, origins, directions)
    P, N, V, _ = mesh.plan_path(hits, radius / spr)
    stamps = int(P.shape[0])
    seeds = list(range(500, 500 + stamps))
    arms = dict(path=lambda tex: m.paint_mesh_path(mesh, tex, origins, directions, radius, stamps_per_radius=spr, seeds=seeds, **st),
                stroke=lambda tex: m.paint_mesh_stroke(mesh, tex, P, N, V, radius, seeds=seeds, **st))
    wall, last = timed(arms, tex0, a.repeats)
    out["paint_mesh_path"] = dict(rays=n_rays, stamps=stamps, path=summary(wall["path"], stamps), stroke_same_stamps=summary(wall["stroke"], stamps),
                                  texture_byte_identical=digest(last["path"]) == digest(last["stroke"]),
                                  median_difference_ms=round(statistics.median(wall["path"]) - statistics.median(wall["stroke"]), 2))

    # ---- the stroke of DESIGN.md 3.21, untouched by this feature: this build against the parent's
    wall, last = timed(dict(stroke=stroke), tex0, a.repeats)
    mine = summary(wall["stroke"], 16)
    out["bleed_0_stroke"] = mine
    if ab is not None:
        # every process is one sample of a library: its median over the repeats.  The spread that a difference has to be held against
        # is the larger of the spread between the processes of one library and the spread of the repeats inside a process.
        med = {k: [p["median_wall_ms"] for p in v] for k, v in ab.items()}
        diff = statistics.median(med["this_build"]) - statistics.median(med["parent"])
        spread = max([max(v) - min(v) for v in med.values()] + [p["spread_ms"] for v in ab.values() for p in v])
        out["bleed_0_stroke_against_the_parent_build"] = dict(
            processes_per_library=a.processes, parent=ab["parent"], this_build=ab["this_build"],
            texture_byte_identical=len({p["sha256"] for v in ab.values() for p in v} | {digest(last["stroke"])}) == 1,
            median_difference_ms_per_stroke=round(diff, 1), spread_ms=round(spread, 1), within_the_spread=abs(diff) <= spread)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
