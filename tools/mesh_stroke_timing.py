#!/usr/bin/env python3
"""What the render and the backprojection of a mesh stroke cost per stamp: one 16-stamp stroke at 512^2 / 20 steps on a
2048^2 texture over the height field refined to about 100 k faces (`paint_mesh_stroke`), against `paint_stroke(max_group=1)` with the
same number of stamps and the same seeds, in one process, alternating, warmed up, three repeats each.  Wall time from the call to the
end of the device work, the host time of the call itself, and the two mesh kernels' groups on their own between events (render =
reset + project + render; backproject = valid + backproject).  A third arm, `paint_mesh_stroke(occlude=1.0)`, runs beside the plain one and is compared with it
alone: the per-stamp difference next to the spread of the repeats of both arms, and the occluded backprojection between events on the
same renders.  Prints one JSON line; --out also writes it to a file.
  With --parent-lib PATH (a libdtp.so built from the parent commit) the tool runs only this: the stroke plain, with bleed=4, with a
one-chart face_mask and with occlude=1.0, in fresh child processes bound in turn to that library ($DTP_LIB) and to this build's, before
this process touches the GPU; per arm the texture digests of the two libraries must be equal (or the exit status is 1), and the
difference of the per-stamp medians is reported next to the spread, with the kernel groups (render, valid + backproject, bleed) between
events (the bleed there is one pass over the whole texture, not a stamp's box) and the coverage build of two texture-filling faces, which the 100 k small faces never hand to the tile pass."""
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


AB_ARMS = ("plain", "bleed_4", "face_mask_one_chart", "occlude_1")


def child(a, m, mesh, tex0, stroke, cams, fov, faces, uvs):
    """One process of the --parent-lib comparison, on whatever library $DTP_LIB names: the four arms of the 16-stamp stroke alternating,
    the sha256 of each arm's texture, and the kernel groups and the coverage build of two large faces on their own between events."""
    import ctypes
    from diffusiontexturepainting_amd import _lib, ops, synthetic
    from diffusiontexturepainting_amd.mesh import faceset_from_bool
    R, T = a.res, a.texture
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    left = faceset_from_bool(uvs[:, :, 0].max(dim=1).values < 0.5).to(tex0.device)  # make_height_field's left chart: u in [0.03, 0.47], the other one starts at 0.53
    arms = dict(zip(AB_ARMS, (dict(), dict(bleed=4), dict(face_mask=left), dict(occlude=1.0))))
    for kw in arms.values():  # build, capture, warm (and the coverage mask)
        stroke(tex0.clone(), **kw)
    torch.cuda.synchronize()
    wall, sha = {k: [] for k in arms}, {}
    for _ in range(a.repeats):
        for name, kw in arms.items():
            tex = tex0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stroke(tex, **kw)
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            sha[name] = hashlib.sha256(tex.cpu().numpy().tobytes()).hexdigest()
    dec = torch.randn(R, R, 4, device=tex0.device)
    mask = torch.ones(R, R, dtype=torch.uint8, device=tex0.device)
    mask[0], mask[-1], mask[:, 0], mask[:, -1] = 0, 0, 0, 0
    groups = {}
    for rep in range(2):  # (the first round warms up)
        groups = dict(render=[], backproject=[], backproject_occluded=[], bleed_4_whole_texture=[])
        for i, cam in enumerate(cams):
            texs = [tex0.clone() for _ in range(2)]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            _, face_idx = ops.mesh_render(mesh, cam, fov, tex0, R)
            ev[1].record()
            order = (False, True) if (i + rep) % 2 == 0 else (True, False)  # (the second of a pair is the slower whatever it is)
            for j, occluded in enumerate(order):
                ops.mesh_backproject(mesh, dec, mask, face_idx, texs[j], fov=fov, occlude=1.0 if occluded else None)
                ev[2 + j].record()
            _lib.check(_lib.load().dtp_mesh_bleed(mesh.handle, _lib.ptr(texs[0]), T, T, 4, None, stream), "dtp_mesh_bleed")
            ev[4].record()
            torch.cuda.synchronize()
            groups["render"].append(ev[0].elapsed_time(ev[1]))
            groups["backproject_occluded" if order[0] else "backproject"].append(ev[1].elapsed_time(ev[2]))
            groups["backproject_occluded" if order[1] else "backproject"].append(ev[2].elapsed_time(ev[3]))
            groups["bleed_4_whole_texture"].append(ev[3].elapsed_time(ev[4]))
    cover = []
    for _ in range(a.repeats + 1):  # cover_faces hands both faces to cover_tiles; the first build warms up
        fresh = m.load_mesh(*synthetic.make_quad())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.mesh_coverage(fresh, T, T)
        torch.cuda.synchronize()
        cover.append((time.perf_counter() - t0) * 1e3)
        fresh.close()
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), sha256=sha, wall_ms={k: [round(v, 1) for v in w] for k, w in wall.items()},
                          kernel_group_ms_median={k: round(statistics.median(v), 4) for k, v in groups.items()},
                          coverage_build_2_faces_wall_ms=[round(v, 3) for v in cover[1:]])))


def against_parent(a):
    """Fresh child processes, bound in turn to the parent's library ($DTP_LIB) and to this build's: per arm the digests must be equal and
    the difference of the per-stamp medians (over all repeats of a library) is held against the spread of those repeats, max - min, of the
    library that spreads more; both spreads are reported."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--res", str(a.res), "--texture", str(a.texture), "--ddim-steps", str(a.ddim_steps),
           "--repeats", str(a.repeats), "--grid", str(a.grid)]
    runs = dict(parent=[], this_build=[])
    for _ in range(a.processes):
        for side, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", "")):
            env = {k: v for k, v in os.environ.items() if k != "DTP_LIB"}
            if lib:
                env["DTP_LIB"] = lib
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"the {side} run failed with status {r.returncode}")
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
            sys.stderr.write(f"[mesh_stroke_timing] {side}: process {len(runs[side])} of {a.processes} done\n")
    out = dict(res=a.res, texture=a.texture, ddim_steps=a.ddim_steps, stamps=16, repeats=a.repeats, processes_per_library=a.processes, arms={})
    for arm in AB_ARMS:
        ms = {side: [w / 16 for p in v for w in p["wall_ms"][arm]] for side, v in runs.items()}  # every repeat of every process, per stamp
        spread = {side: max(v) - min(v) for side, v in ms.items()}
        diff = statistics.median(ms["this_build"]) - statistics.median(ms["parent"])
        digests = {p["sha256"][arm] for v in runs.values() for p in v}
        out["arms"][arm] = dict(per_stamp_ms_median={k: round(statistics.median(v), 3) for k, v in ms.items()},
                                per_stamp_ms_spread_of_the_repeats={k: round(v, 3) for k, v in spread.items()}, per_stamp_difference_ms=round(diff, 3),
                                within_the_spread=abs(diff) <= max(spread.values()), sha256=sorted(digests), texture_byte_identical=len(digests) == 1)
    for key in ("kernel_group_ms_median", "coverage_build_2_faces_wall_ms"):
        out[key] = {side: [p[key] for p in v] for side, v in runs.items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(r["texture_byte_identical"] for r in out["arms"].values()):
        raise SystemExit("the textures of the two libraries differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit: run only the comparison of the four stroke arms with it")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library of the --parent-lib comparison, alternating")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.parent_lib:
        return against_parent(a)
    from diffusiontexturepainting_amd import ops, synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from diffusiontexturepainting_amd.mesh import mesh_camera
    dev = torch.device("cuda", 0)
    R, T = a.res, a.texture
    sd = dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae())
    st = dict(steps=a.ddim_steps, context_pad=150, tg_steps=a.ddim_steps, cfg_weight=2.0, tg_weight=1.0)
    _, brush, _, _ = synthetic.make_stamp_batch(1, R, seed=1000)
    cond, uncond = synthetic.make_conditioning(7)
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    m.set_conditioning(cond, uncond, brush)
    verts, faces, uvs = synthetic.make_height_field(a.grid, a.grid, seed=3)
    mesh = m.load_mesh(verts, faces, uvs)
    # a 4 x 4 grid of brush positions over the field, slightly tilted cameras, windows 0.5 wide (each sees about 1/12 of the faces)
    positions = [(-0.6 + 0.4 * (i % 4), -0.45 + 0.3 * (i // 4), 0.1) for i in range(16)]
    normals = [(0.1 * ((i % 3) - 1), 0.1 * ((i % 2) - 0.5), 1.0) for i in range(16)]
    prevs = [(x, y + 0.1, z) for x, y, z in positions]
    fov = 0.25
    per_row = T // R
    windows = [((i % per_row) * R, (i // per_row) * R) for i in range(16)]
    seeds = list(range(500, 516))
    tex0 = torch.randint(0, 256, (T, T, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)

    arms = {
        "paint_mesh_stroke": lambda tex: m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, fov, seeds=seeds, **st),
        "paint_mesh_stroke_occluded": lambda tex: m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, fov, seeds=seeds, occlude=1.0, **st),
        "paint_stroke_serial": lambda tex: m.paint_stroke(tex, windows, seeds=seeds, max_group=1, margin=1, **st),
    }
    if a.child:
        return child(a, m, mesh, tex0, lambda tex, **kw: m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, fov, seeds=seeds, **kw, **st),
                     [mesh_camera(p, n, q, fov) for p, n, q in zip(positions, normals, prevs)], fov, faces, uvs)
    for fn in arms.values():  # build, capture, warm
        fn(tex0.clone())
    torch.cuda.synchronize()
    wall, host = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, fn in arms.items():
            tex = tex0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(tex)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[name].append((t1 - t0) * 1e3)
            wall[name].append((t2 - t0) * 1e3)
    # the two kernel groups on their own, per stamp
    tex = tex0.clone()
    dec = torch.randn(R, R, 4, device=dev)
    mask = torch.ones(R, R, dtype=torch.uint8, device=dev)
    mask[0], mask[-1], mask[:, 0], mask[:, -1] = 0, 0, 0, 0
    cams = [mesh_camera(p, n, q, fov) for p, n, q in zip(positions, normals, prevs)]
    render_ms, back_ms, shown, written = [], [], [], []
    for rep in range(2):  # (the first round warms up)
        render_ms, back_ms = [], []
        for cam in cams:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            before = tex.clone()
            ev[0].record()
            _, face_idx = ops.mesh_render(mesh, cam, fov, tex, R)
            ev[1].record()
            ops.mesh_backproject(mesh, dec, mask, face_idx, tex)
            ev[2].record()
            torch.cuda.synchronize()
            render_ms.append(ev[0].elapsed_time(ev[1]))
            back_ms.append(ev[1].elapsed_time(ev[2]))
            if rep == 1:
                shown.append(int(face_idx.unique().numel()) - int((face_idx < 0).any()))
                written.append(int((tex != before).any(dim=-1).sum()))
    # valid + backproject, plain against occluded, on the same render's records into a texture each; the second of a pair is the slower
    # whatever it is, so the arms take turns to go first
    pair_ms, differ = {False: [], True: []}, []
    for rep in range(2):
        pair_ms = {False: [], True: []}
        for i, cam in enumerate(cams):
            _, face_idx = ops.mesh_render(mesh, cam, fov, tex0, R)
            texs = {False: tex0.clone(), True: tex0.clone()}
            for occluded in ((False, True) if (i + rep) % 2 == 0 else (True, False)):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                ops.mesh_backproject(mesh, dec, mask, face_idx, texs[occluded], fov=fov, occlude=1.0 if occluded else None)
                ev[1].record()
                torch.cuda.synchronize()
                pair_ms[occluded].append(ev[0].elapsed_time(ev[1]))
            if rep == 1:
                differ.append(int((texs[False] != texs[True]).any(dim=-1).sum()))
    out = dict(res=R, texture=T, faces=int(faces.shape[0]), stamps=16, ddim_steps=a.ddim_steps, repeats=a.repeats)
    for name in arms:
        med = statistics.median(wall[name])
        out[name] = dict(wall_ms=[round(v, 1) for v in wall[name]], median_wall_ms=round(med, 1), per_stamp_ms=round(med / 16, 2),
                         host_ms_until_the_call_returned=round(statistics.median(host[name]), 1))
    diff = (out["paint_mesh_stroke"]["median_wall_ms"] - out["paint_stroke_serial"]["median_wall_ms"]) / 16
    out["per_stamp_difference_ms"] = round(diff, 3)
    out["per_stamp_difference_percent_of_a_stamp"] = round(100 * diff / out["paint_stroke_serial"]["per_stamp_ms"], 2)
    out["kernels_alone"] = dict(render_ms_median=round(statistics.median(render_ms), 3), render_ms_max=round(max(render_ms), 3),
                                backproject_ms_median=round(statistics.median(back_ms), 3), backproject_ms_max=round(max(back_ms), 3),
                                faces_shown_median=int(statistics.median(shown)), texels_written_median=int(statistics.median(written)))
    plain, occl = wall["paint_mesh_stroke"], wall["paint_mesh_stroke_occluded"]
    d = (statistics.median(occl) - statistics.median(plain)) / 16
    out["occlude"] = dict(occlude=1.0, per_stamp_difference_ms_against_the_plain_arm=round(d, 3),
                          per_stamp_difference_percent_of_a_stamp=round(100 * d / out["paint_mesh_stroke"]["per_stamp_ms"], 2),
                          spread_of_the_repeats_ms_per_stamp=dict(plain=round((max(plain) - min(plain)) / 16, 3),
                                                                  occluded=round((max(occl) - min(occl)) / 16, 3)),
                          backproject_ms_median_with_the_arms_taking_turns=dict(plain=round(statistics.median(pair_ms[False]), 3),
                                                                                occluded=round(statistics.median(pair_ms[True]), 3)),
                          backproject_ms_max_with_the_arms_taking_turns=dict(plain=round(max(pair_ms[False]), 3), occluded=round(max(pair_ms[True]), 3)),
                          texels_that_differ_from_the_plain_backprojection_median=int(statistics.median(differ)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
