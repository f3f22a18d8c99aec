#!/usr/bin/env python3
"""What a view of the painted mesh costs, in one process on one MI355X, warmed up, medians with their spread:
  - a frame at 1280 x 720 and 1920 x 1080 of the 100 352-face height field and of a 2^20-face one, from a far pose (most faces smaller
    than a pixel) and a near one (the eye a tenth of a unit above the surface: faces of many pixels, some across more than 2 x 2 bins):
    the device time between events, enqueued behind a blocker so that no host gap is counted, and the wall time of `render_view` until
    its stream is idle; the same frames with the binning bypassed (`ops.mesh_view(binned=False)`: every tile streams every drawn face);
  - the 16-stamp 512^2 `paint_mesh_stroke(bleed=4)` of tools/mesh_bleed_timing.py with a 30 Hz `render_view(live=True)` loop beside it,
    against the same stroke alone, alternating: the per-stamp difference, the frames' latencies, and the two textures' digests;
  - with --parent-lib PATH (a libdtp.so built from the parent commit): the 16-stamp `bleed=0` stroke in fresh child processes, bound in
    turn to that library ($DTP_LIB) and to this build's, before this process touches the GPU (tools/mesh_pick_timing.py --child): the
    texture digests must be identical and the medians within the spread.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_pick_timing import digest, grid_field, stroke_setup, summary  # noqa: E402

SIZES = {"1280x720": (720, 1280), "1920x1080": (1080, 1920)}
# eye, at, up, fov_y, near
POSES = {"far": ((0.0, -6.0, 5.0), (0.0, 0.0, 0.0), (0, 0, 1), 45.0, 0.05),
         "near": ((0.0, 0.0, 0.22), (0.5, 0.3, 0.0), (0, 0, 1), 60.0, 0.01)}


def med(v, nd=4):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def frame_times(m, data, tex, repeats):
    from diffusiontexturepainting_amd import ops
    mesh = m.load_mesh(*data)
    out = dict(faces=int(data[1].shape[0]))
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    for pose, (eye, at, up, fov, near) in POSES.items():
        for label, size in SIZES.items():
            cam = mesh.view_camera(eye, at, up, fov, size, near)
            row = {}
            image, face_idx = m.render_view(mesh, tex, cam, want_face_idx=True)
            torch.cuda.synchronize()
            row["covered_pixels"] = int((face_idx >= 0).sum())
            row["faces_shown"] = int(torch.unique(face_idx).numel()) - 1
            for arm, binned in (("binned", True), ("every_tile_streams_every_face", False)):
                other = ops.mesh_view(mesh, tex, cam, binned=binned, want_depth=False)[0]
                torch.cuda.synchronize()
                row.setdefault("arms_byte_identical", True)
                row["arms_byte_identical"] = row["arms_byte_identical"] and bool(torch.equal(other, image))
                dev, wall = [], []
                for _ in range(repeats):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    for _ in range(4):  # a few milliseconds of queued work: the view's launches are all enqueued before the first one starts
                        blocker @ blocker
                    ev[0].record()
                    ops.mesh_view(mesh, tex, cam, binned=binned, want_face_idx=False, want_depth=False)
                    ev[1].record()
                    torch.cuda.synchronize()
                    dev.append(ev[0].elapsed_time(ev[1]))
                    if binned:
                        t0 = time.perf_counter()
                        m.render_view(mesh, tex, cam, out=image, live=True)
                        m.view_stream.synchronize()
                        wall.append((time.perf_counter() - t0) * 1e3)
                row[arm] = dict(device_ms=med(dev))
                if wall:
                    row[arm]["render_view_wall_ms"] = med(wall)
            row["bins_buy_x"] = round(row["every_tile_streams_every_face"]["device_ms"]["median"] / row["binned"]["device_ms"]["median"], 1)
            out[f"{pose}_{label}"] = row
    mesh.close()
    return out


def stroke_with_views(a, repeats):
    """The bleed = 4 stroke alone, and with a 30 Hz live view loop beside it, alternating."""
    m, mesh, data, st, tex0, _ = stroke_setup(a)
    positions = [(-0.6 + 0.4 * (i % 4), -0.45 + 0.3 * (i // 4), 0.1) for i in range(16)]
    normals = [(0.1 * ((i % 3) - 1), 0.1 * ((i % 2) - 0.5), 1.0) for i in range(16)]
    prevs = [(x, y + 0.1, z) for x, y, z in positions]
    eye, at, up, fov, near = (0.4, -1.9, 1.5), (0.0, 0.0, 0.0), (0, 0, 1), 45.0, 0.05
    cam = mesh.view_camera(eye, at, up, fov, SIZES["1280x720"], near)
    frame = torch.empty(720, 1280, 4, dtype=torch.uint8, device="cuda:0")
    latencies, frames = [], []

    def stroke(tex):
        return m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, 0.25, seeds=list(range(500, 516)), bleed=4, **st)

    def with_views(tex):
        stroke(tex)
        n, t_next = 0, time.perf_counter()
        while not m.stream.query():
            t0 = time.perf_counter()
            m.render_view(mesh, tex, cam, out=frame, live=True)
            m.view_stream.synchronize()
            latencies.append((time.perf_counter() - t0) * 1e3)
            n += 1
            t_next += 1.0 / 30.0
            while time.perf_counter() < t_next and not m.stream.query():
                time.sleep(0.0005)
        frames.append(n)

    arms = dict(alone=stroke, with_views=with_views)
    for f in arms.values():
        f(tex0.clone())
    torch.cuda.synchronize()
    latencies.clear()
    frames.clear()
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
    alone, views = summary(wall["alone"], 16), summary(wall["with_views"], 16)
    return m, data, tex0, dict(alone=alone, with_a_30_hz_live_view_loop=views, frames_per_stroke=frames, frame_latency_ms=med(latencies, 3),
                               per_stamp_difference_ms=round(views["per_stamp_ms"] - alone["per_stamp_ms"], 2),
                               texture_byte_identical=digest(last["alone"]) == digest(last["with_views"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the bleed=0 stroke comparison")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library of the --parent-lib comparison, alternating")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(res=a.res, texture=a.texture, ddim_steps=a.ddim_steps, repeats=a.repeats)
    if a.parent_lib:  # first, each in a process of its own, the two libraries alternating: this process has not opened the GPU yet
        cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_pick_timing.py"), "--child", "--res", str(a.res),
               "--texture", str(a.texture), "--ddim-steps", str(a.ddim_steps), "--repeats", "3", "--grid", str(a.grid)]
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
        meds = {k: [p["median_wall_ms"] for p in v] for k, v in ab.items()}
        diff = statistics.median(meds["this_build"]) - statistics.median(meds["parent"])
        spread = max([max(v) - min(v) for v in meds.values()] + [p["spread_ms"] for v in ab.values() for p in v])
        out["bleed_0_stroke_against_the_parent_build"] = dict(
            processes_per_library=a.processes, parent=ab["parent"], this_build=ab["this_build"],
            texture_byte_identical=len({p["sha256"] for v in ab.values() for p in v}) == 1,
            median_difference_ms_per_stroke=round(diff, 1), spread_ms=round(spread, 1), within_the_spread=abs(diff) <= spread)

    m, data, tex0, out["stroke_bleed_4"] = stroke_with_views(a, min(a.repeats, 3))
    out["frames"] = {"height_field_225": frame_times(m, data, tex0, a.repeats),
                     "height_field_2_to_20": frame_times(m, grid_field(1025, 513), tex0, a.repeats)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
