#!/usr/bin/env python3
"""What the mip pyramid and the trilinear-filtered view cost, in one process on one MI355X, warmed up, medians with
their spread:
  - `build_mips` of a 2048^2 and a 512^2 texture: the device time between events, enqueued behind a blocker so that no host gap is
    counted, and the wall time until the stream is idle;
  - the eight frames of tools/mesh_view_timing.py (the 100 352-face height field and a 2^20-face one, a far and a near pose, 1280 x 720
    and 1920 x 1080) filtered (dtp_mesh_view_mips with a pyramid built beforehand) and unfiltered (dtp_mesh_view), alternating: device
    time, the pixels per level, and `render_view(filter="trilinear")` with the pyramid built inside, wall time;
  - with --parent-lib PATH (a libdtp.so built from the parent commit): the unfiltered frames and the 16-stamp `bleed=0` stroke of
    tools/mesh_pick_timing.py in fresh child processes, bound in turn to that library ($DTP_LIB) and to this build's, before this process
    touches the GPU: the frames' and the texture's digests must be identical and the medians within the spread.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_pick_timing import digest, grid_field, stroke_setup, summary, timed  # noqa: E402
from mesh_view_timing import POSES, SIZES, med  # noqa: E402


def behind_a_blocker(blocker, f, repeats):
    """Device ms of what f() enqueues on the current stream, everything enqueued before the first kernel of it starts."""
    dev = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(4):
            blocker @ blocker
        ev[0].record()
        f()
        ev[1].record()
        torch.cuda.synchronize()
        dev.append(ev[0].elapsed_time(ev[1]))
    return dev


def rows(m, a):
    """(name, mesh data) of the two height fields, and per row (pose_size, camera arguments)."""
    from diffusiontexturepainting_amd import synthetic
    fields = [("height_field_225", synthetic.make_height_field(a.grid, a.grid, seed=3)), ("height_field_2_to_20", grid_field(1025, 513))]
    views = [(f"{pose}_{label}", POSES[pose], size) for pose in POSES for label, size in SIZES.items()]
    return fields, views


def unfiltered_frames(m, tex, a, repeats):
    """The eight unfiltered frames: device ms and the frame's digest (what the parent commit's library computes as well)."""
    from diffusiontexturepainting_amd import ops
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    fields, views = rows(m, a)
    out = {}
    for name, data in fields:
        mesh = m.load_mesh(*data)
        for label, (eye, at, up, fov, near), size in views:
            cam = mesh.view_camera(eye, at, up, fov, size, near)
            image = ops.mesh_view(mesh, tex, cam, want_face_idx=False, want_depth=False)[0]
            torch.cuda.synchronize()
            dev = behind_a_blocker(blocker, lambda: ops.mesh_view(mesh, tex, cam, want_face_idx=False, want_depth=False), repeats)
            out[f"{name}_{label}"] = dict(sha256=digest(image), device_ms=med(dev))
        mesh.close()
    return out


def child(a):
    m, _, _, _, tex0, stroke = stroke_setup(a)
    wall, last = timed(dict(stroke=stroke), tex0, a.repeats)
    frames = unfiltered_frames(m, tex0, a, 5)
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), stroke=dict(sha256=digest(last["stroke"]), **summary(wall["stroke"], 16)),
                          frames=frames)))


def against_the_parent(a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--res", str(a.res), "--texture", str(a.texture), "--ddim-steps", str(a.ddim_steps),
           "--repeats", "3", "--grid", str(a.grid)]
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

    def compare(pick, spread_of):
        """this build's median against the parent's; the spread: the larger of the parent's two runs' distance and any run's own spread."""
        meds = {k: [pick(p)[0] for p in v] for k, v in ab.items()}
        diff = statistics.median(meds["this_build"]) - statistics.median(meds["parent"])
        spread = max([max(meds["parent"]) - min(meds["parent"])] + [spread_of(p) for v in ab.values() for p in v])
        return dict(parent=meds["parent"], this_build=meds["this_build"], byte_identical=len({pick(p)[1] for v in ab.values() for p in v}) == 1,
                    median_difference_ms=round(diff, 4), spread_ms=round(spread, 4), within_the_spread=diff <= spread)

    out = dict(processes_per_library=a.processes,
               stroke_16_stamps_bleed_0=compare(lambda p: (p["stroke"]["median_wall_ms"], p["stroke"]["sha256"]), lambda p: p["stroke"]["spread_ms"]))
    out["unfiltered_frames_device_ms"] = {
        k: compare(lambda p, k=k: (p["frames"][k]["device_ms"]["median"], p["frames"][k]["sha256"]),
                   lambda p, k=k: p["frames"][k]["device_ms"]["max"] - p["frames"][k]["device_ms"]["min"]) for k in ab["parent"][0]["frames"]}
    return out


def pyramid_times(m, repeats):
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    out = {}
    for side in (2048, 512):
        tex = torch.randint(0, 256, (side, side, 4), dtype=torch.uint8, device="cuda:0")
        mips = m.build_mips(tex)
        torch.cuda.synchronize()
        dev = behind_a_blocker(blocker, lambda: m.build_mips(tex, out=mips), repeats)
        wall = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.build_mips(tex, out=mips)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out[f"{side}x{side}"] = dict(bytes_read=4 * side * side, bytes_written=int(mips.numel()), device_ms=med(dev), wall_ms=med(wall))
    return out


def frame_times(m, tex, a, repeats):
    from diffusiontexturepainting_amd import _lib, mesh as _mesh, ops
    lib = _lib.load()
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    mips = m.build_mips(tex)
    levels = ops.mip_layout(tex.shape[0], tex.shape[1])["levels"]
    opts = _mesh.view_opts()
    fields, views = rows(m, a)
    out = {}
    for name, data in fields:
        mesh = m.load_mesh(*data)
        for label, (eye, at, up, fov, near), size in views:
            cam = mesh.view_camera(eye, at, up, fov, size, near)
            st = cam.struct()
            image = torch.empty(*size, 4, dtype=torch.uint8, device="cuda:0")

            def filtered():
                s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.check(lib.dtp_mesh_view_mips(mesh.handle, _lib.ptr(tex), tex.shape[0], tex.shape[1], _lib.ptr(mips), C.byref(st), size[0], size[1],
                                                  C.byref(opts), _lib.ptr(image), None, None, None, s), "dtp_mesh_view_mips")

            def unfiltered():
                s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.check(lib.dtp_mesh_view(mesh.handle, _lib.ptr(tex), tex.shape[0], tex.shape[1], C.byref(st), size[0], size[1], C.byref(opts),
                                             _lib.ptr(image), None, None, s), "dtp_mesh_view")

            frame, face_idx, lod = m.render_view(mesh, tex, cam, filter="trilinear", mips=mips, want_face_idx=True, want_lod=True)
            plain = m.render_view(mesh, tex, cam)
            torch.cuda.synchronize()
            covered = face_idx >= 0
            row = dict(covered_pixels=int(covered.sum()), pixels_that_differ=int((frame != plain).any(dim=2).sum()),
                       pixels_per_level=[int(((lod.floor() == k) & covered).sum()) for k in range(levels)])
            dev = dict(filtered=[], unfiltered=[])
            for _ in range(repeats):  # alternating
                dev["unfiltered"] += behind_a_blocker(blocker, unfiltered, 1)
                dev["filtered"] += behind_a_blocker(blocker, filtered, 1)
            wall = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.render_view(mesh, tex, cam, out=image, live=True, filter="trilinear")  # builds the pyramid on the view's stream first
                m.view_stream.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            row.update(unfiltered_device_ms=med(dev["unfiltered"]), filtered_device_ms=med(dev["filtered"]),
                       filter_adds_ms=round(statistics.median(dev["filtered"]) - statistics.median(dev["unfiltered"]), 4),
                       render_view_trilinear_building_the_pyramid_wall_ms=med(wall))
            out[f"{name}_{label}"] = row
        mesh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the comparison of the unchanged paths")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library of the --parent-lib comparison, alternating")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(res=a.res, texture=a.texture, ddim_steps=a.ddim_steps, repeats=a.repeats)
    if a.parent_lib:  # first, each in a process of its own, the two libraries alternating: this process has not opened the GPU yet
        out["unchanged_paths_against_the_parent_build"] = against_the_parent(a)
    m, _, _, _, tex0, _ = stroke_setup(a)
    out["pyramid"] = pyramid_times(m, a.repeats)
    out["frames"] = frame_times(m, tex0, a, a.repeats)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
