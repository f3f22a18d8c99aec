#!/usr/bin/env python3
"""What the changed tiles of an image cost, against what a client has without them: a copy of the whole image.  The
2048^2 atlas and the 16-stamp 512^2 / 20-step stroke of tools/journal_timing.py, `paint_mesh_stroke(bleed=4)`: a scan after one stamp,
after the whole stroke and with nothing changed -- the three launches between events on the model's stream, the tiles emitted, the bytes
read back, and the wall time of pull() with its read-back -- next to `texture.cpu()` and a copy into pinned memory of the whole atlas.
The same for a 720 x 1280 frame of render_view across a small camera step, pulled on the view's stream.  One process, warmed up, medians
and spread of --repeats runs.

--parent-lib PATH: a libdtp.so built from the parent commit.  The stroke with no tracker then runs in fresh child processes, bound in
turn to that library ($DTP_LIB) and to this build, alternating, before this process touches the GPU: the textures must be byte-identical
and the per-stroke times are recorded side by side.  Prints one JSON line; --out writes it to a file as well."""
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
    mesh = m.load_mesh(*synthetic.make_height_field(a.grid, a.grid, seed=3))
    # the stroke of tools/mesh_stroke_timing.py
    positions = [(-0.6 + 0.4 * (i % 4), -0.45 + 0.3 * (i // 4), 0.1) for i in range(16)]
    normals = [(0.1 * ((i % 3) - 1), 0.1 * ((i % 2) - 0.5), 1.0) for i in range(16)]
    prevs = [(x, y + 0.1, z) for x, y, z in positions]
    tex0 = torch.randint(0, 256, (T, T, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to("cuda:0")

    def stroke(tex, n=16):
        return m.paint_mesh_stroke(mesh, tex, positions[:n], normals[:n], prevs[:n], 0.25, seeds=list(range(500, 500 + n)), bleed=a.bleed, **st)
    return m, mesh, tex0, stroke


def digest(tex):
    return hashlib.sha256(tex.cpu().numpy().tobytes()).hexdigest()


def summary(v, digits=4):
    return dict(runs=[round(x, digits) for x in v], median=round(statistics.median(v), digits), spread=round(max(v) - min(v), digits))


def note(msg):
    sys.stderr.write(f"[delta_timing] {msg}\n")
    sys.stderr.flush()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def child(a):
    _, _, tex0, stroke = setup(a)
    tex = tex0.clone()
    stroke(tex)
    ms = []
    for _ in range(a.repeats):
        tex.copy_(tex0)
        ms.append(wall(lambda: stroke(tex)))
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")) or "this build", sha256=digest(tex), wall_ms=ms)))


def measure(m, tracker, image, on, states, repeats):
    """states: name -> (before, after) images of the tracker's shape.  Per state and repeat: the image takes `before` and is pulled (the
    client is current), takes `after`, and then (a) the three launches of dtp_delta_scan run between events, (b) the same from the
    start, pull() with its read-back against the wall clock."""
    from diffusiontexturepainting_amd import _lib
    lib = _lib.load()
    stream = m.stream if on == "stroke" else m.view_stream
    out = {}
    for name, (before, after) in states.items():
        launch, pull_ms, n_tiles = [], [], 0
        for i in range(repeats + 1):  # (the first round warms up)
            for timed_pull in (False, True):
                image.copy_(before)
                tracker.pull(image, on=on)
                image.copy_(after)
                torch.cuda.synchronize()
                if timed_pull:
                    box = []
                    w = wall(lambda: box.append(tracker.pull(image, on=on)))
                    n_tiles = len(box[0][0])
                    assert box[0][2] == 0
                    if i:
                        pull_ms.append(w)
                else:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        _lib.check(lib.dtp_delta_scan(m._h, tracker.handle, image.data_ptr(), image.shape[0], image.shape[1],
                                                      C.c_void_p(stream.cuda_stream)), "dtp_delta_scan")
                        e1.record()
                    torch.cuda.synchronize()
                    if i:
                        launch.append(e0.elapsed_time(e1) * 1e3)
        out[name] = dict(tiles_emitted=n_tiles, bytes_read_back=8 + n_tiles * 1028, scan_three_launches_us=summary(launch, 1),
                         pull_wall_ms=summary(pull_ms))
    # what a client has without: the whole image
    cpu_ms, pinned_ms = [], []
    pinned = torch.empty(image.shape, dtype=torch.uint8, pin_memory=True)
    for i in range(repeats + 1):
        c = wall(lambda: image.cpu())
        p = wall(lambda: pinned.copy_(image, non_blocking=True))
        if i:
            cpu_ms.append(c); pinned_ms.append(p)
    out["whole_image"] = dict(bytes=image.numel(), cpu_wall_ms=summary(cpu_ms), copy_into_pinned_wall_ms=summary(pinned_ms))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--bleed", type=int, default=4)
    ap.add_argument("--frame", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the stroke with no tracker")
    ap.add_argument("--ab-rounds", type=int, default=2, help="child processes per build, alternating")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(res=a.res, texture=a.texture, stamps=16, ddim_steps=a.ddim_steps, repeats=a.repeats, bleed=a.bleed, frame=list(a.frame))
    ab = None
    if a.parent_lib:  # first, in processes of their own: this one has not opened the GPU yet
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--res", str(a.res), "--texture", str(a.texture), "--ddim-steps",
               str(a.ddim_steps), "--repeats", str(a.repeats), "--grid", str(a.grid), "--bleed", str(a.bleed)]
        ab = dict(parent=dict(wall_ms=[], sha256=set()), this=dict(wall_ms=[], sha256=set()))
        for k in range(2 * a.ab_rounds):
            which = "parent" if k % 2 == 0 else "this"
            note(f"the stroke with no tracker, {which} build, in a child process")
            env = dict(os.environ)
            if which == "parent":
                env["DTP_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("DTP_LIB", None)
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"the {which}-build run failed with status {r.returncode}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            ab[which]["wall_ms"] += got["wall_ms"]
            ab[which]["sha256"].add(got["sha256"])

    note("this build: setup")
    m, mesh, tex0, stroke = setup(a)
    tex = tex0.clone()
    stroke(tex, 1)
    one = tex.clone()
    tex.copy_(tex0)
    stroke(tex)
    whole = tex.clone()
    tracker = m.delta_tracker(tex)
    out["tracker"] = dict(tiles=tracker.capacity_tiles, shadow_MiB=tex.numel() / 2**20, payload_MiB_device_and_pinned=tracker.capacity_tiles / 1024)
    note("the atlas")
    out["atlas"] = measure(m, tracker, tex, "stroke", dict(after_one_stamp=(tex0, one), after_the_stroke=(tex0, whole), nothing_changed=(whole, whole)),
                           a.repeats)
    tracker.close()

    note("the frame")
    from diffusiontexturepainting_amd.mesh import view_camera
    H, W = a.frame
    frames = []
    for eye in ((0.3, -1.7, 2.9), (0.31, -1.7, 2.9)):
        f = torch.empty(H, W, 4, dtype=torch.uint8, device="cuda:0")
        m.render_view(mesh, whole, view_camera(eye, (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 45.0, (H, W), 0.05), out=f)
        frames.append(f)
    torch.cuda.synchronize()
    frame = frames[0].clone()
    tracker = m.delta_tracker(frame)
    out["frame_view"] = measure(m, tracker, frame, "view", dict(after_a_small_camera_step=(frames[0], frames[1]), nothing_changed=(frames[1], frames[1])),
                                a.repeats)
    out["frame_view"]["tiles_of_the_frame"] = tracker.capacity_tiles
    tracker.close()

    if ab is not None:
        p, t = ab["parent"], ab["this"]
        ps, ts = summary(p["wall_ms"], 2), summary(t["wall_ms"], 2)
        out["stroke_with_no_tracker_against_the_parent_build"] = dict(
            parent_wall_ms=ps, this_build_wall_ms=ts, texture_byte_identical=len(p["sha256"] | t["sha256"]) == 1,
            median_difference_ms_per_stroke=round(ts["median"] - ps["median"], 2),
            within_the_spread_of_the_repeats=abs(ts["median"] - ps["median"]) <= max(ps["spread"], ts["spread"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
