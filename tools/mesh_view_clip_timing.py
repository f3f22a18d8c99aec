#!/usr/bin/env python3
"""What the near-plane clip of the view costs, by the method of tools/mesh_view_timing.py: one MI355X, warmed up, five
repeats, medians with their spread, the device time between events with the view's launches enqueued behind a blocker.
  - the frames of the 3.24 table (the 100 352-face height field and a 2^20-face one, far and near pose, 1280 x 720 and 1920 x 1080; none
    has a face across the near plane) WITHOUT the clip, in fresh child processes bound in turn to a libdtp.so of the parent commit
    (--parent-lib, $DTP_LIB) and to this build's, alternating, before this process touches the GPU: the frames' digests must be
    identical and the medians within the spread;
  - the same frames WITH the clip against without it, in one process of this build, alternating: what the extra branch costs;
  - one interior pose at 1280 x 720, reported only: the 12-face cube and the 100 352-face field with the eye inside, both filters;
  - with --stroke: the 16-stamp bleed = 0 stroke of tools/mesh_pick_timing.py --child once per library: its texture's sha256.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_pick_timing import grid_field  # noqa: E402
from mesh_view_timing import POSES, SIZES, med  # noqa: E402

# eye, at, up, fov_y, near
INTERIOR = {"cube_12_faces": ((0.4, -0.3, 0.1), (0.3, 0.5, -0.1), (0, 0, 1), 45.0, 0.05),
            "height_field_225": ((-0.2, 0.0, 0.25), (0.9, 0.1, 0.2), (0, 0, 1), 70.0, 0.2)}


def cube():
    v = [[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)]
    sides = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f, uv = [], []
    for s, (a, b, c, d) in enumerate(sides):
        u0, v0 = 0.05 + 0.3 * (s % 3), 0.05 + 0.45 * (s // 3)
        q = [(u0, v0), (u0 + 0.25, v0), (u0 + 0.25, v0 + 0.4), (u0, v0 + 0.4)]
        f += [[a, b, c], [a, c, d]]
        uv += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int32), torch.tensor(uv, dtype=torch.float32)


def setup(texture):
    from diffusiontexturepainting_amd import weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    m = MI355ConditionalInpainter(64, device=0, weights=dict(unet=W.synthetic_unet(), lora=W.synthetic_lora(), vae=W.synthetic_vae()), max_batch=1)
    tex = torch.randint(0, 256, (texture, texture, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    return m, tex


def device_ms(call, repeats, blocker):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(4):  # a few milliseconds of queued work: the view's launches are all enqueued before the first one starts
            blocker @ blocker
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return out


def table_frames(m, tex, repeats, clip_arms):
    """The frames of the 3.24 table -> {mesh: {pose_size: {arm: device_ms, sha256}}}; arms alternate within a frame."""
    from diffusiontexturepainting_amd import ops, synthetic
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    out = {}
    for name, data in (("height_field_225", synthetic.make_height_field(225, 225, seed=3)), ("height_field_2_to_20", grid_field(1025, 513))):
        mesh = m.load_mesh(*data)
        rows = {}
        for pose, (eye, at, up, fov, near) in POSES.items():
            for label, size in SIZES.items():
                cam = mesh.view_camera(eye, at, up, fov, size, near)
                row, times = {}, {arm: [] for arm in clip_arms}
                for arm in clip_arms:
                    kw = dict(clip_near=True) if arm == "clip_on" else {}
                    image = ops.mesh_view(mesh, tex, cam, **kw)[0]
                    torch.cuda.synchronize()
                    row.setdefault("sha256", {})[arm] = hashlib.sha256(image.cpu().numpy().tobytes()).hexdigest()[:16]
                for _ in range(repeats):  # one repeat of every arm in turn
                    for arm in clip_arms:
                        kw = dict(clip_near=True) if arm == "clip_on" else {}
                        times[arm] += device_ms(lambda: ops.mesh_view(mesh, tex, cam, want_face_idx=False, want_depth=False, **kw), 1, blocker)
                for arm in clip_arms:
                    row[arm] = med(times[arm])
                if len(clip_arms) == 2:
                    row["frames_byte_identical"] = row["sha256"]["clip_on"] == row["sha256"]["clip_off"]
                    row["clip_on_over_clip_off"] = round(row["clip_on"]["median"] / row["clip_off"]["median"], 3)
                rows[f"{pose}_{label}"] = row
        mesh.close()
        out[name] = rows
    return out


def interior(m, tex, repeats):
    from diffusiontexturepainting_amd import synthetic
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    out = {}
    for name, data in (("cube_12_faces", cube()), ("height_field_225", synthetic.make_height_field(225, 225, seed=3))):
        mesh = m.load_mesh(*data)
        eye, at, up, fov, near = INTERIOR[name]
        cam = mesh.view_camera(eye, at, up, fov, SIZES["1280x720"], near)
        row = {}
        mips = m.build_mips(tex)
        for clip in (False, True):
            _, face_idx = m.render_view(mesh, tex, cam, want_face_idx=True, clip_near=clip)
            torch.cuda.synchronize()
            row["covered_pixels_clip_on" if clip else "covered_pixels_clip_off"] = int((face_idx >= 0).sum())
            for filt in ("bilinear", "trilinear"):
                kw = dict(filter=filt, mips=mips) if filt == "trilinear" else {}
                t = device_ms(lambda: m.render_view(mesh, tex, cam, clip_near=clip, **kw), repeats, blocker)  # (the view's stream waits for the blocker)
                row[f"{filt}_clip_{'on' if clip else 'off'}_device_ms"] = med(t)
        mesh.close()
        out[name] = row
    return out


def child(a):
    m, tex = setup(a.texture)
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), frames=table_frames(m, tex, a.repeats, ["clip_off"]))))


def run_child(cmd, lib):
    env = {k: v for k, v in os.environ.items() if k != "DTP_LIB"}
    if lib:
        env["DTP_LIB"] = lib
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"a child run failed with status {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the clip-off comparison")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library, alternating")
    ap.add_argument("--stroke", action="store_true", help="with --parent-lib: also the 16-stamp stroke's sha256, once per library")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    here = os.path.dirname(os.path.abspath(__file__))
    out = dict(texture=a.texture, repeats=a.repeats)
    if a.parent_lib:  # first, each in a process of its own: this process has not opened the GPU yet
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--texture", str(a.texture), "--repeats", str(a.repeats)]
        ab = dict(parent=[], this_build=[])
        for _ in range(a.processes):
            for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", "")):
                ab[arm].append(run_child(cmd, lib)["frames"])
        rows = {}
        for mesh in ab["parent"][0]:
            for frame in ab["parent"][0][mesh]:
                meds = {arm: [p[mesh][frame]["clip_off"]["median"] for p in v] for arm, v in ab.items()}
                spread = max(p[mesh][frame]["clip_off"]["max"] - p[mesh][frame]["clip_off"]["min"] for v in ab.values() for p in v)
                spread = max([spread] + [max(v) - min(v) for v in meds.values()])
                diff = statistics.median(meds["this_build"]) - statistics.median(meds["parent"])
                rows[f"{mesh}_{frame}"] = dict(parent_ms=meds["parent"], this_build_ms=meds["this_build"], difference_ms=round(diff, 4),
                                               spread_ms=round(spread, 4), within_the_spread=abs(diff) <= spread,
                                               frames_byte_identical=len({p[mesh][frame]["sha256"]["clip_off"] for v in ab.values() for p in v}) == 1)
        out["clip_off_against_the_parent_build"] = dict(processes_per_library=a.processes, frames=rows)
        if a.stroke:
            cmd = [sys.executable, os.path.join(here, "mesh_pick_timing.py"), "--child", "--res", "512", "--texture", "2048", "--ddim-steps", "20",
                   "--repeats", "1", "--grid", "225"]
            strokes = {arm: run_child(cmd, lib) for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", ""))}
            out["stroke_16_stamps"] = dict(strokes, texture_byte_identical=strokes["parent"]["sha256"] == strokes["this_build"]["sha256"])
    m, tex = setup(a.texture)
    out["clip_on_against_clip_off"] = table_frames(m, tex, a.repeats, ["clip_off", "clip_on"])
    out["interior_1280x720"] = interior(m, tex, a.repeats)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
