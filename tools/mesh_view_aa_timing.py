#!/usr/bin/env python3
"""What the anti-aliased view costs, by the method of tools/mesh_view_timing.py: one MI355X, one process, warmed up,
five repeats, medians with their spread, the device time between events with the launches enqueued behind a blocker.
  - the 100 352-face height field and a 2^20-face one, far and near pose, at 1280 x 720 with samples = 2 and at 1024 x 576 with
    samples = 4, three arms alternating within a row: `samples=s` (the fused frame); today's frame at s x the size alone; that frame
    plus its resolve with torch integer ops.  The fused frame's bytes must equal the resolved arm's in every row;
  - with --parent-lib: the eight unfiltered frames of the 3.24 table in fresh child processes bound in turn to a libdtp.so of the
    parent commit ($DTP_LIB) and to this build's, alternating, before this process touches the GPU (tools/mesh_view_clip_timing.py
    --child): one sha256 per row, the medians against the spread; with --stroke also the 16-stamp bleed = 0 stroke of
    tools/mesh_pick_timing.py --child once per library: its texture's sha256.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_pick_timing import grid_field  # noqa: E402
from mesh_view_clip_timing import device_ms, run_child, setup  # noqa: E402
from mesh_view_timing import POSES, med  # noqa: E402

CONFIGS = {"1280x720_samples_2": ((720, 1280), 2), "1024x576_samples_4": ((576, 1024), 4)}
ARMS = ("fused", "fine_frame_alone", "fine_frame_plus_resolve")


def resolve(fine, s):
    H, W = fine.shape[0] // s, fine.shape[1] // s
    total = fine.view(H, s, W, s, 4).to(torch.int32).sum(dim=(1, 3))
    return ((total + (s * s) // 2) >> (2 if s == 2 else 4)).to(torch.uint8)


def aa_frames(m, tex, repeats):
    from diffusiontexturepainting_amd import ops, synthetic
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    out = {}
    for name, data in (("height_field_225", synthetic.make_height_field(225, 225, seed=3)), ("height_field_2_to_20", grid_field(1025, 513))):
        mesh = m.load_mesh(*data)
        rows = {}
        for pose, (eye, at, up, fov, near) in POSES.items():
            for label, (size, s) in CONFIGS.items():
                cam = mesh.view_camera(eye, at, up, fov, size, near)
                fine_size = (s * size[0], s * size[1])
                kw = dict(want_face_idx=False, want_depth=False)
                calls = {"fused": lambda: ops.mesh_view(mesh, tex, cam, samples=s, **kw)[0],
                         "fine_frame_alone": lambda: ops.mesh_view(mesh, tex, cam, size=fine_size, **kw)[0],
                         "fine_frame_plus_resolve": lambda: resolve(ops.mesh_view(mesh, tex, cam, size=fine_size, **kw)[0], s)}
                fused, resolved = calls["fused"](), calls["fine_frame_plus_resolve"]()
                _, _, _, coverage = ops.mesh_view(mesh, tex, cam, samples=s, want_coverage=True)
                torch.cuda.synchronize()
                row = dict(faces=int(data[1].shape[0]), sha256=hashlib.sha256(fused.cpu().numpy().tobytes()).hexdigest()[:16],
                           fused_equals_resolved=bool(torch.equal(fused, resolved)),
                           partly_covered_pixels=int(((coverage > 0) & (coverage < s * s)).sum()), covered_pixels=int((coverage > 0).sum()))
                times = {arm: [] for arm in ARMS}
                for _ in range(repeats):  # one repeat of every arm in turn
                    for arm in ARMS:
                        times[arm] += device_ms(calls[arm], 1, blocker)
                for arm in ARMS:
                    row[arm] = med(times[arm])
                row["fused_over_fine_frame_alone"] = round(row["fused"]["median"] / row["fine_frame_alone"]["median"], 3)
                row["fused_over_fine_frame_plus_resolve"] = round(row["fused"]["median"] / row["fine_frame_plus_resolve"]["median"], 3)
                rows[f"{pose}_{label}"] = row
                print(f"[aa timing] {name} {pose} {label}: {row['fused']['median']} ms fused", file=sys.stderr, flush=True)
        mesh.close()
        out[name] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the comparison of the unchanged paths")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library, alternating")
    ap.add_argument("--stroke", action="store_true", help="with --parent-lib: also the 16-stamp stroke's sha256, once per library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    out = dict(texture=a.texture, repeats=a.repeats)
    if a.parent_lib:  # first, each in a process of its own: this process has not opened the GPU yet
        cmd = [sys.executable, os.path.join(here, "mesh_view_clip_timing.py"), "--child", "--texture", str(a.texture), "--repeats", str(a.repeats)]
        ab = dict(parent=[], this_build=[])
        for _ in range(a.processes):
            for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", "")):
                ab[arm].append(run_child(cmd, lib)["frames"])
                print(f"[aa timing] unfiltered frames, {arm}: done", file=sys.stderr, flush=True)
        rows = {}
        for mesh in ab["parent"][0]:
            for frame in ab["parent"][0][mesh]:
                meds = {arm: [p[mesh][frame]["clip_off"]["median"] for p in v] for arm, v in ab.items()}
                spread = max(p[mesh][frame]["clip_off"]["max"] - p[mesh][frame]["clip_off"]["min"] for v in ab.values() for p in v)
                spread = max([spread] + [max(v) - min(v) for v in meds.values()])
                diff = statistics.median(meds["this_build"]) - statistics.median(meds["parent"])
                shas = {p[mesh][frame]["sha256"]["clip_off"] for v in ab.values() for p in v}
                rows[f"{mesh}_{frame}"] = dict(parent_ms=meds["parent"], this_build_ms=meds["this_build"], difference_ms=round(diff, 4),
                                               spread_ms=round(spread, 4), within_the_spread=abs(diff) <= spread, sha256=sorted(shas),
                                               frames_byte_identical=len(shas) == 1)
        out["unfiltered_frames_against_the_parent_build"] = dict(processes_per_library=a.processes, frames=rows)
        if a.stroke:
            cmd = [sys.executable, os.path.join(here, "mesh_pick_timing.py"), "--child", "--res", "512", "--texture", "2048", "--ddim-steps", "20",
                   "--repeats", "1", "--grid", "225"]
            strokes = {arm: run_child(cmd, lib) for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", ""))}
            out["stroke_16_stamps"] = dict(strokes, texture_byte_identical=strokes["parent"]["sha256"] == strokes["this_build"]["sha256"])
    m, tex = setup(a.texture)
    out["anti_aliased_frames"] = aa_frames(m, tex, a.repeats)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
