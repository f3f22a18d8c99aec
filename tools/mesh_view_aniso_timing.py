#!/usr/bin/env python3
"""What the anisotropic view costs, by the method of tools/mesh_view_timing.py: one MI355X, one process, warmed up,
five repeats, medians with their spread, the device time between events with the launches enqueued behind a blocker.
  - the 100 352-face height field at the far and the near pose of the 3.24 table and a two-face floor running away from the eye (the
    floor of tests/view_aniso_ref.py), all at 1280 x 720: `anisotropy` 1 (the trilinear frame through dtp_mesh_view_mips /
    dtp_mesh_view_aa, as before), 2, 4, 8 and 16, each with samples 1 and 2, the arms alternating within a row; with each row the
    number of taps the frame took (mean, largest) and the frame's sha256;
  - with --parent-lib: the frames of the same poses that both builds draw -- bilinear, trilinear and anisotropy 16, each with clip_near
    off and on and with samples 1 and 2 -- in fresh child processes bound in turn to a libdtp.so of the parent commit ($DTP_LIB) and to
    this build's, alternating, before this process touches the GPU: one sha256 per frame, the medians against the spread;
  - with --stroke as well: the 16-stamp bleed = 0 stroke of tools/mesh_pick_timing.py --child once per library: its texture's sha256.
Prints one JSON line; --out writes it to a file as well (profiles/mesh_view_aniso_timing.json; no other tool's file)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_view_clip_timing import device_ms, run_child, setup  # noqa: E402
from mesh_view_timing import POSES, med  # noqa: E402

SIZE = (720, 1280)
FLOOR_POSE = ((0, 0.25, 1), (0, 0, -3), (0, 1, 0), 45.0, 0.05)  # eye, at, up, fov_y, near
LEVELS = (1, 2, 4, 8, 16)
SAMPLES = (1, 2)


def floor():
    v = torch.tensor([(-2, 0, -20), (2, 0, -20), (2, 0, 0), (-2, 0, 0)], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    uv = torch.tensor([[(0, 1), (1, 1), (1, 0)], [(0, 1), (1, 0), (0, 0)]], dtype=torch.float32)
    return v, f, uv


def scenes():
    from diffusiontexturepainting_amd import synthetic
    field = synthetic.make_height_field(225, 225, seed=3)
    return (("height_field_225_far", field, POSES["far"]), ("height_field_225_near", field, POSES["near"]), ("floor_2_faces_grazing", floor(), FLOOR_POSE))


def sha(image):
    return hashlib.sha256(image.cpu().numpy().tobytes()).hexdigest()[:16]


def aniso_frames(m, tex, repeats):
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    mips = m.build_mips(tex)
    out = {}
    for name, data, (eye, at, up, fov, near) in scenes():
        mesh = m.load_mesh(*data)
        cam = mesh.view_camera(eye, at, up, fov, SIZE, near)
        for s in SAMPLES:
            def call(M):
                kw = dict(anisotropy=M) if M > 1 else {}
                return m.render_view(mesh, tex, cam, filter="trilinear", mips=mips, samples=s, **kw)
            row = dict(faces=int(data[1].shape[0]))
            _, face_idx = m.render_view(mesh, tex, cam, filter="trilinear", mips=mips, samples=s, want_face_idx=True)
            row["covered_pixels"] = int((face_idx >= 0).sum())
            for M in LEVELS:
                arm = dict(sha256=sha(call(M)))
                if M > 1:
                    _, taps = m.render_view(mesh, tex, cam, filter="trilinear", mips=mips, samples=s, anisotropy=M, want_taps=True)
                    hit = taps[taps > 0].float()
                    arm.update(mean_taps=round(float(hit.mean()), 3) if hit.numel() else 0.0, most_taps=int(taps.max()))
                row[f"anisotropy_{M}"] = arm
            times = {M: [] for M in LEVELS}
            for _ in range(repeats):  # one repeat of every arm in turn
                for M in LEVELS:
                    times[M] += device_ms(lambda: call(M), 1, blocker)
            for M in LEVELS:
                row[f"anisotropy_{M}"].update(med(times[M]))
                row[f"anisotropy_{M}"]["over_trilinear"] = round(statistics.median(times[M]) / statistics.median(times[1]), 3)
            out[f"{name}_samples_{s}"] = row
            print(f"[aniso timing] {name} samples {s}: " + ", ".join(f"{M}: {row[f'anisotropy_{M}']['median']} ms" for M in LEVELS), file=sys.stderr,
                  flush=True)
        mesh.close()
    return out


def old_frames(m, tex, repeats):
    """The paths both builds have: every scene with each filter (bilinear, trilinear, anisotropy 16), clip_near off and on, samples 1 and 2
    -> {scene_filter_clip_samples: median, min, max, sha256}."""
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device="cuda:0")
    mips = m.build_mips(tex)
    filters = (("bilinear", {}), ("trilinear", dict(filter="trilinear", mips=mips)), ("anisotropy_16", dict(filter="trilinear", mips=mips, anisotropy=16)))
    out = {}
    for name, data, (eye, at, up, fov, near) in scenes():
        mesh = m.load_mesh(*data)
        cam = mesh.view_camera(eye, at, up, fov, SIZE, near)
        calls = {f"{filt}_clip_{'on' if clip else 'off'}_samples_{s}": (lambda kw=kw, clip=clip, s=s: m.render_view(mesh, tex, cam, clip_near=clip, samples=s, **kw))
                 for filt, kw in filters for clip in (False, True) for s in SAMPLES}
        times = {k: [] for k in calls}
        for _ in range(repeats):
            for k, call in calls.items():
                times[k] += device_ms(call, 1, blocker)
        for k, call in calls.items():
            out[f"{name}_{k}"] = dict(med(times[k]), sha256=sha(call()))
        mesh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the comparison of the unchanged paths")
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library, alternating")
    ap.add_argument("--stroke", action="store_true", help="with --parent-lib: also the 16-stamp stroke's sha256, once per library")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        m, tex = setup(a.texture)
        print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), frames=old_frames(m, tex, a.repeats))))
        return
    out = dict(texture=a.texture, repeats=a.repeats, size=list(SIZE))
    if a.parent_lib:  # first, each in a process of its own: this process has not opened the GPU yet
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--texture", str(a.texture), "--repeats", str(a.repeats)]
        ab = dict(parent=[], this_build=[])
        for _ in range(a.processes):
            for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", "")):
                ab[arm].append(run_child(cmd, lib)["frames"])
                print(f"[aniso timing] unchanged frames, {arm}: done", file=sys.stderr, flush=True)
        rows = {}
        for frame in ab["parent"][0]:
            meds = {arm: [p[frame]["median"] for p in v] for arm, v in ab.items()}
            spread = max(p[frame]["max"] - p[frame]["min"] for v in ab.values() for p in v)
            spread = max([spread] + [max(v) - min(v) for v in meds.values()])
            diff = statistics.median(meds["this_build"]) - statistics.median(meds["parent"])
            shas = {p[frame]["sha256"] for v in ab.values() for p in v}
            rows[frame] = dict(parent_ms=meds["parent"], this_build_ms=meds["this_build"], difference_ms=round(diff, 4), spread_ms=round(spread, 4),
                               within_the_spread=abs(diff) <= spread, sha256=sorted(shas), frames_byte_identical=len(shas) == 1)
        out["unchanged_frames_against_the_parent_build"] = dict(processes_per_library=a.processes, frames=rows)
        if a.stroke:
            cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_pick_timing.py"), "--child", "--res", "512", "--texture", "2048",
                   "--ddim-steps", "20", "--repeats", "1", "--grid", "225"]
            strokes = {arm: run_child(cmd, lib) for arm, lib in (("parent", os.path.abspath(a.parent_lib)), ("this_build", ""))}
            out["stroke_16_stamps"] = dict(strokes, texture_byte_identical=strokes["parent"]["sha256"] == strokes["this_build"]["sha256"])
    m, tex = setup(a.texture)
    out["anisotropic_frames"] = aniso_frames(m, tex, a.repeats)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
