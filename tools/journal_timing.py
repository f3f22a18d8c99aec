#!/usr/bin/env python3
"""What the undo / redo journal of a texture costs: the 16-stamp 512^2 / 20-step stroke of tools/mesh_stroke_timing.py on
the 2048^2 atlas of the height field refined to about 100 k faces, `paint_mesh_stroke(bleed=4)` with a record open against the same
call with none, in one process, alternating, warmed up, medians: wall time from the call to the end of the device work.  Then undo and
redo of that record (wall time, they wait for the stream) against the honest alternative a client has without a journal: a device-to-
device clone of the whole texture before the stroke and a copy back on undo.  And the save and swap launches alone between events.

--parent-lib PATH: a libdtp.so built from the parent commit.  The unjournalled arm then runs once more in a fresh child process bound to
that library ($DTP_LIB), before this process touches the GPU; the child's texture must be byte-identical to this build's and its
per-stroke time is recorded next to it.  Prints one JSON line; --out writes it to a file as well."""
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

    def stroke(tex):
        return m.paint_mesh_stroke(mesh, tex, positions, normals, prevs, 0.25, seeds=list(range(500, 516)), bleed=a.bleed, **st)
    return m, tex0, stroke


def digest(tex):
    return hashlib.sha256(tex.cpu().numpy().tobytes()).hexdigest()


def summary(ms, per=16):
    med = statistics.median(ms)
    return dict(wall_ms=[round(v, 2) for v in ms], median_wall_ms=round(med, 2), per_stamp_ms=round(med / per, 3),
                spread_ms=round(max(ms) - min(ms), 2))


def note(msg):
    sys.stderr.write(f"[journal_timing] {msg}\n")
    sys.stderr.flush()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def child(a):
    _, tex0, stroke = setup(a)
    tex = tex0.clone()
    stroke(tex)
    ms = []
    for _ in range(a.repeats):
        tex.copy_(tex0)
        ms.append(wall(lambda: stroke(tex)))
    print(json.dumps(dict(lib=os.path.basename(os.environ.get("DTP_LIB", "")), sha256=digest(tex), **summary(ms))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--bleed", type=int, default=4)
    ap.add_argument("--parent-lib", default=None, help="a libdtp.so of the parent commit for the unjournalled comparison")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(res=a.res, texture=a.texture, stamps=16, ddim_steps=a.ddim_steps, repeats=a.repeats, bleed=a.bleed)
    parent = None
    if a.parent_lib:  # first, and in a process of its own: this one has not opened the GPU yet
        note(f"the unjournalled stroke with {a.parent_lib} in a child process")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--res", str(a.res), "--texture", str(a.texture), "--ddim-steps",
               str(a.ddim_steps), "--repeats", str(a.repeats), "--grid", str(a.grid), "--bleed", str(a.bleed)]
        r = subprocess.run(cmd, env={**os.environ, "DTP_LIB": os.path.abspath(a.parent_lib)}, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"the parent-library run failed with status {r.returncode}")
        parent = json.loads(r.stdout.strip().splitlines()[-1])

    note("this build: setup")
    m, tex0, stroke = setup(a)
    note("warm-up and the alternating arms")
    T = a.texture
    tex = tex0.clone()
    j = m.journal(tex, depth=2)
    out["journal"] = dict(capacity_tiles=j.capacity_tiles, slots_MiB=round(j.capacity_tiles / 1024, 1), tiles_of_the_texture=(T // 16) ** 2)

    def journalled():
        with j.stroke():
            stroke(tex)

    for arm in (lambda: stroke(tex), journalled):  # build, capture, warm (and the coverage mask)
        tex.copy_(tex0)
        arm()
    ms = dict(plain=[], journalled=[])
    plain_digest = None
    for _ in range(a.repeats):  # alternating arms
        tex.copy_(tex0)
        ms["plain"].append(wall(lambda: stroke(tex)))
        if plain_digest is None:
            plain_digest = digest(tex)
        tex.copy_(tex0)
        ms["journalled"].append(wall(journalled))
    out["plain"], out["journalled"] = summary(ms["plain"]), summary(ms["journalled"])
    diff = (out["journalled"]["median_wall_ms"] - out["plain"]["median_wall_ms"]) / 16
    out["per_stamp_difference_ms"] = round(diff, 4)
    out["per_stamp_difference_percent_of_a_stamp"] = round(100 * diff / out["plain"]["per_stamp_ms"], 3)
    out["journalled_texture_byte_identical_to_plain"] = digest(tex) == plain_digest
    info = j.info()
    rec = j.record(info["records"] - 1)
    n = rec["end"] - rec["start"]
    out["record"] = dict(tiles=n, percent_of_the_texture=round(100 * n / (T // 16) ** 2, 2), KiB=n, restorable=rec["restorable"])

    note("undo and redo against clone and copy back")
    # undo and redo of that record against clone-before + copy-back
    painted = tex.clone()
    undo_ms, redo_ms, clone_ms, back_ms = [], [], [], []
    for i in range(a.repeats + 1):  # (the first round warms up)
        u = wall(j.undo)
        ok = torch.equal(tex, tex0)
        r = wall(j.redo)
        ok = ok and torch.equal(tex, painted)
        keep = []
        c = wall(lambda: keep.append(tex.clone()))
        b = wall(lambda: tex.copy_(keep[0]))
        if i:
            undo_ms.append(u); redo_ms.append(r); clone_ms.append(c); back_ms.append(b)
        out["undo_and_redo_exact"] = ok and out.get("undo_and_redo_exact", True)
    out["undo_wall_ms"], out["redo_wall_ms"] = summary(undo_ms, 1), summary(redo_ms, 1)
    out["alternative_clone_before_the_stroke_wall_ms"], out["alternative_copy_back_on_undo_wall_ms"] = summary(clone_ms, 1), summary(back_ms, 1)

    # the launches alone, between events on the model's stream: the save of the record's bounding rectangles and the swap
    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(m.stream):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    side = 512 + 2 * a.bleed  # about one stamp's texel box: under 3 % of the texture
    save, swap, box_tiles = [], [], 0
    for i in range(a.repeats + 1):
        j.begin()
        s = events(lambda: j.touch([(700, 700, 700 + side - 1, 700 + side - 1)]))
        j.end()
        rec = j.record(j.info()["records"] - 1)
        box_tiles = rec["end"] - rec["start"]
        w = events(j.undo)
        if i:
            save.append(s); swap.append(w)
    out["launches_alone"] = dict(tiles_of_one_stamp_box=box_tiles, save_ms=summary(save, 1), undo_ms_with_its_wait_for_the_counters=summary(swap, 1))
    if parent is not None:
        out["plain_against_the_parent_build"] = dict(
            parent=parent, this_build_sha256=plain_digest, texture_byte_identical=parent["sha256"] == plain_digest,
            median_difference_ms_per_stroke=round(out["plain"]["median_wall_ms"] - parent["median_wall_ms"], 2),
            within_the_spread_of_the_repeats=abs(out["plain"]["median_wall_ms"] - parent["median_wall_ms"])
            <= max(out["plain"]["spread_ms"], parent["spread_ms"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
