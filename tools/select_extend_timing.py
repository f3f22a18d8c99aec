#!/usr/bin/env python3
"""What growing a face set costs, on the GPU, in one process, on the height field refined to 100 352 faces:
1. the host time of the first dtp_mesh_topology of a mesh (copy back, dtp_topology_build, allocate, upload), from the call to its return,
   on --builds fresh meshes, and of the host-only dtp_topology_build alone on the same data;
2. the device time of `extend_selection` -- rings=1, rings=8, shrink=1, linked, charts -- from a lasso-sized seed set (what the 1024-vertex
   lasso of tools/select_timing.py selects in a 1280 x 720 frame) and from the full set, the contention case of the mark kernel: between
   device events on the view's stream with the launches enqueued behind a blocker (a few milliseconds of queued matrix products, so that
   the interval holds the device's work and not the host's enqueue), warmed up, median and spread of --repeats calls; beside them the
   lasso itself, for scale;
3. with --parent-lib PATH (a libdtp.so built from the parent commit): the 16-stamp `bleed=0` 512^2 stroke of tools/mesh_pick_timing.py
   in fresh child processes, bound in turn to that library ($DTP_LIB) and to this build's, before this process touches the GPU: the two
   textures must have one sha256.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def stroke_digests(parent_lib):
    """{library: the JSON line of tools/mesh_pick_timing.py --child}: one fresh process per library."""
    out = {}
    for name, lib in (("parent", parent_lib), ("this_build", None)):
        env = dict(os.environ)
        env.pop("DTP_LIB", None)
        if lib:
            env["DTP_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.join(HERE, "mesh_pick_timing.py"), "--child", "--repeats", "1"], env=env, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"the stroke under the {name} library failed:\n{r.stdout}\n{r.stderr}")
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=225, help="vertices per side of the height field (225: 100 352 faces)")
    ap.add_argument("--frame", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(grid=a.grid, frame=list(a.frame), repeats=a.repeats)
    if a.parent_lib:
        strokes = stroke_digests(a.parent_lib)
        out["stroke_16_stamps"] = dict(strokes, texture_byte_identical=strokes["parent"]["sha256"] == strokes["this_build"]["sha256"])
    if not torch.cuda.is_available():
        raise SystemExit("select_extend_timing.py measures on the GPU: no device found")
    from diffusiontexturepainting_amd import mesh as M, synthetic, weights as W
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    from diffusiontexturepainting_amd.mesh import view_camera
    dev = torch.device("cuda", 0)
    R = 64  # (no stamp is made: the smallest context)
    sd = dict(unet=W.synthetic_unet(5), lora=W.synthetic_lora(5), vae=W.synthetic_vae(5), clip=W.synthetic_clip(5), penc=W.synthetic_patch_encoder(5))
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    verts, faces, uvs = synthetic.make_height_field(a.grid, a.grid, seed=3)
    F = int(faces.shape[0])
    out["faces"] = F

    # ---- 1. the first use of a mesh
    import ctypes as C
    from diffusiontexturepainting_amd import _lib
    lib = _lib.load()
    first, again, labels, host = [], [], [], []
    for _ in range(a.builds):
        fresh = m.load_mesh(verts, faces, uvs)
        torch.cuda.synchronize()
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for ms in (first, again):  # the first call builds; the second only returns the counts
            t0 = time.perf_counter()
            _lib.check(lib.dtp_mesh_topology(fresh.handle, None, s), "dtp_mesh_topology")
            ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        topo = fresh.topology()  # (the copy of the labels to the host)
        labels.append((time.perf_counter() - t0) * 1e3)
        fresh.close()
        t0 = time.perf_counter()
        M.topology_build(verts, faces, uvs)
        host.append((time.perf_counter() - t0) * 1e3)
    out["first_use"] = dict(first_dtp_mesh_topology_wall_ms=[round(v, 2) for v in first], median_ms=round(statistics.median(first), 2),
                            later_call_median_ms=round(statistics.median(again), 4), labels_to_host_median_ms=round(statistics.median(labels), 2),
                            host_build_alone_ms=[round(v, 2) for v in host], host_build_alone_median_ms=round(statistics.median(host), 2),
                            points=topo["num_points"], parts=topo["num_parts"], charts=topo["num_charts"])

    # ---- 2. the extends
    mesh = m.load_mesh(verts, faces, uvs)
    H, Wf = a.frame
    cam = view_camera((0.3, -0.5, 2.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, (H, Wf), 0.05)
    tex = torch.zeros(256, 256, 4, dtype=torch.uint8, device=dev)
    _, face_idx = m.render_view(mesh, tex, cam, want_face_idx=True)
    circle = [((0.5 + 0.33 * math.cos(2 * math.pi * k / 1024)) * Wf, (0.5 + 0.45 * math.sin(2 * math.pi * k / 1024)) * H) for k in range(1024)]
    seed = m.select_faces(mesh, face_idx, circle)
    full = ~M.faceset_empty(F, dev)
    dst = M.faceset_empty(F, dev)
    m.extend_selection(mesh, seed, out=dst)  # the first use: builds the topology
    vs = m.view_stream
    blocker = torch.randn(4096, 4096, dtype=torch.float16, device=dev)
    cur = torch.cuda.current_stream(dev)

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(4):  # a few milliseconds of queued work: the call's launches are all enqueued before the first one starts
                blocker @ blocker
            vs.wait_stream(cur)
            ev[0].record(vs)
            fn()
            ev[1].record(vs)
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    rows = {}
    for label, src in (("lasso_seed", seed), ("full_set", full)):
        rows[label] = dict(faces_in=int(M.faceset_to_bool(src, F).sum()))
        for name, how, rings in (("rings_1", "rings", 1), ("rings_8", "rings", 8), ("shrink_1", "shrink", 1), ("linked", "linked", 1),
                                 ("charts", "charts", 1)):
            rows[label][name] = timed(lambda: m.extend_selection(mesh, src, how=how, rings=rings, out=dst), a.repeats)
            rows[label][name]["faces_out"] = int(M.faceset_to_bool(dst, F).sum())
    out["extend"] = rows
    out["lasso_polygon_1024"] = timed(lambda: m.select_faces(mesh, face_idx, circle, out=dst), a.repeats)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
