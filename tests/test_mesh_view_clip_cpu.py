"""The near-plane clip of the view of a textured mesh (include/dtp.h "a view clipped at the near plane": dtp_mesh_view_clip,
dtp_op_mesh_view_clip) without a GPU: the numpy restatement (tests/view_clip_ref.py) on scenes whose answer is known -- a floor under the
eye, a room seen from inside, a shared edge through pixel centres, a face slid across the plane, faces whose plane contains the eye --
and against the pick of the pixels' rays; the argument checks that come before any device call; the header against the binding; and the
stand-alone host program tools/view_clip_host_check.cpp."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mip_ref
import pick_ref
import view_clip_ref as vc
import view_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
f32 = np.float32
WHITE = np.full((4, 4, 4), 255, dtype=np.uint8)


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def ref_camera(pose, size):
    eye, at, up, fov, near = pose
    return view_ref.camera(eye, at, up, fov, size, near)


def hand_cam(size, near=0.5):
    """The camera at the origin looking down -z with fx = fy = 1: camera space is world space, the ray of a pixel is (ndc_x, ndc_y, -1)."""
    return dict(m=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=f32), fx=f32(1), fy=f32(1), near=f32(near), size=size)


def assert_pick_agrees(mesh, cam, out, what):
    """For every covered pixel whose 3 x 3 neighbourhood shows one face, the ray of view_rays through its centre hits that face, at the
    frame's depth and UV (the margins of test_mesh_view_cpu.py); at least a quarter of the covered pixels qualify."""
    v, f, uv = mesh
    H, W = out["face_idx"].shape
    fi = out["face_idx"]
    covered = fi >= 0
    same = np.zeros((H, W), dtype=bool)
    inner = np.ones((H - 2, W - 2), dtype=bool)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            inner &= fi[di:H - 2 + di, dj:W - 2 + dj] == fi[1:-1, 1:-1]
    same[1:-1, 1:-1] = inner & covered[1:-1, 1:-1]
    assert same.sum() >= 0.25 * covered.sum() > 0, (what, covered.sum(), same.sum())
    ii, jj = np.nonzero(same)
    o, d = view_ref.rays(cam, np.stack([jj + 0.5, ii + 0.5], axis=1))
    hits = pick_ref.pick(v, f, uv, o, d)
    wrong = np.nonzero(hits["face"] != fi[ii, jj])[0]
    assert wrong.size == 0, (what, [(int(ii[k]), int(jj[k]), int(fi[ii[k], jj[k]]), int(hits["face"][k])) for k in wrong[:8]])
    b = cam["m"][2, :3].astype(np.float64)
    dist = -(hits["pos"].astype(np.float64) - o.astype(np.float64)) @ b
    assert np.allclose(dist, out["depth"][ii, jj], rtol=1e-4) and np.allclose(hits["uv"], out["uv"][ii, jj], atol=1e-4), what
    return int(same.sum())


# ---------------------------------------------------------------- the scenes of the issue
def test_floor_under_the_eye_is_drawn_below_the_horizon_and_agrees_with_the_pick():
    mesh = vc.floor_mesh()
    cam = ref_camera(vc.FLOOR_POSE, (36, 64))
    off = vc.view(*mesh, WHITE, cam, clip_near=False)
    plain = view_ref.view(*mesh, WHITE, cam)
    assert (off["face_idx"] == -1).all() and all(np.array_equal(off[k], plain[k]) for k in ("image", "face_idx", "depth"))
    on = vc.view(*mesh, WHITE, cam)
    covered = on["face_idx"] >= 0
    # the eye is 1 above the floor and looks down by atan(0.5 / 3): the horizon lies above the frame's middle, the floor's far edge
    # (10 away) under it; every row from there down is floor from side to side
    rows = covered.any(axis=1)
    first = int(np.argmax(rows))
    assert covered.sum() == 1344 and first == 15 and covered[first:].all() and not covered[:first].any()
    assert on["crossing"].sum() == 1344 and on["cr"]["drawn"].all() and (on["depth"][covered] >= cam["near"]).all()
    assert (on["depth"][~covered] == 0).all() and np.isfinite(on["depth"]).all() and np.isfinite(on["uv"][covered]).all()
    # every covered pixel's ray hits the floor, edges included: the view and the pick agree on the face
    ii, jj = np.nonzero(covered)
    o, d = view_ref.rays(cam, np.stack([jj + 0.5, ii + 0.5], axis=1))
    hits = pick_ref.pick(*mesh, o, d)
    assert np.array_equal(hits["face"], on["face_idx"][ii, jj])
    assert assert_pick_agrees(mesh, cam, on, "floor") > 1000


def test_unit_cube_from_inside_covers_every_pixel_and_agrees_with_the_pick():
    mesh = vc.cube_mesh()
    cam = ref_camera(vc.CUBE_INSIDE, (36, 64))
    off = view_ref.view(*mesh, WHITE, cam)
    on = vc.view(*mesh, WHITE, cam)
    assert (on["face_idx"] >= 0).all() and 0 < (off["face_idx"] >= 0).sum() < 36 * 64
    assert on["crossing"].sum() > 500 and (on["depth"] >= cam["near"]).all()
    keep = off["face_idx"] >= 0   # what the unclipped frame shows, the clipped one shows too (a convex room: one face per ray)
    assert np.array_equal(on["face_idx"][keep], off["face_idx"][keep]) and np.array_equal(on["depth"][keep], off["depth"][keep])
    assert_pick_agrees(mesh, cam, on, "cube")
    culled = vc.view(*mesh, WHITE, cam, cull=True)  # from inside every wall is a back face
    assert (culled["face_idx"] == -1).all()
    flipped = vc.view(*mesh, WHITE, cam, cull=True, flip_normals=True)
    assert np.array_equal(flipped["face_idx"], on["face_idx"])


def test_crossing_faces_are_watertight_along_a_shared_edge_through_pixel_centres():
    """A diamond in the plane y = -1 whose diagonal runs along z at x = y = -1, from in front of the eye to behind it: the diagonal's image
    is the line ndc_x = ndc_y, which passes through the centres (i, 7 - i) of an 8 x 8 frame.  Everything is dyadic, so those centres
    lie EXACTLY on the edge both faces share: each face alone covers them (edges are inclusive), and together no pixel of the diamond's
    image is background."""
    v = np.array([(-1, -1, -4), (3, -1, 0), (-1, -1, 4), (-5, -1, 0)], dtype=f32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    uv = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], dtype=f32)
    cam = hand_cam((8, 8), near=0.125)
    both = vc.view(v, f, uv, WHITE, cam, background=(9, 9, 9, 9))
    shared = both["cr"]["n"][0, 1], both["cr"]["n"][1, 2]  # the edge 0-2 lies opposite vertex 1 of face 0 and vertex 2 of face 1
    assert both["cr"]["drawn"].all() and np.array_equal(shared[0], -shared[1]) and sorted(np.abs(shared[0]).tolist()) == [0, 8, 8]
    # the diamond's image, in double: the ray (gx, gy, -1) meets y = -1 at t = -1 / gy (below the horizon), inside |x + 1| + |z| <= 4
    ndc = (2 * np.arange(8) + 1) / 8 - 1
    gx, gy = np.meshgrid(ndc, -ndc)
    t = np.where(gy < 0, -1 / np.where(gy < 0, gy, 1), np.inf)
    inside = (gy < 0) & (np.abs(gx * t + 1) + np.abs(-t) <= 4) & (t >= 0.125)
    on_edge = [(7 - j, j) for j in range(8) if ndc[j] <= -0.25]
    assert on_edge == [(7, 0), (6, 1), (5, 2)] and all(inside[p] for p in on_edge) and inside.sum() > 10
    assert (both["face_idx"][inside] >= 0).all() and (both["image"][inside] != 9).any(axis=-1).all()
    assert (both["face_idx"][~inside] == -1).all()
    for p in on_edge:
        assert both["face_idx"][p] == 0  # equal depth on the shared edge or not, a face covers it; the lower index wins a tie
    for face in (0, 1):
        alone = vc.view(v, f[face:face + 1], uv[face:face + 1], WHITE, cam)
        assert all(alone["face_idx"][p] == 0 for p in on_edge), face


@pytest.mark.parametrize("winding", ["ccw", "cw"])
def test_a_face_slid_across_the_near_plane_keeps_its_facing(winding):
    """Slid along the view axis the face goes from wholly in front to crossing at shift > -0.5; its plane passes through the eye at
    shift = 1.36 / 1.49 = 0.913, and only there may the facing change: before it the snapped area's sign (in front) and D's sign
    (crossing) name the same side, after it the eye sees the other side."""
    tri = np.array([(-0.6, -0.4, 0.0), (0.7, -0.3, -1.0), (0.1, 0.8, -2.0)], dtype=f32)
    f = np.array([[0, 1, 2] if winding == "ccw" else [0, 2, 1]], dtype=np.int32)
    uv = np.zeros((1, 3, 2), dtype=f32)
    cam = hand_cam((32, 32), near=0.5)
    shifts = (-8.0, -2.0, -0.75, -0.5, -0.25, 0.25, 0.75, 1.0)  # the nearest vertex at z = shift, the farthest at shift - 2
    for flip in (False, True):
        fronts = []
        for shift in shifts:
            v = tri + np.array([0, 0, shift], dtype=f32)
            proj = view_ref.project(v, f, cam, 32, 32, False, flip)
            cr = vc.project_crossing(v, f, cam, False, flip)
            in_front, behind, crossing = vc.classify(cr["c"], cam["near"])
            assert in_front[0] == (shift <= -0.5) and crossing[0] == (shift > -0.5) and not behind[0]
            assert in_front[0] == bool(proj["drawn"][0]) and crossing[0] == bool(cr["drawn"][0])
            fronts.append(bool(proj["front"][0]) if in_front[0] else bool(cr["front"][0]))
            for cull in (False, True):
                out = vc.view(v, f, uv, WHITE, cam, cull=cull, flip_normals=flip)
                shown = (out["face_idx"] >= 0).any()
                assert shown == (fronts[-1] or not cull), (winding, flip, shift, cull)
        side = (winding == "ccw") != flip  # A < 0 <=> D < 0: one rule on both sides of the near plane
        assert fronts == [side] * 7 + [not side], (winding, flip, fronts)


def test_degenerate_faces():
    cam = hand_cam((16, 16), near=0.5)
    uv = np.zeros((1, 3, 2), dtype=f32)
    one = np.array([[0, 1, 2]], dtype=np.int32)
    # a face whose plane contains the eye: D == 0, not drawn, nothing non-finite anywhere
    v = np.array([(1, 0, -2), (-1, 0, -2), (0, 0, 1)], dtype=f32)
    out = vc.view(v, one, uv, WHITE, cam, background=(1, 2, 3, 4))
    assert out["cr"]["crossing"][0] and out["cr"]["D"][0] == 0 and not out["cr"]["drawn"][0]
    assert (out["face_idx"] == -1).all() and (out["depth"] == 0).all() and (out["image"] == np.array([1, 2, 3, 4], dtype=np.uint8)).all()
    tri = vc.view(v, one, uv, mip_ref.texture("square")[0], cam, filter="trilinear")
    assert (tri["face_idx"] == -1).all() and (tri["lod"] == 0).all()
    # a vertex exactly on the near plane is in front: with the other two in front the face is view_ref's, bit for bit
    v = np.array([(-1, -1, -0.5), (1, -1, -2), (0, 1, -3)], dtype=f32)
    in_front, behind, crossing = vc.classify(vc.camera_space(v, one, cam), cam["near"])
    assert in_front[0] and not crossing[0] and not behind[0]
    on, off = vc.view(v, one, uv, WHITE, cam), view_ref.view(v, one, uv, WHITE, cam)
    assert (on["face_idx"] >= 0).any() and all(np.array_equal(on[k], off[k]) for k in ("image", "face_idx", "depth"))
    # with one vertex behind, the vertex on the plane does not make it less of a crossing face
    v[2, 2] = 1.0
    _, _, crossing = vc.classify(vc.camera_space(v, one, cam), cam["near"])
    assert crossing[0]
    out = vc.view(v, one, uv, WHITE, cam)
    assert (out["face_idx"] >= 0).any() and (out["depth"][out["face_idx"] >= 0] >= cam["near"]).all()
    # wholly nearer than the plane, behind the eye, and coordinates that overflow: behind, not drawn
    v[2, 2] = -3.0
    with np.errstate(over="ignore"):
        for verts in (v * f32(0.01), v * f32(-1), v * f32(3e38)):
            c = vc.camera_space(verts, one, cam)
            assert vc.classify(c, cam["near"])[1][0] and (vc.view(verts, one, uv, WHITE, cam)["face_idx"] == -1).all()
    # the mixed scene of the GPU test holds every class, and no output of it is non-finite
    m = vc.mixed_mesh()
    out = vc.view(*m, WHITE, ref_camera(vc.MIXED_POSE, (64, 64)))
    in_front, behind, crossing = vc.classify(out["cr"]["c"], f32(0.25))
    assert in_front.sum() > 100 and behind.sum() > 20 and crossing.sum() > 40 and m[1].shape[0] == 257
    assert out["cr"]["D"][253] == 0 and not out["cr"]["drawn"][253] and in_front[254] and crossing[255]
    assert crossing[256] and not np.isfinite(out["cr"]["D"][256]) and not out["cr"]["drawn"][256]
    assert np.isfinite(out["depth"]).all() and np.isfinite(out["uv"][out["face_idx"] >= 0]).all() and out["crossing"].sum() > 300


@pytest.mark.parametrize("filter", ["bilinear", "trilinear"])
def test_a_scene_without_a_crossing_face_is_the_unclipped_frame(filter):
    from diffusiontexturepainting_amd import synthetic
    mesh = [t.numpy() for t in synthetic.make_height_field(17, 13, seed=3)]
    tex, lv = mip_ref.texture("atlas")
    cam = view_ref.camera((0.9, -1.7, 1.3), (0.05, 0.0, 0.0), (0, 0, 1), 50.0, (68, 100), 0.05)
    on = vc.view(*mesh, tex, cam, filter=filter, levels=lv)
    off = vc.view(*mesh, tex, cam, filter=filter, levels=lv, clip_near=False)
    assert not on["cr"]["crossing"].any() and (on["face_idx"] >= 0).sum() > 1500
    for k in ("image", "face_idx", "depth", "uv") + (("lod",) if filter == "trilinear" else ()):
        assert np.array_equal(on[k], off[k], equal_nan=True), k


def test_trilinear_crossing_floor_takes_the_last_level_at_its_horizon():
    tex, lv = mip_ref.texture("atlas")
    L = len(lv)
    out = vc.view(*vc.RUNWAY, tex, ref_camera(vc.RUNWAY_POSE, (32, 32)), filter="trilinear", levels=lv)
    covered = out["face_idx"] >= 0
    assert out["crossing"].sum() == covered.sum() > 300
    rows = np.nonzero(covered.any(axis=1))[0]
    last = int(rows.max())               # upside down: the strip recedes DOWN the frame, and the row under its last one is the horizon's
    assert last == 15 and (out["level"][last][covered[last]] == L - 1).all() and (out["lod"][last][covered[last]] == L - 1).all()
    assert covered[last].sum() == 32 and (out["level"][rows.min()][covered[rows.min()]] == 0).all()
    assert (out["lod"][~covered] == 0).all() and np.isfinite(out["lod"]).all()
    assert (np.diff(out["level"][rows.min():last + 1, 16]) >= 0).all()  # the level does not fall towards the horizon
    # the right way up no covered pixel has the horizon in its neighbourhood
    up = vc.view(*vc.RUNWAY, tex, ref_camera(vc.RUNWAY_POSE[:2] + ((0, 1, 0),) + vc.RUNWAY_POSE[3:], (32, 32)), filter="trilinear", levels=lv)
    assert (up["level"][up["face_idx"] >= 0] < L - 1).all() and (up["face_idx"] >= 0).sum() == covered.sum()


def test_height_field_from_inside_its_hull():
    """The pose of test_faces_behind_the_camera_and_across_the_near_plane: 26 faces cross the plane.  There they lie under the frame
    (ndc_y about -2.2), so that pose alone gains no pixel, 12929 covered either way; a quarter of a unit lower they reach into it."""
    from diffusiontexturepainting_amd import synthetic
    mesh = [t.numpy() for t in synthetic.make_height_field(17, 13, seed=3)]
    counts = {}
    for name, pose in (("inside", vc.FIELD_INSIDE), ("low", vc.FIELD_LOW)):
        cam = ref_camera(pose, (136, 200))
        on, off = vc.view(*mesh, WHITE, cam), view_ref.view(*mesh, WHITE, cam)
        assert on["cr"]["drawn"].sum() == 26
        keep = off["face_idx"] >= 0
        assert (on["face_idx"][keep] >= 0).all()
        counts[name] = (int((on["face_idx"] >= 0).sum()), int(keep.sum()))
    print(counts)
    assert counts["inside"][0] >= counts["inside"][1] and counts["low"][0] > counts["low"][1] + 1000


# ---------------------------------------------------------------- the argument checks, the header, the host program
@pytest.mark.parametrize("entry", ["dtp_mesh_view_clip", "dtp_op_mesh_view_clip"])
def test_clip_refuses_before_any_device_call(lib, entry):
    """No device here: every one of these returns from the checks.  The handle that is not a mesh is looked up, never followed."""
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    fn = getattr(lib, entry)
    tail = (0, None) if entry == "dtp_op_mesh_view_clip" else (None,)
    cam = view_camera((0.3, -1.7, 2.9), (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 45.0, (360, 640), 0.05).struct()
    opts = view_opts()
    tex = (C.c_uint32 * 16)()
    mips = (C.c_uint32 * 8)()
    img = (C.c_uint32 * 16)(*([0x5a5a5a5a] * 16))
    fidx, dep, lod = (C.c_int * 4)(*([7] * 4)), (C.c_float * 4)(*([7.0] * 4)), (C.c_float * 4)(*([7.0] * 4))
    not_a_mesh = (C.c_int * 64)()
    fake = C.cast(not_a_mesh, C.c_void_p)
    vp = (lambda a, off=0: C.c_void_p(C.addressof(a) + off))

    def refused(word, mesh=fake, texture=vp(tex), TH=4, TW=4, m=vp(mips), c=C.byref(cam), H=2, W=2, o=C.byref(opts), filt=1, image=vp(img),
                f=vp(fidx), d=vp(dep), lo=vp(lod)):
        rc = fn(mesh, texture, TH, TW, m, c, H, W, o, filt, image, f, d, lo, *tail)
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(img) == [0x5a5a5a5a] * 16 and list(fidx) == [7] * 4 and list(dep) == [7.0] * 4 and list(lod) == [7.0] * 4

    refused("NULL", mesh=None)
    refused("NULL", texture=None)
    refused("NULL", c=None)
    refused("NULL", o=None)
    refused("NULL", image=None)
    refused("filter is 0", filt=2)
    refused("filter is 0", filt=-1)
    refused("need filter 1", filt=0)
    refused("need filter 1", filt=0, m=None)
    refused("need filter 1", filt=0, lo=None)
    refused("mips is required", m=None)
    refused("aligned", m=vp(mips, 2))
    refused("aligned", lo=vp(lod, 1))
    for H, W in ((0, 2), (2, 0), (4097, 2), (2, 4097)):
        refused(r"1\.\.4096", H=H, W=W)
    for TH, TW in ((0, 4), (4, 32769)):
        refused(r"1\.\.32768", TH=TH, TW=TW)
    refused("aligned", texture=vp(tex, 1))
    refused("aligned", image=vp(img, 2))
    refused("aligned", f=vp(fidx, 1))
    refused("aligned", d=vp(dep, 3))
    broken = view_camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), 0.1).struct()
    broken.near = 0.0
    refused("near", c=C.byref(broken))
    bad = view_opts()
    bad.cull = 2
    refused("0 or 1", o=C.byref(bad))
    bad = view_opts()
    bad.ambient = 1.5
    refused("ambient", o=C.byref(bad))
    refused("not a live mesh")                                      # every argument in order: the look-up is what refuses
    refused("not a live mesh", f=None, d=None, lo=None)             # (the optional outputs may be absent)
    refused("not a live mesh", filt=0, m=None, lo=None)             # (filter 0 takes no pyramid)
    refused("not a live mesh", TH=1, TW=1, m=None)                  # (a 1 x 1 texture has no pyramid)


def test_header_and_binding_agree_on_the_clip(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3
    assert "a view clipped at the near plane" in hdr
    note = hdr[:hdr.index("#define DTP_ABI_VERSION")]
    assert "dtp_mesh_view_clip" in note and "dtp_op_mesh_view_clip" in note
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mesh_view_clip", "dtp_op_mesh_view_clip"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    args = lambda name: re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")  # noqa: E731
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
        assert len(args(name)) == len(_lib.SYMBOLS[name][1]), name
    assert [a.split()[-1] for a in args("dtp_mesh_view_clip")] == ["mesh", "texture", "TH", "TW", "mips", "cam", "H", "W", "opts", "filter", "image",
                                                                  "face_idx", "depth", "lod", "s"]
    assert [a.split()[-1] for a in args("dtp_op_mesh_view_clip")][-2:] == ["binned", "s"]
    # the structs of a view did not grow: the option arrives through the entry points
    assert C.sizeof(_lib.ViewOpts) == 24 and C.sizeof(_lib.ViewCam) == 60


def test_python_surface_takes_the_keyword():
    import inspect
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    assert inspect.signature(MI355ConditionalInpainter.render_view).parameters["clip_near"].default is False
    assert inspect.signature(ops.mesh_view).parameters["clip_near"].default is False


def test_clip_host_check_program_builds_and_passes(tmp_path):
    """tools/view_clip_host_check.cpp drives view_clip_box (csrc/view_host.h) from its own main().  Here it is built plainly and run; the
    sanitizer run is the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/view_clip_host_check.cpp -o view_clip_host_check && ./view_clip_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "view_clip_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "view_clip_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
