"""The anti-aliased view of a textured mesh (include/dtp.h "an anti-aliased view": dtp_mesh_view_aa, dtp_op_mesh_view_aa) without a GPU:
the header against the binding; the argument checks that come before any device call; the ValueErrors of the Python surface; the
stand-alone host program tools/view_aa_host_check.cpp; and the numpy restatement (tests/view_aa_ref.py) on frames whose answer is known
by hand -- a quad that fills the frame, a quad whose edge lies on a column of pixel centres, a background that enters the average -- and
on the poses of the GPU test, where it has to bite: enough pixels that are partly covered, enough whose samples show different faces."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mip_ref
import view_aa_ref as va
import view_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
f32 = np.float32
ENTRIES = ("dtp_mesh_view_aa", "dtp_op_mesh_view_aa")


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------- the header, the checks, the Python surface, the host program
def test_header_and_binding_agree_on_the_anti_aliased_view(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3
    assert "an anti-aliased view" in hdr
    note = hdr[:hdr.index("#define DTP_ABI_VERSION")]
    assert all(name in note for name in ENTRIES)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared and declared == set(_lib.SYMBOLS)
    args = lambda name: re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")  # noqa: E731
    for name in ENTRIES:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
        assert len(args(name)) == len(_lib.SYMBOLS[name][1]), name
    want = ["mesh", "texture", "TH", "TW", "mips", "cam", "H", "W", "opts", "filter", "clip", "samples", "image", "face_idx", "depth", "lod",
            "coverage"]
    assert [a.split()[-1] for a in args("dtp_mesh_view_aa")] == want + ["s"]
    assert [a.split()[-1] for a in args("dtp_op_mesh_view_aa")] == want + ["binned", "s"]
    assert C.sizeof(_lib.ViewOpts) == 24 and C.sizeof(_lib.ViewCam) == 60  # the structs of a view did not grow
    assert _lib.VIEW_SAMPLES == (1, 2, 4)


@pytest.mark.parametrize("entry", ENTRIES)
def test_aa_refuses_before_any_device_call(lib, entry):
    """No device here: every one of these returns from the checks, and nothing is written.  The handle that is not a mesh is looked up,
    never followed."""
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    fn = getattr(lib, entry)
    tail = (0, None) if entry == "dtp_op_mesh_view_aa" else (None,)
    cam = view_camera((0.3, -1.7, 2.9), (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 45.0, (360, 640), 0.05).struct()
    opts = view_opts()
    tex = (C.c_uint32 * 16)()
    mips = (C.c_uint32 * 8)()
    img = (C.c_uint32 * 16)(*([0x5a5a5a5a] * 16))
    fidx, dep, lod = (C.c_int * 4)(*([7] * 4)), (C.c_float * 4)(*([7.0] * 4)), (C.c_float * 4)(*([7.0] * 4))
    cov = (C.c_uint8 * 8)(*([0x5a] * 8))
    fake = C.cast((C.c_int * 64)(), C.c_void_p)
    vp = (lambda a, off=0: C.c_void_p(C.addressof(a) + off))

    def refused(word, mesh=fake, texture=vp(tex), TH=4, TW=4, m=vp(mips), c=C.byref(cam), H=2, W=2, o=C.byref(opts), filt=1, clip=1, samples=2,
                image=vp(img), f=vp(fidx), d=vp(dep), lo=vp(lod), cv=vp(cov)):
        rc = fn(mesh, texture, TH, TW, m, c, H, W, o, filt, clip, samples, image, f, d, lo, cv, *tail)
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(img) == [0x5a5a5a5a] * 16 and list(fidx) == [7] * 4 and list(dep) == [7.0] * 4 and list(lod) == [7.0] * 4
        assert list(cov) == [0x5a] * 8

    for samples in (0, 3, 8, -1, 16):
        refused("samples is 1, 2 or 4", samples=samples)
    # the fine frame has to fit 4096 a side: 4097 itself is s = 1's, and the first H beyond 4096 / s for the others
    for samples, side in ((1, 4097), (2, 2049), (4, 1025)):
        refused(r"1\.\.4096" if samples == 1 else "must not exceed 4096", samples=samples, H=side)
        refused(r"1\.\.4096" if samples == 1 else "must not exceed 4096", samples=samples, W=side)
    refused("must not exceed 4096", samples=4, H=4096, W=4096)
    refused("clip is 0 or 1", clip=2)
    refused("clip is 0 or 1", clip=-1)
    refused("filter is 0", filt=2)
    refused("need filter 1", filt=0)
    refused("need filter 1", filt=0, m=None)
    refused("need filter 1", filt=0, lo=None)
    refused("mips is required", m=None)
    refused("aligned", m=vp(mips, 2))
    refused("aligned", lo=vp(lod, 1))
    refused("NULL", mesh=None)
    refused("NULL", texture=None)
    refused("NULL", c=None)
    refused("NULL", o=None)
    refused("NULL", image=None)
    for H, W in ((0, 2), (2, 0)):
        refused(r"1\.\.4096", H=H, W=W)
    refused(r"1\.\.32768", TW=32769)
    refused("aligned", image=vp(img, 2))
    refused("aligned", f=vp(fidx, 1))
    bad = view_opts()
    bad.cull = 2
    refused("0 or 1", o=C.byref(bad))
    # every argument in order, at every samples, at the limit, with the optional outputs absent: the look-up is what refuses
    for samples in (1, 2, 4):
        refused("not a live mesh", samples=samples)
        refused("not a live mesh", samples=samples, H=4096 // samples, W=4096 // samples)
        refused("not a live mesh", samples=samples, f=None, d=None, lo=None, cv=None)
        refused("not a live mesh", samples=samples, filt=0, clip=0, m=None, lo=None)
    refused("not a live mesh", cv=vp(cov, 1))  # (coverage is bytes: any address)


def test_python_surface_takes_the_keywords_and_refuses_bad_samples(lib):
    from diffusiontexturepainting_amd import _lib, mesh as _mesh, ops
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    for fn in (MI355ConditionalInpainter.render_view, ops.mesh_view):
        p = inspect.signature(fn).parameters
        assert p["samples"].default == 1 and p["want_coverage"].default is False
    cam = _mesh.view_camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (1080, 1920), 0.05)
    a_mesh = object.__new__(_mesh.Mesh)  # never followed: the checks of samples come before the mesh, the texture and the model are used
    for bad in (0, 3, 8, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="samples"):
            _lib.view_samples_check(bad, 4, 4)
        with pytest.raises(ValueError, match="samples"):
            ops.mesh_view(None, None, cam, samples=bad)
        with pytest.raises(ValueError, match="samples"):
            MI355ConditionalInpainter.render_view(None, a_mesh, None, cam, samples=bad)
    for samples, size in ((4, (1080, 1920)), (2, (2049, 8)), (4, (8, 1025)), (2, (4096, 4096))):
        with pytest.raises(ValueError, match="4096"):
            ops.mesh_view(None, None, cam, size=size, samples=samples)
        with pytest.raises(ValueError, match="4096"):
            MI355ConditionalInpainter.render_view(None, a_mesh, None, cam, size=size, samples=samples)
    assert [_lib.view_samples_check(s, 4096 // s, 4096 // s) for s in (1, 2, 4)] == [1, 2, 4]
    with pytest.raises(ValueError, match="trilinear"):
        ops.mesh_view(None, None, cam, samples=2, want_lod=True)
    for s in (0, 3):
        with pytest.raises(ValueError):
            va.view(None, None, None, None, dict(size=(4, 4)), samples=s)
    with pytest.raises(ValueError):
        va.view(None, None, None, None, dict(size=(1025, 4)), samples=4)


def test_aa_host_check_program_builds_and_passes(tmp_path):
    """tools/view_aa_host_check.cpp drives view_aa_check and view_aa_tile_bin (csrc/view_host.h) from its own main().  Here it is built
    plainly and run; the sanitizer run is the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/view_aa_host_check.cpp -o view_aa_host_check && ./view_aa_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "view_aa_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "view_aa_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- frames known by hand
COLOUR = (200, 100, 50, 255)
LOG2 = {1: 0, 2: 2, 4: 4}


def quad(shift=0.0):
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = (t.numpy() for t in synthetic.make_quad())
    v = v.copy()
    v[:, 0] += f32(shift)
    return v, f, uv


def head_on(size):
    """One unit in front of the plane z = 0 looking down -z with fx = fy = 1: the square [-1, 1]^2 is the frame, exactly, and every
    value on the way is dyadic."""
    return dict(m=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -1]], dtype=f32), fx=f32(1), fy=f32(1), near=f32(0.5), size=size)


def uniform_texture():
    return np.broadcast_to(np.array(COLOUR, dtype=np.uint8), (4, 4, 4)).copy()


@pytest.mark.parametrize("filter", ["bilinear", "trilinear"])
def test_a_uniform_opaque_quad_is_the_same_frame_at_every_samples(filter):
    frames = {s: va.view(*quad(), uniform_texture(), head_on((8, 8)), samples=s, filter=filter, shade=False) for s in va.SAMPLES}
    assert (frames[1]["image"] == np.array(COLOUR, dtype=np.uint8)).all() and (frames[1]["face_idx"] >= 0).all()
    for s in (2, 4):
        assert np.array_equal(frames[s]["image"], frames[1]["image"]) and (frames[s]["coverage"] == s * s).all()
        assert tuple(frames[s]["fine"]["image"].shape) == (8 * s, 8 * s, 4)
    assert (frames[1]["coverage"] == 1).all()


@pytest.mark.parametrize("background", [(0, 0, 0, 0), (10, 20, 30, 40), (255, 255, 255, 255)])
@pytest.mark.parametrize("side", ["left", "right"])
def test_a_half_covered_column_carries_half_the_colour(side, background):
    """W = 8: the centre of pixel column j is at ndc_x = (2 j + 1) / 8 - 1.  Shifted by 0.625 the quad's left edge lies on the centres of
    column 2; shifted by -0.625 its right edge on those of column 5.  With s even no sample lies on the edge: the s / 2 sample columns on
    the quad's side are covered, s s / 2 samples.  At s = 1 the centre itself is on the edge, and the top-left rule decides: a left edge
    takes it, a right edge does not."""
    shift, col, inside = (0.625, 2, slice(3, 8)) if side == "left" else (-0.625, 5, slice(0, 5))
    outside = slice(0, 2) if side == "left" else slice(6, 8)
    c, bg = np.array(COLOUR, dtype=np.int64), np.array(background, dtype=np.int64)
    for s in va.SAMPLES:
        out = va.view(*quad(shift), uniform_texture(), head_on((8, 8)), samples=s, shade=False, background=background)
        n = s * s
        assert (out["coverage"][:, inside] == n).all() and (out["coverage"][:, outside] == 0).all()
        assert (out["image"][:, inside] == c).all() and (out["image"][:, outside] == bg).all()
        if s == 1:
            whole = side == "left"
            assert (out["coverage"][:, col] == (1 if whole else 0)).all() and (out["image"][:, col] == (c if whole else bg)).all()
            continue
        assert (out["coverage"][:, col] == n // 2).all()
        by_hand = (c * (n // 2) + bg * (n // 2) + n // 2) >> LOG2[s]
        assert (out["image"][:, col] == by_hand).all(), (s, out["image"][0, col], by_hand)
        if background == (0, 0, 0, 0):  # the colour premultiplied by the coverage, and the coverage in alpha
            assert by_hand.tolist() == [(200 * (n // 2) + n // 2) >> LOG2[s], (100 * (n // 2) + n // 2) >> LOG2[s], (50 * (n // 2) + n // 2) >> LOG2[s],
                                        (255 * (n // 2) + n // 2) >> LOG2[s]]
            assert by_hand.tolist() == [100, 50, 25, 128]
        # which half: the samples on the quad's side of the centre line
        fine = out["fine"]["face_idx"][:, s * col: s * col + s] >= 0
        near, far = (fine[:, s // 2:], fine[:, :s // 2]) if side == "left" else (fine[:, :s // 2], fine[:, s // 2:])
        assert near.all() and not far.any()


def test_resolve_is_a_rounded_box_average_of_bytes():
    g = np.random.default_rng(5)
    fine = g.integers(0, 256, (8, 12, 4), dtype=np.uint8)
    assert np.array_equal(va.resolve(fine, 1), fine)
    for s in (2, 4):
        got = va.resolve(fine, s)
        for i in range(8 // s):
            for j in range(12 // s):
                for ch in range(4):
                    total = sum(int(fine[s * i + a, s * j + b, ch]) for a in range(s) for b in range(s))
                    assert got[i, j, ch] == (total + s * s // 2) // (s * s)
    assert (va.resolve(np.full((4, 4, 4), 255, dtype=np.uint8), 4) == 255).all()  # no overflow, no bias at the top


# ---------------------------------------------------------------- the poses of the GPU test
def pose_frame(name, s, filter="bilinear"):
    tex, eye, at, up, fov, near, _ = mip_ref.POSES[name]
    t, lv = mip_ref.texture(tex)
    mesh = [m.numpy() for m in mip_ref.field()]
    return va.view(*mesh, t, view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near), samples=s, filter=filter, levels=lv)


def test_the_representative_sample_is_the_one_below_and_right_of_the_centre():
    H, W = mip_ref.FRAME
    for s in (1, 2, 4):
        out = pose_frame("grazing", s, "trilinear")
        rows, cols = np.ix_(s * np.arange(H) + s // 2, s * np.arange(W) + s // 2)
        for key in ("face_idx", "depth", "lod"):
            assert np.array_equal(out[key], out["fine"][key][rows, cols]), (s, key)
        assert tuple(out["image"].shape) == (H, W, 4) and out["coverage"].dtype == np.uint8
        # a pixel may show a face that its representative sample misses, and the other way round
        assert ((out["coverage"] > 0) >= (out["face_idx"] >= 0)).all()
    assert ((pose_frame("grazing", 4)["coverage"] > 0) & (pose_frame("grazing", 4)["face_idx"] < 0)).any()


def test_lod_falls_by_about_log2_samples():
    for name, s, least, pixels in (("head_on_3", 2, 1, 300), ("head_on_7.8", 4, 2, 30)):
        one, many = pose_frame(name, 1, "trilinear"), pose_frame(name, s, "trilinear")
        both = (one["face_idx"] >= 0) & (many["face_idx"] >= 0) & (one["lod"] >= least)  # (a level cannot fall below 0)
        fall = (one["lod"] - many["lod"])[both]
        assert both.sum() > pixels and least - 0.5 < float(np.median(fall)) < least + 0.5, (name, int(both.sum()), float(np.median(fall)))


def test_the_poses_bite():
    """The table of the issue: partly covered pixels, and pixels whose samples see more than one face."""
    table = {("head_on_3", 2): (60, 497), ("head_on_3", 4): (82, 580), ("grazing", 2): (22, 410), ("grazing", 4): (38, 568), ("head_on_7.8", 4): (18, 96)}
    got = {}
    for name, s in table:
        out = pose_frame(name, s)
        n = s * s
        got[name, s] = (int(((out["coverage"] > 0) & (out["coverage"] < n)).sum()), int((out["faces_seen"] > 1).sum()))
        one = pose_frame(name, 1)
        assert not np.array_equal(out["image"], one["image"])  # anti-aliasing changes the frame
    print(got)
    for name in ("head_on_3", "grazing"):
        assert got[name, 4][0] >= 20 and got[name, 4][1] >= 400, got
    assert got["head_on_7.8", 4][0] >= 10, got
    assert got == table
