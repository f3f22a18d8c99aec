"""The anisotropic view of a textured mesh (include/dtp.h "an anisotropic view": dtp_mesh_view_aniso, dtp_op_mesh_view_aniso) without a
GPU: the header against the binding; the argument checks that come before any device call; the ValueErrors of the Python surface; and the
numpy restatement (tests/view_aniso_ref.py) on the four properties the rule was built for -- max_aniso 1 is the trilinear frame, a
magnified frame is the bilinear one, a square footprint is the trilinear pixel, visibility never depends on the filter -- on the pinned
histograms of taps and levels, on the floor whose stripes the trilinear filter loses, and on the poses of the GPU test, where every
number of taps from 1 to 16 has to be taken.  Nothing is compared under a tolerance."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mip_ref
import view_aniso_ref as an
import view_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
ENTRIES = ("dtp_mesh_view_aniso", "dtp_op_mesh_view_aniso")
EXACT = ("image", "lod", "face_idx", "depth")


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def field_pose(name):
    tex, eye, at, up, fov, near, _ = mip_ref.POSES[name]
    return "field:" + tex, (eye, at, up, fov, near)


def covered(frame):
    return frame["face_idx"] >= 0


def tap_histogram(frame, M=16):
    return np.bincount(frame["N"][covered(frame)], minlength=M + 1)[1:].tolist()


# ---------------------------------------------------------------- the header, the checks, the Python surface
def test_header_and_binding_agree_on_the_anisotropic_view(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3
    assert "an anisotropic view" in hdr
    note = hdr[:hdr.index("#define DTP_ABI_VERSION")]
    assert all(name in note for name in ENTRIES)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    assert set(ENTRIES) <= declared and declared == set(_lib.SYMBOLS)
    args = lambda name: re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")  # noqa: E731
    for name in ENTRIES:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
        assert len(args(name)) == len(_lib.SYMBOLS[name][1]), name
    want = ["mesh", "texture", "TH", "TW", "mips", "cam", "H", "W", "opts", "clip", "samples", "max_aniso", "image", "face_idx", "depth", "lod",
            "taps", "coverage"]
    assert [a.split()[-1] for a in args("dtp_mesh_view_aniso")] == want + ["s"]
    assert [a.split()[-1] for a in args("dtp_op_mesh_view_aniso")] == want + ["binned", "s"]
    assert C.sizeof(_lib.ViewOpts) == 24 and C.sizeof(_lib.ViewCam) == 60  # the structs of a view did not grow
    assert _lib.VIEW_MAX_ANISO == 16 == an.MAX_ANISO


@pytest.mark.parametrize("entry", ENTRIES)
def test_aniso_refuses_before_any_device_call(lib, entry):
    """No device here: every one of these returns from the checks, and nothing is written.  The handle that is not a mesh is looked up,
    never followed."""
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    fn = getattr(lib, entry)
    tail = (0, None) if entry == "dtp_op_mesh_view_aniso" else (None,)
    cam = view_camera((0.3, -1.7, 2.9), (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 45.0, (360, 640), 0.05).struct()
    opts = view_opts()
    tex = (C.c_uint32 * 16)()
    mips = (C.c_uint32 * 8)()
    img = (C.c_uint32 * 16)(*([0x5a5a5a5a] * 16))
    fidx, dep, lod = (C.c_int * 4)(*([7] * 4)), (C.c_float * 4)(*([7.0] * 4)), (C.c_float * 4)(*([7.0] * 4))
    tap, cov = (C.c_uint8 * 8)(*([0x5a] * 8)), (C.c_uint8 * 8)(*([0x5a] * 8))
    fake = C.cast((C.c_int * 64)(), C.c_void_p)
    vp = (lambda a, off=0: C.c_void_p(C.addressof(a) + off))

    def refused(word, mesh=fake, texture=vp(tex), TH=4, TW=4, m=vp(mips), c=C.byref(cam), H=2, W=2, o=C.byref(opts), clip=1, samples=2, M=4,
                image=vp(img), f=vp(fidx), d=vp(dep), lo=vp(lod), tp=vp(tap), cv=vp(cov)):
        rc = fn(mesh, texture, TH, TW, m, c, H, W, o, clip, samples, M, image, f, d, lo, tp, cv, *tail)
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(img) == [0x5a5a5a5a] * 16 and list(fidx) == [7] * 4 and list(dep) == [7.0] * 4 and list(lod) == [7.0] * 4
        assert list(tap) == [0x5a] * 8 and list(cov) == [0x5a] * 8

    for M in (0, 17, -1, 1 << 20):
        refused(r"max_aniso must lie in 1\.\.16", M=M)
    refused("mips is required", m=None)
    for samples in (3, 0, 8):
        refused("samples is 1, 2 or 4", samples=samples)
    for samples, side in ((1, 4097), (2, 2049), (4, 1025)):
        refused(r"1\.\.4096" if samples == 1 else "must not exceed 4096", samples=samples, H=side)
        refused(r"1\.\.4096" if samples == 1 else "must not exceed 4096", samples=samples, W=side)
    refused("clip is 0 or 1", clip=2)
    refused("aligned", m=vp(mips, 2))
    refused("aligned", lo=vp(lod, 1))
    refused("NULL", mesh=None)
    refused("NULL", texture=None)
    refused("NULL", image=None)
    refused(r"1\.\.32768", TW=32769)
    # every argument in order, at both ends of the range, with the optional outputs absent: the look-up is what refuses
    for M in (1, 16):
        for samples in (1, 2, 4):
            refused("not a live mesh", M=M, samples=samples)
            refused("not a live mesh", M=M, samples=samples, f=None, d=None, lo=None, tp=None, cv=None)
    refused("not a live mesh", tp=vp(tap, 1), cv=vp(cov, 3))  # (taps and coverage are bytes: any address)


def test_python_surface_takes_the_keywords_and_refuses_what_it_must(lib):
    from diffusiontexturepainting_amd import _lib, mesh as _mesh, ops
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    render = MI355ConditionalInpainter.render_view
    p = inspect.signature(render).parameters
    assert p["anisotropy"].default == 1 and p["want_taps"].default is False
    p = inspect.signature(ops.mesh_view).parameters
    assert p["anisotropy"].default is None and p["want_taps"].default is False
    cam = _mesh.view_camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (34, 50), 0.05)
    a_mesh = object.__new__(_mesh.Mesh)  # never followed: these checks come before the mesh, the texture and the model are used
    for bad in (0, 17, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="anisotropy"):
            render(None, a_mesh, None, cam, filter="trilinear", anisotropy=bad)
        if bad is not None:
            with pytest.raises(ValueError, match="anisotropy"):
                ops.mesh_view(None, None, cam, filter="trilinear", anisotropy=bad)
    for M in (2, 16):
        with pytest.raises(ValueError, match="trilinear"):
            render(None, a_mesh, None, cam, anisotropy=M)
        with pytest.raises(ValueError, match="trilinear"):
            ops.mesh_view(None, None, cam, anisotropy=M)
    with pytest.raises(ValueError, match="trilinear"):
        ops.mesh_view(None, None, cam, anisotropy=1)  # at op level a 1 runs the new entry, so it needs the filter too
    for kw in (dict(), dict(anisotropy=1), dict(filter="trilinear"), dict(filter="trilinear", anisotropy=1)):
        with pytest.raises(ValueError, match="want_taps"):
            render(None, a_mesh, None, cam, want_taps=True, **kw)
    with pytest.raises(ValueError, match="want_taps"):
        ops.mesh_view(None, None, cam, want_taps=True)
    # filter= keeps its two values
    with pytest.raises(ValueError, match="bilinear.*trilinear"):
        render(None, a_mesh, None, cam, filter="anisotropic")
    with pytest.raises(ValueError, match="bilinear.*trilinear"):
        render(None, a_mesh, None, cam, filter="anisotropic", anisotropy=4)
    with pytest.raises(ValueError):
        ops.mesh_view(None, None, cam, filter="anisotropic", anisotropy=4)
    assert [_lib.view_anisotropy_check(m, "trilinear", m > 1, least=2) for m in (1, 2, 16)] == [1, 2, 16]
    for M in (0, 17):
        with pytest.raises(ValueError):
            an.fine_view(None, None, None, None, dict(size=(4, 4)), max_aniso=M)


# ---------------------------------------------------------------- the restatement: the four properties
@pytest.mark.parametrize("name", list(mip_ref.POSES))
def test_max_aniso_1_is_the_trilinear_frame(name):
    """P1: rho2 = pmax2, N = 1, o_0 = 0."""
    want = mip_ref.pose_reference(name)
    got = an.reference(*field_pose(name), mip_ref.FRAME, 1)
    for key in EXACT + ("level", "f"):
        assert np.array_equal(got[key], want[key]), (name, key)
    assert np.array_equal(got["rho2"], want["rho2"]) and np.array_equal(got["N"], covered(want).astype(np.int64))
    assert np.array_equal(got["horizon"], want["horizon"])


def test_a_magnified_frame_takes_one_tap_of_level_0_and_is_the_bilinear_frame():
    """P2: pmax2 <= 1 everywhere."""
    tex, eye, at, up, fov, near = mip_ref.MAGNIFIED
    got = an.reference("field:" + tex, (eye, at, up, fov, near), mip_ref.FRAME, 16)
    hit = covered(got)
    assert hit.sum() > 1000 and (got["pmax2"][hit] <= 1).all()
    assert (got["N"][hit] == 1).all() and (got["level"][hit] == 0).all() and (got["f"] == 0).all() and (got["lod"] == 0).all()
    mesh, t, _ = an.scene("field:" + tex)
    want = view_ref.view(*mesh, t, view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near))
    for key in ("image", "face_idx", "depth"):
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("distance", [1.0, 2.0, 4.0])
def test_a_square_footprint_is_the_trilinear_pixel(distance):
    """P3: a flat square quad seen head-on, axis-aligned UVs on a square texture: la2 == lb2, so N = 1 at any M.  Every value is dyadic
    (view_aniso_ref.quad_scene), so the equality is exact: 1.5, 3 and 6 texels per pixel, levels 0, 1 and 2 with a fraction."""
    pose = ((0, 0, distance), (0, 0, 0), (0, 1, 0), 90.0, 0.5)
    mesh, t, lv = an.scene("quad")
    want = mip_ref.view(*mesh, t, view_ref.camera(*pose[:4], (32, 32), pose[4]), levels=lv)
    hit = covered(want)
    assert hit.sum() == (32 / distance) ** 2 and (want["rho2"][hit] == (1.5 * distance) ** 2).all() and (want["f"][hit] > 0).all()
    for M in (2, 5, 16):
        got = an.reference("quad", pose, (32, 32), M)
        assert np.array_equal(got["pmax2"], got["pmin2"]) and (got["N"][hit] == 1).all()
        for key in EXACT + ("level", "f"):
            assert np.array_equal(got[key], want[key]), (M, key)


@pytest.mark.parametrize("name", ["grazing", "head_on_3"])
def test_visibility_never_depends_on_the_filter(name):
    """P4."""
    want = mip_ref.pose_reference(name)
    for M in (2, 16):
        got = an.reference(*field_pose(name), mip_ref.FRAME, M)
        assert np.array_equal(got["face_idx"], want["face_idx"]) and np.array_equal(got["depth"], want["depth"])
        assert (got["lod"] <= want["lod"]).all()  # never coarser than the trilinear level
        assert (got["taps"] == got["N"]).all() and (got["taps"][~covered(got)] == 0).all() and got["taps"].dtype == np.uint8


# ---------------------------------------------------------------- pinned histograms
def test_grazing_pose_histograms_at_4():
    got = an.reference(*field_pose("grazing"), mip_ref.FRAME, 4)
    hit = covered(got)
    assert hit.sum() == 907 == sum(mip_ref.POSES["grazing"][6])
    assert tap_histogram(got, 4) == an.GRAZING_M4_TAPS == [0, 860, 33, 14]
    assert np.bincount(got["level"][hit], minlength=9).tolist() == an.GRAZING_M4_LEVELS == [700, 175, 25, 1, 5, 1, 0, 0, 0]
    assert mip_ref.POSES["grazing"][6][0] == 568  # the trilinear frame takes level 0 on 568 of them


# ---------------------------------------------------------------- the floor
def far_rows(frame):
    hit = covered(frame)
    return [i for i in range(hit.shape[0]) if hit[i].sum() >= 32][:2]


def red_spread(frame, row):
    return float(np.std(frame["image"][row][covered(frame)[row]][:, 0].astype(np.float64)))


def test_the_floor_keeps_its_stripes():
    """The floor of the issue, striped across the line of sight.  In the two farthest rows with at least 32 covered pixels the
    trilinear frame is grey (the restatement: 0.0 and 5.9), the anisotropic one striped (46.6 / 51.6 at 4, 49.6 / 51.8 at 16)."""
    tri = an.reference("floor", an.FLOOR_POSE, an.FLOOR_SIZE, 1, shade=False)
    mesh, t, lv = an.scene("floor")
    eye, at, up, fov, near = an.FLOOR_POSE
    plain = mip_ref.view(*mesh, t, view_ref.camera(eye, at, up, fov, an.FLOOR_SIZE, near), levels=lv, shade=False)
    assert np.array_equal(tri["image"], plain["image"]) and np.array_equal(tri["lod"], plain["lod"])
    rows = far_rows(tri)
    assert len(rows) == 2
    for row in rows:
        print(row, red_spread(tri, row), [red_spread(an.reference("floor", an.FLOOR_POSE, an.FLOOR_SIZE, M, shade=False), row) for M in (4, 16)])
        assert red_spread(tri, row) < 10
        for M in (4, 16):
            got = an.reference("floor", an.FLOOR_POSE, an.FLOOR_SIZE, M, shade=False)
            assert far_rows(got) == rows and red_spread(got, row) > 40, (M, row, red_spread(got, row))


# ---------------------------------------------------------------- the poses of the GPU test
@pytest.mark.parametrize("name", list(an.POSES))
def test_pose_histograms_at_16(name):
    scene, eye, at, up, fov, near, hist, clamped = an.POSES[name]
    got = an.reference(scene, (eye, at, up, fov, near), mip_ref.FRAME, 16)
    hit = covered(got)
    assert tap_histogram(got) == hist
    assert int((hit & (got["N"] == 16) & (got["pmax2"] > np.float32(256) * got["pmin2"])).sum()) == clamped
    for M in (2, 3, 4, 8):
        assert int(an.reference(scene, (eye, at, up, fov, near), mip_ref.FRAME, M)["N"].max()) <= M


def test_every_number_of_taps_is_taken_and_the_clamp_is_hit():
    taken = np.zeros(17, dtype=np.int64)
    clamped = 0
    for scene, eye, at, up, fov, near, _, _ in an.POSES.values():
        got = an.reference(scene, (eye, at, up, fov, near), mip_ref.FRAME, 16)
        taken += np.bincount(got["N"][covered(got)], minlength=17)
        clamped += int((covered(got) & (got["N"] == 16) & (got["pmax2"] > np.float32(256) * got["pmin2"])).sum())
    tex, eye, at, up, fov, near = mip_ref.MAGNIFIED
    got = an.reference("field:" + tex, (eye, at, up, fov, near), mip_ref.FRAME, 16)
    taken += np.bincount(got["N"][covered(got)], minlength=17)
    assert (taken[1:] > 0).all() and clamped >= 1, (taken.tolist(), clamped)


def test_the_horizon_triangle_takes_one_tap_of_the_last_level():
    eye, at, fov, size, near = mip_ref.TRIANGLE_POSE
    last = len(mip_ref.texture("atlas")[1]) - 1
    got = an.reference("triangle", (eye, at, (0, -1, 0), fov, near), size, 16)
    hit = covered(got)
    assert hit.sum() > 0 and got["horizon"][hit].all()
    assert (got["N"][hit] == 1).all() and (got["level"][hit] == last).all() and (got["lod"][hit] == last).all()
    mesh, t, lv = an.scene("triangle")
    want = mip_ref.view(*mesh, t, view_ref.camera(eye, at, (0, -1, 0), fov, size, near), levels=lv)
    for key in EXACT:
        assert np.array_equal(got[key], want[key]), key
    # the right way up none of its pixels is beyond the horizon, and the strip is stretched: more than one tap somewhere
    got = an.reference("triangle", (eye, at, (0, 1, 0), fov, near), size, 16)
    assert not got["horizon"].any() and got["N"].max() > 1


def test_samples_resolve_as_the_anti_aliased_view_resolves():
    """samples = s is the frame at s x the size, resolved by view_aa_ref: at max_aniso 1 that is view_aa_ref's trilinear frame."""
    import view_aa_ref as va
    tex, eye, at, up, fov, near, _ = mip_ref.POSES["grazing"]
    mesh, t, lv = an.scene("field:" + tex)
    for s in (2, 4):
        want = va.view(*mesh, t, view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near), samples=s, filter="trilinear", levels=lv)
        got = an.reference("field:" + tex, (eye, at, up, fov, near), mip_ref.FRAME, 1, samples=s)
        for key in EXACT + ("coverage",):
            assert np.array_equal(got[key], want[key]), (s, key)
        many = an.reference("field:" + tex, (eye, at, up, fov, near), mip_ref.FRAME, 8, samples=s)
        assert np.array_equal(many["coverage"], want["coverage"]) and not np.array_equal(many["image"], want["image"])
        assert np.array_equal(many["taps"], many["fine"]["taps"][s // 2::s, s // 2::s])
