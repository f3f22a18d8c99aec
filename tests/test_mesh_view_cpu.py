"""The host-only part of the view of a textured mesh (include/dtp.h "a view of a textured mesh": dtp_view_camera, dtp_view_rays, the
argument checks of dtp_mesh_view / dtp_op_mesh_view that come before any device call) against the numpy restatement (tests/view_ref.py);
the restatement itself against hand values chosen dyadic, so that every one of them is exact; the rays of a frame's pixels against the
frame; and the stand-alone host program tools/view_host_check.cpp.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_ref
import pick_ref
import view_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# eye, at, up, fov_y, (H, W), near
POSES = {
    "down_minus_z": ((0, 0, 3), (0, 0, 0), (0, 1, 0), 90.0, (64, 64), 0.5),
    "down_minus_z_wide_frame": ((0.25, 0.5, 2), (0.25, 0.5, 0), (0, 1, 0), 45.0, (720, 1280), 0.01),
    "along_x": ((5, -1, 0.5), (0, -1, 0.5), (0, 0, 1), 60.0, (136, 200), 0.125),
    "along_minus_y_up_not_unit": ((0, 7, 0), (0, 0, 0), (0, 0, 2.5), 30.0, (1080, 1920), 1.0),
    "oblique": ((0.3, -1.7, 2.9), (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 45.0, (360, 640), 0.05),
    "oblique_up_tilted": ((-1.2, 1.4, 1.1), (0.4, -0.1, 0.2), (0.3, 0.2, 0.9), 70.0, (24, 4096), 0.01),
    "oblique_far_from_the_origin": ((1234.5, -987.25, 400.125), (1230.0, -990.0, 398.0), (0, 1, 0), 12.5, (4096, 24), 0.25),
    "narrow": ((0, 0, 100), (0, 0, 0), (1, 0, 0), 0.5, (64, 64), 10.0),
    "wide": ((0, 0, 1), (0, 0, 0), (0, -1, 0), 170.0, (1, 1), 0.001),
}


def lib_camera(name):
    from diffusiontexturepainting_amd.mesh import view_camera
    eye, at, up, fov, size, near = POSES[name]
    return view_camera(eye, at, up, fov, size, near)


@pytest.mark.parametrize("name", sorted(POSES))
def test_camera_equals_the_restatement(lib, name):
    from diffusiontexturepainting_amd.mesh import Mesh
    eye, at, up, fov, size, near = POSES[name]
    got, want = lib_camera(name), view_ref.camera(eye, at, up, fov, size, near)
    assert got.m.dtype == torch.float32 and tuple(got.m.shape) == (3, 4) and got.size == size
    assert np.array_equal(got.m.numpy(), want["m"]), (got.m, want["m"])
    assert (f32(got.fx), f32(got.fy), f32(got.near)) == (want["fx"], want["fy"], want["near"])
    assert torch.equal(Mesh.view_camera(eye, at, up, fov, size, near).m, got.m)
    # a rigid frame: the eye maps to 0, `at` lies straight ahead on -z
    rot = want["m"][:, :3].astype(np.float64)
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-6) and np.linalg.det(rot) > 0
    scale = max(1.0, float(np.abs(np.asarray(eye)).max()))
    assert np.allclose(rot @ np.asarray(eye, dtype=np.float64) + want["m"][:, 3], 0, atol=4e-6 * scale)
    ahead = rot @ np.asarray(at, dtype=np.float64) + want["m"][:, 3]
    assert np.allclose(ahead[:2], 0, atol=4e-6 * scale) and ahead[2] < 0
    assert np.isclose(float(want["fy"]), 1 / np.tan(np.radians(fov) / 2), rtol=1e-6) and np.isclose(float(want["fx"]) * size[1], float(want["fy"]) * size[0], rtol=1e-6)


def test_camera_by_hand(lib):
    from diffusiontexturepainting_amd.mesh import view_camera
    cam = view_camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 90.0, (64, 128), 0.5)
    assert torch.equal(cam.m, torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -3]])) and (cam.fx, cam.fy, cam.near) == (0.5, 1.0, 0.5)
    cam = view_camera((2, 0, 0), (0, 0, 0), (0, 0, 1), 90.0, (64, 64), 0.25)
    assert torch.equal(cam.m, torch.tensor([[0.0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, -2]])) and (cam.fx, cam.fy) == (1.0, 1.0)


def pixel_sets(H, W):
    g = np.random.default_rng(H * 4099 + W)
    centres = [(j + 0.5, i + 0.5) for i in (0, H // 2, H - 1) for j in (0, W // 2, W - 1)]
    corners = [(0, 0), (W, 0), (0, H), (W, H), (W / 2, H / 2)]
    loose = (g.random((24, 2)) * [W + 8, H + 8] - 4).tolist()  # fractional positions, some outside the frame
    return np.array(centres + corners + loose, dtype=f32)


@pytest.mark.parametrize("name", sorted(POSES))
def test_rays_equal_the_restatement(lib, name):
    from diffusiontexturepainting_amd.mesh import Mesh, view_rays
    eye, at, up, fov, size, near = POSES[name]
    cam, ref_cam = lib_camera(name), view_ref.camera(eye, at, up, fov, size, near)
    px = pixel_sets(*size)
    o, d = view_rays(cam, px)
    ro, rd = view_ref.rays(ref_cam, px)
    assert o.dtype == torch.float32 and tuple(o.shape) == tuple(d.shape) == (px.shape[0], 3)
    assert np.array_equal(o.numpy(), ro) and np.array_equal(d.numpy(), rd)
    o2, d2 = Mesh.view_rays(cam, torch.from_numpy(px), size=size)
    assert torch.equal(o2, o) and torch.equal(d2, d)
    # the origin is the eye; the ray of a pixel, through the camera and the perspective division, lands on that pixel
    scale = max(1.0, float(np.abs(np.asarray(eye)).max()))
    assert np.allclose(ro, np.asarray(eye, dtype=np.float64), atol=8e-6 * scale)
    m = ref_cam["m"].astype(np.float64)
    c = rd.astype(np.float64) @ m[:, :3].T
    assert (c[:, 2] < 0).all()
    x = (c[:, 0] * float(ref_cam["fx"]) / -c[:, 2] + 1) * size[1] / 2
    y = (1 - c[:, 1] * float(ref_cam["fy"]) / -c[:, 2]) * size[0] / 2
    assert np.allclose(x, px[:, 0], atol=1e-3 * max(size)) and np.allclose(y, px[:, 1], atol=1e-3 * max(size))


def test_rays_by_hand(lib):
    from diffusiontexturepainting_amd.mesh import view_camera, view_rays
    cam = view_camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 90.0, (64, 128), 0.5)
    o, d = view_rays(cam, [(64, 32), (0, 0), (128, 64), (64.5, 31.5)])
    assert torch.equal(o, torch.tensor([[0.0, 0, 3]] * 4))
    assert torch.equal(d, torch.tensor([[0.0, 0, -1], [-2, 1, -1], [2, -1, -1], [1 / 64, 1 / 64, -1]]))
    o, d = view_rays(cam, (64, 32))
    assert tuple(d.shape) == (1, 3)


CAM_REFUSALS = [
    (((0, 0, float("nan")), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), 0.1), "non-finite"),
    (((0, 0, 3), (0, float("inf"), 0), (0, 1, 0), 45.0, (64, 64), 0.1), "non-finite"),
    (((0, 0, 3), (0, 0, 0), (0, float("nan"), 0), 45.0, (64, 64), 0.1), "non-finite"),
    (((1, 2, 3), (1, 2, 3), (0, 1, 0), 45.0, (64, 64), 0.1), "eye == at"),
    (((0, 0, 3), (0, 0, 0), (0, 0, 0), 45.0, (64, 64), 0.1), "up is zero"),
    (((0, 0, 3), (0, 0, 0), (0, 0, -2), 45.0, (64, 64), 0.1), "parallel"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 0.0, (64, 64), 0.1), "fov_y"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 180.0, (64, 64), 0.1), "fov_y"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), -30.0, (64, 64), 0.1), "fov_y"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), float("nan"), (64, 64), 0.1), "fov_y"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), 0.0), "near"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), -1.0), "near"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), float("inf")), "near"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), 1e-45), "fit fp32"),
    (((3e38, 3e38, 3e38), (0, 0, 0), (0, 1, 0), 45.0, (64, 64), 0.1), "fit fp32"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (0, 64), 0.1), r"1\.\.4096"),
    (((0, 0, 3), (0, 0, 0), (0, 1, 0), 45.0, (64, 4097), 0.1), r"1\.\.4096"),
]


@pytest.mark.parametrize("args,word", CAM_REFUSALS)
def test_camera_refusals(lib, args, word):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.mesh import view_camera
    with pytest.raises(DtpError, match=rf"\(code {ARG}\).*{word}"):
        view_camera(*args)
    with pytest.raises(ValueError):
        view_ref.camera(*args)
    eye, at, up, fov, size, near = args
    out = _lib.ViewCam((C.c_float * 12)(*([9.0] * 12)), 9.0, 9.0, 9.0)
    v = [(C.c_float * 3)(*x) for x in (eye, at, up)]
    assert lib.dtp_view_camera(C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.c_float(fov), size[0], size[1], C.c_float(near), C.byref(out)) == ARG
    assert list(out.m) == [9.0] * 12 and (out.fx, out.fy, out.near) == (9.0, 9.0, 9.0)  # a refused call writes nothing
    assert lib.dtp_view_camera(None, C.byref(v[1]), C.byref(v[2]), C.c_float(45.0), 64, 64, C.c_float(0.1), C.byref(out)) == ARG
    assert lib.dtp_view_camera(C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.c_float(45.0), 64, 64, C.c_float(0.1), None) == ARG


def test_rays_refusals(lib):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.mesh import view_rays
    cam = lib_camera("oblique")
    with pytest.raises(DtpError, match=r"pixel 1: a non-finite pixel"):
        view_rays(cam, [(1, 2), (float("nan"), 3)])
    with pytest.raises(DtpError, match=r"1\.\.4096"):
        view_rays(cam, [(1, 2)], size=(0, 5))
    with pytest.raises(DtpError, match=r"at least 1"):
        view_rays(cam, np.zeros((0, 2), dtype=f32))
    ref_cam = view_ref.camera(*POSES["oblique"])
    for bad in ([(1, 2), (float("nan"), 3)], np.zeros((0, 2))):
        with pytest.raises(ValueError):
            view_ref.rays(ref_cam, bad)
    st = cam.struct()
    px = (C.c_float * 4)(1, 2, 3, 4)
    out = (C.c_float * 12)(*([7.0] * 12))

    def refused(c, n, word, xy=px):
        assert lib.dtp_view_rays(c, 64, 64, xy, n, out) == ARG and re.search(word, lib.dtp_last_error().decode()), lib.dtp_last_error()
        assert list(out) == [7.0] * 12

    refused(None, 2, "NULL")
    refused(C.byref(st), 2, "NULL", None)
    refused(C.byref(st), 0, "at least 1")
    for field, value, word in (("fx", 0.0, "fx and fy"), ("fy", float("inf"), "fx and fy"), ("near", 0.0, "near"), ("near", float("nan"), "near")):
        broken = cam.struct()
        setattr(broken, field, value)
        refused(C.byref(broken), 2, word)
    broken = cam.struct()
    broken.m[6] = float("nan")
    refused(C.byref(broken), 2, "matrix")
    assert lib.dtp_view_rays(C.byref(st), 64, 64, px, 2, None) == ARG
    assert _lib.VIEW_MAX == view_ref.VIEW_MAX


@pytest.mark.parametrize("entry", ["dtp_mesh_view", "dtp_op_mesh_view"])
def test_view_refuses_before_any_device_call(lib, entry):
    """No device here: every one of these returns from the checks.  The handle that is not a mesh is looked up, never followed."""
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd.mesh import view_opts
    fn = getattr(lib, entry)
    tail = (1, None) if entry == "dtp_op_mesh_view" else (None,)
    cam = lib_camera("oblique").struct()
    opts = view_opts()
    tex = (C.c_uint32 * 16)()
    img = (C.c_uint32 * 16)(*([0x5a5a5a5a] * 16))
    fidx, dep = (C.c_int * 4)(*([7] * 4)), (C.c_float * 4)(*([7.0] * 4))
    not_a_mesh = (C.c_int * 64)()
    fake = C.cast(not_a_mesh, C.c_void_p)
    vp = (lambda a, off=0: C.c_void_p(C.addressof(a) + off))

    def refused(word, mesh=fake, texture=vp(tex), TH=4, TW=4, c=C.byref(cam), H=2, W=2, o=C.byref(opts), image=vp(img), f=vp(fidx), d=vp(dep)):
        rc = fn(mesh, texture, TH, TW, c, H, W, o, image, f, d, *tail)
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(img) == [0x5a5a5a5a] * 16 and list(fidx) == [7] * 4 and list(dep) == [7.0] * 4

    refused("NULL", mesh=None)
    refused("NULL", texture=None)
    refused("NULL", c=None)
    refused("NULL", o=None)
    refused("NULL", image=None)
    for H, W in ((0, 2), (2, 0), (4097, 2), (2, 4097), (-1, 2)):
        refused(r"1\.\.4096", H=H, W=W)
    for TH, TW in ((0, 4), (4, 0), (32769, 4), (4, 32769)):
        refused(r"1\.\.32768", TH=TH, TW=TW)
    refused("aligned", texture=vp(tex, 1))
    refused("aligned", image=vp(img, 2))
    refused("aligned", f=vp(fidx, 1))
    refused("aligned", d=vp(dep, 3))
    for field, value, word in (("fx", 0.0, "fx and fy"), ("fy", -1.0, "fx and fy"), ("near", 0.0, "near"), ("near", float("inf"), "near"),
                               ("near", 1e-45, "near")):
        broken = lib_camera("oblique").struct()
        setattr(broken, field, value)
        refused(word, c=C.byref(broken))
    broken = lib_camera("oblique").struct()
    broken.m[11] = float("inf")
    refused("matrix", c=C.byref(broken))
    for kw, word in ((dict(cull=2), "0 or 1"), (dict(flip_normals=-1), "0 or 1"), (dict(shade=5), "0 or 1"), (dict(ambient=-0.5), "ambient"),
                     (dict(ambient=1.25), "ambient"), (dict(ambient=float("nan")), "ambient")):
        bad = view_opts()
        for k, v in kw.items():
            setattr(bad, k, v)
        refused(word, o=C.byref(bad))
    refused("not a live mesh")                     # every argument in order: the look-up is what refuses
    refused("not a live mesh", f=None, d=None)     # (the optional outputs may be absent)


def test_header_and_binding_agree_on_the_view(lib):
    from diffusiontexturepainting_amd import _lib, mesh
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3
    assert "a view of a textured mesh" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_view_camera", "dtp_view_rays", "dtp_mesh_view", "dtp_op_mesh_view"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"

    def fields(name):
        m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, code)
        return re.sub(r"\s+", " ", m.group(1)).strip()

    assert fields("dtp_view_cam") == "float m[12]; float fx, fy, near;"
    assert fields("dtp_view_opts") == "int cull, flip_normals, shade; float ambient; uint8_t unpainted[3]; uint8_t background[4];"
    assert [f[0] for f in _lib.ViewCam._fields_] == ["m", "fx", "fy", "near"] and C.sizeof(_lib.ViewCam) == 60 and _lib.ViewCam.fx.offset == 48
    assert [f[0] for f in _lib.ViewOpts._fields_] == ["cull", "flip_normals", "shade", "ambient", "unpainted", "background"]
    assert C.sizeof(_lib.ViewOpts) == 24 and _lib.ViewOpts.ambient.offset == 12 and _lib.ViewOpts.unpainted.offset == 16
    assert _lib.ViewOpts.background.offset == 19
    args = lambda name: len(re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(","))  # noqa: E731
    for name in new:
        assert args(name) == len(_lib.SYMBOLS[name][1]), name
    o = mesh.view_opts(cull=True, ambient=0.5, unpainted=(1, 2, 3), background=(4, 5, 6, 7))
    assert (o.cull, o.flip_normals, o.shade, o.ambient, list(o.unpainted), list(o.background)) == (1, 0, 1, 0.5, [1, 2, 3], [4, 5, 6, 7])
    with pytest.raises(ValueError):
        mesh.view_opts(unpainted=(1, 2))
    with pytest.raises(ValueError):
        mesh.view_opts(background=(1, 2, 3, 256))


# ---------------------------------------------------------------- the restatement against hand values
def hand_cam(size, near=0.5):
    """The camera at the origin looking down -z with fx = fy = 1: camera space is world space, NDC = (x, y) / -z."""
    return dict(m=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=f32), fx=f32(1), fy=f32(1), near=f32(near), size=size)


def quad(corners, uv=((0, 0), (1, 0), (1, 1), (0, 1))):
    """Four corners, counter-clockwise seen from the camera -> vertices, faces (0, 1, 2), (0, 2, 3), face UVs."""
    v = np.array(corners, dtype=f32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    return v, f, np.array(uv, dtype=f32)[f]


# On a 9 x 9 frame the pixel (4, 4) has its centre at NDC (0, 0), and the square |ndc| <= 0.5 covers the pixels 2 .. 6 each way with no
# centre on its border.  TILTED: left edge at z = -1, right edge at z = -4, the same square on the screen.
TILTED = [(-0.5, -0.5, -1), (2, -2, -4), (2, 2, -4), (-0.5, 0.5, -1)]
FLAT = [(-1, -1, -2), (1, -1, -2), (1, 1, -2), (-1, 1, -2)]
WHITE = np.full((4, 4, 4), 255, dtype=np.uint8)


def test_restatement_perspective_correct_uv_differs_from_screen_linear():
    v, f, uv = quad(TILTED)
    out = view_ref.view(v, f, uv, WHITE, hand_cam((9, 9)), shade=False)
    assert np.array_equal(out["face_idx"][2:7, 2:7] >= 0, np.ones((5, 5), bool)) and (out["face_idx"] >= 0).sum() == 25
    proj = out["proj"]
    assert proj["X"].tolist() == [[576, 1728, 1728], [576, 1728, 576]] and proj["iw"].tolist() == [[1, 0.25, 0.25], [1, 0.25, 1]]
    face = int(out["face_idx"][4, 4])
    inside, w = mesh_ref.cover(proj["X"][face], proj["Y"][face], np.array([1152]), np.array([1152]))
    assert inside[0] and sorted(w[0].tolist()) == [0.0, 0.5, 0.5]         # the midpoint of the diagonal the two faces share
    linear = mesh_ref.interp(w[0], uv[face, 0, 0], uv[face, 1, 0], uv[face, 2, 0])
    assert linear == f32(0.5)                                              # screen-linear: halfway
    assert out["uv"][4, 4, 0] == f32(0.125) / f32(0.625) == f32(0.2)      # perspective-correct: (0.5 x 0.25 x 1) / (0.5 x 1 + 0.5 x 0.25)
    assert out["uv"][4, 4, 1] == f32(0.2) and out["depth"][4, 4] == f32(1) / f32(0.625) == f32(1.6)
    # along the row of the midpoint u follows 1 / z, not x: the pixel columns 2 .. 6 have ndc_x = (2 j + 1) / 9 - 1
    want = [(0.5 + n) * 0.25 / ((0.5 - n) * 1 + (0.5 + n) * 0.25) for n in ((2 * j + 1) / 9 - 1 for j in range(2, 7))]
    assert np.allclose(out["uv"][4, 2:7, 0], want, atol=1e-6) and np.all(np.diff(out["uv"][4, 2:7, 0]) > 0)
    assert np.allclose(out["depth"][4, 2:7], [1 / ((0.5 - n) * 1 + (0.5 + n) * 0.25) for n in ((2 * j + 1) / 9 - 1 for j in range(2, 7))], atol=1e-6)
    assert not out["depth"][out["face_idx"] < 0].any()


def test_restatement_interpenetrating_quads_change_winner_along_their_line():
    """The flat quad at depth 2 (d = 0.5) and the tilted one (d = 0.625 - 0.75 ndc_x) meet at ndc_x = 1 / 6: between pixel columns 4 and 5."""
    a, b = quad(FLAT), quad(TILTED)
    for order in (0, 1):
        first, second = (a, b) if order == 0 else (b, a)
        v = np.concatenate([first[0], second[0]])
        f = np.concatenate([first[1], second[1] + 4])
        uv = np.concatenate([first[2], second[2]])
        out = view_ref.view(v, f, uv, WHITE, hand_cam((9, 9)), shade=False)
        tilted_faces = (2, 3) if order == 0 else (0, 1)
        is_tilted = np.isin(out["face_idx"], tilted_faces)
        assert is_tilted[2:7, 2:5].all() and not is_tilted[2:7, 5:7].any() and (out["face_idx"][2:7, 5:7] >= 0).all()
        assert np.array_equal(out["depth"][2:7, 5:7], np.full((5, 2), 2, dtype=f32)) and (out["depth"][2:7, 2:5] < 2).all()


def test_restatement_coincident_faces_go_to_the_lower_index():
    v, f, uv = quad(FLAT)
    v2, f2, uv2 = np.concatenate([v, v]), np.concatenate([f + 4, f]), np.concatenate([uv, uv])  # faces 0, 1 use the second copy
    out = view_ref.view(v2, f2, uv2, WHITE, hand_cam((9, 9)))
    assert set(out["face_idx"][2:7, 2:7].ravel().tolist()) == {0, 1}
    single = view_ref.view(v, f, uv, WHITE, hand_cam((9, 9)))
    assert np.array_equal(out["image"], single["image"]) and np.array_equal(out["depth"], single["depth"])


def test_restatement_a_face_across_the_near_plane_is_dropped_whole():
    v = np.array([[-1, -1, -2], [1, -1, -2], [0, 0.125, -0.25], [0, 0.5, 1.0]], dtype=f32)
    uv = np.zeros((1, 3, 2), dtype=f32)
    one = np.array([[0, 1, 2]], dtype=np.int32)
    assert (view_ref.view(v, one, uv, WHITE, hand_cam((9, 9), near=0.5))["face_idx"] == -1).all()    # one vertex nearer than the plane
    assert (view_ref.view(v, one, uv, WHITE, hand_cam((9, 9), near=0.25))["face_idx"] >= 0).any()    # z == -near is drawn
    behind = np.array([[0, 1, 3]], dtype=np.int32)
    for near in (0.5, 0.001):
        out = view_ref.view(v, behind, uv, WHITE, hand_cam((9, 9), near=near), background=(9, 8, 7, 6))
        assert (out["face_idx"] == -1).all() and (out["image"] == np.array([9, 8, 7, 6], dtype=np.uint8)).all()
    # a face wholly nearer than the plane, and non-finite camera coordinates
    assert not view_ref.project(v * f32(0.1), one, hand_cam((9, 9)), 9, 9)["drawn"].any()
    with np.errstate(over="ignore"):
        assert not view_ref.project(v * f32(3e38), one, hand_cam((9, 9)), 9, 9)["drawn"].any()


def test_restatement_cull_and_flip_in_both_windings():
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = (t.numpy() for t in synthetic.make_quad())
    cam = view_ref.camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 60.0, (16, 16), 0.5)
    # the side the stamp's render calls front, seen from +z
    stamp = mesh_ref.project(v, f, mesh_ref.camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0), 1.0, 16)
    assert stamp["front"].all()
    rev = f[:, [0, 2, 1]]
    covered = {}
    for name, faces in (("ccw", f), ("cw", rev)):
        for cull in (False, True):
            for flip in (False, True):
                proj = view_ref.project(v, faces, cam, 16, 16, cull, flip)
                assert (proj["A"] < 0).all() == (name == "ccw") and proj["front"].all() == ((name == "ccw") != flip)
                out = view_ref.view(v, faces, uv, WHITE, cam, cull=cull, flip_normals=flip)
                covered[name, cull, flip] = int((out["face_idx"] >= 0).sum())
    full = covered["ccw", False, False]
    assert full > 50
    for name in ("ccw", "cw"):
        assert covered[name, False, False] == covered[name, False, True] == full           # no culling: both sides are drawn
        assert covered[name, True, name == "cw"] == full and covered[name, True, name != "cw"] == 0
    # seen from behind, the same faces are back faces
    back = view_ref.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 60.0, (16, 16), 0.5)
    assert not view_ref.project(v, f, back, 16, 16)["front"].any() and view_ref.project(v, f, back, 16, 16, True, False)["drawn"].sum() == 0


def test_restatement_colour():
    """One texel of every kind under the flat quad: painted opaque, unpainted (alpha 0), and the shade of a tilted face."""
    v, f, uv = quad(FLAT)
    tex = np.zeros((2, 2, 4), dtype=np.uint8)
    tex[...] = (255, 51, 0, 255)
    out = view_ref.view(v, f, uv, tex, hand_cam((9, 9)), shade=False)
    assert (out["image"][2:7, 2:7] == np.array([255, 51, 0, 255], dtype=np.uint8)).all()
    tex[..., 3] = 0
    out = view_ref.view(v, f, uv, tex, hand_cam((9, 9)), shade=False, unpainted=(10, 128, 255), background=(1, 2, 3, 4))
    assert (out["image"][2:7, 2:7] == np.array([10, 128, 255, 255], dtype=np.uint8)).all()
    assert (out["image"][0] == np.array([1, 2, 3, 4], dtype=np.uint8)).all()
    out = view_ref.view(v, f, uv, WHITE, hand_cam((9, 9)), shade=True, ambient=0.25)       # facing the camera: |nzu| = 1
    assert (out["image"][2:7, 2:7] == 255).all()
    # a face whose normal is (3, 0, 4) / 5 in camera space: s = 0.25 + 0.75 x 0.8 = 0.85 -> 0.85 x 255 + 0.5 = 217.25
    tv = np.array([(-2, -1, -2.5), (2, -1, -5.5), (2, 1, -5.5), (-2, 1, -2.5)], dtype=f32)
    out = view_ref.view(tv, f, uv, WHITE, hand_cam((9, 9)), shade=True, ambient=0.25)
    assert np.allclose(out["proj"]["nzu"], 0.8) and set(out["image"][out["face_idx"] >= 0][:, 0].tolist()) == {217}
    out = view_ref.view(tv, f, uv, WHITE, hand_cam((9, 9)), shade=True, ambient=1.0)
    assert (out["image"][out["face_idx"] >= 0] == 255).all()


# ---------------------------------------------------------------- the rays of a frame's pixels against the frame
def test_rays_of_a_pixel_hit_the_face_the_frame_shows():
    """Both rules are exact, and a pixel whose 3 x 3 neighbourhood shows one face has its centre at least a pixel from any edge: the ray
    through that centre must hit that face.  Every such pixel is checked."""
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = (t.numpy() for t in synthetic.make_height_field(17, 13, seed=3))
    H, W = 40, 56
    cam = view_ref.camera((0.05, -0.1, 0.9), (0.0, 0.0, 0.0), (0, 1, 0), 30.0, (H, W), 0.05)  # close enough that a face spans several pixels
    out = view_ref.view(v, f, uv, WHITE, cam)
    fi = out["face_idx"]
    covered = fi >= 0
    same = np.zeros((H, W), dtype=bool)
    inner = np.ones((H - 2, W - 2), dtype=bool)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            inner &= fi[di:H - 2 + di, dj:W - 2 + dj] == fi[1:-1, 1:-1]
    same[1:-1, 1:-1] = inner & covered[1:-1, 1:-1]
    assert covered.sum() > 0.9 * H * W and same.sum() >= 0.25 * covered.sum(), (covered.sum(), same.sum())
    ii, jj = np.nonzero(same)
    o, d = view_ref.rays(cam, np.stack([jj + 0.5, ii + 0.5], axis=1))
    hits = pick_ref.pick(v, f, uv, o, d)
    wrong = np.nonzero(hits["face"] != fi[ii, jj])[0]
    assert wrong.size == 0, [(int(ii[k]), int(jj[k]), int(fi[ii[k], jj[k]]), int(hits["face"][k])) for k in wrong[:8]]
    # and the two agree on where: the hit's distance along the view direction is the frame's depth, its UV the frame's
    b = cam["m"][2, :3].astype(np.float64)
    dist = -(hits["pos"].astype(np.float64) - o.astype(np.float64)) @ b
    assert np.allclose(dist, out["depth"][ii, jj], rtol=1e-4) and np.allclose(hits["uv"], out["uv"][ii, jj], atol=1e-4)


# ---------------------------------------------------------------- the stand-alone host program
def test_host_check_program_builds_and_passes(tmp_path):
    """tools/view_host_check.cpp drives csrc/view_host.h from its own main().  Here it is built plainly and run; the sanitizer run is
    the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/view_host_check.cpp -o view_host_check && ./view_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "view_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "view_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
