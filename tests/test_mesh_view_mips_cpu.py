"""The host-only part of the mip pyramid and the trilinear-filtered view (include/dtp.h "the mip pyramid of a texture and a
trilinear-filtered view": dtp_mip_layout, the argument checks of dtp_texture_mips and dtp_mesh_view_mips that come before any device
call) against the numpy restatement (tests/mip_ref.py); the restatement itself against hand values chosen dyadic, so that every one of
them is exact; the levels the poses of the frame tests take; and the stand-alone host program tools/mip_host_check.cpp.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mip_ref
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


# ---------------------------------------------------------------- the layout
@pytest.mark.parametrize("TH,TW", [(1, 1), (1, 7), (5, 3), (64, 64), (65, 63), (96, 160), (4100, 70), (32768, 32768)])
def test_layout_equals_the_restatement(lib, TH, TW):
    from diffusiontexturepainting_amd import ops
    got, want = ops.mip_layout(TH, TW), mip_ref.layout(TH, TW)
    assert got == want, (got, want)
    n = got["levels"]
    assert 1 <= n <= 16 and (got["h"][0], got["w"][0]) == (TH, TW) and (got["h"][-1], got["w"][-1]) == (1, 1)
    assert got["bytes"] == sum(4 * h * w for h, w in zip(got["h"][1:], got["w"][1:]))
    if n > 1:
        assert got["offset"][1] == 0 and all(b - a == 4 * h * w for a, b, h, w in zip(got["offset"][1:], got["offset"][2:], got["h"][1:], got["w"][1:]))


def test_layout_by_hand_and_refusals(lib):
    from diffusiontexturepainting_amd import _lib, ops
    from diffusiontexturepainting_amd._lib import DtpError
    assert ops.mip_layout(1, 1) == dict(levels=1, h=[1], w=[1], offset=[0], bytes=0)
    assert ops.mip_layout(5, 3) == dict(levels=4, h=[5, 3, 2, 1], w=[3, 2, 1, 1], offset=[0, 0, 24, 32], bytes=36)
    assert ops.mip_layout(2048, 2048)["levels"] == 12 and ops.mip_layout(32768, 32768)["levels"] == 16
    assert ops.mip_layout(4100, 70)["levels"] == 14                    # three passes: from levels 0, 6 and 12
    out = _lib.MipLevels()
    C.memset(C.byref(out), 0x5a, C.sizeof(out))
    before = bytes(out)
    for TH, TW in ((0, 4), (4, 0), (-1, 4), (32769, 4), (4, 32769)):
        with pytest.raises(DtpError, match=r"\(code 1\).*1\.\.32768"):
            ops.mip_layout(TH, TW)
        with pytest.raises(ValueError):
            mip_ref.layout(TH, TW)
        assert lib.dtp_mip_layout(TH, TW, C.byref(out)) == ARG and bytes(out) == before  # a refused call writes nothing
    assert lib.dtp_mip_layout(4, 4, None) == ARG and "NULL" in lib.dtp_last_error().decode()


def test_header_and_binding_agree_on_the_mips(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3
    assert "the mip pyramid of a texture and a trilinear-filtered view" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mip_layout", "dtp_texture_mips", "dtp_mesh_view_mips"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    args = lambda name: len(re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(","))  # noqa: E731
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
        assert args(name) == len(_lib.SYMBOLS[name][1]), name
    m = re.search(r"typedef struct \{([^}]*)\} dtp_mip_levels;", code)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int levels; int h[16], w[16]; uint64_t offset[16]; uint64_t bytes;"
    assert [f[0] for f in _lib.MipLevels._fields_] == ["levels", "h", "w", "offset", "bytes"]
    assert C.sizeof(_lib.MipLevels) == 272 and _lib.MipLevels.offset.offset == 136 and _lib.MipLevels.bytes.offset == 264


# ---------------------------------------------------------------- the argument checks, before any device call
def test_texture_mips_refuses_before_any_device_call(lib):
    """No device here: every one of these returns from the checks, and the buffers are host memory that nothing writes."""
    tex = (C.c_uint32 * 16)()
    mips = (C.c_uint32 * 8)(*([0x5a5a5a5a] * 8))
    vp = (lambda a, off=0: C.c_void_p(C.addressof(a) + off))

    def refused(word, texture=vp(tex), TH=4, TW=4, m=vp(mips), n=20):
        rc = lib.dtp_texture_mips(texture, TH, TW, m, n, None)
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(mips) == [0x5a5a5a5a] * 8

    refused("NULL", texture=None)
    refused("NULL", m=None)
    for TH, TW in ((0, 4), (4, 0), (32769, 4), (4, 32769)):
        refused(r"1\.\.32768", TH=TH, TW=TW)
    refused("aligned", texture=vp(tex, 1))
    refused("aligned", m=vp(mips, 2))
    refused("mips_bytes", n=19)
    refused("mips_bytes", n=0)
    assert lib.dtp_texture_mips(vp(tex), 1, 1, None, 0, None) == 0  # one level: mips may be NULL and nothing is launched


def test_view_mips_refuses_before_any_device_call(lib):
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    cam = view_camera((0.3, -1.7, 2.9), (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 45.0, (360, 640), 0.05).struct()
    opts = view_opts()
    tex, mips = (C.c_uint32 * 16)(), (C.c_uint32 * 8)()
    img = (C.c_uint32 * 16)(*([0x5a5a5a5a] * 16))
    fidx, dep, lod = (C.c_int * 4)(*([7] * 4)), (C.c_float * 4)(*([7.0] * 4)), (C.c_float * 4)(*([7.0] * 4))
    not_a_mesh = (C.c_int * 64)()
    fake = C.cast(not_a_mesh, C.c_void_p)
    vp = (lambda a, off=0: C.c_void_p(C.addressof(a) + off))

    def refused(word, mesh=fake, texture=vp(tex), TH=4, TW=4, m=vp(mips), c=C.byref(cam), H=2, W=2, o=C.byref(opts), image=vp(img), f=vp(fidx),
                d=vp(dep), lo=vp(lod)):
        rc = lib.dtp_mesh_view_mips(mesh, texture, TH, TW, m, c, H, W, o, image, f, d, lo, None)
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(img) == [0x5a5a5a5a] * 16 and list(fidx) == [7] * 4 and list(dep) == [7.0] * 4 and list(lod) == [7.0] * 4

    refused("NULL", mesh=None)
    refused("NULL", texture=None)
    refused("NULL", c=None)
    refused("NULL", o=None)
    refused("NULL", image=None)
    refused("NULL.*mips", m=None)
    refused(r"1\.\.4096", H=0)
    refused(r"1\.\.4096", W=4097)
    refused(r"1\.\.32768", TH=0)
    refused(r"1\.\.32768", TW=32769)
    refused("aligned", texture=vp(tex, 1))
    refused("aligned", image=vp(img, 2))
    refused("aligned", f=vp(fidx, 1))
    refused("aligned", d=vp(dep, 3))
    refused("aligned", m=vp(mips, 2))
    refused("aligned", lo=vp(lod, 1))
    bad = view_opts()
    bad.ambient = 1.5
    refused("ambient", o=C.byref(bad))
    refused("not a live mesh")                                   # every argument in order: the look-up is what refuses
    refused("not a live mesh", f=None, d=None, lo=None)          # (the optional outputs may be absent)
    refused("not a live mesh", TH=1, TW=1, m=None)               # (one level: no pyramid to hand over)


# ---------------------------------------------------------------- the pyramid by hand
RED, NONE = (255, 0, 0, 255), (0, 0, 0, 0)


def test_pyramid_by_hand():
    block = np.array([[RED, NONE], [NONE, NONE]], dtype=np.uint8)
    assert mip_ref.next_level(block).tolist() == [[[255, 0, 0, 64]]]         # red, a quarter covered: not a dark red
    assert mip_ref.next_level(np.zeros((2, 2, 4), dtype=np.uint8)).tolist() == [[[0, 0, 0, 0]]]
    hidden = np.array([[(9, 8, 7, 0), (200, 100, 50, 0)], [(1, 2, 3, 0), (255, 255, 255, 0)]], dtype=np.uint8)
    assert mip_ref.next_level(hidden).tolist() == [[[0, 0, 0, 0]]]            # colour under alpha 0 counts for nothing
    # a 3 x 1 strip (three columns): the last texel is doubled, and so is the only row
    strip = np.array([[(10, 20, 30, 255), (30, 40, 50, 255), (7, 9, 11, 100)]], dtype=np.uint8)
    assert mip_ref.next_level(strip).tolist() == [[[20, 30, 40, 255], [7, 9, 11, 100]]]
    assert mip_ref.next_level(strip.transpose(1, 0, 2)).tolist() == [[[20, 30, 40, 255]], [[7, 9, 11, 100]]]
    # rounding: alpha (A + 2) >> 2, colour to the nearest with halves up
    two = np.array([[(3, 0, 255, 1), (4, 0, 0, 1)]], dtype=np.uint8)
    assert mip_ref.next_level(two).tolist() == [[[4, 0, 128, 1]]]             # the row counts twice, A = 4: (4 + 2) >> 2; (14 + 2) / 4; (510 + 2) / 4


def rule(texels):
    """The texel rule on four (r, g, b, a) tuples in plain Python integers."""
    A = sum(t[3] for t in texels)
    return [((sum(t[c] * t[3] for t in texels) + (A >> 1)) // A if A else 0) for c in range(3)] + [(A + 2) >> 2]


def test_pyramid_top_of_a_5_by_3_texture_by_hand():
    t = mip_ref.make_texture(5, 3, 41)
    t[0, 0, 3], t[4, 2, 3], t[2, 1, 3] = 0, 255, 3
    lv = mip_ref.pyramid(t)
    assert [x.shape[:2] for x in lv] == [(5, 3), (3, 2), (2, 1), (1, 1)]
    px = (lambda a, i, j: tuple(int(x) for x in a[min(i, a.shape[0] - 1), min(j, a.shape[1] - 1)]))
    l1 = [[rule([px(t, 2 * i, 2 * j), px(t, 2 * i, 2 * j + 1), px(t, 2 * i + 1, 2 * j), px(t, 2 * i + 1, 2 * j + 1)]) for j in range(2)] for i in range(3)]
    assert lv[1].tolist() == l1
    a1 = np.array(l1)
    l2 = [[rule([px(a1, 2 * i, 0), px(a1, 2 * i, 1), px(a1, 2 * i + 1, 0), px(a1, 2 * i + 1, 1)])] for i in range(2)]
    assert lv[2].tolist() == l2
    a2 = np.array(l2)
    assert lv[3].tolist() == [[rule([px(a2, 0, 0), px(a2, 0, 1), px(a2, 1, 0), px(a2, 1, 1)])]]
    assert lv[3][0, 0, 3] > 0
    packed = mip_ref.pack(lv)
    lay = mip_ref.layout(5, 3)
    assert packed.size == lay["bytes"] and packed[lay["offset"][2]:lay["offset"][2] + 8].tolist() == lv[2].reshape(-1).tolist()


# ---------------------------------------------------------------- the level rule on make_quad() seen head-on
def quad():
    from diffusiontexturepainting_amd import synthetic
    return [t.numpy() for t in synthetic.make_quad()]


@pytest.mark.parametrize("side,lod", [(8, 0.0), (16, 1.0), (32, 2.0)])
def test_level_rule_whole_levels(side, lod):
    """Eye at distance 2, 90 degrees, 16 x 16: a pixel is 1/4 world units = 1/8 of the UV square, so side / 8 texels per pixel.  UV is
    affine on the screen, so the difference to the neighbouring centre is exact."""
    cam = view_ref.camera((0, 0, 2), (0, 0, 0), (0, 1, 0), 90.0, (16, 16), 0.5)
    assert (cam["fx"], cam["fy"]) == (1, 1)
    tex = mip_ref.make_texture(side, side, 5)
    out = mip_ref.view(*quad(), tex, cam)
    inside = out["face_idx"] >= 0
    assert inside.sum() == 64 and inside[4:12, 4:12].all()
    assert set(out["rho2"][inside].tolist()) == {(side / 8) ** 2} and set(out["lod"][inside].tolist()) == {lod}
    assert (out["lod"][~inside] == 0).all() and not out["horizon"].any()
    plain = view_ref.view(*quad(), tex, cam)
    assert np.array_equal(out["face_idx"], plain["face_idx"]) and np.array_equal(out["depth"], plain["depth"])
    if side == 8:
        assert np.array_equal(out["image"], plain["image"])       # rho = 1: the unfiltered frame byte for byte
    else:
        assert not np.array_equal(out["image"], plain["image"])
        level = mip_ref.pyramid(tex)[int(lod)]                   # f = 0: the frame is level l's own unfiltered frame
        assert np.array_equal(out["image"], view_ref.view(*quad(), level, cam)["image"])


def test_level_rule_half_way():
    """rho^2 = 2.5 = 1.5^2 + 0.5^2: a hand-made camera, rolled by 45 degrees and scaled by sqrt 2 (rows (1, 1, 0) and (-1, 1, 0)), at
    distance 4 on 16 x 16: a pixel step is 1/2 in camera space = (1/4, 1/4) in the quad's plane = (1/8, 1/8) in UV, on a 4 x 12
    texture (1.5, 0.5) texels.  f = (2.5 - 1) / 3."""
    cam = dict(m=np.array([[1, 1, 0, 0], [-1, 1, 0, 0], [0, 0, 1, -4]], dtype=f32), fx=f32(1), fy=f32(1), near=f32(0.5), size=(16, 16))
    tex = mip_ref.make_texture(4, 12, 5)
    tex[..., 3] = np.maximum(tex[..., 3], 1)
    out = mip_ref.view(*quad(), tex, cam, shade=False)
    inside = out["face_idx"] >= 0
    assert inside.sum() == 32
    assert set(out["rho2"][inside].tolist()) == {2.5} and set(out["lod"][inside].tolist()) == {0.5} and set(out["level"][inside].tolist()) == {0}
    lv = mip_ref.pyramid(tex)
    lo, hi = mip_ref.sample(lv[0], out["uv"][..., 0], out["uv"][..., 1]), mip_ref.sample(lv[1], out["uv"][..., 0], out["uv"][..., 1])
    t = lo + (hi - lo) * f32(0.5)
    unp = f32(128) / f32(255)
    want = (np.fmin(t[..., :3] * t[..., 3:4] + unp * (f32(1) - t[..., 3:4]), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)
    assert np.array_equal(out["image"][inside][:, :3], want[inside])


def test_filtered_checkerboard_is_one_grey():
    """Black and white opaque texels, two of each in every 2 x 2 block (the phase alternates from block to block, so that texels two apart
    alternate as well).  Distance 4 on 32 x 32: 2 texels of 16 per pixel, and the eye is moved by 1/16 so that the unfiltered taps fall on
    texel centres: the unfiltered frame shows single texels, black or white; the filtered one shows level 1, which is one grey."""
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    tex = np.zeros((16, 16, 4), dtype=np.uint8)
    tex[..., 3] = 255
    tex[(i + j + i // 2 + j // 2) % 2 == 0, :3] = 255
    assert (mip_ref.next_level(tex) == np.array([128, 128, 128, 255], dtype=np.uint8)).all()
    cam = view_ref.camera((1 / 16, 1 / 16, 4), (1 / 16, 1 / 16, 0), (0, 1, 0), 90.0, (32, 32), 0.5)
    out, plain = mip_ref.view(*quad(), tex, cam), view_ref.view(*quad(), tex, cam)
    inside = out["face_idx"] >= 0
    assert inside.sum() == 64 and set(out["lod"][inside].tolist()) == {1.0}
    assert (out["image"][inside] == np.array([128, 128, 128, 255], dtype=np.uint8)).all()
    values, counts = np.unique(plain["image"][inside][:, :3], return_counts=True)
    assert values.tolist() == [0, 255] and counts.min() >= 3 * 16


# ---------------------------------------------------------------- beyond the horizon
def test_beyond_the_horizon_branch():
    v, f, uv = mip_ref.TRIANGLE
    eye, at, fov, size, near = mip_ref.TRIANGLE_POSE
    tex, lv = mip_ref.texture("atlas")
    under = mip_ref.view(v, f, uv, tex, view_ref.camera(eye, at, (0, -1, 0), fov, size, near), levels=lv)
    covered = under["face_idx"] >= 0
    assert covered.sum() == 32 and under["horizon"][covered].all()                 # every covered pixel takes the branch
    assert set(under["lod"][covered].tolist()) == {float(len(lv) - 1)} and (under["f"] == 0).all()
    assert len({tuple(p) for p in under["image"][covered].tolist()}) == 1          # the 1 x 1 level: one colour (the face is flat)
    assert lv[-1][0, 0, 3] > 0
    over = mip_ref.view(v, f, uv, tex, view_ref.camera(eye, at, (0, 1, 0), fov, size, near), levels=lv)
    covered = over["face_idx"] >= 0
    assert covered.sum() == 32 and not over["horizon"].any()
    assert [int((over["level"] == k).sum()) for k in range(len(lv))] == [4, 6, 10, 12, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------- the levels the poses of the frame tests take
@pytest.mark.parametrize("name", sorted(mip_ref.POSES))
def test_pose_takes_its_levels(name):
    out = mip_ref.pose_reference(name)
    tex = mip_ref.POSES[name][0]
    L = len(mip_ref.texture(tex)[1])
    assert [int((out["level"] == k).sum()) for k in range(L)] == mip_ref.POSES[name][6]
    covered = out["face_idx"] >= 0
    assert (out["lod"][covered] >= out["level"][covered]).all() and (out["lod"][covered] < out["level"][covered] + 1).all()
    assert ((out["f"] > 0) == (out["lod"] != np.floor(out["lod"]))).all()


def test_poses_cover_the_rule():
    """A condition on the inputs: every level of both textures is taken by some pixel, and most pixels blend two levels."""
    for tex in mip_ref.TEXTURES:
        L = len(mip_ref.texture(tex)[1])
        names = [n for n in mip_ref.POSES if mip_ref.POSES[n][0] == tex]
        taken = np.sum([mip_ref.POSES[n][6] for n in names], axis=0)
        assert len(taken) == L and (taken > 0).all(), (tex, taken)
    covered = sum(int((mip_ref.pose_reference(n)["face_idx"] >= 0).sum()) for n in mip_ref.POSES)
    blended = sum(int((mip_ref.pose_reference(n)["f"] > 0).sum()) for n in mip_ref.POSES)
    assert covered > 3000 and 2 * blended >= covered, (covered, blended)
    # a magnified pose is the unfiltered frame, byte for byte
    tex, eye, at, up, fov, near = mip_ref.MAGNIFIED
    t, lv = mip_ref.texture(tex)
    mesh = [m.numpy() for m in mip_ref.field()]
    cam = view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near)
    out = mip_ref.view(*mesh, t, cam, levels=lv)
    assert (out["face_idx"] >= 0).sum() > 1000 and (out["lod"] == 0).all()
    assert np.array_equal(out["image"], view_ref.view(*mesh, t, cam)["image"])


# ---------------------------------------------------------------- the stand-alone host program
def test_host_check_program_builds_and_passes(tmp_path):
    """tools/mip_host_check.cpp drives csrc/mips_host.h from its own main().  Here it is built plainly and run; the sanitizer run is
    the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/mip_host_check.cpp -o mip_host_check && ./mip_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "mip_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "mip_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
