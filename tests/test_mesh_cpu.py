"""The host-only part of the mesh strokes (include/dtp.h: dtp_mesh_camera, dtp_mesh_create's argument checks) and the reference the GPU
tests use (tests/mesh_ref.py) against the 2D stroke reference it must agree with on a full-window quad.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref
import stroke_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# pos, normal, prev, fov
POSES = {
    "axis_z": ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0),
    "axis_x_offset": ((2, -3, 5), (1, 0, 0), (2, -3, 7), 0.25),
    "axis_minus_y_long_normal": ((0.5, 0.25, -8), (0, -3, 0), (1.5, 0.25, -8), 7.0),
    "oblique": ((0.3, -1.7, 2.9), (0.2, 0.5, 0.84), (0.1, -1.2, 2.6), 0.37),
    "oblique_far_from_the_origin": ((1234.5, -987.25, 400.125), (-0.6, 0.1, 0.79), (1230.0, -980.0, 401.0), 12.5),
    "prev_not_perpendicular_to_the_normal": ((0, 0, 0), (0, 0, 1), (1, 2, 3), 1.0),
    "prev_nearly_along_the_normal": ((1, 1, 1), (0.3, 0.4, 0.5), (1.31, 1.4, 1.52), 0.01),
}


@pytest.mark.parametrize("name", sorted(POSES))
def test_camera_equals_the_restatement(lib, name):
    from diffusiontexturepainting_amd.mesh import mesh_camera
    pos, normal, prev, fov = POSES[name]
    got = mesh_camera(pos, normal, prev, fov).numpy()
    want = mesh_ref.camera(pos, normal, prev, fov)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert (got == want).all(), (got, want)
    # it is a rigid look-at: orthonormal rows, the brush position on the axis at distance |normal|, prev - pos above it
    rot = got[:, :3].astype(np.float64)
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-6)
    p = rot @ np.asarray(pos, dtype=np.float64) + got[:, 3]
    scale = max(1.0, float(np.abs(np.asarray(pos)).max()))
    assert np.allclose(p, [0, 0, -math.sqrt(sum(x * x for x in normal))], atol=2e-6 * scale)
    up = rot @ (np.asarray(prev, dtype=np.float64) - np.asarray(pos, dtype=np.float64))
    assert abs(up[0]) < 1e-5 * np.abs(up).max() and up[1] > 0


def test_axis_aligned_camera_by_hand(lib):
    from diffusiontexturepainting_amd.mesh import mesh_camera
    got = mesh_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0)
    assert torch.equal(got, torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -1]]))


@pytest.mark.parametrize("pos,normal,prev,fov,word", [
    ((0, 0, 0), (0, 0, 0), (0, 1, 0), 1.0, "normal is zero"),
    ((0, 0, 0), (0.3, 0.5, 0.7), (0.6, 1.0, 1.4), 1.0, "parallel"),
    ((1, 2, 3), (0, 0, 1), (1, 2, 3), 1.0, "zero or parallel"),
    ((0, 0, float("nan")), (0, 0, 1), (0, 1, 0), 1.0, "non-finite"),
    ((0, 0, 0), (0, float("inf"), 1), (0, 1, 0), 1.0, "non-finite"),
    ((0, 0, 0), (0, 0, 1), (0, 1, 0), 0.0, "fov"),
    ((0, 0, 0), (0, 0, 1), (0, 1, 0), -2.0, "fov"),
    ((0, 0, 0), (0, 0, 1), (0, 1, 0), float("nan"), "fov"),
])
def test_camera_refusals(lib, pos, normal, prev, fov, word):
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.mesh import mesh_camera
    with pytest.raises(DtpError, match=rf"\(code {ARG}\).*{word}"):
        mesh_camera(pos, normal, prev, fov)
    with pytest.raises(ValueError):
        mesh_ref.camera(pos, normal, prev, fov)
    out = (C.c_float * 12)(*([9.0] * 12))
    v = [(C.c_float * 3)(*x) for x in (pos, normal, prev)]
    assert lib.dtp_mesh_camera(C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.c_float(fov), C.byref(out)) == ARG
    assert list(out) == [9.0] * 12  # a refused call writes nothing
    assert lib.dtp_mesh_camera(None, C.byref(v[1]), C.byref(v[2]), C.c_float(1.0), C.byref(out)) == ARG


def test_mesh_create_refuses_bad_data_before_any_device_call(lib):
    """Every data check precedes the first HIP call (and the look at ctx), so it runs without a device: with ctx = NULL."""
    verts = (C.c_float * 12)(0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0)
    faces = (C.c_int * 6)(0, 1, 2, 0, 2, 3)
    uvs = (C.c_float * 12)(0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1)
    out = C.c_void_p(0)

    def refused(rc, word):
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert not out.value

    vp = (lambda a: C.cast(a, C.c_void_p))
    refused(lib.dtp_mesh_create(None, None, 4, vp(faces), 2, vp(uvs), C.byref(out)), "NULL")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, None, 2, vp(uvs), C.byref(out)), "NULL")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(faces), 2, None, C.byref(out)), "NULL")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(faces), 2, vp(uvs), None), "NULL")
    refused(lib.dtp_mesh_create(None, vp(verts), 0, vp(faces), 2, vp(uvs), C.byref(out)), "V=0")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(faces), 0, vp(uvs), C.byref(out)), "F=0")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(faces), (1 << 20) + 1, vp(uvs), C.byref(out)), "F=1048577")
    refused(lib.dtp_mesh_create(None, vp(verts), 3, vp(faces), 2, vp(uvs), C.byref(out)), r"face 1 refers to vertex 3 \(0\.\.2\)")
    bad = (C.c_int * 6)(0, 1, 2, 0, -1, 3)
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(bad), 2, vp(uvs), C.byref(out)), r"face 1 refers to vertex -1")
    nan_uv = (C.c_float * 12)(*uvs)
    nan_uv[7] = float("nan")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(faces), 2, vp(nan_uv), C.byref(out)), r"face 1 has a UV")
    inf_v = (C.c_float * 12)(*verts)
    inf_v[8] = float("inf")
    refused(lib.dtp_mesh_create(None, vp(inf_v), 4, vp(faces), 2, vp(uvs), C.byref(out)), r"vertex 2 is not finite")
    refused(lib.dtp_mesh_create(None, vp(verts), 4, vp(faces), 2, vp(uvs), C.byref(out)), "ctx is NULL")
    # destroying nothing is fine
    assert lib.dtp_mesh_destroy(None) == 0


def test_header_and_binding_agree_on_the_mesh_entry_points(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr)
    assert lib.dtp_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mesh_create", "dtp_mesh_destroy", "dtp_mesh_camera", "dtp_mesh_stroke", "dtp_op_mesh_render", "dtp_op_mesh_backproject"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new | {"dtp_last_stroke_info"}:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
    assert [f[0] for f in _lib.MeshStamp._fields_] == ["pos", "normal", "prev", "fov", "mode", "slot", "seed"]
    assert C.sizeof(_lib.MeshStamp) == 56 and _lib.MeshStamp.seed.offset == 48 and _lib.MeshStamp.fov.offset == 36
    assert [f[0] for f in _lib.MeshStrokeOpts._fields_] == ["flip_normals", "margin", "over_y", "over_x", "sample_vae", "strength"]
    assert C.sizeof(_lib.MeshStrokeOpts) == 32 and _lib.MeshStrokeOpts.strength.offset == 24
    m = re.search(r"typedef struct \{([^}]*)\} dtp_mesh_stamp;", code)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "float pos[3], normal[3], prev[3], fov; int mode, slot; uint64_t seed;"
    m = re.search(r"typedef struct \{([^}]*)\} dtp_mesh_stroke_opts;", code)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int flip_normals, margin, over_y, over_x, sample_vae; double strength;"


# ---------------------------------------------------------------- the reference against the 2D reference
def test_the_full_window_quad_ties_the_mesh_contract_to_the_2d_one():
    """Two faces with vertices at NDC +-1 and the unit square as UVs, a 64 x 64 texture, R = 64: the powers of two make every
    barycentric weight exact, so the render IS the window at (0, 0) and the backprojection IS the 2D paste."""
    from diffusiontexturepainting_amd import synthetic
    R = 64
    tex = torch.randint(0, 256, (R, R, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    tex[5:20, 9:40, 3] = 0
    v, f, uv = synthetic.make_quad()
    cam = mesh_ref.camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0)
    for mode in (mesh_ref.INPAINT, mesh_ref.OVERPAINT):
        canvas, face_idx, proj = mesh_ref.render(v, f, uv, cam, 1.0, tex, R, mode=mode, over=(10, 25))
        assert torch.equal(canvas, stroke_ref.gather(tex, 0, 0, R, False, mode, (10, 25)))
        assert int((face_idx < 0).sum()) == 0 and set(face_idx.unique().tolist()) == {0, 1}
    dec = torch.randn(R, R, 4, generator=torch.Generator().manual_seed(5)) * 0.9
    dec[0, :8, :] = torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, 1.0 - 2.0 ** -23, -1.0 + 2.0 ** -23, 255.0 / 256])[:, None]
    for mask in (stroke_ref.make_stamp_mask(R, 3), stroke_ref.disc_mask(R)):
        got, info = mesh_ref.backproject(proj, face_idx, uv, dec, mask, tex)
        assert torch.equal(got, stroke_ref.paste(tex.clone(), stroke_ref.decoded_to_u8(dec), mask, 0, 0))
        assert info["valid"].all() and not torch.equal(got, tex)
        got, _ = mesh_ref.backproject(proj, face_idx, uv, None, mask, tex)
        assert torch.equal(got, stroke_ref.paste(tex.clone(), None, mask, 0, 0, mode=stroke_ref.ERASE))


def test_reference_coverage_owns_every_centre_on_a_shared_edge_once():
    """A 4 x 4 grid of squares whose vertices sit ON pixel centres: every interior centre lies on an edge or a vertex of several
    faces; the top-left rule gives it to exactly one, in both windings."""
    R = 8
    xs = np.arange(5, dtype=np.int64) * 512 + 128  # centres 0, 2, 4, 6, 8 (the last outside the window)
    py, px = np.meshgrid(np.arange(R, dtype=np.int64) * 256 + 128, np.arange(R, dtype=np.int64) * 256 + 128, indexing="ij")
    for flip in (False, True):
        count = np.zeros((R, R), dtype=np.int64)
        for j in range(4):
            for i in range(4):
                a, b, c, d = (xs[i], xs[j]), (xs[i + 1], xs[j]), (xs[i + 1], xs[j + 1]), (xs[i], xs[j + 1])
                for tri in ((a, b, c), (a, c, d)):
                    tri = tri[::-1] if flip else tri
                    X, Y = np.array([p[0] for p in tri]), np.array([p[1] for p in tri])
                    inside, w = mesh_ref.cover(X, Y, px, py)
                    count += inside
                    assert np.allclose(w[inside].sum(axis=-1), 1.0, atol=1e-6)
        assert (count == 1).all()
