"""The host-only part of face sets (include/dtp.h "face sets: a lasso, masked strokes, a tint") and the reference the GPU
tests use (tests/select_ref.py): the numpy lasso against an independent evaluation in exact rationals, the packing of a set, every
refusal that needs no device, the masked backprojection of the reference against the unmasked one, and the stand-alone host program
tools/select_host_check.cpp.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_ref
import select_ref
import stroke_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
H, W = 10, 13


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------- the lasso against exact rationals
def inside_rational(polygon, h, w):
    """The rule of include/dtp.h evaluated with fractions.Fraction in pixel units: the vertices are the snapped ones over 256, the centre of
    pixel (i, j) is (j + 1/2, i + 1/2), an edge counts iff it crosses the centre's row (half-open in y) and the centre is strictly left
    of the crossing x = a.x + (P.y - a.y)(b.x - a.x) / (b.y - a.y)."""
    v = [(Fraction(int(x), 256), Fraction(int(y), 256)) for x, y in select_ref.snap_polygon(polygon)]
    out = np.zeros((h, w), dtype=bool)
    for i in range(h):
        for j in range(w):
            px, py = Fraction(2 * j + 1, 2), Fraction(2 * i + 1, 2)
            count = 0
            for k in range(len(v)):
                (ax, ay), (bx, by) = v[k], v[(k + 1) % len(v)]
                if (ay > py) != (by > py) and px < ax + (py - ay) * (bx - ax) / (by - ay):
                    count += 1
            out[i, j] = count % 2 == 1
    return out


def random_polygon(seed, n, on_grid):
    g = np.random.default_rng(seed)
    if on_grid:  # half-pixel coordinates: many centres on edges and vertices
        return g.integers(-4, 2 * max(H, W) + 4, size=(n, 2)).astype(np.float32) * np.float32(0.5)
    return (g.random((n, 2)) * [W + 6, H + 6] - 3).astype(np.float32)


BIG = float(1 << 26) / 256  # a coordinate beyond it is clamped
POLYGONS = {
    "random_3": random_polygon(1, 3, False),
    "random_7": random_polygon(2, 7, False),
    "random_23": random_polygon(3, 23, False),
    "random_grid_5": random_polygon(4, 5, True),
    "random_grid_12": random_polygon(5, 12, True),
    "random_grid_40": random_polygon(6, 40, True),
    "vertex_on_a_centre": [(2.5, 1.5), (9.5, 3.5), (4.5, 7.5)],
    "horizontal_edge_through_a_row_of_centres": [(1.0, 2.5), (11.0, 2.5), (6.0, 9.0)],
    "rectangle_with_corners_on_centres": [(2.5, 3.5), (6.5, 3.5), (6.5, 5.5), (2.5, 5.5)],
    "bow_tie": [(0.0, 0.0), (8.0, 8.0), (8.0, 0.0), (0.0, 8.0)],
    "outside_the_frame": [(20.0, 3.0), (30.0, 3.0), (25.0, 9.0)],
    "clamped_covers_the_frame": [(-2 * BIG, -3 * BIG), (4 * BIG, -3 * BIG), (4 * BIG, 2 * BIG), (-2 * BIG, 2 * BIG)],
    "clamped_sliver": [(-1e30, 4.0), (1e30, 4.2), (3e38, 6.0), (-3e38, 5.0)],
    "inside_one_pixel_around_no_centre": [(3.6, 3.6), (3.9, 3.6), (3.9, 3.9)],
}


@pytest.mark.parametrize("name", sorted(POLYGONS))
def test_the_numpy_lasso_equals_the_rational_evaluation(name):
    poly = POLYGONS[name]
    got = select_ref.inside(select_ref.snap_polygon(poly), H, W)
    assert got.dtype == bool and got.shape == (H, W)
    assert (got == inside_rational(poly, H, W)).all()
    n = int(got.sum())
    if name.startswith("random"):
        assert 0 < n < H * W
    if name == "rectangle_with_corners_on_centres":  # the left column and the top row are in, the right and the bottom are not
        want = np.zeros((H, W), dtype=bool)
        want[3:5, 2:6] = True
        assert (got == want).all()
    if name == "horizontal_edge_through_a_row_of_centres":  # the row ON the edge is in (a.y > P.y is false for it, b.y > P.y below it true)
        assert got[2, 1:11].all() and not got[1].any()
    if name == "vertex_on_a_centre":
        assert n > 5
    if name == "bow_tie":
        assert got[4, 0] and got[3, 7] and not got[0, 4] and not got[7, 3]
    if name in ("outside_the_frame", "inside_one_pixel_around_no_centre"):
        assert n == 0
    if name == "clamped_covers_the_frame":
        assert n == H * W
        xy = select_ref.snap_polygon(poly)
        assert int(np.abs(xy).max()) == 1 << 26 and int(np.abs(xy).min()) == 1 << 26
    if name == "clamped_sliver":
        assert got[4, :].all() and not got[3, :].any() and not got[6, :].any()


def test_hit_faces_skips_what_is_no_face_of_the_mesh():
    face_idx = np.full((H, W), -1, dtype=np.int32)
    face_idx[3, 2], face_idx[3, 3], face_idx[4, 2], face_idx[4, 5] = 49, 50, -7, 2 ** 31 - 1
    face_idx[8, 8] = 3  # outside the polygon
    rect = POLYGONS["rectangle_with_corners_on_centres"]
    assert np.nonzero(select_ref.hit_faces(face_idx, rect, 50))[0].tolist() == [49]
    before = np.zeros(50, dtype=bool)
    before[[3, 49]] = True
    assert np.nonzero(select_ref.select(face_idx, rect, 50, "add", before))[0].tolist() == [3, 49]
    assert np.nonzero(select_ref.select(face_idx, rect, 50, "subtract", before))[0].tolist() == [3]
    assert np.nonzero(select_ref.select(face_idx, rect, 50, "replace", before))[0].tolist() == [49]


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("F", [1, 32, 33, 50])
def test_pack_and_unpack_round_trip(F):
    from diffusiontexturepainting_amd import mesh
    g = torch.Generator().manual_seed(F)
    for mask in (torch.rand(F, generator=g) < 0.5, torch.ones(F, dtype=torch.bool), torch.zeros(F, dtype=torch.bool)):
        sel = mesh.faceset_from_bool(mask)
        assert sel.dtype == torch.int32 and tuple(sel.shape) == ((F + 31) // 32,)
        assert torch.equal(sel, select_ref.pack(mask.numpy()))
        assert torch.equal(mesh.faceset_to_bool(sel, F), mask)
        assert (select_ref.unpack(sel, F) == mask.numpy()).all()
        # the complement carries stray high bits in its last word; they are dropped
        inv = ~sel
        assert torch.equal(mesh.faceset_to_bool(inv, F), ~mask) and (select_ref.unpack(inv, F) == ~mask.numpy()).all()
        if F % 32:
            assert int(inv[-1]) >> (F % 32) != 0
        for f in range(F):  # the layout itself: bit f % 32 of word f // 32
            assert bool((int(sel[f // 32]) >> (f % 32)) & 1) == bool(mask[f])
    assert torch.equal(mesh.faceset_empty(F, "cpu"), torch.zeros((F + 31) // 32, dtype=torch.int32))
    assert torch.equal(mesh.faceset_from_bool(torch.ones(F, dtype=torch.bool)) & mesh.faceset_empty(F, "cpu"), mesh.faceset_empty(F, "cpu"))


# ---------------------------------------------------------------- refusals, before any device call
def test_select_refuses_bad_polygons_before_any_device_call(lib):
    """The polygon, the op and the frame's size are checked before the mesh is looked at, so the checks run without a device: with
    mesh = NULL, which a good polygon then meets."""
    good = (C.c_float * 8)(1, 1, 9, 1, 9, 7, 1, 7)
    many = (C.c_float * (2 * 1025))(*([1.0] * (2 * 1025)))

    def refused(rc, word):
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())

    vp = (lambda a: C.cast(a, C.c_void_p))
    refused(lib.dtp_mesh_select(None, None, H, W, vp(good), 2, 0, None, 1, None), r"n=2 vertices \(3\.\.1024\)")
    refused(lib.dtp_mesh_select(None, None, H, W, vp(many), 1025, 0, None, 1, None), r"n=1025 vertices \(3\.\.1024\)")
    refused(lib.dtp_mesh_select(None, None, H, W, vp(good), 0, 0, None, 1, None), r"n=0")
    for k, value in ((0, float("nan")), (5, float("inf")), (6, float("-inf"))):
        bad = (C.c_float * 8)(*good)
        bad[k] = value
        refused(lib.dtp_mesh_select(None, None, H, W, vp(bad), 4, 0, None, 1, None), rf"vertex {k // 2} of the polygon is not finite")
    refused(lib.dtp_mesh_select(None, None, H, W, vp(good), 4, 3, None, 1, None), r"unknown op 3")
    refused(lib.dtp_mesh_select(None, None, H, W, vp(good), 4, -1, None, 1, None), r"unknown op -1")
    refused(lib.dtp_mesh_select(None, None, 0, W, vp(good), 4, 0, None, 1, None), r"0 x 13 frame")
    refused(lib.dtp_mesh_select(None, None, H, 4097, vp(good), 4, 0, None, 1, None), r"10 x 4097 frame")
    refused(lib.dtp_mesh_select(None, None, H, W, None, 4, 0, None, 1, None), r"NULL")
    refused(lib.dtp_mesh_select(None, None, H, W, vp(good), 4, 0, None, 1, None), r"NULL")  # a good polygon: now the pointers
    # the masked stroke and the tint look at their handles first: NULL
    refused(lib.dtp_mesh_stroke_masked(None, None, None, 8, 8, None, 1, None, None, None, 0, None, 1, None), r"NULL")
    refused(lib.dtp_op_mesh_backproject_masked(None, None, 0, None, None, 64, None, 8, 8, None, 1, None), r"NULL")
    refused(lib.dtp_view_tint(None, None, None, 8, 8, None, 1, 8, None, 128, None), r"NULL")


def test_a_face_set_of_the_wrong_kind_is_refused_before_any_device_call():
    """What paint_mesh_stroke, paint_mesh_path, ops.mesh_backproject, select_faces(out=) and the tint check of a face set, in the order
    they check it; the device of this test is one the tensor is not on."""
    from diffusiontexturepainting_amd import mesh
    F = 50
    good = mesh.faceset_empty(F, "cpu")
    assert mesh.faceset_check(good, F, "cpu") is good
    with pytest.raises(ValueError, match="int32"):
        mesh.faceset_check(good.to(torch.int64), F, "cpu")
    with pytest.raises(ValueError, match="int32"):
        mesh.faceset_check(torch.zeros(F, dtype=torch.bool), F, "cpu")
    with pytest.raises(ValueError, match="int32"):
        mesh.faceset_check([0, 0], F, "cpu")
    with pytest.raises(ValueError, match=r"2 words for 50 faces"):
        mesh.faceset_check(torch.zeros(3, dtype=torch.int32), F, "cpu")
    with pytest.raises(ValueError, match=r"2 words for 50 faces"):
        mesh.faceset_check(torch.zeros(1, dtype=torch.int32), F, "cpu")
    with pytest.raises(ValueError, match=r"2 words for 50 faces"):
        mesh.faceset_check(torch.zeros(1, 2, dtype=torch.int32), F, "cpu")
    with pytest.raises(ValueError, match=r"cuda:0.*it is on cpu"):
        mesh.faceset_check(good, F, "cuda:0")
    with pytest.raises(ValueError, match="contiguous"):
        mesh.faceset_check(torch.zeros(4, dtype=torch.int32)[::2], F, "cpu")
    with pytest.raises(ValueError, match="bool"):
        mesh.faceset_from_bool(torch.zeros(F, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"int32 \[2\]"):
        mesh.faceset_to_bool(torch.zeros(3, dtype=torch.int32), F)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        mesh.lasso_polygon([1.0, 2.0, 3.0])


def test_header_and_binding_agree_on_the_face_set_entry_points(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mesh_select", "dtp_mesh_stroke_masked", "dtp_op_mesh_backproject_masked", "dtp_view_tint"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
    for name, value in _lib.SELECT_OPS.items():
        assert re.search(rf"#define\s+DTP_SELECT_{name.upper()}\s+{value}\b", hdr)
    assert lib.dtp_abi_version() == 3


def test_host_check_program_builds_and_passes(tmp_path):
    """tools/select_host_check.cpp drives csrc/select_host.h from its own main().  Here it is built plainly and run; the sanitizer run is
    the same program, built and run by hand (never from pytest, never with a preload):
        c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \\
            tools/select_host_check.cpp -o select_host_check && ./select_host_check
    """
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "select_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "diffusiontexturepainting_amd", "csrc"),
                        os.path.join(ROOT, "tools", "select_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the masked backprojection of the reference
R, TEX = 64, 128


@pytest.fixture(scope="module")
def field():
    """The 50-face height field seen whole: the render, and the unmasked backprojection of a seeded stamp into a 128^2 texture."""
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = synthetic.make_height_field(6, 6)
    assert f.shape[0] == 50
    tex = torch.randint(0, 256, (TEX, TEX, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(21))
    dec = torch.randn(R, R, 4, generator=torch.Generator().manual_seed(22)) * 0.9
    cam = mesh_ref.camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.1)
    _, face_idx, proj = mesh_ref.render(v, f, uv, cam, 1.1, tex, R)
    mask = stroke_ref.make_stamp_mask(R, 1)
    plain, info = mesh_ref.backproject(proj, face_idx, uv, dec, mask, tex)
    assert int(info["valid"].sum()) > 20 and int(info["written"].sum()) > 1000
    return dict(uv=uv, tex=tex, dec=dec, face_idx=face_idx, proj=proj, mask=mask, plain=plain, info=info)


def field_masks():
    F = 50
    every_other = np.arange(F) % 2 == 0
    chart = np.zeros(F, dtype=bool)  # make_height_field(6, 6): the faces left of the middle column are the first chart
    for j in range(5):
        chart[2 * (5 * j): 2 * (5 * j + 2)] = True
    return {"empty": np.zeros(F, dtype=bool), "all": np.ones(F, dtype=bool), "every_other": every_other, "one_chart": chart,
            "one_face": np.arange(F) == 24}


@pytest.mark.parametrize("name", sorted(field_masks()))
@pytest.mark.parametrize("erase", [False, True])
def test_masked_backprojection_is_the_unmasked_one_on_the_selected_faces(field, name, erase):
    sel = field_masks()[name]
    dec = None if erase else field["dec"]
    plain = mesh_ref.backproject(field["proj"], field["face_idx"], field["uv"], dec, field["mask"], field["tex"])[0] if erase else field["plain"]
    upright_before = field["proj"]["upright"].copy()
    got, info = select_ref.backproject(field["proj"], field["face_idx"], field["uv"], dec, field["mask"], field["tex"], sel)
    assert (field["proj"]["upright"] == upright_before).all()  # the shared reference is left unchanged
    # the UV charts of this mesh do not overlap: a texel has one covering face, so its winner is selected or the texel is left alone
    winner = field["info"]["tex_face"]
    chosen = torch.from_numpy((winner >= 0) & sel[np.where(winner >= 0, winner, 0)])
    want = torch.where(chosen[..., None], plain, field["tex"])
    assert torch.equal(got, want)
    assert (info["valid"] == (field["info"]["valid"] & sel)).all()
    written = int(info["written"].sum())
    if name == "empty":
        assert torch.equal(got, field["tex"]) and written == 0
    elif name == "all":
        assert torch.equal(got, plain) and written == int(field["info"]["written"].sum())
    else:
        assert 0 < written < int(field["info"]["written"].sum())
    if name == "one_chart":  # the first chart lies in u < 0.5: nothing right of the middle of the texture changes
        assert torch.equal(got[:, TEX // 2:], field["tex"][:, TEX // 2:]) and not torch.equal(got[:, :TEX // 2], field["tex"][:, :TEX // 2])


# ---------------------------------------------------------------- the tint of the reference, by hand
def test_the_reference_tint_by_hand():
    frame = torch.tensor([[[0, 255, 100, 7], [10, 20, 30, 40]], [[200, 200, 200, 255], [1, 2, 3, 4]]], dtype=torch.uint8)
    face_idx = torch.tensor([[0, 1], [-1, 2]], dtype=torch.int32)
    sel = np.array([True, False, True])
    got = select_ref.tint(frame, face_idx, sel, color=(255, 160, 0), opacity=128)
    # (0 * 127 + 255 * 128 + 127) // 255 = 128; (255 * 127 + 160 * 128 + 127) // 255 = 207; (100 * 127 + 0 + 127) // 255 = 50
    assert got[0, 0].tolist() == [128, 207, 50, 7]
    assert got[0, 1].tolist() == [10, 20, 30, 40] and got[1, 0].tolist() == [200, 200, 200, 255]
    assert got[1, 1].tolist() == [(1 * 127 + 255 * 128 + 127) // 255, (2 * 127 + 160 * 128 + 127) // 255, (3 * 127 + 127) // 255, 4]
    assert torch.equal(select_ref.tint(frame, face_idx, sel, opacity=0), frame)
    full = select_ref.tint(frame, face_idx, sel, color=(9, 8, 7), opacity=255)
    assert full[0, 0].tolist() == [9, 8, 7, 7] and full[1, 1].tolist() == [9, 8, 7, 4] and full[0, 1].tolist() == [10, 20, 30, 40]
