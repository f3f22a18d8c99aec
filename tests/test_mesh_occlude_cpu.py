"""The host-only part of the occlusion test of the backprojection (include/dtp.h "occlusion in the backprojection") and
the reference the GPU tests use (tests/mesh_occlude_ref.py): the table scene, where the answer is known from the geometry; the plain
reference byte for byte with the option off; the count of rejected taps on the smooth height field, on which the GPU identity test
rests; header against binding; and every refusal that needs no device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_occlude_ref as occ
import mesh_ref
import stroke_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
R, TEX = 32, 64
STRAIGHT = ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0)            # pos, normal, prev, fov: from straight above, the window is the floor
TILTED = ((0, 0, 0), (0.3, -0.2, 0.9), (0, 1, 0.1), 1.0)
POSES = {"straight": STRAIGHT, "tilted": TILTED}
# the height field seen whole, as tests/test_gpu_mesh_occlude.py sees it
FIELD_R, FIELD_H, FIELD_W = 64, 96, 160
FIELD_STRAIGHT = ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.1)
FIELD_TILTED = ((0, 0, 0), (0.35, -0.2, 0.9), (0.0, 1.0, 0.15), 1.1)


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def table_stamp(pose, r=R, h=TEX, w=TEX):
    """The table scene rendered from `pose`, and a stamp image that is red where the window shows the table top and blue elsewhere."""
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = synthetic.make_table_on_floor()
    tex = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    tex[..., 0] = 7  # no texel is red before the stamp: a red byte other than 7 was written
    cam = mesh_ref.camera(*pose)
    _, face_idx, proj = mesh_ref.render(v, f, uv, cam, pose[3], tex, r)
    top = face_idx.numpy() >= 2
    dec = np.full((r, r, 4), -1.0, dtype=np.float32)
    dec[..., 0] = np.where(top, 1.0, -1.0)
    dec[..., 2] = np.where(top, -1.0, 1.0)
    return dict(v=v, f=f, uv=uv, tex=tex, cam=cam, face_idx=face_idx, proj=proj, dec=torch.from_numpy(dec), mask=stroke_ref.make_stamp_mask(r, 1),
                fov=pose[3])


# ---------------------------------------------------------------- the table scene
@pytest.mark.parametrize("pose", sorted(POSES))
def test_the_floor_under_the_table_is_left_alone_and_takes_none_of_its_colour(pose):
    s = table_stamp(POSES[pose])
    assert set(np.unique(s["face_idx"].numpy())) >= {0, 1, 2, 3} and s["proj"]["upright"].all()
    args = (s["proj"], s["face_idx"], s["uv"], s["dec"], s["mask"], s["tex"])
    plain, plain_info = mesh_ref.backproject(*args)
    got, info = occ.backproject(*args, fov=s["fov"], occlude=1.0)
    floor = np.zeros((TEX, TEX), dtype=bool)
    floor[:, :TEX // 2] = True
    behind = occ.table_floor_behind_the_top(s["cam"], s["fov"], R, TEX, TEX)
    assert int(behind.sum()) > 100 and not (behind & ~floor).any()
    # the leak, as it stands without the test: floor texels behind the top are written, and floor texels carry the top's red
    assert (plain_info["written"] & behind).sum() == behind.sum()
    leaked = plain_info["written"] & floor & (plain.numpy()[..., 0] > 0)
    assert int(leaked.sum()) > 250
    # with it: none of them is written, and no written floor texel has any red
    assert not (info["written"] & behind).any()
    assert torch.equal(got[torch.from_numpy(behind)], s["tex"][torch.from_numpy(behind)])
    written_floor = info["written"] & floor
    assert int(written_floor.sum()) > 1000 and (got.numpy()[..., 0][written_floor] == 0).all()
    # the blue of the floor's own pixels, renormalised to full: a sum of weights over itself, within an ulp of 1, truncated to a byte
    assert (got.numpy()[..., 2][written_floor] >= 254).all()
    # the top's own texels are the plain stamp's, byte for byte
    assert torch.equal(got[:, TEX // 2:], plain[:, TEX // 2:]) and int(info["written"][:, TEX // 2:].sum()) > 200
    assert info["n_rejected"] >= int(leaked.sum()) and info["n_unwritten"] >= int(behind.sum())
    if pose == "straight":  # the figures of the experiment this rule came from
        assert int(leaked.sum()) == 288 and info["n_rejected"] == 288 and info["n_unwritten"] == 220
    # what is not written keeps its bytes
    assert torch.equal(got[torch.from_numpy(~info["written"])], s["tex"][torch.from_numpy(~info["written"])])


def test_zeroing_the_alpha_alone_would_leave_red_at_the_rim():
    """Why the weights are renormalised: a texel at the rim of the table's shadow has taps on both faces; the plain blend of its colour
    carries the top's red whatever its alpha says."""
    s = table_stamp(STRAIGHT)
    args = (s["proj"], s["face_idx"], s["uv"], s["dec"], s["mask"], s["tex"])
    plain, _ = mesh_ref.backproject(*args)
    got, info = occ.backproject(*args, fov=s["fov"], occlude=1.0)
    rim = info["rejected"] & info["written"]
    rim[:, TEX // 2:] = False
    assert int(rim.sum()) == 288 - 220
    assert int((plain.numpy()[..., 0][rim] > 127).sum()) == 64 and (got.numpy()[..., 0][rim] == 0).all()


def test_erase_follows_the_same_written_rule():
    s = table_stamp(TILTED)
    disc = stroke_ref.disc_mask(R)
    _, painted = occ.backproject(s["proj"], s["face_idx"], s["uv"], s["dec"], disc, s["tex"], fov=s["fov"], occlude=1.0)
    got, info = occ.backproject(s["proj"], s["face_idx"], s["uv"], None, disc, s["tex"], fov=s["fov"], occlude=1.0)
    assert (info["written"] == painted["written"]).all() and int(info["written"].sum()) > 500 and info["n_unwritten"] > 50
    w = torch.from_numpy(info["written"])
    assert int(got[w].sum()) == 0 and torch.equal(got[~w], s["tex"][~w])


# ---------------------------------------------------------------- off is the plain reference
@pytest.mark.parametrize("erase", [False, True])
def test_occlude_none_is_the_plain_reference(erase):
    s = table_stamp(TILTED)
    dec = None if erase else s["dec"]
    want, want_info = mesh_ref.backproject(s["proj"], s["face_idx"], s["uv"], dec, s["mask"], s["tex"])
    got, info = occ.backproject(s["proj"], s["face_idx"], s["uv"], dec, s["mask"], s["tex"], fov=s["fov"], occlude=None)
    assert torch.equal(got, want) and (info["written"] == want_info["written"]).all()
    assert info["n_rejected"] == 0 and info["n_unwritten"] == 0 and not info["rejected"].any()
    # a tolerance no depth of the scene reaches is the plain reference too, through the other code path
    got, info = occ.backproject(s["proj"], s["face_idx"], s["uv"], dec, s["mask"], s["tex"], fov=s["fov"], occlude=1e6)
    assert torch.equal(got, want) and info["n_rejected"] == 0


# ---------------------------------------------------------------- a smooth surface passes untouched at 1.0
@pytest.mark.parametrize("pose", ["straight", "tilted"])
def test_the_smooth_height_field_rejects_no_tap_at_one_pixel(pose):
    """tests/test_gpu_mesh_occlude.py compares occlude = 1.0 on this field, from these poses, with the plain backprojection byte for
    byte: that rests on this count."""
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = synthetic.make_height_field(bump=0.1)
    p = FIELD_STRAIGHT if pose == "straight" else FIELD_TILTED
    tex = torch.randint(0, 256, (FIELD_H, FIELD_W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(77))
    dec = torch.randn(FIELD_R, FIELD_R, 4, generator=torch.Generator().manual_seed(5)) * 0.9
    _, face_idx, proj = mesh_ref.render(v, f, uv, mesh_ref.camera(*p), p[3], tex, FIELD_R)
    mask = stroke_ref.make_stamp_mask(FIELD_R, 1)
    got, info = occ.backproject(proj, face_idx, uv, dec, mask, tex, fov=p[3], occlude=1.0)
    assert info["n_rejected"] == 0 and info["n_unwritten"] == 0
    plain, plain_info = mesh_ref.backproject(proj, face_idx, uv, dec, mask, tex)
    assert torch.equal(got, plain) and int(plain_info["written"].sum()) > 10000
    # and at 0 the shared edges of neighbouring faces reject: the tolerance cannot be 0
    _, at0 = occ.backproject(proj, face_idx, uv, dec, mask, tex, fov=p[3], occlude=0.0)
    assert at0["n_rejected"] > 4000


def test_the_tolerance_is_rounded_once():
    assert occ.tolerance(1.0, 1.0, 32) == np.float32(0.0625)
    assert occ.tolerance(0.1, 0.3, 7) == np.float32(float(np.float32(0.1)) * 2.0 * float(np.float32(0.3)) / 7.0)
    assert occ.tolerance(1e-30, 1e-30, 4096) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            occ.tolerance(bad, 1.0, 32)
    with pytest.raises(ValueError):
        occ.tolerance(3e38, 3e38, 4096)


# ---------------------------------------------------------------- header, binding, refusals
def test_header_and_binding_agree_on_the_occluded_entry_points(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mesh_stroke_occluded", "dtp_op_mesh_backproject_occluded"}
    assert new <= declared and declared == set(_lib.SYMBOLS)

    def args(name):
        return [a.strip() for a in re.search(rf"\b{name}\s*\(([^)]*)\)", code).group(1).split(",")]

    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"
        decl, bound = args(name), _lib.SYMBOLS[name][1]
        assert len(decl) == len(bound), name
        for d, b in zip(decl, bound):  # a float travels as a float, an int as an int, everything else as a pointer
            want = C.c_float if d.startswith("float ") and "*" not in d else C.c_int if d.startswith("int ") and "*" not in d else None
            assert (b is want) if want else (b not in (C.c_float, C.c_int)), (name, d, b)
    # the masked entry points with the tolerance (and the fov) before the stream
    assert args("dtp_mesh_stroke_occluded")[:-2] == args("dtp_mesh_stroke_masked")[:-1]
    assert args("dtp_mesh_stroke_occluded")[-2:] == ["float occlude", "dtp_stream s"]
    assert args("dtp_op_mesh_backproject_occluded")[:-3] == args("dtp_op_mesh_backproject_masked")[:-1]
    assert args("dtp_op_mesh_backproject_occluded")[-3:] == ["float fov", "float occlude", "dtp_stream s"]
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3


def test_refusals_come_before_any_device_call(lib):
    """The setting is checked before the handles are looked at, so the checks run without a device: with NULL handles, which a good
    setting then meets."""
    f = C.c_float

    def refused(rc, word):
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())

    for bad, word in ((-1.0, r"occlude=-1 "), (-1e-30, r"occlude=-1e-30 "), (float("nan"), r"occlude=-?nan"), (float("inf"), r"occlude=inf"),
                      (float("-inf"), r"occlude=-inf")):
        refused(lib.dtp_mesh_stroke_occluded(None, None, None, 8, 8, None, 1, None, None, None, 0, None, 0, f(bad), None),
                r"dtp_mesh_stroke_occluded: " + word)
        refused(lib.dtp_op_mesh_backproject_occluded(None, None, 0, None, None, 64, None, 8, 8, None, 0, f(1.0), f(bad), None),
                r"dtp_op_mesh_backproject_occluded: " + word)
    refused(lib.dtp_mesh_stroke_occluded(None, None, None, 8, 8, None, 1, None, None, None, 17, None, 0, f(1.0), None), r"bleed=17")
    refused(lib.dtp_mesh_stroke_occluded(None, None, None, 8, 8, None, 1, None, None, None, 0, None, 0, f(1.0), None), r"NULL")
    refused(lib.dtp_mesh_stroke_occluded(None, None, None, 8, 8, None, 1, None, None, None, 0, None, 0, f(0.0), None), r"NULL")  # 0 is legal
    for fov, word in ((0.0, r"fov=0 "), (-1.0, r"fov=-1 "), (float("nan"), r"fov=-?nan"), (float("inf"), r"fov=inf")):
        refused(lib.dtp_op_mesh_backproject_occluded(None, None, 0, None, None, 64, None, 8, 8, None, 0, f(fov), f(1.0), None), word)
    refused(lib.dtp_op_mesh_backproject_occluded(None, None, 0, None, None, 0, None, 8, 8, None, 0, f(1.0), f(1.0), None), r"R=0 ")
    refused(lib.dtp_op_mesh_backproject_occluded(None, None, 0, None, None, 4097, None, 8, 8, None, 0, f(1.0), f(1.0), None), r"R=4097 ")
    refused(lib.dtp_op_mesh_backproject_occluded(None, None, 0, None, None, 64, None, 8, 8, None, 0, f(3e38), f(3e38), None), r"does not fit fp32")
    refused(lib.dtp_op_mesh_backproject_occluded(None, None, 0, None, None, 64, None, 8, 8, None, 0, f(1.0), f(1.0), None), r"NULL")


def test_the_python_keyword():
    from diffusiontexturepainting_amd import mesh, ops
    assert mesh.occlude_arg(None) is None and mesh.occlude_arg(False) is None
    assert mesh.occlude_arg(True) == 1.0 and mesh.OCCLUDE_DEFAULT == 1.0
    assert mesh.occlude_arg(0) == 0.0 and mesh.occlude_arg(0.0) == 0.0 and mesh.occlude_arg(0.25) == 0.25  # 0 is a tolerance, not "off"
    assert mesh.occlude_arg(torch.tensor(2.5)) == 2.5 and mesh.occlude_arg(np.float32(0.5)) == 0.5
    for bad in (-0.5, float("nan"), float("inf"), 1e39, "one", [1.0, 2.0]):
        with pytest.raises(ValueError, match="occlude"):
            mesh.occlude_arg(bad)
    # ops.mesh_backproject asks for the fov before it touches anything
    with pytest.raises(ValueError, match="occlude needs fov"):
        ops.mesh_backproject(None, None, None, None, None, occlude=True)
    with pytest.raises(ValueError, match="occlude"):
        ops.mesh_backproject(None, None, None, None, None, fov=1.0, occlude=-1.0)


def test_the_table_scene_is_what_the_docstring_says():
    from diffusiontexturepainting_amd import synthetic
    v, f, uv = synthetic.make_table_on_floor()
    assert tuple(v.shape) == (8, 3) and tuple(f.shape) == (4, 3) and tuple(uv.shape) == (4, 3, 2)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and uv.dtype == torch.float32
    assert (v[:4, 2] == 0).all() and (v[4:, 2] == 0.5).all() and float(v[:4, :2].abs().max()) == 1.0
    assert torch.allclose(v[4:, :2].abs(), torch.tensor(0.4))
    assert float(uv[:2, :, 0].min()) == pytest.approx(0.02) and float(uv[:2, :, 0].max()) == pytest.approx(0.48)
    assert float(uv[2:, :, 0].min()) == pytest.approx(0.52) and float(uv[2:, :, 0].max()) == pytest.approx(0.98)
    tri = v[f.long()]
    assert (torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)[:, 2] > 0).all()  # every normal towards +z
