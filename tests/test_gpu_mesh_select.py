"""Face sets on the device (dtp_mesh_select, dtp_mesh_stroke_masked, dtp_view_tint; `select_faces`, `paint_mesh_stroke(face_mask=)`,
`tint_selection`; include/dtp.h "face sets: a lasso, masked strokes, a tint") against the numpy restatement of the contract
(tests/select_ref.py): the lasso with every op, the masked backprojection and masked strokes against the host loop byte for byte, the
texels a masked stroke must leave alone, undo, the bleed pass, select-then-paint without a synchronise, and the tint.  Every comparison
is torch.equal or ==: the feature has no float.  One 64^2 context, DDIM, 4 steps, as tests/test_gpu_mesh.py."""
import math
import re

import numpy as np
import pytest
import torch

import bleed_ref
import mesh_ref
import select_ref
import stroke_ref
from mesh_ref import ERASE, INPAINT, OVERPAINT

pytestmark = pytest.mark.gpu

R = 64
H, W = 96, 160
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
OVER = (10, 25)
DEV = "cuda:0"
INT_MAX = 2 ** 31 - 1


def random_texture(h, w, seed):
    return torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import synthetic, weights as Wt
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    sd = dict(unet=Wt.synthetic_unet(5), lora=Wt.synthetic_lora(5), vae=Wt.synthetic_vae(5), clip=Wt.synthetic_clip(5),
              penc=Wt.synthetic_patch_encoder(5))
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    _, brush, _, _ = synthetic.make_stamp_batch(1, R, 6000)
    cond, uncond = synthetic.make_conditioning(6100)
    m.set_conditioning(cond, uncond, brush, slot=0)
    return m


# ---------------------------------------------------------------- meshes, frames, polygons
def field(name):
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_height_field(6, 6) if name == "faces_50" else synthetic.make_height_field(17, 13, seed=3)


FACES = {"faces_50": 50, "faces_384": 384}   # two words, the second partial; twelve full words
SIZES = [(48, 80), (45, 77)]                 # both sides a multiple of the 16-pixel tile; neither
EYE, AT, UP, FOV, NEAR = (0.3, -0.5, 2.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.05

_meshes, _frames = {}, {}


def device_mesh(model, name):
    if name not in _meshes:
        _meshes[name] = model.load_mesh(*field(name))
    return _meshes[name]


def frame(model, name, size, samples=1):
    """(face_idx on the device, on the host) of the view of a field: rendered once per mesh and size and left unchanged."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    key = (name, size, samples)
    if key not in _frames:
        cam = view_camera(EYE, AT, UP, FOV, size, NEAR)
        tex = random_texture(H, W, 5).to(DEV)
        if samples == 1:
            face_idx = ops.mesh_view(device_mesh(model, name), tex, cam, size)[1]
        else:
            face_idx = model.render_view(device_mesh(model, name), tex, cam, size, samples=samples, want_face_idx=True)[1]
        torch.cuda.synchronize()
        _frames[key] = (face_idx, face_idx.cpu())
        shown = set(face_idx.cpu().unique().tolist()) - {-1}
        assert len(shown) > FACES[name] // 2 and int((face_idx < 0).sum()) > 0  # most of the mesh, and some background
    return _frames[key]


def polygons(h, w):
    star = [((0.5 + (0.45 if k % 2 == 0 else 0.18) * math.cos(math.pi * k / 6)) * w, (0.5 + (0.45 if k % 2 == 0 else 0.18) * math.sin(math.pi * k / 6)) * h)
            for k in range(12)]
    circle = [((0.5 + 0.41 * math.cos(2 * math.pi * k / 1024)) * w, (0.48 + 0.43 * math.sin(2 * math.pi * k / 1024)) * h) for k in range(1024)]
    return {
        "triangle": [(0.1 * w, 0.15 * h), (0.9 * w, 0.3 * h), (0.35 * w, 0.95 * h)],
        "concave_12_gon": star,
        "bow_tie": [(0.1 * w, 0.1 * h), (0.9 * w, 0.9 * h), (0.9 * w, 0.1 * h), (0.1 * w, 0.9 * h)],
        "circle_1024": circle,
        "partly_outside": [(-0.4 * w, 0.3 * h), (0.6 * w, -0.5 * h), (1.7 * w, 0.55 * h), (0.5 * w, 1.3 * h)],
        "inside_one_pixel": [(20.6, 20.6), (20.9, 20.6), (20.9, 20.9)],
    }


POLYGON_NAMES = sorted(polygons(48, 80))


def random_set(F, seed):
    return np.random.default_rng(seed).random(F) < 0.4


# ---------------------------------------------------------------- the lasso
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(FACES))
@pytest.mark.parametrize("polygon", POLYGON_NAMES)
def test_lasso_matches_the_restatement_for_every_op(model, polygon, name, size):
    from diffusiontexturepainting_amd import mesh as M
    F, dm = FACES[name], device_mesh(model, name)
    face_idx, host_idx = frame(model, name, size)
    poly = polygons(*size)[polygon]
    hit = select_ref.hit_faces(host_idx, poly, F)
    # replace, into a fresh set and into a set that held something else
    got = model.select_faces(dm, face_idx, poly)
    assert got.dtype == torch.int32 and tuple(got.shape) == ((F + 31) // 32,) and got.device == face_idx.device
    assert torch.equal(got.cpu(), select_ref.pack(hit))
    assert torch.equal(M.faceset_to_bool(got, F).cpu(), torch.from_numpy(hit))
    before = random_set(F, 7)
    out = select_ref.pack(before).to(DEV)
    assert model.select_faces(dm, face_idx, poly, op="replace", out=out) is out
    assert torch.equal(out.cpu(), select_ref.pack(hit))
    for op in ("add", "subtract"):
        out = select_ref.pack(before).to(DEV)
        assert model.select_faces(dm, face_idx, poly, op=op, out=out) is out
        assert torch.equal(out.cpu(), select_ref.pack(select_ref.select(host_idx, poly, F, op, before))), op
    # add, then subtract the same polygon: a set that shared no face with the polygon is restored, stray high bits included
    start = ~select_ref.pack(before | hit).to(DEV)
    kept = start.clone()
    model.select_faces(dm, face_idx, poly, op="add", out=start)
    assert torch.equal(M.faceset_to_bool(start, F).cpu(), torch.from_numpy(~before | hit))
    model.select_faces(dm, face_idx, poly, op="subtract", out=start)
    assert torch.equal(start, kept)
    assert torch.equal(face_idx.cpu(), host_idx)  # the frame is only read
    # what each polygon is there for
    n = int(hit.sum())
    if polygon == "inside_one_pixel":
        assert n == 0
    elif polygon == "bow_tie":
        inside = select_ref.inside(select_ref.snap_polygon(poly), *size)
        assert inside[size[0] // 2, size[1] // 5] and not inside[size[0] // 5, size[1] // 2] and 0 < n < F
    elif polygon == "partly_outside":
        xy = select_ref.snap_polygon(poly)
        assert xy[:, 0].min() < 0 and xy[:, 0].max() > 256 * size[1] and 0 < n
    elif polygon == "triangle":
        assert 0 < n < F
    else:
        assert 0 < n


def test_lasso_skips_face_indices_that_are_no_face_and_stays_inside_its_words(model):
    """A hand-made frame holding F, F + 31 (a bit of the word BEHIND the set), -7 and INT_MAX: nothing is used as an index.  The set is
    the middle of a larger tensor whose other words keep their sentinel."""
    from diffusiontexturepainting_amd import mesh as M
    h, w = 45, 77
    poly = [(2.0, 2.0), (75.0, 3.0), (70.0, 43.0), (4.0, 40.0)]
    for name, F in sorted(FACES.items()):
        dm, words = device_mesh(model, name), (F + 31) // 32
        bad = torch.tensor([F, F + 31, -7, INT_MAX, F + 32 * 40, -INT_MAX - 1], dtype=torch.int32)
        host_idx = bad[torch.randint(0, len(bad), (h, w), generator=torch.Generator().manual_seed(F))]
        assert not select_ref.hit_faces(host_idx, poly, F).any() and select_ref.inside(select_ref.snap_polygon(poly), h, w).sum() > 2000
        face_idx = host_idx.to(DEV)
        pattern = select_ref.pack(random_set(F, 9))
        for op in ("add", "subtract", "replace"):
            big = torch.full((words + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            out = big[4:4 + words]
            out.copy_(pattern)
            model.select_faces(dm, face_idx, poly, op=op, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), torch.zeros_like(pattern) if op == "replace" else pattern), op
            assert (big[:4] == 0x5A5A5A5A).all() and (big[4 + words:] == 0x5A5A5A5A).all(), op
        # one real face among them is found
        host_idx[20, 30] = F - 1
        got = model.select_faces(dm, host_idx.to(DEV), poly)
        assert np.nonzero(M.faceset_to_bool(got, F).cpu().numpy())[0].tolist() == [F - 1]


def test_lasso_on_the_frame_of_an_anti_aliased_view(model):
    name, size, F = "faces_384", (45, 77), 384
    face_idx, host_idx = frame(model, name, size, samples=2)
    assert not torch.equal(host_idx, frame(model, name, size)[1])  # the centre SAMPLE's face, not the centre's
    for polygon in ("concave_12_gon", "circle_1024"):
        poly = polygons(*size)[polygon]
        got = model.select_faces(device_mesh(model, name), face_idx, poly)
        want = select_ref.hit_faces(host_idx, poly, F)
        assert torch.equal(got.cpu(), select_ref.pack(want)) and 0 < int(want.sum()) < F


def test_select_refusals_leave_the_set_alone(model):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd._lib import DtpError
    name, size, F = "faces_50", (48, 80), 50
    dm = device_mesh(model, name)
    face_idx, _ = frame(model, name, size)
    tri = polygons(*size)["triangle"]
    out = select_ref.pack(random_set(F, 3)).to(DEV)
    kept = out.clone()

    def refused(pattern, polygon=tri, **kw):
        with pytest.raises(DtpError) as e:
            model.select_faces(dm, face_idx, polygon, out=out, **kw)
        assert re.search(r"\(code 1\)", str(e.value)) and re.search(pattern, str(e.value)), str(e.value)

    refused(r"n=2 vertices", polygon=tri[:2])
    refused(r"n=1025 vertices", polygon=[(1.0 + 0.01 * k, 2.0) for k in range(1025)])
    refused(r"vertex 1 of the polygon is not finite", polygon=[tri[0], (float("nan"), 3.0), tri[2]])
    refused(r"vertex 2 of the polygon is not finite", polygon=[tri[0], tri[1], (4.0, float("inf"))])
    with pytest.raises(ValueError, match="op 'toggle'"):
        model.select_faces(dm, face_idx, tri, op="toggle", out=out)
    with pytest.raises(ValueError, match="2 words for 50 faces"):
        model.select_faces(dm, face_idx, tri, out=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="int32"):
        model.select_faces(dm, face_idx, tri, out=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="it is on cpu"):
        model.select_faces(dm, face_idx, tri, out=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        model.select_faces(dm, face_idx, tri, out=torch.zeros(4, dtype=torch.int32, device=DEV)[::2])
    with pytest.raises(ValueError, match="face_idx"):
        model.select_faces(dm, face_idx.float(), tri)
    with pytest.raises(ValueError, match="load_mesh"):
        model.select_faces(None, face_idx, tri)
    # the C entry point itself: the set's size against the mesh, a dead mesh, an op it does not know
    lib = _lib.load()
    poly = torch.tensor(tri, dtype=torch.float32)
    vs = model.view_stream.cuda_stream
    args = [dm.handle, _lib.ptr(face_idx), size[0], size[1], _lib.ptr(poly), 3, 0, _lib.ptr(out), 2, vs]
    for i, v, word in ((8, 1, b"1 words for 50 faces"), (8, 3, b"3 words for 50 faces"), (6, 3, b"unknown op 3"), (0, None, b"NULL"), (1, None, b"NULL"),
                       (7, None, b"NULL"), (7, out.data_ptr() + 2, b"aligned")):
        bad = list(args)
        bad[i] = v
        assert lib.dtp_mesh_select(*bad) == 1 and word in lib.dtp_last_error(), lib.dtp_last_error()
    dead = model.load_mesh(*field(name))
    handle = dead.handle
    dead.close()
    assert lib.dtp_mesh_select(handle, *args[1:]) == 1 and b"not a live mesh" in lib.dtp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, kept)


# ---------------------------------------------------------------- the masked backprojection
FRONT = ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.1)          # pos, normal, prev, fov: the whole field
OBLIQUE = ((0.1, -0.05, 0.1), (0.35, -0.2, 0.9), (0.0, 0.3, 0.15), 0.45)


def masks(name):
    """bool [F] each: empty, all, every other face, the first UV chart (the faces left of the middle column)."""
    F = FACES[name]
    per_row, left = (10, 4) if name == "faces_50" else (32, 16)
    chart = (np.arange(F) % per_row) < left
    return {"empty": np.zeros(F, dtype=bool), "all": np.ones(F, dtype=bool), "every_other": np.arange(F) % 2 == 0, "one_chart": chart}


_renders = {}


def reference_render(name, pose, texture):
    """mesh_ref's render of a field, computed once and left unchanged (select_ref.backproject copies what it masks)."""
    key = (name, pose)
    if key not in _renders:
        v, f, uv = field(name)
        cam = mesh_ref.camera(*pose)
        _, face_idx, proj = mesh_ref.render(v, f, uv, cam, pose[3], texture, R)
        _renders[key] = (uv, face_idx, proj)
    return _renders[key]


@pytest.mark.parametrize("which", ["empty", "all", "every_other", "one_chart"])
@pytest.mark.parametrize("name,pose", [("faces_50", FRONT), ("faces_384", OBLIQUE)], ids=["faces_50", "faces_384"])
def test_masked_backprojection_matches_the_restatement(model, name, pose, which):
    from diffusiontexturepainting_amd import mesh as M, ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    texture = random_texture(H, W, 77)
    dec = torch.randn(R, R, 4, generator=torch.Generator().manual_seed(5)) * 0.9
    uv, ref_idx, proj = reference_render(name, pose, texture)
    sel = masks(name)[which]
    dm = device_mesh(model, name)
    face_mask = M.faceset_from_bool(torch.from_numpy(sel)).to(DEV)
    assert torch.equal(face_mask.cpu(), select_ref.pack(sel))
    square, disc = stroke_ref.make_stamp_mask(R, 1), stroke_ref.disc_mask(R)
    for d, mask in ((dec, square), (None, disc)):  # a stamp, and an Erase stamp
        dtex = texture.to(DEV)
        _, face_idx = ops.mesh_render(dm, mesh_camera(*pose), pose[3], dtex, R)
        assert torch.equal(face_idx.cpu(), ref_idx)
        out = ops.mesh_backproject(dm, None if d is None else d.to(DEV), mask.to(DEV), face_idx, dtex, face_mask=face_mask)
        want, info = select_ref.backproject(proj, ref_idx, uv, d, mask, texture, sel)
        assert out is dtex and torch.equal(out.cpu(), want)
        written = torch.from_numpy(info["written"])
        assert torch.equal(out.cpu()[~written], texture[~written])
        plain, plain_info = mesh_ref.backproject(proj, ref_idx, uv, d, mask, texture)
        if which == "empty":
            assert int(written.sum()) == 0 and torch.equal(out.cpu(), texture)
        elif which == "all":
            assert torch.equal(out.cpu(), plain)
            # and the complement of the empty set, stray bits and all, is "all" too
            again = ops.mesh_backproject(dm, None if d is None else d.to(DEV), mask.to(DEV), face_idx, texture.to(DEV),
                                         face_mask=~M.faceset_empty(FACES[name], DEV))
            assert torch.equal(again.cpu(), plain)
        else:
            assert 0 < int(written.sum()) < int(plain_info["written"].sum())
        if d is None and which != "empty":
            assert int(out.cpu()[written].sum()) == 0


# ---------------------------------------------------------------- masked strokes
# the three stamps of tests/test_gpu_mesh.py, twice: their windows span the seam between the two charts
POSES = dict(positions=[(0.1, -0.05, 0.1), (0.3, 0.05, 0.1), (0.2, 0.2, 0.1)] * 2,
             normals=[(0.35, -0.2, 0.9), (0.0, 0.0, 1.0), (-0.2, 0.1, 0.95)] * 2,
             prevs=[(0.0, 0.3, 0.15), (0.1, -0.05, 0.1), (0.3, 0.05, 0.1)] * 2,
             fov=[0.45, 0.4, 0.5, 0.42, 0.47, 0.38])
ARGS = (POSES["positions"], POSES["normals"], POSES["prevs"], POSES["fov"])
MODES = [INPAINT, OVERPAINT, ERASE, OVERPAINT, ERASE, INPAINT]
SEEDS = [700, 701, 702, 703, 704, 705]
STROKE_MESH = "faces_384"


def host_loop(model, dm, data, tex, face_mask, sel, k=0):
    """Per stamp: ops.mesh_render -> generate_raw -> ops.mesh_backproject(face_mask=) (-> the bleed restatement's pass over the box of the
    SELECTED valid faces grown by k)."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    v, f, uv = data
    h, w = tex.shape[:2]
    cov = bleed_ref.coverage(uv, h, w) if k else None
    tex = tex.clone()
    for i in range(len(SEEDS)):
        pose = (ARGS[0][i], ARGS[1][i], ARGS[2][i], ARGS[3][i])
        canvas, face_idx = ops.mesh_render(dm, mesh_camera(*pose), pose[3], tex, R, mode=MODES[i], over_y=OVER[0], over_x=OVER[1])
        if MODES[i] == ERASE:
            ops.mesh_backproject(dm, None, stroke_ref.disc_mask(R).to(DEV), face_idx, tex, face_mask=face_mask)
        else:
            painted = model.generate_raw(canvas, seeds=[SEEDS[i]], **ST)
            ops.mesh_backproject(dm, None, stroke_ref.make_stamp_mask(R, 1).to(DEV), face_idx, tex, painted=painted, face_mask=face_mask)
        if k:
            proj = dict(mesh_ref.project(v, f, mesh_ref.camera(*pose), pose[3], R))
            if sel is not None:
                proj["upright"] = proj["upright"] & sel
            rect = bleed_ref.stamp_rect(proj, face_idx, uv, h, w, k)
            if rect is not None:
                tex = bleed_ref.bleed(tex, cov, k, rect).to(DEV)
    return tex


@pytest.fixture(scope="module")
def strokes(model):
    """The unmasked 6-stamp stroke and the stroke masked to one chart, each painted once."""
    from diffusiontexturepainting_amd import mesh as M
    dm = device_mesh(model, STROKE_MESH)
    texture = random_texture(H, W, 77)
    sel = masks(STROKE_MESH)["one_chart"]
    face_mask = M.faceset_from_bool(torch.from_numpy(sel)).to(DEV)
    plain = model.paint_mesh_stroke(dm, texture.to(DEV), *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, **ST)
    info = model.stroke_info()
    masked = model.paint_mesh_stroke(dm, texture.to(DEV), *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, face_mask=face_mask, **ST)
    assert model.stroke_info() == info == dict(stamps=6, groups=6, unet_evals=3 * 4)  # the mask changes no stamp: 4 stamps of 3 evaluations
    torch.cuda.synchronize()
    return dict(dm=dm, texture=texture, sel=sel, face_mask=face_mask, plain=plain, masked=masked)


def test_masked_stroke_equals_the_host_loop_and_leaves_the_rest_alone(model, strokes):
    from diffusiontexturepainting_amd import ops
    s = strokes
    want = host_loop(model, s["dm"], field(STROKE_MESH), s["texture"].to(DEV), s["face_mask"], s["sel"])
    assert torch.equal(s["masked"], want)
    got, texture = s["masked"].cpu(), s["texture"]
    # every texel whose centre no selected face covers keeps its old bytes: the coverage of a mesh built from the selected faces alone
    v, f, uv = field(STROKE_MESH)
    keep = torch.from_numpy(s["sel"])
    part = model.load_mesh(v, f[keep].contiguous(), uv[keep].contiguous())
    covered = ops.mesh_coverage(part, H, W).cpu()
    part.close()
    assert torch.equal(got[~covered], texture[~covered])
    changed = (got != texture).any(dim=-1)
    assert int(changed.sum()) > 200 and not bool(changed[:, W // 2:].any())  # the first chart lies in u < 0.5
    # the unmasked stroke painted both charts, and on the selected chart the first stamp's bytes are the same
    plain_changed = (s["plain"].cpu() != texture).any(dim=-1)
    assert bool(plain_changed[:, W // 2:].any()) and int(plain_changed.sum()) > int(changed.sum())


def test_a_full_mask_is_the_unmasked_stroke(model, strokes):
    from diffusiontexturepainting_amd import mesh as M
    s, F = strokes, FACES[STROKE_MESH]
    for full in (M.faceset_from_bool(torch.ones(F, dtype=torch.bool)).to(DEV), ~M.faceset_empty(F, DEV)):
        out = model.paint_mesh_stroke(s["dm"], s["texture"].to(DEV), *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, face_mask=full, **ST)
        assert torch.equal(out, s["plain"])
    # and an empty one paints nothing and is no error
    out = model.paint_mesh_stroke(s["dm"], s["texture"].to(DEV), *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER,
                                  face_mask=M.faceset_empty(F, DEV), **ST)
    assert torch.equal(out.cpu(), s["texture"])


def test_an_erase_stamp_with_a_mask(model, strokes):
    s = strokes
    pose = (ARGS[0][1], ARGS[1][1], ARGS[2][1], ARGS[3][1])
    uv, ref_idx, proj = reference_render(STROKE_MESH, pose, s["texture"])
    want, info = select_ref.backproject(proj, ref_idx, uv, None, stroke_ref.disc_mask(R), s["texture"], s["sel"])
    out = model.paint_mesh_stroke(s["dm"], s["texture"].to(DEV), [pose[0]], [pose[1]], [pose[2]], pose[3], modes="erase", face_mask=s["face_mask"], **ST)
    assert torch.equal(out.cpu(), want) and int(info["written"].sum()) > 50
    assert model.stroke_info() == dict(stamps=1, groups=1, unet_evals=0)
    plain, plain_info = mesh_ref.backproject(proj, ref_idx, uv, None, stroke_ref.disc_mask(R), s["texture"])
    assert int(plain_info["written"].sum()) > int(info["written"].sum())


def test_undo_restores_the_texture_after_a_masked_stroke(model, strokes):
    s = strokes
    tex = s["texture"].to(DEV)
    j = model.journal(tex)
    with j.stroke():
        model.paint_mesh_stroke(s["dm"], tex, *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, face_mask=s["face_mask"], **ST)
    assert torch.equal(tex, s["masked"])
    masked_tiles = set(j.tiles(0))
    assert j.undo() is True and torch.equal(tex.cpu(), s["texture"])
    assert j.redo() is True and torch.equal(tex, s["masked"])
    j.close()
    # the record holds the tiles of the selected faces' box alone: fewer than the unmasked stroke's
    tex = s["texture"].to(DEV)
    j = model.journal(tex)
    with j.stroke():
        model.paint_mesh_stroke(s["dm"], tex, *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, **ST)
    plain_tiles = set(j.tiles(0))
    j.close()
    assert masked_tiles < plain_tiles


def test_masked_stroke_with_bleed_equals_the_host_loop(model, strokes):
    s = strokes
    out = model.paint_mesh_stroke(s["dm"], s["texture"].to(DEV), *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, bleed=2,
                                  face_mask=s["face_mask"], **ST)
    want = host_loop(model, s["dm"], field(STROKE_MESH), s["texture"].to(DEV), s["face_mask"], s["sel"], k=2)
    assert torch.equal(out, want)
    cov = torch.from_numpy(bleed_ref.coverage(field(STROKE_MESH)[2], H, W))
    gutter = (out.cpu() != s["texture"]).any(dim=-1) & ~cov
    assert int(gutter.sum()) > 20  # the pass wrote


def test_select_then_paint_needs_no_synchronise(model, strokes):
    """render_view -> select_faces -> paint_mesh_stroke(face_mask=) enqueued back to back equals the same with a synchronise between
    every call; the set is written on the view's stream and read on the stroke's."""
    from diffusiontexturepainting_amd.mesh import view_camera
    s, size = strokes, (48, 80)
    cam = view_camera(EYE, AT, UP, FOV, size, NEAR)
    poly = polygons(*size)["concave_12_gon"]

    def run(sync):
        wait = torch.cuda.synchronize if sync else (lambda: None)
        tex = s["texture"].to(DEV)
        wait()
        _, face_idx = model.render_view(s["dm"], tex, cam, size, want_face_idx=True)
        wait()
        sel = model.select_faces(s["dm"], face_idx, poly)
        wait()
        model.paint_mesh_stroke(s["dm"], tex, *ARGS, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, face_mask=sel, **ST)
        wait()
        shown = model.render_view(s["dm"], tex, cam, size, selection=sel)
        torch.cuda.synchronize()
        return tex.cpu(), sel.cpu(), shown.cpu()

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    picked = select_ref.unpack(a[1], FACES[STROKE_MESH])
    assert 0 < int(picked.sum()) < FACES[STROKE_MESH] and not torch.equal(a[0], s["texture"]) and not torch.equal(a[0], s["plain"].cpu())


def test_stroke_refusals_leave_the_texture_alone(model, strokes):
    import ctypes as C
    from diffusiontexturepainting_amd import _lib, mesh as _mesh, ops
    s = strokes
    tex = s["texture"].to(DEV)
    good = s["face_mask"]

    def refused(pattern, face_mask):
        with pytest.raises(ValueError, match=pattern):
            model.paint_mesh_stroke(s["dm"], tex, *ARGS, seeds=SEEDS, modes=MODES, face_mask=face_mask, **ST)
        with pytest.raises(ValueError, match=pattern):
            model.paint_mesh_path(s["dm"], tex, [(0.0, 0.0, 3.0), (0.4, 0.1, 3.0)], [(0.0, 0.0, -1.0)] * 2, 0.3, face_mask=face_mask, **ST)
        _, face_idx = ops.mesh_render(s["dm"], _mesh.mesh_camera(*FRONT), FRONT[3], tex, R)
        with pytest.raises(ValueError, match=pattern):
            ops.mesh_backproject(s["dm"], None, stroke_ref.disc_mask(R).to(DEV), face_idx, tex, face_mask=face_mask)

    refused("int32", good.to(torch.int64))
    refused("int32", torch.ones(384, dtype=torch.bool, device=DEV))
    refused(r"12 words for 384 faces", torch.zeros(11, dtype=torch.int32, device=DEV))
    refused(r"12 words for 384 faces", torch.zeros(13, dtype=torch.int32, device=DEV))
    refused("it is on cpu", good.cpu())
    refused("contiguous", torch.zeros(24, dtype=torch.int32, device=DEV)[::2])
    # the C entry points: the words against the mesh's faces, alignment
    lib = _lib.load()
    stamps = _mesh.mesh_stamps(*ARGS, SEEDS, MODES, None)
    st = _lib.Settings(ST["steps"], ST["context_pad"], ST["tg_steps"], ST["cfg_weight"], 1.0, 0, 0)
    opts = _lib.MeshStrokeOpts(0, 1, OVER[0], OVER[1], 1, 1.0)
    args = [model._h, s["dm"].handle, _lib.ptr(tex), H, W, stamps, 6, C.byref(st), C.byref(opts), None, 0, _lib.ptr(good), 12, model._s()]
    for i, v, word in ((12, 11, b"11 words for 384 faces"), (12, 13, b"13 words"), (11, good.data_ptr() + 1, b"aligned"), (10, 17, b"bleed=17")):
        bad = list(args)
        bad[i] = v
        assert lib.dtp_mesh_stroke_masked(*bad) == 1 and word in lib.dtp_last_error(), lib.dtp_last_error()
    _, face_idx = ops.mesh_render(s["dm"], _mesh.mesh_camera(*FRONT), FRONT[3], tex, R)
    disc = stroke_ref.disc_mask(R).to(DEV)
    cur = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dtp_op_mesh_backproject_masked(s["dm"].handle, None, 0, _lib.ptr(disc), _lib.ptr(face_idx), R, _lib.ptr(tex), H, W, _lib.ptr(good), 11,
                                              cur) == 1 and b"11 words" in lib.dtp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(tex.cpu(), s["texture"])


# ---------------------------------------------------------------- the tint
@pytest.mark.parametrize("opacity", [0, 128, 255])
def test_tint_matches_the_rule(model, opacity):
    from diffusiontexturepainting_amd import mesh as M
    from diffusiontexturepainting_amd.mesh import view_camera
    name, size, F = "faces_50", (45, 77), 50
    dm = device_mesh(model, name)
    cam = view_camera(EYE, AT, UP, FOV, size, NEAR)
    tex = random_texture(H, W, 31).to(DEV)
    sel = masks(name)["every_other"]
    face_mask = M.faceset_from_bool(torch.from_numpy(sel)).to(DEV)
    frame_, face_idx = model.render_view(dm, tex, cam, size, want_face_idx=True)
    before = frame_.cpu()
    for color in ((255, 160, 0), (3, 250, 77)):
        work = frame_.clone()
        assert model.tint_selection(work, face_idx, face_mask, color=color, opacity=opacity, num_faces=F) is work
        want = select_ref.tint(before, face_idx, sel, color, opacity)
        got = work.cpu()
        assert torch.equal(got, want)
        assert torch.equal(got[..., 3], before[..., 3])  # alpha
        on = torch.from_numpy(sel)[face_idx.cpu().long().clamp(min=0)] & (face_idx.cpu() >= 0)
        assert torch.equal(got[~on], before[~on]) and 100 < int(on.sum()) < size[0] * size[1]
        if opacity == 0:
            assert torch.equal(got, before)
        if opacity == 255:
            assert (got[on][:, :3] == torch.tensor(color, dtype=torch.uint8)).all()
        # render_view(selection=) is render_view followed by tint_selection
        shown = model.render_view(dm, tex, cam, size, selection=face_mask, selection_color=color, selection_opacity=opacity)
        assert isinstance(shown, torch.Tensor) and torch.equal(shown.cpu(), want)
    # the complement, with its stray high bits, tints the other faces; the default colour and opacity
    work = frame_.clone()
    model.tint_selection(work, face_idx, ~face_mask, num_faces=F)
    assert torch.equal(work.cpu(), select_ref.tint(before, face_idx, ~sel))
    out = model.render_view(dm, tex, cam, size, selection=~face_mask, want_face_idx=True, samples=2)
    assert len(out) == 2 and torch.equal(out[0].cpu(), select_ref.tint(model.render_view(dm, tex, cam, size, samples=2).cpu(), out[1], ~sel))
    with pytest.raises(ValueError, match="opacity"):
        model.tint_selection(work, face_idx, face_mask, opacity=256)
    with pytest.raises(ValueError, match="2 words for 50 faces"):
        model.tint_selection(work, face_idx, torch.zeros(3, dtype=torch.int32, device=DEV), num_faces=F)
    with pytest.raises(ValueError, match="face_idx"):
        model.tint_selection(work, face_idx[:10], face_mask, num_faces=F)
