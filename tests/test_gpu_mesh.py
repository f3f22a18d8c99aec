"""Strokes on a textured mesh (dtp_mesh_stroke, `paint_mesh_stroke`): the render and backprojection kernels bit for bit against the numpy
restatement of the contract (tests/mesh_ref.py) -- face_idx, the canvas and the pasted texture with torch.equal --, a stroke against
the host loop over ops.mesh_render -> generate_raw -> ops.mesh_backproject byte for byte, the full-window quad against the 2D stroke,
enqueue without a host wait, and the refusals, which leave the texture alone.  One 64^2 context, DDIM, 4 steps; a 96 x 160 texture of
seeded random bytes (make_texture's recipe of test_gpu_stroke.py).  No fp32 operation had to be compared under a tolerance."""
import re
import time

import numpy as np
import pytest
import torch

import mesh_ref
import stroke_ref
from mesh_ref import ERASE, INPAINT, OVERPAINT

pytestmark = pytest.mark.gpu

R = 64
H, W = 96, 160
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
OVER = (10, 25)
DEV = "cuda:0"
SQUARE, DISC = "square", "disc"


def make_texture(h, w, seed):
    """Seeded random RGBA bytes with an alpha-0 (unknown) and an alpha-255 (known) region."""
    t = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    t[h // 4: h // 2, w // 8: w // 2, 3] = 0
    t[h // 2:, w // 2:, 3] = 255
    t[: h // 8, :, 3] = 0
    return t


@pytest.fixture(scope="module")
def texture():
    return make_texture(H, W, 77)


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


@pytest.fixture(scope="module")
def dec():
    """A decoder output that leaves [-1, 1] on both sides (the clamp) and hits the ends exactly."""
    d = torch.randn(R, R, 4, generator=torch.Generator().manual_seed(5)) * 0.9
    d[0, :8, :] = torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, 1.0 - 2.0 ** -23, -1.0 + 2.0 ** -23, 255.0 / 256])[:, None]
    return d


# ---------------------------------------------------------------- meshes
def _t(v, f, uv):
    return (torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int32), torch.tensor(uv, dtype=torch.float32))


def quad():
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_quad()


def height_field():
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_height_field(17, 13, seed=3)


TRI_UV = [[0.1, 0.1], [0.9, 0.15], [0.2, 0.9]]
TRI_UV2 = [[0.95, 0.95], [0.3, 0.8], [0.85, 0.2]]


def two_triangles(z0, z1):
    """Two overlapping triangles with normals towards +z at heights z0 (face 0) and z1 (face 1)."""
    return _t([[-0.8, -0.7, z0], [0.9, -0.5, z0], [-0.1, 0.8, z0], [-0.9, 0.1, z1], [0.7, -0.9, z1], [0.6, 0.7, z1]],
              [[0, 1, 2], [3, 4, 5]], [TRI_UV, TRI_UV2])


def coplanar_copies():
    v = [[-0.8, -0.7, 0.25], [0.9, -0.5, 0.25], [-0.1, 0.8, 0.25]]
    return _t(v + v, [[0, 1, 2], [3, 4, 5]], [TRI_UV, TRI_UV2])


def mixed_facing():
    """Face 0 towards the camera; face 1 back-facing (its winding reversed); face 2 steep: unit normal z = 0.3 / sqrt(0.3^2 + 1) = 0.29;
    face 3 has zero area (two corners coincide)."""
    return _t([[-0.9, -0.9, 0.0], [-0.1, -0.9, 0.0], [-0.5, -0.1, 0.0],      # 0
               [0.1, -0.9, 0.0], [0.9, -0.9, 0.0], [0.5, -0.1, 0.0],         # 1 (reversed below)
               [-0.9, 0.1, 0.0], [-0.6, 0.1, 1.0], [-0.9, 0.9, 0.0],         # 2: the edge in x rises 1.0 over 0.3
               [0.2, 0.2, 0.0], [0.8, 0.8, 0.0], [0.8, 0.8, 0.0]],           # 3
              [[0, 1, 2], [3, 5, 4], [6, 7, 8], [9, 10, 11]], [TRI_UV, TRI_UV2, TRI_UV, TRI_UV2])


def centre_grid():
    """A 6 x 5 grid of squares whose vertices land exactly on pixel centres (NDC (2 k + 1) / 64 - 1, every operation exact) and whose UVs
    land, after the snap, exactly on texel centres of the 96 x 160 texture."""
    cols, rows = [3, 10, 11, 30, 45, 60, 63], [0, 7, 20, 22, 40, 62]   # pixel columns / rows of the vertices (row 0 = the top)
    tcols, trows = [4, 20, 33, 70, 100, 150, 159], [2, 9, 30, 50, 77, 95]
    v, uv_of = [], []
    for r, tr in zip(rows, trows):
        for c, tc in zip(cols, tcols):
            v.append([(2 * c + 1) / 64 - 1, 1 - (2 * r + 1) / 64, 0.0])
            uv_of.append([(tc + 0.5) / W, 1 - (tr + 0.5) / H])
    n = len(cols)
    f, uv = [], []
    for j in range(len(rows) - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i  # a top-left, d bottom-left: y falls with the row
            for tri in ((a, d, c), (a, c, b)):
                f.append(list(tri))
                uv.append([uv_of[k] for k in tri])
    return _t(v, f, uv)


def far_vertex():
    """One corner 10^6 window widths away (the window is 2 fov wide): its snapped position is clamped to 2^26."""
    return _t([[-0.5, -0.6, 0.0], [2.0e6, 0.3, 0.0], [-0.4, 0.7, 0.0]], [[0, 1, 2]], [TRI_UV])


def first_faces(mesh, n):
    v, f, uv = mesh
    return v, f[:n].contiguous(), uv[:n].contiguous()


FRONT = ((0, 0, 0), (0, 0, 1), (0, 1, 0))            # pos, normal, prev: the camera of make_quad
OBLIQUE = ((0.1, -0.05, 0.1), (0.35, -0.2, 0.9), (0.0, 0.3, 0.15))
# name: (mesh, pose, fov, flip_normals, mode, mask)
CASES = {
    "quad": (quad, FRONT, 1.0, False, INPAINT, SQUARE),
    "quad_overpaint_disc": (quad, FRONT, 1.0, False, OVERPAINT, DISC),
    "quad_erase": (quad, FRONT, 1.0, False, ERASE, DISC),
    "quad_partly_outside": (quad, ((0.7, -0.4, 0), (0, 0, 1), (0.9, 0.3, 0)), 0.8, False, INPAINT, SQUARE),
    "occlusion_upper_face_second": (lambda: two_triangles(0.0, 0.3), FRONT, 1.0, False, INPAINT, SQUARE),
    "occlusion_upper_face_first": (lambda: two_triangles(0.3, 0.0), FRONT, 1.0, False, INPAINT, SQUARE),
    "coplanar_copies": (coplanar_copies, FRONT, 1.0, False, INPAINT, SQUARE),
    "mixed_facing": (mixed_facing, FRONT, 1.0, False, INPAINT, SQUARE),
    "mixed_facing_flipped": (mixed_facing, FRONT, 1.0, True, INPAINT, SQUARE),
    "centre_grid": (centre_grid, FRONT, 1.0, False, INPAINT, SQUARE),
    "height_field_oblique": (height_field, OBLIQUE, 0.45, False, INPAINT, SQUARE),
    "height_field_oblique_overpaint": (height_field, OBLIQUE, 0.45, False, OVERPAINT, DISC),
    "height_field_oblique_erase": (height_field, OBLIQUE, 0.45, False, ERASE, DISC),
    "height_field_whole": (height_field, FRONT, 1.1, False, INPAINT, SQUARE),
    "height_field_flipped": (height_field, OBLIQUE, 0.45, True, INPAINT, SQUARE),
    "one_face": (lambda: first_faces(height_field(), 1), ((-0.95, -0.7, 0.1), (0, 0, 1), (-0.95, 0, 0.1)), 0.1, False, INPAINT, SQUARE),
    "faces_257": (lambda: first_faces(height_field(), 257), FRONT, 1.1, False, INPAINT, DISC),
    "far_vertex": (far_vertex, FRONT, 1.0, False, INPAINT, SQUARE),
    "window_without_a_face": (height_field, ((5, 5, 0), (0, 0, 1), (5, 6, 0)), 0.5, False, INPAINT, SQUARE),
}


def _mask(kind):
    return stroke_ref.disc_mask(R) if kind == DISC else stroke_ref.make_stamp_mask(R, 1)


_ref = {}


def reference(case, texture, dec):
    """Computed once per case and left unchanged."""
    if case not in _ref:
        make, pose, fov, flip, mode, kind = CASES[case]
        v, f, uv = make()
        cam = mesh_ref.camera(*pose, fov)
        canvas, face_idx, proj = mesh_ref.render(v, f, uv, cam, fov, texture, R, flip, mode, OVER)
        pasted, info = mesh_ref.backproject(proj, face_idx, uv, None if mode == ERASE else dec, _mask(kind), texture)
        _ref[case] = dict(mesh=(v, f, uv), canvas=canvas, face_idx=face_idx, proj=proj, pasted=pasted, info=info)
    return _ref[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_render_and_backproject_kernels_match_the_restatement(model, texture, dec, case):
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    _, pose, fov, flip, mode, kind = CASES[case]
    ref = reference(case, texture, dec)
    mesh = model.load_mesh(*ref["mesh"])
    cam = mesh_camera(*pose, fov)
    assert (cam.numpy() == mesh_ref.camera(*pose, fov)).all()
    dtex = texture.to(DEV)
    canvas, face_idx = ops.mesh_render(mesh, cam, fov, dtex, R, flip_normals=flip, mode=mode, over_y=OVER[0], over_x=OVER[1])
    assert torch.equal(face_idx.cpu(), ref["face_idx"])
    assert torch.equal(canvas.cpu(), ref["canvas"])
    assert torch.equal(dtex.cpu(), texture)  # the render reads only
    out = ops.mesh_backproject(mesh, None if mode == ERASE else dec.to(DEV), _mask(kind).to(DEV), face_idx, dtex)
    assert out.data_ptr() == dtex.data_ptr()
    out = out.cpu()
    assert torch.equal(out, ref["pasted"])
    written = torch.from_numpy(ref["info"]["written"])
    assert torch.equal(out[~written], texture[~written])  # texels no valid face covers: bit-unchanged
    mesh.close()

    # what each case is there for
    fi, valid = ref["face_idx"], ref["info"]["valid"]
    shown = set(fi[fi >= 0].tolist())
    if case.startswith("quad") and "outside" not in case:
        assert shown == {0, 1} and int((fi < 0).sum()) == 0
    if case == "quad_partly_outside":
        assert 0 < int((fi >= 0).sum()) < R * R
    if case == "occlusion_upper_face_second":
        assert shown == {0, 1} and _both_cover(ref, winner=1)
    if case == "occlusion_upper_face_first":
        assert shown == {0, 1} and _both_cover(ref, winner=0)
    if case == "coplanar_copies":
        assert shown == {0} and list(valid) == [True, False]
    if case == "mixed_facing":
        assert shown == {0, 2} and list(valid) == [True, False, False, False]   # 1 is back-facing, 3 has no area; 2 is shown, not pasted
        assert 0 < ref["proj"]["nzu"][2] < 0.5
    if case == "mixed_facing_flipped":
        assert shown == {1} and list(valid) == [False, True, False, False]
    if case == "centre_grid":
        # every centre of columns [3, 63) x rows [0, 62) is owned once: the right column and the bottom row are not top-left
        want = torch.zeros(R, R, dtype=torch.bool)
        want[0:62, 3:63] = True
        assert torch.equal(fi >= 0, want)
        tf = torch.from_numpy(ref["info"]["tex_face"] >= 0)
        want_t = torch.zeros(H, W, dtype=torch.bool)
        want_t[2:95, 4:159] = True
        assert torch.equal(tf, want_t)
    if case.startswith("height_field_oblique"):
        assert len(shown) > 100 and 0 < int(valid.sum()) < len(shown)  # some shown faces are steep
    if case == "height_field_whole":
        assert len(shown) == 384 and int((fi < 0).sum()) > 0           # the window looks past the mesh's border
    if case == "one_face":
        assert shown == {0} and int(written.sum()) > 0
    if case == "faces_257":
        assert max(shown) == 256
    if case == "far_vertex":
        assert int(ref["proj"]["X"].max()) == 1 << 26 and shown == {0}
    if case == "window_without_a_face":
        assert not shown and int(written.sum()) == 0 and float(ref["canvas"].abs().max()) == 0.0
    if mode == ERASE and shown:
        assert int(out[written].sum()) == 0 and int(written.sum()) > 0
    if mode == OVERPAINT:
        assert float(ref["canvas"][..., OVER[0]:R - OVER[0], OVER[1]:R - OVER[1]].abs().max()) == 0.0


def _both_cover(ref, winner):
    """Some pixel is covered by both triangles and goes to `winner`."""
    p = ref["proj"]
    py, px = np.meshgrid(np.arange(R, dtype=np.int64) * 256 + 128, np.arange(R, dtype=np.int64) * 256 + 128, indexing="ij")
    both = mesh_ref.cover(p["X"][0], p["Y"][0], px, py)[0] & mesh_ref.cover(p["X"][1], p["Y"][1], px, py)[0]
    return both.sum() > 100 and (ref["face_idx"].numpy()[both] == winner).all()


def test_the_quad_is_the_2d_stroke(model, dec):
    """Power-of-two sizes make every barycentric weight exact (tests/test_mesh_cpu.py): on a 64 x 64 texture the quad's render IS
    ops.stroke_gather at (0, 0) and its backprojection IS ops.stroke_paste."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    tex = make_texture(R, R, 1064)
    mesh = model.load_mesh(*quad())
    cam = mesh_camera(*FRONT, 1.0)
    for mode in (INPAINT, OVERPAINT):
        canvas, face_idx = ops.mesh_render(mesh, cam, 1.0, tex.to(DEV), R, mode=mode, over_y=OVER[0], over_x=OVER[1])
        assert torch.equal(canvas, ops.stroke_gather(tex.to(DEV), [0], [0], R, modes=[mode], over_y=OVER[0], over_x=OVER[1]))
    for mask in (stroke_ref.make_stamp_mask(R, 3), stroke_ref.disc_mask(R)):
        a = ops.mesh_backproject(mesh, dec.to(DEV), mask.to(DEV), face_idx, tex.to(DEV))
        b = ops.stroke_paste(dec[None].to(DEV), mask.to(DEV), tex.to(DEV), [0], [0])
        assert torch.equal(a, b) and not torch.equal(a.cpu(), tex)
        a = ops.mesh_backproject(mesh, None, mask.to(DEV), face_idx, tex.to(DEV))
        b = ops.stroke_paste(None, mask.to(DEV), tex.to(DEV), [0], [0], modes=[ERASE])
        assert torch.equal(a, b)


# ---------------------------------------------------------------- strokes against the host loop
# three stamps over the height field whose footprints overlap
STROKE = dict(positions=[(0.1, -0.05, 0.1), (0.3, 0.05, 0.1), (0.2, 0.2, 0.1)],
              normals=[(0.35, -0.2, 0.9), (0.0, 0.0, 1.0), (-0.2, 0.1, 0.95)],
              prevs=[(0.0, 0.3, 0.15), (0.1, -0.05, 0.1), (0.3, 0.05, 0.1)],
              fov=[0.45, 0.4, 0.5])


def host_mesh_stroke(model, mesh, tex, positions, normals, prevs, fov, seeds, modes, margin=1, mask=None, flip=False):
    """TexturePainterManager.stamp (manager.py:232-271) on the host: one render, one generate_raw and one backprojection per stamp."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    tex = tex.clone()
    for i in range(len(positions)):
        cam = mesh_camera(positions[i], normals[i], prevs[i], fov[i])
        canvas, face_idx = ops.mesh_render(mesh, cam, fov[i], tex, R, flip_normals=flip, mode=modes[i], over_y=OVER[0], over_x=OVER[1])
        if modes[i] == ERASE:
            m = mask if mask is not None else stroke_ref.disc_mask(R)
            ops.mesh_backproject(mesh, None, m.to(DEV), face_idx, tex)
            continue
        painted = model.generate_raw(canvas, seeds=[seeds[i]], **ST)
        m = mask if mask is not None else stroke_ref.make_stamp_mask(R, margin)
        ops.mesh_backproject(mesh, None, m.to(DEV), face_idx, tex, painted=painted)
    return tex


def test_stroke_equals_the_host_loop(model, texture):
    mesh = model.load_mesh(*height_field())
    modes = [INPAINT, OVERPAINT, ERASE]
    seeds = [700, 701, 702]
    tex = texture.to(DEV)
    out = model.paint_mesh_stroke(mesh, tex, STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"], seeds=700,
                                  modes=["inpaint", "overpaint", "erase"], overpaint_margins=OVER, **ST)
    assert out is tex
    assert model.stroke_info() == dict(stamps=3, groups=3, unet_evals=2 * 3)  # DDIM, 4 steps: 3 evaluations; the Erase stamp runs none
    want = host_mesh_stroke(model, mesh, texture.to(DEV), STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"], seeds, modes)
    assert torch.equal(out, want)
    changed = (out.cpu() != texture).any(dim=-1)
    assert 200 < int(changed.sum()) < H * W
    # the stroke is a function of its arguments: again, on a fresh copy, with a caller's mask for every stamp
    disc = stroke_ref.disc_mask(R)
    a = model.paint_mesh_stroke(mesh, texture.to(DEV), STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"], seeds=seeds,
                                modes=modes, mask=disc, **ST)
    b = host_mesh_stroke(model, mesh, texture.to(DEV), STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"], seeds, modes,
                         mask=disc)
    assert torch.equal(a, b) and not torch.equal(a, want)


def test_quad_stroke_equals_paint_stroke(model):
    """The mesh stroke over the full-window quad is the 2D stroke at (0, 0), byte for byte (margin: the same square mask)."""
    tex = make_texture(R, R, 1064)
    mesh = model.load_mesh(*quad())
    for mode, margin in ((INPAINT, 1), (OVERPAINT, 4)):
        a = model.paint_mesh_stroke(mesh, tex.to(DEV), [FRONT[0]], [FRONT[1]], [FRONT[2]], 1.0, seeds=[41], modes=mode, margin=margin, **ST)
        b = model.paint_stroke(tex.to(DEV), [(0, 0)], seeds=[41], modes=mode, margin=margin, **ST)
        assert torch.equal(a, b) and not torch.equal(a.cpu(), tex)


def test_a_window_off_the_mesh_paints_nothing(model, texture):
    mesh = model.load_mesh(*height_field())
    tex = texture.to(DEV)
    # far from the bounding box of the mesh: skipped on the host, no stamp runs
    model.paint_mesh_stroke(mesh, tex, [(50, 50, 0)], [(0, 0, 1)], [(50, 51, 0)], 0.5, seeds=1, **ST)
    assert model.stroke_info() == dict(stamps=1, groups=1, unet_evals=0)
    # inside the bounding box of the vertices, but the one face of this mesh is in a corner: the stamp runs and nothing is pasted
    lonely = model.load_mesh(*first_faces(height_field(), 1))
    model.paint_mesh_stroke(lonely, tex, [(0, 0, 0)], [(0, 0, 1)], [(0, 1, 0)], 0.25, seeds=1, **ST)
    assert model.stroke_info() == dict(stamps=1, groups=1, unet_evals=3)
    assert torch.equal(tex.cpu(), texture)


def test_mesh_stroke_enqueue_does_not_block_the_host(model, texture):
    """The criterion of test_stroke_enqueue_does_not_block_the_host: the host is back long before the device is done."""
    mesh = model.load_mesh(*height_field())
    tex = texture.to(DEV)
    args = (STROKE["positions"] * 2, STROKE["normals"] * 2, STROKE["prevs"] * 2, STROKE["fov"] * 2)
    for _ in range(2):  # programs, graphs and the masks exist from here on
        model.paint_mesh_stroke(mesh, tex, *args, seeds=1, **ST)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.paint_mesh_stroke(mesh, tex, *args, seeds=1, **ST)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"host enqueue of a 6-stamp mesh stroke {t_host * 1e3:.1f} ms, device done after {t_all * 1e3:.1f} ms")
    assert t_host < 0.5 * t_all


def test_refusals_leave_the_texture_alone(model, texture):
    from diffusiontexturepainting_amd import _lib, synthetic, weights as Wt
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    mesh = model.load_mesh(*height_field())
    tex = texture.to(DEV)
    P, N, V, F = STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"]

    def refused(code, pattern, t=None, mesh_=None, **kw):
        t = tex if t is None else t
        before = t.clone()
        with pytest.raises(DtpError) as e:
            model.paint_mesh_stroke(mesh_ or mesh, t, kw.pop("positions", P), kw.pop("normals", N), kw.pop("prevs", V), kw.pop("fov", F),
                                    seeds=3, **kw, **ST)
        torch.cuda.synchronize()
        assert re.search(rf"\(code {code}\)", str(e.value)) and re.search(pattern, str(e.value)), str(e.value)
        assert torch.equal(t, before)

    refused(3, r"stamp 1\b.*slot 5", slots=[0, 5, 0])                          # an unset slot: DTP_ERR_STATE, as dtp_stamp_seeded
    refused(1, r"slot 16 of stamp 2\b", slots=[0, 0, 16])
    refused(1, r"stamp 1\b.*mode 7", modes=[0, 7, 0])
    refused(1, r"stamp 2\b.*Overpaint", modes=[0, 0, 2], overpaint_margins=(32, 25))
    refused(1, r"margin=32", margin=32)
    refused(1, r"margin=-1", margin=-1)
    refused(1, r"stamp 1: the normal is zero", normals=[N[0], (0, 0, 0), N[2]])
    refused(1, r"stamp 2: up = prev - pos is zero or parallel", prevs=[V[0], V[1], P[2]])
    refused(1, r"stamp 0: a non-finite", positions=[(float("nan"), 0, 0), P[1], P[2]])
    refused(1, r"stamp 2: fov=0", fov=[0.4, 0.4, 0.0])
    # a destroyed mesh; the mesh of another handle
    dead = model.load_mesh(*quad())
    handle = dead.handle
    dead.close()
    dead._h = handle
    refused(1, r"not a live mesh", mesh_=dead)
    dead._h = None
    sd = dict(unet=Wt.synthetic_unet(5), lora=Wt.synthetic_lora(5), vae=Wt.synthetic_vae(5))
    other = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=1)
    theirs = other.load_mesh(*quad())
    refused(1, r"another handle", mesh_=theirs)
    theirs.close()
    del other
    # NULL pointers and an empty texture: the C entry point itself
    lib = _lib.load()
    stamps = (_lib.MeshStamp * 1)(_lib.MeshStamp((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0, 0, 0, 1))
    st = _lib.Settings(4, 9, 2, 2.5, 1.0, 0, 0)
    opts = _lib.MeshStrokeOpts(0, 1, 10, 25, 1, 1.0)
    before = tex.clone()
    good = [model._h, mesh.handle, _lib.ptr(tex), H, W, stamps, 1, st, opts, None, model._s()]
    for i in (0, 1, 2, 5, 7, 8):
        bad = list(good)
        bad[i] = None
        assert lib.dtp_mesh_stroke(*bad) == 1 and b"NULL" in lib.dtp_last_error()
    for i, v in ((3, 0), (4, 0), (3, -5), (6, 0)):
        bad = list(good)
        bad[i] = v
        assert lib.dtp_mesh_stroke(*bad) == 1, lib.dtp_last_error()
    bad_st = _lib.Settings(4, 9, 2, 2.5, 1.0, 1, 0)  # composite set: dtp_stamp_seeded's own check of a pasting stamp
    bad = list(good)
    bad[7] = bad_st
    assert lib.dtp_mesh_stroke(*bad) == 1 and b"composite" in lib.dtp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(tex, before)
    with pytest.raises(ValueError, match="uint8"):
        model.paint_mesh_stroke(mesh, tex.float(), P, N, V, F, **ST)
    with pytest.raises(ValueError, match="load_mesh"):
        model.paint_mesh_stroke(None, tex, P, N, V, F, **ST)
    # an Erase stamp needs no slot
    model.paint_mesh_stroke(mesh, tex.clone(), P, N, V, F, seeds=3, modes=[0, "erase", 0], slots=[0, 5, 0], **ST)
    torch.cuda.synchronize()
