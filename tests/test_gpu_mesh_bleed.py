"""The bleed pass of the mesh strokes (dtp_mesh_stroke_bleed, dtp_mesh_bleed, dtp_op_mesh_coverage; `paint_mesh_stroke(bleed=k)`,
`bleed_texture`, `ops.mesh_coverage`) against the numpy restatement of the contract (tests/bleed_ref.py): the coverage mask, the pass
over whole textures and rectangles, and strokes against the host loop, all with torch.equal -- the contract is integer arithmetic --,
the seam a second render sees, enqueue without a host wait, and the refusals.  One 64^2 context, DDIM, 4 steps, as tests/test_gpu_mesh.py."""
import re
import time

import numpy as np
import pytest
import torch

import bleed_ref
import mesh_ref
import stroke_ref
from mesh_ref import ERASE, INPAINT, OVERPAINT

pytestmark = pytest.mark.gpu

R = 64
H, W = 96, 160
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
OVER = (10, 25)
DEV = "cuda:0"


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


# ---------------------------------------------------------------- meshes
def quad():
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_quad()


def height_field():
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_height_field(17, 13, seed=3)


def from_uvs(uvs):
    """A mesh for its UVs alone: coverage looks at no vertex."""
    uv = torch.tensor(uvs, dtype=torch.float32)
    n = uv.shape[0]
    return torch.zeros(3 * n, 3), torch.arange(3 * n, dtype=torch.int32).reshape(n, 3), uv


def sliver():
    """One face with an area, thinner than a texel and between two rows of centres: it holds no centre of a 96 x 160 texture."""
    return from_uvs([[[0.1, 0.5 - 0.1 / H], [0.9, 0.5 - 0.2 / H], [0.9, 0.5 - 0.4 / H]]])


def shared_edge():
    """Two faces of opposite winding that share the edge (0.2, 0.9) - (0.7, 0.15), which crosses texel centres at no special place."""
    return from_uvs([[[0.2, 0.9], [0.7, 0.15], [0.05, 0.1]], [[0.2, 0.9], [0.7, 0.15], [0.95, 0.8]]])


def partly_outside():
    return from_uvs([[[-0.4, 0.3], [0.6, -0.3], [0.5, 1.4]], [[0.8, 0.8], [1.7, 0.9], [0.9, 2.5]]])


def islands(h, w):
    """3 x 3-texel squares every 10 columns and 9 rows: gutters 7 and 6 texels wide, so that a gutter texel has sources at equal
    distances to its left and right, and above and beside it."""
    uvs = []
    for y in range(2, h - 3, 9):
        for x in range(2, w - 3, 10):
            a, b, c, d = (x / w, 1 - y / h), ((x + 3) / w, 1 - y / h), ((x + 3) / w, 1 - (y + 3) / h), (x / w, 1 - (y + 3) / h)
            uvs += [[a, b, c], [a, c, d]]
    return from_uvs(uvs)


COVERAGE = {
    "quad_every_texel": (quad, 64, 64),
    "height_field": (height_field, H, W),
    "height_field_75x101": (height_field, 75, 101),
    "sliver_without_a_centre": (sliver, H, W),
    "shared_edge": (shared_edge, H, W),
    "partly_outside_the_unit_square": (partly_outside, H, W),
    "one_texel": (quad, 1, 1),
    "islands_75x101": (lambda: islands(75, 101), 75, 101),
}
_cov = {}


def coverage_ref(name):
    """Computed once per case and left unchanged."""
    if name not in _cov:
        make, h, w = COVERAGE[name]
        mesh = make()
        _cov[name] = (mesh, bleed_ref.coverage(mesh[2], h, w))
    return _cov[name]


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("name", sorted(COVERAGE))
def test_coverage_matches_the_restatement(model, name):
    from diffusiontexturepainting_amd import ops
    _, h, w = COVERAGE[name]
    mesh_data, want = coverage_ref(name)
    mesh = model.load_mesh(*mesh_data)
    got = ops.mesh_coverage(mesh, h, w)
    assert got.dtype == torch.bool and tuple(got.shape) == (h, w)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(ops.mesh_coverage(mesh, h, w), got)  # the kept mask
    mesh.close()
    # what each case is there for
    if name in ("quad_every_texel", "one_texel"):
        assert want.all()
    if name == "sliver_without_a_centre":
        X, Y = bleed_ref.snap_uvs(mesh_data[2], h, w)
        assert mesh_ref.orient(X[0, 0], Y[0, 0], X[0, 1], Y[0, 1], X[0, 2], Y[0, 2]) != 0 and not want.any()
    if name == "shared_edge":
        # the union of the two faces is the quadrilateral: every row's covered texels are one run without a hole
        for row in want:
            cols = np.nonzero(row)[0]
            assert len(cols) == 0 or len(cols) == cols.max() - cols.min() + 1
        assert want.sum() > 4000
    if name == "partly_outside_the_unit_square":
        assert want[:, 0].any() and want[0, :].any() and want[:, -1].any() and 0 < want.sum() < h * w
    if name.startswith("height_field"):
        assert 0 < want.sum() < h * w and not want[:, w // 2].any()  # the gutter between the two charts


def test_another_size_rebuilds_the_mask(model):
    from diffusiontexturepainting_amd import ops
    mesh = model.load_mesh(*height_field())
    for name in ("height_field", "height_field_75x101", "height_field"):
        _, h, w = COVERAGE[name]
        assert torch.equal(ops.mesh_coverage(mesh, h, w).cpu(), torch.from_numpy(coverage_ref(name)[1]))
    mesh.close()


def _extreme(model, mesh_data, what):
    """Coverage of a 2048^2 texture, first use: allocation, kernels and the wait, bounded by the wall time of a quick test (1 s: it is
    a bound on the shape of the work -- a pass that is quadratic in faces x tiles does not meet it -- not a measurement)."""
    from diffusiontexturepainting_amd import ops
    T = 2048
    want = torch.from_numpy(bleed_ref.coverage_batched(mesh_data[2], T, T)).to(DEV)
    mesh = model.load_mesh(*mesh_data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = ops.mesh_coverage(mesh, T, T)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"coverage of 2048^2 by {what}: first use {dt * 1e3:.2f} ms, {int(want.sum())} texels covered")
    assert torch.equal(got, want)
    mesh.close()
    assert dt < 1.0
    return want


def test_coverage_extreme_two_faces_over_2048(model):
    want = _extreme(model, quad(), "2 faces")
    assert bool(want.all())


def test_coverage_extreme_100k_faces_over_2048(model):
    from diffusiontexturepainting_amd import synthetic
    data = synthetic.make_height_field(225, 225, seed=3)
    assert data[1].shape[0] == 100352
    want = _extreme(model, data, "100 352 faces")
    assert 0 < int(want.sum()) < 2048 * 2048


# ---------------------------------------------------------------- the pass
RECTS = {
    "whole": None,
    "cuts_tiles": (70, 30, 90, 47),
    "corner_top_left": (0, 0, 20, 10),
    "corner_bottom_right": (140, 80, 159, 95),
    "clipped_to_the_texture": (-7, -3, 11, 200),
    "one_texel": (79, 40, 79, 40),
}


@pytest.mark.parametrize("k", [1, 2, 5, 16])
@pytest.mark.parametrize("rect", sorted(RECTS))
def test_pass_on_the_height_field(model, k, rect):
    mesh_data, cov = coverage_ref("height_field")
    mesh = model.load_mesh(*mesh_data)
    tex = random_texture(H, W, 300 + k)
    r = RECTS[rect]
    clipped = None if r is None else (max(r[0], 0), max(r[1], 0), min(r[2], W - 1), min(r[3], H - 1))
    want = bleed_ref.bleed(tex, cov, k, clipped)
    dtex = tex.to(DEV)
    out = model.bleed_texture(mesh, dtex, k, rect=r)
    assert out is dtex
    assert torch.equal(out.cpu(), want)
    if rect == "whole" or k >= 5:
        assert not torch.equal(want, tex)
    assert torch.equal(want[torch.from_numpy(cov)], tex[torch.from_numpy(cov)])  # covered texels are only read
    again = model.bleed_texture(mesh, out.clone(), k, rect=r)
    assert torch.equal(again, out)  # a second application changes nothing
    mesh.close()


@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_pass_on_islands_with_equidistant_sources(model, k):
    h, w = 75, 101
    mesh_data, cov = coverage_ref("islands_75x101")
    assert cov[2:5, 2:5].all() and not cov[2:5, 5:12].any() and cov[2:5, 12:15].all() and not cov[5:11, 2:5].any() and cov[11:14, 2:5].all()
    mesh = model.load_mesh(*mesh_data)
    tex = random_texture(h, w, 400 + k)
    want = bleed_ref.bleed(tex, cov, k)
    out = model.bleed_texture(mesh, tex.to(DEV), k)
    assert torch.equal(out.cpu(), want)
    if k >= 5:
        # islands cover rows and columns 2..4, rows 11..13, columns 12..14
        assert torch.equal(want[3, 8], tex[3, 4]) and not torch.equal(tex[3, 4], tex[3, 12])    # (0, -4) before (0, 4)
        assert torch.equal(want[7, 4], tex[4, 4])                                                # 3 above, 4 below
        assert torch.equal(want[8, 8], tex[11, 4]) and not torch.equal(tex[11, 4], tex[11, 12])  # (3, -4) before (3, 4)
        assert torch.equal(want[7, 7], tex[4, 4])                                                # (-3, -3), not (4, -3)
    assert torch.equal(model.bleed_texture(mesh, out.clone(), k), out)
    mesh.close()


def test_radius_zero_and_an_empty_rectangle_do_nothing(model):
    mesh = model.load_mesh(*height_field())
    tex = random_texture(H, W, 9)
    assert torch.equal(model.bleed_texture(mesh, tex.to(DEV), 0).cpu(), tex)
    assert torch.equal(model.bleed_texture(mesh, tex.to(DEV), 4, rect=(200, 10, 300, 20)).cpu(), tex)   # right of the texture
    assert torch.equal(model.bleed_texture(mesh, tex.to(DEV), 4, rect=(10, -30, 20, -1)).cpu(), tex)    # above it
    mesh.close()


# ---------------------------------------------------------------- strokes
# the three stamps of tests/test_gpu_mesh.py: their windows span x = -0.35 .. 0.8 and so the seam between the charts at x = 0
STROKE = dict(positions=[(0.1, -0.05, 0.1), (0.3, 0.05, 0.1), (0.2, 0.2, 0.1)],
              normals=[(0.35, -0.2, 0.9), (0.0, 0.0, 1.0), (-0.2, 0.1, 0.95)],
              prevs=[(0.0, 0.3, 0.15), (0.1, -0.05, 0.1), (0.3, 0.05, 0.1)],
              fov=[0.45, 0.4, 0.5])
ARGS = (STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"])


def host_loop(model, mesh, mesh_data, tex, seeds, modes, k, positions=None, normals=None, prevs=None, fov=None):
    """Per stamp: ops.mesh_render -> generate_raw -> ops.mesh_backproject -> the restatement's pass over the contract's rectangle."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    positions, normals, prevs, fov = positions or ARGS[0], normals or ARGS[1], prevs or ARGS[2], fov or ARGS[3]
    v, f, uv = mesh_data
    h, w = tex.shape[:2]
    cov = bleed_ref.coverage(uv, h, w)
    tex = tex.clone()
    rects = []
    for i in range(len(positions)):
        cam = mesh_camera(positions[i], normals[i], prevs[i], fov[i])
        canvas, face_idx = ops.mesh_render(mesh, cam, fov[i], tex, R, mode=modes[i], over_y=OVER[0], over_x=OVER[1])
        if modes[i] == ERASE:
            ops.mesh_backproject(mesh, None, stroke_ref.disc_mask(R).to(DEV), face_idx, tex)
        else:
            painted = model.generate_raw(canvas, seeds=[seeds[i]], **ST)
            ops.mesh_backproject(mesh, None, stroke_ref.make_stamp_mask(R, 1).to(DEV), face_idx, tex, painted=painted)
        if k:
            proj = mesh_ref.project(v, f, mesh_ref.camera(positions[i], normals[i], prevs[i], fov[i]), fov[i], R)
            rect = bleed_ref.stamp_rect(proj, face_idx, uv, h, w, k)
            rects.append(rect)
            if rect is not None:
                tex = bleed_ref.bleed(tex, cov, k, rect).to(DEV)
    return tex, rects


def test_stroke_with_bleed_equals_the_host_loop(model):
    data = height_field()
    mesh = model.load_mesh(*data)
    texture = random_texture(H, W, 77)
    modes, seeds = [INPAINT, OVERPAINT, ERASE], [700, 701, 702]
    out = model.paint_mesh_stroke(mesh, texture.to(DEV), *ARGS, seeds=700, modes=["inpaint", "overpaint", "erase"],
                                  overpaint_margins=OVER, bleed=2, **ST)
    want, rects = host_loop(model, mesh, data, texture.to(DEV), seeds, modes, 2)
    assert torch.equal(out, want)
    assert all(r is not None for r in rects)
    cov = torch.from_numpy(bleed_ref.coverage(data[2], H, W))
    gutter = (out.cpu() != texture).any(dim=-1) & ~cov
    assert int(gutter.sum()) > 50 and bool(gutter[:, 75:85].any())  # the pass wrote, and wrote between the charts
    # without the pass the same stroke leaves every uncovered texel alone, and the covered ones are the same bytes
    plain = model.paint_mesh_stroke(mesh, texture.to(DEV), *ARGS, seeds=700, modes=modes, overpaint_margins=OVER, **ST).cpu()
    assert torch.equal(plain[~cov], texture[~cov]) and not torch.equal(plain, out.cpu())
    mesh.close()


def test_bleed_zero_is_the_mesh_stroke(model):
    """bleed=0 through either entry point is dtp_mesh_stroke: the same bytes as the host loop of tests/test_gpu_mesh.py."""
    import ctypes as C
    from diffusiontexturepainting_amd import _lib, mesh as _mesh
    data = height_field()
    mesh = model.load_mesh(*data)
    texture = random_texture(H, W, 77)
    modes, seeds = [INPAINT, OVERPAINT, ERASE], [700, 701, 702]
    a = model.paint_mesh_stroke(mesh, texture.to(DEV), *ARGS, seeds=seeds, modes=modes, overpaint_margins=OVER, bleed=0, **ST)
    want, _ = host_loop(model, mesh, data, texture.to(DEV), seeds, modes, 0)
    assert torch.equal(a, want)
    stamps = _mesh.mesh_stamps(*ARGS, seeds, modes, None)
    st = _lib.Settings(ST["steps"], ST["context_pad"], ST["tg_steps"], ST["cfg_weight"], 1.0, 0, 0)
    opts = _lib.MeshStrokeOpts(0, 1, OVER[0], OVER[1], 1, 1.0)
    b = texture.to(DEV)
    torch.cuda.synchronize()
    rc = _lib.load().dtp_mesh_stroke_bleed(model._h, mesh.handle, _lib.ptr(b), H, W, stamps, 3, C.byref(st), C.byref(opts), None, 0, model._s())
    assert rc == 0, _lib.load().dtp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    mesh.close()


def test_stroke_on_a_bled_texture_is_a_fixed_point_of_the_pass(model):
    mesh = model.load_mesh(*height_field())
    tex = model.bleed_texture(mesh, random_texture(H, W, 78).to(DEV), 2)
    before = tex.clone()
    out = model.paint_mesh_stroke(mesh, tex, *ARGS, seeds=40, modes=["inpaint", "inpaint", "overpaint"], overpaint_margins=OVER, bleed=2, **ST)
    assert not torch.equal(out, before)
    assert torch.equal(model.bleed_texture(mesh, out.clone(), 2), out)
    # a stroke without the pass on the same texture is none: the gutter along what it painted is stale
    plain = model.paint_mesh_stroke(mesh, before.clone(), *ARGS, seeds=40, modes=["inpaint", "inpaint", "overpaint"], overpaint_margins=OVER, **ST)
    assert not torch.equal(model.bleed_texture(mesh, plain.clone(), 2), plain)
    mesh.close()


def test_an_erase_stamp_bleeds_zeros(model):
    data = height_field()
    mesh = model.load_mesh(*data)
    full = torch.full((H, W, 4), 255, dtype=torch.uint8)
    out = model.paint_mesh_stroke(mesh, full.to(DEV), [ARGS[0][1]], [ARGS[1][1]], [ARGS[2][1]], [ARGS[3][1]], modes="erase", bleed=3, **ST)
    assert model.stroke_info()["unet_evals"] == 0
    want, rects = host_loop(model, mesh, data, full.to(DEV), [0], [ERASE], 3, [ARGS[0][1]], [ARGS[1][1]], [ARGS[2][1]], [ARGS[3][1]])
    assert torch.equal(out, want)
    cov = torch.from_numpy(bleed_ref.coverage(data[2], H, W))
    out = out.cpu()
    zero = (out == 0).all(dim=-1)
    assert int((zero & cov).sum()) > 100 and int((zero & ~cov).sum()) > 10  # erased texels, and the zeros bled into the gutter
    assert bool(((out == 0) | (out == 255)).all())
    mesh.close()


def test_the_seam_closes_on_the_device_render(model):
    """The figure of tests/test_mesh_bleed_cpu.py on the device: a blank 256^2 texture, one stamp over the default height field, and a
    render of the same window.  The interior canvas alpha (8 px in, a face shown) is the next stamp's inpainting mask."""
    from diffusiontexturepainting_amd import ops, synthetic
    from diffusiontexturepainting_amd.mesh import mesh_camera
    T = 256
    pose, fov = ((0, 0, 0.2), (0, 0, 1), (0, -1, 0.2)), 0.45
    mesh = model.load_mesh(*synthetic.make_height_field())
    cam = mesh_camera(*pose, fov)
    low = {}
    for k in (0, 1, 4):
        tex = torch.zeros(T, T, 4, dtype=torch.uint8, device=DEV)
        model.paint_mesh_stroke(mesh, tex, [pose[0]], [pose[1]], [pose[2]], fov, seeds=11, bleed=k, **ST)
        canvas, face_idx = ops.mesh_render(mesh, cam, fov, tex, R)
        interior = torch.zeros(R, R, dtype=torch.bool, device=DEV)
        interior[8:R - 8, 8:R - 8] = True
        interior &= face_idx != -1
        assert int(interior.sum()) == 2304
        alpha = canvas[0, 3][interior]
        low[k] = float(alpha.min())
        print(f"bleed {k}: min interior alpha {low[k]:.5f}, {int((alpha < 0.999).sum())} of 2304 below 0.999")
    assert low[1] >= 254 / 255 - 1e-6 and low[4] >= 254 / 255 - 1e-6
    assert low[1] > low[0] and low[4] > low[0]
    mesh.close()


def test_stroke_with_bleed_does_not_block_the_host(model):
    """The criterion of test_mesh_stroke_enqueue_does_not_block_the_host: the host is back long before the device is done."""
    mesh = model.load_mesh(*height_field())
    tex = random_texture(H, W, 77).to(DEV)
    args = tuple(a * 2 for a in ARGS)
    for _ in range(2):  # programs, graphs, the masks and the coverage exist from here on
        model.paint_mesh_stroke(mesh, tex, *args, seeds=1, bleed=2, **ST)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.paint_mesh_stroke(mesh, tex, *args, seeds=1, bleed=2, **ST)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"host enqueue of a 6-stamp mesh stroke with bleed {t_host * 1e3:.1f} ms, device done after {t_all * 1e3:.1f} ms")
    assert t_host < 0.5 * t_all
    mesh.close()


def test_refusals_leave_the_texture_alone(model):
    from diffusiontexturepainting_amd._lib import DtpError
    mesh = model.load_mesh(*height_field())
    tex = random_texture(H, W, 77).to(DEV)
    before = tex.clone()

    def refused(code, pattern, call):
        with pytest.raises(DtpError) as e:
            call()
        torch.cuda.synchronize()
        assert re.search(rf"\(code {code}\)", str(e.value)) and re.search(pattern, str(e.value)), str(e.value)
        assert torch.equal(tex, before)

    refused(1, r"dtp_mesh_stroke_bleed: bleed=17", lambda: model.paint_mesh_stroke(mesh, tex, *ARGS, seeds=3, bleed=17, **ST))
    refused(1, r"bleed=-1", lambda: model.paint_mesh_stroke(mesh, tex, *ARGS, seeds=3, bleed=-1, **ST))
    # what dtp_mesh_stroke refuses is refused with the pass as well, under the entry point's own name
    refused(3, r"dtp_mesh_stroke_bleed: stamp 1\b.*slot 5", lambda: model.paint_mesh_stroke(mesh, tex, *ARGS, seeds=3, slots=[0, 5, 0], bleed=2, **ST))
    refused(1, r"stamp 2: fov=0", lambda: model.paint_mesh_stroke(mesh, tex, ARGS[0], ARGS[1], ARGS[2], [0.4, 0.4, 0.0], seeds=3, bleed=2, **ST))
    refused(1, r"margin=32", lambda: model.paint_mesh_stroke(mesh, tex, *ARGS, seeds=3, margin=32, bleed=2, **ST))
    refused(1, r"dtp_mesh_bleed: bleed=17", lambda: model.bleed_texture(mesh, tex, 17))
    refused(1, r"bleed=-2", lambda: model.bleed_texture(mesh, tex, -2))
    refused(1, r"x0 > x1", lambda: model.bleed_texture(mesh, tex, 2, rect=(30, 0, 10, 5)))
    refused(1, r"y0 > y1", lambda: model.bleed_texture(mesh, tex, 2, rect=(0, 6, 10, 5)))
    dead = model.load_mesh(*quad())
    handle = dead.handle
    dead.close()
    dead._h = handle
    refused(1, r"not a live mesh", lambda: model.bleed_texture(dead, tex, 2))
    refused(1, r"not a live mesh", lambda: model.paint_mesh_stroke(dead, tex, *ARGS, seeds=3, bleed=2, **ST))
    dead._h = None
    with pytest.raises(ValueError, match="uint8"):
        model.bleed_texture(mesh, tex.float(), 2)
    with pytest.raises(ValueError, match="load_mesh"):
        model.bleed_texture(None, tex, 2)
    with pytest.raises(ValueError, match="rect"):
        model.bleed_texture(mesh, tex, 2, rect=(1, 2, 3))
    assert torch.equal(tex, before)
    mesh.close()
