"""The view of a textured mesh (dtp_mesh_view, `model.render_view`, `ops.mesh_view`; include/dtp.h "a view of a textured mesh"): the
device's frame, face indices and depth against the numpy restatement (tests/view_ref.py) with torch.equal; the binned frame against the
unbinned one; a frame after a stroke; a live frame that answers while a stroke is still queued, and leaves the stroke's texture alone;
the refusals.  One 64^2 context with synthetic weights, DDIM.  Nothing is compared under a tolerance."""
import ctypes as C
import re
import time

import numpy as np
import pytest
import torch

import view_ref

pytestmark = pytest.mark.gpu

R = 64
DEV = "cuda:0"
f32 = np.float32
TH, TW = 96, 160


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


def make_texture(h, w, seed):
    """Seeded random RGBA bytes with alpha-0 (unpainted) regions, an alpha-255 region and every alpha in between."""
    t = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    t[h // 4: h // 2, w // 8: w // 2, 3] = 0
    t[h // 2:, w // 2:, 3] = 255
    t[: h // 8, :, 3] = 0
    return t


@pytest.fixture(scope="module")
def texture():
    return make_texture(TH, TW, 77)


# ---------------------------------------------------------------- meshes
def _t(v, f, uv):
    return (torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int32), torch.tensor(uv, dtype=torch.float32))


_cache = {}


def field(nx, ny, seed=0):
    from diffusiontexturepainting_amd import synthetic
    if (nx, ny, seed) not in _cache:
        _cache[nx, ny, seed] = synthetic.make_height_field(nx, ny, seed=seed)
    return _cache[nx, ny, seed]


def first_faces(mesh, n):
    v, f, uv = mesh
    return v, f[:n].contiguous(), uv[:n].contiguous()


def cube():
    """The cube [-0.5, 0.5]^3, 12 faces counter-clockwise seen from outside, each side a different patch of the texture."""
    v = [[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)]
    sides = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f, uv = [], []
    for s, (a, b, c, d) in enumerate(sides):
        u0, v0 = 0.05 + 0.3 * (s % 3), 0.05 + 0.45 * (s // 3)
        q = [(u0, v0), (u0 + 0.25, v0), (u0 + 0.25, v0 + 0.4), (u0, v0 + 0.4)]
        f += [[a, b, c], [a, c, d]]
        uv += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return _t(v, f, uv)


def both_windings():
    """Face 0 counter-clockwise seen from +z, face 1 clockwise, face 2 steep, face 3 of zero area on top of face 0, face 4 a sliver whose
    snapped area may vanish, face 5 under face 0, face 6 so large that its camera coordinates overflow under a camera whose up is the diagonal (1, 1, 0)."""
    return _t([[-0.9, -0.9, 0.0], [-0.1, -0.9, 0.0], [-0.5, -0.1, 0.0],
               [0.1, -0.9, 0.0], [0.9, -0.9, 0.0], [0.5, -0.1, 0.0],
               [-0.9, 0.1, 0.0], [-0.6, 0.1, 1.0], [-0.9, 0.9, 0.0],
               [-0.7, -0.8, 0.5], [-0.3, -0.4, 0.5], [-0.3, -0.4, 0.5],
               [0.2, 0.2, 0.0], [0.8, 0.8, 0.0], [0.5, 0.5 + 1e-9, 0.0],
               [-0.9, -0.9, -0.25], [-0.1, -0.9, -0.25], [-0.5, -0.1, -0.25],
               [3e38, 3e38, 0.0], [-3e38, -3e38, 0.0], [3e38, -3e38, 0.0]],
              [[0, 1, 2], [3, 5, 4], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 17, 16], [18, 19, 20]],
              [[[0.1, 0.1], [0.9, 0.15], [0.2, 0.9]]] * 7)


TILTED = [(-0.5, -0.5, -1), (2, -2, -4), (2, 2, -4), (-0.5, 0.5, -1)]
FLAT = [(-1, -1, -2), (1, -1, -2), (1, 1, -2), (-1, 1, -2)]


def quads(*corner_sets):
    v, f, uv = [], [], []
    for k, corners in enumerate(corner_sets):
        v += [list(c) for c in corners]
        f += [[4 * k, 4 * k + 1, 4 * k + 2], [4 * k, 4 * k + 2, 4 * k + 3]]
        uv += [[(0.1, 0.1), (0.9, 0.1), (0.9, 0.9)], [(0.1, 0.1), (0.9, 0.9), (0.1, 0.9)]]
    return _t(v, f, uv)


# eye, at, up, fov_y, near
ABOVE = ((0.1, -0.2, 2.2), (0.0, 0.0, 0.0), (0, 1, 0), 45.0, 0.05)
OBLIQUE = ((0.9, -1.7, 1.3), (0.05, 0.0, 0.0), (0, 0, 1), 50.0, 0.05)
HAND = ((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, 0.5)  # on a square frame: camera space is world space, fx = fy = 1


# ---------------------------------------------------------------- device frames against the restatement
_ref = {}


def reference(key, mesh, tex, pose, size, **opts):
    """Computed once per case and left unchanged."""
    if key not in _ref:
        eye, at, up, fov, near = pose
        cam = view_ref.camera(eye, at, up, fov, size, near)
        _ref[key] = view_ref.view(mesh[0].numpy(), mesh[1].numpy(), mesh[2].numpy(), tex.numpy(), cam, **opts)
    return _ref[key]


def small_ref(name, texture):
    """The 17 x 13 field from OBLIQUE at 200 x 136 under an option set: shared by the tests that need it, whichever runs first."""
    return reference("small_" + name, field(17, 13, 3), texture, OBLIQUE, (136, 200), **OPTIONS[name])


def assert_frame(got, want, what):
    image, face_idx, depth = got
    assert image.dtype == torch.uint8 and face_idx.dtype == torch.int32 and depth.dtype == torch.float32
    for name, g, w in (("face_idx", face_idx, want["face_idx"]), ("depth", depth, want["depth"]), ("image", image, want["image"])):
        g, w = g.cpu(), torch.from_numpy(w)
        if not torch.equal(g, w):
            bad = torch.nonzero((g != w).reshape(g.shape[0], g.shape[1], -1).any(dim=2))
            i, j = bad[0].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad.shape[0]} pixels, first (row {i}, column {j}): got {g[i, j].tolist()!r} "
                                 f"(face {int(face_idx[i, j])}), want {w[i, j].tolist()!r} (face {int(want['face_idx'][i, j])})")


def check(model, key, mesh, tex, pose, size, unbinned=True, **opts):
    """model.render_view (the view's stream) and ops.mesh_view with the binning bypassed both equal the restatement."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    want = reference(key, mesh, tex, pose, size, **opts)
    eye, at, up, fov, near = pose
    cam = view_camera(eye, at, up, fov, size, near)
    dm = model.load_mesh(*mesh)
    dev_tex = tex.to(DEV)
    got = model.render_view(dm, dev_tex, cam, want_face_idx=True, want_depth=True, **opts)
    assert got[0].device.type == "cuda" and tuple(got[0].shape) == (*size, 4)
    assert_frame(got, want, key)
    if unbinned:
        assert_frame(ops.mesh_view(dm, dev_tex, cam, binned=False, **opts), want, key + " (every tile streams every face)")
    dm.close()
    return want


def test_one_face(model, texture):
    want = check(model, "one_face", first_faces(field(17, 13, 3), 1), texture, ((-0.95, -0.7, 0.6), (-0.95, -0.7, 0.0), (0, 1, 0), 40.0, 0.05), (64, 64))
    n = int((want["face_idx"] == 0).sum())
    assert 100 < n < 64 * 64 and (want["face_idx"] <= 0).all() and (want["image"][want["face_idx"] < 0] == 0).all()


def test_cube_from_close_by_all_faces_large(model, texture):
    want = check(model, "cube", cube(), texture, ((0.9, -1.1, 0.8), (0, 0, 0), (0, 0, 1), 60.0, 0.05), (136, 200))
    seen = set(want["face_idx"][want["face_idx"] >= 0].tolist())
    assert len(seen) == 6 and (want["face_idx"] >= 0).sum() > 0.3 * 136 * 200  # three sides, every face across more than 2 x 2 bins
    want = check(model, "cube_culled", cube(), texture, ((0.9, -1.1, 0.8), (0, 0, 0), (0, 0, 1), 60.0, 0.05), (136, 200), cull=True)
    assert set(want["face_idx"][want["face_idx"] >= 0].tolist()) == seen  # a closed surface: culling the back changes nothing


OPTIONS = {
    "default": dict(),
    "no_shade": dict(shade=False),
    "cull": dict(cull=True),
    "cull_flip": dict(cull=True, flip_normals=True),
    "flip_colours": dict(flip_normals=True, ambient=0.6, unpainted=(200, 30, 90), background=(10, 20, 30, 255)),
    "ambient_0": dict(ambient=0.0),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_small_field_across_bin_borders(model, texture, name):
    """200 x 136: 13 x 9 tiles with partial ones on two sides, 4 x 3 bins with partial ones; faces of about 12 pixels straddle their borders."""
    want = check(model, "small_" + name, field(17, 13, 3), texture, OBLIQUE, (136, 200), **OPTIONS[name])
    covered = int((want["face_idx"] >= 0).sum())
    if name == "cull_flip":
        assert covered < 300  # the field faces the camera: flipped and culled, almost nothing is left
    else:
        assert covered > 7000 and len(set(want["face_idx"].ravel().tolist())) > 250


def test_small_field_option_sets_differ(model, texture):
    a, b, c = (small_ref(k, texture) for k in ("default", "no_shade", "flip_colours"))
    assert np.array_equal(a["face_idx"], b["face_idx"]) and not np.array_equal(a["image"], b["image"])
    assert np.array_equal(a["face_idx"], c["face_idx"]) and (c["image"][c["face_idx"] < 0] == np.array([10, 20, 30, 255], dtype=np.uint8)).all()
    assert (a["image"][a["face_idx"] >= 0][:, 3] == 255).all() and (a["image"][a["face_idx"] < 0] == 0).all()


def test_64_square_frame(model, texture):
    want = check(model, "small_64", field(17, 13, 3), texture, ABOVE, (64, 64))
    assert (want["face_idx"] >= 0).sum() > 2000


def test_faces_257(model, texture):
    want = check(model, "faces_257", first_faces(field(17, 13, 3), 257), texture, ABOVE, (64, 64))
    assert want["face_idx"].max() == 256 and len(set(want["face_idx"].ravel().tolist())) > 150


def test_dense_field_sub_pixel_faces_and_slivers(model, texture):
    want = check(model, "dense", field(65, 65), texture, ((1.4, -2.6, 1.9), (0.0, 0.0, 0.0), (0, 0, 1), 40.0, 0.05), (136, 200))
    shown = len(set(want["face_idx"][want["face_idx"] >= 0].tolist()))
    assert 2000 < shown < 8192 - 1000  # 8192 faces over fewer pixels than that: many own no pixel centre


def test_widest_frame(model, texture):
    """4096 x 24: 64 bins in a row, pixel columns up to 4095 in the packed ranges; every face is far wider than two bins."""
    want = check(model, "wide", field(17, 13, 3), texture, ((0.0, -0.05, 3.0), (0.0, -0.05, 0.0), (0, 1, 0), 0.25, 0.05), (24, 4096))
    cols = np.nonzero((want["face_idx"] >= 0).any(axis=0))[0]
    assert cols.min() < 700 and cols.max() > 3400 and (want["face_idx"] >= 0).sum() > 50000


def test_tallest_frame(model, texture):
    want = check(model, "tall", field(17, 13, 3), texture, ((0.05, 0.0, 3.0), (0.05, 0.0, 0.0), (1, 0, 0), 40.0, 0.05), (4096, 24))
    rows = np.nonzero((want["face_idx"] >= 0).any(axis=1))[0]
    assert rows.min() < 1200 and rows.max() > 2900


def test_both_windings_zero_area_and_overflowing_faces(model, texture):
    # seen from above face 0 is front, faces 1, 2 and 5 are back faces; face 5 lies under face 0 and shows beside it
    for name, opts, faces in (("windings", dict(), {0, 1, 2, 5}), ("windings_cull", dict(cull=True), {0}), ("windings_flip", dict(cull=True, flip_normals=True), {1, 2, 5})):
        want = check(model, name, both_windings(), texture, ((0.05, 0.02, 2.5), (0.0, 0.0, 0.0), (1, 1, 0), 50.0, 0.05), (64, 64), **opts)
        seen = set(want["face_idx"][want["face_idx"] >= 0].tolist())
        assert seen == faces
        assert not want["proj"]["drawn"][[3, 4, 6]].any()  # zero area, a sliver whose snapped area vanishes, overflow


def test_interpenetrating_and_coincident_quads(model, texture):
    want = check(model, "interpenetrating", quads(FLAT, TILTED), texture, HAND, (9, 9), shade=False)
    assert np.isin(want["face_idx"][2:7, 2:5], (2, 3)).all() and np.isin(want["face_idx"][2:7, 5:7], (0, 1)).all()
    want = check(model, "coincident", quads(FLAT, FLAT, FLAT), texture, HAND, (9, 9))
    assert set(want["face_idx"][2:7, 2:7].ravel().tolist()) == {0, 1}
    big = check(model, "interpenetrating_big", quads(FLAT, TILTED), texture, HAND, (200, 200))
    tilted = np.isin(big["face_idx"], (2, 3))
    assert tilted[60:140, 52:115].all() and not tilted[60:140, 118:148].any()  # the line at ndc_x = 1 / 6: column 116.7


def test_faces_behind_the_camera_and_across_the_near_plane(model, texture):
    """The eye hovers just above the field and looks along it: faces behind it, around it and through the near plane are dropped whole."""
    pose = ((-0.2, 0.0, 0.45), (0.9, 0.1, 0.2), (0, 0, 1), 70.0, 0.2)
    want = check(model, "inside", field(17, 13, 3), texture, pose, (136, 200))
    z = want["proj"]["z"]
    behind, across = (z > 0).all(axis=1), (z.max(axis=1) > -0.2) & (z.min(axis=1) <= -0.2)
    assert behind.sum() > 50 and across.sum() > 5 and not want["proj"]["drawn"][behind | across].any()
    assert 3000 < (want["face_idx"] >= 0).sum() < 136 * 200


def test_big_height_field_once(model, texture):
    mesh = field(225, 225)
    assert mesh[1].shape[0] == 100352
    want = check(model, "big", mesh, texture, ((1.5, -3.6, 2.6), (0.0, 0.0, 0.0), (0, 0, 1), 35.0, 0.05), (360, 640), unbinned=False)
    shown = len(set(want["face_idx"][want["face_idx"] >= 0].tolist()))
    assert shown > 20000 and want["face_idx"].max() > 90000


# ---------------------------------------------------------------- the optional outputs, repeats
def test_optional_outputs_absent_and_two_frames_equal(model, texture):
    from diffusiontexturepainting_amd.mesh import view_camera
    want = small_ref("default", texture)
    eye, at, up, fov, near = OBLIQUE
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    dm = model.load_mesh(*field(17, 13, 3))
    tex = texture.to(DEV)
    image = model.render_view(dm, tex, cam)
    assert isinstance(image, torch.Tensor) and torch.equal(image.cpu(), torch.from_numpy(want["image"]))
    image2, face_idx = model.render_view(dm, tex, cam, want_face_idx=True)
    image3, depth = model.render_view(dm, tex, cam, want_depth=True)
    assert torch.equal(image2, image) and torch.equal(image3, image)  # two frames of one pose: byte for byte
    assert torch.equal(face_idx.cpu(), torch.from_numpy(want["face_idx"])) and torch.equal(depth.cpu(), torch.from_numpy(want["depth"]))
    out = torch.full((136, 200, 4), 0x5a, dtype=torch.uint8, device=DEV)
    assert model.render_view(dm, tex, cam, out=out) is out and torch.equal(out, image)
    assert torch.equal(model.render_view(dm, tex, cam, size=(136, 200), live=True), image)
    dm.close()


# ---------------------------------------------------------------- frames and strokes
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
STROKE = dict(positions=[(0.1, -0.05, 0.1), (0.3, 0.05, 0.1), (0.2, 0.2, 0.1)],
              normals=[(0.35, -0.2, 0.9), (0.0, 0.0, 1.0), (-0.2, 0.1, 0.95)],
              prevs=[(0.0, 0.3, 0.15), (0.1, -0.05, 0.1), (0.3, 0.05, 0.1)],
              fov=[0.45, 0.4, 0.5])


def test_frame_after_a_stroke_shows_the_stroke(model, texture):
    from diffusiontexturepainting_amd.mesh import view_camera
    mesh = field(17, 13, 3)
    dm = model.load_mesh(*mesh)
    tex = texture.to(DEV)
    eye, at, up, fov, near = ABOVE
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    before = model.render_view(dm, tex, cam).cpu()
    model.paint_mesh_stroke(dm, tex, STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"], seeds=11, bleed=2, **ST)
    got = model.render_view(dm, tex, cam, want_face_idx=True, want_depth=True)  # (no synchronisation in between: live=False waits on the device)
    painted = tex.cpu()
    assert not torch.equal(painted, texture)
    want = view_ref.view(mesh[0].numpy(), mesh[1].numpy(), mesh[2].numpy(), painted.numpy(), view_ref.camera(eye, at, up, fov, (136, 200), near))
    assert_frame(got, want, "after the stroke")
    assert int((got[0].cpu() != before).any(dim=2).sum()) > 500
    dm.close()


def test_live_view_answers_while_a_stroke_is_queued(model, texture):
    """The criterion of test_pick_answers_while_a_stroke_is_queued, for the view's own stream: behind the 6-stamp stroke on the stroke's
    stream the frame would take the rest of the stroke's wall time, more than half of it.  A live frame's face indices and depth do not
    depend on the texture and are exact; the stroke's texture is what the same stroke leaves without any view."""
    from diffusiontexturepainting_amd.mesh import view_camera
    mesh = field(17, 13, 3)
    dm = model.load_mesh(*mesh)
    args = (STROKE["positions"] * 2, STROKE["normals"] * 2, STROKE["prevs"] * 2, STROKE["fov"] * 2)
    eye, at, up, fov, near = OBLIQUE
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    want = small_ref("default", texture)
    scratch = texture.to(DEV)
    for _ in range(2):  # programs, graphs, the masks and the view's buffers exist from here on
        model.paint_mesh_stroke(dm, scratch, *args, seeds=1, **ST)
        model.render_view(dm, scratch, cam, want_face_idx=True, want_depth=True, live=True)
    torch.cuda.synchronize()
    alone = texture.to(DEV)
    model.paint_mesh_stroke(dm, alone, *args, seeds=1, **ST)
    torch.cuda.synchronize()
    tex = texture.to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.paint_mesh_stroke(dm, tex, *args, seeds=1, **ST)
    t1 = time.perf_counter()
    frames = [model.render_view(dm, tex, cam, want_face_idx=True, want_depth=True, live=True) for _ in range(3)]
    model.view_stream.synchronize()
    t_view = time.perf_counter() - t1
    still_running = not model.stream.query()
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"6-stamp mesh stroke: enqueued in {(t1 - t0) * 1e3:.1f} ms, done after {t_all * 1e3:.1f} ms; three live 200 x 136 frames behind it "
          f"returned in {t_view * 1e3:.2f} ms (stroke still running: {still_running})")
    for image, face_idx, depth in frames:
        assert torch.equal(face_idx.cpu(), torch.from_numpy(want["face_idx"])) and torch.equal(depth.cpu(), torch.from_numpy(want["depth"]))
        assert (image.cpu()[..., 3] == torch.from_numpy(np.where(want["face_idx"] >= 0, 255, 0).astype(np.uint8))).all()
    assert t_view < 0.5 * t_all
    assert torch.equal(tex, alone) and not torch.equal(tex.cpu(), texture)
    dm.close()


def test_refusals_leave_the_outputs_alone(model, texture):
    from diffusiontexturepainting_amd import _lib, ops
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    lib = _lib.load()
    dm = model.load_mesh(*field(17, 13, 3))
    tex = texture.to(DEV)
    eye, at, up, fov, near = OBLIQUE
    camera = view_camera(eye, at, up, fov, (64, 64), near)
    image = torch.full((64, 64, 4), 0x5a, dtype=torch.uint8, device=DEV)
    face_idx = torch.full((64, 64), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    depth = torch.full((64, 64), 7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(model.view_stream.cuda_stream)
    p = (lambda t, off=0: C.c_void_p(t.data_ptr() + off))

    def refused(word, mesh=dm.handle, texture_=p(tex), th=TH, tw=TW, cam=None, H=64, W=64, opts=None, img=p(image), f=p(face_idx), d=p(depth)):
        cam = camera.struct() if cam is None else cam
        opts = view_opts() if opts is None else opts
        for fn, tail in ((lib.dtp_mesh_view, (s,)), (lib.dtp_op_mesh_view, (1, s))):
            rc = fn(mesh, texture_, th, tw, C.byref(cam), H, W, C.byref(opts), img, f, d, *tail)
            assert rc == 1 and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        torch.cuda.synchronize()
        assert (image == 0x5a).all() and (face_idx == 0x5a5a5a5a).all() and (depth == 7.0).all()

    refused("NULL", mesh=None)
    refused("NULL", texture_=None)
    refused("NULL", img=None)
    refused(r"1\.\.4096", H=0)
    refused(r"1\.\.4096", W=4097)
    refused(r"1\.\.32768", th=0)
    refused("aligned", texture_=p(tex, 2))
    refused("aligned", img=p(image, 1))
    broken = camera.struct()
    broken.near = 0.0
    refused("near", cam=broken)
    broken = camera.struct()
    broken.m[2] = float("nan")
    refused("matrix", cam=broken)
    bad = view_opts()
    bad.ambient = 2.0
    refused("ambient", opts=bad)
    bad = view_opts()
    bad.cull = 3
    refused("0 or 1", opts=bad)
    dead = model.load_mesh(*first_faces(field(17, 13, 3), 4))
    handle = dead.handle
    dead.close()
    refused("not a live mesh", mesh=handle)
    # the Python surface
    with pytest.raises(ValueError, match="load_mesh"):
        model.render_view(None, tex, camera)
    with pytest.raises(ValueError, match="view_camera"):
        model.render_view(dm, tex, torch.zeros(3, 4))
    with pytest.raises(ValueError, match="texture"):
        model.render_view(dm, tex.cpu(), camera)
    with pytest.raises(ValueError, match="size"):
        model.render_view(dm, tex, camera, size=(64, 5000))
    with pytest.raises(ValueError, match="out must be"):
        model.render_view(dm, tex, camera, out=image[:32])
    with pytest.raises(DtpError, match=r"\(code 1\).*ambient"):
        model.render_view(dm, tex, camera, ambient=-1.0, out=image)
    with pytest.raises(DtpError, match=r"\(code 1\).*ambient"):
        ops.mesh_view(dm, tex, camera, ambient=1.5)
    with pytest.raises(ValueError, match="0..255"):
        model.render_view(dm, tex, camera, unpainted=(1, 2, 300))
    torch.cuda.synchronize()
    assert (image == 0x5a).all()
    # and the view still works
    want = reference("after_refusals", field(17, 13, 3), texture, OBLIQUE, (64, 64))
    assert_frame(model.render_view(dm, tex, camera, want_face_idx=True, want_depth=True, out=image), want, "after the refusals")
    dm.close()
