"""The mip pyramid of a texture and the trilinear-filtered view on the device (dtp_texture_mips, dtp_mesh_view_mips, `model.build_mips`,
`model.render_view(filter="trilinear")`; include/dtp.h "the mip pyramid of a texture and a trilinear-filtered view"): the pyramid's
bytes, and the frame, its map of lod, face indices and depth, against the numpy restatement (tests/mip_ref.py) with torch.equal; the
filtered frame's visibility against the unfiltered call's; the refusals.  One 64^2 context with synthetic weights, DDIM.  Nothing is
compared under a tolerance."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mip_ref
import view_ref

pytestmark = pytest.mark.gpu

R = 64
DEV = "cuda:0"


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


# ---------------------------------------------------------------- the pyramid
def assert_pyramid(got, tex, what):
    """got: the device's bytes; tex: numpy uint8 [h, w, 4].  Level by level, so that a failure names the level and the texel."""
    lay = mip_ref.layout(*tex.shape[:2])
    levels = mip_ref.pyramid(tex)
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (lay["bytes"],) and len(levels) == lay["levels"]
    for k in range(1, lay["levels"]):
        h, w = lay["h"][k], lay["w"][k]
        g = got[lay["offset"][k]: lay["offset"][k] + 4 * h * w].reshape(h, w, 4)
        if not np.array_equal(g, levels[k]):
            bad = np.argwhere((g != levels[k]).any(axis=2))
            i, j = bad[0]
            raise AssertionError(f"{what}: level {k} ({h} x {w}) differs at {len(bad)} texels, first ({i}, {j}): got {g[i, j].tolist()}, want {levels[k][i, j].tolist()}")
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(mip_ref.pack(levels)))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (5, 3), (63, 65), (64, 64), (96, 160), (200, 136), (4100, 70), (2048, 2048)])
def test_pyramid_equals_the_restatement(model, h, w):
    """63 x 65 and 200 x 136: partial tiles, rows that are no multiple of four texels (no 16-byte loads); 4100 x 70: 14 levels, three
    passes, the second and third reading what the first wrote; 2048 x 2048: 1024 tiles, two passes."""
    from diffusiontexturepainting_amd import ops
    tex = mip_ref.make_texture(h, w, 100 + h)
    if h >= 8 and w >= 8:
        assert (tex[..., 3] == 0).any() and (tex[..., 3] == 255).any()
    lay = ops.mip_layout(h, w)
    assert lay == mip_ref.layout(h, w)
    got = model.build_mips(torch.from_numpy(tex).to(DEV))
    assert got.device.type == "cuda" and got.dtype == torch.uint8 and tuple(got.shape) == (lay["bytes"],)
    assert_pyramid(got, tex, f"{h} x {w}")


def test_pyramid_into_a_buffer_one_byte_short_and_other_refusals(model):
    from diffusiontexturepainting_amd import _lib
    lib = _lib.load()
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    need = mip_ref.layout(96, 160)["bytes"]
    buf = torch.full((need + 64,), 0x5a, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = (lambda t, off=0: C.c_void_p(t.data_ptr() + off))

    def refused(word, texture=p(tex), th=96, tw=160, m=p(buf), n=need):
        rc = lib.dtp_texture_mips(texture, th, tw, m, n, s)
        assert rc == 1 and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        torch.cuda.synchronize()
        assert (buf == 0x5a).all()

    refused("mips_bytes", n=need - 1)
    refused("NULL", texture=None)
    refused("NULL", m=None)
    refused(r"1\.\.32768", th=0)
    refused("aligned", texture=p(tex, 2))
    refused("aligned", m=p(buf, 1))
    with pytest.raises(ValueError, match="texture"):
        model.build_mips(tex.cpu())
    with pytest.raises(ValueError, match="out must be"):
        model.build_mips(tex, out=buf[: need - 1])
    # an exact fit writes the pyramid and nothing behind it
    assert model.build_mips(tex, out=buf) is buf
    assert_pyramid(buf[:need], mip_ref.texture("atlas")[0], "into a canary-filled buffer")
    assert (buf[need:] == 0x5a).all()


ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
STROKE = dict(positions=[(0.1, -0.05, 0.1), (0.3, 0.05, 0.1), (0.2, 0.2, 0.1)],
              normals=[(0.35, -0.2, 0.9), (0.0, 0.0, 1.0), (-0.2, 0.1, 0.95)],
              prevs=[(0.0, 0.3, 0.15), (0.1, -0.05, 0.1), (0.3, 0.05, 0.1)],
              fov=[0.45, 0.4, 0.5])


def test_pyramid_and_frame_after_a_stroke(model):
    """No synchronisation between the stroke and what follows: the pyramid is built on the stroke's stream order (the current stream waits
    for the stroke on the device), the filtered frame after the waits a frame makes."""
    from diffusiontexturepainting_amd.mesh import view_camera
    mesh = mip_ref.field()
    dm = model.load_mesh(*mesh)
    start = mip_ref.texture("atlas")[0]
    tex = torch.from_numpy(start).to(DEV)
    model.paint_mesh_stroke(dm, tex, STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"], seeds=11, bleed=2, **ST)
    torch.cuda.current_stream().wait_stream(model.stream)
    mips = model.build_mips(tex)
    eye, at, up, fov, near = (0.1, -0.2, 4.0), (0.0, 0.0, 0.0), (0, 1, 0), 45.0, 0.05
    got = model.render_view(dm, tex, view_camera(eye, at, up, fov, mip_ref.FRAME, near), filter="trilinear", want_face_idx=True, want_depth=True, want_lod=True)
    painted = tex.cpu().numpy()
    assert not np.array_equal(painted, start)
    assert_pyramid(mips, painted, "after the stroke")
    want = mip_ref.view(*[m.numpy() for m in mesh], painted, view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near))
    assert_frame(got, want, "after the stroke")
    assert (want["level"] >= 1).sum() > 200
    dm.close()


# ---------------------------------------------------------------- frames against the restatement
def assert_frame(got, want, what):
    image, face_idx, depth, lod = got
    assert image.dtype == torch.uint8 and face_idx.dtype == torch.int32 and depth.dtype == torch.float32 and lod.dtype == torch.float32
    for name, g, w in (("face_idx", face_idx, want["face_idx"]), ("depth", depth, want["depth"]), ("lod", lod, want["lod"]), ("image", image, want["image"])):
        g, w = g.cpu(), torch.from_numpy(w)
        if not torch.equal(g, w):
            bad = torch.nonzero((g != w).reshape(g.shape[0], g.shape[1], -1).any(dim=2))
            i, j = bad[0].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad.shape[0]} pixels, first (row {i}, column {j}): got {g[i, j].tolist()!r}, want "
                                 f"{w[i, j].tolist()!r} (face {int(want['face_idx'][i, j])}, lod {float(want['lod'][i, j])!r})")


def check(model, mesh, tex, want, cam, what, **opts):
    """The filtered frame equals the restatement; its face indices and depth equal the unfiltered call's."""
    dm = model.load_mesh(*mesh)
    dev_tex = torch.from_numpy(tex).to(DEV)
    got = model.render_view(dm, dev_tex, cam, filter="trilinear", want_face_idx=True, want_depth=True, want_lod=True, **opts)
    assert got[0].device.type == "cuda" and tuple(got[0].shape) == (*cam.size, 4) and tuple(got[3].shape) == tuple(cam.size)
    assert_frame(got, want, what)
    plain = model.render_view(dm, dev_tex, cam, want_face_idx=True, want_depth=True, **opts)
    assert torch.equal(plain[1], got[1]) and torch.equal(plain[2], got[2])
    dm.close()
    return got, plain


@pytest.mark.parametrize("name", sorted(mip_ref.POSES))
def test_pose_equals_the_restatement(model, name):
    from diffusiontexturepainting_amd.mesh import view_camera
    tex, eye, at, up, fov, near, counts = mip_ref.POSES[name]
    want = mip_ref.pose_reference(name)
    got, plain = check(model, mip_ref.field(), mip_ref.texture(tex)[0], want, view_camera(eye, at, up, fov, mip_ref.FRAME, near), name)
    lod = got[3].cpu().numpy()
    covered = want["face_idx"] >= 0
    assert [int(((np.floor(lod) == k) & covered).sum()) for k in range(len(counts))] == counts
    if name == "grazing":
        assert int((got[0] != plain[0]).any(dim=2).sum()) > 200      # the filter shows


OBLIQUE = ((0.9, -1.7, 1.3), (0.05, 0.0, 0.0), (0, 0, 1), 50.0, 0.05)
_ref = {}


def reference(key, mesh, tex, pose, size, **opts):
    """Computed once per case and left unchanged."""
    if key not in _ref:
        eye, at, up, fov, near = pose
        _ref[key] = mip_ref.view(*[m.numpy() for m in mesh], tex, view_ref.camera(eye, at, up, fov, size, near), **opts)
    return _ref[key]


@pytest.mark.parametrize("name,opts", [("default", dict()), ("colours", dict(flip_normals=True, ambient=0.6, unpainted=(200, 30, 90), background=(10, 20, 30, 255), shade=True)),
                                       ("no_shade_cull", dict(shade=False, cull=True))])
def test_small_field_across_tile_and_bin_borders(model, name, opts):
    """200 x 136: 13 x 9 tiles with partial ones on two sides, 4 x 3 bins with partial ones."""
    from diffusiontexturepainting_amd.mesh import view_camera
    tex = mip_ref.texture("atlas")[0]
    want = reference("oblique_" + name, mip_ref.field(), tex, OBLIQUE, (136, 200), **opts)
    eye, at, up, fov, near = OBLIQUE
    check(model, mip_ref.field(), tex, want, view_camera(eye, at, up, fov, (136, 200), near), "oblique " + name, **opts)
    assert (want["face_idx"] >= 0).sum() > 7000 and (want["level"] >= 1).sum() > 500 and (want["f"] > 0).sum() > 3000


def test_dense_field_sub_pixel_faces(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    pose = ((1.4, -2.6, 1.9), (0.0, 0.0, 0.0), (0, 0, 1), 40.0, 0.05)
    tex = mip_ref.texture("atlas")[0]
    mesh = mip_ref.field(65, 65, 0)
    want = reference("dense", mesh, tex, pose, (136, 200))
    eye, at, up, fov, near = pose
    check(model, mesh, tex, want, view_camera(eye, at, up, fov, (136, 200), near), "dense")
    assert len(set(want["face_idx"][want["face_idx"] >= 0].tolist())) > 2000 and (want["level"] >= 1).sum() > 500


@pytest.mark.parametrize("up,branch", [((0, -1, 0), True), ((0, 1, 0), False)])
def test_triangle_beyond_the_horizon(model, up, branch):
    from diffusiontexturepainting_amd.mesh import view_camera
    v, f, uv = (torch.from_numpy(a) for a in mip_ref.TRIANGLE)
    eye, at, fov, size, near = mip_ref.TRIANGLE_POSE
    tex, lv = mip_ref.texture("atlas")
    want = mip_ref.view(*mip_ref.TRIANGLE, tex, view_ref.camera(eye, at, up, fov, size, near), levels=lv)
    covered = want["face_idx"] >= 0
    assert covered.sum() == 32 and want["horizon"][covered].all() == branch and want["horizon"].any() == branch
    got, _ = check(model, (v, f, uv), tex, want, view_camera(eye, at, up, fov, size, near), f"triangle, up {up}")
    if branch:
        assert (got[3].cpu().numpy()[covered] == len(lv) - 1).all()


def test_magnified_pose_is_the_bilinear_frame(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    tex, eye, at, up, fov, near = mip_ref.MAGNIFIED
    t = mip_ref.texture(tex)[0]
    cam = view_camera(eye, at, up, fov, mip_ref.FRAME, near)
    dm = model.load_mesh(*mip_ref.field())
    dev_tex = torch.from_numpy(t).to(DEV)
    image, lod = model.render_view(dm, dev_tex, cam, filter="trilinear", want_lod=True)
    assert (lod == 0).all() and torch.equal(image, model.render_view(dm, dev_tex, cam, filter="bilinear"))
    assert torch.equal(image, model.render_view(dm, dev_tex, cam)) and int((image[..., 3] == 255).sum()) > 1000
    dm.close()


def test_one_level_needs_no_pyramid(model):
    """A 1 x 1 texture is its own pyramid: mips=None builds nothing, an empty `mips=` is taken, and every pixel is that texel."""
    from diffusiontexturepainting_amd.mesh import view_camera
    _, eye, at, up, fov, near, _ = mip_ref.POSES["head_on_3"]
    one = np.array([[[200, 100, 50, 128]]], dtype=np.uint8)
    cam = view_camera(eye, at, up, fov, mip_ref.FRAME, near)
    want = mip_ref.view(*[m.numpy() for m in mip_ref.field()], one, view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near))
    assert (want["lod"] == 0).all()
    got, plain = check(model, mip_ref.field(), one, want, cam, "1 x 1 texture")
    assert torch.equal(got[0], plain[0])
    dm = model.load_mesh(*mip_ref.field())
    dev = torch.from_numpy(one).to(DEV)
    empty = model.build_mips(dev)
    assert empty.numel() == 0 and torch.equal(model.render_view(dm, dev, cam, filter="trilinear", mips=empty), got[0])
    dm.close()


def test_optional_outputs_prebuilt_pyramid_and_repeats(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    tex, eye, at, up, fov, near, _ = mip_ref.POSES["grazing"]
    want = mip_ref.pose_reference("grazing")
    cam = view_camera(eye, at, up, fov, mip_ref.FRAME, near)
    dm = model.load_mesh(*mip_ref.field())
    dev_tex = torch.from_numpy(mip_ref.texture(tex)[0]).to(DEV)
    kw = dict(filter="trilinear")
    image = model.render_view(dm, dev_tex, cam, **kw)
    assert isinstance(image, torch.Tensor) and torch.equal(image.cpu(), torch.from_numpy(want["image"]))
    image2, lod = model.render_view(dm, dev_tex, cam, want_lod=True, **kw)
    image3, face_idx = model.render_view(dm, dev_tex, cam, want_face_idx=True, **kw)
    image4, depth = model.render_view(dm, dev_tex, cam, want_depth=True, **kw)
    image5, depth2, lod2 = model.render_view(dm, dev_tex, cam, want_depth=True, want_lod=True, **kw)
    for other in (image2, image3, image4, image5):
        assert torch.equal(other, image)                           # two frames of one pose: byte for byte
    assert torch.equal(lod.cpu(), torch.from_numpy(want["lod"])) and torch.equal(lod2, lod) and torch.equal(depth2, depth)
    assert torch.equal(face_idx.cpu(), torch.from_numpy(want["face_idx"])) and torch.equal(depth.cpu(), torch.from_numpy(want["depth"]))
    # a pyramid built beforehand against the one built inside; a live frame of a texture at rest
    mips = model.build_mips(dev_tex)
    assert torch.equal(model.render_view(dm, dev_tex, cam, mips=mips, **kw), image)
    assert torch.equal(mips, model._view_mips[96, 160])
    assert torch.equal(model.render_view(dm, dev_tex, cam, live=True, **kw), image)
    out = torch.full((*mip_ref.FRAME, 4), 0x5a, dtype=torch.uint8, device=DEV)
    assert model.render_view(dm, dev_tex, cam, out=out, mips=mips, **kw) is out and torch.equal(out, image)
    dm.close()


def test_refusals_leave_the_outputs_alone(model):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    lib = _lib.load()
    dm = model.load_mesh(*mip_ref.field())
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    mips = model.build_mips(tex)
    eye, at, up, fov, near = OBLIQUE
    camera = view_camera(eye, at, up, fov, (64, 64), near)
    image = torch.full((64, 64, 4), 0x5a, dtype=torch.uint8, device=DEV)
    face_idx = torch.full((64, 64), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    depth = torch.full((64, 64), 7.0, dtype=torch.float32, device=DEV)
    lod = torch.full((64, 64), 7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(model.view_stream.cuda_stream)
    p = (lambda t, off=0: C.c_void_p(t.data_ptr() + off))

    def refused(word, mesh=dm.handle, texture_=p(tex), th=96, tw=160, m=p(mips), cam=None, H=64, W=64, opts=None, img=p(image), f=p(face_idx), d=p(depth),
                lo=p(lod)):
        cam = camera.struct() if cam is None else cam
        opts = view_opts() if opts is None else opts
        rc = lib.dtp_mesh_view_mips(mesh, texture_, th, tw, m, C.byref(cam), H, W, C.byref(opts), img, f, d, lo, s)
        assert rc == 1 and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        torch.cuda.synchronize()
        assert (image == 0x5a).all() and (face_idx == 0x5a5a5a5a).all() and (depth == 7.0).all() and (lod == 7.0).all()

    refused("NULL", mesh=None)
    refused("NULL", texture_=None)
    refused("NULL", img=None)
    refused("NULL.*mips", m=None)
    refused(r"1\.\.4096", H=0)
    refused(r"1\.\.32768", tw=32769)
    refused("aligned", texture_=p(tex, 2))
    refused("aligned", m=p(mips, 1))
    refused("aligned", lo=p(lod, 2))
    broken = camera.struct()
    broken.near = 0.0
    refused("near", cam=broken)
    bad = view_opts()
    bad.ambient = 2.0
    refused("ambient", opts=bad)
    dead = model.load_mesh(*mip_ref.field())
    handle = dead.handle
    dead.close()
    refused("not a live mesh", mesh=handle)
    # the Python surface
    with pytest.raises(ValueError, match="bilinear.*trilinear"):
        model.render_view(dm, tex, camera, filter="anisotropic")
    with pytest.raises(ValueError, match="need filter"):
        model.render_view(dm, tex, camera, want_lod=True)
    with pytest.raises(ValueError, match="need filter"):
        model.render_view(dm, tex, camera, mips=mips)
    with pytest.raises(ValueError, match="mips must be"):
        model.render_view(dm, tex, camera, filter="trilinear", mips=mips[:-4], out=image)
    with pytest.raises(ValueError, match="mips must be"):
        model.render_view(dm, tex, camera, filter="trilinear", mips=mips.cpu(), out=image)
    torch.cuda.synchronize()
    assert (image == 0x5a).all()
    # and the filtered view still works
    want = reference("after_refusals", mip_ref.field(), mip_ref.texture("atlas")[0], OBLIQUE, (64, 64))
    got = model.render_view(dm, tex, camera, filter="trilinear", mips=mips, want_face_idx=True, want_depth=True, want_lod=True, out=image)
    assert_frame(got, want, "after the refusals")
    dm.close()
