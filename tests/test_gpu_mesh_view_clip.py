"""The view of a textured mesh clipped at the near plane on the device (dtp_mesh_view_clip, dtp_op_mesh_view_clip,
`model.render_view(clip_near=True)`, `ops.mesh_view(clip_near=True)`; include/dtp.h "a view clipped at the near plane"): the device's
frame, face indices, depth and lod against the numpy restatement (tests/view_clip_ref.py) with torch.equal, with both filters, binned and
with every crossing face given the whole frame as its range; every scene of test_gpu_mesh_view.py seen from outside against the frame
without the keyword; a frame after a stroke; the refusals.  One 64^2 context with synthetic weights.  Nothing is compared under a
tolerance."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mip_ref
import test_gpu_mesh_view as base
import view_clip_ref as vc
import view_ref

pytestmark = pytest.mark.gpu

R = 64
DEV = "cuda:0"
FILTERS = ("bilinear", "trilinear")


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


def tensors(mesh):
    return tuple(torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m for m in mesh)


def arrays(mesh):
    return tuple(m if isinstance(m, np.ndarray) else m.numpy() for m in mesh)


def field():
    return arrays(mip_ref.field())


_ref = {}


def reference(key, filt, mesh, pose, size, **opts):
    """The restatement's frame on the 96 x 160 texture with alpha-0 regions: computed once per case and left unchanged."""
    if (key, filt) not in _ref:
        eye, at, up, fov, near = pose
        tex, lv = mip_ref.texture("atlas")
        _ref[key, filt] = vc.view(*arrays(mesh), tex, view_ref.camera(eye, at, up, fov, size, near), filter=filt, levels=lv, **opts)
    return _ref[key, filt]


def assert_frame(got, want, what):
    names = ("image", "face_idx", "depth", "lod")[:len(got)]
    for name, g in zip(names, got):
        g, w = g.cpu(), torch.from_numpy(want[name])
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name)
        if not torch.equal(g, w):
            bad = torch.nonzero((g != w).reshape(g.shape[0], g.shape[1], -1).any(dim=2))
            i, j = bad[0].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad.shape[0]} pixels, first (row {i}, column {j}): got {g[i, j].tolist()!r}, want "
                                 f"{w[i, j].tolist()!r} (face {int(want['face_idx'][i, j])}, crossing {bool(want['crossing'][i, j])})")


def check(model, key, mesh, pose, size, **opts):
    """model.render_view(clip_near=True) (binned, on the view's stream) and ops.mesh_view(clip_near=True, binned=False) (every crossing
    face with the whole frame as its range) both equal the restatement, with both filters -> the bilinear reference."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    eye, at, up, fov, near = pose
    cam = view_camera(eye, at, up, fov, size, near)
    dm = model.load_mesh(*tensors(mesh))
    dev_tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    mips = model.build_mips(dev_tex)
    for filt in FILTERS:
        tri = filt == "trilinear"
        want = reference(key, filt, mesh, pose, size, **opts)
        got = model.render_view(dm, dev_tex, cam, clip_near=True, filter=filt, want_face_idx=True, want_depth=True, want_lod=tri, **opts)
        assert got[0].device.type == "cuda" and tuple(got[0].shape) == (*size, 4)
        assert_frame(got, want, f"{key}, {filt}")
        got = ops.mesh_view(dm, dev_tex, cam, binned=False, clip_near=True, filter=filt, mips=mips if tri else None, want_lod=tri, **opts)
        assert_frame(got, want, f"{key}, {filt}, every crossing face over the whole frame")
    dm.close()
    return reference(key, "bilinear", mesh, pose, size, **opts)


# ---------------------------------------------------------------- the scenes with crossing faces
@pytest.mark.parametrize("size", [(36, 64), (136, 200), (9, 9), (24, 4096)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_floor_under_the_eye(model, size):
    want = check(model, f"floor_{size}", vc.floor_mesh(), vc.FLOOR_POSE, size)
    covered = want["face_idx"] >= 0
    assert want["cr"]["drawn"].all() and covered.sum() == want["crossing"].sum() and (want["depth"][covered] >= np.float32(0.01)).all()
    assert not covered[0].any() and covered[-1, size[1] // 2]
    if size == (24, 4096):  # 70 times as wide as the floor is at the bottom row's depth: a band in the middle
        assert covered.sum() > 2500 and not covered[:, :1500].any() and not covered[:, -1500:].any()
    else:
        assert covered.sum() > 0.5 * size[0] * size[1] and covered[-1].all()
    if size == (36, 64):
        assert covered.sum() == 1344


def test_cube_from_inside_uses_the_large_list_alone(model):
    want = check(model, "cube_inside", vc.cube_mesh(), vc.CUBE_INSIDE, (136, 200))
    # a closed room covers every pixel -- but for the one at (116, 137), whose centre lies on the edge between face 7, in front, and face
    # 10, crossing: there the integer rule and the fp32 edge function meet, and neither claims it (the mixed-edge property of the contract)
    holes = np.argwhere(want["face_idx"] < 0).tolist()
    assert holes == [[116, 137]] and not want["crossing"][116, 136] and want["crossing"][116, 138]
    assert want["crossing"].sum() > 5000 and want["cr"]["drawn"].sum() == 8
    want = check(model, "cube_inside_culled_flipped", vc.cube_mesh(), vc.CUBE_INSIDE, (36, 64), cull=True, flip_normals=True)
    assert (want["face_idx"] >= 0).all()
    want = check(model, "cube_inside_culled", vc.cube_mesh(), vc.CUBE_INSIDE, (36, 64), cull=True, background=(10, 20, 30, 255))
    assert (want["face_idx"] == -1).all()


def test_height_field_from_inside_its_hull(model):
    """The pose of test_faces_behind_the_camera_and_across_the_near_plane, 26 faces across the plane, and the same a quarter of a unit
    lower.  In the first the crossing faces lie under the frame (ndc_y about -2.2): 12929 pixels covered with the clip and without.  In
    the second the clip covers 13027 against 9549.  Both poses equal their restatements, with the clip here and without it there."""
    from diffusiontexturepainting_amd.mesh import view_camera
    dm = model.load_mesh(*mip_ref.field())
    dev_tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    for name, pose in (("inside", vc.FIELD_INSIDE), ("low", vc.FIELD_LOW)):
        want = check(model, "field_" + name, field(), pose, (136, 200))
        assert want["cr"]["drawn"].sum() == 26
        eye, at, up, fov, near = pose
        off = model.render_view(dm, dev_tex, view_camera(eye, at, up, fov, (136, 200), near), want_face_idx=True, want_depth=True)
        plain = view_ref.view(*field(), mip_ref.texture("atlas")[0], view_ref.camera(eye, at, up, fov, (136, 200), near))
        assert_frame(off, plain | dict(crossing=np.zeros((136, 200), bool)), "without the clip, " + name)
        n_on, n_off = int((want["face_idx"] >= 0).sum()), int((plain["face_idx"] >= 0).sum())
        print(f"{name}: {n_on} pixels covered with the clip, {n_off} without")
        assert n_on >= n_off and (name == "inside" or n_on > n_off)
    dm.close()


def test_faces_257_of_every_class_in_both_windings(model):
    want = check(model, "mixed", vc.mixed_mesh(), vc.MIXED_POSE, (64, 64))
    assert want["crossing"].sum() > 300 and (~want["crossing"] & (want["face_idx"] >= 0)).sum() > 1000
    want = check(model, "mixed_cull", vc.mixed_mesh(), vc.MIXED_POSE, (64, 64), cull=True, shade=False)
    assert 0 < want["crossing"].sum() and len(set(want["face_idx"][want["crossing"]].tolist())) >= 3
    want = check(model, "mixed_flip", vc.mixed_mesh(), vc.MIXED_POSE, (136, 200), cull=True, flip_normals=True, ambient=0.6, unpainted=(200, 30, 90),
                 background=(10, 20, 30, 255))
    assert 0 < want["crossing"].sum()


def test_runway_takes_the_last_level_at_its_horizon(model):
    want = reference("runway", "trilinear", vc.RUNWAY, vc.RUNWAY_POSE, (32, 32))
    check(model, "runway", vc.RUNWAY, vc.RUNWAY_POSE, (32, 32))
    L = len(mip_ref.texture("atlas")[1])
    assert (want["lod"][15] == L - 1).all() and (want["face_idx"][15] >= 0).all() and (want["face_idx"][16:] == -1).all()


# ---------------------------------------------------------------- the optional outputs, repeats
def test_optional_outputs_absent_and_two_frames_equal(model):
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    eye, at, up, fov, near = vc.CUBE_INSIDE
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    dm = model.load_mesh(*tensors(vc.cube_mesh()))
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    for filt in FILTERS:
        want = reference("cube_inside", filt, vc.cube_mesh(), vc.CUBE_INSIDE, (136, 200))
        kw = dict(clip_near=True, filter=filt)
        image = model.render_view(dm, tex, cam, **kw)
        assert isinstance(image, torch.Tensor) and torch.equal(image.cpu(), torch.from_numpy(want["image"]))
        image2, face_idx = model.render_view(dm, tex, cam, want_face_idx=True, **kw)
        image3, depth = model.render_view(dm, tex, cam, want_depth=True, **kw)
        assert torch.equal(image2, image) and torch.equal(image3, image)  # two frames of one pose: byte for byte
        assert torch.equal(face_idx.cpu(), torch.from_numpy(want["face_idx"])) and torch.equal(depth.cpu(), torch.from_numpy(want["depth"]))
        out = torch.full((136, 200, 4), 0x5a, dtype=torch.uint8, device=DEV)
        assert model.render_view(dm, tex, cam, out=out, **kw) is out and torch.equal(out, image)
        assert torch.equal(model.render_view(dm, tex, cam, live=True, **kw), image)
        if filt == "trilinear":
            image4, lod = model.render_view(dm, tex, cam, want_lod=True, **kw)
            assert torch.equal(image4, image) and torch.equal(lod.cpu(), torch.from_numpy(want["lod"]))
            mips = model.build_mips(tex)
            assert torch.equal(model.render_view(dm, tex, cam, mips=mips, **kw), image)
            got = ops.mesh_view(dm, tex, cam, want_face_idx=False, want_depth=False, mips=mips, **kw)
        else:
            got = ops.mesh_view(dm, tex, cam, want_face_idx=False, want_depth=False, **kw)
        assert len(got) == 3 and got[1] is None and got[2] is None and torch.equal(got[0], image)
    dm.close()


# ---------------------------------------------------------------- scenes without a crossing face: the frame without the keyword
OUTSIDE = {
    "one_face": (lambda: base.first_faces(base.field(17, 13, 3), 1), ((-0.95, -0.7, 0.6), (-0.95, -0.7, 0.0), (0, 1, 0), 40.0, 0.05), (64, 64), {}),
    "cube": (base.cube, ((0.9, -1.1, 0.8), (0, 0, 0), (0, 0, 1), 60.0, 0.05), (136, 200), {}),
    "cube_culled": (base.cube, ((0.9, -1.1, 0.8), (0, 0, 0), (0, 0, 1), 60.0, 0.05), (136, 200), dict(cull=True)),
    "small_64": (lambda: base.field(17, 13, 3), base.ABOVE, (64, 64), {}),
    "faces_257": (lambda: base.first_faces(base.field(17, 13, 3), 257), base.ABOVE, (64, 64), {}),
    "dense": (lambda: base.field(65, 65), ((1.4, -2.6, 1.9), (0.0, 0.0, 0.0), (0, 0, 1), 40.0, 0.05), (136, 200), {}),
    "wide": (lambda: base.field(17, 13, 3), ((0.0, -0.05, 3.0), (0.0, -0.05, 0.0), (0, 1, 0), 0.25, 0.05), (24, 4096), {}),
    "tall": (lambda: base.field(17, 13, 3), ((0.05, 0.0, 3.0), (0.05, 0.0, 0.0), (1, 0, 0), 40.0, 0.05), (4096, 24), {}),
    "windings": (base.both_windings, ((0.05, 0.02, 2.5), (0.0, 0.0, 0.0), (1, 1, 0), 50.0, 0.05), (64, 64), {}),
    "windings_cull": (base.both_windings, ((0.05, 0.02, 2.5), (0.0, 0.0, 0.0), (1, 1, 0), 50.0, 0.05), (64, 64), dict(cull=True)),
    "windings_flip": (base.both_windings, ((0.05, 0.02, 2.5), (0.0, 0.0, 0.0), (1, 1, 0), 50.0, 0.05), (64, 64), dict(cull=True, flip_normals=True)),
    "interpenetrating": (lambda: base.quads(base.FLAT, base.TILTED), base.HAND, (9, 9), dict(shade=False)),
    "coincident": (lambda: base.quads(base.FLAT, base.FLAT, base.FLAT), base.HAND, (9, 9), {}),
    "interpenetrating_big": (lambda: base.quads(base.FLAT, base.TILTED), base.HAND, (200, 200), {}),
    "big": (lambda: base.field(225, 225), ((1.5, -3.6, 2.6), (0.0, 0.0, 0.0), (0, 0, 1), 35.0, 0.05), (360, 640), {}),
}
OUTSIDE.update({"small_" + k: (lambda: base.field(17, 13, 3), base.OBLIQUE, (136, 200), o) for k, o in base.OPTIONS.items()})


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_scene_seen_from_outside_equals_the_frame_without_the_keyword(model, name):
    from diffusiontexturepainting_amd.mesh import view_camera
    make, pose, size, opts = OUTSIDE[name]
    mesh = make()
    eye, at, up, fov, near = pose
    cam = view_camera(eye, at, up, fov, size, near)
    c = vc.camera_space(mesh[0].numpy(), mesh[1].numpy(), view_ref.camera(eye, at, up, fov, size, near))
    assert not vc.classify(c, np.float32(near))[2].any()  # no face crosses the plane
    dm = model.load_mesh(*mesh)
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    for filt in FILTERS:
        kw = dict(filter=filt, want_face_idx=True, want_depth=True, want_lod=filt == "trilinear", **opts)
        plain = model.render_view(dm, tex, cam, **kw)
        clipped = model.render_view(dm, tex, cam, clip_near=True, **kw)
        assert int((plain[1] >= 0).sum()) > 0
        for a, b in zip(plain, clipped):
            assert torch.equal(a, b), (name, filt)
    dm.close()


# ---------------------------------------------------------------- a frame after a stroke
def test_clipped_frame_after_a_stroke_shows_the_stroke(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    mesh = mip_ref.field()
    dm = model.load_mesh(*mesh)
    start = mip_ref.texture("atlas")[0]
    tex = torch.from_numpy(start).to(DEV)
    eye, at, up, fov, near = vc.FIELD_LOW
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    before = model.render_view(dm, tex, cam, clip_near=True).cpu()
    model.paint_mesh_stroke(dm, tex, base.STROKE["positions"], base.STROKE["normals"], base.STROKE["prevs"], base.STROKE["fov"], seeds=11, bleed=2,
                            **base.ST)
    got = model.render_view(dm, tex, cam, clip_near=True, want_face_idx=True, want_depth=True)  # (live=False waits on the device)
    painted = tex.cpu().numpy()
    assert not np.array_equal(painted, start)
    want = vc.view(*field(), painted, view_ref.camera(eye, at, up, fov, (136, 200), near))
    assert_frame(got, want, "after the stroke")
    assert int((got[0].cpu() != before).any(dim=2).sum()) > 100 and want["crossing"].sum() > 1000
    dm.close()


# ---------------------------------------------------------------- the refusals
def test_refusals_leave_the_outputs_alone(model):
    from diffusiontexturepainting_amd import _lib, ops
    from diffusiontexturepainting_amd.mesh import view_camera, view_opts
    lib = _lib.load()
    dm = model.load_mesh(*tensors(vc.cube_mesh()))
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    mips = model.build_mips(tex)
    eye, at, up, fov, near = vc.CUBE_INSIDE
    camera = view_camera(eye, at, up, fov, (36, 64), near)
    image = torch.full((36, 64, 4), 0x5a, dtype=torch.uint8, device=DEV)
    face_idx = torch.full((36, 64), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    depth = torch.full((36, 64), 7.0, dtype=torch.float32, device=DEV)
    lod = torch.full((36, 64), 7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(model.view_stream.cuda_stream)
    p = (lambda t, off=0: C.c_void_p(t.data_ptr() + off))

    def refused(word, mesh=dm.handle, texture_=p(tex), th=96, tw=160, m=p(mips), cam=None, H=36, W=64, opts=None, filt=1, img=p(image), f=p(face_idx),
                d=p(depth), lo=p(lod)):
        cam = camera.struct() if cam is None else cam
        opts = view_opts() if opts is None else opts
        for fn, tail in ((lib.dtp_mesh_view_clip, (s,)), (lib.dtp_op_mesh_view_clip, (0, s))):
            rc = fn(mesh, texture_, th, tw, m, C.byref(cam), H, W, C.byref(opts), filt, img, f, d, lo, *tail)
            assert rc == 1 and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        torch.cuda.synchronize()
        assert (image == 0x5a).all() and (face_idx == 0x5a5a5a5a).all() and (depth == 7.0).all() and (lod == 7.0).all()

    refused("NULL", mesh=None)
    refused("NULL", texture_=None)
    refused("NULL", img=None)
    refused("filter is 0", filt=3)
    refused("need filter 1", filt=0)
    refused("mips is required", m=None)
    refused("aligned", m=p(mips, 2))
    refused("aligned", lo=p(lod, 2))
    refused(r"1\.\.4096", H=0)
    refused(r"1\.\.32768", tw=0)
    broken = camera.struct()
    broken.near = 0.0
    refused("near", cam=broken)
    bad = view_opts()
    bad.shade = 3
    refused("0 or 1", opts=bad)
    dead = model.load_mesh(*tensors(vc.floor_mesh()))
    handle = dead.handle
    dead.close()
    refused("not a live mesh", mesh=handle)
    # the Python surface
    with pytest.raises(ValueError, match="trilinear"):
        model.render_view(dm, tex, camera, clip_near=True, mips=mips)
    with pytest.raises(ValueError, match="trilinear"):
        model.render_view(dm, tex, camera, clip_near=True, want_lod=True)
    with pytest.raises(ValueError, match="clip_near"):
        ops.mesh_view(dm, tex, camera, filter="trilinear", mips=mips)
    with pytest.raises(ValueError, match="filter"):
        ops.mesh_view(dm, tex, camera, clip_near=True, filter="anisotropic")
    torch.cuda.synchronize()
    assert (image == 0x5a).all()
    # and the view still works
    want = reference("cube_inside_36", "trilinear", vc.cube_mesh(), vc.CUBE_INSIDE, (36, 64))
    got = model.render_view(dm, tex, camera, clip_near=True, filter="trilinear", mips=mips, want_face_idx=True, want_depth=True, want_lod=True, out=image)
    assert_frame(got, want, "after the refusals")
    dm.close()
