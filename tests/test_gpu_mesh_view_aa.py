"""The anti-aliased view of a textured mesh on the device (dtp_mesh_view_aa, dtp_op_mesh_view_aa, `model.render_view(samples=)`,
`ops.mesh_view(samples=)`; include/dtp.h "an anti-aliased view"): the device's frame, face indices, depth, lod and coverage against the
numpy restatement (tests/view_aa_ref.py: the existing restatements at samples x the size, resolved in integers) with torch.equal, with
both filters, with and without the near-plane clip, binned and with every face on the list every tile streams; against the device's own
frame at samples x the size resolved with torch; samples=1 against the call without the keyword; the optional outputs, a frame after a
stroke, out=, the delta tracker, the refusals.  One 64^2 context with synthetic weights.  Nothing is compared under a tolerance."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mip_ref
import test_gpu_mesh_view as base
import view_aa_ref as va
import view_clip_ref as vc
import view_ref

pytestmark = pytest.mark.gpu

R = 64
DEV = "cuda:0"
FILTERS = ("bilinear", "trilinear")
NAMES = ("image", "face_idx", "depth", "lod", "coverage")


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


def assert_frame(got, want, what):
    """got: (image, face_idx, depth[, lod], coverage) of the device; want: view_aa_ref.view's dict."""
    names = [n for n in NAMES if n != "lod" or len(got) == 5]
    assert len(got) == len(names)
    for name, g in zip(names, got):
        g, w = g.cpu(), torch.from_numpy(want[name])
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, tuple(g.shape))
        if not torch.equal(g, w):
            bad = torch.nonzero((g != w).reshape(g.shape[0], g.shape[1], -1).any(dim=2))
            i, j = bad[0].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad.shape[0]} pixels, first (row {i}, column {j}): got {g[i, j].tolist()!r}, want "
                                 f"{w[i, j].tolist()!r} (face {int(want['face_idx'][i, j])}, coverage {int(want['coverage'][i, j])})")


def check(model, what, mesh, pose, size, samples=(2, 4), filters=FILTERS, clip_near=False, texture="atlas", **opts):
    """For every filter and samples: model.render_view (binned, on the view's stream) and ops.mesh_view(binned=False) both equal the
    restatement in image, face_idx, depth, lod and coverage.  -> {(filter, samples): the restatement's frame}."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    eye, at, up, fov, near = pose
    cam, ref_cam = view_camera(eye, at, up, fov, size, near), view_ref.camera(eye, at, up, fov, size, near)
    tex, lv = mip_ref.texture(texture)
    dm = model.load_mesh(*tensors(mesh))
    dev_tex = torch.from_numpy(tex).to(DEV)
    mips = model.build_mips(dev_tex)
    wants = {}
    for filt in filters:
        tri = filt == "trilinear"
        for s in samples:
            want = va.view(*arrays(mesh), tex, ref_cam, samples=s, filter=filt, clip_near=clip_near, levels=lv if tri else None, **opts)
            kw = dict(samples=s, filter=filt, clip_near=clip_near, want_lod=tri, want_coverage=True, **opts)
            got = model.render_view(dm, dev_tex, cam, want_face_idx=True, want_depth=True, **kw)
            assert got[0].device.type == "cuda" and tuple(got[0].shape) == (*size, 4)
            assert_frame(got, want, f"{what}, {filt}, samples {s}")
            got = ops.mesh_view(dm, dev_tex, cam, binned=False, mips=mips if tri else None, **kw)
            assert_frame(got, want, f"{what}, {filt}, samples {s}, every tile streams every face")
            wants[filt, s] = want
    dm.close()
    return wants


def partly(want, s):
    return int(((want["coverage"] > 0) & (want["coverage"] < s * s)).sum())


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", ["head_on_3", "grazing", "head_on_7.8"])
def test_poses_of_the_field(model, name):
    tex, eye, at, up, fov, near, _ = mip_ref.POSES[name]
    wants = check(model, name, mip_ref.field(), (eye, at, up, fov, near), mip_ref.FRAME, texture=tex)
    want = wants["trilinear", 4]
    assert partly(want, 4) >= 10 and (name == "head_on_7.8" or (partly(want, 4) >= 20 and (want["faces_seen"] > 1).sum() >= 400))
    assert not np.array_equal(wants["bilinear", 4]["image"], wants["bilinear", 2]["image"])


@pytest.mark.parametrize("name", ["cull", "cull_flip", "no_shade", "flip_colours"])
def test_field_under_option_sets(model, name):
    wants = check(model, "options " + name, base.field(17, 13, 3), base.OBLIQUE, (34, 50), filters=("bilinear",), **base.OPTIONS[name])
    want = wants["bilinear", 4]
    covered = int((want["coverage"] > 0).sum())
    assert covered < 100 if name == "cull_flip" else covered > 500  # the field faces the camera: flipped and culled, almost nothing is left
    if name == "flip_colours":  # the background's bytes enter the average
        edge = (want["coverage"] > 0) & (want["coverage"] < 16)
        assert edge.sum() > 20 and (want["image"][want["coverage"] == 0] == np.array([10, 20, 30, 255], dtype=np.uint8)).all()
        assert (want["image"][edge][:, 3] == 255).all()


def test_one_face_and_the_cube_on_the_large_list(model):
    one = base.first_faces(base.field(17, 13, 3), 1)
    wants = check(model, "one face", one, ((-0.95, -0.7, 0.6), (-0.95, -0.7, 0.0), (0, 1, 0), 40.0, 0.05), (32, 32))
    assert partly(wants["bilinear", 4], 4) > 20 and (wants["bilinear", 4]["face_idx"] <= 0).all()
    # every face of the cube spans more than 2 x 2 bins of the fine frame (136 x 200 and 272 x 400): the large list alone
    wants = check(model, "cube", base.cube(), ((0.9, -1.1, 0.8), (0, 0, 0), (0, 0, 1), 60.0, 0.05), (68, 100))
    want = wants["trilinear", 2]
    assert len(set(want["fine"]["face_idx"][want["fine"]["face_idx"] >= 0].tolist())) == 6 and partly(want, 2) > 100


def test_interpenetrating_and_coincident_quads(model):
    wants = check(model, "interpenetrating", base.quads(base.FLAT, base.TILTED), base.HAND, (9, 9), shade=False)
    assert (wants["bilinear", 4]["faces_seen"] > 1).sum() > 5  # the line where the two quads cut each other crosses pixels
    wants = check(model, "coincident", base.quads(base.FLAT, base.FLAT, base.FLAT), base.HAND, (9, 9))
    assert set(wants["bilinear", 4]["fine"]["face_idx"].reshape(-1).tolist()) <= {-1, 0, 1}  # the lowest index wins every tie


@pytest.mark.parametrize("scene", ["floor", "cube", "mixed"])
def test_scenes_across_the_near_plane(model, scene):
    mesh, pose, size = dict(floor=(vc.floor_mesh(), vc.FLOOR_POSE, (36, 64)), cube=(vc.cube_mesh(), vc.CUBE_INSIDE, (36, 64)),
                            mixed=(vc.mixed_mesh(), vc.MIXED_POSE, (32, 32)))[scene]
    wants = check(model, scene, mesh, pose, size, clip_near=True)
    for key, want in wants.items():
        assert want["fine"]["crossing"].sum() > 300, key
    if scene == "floor":  # the horizon is a silhouette: the row it crosses is partly covered
        assert partly(wants["bilinear", 4], 4) >= 32


def test_horizon_triangle_trilinear(model):
    eye, at, fov, size, near = mip_ref.TRIANGLE_POSE
    wants = check(model, "horizon", mip_ref.TRIANGLE, (eye, at, (0, -1, 0), fov, near), size, samples=(2,), filters=("trilinear",))
    want = wants["trilinear", 2]
    assert want["fine"]["horizon"].sum() > 0 and (want["fine"]["lod"][want["fine"]["horizon"]] == len(mip_ref.texture("atlas")[1]) - 1).all()


@pytest.mark.parametrize("size,samples", [((9, 9), (2, 4)), ((6, 1024), (4,)), ((1024, 6), (4,)), ((2048, 6), (2,))],
                         ids=["9x9", "1024x6", "6x1024", "6x2048"])
def test_frames_at_the_extremes(model, size, samples):
    """The fine frames of the last three are 4096 on one side: the limit of the packed ranges and of the bin counters."""
    H, W = size
    if H == W:
        pose = base.ABOVE
    elif W > H:
        pose = ((0.0, -0.05, 3.0), (0.0, -0.05, 0.0), (0, 1, 0), 0.25, 0.05)
    else:
        pose = ((0.05, 0.0, 3.0), (0.05, 0.0, 0.0), (1, 0, 0), 40.0, 0.05)
    wants = check(model, f"{W}x{H}", base.field(17, 13, 3), pose, size, samples=samples, filters=("bilinear",) if H != W else FILTERS)
    for (filt, s), want in wants.items():
        assert max(s * H, s * W) == 4096 or size == (9, 9)
        assert (want["coverage"] > 0).sum() > 20 and len(set(want["fine"]["face_idx"].reshape(-1).tolist())) > 10, (filt, s)


# ---------------------------------------------------------------- against the device itself
def torch_resolve(fine, s):
    H, W = fine.shape[0] // s, fine.shape[1] // s
    total = fine.reshape(H, s, W, s, 4).to(torch.int32).sum(dim=(1, 3))
    return ((total + (s * s) // 2) >> {2: 2, 4: 4}[s]).to(torch.uint8)


def test_dense_field_equals_the_frame_of_twice_the_size_resolved(model):
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    mesh = base.field(65, 65)
    pose = ((1.4, -2.6, 1.9), (0.0, 0.0, 0.0), (0, 0, 1), 40.0, 0.05)
    wants = check(model, "dense", mesh, pose, (136, 200), samples=(2,), filters=("bilinear",))
    want = wants["bilinear", 2]
    assert (want["faces_seen"] > 1).sum() > 4000  # sub-pixel faces: most covered pixels see several
    eye, at, up, fov, near = pose
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    dm = model.load_mesh(*mesh)
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    fine, fine_idx, fine_depth = ops.mesh_view(dm, tex, cam, size=(272, 400))  # today's entry point, today's kernel
    got, face_idx, depth, coverage = ops.mesh_view(dm, tex, cam, samples=2, want_coverage=True)
    assert torch.equal(got, torch_resolve(fine, 2)) and torch.equal(got.cpu(), torch.from_numpy(want["image"]))
    assert torch.equal(face_idx, fine_idx[1::2, 1::2]) and torch.equal(depth, fine_depth[1::2, 1::2])
    assert torch.equal(coverage.to(torch.int64), (fine_idx >= 0).reshape(136, 2, 200, 2).sum(dim=(1, 3)))
    dm.close()


@pytest.mark.parametrize("clip_near", [False, True])
@pytest.mark.parametrize("filter", FILTERS)
def test_samples_1_is_the_call_without_the_keyword(model, filter, clip_near):
    from diffusiontexturepainting_amd.mesh import view_camera
    eye, at, up, fov, near = vc.FIELD_LOW
    cam = view_camera(eye, at, up, fov, (136, 200), near)
    dm = model.load_mesh(*mip_ref.field())
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    kw = dict(filter=filter, clip_near=clip_near, want_face_idx=True, want_depth=True, want_lod=filter == "trilinear")
    plain = model.render_view(dm, tex, cam, **kw)
    same = model.render_view(dm, tex, cam, samples=1, **kw)
    counted = model.render_view(dm, tex, cam, samples=1, want_coverage=True, **kw)  # samples 1 of the new entry point
    assert int((plain[1] >= 0).sum()) > 5000 and len(same) == len(plain) and len(counted) == len(plain) + 1
    for a, b, c in zip(plain, same, counted):
        assert torch.equal(a, b) and torch.equal(a, c), (filter, clip_near)
    assert counted[-1].dtype == torch.uint8 and torch.equal(counted[-1].bool(), plain[1] >= 0) and int(counted[-1].max()) == 1
    dm.close()


# ---------------------------------------------------------------- the optional outputs, repeats, out=, live
def test_optional_outputs_absent_and_two_frames_equal(model):
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import view_camera
    tex_name, eye, at, up, fov, near, _ = mip_ref.POSES["grazing"]
    cam, ref_cam = view_camera(eye, at, up, fov, mip_ref.FRAME, near), view_ref.camera(eye, at, up, fov, mip_ref.FRAME, near)
    H, W = mip_ref.FRAME
    t, lv = mip_ref.texture(tex_name)
    dm = model.load_mesh(*mip_ref.field())
    tex = torch.from_numpy(t).to(DEV)
    for s in (2, 4):
        want = va.view(*arrays(mip_ref.field()), t, ref_cam, samples=s, filter="trilinear", levels=lv)
        kw = dict(samples=s, filter="trilinear")
        image = model.render_view(dm, tex, cam, **kw)
        assert isinstance(image, torch.Tensor) and torch.equal(image.cpu(), torch.from_numpy(want["image"]))
        for key, flag in (("face_idx", "want_face_idx"), ("depth", "want_depth"), ("lod", "want_lod"), ("coverage", "want_coverage")):
            again, extra = model.render_view(dm, tex, cam, **{flag: True}, **kw)
            assert torch.equal(again, image) and torch.equal(extra.cpu(), torch.from_numpy(want[key])), (s, key)  # two frames: byte for byte
        out = torch.full((H, W, 4), 0x5a, dtype=torch.uint8, device=DEV)
        assert model.render_view(dm, tex, cam, out=out, **kw) is out and torch.equal(out, image)
        assert torch.equal(model.render_view(dm, tex, cam, live=True, **kw), image)
        mips = model.build_mips(tex)
        assert torch.equal(model.render_view(dm, tex, cam, mips=mips, **kw), image)
        got = ops.mesh_view(dm, tex, cam, want_face_idx=False, want_depth=False, mips=mips, **kw)
        assert len(got) == 3 and got[1] is None and got[2] is None and torch.equal(got[0], image)
    dm.close()


def test_frame_after_a_stroke_shows_the_stroke(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    dm = model.load_mesh(*mip_ref.field())
    start = mip_ref.texture("atlas")[0]
    tex = torch.from_numpy(start).to(DEV)
    eye, at, up, fov, near = base.OBLIQUE
    size = (68, 100)
    cam = view_camera(eye, at, up, fov, size, near)
    before = model.render_view(dm, tex, cam, samples=2).cpu()
    model.paint_mesh_stroke(dm, tex, base.STROKE["positions"], base.STROKE["normals"], base.STROKE["prevs"], base.STROKE["fov"], seeds=11, bleed=2,
                            **base.ST)
    got = model.render_view(dm, tex, cam, samples=2, want_face_idx=True, want_depth=True, want_coverage=True)  # (live=False waits on the device)
    painted = tex.cpu().numpy()
    assert not np.array_equal(painted, start)
    want = va.view(*arrays(mip_ref.field()), painted, view_ref.camera(eye, at, up, fov, size, near), samples=2)
    assert_frame(got, want, "after the stroke")
    assert int((got[0].cpu() != before).any(dim=2).sum()) > 50
    dm.close()


def test_delta_tracker_pulls_an_anti_aliased_frame(model):
    from diffusiontexturepainting_amd import delta
    from diffusiontexturepainting_amd.mesh import view_camera
    H, W = 68, 100
    dm = model.load_mesh(*mip_ref.field())
    tex = torch.from_numpy(mip_ref.texture("atlas")[0]).to(DEV)
    frame = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
    t = model.delta_tracker(frame)
    mirror = np.zeros((H, W, 4), np.uint8)
    counts = []
    for eye in ((0.0, 0.0, 4.0), (0.03, 0.0, 4.0)):
        assert model.render_view(dm, tex, view_camera(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, (H, W), 0.05), out=frame, samples=4) is frame
        b = t.frame(frame, on="view")
        delta.apply_frame(mirror, b)
        torch.cuda.synchronize()
        counts.append(len(delta.decode_frame(b)["ids"]))
        assert np.array_equal(mirror, frame.cpu().numpy())
    assert counts[0] == 5 * 7 and 0 < counts[1] < counts[0]  # the first frame whole, the second the tiles the mesh moved in
    t.close()
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
    coverage = torch.full((36, 64), 0x5a, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(model.view_stream.cuda_stream)
    p = (lambda t, off=0: C.c_void_p(t.data_ptr() + off))

    def refused(word, mesh=dm.handle, m=p(mips), H=36, W=64, filt=1, clip=1, samples=2, img=p(image), lo=p(lod)):
        cam, opts = camera.struct(), view_opts()
        for fn, tail in ((lib.dtp_mesh_view_aa, (s,)), (lib.dtp_op_mesh_view_aa, (0, s))):
            rc = fn(mesh, p(tex), 96, 160, m, C.byref(cam), H, W, C.byref(opts), filt, clip, samples, img, p(face_idx), p(depth), lo, p(coverage), *tail)
            assert rc == 1 and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        torch.cuda.synchronize()
        assert (image == 0x5a).all() and (face_idx == 0x5a5a5a5a).all() and (depth == 7.0).all() and (lod == 7.0).all() and (coverage == 0x5a).all()

    for samples in (0, 3, 8):
        refused("samples is 1, 2 or 4", samples=samples)
    refused("must not exceed 4096", samples=2, H=2049)
    refused("must not exceed 4096", samples=4, W=1025)
    refused(r"1\.\.4096", samples=1, H=4097)
    refused("clip is 0 or 1", clip=2)
    refused("filter is 0", filt=3)
    refused("need filter 1", filt=0)
    refused("mips is required", m=None)
    refused("aligned", lo=p(lod, 2))
    refused("NULL", mesh=None)
    refused("NULL", img=None)
    dead = model.load_mesh(*tensors(vc.floor_mesh()))
    handle = dead.handle
    dead.close()
    refused("not a live mesh", mesh=handle)
    # the Python surface
    for bad in (0, 3, 8):
        with pytest.raises(ValueError, match="samples"):
            model.render_view(dm, tex, camera, samples=bad, out=image)
        with pytest.raises(ValueError, match="samples"):
            ops.mesh_view(dm, tex, camera, samples=bad)
    with pytest.raises(ValueError, match="4096"):
        model.render_view(dm, tex, camera, size=(1025, 8), samples=4)
    with pytest.raises(ValueError, match="trilinear"):
        model.render_view(dm, tex, camera, samples=2, want_lod=True)
    torch.cuda.synchronize()
    assert (image == 0x5a).all()
    # and the view still works
    t, lv = mip_ref.texture("atlas")
    want = va.view(*vc.cube_mesh(), t, view_ref.camera(eye, at, up, fov, (36, 64), near), samples=2, filter="trilinear", clip_near=True, levels=lv)
    got = model.render_view(dm, tex, camera, samples=2, clip_near=True, filter="trilinear", mips=mips, want_face_idx=True, want_depth=True, want_lod=True,
                            want_coverage=True, out=image)
    assert got[0] is image
    assert_frame(got, want, "after the refusals")
    dm.close()
