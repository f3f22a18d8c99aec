"""The anisotropic view of a textured mesh on the device (dtp_mesh_view_aniso, dtp_op_mesh_view_aniso, `model.render_view(anisotropy=)`,
`ops.mesh_view(anisotropy=)`; include/dtp.h "an anisotropic view"): the device's frame, face indices, depth, lod, taps and coverage
against the numpy restatement (tests/view_aniso_ref.py) with torch.equal, at max_aniso 1, 2, 3, 4, 8 and 16, binned and with every face
on the list every tile streams, with and without the near-plane clip, at 1, 2 and 4 samples a side; max_aniso 1 through the new entry
against the trilinear frame of the old one, a magnified frame against the bilinear one; the optional outputs, out=, live=, the pyramid
the model builds itself, and the old filters after the new one.  One 64^2 context with synthetic weights.  Nothing is compared under a
tolerance."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mip_ref
import view_aniso_ref as an
import view_clip_ref as vc
import view_ref

pytestmark = pytest.mark.gpu

R = 64
DEV = "cuda:0"
NAMES = ("image", "face_idx", "depth", "lod", "taps", "coverage")
MS = (1, 2, 3, 4, 8, 16)
KW = dict(filter="trilinear", want_lod=True, want_taps=True, want_coverage=True)


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


def assert_frame(got, want, what, names=NAMES):
    assert len(got) == len(names), (what, len(got))
    for name, g in zip(names, got):
        g, w = g.cpu(), torch.from_numpy(np.ascontiguousarray(want[name]))
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, tuple(g.shape))
        if not torch.equal(g, w):
            bad = torch.nonzero((g != w).reshape(g.shape[0], g.shape[1], -1).any(dim=2))
            i, j = bad[0].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad.shape[0]} pixels, first (row {i}, column {j}): got {g[i, j].tolist()!r}, want "
                                 f"{w[i, j].tolist()!r} (face {int(want['face_idx'][i, j])}, taps {int(want['taps'][i, j])}, lod "
                                 f"{float(want['lod'][i, j])})")


class Scene:
    """The mesh, the texture and its pyramid of view_aniso_ref.scene(name) on the device."""

    def __init__(self, model, name):
        mesh, tex, _ = an.scene(name)
        self.name = name
        self.mesh = model.load_mesh(*(torch.from_numpy(np.ascontiguousarray(m)) for m in mesh))
        self.tex = torch.from_numpy(tex).to(DEV)
        self.mips = model.build_mips(self.tex)

    def camera(self, pose, size):
        from diffusiontexturepainting_amd.mesh import view_camera
        eye, at, up, fov, near = pose
        return view_camera(eye, at, up, fov, size, near)

    def close(self):
        self.mesh.close()


def check(model, name, pose, size, Ms=MS, clip_near=False, samples=1, **opts):
    """At every M: ops.mesh_view binned and not, and model.render_view where M > 1, equal the restatement in all six outputs.
    -> {M: the restatement's frame}."""
    from diffusiontexturepainting_amd import ops
    sc = Scene(model, name)
    cam = sc.camera(pose, size)
    wants = {}
    for M in Ms:
        want = wants[M] = an.reference(name, pose, size, M, clip_near=clip_near, samples=samples, **opts)
        kw = dict(clip_near=clip_near, samples=samples, anisotropy=M, **KW, **opts)
        what = f"{name}, max_aniso {M}, samples {samples}, clip {clip_near}"
        for binned in (True, False):
            got = ops.mesh_view(sc.mesh, sc.tex, cam, binned=binned, mips=sc.mips, **kw)
            assert_frame(got, want, what + (", binned" if binned else ", every tile streams every face"))
        if M > 1:
            got = model.render_view(sc.mesh, sc.tex, cam, mips=sc.mips, want_face_idx=True, want_depth=True, **kw)
            assert got[0].device.type == "cuda" and tuple(got[0].shape) == (*size, 4)
            assert_frame(got, want, what + ", render_view")
    sc.close()
    return wants


def field_pose(name):
    tex, eye, at, up, fov, near, _ = mip_ref.POSES[name]
    return "field:" + tex, (eye, at, up, fov, near)


# ---------------------------------------------------------------- against the restatement
def test_grazing_pose_of_the_field(model):
    wants = check(model, *field_pose("grazing"), mip_ref.FRAME)
    hit = wants[4]["face_idx"] >= 0
    assert np.bincount(wants[4]["N"][hit], minlength=5)[1:].tolist() == an.GRAZING_M4_TAPS
    assert not np.array_equal(wants[4]["image"], wants[1]["image"]) and not np.array_equal(wants[16]["image"], wants[4]["image"])


def test_the_floor_keeps_its_stripes_on_the_device(model):
    wants = check(model, "floor", an.FLOOR_POSE, an.FLOOR_SIZE, shade=False)
    hit = wants[1]["face_idx"] >= 0
    rows = [i for i in range(hit.shape[0]) if hit[i].sum() >= 32][:2]
    spread = lambda M, row: float(np.std(wants[M]["image"][row][hit[row]][:, 0].astype(np.float64)))  # noqa: E731
    for row in rows:
        assert spread(1, row) < 10 and spread(4, row) > 40 and spread(16, row) > 40


@pytest.mark.parametrize("name", list(an.POSES))
def test_poses_that_take_every_number_of_taps(model, name):
    scene, eye, at, up, fov, near, hist, clamped = an.POSES[name]
    wants = check(model, scene, (eye, at, up, fov, near), mip_ref.FRAME)
    want = wants[16]
    hit = want["face_idx"] >= 0
    assert np.bincount(want["N"][hit], minlength=17)[1:].tolist() == hist
    assert int((hit & (want["N"] == 16) & (want["pmax2"] > np.float32(256) * want["pmin2"])).sum()) == clamped


def test_horizon_triangle_takes_one_tap_of_the_last_level(model):
    eye, at, fov, size, near = mip_ref.TRIANGLE_POSE
    wants = check(model, "triangle", (eye, at, (0, -1, 0), fov, near), size, Ms=(1, 4, 16))
    want = wants[16]
    hit = want["face_idx"] >= 0
    assert hit.sum() > 0 and want["horizon"][hit].all() and (want["taps"][hit] == 1).all()
    assert (want["lod"][hit] == len(mip_ref.texture("atlas")[1]) - 1).all()
    check(model, "triangle", (eye, at, (0, 1, 0), fov, near), size, Ms=(16,))


@pytest.mark.parametrize("name,pose,size", [("cube", vc.CUBE_INSIDE, (36, 64)), ("clip_floor", vc.FLOOR_POSE, (36, 64))], ids=["cube", "floor"])
def test_eye_inside_with_crossing_winners(model, name, pose, size):
    wants = check(model, name, pose, size, Ms=(1, 4, 16), clip_near=True)
    want = wants[16]
    assert want["crossing"].sum() > 300 and (want["N"][want["crossing"]] >= 2).sum() > 100  # crossing winners that take several taps
    assert want["N"].max() >= 6


@pytest.mark.parametrize("samples,name,clip_near", [(2, "grazing", False), (2, "cube", True), (4, "floor_low", False), (4, "clip_floor", True)])
def test_samples_with_and_without_the_clip(model, samples, name, clip_near):
    if name == "grazing":
        scene, pose, size = *field_pose(name), mip_ref.FRAME
    elif name == "floor_low":
        scene, pose, size = an.POSES[name][0], an.POSES[name][1:6], mip_ref.FRAME
    else:
        scene, pose, size = name, vc.CUBE_INSIDE if name == "cube" else vc.FLOOR_POSE, (36, 64)
    wants = check(model, scene, pose, size, Ms=(1, 16), clip_near=clip_near, samples=samples)
    want = wants[16]
    assert want["fine"]["N"].max() >= 2 and tuple(want["fine"]["image"].shape) == (samples * size[0], samples * size[1], 4)
    assert not np.array_equal(want["image"], wants[1]["image"])
    if not clip_near:  # the field and the low floor have silhouettes inside the frame
        assert ((want["coverage"] > 0) & (want["coverage"] < samples * samples)).any()


def test_alpha_0_texels_enter_the_plain_average(model):
    """The atlas texture of mip_ref has unpainted (alpha 0) regions next to painted ones: taps on both sides of such a border are averaged
    plainly, all four channels, and the unpainted colour is mixed in afterwards."""
    scene, eye, at, up, fov, near, _, _ = an.POSES["floor_low"]
    wants = check(model, "floor:atlas", (eye, at, up, fov, near), mip_ref.FRAME, Ms=(4, 16))
    tex = an.scene("floor:atlas")[1]
    assert (tex[..., 3] == 0).any() and (tex[..., 3] == 255).any()
    assert (wants[16]["N"] >= 4).sum() > 50 and not np.array_equal(wants[16]["image"], wants[4]["image"])


# ---------------------------------------------------------------- the properties, on the device
def test_max_aniso_1_through_the_new_entry_is_the_trilinear_frame(model):
    """P1 on the device: ops.mesh_view(anisotropy=1) runs dtp_op_mesh_view_aniso, render_view(filter="trilinear") dtp_mesh_view_mips."""
    from diffusiontexturepainting_amd import ops
    for name, pose, size, clip_near in ((*field_pose("grazing"), mip_ref.FRAME, False), ("floor", an.FLOOR_POSE, an.FLOOR_SIZE, False),
                                        ("cube", vc.CUBE_INSIDE, (36, 64), True)):
        sc = Scene(model, name)
        cam = sc.camera(pose, size)
        old = model.render_view(sc.mesh, sc.tex, cam, filter="trilinear", mips=sc.mips, clip_near=clip_near, want_face_idx=True, want_depth=True,
                                want_lod=True)
        for samples, want_coverage in ((1, False), (1, True)):  # the plain raster kernel, and the anti-aliased one at one sample
            new = ops.mesh_view(sc.mesh, sc.tex, cam, filter="trilinear", mips=sc.mips, clip_near=clip_near, anisotropy=1, want_lod=True,
                                want_taps=True, samples=samples, want_coverage=want_coverage)
            for a, b in zip(old, new[:4]):
                assert torch.equal(a, b), (name, samples, want_coverage)
            assert torch.equal(new[4], (old[1] >= 0).to(torch.uint8)) and int((old[1] >= 0).sum()) > 500
        sc.close()


def test_a_magnified_frame_is_the_bilinear_frame(model):
    """P2."""
    tex, eye, at, up, fov, near = mip_ref.MAGNIFIED
    sc = Scene(model, "field:" + tex)
    cam = sc.camera((eye, at, up, fov, near), mip_ref.FRAME)
    plain = model.render_view(sc.mesh, sc.tex, cam, want_face_idx=True, want_depth=True)
    got = model.render_view(sc.mesh, sc.tex, cam, filter="trilinear", anisotropy=16, want_face_idx=True, want_depth=True, want_lod=True, want_taps=True)
    for a, b in zip(plain, got[:3]):
        assert torch.equal(a, b)
    assert int((got[1] >= 0).sum()) > 1000 and (got[3] == 0).all() and torch.equal(got[4], (got[1] >= 0).to(torch.uint8))
    want = an.reference("field:" + tex, (eye, at, up, fov, near), mip_ref.FRAME, 16)
    assert_frame(got, want, "magnified", names=("image", "face_idx", "depth", "lod", "taps"))
    sc.close()


# ---------------------------------------------------------------- the optional outputs, repeats, out=, live, the model's own pyramid
def test_optional_outputs_absent_two_frames_equal_out_and_live(model):
    from diffusiontexturepainting_amd import ops
    scene, pose = field_pose("grazing")
    H, W = mip_ref.FRAME
    sc = Scene(model, scene)
    cam = sc.camera(pose, mip_ref.FRAME)
    for samples in (1, 2):
        want = an.reference(scene, pose, mip_ref.FRAME, 8, samples=samples)
        kw = dict(filter="trilinear", anisotropy=8, samples=samples)
        image = model.render_view(sc.mesh, sc.tex, cam, **kw)  # mips=None: the model builds the pyramid on the view's stream
        assert isinstance(image, torch.Tensor) and torch.equal(image.cpu(), torch.from_numpy(want["image"]))
        for key, flag in (("face_idx", "want_face_idx"), ("depth", "want_depth"), ("lod", "want_lod"), ("taps", "want_taps"),
                          ("coverage", "want_coverage")):
            again, extra = model.render_view(sc.mesh, sc.tex, cam, **{flag: True}, **kw)
            assert torch.equal(again, image) and torch.equal(extra.cpu(), torch.from_numpy(want[key])), (samples, key)  # two frames: byte for byte
        out = torch.full((H, W, 4), 0x5a, dtype=torch.uint8, device=DEV)
        assert model.render_view(sc.mesh, sc.tex, cam, out=out, **kw) is out and torch.equal(out, image)
        assert torch.equal(model.render_view(sc.mesh, sc.tex, cam, live=True, mips=sc.mips, **kw), image)
        got = ops.mesh_view(sc.mesh, sc.tex, cam, want_face_idx=False, want_depth=False, mips=sc.mips, **kw)
        assert len(got) == 3 and got[1] is None and got[2] is None and torch.equal(got[0], image)
        got = ops.mesh_view(sc.mesh, sc.tex, cam, mips=sc.mips, want_taps=True, want_coverage=True, **kw)
        assert_frame(got, want, "taps before coverage", names=("image", "face_idx", "depth", "taps", "coverage"))
    sc.close()


def test_the_old_filters_after_an_anisotropic_frame(model):
    """No shared state: a trilinear and a bilinear frame rendered after an anisotropic one equal their own restatements."""
    scene, pose = field_pose("grazing")
    sc = Scene(model, scene)
    cam = sc.camera(pose, mip_ref.FRAME)
    mesh, t, lv = an.scene(scene)
    ref_cam = view_ref.camera(*pose[:4], mip_ref.FRAME, pose[4])
    want = an.reference(scene, pose, mip_ref.FRAME, 16)
    got = model.render_view(sc.mesh, sc.tex, cam, filter="trilinear", anisotropy=16)
    assert torch.equal(got.cpu(), torch.from_numpy(want["image"]))
    tri = mip_ref.pose_reference("grazing")
    got = model.render_view(sc.mesh, sc.tex, cam, filter="trilinear", want_face_idx=True, want_depth=True, want_lod=True)
    assert_frame(got, tri, "trilinear afterwards", names=("image", "face_idx", "depth", "lod"))
    got = model.render_view(sc.mesh, sc.tex, cam, want_face_idx=True, want_depth=True)
    assert_frame(got, view_ref.view(*mesh, t, ref_cam), "bilinear afterwards", names=("image", "face_idx", "depth"))
    got = model.render_view(sc.mesh, sc.tex, cam, filter="trilinear", anisotropy=16)
    assert torch.equal(got.cpu(), torch.from_numpy(want["image"]))
    sc.close()


# ---------------------------------------------------------------- the refusals
def test_refusals_leave_the_outputs_alone(model):
    from diffusiontexturepainting_amd import _lib, ops
    from diffusiontexturepainting_amd.mesh import view_opts
    lib = _lib.load()
    sc = Scene(model, "cube")
    camera = sc.camera(vc.CUBE_INSIDE, (36, 64))
    image = torch.full((36, 64, 4), 0x5a, dtype=torch.uint8, device=DEV)
    face_idx = torch.full((36, 64), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    depth = torch.full((36, 64), 7.0, dtype=torch.float32, device=DEV)
    lod = torch.full((36, 64), 7.0, dtype=torch.float32, device=DEV)
    taps = torch.full((36, 64), 0x5a, dtype=torch.uint8, device=DEV)
    coverage = torch.full((36, 64), 0x5a, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(model.view_stream.cuda_stream)
    p = (lambda t, off=0: C.c_void_p(t.data_ptr() + off))

    def refused(word, m=p(sc.mips), H=36, W=64, clip=1, samples=2, M=4):
        cam, opts = camera.struct(), view_opts()
        for fn, tail in ((lib.dtp_mesh_view_aniso, (s,)), (lib.dtp_op_mesh_view_aniso, (0, s))):
            rc = fn(sc.mesh.handle, p(sc.tex), 96, 160, m, C.byref(cam), H, W, C.byref(opts), clip, samples, M, p(image), p(face_idx), p(depth),
                    p(lod), p(taps), p(coverage), *tail)
            assert rc == 1 and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        torch.cuda.synchronize()
        assert (image == 0x5a).all() and (face_idx == 0x5a5a5a5a).all() and (depth == 7.0).all() and (lod == 7.0).all()
        assert (taps == 0x5a).all() and (coverage == 0x5a).all()

    for M in (0, 17, -1):
        refused(r"max_aniso must lie in 1\.\.16", M=M)
    refused("mips is required", m=None)
    refused("samples is 1, 2 or 4", samples=3)
    refused("must not exceed 4096", samples=2, H=2049)
    refused("clip is 0 or 1", clip=2)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="anisotropy"):
            model.render_view(sc.mesh, sc.tex, camera, filter="trilinear", anisotropy=bad, out=image)
        with pytest.raises(ValueError, match="anisotropy"):
            ops.mesh_view(sc.mesh, sc.tex, camera, filter="trilinear", mips=sc.mips, anisotropy=bad)
    with pytest.raises(ValueError, match="trilinear"):
        model.render_view(sc.mesh, sc.tex, camera, anisotropy=4, out=image)
    with pytest.raises(ValueError, match="want_taps"):
        model.render_view(sc.mesh, sc.tex, camera, filter="trilinear", want_taps=True, out=image)
    with pytest.raises(ValueError, match="bilinear.*trilinear"):
        model.render_view(sc.mesh, sc.tex, camera, filter="anisotropic", out=image)
    torch.cuda.synchronize()
    assert (image == 0x5a).all()
    # and the view still works
    want = an.reference("cube", vc.CUBE_INSIDE, (36, 64), 4, clip_near=True, samples=2)
    got = model.render_view(sc.mesh, sc.tex, camera, samples=2, clip_near=True, filter="trilinear", anisotropy=4, mips=sc.mips, want_face_idx=True,
                            want_depth=True, want_lod=True, want_taps=True, want_coverage=True, out=image)
    assert got[0] is image
    assert_frame(got, want, "after the refusals")
    sc.close()
