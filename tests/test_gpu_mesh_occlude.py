"""The occlusion test of the backprojection on the device (dtp_mesh_stroke_occluded, dtp_op_mesh_backproject_occluded;
`paint_mesh_stroke(occlude=)`, `ops.mesh_backproject(fov=, occlude=)`; include/dtp.h "occlusion in the backprojection") against the numpy
restatement of the contract (tests/mesh_occlude_ref.py).  Every comparison is torch.equal: the rule fixes every operation.  One 64^2
context, DDIM, 4 steps, as tests/test_gpu_mesh.py."""
import ctypes as C
import re
import time

import numpy as np
import pytest
import torch

import mesh_occlude_ref as occ
import mesh_ref
import select_ref
import stroke_ref
from mesh_ref import ERASE, INPAINT

pytestmark = pytest.mark.gpu

R = 64
H, W = 96, 160
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
DEV = "cuda:0"

# pos, normal, prev, fov
POSES = {
    "table_straight": ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0),           # the window is the floor
    "table_tilted": ((0, 0, 0), (0.3, -0.2, 0.9), (0, 1, 0.1), 1.0),
    "table_close": ((0.2, 0.1, 0), (0.25, -0.2, 0.9), (0.2, 1, 0.1), 0.55),  # the floor runs out of the window: its taps clamp at the border
    "field_straight": ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.1),
    "field_tilted": ((0, 0, 0), (0.35, -0.2, 0.9), (0.0, 1.0, 0.15), 1.1),
}


_pads = []  # (see the model fixture)


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
    # A good neighbour in the suite's process: a process has four hardware queues, the runtime hands streams to them in turn (DESIGN.md
    # 3.24, "Streams"), and test_gpu_mesh_pick.py::test_pick_answers_while_a_stroke_is_queued, which runs after this module, passes or
    # not with the queue its pick stream lands in.  This model takes two streams (the stroke's, and the pick's through paint_mesh_path);
    # two more, used once, make it four, so that every later module finds its streams in the queues they had before this file existed.
    for _ in range(2):
        pad = torch.cuda.Stream(device=0)
        with torch.cuda.stream(pad):
            torch.zeros(1, device=DEV)
        _pads.append(pad)
    return m


def scene(name):
    from diffusiontexturepainting_amd import synthetic
    if name == "table":            # F = 4
        return synthetic.make_table_on_floor()
    if name == "field":            # F = 384: a chunk of 256 and a part of one
        return synthetic.make_height_field()
    return synthetic.make_height_field(bump=0.1)  # "smooth"


TEXTURE = random_texture(H, W, 77)
DEC = torch.randn(R, R, 4, generator=torch.Generator().manual_seed(5)) * 0.9
_meshes, _renders = {}, {}


def device_mesh(model, name):
    if name not in _meshes:
        _meshes[name] = model.load_mesh(*scene(name))
    return _meshes[name]


def reference_render(name, pose):
    """mesh_ref's render of a scene from a pose, computed once and left unchanged."""
    key = (name, pose)
    if key not in _renders:
        v, f, uv = scene(name)
        p = POSES[pose]
        _, face_idx, proj = mesh_ref.render(v, f, uv, mesh_ref.camera(*p), p[3], TEXTURE, R)
        _renders[key] = (uv, face_idx, proj)
    return _renders[key]


def device_backproject(model, name, pose, dec, mask, painted=None, face_mask=None, occlude=None, texture=TEXTURE):
    """ops.mesh_render -> ops.mesh_backproject on the device -> (the texture on the host, face_idx on the host)."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    p = POSES[pose]
    dm = device_mesh(model, name)
    dtex = texture.to(DEV)
    _, face_idx = ops.mesh_render(dm, mesh_camera(*p), p[3], dtex, R)
    out = ops.mesh_backproject(dm, None if dec is None else dec.to(DEV), mask.to(DEV), face_idx, dtex,
                               painted=None if painted is None else painted.to(DEV), face_mask=face_mask,
                               fov=None if occlude is None else p[3], occlude=occlude)
    assert out is dtex
    return out.cpu(), face_idx.cpu()


# ---------------------------------------------------------------- op level: the table scene
def caller_mask():
    m = torch.zeros(R, R, dtype=torch.uint8)
    m[5:50, 9:60] = 3   # any value > 0 counts; the rectangle cuts the top and the floor
    m[20:30, 25:35] = 0
    return m


KINDS = ("dec", "painted", "erase_disc", "caller_mask")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pose", ["table_straight", "table_tilted", "table_close"])
def test_table_scene_matches_the_restatement(model, pose, kind):
    uv, ref_idx, proj = reference_render("table", pose)
    fov = POSES[pose][3]
    dec, painted, mask = DEC, None, stroke_ref.make_stamp_mask(R, 1)
    if kind == "painted":
        dec, painted = None, torch.rand(3, R, R, generator=torch.Generator().manual_seed(8))
    elif kind == "erase_disc":
        dec, mask = None, stroke_ref.disc_mask(R)
    elif kind == "caller_mask":
        mask = caller_mask()
    got, face_idx = device_backproject(model, "table", pose, dec, mask, painted=painted, occlude=1.0)
    assert torch.equal(face_idx, ref_idx)
    want, info = occ.backproject(proj, ref_idx, uv, dec, mask, TEXTURE, fov=fov, occlude=1.0, painted=painted)
    assert torch.equal(got, want)
    written = torch.from_numpy(info["written"])
    assert torch.equal(got[~written], TEXTURE[~written])
    # the case does what it is there for: texels with some taps rejected are written, texels with all of them rejected are not
    assert int((info["rejected"] & info["written"]).sum()) > 20 and info["n_unwritten"] > 100
    plain, plain_info = mesh_ref.backproject(proj, ref_idx, uv, dec, mask, TEXTURE, painted=painted)
    assert not torch.equal(want, plain)
    if kind == "erase_disc":
        assert int(got[written].sum()) == 0
    if pose == "table_close":
        assert float(np.abs(proj["ndc_x"]).max()) > 1.5 and float(np.abs(proj["ndc_y"]).max()) > 1.5
    else:  # the floor behind the top, from the geometry: left alone
        behind = torch.from_numpy(occ.table_floor_behind_the_top(mesh_ref.camera(*POSES[pose]), fov, R, H, W))
        assert int(behind.sum()) > 500 and torch.equal(got[behind], TEXTURE[behind])
        if kind == "dec":
            assert bool((plain[behind] != TEXTURE[behind]).any(dim=-1).all())  # the plain backprojection writes every one of them


def test_option_off_is_the_plain_call(model):
    """ops.mesh_backproject without the keyword, with None and with False: the plain entry point, the plain reference's bytes."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    uv, ref_idx, proj = reference_render("table", "table_tilted")
    mask = stroke_ref.make_stamp_mask(R, 1)
    want, _ = mesh_ref.backproject(proj, ref_idx, uv, DEC, mask, TEXTURE)
    got, _ = device_backproject(model, "table", "table_tilted", DEC, mask)
    assert torch.equal(got, want)
    p = POSES["table_tilted"]
    for off in (None, False):
        dtex = TEXTURE.to(DEV)
        _, face_idx = ops.mesh_render(device_mesh(model, "table"), mesh_camera(*p), p[3], dtex, R)
        ops.mesh_backproject(device_mesh(model, "table"), DEC.to(DEV), mask.to(DEV), face_idx, dtex, occlude=off)  # (no fov needed)
        assert torch.equal(dtex.cpu(), want)


# ---------------------------------------------------------------- op level: the height field
@pytest.mark.parametrize("occlude", [0.0, 0.25, 1.0])
def test_bumpy_field_from_a_tilted_pose_matches_the_restatement(model, occlude):
    uv, ref_idx, proj = reference_render("field", "field_tilted")
    fov = POSES["field_tilted"][3]
    mask = stroke_ref.make_stamp_mask(R, 1)
    got, face_idx = device_backproject(model, "field", "field_tilted", DEC, mask, occlude=occlude)
    assert torch.equal(face_idx, ref_idx)
    want, info = occ.backproject(proj, ref_idx, uv, DEC, mask, TEXTURE, fov=fov, occlude=occlude)
    assert torch.equal(got, want)
    some = int((info["rejected"] & info["written"]).sum())
    assert some > 0 and int(info["written"].sum()) > 9000
    if occlude == 0.0:  # neighbours across every shared edge reject each other: most texels take the renormalised branch, some lose all taps
        assert some > 4000 and info["n_unwritten"] > 10
    if occlude == 1.0:  # only where the bumps of the tilted field really hide each other
        assert some < 50
    erased, _ = device_backproject(model, "field", "field_tilted", None, stroke_ref.disc_mask(R), occlude=occlude)
    assert torch.equal(erased, occ.backproject(proj, ref_idx, uv, None, stroke_ref.disc_mask(R), TEXTURE, fov=fov, occlude=occlude)[0])


@pytest.mark.parametrize("pose", ["field_straight", "field_tilted"])
def test_one_pixel_on_the_smooth_field_is_the_plain_backprojection(model, pose):
    """No tap is rejected (tests/test_mesh_occlude_cpu.py asserts the count), so every texel takes the plain branch of the occluded
    kernel: its bytes are the plain kernel's."""
    mask = stroke_ref.make_stamp_mask(R, 1)
    plain, _ = device_backproject(model, "smooth", pose, DEC, mask)
    got, _ = device_backproject(model, "smooth", pose, DEC, mask, occlude=1.0)
    assert torch.equal(got, plain) and int((plain != TEXTURE).any(dim=-1).sum()) > 10000
    uv, ref_idx, proj = reference_render("smooth", pose)
    assert torch.equal(plain, mesh_ref.backproject(proj, ref_idx, uv, DEC, mask, TEXTURE)[0])


def test_a_face_set_together_with_occlude(model):
    from diffusiontexturepainting_amd import mesh as M
    uv, ref_idx, proj = reference_render("table", "table_tilted")
    fov = POSES["table_tilted"][3]
    mask = stroke_ref.make_stamp_mask(R, 1)
    for sel in (np.array([True, False, True, False]), np.array([True, True, False, False]), np.zeros(4, dtype=bool)):
        face_mask = M.faceset_from_bool(torch.from_numpy(sel)).to(DEV)
        got, _ = device_backproject(model, "table", "table_tilted", DEC, mask, face_mask=face_mask, occlude=1.0)
        want, info = occ.backproject(proj, ref_idx, uv, DEC, mask, TEXTURE, fov=fov, occlude=1.0, selected=sel)
        assert torch.equal(got, want)
        # the set decides which faces are written, the test which of their texels: the unselected top still hides the floor
        only_set, _ = select_ref.backproject(proj, ref_idx, uv, DEC, mask, TEXTURE, sel)
        if sel.any():
            assert info["n_unwritten"] > 100 and not torch.equal(want, only_set)
        else:
            assert torch.equal(got, TEXTURE)


# ---------------------------------------------------------------- strokes
STAMP = POSES["table_straight"]
SEED = 900


def stroke_args(n=1):
    return ([STAMP[0]] * n, [STAMP[1]] * n, [STAMP[2]] * n, STAMP[3])


def host_loop(model, dm, tex, occlude):
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    tex = tex.clone()
    canvas, face_idx = ops.mesh_render(dm, mesh_camera(*STAMP), STAMP[3], tex, R)
    painted = model.generate_raw(canvas, seeds=[SEED], **ST)
    ops.mesh_backproject(dm, None, stroke_ref.make_stamp_mask(R, 1).to(DEV), face_idx, tex, painted=painted, fov=STAMP[3], occlude=occlude)
    return tex


@pytest.fixture(scope="module")
def strokes(model):
    """The one-stamp stroke on the table scene from straight above, with the test and without, each painted once."""
    dm = device_mesh(model, "table")
    plain = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), *stroke_args(), seeds=[SEED], **ST)
    info = model.stroke_info()
    occluded = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), *stroke_args(), seeds=[SEED], occlude=True, **ST)
    assert model.stroke_info() == info == dict(stamps=1, groups=1, unet_evals=3)
    torch.cuda.synchronize()
    return dict(dm=dm, plain=plain, occluded=occluded)


def test_stroke_leaves_the_floor_under_the_table_alone_and_equals_the_host_loop(model, strokes):
    s = strokes
    behind = torch.from_numpy(occ.table_floor_behind_the_top(mesh_ref.camera(*STAMP), STAMP[3], R, H, W))
    assert int(behind.sum()) > 500
    got = s["occluded"].cpu()
    assert torch.equal(got[behind], TEXTURE[behind])
    assert torch.equal(s["occluded"], host_loop(model, s["dm"], TEXTURE.to(DEV), True))
    assert torch.equal(s["occluded"], host_loop(model, s["dm"], TEXTURE.to(DEV), 1.0))
    # the rest of the floor and the top were painted
    changed = (got != TEXTURE).any(dim=-1)
    assert int(changed[:, :W // 2].sum()) > 4000 and int(changed[:, W // 2:].sum()) > 4000
    # without the option those texels change -- the leak, pinned -- and the call is the plain one
    plain = s["plain"].cpu()
    assert bool((plain[behind] != TEXTURE[behind]).any(dim=-1).all())
    assert torch.equal(s["plain"], host_loop(model, s["dm"], TEXTURE.to(DEV), None))
    assert torch.equal(plain[:, W // 2:], got[:, W // 2:])  # the top's own texels do not depend on the option
    for off in (None, False):
        again = model.paint_mesh_stroke(s["dm"], TEXTURE.to(DEV), *stroke_args(), seeds=[SEED], occlude=off, **ST)
        assert torch.equal(again, s["plain"])


def test_an_erase_stroke_follows_the_rule(model, strokes):
    uv, ref_idx, proj = reference_render("table", "table_straight")
    want, info = occ.backproject(proj, ref_idx, uv, None, stroke_ref.disc_mask(R), TEXTURE, fov=STAMP[3], occlude=0.5)
    out = model.paint_mesh_stroke(strokes["dm"], TEXTURE.to(DEV), *stroke_args(), modes="erase", occlude=0.5, **ST)
    assert torch.equal(out.cpu(), want) and info["n_unwritten"] > 100
    assert model.stroke_info() == dict(stamps=1, groups=1, unet_evals=0)


def test_the_path_passes_the_option_through(model, strokes):
    """paint_mesh_path(occlude=) is paint_mesh_stroke(occlude=) on the stamps it plans."""
    dm = strokes["dm"]
    origins, directions = [(-0.7, -0.6, 3.0), (-0.2, -0.6, 3.0)], [(0.0, 0.0, -1.0)] * 2
    hits = model.pick(dm, origins, directions)
    positions, normals, prevs, _ = dm.plan_path(hits, 0.4)
    assert positions.shape[0] == 1
    tex, _, n = model.paint_mesh_path(dm, TEXTURE.to(DEV), origins, directions, 0.4, fov=0.9, seeds=[SEED], occlude=0.75, **ST)
    want = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), positions, normals, prevs, 0.9, seeds=[SEED], occlude=0.75, **ST)
    plain = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), positions, normals, prevs, 0.9, seeds=[SEED], **ST)
    assert n == 1 and torch.equal(tex, want) and not torch.equal(tex, plain)


def test_bleed_journal_and_undo_with_occlude(model, strokes):
    dm = strokes["dm"]
    tex = TEXTURE.to(DEV)
    j = model.journal(tex)
    with j.stroke():
        model.paint_mesh_stroke(dm, tex, *stroke_args(2), seeds=[SEED, SEED + 1], modes=[INPAINT, ERASE], bleed=2, occlude=True, **ST)
    painted = tex.clone()
    behind = torch.from_numpy(occ.table_floor_behind_the_top(mesh_ref.camera(*STAMP), STAMP[3], R, H, W))
    assert not torch.equal(painted.cpu(), TEXTURE) and torch.equal(painted.cpu()[behind], TEXTURE[behind])
    assert j.undo() is True and torch.equal(tex.cpu(), TEXTURE)
    assert j.redo() is True and torch.equal(tex, painted)
    assert j.undo() is True and torch.equal(tex.cpu(), TEXTURE)
    j.close()
    # the same stroke without a journal paints the same bytes, and the bleed pass wrote the gutter
    again = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), *stroke_args(2), seeds=[SEED, SEED + 1], modes=[INPAINT, ERASE], bleed=2, occlude=True, **ST)
    assert torch.equal(again, painted)
    no_bleed = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), *stroke_args(2), seeds=[SEED, SEED + 1], modes=[INPAINT, ERASE], occlude=True, **ST)
    assert int((again != no_bleed).any(dim=-1).sum()) > 20


def test_refusals_leave_the_texture_alone_and_do_not_wait(model, strokes):
    from diffusiontexturepainting_amd import _lib, mesh as _mesh, ops
    dm = strokes["dm"]
    tex = TEXTURE.to(DEV)
    lib = _lib.load()
    # ---- the Python keyword, before anything is enqueued
    for bad in (-1.0, float("nan"), float("inf"), "yes"):
        with pytest.raises(ValueError, match="occlude"):
            model.paint_mesh_stroke(dm, tex, *stroke_args(), seeds=[SEED], occlude=bad, **ST)
        with pytest.raises(ValueError, match="occlude"):
            model.paint_mesh_path(dm, tex, [(-0.7, -0.6, 3.0), (-0.2, -0.6, 3.0)], [(0.0, 0.0, -1.0)] * 2, 0.4, occlude=bad, **ST)
    _, face_idx = ops.mesh_render(dm, _mesh.mesh_camera(*STAMP), STAMP[3], tex, R)
    disc = stroke_ref.disc_mask(R).to(DEV)
    with pytest.raises(ValueError, match="occlude needs fov"):
        ops.mesh_backproject(dm, None, disc, face_idx, tex, occlude=True)
    with pytest.raises(ValueError, match="occlude"):
        ops.mesh_backproject(dm, None, disc, face_idx, tex, fov=STAMP[3], occlude=-2.0)
    with pytest.raises(_lib.DtpError, match="fov=0"):
        ops.mesh_backproject(dm, None, disc, face_idx, tex, fov=0.0, occlude=1.0)
    # ---- the C entry points, behind a queued stroke: each refusal returns at once
    st = _lib.Settings(ST["steps"], ST["context_pad"], ST["tg_steps"], ST["cfg_weight"], 1.0, 0, 0)
    opts = _lib.MeshStrokeOpts(0, 1, 10, 25, 1, 1.0)
    far = 1e5  # a legal fov at which 3e38 pixels of tolerance overflow fp32

    def stamps(fovs):
        n = len(fovs)
        return _mesh.mesh_stamps([STAMP[0]] * n, [STAMP[1]] * n, [STAMP[2]] * n, fovs, [SEED] * n, [INPAINT] * n, None)

    def stroke(occlude, fovs=(1.0,), bleed=0, words=0, face_mask=None):
        return lib.dtp_mesh_stroke_occluded(model._h, dm.handle, _lib.ptr(tex), H, W, stamps(list(fovs)), len(fovs), C.byref(st), C.byref(opts), None,
                                            bleed, face_mask, words, C.c_float(occlude), model._s())

    cur = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def op(fov, occlude, r=R, words=0, face_mask=None):
        return lib.dtp_op_mesh_backproject_occluded(dm.handle, None, 0, _lib.ptr(disc), _lib.ptr(face_idx), r, _lib.ptr(tex), H, W, face_mask, words,
                                                    C.c_float(fov), C.c_float(occlude), cur)

    good = _mesh.faceset_from_bool(torch.ones(4, dtype=torch.bool)).to(DEV)
    torch.cuda.synchronize()
    work = TEXTURE.to(DEV)
    t0 = time.perf_counter()
    model.paint_mesh_stroke(dm, work, *stroke_args(4), seeds=[SEED] * 4, occlude=True, **ST)  # keeps the stroke's stream busy
    t1 = time.perf_counter()
    cases = [(lambda: stroke(-1.0), rb"dtp_mesh_stroke_occluded: occlude=-1 "), (lambda: stroke(float("nan")), rb"occlude=-?nan"),
             (lambda: stroke(float("inf")), rb"occlude=inf"),
             (lambda: stroke(3e38, fovs=(far,)), rb"stamp 0: the tolerance of occlude=3e\+38 at fov=100000 does not fit fp32"),
             (lambda: stroke(3e38, fovs=(1.0, far)), rb"stamp 1: the tolerance"),
             (lambda: stroke(1.0, bleed=17), rb"bleed=17"),
             (lambda: stroke(1.0, words=2, face_mask=_lib.ptr(good)), rb"2 words for 4 faces"),
             (lambda: op(1.0, -1.0), rb"dtp_op_mesh_backproject_occluded: occlude=-1 "), (lambda: op(float("inf"), 1.0), rb"fov=inf"),
             (lambda: op(far, 3e38), rb"does not fit fp32"), (lambda: op(1.0, 1.0, r=0), rb"R=0 "),
             (lambda: op(1.0, 1.0, words=3, face_mask=_lib.ptr(good)), rb"3 words for 4 faces")]
    for call, word in cases:
        assert call() == 1 and re.search(word, lib.dtp_last_error()), lib.dtp_last_error()
    t_refusals = time.perf_counter() - t1
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"4-stamp stroke enqueued in {(t1 - t0) * 1e3:.1f} ms, done after {t_all * 1e3:.1f} ms; {len(cases)} refusals behind it returned in "
          f"{t_refusals * 1e3:.2f} ms")
    assert t_refusals < 0.5 * t_all
    assert torch.equal(tex.cpu(), TEXTURE)
    # a legal call with the largest tolerance is the plain stroke: nothing is in front by that much
    huge = model.paint_mesh_stroke(dm, TEXTURE.to(DEV), *stroke_args(), seeds=[SEED], occlude=1e30, **ST)
    assert torch.equal(huge, strokes["plain"])
