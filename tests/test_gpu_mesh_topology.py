"""Growing a face set on the device (dtp_mesh_topology, dtp_mesh_topology_labels, dtp_mesh_select_extend; `Mesh.topology`,
`extend_selection`, `select_faces(extend=)`, `ops.faceset_extend`; include/dtp.h "growing a face set") against the numpy restatement
(tests/topo_ref.py): the labels, every extend on sets with and without stray tail bits, fresh and in place, linked as the fixed point of
rings, lasso -> extend -> masked stroke without a synchronise, and the refusals on a live mesh.  Every comparison is torch.equal or ==:
the feature has no float.  One 64^2 context, DDIM, 4 steps, as tests/test_gpu_mesh_select.py."""
import re

import numpy as np
import pytest
import torch

import select_ref
import topo_ref
from mesh_ref import ERASE, INPAINT

pytestmark = pytest.mark.gpu

R = 64
H, W = 96, 160
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
DEV = "cuda:0"
EYE, AT, UP, FOV, NEAR = (0.3, -0.5, 2.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.05


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


# ---------------------------------------------------------------- meshes and their reference topology, each made once and left unchanged
def mesh_data(name):
    from diffusiontexturepainting_amd import synthetic
    made = {"quad": synthetic.make_quad, "table_on_floor": synthetic.make_table_on_floor, "field_50": lambda: synthetic.make_height_field(6, 6),
            "field_384": lambda: synthetic.make_height_field(17, 13, seed=3), "field_2262": lambda: synthetic.make_height_field(40, 30)}
    if name in made:
        return tuple(t.numpy() for t in made[name]())
    if name == "field_50_split_seam":
        return topo_ref.split_seam(*mesh_data("field_50"))
    return {"fan": topo_ref.fan, "touching": topo_ref.touching, "touching_degenerate": lambda: topo_ref.touching(degenerate=True)}[name]()


LABEL_MESHES = ["quad", "table_on_floor", "field_50", "field_384", "field_50_split_seam", "fan", "touching", "touching_degenerate", "field_2262"]
# one word; two words, the second partial; twelve full words; 71 words, the last partial, and nine workgroups of 256
EXTEND_MESHES = {"table_on_floor": 4, "field_50": 50, "field_384": 384, "field_2262": 2262}
_meshes, _topos = {}, {}


def device_mesh(model, name):
    if name not in _meshes:
        _meshes[name] = model.load_mesh(*[torch.from_numpy(np.ascontiguousarray(a)) for a in mesh_data(name)])
    return _meshes[name]


def reference(name):
    if name not in _topos:
        _topos[name] = topo_ref.topology(*mesh_data(name))
    return _topos[name]


def sets(F):
    g = np.random.default_rng(100 + F)
    return {"empty": np.zeros(F, dtype=bool), "full": np.ones(F, dtype=bool), "one_face": np.arange(F) == F // 3, "last_face": np.arange(F) == F - 1,
            "random_0.02": g.random(F) < 0.02, "random_0.5": g.random(F) < 0.5}


def tail_bits(F):
    """int32 [(F + 31) // 32]: every bit at a position >= F."""
    return select_ref.pack(np.arange(32 * ((F + 31) // 32)) >= F)[:(F + 31) // 32]


# ---------------------------------------------------------------- labels
@pytest.mark.parametrize("name", LABEL_MESHES)
def test_topology_labels_match_the_restatement(model, name):
    dm, ref = device_mesh(model, name), reference(name)
    got = dm.topology()
    assert dm.topology() is got  # cached on the object
    assert sorted(got) == sorted(ref)
    for key in ("point", "part", "chart"):
        assert got[key].dtype == np.int32 and got[key].shape == ref[key].shape and (got[key] == ref[key]).all(), key
    for key in ("num_points", "num_parts", "num_charts", "num_faces"):
        assert got[key] == ref[key], key
    if name == "field_2262":
        assert got["num_faces"] == 2262 and got["num_parts"] == 1 and got["num_charts"] == 2
    # the library's two ways to the labels agree: the host-only entry point gives what the device holds
    from diffusiontexturepainting_amd import mesh as M
    host = M.topology_build(*[torch.from_numpy(np.ascontiguousarray(a)) for a in mesh_data(name)])
    assert all((host[k] == got[k]).all() for k in ("point", "part", "chart"))


# ---------------------------------------------------------------- extends
HOWS = [("rings", 1), ("rings", 2), ("rings", 5), ("shrink", 1), ("shrink", 2), ("shrink", 5), ("linked", 1), ("charts", 1)]


@pytest.mark.parametrize("name", sorted(EXTEND_MESHES, key=EXTEND_MESHES.get))
@pytest.mark.parametrize("how,rings", HOWS, ids=[f"{h}_{r}" for h, r in HOWS])
def test_extend_matches_the_restatement(model, how, rings, name):
    """Every set, plain and with every tail bit >= F set, into a fresh out (whose old words must not matter) and in place; all enqueued
    back to back on one stream, then compared."""
    from diffusiontexturepainting_amd import ops
    F, dm, topo = EXTEND_MESHES[name], device_mesh(model, name), reference(name)
    words, tail = (F + 31) // 32, tail_bits(F)
    runs = []
    for which, sel in sets(F).items():
        want = select_ref.pack(topo_ref.extend(topo, sel, how, rings))
        for stray in (False, True):
            src = select_ref.pack(sel) | tail if stray else select_ref.pack(sel)
            assert (select_ref.unpack(src, F) == sel).all()
            given = src.to(DEV)
            out = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            assert model.extend_selection(dm, given, how=how, rings=rings, out=out) is out
            fresh = model.extend_selection(dm, given, how=how, rings=rings)
            bare = ops.faceset_extend(dm, given, how, rings)
            place = src.to(DEV)
            assert model.extend_selection(dm, place, how=how, rings=rings, out=place) is place
            runs.append((which, stray, src, want, given, out, fresh, bare, place))
    torch.cuda.synchronize()
    for which, stray, src, want, given, out, fresh, bare, place in runs:
        assert torch.equal(given.cpu(), src), (which, stray)  # the source is only read
        for got in (out, fresh, bare, place):
            assert got.dtype == torch.int32 and tuple(got.shape) == (words,) and torch.equal(got.cpu(), want), (which, stray)
    by_name = {which: want for which, stray, _, want, *_ in runs if not stray}
    assert not by_name["empty"].any()                                     # the empty set stays empty in every mode
    assert torch.equal(by_name["full"], select_ref.pack(np.ones(F, dtype=bool)))  # and the full set full, SHRINK included; tail bits 0


# ---------------------------------------------------------------- linked is the fixed point of rings
def test_linked_is_the_fixed_point_of_rings(model):
    dm, F = device_mesh(model, "field_384"), 384
    corner = select_ref.pack(np.arange(F) == 0).to(DEV)
    linked = model.extend_selection(dm, corner, how="linked")
    assert torch.equal(model.extend_selection(dm, corner, how="rings", rings=16), linked)  # max(nx, ny) - 1 = 16 rings reach every face
    assert select_ref.unpack(linked, F).all()
    assert not select_ref.unpack(model.extend_selection(dm, corner, how="rings", rings=3), F).all()
    # 64 rings, the cap: 192 launches, the two scratch sets in turn
    assert torch.equal(model.extend_selection(dm, corner, how="rings", rings=64), linked)
    table = device_mesh(model, "table_on_floor")
    face_2 = select_ref.pack(np.arange(4) == 2).to(DEV)
    for how, rings in (("linked", 1), ("rings", 1), ("rings", 64), ("charts", 1)):
        assert np.nonzero(select_ref.unpack(model.extend_selection(table, face_2, how=how, rings=rings), 4))[0].tolist() == [2, 3], how


# ---------------------------------------------------------------- lasso -> extend -> masked stroke, in stream order
POSES = ([(0.1, -0.05, 0.1), (0.2, 0.2, 0.1)], [(0.35, -0.2, 0.9), (-0.2, 0.1, 0.95)], [(0.0, 0.3, 0.15), (0.3, 0.05, 0.1)],
         [0.45, 0.5])  # two stamps whose windows span the seam between the two charts
MODES, SEEDS, OVER = [INPAINT, ERASE], [700, 702], (10, 25)


def rectangle_inside_chart(host_idx, chart, label):
    """A 5 x 5 pixel rectangle of the frame whose every pixel shows a face of the chart `label`, as a polygon."""
    idx = host_idx.numpy()
    ok = (idx >= 0) & (chart[np.clip(idx, 0, None)] == label)
    whole = np.zeros_like(ok)
    whole[2:-2, 2:-2] = True
    for di in range(-2, 3):
        for dj in range(-2, 3):
            whole &= np.roll(ok, (di, dj), axis=(0, 1))
    at = np.argwhere(whole)
    assert len(at) > 0
    i, j = at[len(at) // 2]
    return [(j - 2.0, i - 2.0), (j + 3.0, i - 2.0), (j + 3.0, i + 3.0), (j - 2.0, i + 3.0)]


def test_lasso_extend_paint_needs_no_synchronise(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    name, F, size = "field_50", 50, (48, 80)
    dm, topo = device_mesh(model, name), reference(name)
    cam = view_camera(EYE, AT, UP, FOV, size, NEAR)
    texture = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(77))
    # the reference: the frame's faces, the lasso and the growth by numpy; the stroke masked by that set, with a synchronise at every step
    _, face_idx = model.render_view(dm, texture.to(DEV), cam, size, want_face_idx=True)
    torch.cuda.synchronize()
    host_idx = face_idx.cpu()
    poly = rectangle_inside_chart(host_idx, topo["chart"], 4)  # the chart right of the seam: the stamps' windows lie mostly in it
    hit = select_ref.hit_faces(host_idx, poly, F)
    grown = topo_ref.extend(topo, hit, "charts")
    assert 0 < int(hit.sum()) < int(grown.sum()) == 30 and (grown == (topo["chart"] == 4)).all()
    want = model.paint_mesh_stroke(dm, texture.to(DEV), *POSES, seeds=SEEDS, modes=MODES, overpaint_margins=OVER,
                                   face_mask=select_ref.pack(grown).to(DEV), **ST)
    torch.cuda.synchronize()
    want = want.cpu()
    # the device: enqueued back to back
    tex = texture.to(DEV)
    _, face_idx = model.render_view(dm, tex, cam, size, want_face_idx=True)
    sel = model.select_faces(dm, face_idx, poly, extend="charts")
    model.paint_mesh_stroke(dm, tex, *POSES, seeds=SEEDS, modes=MODES, overpaint_margins=OVER, face_mask=sel, **ST)
    torch.cuda.synchronize()
    assert torch.equal(sel.cpu(), select_ref.pack(grown))
    got = tex.cpu()
    assert torch.equal(got, want)
    # that chart lies in u > 0.5: the texels of the other chart are the input's, and the stroke did paint
    assert torch.equal(got[:, :W // 2], texture[:, :W // 2]) and int((got != texture).any(dim=-1).sum()) > 200
    # extend_selection after the lasso is the keyword, and "add" grows the edited set
    sel2 = model.extend_selection(dm, model.select_faces(dm, face_idx, poly), how="charts")
    assert torch.equal(sel2, sel)
    start = select_ref.pack(np.arange(F) == 0).to(DEV)
    model.select_faces(dm, face_idx, poly, op="add", out=start, extend="charts")
    assert select_ref.unpack(start, F).all()  # face 0 lies in the other chart


def test_select_faces_without_the_keyword_is_the_call_it_was(model):
    from diffusiontexturepainting_amd.mesh import view_camera
    name, F, size = "field_384", 384, (45, 77)
    dm = device_mesh(model, name)
    cam = view_camera(EYE, AT, UP, FOV, size, NEAR)
    _, face_idx = model.render_view(dm, torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV), cam, size, want_face_idx=True)
    poly = [(0.1 * size[1], 0.15 * size[0]), (0.9 * size[1], 0.3 * size[0]), (0.35 * size[1], 0.95 * size[0])]
    plain = model.select_faces(dm, face_idx, poly)
    assert torch.equal(model.select_faces(dm, face_idx, poly, extend=None), plain)
    assert torch.equal(model.select_faces(dm, face_idx, poly, extend=None, rings=7), plain)
    assert torch.equal(plain.cpu(), select_ref.pack(select_ref.hit_faces(face_idx.cpu(), poly, F))) and 0 < int(select_ref.unpack(plain, F).sum()) < F
    ring = model.select_faces(dm, face_idx, poly, extend="rings", rings=2)
    assert torch.equal(ring.cpu(), select_ref.pack(topo_ref.extend(reference(name), select_ref.unpack(plain, F), "rings", 2)))
    # a growth the library refuses leaves the lasso's set, and the caller's stream still waits for it
    from diffusiontexturepainting_amd._lib import DtpError
    out = torch.full_like(plain, 0x5A5A5A5A)
    with pytest.raises(DtpError, match="rings=65"):
        model.select_faces(dm, face_idx, poly, out=out, extend="rings", rings=65)
    assert torch.equal(out, plain)


# ---------------------------------------------------------------- refusals on a live mesh
def test_extend_refusals_leave_out_alone(model):
    from diffusiontexturepainting_amd import _lib, ops
    from diffusiontexturepainting_amd._lib import DtpError
    name, F = "field_50", 50
    dm = device_mesh(model, name)
    sel = select_ref.pack(sets(F)["random_0.5"]).to(DEV)
    big = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out = big[2:4]
    kept = big.clone()
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    args = [dm.handle, sel.data_ptr(), out.data_ptr(), 2, 0, 1, s]
    cases = [(3, 1, b"1 words for 50 faces"), (3, 3, b"3 words for 50 faces"), (4, 4, b"unknown how 4"), (5, 0, b"rings=0"), (5, 65, b"rings=65"),
             (0, None, b"NULL"), (1, None, b"NULL"), (2, None, b"NULL"), (1, sel.data_ptr() + 2, b"aligned"), (2, out.data_ptr() + 1, b"aligned"),
             (1, out.data_ptr() + 4, b"overlap"), (1, out.data_ptr() - 4, b"overlap")]
    for i, v, word in cases:
        bad = list(args)
        bad[i] = v
        assert lib.dtp_mesh_select_extend(*bad) == 1 and word in lib.dtp_last_error(), (i, v, lib.dtp_last_error())
    dead = model.load_mesh(*[torch.from_numpy(np.ascontiguousarray(a)) for a in mesh_data(name)])
    handle = dead.handle
    dead.close()
    assert lib.dtp_mesh_select_extend(handle, *args[1:]) == 1 and b"not a live mesh" in lib.dtp_last_error()
    assert lib.dtp_mesh_topology(handle, None, s) == 1 and b"not a live mesh" in lib.dtp_last_error()
    # the Python layer: the keywords and the sets, before anything is enqueued
    with pytest.raises(ValueError, match="how 'grow'"):
        model.extend_selection(dm, sel, how="grow", out=out)
    with pytest.raises(ValueError, match="rings"):
        model.extend_selection(dm, sel, rings=1.5, out=out)
    with pytest.raises(DtpError, match=re.escape("rings=65 (1..64)")):
        model.extend_selection(dm, sel, how="shrink", rings=65, out=out)
    with pytest.raises(ValueError, match="2 words for 50 faces"):
        model.extend_selection(dm, torch.zeros(3, dtype=torch.int32, device=DEV), out=out)
    with pytest.raises(ValueError, match="2 words for 50 faces"):
        model.extend_selection(dm, sel, out=big)
    with pytest.raises(ValueError, match="int32"):
        model.extend_selection(dm, sel.to(torch.int64), out=out)
    with pytest.raises(ValueError, match="it is on cpu"):
        model.extend_selection(dm, sel.cpu(), out=out)
    with pytest.raises(ValueError, match="contiguous"):
        model.extend_selection(dm, sel, out=big[::4])
    with pytest.raises(ValueError, match="load_mesh"):
        model.extend_selection(None, sel, out=out)
    with pytest.raises(ValueError, match="how 'grow'"):
        ops.faceset_extend(dm, sel, "grow")
    with pytest.raises(DtpError, match="overlap"):
        model.extend_selection(dm, big[1:3], out=out)
    with pytest.raises(ValueError, match="how 'grow'"):
        model.select_faces(dm, torch.zeros(8, 8, dtype=torch.int32, device=DEV), [(1, 1), (5, 1), (3, 5)], out=out, extend="grow")
    torch.cuda.synchronize()
    assert torch.equal(big, kept)
    # and a good call through the same view writes its two words alone
    model.extend_selection(dm, sel, how="linked", out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), select_ref.pack(np.ones(F, dtype=bool))) and (big[:2] == 0x5A5A5A5A).all() and (big[4:] == 0x5A5A5A5A).all()
