"""The undo / redo journal of a texture on the device (dtp_journal_*, `model.journal`; include/dtp.h "undo / redo journal of a texture")
against the numpy restatement of the contract (tests/journal_ref.py): the op-level save and swap, 2D strokes, mesh strokes with and
without the bleed pass, several records, the ring, strokes that are not journalled, enqueue without a host wait, and the refusals.  Every
comparison is torch.equal: the journal moves bytes.  One 64^2 context (max_batch 2), DDIM, 4 steps, as tests/test_gpu_mesh_bleed.py."""
import re
import time

import pytest
import torch

import bleed_ref
import journal_ref
import mesh_ref

pytestmark = pytest.mark.gpu

R = 64
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
OVER = (10, 25)
DEV = "cuda:0"
SIZES = [(96, 160), (90, 150)]


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
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=2)
    _, brush, _, _ = synthetic.make_stamp_batch(1, R, 6000)
    cond, uncond = synthetic.make_conditioning(6100)
    m.set_conditioning(cond, uncond, brush, slot=0)
    return m


def height_field():
    from diffusiontexturepainting_amd import synthetic
    return synthetic.make_height_field(17, 13, seed=3)


@pytest.fixture(scope="module")
def mesh(model):
    return model.load_mesh(*height_field())


def roundtrip(model, tex0, paint, want_tiles, **kw):
    """tex0 (host) painted by paint(texture) inside one record: the bytes are the unjournalled ones, the saved tiles are want_tiles, each
    once, head advanced by their number, undo gives tex0 and redo the painted texture.  -> the painted texture (host)."""
    plain = tex0.to(DEV)
    paint(plain)
    tex = tex0.to(DEV)
    j = model.journal(tex, **kw)
    assert j.info() == dict(records=0, cursor=0, open=False, head=0)
    with j.stroke():
        assert j.info()["open"]
        paint(tex)
    assert torch.equal(tex, plain)
    info = j.info()
    tiles = j.tiles(0)
    assert len(tiles) == len(set(tiles)), "a tile was saved twice in one record"
    assert set(tiles) == set(want_tiles)
    assert info == dict(records=1, cursor=1, open=False, head=len(tiles))
    assert j.record(0) == dict(start=0, end=len(tiles), restorable=True)
    assert j.undo() is True
    assert torch.equal(tex.cpu(), tex0)
    assert j.info() == dict(records=1, cursor=0, open=False, head=len(tiles))
    assert j.redo() is True
    assert torch.equal(tex, plain)
    assert j.undo() and torch.equal(tex.cpu(), tex0) and j.redo() and torch.equal(tex, plain)  # the swap is its own inverse, again
    j.close()
    return plain.cpu()


# ---------------------------------------------------------------- 1. op level: touch, overwrite with torch, undo, redo
TOUCH = {
    "one_texel": ((96, 160), [[(37, 21, 37, 21)]]),
    "on_one_tile": ((96, 160), [[(33, 17, 40, 30)]]),
    "straddles_four_tiles": ((96, 160), [[(10, 10, 20, 20)]]),
    "whole_texture": ((96, 160), [[(0, 0, 159, 95)]]),
    "same_tile_twice_in_one_call": ((96, 160), [[(1, 1, 3, 3), (5, 5, 9, 9), (0, 0, 20, 3), (1, 1, 3, 3)]]),
    "same_tile_in_two_calls": ((96, 160), [[(33, 17, 40, 30)], [(30, 20, 50, 25)], [(33, 17, 40, 30)]]),
    "partial_corner_tile_90x150": ((90, 150), [[(145, 85, 149, 89)]]),
    "partial_edges_90x150": ((90, 150), [[(0, 80, 149, 89)], [(144, 0, 149, 89)]]),
    "whole_90x150_clipped": ((90, 150), [[(-5, -5, 400, 400)]]),
    "forty_rectangles_in_one_call": ((90, 150), [[(3 * i, 2 * i, 3 * i + 20, 2 * i + 9) for i in range(40)]]),
    "partly_and_wholly_outside": ((96, 160), [[(150, 90, 170, 99), (160, 0, 170, 5), (-9, -9, -1, -1)]]),
}


@pytest.mark.parametrize("name", sorted(TOUCH))
def test_touch_overwrite_undo_redo(model, name):
    (h, w), calls = TOUCH[name]
    want = set()
    for rects in calls:
        for r in rects:
            want |= journal_ref.rect_tiles(h, w, r)
    fill = random_texture(h, w, 11).to(DEV)

    def paint(tex, j=None):
        for rects in calls:
            if j is not None:
                j.touch(rects)
            for x0, y0, x1, y1 in rects:  # the client's own write, through torch
                ys, xs = slice(max(y0, 0), max(y1 + 1, 0)), slice(max(x0, 0), max(x1 + 1, 0))
                tex[ys, xs] = fill[ys, xs]

    tex0 = random_texture(h, w, 10)
    plain = tex0.to(DEV)
    paint(plain)
    tex = tex0.to(DEV)
    j = model.journal(tex, capacity_tiles=journal_ref.tile_count(h, w))
    with j.stroke():
        paint(tex, j)
    tiles = j.tiles(0)
    assert len(tiles) == len(set(tiles)) and set(tiles) == want
    assert j.info() == dict(records=1, cursor=1, open=False, head=len(want))
    assert torch.equal(tex, plain) and not torch.equal(tex.cpu(), tex0)
    assert j.undo() and torch.equal(tex.cpu(), tex0)
    assert j.redo() and torch.equal(tex, plain)
    # the restatement's journal goes through the same states
    ref_tex = tex0.numpy().copy()
    ref = journal_ref.Journal(ref_tex, journal_ref.tile_count(h, w))
    ref.begin()
    for rects in calls:
        ref.touch(rects)
    ref.end()
    assert set(ref.tiles(0)) == set(tiles)
    j.close()


# ---------------------------------------------------------------- 2. 2D strokes
STROKES_2D = {
    # name: (size, positions, modes, wrap, max_group)
    "three_modes": ((96, 160), [(10, 8), (60, 20), (100, 30)], ["inpaint", "overpaint", "erase"], False, 1),
    "partly_outside": ((90, 150), [(-20, 50), (120, -30)], ["inpaint", "erase"], False, 1),
    "wrap_across_the_border": ((90, 150), [(130, 60), (-10, -10)], ["inpaint", "overpaint"], True, 1),
    "wrap_pieces_share_a_tile": ((64, 72), [(12, 3)], ["erase"], True, 1),
    "group_of_two_sharing_a_tile": ((96, 160), [(8, 0), (72, 16)], ["inpaint", "inpaint"], False, 2),
}


@pytest.mark.parametrize("name", sorted(STROKES_2D))
def test_2d_stroke(model, name):
    (h, w), positions, modes, wrap, max_group = STROKES_2D[name]
    want = set()
    per_window = [set(journal_ref.window_tiles(h, w, R, x, y, wrap)) for x, y in positions]
    for t in per_window:
        want |= t
    if name == "group_of_two_sharing_a_tile":
        assert model.plan_stroke(positions, h, w, modes=modes, wrap=wrap, max_group=2) == [0, 0]  # one group, disjoint windows
        assert per_window[0] & per_window[1]
    if name == "wrap_pieces_share_a_tile":
        assert len(want) == 20  # all of them: the pieces 12 .. 71 and 0 .. 3 both meet tile column 0

    def paint(tex):
        model.paint_stroke(tex, positions, seeds=40, modes=modes, wrap=wrap, max_group=max_group, overpaint_margins=OVER, **ST)

    tex0 = random_texture(h, w, 21)
    after = roundtrip(model, tex0, paint, want)
    assert not torch.equal(after, tex0)
    if name == "group_of_two_sharing_a_tile":
        assert model.stroke_info()["groups"] == 1


# ---------------------------------------------------------------- 3. mesh strokes
# the three stamps of tests/test_gpu_mesh.py, and one from below the field: its window meets the mesh's box and shows no front face
STROKE = dict(positions=[(0.1, -0.05, 0.1), (0.3, 0.05, 0.1), (0.2, 0.2, 0.1)],
              normals=[(0.35, -0.2, 0.9), (0.0, 0.0, 1.0), (-0.2, 0.1, 0.95)],
              prevs=[(0.0, 0.3, 0.15), (0.1, -0.05, 0.1), (0.3, 0.05, 0.1)],
              fov=[0.45, 0.4, 0.5])
ARGS = (STROKE["positions"], STROKE["normals"], STROKE["prevs"], STROKE["fov"])
MODES = ["inpaint", "overpaint", "erase"]
BELOW = ([(0.1, 0.0, 0.0)], [(0.0, 0.0, -1.0)], [(0.1, 0.4, 0.0)], [0.4])


def stamp_tiles(model, mesh, h, w, args, k):
    """The tiles of each stamp's valid-face texel box grown by k, from the restatements, on the host loop: face_idx depends on the mesh
    and the camera alone, so a render of any texture gives it."""
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd.mesh import mesh_camera
    v, f, uv = height_field()
    blank = torch.zeros(h, w, 4, dtype=torch.uint8, device=DEV)
    out = []
    for i in range(len(args[0])):
        cam = mesh_camera(args[0][i], args[1][i], args[2][i], args[3][i])
        _, face_idx = ops.mesh_render(mesh, cam, args[3][i], blank, R)
        proj = mesh_ref.project(v, f, mesh_ref.camera(args[0][i], args[1][i], args[2][i], args[3][i]), args[3][i], R)
        rect = bleed_ref.stamp_rect(proj, face_idx, uv, h, w, k)
        out.append(set() if rect is None else journal_ref.rect_tiles(h, w, rect))
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bleed", [0, 3])
def test_mesh_stroke(model, mesh, bleed, size):
    h, w = size
    per_stamp = stamp_tiles(model, mesh, h, w, ARGS, bleed)
    assert all(per_stamp) and per_stamp[0] & per_stamp[1]  # every stamp saves something, and they overlap
    want = set().union(*per_stamp)
    assert len(want) < journal_ref.tile_count(h, w)  # a part of the texture, not all of it

    def paint(tex):  # bleed 0: dtp_mesh_stroke; otherwise dtp_mesh_stroke_bleed
        model.paint_mesh_stroke(mesh, tex, *ARGS, seeds=700, modes=MODES, overpaint_margins=OVER, bleed=bleed, **ST)

    tex0 = random_texture(h, w, 77)
    after = roundtrip(model, tex0, paint, want)
    changed = (after != tex0).any(dim=-1)
    assert int(changed.sum()) > 200
    # every texel that changed lies on a saved tile
    rows, cols = torch.nonzero(changed, as_tuple=True)
    assert set(((rows // 16) * journal_ref.tiles_x(w) + cols // 16).tolist()) <= want


@pytest.mark.parametrize("bleed", [0, 3])
def test_a_stamp_that_shows_no_face_saves_nothing(model, mesh, bleed):
    h, w = 96, 160
    assert stamp_tiles(model, mesh, h, w, BELOW, bleed) == [set()]

    def paint(tex):
        model.paint_mesh_stroke(mesh, tex, *BELOW, seeds=5, bleed=bleed, **ST)

    tex0 = random_texture(h, w, 78)
    after = roundtrip(model, tex0, paint, set())
    assert model.stroke_info()["unet_evals"] > 0  # the window met the mesh's box: the stamp ran
    assert torch.equal(after, tex0)
    # and among stamps that do paint, undo still restores
    args = tuple(a + b for a, b in zip(BELOW, ARGS))
    want = set().union(*stamp_tiles(model, mesh, h, w, args, bleed))

    def paint4(tex):
        model.paint_mesh_stroke(mesh, tex, *args, seeds=5, modes=["inpaint"] + MODES, overpaint_margins=OVER, bleed=bleed, **ST)

    roundtrip(model, tex0, paint4, want)


def test_a_pointer_path_in_two_calls_is_one_record(model, mesh):
    h, w = 96, 160
    o = [(-0.62, -0.3, 2.0), (-0.5, -0.22, 2.0), (2.5, 0.0, 2.0), (-0.2, -0.1, 2.0), (-0.12, -0.08, 2.0), (0.15, 0.05, 2.0), (0.45, 0.2, 2.0),
         (0.7, 0.3, 2.0)]
    d = [(0.05, 0.02, -1.0)] * 8
    tex0 = random_texture(h, w, 79)
    plain = tex0.to(DEV)
    _, _, n = model.paint_mesh_path(mesh, plain, o, d, 0.25, seeds=900, bleed=2, **ST)
    assert n >= 4
    tex = tex0.to(DEV)
    j = model.journal(tex)
    j.begin()
    _, state, n1 = model.paint_mesh_path(mesh, tex, o[:4], d[:4], 0.25, seeds=900, bleed=2, **ST)
    _, state, n2 = model.paint_mesh_path(mesh, tex, o[4:], d[4:], 0.25, seeds=900 + n1, bleed=2, state=state, **ST)
    j.end()
    assert n1 > 0 and n2 > 0 and n1 + n2 == n
    assert torch.equal(tex, plain)
    info = j.info()
    tiles = j.tiles(0)
    assert info["records"] == 1 and info["head"] == len(tiles) == len(set(tiles)) > 0
    assert j.undo() and torch.equal(tex.cpu(), tex0)
    assert j.undo() is False
    assert j.redo() and torch.equal(tex, plain)
    j.close()


# ---------------------------------------------------------------- 4. several records
def three_strokes(model, tex, j=None):
    """Three overlapping strokes, each its own record when a journal is given -> the textures before, between and after (host)."""
    import contextlib
    states = [tex.cpu()]
    strokes = [dict(positions=[(10, 8)], modes="inpaint"), dict(positions=[(40, 20), (70, 30)], modes=["erase", "inpaint"]),
               dict(positions=[(30, -10)], modes="overpaint")]
    for i, s in enumerate(strokes):
        with (j.stroke() if j is not None else contextlib.nullcontext()):
            model.paint_stroke(tex, seeds=300 + 10 * i, overpaint_margins=OVER, **s, **ST)
        states.append(tex.cpu())
    return states


def test_three_records_undo_and_redo_in_turn(model):
    tex = random_texture(96, 160, 31).to(DEV)
    j = model.journal(tex)
    states = three_strokes(model, tex, j)
    assert not any(torch.equal(states[i], states[i + 1]) for i in range(3))
    want = three_strokes(model, states[0].to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(states, want))
    assert j.info()["records"] == 3 and j.info()["cursor"] == 3
    sizes = [len(j.tiles(i)) for i in range(3)]
    assert sizes == [len(journal_ref.window_tiles(96, 160, R, 10, 8)),
                     len(set(journal_ref.window_tiles(96, 160, R, 40, 20)) | set(journal_ref.window_tiles(96, 160, R, 70, 30))),
                     len(journal_ref.window_tiles(96, 160, R, 30, -10))]
    assert [j.record(i)["start"] for i in range(3)] == [0, sizes[0], sizes[0] + sizes[1]]
    for k in (2, 1, 0):
        assert j.undo() and torch.equal(tex.cpu(), states[k])
        assert j.info()["cursor"] == k
    assert j.undo() is False and torch.equal(tex.cpu(), states[0])
    for k in (1, 2, 3):
        assert j.redo() and torch.equal(tex.cpu(), states[k])
    assert j.redo() is False and torch.equal(tex.cpu(), states[3])
    # undo once, then a new stroke: the undone record is gone, and head was not rewound
    assert j.undo() and torch.equal(tex.cpu(), states[2])
    head = j.info()["head"]
    with j.stroke():
        model.paint_stroke(tex, [(90, 40)], seeds=7, modes="erase", **ST)
    newest = tex.cpu()
    assert j.redo() is False and torch.equal(tex.cpu(), newest)
    info = j.info()
    assert info["records"] == 3 and info["cursor"] == 3 and info["head"] == head + len(journal_ref.window_tiles(96, 160, R, 90, 40))
    assert j.record(2)["start"] == head
    assert j.undo() and torch.equal(tex.cpu(), states[2]) and j.undo() and torch.equal(tex.cpu(), states[1])
    j.close()


def test_depth_two_keeps_two_records(model):
    tex = random_texture(96, 160, 32).to(DEV)
    j = model.journal(tex, depth=2)
    states = three_strokes(model, tex, j)
    assert j.info()["records"] == 2
    assert j.undo() and torch.equal(tex.cpu(), states[2])
    assert j.undo() and torch.equal(tex.cpu(), states[1])
    assert j.undo() is False
    assert torch.equal(tex.cpu(), states[1])
    assert j.redo() and j.redo() and torch.equal(tex.cpu(), states[3])
    j.close()


# ---------------------------------------------------------------- 5. the ring
def test_the_ring_forgets_the_oldest_record_first(model):
    from diffusiontexturepainting_amd._lib import DtpError
    h, w = 96, 160
    a, b = (0, 0), (40, 20)
    n1, n2 = len(journal_ref.window_tiles(h, w, R, *a)), len(journal_ref.window_tiles(h, w, R, *b))
    ref = journal_ref.Records(capacity=n1 + n2 - 1, depth=10)  # the second record's last slot lands on the first record's first
    for n in (n1, n2):
        ref.begin(); ref.take(n); ref.end()
    assert not ref.restorable(0) and ref.restorable(1)
    tex0 = random_texture(h, w, 41)
    plain = tex0.to(DEV)
    model.paint_stroke(plain, [a], seeds=50, **ST)
    mid = plain.cpu()
    model.paint_stroke(plain, [b], seeds=51, modes="overpaint", overpaint_margins=OVER, **ST)
    tex = tex0.to(DEV)
    j = model.journal(tex, capacity_tiles=n1 + n2 - 1)
    with j.stroke():
        model.paint_stroke(tex, [a], seeds=50, **ST)
    with j.stroke():
        model.paint_stroke(tex, [b], seeds=51, modes="overpaint", overpaint_margins=OVER, **ST)
    assert torch.equal(tex, plain)  # a full ring changes nothing of what is painted
    assert j.record(0) == dict(start=0, end=n1, restorable=False) and j.record(1) == dict(start=n1, end=n1 + n2, restorable=True)
    assert j.undo() and torch.equal(tex.cpu(), mid)
    with pytest.raises(DtpError) as e:
        j.undo()
    assert re.search(r"\(code 3\)", str(e.value)) and re.search(rf"overwritten.*saved {n1} tiles.*capacity {n1 + n2 - 1}", str(e.value)), str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(tex.cpu(), mid)
    assert j.info() == dict(records=1, cursor=0, open=False, head=n1 + n2)  # it was dropped; the undone one stays
    assert j.undo() is False
    assert j.redo() and torch.equal(tex, plain)
    j.close()


def test_a_record_larger_than_the_ring_cannot_be_undone(model):
    from diffusiontexturepainting_amd._lib import DtpError
    h, w = 96, 160
    n1 = len(journal_ref.window_tiles(h, w, R, 40, 20))
    tex0 = random_texture(h, w, 42)
    plain = tex0.to(DEV)
    model.paint_stroke(plain, [(40, 20)], seeds=52, **ST)
    tex = tex0.to(DEV)
    j = model.journal(tex, capacity_tiles=n1 - 1)
    with j.stroke():
        model.paint_stroke(tex, [(40, 20)], seeds=52, **ST)
    assert torch.equal(tex, plain)
    assert j.record(0) == dict(start=0, end=n1, restorable=False)
    with pytest.raises(DtpError, match="overwritten"):
        j.tiles(0)
    with pytest.raises(DtpError, match=rf"overwritten.*saved {n1} tiles.*capacity {n1 - 1}"):
        j.undo()
    torch.cuda.synchronize()
    assert torch.equal(tex, plain)
    assert j.info() == dict(records=0, cursor=0, open=False, head=n1)
    # the journal goes on: a record that fits
    with j.stroke():
        model.paint_stroke(tex, [(-50, -50)], seeds=53, modes="erase", **ST)
    assert j.undo() and torch.equal(tex, plain)
    j.close()


# ---------------------------------------------------------------- 6. not armed, or not this texture
def test_strokes_that_are_not_journalled(model, mesh):
    h, w = 96, 160
    tex0 = random_texture(h, w, 51)

    def paint2d(t):
        model.paint_stroke(t, [(10, 8), (100, 30)], seeds=60, modes=["inpaint", "erase"], **ST)

    def paint_mesh(t):
        model.paint_mesh_stroke(mesh, t, *ARGS, seeds=61, modes=MODES, overpaint_margins=OVER, bleed=2, **ST)

    want2d, want_mesh = tex0.to(DEV), tex0.to(DEV)
    paint2d(want2d)
    paint_mesh(want_mesh)
    tex = tex0.to(DEV)
    j = model.journal(tex)
    # no record open
    paint2d(tex)
    assert torch.equal(tex, want2d) and j.info() == dict(records=0, cursor=0, open=False, head=0)
    # a record open, and strokes on another tensor of the same size, and on one of another size
    other, other_mesh, small = tex0.to(DEV), tex0.to(DEV), random_texture(90, 150, 52).to(DEV)
    small_want = small.clone()
    paint2d(small_want)
    j.begin()
    paint2d(other)
    paint_mesh(other_mesh)
    paint2d(small)
    assert j.info() == dict(records=1, cursor=1, open=True, head=0)
    j.end()
    assert torch.equal(other, want2d) and torch.equal(other_mesh, want_mesh) and torch.equal(small, small_want)
    assert j.tiles(0) == [] and torch.equal(tex, want2d)
    assert j.undo() and torch.equal(tex, want2d)  # an empty record: nothing to swap
    j.close()


# ---------------------------------------------------------------- 7. asynchrony
def test_journalled_mesh_stroke_does_not_block_the_host(model, mesh):
    """The criterion of test_mesh_stroke_enqueue_does_not_block_the_host: the host is back long before the device is done."""
    tex = random_texture(96, 160, 77).to(DEV)
    args = tuple(a * 2 for a in ARGS)
    j = model.journal(tex)
    for _ in range(2):  # programs, graphs, the masks and the coverage exist from here on
        with j.stroke():
            model.paint_mesh_stroke(mesh, tex, *args, seeds=1, bleed=2, **ST)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    j.begin()
    model.paint_mesh_stroke(mesh, tex, *args, seeds=1, bleed=2, **ST)
    j.end()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"host enqueue of a journalled 6-stamp mesh stroke {t_host * 1e3:.1f} ms, device done after {t_all * 1e3:.1f} ms")
    assert t_host < 0.5 * t_all
    assert j.info()["records"] == 3 and len(j.tiles(2)) > 0
    j.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_texture_and_journal_alone(model):
    from diffusiontexturepainting_amd._lib import DtpError
    tex = random_texture(96, 160, 61).to(DEV)
    j = model.journal(tex, capacity_tiles=8, depth=3)
    before = tex.clone()

    def refused(code, pattern, call):
        info = j.info()
        with pytest.raises(DtpError) as e:
            call()
        torch.cuda.synchronize()
        assert re.search(rf"\(code {code}\)", str(e.value)) and re.search(pattern, str(e.value)), str(e.value)
        assert torch.equal(tex, before) and j.info() == info

    refused(3, "dtp_journal_end: no record is open", j.end)
    refused(3, "dtp_journal_touch: no record is open", lambda: j.touch([(0, 0, 5, 5)]))
    assert j.undo() is False and j.redo() is False
    assert b"nothing to redo" in model._lib.dtp_last_error()
    j.begin()
    j.touch([(0, 0, 5, 5)])
    tex[0:6, 0:6] = 7
    before = tex.clone()
    refused(3, "dtp_journal_begin: a record is open already", j.begin)
    refused(3, "dtp_journal_undo: a record is open", j.undo)
    refused(3, "dtp_journal_redo: a record is open", j.redo)
    refused(1, r"rectangle 1 \(9, 0, 8, 0\)", lambda: j.touch([(0, 0, 40, 40), (9, 0, 8, 0)]))
    refused(1, r"n=0 rectangles", lambda: j.touch([]))
    other = model.journal(tex.clone())
    with pytest.raises(DtpError, match=r"\(code 3\).*another journal of this handle"):
        other.begin()
    assert other.info() == dict(records=0, cursor=0, open=False, head=0)
    j.end()
    assert j.info() == dict(records=1, cursor=1, open=False, head=1)
    other.begin()  # now it may
    other.end()
    other.close()
    with pytest.raises(DtpError, match=r"record 5 outside 0\.\.0"):
        j.record(5)
    # creation
    with pytest.raises(DtpError, match="capacity_tiles=0"):
        model.journal(tex, capacity_tiles=0)
    with pytest.raises(DtpError, match="depth=65"):
        model.journal(tex, depth=65)
    with pytest.raises(ValueError, match="uint8"):
        model.journal(tex.float())
    # a destroyed journal is refused, not followed
    handle = j.handle
    j.close()
    j._h = handle
    for call in (j.begin, j.end, j.undo, j.redo, j.info, lambda: j.touch([(0, 0, 1, 1)]), lambda: j.tiles(0)):
        with pytest.raises(DtpError, match=r"\(code 1\).*not a live journal"):
            call()
    j._h = None
    assert torch.equal(tex, before)
