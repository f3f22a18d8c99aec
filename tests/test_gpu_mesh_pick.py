"""Picking on a mesh (dtp_mesh_pick, `model.pick`, `paint_mesh_path`; include/dtp.h "picking on a mesh"): the device's records against
the numpy restatement (tests/pick_ref.py) with torch.equal, field by field; the pointer-to-paint call byte for byte against the
restatement's picks and plan fed to paint_mesh_stroke; a pick that answers while a stroke is still queued; the refusals.  One 64^2
context with synthetic weights, DDIM.  Nothing is compared under a tolerance."""
import ctypes as C
import re
import time

import numpy as np
import pytest
import torch

import pick_ref

pytestmark = pytest.mark.gpu

R = 64
DEV = "cuda:0"
f32 = np.float32
DOWN, UP = (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)


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
def _t(v, f, uv):
    return (torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int32), torch.tensor(uv, dtype=torch.float32))


_cache = {}


def small_field():
    from diffusiontexturepainting_amd import synthetic
    if "small" not in _cache:
        _cache["small"] = synthetic.make_height_field(17, 13, seed=3)
    return _cache["small"]


def big_field():
    """100 352 faces over [-1, 1] x [-0.75, 0.75], z within about +-0.45."""
    from diffusiontexturepainting_amd import synthetic
    if "big" not in _cache:
        _cache["big"] = synthetic.make_height_field(225, 225)
    return _cache["big"]


def first_faces(mesh, n):
    v, f, uv = mesh
    return v, f[:n].contiguous(), uv[:n].contiguous()


LATTICE = [-0.75, -0.25, 0.25, 0.75]  # dyadic: a vertical ray through a vertex or an edge's midpoint passes through it exactly


def grid_3x3():
    """A 3 x 3 grid of squares, 18 faces, over dyadic coordinates with dyadic heights."""
    v = [[x, y, 0.125 * ((i * j) % 3)] for j, y in enumerate(LATTICE) for i, x in enumerate(LATTICE)]
    f, uv = [], []
    for j in range(3):
        for i in range(3):
            a, b, c, d = 4 * j + i, 4 * j + i + 1, 4 * j + i + 5, 4 * j + i + 4
            for tri in ((a, b, c), (a, c, d)):
                f.append(list(tri))
                uv.append([[(v[k][0] + 1) / 2, (v[k][1] + 1) / 2] for k in tri])
    return _t(v, f, uv)


def grid_points():
    """-> (shared, border): the interior lattice vertices and the midpoints of the edges two faces share; the midpoints of the border's
    edges, which one face has alone (the top-left rule gives such an edge to its face on two sides of the square only)."""
    shared = [(LATTICE[i], LATTICE[j]) for j in (1, 2) for i in (1, 2)]
    border = []
    for j in range(4):
        for i in range(3):
            mid = (LATTICE[i] + 0.25, LATTICE[j])
            (border if j in (0, 3) else shared).append(mid)            # along x
            (border if j in (0, 3) else shared).append(mid[::-1])      # along y
    shared += [(LATTICE[i] + 0.25, LATTICE[j] + 0.25) for j in range(3) for i in range(3)]  # the diagonals
    return shared, border


def both_windings():
    """Face 0 counter-clockwise seen from +z, face 1 clockwise, face 2 steep, face 3 of zero area ON TOP of face 0, face 4 a sliver whose
    snapped area may vanish, face 5 under face 0 (hidden from above, first from below)."""
    return _t([[-0.9, -0.9, 0.0], [-0.1, -0.9, 0.0], [-0.5, -0.1, 0.0],
               [0.1, -0.9, 0.0], [0.9, -0.9, 0.0], [0.5, -0.1, 0.0],
               [-0.9, 0.1, 0.0], [-0.6, 0.1, 1.0], [-0.9, 0.9, 0.0],
               [-0.7, -0.8, 0.5], [-0.3, -0.4, 0.5], [-0.3, -0.4, 0.5],
               [0.2, 0.2, 0.0], [0.8, 0.8, 0.0], [0.5, 0.5 + 1e-9, 0.0],
               [-0.9, -0.9, -0.25], [-0.1, -0.9, -0.25], [-0.5, -0.1, -0.25]],
              [[0, 1, 2], [3, 5, 4], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 17, 16]],
              [[[0.1, 0.1], [0.9, 0.15], [0.2, 0.9]]] * 6)


def scatter(n, seed, z=2.0, spread=(1.1, 0.85)):
    """n rays from a plane above (z > 0) or below the field: origins scattered a little beyond it, directions tilted."""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([spread[0], spread[1], 0.0]) + torch.tensor([0.0, 0.0, z])
    d = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([0.3, 0.3, 0.0]) + torch.tensor([0.0, 0.0, -1.0 if z > 0 else 1.0])
    return o, d


def field_rays():
    """The 64 rays of the big height field: straight down, oblique, grazing, missing the bounding box, starting inside the z range."""
    g = torch.Generator().manual_seed(17)
    u = (lambda n: torch.rand(n, generator=g) * 2 - 1)
    zeros, ones = torch.zeros(16), torch.ones(16)
    down = (torch.stack([u(16) * 0.98, u(16) * 0.73, 2 * ones], 1), torch.stack([zeros, zeros, -ones], 1))
    oblique = (torch.stack([u(16) * 0.5, u(16) * 0.4, 1.5 * ones], 1), torch.stack([u(16) * 0.6, u(16) * 0.6, -ones], 1))
    grazing = (torch.stack([-1.5 * ones, u(16) * 0.7, 0.3 + 0.2 * u(16)], 1), torch.stack([ones, u(16) * 0.2, -0.04 + 0.05 * u(16)], 1))
    h = torch.zeros(8)
    missing = (torch.stack([3 + u(8), u(8), 2 + h], 1), torch.stack([h, h, -1 + h], 1))          # beside the box, or pointing away from it
    missing[0][4:, 0] = u(4) * 0.9
    missing[1][4:, 2] = 1.0
    inside = (torch.stack([u(8) * 0.9, u(8) * 0.7, 0.1 * u(8)], 1), torch.stack([u(8), u(8), u(8)], 1))   # z of the origin inside the surface's range
    parts = (down, oblique, grazing, missing, inside)
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


# ---------------------------------------------------------------- device records against the restatement
_ref = {}


def reference(key, mesh, o, d):
    """Computed once per case and left unchanged."""
    if key not in _ref:
        _ref[key] = pick_ref.pick(mesh[0].numpy(), mesh[1].numpy(), mesh[2].numpy(), o.numpy(), d.numpy())
    return _ref[key]


def assert_equal(got, want, what):
    for k in pick_ref.FIELDS:
        g = got[k].cpu()
        assert g.dtype == (torch.int32 if k == "face" else torch.float32)
        w = torch.from_numpy(want[k])
        if not torch.equal(g, w):
            rows = torch.nonzero((g != w).reshape(g.shape[0], -1).any(dim=1)).flatten().tolist()
            i = rows[0]
            raise AssertionError(f"{what}: {k} differs for rays {rows[:16]}; ray {i}: got {g[i].tolist()!r} (face {int(got['face'][i])}), "
                                 f"want {w[i].tolist()!r} (face {int(want['face'][i])})")


def check(model, key, mesh, o, d):
    """ops.mesh_pick (records on the device) and model.pick (records on the host, the pick stream) both equal the restatement."""
    from diffusiontexturepainting_amd import ops
    o, d = torch.as_tensor(o, dtype=torch.float32).reshape(-1, 3), torch.as_tensor(d, dtype=torch.float32).reshape(-1, 3)
    want = reference(key, mesh, o, d)
    dm = model.load_mesh(*mesh)
    got = ops.mesh_pick(dm, o, d)
    assert got["face"].device.type == "cuda"
    assert_equal(got, want, key + " (op)")
    host = model.pick(dm, o, d)
    assert host["face"].device.type == "cpu"
    assert_equal(host, want, key + " (model.pick)")
    miss = want["face"] < 0
    for k in ("w", "pos", "normal", "uv", "t"):
        assert not want[k][miss].any()
    dm.close()
    return want


def test_one_face(model):
    mesh = first_faces(small_field(), 1)
    c = mesh[0][mesh[1][0].long()].mean(dim=0).tolist()
    o = [(c[0], c[1], 2), (c[0], c[1], -2), (0.5, 0.5, 2), (c[0] + 0.01, c[1] - 0.01, 1), (c[0], c[1], 2)]
    d = [DOWN, UP, DOWN, (0.02, -0.03, -1), UP]
    want = check(model, "one_face", mesh, o, d)
    assert want["face"].tolist() == [0, 0, -1, 0, -1]
    assert want["normal"][0, 2] > 0 and want["normal"][1, 2] < 0  # towards the ray's origin, from either side


def test_grid_shared_edges_and_vertices(model):
    mesh = grid_3x3()
    assert mesh[1].shape[0] == 18
    shared, border = grid_points()
    assert len(shared) == 4 + 12 + 9 and len(border) == 12
    pts = shared + border
    o = [(x, y, 2) for x, y in pts] + [(x, y, -2) for x, y in pts]
    d = [DOWN] * len(pts) + [UP] * len(pts)
    want = check(model, "grid", mesh, o, d)
    hit = want["face"] >= 0
    n = len(shared)
    assert hit[:n].all() and hit[len(pts):len(pts) + n].all()  # a shared edge or vertex always has an owner ...
    p = mesh[0][mesh[1].long()].numpy()
    lo, hi = mesh[0].numpy().min(axis=0).astype(np.float64), mesh[0].numpy().max(axis=0).astype(np.float64)
    for oi, di in zip(o[:n] + o[len(pts):len(pts) + n], d[:n] + d[len(pts):len(pts) + n]):
        assert len(pick_ref.candidates(p, lo, hi, oi, di)) == 1  # ... and only one (the mesh is a single sheet)
    got_xy = want["pos"][:n, :2]
    assert np.array_equal(got_xy, np.array(shared, dtype=f32))  # dyadic: the hit is the lattice point itself
    assert 0 < int(hit[n:len(pts)].sum()) < len(border)          # a border edge belongs to its face on two sides of the square only


def test_faces_257(model):
    mesh = first_faces(small_field(), 257)
    o, d = scatter(48, 5)
    o2, d2 = scatter(16, 6, z=-2.0)
    want = check(model, "faces_257", mesh, torch.cat([o, o2]), torch.cat([d, d2]))
    assert (want["face"] >= 0).sum() >= 20 and (want["face"] < 0).sum() >= 5 and want["face"].max() > 200


def test_big_height_field(model):
    o, d = field_rays()
    assert o.shape == (64, 3) and big_field()[1].shape[0] == 100352
    want = check(model, "big", big_field(), o, d)
    face = want["face"]
    assert (face[:16] >= 0).all() and (want["normal"][:16, 2] > 0).all() and np.array_equal(want["pos"][:16, :2] != 0, np.ones((16, 2), bool))
    assert (face[16:32] >= 0).sum() >= 8              # oblique: some leave over the border
    assert 0 < (face[32:48] >= 0).sum()                # grazing: some catch a bump, the frame is far from axis-aligned
    assert (face[48:56] < 0).all()                     # beside the box, or pointing away from it
    assert 0 < (face[56:] >= 0).sum() < 8              # from inside the z range: up or down, hit or miss
    hit = face >= 0
    assert (np.einsum("ij,ij->i", want["normal"][hit], d.numpy()[hit]) <= 0).all() and (want["t"][hit] >= 0).all()
    assert len(set(face[hit].tolist())) > 30 and face.max() > 50000


@pytest.mark.parametrize("n", [1, 256, 257])
def test_ray_counts(model, n):
    o, d = scatter(n, 100 + n)
    want = check(model, f"rays_{n}", small_field(), o, d)
    assert (want["face"] >= 0).any()


def test_both_windings_and_degenerate_faces(model):
    mesh = both_windings()
    o = [(-0.5, -0.6, 2), (0.5, -0.6, 2), (-0.8, 0.4, 2), (-0.5, -0.6, -2), (0.5, -0.6, -2), (0.5, 0.5, 2), (-0.4, -0.5, 2), (-0.75, 0.3, 2)]
    d = [DOWN, DOWN, DOWN, UP, UP, DOWN, DOWN, (-0.05, 0.1, -1)]
    want = check(model, "windings", mesh, o, d)
    assert want["face"][:5].tolist() == [0, 1, 2, 5, 1]      # either winding, from either side; the zero-area face 3 above face 0 never
    assert want["face"][6] == 0 and 3 not in want["face"].tolist()
    assert (want["normal"][[0, 1], 2] == 1).all() and (want["normal"][[3, 4], 2] == -1).all()


def test_winding_does_not_matter(model):
    """Picking has no flip option: the same surface with every face's winding reversed is hit by the same rays on the same faces, with
    the normal towards the ray's origin either way."""
    v, f, uv = small_field()
    o, d = scatter(64, 9)
    a = check(model, "winding_a", (v, f, uv), o, d)
    rev = [0, 2, 1]
    b = check(model, "winding_b", (v, f[:, rev].contiguous(), uv[:, rev].contiguous()), o, d)
    assert np.array_equal(a["face"], b["face"]) and (a["face"] >= 0).sum() > 30
    assert np.array_equal(np.sign(a["normal"][:, 2]), np.sign(b["normal"][:, 2]))
    assert np.abs(a["pos"] - b["pos"]).max() < 1e-5  # (the order of the corners changes the rounding, not the point)


# ---------------------------------------------------------------- from the pointer's rays to paint
ST = dict(steps=5, tg_steps=2, cfg_weight=2.5, context_pad=9)
RADIUS = 0.25
# a pointer path of 8 events over the big height field, the third off the mesh
PATH_O = [(-0.62, -0.3, 2.0), (-0.5, -0.22, 2.0), (2.5, 0.0, 2.0), (-0.2, -0.1, 2.0), (-0.12, -0.08, 2.0), (0.15, 0.05, 2.0), (0.45, 0.2, 2.0),
          (0.7, 0.3, 2.0)]
PATH_D = [(0.05, 0.02, -1.0)] * 8


def restated_path(origins, directions, state=None):
    v, f, uv = big_field()
    hits = pick_ref.pick(v.numpy(), f.numpy(), uv.numpy(), np.asarray(origins, dtype=f32), np.asarray(directions, dtype=f32))
    return pick_ref.plan_path(hits, f32(RADIUS / 1), state)


@pytest.fixture(scope="module")
def big_mesh(model):
    return model.load_mesh(*big_field())


@pytest.mark.parametrize("bleed", [0, 2])
def test_paint_mesh_path_equals_pick_plan_stroke(model, big_mesh, bleed):
    P, N, V, rst = restated_path(PATH_O, PATH_D)
    assert 4 <= P.shape[0] <= 6
    tex = torch.zeros(256, 256, 4, dtype=torch.uint8, device=DEV)
    out, state, n = model.paint_mesh_path(big_mesh, tex, PATH_O, PATH_D, RADIUS, seeds=900, bleed=bleed, **ST)
    assert out is tex and n == P.shape[0] and state == rst
    want = model.paint_mesh_stroke(big_mesh, torch.zeros_like(tex), torch.from_numpy(P), torch.from_numpy(N), torch.from_numpy(V), RADIUS,
                                   seeds=900, bleed=bleed, **ST)
    assert torch.equal(out, want)
    assert int((out.cpu() != 0).any(dim=-1).sum()) > 500
    _cache[("painted", bleed)] = out.cpu()


def test_paint_mesh_path_in_two_calls(model, big_mesh):
    whole = _cache.get(("painted", 0))
    if whole is None:
        whole = model.paint_mesh_path(big_mesh, torch.zeros(256, 256, 4, dtype=torch.uint8, device=DEV), PATH_O, PATH_D, RADIUS, seeds=900, **ST)[0].cpu()
    for cut in (4, 6):
        tex = torch.zeros(256, 256, 4, dtype=torch.uint8, device=DEV)
        _, state, n1 = model.paint_mesh_path(big_mesh, tex, PATH_O[:cut], PATH_D[:cut], RADIUS, seeds=900, **ST)
        _, state, n2 = model.paint_mesh_path(big_mesh, tex, PATH_O[cut:], PATH_D[cut:], RADIUS, seeds=900 + n1, state=state, **ST)
        assert n1 > 0 and n2 > 0 and state == restated_path(PATH_O, PATH_D)[3]
        assert torch.equal(tex.cpu(), whole)


def test_a_path_that_misses_paints_nothing(model, big_mesh):
    tex = torch.randint(0, 256, (256, 256, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(DEV)
    before = tex.clone()
    o = [(3.0 + 0.1 * i, 0.0, 2.0) for i in range(6)]
    out, state, n = model.paint_mesh_path(big_mesh, tex, o, [DOWN] * 6, RADIUS, seeds=1, bleed=2, **ST)
    torch.cuda.synchronize()
    assert n == 0 and state == dict(has_prev=False, prev=(0.0, 0.0, 0.0)) and torch.equal(out, before)
    # one hit only starts the path; the pointer has to move before anything is painted
    out, state, n = model.paint_mesh_path(big_mesh, tex, [(0.0, 0.0, 2.0), (0.01, 0.0, 2.0)], [DOWN] * 2, RADIUS, seeds=1, **ST)
    torch.cuda.synchronize()
    assert n == 0 and state["has_prev"] and torch.equal(out, before)


def test_pick_answers_while_a_stroke_is_queued(model):
    """The criterion of test_mesh_stroke_enqueue_does_not_block_the_host, for the pick's own stream: behind the 6-stamp stroke on the
    stroke's stream the pick would take the rest of the stroke's wall time, more than half of it."""
    from test_gpu_mesh import H, ST as ST4, STROKE, W, make_texture
    mesh = model.load_mesh(*small_field())
    tex = make_texture(H, W, 77).to(DEV)
    args = (STROKE["positions"] * 2, STROKE["normals"] * 2, STROKE["prevs"] * 2, STROKE["fov"] * 2)
    o, d = scatter(64, 31)
    want = reference("queued", small_field(), o, d)
    for _ in range(2):  # programs, graphs, the masks and the pick's buffers exist from here on
        model.paint_mesh_stroke(mesh, tex, *args, seeds=1, **ST4)
        model.pick(mesh, o, d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.paint_mesh_stroke(mesh, tex, *args, seeds=1, **ST4)
    t1 = time.perf_counter()
    got = model.pick(mesh, o, d)
    t_pick = time.perf_counter() - t1
    still_running = not model.stream.query()
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"6-stamp mesh stroke: enqueued in {(t1 - t0) * 1e3:.1f} ms, done after {t_all * 1e3:.1f} ms; a 64-ray pick behind it returned in "
          f"{t_pick * 1e3:.2f} ms (stroke still running: {still_running})")
    assert_equal(got, want, "queued")
    assert (want["face"] >= 0).sum() > 20
    assert t_pick < 0.5 * t_all


def test_refusals_leave_the_hits_and_the_texture_alone(model, big_mesh):
    from diffusiontexturepainting_amd import _lib, ops
    from diffusiontexturepainting_amd._lib import DtpError
    lib = _lib.load()
    mesh = model.load_mesh(*small_field())
    o, d = scatter(8, 77)
    host = torch.full((8, 13), 0x5a5a5a5a, dtype=torch.int32)
    dev = torch.full((8, 13), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    s = C.c_void_p(model.pick_stream.cuda_stream)

    def rays(o_, d_):
        t = torch.cat([torch.as_tensor(o_, dtype=torch.float32).reshape(-1, 3), torch.as_tensor(d_, dtype=torch.float32).reshape(-1, 3)], dim=1).contiguous()
        return t, C.cast(t.data_ptr(), C.POINTER(_lib.Ray))

    def refused(word, mesh_h, r, n):
        for fn, out in ((lib.dtp_mesh_pick, host), (lib.dtp_op_mesh_pick, dev)):
            assert fn(mesh_h, r, n, C.c_void_p(out.data_ptr()), s) == 1 and re.search(word, lib.dtp_last_error().decode()), lib.dtp_last_error()
        torch.cuda.synchronize()
        assert (host == 0x5a5a5a5a).all() and (dev.cpu() == 0x5a5a5a5a).all()

    keep, good = rays(o, d)
    refused(r"n=0 rays", mesh.handle, good, 0)
    refused(r"n=4097", mesh.handle, good, 4097)
    d_zero = d.clone()
    d_zero[3] = 0
    keep2, bad = rays(o, d_zero)
    refused(r"ray 3: the direction is zero", mesh.handle, bad, 8)
    d_nan = d.clone()
    d_nan[7, 1] = float("nan")
    keep3, bad = rays(o, d_nan)
    refused(r"ray 7: a non-finite direction", mesh.handle, bad, 8)
    o_inf = o.clone()
    o_inf[0, 2] = float("inf")
    keep4, bad = rays(o_inf, d)
    refused(r"ray 0: a non-finite origin", mesh.handle, bad, 8)
    refused(r"NULL", None, good, 8)
    dead = model.load_mesh(*first_faces(small_field(), 4))
    handle = dead.handle
    dead.close()
    refused(r"not a live mesh", handle, good, 8)
    # the Python surface; a refused path paints nothing
    with pytest.raises(DtpError, match=r"\(code 1\).*ray 3"):
        model.pick(mesh, o, d_zero)
    with pytest.raises(DtpError, match=r"\(code 1\).*ray 3"):
        ops.mesh_pick(mesh, o, d_zero)
    with pytest.raises(ValueError, match="load_mesh"):
        model.pick(None, o, d)
    with pytest.raises(ValueError, match="origins"):
        model.pick(mesh, o, d[:3])
    tex = torch.randint(0, 256, (256, 256, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(DEV)
    before = tex.clone()
    bad_d = [tuple(x) for x in PATH_D]
    bad_d[5] = (0.0, 0.0, 0.0)
    with pytest.raises(DtpError, match=r"ray 5"):
        model.paint_mesh_path(big_mesh, tex, PATH_O, bad_d, RADIUS, seeds=1, **ST)
    with pytest.raises(DtpError, match=r"stamp_distance"):
        model.paint_mesh_path(big_mesh, tex, PATH_O, PATH_D, 0.0, stamps_per_radius=1, fov=0.25, seeds=1, **ST)
    torch.cuda.synchronize()
    assert torch.equal(tex, before)
    # and the pick still works
    assert_equal(model.pick(mesh, o, d), reference("after_refusals", small_field(), o, d), "after the refusals")
