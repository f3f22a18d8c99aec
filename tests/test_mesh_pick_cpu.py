"""The host-only part of picking on a mesh (include/dtp.h "picking on a mesh": dtp_mesh_ray_frame, dtp_mesh_path_plan, the argument
checks of dtp_mesh_pick / dtp_op_mesh_pick that come before any device call) against the numpy restatement (tests/pick_ref.py), and the
restatement itself against hand values chosen dyadic, so that every one of them is exact.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pick_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1  # DTP_ERR_ARG
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from diffusiontexturepainting_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# origin, direction
RAYS = {
    "down_minus_z": ((0.25, 0.5, 2), (0, 0, -1)),                   # d0 = d1 = 0: the helper is x (the lowest index of a tie)
    "up_plus_z_not_unit": ((1, 2, -3), (0, 0, 2.5)),
    "along_x": ((5, -1, 0.5), (1, 0, 0)),                           # d1 = d2 = 0: the helper is y
    "along_minus_y": ((0, 7, 0), (0, -3, 0)),
    "tie_of_two_small_components": ((0.3, 0.2, 0.1), (0.5, -0.5, 1)),    # |d0| = |d1|: x
    "tie_of_all_three": ((1, 1, 1), (-1, 1, -1)),
    "tie_of_the_last_two": ((1, 1, 1), (2, 1, -1)),                 # |d1| = |d2| < |d0|: y
    "oblique": ((0.3, -1.7, 2.9), (0.2, 0.5, -0.84)),
    "oblique_far_from_the_origin": ((1234.5, -987.25, 400.125), (-0.6, 0.1, 0.79)),
    "tiny_direction": ((0, 0, 1), (1e-30, -2e-30, -3e-30)),
}


@pytest.mark.parametrize("name", sorted(RAYS))
def test_ray_frame_equals_the_restatement(lib, name):
    from diffusiontexturepainting_amd.mesh import Mesh, ray_frame
    o, d = RAYS[name]
    got = ray_frame(o, d).numpy()
    want = pick_ref.ray_frame(o, d)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.array_equal(got, want), (got, want)
    assert torch.equal(Mesh.ray_frame(o, d), torch.from_numpy(want))
    # a rigid frame whose -z axis is the ray: the origin maps to 0, a point along the ray to (0, 0, -s)
    rot = got[:, :3].astype(np.float64)
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-6) and np.linalg.det(rot) > 0
    scale = max(1.0, float(np.abs(np.asarray(o)).max()))
    assert np.allclose(rot @ np.asarray(o, dtype=np.float64) + got[:, 3], 0, atol=2e-6 * scale)
    dn = np.asarray(d, dtype=np.float64) / np.linalg.norm(np.asarray(d, dtype=np.float64))
    assert np.allclose(rot @ dn, [0, 0, -1], atol=1e-6)


def test_ray_frames_by_hand(lib):
    from diffusiontexturepainting_amd.mesh import ray_frame
    assert torch.equal(ray_frame((1, 2, 3), (0, 0, -1)), torch.tensor([[0.0, -1, 0, 2], [1, 0, 0, -1], [0, 0, 1, -3]]))
    assert torch.equal(ray_frame((0, 0, 0), (4, 0, 0)), torch.tensor([[0.0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0]]))


@pytest.mark.parametrize("o,d,word", [
    ((0, 0, 0), (0, 0, 0), "direction is zero"),
    ((0, 0, 0), (float("nan"), 0, 1), "non-finite direction"),
    ((0, 0, 0), (0, float("inf"), 1), "non-finite direction"),
    ((0, float("nan"), 0), (0, 0, 1), "non-finite origin"),
    ((3e38, 3e38, 3e38), (1, 1, 1), "does not fit fp32"),
])
def test_ray_frame_refusals(lib, o, d, word):
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.mesh import ray_frame
    with pytest.raises(DtpError, match=rf"\(code {ARG}\).*{word}"):
        ray_frame(o, d)
    with pytest.raises(ValueError):
        pick_ref.ray_frame(o, d)
    out = (C.c_float * 12)(*([9.0] * 12))
    v = [(C.c_float * 3)(*x) for x in (o, d)]
    assert lib.dtp_mesh_ray_frame(C.byref(v[0]), C.byref(v[1]), C.byref(out)) == ARG
    assert list(out) == [9.0] * 12  # a refused call writes nothing
    assert lib.dtp_mesh_ray_frame(None, C.byref(v[1]), C.byref(out)) == ARG


@pytest.mark.parametrize("entry", ["dtp_mesh_pick", "dtp_op_mesh_pick"])
def test_pick_refuses_before_any_device_call(lib, entry):
    """No device here: every one of these returns from the checks.  The handle that is not a mesh is looked up, never followed."""
    from diffusiontexturepainting_amd import _lib
    fn = getattr(lib, entry)
    rays = (_lib.Ray * 2)(_lib.Ray((0, 0, 1), (0, 0, -1)), _lib.Ray((0, 0, 1), (0, 0, 0)))
    out = (C.c_int * 26)(*([7] * 26))
    not_a_mesh = (C.c_int * 64)()
    fake = C.cast(not_a_mesh, C.c_void_p)

    def refused(rc, word):
        assert rc == ARG and re.search(word, lib.dtp_last_error().decode()), (rc, lib.dtp_last_error())
        assert list(out) == [7] * 26

    refused(fn(None, rays, 1, C.cast(out, C.c_void_p), None), "NULL")
    refused(fn(fake, None, 1, C.cast(out, C.c_void_p), None), "NULL")
    refused(fn(fake, rays, 1, None, None), "NULL")
    refused(fn(fake, rays, 0, C.cast(out, C.c_void_p), None), r"n=0 rays \(1\.\.4096\)")
    refused(fn(fake, rays, 4097, C.cast(out, C.c_void_p), None), "n=4097")
    refused(fn(fake, rays, -1, C.cast(out, C.c_void_p), None), "n=-1")
    refused(fn(fake, rays, 2, C.cast(out, C.c_void_p), None), "not a live mesh")


def test_header_and_binding_agree_on_picking(lib):
    from diffusiontexturepainting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dtp.h")).read()
    assert re.search(r"#define\s+DTP_ABI_VERSION\s+3\b", hdr) and lib.dtp_abi_version() == 3
    assert "picking on a mesh" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dtp_[a-z0-9_]+)\s*\(", code))
    new = {"dtp_mesh_pick", "dtp_mesh_ray_frame", "dtp_mesh_path_plan", "dtp_op_mesh_pick"}
    assert new <= declared and declared == set(_lib.SYMBOLS)
    for name in new:
        assert hasattr(lib, name), f"libdtp.so does not export {name}"

    def fields(name):
        m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, code)
        return re.sub(r"\s+", " ", m.group(1)).strip()

    assert fields("dtp_ray") == "float origin[3], dir[3];"
    assert fields("dtp_mesh_hit") == "int face; float w[3], pos[3], normal[3], uv[2], t;"
    assert fields("dtp_path_state") == "int has_prev; float prev[3];"
    assert [f[0] for f in _lib.Ray._fields_] == ["origin", "dir"] and C.sizeof(_lib.Ray) == 24
    assert [f[0] for f in _lib.MeshHit._fields_] == ["face", "w", "pos", "normal", "uv", "t"]
    assert C.sizeof(_lib.MeshHit) == 52 and _lib.MeshHit.pos.offset == 16 and _lib.MeshHit.uv.offset == 40 and _lib.MeshHit.t.offset == 48
    assert [f[0] for f in _lib.PathState._fields_] == ["has_prev", "prev"] and C.sizeof(_lib.PathState) == 16
    from diffusiontexturepainting_amd import mesh
    assert mesh.HIT_WORDS * 4 == C.sizeof(_lib.MeshHit)


# ---------------------------------------------------------------- the restatement against hand values
def unit_quad(z=0.0):
    v = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], dtype=f32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    return v, f, v[f][..., :2].copy()


def n_candidates(v, f, o, d):
    return len(pick_ref.candidates(v[f], v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64), o, d))


def test_restatement_unit_quad_from_above_and_below():
    v, f, uv = unit_quad()
    pts = [(0.25, 0.5), (0.75, 0.25), (0.125, 0.875), (0.5, 0.25)]
    got = pick_ref.pick(v, f, uv, [(x, y, 2) for x, y in pts], [(0, 0, -1)] * 4)
    assert got["face"].tolist() == [1, 0, 1, 0]
    assert np.array_equal(got["pos"], np.array([(x, y, 0) for x, y in pts], dtype=f32))
    assert np.array_equal(got["uv"], np.array(pts, dtype=f32))
    assert np.array_equal(got["t"], np.full(4, 2, dtype=f32))
    assert np.array_equal(got["normal"], np.array([[0, 0, 1]] * 4, dtype=f32))
    assert np.array_equal(got["w"][0], np.array([0.5, 0.25, 0.25], dtype=f32)) and np.array_equal(got["w"].sum(axis=1), np.ones(4, dtype=f32))
    # from below, with a direction that is no unit vector: t counts in units of the normalised direction
    got = pick_ref.pick(v, f, uv, [(0.75, 0.25, -3)], [(0, 0, 2)])
    assert got["face"].tolist() == [0] and np.array_equal(got["pos"], np.array([[0.75, 0.25, 0]], dtype=f32))
    assert np.array_equal(got["normal"], np.array([[0, 0, -1]], dtype=f32)) and got["t"].tolist() == [3.0]


def test_restatement_shared_edges_and_vertices_have_one_owner():
    v, f, uv = unit_quad()
    for o, d in (((0.5, 0.5, 2), (0, 0, -1)), ((0.25, 0.25, 2), (0, 0, -1)), ((0.5, 0.5, -2), (0, 0, 1)), ((0.75, 0.75, -1), (0, 0, 4))):
        assert n_candidates(v, f, o, d) == 1  # on the shared diagonal
    # the two shared corners lie on the quad's border, which is no shared edge of a closed surface: one owner or none
    for corner in ((0, 0), (1, 1)):
        for o, d in (((*corner, 2), (0, 0, -1)), ((*corner, -2), (0, 0, 1))):
            assert n_candidates(v, f, o, d) <= 1
    # a 2 x 2 grid of quads: the centre vertex is shared by six faces, the edge midpoints by two or three; exactly one owns each
    xs = np.array([0, 0.5, 1], dtype=f32)
    gv = np.array([[x, y, 0] for y in xs for x in xs], dtype=f32)
    gf = []
    for j in range(2):
        for i in range(2):
            a, b, c, e = 3 * j + i, 3 * j + i + 1, 3 * j + i + 4, 3 * j + i + 3
            gf += [[a, b, c], [a, c, e]]
    gf = np.array(gf, dtype=np.int32)
    for x, y in ((0.5, 0.5), (0.5, 0.25), (0.25, 0.5), (0.75, 0.5), (0.5, 0.75), (0.25, 0.25), (0.75, 0.75)):
        for o, d in (((x, y, 1), (0, 0, -1)), ((x, y, -1), (0, 0, 1))):
            assert n_candidates(gv, gf, o, d) == 1, (x, y, d)
        # the same with the winding of every other face reversed
        mixed = gf.copy()
        mixed[::2] = mixed[::2, ::-1]
        assert n_candidates(gv, mixed, (x, y, 1), (0, 0, -1)) == 1


def test_restatement_misses_depth_order_ties_and_degenerate_faces():
    v, f, uv = unit_quad()
    # past the quad and pointing away; beside it; parallel to it
    got = pick_ref.pick(v, f, uv, [(0.5, 0.25, -1), (1.5, 0.5, 2), (0.5, 0.25, 1)], [(0, 0, -1), (0, 0, -1), (1, 0, 0)])
    assert got["face"].tolist() == [-1, -1, -1]
    for key in ("w", "pos", "normal", "uv", "t"):
        assert not got[key].any()
    # a ray that starts ON the surface hits it at t = 0
    got = pick_ref.pick(v, f, uv, [(0.5, 0.25, 0)], [(0, 0, -1)])
    assert got["face"].tolist() == [0] and got["t"].tolist() == [0.0]
    # two stacked quads: the nearer one wins, from either side, whatever the order of the faces
    lo_, hi_ = unit_quad(0.0), unit_quad(0.5)
    for first, second, hi_faces in ((lo_, hi_, (2, 3)), (hi_, lo_, (0, 1))):
        sv = np.concatenate([first[0], second[0]])
        sf = np.concatenate([first[1], second[1] + 4])
        suv = np.concatenate([first[2], second[2]])
        got = pick_ref.pick(sv, sf, suv, [(0.5, 0.25, 2), (0.5, 0.25, -2)], [(0, 0, -1), (0, 0, 1)])
        assert got["face"][0] in hi_faces and got["face"][1] not in hi_faces
        assert got["pos"][:, 2].tolist() == [0.5, 0.0] and got["t"].tolist() == [1.5, 2.0]
    # two coincident faces: the lower index
    cv = np.concatenate([v, v])
    cf = np.concatenate([f, f + 4])
    got = pick_ref.pick(cv, cf, np.concatenate([uv, uv]), [(0.5, 0.25, 2), (0.25, 0.5, 2)], [(0, 0, -1)] * 2)
    assert got["face"].tolist() == [0, 1]
    # a zero-area face on top of the quad is never hit, as first or as last face
    dv = np.concatenate([v, np.array([[0, 0, 1], [1, 1, 1], [1, 1, 1]], dtype=f32)])
    for df in (np.concatenate([f, [[4, 5, 6]]]), np.concatenate([[[4, 5, 6]], f])):
        duv = np.zeros((3, 3, 2), dtype=f32)
        got = pick_ref.pick(dv, df.astype(np.int32), duv, [(0.5, 0.5, 2), (0.25, 0.25, 2)], [(0, 0, -1)] * 2)
        assert (got["face"] >= 0).all() and (df[got["face"]] < 4).all()


def test_restatement_grid_exponent():
    fr = pick_ref.ray_frame((0, 0, 2), (0, 0, -1))
    assert pick_ref.exponent(fr, (0, 0, 0), (1, 1, 0)) == 25            # max = 1 = 0.5 * 2^1: 2^25 * 1 <= 2^25
    assert pick_ref.exponent(fr, (0, 0, 0), (1.5, 1, 0)) == 24
    assert pick_ref.exponent(fr, (-4, 0, 0), (1, 1, 0)) == 23
    assert pick_ref.exponent(fr, (0, 0, -5), (0, 0, 7)) == 64            # every corner on the ray
    assert pick_ref.exponent(fr, (0, 0, 0), (2.0 ** -60, 0, 0)) == 64    # clamped
    assert pick_ref.exponent(fr, (0, 0, 0), (2.0 ** 100, 0, 0)) == -64


# ---------------------------------------------------------------- the planner
def hits_of(rows):
    """rows: (x, y, z) or None for a miss; the normal of hit i is (i, 0, 1)."""
    face = np.array([-1 if r is None else 3 for r in rows], dtype=np.int32)
    pos = np.array([(0, 0, 0) if r is None else r for r in rows], dtype=f32)
    nrm = np.array([(i, 0, 1) for i in range(len(rows))], dtype=f32)
    return dict(face=face, pos=pos, normal=nrm)


def both(hits, sd, state=None):
    """The library's plan and the restatement's, which must be equal; -> the library's."""
    from diffusiontexturepainting_amd.mesh import plan_path
    P, N, V, st = plan_path({k: torch.from_numpy(v) for k, v in hits.items()}, sd, state)
    rP, rN, rV, rst = pick_ref.plan_path(hits, sd, state)
    assert np.array_equal(P.numpy(), rP) and np.array_equal(N.numpy(), rN) and np.array_equal(V.numpy(), rV) and st == rst
    return P.numpy(), N.numpy(), V.numpy(), st


def test_planner_hand_cases(lib):
    # the first hit gives no stamp
    P, N, V, st = both(hits_of([(1, 2, 3)]), 0.5)
    assert P.shape == (0, 3) and st == dict(has_prev=True, prev=(1.0, 2.0, 3.0))
    # dist = 2.5 x the stamp distance: 2 stamps 1.25 x the distance apart, the hit's normal, a chained prev
    P, N, V, st = both(hits_of([(0, 0, 0), (5, 0, 0)]), 2.0)
    assert P.tolist() == [[2.5, 0, 0], [5, 0, 0]] and V.tolist() == [[0, 0, 0], [2.5, 0, 0]] and N.tolist() == [[1, 0, 1]] * 2
    assert st == dict(has_prev=True, prev=(5.0, 0.0, 0.0))
    # too near: nothing changes, the previous hit stays; exactly the distance: one stamp
    P, _, _, st = both(hits_of([(0, 0, 0), (0, 0.75, 0)]), 1.0)
    assert P.shape == (0, 3) and st["prev"] == (0.0, 0.0, 0.0)
    P, _, V, st = both(hits_of([(0, 0, 0), (0, 0.75, 0), (0, 1, 0)]), 1.0)
    assert P.tolist() == [[0, 1, 0]] and V.tolist() == [[0, 0, 0]]
    # a miss in the middle leaves the state alone
    a = both(hits_of([(0, 0, 0), None, (0, 0, 3)]), 1.0)
    b = both(hits_of([(0, 0, 0), (0, 0, 3)]), 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[0].shape == (3, 3)
    assert a[1].tolist() == [[2, 0, 1]] * 3 and b[1].tolist() == [[1, 0, 1]] * 3
    _, _, _, st = both(hits_of([None, None]), 1.0)
    assert st == dict(has_prev=False, prev=(0.0, 0.0, 0.0))
    # an oblique path with inexact steps: the restatement decides (inside both())
    rows = [(0.1, 0.2, 0.3), (0.9, -0.4, 0.35), None, (0.95, -0.38, 0.3), (-0.7, 0.6, 0.1), (-0.7, 0.6, 0.1), (0.3, 0.3, 0.3)]
    whole = both(hits_of(rows), 0.23)
    assert whole[0].shape[0] > 10
    # the same path in two calls that carry the state
    for cut in (1, 2, 3, 5):
        h = hits_of(rows)
        first = both({k: v[:cut] for k, v in h.items()}, 0.23)
        second = both({k: v[cut:] for k, v in h.items()}, 0.23, first[3])
        for k in range(3):
            assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k])
        assert second[3] == whole[3]


def test_planner_capacity_and_refusals(lib):
    from diffusiontexturepainting_amd import _lib
    from diffusiontexturepainting_amd._lib import DtpError
    from diffusiontexturepainting_amd.mesh import _hit_records, plan_path
    rec = _hit_records({k: torch.from_numpy(v) for k, v in hits_of([(0, 0, 0), (5, 0, 0), (5, 3, 0)]).items()})
    want = pick_ref.plan_path(hits_of([(0, 0, 0), (5, 0, 0), (5, 3, 0)]), 1.0)
    assert want[0].shape[0] == 8
    st = _lib.PathState(0, (0, 0, 0))
    bufs = [torch.full((8, 3), 9.0) for _ in range(3)]
    count = C.c_int(-1)

    def args(cap):
        return (C.c_void_p(rec.data_ptr()), 3, C.c_float(1.0), C.byref(st), *[C.c_void_p(b.data_ptr()) for b in bufs], cap, C.byref(count))
    # too small: the count that is needed, the state unchanged
    assert lib.dtp_mesh_path_plan(*args(7)) == ARG and count.value == 8 and b"capacity 7" in lib.dtp_last_error()
    assert st.has_prev == 0 and tuple(st.prev) == (0.0, 0.0, 0.0)
    assert float(bufs[0][7, 0]) == 9.0  # nothing beyond the capacity is written
    with pytest.raises(ValueError, match="count 8"):
        pick_ref.plan_path(hits_of([(0, 0, 0), (5, 0, 0), (5, 3, 0)]), 1.0, cap=7)
    assert lib.dtp_mesh_path_plan(*args(8)) == 0 and count.value == 8
    assert st.has_prev == 1 and tuple(st.prev) == (5.0, 3.0, 0.0)
    for b, w in zip(bufs, want[:3]):
        assert np.array_equal(b.numpy(), w)
    # refusals: the state and the count stay
    st2 = _lib.PathState(1, (1, 1, 1))
    count.value = -7
    for sd in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dtp_mesh_path_plan(C.c_void_p(rec.data_ptr()), 3, C.c_float(sd), C.byref(st2), None, None, None, 0, C.byref(count)) == ARG
        assert b"stamp_distance" in lib.dtp_last_error()
        with pytest.raises(ValueError):
            pick_ref.plan_path(hits_of([(0, 0, 0)]), sd)
    assert lib.dtp_mesh_path_plan(C.c_void_p(rec.data_ptr()), 3, C.c_float(1e-9), C.byref(st2), None, None, None, 0, C.byref(count)) == ARG
    assert b"chord" in lib.dtp_last_error()
    assert lib.dtp_mesh_path_plan(None, 3, C.c_float(1.0), C.byref(st2), None, None, None, 0, C.byref(count)) == ARG
    assert lib.dtp_mesh_path_plan(C.c_void_p(rec.data_ptr()), 3, C.c_float(1.0), None, None, None, None, 0, C.byref(count)) == ARG
    assert lib.dtp_mesh_path_plan(C.c_void_p(rec.data_ptr()), 3, C.c_float(1.0), C.byref(st2), None, None, None, 0, None) == ARG
    assert lib.dtp_mesh_path_plan(C.c_void_p(rec.data_ptr()), 3, C.c_float(1.0), C.byref(st2), None, None, None, 4, C.byref(count)) == ARG
    assert lib.dtp_mesh_path_plan(C.c_void_p(rec.data_ptr()), -1, C.c_float(1.0), C.byref(st2), None, None, None, 0, C.byref(count)) == ARG
    assert count.value == -7 and st2.has_prev == 1 and tuple(st2.prev) == (1.0, 1.0, 1.0)
    with pytest.raises(DtpError, match="stamp_distance"):
        plan_path(dict(face=torch.tensor([0]), pos=torch.zeros(1, 3), normal=torch.zeros(1, 3)), 0.0)
