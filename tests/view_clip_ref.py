"""Numpy restatement of the near-plane clip of the view of a textured mesh (dtp_mesh_view_clip, dtp_op_mesh_view_clip; csrc/view.hip,
csrc/view_host.h) for the tests, written from the contract in include/dtp.h ("a view clipped at the near plane") operation for operation.
A face wholly in front of the near plane is view_ref's, untouched: its projection, its integer coverage, its q_k and d.  A face that
CROSSES the plane is rasterised in homogeneous form: per face the three cross products of its camera-space vertices and their determinant,
per pixel the edge functions of those against the pixel's ray, in fp32 with every operation rounded once (numpy float32 arrays: no
contraction).  The winner, the UV, the sample, the level of the pyramid and the colour are view_ref's and mip_ref's.  The pixel range of
a crossing face is no part of the contract (it only has to hold every covered centre; tools/view_clip_host_check.cpp checks that), so
this file covers the whole frame with each of them.  Everything runs on the CPU."""
import numpy as np

import mesh_ref
import mip_ref
import view_ref

f32 = np.float32


def camera_space(vertices, faces, cam):
    """-> float32 [F, 3, 3]: the camera-space vertices exactly as view_ref.project computes them."""
    v = np.asarray(vertices, dtype=f32)[np.asarray(faces, dtype=np.int64)]
    m = np.asarray(cam["m"], dtype=f32)
    with np.errstate(all="ignore"):
        return np.stack([((m[r, 0] * v[..., 0] + m[r, 1] * v[..., 1]) + m[r, 2] * v[..., 2]) + m[r, 3] for r in range(3)], axis=-1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=-1)


def classify(c, near):
    """c float32 [F, 3, 3] -> (front_of_plane, behind, crossing) bool [F]."""
    with np.errstate(all="ignore"):
        finite = np.isfinite(c).all(axis=(1, 2))
        ahead = c[..., 2] <= -f32(near)
    in_front = finite & ahead.all(axis=1)
    crossing = finite & ahead.any(axis=1) & ~ahead.all(axis=1)
    return in_front, ~(in_front | crossing), crossing


def project_crossing(vertices, faces, cam, cull=False, flip_normals=False):
    """Per face: crossing bool [F], n float32 [F, 3, 3] = sign(D) n_k, inv float32 [F] = 1 / |D|, D float32 [F], front, drawn bool [F]
    (drawn: crossing, D finite and not 0, not culled)."""
    c = camera_space(vertices, faces, cam)
    _, _, crossing = classify(c, cam["near"])
    with np.errstate(all="ignore"):
        c0, c1, c2 = c[:, 0], c[:, 1], c[:, 2]
        n0, n1, n2 = _cross(c1, c2), _cross(c2, c0), _cross(c0, c1)
        D = (c0[:, 0] * n0[:, 0] + c0[:, 1] * n0[:, 1]) + c0[:, 2] * n0[:, 2]
        neg = D < 0
        n = np.stack([n0, n1, n2], axis=1)
        n = np.where(neg[:, None, None], -n, n)
        inv = f32(1) / np.abs(D)
    front = neg != bool(flip_normals)
    drawn = crossing & np.isfinite(D) & (D != 0) & (front | (not cull))
    return dict(crossing=crossing, n=n, inv=inv, D=D, front=front, drawn=drawn, c=c)


def pixel_rays(cam, H, W, dx=0, dy=0):
    """-> (g_x float32 [W], g_y float32 [H]) of the centres of pixels (i + dy, j + dx): ndc_x = (2 j + 1) / W - 1, ndc_y = 1 - (2 i + 1) / H
    with the integers converted exactly, g = (ndc_x / fx, ndc_y / fy, -1)."""
    jx = (2 * (np.arange(W, dtype=np.int64) + dx) + 1).astype(f32)
    iy = (2 * (np.arange(H, dtype=np.int64) + dy) + 1).astype(f32)
    gx = (jx / f32(W) - f32(1)) / f32(cam["fx"])
    gy = (f32(1) - iy / f32(H)) / f32(cam["fy"])
    return gx, gy


def edge_q(n, inv, gx, gy):
    """n float32 [..., 3, 3], inv float32 [...] broadcast against gx, gy -> (E float32 [..., 3], q float32 [..., 3], d float32 [...])."""
    with np.errstate(all="ignore"):
        E = np.stack([(n[..., k, 0] * gx + n[..., k, 1] * gy) - n[..., k, 2] for k in range(3)], axis=-1)
        q = E * inv[..., None]
        d = (q[..., 0] + q[..., 1]) + q[..., 2]
    return E, q, d


def rasterize(proj, cr, cam, H, W):
    """view_ref.rasterize of the faces in front, then every drawn crossing face over the whole frame -> (face_idx, q, d, crossing winner
    bool [H, W])."""
    best, best_q, best_d = view_ref.rasterize(proj, H, W)
    gx, gy = pixel_rays(cam, H, W)
    gx, gy = np.broadcast_to(gx[None, :], (H, W)), np.broadcast_to(gy[:, None], (H, W))
    near = f32(cam["near"])
    is_cross = np.zeros((H, W), dtype=bool)
    for f in np.nonzero(cr["drawn"])[0]:
        E, q, d = edge_q(cr["n"][f], cr["inv"][f], gx, gy)
        with np.errstate(all="ignore"):
            inside = (E >= 0).all(axis=-1) & np.isfinite(d) & (d > 0)
            inside &= np.where(inside, f32(1) / np.where(inside, d, f32(1)), f32(0)) >= near
        take = inside & ((best < 0) | (d > best_d) | ((d == best_d) & (f < best)))
        best[take] = f
        best_d[take] = d[take]
        best_q[take] = q[take]
        is_cross[take] = True
    # (a face in front that takes a pixel from a crossing one cannot happen in this order: the crossing faces come last)
    return best, best_q, best_d, is_cross


def view(vertices, faces, face_uvs, texture, cam, size=None, cull=False, flip_normals=False, shade=True, ambient=0.25,
         unpainted=(128, 128, 128), background=(0, 0, 0, 0), clip_near=True, filter="bilinear", levels=None):
    """-> dict(image uint8 [H, W, 4], face_idx int32 [H, W], depth float32 [H, W], uv float32 [H, W, 2], lod float32 [H, W] (trilinear
    only), crossing bool [H, W], proj, cr).  clip_near=False: view_ref.view / mip_ref.view themselves."""
    opts = dict(size=size, cull=cull, flip_normals=flip_normals, shade=shade, ambient=ambient, unpainted=unpainted, background=background)
    trilinear = filter == "trilinear"
    if not clip_near:
        return mip_ref.view(vertices, faces, face_uvs, texture, cam, levels=levels, **opts) if trilinear else \
            view_ref.view(vertices, faces, face_uvs, texture, cam, **opts)
    H, W = cam["size"] if size is None else size
    tex = np.asarray(texture)
    lv = (mip_ref.pyramid(tex) if levels is None else levels) if trilinear else [np.ascontiguousarray(tex, dtype=np.uint8)]
    L = len(lv)
    TH, TW = lv[0].shape[:2]
    uvs = np.asarray(face_uvs, dtype=f32)
    proj = view_ref.project(vertices, faces, cam, H, W, cull, flip_normals)
    cr = project_crossing(vertices, faces, cam, cull, flip_normals)
    face_idx, q, d, is_cross = rasterize(proj, cr, cam, H, W)
    hit = face_idx >= 0
    fi = np.where(hit, face_idx, 0)
    U, V = (uvs[fi, 0, 0], uvs[fi, 1, 0], uvs[fi, 2, 0]), (uvs[fi, 0, 1], uvs[fi, 1, 1], uvs[fi, 2, 1])
    with np.errstate(all="ignore"):
        dd = np.where(hit, d, f32(1))
        u = mesh_ref.interp(q, *U) / dd
        v = mesh_ref.interp(q, *V) / dd
        level, f = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=f32)
        if trilinear:
            py, px = np.meshgrid(np.arange(H, dtype=np.int64) * 256 + 128, np.arange(W, dtype=np.int64) * 256 + 128, indexing="ij")
            X, Y, iw = proj["X"][fi], proj["Y"][fi], proj["iw"][fi]
            foot, ok = [], hit.copy()
            for ox, oy in ((1, 0), (0, 1)):
                qn = mip_ref.weights_at(X, Y, px + 256 * ox, py + 256 * oy) * iw
                gx, gy = pixel_rays(cam, H, W, ox, oy)
                _, qc, _ = edge_q(cr["n"][fi], cr["inv"][fi], np.broadcast_to(gx[None, :], (H, W)), np.broadcast_to(gy[:, None], (H, W)))
                qn = np.where(is_cross[..., None], qc, qn)
                dn = (qn[..., 0] + qn[..., 1]) + qn[..., 2]
                ok &= np.isfinite(dn) & (dn > 0)
                un, vn = mesh_ref.interp(qn, *U) / dn, mesh_ref.interp(qn, *V) / dn
                a, b = (un - u) * f32(TW), (vn - v) * f32(TH)
                foot.append(a * a + b * b)
            rho2 = np.fmax(foot[0], foot[1])
            rho2 = np.where(ok & np.isfinite(rho2), rho2, f32(np.inf)).astype(f32)
            rho2[~hit] = 0
            p4 = np.ones((H, W), dtype=f32)
            for k in range(1, L):
                step = (level == k - 1) & (p4 * f32(4) <= rho2)
                level[step] = k
                p4 = np.where(step, p4 * f32(4), p4)
            f = np.where((level == L - 1) | (rho2 <= p4), f32(0), ((rho2 / p4) - f32(1)) / f32(3)).astype(f32)
        lod = np.where(hit, level.astype(f32) + f, f32(0)).astype(f32)
        t = np.zeros((H, W, 4), dtype=f32)
        for k in range(L):
            here, above = hit & (level == k), hit & (level == k - 1) & (f > 0)
            if here.any() or above.any():
                tk = mip_ref.sample(lv[k], u, v)
                t[here] = tk[here]
                if above.any():
                    low = mip_ref.sample(lv[k - 1], u, v)
                    t[above] = (low + (tk - low) * f[..., None])[above]
        amb = f32(ambient)
        s = amb + (f32(1) - amb) * np.abs(proj["nzu"][fi]) if shade else np.ones((H, W), dtype=f32)
        unp = np.asarray(unpainted, dtype=np.uint8).astype(f32) / f32(255)
        ta = t[..., 3:4]
        c = (t[..., :3] * ta + unp * (f32(1) - ta)) * s[..., None]
        rgb = (np.fmin(c, f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)
        depth = np.where(hit, f32(1) / dd, f32(0)).astype(f32)
    image = np.empty((H, W, 4), dtype=np.uint8)
    image[..., :3] = rgb
    image[..., 3] = 255
    image[~hit] = np.asarray(background, dtype=np.uint8)
    out = dict(image=image, face_idx=face_idx, depth=depth, uv=np.stack([u, v], axis=-1), crossing=is_cross & hit, proj=proj, cr=cr,
               level=np.where(hit, level, -1))
    if trilinear:
        out["lod"] = lod
    return out


# ---------------------------------------------------------------- the cases the CPU and the GPU tests share
def floor_mesh():
    """A 20 x 20 floor quad at y = 0, two faces, counter-clockwise seen from above."""
    v = np.array([(-10, 0, -10), (10, 0, -10), (10, 0, 10), (-10, 0, 10)], dtype=f32)
    f = np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32)
    uv = np.array([[(0.05, 0.05), (0.95, 0.95), (0.95, 0.05)], [(0.05, 0.05), (0.05, 0.95), (0.95, 0.95)]], dtype=f32)
    return v, f, uv


def cube_mesh():
    """The cube [-0.5, 0.5]^3, 12 faces counter-clockwise seen from outside, each side a different patch of the texture."""
    v = [[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)]
    sides = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f, uv = [], []
    for s, (a, b, c, d) in enumerate(sides):
        u0, v0 = 0.05 + 0.3 * (s % 3), 0.05 + 0.45 * (s // 3)
        q = [(u0, v0), (u0 + 0.25, v0), (u0 + 0.25, v0 + 0.4), (u0, v0 + 0.4)]
        f += [[a, b, c], [a, c, d]]
        uv += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(v, dtype=f32), np.array(f, dtype=np.int32), np.array(uv, dtype=f32)


def mixed_mesh():
    """257 faces for the camera MIXED_POSE (at the origin, looking down -z, near 0.25): triangles of a seeded cloud in front of, behind and
    across the near plane, in both windings, then by hand a face of zero area, one whose plane contains the eye (D == 0), one with a vertex
    exactly on the near plane (in front), one with a vertex exactly on the eye plane, and a crossing one whose cross products overflow."""
    g = np.random.default_rng(257)
    n = 252
    centre = np.stack([g.uniform(-1.5, 1.5, n), g.uniform(-1.0, 1.0, n), g.uniform(-4.0, 1.0, n)], axis=1)
    tri = centre[:, None, :] + g.uniform(-0.6, 0.6, (n, 3, 3)) * np.array([1.0, 1.0, 1.5])
    hand = np.array([[(-0.5, -0.5, -2), (0.5, 0.5, -2), (0.5, 0.5, -2)],
                     [(1, 0, -2), (-1, 0, -2), (0, 0, 1)],
                     [(-1, -1, -0.25), (0, -1, -3), (-1, 0, -3)],
                     [(1, 1, 0), (0.2, 1, -3), (1, 0.2, -3)],
                     [(3e38, 3e38, -1), (-3e38, -3e38, -1), (3e38, -3e38, 1)]])
    v = np.concatenate([tri, hand]).astype(f32).reshape(-1, 3)
    f = np.arange(3 * (n + 5), dtype=np.int32).reshape(-1, 3)
    f[1::2] = f[1::2][:, [0, 2, 1]]  # every other face the other way round
    uv = g.uniform(0.02, 0.98, (n + 5, 3, 2)).astype(f32)
    return v, f, uv


# eye, at, up, fov_y, near
FLOOR_POSE = ((0, 1, 0), (0, 0.5, -3), (0, 1, 0), 45.0, 0.01)
FLOOR_UPSIDE_DOWN = ((0, 1, 0), (0, 0.5, -3), (0, -1, 0), 45.0, 0.01)     # the horizon lies BELOW the floor's pixels: their y neighbour
CUBE_INSIDE = ((0.4, -0.3, 0.1), (0.3, 0.5, -0.1), (0, 0, 1), 45.0, 0.05)  # a tenth of a unit from the wall x = 0.5, looking along it
FIELD_INSIDE = ((-0.2, 0.0, 0.45), (0.9, 0.1, 0.2), (0, 0, 1), 70.0, 0.2)  # make_height_field(17, 13, seed=3): faces across the plane
MIXED_POSE = ((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 0.25)
FIELD_LOW = ((-0.2, 0.0, 0.25), (0.9, 0.1, 0.2), (0, 0, 1), 70.0, 0.2)     # the same, lower: the crossing faces reach into the frame
# A strip of floor in the plane y = -1/64 from behind the eye (z = 1) to z = -64, seen from the origin down -z at 32 x 32, 45 degrees:
# with up = (0, -1, 0) the plane's horizon lies under the last row the strip covers, within that row's y neighbour.
RUNWAY = (np.array([(-1, -1 / 64, 1), (1, -1 / 64, 1), (1, -1 / 64, -64), (-1, -1 / 64, -64)], dtype=f32),
          np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32),
          np.array([[(0.1, 0.1), (0.9, 0.1), (0.9, 0.9)], [(0.1, 0.1), (0.9, 0.9), (0.1, 0.9)]], dtype=f32))
RUNWAY_POSE = ((0, 0, 0), (0, 0, -1), (0, -1, 0), 45.0, 0.05)
