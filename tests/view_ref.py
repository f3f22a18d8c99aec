"""Numpy restatement of the view of a textured mesh (dtp_view_camera, dtp_view_rays, dtp_mesh_view; csrc/view.hip, csrc/view_host.h) for
the tests, written from the contract in include/dtp.h ("a view of a textured mesh") operation for operation: the camera and the rays in
double, rounded to fp32 once; the projection, the inverse depth, the perspective-correct UV and the colour in fp32 with every operation
rounded once (numpy float32 arrays: no contraction); coverage, interpolation, taps and blend are the strokes' own (mesh_ref.snap / cover /
interp / taps / blend).  The winner of a pixel is the largest (inverse depth, -face index).  Everything runs on the CPU."""
import math

import numpy as np

import mesh_ref

f32 = np.float32
VIEW_MAX = 4096


# ---------------------------------------------------------------- host, double
def _cam_ok(m, fx, fy, near):
    with np.errstate(all="ignore"):
        return bool(np.isfinite(m).all() and np.isfinite(fx) and np.isfinite(fy) and fx > 0 and fy > 0 and np.isfinite(near) and near > 0
                    and np.isfinite(f32(1) / f32(near)))


def camera(eye, at, up, fov_y=45.0, size=(720, 1280), near=0.01):
    """-> dict(m float32 [3, 4], fx, fy, near float32, size).  ValueError for what dtp_view_camera refuses."""
    H, W = int(size[0]), int(size[1])
    eye, at, up = (np.asarray(v, dtype=f32).astype(np.float64) for v in (eye, at, up))
    fov, near = f32(fov_y), f32(near)
    if not (np.isfinite(eye).all() and np.isfinite(at).all() and np.isfinite(up).all()):
        raise ValueError("non-finite")
    if not (np.isfinite(fov) and 0 < fov < 180):
        raise ValueError("fov_y")
    if not (np.isfinite(near) and near > 0):
        raise ValueError("near")
    if not (1 <= H <= VIEW_MAX and 1 <= W <= VIEW_MAX):
        raise ValueError("size")

    def norm(v):
        return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])

    def cross(a, c):
        return np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
    b = eye - at
    lb, lu = norm(b), norm(up)
    if not lb > 0:
        raise ValueError("eye == at")
    b = b / lb
    r = cross(up, b)
    lr = norm(r)
    if not lu > 0 or not lr > 1e-9 * lu:
        raise ValueError("up is zero or parallel")
    r = r / lr
    u = cross(b, r)
    m = np.zeros((3, 4), dtype=f32)
    with np.errstate(over="ignore"):
        for k, row in enumerate((r, u, b)):
            m[k, :3] = row.astype(f32)
            m[k, 3] = f32(-((row[0] * eye[0] + row[1] * eye[1]) + row[2] * eye[2]))
        fy = 1.0 / math.tan((float(fov) * math.pi) / 360.0)
        fx = (fy * float(H)) / float(W)
        fx, fy = f32(fx), f32(fy)
    if not _cam_ok(m, fx, fy, near):
        raise ValueError("does not fit fp32")
    return dict(m=m, fx=fx, fy=fy, near=near, size=(H, W))


def rays(cam, pixels, size=None):
    """-> (origins float32 [n, 3], directions float32 [n, 3]) of pixel positions (x, y).  ValueError for what dtp_view_rays refuses."""
    H, W = cam["size"] if size is None else size
    xy = np.asarray(pixels, dtype=f32).reshape(-1, 2).astype(np.float64)
    if not _cam_ok(cam["m"], cam["fx"], cam["fy"], cam["near"]) or not (1 <= H <= VIEW_MAX and 1 <= W <= VIEW_MAX) or xy.shape[0] < 1:
        raise ValueError("camera, size or n")
    if not np.isfinite(xy).all():
        raise ValueError("non-finite pixel")
    m = np.asarray(cam["m"], dtype=f32).astype(np.float64)
    with np.errstate(over="ignore"):
        eye = np.array([-((m[0, i] * m[0, 3] + m[1, i] * m[1, 3]) + m[2, i] * m[2, 3]) for i in range(3)]).astype(f32)
    if not np.isfinite(eye).all():
        raise ValueError("the eye does not fit fp32")
    fx, fy = float(cam["fx"]), float(cam["fy"])
    nx = (2.0 * xy[:, 0]) / float(W) - 1.0
    ny = 1.0 - (2.0 * xy[:, 1]) / float(H)
    a, c = nx / fx, ny / fy
    d = np.stack([(m[0, i] * a + m[1, i] * c) - m[2, i] for i in range(3)], axis=1).astype(f32)
    return np.broadcast_to(eye, d.shape).copy(), d


# ---------------------------------------------------------------- the device's part, fp32
def project(vertices, faces, cam, H, W, cull=False, flip_normals=False):
    """Per face: X, Y int64 [F, 3], iw float32 [F, 3], nzu float32 [F], A int64 [F], front, drawn bool [F] (drawn: in front of the near
    plane with finite coordinates, a non-zero snapped area, and not culled; whether a pixel centre lies in its box is the raster's)."""
    v = np.asarray(vertices, dtype=f32)[np.asarray(faces, dtype=np.int64)]  # [F, 3, 3]
    m, fx, fy, near = np.asarray(cam["m"], dtype=f32), f32(cam["fx"]), f32(cam["fy"]), f32(cam["near"])
    with np.errstate(all="ignore"):
        c = np.stack([((m[r, 0] * v[..., 0] + m[r, 1] * v[..., 1]) + m[r, 2] * v[..., 2]) + m[r, 3] for r in range(3)], axis=-1)
        ahead = np.isfinite(c).all(axis=(1, 2)) & (c[..., 2] <= -near).all(axis=1)
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        nzu = nz / np.sqrt((nx * nx + ny * ny) + nz * nz)
        iw = f32(1) / (f32(0) - c[..., 2])
        X = mesh_ref.snap((((c[..., 0] * fx) * iw) + f32(1)) * (f32(128) * f32(W)))
        Y = mesh_ref.snap((f32(1) - ((c[..., 1] * fy) * iw)) * (f32(128) * f32(H)))
    X[~ahead], Y[~ahead] = 0, 0
    A = mesh_ref.orient(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    front = (A < 0) != bool(flip_normals)
    drawn = ahead & (A != 0) & (front | (not cull))
    return dict(X=X, Y=Y, iw=iw, nzu=nzu, A=A, front=front, drawn=drawn, z=c[..., 2].copy())


def rasterize(proj, H, W):
    """-> (face_idx int32 [H, W], q float32 [H, W, 3] = w_k iw_k of the winner, d float32 [H, W] = (q0 + q1) + q2): per centre
    (256 j + 128, 256 i + 128) the covering drawn face with the largest (d, -index)."""
    X, Y, iw = proj["X"], proj["Y"], proj["iw"]
    py, px = np.meshgrid(np.arange(H, dtype=np.int64) * 256 + 128, np.arange(W, dtype=np.int64) * 256 + 128, indexing="ij")
    best = np.full((H, W), -1, dtype=np.int32)
    best_d = np.zeros((H, W), dtype=f32)
    best_q = np.zeros((H, W, 3), dtype=f32)
    j0 = np.maximum((X.min(axis=1) - 128 + 255) >> 8, 0)
    j1 = np.minimum((X.max(axis=1) - 128) >> 8, W - 1)
    i0 = np.maximum((Y.min(axis=1) - 128 + 255) >> 8, 0)
    i1 = np.minimum((Y.max(axis=1) - 128) >> 8, H - 1)
    for f in np.nonzero(proj["drawn"] & (j0 <= j1) & (i0 <= i1))[0]:
        sl = (slice(int(i0[f]), int(i1[f]) + 1), slice(int(j0[f]), int(j1[f]) + 1))
        inside, w = mesh_ref.cover(X[f], Y[f], px[sl], py[sl])
        if not inside.any():
            continue
        q = w * iw[f]
        d = (q[..., 0] + q[..., 1]) + q[..., 2]
        take = inside & ((best[sl] < 0) | (d > best_d[sl]) | ((d == best_d[sl]) & (f < best[sl])))
        best[sl][take] = f
        best_d[sl][take] = d[take]
        best_q[sl][take] = q[take]
    return best, best_q, best_d


def view(vertices, faces, face_uvs, texture, cam, size=None, cull=False, flip_normals=False, shade=True, ambient=0.25,
         unpainted=(128, 128, 128), background=(0, 0, 0, 0)):
    """-> dict(image uint8 [H, W, 4], face_idx int32 [H, W], depth float32 [H, W], uv float32 [H, W, 2], proj).  texture uint8
    [TH, TW, 4] (numpy, or anything np.asarray takes)."""
    H, W = cam["size"] if size is None else size
    tex = np.asarray(texture)
    TH, TW = tex.shape[:2]
    uvs = np.asarray(face_uvs, dtype=f32)
    proj = project(vertices, faces, cam, H, W, cull, flip_normals)
    face_idx, q, d = rasterize(proj, H, W)
    hit = face_idx >= 0
    fi = np.where(hit, face_idx, 0)
    with np.errstate(all="ignore"):
        dd = np.where(hit, d, f32(1))
        u = mesh_ref.interp(q, uvs[fi, 0, 0], uvs[fi, 1, 0], uvs[fi, 2, 0]) / dd
        v = mesh_ref.interp(q, uvs[fi, 0, 1], uvs[fi, 1, 1], uvs[fi, 2, 1]) / dd
        texf = tex.astype(f32) / np.full(tex.shape, 255.0, dtype=f32)
        t = mesh_ref.blend(texf, mesh_ref.taps(u * f32(TW) - f32(0.5), (f32(1) - v) * f32(TH) - f32(0.5), TH, TW))  # [H, W, 4]
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
    return dict(image=image, face_idx=face_idx, depth=depth, uv=np.stack([u, v], axis=-1), proj=proj)
