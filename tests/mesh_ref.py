"""Numpy restatement of the mesh strokes (dtp_mesh_stroke, csrc/mesh.hip) for the tests, written from the contract in include/dtp.h
operation for operation: the camera in double, rounded to fp32 once; projection and interpolation in fp32 with every operation rounded
once (numpy float32 arrays: no contraction); coverage in int64 on vertices snapped to 1/256 pixel with the top-left fill rule; the winner
of a pixel the largest (camera z, -face index).  What the Kit app does around it (manager.py:199-271, util/render.py:22-178) is the
frame: render -> stamp -> backproject.  Everything runs on the CPU."""
import numpy as np
import torch

f32 = np.float32
SNAP_MAX = float(1 << 26)
INPAINT, ERASE, OVERPAINT = 0, 1, 2


# ---------------------------------------------------------------- camera (host, double)
def camera(pos, normal, prev, fov):
    """-> float32 [3, 4]: rows (r, u, b) and t = -row . eye.  ValueError for what dtp_mesh_camera refuses."""
    pos, normal, prev = (np.asarray(v, dtype=f32).astype(np.float64) for v in (pos, normal, prev))
    fov = f32(fov)
    if not (np.isfinite(pos).all() and np.isfinite(normal).all() and np.isfinite(prev).all()):
        raise ValueError("non-finite")
    if not (fov > 0 and np.isfinite(fov)):
        raise ValueError("fov")
    eye, up = pos + normal, prev - pos
    b = eye - pos

    def norm(v):
        return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])

    def cross(a, c):
        return np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
    lb, lu = norm(b), norm(up)
    if not lb > 0:
        raise ValueError("normal is zero")
    b = b / lb
    r = cross(up, b)
    lr = norm(r)
    if not lu > 0 or not lr > 1e-9 * lu:
        raise ValueError("up is zero or parallel")
    r = r / lr
    u = cross(b, r)
    out = np.zeros((3, 4), dtype=f32)
    with np.errstate(over="ignore"):
        for k, row in enumerate((r, u, b)):
            out[k, :3] = row.astype(f32)
            out[k, 3] = f32(-((row[0] * eye[0] + row[1] * eye[1]) + row[2] * eye[2]))
    if not np.isfinite(out).all():
        raise ValueError("does not fit fp32")
    return out


# ---------------------------------------------------------------- shared arithmetic
def snap(t):
    return np.fmin(np.fmax(np.rint(t), f32(-SNAP_MAX)), f32(SNAP_MAX)).astype(np.int64)


def orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def cover(X, Y, px, py):
    """X, Y int64 [3]; px, py int64 arrays of centres -> (inside bool, weights float32 [..., 3])."""
    A = orient(X[0], Y[0], X[1], Y[1], X[2], Y[2])
    w = np.zeros(px.shape + (3,), dtype=f32)
    if A == 0:
        return np.zeros(px.shape, dtype=bool), w
    s = 1 if A > 0 else -1
    inside = np.ones(px.shape, dtype=bool)
    fa = f32(np.int64(s * A))
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        E = s * orient(X[a], Y[a], X[b], Y[b], px, py)
        dx, dy = s * (X[b] - X[a]), s * (Y[b] - Y[a])
        top_left = dy < 0 or (dy == 0 and dx > 0)
        inside &= (E > 0) | ((E == 0) & top_left)
        w[..., k] = E.astype(f32) / fa
    return inside, w


def interp(w, a0, a1, a2):
    return (w[..., 0] * f32(a0) + w[..., 1] * f32(a1)) + w[..., 2] * f32(a2)


def rasterize(X, Y, z, eligible, rows, cols):
    """X, Y int64 [F, 3], z float32 [F, 3], eligible bool [F] -> (face_idx int32 [rows, cols], weights float32 [rows, cols, 3]): per
    centre (256 j + 128, 256 i + 128) the covering eligible face with the largest (interpolated z, -index)."""
    py, px = np.meshgrid(np.arange(rows, dtype=np.int64) * 256 + 128, np.arange(cols, dtype=np.int64) * 256 + 128, indexing="ij")
    best = np.full((rows, cols), -1, dtype=np.int32)
    best_z = np.zeros((rows, cols), dtype=f32)
    best_w = np.zeros((rows, cols, 3), dtype=f32)
    for f in np.nonzero(eligible)[0]:
        # (only the centres inside the face's bounding box can be covered)
        j0, j1 = max(int((X[f].min() - 128 + 255) >> 8), 0), min(int((X[f].max() - 128) >> 8), cols - 1)
        i0, i1 = max(int((Y[f].min() - 128 + 255) >> 8), 0), min(int((Y[f].max() - 128) >> 8), rows - 1)
        if j0 > j1 or i0 > i1:
            continue
        sl = (slice(i0, i1 + 1), slice(j0, j1 + 1))
        inside, w = cover(X[f], Y[f], px[sl], py[sl])
        zi = interp(w, z[f, 0], z[f, 1], z[f, 2])
        take = inside & ((best[sl] < 0) | (zi > best_z[sl]) | ((zi == best_z[sl]) & (f < best[sl])))
        best[sl][take] = f
        best_z[sl][take] = zi[take]
        best_w[sl][take] = w[take]
    return best, best_w


def taps(x, y, Hs, Ws):
    x = np.fmin(np.fmax(x, f32(0)), f32(Ws - 1))
    y = np.fmin(np.fmax(y, f32(0)), f32(Hs - 1))
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    gx, gy = f32(1) - fx, f32(1) - fy
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
    return (x0, x1, y0, y1), (gx * gy, fx * gy, gx * fy, fx * fy)


def blend(img, tp):
    """img float32 [Hs, Ws, C] at the taps -> float32 [..., C]: ((v00 w00 + v01 w01) + v10 w10) + v11 w11."""
    (x0, x1, y0, y1), (w00, w01, w10, w11) = tp
    e = (lambda a: a[..., None])
    return ((img[y0, x0] * e(w00) + img[y0, x1] * e(w01)) + img[y1, x0] * e(w10)) + img[y1, x1] * e(w11)


# ---------------------------------------------------------------- the two halves of a stamp
def project(vertices, faces, cam, fov, R, flip_normals=False):
    v = np.asarray(vertices, dtype=f32)[np.asarray(faces, dtype=np.int64)]  # [F, 3, 3]
    cam, fov = np.asarray(cam, dtype=f32), f32(fov)
    with np.errstate(all="ignore"):
        c = np.stack([((cam[r, 0] * v[..., 0] + cam[r, 1] * v[..., 1]) + cam[r, 2] * v[..., 2]) + cam[r, 3] for r in range(3)], axis=-1)
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        nzu = nz / np.sqrt((nx * nx + ny * ny) + nz * nz)
        if flip_normals:
            nzu = -nzu
        raster = np.isfinite(c).all(axis=(1, 2)) & np.isfinite(nzu)
        ndc_x, ndc_y = c[..., 0] / fov, c[..., 1] / fov
        half = f32(128.0) * f32(R)
        X, Y = snap((ndc_x + f32(1)) * half), snap((f32(1) - ndc_y) * half)
        front, upright = raster & (nzu >= 0), raster & (nzu >= f32(0.5))
    return dict(X=X, Y=Y, z=c[..., 2].copy(), ndc_x=ndc_x, ndc_y=ndc_y, front=front, upright=upright, nzu=nzu)


def render(vertices, faces, face_uvs, cam, fov, texture, R, flip_normals=False, mode=INPAINT, over=(10, 25)):
    """-> (canvas torch f32 [1, 4, R, R], face_idx torch i32 [R, R], proj): texture u8 [H, W, 4] (torch or numpy)."""
    tex = np.asarray(texture.cpu() if isinstance(texture, torch.Tensor) else texture)
    H, W = tex.shape[:2]
    uvs = np.asarray(face_uvs, dtype=f32)
    proj = project(vertices, faces, cam, fov, R, flip_normals)
    face_idx, w = rasterize(proj["X"], proj["Y"], proj["z"], proj["front"], R, R)
    hit = face_idx >= 0
    fi = np.where(hit, face_idx, 0)
    u = (w[..., 0] * uvs[fi, 0, 0] + w[..., 1] * uvs[fi, 1, 0]) + w[..., 2] * uvs[fi, 2, 0]
    v = (w[..., 0] * uvs[fi, 0, 1] + w[..., 1] * uvs[fi, 1, 1]) + w[..., 2] * uvs[fi, 2, 1]
    texf = tex.astype(f32) / np.full(tex.shape, 255.0, dtype=f32)
    val = blend(texf, taps(u * f32(W) - f32(0.5), (f32(1) - v) * f32(H) - f32(0.5), H, W))
    val = np.where(hit[..., None], val, f32(0))
    if mode == OVERPAINT:
        val[over[0]:R - over[0], over[1]:R - over[1]] = 0
    canvas = torch.from_numpy(np.ascontiguousarray(val.transpose(2, 0, 1))[None])
    return canvas, torch.from_numpy(face_idx), proj


def finish_value(dec):
    dec = np.asarray(dec, dtype=f32)
    return np.fmin(np.fmax(dec / f32(2) + f32(0.5), f32(0)), f32(1))


def backproject(proj, face_idx, face_uvs, dec, mask, texture, painted=None):
    """The texture (u8 [H, W, 4], torch) after the backprojection, as a new tensor.  dec f32 [R, R, >= 3] (the decoder's output around
    -1..1), or painted f32 [3, R, R] in 0..1 (generate_raw's, used as it is); neither: erase.  mask u8 [R, R], face_idx / proj: the
    render's."""
    tex = texture.cpu().numpy().copy()
    H, W = tex.shape[:2]
    face_idx = np.asarray(face_idx)
    R = face_idx.shape[0]
    uvs = np.asarray(face_uvs, dtype=f32)
    F = uvs.shape[0]
    owned = np.zeros(F, dtype=bool)
    owned[face_idx[face_idx >= 0]] = True
    valid = proj["front"] & proj["upright"] & owned
    X = snap((uvs[..., 0] * f32(W)) * f32(256))
    Y = snap(((f32(1) - uvs[..., 1]) * f32(H)) * f32(256))
    tex_face, w = rasterize(X, Y, np.zeros((F, 3), dtype=f32), valid, H, W)
    hit = tex_face >= 0
    fi = np.where(hit, tex_face, 0)
    with np.errstate(all="ignore"):
        pf, qf = proj["ndc_x"] / f32(2) + f32(0.5), proj["ndc_y"] / f32(2) + f32(0.5)
        p = (w[..., 0] * pf[fi, 0] + w[..., 1] * pf[fi, 1]) + w[..., 2] * pf[fi, 2]
        q = (w[..., 0] * qf[fi, 0] + w[..., 1] * qf[fi, 1]) + w[..., 2] * qf[fi, 2]
        tp = taps(p * f32(R) - f32(0.5), (f32(1) - q) * f32(R) - f32(0.5), R, R)
    alpha = ((np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask) > 0) & (face_idx != -1)).astype(f32)
    img = np.zeros((R, R, 4), dtype=f32)
    img[..., 3] = alpha
    if dec is not None:
        img[..., :3] = finish_value(np.asarray(dec.cpu() if isinstance(dec, torch.Tensor) else dec)[..., :3])
    elif painted is not None:
        img[..., :3] = painted.detach().cpu().reshape(3, R, R).permute(1, 2, 0).numpy()
    erase = dec is None and painted is None
    val = blend(img, tp)
    write = hit & (val[..., 3] > 0)
    px = np.zeros((H, W, 4), dtype=np.uint8) if erase else (np.fmin(val, f32(1)) * f32(255.0)).astype(np.uint8)
    tex[write] = px[write]
    return torch.from_numpy(tex), dict(valid=valid, tex_face=tex_face, written=write)
