"""Numpy restatement of the per-texel occlusion test of the mesh strokes' backprojection (include/dtp.h "occlusion in the
backprojection"; csrc/mesh.hip: the second instantiation of mesh_backproject_kernel) for the tests, written from the
contract operation for operation on top of mesh_ref: the tolerance in double rounded to fp32 once, the two faces' planes at a tap's
pixel centre by weights_at (the edge functions of the coverage with no inside test), one fp32 subtraction and comparison per tap, and
for a texel with a rejected tap the blend over the remaining taps divided by the sum of their weights.  Everything runs on the CPU."""
import numpy as np
import torch

import mesh_ref
from mesh_ref import f32


def tolerance(occlude, fov, R):
    """tol = occlude 2 fov / R in double from the fp32 occlude and fov, rounded to fp32 once.  ValueError for what the library refuses."""
    occlude, fov = f32(occlude), f32(fov)
    if not (np.isfinite(occlude) and occlude >= 0):
        raise ValueError("occlude")
    with np.errstate(over="ignore"):
        tol = f32(((float(occlude) * 2.0) * float(fov)) / float(R))
    if not np.isfinite(tol):
        raise ValueError("tol does not fit fp32")
    return tol


def weights_at(X, Y, px, py):
    """X, Y int64 [..., 3] (one triangle per point), px, py int64 [...] -> float32 [..., 3]: the sign-normalised edge functions of
    mesh_ref.cover over |A|, with no inside test (a weight is negative outside the triangle).  A zero area gives non-finite weights; the
    rule never asks for one."""
    A = mesh_ref.orient(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], X[..., 2], Y[..., 2])
    s = np.where(A > 0, 1, -1).astype(np.int64)
    w = np.zeros(px.shape + (3,), dtype=f32)
    with np.errstate(all="ignore"):
        fa = (s * A).astype(f32)
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            w[..., k] = (s * mesh_ref.orient(X[..., a], Y[..., a], X[..., b], Y[..., b], px, py)).astype(f32) / fa
    return w


def plane_z(proj, face, px, py):
    """The camera z of each face's plane at the points: face int64 [...], px, py int64 [...] -> float32 [...]."""
    w = weights_at(proj["X"][face], proj["Y"][face], px, py)
    z = proj["z"][face]
    with np.errstate(all="ignore"):
        return (w[..., 0] * z[..., 0] + w[..., 1] * z[..., 1]) + w[..., 2] * z[..., 2]


def backproject(proj, face_idx, face_uvs, dec, mask, texture, fov=None, occlude=None, painted=None, selected=None):
    """mesh_ref.backproject with the occlusion test: occlude None is mesh_ref.backproject itself; otherwise a tolerance in stamp pixels
    (with `fov`, the stamp's).  selected: a face set as bool [F] (select_ref.backproject's) or None.  -> (texture u8 [H, W, 4] as a new
    tensor, info): info as mesh_ref's plus rejected bool [H, W], the texels with one or more rejected taps, their number n_rejected,
    and n_unwritten, the texels the plain rule writes and this one does not."""
    if selected is not None:
        proj = dict(proj)
        proj["upright"] = proj["upright"] & np.asarray(selected, dtype=bool)
    if occlude is None:
        out, info = mesh_ref.backproject(proj, face_idx, face_uvs, dec, mask, texture, painted=painted)
        info = dict(info, rejected=np.zeros(info["written"].shape, dtype=bool), n_rejected=0, n_unwritten=0)
        return out, info
    tex = texture.cpu().numpy().copy()
    H, W = tex.shape[:2]
    face_idx = np.asarray(face_idx)
    R = face_idx.shape[0]
    tol = tolerance(occlude, fov, R)
    uvs = np.asarray(face_uvs, dtype=f32)
    F = uvs.shape[0]
    owned = np.zeros(F, dtype=bool)
    owned[face_idx[face_idx >= 0]] = True
    valid = proj["front"] & proj["upright"] & owned
    X = mesh_ref.snap((uvs[..., 0] * f32(W)) * f32(256))
    Y = mesh_ref.snap(((f32(1) - uvs[..., 1]) * f32(H)) * f32(256))
    tex_face, w = mesh_ref.rasterize(X, Y, np.zeros((F, 3), dtype=f32), valid, H, W)
    hit = tex_face >= 0
    fi = np.where(hit, tex_face, 0).astype(np.int64)
    with np.errstate(all="ignore"):
        pf, qf = proj["ndc_x"] / f32(2) + f32(0.5), proj["ndc_y"] / f32(2) + f32(0.5)
        p = (w[..., 0] * pf[fi, 0] + w[..., 1] * pf[fi, 1]) + w[..., 2] * pf[fi, 2]
        q = (w[..., 0] * qf[fi, 0] + w[..., 1] * qf[fi, 1]) + w[..., 2] * qf[fi, 2]
        tp = mesh_ref.taps(p * f32(R) - f32(0.5), (f32(1) - q) * f32(R) - f32(0.5), R, R)
    (x0, x1, y0, y1), wts = tp
    alpha = ((np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask) > 0) & (face_idx != -1)).astype(f32)
    img = np.zeros((R, R, 4), dtype=f32)
    img[..., 3] = alpha
    if dec is not None:
        img[..., :3] = mesh_ref.finish_value(np.asarray(dec.cpu() if isinstance(dec, torch.Tensor) else dec)[..., :3])
    elif painted is not None:
        img[..., :3] = painted.detach().cpu().reshape(3, R, R).permute(1, 2, 0).numpy()
    erase = dec is None and painted is None
    # ---- the test, per tap: the tap's winner g against the texel's face f, both planes at the tap's pixel centre
    rej = []
    for ty, tx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        g = face_idx[ty, tx].astype(np.int64)
        ask = hit & (g >= 0) & (g < F) & (g != fi)  # (-1, and a value that is no face of the mesh, is skipped)
        cx, cy = 256 * tx + 128, 256 * ty + 128
        zg = plane_z(proj, np.where(ask, g, 0), cx, cy)
        zf = plane_z(proj, fi, cx, cy)
        with np.errstate(all="ignore"):
            rej.append(ask & ((zg - zf) > tol))  # (a NaN compares false)
    rejected = rej[0] | rej[1] | rej[2] | rej[3]
    # ---- the texels without a rejected tap: the plain arithmetic
    with np.errstate(all="ignore"):
        plain = mesh_ref.blend(img, tp)
        plain_write = hit & (plain[..., 3] > 0)
        # ---- the others: a rejected tap's weight is 0, the blend is divided by the sum of the weights
        wz = [np.where(r, f32(0), wt) for r, wt in zip(rej, wts)]
        S = ((wz[0] + wz[1]) + wz[2]) + wz[3]
        val = mesh_ref.blend(img, ((x0, x1, y0, y1), tuple(wz))) / S[..., None]
        occ_write = hit & (S > 0) & (val[..., 3] > 0)
        val = np.where(rejected[..., None], val, plain)
        write = np.where(rejected, occ_write, plain_write)
        px = np.zeros((H, W, 4), dtype=np.uint8) if erase else (np.fmin(val, f32(1)) * f32(255.0)).astype(np.uint8)
    tex[write] = px[write]
    info = dict(valid=valid, tex_face=tex_face, written=write, rejected=rejected, n_rejected=int(rejected.sum()),
                n_unwritten=int((plain_write & ~write).sum()))
    return torch.from_numpy(tex), info


# ---------------------------------------------------------------- the table scene, from its geometry
def table_floor_behind_the_top(cam, fov, R, H, W):
    """synthetic.make_table_on_floor() seen through `cam` (mesh_ref.camera's [3, 4]) -> bool [H, W]: the floor chart's texels whose
    centre lies behind the table top by more than 1.5 stamp pixels from the top's rim -- from the geometry alone, in double: the texel's
    point on the floor, moved along the view direction up to the plane of the top, lies inside the top shrunk by that margin."""
    back = np.asarray(cam, dtype=np.float64)[2, :3]  # the camera looks down -back
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v = (j + 0.5) / W, 1.0 - (i + 0.5) / H
    x, y = 2.0 * (u - 0.02) / 0.46 - 1.0, 2.0 * (v - 0.02) / 0.96 - 1.0
    on_floor = (np.abs(x) <= 1.0) & (np.abs(y) <= 1.0)
    t = 0.5 / back[2]
    xt, yt = x + t * back[0], y + t * back[1]
    lim = 0.4 - 1.5 * (2.0 * fov / R)
    return on_floor & (np.abs(xt) < lim) & (np.abs(yt) < lim)
