"""Numpy restatement of the bleed pass of the mesh strokes (dtp_mesh_stroke_bleed, dtp_mesh_bleed, dtp_op_mesh_coverage; csrc/mesh_bleed.hip,
DESIGN.md 3.21) for the tests, written from the contract in include/dtp.h: coverage of a texture by ALL faces of a mesh through
mesh_ref.snap / mesh_ref.rasterize, the texel rectangle of a stamp, the order of the candidate offsets, and the pass by brute force.
Everything is integer arithmetic and runs on the CPU."""
import numpy as np
import torch

import mesh_ref

f32 = np.float32
MAX_RADIUS = 16


# ---------------------------------------------------------------- the offset order
def offsets(k):
    """int8 [n, 2]: every (di, dj) with 0 < di^2 + dj^2 <= k^2, sorted by (di^2 + dj^2, di, dj)."""
    if not 1 <= k <= MAX_RADIUS:
        raise ValueError("radius")
    cand = [(di * di + dj * dj, di, dj) for di in range(-k, k + 1) for dj in range(-k, k + 1) if 0 < di * di + dj * dj <= k * k]
    return np.array([(di, dj) for _, di, dj in sorted(cand)], dtype=np.int8)


# ---------------------------------------------------------------- coverage
def snap_uvs(face_uvs, H, W):
    """-> X, Y int64 [F, 3]: the backprojection's texture-space positions, snapped to 1/256 texel."""
    uvs = np.asarray(face_uvs, dtype=f32)
    return mesh_ref.snap((uvs[..., 0] * f32(W)) * f32(256)), mesh_ref.snap(((f32(1) - uvs[..., 1]) * f32(H)) * f32(256))


def coverage(face_uvs, H, W):
    """bool [H, W]: the texel centres that at least one of all F faces covers (mesh_ref.rasterize: a winner exists)."""
    X, Y = snap_uvs(face_uvs, H, W)
    F = X.shape[0]
    tex_face, _ = mesh_ref.rasterize(X, Y, np.zeros((F, 3), dtype=f32), np.ones(F, dtype=bool), H, W)
    return tex_face >= 0


def centre_range(a, b, n):
    """The texel indices 0 .. n - 1 whose centres 256 i + 128 lie in [a, b] (arrays): lo, hi; empty where lo > hi."""
    return np.maximum((a - 128 + 255) >> 8, 0), np.minimum((b - 128) >> 8, n - 1)


def coverage_batched(face_uvs, H, W, budget=1 << 22):
    """coverage() for meshes of many faces: the same integer rule (mesh_ref.cover's expressions on arrays of faces), evaluated for
    batches of faces over their own texel boxes at once.  tests/test_mesh_bleed_cpu.py holds it equal to coverage()."""
    X, Y = snap_uvs(face_uvs, H, W)
    A = mesh_ref.orient(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    x0, x1 = centre_range(X.min(axis=1), X.max(axis=1), W)
    y0, y1 = centre_range(Y.min(axis=1), Y.max(axis=1), H)
    keep = np.nonzero((A != 0) & (x0 <= x1) & (y0 <= y1))[0]
    # faces grouped by their box rounded up to powers of two: every batch is one padded [n, mh, mw] block within the budget
    pw = np.ceil(np.log2((x1 - x0 + 1)[keep])).astype(np.int64)
    ph = np.ceil(np.log2((y1 - y0 + 1)[keep])).astype(np.int64)
    cov = np.zeros(H * W, dtype=bool)
    batches = []
    for key in np.unique(ph * 64 + pw):
        group = keep[ph * 64 + pw == key]
        step = max(1, budget >> int((key >> 6) + (key & 63)))
        batches += [group[i:i + step] for i in range(0, len(group), step)]
    for f in batches:
        mw, mh = int((x1 - x0 + 1)[f].max()), int((y1 - y0 + 1)[f].max())
        col = x0[f][:, None, None] + np.arange(mw, dtype=np.int64)[None, None, :]
        row = y0[f][:, None, None] + np.arange(mh, dtype=np.int64)[None, :, None]
        inside = (col <= x1[f][:, None, None]) & (row <= y1[f][:, None, None])
        px, py = col * 256 + 128, row * 256 + 128
        s = np.where(A[f] > 0, 1, -1).astype(np.int64)[:, None, None]
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            Xa, Ya, Xb, Yb = (v[f][:, None, None] for v in (X[:, a], Y[:, a], X[:, b], Y[:, b]))
            E = s * mesh_ref.orient(Xa, Ya, Xb, Yb, px, py)
            dx, dy = s * (Xb - Xa), s * (Yb - Ya)
            top_left = (dy < 0) | ((dy == 0) & (dx > 0))
            inside = inside & ((E > 0) | ((E == 0) & top_left))
        flat = (row * W + col)
        cov[np.broadcast_to(flat, inside.shape)[inside]] = True
    return cov.reshape(H, W)


# ---------------------------------------------------------------- the rectangle of a stamp
def stamp_rect(proj, face_idx, face_uvs, H, W, k):
    """(x0, y0, x1, y1) inclusive, or None: the union of the texel ranges of the valid faces of a render (front, not steep, the winner
    of a pixel, a non-zero area in texture space and a texel centre in their box) grown by k and clipped to the texture."""
    face_idx = np.asarray(face_idx.cpu() if isinstance(face_idx, torch.Tensor) else face_idx)
    F = np.asarray(face_uvs).shape[0]
    owned = np.zeros(F, dtype=bool)
    owned[face_idx[face_idx >= 0]] = True
    X, Y = snap_uvs(face_uvs, H, W)
    A = mesh_ref.orient(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    x0, x1 = centre_range(X.min(axis=1), X.max(axis=1), W)
    y0, y1 = centre_range(Y.min(axis=1), Y.max(axis=1), H)
    valid = proj["front"] & proj["upright"] & owned & (A != 0) & (x0 <= x1) & (y0 <= y1)
    if not valid.any():
        return None
    return (max(int(x0[valid].min()) - k, 0), max(int(y0[valid].min()) - k, 0),
            min(int(x1[valid].max()) + k, W - 1), min(int(y1[valid].max()) + k, H - 1))


# ---------------------------------------------------------------- the pass
def source(cov, k, rect=None):
    """-> (has bool [H, W], si int64 [H, W], sj int64 [H, W]): per uncovered texel of the rectangle (None: the whole texture) whether it
    has a source, and the source's row and column: the covered texel inside the texture at the first offset of offsets(k)."""
    cov = np.asarray(cov, dtype=bool)
    H, W = cov.shape
    todo = ~cov
    if rect is not None:
        x0, y0, x1, y1 = rect
        inside = np.zeros((H, W), dtype=bool)
        inside[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = True
        todo &= inside
    ii, jj = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    has = np.zeros((H, W), dtype=bool)
    si, sj = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    for di, dj in offsets(k).astype(np.int64):
        i, j = ii + di, jj + dj
        ok = (i >= 0) & (i < H) & (j >= 0) & (j < W)
        take = todo & ok & cov[np.clip(i, 0, H - 1), np.clip(j, 0, W - 1)]
        has |= take
        si[take], sj[take] = i[take], j[take]
        todo &= ~take
    return has, si, sj


def bleed(texture, cov, k, rect=None):
    """The texture (u8 [H, W, 4], torch) after the pass, as a new tensor: every uncovered texel of the rectangle that has a source gets
    the four bytes of its source.  Sources are covered texels, which the pass never writes: reading the input is reading the output."""
    tex = texture.cpu().numpy().copy()
    has, si, sj = source(cov, k, rect)
    tex[has] = tex[si[has], sj[has]]
    return torch.from_numpy(tex)
