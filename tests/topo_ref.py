"""The numpy restatement of growing a face set (include/dtp.h "growing a face set"): the topology of a mesh -- points by
np.unique over the rows of bit patterns after -0.0 -> +0.0, parts and charts by label propagation to a fixed point -- and the four
extends on boolean arrays.  It imports nothing from the library."""
import numpy as np


def _bits(x):
    """float32 [...] -> uint32 [...]: the bit patterns, -0.0 taken as +0.0 (x + 0.0 is +0.0 for either zero and x for anything else)."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32) + np.float32(0.0)).view(np.uint32)


def points(vertices, faces):
    """int32 [F, 3]: per corner, the lowest vertex index that carries the corner's coordinates."""
    rows = _bits(np.asarray(vertices).reshape(-1, 3))
    _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)  # (first: the lowest index of each distinct row)
    name = first[np.asarray(inverse).reshape(-1)]
    return name[np.asarray(faces, dtype=np.int64)].astype(np.int32)


def _propagate(F, group, face):
    """The classes of faces 0 .. F - 1 under "two faces appear in one group", each labelled by its lowest face: group [n] and face [n]
    list the memberships.  Every round a group takes the lowest label among its faces and a face the lowest among its groups."""
    label = np.arange(F, dtype=np.int64)
    n_groups = int(group.max()) + 1 if len(group) else 0
    while True:
        low = np.full(n_groups, F, dtype=np.int64)
        np.minimum.at(low, group, label[face])
        new = label.copy()
        np.minimum.at(new, face, low[group])
        if (new == label).all():
            return label.astype(np.int32)
        label = new


def parts(point):
    """int32 [F]: the lowest face of the faces linked to f through shared points."""
    F = point.shape[0]
    return _propagate(F, point.reshape(-1).astype(np.int64), np.repeat(np.arange(F, dtype=np.int64), 3))


def charts(point, face_uvs):
    """int32 [F]: the lowest face of the faces linked to f through edges -- unordered pairs of two different points -- on which the UVs
    both faces carry at the two points are equal."""
    F = point.shape[0]
    uv = _bits(np.asarray(face_uvs).reshape(F, 3, 2)).astype(np.int64)
    rows, face = [], []
    for k in range(3):
        j = (k + 1) % 3
        a, b = point[:, k].astype(np.int64), point[:, j].astype(np.int64)
        swap = (a > b)[:, None]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        uv_lo, uv_hi = np.where(swap, uv[:, j], uv[:, k]), np.where(swap, uv[:, k], uv[:, j])
        keep = a != b
        rows.append(np.concatenate([lo[:, None], hi[:, None], uv_lo, uv_hi], axis=1)[keep])
        face.append(np.arange(F, dtype=np.int64)[keep])
    rows, face = np.concatenate(rows), np.concatenate(face)
    if len(rows) == 0:
        return np.arange(F, dtype=np.int32)
    _, group = np.unique(rows, axis=0, return_inverse=True)
    return _propagate(F, np.asarray(group).reshape(-1), face)


def topology(vertices, faces, face_uvs):
    """dict(point, part, chart, num_points, num_parts, num_charts, num_faces), as Mesh.topology() returns it."""
    point = points(vertices, faces)
    part, chart = parts(point), charts(point, face_uvs)
    return dict(point=point, part=part, chart=chart, num_points=len(np.unique(point)), num_parts=len(np.unique(part)),
                num_charts=len(np.unique(chart)), num_faces=point.shape[0])


# ---------------------------------------------------------------- three small meshes the tests share (numpy: vertices, faces, face_uvs)
def split_seam(vertices, faces, face_uvs, nx=6, ny=6):
    """A make_height_field(nx, ny) with the seam column moved to x = 0 and its vertices DUPLICATED, one copy per side: the faces right of
    the seam use the copies, and the copies of the odd rows write x as -0.0.  The same points, parts and charts as the field itself."""
    v, f = np.array(vertices, dtype=np.float32), np.array(faces, dtype=np.int32)
    mid = (nx - 1) // 2
    seam = np.arange(ny) * nx + mid
    v[seam, 0] = 0.0
    copies = v[seam].copy()
    copies[1::2, 0] = -0.0
    right = (np.arange(f.shape[0]) % (2 * (nx - 1))) >= 2 * mid
    remap = np.arange(v.shape[0])
    remap[seam] = v.shape[0] + np.arange(ny)
    f[right] = remap[f[right]]
    return np.concatenate([v, copies]), f, np.array(face_uvs, dtype=np.float32)


def fan():
    """Three faces on the edge (0, 1): faces 0 and 2 carry the same UVs along it, face 1 does not.  One part, charts {0, 2} and {1}."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [1, 0, 3], [1, 0, 4]], dtype=np.int32)
    uv = np.array([[[0.1, 0.1], [0.3, 0.1], [0.1, 0.3]], [[0.8, 0.1], [0.6, 0.1], [0.6, 0.3]], [[0.3, 0.1], [0.1, 0.1], [0.2, 0.0]]], dtype=np.float32)
    return v, f, uv


def touching(degenerate=False):
    """Two triangles that touch in point 0 only: one part, charts {0} and {1}, though their UVs at the point agree.  degenerate: also a
    face (0, 0, 1) with a repeated vertex, whose real edge joins face 0, and a face that is point 0 three times: one part, charts {0, 2},
    {1} and {3} -- a side of zero length unites nothing."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 3, 4], [0, 0, 1], [0, 0, 0]], dtype=np.int32)
    uv = np.array([[[0.5, 0.5], [0.7, 0.5], [0.5, 0.7]], [[0.5, 0.5], [0.3, 0.5], [0.5, 0.3]], [[0.5, 0.5], [0.5, 0.5], [0.7, 0.5]],
                   [[0.5, 0.5], [0.5, 0.5], [0.5, 0.5]]], dtype=np.float32)
    n = 4 if degenerate else 2
    return v, f[:n].copy(), uv[:n].copy()


# ---------------------------------------------------------------- the extends
def _touched(point, sel):
    """bool [F]: the faces that share a point with a face of sel."""
    marked = np.zeros(int(point.max()) + 1, dtype=bool)
    marked[point[sel].reshape(-1)] = True
    return marked[point].any(axis=1)


def extend(topo, sel, how, rings=1):
    """bool [F] -> bool [F]: the set grown by how = "rings", "shrink", "linked" or "charts"."""
    sel = np.asarray(sel, dtype=bool).copy()
    assert sel.shape == (topo["num_faces"],)
    if how == "rings":
        for _ in range(rings):
            sel = _touched(topo["point"], sel)
    elif how == "shrink":
        for _ in range(rings):
            sel = sel & ~_touched(topo["point"], ~sel)
    elif how in ("linked", "charts"):
        label = topo["part" if how == "linked" else "chart"]
        sel = np.isin(label, label[sel])
    else:
        raise ValueError(how)
    return sel
