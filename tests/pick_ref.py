"""Numpy restatement of picking on a mesh (dtp_mesh_pick, dtp_mesh_ray_frame, dtp_mesh_path_plan; csrc/mesh_pick.hip, csrc/mesh_host.h) for
the tests, written from the contract in include/dtp.h ("picking on a mesh") operation for operation: the ray frame and the grid's
exponent in double, rounded to fp32 once; the per-face test in fp32 with every operation rounded once, on the render's snap, coverage and
interpolation (mesh_ref.snap / cover / interp); the winner the largest (z, -face index); the record; the stamp spacing of a pointer path
(the Kit app's ui/brush.py:158-198) in double.  Everything runs on the CPU."""
import math

import numpy as np

import mesh_ref

f32 = np.float32
E_MIN, E_MAX = -64, 64
MAX_CHORD = 1 << 20
FIELDS = ("face", "w", "pos", "normal", "uv", "t")


# ---------------------------------------------------------------- host, double
def ray_frame(origin, direction):
    """-> float32 [3, 4]: rows (r, u, b), each followed by -row . o.  ValueError for what dtp_mesh_ray_frame refuses."""
    o = np.asarray(origin, dtype=f32).astype(np.float64)
    d = np.asarray(direction, dtype=f32).astype(np.float64)
    if not (np.isfinite(o).all() and np.isfinite(d).all()):
        raise ValueError("non-finite")
    ld = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if not ld > 0:
        raise ValueError("the direction is zero")
    b = -(d / ld)
    k = 0
    for i in (1, 2):
        if abs(d[i]) < abs(d[k]):
            k = i
    h = np.zeros(3)
    h[k] = 1.0

    def cross(a, c):
        return np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
    r = cross(h, b)
    r = r / np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    u = cross(b, r)
    out = np.zeros((3, 4), dtype=f32)
    with np.errstate(over="ignore"):
        for j, row in enumerate((r, u, b)):
            out[j, :3] = row.astype(f32)
            out[j, 3] = f32(-((row[0] * o[0] + row[1] * o[1]) + row[2] * o[2]))
    if not np.isfinite(out).all():
        raise ValueError("does not fit fp32")
    return out


def exponent(frame, lo, hi):
    """e of the grid S = 2^e: the largest with 2^e max(|x|, |y|) <= 2^25 over the eight corners of the box, clamped to [-64, 64]."""
    fr = np.asarray(frame, dtype=f32).astype(np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    m = 0.0
    for corner in range(8):
        v = [hi[i] if corner >> i & 1 else lo[i] for i in range(3)]
        for k in range(2):
            x = ((fr[k, 0] * v[0] + fr[k, 1] * v[1]) + fr[k, 2] * v[2]) + fr[k, 3]
            m = max(m, abs(float(x)))
    if not m > 0:
        return E_MAX
    if not math.isfinite(m):
        return E_MIN
    f, k = math.frexp(m)
    return min(max(25 - k + (1 if f == 0.5 else 0), E_MIN), E_MAX)


# ---------------------------------------------------------------- the device's part, fp32
def candidates(p, lo, hi, origin, direction):
    """p float32 [F, 3 corners, 3], the box of the vertices -> [(face, z, w)] in face order: the faces the ray meets not behind its
    origin, with the interpolated camera z (<= 0) and the weights."""
    m = ray_frame(origin, direction)
    S = f32(np.ldexp(1.0, exponent(m, lo, hi)))
    with np.errstate(all="ignore"):
        c = np.stack([((m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]) + m[r, 2] * p[..., 2]) + m[r, 3] for r in range(3)], axis=-1)  # [F, 3, xyz]
        X, Y = mesh_ref.snap(c[..., 0] * S), mesh_ref.snap(c[..., 1] * S)
    finite = np.isfinite(c).all(axis=(1, 2))
    # (the kernel first drops a face whose three X or three Y share a strict sign: such a face cannot cover (0, 0))
    maybe = finite & (X.min(axis=1) <= 0) & (X.max(axis=1) >= 0) & (Y.min(axis=1) <= 0) & (Y.max(axis=1) >= 0)
    centre = np.zeros(1, dtype=np.int64)
    found = []
    for f in np.nonzero(maybe)[0]:
        inside, w = mesh_ref.cover(X[f], Y[f], centre, centre)
        if not inside[0]:
            continue
        w = w[0]
        with np.errstate(all="ignore"):
            z = mesh_ref.interp(w, c[f, 0, 2], c[f, 1, 2], c[f, 2, 2])
        if z == 0:
            z = f32(0)  # (-0 is +0)
        if z <= 0:
            found.append((int(f), z, w))
    return found


def pick(vertices, faces, face_uvs, origins, directions):
    """-> dict of numpy arrays as MI355ConditionalInpainter.pick returns them: face i32 [n], w, pos, normal f32 [n, 3], uv [n, 2], t [n]."""
    verts = np.asarray(vertices, dtype=f32)
    p = verts[np.asarray(faces, dtype=np.int64)]  # [F, 3 corners, 3]
    uvs = np.asarray(face_uvs, dtype=f32)
    F = p.shape[0]
    o = np.asarray(origins, dtype=f32).reshape(-1, 3)
    d = np.asarray(directions, dtype=f32).reshape(-1, 3)
    n = o.shape[0]
    lo, hi = verts.astype(np.float64).min(axis=0), verts.astype(np.float64).max(axis=0)
    out = dict(face=np.full(n, -1, dtype=np.int32), w=np.zeros((n, 3), f32), pos=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32),
               uv=np.zeros((n, 2), f32), t=np.zeros(n, f32))
    for i in range(n):
        best, best_z, best_w = -1, f32(0), None
        for f, z, w in candidates(p, lo, hi, o[i], d[i]):
            if best < 0 or z > best_z:  # (f rises: on a tie the lower index stays)
                best, best_z, best_w = f, z, w
        if best < 0:
            continue
        w, q = best_w, p[best]
        e1, e2 = q[1] - q[0], q[2] - q[0]
        with np.errstate(all="ignore"):
            nrm = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], dtype=f32)
            length = np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2])
            away = (nrm[0] * d[i, 0] + nrm[1] * d[i, 1]) + nrm[2] * d[i, 2] > 0
            nrm = nrm / length
        out["face"][i] = best
        out["w"][i] = w
        out["pos"][i] = [mesh_ref.interp(w, q[0, k], q[1, k], q[2, k]) for k in range(3)]
        out["normal"][i] = -nrm if away else nrm
        out["uv"][i] = [mesh_ref.interp(w, uvs[best, 0, k], uvs[best, 1, k], uvs[best, 2, k]) for k in range(2)]
        out["t"][i] = f32(0) - best_z
    return out


# ---------------------------------------------------------------- the planner (host, double)
def plan_path(hits, stamp_distance, state=None, cap=None):
    """-> (positions f32 [m, 3], normals, prev_positions, state).  state: dict(has_prev, prev) or None.  ValueError for a refused
    stamp_distance or chord; with cap and more stamps than it: ValueError carrying the count, as dtp_mesh_path_plan reports it."""
    sd = f32(stamp_distance)
    if not (sd > 0 and np.isfinite(sd)):
        raise ValueError("stamp_distance")
    sd = float(sd)
    has = bool(state["has_prev"]) if state else False
    prev = np.asarray(state["prev"], dtype=f32) if state else np.zeros(3, f32)
    face = np.asarray(hits["face"])
    pos, nrm = np.asarray(hits["pos"], dtype=f32), np.asarray(hits["normal"], dtype=f32)
    P, N, V = [], [], []
    for i in range(face.shape[0]):
        if face[i] < 0:
            continue
        if not has:
            has, prev = True, pos[i].copy()
            continue
        dl = pos[i].astype(np.float64) - prev.astype(np.float64)
        dist = float(np.sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]))
        if not dist >= sd:
            continue
        q = dist / sd
        if not q <= MAX_CHORD:
            raise ValueError("chord")
        num = int(q)
        step = dist / num
        cur = prev.astype(np.float64)
        for _ in range(num):
            nxt = step * (dl / dist) + cur
            P.append(nxt.astype(f32))
            N.append(nrm[i].copy())
            V.append(cur.astype(f32))
            cur = nxt
        prev = pos[i].copy()
    if cap is not None and len(P) > cap:
        raise ValueError(f"count {len(P)}")
    arr = (lambda rows: np.stack(rows).astype(f32) if rows else np.zeros((0, 3), f32))
    return arr(P), arr(N), arr(V), dict(has_prev=has, prev=tuple(float(x) for x in prev))
