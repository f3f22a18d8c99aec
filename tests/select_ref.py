"""Numpy restatement of face sets (include/dtp.h "face sets: a lasso, masked strokes, a tint"; csrc/select.hip, csrc/select_host.h) for
the tests, written from the contract: the lasso's vertices snapped in fp32 by the raster's snap, the even-odd inside test in int64 with no
float anywhere, the packing of a set into 32-bit words, the masked backprojection as mesh_ref's with one more condition on a valid face,
and the tint in integers.  Everything runs on the CPU."""
import numpy as np
import torch

import mesh_ref

f32 = np.float32
REPLACE, ADD, SUBTRACT = "replace", "add", "subtract"


# ---------------------------------------------------------------- the lasso
def snap_polygon(polygon):
    """float [n, 2] as (x, y) -> int64 [n, 2]: snap(256.0f * x) in fp32 (rint, clamped to +-2^26)."""
    p = np.asarray(polygon, dtype=f32).reshape(-1, 2)
    with np.errstate(over="ignore"):
        return mesh_ref.snap(f32(256.0) * p)


def inside(xy, H, W):
    """xy int64 [n, 2] snapped -> bool [H, W]: the pixels whose centre (256 j + 128, 256 i + 128) is inside by the even-odd rule."""
    xy = np.asarray(xy, dtype=np.int64)
    py, px = np.meshgrid(np.arange(H, dtype=np.int64) * 256 + 128, np.arange(W, dtype=np.int64) * 256 + 128, indexing="ij")
    odd = np.zeros((H, W), dtype=bool)
    n = xy.shape[0]
    for k in range(n):
        (ax, ay), (bx, by) = xy[k], xy[(k + 1) % n]
        crosses = (ay > py) != (by > py)
        dy = by - ay
        D = (px - ax) * dy - (py - ay) * (bx - ax)
        odd ^= crosses & (D != 0) & ((D < 0) == (dy > 0))
    return odd


def hit_faces(face_idx, polygon, F):
    """-> bool [F]: the faces 0 <= f < F that are face_idx at one or more inside pixels."""
    fi = np.asarray(face_idx.cpu() if isinstance(face_idx, torch.Tensor) else face_idx).astype(np.int64)
    H, W = fi.shape
    f = fi[inside(snap_polygon(polygon), H, W)]
    f = f[(f >= 0) & (f < F)]
    hit = np.zeros(F, dtype=bool)
    hit[f] = True
    return hit


def select(face_idx, polygon, F, op=REPLACE, before=None):
    """The set after model.select_faces(op=...) as bool [F]; before: the set it edits, bool [F] (default empty)."""
    before = np.zeros(F, dtype=bool) if before is None else np.asarray(before, dtype=bool)
    hit = hit_faces(face_idx, polygon, F)
    if op == REPLACE:
        return hit
    if op == ADD:
        return before | hit
    if op == SUBTRACT:
        return before & ~hit
    raise ValueError(op)


# ---------------------------------------------------------------- packing
def pack(mask):
    """bool [F] -> int32 [(F + 31) // 32]: bit f % 32 of word f // 32 is face f."""
    mask = np.asarray(mask, dtype=bool)
    F = mask.shape[0]
    bits = np.zeros(32 * ((F + 31) // 32), dtype=np.uint64)
    bits[:F] = mask
    words = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def unpack(sel, F):
    """int32 words -> bool [F]; bits at positions >= F are dropped."""
    w = np.asarray(sel.cpu() if isinstance(sel, torch.Tensor) else sel).astype(np.int32).view(np.uint32)
    bits = (w[:, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(-1)[:F].astype(bool)


# ---------------------------------------------------------------- the masked backprojection
def backproject(proj, face_idx, face_uvs, dec, mask, texture, selected, painted=None):
    """mesh_ref.backproject with the face set `selected` (bool [F]): valid = front, not steep, owned AND selected.  proj is left as it
    was."""
    masked = dict(proj)
    masked["upright"] = proj["upright"] & np.asarray(selected, dtype=bool)
    return mesh_ref.backproject(masked, face_idx, face_uvs, dec, mask, texture, painted=painted)


# ---------------------------------------------------------------- the tint
def tint(frame, face_idx, selected, color=(255, 160, 0), opacity=128):
    """frame u8 [H, W, 4], face_idx i32 [H, W] (torch), selected bool [F] -> the tinted frame as a new tensor."""
    out = frame.cpu().numpy().copy()
    fi = face_idx.cpu().numpy().astype(np.int64)
    sel = np.asarray(selected, dtype=bool)
    F = sel.shape[0]
    ok = (fi >= 0) & (fi < F)
    on = np.zeros(fi.shape, dtype=bool)
    on[ok] = sel[fi[ok]]
    a = int(opacity)
    for ch in range(3):
        c = out[..., ch].astype(np.int64)
        out[..., ch] = np.where(on, (c * (255 - a) + int(color[ch]) * a + 127) // 255, c).astype(np.uint8)
    return torch.from_numpy(out)
