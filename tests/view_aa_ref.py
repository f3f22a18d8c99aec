"""Numpy restatement of the anti-aliased view (dtp_mesh_view_aa, dtp_op_mesh_view_aa; csrc/view.hip) for the tests, written from the
contract in include/dtp.h ("an anti-aliased view"): the FINE frame is what view_ref.view, mip_ref.view or view_clip_ref.view gives for the
same camera at size (s H, s W) -- those modules are used as they are -- and the frame is its resolve: per channel the rounded box average
of the s x s bytes, in integers; face_idx, depth and lod of fine pixel (s i + s / 2, s j + s / 2); coverage the number of the s x s fine
pixels that show a face.  Everything runs on the CPU."""
import numpy as np

import mip_ref
import view_clip_ref
import view_ref

SAMPLES = (1, 2, 4)
VIEW_MAX = 4096


def resolve(fine, s):
    """fine uint8 [s H, s W, 4] -> uint8 [H, W, 4]: (the sum of the s x s bytes + s s / 2) >> log2(s s), per channel."""
    fine = np.asarray(fine)
    assert s in SAMPLES and fine.dtype == np.uint8 and fine.shape[0] % s == 0 and fine.shape[1] % s == 0 and fine.shape[2] == 4
    H, W = fine.shape[0] // s, fine.shape[1] // s
    total = fine.reshape(H, s, W, s, 4).astype(np.int64).sum(axis=(1, 3))
    return ((total + (s * s) // 2) >> {1: 0, 2: 2, 4: 4}[s]).astype(np.uint8)


def representative(fine, s):
    """fine [s H, s W] -> [H, W]: the fine pixel (s i + s / 2, s j + s / 2) of every pixel."""
    return np.ascontiguousarray(np.asarray(fine)[s // 2::s, s // 2::s])


def coverage(fine_face_idx, s):
    """fine face_idx int32 [s H, s W] -> uint8 [H, W]: how many of the pixel's s x s samples show a face."""
    hit = np.asarray(fine_face_idx) >= 0
    H, W = hit.shape[0] // s, hit.shape[1] // s
    return hit.reshape(H, s, W, s).sum(axis=(1, 3)).astype(np.uint8)


def view(vertices, faces, face_uvs, texture, cam, size=None, samples=1, filter="bilinear", clip_near=False, levels=None, **opts):
    """-> dict(image uint8 [H, W, 4], face_idx int32 [H, W], depth float32 [H, W], coverage uint8 [H, W], lod float32 [H, W] (trilinear
    only), faces_seen int [H, W] (how many different face indices the pixel's samples show, the background's -1 counted as one), fine
    (the fine frame's dict)).  ValueError for what dtp_mesh_view_aa refuses of samples and the size.  opts: view_ref.view's."""
    H, W = cam["size"] if size is None else size
    s = samples
    if s not in SAMPLES:
        raise ValueError("samples")
    if not (1 <= H and 1 <= W and s * H <= VIEW_MAX and s * W <= VIEW_MAX):
        raise ValueError("size")
    if filter not in ("bilinear", "trilinear"):
        raise ValueError("filter")
    trilinear = filter == "trilinear"
    fsize = (s * H, s * W)
    if clip_near:
        fine = view_clip_ref.view(vertices, faces, face_uvs, texture, cam, size=fsize, clip_near=True, filter=filter, levels=levels, **opts)
    elif trilinear:
        fine = mip_ref.view(vertices, faces, face_uvs, texture, cam, size=fsize, levels=levels, **opts)
    else:
        fine = view_ref.view(vertices, faces, face_uvs, texture, cam, size=fsize, **opts)
    fi = fine["face_idx"]
    blocks = np.sort(fi.reshape(H, s, W, s).transpose(0, 2, 1, 3).reshape(H, W, s * s), axis=2)
    seen = 1 + (blocks[..., 1:] != blocks[..., :-1]).sum(axis=2)
    out = dict(image=resolve(fine["image"], s), face_idx=representative(fi, s), depth=representative(fine["depth"], s), coverage=coverage(fi, s),
               faces_seen=seen, fine=fine)
    if trilinear:
        out["lod"] = representative(fine["lod"], s)
    return out
