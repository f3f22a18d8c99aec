"""The Python side of the mesh strokes (include/dtp.h: dtp_mesh_*): the device-resident mesh, the host-only camera and
the stamp array of a stroke.  The stroke itself is MI355ConditionalInpainter.paint_mesh_stroke; the two kernels' op-level entry points
are ops.mesh_render / ops.mesh_backproject.  The bleed pass that pads the UV charts is paint_mesh_stroke(bleed=k) and
MI355ConditionalInpainter.bleed_texture; ops.mesh_coverage / ops.mesh_bleed_offsets show what it works from."""
import ctypes as C

import torch

from . import _lib
from ._lib import check


def _vec3(v, what):
    v = [float(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    if len(v) != 3:
        raise ValueError(f"{what} must have 3 components, got {len(v)}")
    return (C.c_float * 3)(*v)


def mesh_camera(position, normal, prev_position, fov):
    """The view matrix of a stamp (make_camera, manager.py:199-227; dtp_mesh_camera: host only, needs no GPU): float32 [3, 4], rows
    (right, up, back) of the look-at from position + normal at position with up = prev_position - position, each followed by its
    translation.  NDC = camera x, y / fov.  DtpError for a zero normal, an up that is zero or parallel to the normal, a non-finite input
    or fov <= 0."""
    out = (C.c_float * 12)()
    check(_lib.load().dtp_mesh_camera(C.byref(_vec3(position, "position")), C.byref(_vec3(normal, "normal")),
                                      C.byref(_vec3(prev_position, "prev_position")), C.c_float(float(fov)), C.byref(out)), "dtp_mesh_camera")
    return torch.tensor(list(out), dtype=torch.float32).reshape(3, 4)


class Mesh:
    """A mesh on the device of a handle (dtp_mesh_create): vertices [V, 3] float, faces [F, 3] int, face_uvs [F, 3, 2] float (UVs in
    0..1, v up; kaolin's SurfaceMesh.face_uvs), copied from the host.  Freed by close(), by garbage collection, or with its handle."""

    def __init__(self, handle, vertices, faces, face_uvs, keep=None):
        v = torch.as_tensor(vertices).detach().to("cpu", torch.float32).contiguous()
        f = torch.as_tensor(faces).detach().to("cpu", torch.int32).contiguous()
        uv = torch.as_tensor(face_uvs).detach().to("cpu", torch.float32).contiguous()
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or tuple(uv.shape) != (f.shape[0], 3, 2):
            raise ValueError(f"vertices [V, 3], faces [F, 3] and face_uvs [F, 3, 2] expected, got {tuple(v.shape)}, {tuple(f.shape)}, "
                             f"{tuple(uv.shape)}")
        self._lib = _lib.load()
        self._keep = keep  # the model: its handle must outlive the mesh
        self.num_vertices, self.num_faces = v.shape[0], f.shape[0]
        h = C.c_void_p()
        check(self._lib.dtp_mesh_create(handle, C.c_void_p(v.data_ptr()), v.shape[0], C.c_void_p(f.data_ptr()), f.shape[0],
                                        C.c_void_p(uv.data_ptr()), C.byref(h)), "dtp_mesh_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            check(self._lib.dtp_mesh_destroy(h), "dtp_mesh_destroy")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.dtp_mesh_destroy(self._h)  # (already freed with its handle: refused, nothing followed)
                self._h = None
        except Exception:
            pass


def mesh_stamps(positions, normals, prev_positions, fov, seeds, mode_ids, slots):
    """The dtp_mesh_stamp array of a stroke (the per-stamp lists are already of one length n; fov: one float or n)."""
    n = len(positions)
    if len(normals) != n or len(prev_positions) != n:
        raise ValueError(f"{n} positions, {len(normals)} normals and {len(prev_positions)} previous positions")
    fovs = [float(fov)] * n if isinstance(fov, (int, float)) else [float(x) for x in fov]
    if len(fovs) != n:
        raise ValueError(f"{len(fovs)} fov values for {n} stamps")
    arr = (_lib.MeshStamp * n)()
    for i in range(n):
        arr[i] = _lib.MeshStamp(_vec3(positions[i], "a position"), _vec3(normals[i], "a normal"), _vec3(prev_positions[i], "a previous position"),
                                fovs[i], mode_ids[i], int(slots[i]) if slots is not None else 0, seeds[i])
    return arr
