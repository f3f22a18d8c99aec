"""The Python side of the mesh strokes (include/dtp.h: dtp_mesh_*): the device-resident mesh, the host-only camera and
the stamp array of a stroke.  The stroke itself is MI355ConditionalInpainter.paint_mesh_stroke; the two kernels' op-level entry points
are ops.mesh_render / ops.mesh_backproject.  The bleed pass that pads the UV charts is paint_mesh_stroke(bleed=k) and
MI355ConditionalInpainter.bleed_texture; ops.mesh_coverage / ops.mesh_bleed_offsets show what it works from.  Picking:
the host-only ray frame and the stamp spacing of a pointer path live here; the pick itself is MI355ConditionalInpainter.pick and the
pointer-to-paint call paint_mesh_path.  The view: the host-only perspective camera and the rays of its pixels live here;
the frame itself is MI355ConditionalInpainter.render_view (ops.mesh_view at op level).  Face sets: the packing of a
set of faces into int32 words and its checks live here; the lasso is MI355ConditionalInpainter.select_faces, the stroke that respects a
set paint_mesh_stroke(face_mask=), the tint tint_selection.  The occlusion test of the backprojection: the reading of
the `occlude` keyword lives here; the test itself is paint_mesh_stroke(occlude=) and ops.mesh_backproject(fov=, occlude=).  Growing a
face set: Mesh.topology() and the host-only topology_build live here; the growth itself is
MI355ConditionalInpainter.extend_selection and select_faces(extend=) (ops.faceset_extend at op level)."""
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


def ray_frame(origin, direction):
    """The frame of a picking ray (dtp_mesh_ray_frame: host only, needs no GPU): float32 [3, 4], rows (right, up, back) with
    back = -normalize(direction) and right = normalize(cross(helper, back)), helper the unit axis of the smallest |direction_k|, each
    followed by -row . origin.  The ray is the frame's -z axis through x = y = 0.  DtpError for a zero or non-finite direction, a
    non-finite origin or a frame that does not fit fp32."""
    out = (C.c_float * 12)()
    check(_lib.load().dtp_mesh_ray_frame(C.byref(_vec3(origin, "origin")), C.byref(_vec3(direction, "direction")), C.byref(out)),
          "dtp_mesh_ray_frame")
    return torch.tensor(list(out), dtype=torch.float32).reshape(3, 4)


def rays(origins, directions):
    """-> (float32 [n, 6] on the host: the dtp_ray array of a pick, n).  origins, directions: [n, 3] (or [3] for one ray)."""
    o = torch.as_tensor(origins).detach().to("cpu", torch.float32).reshape(-1, 3)
    d = torch.as_tensor(directions).detach().to("cpu", torch.float32).reshape(-1, 3)
    if o.shape[0] != d.shape[0]:
        raise ValueError(f"{o.shape[0]} origins and {d.shape[0]} directions")
    return torch.cat([o, d], dim=1).contiguous(), o.shape[0]


HIT_WORDS = 13  # sizeof(dtp_mesh_hit) / 4


def hits_dict(records):
    """int32 [n, 13] (dtp_mesh_hit records as words) -> dict(face i32 [n], w f32 [n, 3], pos [n, 3], normal [n, 3], uv [n, 2], t [n])."""
    fl = records.view(torch.float32)
    return dict(face=records[:, 0].clone(), w=fl[:, 1:4].clone(), pos=fl[:, 4:7].clone(), normal=fl[:, 7:10].clone(), uv=fl[:, 10:12].clone(),
                t=fl[:, 12].clone())


def _hit_records(hits):
    """The inverse of hits_dict, on the host; a planner needs face, pos and normal only: the other fields may be missing."""
    face = torch.as_tensor(hits["face"]).detach().to("cpu", torch.int32).reshape(-1)
    n = face.shape[0]
    rec = torch.zeros(n, HIT_WORDS, dtype=torch.int32)
    rec[:, 0] = face
    fl = rec.view(torch.float32)
    for key, sl in (("w", slice(1, 4)), ("pos", slice(4, 7)), ("normal", slice(7, 10)), ("uv", slice(10, 12)), ("t", slice(12, 13))):
        if key in hits:
            fl[:, sl] = torch.as_tensor(hits[key]).detach().to("cpu", torch.float32).reshape(n, -1)
    return rec


def plan_path(hits, stamp_distance, state=None):
    """The stamps of a pointer path (dtp_mesh_path_plan: host only; the Kit app's ui/brush.py:158-198): hits the dict model.pick
    returns (face, pos and normal are used), in pointer order; stamp_distance = radius / stamps_per_radius.  A miss is skipped, the
    first hit only starts the path, and the chord from the previous hit to a hit at least stamp_distance away is cut into
    int(dist / stamp_distance) equal steps: each stamp carries that hit's normal and the stamp before it as its previous position.
    state: None for a new path, or what an earlier call returned (a path may arrive in several calls).
    -> (positions f32 [m, 3], normals [m, 3], prev_positions [m, 3], state) for paint_mesh_stroke."""
    lib = _lib.load()
    rec = _hit_records(hits)
    n = rec.shape[0]
    st = _lib.PathState(0, (0.0, 0.0, 0.0)) if state is None else _lib.PathState(int(state["has_prev"]), tuple(float(x) for x in state["prev"]))
    count = C.c_int(-1)
    rc = lib.dtp_mesh_path_plan(_lib.ptr(rec), n, C.c_float(float(stamp_distance)), C.byref(st), None, None, None, 0, C.byref(count))
    m = count.value
    if rc != 0 and m <= 0:
        check(rc, "dtp_mesh_path_plan")
    out = torch.zeros(3, max(m, 0), 3, dtype=torch.float32)
    if m > 0:
        check(lib.dtp_mesh_path_plan(_lib.ptr(rec), n, C.c_float(float(stamp_distance)), C.byref(st), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                     m, C.byref(count)), "dtp_mesh_path_plan")
    return out[0], out[1], out[2], dict(has_prev=bool(st.has_prev), prev=tuple(st.prev))


class ViewCamera:
    """A perspective camera of render_view (dtp_view_cam): m float32 [3, 4], rows (right, up, back) of the look-at, each followed by its
    translation; fx, fy the focal lengths in NDC units; near the near plane's distance; size = (H, W) of the frame it was made for."""

    def __init__(self, m, fx, fy, near, size):
        self.m, self.fx, self.fy, self.near, self.size = m, float(fx), float(fy), float(near), (int(size[0]), int(size[1]))

    def struct(self):
        return _lib.ViewCam((C.c_float * 12)(*[float(v) for v in torch.as_tensor(self.m).reshape(-1).tolist()]), self.fx, self.fy, self.near)

    def __repr__(self):
        return f"ViewCamera(m={self.m.tolist()}, fx={self.fx}, fy={self.fy}, near={self.near}, size={self.size})"


def view_camera(eye, at, up, fov_y=45.0, size=(720, 1280), near=0.01):
    """The perspective camera of a view (dtp_view_camera: host only, needs no GPU): the look-at from `eye` at `at` with `up`, a vertical
    field of view of fov_y degrees over a frame of size = (H, W) pixels; faces nearer than `near` along the view direction are not
    drawn.  -> ViewCamera.  DtpError for anything non-finite, eye == at, an up that is zero or parallel to the view direction, fov_y
    outside (0, 180), near <= 0, a side outside 1..4096."""
    out = _lib.ViewCam()
    check(_lib.load().dtp_view_camera(C.byref(_vec3(eye, "eye")), C.byref(_vec3(at, "at")), C.byref(_vec3(up, "up")), C.c_float(float(fov_y)),
                                      int(size[0]), int(size[1]), C.c_float(float(near)), C.byref(out)), "dtp_view_camera")
    return ViewCamera(torch.tensor(list(out.m), dtype=torch.float32).reshape(3, 4), out.fx, out.fy, out.near, size)


def view_rays(camera, pixels, size=None):
    """The rays of pixel positions of a view (dtp_view_rays: host only): pixels [n, 2] (or [2]) as (x, y), the centre of pixel (row i,
    column j) being (j + 0.5, i + 0.5); size = (H, W), default the camera's.  -> (origins f32 [n, 3], directions f32 [n, 3]) on the
    host, ready for model.pick and paint_mesh_path: the face a frame shows at a pixel is the face its ray hits.  That holds for the
    faces wholly in front of the camera's near plane; a face across it is shown only by render_view(clip_near=True), and with that
    keyword it holds for those too (a ray also hits what no frame shows: faces nearer than the plane)."""
    H, W = camera.size if size is None else size
    xy = torch.as_tensor(pixels).detach().to("cpu", torch.float32).reshape(-1, 2).contiguous()
    n = xy.shape[0]
    out = torch.zeros(max(n, 1), 6, dtype=torch.float32)
    cam = camera.struct()
    src = xy if n else torch.zeros(1, 2, dtype=torch.float32)  # (an empty tensor has no address; n = 0 is the library's to refuse)
    check(_lib.load().dtp_view_rays(C.byref(cam), int(H), int(W), _lib.ptr(src), n, _lib.ptr(out)), "dtp_view_rays")
    return out[:n, :3].clone(), out[:n, 3:].clone()


def view_opts(cull=False, flip_normals=False, shade=True, ambient=0.25, unpainted=(128, 128, 128), background=(0, 0, 0, 0)):
    """The dtp_view_opts of a view."""
    if len(unpainted) != 3 or len(background) != 4 or not all(0 <= int(v) <= 255 for v in tuple(unpainted) + tuple(background)):
        raise ValueError(f"unpainted is 3 and background 4 bytes in 0..255, got {unpainted!r} and {background!r}")
    return _lib.ViewOpts(int(bool(cull)), int(bool(flip_normals)), int(bool(shade)), float(ambient), (C.c_uint8 * 3)(*[int(v) for v in unpainted]),
                         (C.c_uint8 * 4)(*[int(v) for v in background]))


# ---------------------------------------------------------------- face sets
def faceset_words(F):
    """The int32 words of a face set of F faces."""
    return (int(F) + 31) // 32


def faceset_empty(F, device):
    """The empty face set of a mesh of F faces: int32 [(F + 31) // 32] of zeros on `device`.  Bit f % 32 of word f // 32 is face f; the
    bits at positions >= F are ignored by every kernel, so ~sel is a face set, and | and & are union and intersection."""
    return torch.zeros(faceset_words(F), dtype=torch.int32, device=device)


def faceset_from_bool(mask):
    """bool [F] (any device) -> the face set with exactly those faces, on the same device."""
    mask = torch.as_tensor(mask)
    if mask.dim() != 1 or mask.dtype != torch.bool:
        raise ValueError(f"a bool [F] tensor expected, got {mask.dtype} {tuple(mask.shape)}")
    F = mask.shape[0]
    bits = torch.zeros(32 * faceset_words(F), dtype=torch.int64, device=mask.device)
    bits[:F] = mask
    w = (bits.reshape(-1, 32) << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(dim=1)  # 0 .. 2^32 - 1
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def faceset_to_bool(sel, F):
    """A face set -> bool [F] on its device; stray bits at positions >= F (of ~sel, say) are dropped."""
    if sel.dtype != torch.int32 or sel.dim() != 1 or sel.shape[0] != faceset_words(F):
        raise ValueError(f"a face set of {F} faces is int32 [{faceset_words(F)}], got {sel.dtype} {tuple(sel.shape)}")
    bits = (sel.to(torch.int64)[:, None] >> torch.arange(32, dtype=torch.int64, device=sel.device)) & 1
    return bits.reshape(-1)[:int(F)].bool()


def faceset_check(sel, F, device, what="face_mask"):
    """ValueError for what a stroke, a select or a tint refuses of a face set: the wrong dtype, length or device, or a view that is not
    contiguous.  Before anything is enqueued."""
    if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int32:
        raise ValueError(f"{what} must be a torch.int32 tensor (a face set), got {getattr(sel, 'dtype', type(sel))}")
    if sel.dim() != 1 or sel.shape[0] != faceset_words(F):
        raise ValueError(f"{what} must have (F + 31) // 32 = {faceset_words(F)} words for {F} faces, got shape {tuple(sel.shape)}")
    if sel.device != torch.device(device):
        raise ValueError(f"{what} must be on {device}, the mesh's device; it is on {sel.device}")
    if not sel.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return sel


def topology_build(vertices, faces, face_uvs):
    """The topology of a mesh on the host (dtp_topology_build: host only, needs no GPU), from vertices [V, 3], faces [F, 3] and face_uvs
    [F, 3, 2] -> the dict of Mesh.topology().  DtpError for what load_mesh refuses of the data."""
    v = torch.as_tensor(vertices).detach().to("cpu", torch.float32).contiguous()
    f = torch.as_tensor(faces).detach().to("cpu", torch.int32).contiguous()
    uv = torch.as_tensor(face_uvs).detach().to("cpu", torch.float32).contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or tuple(uv.shape) != (f.shape[0], 3, 2):
        raise ValueError(f"vertices [V, 3], faces [F, 3] and face_uvs [F, 3, 2] expected, got {tuple(v.shape)}, {tuple(f.shape)}, {tuple(uv.shape)}")
    F, n = f.shape[0], max(f.shape[0], 1)  # (an empty tensor has no address; F = 0 is the library's to refuse)
    point, part, chart = torch.zeros(n, 3, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    counts = (C.c_int * 3)()
    src = [t if t.numel() else torch.zeros(1, dtype=t.dtype) for t in (v, f, uv)]
    check(_lib.load().dtp_topology_build(_lib.ptr(src[0]), v.shape[0], _lib.ptr(src[1]), F, _lib.ptr(src[2]), _lib.ptr(point), _lib.ptr(part),
                                         _lib.ptr(chart), C.byref(counts)), "dtp_topology_build")
    return dict(point=point.numpy(), part=part.numpy(), chart=chart.numpy(), num_points=counts[0], num_parts=counts[1], num_charts=counts[2],
                num_faces=F)


OCCLUDE_DEFAULT = 1.0  # stamp pixels: what occlude=True means


def occlude_arg(occlude):
    """The `occlude` keyword of paint_mesh_stroke and ops.mesh_backproject -> None (off: None or False) or the tolerance in stamp pixels as
    a float (True: OCCLUDE_DEFAULT).  ValueError for a value that is negative, not finite or not fp32-sized, before anything is enqueued."""
    if occlude is None or occlude is False:
        return None
    if occlude is True:
        return OCCLUDE_DEFAULT
    try:
        value = float(occlude)
    except (TypeError, ValueError):
        raise ValueError(f"occlude must be None, a bool or a float >= 0 (a tolerance in stamp pixels), got {occlude!r}") from None
    if not (0.0 <= value <= 3.4028234663852886e38):
        raise ValueError(f"occlude must be a finite float >= 0 that fits fp32 (a tolerance in stamp pixels), got {occlude!r}")
    return value


def lasso_polygon(polygon):
    """float [n, 2] as (x, y) pixel coordinates -> (contiguous float32 [n, 2] on the host, n); the count and the values are the
    library's to refuse."""
    p = torch.as_tensor(polygon).detach().to("cpu", torch.float32)
    if p.dim() != 2 or p.shape[1] != 2:
        raise ValueError(f"polygon must be [n, 2] as (x, y), got {tuple(p.shape)}")
    return p.contiguous(), p.shape[0]


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

    ray_frame = staticmethod(ray_frame)  # host only: see the functions of this module
    plan_path = staticmethod(plan_path)
    view_camera = staticmethod(view_camera)
    view_rays = staticmethod(view_rays)

    def topology(self):
        """The topology that extend_selection grows a face set by (dtp_mesh_topology, dtp_mesh_topology_labels), as numpy
        on the host: point int32 [F, 3] (the lowest vertex index with the coordinates of that corner, -0.0 taken as +0.0: vertices split
        along a UV seam weld), part int32 [F] (the lowest face of the faces linked to it through shared points), chart int32 [F] (the
        lowest face of its UV chart: linked through edges on which the UVs agree), num_points, num_parts, num_charts and num_faces.  Built
        on the first call, on the current stream, which it waits for; cached on the object."""
        if getattr(self, "_topology", None) is None:
            if not self._h:
                raise ValueError("the mesh is closed")
            F = self.num_faces
            point, part, chart = torch.zeros(F, 3, dtype=torch.int32), torch.zeros(F, dtype=torch.int32), torch.zeros(F, dtype=torch.int32)
            counts = (C.c_int * 3)()
            dev = self._keep._device if self._keep is not None else torch.device("cuda", torch.cuda.current_device())
            s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            check(self._lib.dtp_mesh_topology(self._h, C.byref(counts), s), "dtp_mesh_topology")
            check(self._lib.dtp_mesh_topology_labels(self._h, _lib.ptr(point), _lib.ptr(part), _lib.ptr(chart), s), "dtp_mesh_topology_labels")
            self._topology = dict(point=point.numpy(), part=part.numpy(), chart=chart.numpy(), num_points=counts[0], num_parts=counts[1],
                                  num_charts=counts[2], num_faces=F)
        return self._topology

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
