"""Numpy restatement of the anisotropic view (dtp_mesh_view_aniso, dtp_op_mesh_view_aniso; csrc/view.hip) for the tests, written from the
contract in include/dtp.h ("an anisotropic view") operation for operation, on top of mip_ref, view_ref, view_clip_ref and view_aa_ref,
which it uses as they are: the projection, the coverage and the winner (with the faces across the near plane when clip_near) are
view_ref's and view_clip_ref's, the two neighbour evaluations of the winner are written as view_clip_ref writes them, the pyramid and the
bilinear sample of a level are mip_ref's, and the resolve of samples x samples fine pixels is view_aa_ref's.  What is new: the two
footprint vectors kept apart, the level from the shorter one, up to max_aniso trilinear taps along the longer one, their plain average.
fp32 with every operation rounded once (numpy float32 arrays: no contraction).  Everything runs on the CPU."""
import numpy as np

import mesh_ref
import mip_ref
import view_aa_ref
import view_clip_ref
import view_ref

f32 = np.float32
MAX_ANISO = 16


def fine_view(vertices, faces, face_uvs, texture, cam, size=None, max_aniso=1, clip_near=False, levels=None, cull=False, flip_normals=False,
              shade=True, ambient=0.25, unpainted=(128, 128, 128), background=(0, 0, 0, 0)):
    """One sample per pixel -> dict(image uint8 [H, W, 4], face_idx int32 [H, W], depth, lod float32 [H, W], taps uint8 [H, W] (N, 0
    where no face is), level int [H, W] (-1 where no face is), f, rho2, pmax2, pmin2 float32 [H, W], N int [H, W], horizon bool [H, W]
    (the pixels of step 2), crossing bool [H, W], uv)."""
    M = int(max_aniso)
    if not 1 <= M <= MAX_ANISO:
        raise ValueError("max_aniso")
    H, W = cam["size"] if size is None else size
    lv = mip_ref.pyramid(texture) if levels is None else levels
    L = len(lv)
    TH, TW = lv[0].shape[:2]
    uvs = np.asarray(face_uvs, dtype=f32)
    proj = view_ref.project(vertices, faces, cam, H, W, cull, flip_normals)
    cr = view_clip_ref.project_crossing(vertices, faces, cam, cull, flip_normals)
    if clip_near:
        face_idx, q, d, is_cross = view_clip_ref.rasterize(proj, cr, cam, H, W)
    else:
        face_idx, q, d = view_ref.rasterize(proj, H, W)
        is_cross = np.zeros((H, W), dtype=bool)
    hit = face_idx >= 0
    fi = np.where(hit, face_idx, 0)
    U, V = (uvs[fi, 0, 0], uvs[fi, 1, 0], uvs[fi, 2, 0]), (uvs[fi, 0, 1], uvs[fi, 1, 1], uvs[fi, 2, 1])
    py, px = np.meshgrid(np.arange(H, dtype=np.int64) * 256 + 128, np.arange(W, dtype=np.int64) * 256 + 128, indexing="ij")
    with np.errstate(all="ignore"):
        dd = np.where(hit, d, f32(1))
        u = mesh_ref.interp(q, *U) / dd
        v = mesh_ref.interp(q, *V) / dd
        # steps 1-2: the two neighbours, the two vectors, kept apart
        X, Y, iw = proj["X"][fi], proj["Y"][fi], proj["iw"][fi]
        ok, axes = hit.copy(), []
        for ox, oy in ((1, 0), (0, 1)):
            qn = mip_ref.weights_at(X, Y, px + 256 * ox, py + 256 * oy) * iw
            if clip_near:
                gx, gy = view_clip_ref.pixel_rays(cam, H, W, ox, oy)
                _, qc, _ = view_clip_ref.edge_q(cr["n"][fi], cr["inv"][fi], np.broadcast_to(gx[None, :], (H, W)), np.broadcast_to(gy[:, None], (H, W)))
                qn = np.where(is_cross[..., None], qc, qn)
            dn = (qn[..., 0] + qn[..., 1]) + qn[..., 2]
            ok &= np.isfinite(dn) & (dn > 0)
            dun, dvn = mesh_ref.interp(qn, *U) / dn - u, mesh_ref.interp(qn, *V) / dn - v
            a, b = dun * f32(TW), dvn * f32(TH)
            axes.append((dun, dvn, a * a + b * b))
        (dua, dva, la2), (dub, dvb, lb2) = axes
        ok &= np.isfinite(la2) & np.isfinite(lb2)
        horizon = hit & ~ok
        # steps 3-5
        pmax2, pmin2 = np.fmax(la2, lb2), np.fmin(la2, lb2)
        a_major = la2 >= lb2
        du, dv = np.where(a_major, dua, dub), np.where(a_major, dva, dvb)
        rho2 = np.fmin(pmax2, np.fmax(np.fmax(pmin2, f32(1)), pmax2 / f32(M * M)))
        N = np.full((H, W), M, dtype=np.int64)
        for n in range(M, 0, -1):
            N[pmax2 <= f32(n * n) * rho2] = n
        du, dv = np.where(ok, du, f32(0)).astype(f32), np.where(ok, dv, f32(0)).astype(f32)
        N[~ok] = 1
        rho2 = np.where(ok, rho2, f32(np.inf)).astype(f32)
        rho2[~hit] = 0
        # step 6: mip_ref's walk
        level, p4 = np.zeros((H, W), dtype=np.int64), np.ones((H, W), dtype=f32)
        for k in range(1, L):
            step = (level == k - 1) & (p4 * f32(4) <= rho2)
            level[step] = k
            p4 = np.where(step, p4 * f32(4), p4)
        f = np.where((level == L - 1) | (rho2 <= p4), f32(0), ((rho2 / p4) - f32(1)) / f32(3)).astype(f32)
        lod = np.where(hit, level.astype(f32) + f, f32(0)).astype(f32)
        # steps 7-8
        total = np.zeros((H, W, 4), dtype=f32)
        twice = (2 * N).astype(f32)
        for i in range(M):
            act = hit & (i < N)
            if not act.any():
                break
            o = f32(2 * i + 1) / twice - f32(0.5)
            ui, vi = u + du * o, v + dv * o
            t = np.zeros((H, W, 4), dtype=f32)
            for k in range(L):
                here = act & (level == k)
                if not here.any():
                    continue
                tk = mip_ref.sample(lv[k], ui, vi)
                t[here] = tk[here]
                both = here & (f > 0)
                if both.any():
                    up = mip_ref.sample(lv[k + 1], ui, vi)
                    t[both] = (tk + (up - tk) * f[..., None])[both]
            total = np.where(act[..., None], total + t, total)
        t = total / np.maximum(N, 1).astype(f32)[..., None]
        # step 9: view_ref's
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
    N = np.where(hit, N, 0)
    return dict(image=image, face_idx=face_idx, depth=depth, lod=lod, taps=N.astype(np.uint8), level=np.where(hit, level, -1),
                f=np.where(hit, f, f32(0)), N=N, rho2=rho2, pmax2=np.where(hit & ok, pmax2, f32(0)), pmin2=np.where(hit & ok, pmin2, f32(0)),
                horizon=horizon, crossing=is_cross & hit, uv=np.stack([u, v], axis=-1))


def view(vertices, faces, face_uvs, texture, cam, size=None, max_aniso=1, clip_near=False, samples=1, levels=None, **opts):
    """The frame of dtp_mesh_view_aniso -> fine_view's dict with image, face_idx, depth, lod, taps resolved as view_aa_ref resolves them
    (taps travels with face_idx), plus coverage uint8 [H, W] and fine (the fine frame's dict).  samples=1: the fine frame is the frame."""
    H, W = cam["size"] if size is None else size
    s = samples
    if s not in view_aa_ref.SAMPLES:
        raise ValueError("samples")
    if not (1 <= H and 1 <= W and s * H <= view_aa_ref.VIEW_MAX and s * W <= view_aa_ref.VIEW_MAX):
        raise ValueError("size")
    fine = fine_view(vertices, faces, face_uvs, texture, cam, size=(s * H, s * W), max_aniso=max_aniso, clip_near=clip_near, levels=levels, **opts)
    out = dict(fine)
    out["image"] = view_aa_ref.resolve(fine["image"], s)
    for key in ("face_idx", "depth", "lod", "taps", "level", "f", "N", "rho2", "pmax2", "pmin2", "horizon", "crossing"):
        out[key] = view_aa_ref.representative(fine[key], s)
    out["coverage"] = view_aa_ref.coverage(fine["face_idx"], s)
    out["fine"] = fine
    return out


# ---------------------------------------------------------------- the cases the CPU and the GPU tests share
def floor_scene():
    """A floor running away from the eye, striped ACROSS the line of sight: -> (vertices, faces, face_uvs, texture uint8 [256, 256, 4])."""
    v = np.array([(-2, 0, -20), (2, 0, -20), (2, 0, 0), (-2, 0, 0)], dtype=f32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    uv = np.array([[(0, 1), (1, 1), (1, 0)], [(0, 1), (1, 0), (0, 0)]], dtype=f32)
    x = np.arange(256)
    tex = np.zeros((256, 256, 4), dtype=np.uint8)
    tex[:, (x // 8) % 2 == 0, :3] = 255
    tex[..., 3] = 255
    return v, f, uv, tex


def quad_scene():
    """A flat square quad with axis-aligned UVs over the whole of a square texture, 48 x 48: seen head-on, la2 == lb2 in real
    arithmetic.  From (0, 0, 2^k) with a 90 degree camera (fx = fy = 1 exactly) and a square frame of 32 pixels every value on the way
    is dyadic, so the two are equal in fp32 too, and at 1.5 2^k texels per pixel the level has a fraction."""
    v = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], dtype=f32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    uv = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], dtype=f32)
    return v, f, uv


FLOOR_POSE = ((0, 0.25, 1), (0, 0, -3), (0, 1, 0), 45.0, 0.05)   # eye, at, up, fov_y, near
FLOOR_SIZE = (48, 64)
# The number of covered pixels of mip_ref.POSES["grazing"] that take N = 1 .. 4 taps at M = 4, and that take each level, pinned as
# mip_ref.POSES pins its levels.
GRAZING_M4_TAPS = [0, 860, 33, 14]
GRAZING_M4_LEVELS = [700, 175, 25, 1, 5, 1, 0, 0, 0]
# Two more poses at mip_ref.FRAME, picked on this restatement: name -> (scene, eye, at, up, fov_y, near, the number of covered pixels
# that take N = 1 .. 16 at M = 16, the number of those with N = 16 whose footprint is more than 16 times longer than wide: the clamp).
# "floor_low" skims the striped floor with a rolled camera and takes every N from 2 to 16; N = 1 is the magnified pose's, the head-on
# quad's and the horizon triangle's.  "field_skim" is the height field seen from just above it: many small faces, few taps each.
POSES = {
    "floor_low": ("floor", (0.3, 0.12, 1), (0.1, 0, -3), (0.1, 1, 0), 45.0, 0.05, [0, 21, 64, 57, 17, 10, 6, 6, 8, 2, 3, 3, 2, 3, 3, 6], 5),
    "field_skim": ("field:atlas", (-1.3, -0.1, 0.2), (0.8, 0.0, 0.1), (0, 0, 1), 45.0, 0.05, [0, 867, 44, 9, 8, 1, 0, 0, 6, 0, 0, 0, 0, 0, 0, 0], 0),
}
_cache = {}


def scene(name):
    """-> ((vertices, faces, face_uvs), texture, its pyramid), numpy arrays, made once.  name: "floor" (the striped floor), "quad",
    "triangle" (mip_ref.TRIANGLE), "cube" and "clip_floor" (view_clip_ref's), "field" (make_height_field(17, 13, seed=3)); the texture
    is mip_ref's "atlas" unless the scene has its own or the name says which: "field:square", "floor:atlas"."""
    if ("scene", name) not in _cache:
        base, _, tex_name = name.partition(":")
        if base == "floor":
            mesh, own = floor_scene()[:3], floor_scene()[3]
        elif base == "quad":
            mesh, own = quad_scene(), mip_ref.make_texture(48, 48, 79)
        else:
            mesh = dict(triangle=lambda: mip_ref.TRIANGLE, cube=view_clip_ref.cube_mesh, clip_floor=view_clip_ref.floor_mesh,
                        field=lambda: tuple(m.numpy() for m in mip_ref.field()))[base]()
            own = None
        if tex_name or own is None:
            tex, lv = mip_ref.texture(tex_name or "atlas")
        else:
            tex, lv = own, mip_ref.pyramid(own)
        _cache["scene", name] = (tuple(mesh), tex, lv)
    return _cache["scene", name]


def reference(name, pose, size, M, clip_near=False, samples=1, **opts):
    """The restatement's frame of scene(name) at pose = (eye, at, up, fov_y, near): computed once, shared, left unchanged."""
    key = (name, pose, tuple(size), M, clip_near, samples, tuple(sorted(opts.items())))
    if key not in _cache:
        mesh, tex, lv = scene(name)
        eye, at, up, fov, near = pose
        _cache[key] = view(*mesh, tex, view_ref.camera(eye, at, up, fov, size, near), max_aniso=M, clip_near=clip_near, samples=samples, levels=lv,
                           **opts)
    return _cache[key]
