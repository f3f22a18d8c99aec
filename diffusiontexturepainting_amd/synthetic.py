"""Seeded synthetic stamp inputs: procedural texture canvases, brush images
and alpha masks in the spirit of the reference's training-time stamp masks
(training/mask_generator.py:78-182: a few rotated square stamps already painted along one side of
the patch, white = known; 20 % completely empty; sometimes the centre is cleared), plus the two
deterministic cases `preview_mask` (handler.py:48-52) and all-zero alpha.

Everything is generated on the CPU from `torch.Generator().manual_seed(seed)` so CPU-oracle and GPU
runs see identical inputs.
"""
import math

import torch


def texture(res, g, channels=3):
    """Smooth band-limited colour texture in 0..1: a few random sinusoid gratings per channel."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, res), torch.linspace(0, 1, res), indexing="ij")
    img = torch.zeros(channels, res, res)
    for c in range(channels):
        for _ in range(6):
            fx, fy = (torch.rand(2, generator=g) * 14 - 7).tolist()
            ph, amp = (torch.rand(2, generator=g) * torch.tensor([2 * math.pi, 0.25])).tolist()
            img[c] += amp * torch.sin(2 * math.pi * (fx * xx + fy * yy) + ph)
    img = img + 0.05 * torch.randn(channels, res, res, generator=g)
    return (img * 0.6 + 0.5).clamp(0, 1)


def stamp_mask(res, g, prob_empty=0.2, prob_center_clear=0.2):
    """[1,res,res] alpha, 1 = already painted (known)."""
    if torch.rand(1, generator=g).item() < prob_empty:
        return torch.zeros(1, res, res)
    yy, xx = torch.meshgrid(torch.arange(res, dtype=torch.float32), torch.arange(res, dtype=torch.float32), indexing="ij")
    mask = torch.zeros(res, res, dtype=torch.bool)
    n = int(torch.randint(1, 5, (1,), generator=g).item())
    side = 0 if torch.rand(1, generator=g).item() < 0.6 else int(torch.randint(1, 4, (1,), generator=g).item())
    for _ in range(n):
        size = res * (0.45 + 0.35 * torch.rand(1, generator=g).item())
        cx = res * torch.rand(1, generator=g).item()
        cy = -size * 0.15 + size * 0.45 * torch.rand(1, generator=g).item()  # hugging the top edge
        ang = (torch.rand(1, generator=g).item() - 0.5) * math.pi / 2
        dx, dy = xx - cx, yy - cy
        u = dx * math.cos(ang) + dy * math.sin(ang)
        v = -dx * math.sin(ang) + dy * math.cos(ang)
        mask |= (u.abs() < size / 2) & (v.abs() < size / 2)
    mask = torch.rot90(mask, k=side, dims=(0, 1))
    if torch.rand(1, generator=g).item() < prob_center_clear:
        m = int(res * (0.03 + 0.1 * torch.rand(1, generator=g).item()))
        mask[m:res - m, m:res - m] = False
    return mask.float().unsqueeze(0)


def preview_mask(res):
    m = torch.zeros(1, res, res)
    m[:, : res // 2, : res // 2] = 1
    return m


def make_stamp_batch(batch, res, seed):
    """canvas [B,4,R,R], brush [1,3,R,R], latents [B,4,h,h], vae_eps [2,B,4,h,h] -- all fp32 CPU."""
    g = torch.Generator().manual_seed(seed)
    brush = texture(res, g).unsqueeze(0)
    canv = []
    for _ in range(batch):
        canv.append(torch.cat([texture(res, g), stamp_mask(res, g)], dim=0))
    canvas = torch.stack(canv)
    h = res // 8
    latents = torch.randn(batch, 4, h, h, generator=g)
    eps = torch.randn(2, batch, 4, h, h, generator=g)
    return canvas, brush, latents, eps


def make_conditioning(seed):
    """Synthetic [1,14,768] cond / uncond embeddings (used when the brush encoder is bypassed)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 14, 768, generator=g), torch.randn(1, 14, 768, generator=g)


# ---------------------------------------------------------------- meshes for the mesh strokes (tests/test_gpu_mesh.py, tools/mesh_stroke_timing.py)
def make_quad():
    """The square [-1, 1]^2 in the plane z = 0 as two faces whose normal is +z, UVs the unit square (u = (x + 1) / 2, v = (y + 1) / 2):
    seen from +z with fov 1 it fills the stamp window exactly.  -> vertices f32 [4, 3], faces i32 [2, 3], face_uvs f32 [2, 3, 2]."""
    v = torch.tensor([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    return v, f, ((v[:, :2] + 1) / 2)[f.long()].contiguous()


def make_table_on_floor():
    """A floor and a table top that hides part of it: the floor is the square [-1, 1]^2 in the plane z = 0, the top the
    square [-0.4, 0.4]^2 in the plane z = 0.5, two faces each (floor: faces 0 and 1, top: 2 and 3), all normals towards +z.  The floor's
    chart fills u in [0.02, 0.48], the top's u in [0.52, 0.98]; v in [0.02, 0.98] for both.  Seen from +z the middle of the floor, a
    part of two large faces, lies behind the top.  -> vertices f32 [8, 3], faces i32 [4, 3], face_uvs f32 [4, 3, 2]."""
    corners = [(-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)]
    v = torch.tensor([[x, y, 0.0] for x, y in corners] + [[0.4 * x, 0.4 * y, 0.5] for x, y in corners])
    f = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=torch.int32)
    s = (torch.tensor(corners) + 1) / 2  # the corner in its chart's unit square
    chart = torch.cat([torch.stack([0.02 + 0.46 * s[:, 0], 0.02 + 0.96 * s[:, 1]], dim=1),
                       torch.stack([0.52 + 0.46 * s[:, 0], 0.02 + 0.96 * s[:, 1]], dim=1)])
    return v, f, chart[f.long()].contiguous()


def make_height_field(nx=17, ny=13, seed=0, bump=0.35):
    """A bumpy height field over [-1, 1] x [-0.75, 0.75]: nx x ny vertices, 2 (nx - 1)(ny - 1) faces with normals towards +z, and a
    two-chart UV atlas: the faces left of the middle column fill u in [0.03, 0.47], the others u in [0.53, 0.97] MIRRORED (u falls as x
    grows); v in [0.05, 0.95] for both.  Seeded, so every caller gets the same mesh.  -> vertices, faces, face_uvs as make_quad."""
    g = torch.Generator().manual_seed(seed)
    xs, ys = torch.linspace(-1.0, 1.0, nx, dtype=torch.float64), torch.linspace(-0.75, 0.75, ny, dtype=torch.float64)
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    zz = bump * (torch.sin(3.1 * xx + 0.4) * torch.cos(2.3 * yy - 0.2) + 0.25 * torch.sin(9.0 * xx * yy))
    zz = zz + 0.02 * torch.rand(ny, nx, generator=g, dtype=torch.float64)
    verts = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).to(torch.float32)
    mid = (nx - 1) // 2
    faces, uvs = [], []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i

            def uv(col, row, left=i < mid):
                s = col / mid if left else (col - mid) / (nx - 1 - mid)
                return (0.03 + 0.44 * s) if left else (0.97 - 0.44 * s), 0.05 + 0.9 * row / (ny - 1)
            ua, ub, uc, ud = uv(i, j), uv(i + 1, j), uv(i + 1, j + 1), uv(i, j + 1)
            faces += [[a, b, c], [a, c, d]]
            uvs += [[ua, ub, uc], [ua, uc, ud]]
    return verts, torch.tensor(faces, dtype=torch.int32), torch.tensor(uvs, dtype=torch.float32)
