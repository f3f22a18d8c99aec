"""Torch restatement of the stroke layer (dtp_stroke, csrc/stroke.hip) for the tests, written from the arithmetic of the reference's
Kit app, kit_app/source/extensions/aitoybox.texture_painter/python/manager.py:

  :229-230  renderable_texture():  texture u8 -> float32 / 255
  :37-39    overpaint_canvas():    canvas[..., m0:-m0, m1:-m1] = 0  (all four channels; mode Overpaint)
  :42-45    make_stamp_mask():     1 on [margin, R - margin)^2
  :254,266-268  the update: where the pasted alpha (the stamp mask) is > 0 the texel becomes (painted.clip(max=1) * 255).to(uint8), the
            mask itself giving alpha 255
  :270      mode Erase:            ~update_mask * texture, i.e. 0 in all four channels under the mask
  :70       the brush modes        Inpaint, Erase, Overpaint = 0, 1, 2

in 2D: the "render" of a stamp is an axis-aligned R x R window of the texture.  Everything runs on the CPU.  Also a pure-Python planner
of the grouping rule, written independently of the C one: window overlap is decided by intersecting the sets of texel coordinates."""
import torch

INPAINT, ERASE, OVERPAINT = 0, 1, 2


def _coords(a, R, L, wrap):
    """Texel index and validity of the R coordinates a .. a + R - 1 on an axis of length L."""
    idx = torch.arange(a, a + R, dtype=torch.int64)
    if wrap:
        return torch.remainder(idx, L), torch.ones(R, dtype=torch.bool)
    ok = (idx >= 0) & (idx < L)
    return idx.clamp(0, L - 1), ok


def make_stamp_mask(R, margin):
    m = torch.zeros(R, R, dtype=torch.uint8)
    m[margin:R - margin, margin:R - margin] = 1
    return m


def disc_mask(R, margin=2):
    """A non-trivial paste mask: a disc (the shape of the Kit app's circle_mask, manager.py:48-52), u8 [R, R]."""
    c = (R - 1) / 2.0
    yy, xx = torch.meshgrid(torch.arange(R, dtype=torch.float64), torch.arange(R, dtype=torch.float64), indexing="ij")
    return (((yy - c) ** 2 + (xx - c) ** 2) <= (R / 2.0 - margin) ** 2).to(torch.uint8)


def gather(texture, x, y, R, wrap=False, mode=INPAINT, over=(10, 25)):
    """texture u8 [H, W, 4] -> canvas f32 [1, 4, R, R] of the window whose top-left texel is (row y, column x).  The division is a
    tensor / tensor one: torch turns `t / 255` with a Python scalar into a multiplication by the reciprocal on some devices, which is
    not the same number for every byte."""
    t = texture.cpu()
    H, W = t.shape[0], t.shape[1]
    rows, ok_r = _coords(y, R, H, wrap)
    cols, ok_c = _coords(x, R, W, wrap)
    win = t[rows][:, cols] * (ok_r[:, None] & ok_c[None, :])[..., None].to(torch.uint8)  # outside a non-wrapping texture: 0 x 4
    canvas = win.permute(2, 0, 1).unsqueeze(0).to(torch.float32)
    canvas = torch.div(canvas, torch.full_like(canvas, 255.0))
    if mode == OVERPAINT:
        canvas[..., over[0]:R - over[0], over[1]:R - over[1]] = 0
    return canvas


def decoded_to_u8(dec):
    """dec f32 [R, R, >= 3], the VAE decoder's output around -1 .. 1 -> u8 [R, R, 3]: the clamp of inpaint_pipeline.py:148 and the
    truncating conversion of handler.py:55-56, i.e. what generate_u8(composite=False) returns."""
    return ((dec[..., :3].cpu() / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8)


def footprint(H, W, x, y, mask, wrap=False):
    """bool [H, W]: the texels a paste of this window through `mask` may write."""
    R = mask.shape[0]
    rows, ok_r = _coords(y, R, H, wrap)
    cols, ok_c = _coords(x, R, W, wrap)
    sel = (mask.cpu() > 0) & ok_r[:, None] & ok_c[None, :]
    fp = torch.zeros(H, W, dtype=torch.bool)
    fp[rows[:, None].expand(R, R)[sel], cols[None, :].expand(R, R)[sel]] = True
    return fp


def paste(texture, painted_u8, mask, x, y, wrap=False, mode=INPAINT):
    """In place on the CPU tensor texture u8 [H, W, 4]: under mask > 0 (and inside a non-wrapping texture) the texel becomes
    (painted_u8 [R, R, 3], 255), or 0 x 4 in mode Erase (painted_u8 unused).  Returns texture."""
    R = mask.shape[0]
    H, W = texture.shape[0], texture.shape[1]
    rows, ok_r = _coords(y, R, H, wrap)
    cols, ok_c = _coords(x, R, W, wrap)
    sel = (mask.cpu() > 0) & ok_r[:, None] & ok_c[None, :]
    if mode == ERASE:
        px = torch.zeros(R, R, 4, dtype=torch.uint8)
    else:
        px = torch.cat([painted_u8.cpu(), torch.full((R, R, 1), 255, dtype=torch.uint8)], dim=2)
    texture[rows[:, None].expand(R, R)[sel], cols[None, :].expand(R, R)[sel]] = px[sel]
    return texture


# ---------------------------------------------------------------- the planner
def _axis_cells(a, R, L, wrap):
    return {(a + i) % L for i in range(R)} if wrap else set(range(a, a + R))


def windows_overlap(p, q, H, W, R, wrap):
    """p, q: (x, y).  Two windows overlap iff they share a texel coordinate on x AND on y."""
    return bool(_axis_cells(p[0], R, W, wrap) & _axis_cells(q[0], R, W, wrap)) and \
        bool(_axis_cells(p[1], R, H, wrap) & _axis_cells(q[1], R, H, wrap))


def plan(H, W, R, wrap, stamps, max_group):
    """stamps: (x, y, mode) in the caller's order -> group_of.  A stamp joins the last group iff that group is not full, no Erase stamp
    is involved and its window overlaps none of the group's; otherwise it opens the next group."""
    groups = []
    for i, (x, y, mode) in enumerate(stamps):
        cur = groups[-1] if groups else None
        joins = (cur is not None and len(cur) < max_group and mode != ERASE and all(stamps[j][2] != ERASE for j in cur)
                 and not any(windows_overlap((x, y), stamps[j][:2], H, W, R, wrap) for j in cur))
        if joins:
            cur.append(i)
        else:
            groups.append([i])
    group_of = [0] * len(stamps)
    for g, members in enumerate(groups):
        for i in members:
            group_of[i] = g
    return group_of
