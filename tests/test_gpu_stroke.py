"""Strokes on a device-resident texture (dtp_stroke, `paint_stroke`): the gather and paste kernels bit for bit against the torch
restatement of the Kit app's loop (tests/stroke_ref.py), a serial stroke against the host loop over generate_u8 byte for byte, a grouped
stroke against the host loop that issues the same batches, enqueue without a host wait, and the refusals, which leave the texture alone.
One 64^2 context, max_batch 2, DDIM, 4 steps; a 96 x 160 texture of seeded random bytes."""
import re
import time

import pytest
import torch

import stroke_ref
from stroke_ref import ERASE, INPAINT, OVERPAINT

pytestmark = pytest.mark.gpu

R = 64
H, W = 96, 160
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
OVER = (10, 25)  # the Kit app's overpaint margins (manager.py:37)
DEV = "cuda:0"


def make_texture(h, w, seed):
    """Seeded random RGBA bytes with an alpha-0 (unknown) and an alpha-255 (known) region."""
    t = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    t[h // 4: h // 2, w // 8: w // 2, 3] = 0
    t[h // 2:, w // 2:, 3] = 255
    t[: h // 8, :, 3] = 0
    return t


@pytest.fixture(scope="module")
def texture():
    return make_texture(H, W, 77)


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import synthetic, weights as Wt
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    sd = dict(unet=Wt.synthetic_unet(5), lora=Wt.synthetic_lora(5), vae=Wt.synthetic_vae(5), clip=Wt.synthetic_clip(5),
              penc=Wt.synthetic_patch_encoder(5))
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=2)
    for slot in range(2):
        _, brush, _, _ = synthetic.make_stamp_batch(1, R, 6000 + slot)
        cond, uncond = synthetic.make_conditioning(6100 + slot)
        m.set_conditioning(cond, uncond, brush, slot=slot)
    return m


# ---------------------------------------------------------------- op level
# name: (texture size, windows [(x, y, mode)] -- the two are disjoint, B = 1 takes the first --, wrap, mask)
SQUARE, DISC = "square", "disc"
CASES = {
    "inside": ((H, W), [(10, 5, INPAINT), (80, 20, INPAINT)], False, SQUARE),
    "inside_flush_with_the_far_corner": ((H, W), [(W - R, H - R, INPAINT), (0, 0, INPAINT)], False, SQUARE),
    "wrap_over_both_borders": ((H, W), [(140, 70, INPAINT), (76, 70, INPAINT)], True, SQUARE),
    "wrap_from_negative_and_far_coordinates": ((H, W), [(-20 - 3 * W, -9, INPAINT), (50 + 2 * W, -9 + 5 * H, INPAINT)], True, SQUARE),
    "partly_outside_negative_x_and_y": ((H, W), [(-13, -7, INPAINT), (110, 40, INPAINT)], False, SQUARE),  # the second: x + R > W, y + R > H
    "overpaint": ((H, W), [(10, 5, OVERPAINT), (80, 20, INPAINT)], False, SQUARE),
    "overpaint_wrapped": ((H, W), [(140, 70, OVERPAINT), (76, 70, OVERPAINT)], True, SQUARE),
    "erase": ((H, W), [(10, 5, ERASE), (80, 20, ERASE)], False, SQUARE),
    "erase_next_to_inpaint_partly_outside": ((H, W), [(-13, 50, ERASE), (110, -30, INPAINT)], False, DISC),
    "disc_mask": ((H, W), [(10, 5, INPAINT), (80, 20, OVERPAINT)], False, DISC),
    "disc_mask_wrapped": ((H, W), [(140, 70, INPAINT), (76, 70, ERASE)], True, DISC),
    "texture_136x200": ((136, 200), [(150, 100, INPAINT), (20, 100, OVERPAINT)], True, DISC),
    "texture_136x200_clipped": ((136, 200), [(150, 100, INPAINT), (-30, -30, INPAINT)], False, SQUARE),
}


def _mask(kind):
    return stroke_ref.disc_mask(R) if kind == DISC else stroke_ref.make_stamp_mask(R, 3)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_gather_and_paste_kernels_match_the_restatement(case, B):
    from diffusiontexturepainting_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    (h, w), wins, wrap, kind = CASES[case]
    wins = wins[:B]
    tex = make_texture(h, w, 1000 + h)
    xs, ys, modes = [p[0] for p in wins], [p[1] for p in wins], [p[2] for p in wins]
    # gather
    got = ops.stroke_gather(tex.to(DEV), xs, ys, R, modes=modes, wrap=wrap, over_y=OVER[0], over_x=OVER[1]).cpu()
    want = torch.cat([stroke_ref.gather(tex, x, y, R, wrap, m, OVER) for x, y, m in wins])
    assert got.shape == (B, 4, R, R) and torch.equal(got, want)
    # paste: a decoder output that leaves [-1, 1] on both sides (the clamp) and hits the ends exactly
    dec = torch.randn(B, R, R, 4, generator=torch.Generator().manual_seed(5)) * 0.9
    dec[:, 0, :8, :] = torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, 1.0 - 2.0 ** -23, -1.0 + 2.0 ** -23, 255.0 / 256])[None, :, None]
    mask = _mask(kind)
    dtex = tex.to(DEV)
    all_erase = all(m == ERASE for m in modes)
    out = ops.stroke_paste(None if all_erase else dec.to(DEV), mask.to(DEV), dtex, xs, ys, modes=modes, wrap=wrap)
    assert out.data_ptr() == dtex.data_ptr()
    out = out.cpu()
    want, fp = tex.clone(), torch.zeros(h, w, dtype=torch.bool)
    for b, (x, y, m) in enumerate(wins):
        stroke_ref.paste(want, stroke_ref.decoded_to_u8(dec[b]), mask, x, y, wrap, m)
        fp |= stroke_ref.footprint(h, w, x, y, mask, wrap)
    assert torch.equal(out, want)
    assert 0 < int(fp.sum()) < h * w
    assert torch.equal(out[~fp], tex[~fp])  # texels outside the mask: bit-unchanged against the copy
    painted = out[fp]
    if all_erase:
        assert int(painted.sum()) == 0
    elif ERASE not in modes:
        assert bool((painted[:, 3] == 255).all())


def test_op_refusals():
    from diffusiontexturepainting_amd import ops
    from diffusiontexturepainting_amd._lib import DtpError
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    tex = make_texture(H, W, 3).to(DEV)
    with pytest.raises(DtpError, match=r"code 1"):
        ops.stroke_gather(tex[:32].contiguous(), [0], [0], R)  # H < R
    with pytest.raises(DtpError, match=r"code 1.*window 0"):
        ops.stroke_gather(tex, [0], [0], R, modes=[5])
    with pytest.raises(DtpError, match=r"code 1.*Overpaint"):
        ops.stroke_gather(tex, [0], [0], R, modes=[OVERPAINT], over_y=0, over_x=25)
    with pytest.raises(DtpError, match=r"code 1.*not an Erase"):
        ops.stroke_paste(None, stroke_ref.make_stamp_mask(R, 0).to(DEV), tex, [0], [0], modes=[INPAINT])


# ---------------------------------------------------------------- strokes against the host loop
def host_stroke(model, tex, positions, seeds, modes, mask, wrap, groups=None, slots=None):
    """The Kit manager's loop (manager.py:232-271) on the host, one generate_u8 call per group (default: per stamp)."""
    tex = tex.clone()
    n = len(positions)
    groups = groups if groups is not None else list(range(n))
    for g in sorted(set(groups)):
        members = [i for i in range(n) if groups[i] == g]
        if modes[members[0]] == ERASE:
            (i,) = members
            stroke_ref.paste(tex, None, mask, *positions[i], wrap, ERASE)
            continue
        canvas = torch.cat([stroke_ref.gather(tex, *positions[i], R, wrap, modes[i], OVER) for i in members])
        painted = model.generate_u8(canvas, composite=False, seeds=[seeds[i] for i in members],
                                    slots=[slots[i] for i in members] if slots else None, **ST).cpu()
        for b, i in enumerate(members):
            stroke_ref.paste(tex, painted[b], mask, *positions[i], wrap, modes[i])
    return tex


def test_serial_stroke_equals_the_host_loop(model, texture):
    # overlapping the previous one; over the right edge; over the bottom edge, Overpaint; Erase; over both edges, another brush
    positions = [(8, 4), (40, 20), (130, 10), (20, 60), (50, 30), (120, 50)]
    modes = [INPAINT, INPAINT, INPAINT, OVERPAINT, ERASE, INPAINT]
    slots = [0, 0, 1, 0, 0, 1]
    seeds = [900 + i for i in range(6)]
    mask = stroke_ref.make_stamp_mask(R, 4)
    tex = texture.to(DEV)
    out = model.paint_stroke(tex, positions, seeds=900, modes=["inpaint", "inpaint", 0, "overpaint", "erase", INPAINT], slots=slots,
                             wrap=True, margin=4, overpaint_margins=OVER, **ST)
    assert out is tex
    assert model.stroke_info() == dict(stamps=6, groups=6, unet_evals=5 * 3)  # DDIM, 4 steps: 3 evaluations; the Erase stamp runs none
    want = host_stroke(model, texture, positions, seeds, modes, mask, True, slots=slots)
    assert torch.equal(out.cpu(), want)
    assert not torch.equal(want, texture)
    # the stroke is a function of its arguments: again, on a fresh copy
    again = model.paint_stroke(texture.to(DEV), positions, seeds=seeds, modes=modes, slots=slots, wrap=True, margin=4, **ST)
    assert torch.equal(again.cpu(), want)


def test_serial_stroke_without_wrap_and_with_a_mask(model, texture):
    positions = [(-20, -10), (120, 50), (100, 40)]  # partly outside at the top left / the bottom right; overlapping the previous one
    modes = [INPAINT, OVERPAINT, INPAINT]
    seeds = [5, 1 << 63, 77]
    mask = stroke_ref.disc_mask(R)
    out = model.paint_stroke(texture.to(DEV), positions, seeds=seeds, modes=modes, mask=mask, **ST).cpu()
    want = host_stroke(model, texture, positions, seeds, modes, mask, False)
    assert torch.equal(out, want)
    fp = torch.zeros(H, W, dtype=torch.bool)
    for x, y in positions:
        fp |= stroke_ref.footprint(H, W, x, y, mask, False)
    assert torch.equal(out[~fp], texture[~fp]) and not torch.equal(out[fp], texture[fp])


def test_grouped_stroke_equals_the_host_loop_of_the_same_batches(model, texture):
    positions = [(0, 0), (64, 0), (32, 0), (96, 16)]
    seeds = [40, 41, 42, 43]
    groups = model.plan_stroke(positions, H, W, max_group=2)
    assert groups == [0, 0, 1, 1]
    assert groups == stroke_ref.plan(H, W, R, False, [(x, y, INPAINT) for x, y in positions], 2)
    assert model.plan_stroke(positions, H, W, max_group=8) == groups  # max_batch = 2 bounds the groups
    mask = stroke_ref.make_stamp_mask(R, 0)
    runs = [model.paint_stroke(texture.to(DEV), positions, seeds=seeds, max_group=2, **ST).cpu() for _ in range(2)]
    assert model.stroke_info() == dict(stamps=4, groups=2, unet_evals=2 * 3)
    assert model.stamp_unet_rows() == 2 * (2 * 2 + 2) + (2 * 2)  # the last group: one B = 2 stamp, tg for 2 of its 3 evaluations
    want = host_stroke(model, texture, positions, seeds, [INPAINT] * 4, mask, False, groups=groups)
    assert torch.equal(runs[0], want)
    assert torch.equal(runs[0], runs[1])
    # max_group is a throughput knob with a visible meaning: the serial stroke differs (B = 1 stamps; and 32,0 sees 0,0 AND 64,0 pasted)
    serial = model.paint_stroke(texture.to(DEV), positions, seeds=seeds, max_group=1, **ST).cpu()
    assert torch.equal(serial, host_stroke(model, texture, positions, seeds, [INPAINT] * 4, mask, False))


def test_stroke_enqueue_does_not_block_the_host(model, texture):
    """The criterion of test_stamp_enqueue_does_not_block_the_host: the host is back long before the device is done."""
    positions = [(8, 4), (40, 20), (130, 10), (20, 60), (50, 30), (90, 0)]
    tex = texture.to(DEV)
    for _ in range(2):  # programs, graphs and the mask exist from here on
        model.paint_stroke(tex, positions, seeds=1, wrap=True, **ST)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.paint_stroke(tex, positions, seeds=1, wrap=True, **ST)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f"host enqueue of a 6-stamp stroke {t_host * 1e3:.1f} ms, device done after {t_all * 1e3:.1f} ms")
    assert t_host < 0.5 * t_all


def test_refusals_leave_the_texture_alone(model, texture):
    from diffusiontexturepainting_amd._lib import DtpError
    pos = [(0, 0), (70, 0), (10, 20), (90, 30), (5, 5)]
    tex = texture.to(DEV)

    def refused(code, pattern, t=None, **kw):
        t = tex if t is None else t
        before = t.clone()
        with pytest.raises(DtpError) as e:
            model.paint_stroke(t, kw.pop("positions", pos), seeds=3, **kw, **ST)
        torch.cuda.synchronize()
        assert re.search(rf"\(code {code}\)", str(e.value)) and re.search(pattern, str(e.value)), str(e.value)
        assert torch.equal(t, before)

    refused(3, r"stamp 3\b.*slot 5", slots=[0, 0, 0, 5, 0])                       # an unset slot in stamp 3: DTP_ERR_STATE, as dtp_stamp_seeded
    refused(1, r"slot 16 of stamp 2\b", slots=[0, 0, 16, 0, 0])
    refused(1, r"smaller", t=tex[:32].contiguous())                               # H < R
    refused(1, r"smaller", t=tex[:, :40].contiguous())                            # W < R
    refused(1, r"stamp 1\b.*mode 7", modes=[0, 7, 0, 0, 0])                       # a bad mode
    refused(1, r"stamp 4\b.*outside", positions=pos[:4] + [(W, 0)])               # a window wholly outside
    refused(1, r"stamp 0\b.*outside", positions=[(0, -R)] + pos[1:])
    refused(1, r"stamp 2\b.*Overpaint", modes=[0, 0, 2, 0, 0], overpaint_margins=(32, 25))
    refused(1, r"margin=32", margin=32)
    refused(1, r"margin=-1", margin=-1)
    with pytest.raises(ValueError, match="strength"):
        model.paint_stroke(tex, pos, strength=0.0, **ST)
    with pytest.raises(ValueError, match="uint8"):
        model.paint_stroke(tex.float(), pos, **ST)
    with pytest.raises(ValueError, match="uint8"):
        model.paint_stroke(tex[:, :100], pos, **ST)  # not contiguous: it could not be painted in place
    # the same windows are fine with wrap, and an Erase stamp needs no slot
    model.paint_stroke(tex.clone(), pos[:4] + [(W, 0)], seeds=3, wrap=True, modes=[0, 0, 0, "erase", 0], slots=[0, 0, 0, 5, 0], **ST)
    torch.cuda.synchronize()


def test_strength_below_one_runs_through_the_stroke(model, texture):
    """strength < 1 stages the init image from the gathered canvas: again the host loop, with generate_u8(strength=...)."""
    positions, seeds = [(100, 40), (130, 60)], [11, 12]
    mask = stroke_ref.make_stamp_mask(R, 0)
    out = model.paint_stroke(texture.to(DEV), positions, seeds=seeds, wrap=True, strength=0.5, **ST).cpu()
    assert model.stroke_info()["unet_evals"] == 2 * 2
    want = texture.clone()
    for (x, y), seed in zip(positions, seeds):
        canvas = stroke_ref.gather(want, x, y, R, True)
        stroke_ref.paste(want, model.generate_u8(canvas, composite=False, seeds=[seed], strength=0.5, **ST)[0].cpu(), mask, x, y, True)
    assert torch.equal(out, want)
