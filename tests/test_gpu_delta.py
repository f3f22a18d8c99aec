"""The changed tiles of a device image (dtp_delta_*, `model.delta_tracker`; include/dtp.h "changed tiles of an image") against the numpy
restatement of the contract (tests/delta_ref.py): key frames, single bytes, random tile sets across every workgroup border of the
passes, capped scans that continue, changes made back, an unaligned image, two trackers, painting with the journal, a view, and the
device outputs.  Every comparison is torch.equal or np.array_equal: the tracker moves bytes.  One 64^2 context (max_batch 2), DDIM,
4 steps, as tests/test_gpu_journal.py."""
import numpy as np
import pytest
import torch

import delta_ref
import journal_ref

pytestmark = pytest.mark.gpu

R = 64
ST = dict(steps=4, tg_steps=2, cfg_weight=2.5, context_pad=9)
OVER = (10, 25)
DEV = "cuda:0"
# 2048 x 2064: 128 x 129 = 16 512 tiles, 258 workgroups in the flag and gather passes, more than one wave of the scan
SIZES = [(1, 1), (16, 16), (17, 33), (90, 150), (96, 160), (2048, 2064)]
ids_of = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def random_image(h, w, seed):
    return torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffusiontexturepainting_amd import synthetic, weights as Wt
    from diffusiontexturepainting_amd.inpainter import MI355ConditionalInpainter
    sd = dict(unet=Wt.synthetic_unet(5), lora=Wt.synthetic_lora(5), vae=Wt.synthetic_vae(5), clip=Wt.synthetic_clip(5),
              penc=Wt.synthetic_patch_encoder(5))
    m = MI355ConditionalInpainter(R, device=0, weights=sd, max_batch=2)
    _, brush, _, _ = synthetic.make_stamp_batch(1, R, 6000)
    cond, uncond = synthetic.make_conditioning(6100)
    m.set_conditioning(cond, uncond, brush, slot=0)
    return m


@pytest.fixture(scope="module")
def mesh(model):
    from diffusiontexturepainting_amd import synthetic
    return model.load_mesh(*synthetic.make_height_field(17, 13, seed=3))


def pull_copy(tracker, image, **kw):
    """pull() with the views copied: (ids list, tiles numpy, remaining)."""
    ids, tiles, remaining = tracker.pull(image, **kw)
    if isinstance(ids, torch.Tensor):
        ids, tiles = ids.cpu().numpy(), tiles.cpu().numpy()
    return ids.tolist(), np.array(tiles, copy=True), remaining


def apply_tiles(mirror, ids, tiles):
    from diffusiontexturepainting_amd import delta
    h, w = mirror.shape[:2]
    delta.apply_frame(mirror, delta.encode_frame(h, w, 0, ids, tiles))


def change_tiles(img, tiles, rng):
    """One byte inside the image of every tile of `tiles` takes another value (numpy image, in place)."""
    h, w = img.shape[:2]
    for t in tiles:
        r0, c0, rows, cols = delta_ref.tile_box(h, w, int(t))
        img[r0 + rng.integers(rows), c0 + rng.integers(cols), rng.integers(4)] ^= np.uint8(1 + rng.integers(255))


# ---------------------------------------------------------------- 1. the key frame
@pytest.mark.parametrize("size", SIZES, ids=ids_of)
def test_key_frame_then_nothing(model, size):
    from diffusiontexturepainting_amd import delta
    h, w = size
    n = journal_ref.tile_count(h, w)
    host = random_image(h, w, 1)
    img = host.to(DEV)
    t = model.delta_tracker(img)
    assert (t.H, t.W, t.capacity_tiles) == (h, w, n)
    f = delta.decode_frame(t.frame(img))
    assert (f["H"], f["W"], f["seq"], f["first"], f["remaining"]) == (h, w, 0, True, 0)
    assert f["ids"].tolist() == list(range(n))  # every tile, in order
    ref = delta_ref.Tracker(h, w)
    want_ids, want_tiles, want_counts = ref.scan(host.numpy())
    assert want_counts == [n, 0] and np.array_equal(f["tiles"], want_tiles)  # texels outside the image are zero
    mirror = np.zeros((h, w, 4), np.uint8)
    apply_tiles(mirror, f["ids"], f["tiles"])
    assert np.array_equal(mirror, host.numpy())
    # a second pull emits nothing and leaves ids and tiles as they were, on the host and on the device
    dev_ids, dev_tiles, _ = (v.clone() for v in t._device_views())
    f2 = delta.decode_frame(t.frame(img))
    assert (f2["seq"], f2["first"], f2["remaining"], f2["ids"].size) == (1, False, 0, 0)
    assert t._host_ids.tolist() == list(range(n)) and np.array_equal(t._host_tiles, want_tiles)
    now_ids, now_tiles, counts = t._device_views()
    assert torch.equal(now_ids, dev_ids) and torch.equal(now_tiles, dev_tiles) and counts.tolist() == [0, 0]
    assert dev_ids.tolist() == list(range(n)) and np.array_equal(dev_tiles.cpu().numpy(), want_tiles)
    t.close()


# ---------------------------------------------------------------- 2. one byte
@pytest.mark.parametrize("size", SIZES, ids=ids_of)
def test_one_byte_emits_exactly_its_tile(model, size):
    h, w = size
    tx = journal_ref.tiles_x(w)
    img = random_image(h, w, 2).to(DEV)
    t = model.delta_tracker((h, w))
    assert len(t.pull(img)[0]) == journal_ref.tile_count(h, w)
    # the red byte of texel (0, 0); an alpha byte alone; the last texel inside the first row's last tile (partial where W % 16 != 0);
    # the image's last texel
    for r, c, ch in [(0, 0, 0), (h // 2, w // 2, 3), (min(15, h - 1), w - 1, 1), (h - 1, w - 1, 2)]:
        img[r, c, ch] ^= 0x40
        ids, tiles, remaining = pull_copy(t, img)
        assert ids == [(r // 16) * tx + c // 16] and remaining == 0, (r, c, ch)
        assert np.array_equal(tiles[0], delta_ref.payload(img.cpu().numpy(), ids[0]))
        assert pull_copy(t, img)[0] == []
    t.close()


# ---------------------------------------------------------------- 3. random tile sets, against the restatement's whole state
@pytest.mark.parametrize("size", SIZES, ids=ids_of)
def test_random_tile_sets_ids_payload_counts_and_shadow(model, size):
    from diffusiontexturepainting_amd import ops
    h, w = size
    n = journal_ref.tile_count(h, w)
    rng = np.random.default_rng(h * 7 + w)
    host = random_image(h, w, 3).numpy().copy()
    t = model.delta_tracker((h, w))
    ref = delta_ref.Tracker(h, w)
    # the tiles on both sides of every border between two workgroups of the flag and gather passes (64 tiles each; the scan's threads
    # take one group each up to 1024 groups, so these are its borders too)
    borders = [b for g in range(delta_ref.GROUP, n, delta_ref.GROUP) for b in (g - 1, g)]
    sets = [None, [int(rng.integers(n))], sorted(set(rng.choice(n, max(n // 100, 1), replace=False).tolist() + borders)),
            np.flatnonzero(rng.random(n) < 0.5).tolist(), list(range(n))]
    for k, tiles_to_change in enumerate(sets):  # the first scan is the key frame
        if tiles_to_change is not None:
            change_tiles(host, tiles_to_change, rng)
        img = torch.from_numpy(host).to(DEV)
        ids, tiles, counts, shadow, stale = ops.delta_scan(t, img)
        want_ids, want_tiles, want_counts = ref.scan(host)
        if tiles_to_change is not None:
            assert want_ids.tolist() == sorted(tiles_to_change), k
        assert counts == want_counts, k
        assert np.array_equal(ids.numpy(), want_ids), k
        assert np.array_equal(tiles.numpy(), want_tiles), k
        assert np.array_equal(shadow.numpy(), ref.shadow) and np.array_equal(stale.numpy(), ref.stale), k
    t.close()


def test_more_groups_than_the_scan_has_threads(model):
    """1040 x 16384: 65 x 1024 = 66 560 tiles in 1040 groups, so the scan's 1024 threads take runs of two groups each and the last 504
    threads none.  The ids of a key frame and of a set with tiles on both sides of every border between two runs must be the ascending
    lists, each payload the image's tile: a wrong base anywhere shifts everything behind it."""
    h, w = 1040, 16384
    n = journal_ref.tile_count(h, w)
    assert n == 66560 and -(-n // delta_ref.GROUP) == 1040
    rng = np.random.default_rng(12)
    img = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=DEV)
    t = model.delta_tracker(img)
    ids, tiles, remaining = t.pull(img, device=True)
    assert remaining == 0 and torch.equal(ids.cpu(), torch.arange(n, dtype=torch.int32))
    def tiles_of(image):  # every tile is whole at this size
        return image.view(65, 16, 1024, 16, 4).permute(0, 2, 1, 3, 4).reshape(n, 16, 16, 4)

    assert torch.equal(tiles, tiles_of(img))
    run = 2 * delta_ref.GROUP  # tiles per thread of the scan
    changed = sorted(set(rng.choice(n, 300, replace=False).tolist() + [b for g in range(run, n, run) for b in (g - 1, g)]))
    rows = torch.tensor([(c // 1024) * 16 + 3 for c in changed], device=DEV)
    cols = torch.tensor([(c % 1024) * 16 + 5 for c in changed], device=DEV)
    img[rows, cols, 2] ^= 0x11
    ids, tiles, remaining = t.pull(img, device=True)
    assert remaining == 0 and ids.tolist() == changed
    assert torch.equal(tiles, tiles_of(img)[torch.tensor(changed, device=DEV)])
    assert t.pull(img, device=True)[0].numel() == 0
    t.close()


# ---------------------------------------------------------------- 4. capped scans
def test_capacity_seven_against_forty_changed_tiles(model):
    h, w = 90, 150
    rng = np.random.default_rng(4)
    host = random_image(h, w, 4).numpy().copy()
    t = model.delta_tracker((h, w), capacity_tiles=7)
    ref = delta_ref.Tracker(h, w, capacity=7)
    mirror = np.zeros((h, w, 4), np.uint8)
    img = torch.from_numpy(host).to(DEV)

    def pull():
        ids, tiles, remaining = pull_copy(t, img)
        want_ids, want_tiles, want_counts = ref.scan(host)
        assert ids == want_ids.tolist() and np.array_equal(tiles, want_tiles) and remaining == want_counts[1]
        apply_tiles(mirror, ids, tiles)
        return ids, remaining

    # the key frame in runs of 7: 60 tiles, consecutive, remaining counts down
    got, left = [], 60
    while True:
        ids, remaining = pull()
        got += ids
        left -= len(ids)
        assert remaining == left
        if remaining == 0:
            break
    assert got == list(range(60)) and np.array_equal(mirror, host)
    # 40 changed tiles: successive pulls give consecutive runs of the ascending list
    changed = sorted(rng.choice(60, 40, replace=False).tolist())
    change_tiles(host, changed, rng)
    img = torch.from_numpy(host).to(DEV)
    first, remaining = pull()
    assert first == changed[:7] and remaining == 33
    second, remaining = pull()
    assert second == changed[7:14] and remaining == 26
    # a tile that was emitted already is changed again between two pulls: it is emitted again
    change_tiles(host, [changed[2]], rng)
    img = torch.from_numpy(host).to(DEV)
    third, remaining = pull()
    assert third == [changed[2]] + changed[14:20] and remaining == 20
    rest = []
    while remaining:
        ids, remaining = pull()
        rest += ids
    assert rest == changed[20:] and np.array_equal(mirror, host)
    assert pull() == ([], 0)
    t.close()


def test_capacity_one(model):
    h, w = 17, 33
    host = random_image(h, w, 5).numpy().copy()
    img = torch.from_numpy(host).to(DEV)
    t = model.delta_tracker(img, capacity_tiles=1)
    mirror = np.zeros((h, w, 4), np.uint8)
    for k in range(6):
        ids, tiles, remaining = pull_copy(t, img)
        assert ids == [k] and remaining == 5 - k
        apply_tiles(mirror, ids, tiles)
    assert np.array_equal(mirror, host) and pull_copy(t, img)[0] == []
    img[16, 32, 0] ^= 1  # the corner tile and the first
    img[0, 0, 3] ^= 1
    assert pull_copy(t, img)[0::2] == ([0], 1) and pull_copy(t, img)[0::2] == ([5], 0) and pull_copy(t, img)[0::2] == ([], 0)
    t.close()


# ---------------------------------------------------------------- 5. change and change back; reset
@pytest.mark.parametrize("size", [(90, 150), (2048, 2064)], ids=ids_of)
def test_a_change_made_back_costs_nothing_and_reset_sends_everything(model, size):
    from diffusiontexturepainting_amd import delta
    h, w = size
    n = journal_ref.tile_count(h, w)
    img = random_image(h, w, 6).to(DEV)
    t = model.delta_tracker(img)
    assert len(t.pull(img)[0]) == n
    old = img[h - 3, w - 2].clone()
    img[h - 3, w - 2] = old ^ 0xFF
    img[h - 3, w - 2] = old
    assert pull_copy(t, img)[0::2] == ([], 0)
    t.reset()
    f = delta.decode_frame(t.frame(img))
    assert f["first"] and f["ids"].tolist() == list(range(n)) and f["remaining"] == 0
    assert np.array_equal(f["tiles"], delta_ref.Tracker(h, w).scan(img.cpu().numpy())[1])
    assert not delta.decode_frame(t.frame(img))["first"]
    t.close()


# ---------------------------------------------------------------- 6. an image that is 4-byte aligned and no more
@pytest.mark.parametrize("size", [(17, 33), (90, 150)], ids=ids_of)
def test_an_image_four_bytes_into_a_buffer(model, size):
    h, w = size
    rng = np.random.default_rng(6)
    host = random_image(h, w, 7).numpy().copy()
    buf = torch.zeros(h * w * 4 + 4, dtype=torch.uint8, device=DEV)
    off = buf[4:].view(h, w, 4)
    assert off.data_ptr() % 8 == 4 and off.is_contiguous()
    ta, tb = model.delta_tracker((h, w)), model.delta_tracker((h, w))
    for changed in (None, [0, journal_ref.tile_count(h, w) - 1], [1, 2, 4]):
        if changed:
            change_tiles(host, changed, rng)
        aligned = torch.from_numpy(host).to(DEV)
        off.copy_(aligned)
        a, b = pull_copy(ta, aligned), pull_copy(tb, off)
        assert a[0] == b[0] == (changed or list(range(journal_ref.tile_count(h, w)))) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0
    assert buf[:4].tolist() == [0, 0, 0, 0]
    ta.close(); tb.close()


# ---------------------------------------------------------------- 7. two trackers; another shape
def test_two_trackers_are_independent_and_another_shape_is_refused(model):
    from diffusiontexturepainting_amd._lib import DtpError
    h, w = 96, 160
    img = random_image(h, w, 8).to(DEV)
    a, b = model.delta_tracker(img), model.delta_tracker(img, capacity_tiles=60)
    assert len(a.pull(img)[0]) == 60
    img[40, 40, 1] ^= 1
    assert pull_copy(a, img)[0] == [2 * 10 + 2]
    assert pull_copy(b, img)[0] == list(range(60))  # b had not seen the image at all
    img[95, 159, 0] ^= 1
    assert pull_copy(b, img)[0] == [59] and pull_copy(a, img)[0] == [59] and pull_copy(a, img)[0] == []
    # an image of another shape: refused, the outputs untouched
    host_before = (a._host_ids.copy(), a._host_tiles.copy())
    dev_before = [v.clone() for v in a._device_views()]
    for other in (torch.zeros(160, 96, 4, dtype=torch.uint8, device=DEV), torch.zeros(96, 161, 4, dtype=torch.uint8, device=DEV)):
        for kw in (dict(), dict(device=True)):
            with pytest.raises(DtpError, match="the tracker was created for 96 x 160"):
                a.pull(other, **kw)
    with pytest.raises(ValueError, match="contiguous uint8"):
        a.pull(img.cpu())
    assert np.array_equal(a._host_ids, host_before[0]) and np.array_equal(a._host_tiles, host_before[1])
    assert all(torch.equal(x, y) for x, y in zip(a._device_views(), dev_before))
    assert pull_copy(a, img)[0] == []  # and its state too
    a.close(); b.close()
    with pytest.raises(DtpError, match="closed"):
        a.pull(img)


# ---------------------------------------------------------------- 8. painting and the journal
def test_strokes_undo_and_redo_reach_the_mirror(model, mesh):
    from diffusiontexturepainting_amd import delta
    h, w = 90, 150
    tex = random_image(h, w, 9).to(DEV)
    j = model.journal(tex)
    t = model.delta_tracker(tex)
    mirror = np.zeros((h, w, 4), np.uint8)
    seq = [None]

    def step():
        """The pulled frame applied to the mirror gives texture.cpu() -> the emitted ids."""
        b = t.frame(tex)
        s, remaining = delta.apply_frame(mirror, b, expect_seq=seq[0])
        seq[0] = s + 1
        assert remaining == 0 and np.array_equal(mirror, tex.cpu().numpy())
        return set(delta.decode_frame(b)["ids"].tolist())

    assert step() == set(range(60))
    with j.stroke():  # wrapped across the border
        model.paint_stroke(tex, [(130, 60), (-10, -10)], seeds=40, modes=["inpaint", "overpaint"], wrap=True, overpaint_margins=OVER, **ST)
    painted = step()
    assert painted and painted <= set(j.tiles(0))  # the saved set bounds the written set
    with j.stroke():
        model.paint_mesh_stroke(mesh, tex, [(0.1, -0.05, 0.1), (0.3, 0.05, 0.1)], [(0.35, -0.2, 0.9), (0.0, 0.0, 1.0)],
                                [(0.0, 0.3, 0.15), (0.1, -0.05, 0.1)], [0.45, 0.4], seeds=700, modes=["inpaint", "overpaint"],
                                overpaint_margins=OVER, bleed=3, **ST)
    saved = set(j.tiles(1))
    meshed = step()
    assert meshed and meshed <= saved and len(saved) < 60
    assert j.undo()
    undone = step()
    assert undone and undone <= saved  # at most the tiles of the same record
    assert undone == meshed            # exactly the tiles the stroke changed come back
    assert j.redo()
    assert step() == meshed
    assert j.undo() and j.undo()
    assert step() == painted | meshed
    assert step() == set()
    t.close(); j.close()


# ---------------------------------------------------------------- 9. a view
def test_a_view_and_a_camera_step(model, mesh):
    from diffusiontexturepainting_amd import delta
    from diffusiontexturepainting_amd.mesh import view_camera
    H, W = 90, 150
    tex = random_image(96, 160, 10).to(DEV)
    tex[..., 3] = 255
    frame = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
    t = model.delta_tracker(frame)
    mirror = np.zeros((H, W, 4), np.uint8)
    counts = []
    for eye in ((0.0, 0.0, 4.0), (0.03, 0.0, 4.0)):
        model.render_view(mesh, tex, view_camera(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, (H, W), 0.05), out=frame)
        b = t.frame(frame, on="view")
        delta.apply_frame(mirror, b)
        torch.cuda.synchronize()
        assert np.array_equal(mirror, frame.cpu().numpy())
        counts.append(delta.decode_frame(b)["ids"].size)
    assert counts[0] == 60 and 0 < counts[1] < 60  # the background's tiles stay at home
    assert (mirror[..., 3] == 255).any() and (mirror[..., 3] == 0).any()
    t.close()


# ---------------------------------------------------------------- 10. the device outputs
@pytest.mark.parametrize("size", [(90, 150), (2048, 2064)], ids=ids_of)
def test_device_pull_gives_the_host_pulls_bytes(model, size):
    h, w = size
    rng = np.random.default_rng(10)
    host = random_image(h, w, 11).numpy().copy()
    a, b = model.delta_tracker((h, w)), model.delta_tracker((h, w))
    for changed in (None, sorted(rng.choice(journal_ref.tile_count(h, w), 9, replace=False).tolist())):
        if changed:
            change_tiles(host, changed, rng)
        img = torch.from_numpy(host).to(DEV)
        ids, tiles, remaining = b.pull(img, device=True)
        assert ids.device == img.device and ids.dtype == torch.int32 and tiles.dtype == torch.uint8 and tuple(tiles.shape[1:]) == (16, 16, 4)
        want = pull_copy(a, img)
        assert ids.tolist() == want[0] == (changed or list(range(journal_ref.tile_count(h, w))))
        assert np.array_equal(tiles.cpu().numpy(), want[1]) and remaining == want[2] == 0
    a.close(); b.close()
