"""The contract of the changed tiles of an image (include/dtp.h: "changed tiles of an image") restated in numpy and plain
Python: the layout of what a tracker owns, a scan over arrays, and the wire frame's codec written from the header text of
diffusiontexturepainting_amd/delta.py.  The tiles and their numbers are the journal's (tests/journal_ref.py)."""
import struct

import numpy as np

import journal_ref

TILE = 16
TILE_BYTES = 1024
GROUP = 64  # tiles per workgroup of the flag and gather passes
MAX_SIDE = 16384


def layout(H, W, capacity=None):
    """What dtp_delta_layout answers."""
    n = journal_ref.tile_count(H, W)
    cap = n if capacity is None else capacity
    groups = -(-n // GROUP)
    ids_bytes = 4 * cap
    host_tiles_offset = 16 + -(-ids_bytes // 16) * 16
    return dict(tiles_x=journal_ref.tiles_x(W), tiles_y=journal_ref.tiles_x(H), n_tiles=n, n_groups=groups, capacity=cap,
                shadow_bytes=H * W * 4, stale_bytes=n, flag_bytes=n, group_bytes=8 * groups, ids_bytes=ids_bytes,
                tiles_bytes=cap * TILE_BYTES, counts_bytes=8, host_ids_offset=16, host_tiles_offset=host_tiles_offset,
                host_bytes=host_tiles_offset + cap * TILE_BYTES)


def tile_box(H, W, t):
    """(r0, c0, rows, cols): the texels of tile t inside the image."""
    tx = journal_ref.tiles_x(W)
    r0, c0 = (t // tx) * TILE, (t % tx) * TILE
    return r0, c0, min(TILE, H - r0), min(TILE, W - c0)


def changed_tiles(image, shadow, stale):
    """The ascending list of changed tiles: stale, or a byte inside the image differs from the shadow."""
    H, W = image.shape[:2]
    out = []
    for t in range(journal_ref.tile_count(H, W)):
        r0, c0, rows, cols = tile_box(H, W, t)
        if stale[t] or not np.array_equal(image[r0:r0 + rows, c0:c0 + cols], shadow[r0:r0 + rows, c0:c0 + cols]):
            out.append(t)
    return out


def payload(image, t):
    H, W = image.shape[:2]
    r0, c0, rows, cols = tile_box(H, W, t)
    p = np.zeros((TILE, TILE, 4), np.uint8)
    p[:rows, :cols] = image[r0:r0 + rows, c0:c0 + cols]
    return p


def scan(image, shadow, stale, capacity):
    """image, shadow uint8 [H, W, 4], stale uint8 [n_tiles], capacity -> (ids, tiles, counts, new shadow, new stale); the inputs are
    not changed."""
    H, W = image.shape[:2]
    changed = changed_tiles(image, shadow, stale)
    emit = changed[:capacity]
    shadow, stale = shadow.copy(), stale.copy()
    tiles = np.zeros((len(emit), TILE, TILE, 4), np.uint8)
    for k, t in enumerate(emit):
        tiles[k] = payload(image, t)
        r0, c0, rows, cols = tile_box(H, W, t)
        shadow[r0:r0 + rows, c0:c0 + cols] = image[r0:r0 + rows, c0:c0 + cols]
        stale[t] = 0
    return np.array(emit, np.int32), tiles, [len(emit), len(changed) - len(emit)], shadow, stale


class Tracker:
    """The state of a tracker: a zero shadow and every tile stale."""

    def __init__(self, H, W, capacity=None):
        self.H, self.W = H, W
        self.capacity = journal_ref.tile_count(H, W) if capacity is None else capacity
        self.shadow = np.zeros((H, W, 4), np.uint8)
        self.stale = np.ones(journal_ref.tile_count(H, W), np.uint8)

    def reset(self):
        self.stale[:] = 1

    def scan(self, image):
        ids, tiles, counts, self.shadow, self.stale = scan(image, self.shadow, self.stale, self.capacity)
        return ids, tiles, counts


# ---------------------------------------------------------------- the wire frame, from the header text
# magic "DTPD" | version u8 = 1 | flags u8 (bit 0: first frame) | tile u16 = 16 | W i32 | H i32 | seq u32 | count i32 | remaining i32 |
# ids count x i32 | tiles count x 1024 bytes; little-endian
def encode(H, W, seq, ids, tiles, remaining=0, first=False, magic=b"DTPD", version=1, tile=16, count=None):
    ids = [int(t) for t in ids]
    n = len(ids) if count is None else count
    b = magic + struct.pack("<BBH", version, 1 if first else 0, tile) + struct.pack("<ii", W, H) + struct.pack("<I", seq) + struct.pack("<ii", n, remaining)
    b += b"".join(struct.pack("<i", t) for t in ids)
    return b + np.ascontiguousarray(tiles, dtype=np.uint8).tobytes()


def decode(b):
    if b[:4] != b"DTPD":
        raise ValueError("magic")
    version, flags, tile = struct.unpack_from("<BBH", b, 4)
    W, H = struct.unpack_from("<ii", b, 8)
    (seq,) = struct.unpack_from("<I", b, 16)
    count, remaining = struct.unpack_from("<ii", b, 20)
    if version != 1 or tile != 16:
        raise ValueError("version or tile")
    if len(b) != 28 + count * 1028:
        raise ValueError("length")
    ids = list(struct.unpack_from(f"<{count}i", b, 28))
    tiles = np.frombuffer(b, np.uint8, count * 1024, 28 + 4 * count).reshape(count, 16, 16, 4)
    return dict(H=H, W=W, seq=seq, first=bool(flags & 1), remaining=remaining, ids=ids, tiles=tiles)


def apply(image, b):
    f = decode(b)
    for t, p in zip(f["ids"], f["tiles"]):
        r0, c0, rows, cols = tile_box(f["H"], f["W"], t)
        image[r0:r0 + rows, c0:c0 + cols] = p[:rows, :cols]
    return f["seq"], f["remaining"]
