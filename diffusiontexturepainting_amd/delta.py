"""Changed tiles of a device image for a client that keeps a mirror of it (include/dtp.h: "changed tiles of an image", dtp_delta_*;
DESIGN.md 3.26).  A DeltaTracker, from MI355ConditionalInpainter.delta_tracker(), owns a shadow copy of what its client already has; pull()
compares a texture or a rendered frame with it on the device and reads back only the 16 x 16-texel tiles whose bytes changed, in
ascending tile order; frame() packs them for the wire.  decode_frame() and apply_frame() are the client's side: this module imports
without torch and without a GPU (numpy alone), because a client has neither.

The wire frame, little-endian:
    magic "DTPD" | version u8 = 1 | flags u8 (bit 0: first frame since create or reset) | tile u16 = 16 | W i32 | H i32 | seq u32 |
    count i32 | remaining i32 | ids count x i32 | tiles count x 1024 bytes
Tile t = (row / 16) * ceil(W / 16) + col / 16, the journal's numbering; a payload is 16 rows of 16 RGBA texels, zero outside the image."""
import ctypes as C
import struct

import numpy as np

MAGIC = b"DTPD"
VERSION = 1
TILE = 16
TILE_BYTES = TILE * TILE * 4
FLAG_FIRST = 1
HEADER = struct.Struct("<4sBBHiiIii")


def _tiles_xy(H, W):
    return (int(W) + TILE - 1) // TILE, (int(H) + TILE - 1) // TILE


def encode_frame(H, W, seq, ids, tiles, remaining=0, first=False):
    """The wire frame of `ids` (int32 [n], strictly ascending tiles of an H x W image) with their payloads `tiles` (uint8 [n, 16, 16, 4])."""
    ids = np.ascontiguousarray(ids, dtype="<i4").reshape(-1)
    tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
    if tiles.size != ids.size * TILE_BYTES:
        raise ValueError(f"{ids.size} ids need {ids.size * TILE_BYTES} payload bytes, got {tiles.size}")
    head = HEADER.pack(MAGIC, VERSION, FLAG_FIRST if first else 0, TILE, int(W), int(H), int(seq) & 0xFFFFFFFF, int(ids.size), int(remaining))
    return head + ids.tobytes() + tiles.tobytes()


def decode_frame(b):
    """A wire frame -> dict(H, W, seq, first, remaining, ids int32 [n], tiles uint8 [n, 16, 16, 4]); the arrays are read-only views of
    `b`.  ValueError for a bad magic, version or tile size, a length that does not match count, a shape outside 1..16384, an id outside
    the image, or ids that do not strictly ascend."""
    b = bytes(b) if not isinstance(b, (bytes, bytearray, memoryview)) else b
    if len(b) < HEADER.size:
        raise ValueError(f"a frame has at least {HEADER.size} bytes, got {len(b)}")
    magic, version, flags, tile, W, H, seq, count, remaining = HEADER.unpack_from(b, 0)
    if magic != MAGIC:
        raise ValueError(f"bad magic {magic!r} (expected {MAGIC!r})")
    if version != VERSION:
        raise ValueError(f"frame version {version}, this decoder reads version {VERSION}")
    if tile != TILE:
        raise ValueError(f"tile size {tile}, expected {TILE}")
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"a {H} x {W} image (each side 1..16384)")
    if count < 0 or remaining < 0:
        raise ValueError(f"count={count}, remaining={remaining}: negative")
    want = HEADER.size + count * (4 + TILE_BYTES)
    if len(b) != want:
        raise ValueError(f"a frame of {count} tiles has {want} bytes, got {len(b)}")
    ids = np.frombuffer(b, dtype="<i4", count=count, offset=HEADER.size)
    tiles = np.frombuffer(b, dtype=np.uint8, count=count * TILE_BYTES, offset=HEADER.size + 4 * count).reshape(count, TILE, TILE, 4)
    tx, ty = _tiles_xy(H, W)
    if count and (int(ids.min()) < 0 or int(ids.max()) >= tx * ty):
        raise ValueError(f"a tile id outside 0..{tx * ty - 1} of a {H} x {W} image")
    if count > 1 and not bool((ids[1:] > ids[:-1]).all()):
        raise ValueError("tile ids do not strictly ascend")
    return dict(H=H, W=W, seq=seq, first=bool(flags & FLAG_FIRST), remaining=remaining, ids=ids, tiles=tiles)


def apply_frame(image, b, expect_seq=None):
    """Write the tiles of wire frame `b` into the mirror `image` (numpy uint8 [H, W, 4], changed in place), clipped at the image's edge
    -> (seq, remaining).  expect_seq: the sequence number this frame must carry (the last one + 1).  ValueError, with the mirror
    untouched, for anything decode_frame refuses, a frame of another shape than the mirror's, and a sequence gap."""
    if not (isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 4):
        raise ValueError("the mirror must be a numpy uint8 [H, W, 4] array")
    f = decode_frame(b)
    H, W = image.shape[:2]
    if (f["H"], f["W"]) != (H, W):
        raise ValueError(f"a frame of a {f['H']} x {f['W']} image, the mirror is {H} x {W}")
    if expect_seq is not None and f["seq"] != (int(expect_seq) & 0xFFFFFFFF):
        raise ValueError(f"sequence gap: frame {f['seq']}, expected {int(expect_seq) & 0xFFFFFFFF}")
    tx, _ = _tiles_xy(H, W)
    for t, tile in zip(f["ids"].tolist(), f["tiles"]):
        r0, c0 = (t // tx) * TILE, (t % tx) * TILE
        rows, cols = min(TILE, H - r0), min(TILE, W - c0)
        image[r0:r0 + rows, c0:c0 + cols] = tile[:rows, :cols]
    return f["seq"], f["remaining"]


class DeltaTracker:
    """The changed-tile tracker of images of one shape (dtp_delta_create): a shadow image, a stale mark per tile, the device outputs and
    a pinned host block, all allocated here.  A new tracker has every tile stale, so its first pull is a key frame.  capacity_tiles: the
    most tiles one pull emits; the rest stay changed and come with the next pulls.  Freed by close(), by garbage collection, or with the
    model's handle."""

    def __init__(self, model, H, W, capacity_tiles):
        from . import _lib
        self._libmod = _lib
        self._lib = _lib.load()
        self._model = model  # its handle must outlive the tracker; its streams order the scans with the strokes and the views
        self.H, self.W, self.capacity_tiles = int(H), int(W), int(capacity_tiles)
        h = C.c_void_p()
        _lib.check(self._lib.dtp_delta_create(model._h, self.H, self.W, self.capacity_tiles, C.byref(h)), "dtp_delta_create")
        self._h = h
        self._seq, self._first = 0, True
        cap = self.capacity_tiles
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.dtp_delta_host(h, C.byref(a), C.byref(b)), "dtp_delta_host")
        self._host_ids_p, self._host_tiles_p = a.value, b.value
        self._host_ids = np.ctypeslib.as_array((C.c_int32 * cap).from_address(a.value))
        self._host_tiles = np.ctypeslib.as_array((C.c_uint8 * (cap * TILE_BYTES)).from_address(b.value)).reshape(cap, TILE, TILE, 4)
        a, b = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.dtp_delta_device(h, C.byref(a), C.byref(b), C.byref(c)), "dtp_delta_device")
        self._dev_p = (a.value, b.value, c.value)
        self._dev = None  # torch views of the device outputs, made at the first device pull

    @property
    def handle(self):
        return self._h

    def _alive(self):
        if not getattr(self, "_h", None):
            raise self._libmod.DtpError("the tracker is closed")

    def _image(self, image):
        import torch
        m = self._model
        if not (isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 4
                and image.device == m._device and image.is_contiguous()):
            raise ValueError(f"image must be a contiguous uint8 [H, W, 4] tensor on {m._device}")
        return image

    def _stream(self, on):
        if on not in ("stroke", "view"):
            raise ValueError(f"on={on!r}: choose 'stroke' or 'view'")
        return self._model.stream if on == "stroke" else self._model.view_stream

    def _device_views(self):
        import torch
        if self._dev is None:
            dev = self._model._device

            class _Blob:  # a tracker-owned device buffer as torch sees it; the view keeps the tracker alive
                def __init__(blob, owner, p, shape, typestr):
                    blob.owner = owner
                    blob.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(p, False), version=2)

            cap = self.capacity_tiles
            self._dev = (torch.as_tensor(_Blob(self, self._dev_p[0], (cap,), "<i4"), device=dev),
                         torch.as_tensor(_Blob(self, self._dev_p[1], (cap, TILE, TILE, 4), "|u1"), device=dev),
                         torch.as_tensor(_Blob(self, self._dev_p[2], (2,), "<i4"), device=dev))
        return self._dev

    def pull(self, image, on="stroke", device=False):
        """The tiles of `image` (uint8 [H, W, 4] on the model's device, contiguous, the tracker's shape) that changed since they were last
        emitted -> (ids int32 [n], tiles uint8 [n, 16, 16, 4], remaining).  n <= capacity_tiles; remaining > 0: pull again for the next
        tiles.  on="stroke": the scan runs on model.stream after the caller's stream, as bleed_texture does, for a texture the strokes
        paint.  on="view": on model.view_stream, after the frame that render_view(out=image) queued there.  device=False
        (dtp_delta_pull): numpy views into the tracker's pinned block, valid until the next pull; the host waits for the scan and for
        the copy of n KiB.  device=True (dtp_delta_scan): torch slices of the device outputs, valid until the next pull; the host waits
        for the 8 bytes of the counts alone."""
        import torch
        self._alive()
        lib, check, m = self._lib, self._libmod.check, self._model
        image = self._image(image)
        stream = self._stream(on)
        cur = torch.cuda.current_stream(m._device)
        stream.wait_stream(cur)
        s = C.c_void_p(stream.cuda_stream)
        H, W = int(image.shape[0]), int(image.shape[1])
        if device:
            ids, tiles, counts = self._device_views()
            check(lib.dtp_delta_scan(m._h, self._h, image.data_ptr(), H, W, s), "dtp_delta_scan")
            with torch.cuda.stream(stream):
                n, remaining = counts.cpu().tolist()
            out = (ids[:n], tiles[:n], remaining)
        else:
            n, remaining = C.c_int(0), C.c_int(0)
            check(lib.dtp_delta_pull(m._h, self._h, image.data_ptr(), H, W, s, self._host_ids_p, self._host_tiles_p, self.capacity_tiles,
                                     C.byref(n), C.byref(remaining)), "dtp_delta_pull")
            out = (self._host_ids[:n.value], self._host_tiles[:n.value], remaining.value)
        cur.wait_stream(stream)
        image.record_stream(stream)
        return out

    def frame(self, image, on="stroke"):
        """pull(image, on) as one wire frame (bytes) with the next sequence number; the first frame since create or reset says so."""
        ids, tiles, remaining = self.pull(image, on=on)
        b = encode_frame(self.H, self.W, self._seq, ids, tiles, remaining, first=self._first)
        self._seq, self._first = (self._seq + 1) & 0xFFFFFFFF, False
        return b

    def reset(self, on="stroke"):
        """Every tile is stale again (dtp_delta_reset): the next pulls send the whole image, for a client that reconnected.  One memset,
        in stream order on the stream pull(on=...) uses.  Only enqueues."""
        import torch
        self._alive()
        m = self._model
        stream = self._stream(on)
        cur = torch.cuda.current_stream(m._device)
        stream.wait_stream(cur)
        self._libmod.check(self._lib.dtp_delta_reset(self._h, C.c_void_p(stream.cuda_stream)), "dtp_delta_reset")
        cur.wait_stream(stream)
        self._first = True

    def close(self):
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            self._libmod.check(self._lib.dtp_delta_destroy(h), "dtp_delta_destroy")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.dtp_delta_destroy(self._h)  # (already freed with its handle: refused, nothing followed)
                self._h = None
        except Exception:
            pass
