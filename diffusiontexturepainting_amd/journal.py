"""The Python side of the undo / redo journal of a texture (include/dtp.h: dtp_journal_*): a copy-on-write journal of
16 x 16-texel tiles kept on the device.  While a record is open, paint_stroke, paint_mesh_stroke and paint_mesh_path save the old bytes
of every tile they are about to write, once per record; undo() and redo() swap them back, byte for byte, without the host holding a copy
of the texture.  A journal comes from MI355ConditionalInpainter.journal(texture)."""
import contextlib
import ctypes as C

import torch

from . import _lib
from ._lib import check

TILE = 16


def tile_count(H, W):
    """The 16 x 16-texel tiles of an H x W texture (edge tiles are partial)."""
    return ((int(H) + TILE - 1) // TILE) * ((int(W) + TILE - 1) // TILE)


def window_tiles(H, W, R, x, y, wrap=False):
    """The ascending tile indices a 2D stroke window at (x, y) saves (dtp_journal_window_tiles: host only, needs no GPU): every tile that
    meets the R x R window clipped to the H x W texture, or with wrap its wrapped pieces.  Tile t = (row / 16) * ceil(W / 16) + col / 16."""
    lib = _lib.load()
    n = C.c_int(-1)
    rc = lib.dtp_journal_window_tiles(int(H), int(W), int(R), int(bool(wrap)), int(x), int(y), None, 0, C.byref(n))
    if rc != 0 and n.value <= 0:
        check(rc, "dtp_journal_window_tiles")
    if n.value == 0:
        return []
    out = (C.c_int * n.value)()
    check(lib.dtp_journal_window_tiles(int(H), int(W), int(R), int(bool(wrap)), int(x), int(y), out, n.value, C.byref(n)),
          "dtp_journal_window_tiles")
    return list(out)


class Journal:
    """The journal of one texture (dtp_journal_create): uint8 [H, W, 4] on the model's device, contiguous; it is the tensor the strokes
    paint, and the journal keeps it alive.  capacity_tiles slots of 1 KiB form a ring, depth is the most records kept.  Freed by close(),
    by garbage collection, or with the model's handle."""

    def __init__(self, model, texture, capacity_tiles, depth):
        if not (isinstance(texture, torch.Tensor) and texture.dtype == torch.uint8 and texture.dim() == 3 and texture.shape[2] == 4
                and texture.device == model._device and texture.is_contiguous()):
            raise ValueError(f"texture must be a contiguous uint8 [H, W, 4] tensor on {model._device}")
        self._lib = _lib.load()
        self._model = model  # its handle must outlive the journal; its stream orders the journal's work with the strokes
        self.texture = texture
        self.H, self.W = int(texture.shape[0]), int(texture.shape[1])
        self.capacity_tiles, self.depth = int(capacity_tiles), int(depth)
        h = C.c_void_p()
        check(self._lib.dtp_journal_create(model._h, _lib.ptr(texture), self.H, self.W, self.capacity_tiles, self.depth, C.byref(h)),
              "dtp_journal_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    # every call runs on the model's stream, between the two halves of the hand-shake the strokes use
    def _enter(self):
        m = self._model
        m.stream.wait_stream(torch.cuda.current_stream(m._device))
        return C.c_void_p(m.stream.cuda_stream)

    def _leave(self):
        m = self._model
        torch.cuda.current_stream(m._device).wait_stream(m.stream)

    def begin(self):
        """Open a record (dtp_journal_begin): from now on the strokes on this texture save what they overwrite.  Drops the undone
        records, and the oldest one when `depth` exist.  DtpError when a record is open on this model already.  Only enqueues."""
        s = self._enter()
        check(self._lib.dtp_journal_begin(self._h, s), "dtp_journal_begin")
        self._leave()

    def end(self):
        """Close the open record (dtp_journal_end).  Only enqueues."""
        s = self._enter()
        check(self._lib.dtp_journal_end(self._h, s), "dtp_journal_end")
        self._leave()

    @contextlib.contextmanager
    def stroke(self):
        """with journal.stroke(): ... -- one record around everything painted inside."""
        self.begin()
        try:
            yield self
        finally:
            self.end()

    def touch(self, rects):
        """Save the tiles of rectangles (x0, y0, x1, y1), inclusive texel bounds clipped to the texture, into the open record
        (dtp_journal_touch): call it before writing those texels yourself (bleed_texture, a fill, an upload) and the write can be
        undone.  Only enqueues; the current stream waits for it, so a torch write that follows is ordered behind the save."""
        r = [int(v) for rect in rects for v in rect]
        if len(r) % 4 != 0:
            raise ValueError("every rectangle is (x0, y0, x1, y1)")
        n = len(r) // 4
        arr = (C.c_int * max(len(r), 1))(*r)
        s = self._enter()
        check(self._lib.dtp_journal_touch(self._h, arr, n, s), "dtp_journal_touch")
        self._leave()

    def _step(self, fn, name):
        s = self._enter()
        rc = fn(self._h, s)
        self._leave()
        if rc == 3 and b"nothing to" in (self._lib.dtp_last_error() or b""):
            return False
        check(rc, name)
        return True

    def undo(self):
        """Take back the newest record that is not undone (dtp_journal_undo): afterwards the texture holds what it held at that
        record's begin.  False: nothing to undo.  DtpError when the record was overwritten in the ring (it and every older record are
        dropped then) or a record is open.  Waits for the stream once."""
        return self._step(self._lib.dtp_journal_undo, "dtp_journal_undo")

    def redo(self):
        """Put back the oldest undone record (dtp_journal_redo): the texture holds what it held at that record's end.  False: nothing
        to redo."""
        return self._step(self._lib.dtp_journal_redo, "dtp_journal_redo")

    def info(self):
        """dict(records, cursor, open, head): the records kept, how many of them are applied (the others are undone), whether a record is
        open, and the slots ever taken (dtp_journal_info; waits for the stream)."""
        a, b, o, h = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        check(self._lib.dtp_journal_info(self._h, C.byref(a), C.byref(b), C.byref(o), C.byref(h)), "dtp_journal_info")
        return dict(records=a.value, cursor=b.value, open=bool(o.value), head=h.value)

    def record(self, index):
        """dict(start, end, restorable) of record `index`, 0 = the oldest (dtp_journal_record_info)."""
        a, b, r = C.c_uint64(), C.c_uint64(), C.c_int()
        check(self._lib.dtp_journal_record_info(self._h, int(index), C.byref(a), C.byref(b), C.byref(r)), "dtp_journal_record_info")
        return dict(start=a.value, end=b.value, restorable=bool(r.value))

    def tiles(self, record):
        """The tile indices record `record` saved, in slot order (dtp_op_journal_tiles)."""
        rec = self.record(record)
        n = C.c_int(0)
        out = (C.c_int * max(rec["end"] - rec["start"], 1))()
        check(self._lib.dtp_op_journal_tiles(self._h, int(record), out, len(out), C.byref(n)), "dtp_op_journal_tiles")
        return list(out[:n.value])

    def close(self):
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            check(self._lib.dtp_journal_destroy(h), "dtp_journal_destroy")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.dtp_journal_destroy(self._h)  # (already freed with its handle: refused, nothing followed)
                self._h = None
        except Exception:
            pass
