"""The contract of the undo / redo journal (include/dtp.h: "undo / redo journal of a texture") restated in numpy: the tiles of a rectangle
and of a 2D stroke window, the record list with its cursor, depth and the ring's restorability rule as a pure state machine, and a model
of a journal over a numpy texture that saves, swaps and redoes.  Written from the header's text, not from the library's code."""
import numpy as np

TILE = 16


def tiles_x(W):
    return -(-W // TILE)


def tile_count(H, W):
    return tiles_x(H) * tiles_x(W)


def rect_tiles(H, W, rect):
    """The set of tiles that meet the inclusive texel rectangle (x0, y0, x1, y1) clipped to the texture."""
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[2], W - 1), min(rect[3], H - 1)
    if x0 > x1 or y0 > y1:
        return set()
    return {ty * tiles_x(W) + tx for ty in range(y0 // TILE, y1 // TILE + 1) for tx in range(x0 // TILE, x1 // TILE + 1)}


def window_tiles(H, W, R, x, y, wrap=False):
    """The ascending tile list of ONE 2D stroke window, texel by texel: the tile of every texel the window holds (wrapped, or clipped)."""
    rows, cols = np.arange(y, y + R), np.arange(x, x + R)
    if wrap:
        rows, cols = rows % H, cols % W
    else:
        rows, cols = rows[(rows >= 0) & (rows < H)], cols[(cols >= 0) & (cols < W)]
    t = (rows[:, None] // TILE) * tiles_x(W) + cols[None, :] // TILE
    return sorted(set(t.reshape(-1).tolist()))


def tile_slices(H, W, t):
    ty, tx = divmod(t, tiles_x(W))
    return slice(ty * TILE, min(ty * TILE + TILE, H)), slice(tx * TILE, min(tx * TILE + TILE, W))


class Records:
    """The list of records as a pure state machine: each record is [start, end]; records[:cursor] are applied, records[cursor:] undone."""

    def __init__(self, capacity, depth):
        self.capacity, self.depth = capacity, depth
        self.head = 0
        self.records, self.cursor, self.open = [], 0, False

    def begin(self):
        if self.open:
            raise RuntimeError("state: a record is open")
        del self.records[self.cursor:]  # the undone ones: head is not rewound
        if len(self.records) >= self.depth:
            del self.records[0]
        self.records.append([self.head, self.head])
        self.cursor = len(self.records)
        self.open = True

    def take(self, n):
        """n slots are taken by the open record -> their ring positions."""
        if not self.open:
            raise RuntimeError("state: no record is open")
        slots = [(self.head + i) % self.capacity for i in range(n)]
        self.head += n
        return slots

    def end(self):
        if not self.open:
            raise RuntimeError("state: no record is open")
        self.records[-1][1] = self.head
        self.open = False

    def restorable(self, i):
        return self.head - self.records[i][0] <= self.capacity

    def _pick(self, i, what):
        """-> the record to swap, or None (nothing to do); RuntimeError("overwritten") drops it and every older one."""
        if self.open:
            raise RuntimeError("state: a record is open")
        if i is None:
            return None
        if not self.restorable(i):
            del self.records[:i + 1]
            self.cursor = max(self.cursor - (i + 1), 0)
            raise RuntimeError(f"overwritten: cannot {what}")
        return self.records[i]

    def undo(self):
        r = self._pick(self.cursor - 1 if self.cursor > 0 else None, "undo")
        if r is not None:
            self.cursor -= 1
        return r

    def redo(self):
        r = self._pick(self.cursor if self.cursor < len(self.records) else None, "redo")
        if r is not None:
            self.cursor += 1
        return r


class Journal:
    """A journal over a numpy texture u8 [H, W, 4] (changed in place by undo / redo)."""

    def __init__(self, texture, capacity, depth=10):
        self.tex = texture
        self.H, self.W = texture.shape[:2]
        self.rec = Records(capacity, depth)
        self.slots = np.zeros((capacity, TILE, TILE, 4), dtype=np.uint8)
        self.slot_tile = np.full(capacity, -1, dtype=np.int64)
        self.saved = set()  # the tiles of the open record

    def begin(self):
        self.rec.begin()
        self.saved = set()

    def end(self):
        self.rec.end()

    def touch(self, rects):
        """Save the tiles of the rectangles, each once per record, BEFORE the caller writes them -> the tiles newly saved."""
        new = []
        for r in rects:
            for t in sorted(rect_tiles(self.H, self.W, r)):
                if t not in self.saved:
                    self.saved.add(t)
                    new.append(t)
        for t, slot in zip(new, self.rec.take(len(new))):
            rs, cs = tile_slices(self.H, self.W, t)
            part = self.tex[rs, cs]
            self.slots[slot, :part.shape[0], :part.shape[1]] = part
            self.slot_tile[slot] = t
        return new

    def tiles(self, i):
        a, b = self.rec.records[i]
        return [int(self.slot_tile[k % self.rec.capacity]) for k in range(a, b)]

    def _swap(self, r):
        for k in range(r[0], r[1]):
            slot = k % self.rec.capacity
            rs, cs = tile_slices(self.H, self.W, int(self.slot_tile[slot]))
            part = self.tex[rs, cs].copy()
            self.tex[rs, cs] = self.slots[slot, :part.shape[0], :part.shape[1]]
            self.slots[slot, :part.shape[0], :part.shape[1]] = part

    def undo(self):
        r = self.rec.undo()
        if r is None:
            return False
        self._swap(r)
        return True

    def redo(self):
        r = self.rec.redo()
        if r is None:
            return False
        self._swap(r)
        return True
