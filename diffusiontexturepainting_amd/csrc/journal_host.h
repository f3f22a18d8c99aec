// The host-only part of the undo / redo journal of a texture (include/dtp.h: "undo / redo journal of a texture"): the
// tiles of a rectangle and of a 2D stroke window, the list of records with its cursor, depth eviction and the ring's restorability rule,
// and the argument checks that need no device.  No device call, so the stand-alone sanitizer program (tools/journal_host_check.cpp)
// drives it directly.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

constexpr int JOURNAL_TILE = 16;       // a tile is 16 x 16 texels, a slot 256 RGBA texels = 1 KiB
constexpr int JOURNAL_MAX_DEPTH = 64;  // the records a journal can keep
constexpr int JOURNAL_MAX_TEX = 32768;

inline int journal_tiles_x(int W) { return (W + JOURNAL_TILE - 1) / JOURNAL_TILE; }
inline int journal_tile_count(int H, int W) { return journal_tiles_x(H) * journal_tiles_x(W); }  // (at most 2048 * 2048)

// ---------------------------------------------------------------- argument checks: false, and `why` says what is wrong
inline bool journal_check_texture(const void* texture, int H, int W, char* why, size_t n) {
  if (!texture) { snprintf(why, n, "texture is NULL"); return false; }
  if (H < 1 || W < 1 || H > JOURNAL_MAX_TEX || W > JOURNAL_MAX_TEX) {
    snprintf(why, n, "a %d x %d texture (each side 1..%d)", H, W, JOURNAL_MAX_TEX);
    return false;
  }
  if (((uintptr_t)texture & 3) != 0) { snprintf(why, n, "texture must be 4-byte aligned (one RGBA texel per load)"); return false; }
  return true;
}
inline bool journal_check_create(const void* texture, int H, int W, int capacity_tiles, int depth, char* why, size_t n) {
  if (!journal_check_texture(texture, H, W, why, n)) return false;
  if (capacity_tiles < 1) { snprintf(why, n, "capacity_tiles=%d (at least 1)", capacity_tiles); return false; }
  if (depth < 1 || depth > JOURNAL_MAX_DEPTH) { snprintf(why, n, "depth=%d outside 1..%d", depth, JOURNAL_MAX_DEPTH); return false; }
  return true;
}
// rects: int[n][4] inclusive {x0, y0, x1, y1}
inline bool journal_check_rects(const int* rects, int n, char* why, size_t len) {
  if (!rects) { snprintf(why, len, "rects is NULL"); return false; }
  if (n < 1) { snprintf(why, len, "n=%d rectangles (at least 1)", n); return false; }
  for (int i = 0; i < n; ++i) {
    const int* r = rects + 4 * (size_t)i;
    if (r[0] > r[2] || r[1] > r[3]) {
      snprintf(why, len, "rectangle %d (%d, %d, %d, %d) has x0 > x1 or y0 > y1", i, r[0], r[1], r[2], r[3]);
      return false;
    }
  }
  return true;
}

// ---------------------------------------------------------------- rectangles and tiles
// the rectangle (x0 <= x1, y0 <= y1) clipped to the texture; false: nothing of it lies inside
inline bool journal_clip_rect(const int r[4], int H, int W, int out[4]) {
  out[0] = std::max(r[0], 0); out[1] = std::max(r[1], 0);
  out[2] = std::min(r[2], W - 1); out[3] = std::min(r[3], H - 1);
  return out[0] <= out[2] && out[1] <= out[3];
}
// a clipped texel rectangle as the rectangle of tiles that meet it
inline void journal_tile_rect(const int r[4], int out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = r[k] / JOURNAL_TILE;
}

// the pieces [lo, hi] of the R texels from `a` on an axis of length L (R <= L): clipped, or wrapped; at most two
inline int journal_axis_pieces(long long a, int R, int L, bool wrap, int lo[2], int hi[2]) {
  if (!wrap) {
    const long long p = std::max<long long>(a, 0), q = std::min<long long>(a + R - 1, L - 1);
    if (p > q) return 0;
    lo[0] = (int)p; hi[0] = (int)q;
    return 1;
  }
  long long m = a % L;
  if (m < 0) m += L;
  if (m + R <= L) { lo[0] = (int)m; hi[0] = (int)(m + R - 1); return 1; }
  lo[0] = (int)m; hi[0] = L - 1;
  lo[1] = 0; hi[1] = (int)(m + R - 1 - L);
  return 2;
}
// The texel rectangles a 2D stroke window at (x, y) may write: the window clipped to the texture, or with `wrap` its wrapped pieces.
// At most four; returns their number (0: the window lies outside a non-wrapping texture).  R <= H, R <= W.
inline int journal_window_rects(int H, int W, int R, bool wrap, int x, int y, int out[4][4]) {
  int xl[2], xh[2], yl[2], yh[2];
  const int nx = journal_axis_pieces(x, R, W, wrap, xl, xh), ny = journal_axis_pieces(y, R, H, wrap, yl, yh);
  int n = 0;
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i, ++n) { out[n][0] = xl[i]; out[n][1] = yl[j]; out[n][2] = xh[i]; out[n][3] = yh[j]; }
  return n;
}
// the tiles of n clipped texel rectangles, ascending, each once
inline std::vector<int> journal_rect_tiles(int W, const int (*rects)[4], int n) {
  std::vector<int> t;
  const int tw = journal_tiles_x(W);
  for (int i = 0; i < n; ++i) {
    int q[4];
    journal_tile_rect(rects[i], q);
    for (int ty = q[1]; ty <= q[3]; ++ty)
      for (int tx = q[0]; tx <= q[2]; ++tx) t.push_back(ty * tw + tx);
  }
  std::sort(t.begin(), t.end());
  t.erase(std::unique(t.begin(), t.end()), t.end());
  return t;
}
inline std::vector<int> journal_window_tiles(int H, int W, int R, bool wrap, int x, int y) {
  int rects[4][4];
  const int n = journal_window_rects(H, W, R, wrap, x, y, rects);
  return journal_rect_tiles(W, rects, n);
}

// ---------------------------------------------------------------- the ring
// Slot k of all slots ever taken lives at k mod capacity; a record that took its first slot at `start` can be restored while no later
// slot has landed on that one.
inline bool journal_restorable(uint64_t head, uint64_t start, uint64_t capacity) { return head - start <= capacity; }

// ---------------------------------------------------------------- the records
// row: where the record's (start, end) pair lives on the device, 0 .. depth - 1; gen: the value a tile's word takes when this record saves
// it (never 0, never that of another live record)
struct JournalRec { int row, gen; };

// The list: recs[0 .. cursor) are applied, oldest first, recs[cursor ..) are undone, oldest first.  An open record is the last one.
struct JournalList {
  int depth = 1;
  std::vector<JournalRec> recs;
  int cursor = 0;
  bool open = false;
  int next_gen = 1;
  uint64_t rows_used = 0;

  void release(int from, int to) {  // recs[from .. to) leave
    for (int i = from; i < to; ++i) rows_used &= ~(1ull << recs[i].row);
    recs.erase(recs.begin() + from, recs.begin() + to);
  }
  // opens a record: the undone ones go, then the oldest if `depth` records exist already.  false: one is open.
  bool begin(JournalRec* out) {
    if (open) return false;
    release(cursor, (int)recs.size());
    if ((int)recs.size() >= depth) release(0, (int)recs.size() - depth + 1);
    JournalRec r;
    r.row = 0;
    while (rows_used & (1ull << r.row)) ++r.row;  // (fewer than depth <= 64 rows are in use)
    rows_used |= 1ull << r.row;
    r.gen = next_gen;
    next_gen = next_gen == 0x7fffffff ? 1 : next_gen + 1;
    recs.push_back(r);
    cursor = (int)recs.size();
    open = true;
    if (out) *out = r;
    return true;
  }
  bool end() {
    if (!open) return false;
    open = false;
    return true;
  }
  int undo_pick() const { return cursor > 0 ? cursor - 1 : -1; }            // the newest record that is not undone
  int redo_pick() const { return cursor < (int)recs.size() ? cursor : -1; }  // the oldest undone record
  void undo_done() { --cursor; }
  void redo_done() { ++cursor; }
  // record i was overwritten in the ring: it and every older one go
  void drop_through(int i) {
    release(0, i + 1);
    cursor = std::max(cursor - (i + 1), 0);
  }
};
