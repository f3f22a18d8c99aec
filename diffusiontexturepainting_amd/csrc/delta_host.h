// The host-only part of the changed-tile tracker of an image (include/dtp.h: "changed tiles of an image"): the layout of
// everything a tracker owns, the argument checks that need no device, the set of live trackers, and a scan over byte arrays on the CPU
// that goes through the three passes of the kernels (csrc/delta.hip) with their grouping.  The tiles and their numbers are the journal's
// (journal_host.h); no second numbering.  No device call, so the stand-alone sanitizer program (tools/delta_host_check.cpp) drives it
// directly, built by a plain C++ compiler.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <set>
#include <vector>

#include "../../include/dtp.h"
#include "journal_host.h"

constexpr int DELTA_MAX_SIDE = 16384;  // 1024 x 1024 tiles at most
constexpr int DELTA_GROUP = 64;        // tiles per workgroup of the flag and gather passes: one ballot's width
constexpr int DELTA_TILE_BYTES = JOURNAL_TILE * JOURNAL_TILE * 4;
constexpr int DELTA_HOST_HEAD = 16;    // the pinned block: counts (8 bytes, padded), then ids, then tiles

inline int delta_groups(int n_tiles) { return (n_tiles + DELTA_GROUP - 1) / DELTA_GROUP; }
inline uint64_t delta_round16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// ---------------------------------------------------------------- argument checks: false, and `why` says what is wrong
inline bool delta_check_shape(int H, int W, char* why, size_t n) {
  if (H < 1 || W < 1 || H > DELTA_MAX_SIDE || W > DELTA_MAX_SIDE) {
    snprintf(why, n, "a %d x %d image (each side 1..%d)", H, W, DELTA_MAX_SIDE);
    return false;
  }
  return true;
}
inline bool delta_check_create(int H, int W, int capacity_tiles, char* why, size_t n) {
  if (!delta_check_shape(H, W, why, n)) return false;
  if (capacity_tiles < 1) { snprintf(why, n, "capacity_tiles=%d (at least 1)", capacity_tiles); return false; }
  return true;
}
// an image handed to a tracker made for th x tw
inline bool delta_check_image(const void* image, int H, int W, int th, int tw, char* why, size_t n) {
  if (!image) { snprintf(why, n, "image is NULL"); return false; }
  if (!delta_check_shape(H, W, why, n)) return false;
  if (H != th || W != tw) { snprintf(why, n, "a %d x %d image, the tracker was created for %d x %d", H, W, th, tw); return false; }
  if (((uintptr_t)image & 3) != 0) { snprintf(why, n, "image must be 4-byte aligned (one RGBA texel per load)"); return false; }
  return true;
}
inline bool delta_check_pull(const void* host_ids, const void* host_tiles, const void* count, const void* remaining, int max_tiles,
                             int capacity, char* why, size_t n) {
  if (!host_ids || !host_tiles || !count || !remaining) { snprintf(why, n, "NULL argument (host_ids, host_tiles, count and remaining are required)"); return false; }
  if (max_tiles < capacity) { snprintf(why, n, "max_tiles=%d is below the tracker's capacity of %d tiles", max_tiles, capacity); return false; }
  return true;
}

// ---------------------------------------------------------------- the layout
// every check of dtp_delta_layout: true and *out written, or false, `why` says what is wrong and nothing is written
inline bool delta_layout(int H, int W, int capacity_tiles, dtp_delta_sizes* out, char* why, size_t n) {
  if (!out) { snprintf(why, n, "out is NULL"); return false; }
  if (!delta_check_create(H, W, capacity_tiles, why, n)) return false;
  dtp_delta_sizes d;
  memset(&d, 0, sizeof d);
  d.tiles_x = journal_tiles_x(W);
  d.tiles_y = journal_tiles_x(H);
  d.n_tiles = journal_tile_count(H, W);
  d.n_groups = delta_groups(d.n_tiles);
  d.capacity = capacity_tiles;
  d.shadow_bytes = (uint64_t)H * (uint64_t)W * 4;
  d.stale_bytes = (uint64_t)d.n_tiles;
  d.flag_bytes = (uint64_t)d.n_tiles;
  d.group_bytes = (uint64_t)d.n_groups * 4 * 2;  // a count and a base per group
  d.ids_bytes = (uint64_t)capacity_tiles * 4;
  d.tiles_bytes = (uint64_t)capacity_tiles * DELTA_TILE_BYTES;
  d.counts_bytes = 8;
  d.host_ids_offset = DELTA_HOST_HEAD;
  d.host_tiles_offset = DELTA_HOST_HEAD + delta_round16(d.ids_bytes);
  d.host_bytes = d.host_tiles_offset + d.tiles_bytes;
  *out = d;
  return true;
}

// ---------------------------------------------------------------- the live set
// The trackers that exist, each with the handle it belongs to.  A pointer that is not in the set is refused, not followed.
class DeltaLive {
 public:
  void add(const void* tracker, const void* owner) {
    std::lock_guard<std::mutex> lock(mu_);
    live_.insert({tracker, owner});
  }
  // the owner of a live tracker, or null
  const void* owner(const void* tracker) {
    std::lock_guard<std::mutex> lock(mu_);
    auto it = live_.lower_bound({tracker, nullptr});
    return it != live_.end() && it->first == tracker ? it->second : nullptr;
  }
  // false: not there
  bool remove(const void* tracker) {
    std::lock_guard<std::mutex> lock(mu_);
    auto it = live_.lower_bound({tracker, nullptr});
    if (it == live_.end() || it->first != tracker) return false;
    live_.erase(it);
    return true;
  }
  // every tracker of `owner` leaves the set; -> them
  std::vector<const void*> take_owner(const void* owner) {
    std::lock_guard<std::mutex> lock(mu_);
    std::vector<const void*> mine;
    for (auto it = live_.begin(); it != live_.end();)
      if (it->second == owner) { mine.push_back(it->first); it = live_.erase(it); } else ++it;
    return mine;
  }
  size_t size() {
    std::lock_guard<std::mutex> lock(mu_);
    return live_.size();
  }

 private:
  std::mutex mu_;
  std::set<std::pair<const void*, const void*>> live_;
};

// ---------------------------------------------------------------- the scan on the CPU, pass by pass as the kernels run it
// does any byte of tile t inside the image differ from the shadow?
inline bool delta_tile_differs(const uint8_t* image, const uint8_t* shadow, int H, int W, int t) {
  const int tw = journal_tiles_x(W), ty = t / tw, tx = t - ty * tw;
  const int r0 = ty * JOURNAL_TILE, c0 = tx * JOURNAL_TILE;
  const int rows = std::min(JOURNAL_TILE, H - r0), cols = std::min(JOURNAL_TILE, W - c0);
  for (int r = 0; r < rows; ++r) {
    const size_t at = ((size_t)(r0 + r) * W + c0) * 4;
    if (memcmp(image + at, shadow + at, (size_t)cols * 4) != 0) return true;
  }
  return false;
}

// image, shadow u8 [H][W][4]; stale u8 [n_tiles]; ids i32 [capacity]; tiles u8 [capacity][1024]; counts i32 [2].  Pass 1 flags the tiles
// and counts per group of DELTA_GROUP tiles, pass 2 is the exclusive scan of the counts, pass 3 gives every flagged tile its rank -- the
// group's base plus the flagged tiles before it in the group -- and a tile with a rank below the capacity writes its id, its payload
// (texels outside the image zero), its part of the shadow, and clears its stale mark.  Slots beyond `emitted` are left as they were.
inline void delta_scan_host(const uint8_t* image, uint8_t* shadow, uint8_t* stale, int H, int W, int capacity, int* ids, uint8_t* tiles,
                            int counts[2]) {
  const int n_tiles = journal_tile_count(H, W), n_groups = delta_groups(n_tiles), tw = journal_tiles_x(W);
  std::vector<uint8_t> flag((size_t)n_tiles);
  std::vector<int> count((size_t)n_groups, 0), base((size_t)n_groups, 0);
  for (int t = 0; t < n_tiles; ++t) {
    flag[t] = stale[t] != 0 || delta_tile_differs(image, shadow, H, W, t);
    count[t / DELTA_GROUP] += flag[t];
  }
  int total = 0;
  for (int g = 0; g < n_groups; ++g) { base[g] = total; total += count[g]; }
  const int emitted = std::min(total, capacity);
  counts[0] = emitted; counts[1] = total - emitted;
  for (int g = 0; g < n_groups; ++g) {
    int rank = base[g];
    for (int t = g * DELTA_GROUP; t < std::min(n_tiles, (g + 1) * DELTA_GROUP); ++t) {
      if (!flag[t]) continue;
      const int k = rank++;
      if (k >= capacity) continue;
      ids[k] = t;
      uint8_t* dst = tiles + (size_t)k * DELTA_TILE_BYTES;
      memset(dst, 0, DELTA_TILE_BYTES);
      const int ty = t / tw, tx = t - ty * tw, r0 = ty * JOURNAL_TILE, c0 = tx * JOURNAL_TILE;
      const int rows = std::min(JOURNAL_TILE, H - r0), cols = std::min(JOURNAL_TILE, W - c0);
      for (int r = 0; r < rows; ++r) {
        const size_t at = ((size_t)(r0 + r) * W + c0) * 4;
        memcpy(dst + (size_t)r * JOURNAL_TILE * 4, image + at, (size_t)cols * 4);
        memcpy(shadow + at, image + at, (size_t)cols * 4);
      }
      stale[t] = 0;
    }
  }
}
