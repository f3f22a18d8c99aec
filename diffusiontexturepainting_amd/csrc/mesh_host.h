// The host-only arithmetic of the bleed pass of the mesh strokes (include/dtp.h: dtp_mesh_bleed_offsets, dtp_mesh_bleed; DESIGN.md
// 3.21): the table of candidate offsets in the contract's order and the clipping of a caller's rectangle.  No device call, so the
// stand-alone sanitizer program (tools/mesh_host_check.cpp) drives it directly.
#pragma once
#include <algorithm>
#include <array>

constexpr int MESH_MAX_BLEED = 16;  // the largest radius
constexpr int MESH_MAX_OFF = 796;   // the offsets (di, dj) with 0 < di^2 + dj^2 <= 16^2

// d[2 o], d[2 o + 1] = (di, dj) of candidate o, sorted by (di^2 + dj^2, di, dj); count[k] = the candidates with di^2 + dj^2 <= k^2: the
// table of radius k is the first count[k] entries of the one table
struct MeshBleedTable {
  int count[MESH_MAX_BLEED + 1];
  signed char d[2 * MESH_MAX_OFF];
};

inline const MeshBleedTable& mesh_bleed_table() {
  static const MeshBleedTable table = [] {
    MeshBleedTable t = {};
    std::array<int, 3> key[MESH_MAX_OFF];
    int n = 0;
    for (int di = -MESH_MAX_BLEED; di <= MESH_MAX_BLEED; ++di)
      for (int dj = -MESH_MAX_BLEED; dj <= MESH_MAX_BLEED; ++dj) {
        const int d2 = di * di + dj * dj;
        if (d2 > 0 && d2 <= MESH_MAX_BLEED * MESH_MAX_BLEED && n < MESH_MAX_OFF) key[n++] = {d2, di, dj};
      }
    std::sort(key, key + n);
    for (int o = 0; o < n; ++o) {
      t.d[2 * o] = (signed char)key[o][1];
      t.d[2 * o + 1] = (signed char)key[o][2];
      for (int k = 1; k <= MESH_MAX_BLEED; ++k)
        if (key[o][0] <= k * k) ++t.count[k];
    }
    return t;
  }();
  return table;
}

// The caller's rectangle (x0, y0, x1, y1 inclusive; NULL = the whole texture) clipped to an H x W texture.  0: out holds at least one
// texel; 1: nothing of it lies inside the texture; -1: x0 > x1 or y0 > y1 as given.
inline int mesh_clip_rect(const int* rect, int H, int W, int out[4]) {
  if (!rect) { out[0] = 0; out[1] = 0; out[2] = W - 1; out[3] = H - 1; return 0; }
  if (rect[0] > rect[2] || rect[1] > rect[3]) return -1;
  out[0] = std::max(rect[0], 0); out[1] = std::max(rect[1], 0);
  out[2] = std::min(rect[2], W - 1); out[3] = std::min(rect[3], H - 1);
  return out[0] > out[2] || out[1] > out[3] ? 1 : 0;
}
