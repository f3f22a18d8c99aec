// The host-only arithmetic of face sets (include/dtp.h "face sets: a lasso, masked strokes, a tint"): the snap of a
// lasso's vertices, every argument check of dtp_mesh_select but the look-up of the mesh, the pixel box of a snapped polygon, and the
// even-odd inside test, which the kernel of csrc/select.hip runs as it stands.  Integers only past the snap.  No device call, so the
// stand-alone sanitizer program (tools/select_host_check.cpp) drives it directly, built by a plain C++ compiler.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <cmath>

#include "../../include/dtp.h"

#ifdef __HIPCC__
#define SELECT_HD __host__ __device__
#else
#define SELECT_HD
#endif

constexpr int SELECT_MIN_VERTS = 3, SELECT_MAX_VERTS = 1024;  // the polygon is staged in LDS whole: 8 KB
constexpr int SELECT_MAX_SIDE = 4096;                         // the largest frame side, as the views'
constexpr int SELECT_SNAP_MAX = 1 << 26;                      // SNAP_MAX of mesh_dev.h: the raster's clamp

// the raster's snap (mesh_dev.h) on the host: rintf rounds to nearest even as the device's does
inline int select_snap(float t) { return (int)fminf(fmaxf(rintf(t), -(float)SELECT_SNAP_MAX), (float)SELECT_SNAP_MAX); }

// (x, y) float pixel coordinates -> xy[2 i], xy[2 i + 1] = snap(256.0f * x), snap(256.0f * y)
inline void select_snap_polygon(const float* polygon, int n, int* xy) {
#pragma clang fp contract(off)
  for (int i = 0; i < 2 * n; ++i) xy[i] = select_snap(256.0f * polygon[i]);
}

// nullptr, or what dtp_mesh_select refuses before it looks at the mesh; `why` holds the message
inline const char* select_check(const float* polygon, int n, int op, int H, int W, char why[160]) {
  if (n < SELECT_MIN_VERTS || n > SELECT_MAX_VERTS) {
    snprintf(why, 160, "a polygon of n=%d vertices (%d..%d)", n, SELECT_MIN_VERTS, SELECT_MAX_VERTS);
    return why;
  }
  if (op != DTP_SELECT_REPLACE && op != DTP_SELECT_ADD && op != DTP_SELECT_SUBTRACT) {
    snprintf(why, 160, "unknown op %d (REPLACE = 0, ADD = 1, SUBTRACT = 2)", op);
    return why;
  }
  if (H < 1 || W < 1 || H > SELECT_MAX_SIDE || W > SELECT_MAX_SIDE) {
    snprintf(why, 160, "a %d x %d frame (each side 1..%d)", H, W, SELECT_MAX_SIDE);
    return why;
  }
  for (int i = 0; i < 2 * n; ++i)
    if (!std::isfinite(polygon[i])) {
      snprintf(why, 160, "vertex %d of the polygon is not finite", i / 2);
      return why;
    }
  return nullptr;
}

// floor(a / 256) for either sign (a shift of a negative int is left to the implementation before C++20)
SELECT_HD inline int select_floor256(int a) { return a >= 0 ? a / 256 : -((255 - a) / 256); }

// The pixels [x0, x1] x [y0, y1] of an H x W frame whose centres (256 j + 128, 256 i + 128) lie in the bounding box of the snapped polygon:
// no other centre can be inside it.  false: there is none.
inline bool select_box(const int* xy, int n, int H, int W, int& x0, int& x1, int& y0, int& y1) {
  int lx = xy[0], hx = xy[0], ly = xy[1], hy = xy[1];
  for (int i = 1; i < n; ++i) {
    lx = xy[2 * i] < lx ? xy[2 * i] : lx; hx = xy[2 * i] > hx ? xy[2 * i] : hx;
    ly = xy[2 * i + 1] < ly ? xy[2 * i + 1] : ly; hy = xy[2 * i + 1] > hy ? xy[2 * i + 1] : hy;
  }
  x0 = select_floor256(lx - 128 + 255); x1 = select_floor256(hx - 128);
  y0 = select_floor256(ly - 128 + 255); y1 = select_floor256(hy - 128);
  x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
  x1 = x1 > W - 1 ? W - 1 : x1; y1 = y1 > H - 1 ? H - 1 : y1;
  return x0 <= x1 && y0 <= y1;
}

// Does the edge (a, b) count for the centre P?  It crosses P's row -- (a.y > P.y) != (b.y > P.y) -- and P lies strictly left of the
// crossing: D = (P.x - a.x)(b.y - a.y) - (P.y - a.y)(b.x - a.x) is not zero and negative exactly when b.y - a.y is positive.  Every
// coordinate is within +-2^26 and a centre within 0 .. 2^20, so a difference is below 2^27 + 2^20, a product below 2^55, D below 2^56.
SELECT_HD inline bool select_edge_counts(int ax, int ay, int bx, int by, int px, int py) {
  if ((ay > py) == (by > py)) return false;
  const long long dy = (long long)by - ay;
  const long long D = ((long long)px - ax) * dy - ((long long)py - ay) * ((long long)bx - ax);
  return D != 0 && (D < 0) == (dy > 0);
}

// even-odd over the n edges (i, i + 1 mod n) of the snapped polygon
SELECT_HD inline bool select_inside(const int* xy, int n, int px, int py) {
  bool in = false;
  for (int i = 0; i < n; ++i) {
    const int j = i + 1 == n ? 0 : i + 1;
    if (select_edge_counts(xy[2 * i], xy[2 * i + 1], xy[2 * j], xy[2 * j + 1], px, py)) in = !in;
  }
  return in;
}

// the checks of a face set handed to a kernel: `words` int32 words for F faces, 4-byte aligned; nullptr or the message
inline const char* select_check_set(const void* set, int words, int F, char why[160]) {
  if (words != (F + 31) / 32) {
    snprintf(why, 160, "a face set of %d words for %d faces ((F + 31) / 32 = %d)", words, F, (F + 31) / 32);
    return why;
  }
  if (((uintptr_t)set & 3) != 0) {
    snprintf(why, 160, "the face set must be 4-byte aligned");
    return why;
  }
  return nullptr;
}
