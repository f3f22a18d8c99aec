// The host-only arithmetic of the bleed pass of the mesh strokes (include/dtp.h: dtp_mesh_bleed_offsets, dtp_mesh_bleed; DESIGN.md
// 3.21): the table of candidate offsets in the contract's order and the clipping of a caller's rectangle; and of picking (dtp_mesh_pick,
// dtp_mesh_path_plan): the ray frame, the exponent of a ray's grid and the stamp spacing of a pointer path; and of the
// occlusion test (dtp_mesh_stroke_occluded): the check of the setting and the tolerance it becomes.  No device
// call, so the stand-alone sanitizer programs (tools/mesh_host_check.cpp, tools/mesh_pick_host_check.cpp) drive it directly.
#pragma once
#include <math.h>
#include <algorithm>
#include <array>
#include <cmath>

#include "../../include/dtp.h"

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

// ---------------------------------------------------------------- the occlusion test of the backprojection
// occlude: a tolerance in stamp pixels, finite and >= 0
inline bool mesh_occlude_ok(float occlude) { return std::isfinite(occlude) && occlude >= 0.f; }
// The depth, in camera units, of `occlude` pixel widths of an R x R window that spans 2 fov camera units: ((occlude 2) fov) / R in double
// from the fp32 inputs, rounded to fp32 once.  false: it does not fit fp32 (*tol untouched).
inline bool mesh_occlude_tol(float occlude, float fov, int R, float* tol) {
#pragma clang fp contract(off)
  const float t = (float)((((double)occlude * 2.0) * (double)fov) / (double)R);
  if (!std::isfinite(t)) return false;
  *tol = t;
  return true;
}

// ---------------------------------------------------------------- picking
constexpr int PICK_MAX_RAYS = 4096;
constexpr int PICK_E_MIN = -64, PICK_E_MAX = 64;  // the grid's exponent is clamped to this range
constexpr int PATH_MAX_CHORD = 1 << 20;           // the stamps one chord may be cut into

// The frame of a ray, in double from the fp32 origin and direction, rounded to fp32 once: b = -normalize(d) (the frame looks down -z, as
// the stamp camera does), helper = the unit axis of the smallest |d_k| (the lowest k on a tie), r = normalize(cross(helper, b)),
// u = cross(b, r); out = the rows (r, u, b), each followed by -row . o.  nullptr, or what is wrong with the ray.
inline const char* mesh_ray_frame(const float o[3], const float d[3], float out[12]) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i) {
    if (!std::isfinite(o[i])) return "a non-finite origin";
    if (!std::isfinite(d[i])) return "a non-finite direction";
  }
  const double dd[3] = {(double)d[0], (double)d[1], (double)d[2]}, od[3] = {(double)o[0], (double)o[1], (double)o[2]};
  const double ld = sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);
  if (!(ld > 0.0)) return "the direction is zero";
  double b[3], h[3] = {0.0, 0.0, 0.0}, r[3], u[3];
  for (int i = 0; i < 3; ++i) b[i] = -(dd[i] / ld);
  int k = 0;
  for (int i = 1; i < 3; ++i)
    if (std::fabs(dd[i]) < std::fabs(dd[k])) k = i;
  h[k] = 1.0;
  r[0] = h[1] * b[2] - h[2] * b[1]; r[1] = h[2] * b[0] - h[0] * b[2]; r[2] = h[0] * b[1] - h[1] * b[0];
  const double lr = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);  // >= sqrt(2 / 3): b is a unit vector and k its smallest component
  for (int i = 0; i < 3; ++i) r[i] /= lr;
  u[0] = b[1] * r[2] - b[2] * r[1]; u[1] = b[2] * r[0] - b[0] * r[2]; u[2] = b[0] * r[1] - b[1] * r[0];
  const double* rows[3] = {r, u, b};
  float f[12];
  for (int j = 0; j < 3; ++j) {
    for (int i = 0; i < 3; ++i) f[4 * j + i] = (float)rows[j][i];
    f[4 * j + 3] = (float)-((rows[j][0] * od[0] + rows[j][1] * od[1]) + rows[j][2] * od[2]);
  }
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(f[i])) return "the ray frame does not fit fp32";
  for (int i = 0; i < 12; ++i) out[i] = f[i];
  return nullptr;
}

// The exponent e of a ray's grid S = 2^e: the eight corners of the box [lo, hi] through the fp32 frame in double, x = ((m0 v0 + m1 v1) +
// m2 v2) + m3 for rows 0 and 1; e is the largest with 2^e max(|x|, |y|) <= 2^25, clamped to [PICK_E_MIN, PICK_E_MAX] (a box on the ray's
// axis, max = 0: PICK_E_MAX).
inline int mesh_pick_exponent(const float frame[12], const double lo[3], const double hi[3]) {
#pragma clang fp contract(off)
  double m = 0.0;
  for (int corner = 0; corner < 8; ++corner) {
    const double v[3] = {corner & 1 ? hi[0] : lo[0], corner & 2 ? hi[1] : lo[1], corner & 4 ? hi[2] : lo[2]};
    for (int k = 0; k < 2; ++k) {
      const double x = (((double)frame[4 * k] * v[0] + (double)frame[4 * k + 1] * v[1]) + (double)frame[4 * k + 2] * v[2]) + (double)frame[4 * k + 3];
      m = std::max(m, std::fabs(x));
    }
  }
  if (!(m > 0.0)) return PICK_E_MAX;
  if (!std::isfinite(m)) return PICK_E_MIN;
  int k;
  const double f = frexp(m, &k);  // m = f 2^k, 0.5 <= f < 1
  const int e = 25 - k + (f == 0.5 ? 1 : 0);
  return std::min(std::max(e, PICK_E_MIN), PICK_E_MAX);
}

// The stamp spacing of a pointer path (the reference's ui/brush.py:158-198), in double from fp32 inputs, every result rounded to fp32
// once.  Stamps beyond `cap` are counted and not written.  Returns the number of stamps the hits plan, or -1 for a chord that would be
// cut into more than PATH_MAX_CHORD stamps; *state is advanced only when the plan fits (count <= cap).
inline long long mesh_path_plan(const dtp_mesh_hit* hits, int n, float stamp_distance, dtp_path_state* state, float* pos, float* normal, float* prev,
                                int cap) {
#pragma clang fp contract(off)
  const double sd = (double)stamp_distance;
  bool has = state->has_prev != 0;
  float p[3] = {state->prev[0], state->prev[1], state->prev[2]};
  long long count = 0;
  for (int i = 0; i < n; ++i) {
    const dtp_mesh_hit& h = hits[i];
    if (h.face < 0) continue;  // a miss: skipped
    if (!has) { has = true; p[0] = h.pos[0]; p[1] = h.pos[1]; p[2] = h.pos[2]; continue; }
    const double dl[3] = {(double)h.pos[0] - (double)p[0], (double)h.pos[1] - (double)p[1], (double)h.pos[2] - (double)p[2]};
    const double dist = sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
    if (!(dist >= sd)) continue;  // too near: nothing changes
    const double q = dist / sd;
    if (!(q <= (double)PATH_MAX_CHORD)) return -1;
    const int num = (int)q;
    const double step = dist / (double)num;
    double cur[3] = {(double)p[0], (double)p[1], (double)p[2]};
    for (int k = 0; k < num; ++k, ++count) {
      double next[3];
      for (int c = 0; c < 3; ++c) next[c] = step * (dl[c] / dist) + cur[c];
      if (count < cap)
        for (int c = 0; c < 3; ++c) {
          pos[3 * count + c] = (float)next[c];
          normal[3 * count + c] = h.normal[c];
          prev[3 * count + c] = (float)cur[c];
        }
      for (int c = 0; c < 3; ++c) cur[c] = next[c];
    }
    p[0] = h.pos[0]; p[1] = h.pos[1]; p[2] = h.pos[2];
  }
  if (count <= cap) { state->has_prev = has ? 1 : 0; state->prev[0] = p[0]; state->prev[1] = p[1]; state->prev[2] = p[2]; }
  return count;
}
