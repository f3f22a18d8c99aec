// The host-only arithmetic of the view of a textured mesh (include/dtp.h "a view of a textured mesh": dtp_view_camera, dtp_view_rays,
// dtp_mesh_view): the perspective camera and the rays of its pixels in double, rounded to fp32 once; every argument check
// of a view but the look-up of the mesh; the bins a face's pixel range meets; the pixel range of a face that crosses the near plane; the
// checks of the anti-aliased view and the bin of one of its tiles.  No device call, so the stand-alone sanitizer programs
// (tools/view_host_check.cpp, tools/view_clip_host_check.cpp, tools/view_aa_host_check.cpp) drive it directly, built by a plain C++
// compiler.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <cmath>

#include "../../include/dtp.h"

#ifdef __HIPCC__
#define VIEW_HD __host__ __device__
#else
#define VIEW_HD
#endif

constexpr int VIEW_MAX = 4096;                             // the largest frame side: pixel ranges are packed in 16 bits
constexpr int VIEW_BIN_SHIFT = 6, VIEW_BIN = 1 << VIEW_BIN_SHIFT;  // bins of 64 x 64 pixels = 4 x 4 tiles of 16 x 16
constexpr int VIEW_MAX_BINS = (VIEW_MAX / VIEW_BIN) * (VIEW_MAX / VIEW_BIN);  // 4096: one workgroup scans them
constexpr int VIEW_MAX_TEX = 32768;                        // as the strokes: a texture side
constexpr int VIEW_MAX_ANISO = 16;                         // the most taps of an anisotropic sample (dtp_mesh_view_aniso)

// The bins [bx0, bx1] x [by0, by1] that a face's pixel ranges (x0 | x1 << 16, y0 | y1 << 16; not empty) meet.  true: a SMALL face, at
// most 2 x 2 bins, which gets one entry in each of them; false: a LARGE face, which every tile streams.
VIEW_HD inline bool view_bins(int px, int py, int& bx0, int& bx1, int& by0, int& by1) {
  bx0 = (px & 0xffff) >> VIEW_BIN_SHIFT; bx1 = (px >> 16) >> VIEW_BIN_SHIFT;
  by0 = (py & 0xffff) >> VIEW_BIN_SHIFT; by1 = (py >> 16) >> VIEW_BIN_SHIFT;
  return bx1 - bx0 <= 1 && by1 - by0 <= 1;
}
inline int view_bins_across(int n) { return (n + VIEW_BIN - 1) >> VIEW_BIN_SHIFT; }

// The pixel ranges of a face that CROSSES the near plane (include/dtp.h "a view clipped at the near plane"; c: its camera-space vertices,
// finite, at least one with z <= -near and one nearer).  The face is rasterised in homogeneous form and never cut, so the ranges are used
// for the reject and the bins alone and only have to be conservative: the box of the projections of the polygon cut at z = -near (its
// vertices in front, and where its edges meet the plane: up to four points, in fp32), grown by a pixel and a half and by a bound on the
// rounding of the cut points, which are differences of coordinates divided by near.  true: [x0, x1] x [y0, y1], inclusive pixel indices
// clamped to the frame; the whole frame where an intermediate is not finite.  false: the box misses the frame (nothing written).
VIEW_HD inline bool view_clip_box(const float c[3][3], float fx, float fy, float near, int H, int W, int& x0, int& x1, int& y0, int& y1) {
#pragma clang fp contract(off)
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H, inear = 1.0f / near, big = 3.4028235e38f;
  float lox = big, hix = -big, loy = big, hiy = -big, slack = 0.f;
  bool finite = true;
  for (int k = 0; k < 3; ++k) {
    const float* a = c[k];
    const float* b = c[(k + 1) % 3];
    const bool a_in = a[2] <= -near, b_in = b[2] <= -near;
    for (int cut = 0; cut < 2; ++cut) {
      if (cut == 0 ? !a_in : a_in == b_in) continue;
      float nx, ny, err = 0.f;
      if (cut == 0) {
        const float iw = 1.0f / (0.0f - a[2]);
        nx = (a[0] * fx) * iw; ny = (a[1] * fy) * iw;
      } else {
        const float t = ((0.0f - near) - a[2]) / (b[2] - a[2]);
        nx = ((a[0] + t * (b[0] - a[0])) * fx) * inear; ny = ((a[1] + t * (b[1] - a[1])) * fy) * inear;
        err = fmaxf((((fabsf(a[0]) + fabsf(b[0])) * fx) * inear) * hw, (((fabsf(a[1]) + fabsf(b[1])) * fy) * inear) * hh) * 1e-6f;
      }
      const float sx = (nx + 1.0f) * hw, sy = (1.0f - ny) * hh;
      finite = finite && fabsf(sx) <= big && fabsf(sy) <= big && fabsf(err) <= big;  // (false for a NaN)
      lox = fminf(lox, sx); hix = fmaxf(hix, sx); loy = fminf(loy, sy); hiy = fmaxf(hiy, sy);
      slack = fmaxf(slack, err);
    }
  }
  const float grow = 1.5f + slack;
  const float ax = floorf(lox - grow), bx = ceilf(hix + grow), ay = floorf(loy - grow), by = ceilf(hiy + grow);
  if (!finite || !(fabsf(ax) <= big && fabsf(bx) <= big && fabsf(ay) <= big && fabsf(by) <= big)) {
    x0 = 0; x1 = W - 1; y0 = 0; y1 = H - 1;
    return true;
  }
  if (bx < 0.f || ax > (float)(W - 1) || by < 0.f || ay > (float)(H - 1)) return false;
  x0 = (int)fmaxf(ax, 0.f); x1 = (int)fminf(bx, (float)(W - 1));
  y0 = (int)fmaxf(ay, 0.f); y1 = (int)fminf(by, (float)(H - 1));
  return true;
}

// nullptr, or what is wrong with a camera that was not made by dtp_view_camera
inline const char* view_cam_check(const dtp_view_cam* c) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(c->m[i])) return "the camera matrix is not finite";
  if (!(c->fx > 0.f) || !(c->fy > 0.f) || !std::isfinite(c->fx) || !std::isfinite(c->fy)) return "fx and fy must be finite values > 0";
  if (!(c->near > 0.f) || !std::isfinite(c->near) || !std::isfinite(1.0f / c->near)) return "near must be a finite value > 0 with a finite reciprocal";
  return nullptr;
}
inline const char* view_size_check(int H, int W) {
  return (H < 1 || W < 1 || H > VIEW_MAX || W > VIEW_MAX) ? "the frame's H and W must lie in 1..4096" : nullptr;
}

// The anti-aliased view (include/dtp.h "an anti-aliased view"): samples = the side s of the sample grid of a pixel.  The frame that is
// binned is the FINE one, s H x s W, so that is what has to fit the packed ranges and the bin counters.  nullptr, or what is wrong.
inline const char* view_aa_check(int samples, int H, int W) {
  if (samples != 1 && samples != 2 && samples != 4) return "samples is 1, 2 or 4 (the side of the sample grid of a pixel)";
  if (const char* why = view_size_check(H, W)) return why;
  if (samples * H > VIEW_MAX || samples * W > VIEW_MAX) return "samples * H and samples * W must not exceed 4096";
  return nullptr;
}
// The bin of the fine frame that holds ALL fine pixels of the output tile whose first pixel is (row0, col0) (multiples of 16): the tile
// is 16 s <= 64 fine pixels a side and starts at a multiple of 16 s, so it never straddles a bin.  nbx: view_bins_across(s W).
VIEW_HD inline int view_aa_tile_bin(int s, int row0, int col0, int nbx) {
  return ((s * row0) >> VIEW_BIN_SHIFT) * nbx + ((s * col0) >> VIEW_BIN_SHIFT);
}

// dtp_view_camera: in double from the fp32 inputs, rounded to fp32 once.  b = normalize(eye - at), r = normalize(cross(up, b)),
// u = cross(b, r); m = the rows (r, u, b), each followed by -row . eye; fy = 1 / tan((fov_y pi) / 360), fx = (fy H) / W.
// nullptr and *out written, or what is wrong (nothing written).
inline const char* view_camera(const float eye[3], const float at[3], const float up[3], float fov_y, int H, int W, float near, dtp_view_cam* out) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(eye[i]) || !std::isfinite(at[i]) || !std::isfinite(up[i])) return "a non-finite eye, at or up";
  if (!std::isfinite(fov_y) || !(fov_y > 0.f) || !(fov_y < 180.f)) return "fov_y must lie inside (0, 180) degrees";
  if (!(near > 0.f) || !std::isfinite(near)) return "near must be a finite value > 0";
  if (const char* why = view_size_check(H, W)) return why;
  double e[3], upd[3], b[3], r[3], u[3];
  for (int i = 0; i < 3; ++i) { e[i] = (double)eye[i]; upd[i] = (double)up[i]; b[i] = (double)eye[i] - (double)at[i]; }
  auto norm = [](const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); };
  auto cross = [](const double* a, const double* c, double* o) {
    o[0] = a[1] * c[2] - a[2] * c[1]; o[1] = a[2] * c[0] - a[0] * c[2]; o[2] = a[0] * c[1] - a[1] * c[0];
  };
  const double lb = norm(b), lu = norm(upd);
  if (!(lb > 0.0)) return "eye == at";
  for (int i = 0; i < 3; ++i) b[i] /= lb;
  cross(upd, b, r);
  const double lr = norm(r);
  if (!(lu > 0.0) || !(lr > 1e-9 * lu)) return "up is zero or parallel to the view direction";
  for (int i = 0; i < 3; ++i) r[i] /= lr;
  cross(b, r, u);
  const double* rows[3] = {r, u, b};
  dtp_view_cam c;
  for (int k = 0; k < 3; ++k) {
    for (int i = 0; i < 3; ++i) c.m[4 * k + i] = (float)rows[k][i];
    c.m[4 * k + 3] = (float)-((rows[k][0] * e[0] + rows[k][1] * e[1]) + rows[k][2] * e[2]);
  }
  const double fy = 1.0 / tan(((double)fov_y * M_PI) / 360.0);
  c.fy = (float)fy;
  c.fx = (float)((fy * (double)H) / (double)W);
  c.near = near;
  if (view_cam_check(&c)) return "the camera does not fit fp32";
  *out = c;
  return nullptr;
}

// dtp_view_rays: the ray of pixel position (x, y) -- the centre of pixel (i, j) is (j + 0.5, i + 0.5) -- in double from the fp32 camera,
// rounded to fp32 once: origin = the eye, -((r t_r + u t_u) + b t_b) with t the fourth column; direction = (r (ndc_x / fx) + u (ndc_y /
// fy)) - b with ndc_x = (2 x) / W - 1, ndc_y = 1 - (2 y) / H.  nullptr and out[0 .. n - 1] written, or what is wrong (nothing written).
inline const char* view_rays(const dtp_view_cam* cam, int H, int W, const float* xy, int n, dtp_ray* out, int* bad) {
#pragma clang fp contract(off)
  *bad = -1;
  if (const char* why = view_cam_check(cam)) return why;
  if (const char* why = view_size_check(H, W)) return why;
  if (n < 1) return "n must be at least 1";
  for (int i = 0; i < 2 * n; ++i)
    if (!std::isfinite(xy[i])) { *bad = i / 2; return "a non-finite pixel position"; }
  double m[12];
  for (int i = 0; i < 12; ++i) m[i] = (double)cam->m[i];
  float eye[3];
  for (int i = 0; i < 3; ++i) eye[i] = (float)-((m[i] * m[3] + m[4 + i] * m[7]) + m[8 + i] * m[11]);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(eye[i])) return "the eye does not fit fp32";
  const double fx = (double)cam->fx, fy = (double)cam->fy;
  for (int k = 0; k < n; ++k) {
    const double nx = (2.0 * (double)xy[2 * k]) / (double)W - 1.0, ny = 1.0 - (2.0 * (double)xy[2 * k + 1]) / (double)H;
    const double a = nx / fx, c = ny / fy;
    for (int i = 0; i < 3; ++i) {
      out[k].origin[i] = eye[i];
      out[k].dir[i] = (float)((m[i] * a + m[4 + i] * c) - m[8 + i]);
    }
  }
  return nullptr;
}

// Every check of dtp_mesh_view that needs no mesh: nullptr, or what is wrong.
inline const char* view_check(const void* texture, int TH, int TW, const dtp_view_cam* cam, int H, int W, const dtp_view_opts* o, const void* image,
                              const void* face_idx, const void* depth) {
  if (!texture || !cam || !o || !image) return "NULL argument (mesh, texture, cam, opts and image are required)";
  if (const char* why = view_size_check(H, W)) return why;
  if (TH < 1 || TW < 1 || TH > VIEW_MAX_TEX || TW > VIEW_MAX_TEX) return "the texture's TH and TW must lie in 1..32768";
  if (((uintptr_t)texture & 3) != 0 || ((uintptr_t)image & 3) != 0 || ((uintptr_t)face_idx & 3) != 0 || ((uintptr_t)depth & 3) != 0)
    return "texture, image, face_idx and depth must be 4-byte aligned";
  if (const char* why = view_cam_check(cam)) return why;
  if ((o->cull != 0 && o->cull != 1) || (o->flip_normals != 0 && o->flip_normals != 1) || (o->shade != 0 && o->shade != 1))
    return "cull, flip_normals and shade are 0 or 1";
  if (!(o->ambient >= 0.f) || !(o->ambient <= 1.f)) return "ambient must lie in 0..1";
  return nullptr;
}
