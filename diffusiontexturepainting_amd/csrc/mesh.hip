// Strokes on a textured mesh (dtp_mesh_stroke): what the reference's Kit app does around every stamp when it paints on a
// mesh (kit_app/.../python/manager.py:199-271, util/render.py:22-178: an orthographic look-at camera at the brush, a rasterisation of the
// mesh into the R x R stamp window with the texture sampled through the interpolated UVs, generate_raw, and a second rasterisation of
// the visible faces in UV space that carries the painted stamp back into the texture).  The reference's two rasterisations are kaolin's;
// these are written from the contract of include/dtp.h: coverage in exact integer arithmetic on vertices snapped to 1/256 pixel,
// interpolation in fp32 one rounded operation at a time (contraction is off for this whole file), a winner per pixel that does not depend
// on the order in which faces are visited.  Plain HIP: vector loads, stores and atomics only.
// This file holds the mesh object (mesh_obj.h) and the stroke; the bleed pass that may follow a backprojection is
// mesh_bleed.hip's, picking is mesh_pick.hip's.
// Masked strokes (dtp_mesh_stroke_masked): a face set keeps the faces whose bit is 0 out of the valid list; nothing else
// of a stamp changes.  The lasso that makes a set and the tint that shows one are select.hip's.
// Occluded strokes (dtp_mesh_stroke_occluded): a second instantiation of the backprojection kernel leaves out the taps
// that show a face in front of the texel's own; the render, the valid list, the bleed pass and the journal hook do not know of it.
#pragma clang fp contract(off)
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "mesh_obj.h"
#include "select_host.h"

namespace {

struct MeshCam { float m[12], fov; };  // travels as a kernel argument

std::mutex g_mu;
std::set<Mesh*> g_meshes;  // the live meshes: a destroyed handle is refused, not followed

// ---------------------------------------------------------------- device: the kernels (the shared arithmetic: mesh_dev.h)
__global__ void mesh_reset_kernel(MeshState* st) {
  st->n_win = 0; st->n_val = 0;
  st->bb[0] = st->bb[1] = 0x7fffffff; st->bb[2] = st->bb[3] = -1;
}

// One thread per face: camera space, the unit normal's z, NDC, the snapped window position; the faces that are front, have an area in
// the window and a pixel centre inside their bounding box are appended to `win` (in any order: the render does not depend on it).
__global__ __launch_bounds__(256) void mesh_project_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int F, MeshCam cam,
                                                           int R, int flip, FaceRec* __restrict__ rec, int* __restrict__ owned,
                                                           int4* __restrict__ win, MeshState* st) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  float c[3][3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = verts + (size_t)3 * faces[(size_t)3 * f + k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      c[k][r] = ((cam.m[4 * r] * v[0] + cam.m[4 * r + 1] * v[1]) + cam.m[4 * r + 2] * v[2]) + cam.m[4 * r + 3];
      finite = finite && isfinite(c[k][r]);
    }
  }
  const float e1x = c[1][0] - c[0][0], e1y = c[1][1] - c[0][1], e1z = c[1][2] - c[0][2];
  const float e2x = c[2][0] - c[0][0], e2y = c[2][1] - c[0][1], e2z = c[2][2] - c[0][2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  float nzu = nz / __fsqrt_rn((nx * nx + ny * ny) + nz * nz);  // a zero area: 0 / 0
  if (flip) nzu = -nzu;
  const bool raster = finite && isfinite(nzu);
  FaceRec r;
  const float half = 128.0f * (float)R;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.z[k] = c[k][2];
    r.nx[k] = c[k][0] / cam.fov;
    r.ny[k] = c[k][1] / cam.fov;
    r.X[k] = snap((r.nx[k] + 1.0f) * half);
    r.Y[k] = snap((1.0f - r.ny[k]) * half);
  }
  r.flags = raster ? (MF_RASTER | (nzu >= 0.0f ? MF_FRONT : 0) | (nzu >= 0.5f ? MF_UPRIGHT : 0)) : 0;
  rec[f] = r;
  owned[f] = 0;
  if (!(r.flags & MF_FRONT) || orient(r.X[0], r.Y[0], r.X[1], r.Y[1], r.X[2], r.Y[2]) == 0) return;
  int x0, x1, y0, y1;
  centre_range(min3(r.X[0], r.X[1], r.X[2]), max3(r.X[0], r.X[1], r.X[2]), R, x0, x1);
  centre_range(min3(r.Y[0], r.Y[1], r.Y[2]), max3(r.Y[0], r.Y[1], r.Y[2]), R, y0, y1);
  if (x0 > x1 || y0 > y1) return;
  const int at = atomicAdd(&st->n_win, 1);
  if (at < F) win[at] = pack_box(f, x0, x1, y0, y1);  // (always, unless two renders of one mesh race)
}

// One workgroup per 16 x 16 pixel tile, one thread per pixel.  The window's faces stream through LDS CHUNK at a time; a face whose pixel
// range misses the tile is dropped on the way in.  Winner: the largest (camera z, -face index) among the front faces that cover the
// centre.  canvas f32 [4][R][R] = the bilinear sample of the texture at the interpolated UV (0 x 4 where no face is, and in an Overpaint
// window's inner rectangle); face_idx i32 [R][R]; owned[f] = 1 for every winner (the same value from every writer).
__global__ __launch_bounds__(256) void mesh_render_kernel(const FaceRec* __restrict__ rec, const int4* __restrict__ win, const MeshState* st, int F,
                                                          const float* __restrict__ uvs, const unsigned int* __restrict__ tex, int H, int W,
                                                          int R, int overpaint, int over_y, int over_x, float* __restrict__ canvas,
                                                          int* __restrict__ face_idx, int* __restrict__ owned) {
  __shared__ int s_n, s_face[CHUNK], s_X[CHUNK][3], s_Y[CHUNK][3];
  __shared__ float s_z[CHUNK][3];
  const int t = threadIdx.x, col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
  const int col = col0 + (t & 15), row = row0 + (t >> 4);
  const bool live = col < R && row < R;
  const int px = 256 * col + 128, py = 256 * row + 128;
  const int n_win = min(st->n_win, F);
  int best = -1;
  float best_z = 0.f, bw[3] = {0.f, 0.f, 0.f};
  stream_faces(win, n_win, col0, row0, live, s_n,
      [&](int slot, const int4& e) {
        const FaceRec& r = rec[e.x];
        s_face[slot] = e.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_X[slot][k] = r.X[k]; s_Y[slot][k] = r.Y[k]; s_z[slot][k] = r.z[k]; }
      },
      [&](int i) {
        float w[3];
        if (!cover(s_X[i], s_Y[i], px, py, w)) return;
        const float z = interp(w, s_z[i][0], s_z[i][1], s_z[i][2]);
        const int f = s_face[i];
        if (best < 0 || z > best_z || (z == best_z && f < best)) { best = f; best_z = z; bw[0] = w[0]; bw[1] = w[1]; bw[2] = w[2]; }
      });
  if (!live) return;
  const size_t RR = (size_t)R * R, pix = (size_t)row * R + col;
  face_idx[pix] = best;
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  if (best >= 0) {
    owned[best] = 1;
    const bool blank = overpaint && row >= over_y && row < R - over_y && col >= over_x && col < R - over_x;
    if (!blank) {
      const float* uv = uvs + (size_t)6 * best;
      const float u = interp(bw, uv[0], uv[2], uv[4]), v = interp(bw, uv[1], uv[3], uv[5]);
      sample_bilinear(tex, H, W, u, v, out);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) canvas[(size_t)ch * RR + pix] = out[ch];
}

// The faces that are backprojected (get_valid_faces, render.py:113-130): front, not steep, and the winner of at least one pixel; with a
// face set `sel` (or null: every face) also selected: bit f % 32 of word f / 32.  Those with a texel centre in their UV
// bounding box go to `val`, and the union of their texel ranges to st->bb.
__global__ __launch_bounds__(256) void mesh_valid_kernel(const FaceRec* __restrict__ rec, const int* __restrict__ owned,
                                                         const int4* __restrict__ win, const float* __restrict__ uvs, int F, int H,
                                                         int W, int4* __restrict__ val, MeshState* st, const unsigned int* __restrict__ sel) {
  const int n_win = min(st->n_win, F);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_win; i += gridDim.x * 256) {
    const int f = win[i].x;
    if ((rec[f].flags & (MF_FRONT | MF_UPRIGHT)) != (MF_FRONT | MF_UPRIGHT) || !owned[f]) continue;
    if (sel && !((sel[f >> 5] >> (f & 31)) & 1u)) continue;  // (f < F: inside the set's (F + 31) / 32 words)
    int X[3], Y[3], x0, x1, y0, y1;
    if (!face_texels(uvs + (size_t)6 * f, H, W, X, Y, x0, x1, y0, y1)) continue;
    const int at = atomicAdd(&st->n_val, 1);
    if (at < F) val[at] = pack_box(f, x0, x1, y0, y1);
    atomicMin(&st->bb[0], x0); atomicMin(&st->bb[1], y0); atomicMax(&st->bb[2], x1); atomicMax(&st->bb[3], y1);
  }
}

// One workgroup per 16 x 16 texel tile; a tile outside the valid faces' bounding box leaves at once.  Per texel the lowest valid face
// index that covers its centre (all depths are equal) gives (p, q) = the face's stamp NDC / 2 + 0.5; the stamp image -- RGB the decoder's
// clamped value, A = mask * (face_idx != -1) -- is sampled there, and where the sampled A is > 0 all four bytes of the texel become
// (unsigned char)(min(v, 1) * 255.0f); dec == null (Erase): 0 x 4 instead.  Other texels are neither read nor written.  `finished`: dec
// holds the clamped 0..1 values already (dtp_op_mesh_backproject on what dtp_stamp returned).
//   OCC (the occluded instantiation): a tap whose pixel shows another face g that lies in front of the texel's face f by
// more than `tol` at that pixel's centre -- both planes by weights_at from rec[g] and rec[f], which is re-read here after the loop, not
// staged -- is rejected; a texel with a rejected tap blends the remaining taps and divides by the sum of their weights.  A texel without
// one runs the arithmetic of the plain instantiation, operation for operation; OCC false compiles to the kernel this was before.
template <bool OCC>
__device__ __forceinline__ void backproject_texel(const FaceRec* __restrict__ rec, const int4* __restrict__ val, const MeshState* st, int F,
                                                  const float* __restrict__ uvs, const float* __restrict__ dec, int finished,
                                                  const unsigned char* __restrict__ mask, const int* __restrict__ face_idx, int R,
                                                  unsigned int* __restrict__ tex, int H, int W, float tol) {
  __shared__ int s_n, s_face[CHUNK], s_X[CHUNK][3], s_Y[CHUNK][3];
  __shared__ float s_p[CHUNK][3], s_q[CHUNK][3];
  const int t = threadIdx.x, col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
  const int n_val = min(st->n_val, F);
  if (n_val == 0 || col0 > st->bb[2] || col0 + 15 < st->bb[0] || row0 > st->bb[3] || row0 + 15 < st->bb[1]) return;  // (uniform)
  const int col = col0 + (t & 15), row = row0 + (t >> 4);
  const bool live = col < W && row < H;
  const int px = 256 * col + 128, py = 256 * row + 128;
  int best = -1;
  float p = 0.f, q = 0.f;
  for (int base = 0; base < n_val; base += CHUNK) {  // (stream_faces' loop in its own text: through it the plain kernel takes 33 VGPRs, not 36)
    if (t == 0) s_n = 0;
    __syncthreads();
    if (base + t < n_val) {
      const int4 e = val[base + t];
      if (ranges_meet(e.y, col0, col0 + 15) && ranges_meet(e.z, row0, row0 + 15)) {
        const int slot = atomicAdd(&s_n, 1);
        const FaceRec& r = rec[e.x];
        s_face[slot] = e.x;
        snap_uvs(uvs + (size_t)6 * e.x, H, W, s_X[slot], s_Y[slot]);
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_p[slot][k] = r.nx[k] / 2.0f + 0.5f; s_q[slot][k] = r.ny[k] / 2.0f + 0.5f; }
      }
    }
    __syncthreads();
    const int n = s_n;
    if (live)
      for (int i = 0; i < n; ++i) {
        const int f = s_face[i];
        float w[3];
        if ((best >= 0 && f > best) || !cover(s_X[i], s_Y[i], px, py, w)) continue;
        best = f;
        p = interp(w, s_p[i][0], s_p[i][1], s_p[i][2]);
        q = interp(w, s_q[i][0], s_q[i][1], s_q[i][2]);
      }
    __syncthreads();
  }
  if (!live || best < 0) return;
  const Taps tp = taps(p * (float)R - 0.5f, (1.0f - q) * (float)R - 0.5f, R, R);
  const int i00 = tp.y0 * R + tp.x0, i01 = tp.y0 * R + tp.x1, i10 = tp.y1 * R + tp.x0, i11 = tp.y1 * R + tp.x1;
  auto alpha = [&](int i) { return (mask[i] != 0 && face_idx[i] != -1) ? 1.0f : 0.0f; };
  Taps tq = tp;        // the taps a rejection left (OCC); tp itself otherwise
  bool renorm = false;  // a tap was rejected: every blend is divided by S, the sum of the weights left
  float S = 1.0f;
  if constexpr (OCC) {
    const int ti[4] = {i00, i01, i10, i11}, tx[4] = {tp.x0, tp.x1, tp.x0, tp.x1}, ty[4] = {tp.y0, tp.y0, tp.y1, tp.y1};
    bool rej[4] = {false, false, false, false};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int g = face_idx[ti[k]];
      if (g == best || (unsigned int)g >= (unsigned int)F) continue;  // (-1, and any value that is no face of the mesh: never an index)
      const FaceRec &rg = rec[g], &rf = rec[best];
      const int cx = 256 * tx[k] + 128, cy = 256 * ty[k] + 128;
      float wg[3], wf[3];
      if (!weights_at(rg.X, rg.Y, cx, cy, wg) || !weights_at(rf.X, rf.Y, cx, cy, wf)) continue;  // (both won a pixel: never)
      const float zg = interp(wg, rg.z[0], rg.z[1], rg.z[2]), zf = interp(wf, rf.z[0], rf.z[1], rf.z[2]);
      rej[k] = (zg - zf) > tol;  // (a NaN does not reject)
    }
    if (rej[0] || rej[1] || rej[2] || rej[3]) {
      renorm = true;
      if (rej[0]) tq.w00 = 0.f;
      if (rej[1]) tq.w01 = 0.f;
      if (rej[2]) tq.w10 = 0.f;
      if (rej[3]) tq.w11 = 0.f;
      S = ((tq.w00 + tq.w01) + tq.w10) + tq.w11;
      if (!(S > 0.f)) return;
    }
  }
  float a = blend(tq, alpha(i00), alpha(i01), alpha(i10), alpha(i11));
  if (OCC && renorm) a = a / S;
  if (!(a > 0.f)) return;
  unsigned int texel = 0u;
  if (dec) {
    texel = (unsigned int)(unsigned char)(fminf(a, 1.0f) * 255.0f) << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float d00 = dec[(size_t)i00 * 4 + ch], d01 = dec[(size_t)i01 * 4 + ch], d10 = dec[(size_t)i10 * 4 + ch], d11 = dec[(size_t)i11 * 4 + ch];
      float v = finished ? blend(tq, d00, d01, d10, d11) : blend(tq, finish_value(d00), finish_value(d01), finish_value(d10), finish_value(d11));
      if (OCC && renorm) v = v / S;
      texel |= (unsigned int)(unsigned char)(fminf(v, 1.0f) * 255.0f) << (8 * ch);
    }
  }
  tex[(size_t)row * W + col] = texel;
}

__global__ __launch_bounds__(256) void mesh_backproject_kernel(const FaceRec* __restrict__ rec, const int4* __restrict__ val,
                                                               const MeshState* st, int F, const float* __restrict__ uvs,
                                                               const float* __restrict__ dec, int finished,
                                                               const unsigned char* __restrict__ mask,
                                                               const int* __restrict__ face_idx, int R, unsigned int* __restrict__ tex,
                                                               int H, int W) {
  backproject_texel<false>(rec, val, st, F, uvs, dec, finished, mask, face_idx, R, tex, H, W, 0.f);
}

// the same with the occlusion test (dtp_mesh_stroke_occluded): tol, in camera units, is the host's occlude 2 fov / R
__global__ __launch_bounds__(256) void mesh_backproject_occluded_kernel(const FaceRec* __restrict__ rec, const int4* __restrict__ val,
                                                                        const MeshState* st, int F, const float* __restrict__ uvs,
                                                                        const float* __restrict__ dec, int finished,
                                                                        const unsigned char* __restrict__ mask,
                                                                        const int* __restrict__ face_idx, int R,
                                                                        unsigned int* __restrict__ tex, int H, int W, float tol) {
  backproject_texel<true>(rec, val, st, F, uvs, dec, finished, mask, face_idx, R, tex, H, W, tol);
}

// the Erase stamp's default mask: the analytic disc of radius R / 2 - 2 around the window's centre (the shape of the Kit app's circle_mask,
// manager.py:48-52, which PIL draws), in integers: (2 i - (R - 1))^2 + (2 j - (R - 1))^2 <= (R - 4)^2
__global__ void mesh_disc_kernel(unsigned char* __restrict__ mask, int R) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < R * R; i += gridDim.x * 256) {
    const long long dy = 2 * (i / R) - (R - 1), dx = 2 * (i % R) - (R - 1), d = R - 4;
    mask[i] = (dy * dy + dx * dx <= d * d) ? 1 : 0;
  }
}

// ---------------------------------------------------------------- host
bool known_mode(int m) { return m == DTP_STROKE_INPAINT || m == DTP_STROKE_ERASE || m == DTP_STROKE_OVERPAINT; }

// make_camera (manager.py:199-227) in double, rounded to fp32 once: out = the rows (r, u, b) of the view matrix, each followed by its
// translation -row . eye.  `stamp` >= 0 names the stamp in a refusal.
int make_camera(const char* who, int stamp, const float* pos, const float* normal, const float* prev, float fov, float out[12]) {
  char at[32] = "";
  if (stamp >= 0) snprintf(at, sizeof at, "stamp %d: ", stamp);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(pos[i]) || !std::isfinite(normal[i]) || !std::isfinite(prev[i])) {
      dtp_set_error("%s: %sa non-finite position, normal or previous position", who, at);
      return DTP_ERR_ARG;
    }
  if (!(fov > 0.f) || !std::isfinite(fov)) { dtp_set_error("%s: %sfov=%g (a finite value > 0)", who, at, (double)fov); return DTP_ERR_ARG; }
  double eye[3], up[3], b[3], r[3], u[3];
  for (int i = 0; i < 3; ++i) { eye[i] = (double)pos[i] + (double)normal[i]; up[i] = (double)prev[i] - (double)pos[i]; b[i] = eye[i] - (double)pos[i]; }
  auto norm = [](const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); };
  auto cross = [](const double* a, const double* c, double* o) {
    o[0] = a[1] * c[2] - a[2] * c[1]; o[1] = a[2] * c[0] - a[0] * c[2]; o[2] = a[0] * c[1] - a[1] * c[0];
  };
  const double lb = norm(b), lu = norm(up);
  if (!(lb > 0.0)) { dtp_set_error("%s: %sthe normal is zero", who, at); return DTP_ERR_ARG; }
  for (int i = 0; i < 3; ++i) b[i] /= lb;
  cross(up, b, r);
  const double lr = norm(r);
  if (!(lu > 0.0) || !(lr > 1e-9 * lu)) {
    dtp_set_error("%s: %sup = prev - pos is zero or parallel to the normal", who, at);
    return DTP_ERR_ARG;
  }
  for (int i = 0; i < 3; ++i) r[i] /= lr;
  cross(b, r, u);
  const double* rows[3] = {r, u, b};
  for (int k = 0; k < 3; ++k) {
    for (int i = 0; i < 3; ++i) out[4 * k + i] = (float)rows[k][i];
    out[4 * k + 3] = (float)-((rows[k][0] * eye[0] + rows[k][1] * eye[1]) + rows[k][2] * eye[2]);
  }
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(out[i])) { dtp_set_error("%s: %sthe camera does not fit fp32", who, at); return DTP_ERR_ARG; }
  return DTP_OK;
}

// Can the window see the mesh at all?  The eight corners of the vertices' bounding box through the fp32 camera, in double, against the
// NDC square with a margin far above the fp32 error of the device's projection.  false: no face can cover a pixel centre.
bool box_meets_window(const Mesh* m, const float cam[12], float fov, int R) {
  double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300}, big = 0.0;
  for (int corner = 0; corner < 8; ++corner) {
    const double v[3] = {corner & 1 ? m->hi[0] : m->lo[0], corner & 2 ? m->hi[1] : m->lo[1], corner & 4 ? m->hi[2] : m->lo[2]};
    for (int k = 0; k < 2; ++k) {
      double mag = std::fabs((double)cam[4 * k + 3]);
      for (int i = 0; i < 3; ++i) mag += std::fabs(cam[4 * k + i] * v[i]);
      const double x = (cam[4 * k] * v[0] + cam[4 * k + 1] * v[1] + cam[4 * k + 2] * v[2] + cam[4 * k + 3]) / fov;
      lo[k] = std::min(lo[k], x); hi[k] = std::max(hi[k], x); big = std::max(big, mag / fov);
    }
  }
  const double slack = 4.0 / R + 1e-5 * big;
  if (!std::isfinite(big)) return true;
  return lo[0] <= 1.0 + slack && hi[0] >= -1.0 - slack && lo[1] <= 1.0 + slack && hi[1] >= -1.0 - slack;
}

void mesh_free(Mesh* m) {
  (void)hipFree(m->verts); (void)hipFree(m->faces); (void)hipFree(m->uvs); (void)hipFree(m->rec); (void)hipFree(m->owned);
  (void)hipFree(m->win); (void)hipFree(m->val); (void)hipFree(m->state); (void)hipFree(m->cov);
  (void)hipFree(m->sel_poly);
  (void)hipFree(m->pick_rays); (void)hipFree(m->pick_slots); (void)hipFree(m->pick_out);
  if (m->pick_host) (void)hipHostFree(m->pick_host);
  view_free(m->view);
  topo_free(m->topo);
  delete m;
}

int check_over(const char* who, int stamp, int mode, int over_y, int over_x, int R) {
  if (mode == DTP_STROKE_OVERPAINT && (over_y < 1 || over_y >= R / 2 || over_x < 1 || over_x >= R / 2)) {
    dtp_set_error("%s: stamp %d is an Overpaint stamp and over_y=%d / over_x=%d lie outside [1, %d)", who, stamp, over_y, over_x, R / 2);
    return DTP_ERR_ARG;
  }
  return DTP_OK;
}

// reset -> project -> render of one window (arguments checked by the callers)
int enqueue_render(Mesh* m, const float cam[12], float fov, int flip, const unsigned char* texture, int H, int W, int R, int mode, int over_y,
                   int over_x, float* canvas, int* face_idx, hipStream_t s) {
  MeshCam mc;
  memcpy(mc.m, cam, sizeof mc.m);
  mc.fov = fov;
  hipLaunchKernelGGL(mesh_reset_kernel, dim3(1), dim3(1), 0, s, m->state);
  hipLaunchKernelGGL(mesh_project_kernel, dim3((m->F + 255) / 256), dim3(256), 0, s, m->verts, m->faces, m->F, mc, R, flip, m->rec, m->owned,
                     m->win, m->state);
  const int tiles = (R + 15) / 16;
  hipLaunchKernelGGL(mesh_render_kernel, dim3(tiles, tiles), dim3(256), 0, s, m->rec, m->win, m->state, m->F, m->uvs, (const unsigned int*)texture, H, W,
                     R, mode == DTP_STROKE_OVERPAINT ? 1 : 0, over_y, over_x, canvas, face_idx, m->owned);
  return launch_ok();
}

// One backprojection of the window rendered last on a mesh.  dec null: erase.  journal (or null): the one whose open record guards this
// texture; the tiles of the valid faces' texel box grown by `grow` are saved before they are written; a bleed pass of that radius follows (0: none).
// sel (or null), of mask_words words: the face set outside which no face is valid.  occluded: the kernel with the occlusion test, at tol.
struct BackprojectCall {
  const float* dec; int finished; const unsigned char* mask; const int* face_idx; int R; unsigned char* texture; int H, W;
  Journal* journal = nullptr; int grow = 0; const uint32_t* sel = nullptr; int mask_words = 0; bool occluded = false; float tol = 0.f;
};

// valid (-> journal) -> backproject (-> bleed)
int enqueue_backproject(Mesh* m, const BackprojectCall& b, hipStream_t s) {
  const dim3 tiles((b.W + 15) / 16, (b.H + 15) / 16);
  unsigned int* tex = (unsigned int*)b.texture;
  hipLaunchKernelGGL(mesh_valid_kernel, dim3(std::min((m->F + 255) / 256, 1024)), dim3(256), 0, s, m->rec, m->owned, m->win, m->uvs, m->F, b.H,
                     b.W, m->val, m->state, b.sel);
  if (b.journal) RC(journal_save_box(b.journal, m->state->bb, b.grow, s));
  if (b.occluded)
    hipLaunchKernelGGL(mesh_backproject_occluded_kernel, tiles, dim3(256), 0, s, m->rec, m->val, m->state, m->F, m->uvs, b.dec, b.finished, b.mask,
                       b.face_idx, b.R, tex, b.H, b.W, b.tol);
  else
    hipLaunchKernelGGL(mesh_backproject_kernel, tiles, dim3(256), 0, s, m->rec, m->val, m->state, m->F, m->uvs, b.dec, b.finished, b.mask, b.face_idx,
                       b.R, tex, b.H, b.W);
  RC(launch_ok());
  return b.grow ? enqueue_bleed(m, b.texture, b.H, b.W, b.grow, nullptr, s) : DTP_OK;
}

// the occlusion test's setting, before anything else of a call is looked at
int check_occlude(const char* who, float occlude) {
  if (!mesh_occlude_ok(occlude)) { dtp_set_error("%s: occlude=%g (a finite value >= 0, in stamp pixels)", who, (double)occlude); return DTP_ERR_ARG; }
  return DTP_OK;
}

int disc_mask(Ctx* c, hipStream_t s, const unsigned char** out) {
  if (!c->mesh_disc) {
    void* p;
    RC(ctx_persistent(c, (size_t)c->R * c->R, &p, false));
    hipLaunchKernelGGL(mesh_disc_kernel, dim3((c->R * c->R + 255) / 256), dim3(256), 0, s, (unsigned char*)p, c->R);
    RC(launch_ok());
    c->mesh_disc = (unsigned char*)p;
  }
  *out = c->mesh_disc;
  return DTP_OK;
}

// one stamp of a mesh stroke: the storage its StampPlan points into
struct MeshStep {
  float cam[12];
  bool skip = false;  // the window misses the mesh's bounding box
  float tol = 0.f;    // the occlusion test's tolerance at this stamp's fov (dtp_mesh_stroke_occluded)
  dtp_settings st;
  uint64_t seed = 0;
  int slot = 0;
  StampPlan plan;
};

// a caller's face set (or null: none) against the mesh: (F + 31) / 32 words, 4-byte aligned
int check_face_mask(const char* who, const Mesh* m, const uint32_t* face_mask, int mask_words) {
  char why[160];
  if (face_mask && select_check_set(face_mask, mask_words, m->F, why)) { dtp_set_error("%s: face_mask: %s", who, why); return DTP_ERR_ARG; }
  return DTP_OK;
}

// A mesh stroke, as its four entry points ask for it: dtp_mesh_stroke fills the first line, dtp_mesh_stroke_bleed adds bleed,
// dtp_mesh_stroke_masked face_mask (or null: no set) and dtp_mesh_stroke_occluded the occlusion test.  `who` names the entry point in a refusal.
struct StrokeCall {
  const char* who; dtp_ctx* ctx; dtp_mesh* mesh; uint8_t* texture; int H, W; const dtp_mesh_stamp* stamps; int n; const dtp_settings* st;
  const dtp_mesh_stroke_opts* o; const uint8_t* paste_mask; dtp_stream s;
  int bleed = 0; const uint32_t* face_mask = nullptr; int mask_words = 0; bool occluded = false; float occlude = 0.f;
};

int mesh_stroke(const StrokeCall& k) {
  Ctx* c = (Ctx*)k.ctx;
  Mesh* m = (Mesh*)k.mesh;
  hipStream_t s = (hipStream_t)k.s;
  // ---- every check, before anything is enqueued
  RC(check_bleed(k.who, k.bleed));
  if (k.occluded) RC(check_occlude(k.who, k.occlude));
  if (!c || !m || !k.texture || !k.stamps || !k.st || !k.o) {
    dtp_set_error("%s: NULL argument (ctx, mesh, texture, stamps, st and o are required)", k.who);
    return DTP_ERR_ARG;
  }
  if (!c->finalized) { dtp_set_error("%s: weights not finalized", k.who); return DTP_ERR_STATE; }
  RC(check_mesh(k.who, m));
  if (m->ctx != c) { dtp_set_error("%s: the mesh belongs to another handle", k.who); return DTP_ERR_ARG; }
  RC(check_face_mask(k.who, m, k.face_mask, k.mask_words));
  const int R = c->R;
  RC(check_texture(k.who, k.texture, k.H, k.W));
  if (k.n < 1) { dtp_set_error("%s: n=%d stamps (at least 1)", k.who, k.n); return DTP_ERR_ARG; }
  if (R > MAX_WIN) { dtp_set_error("%s: resolution %d above %d", k.who, R, MAX_WIN); return DTP_ERR_ARG; }
  if (k.o->margin < 0 || k.o->margin >= R / 2) { dtp_set_error("%s: margin=%d outside [0, %d)", k.who, k.o->margin, R / 2); return DTP_ERR_ARG; }
  std::vector<MeshStep> steps(k.n);
  int evals = 0;
  bool any_erase = false, any_stamp = false;
  for (int i = 0; i < k.n; ++i) {
    const dtp_mesh_stamp& t = k.stamps[i];
    MeshStep& q = steps[i];
    if (!known_mode(t.mode)) {
      dtp_set_error("%s: stamp %d has unknown mode %d (INPAINT = 0, ERASE = 1, OVERPAINT = 2)", k.who, i, t.mode);
      return DTP_ERR_ARG;
    }
    RC(check_over(k.who, i, t.mode, k.o->over_y, k.o->over_x, R));
    RC(make_camera(k.who, i, t.pos, t.normal, t.prev, t.fov, q.cam));
    if (k.occluded && !mesh_occlude_tol(k.occlude, t.fov, R, &q.tol)) {
      dtp_set_error("%s: stamp %d: the tolerance of occlude=%g at fov=%g does not fit fp32", k.who, i, (double)k.occlude, (double)t.fov);
      return DTP_ERR_ARG;
    }
    q.skip = !box_meets_window(m, q.cam, t.fov, R);
    if (t.mode == DTP_STROKE_ERASE) { any_erase = any_erase || !q.skip; continue; }  // (runs no stamp: its slot and seed are unused)
    if (t.slot < 0 || t.slot >= DTP_MAX_SLOTS) { dtp_set_error("%s: slot %d of stamp %d outside 0..%d", k.who, t.slot, i, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
    if (!c->slot_set[t.slot]) {
      dtp_set_error("%s: stamp %d: no brush set in slot %d (call dtp_set_brush / dtp_set_conditioning)", k.who, i, t.slot);
      return DTP_ERR_STATE;
    }
    // the stamp, as dtp_stamp_seeded would stage it, with the two hooks
    q.st = *k.st; q.seed = t.seed; q.slot = t.slot;
    StampPlan& p = q.plan;
    p.st = &q.st; p.B = 1; p.slot_ids = &q.slot; p.strength = k.o->strength;
    p.seeded = true; p.seeds = &q.seed; p.sample_vae = k.o->sample_vae != 0;
    p.canvas_staged = true;
    p.paste = [](const float*, int, int, hipStream_t) { return DTP_OK; };  // (set for the checks; the launcher proper follows below)
    const int rc = stamp_plan(c, p);
    if (rc) {  // dtp_stamp_seeded's refusal and code, with the stamp it is about
      const std::string why = dtp_last_error();
      dtp_set_error("%s: stamp %d: %s", k.who, i, why.c_str());
      return rc;
    }
    if (!q.skip) { evals += p.E; any_stamp = true; }
  }
  // ---- enqueue: per stamp reset -> project -> render -> stamp -> valid -> backproject (-> bleed); the stream orders the stamps
  HIP_CHECK(hipSetDevice(c->device));
  if (k.bleed && (any_stamp || any_erase)) RC(ensure_coverage(m, k.H, k.W, s));
  const unsigned char *square = k.paste_mask, *disc = k.paste_mask;
  if (!k.paste_mask && any_stamp) RC(stroke_default_mask(c, k.o->margin, s, &square));
  if (!k.paste_mask && any_erase) RC(disc_mask(c, s, &disc));
  Journal* journal = journal_armed(c, k.texture, k.H, k.W);
  for (int i = 0; i < k.n; ++i) {
    const dtp_mesh_stamp& t = k.stamps[i];
    MeshStep& q = steps[i];
    if (q.skip) continue;
    RC(enqueue_render(m, q.cam, t.fov, k.o->flip_normals != 0, k.texture, k.H, k.W, R, t.mode, k.o->over_y, k.o->over_x, c->canvas32, c->mesh_face_idx, s));
    // (the erase stamp's call; the paste hook keeps its own copy, and gets the decoder's output when it runs)
    BackprojectCall b{nullptr, 0, disc, c->mesh_face_idx, R, k.texture, k.H, k.W, journal, k.bleed, k.face_mask, k.mask_words, k.occluded, q.tol};
    if (t.mode == DTP_STROKE_ERASE) { RC(enqueue_backproject(m, b, s)); continue; }
    b.mask = square;
    q.plan.paste = [m, b](const float* dec, int, int, hipStream_t q_s) mutable { b.dec = dec; return enqueue_backproject(m, b, q_s); };
    RC(stamp_enqueue(c, q.plan, s));
  }
  c->last_stroke_stamps = k.n; c->last_stroke_groups = k.n; c->last_stroke_evals = evals;
  return DTP_OK;
}

// The three dtp_op_mesh_backproject*, b as the entry point filled it; list: what its NULL refusal says of the arguments.  The occluded one
// has looked at its own settings, R among them, before anything else; the other two check R after the mesh.
int op_backproject(const char* who, const char* list, dtp_mesh* mesh, const BackprojectCall& b, dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  RC(check_mesh(who, m, b.mask && b.face_idx && b.texture, list));
  RC(check_face_mask(who, m, b.sel, b.mask_words));
  if (!b.occluded && (b.R < 1 || b.R > MAX_WIN)) { dtp_set_error("%s: R=%d (1..%d)", who, b.R, MAX_WIN); return DTP_ERR_ARG; }
  RC(check_texture(who, b.texture, b.H, b.W));
  HIP_CHECK(hipSetDevice(m->ctx->device));
  return enqueue_backproject(m, b, (hipStream_t)s);
}

}  // namespace

bool mesh_alive(const Mesh* m) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_meshes.count(const_cast<Mesh*>(m)) != 0;
}
int check_texture(const char* who, const void* texture, int H, int W) {
  if (H < 1 || W < 1 || H > MAX_TEX || W > MAX_TEX) { dtp_set_error("%s: a %d x %d texture (each side 1..%d)", who, H, W, MAX_TEX); return DTP_ERR_ARG; }
  if (((uintptr_t)texture & 3) != 0) { dtp_set_error("%s: texture must be 4-byte aligned (one RGBA texel per load)", who); return DTP_ERR_ARG; }
  return DTP_OK;
}
int check_bleed(const char* who, int bleed) {
  if (bleed < 0 || bleed > MESH_MAX_BLEED) { dtp_set_error("%s: bleed=%d outside 0..%d", who, bleed, MESH_MAX_BLEED); return DTP_ERR_ARG; }
  return DTP_OK;
}

bool mesh_geom(dtp_mesh* mesh, MeshGeom* out) {
  Mesh* m = (Mesh*)mesh;
  if (!mesh_alive(m)) return false;
  *out = MeshGeom{m->ctx, m->F, m->verts, m->faces, m->uvs, &m->view, m->sel_poly};
  return true;
}

void mesh_drop_ctx(Ctx* c) {
  std::vector<Mesh*> mine;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    for (Mesh* m : g_meshes)
      if (m->ctx == c) mine.push_back(m);
    for (Mesh* m : mine) g_meshes.erase(m);
  }
  for (Mesh* m : mine) mesh_free(m);
}

extern "C" {

int dtp_mesh_camera(const float pos[3], const float normal[3], const float prev[3], float fov, float out[12]) {
  if (!pos || !normal || !prev || !out) { dtp_set_error("dtp_mesh_camera: NULL argument"); return DTP_ERR_ARG; }
  float cam[12];
  RC(make_camera("dtp_mesh_camera", -1, pos, normal, prev, fov, cam));
  memcpy(out, cam, sizeof cam);
  return DTP_OK;
}

int dtp_mesh_create(dtp_ctx* ctx, const float* vertices, int V, const int* faces, int F, const float* face_uvs, dtp_mesh** out) {
  Ctx* c = (Ctx*)ctx;
  // ---- the data, before the first HIP call
  if (!vertices || !faces || !face_uvs || !out) { dtp_set_error("dtp_mesh_create: NULL argument (vertices, faces, face_uvs and out are required)"); return DTP_ERR_ARG; }
  if (V < 1 || F < 1 || F > MAX_FACES) { dtp_set_error("dtp_mesh_create: V=%d vertices, F=%d faces (V >= 1, 1 <= F <= %d)", V, F, MAX_FACES); return DTP_ERR_ARG; }
  for (size_t i = 0; i < (size_t)3 * V; ++i)
    if (!std::isfinite(vertices[i])) { dtp_set_error("dtp_mesh_create: vertex %d is not finite", (int)(i / 3)); return DTP_ERR_ARG; }
  for (int f = 0; f < F; ++f) {
    for (int k = 0; k < 3; ++k)
      if (faces[3 * (size_t)f + k] < 0 || faces[3 * (size_t)f + k] >= V) {
        dtp_set_error("dtp_mesh_create: face %d refers to vertex %d (0..%d)", f, faces[3 * (size_t)f + k], V - 1);
        return DTP_ERR_ARG;
      }
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(face_uvs[6 * (size_t)f + k])) { dtp_set_error("dtp_mesh_create: face %d has a UV that is not finite", f); return DTP_ERR_ARG; }
  }
  if (!c) { dtp_set_error("dtp_mesh_create: ctx is NULL"); return DTP_ERR_ARG; }
  // ---- the copy
  HIP_CHECK(hipSetDevice(c->device));
  Mesh* m = new Mesh();
  m->ctx = c; m->V = V; m->F = F;
  for (int i = 0; i < 3; ++i) { m->lo[i] = 1e300; m->hi[i] = -1e300; }
  for (size_t i = 0; i < (size_t)3 * V; ++i) { m->lo[i % 3] = std::min(m->lo[i % 3], (double)vertices[i]); m->hi[i % 3] = std::max(m->hi[i % 3], (double)vertices[i]); }
  const size_t nf = (size_t)F;
  hipError_t e = hipMalloc((void**)&m->verts, (size_t)V * 12);
  if (e == hipSuccess) e = hipMalloc((void**)&m->faces, nf * 12);
  if (e == hipSuccess) e = hipMalloc((void**)&m->uvs, nf * 24);
  if (e == hipSuccess) e = hipMalloc((void**)&m->rec, nf * sizeof(FaceRec));
  if (e == hipSuccess) e = hipMalloc((void**)&m->owned, nf * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&m->win, nf * sizeof(int4));
  if (e == hipSuccess) e = hipMalloc((void**)&m->val, nf * sizeof(int4));
  if (e == hipSuccess) e = hipMalloc((void**)&m->state, sizeof(MeshState));
  if (e == hipSuccess) e = hipMalloc((void**)&m->sel_poly, (size_t)2 * SELECT_MAX_VERTS * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(m->verts, vertices, (size_t)V * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->faces, faces, nf * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->uvs, face_uvs, nf * 24, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(m->rec, 0, nf * sizeof(FaceRec));
  if (e == hipSuccess) e = hipMemset(m->owned, 0, nf * 4);
  if (e == hipSuccess) e = hipMemset(m->win, 0, nf * sizeof(int4));  // (every entry names a face of the mesh at all times)
  if (e == hipSuccess) e = hipMemset(m->val, 0, nf * sizeof(int4));
  if (e == hipSuccess) e = hipMemset(m->state, 0, sizeof(MeshState));  // (no window rendered yet: a backprojection finds no face)
  if (e != hipSuccess) {
    dtp_set_error("dtp_mesh_create: %s (V=%d, F=%d)", hipGetErrorString(e), V, F);
    mesh_free(m);
    return DTP_ERR_HIP;
  }
  {
    std::lock_guard<std::mutex> lock(g_mu);
    g_meshes.insert(m);
  }
  *out = (dtp_mesh*)m;
  return DTP_OK;
}

int dtp_mesh_destroy(dtp_mesh* mesh) {
  Mesh* m = (Mesh*)mesh;
  if (!m) return DTP_OK;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (!g_meshes.erase(m)) { dtp_set_error("dtp_mesh_destroy: not a live mesh"); return DTP_ERR_ARG; }
  }
  (void)hipSetDevice(m->ctx->device);
  mesh_free(m);  // (hipFree waits for the work that still reads it)
  return DTP_OK;
}

int dtp_mesh_stroke(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                    const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, dtp_stream s) {
  return mesh_stroke(StrokeCall{"dtp_mesh_stroke", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, s});
}

int dtp_mesh_stroke_bleed(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                          const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, dtp_stream s) {
  return mesh_stroke(StrokeCall{"dtp_mesh_stroke_bleed", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, s, bleed});
}

int dtp_mesh_stroke_masked(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                           const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, const uint32_t* face_mask, int mask_words, dtp_stream s) {
  return mesh_stroke(StrokeCall{"dtp_mesh_stroke_masked", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, s, bleed, face_mask, mask_words});
}

int dtp_mesh_stroke_occluded(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                             const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, const uint32_t* face_mask, int mask_words, float occlude,
                             dtp_stream s) {
  return mesh_stroke(StrokeCall{"dtp_mesh_stroke_occluded", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, s, bleed, face_mask, mask_words, true,
                                occlude});
}

int dtp_op_mesh_render(dtp_mesh* mesh, const float cam[12], float fov, int flip_normals, const uint8_t* texture, int H, int W, int R, int mode,
                       int over_y, int over_x, float* canvas, int* face_idx, dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  RC(check_mesh("dtp_op_mesh_render", m, cam && texture && canvas && face_idx));
  if (R < 1 || R > MAX_WIN) { dtp_set_error("dtp_op_mesh_render: R=%d (1..%d)", R, MAX_WIN); return DTP_ERR_ARG; }
  RC(check_texture("dtp_op_mesh_render", texture, H, W));
  if (!known_mode(mode)) { dtp_set_error("dtp_op_mesh_render: unknown mode %d", mode); return DTP_ERR_ARG; }
  RC(check_over("dtp_op_mesh_render", 0, mode, over_y, over_x, R));
  bool finite = fov > 0.f && std::isfinite(fov);
  for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(cam[i]);
  if (!finite) { dtp_set_error("dtp_op_mesh_render: the camera is not finite or fov=%g is not > 0", (double)fov); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(m->ctx->device));
  return enqueue_render(m, cam, fov, flip_normals != 0, texture, H, W, R, mode, over_y, over_x, canvas, face_idx, (hipStream_t)s);
}

int dtp_op_mesh_backproject(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R, uint8_t* texture, int H, int W,
                            dtp_stream s) {
  return op_backproject("dtp_op_mesh_backproject", " (dec alone may be NULL: erase)", mesh,
                        BackprojectCall{dec, dec_finished != 0, mask, face_idx, R, texture, H, W}, s);
}

int dtp_op_mesh_backproject_masked(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R, uint8_t* texture,
                                   int H, int W, const uint32_t* face_mask, int mask_words, dtp_stream s) {
  return op_backproject("dtp_op_mesh_backproject_masked", " (dec alone may be NULL: erase; face_mask: no set)", mesh,
                        BackprojectCall{dec, dec_finished != 0, mask, face_idx, R, texture, H, W, nullptr, 0, face_mask, mask_words}, s);
}

int dtp_op_mesh_backproject_occluded(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R, uint8_t* texture,
                                     int H, int W, const uint32_t* face_mask, int mask_words, float fov, float occlude, dtp_stream s) {
  const char* who = "dtp_op_mesh_backproject_occluded";
  BackprojectCall b{dec, dec_finished != 0, mask, face_idx, R, texture, H, W, nullptr, 0, face_mask, mask_words, true};
  RC(check_occlude(who, occlude));
  if (R < 1 || R > MAX_WIN) { dtp_set_error("%s: R=%d (1..%d)", who, R, MAX_WIN); return DTP_ERR_ARG; }
  if (!(fov > 0.f) || !std::isfinite(fov)) { dtp_set_error("%s: fov=%g (a finite value > 0)", who, (double)fov); return DTP_ERR_ARG; }
  if (!mesh_occlude_tol(occlude, fov, R, &b.tol)) {
    dtp_set_error("%s: the tolerance of occlude=%g at fov=%g does not fit fp32", who, (double)occlude, (double)fov);
    return DTP_ERR_ARG;
  }
  return op_backproject(who, " (dec alone may be NULL: erase; face_mask: no set)", mesh, b, s);
}

}  // extern "C"
