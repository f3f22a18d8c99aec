// Strokes on a textured mesh (dtp_mesh_stroke): what the reference's Kit app does around every stamp when it paints on a
// mesh (kit_app/.../python/manager.py:199-271, util/render.py:22-178: an orthographic look-at camera at the brush, a rasterisation of the
// mesh into the R x R stamp window with the texture sampled through the interpolated UVs, generate_raw, and a second rasterisation of
// the visible faces in UV space that carries the painted stamp back into the texture).  The reference's two rasterisations are kaolin's;
// these are written from the contract of include/dtp.h: coverage in exact integer arithmetic on vertices snapped to 1/256 pixel,
// interpolation in fp32 one rounded operation at a time (contraction is off for this whole file), a winner per pixel that does not depend
// on the order in which faces are visited.  Plain HIP: vector loads, stores and atomics only.
// The bleed pass (dtp_mesh_stroke_bleed, dtp_mesh_bleed) pads the UV charts after a backprojection: the texels no face of
// the mesh covers take the nearest covered texel, by the same integer coverage.
// Picking (dtp_mesh_pick) is the render's visibility rule at one sample per ray: the closest hit of N rays, from the
// vertices, faces and UVs alone, so that it runs on a stream of its own beside a stroke.
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

#include "mesh_dev.h"
#include "mesh_host.h"
#include "select_host.h"
#include "stamp.h"

namespace {

constexpr int SMALL_BOX = 1024;    // coverage build: a face whose texel box holds at most this many centres is rasterised by one wave

enum { MF_RASTER = 1, MF_FRONT = 2, MF_UPRIGHT = 4 };  // finite with a non-zero area; unit normal z >= 0; >= 0.5 (not steep)

// what one stamp's projection leaves per face: window position snapped to 1/256 pixel, camera z, NDC (the backprojection's feature)
struct FaceRec { int X[3], Y[3]; float z[3], nx[3], ny[3]; int flags; };
// per mesh, on the device: the faces that can cover a pixel centre of the window, those that are backprojected, and the texel bounding box
// of the latter (x0, y0, x1, y1); n_big: the faces a coverage build hands to its tile pass
struct MeshState { int n_win, n_val, bb[4], n_big; };
struct MeshCam { float m[12], fov; };  // travels as a kernel argument
constexpr int PICK_CHUNK = 256;        // ray frames staged in LDS per workgroup of the pick
struct PickRay { float m[12], S, d[3]; };  // 64 B: the ray's frame, its grid S = 2^e, its direction
static_assert(sizeof(PickRay) == 64 && sizeof(dtp_mesh_hit) == 52, "the pick's records are copied as bytes");

struct Mesh {
  Ctx* ctx = nullptr;
  int V = 0, F = 0;
  float* verts = nullptr;  // [V][3]
  int* faces = nullptr;    // [F][3]
  float* uvs = nullptr;    // [F][3][2]
  FaceRec* rec = nullptr;  // [F], of the last projection
  int* owned = nullptr;    // [F]: the face won at least one pixel of the last render
  int4* win = nullptr;     // [F] {face, px0 | px1 << 16, py0 | py1 << 16, 0}
  int4* val = nullptr;     // [F] the same in texels
  MeshState* state = nullptr;
  // the texels of a cov_H x cov_W texture that any face covers, 1 bit per texel in rows of (cov_W + 31) / 32 words, followed by the
  // table of bleed offsets (2 * MESH_MAX_OFF bytes); built at the first use of a size, one per mesh
  unsigned int* cov = nullptr;
  int cov_H = 0, cov_W = 0;
  double lo[3], hi[3];     // the vertices' bounding box (host): a window it misses is skipped without a launch
  // picking: allocated at the first pick, in steps of PICK_CHUNK rays; no stroke reads or writes them
  PickRay* pick_rays = nullptr;               // [pick_cap]
  unsigned long long* pick_slots = nullptr;   // [pick_cap]: the winner's (order-preserving bits of z) << 32 | ~face; 0: no hit
  dtp_mesh_hit* pick_out = nullptr;           // [pick_cap]
  char* pick_host = nullptr;                  // pinned: [pick_cap] PickRay, then [pick_cap] dtp_mesh_hit
  int pick_cap = 0;
  int* sel_poly = nullptr;  // [2 * 1024]: the snapped polygon of the lasso in flight (select.hip); no stroke, pick or view touches it
  void* view = nullptr;  // the buffers of dtp_mesh_view (view.hip): allocated at the first view; no stroke or pick touches them
};

std::mutex g_mu;
std::set<Mesh*> g_meshes;  // the live meshes: a destroyed handle is refused, not followed

// ---------------------------------------------------------------- device: the shared arithmetic (snap, orient, top_left, cover, interp, taps, blend, centre_range: mesh_dev.h)
// texture-space position of a face's three UVs, snapped to 1/256 texel
__device__ __forceinline__ void snap_uvs(const float* __restrict__ uv, int H, int W, int X[3], int Y[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    X[k] = snap((uv[2 * k] * (float)W) * 256.0f);
    Y[k] = snap(((1.0f - uv[2 * k + 1]) * (float)H) * 256.0f);
  }
}

// ---------------------------------------------------------------- device: the kernels
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
  if (at < F) win[at] = make_int4(f, x0 | (x1 << 16), y0 | (y1 << 16), 0);  // (always, unless two renders of one mesh race)
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
  for (int base = 0; base < n_win; base += CHUNK) {
    if (t == 0) s_n = 0;
    __syncthreads();
    if (base + t < n_win) {
      const int4 e = win[base + t];
      if (ranges_meet(e.y, col0, col0 + 15) && ranges_meet(e.z, row0, row0 + 15)) {
        const int slot = atomicAdd(&s_n, 1);
        const FaceRec& r = rec[e.x];
        s_face[slot] = e.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_X[slot][k] = r.X[k]; s_Y[slot][k] = r.Y[k]; s_z[slot][k] = r.z[k]; }
      }
    }
    __syncthreads();
    const int n = s_n;
    if (live)
      for (int i = 0; i < n; ++i) {
        float w[3];
        if (!cover(s_X[i], s_Y[i], px, py, w)) continue;
        const float z = interp(w, s_z[i][0], s_z[i][1], s_z[i][2]);
        const int f = s_face[i];
        if (best < 0 || z > best_z || (z == best_z && f < best)) { best = f; best_z = z; bw[0] = w[0]; bw[1] = w[1]; bw[2] = w[2]; }
      }
    __syncthreads();
  }
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
    snap_uvs(uvs + (size_t)6 * f, H, W, X, Y);
    if (orient(X[0], Y[0], X[1], Y[1], X[2], Y[2]) == 0) continue;
    centre_range(min3(X[0], X[1], X[2]), max3(X[0], X[1], X[2]), W, x0, x1);
    centre_range(min3(Y[0], Y[1], Y[2]), max3(Y[0], Y[1], Y[2]), H, y0, y1);
    if (x0 > x1 || y0 > y1) continue;
    const int at = atomicAdd(&st->n_val, 1);
    if (at < F) val[at] = make_int4(f, x0 | (x1 << 16), y0 | (y1 << 16), 0);
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
  for (int base = 0; base < n_val; base += CHUNK) {
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

// ---------------------------------------------------------------- device: coverage and the bleed pass
// a face in texture space: false for a zero area or a texel box without a centre
__device__ __forceinline__ bool face_texels(const float* __restrict__ uv, int H, int W, int X[3], int Y[3], int& x0, int& x1, int& y0, int& y1) {
  snap_uvs(uv, H, W, X, Y);
  if (orient(X[0], Y[0], X[1], Y[1], X[2], Y[2]) == 0) return false;
  centre_range(min3(X[0], X[1], X[2]), max3(X[0], X[1], X[2]), W, x0, x1);
  centre_range(min3(Y[0], Y[1], Y[2]), max3(Y[0], Y[1], Y[2]), H, y0, y1);
  return x0 <= x1 && y0 <= y1;
}

// Coverage build, pass 1: one wave per face, ALL faces of the mesh.  A face whose texel box is small is rasterised here, the lanes
// striding over the box; any other is appended to `big` for the tile pass.  The result is a union of bits: order-free.
__global__ __launch_bounds__(256) void mesh_cover_faces_kernel(const float* __restrict__ uvs, int F, int H, int W, unsigned int* __restrict__ cov,
                                                               int4* __restrict__ big, MeshState* st) {
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= F) return;
  int X[3], Y[3], x0, x1, y0, y1;
  if (!face_texels(uvs + (size_t)6 * f, H, W, X, Y, x0, x1, y0, y1)) return;
  const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);  // (at most 2^30)
  if (n > SMALL_BOX) {
    if (lane == 0) {
      const int at = atomicAdd(&st->n_big, 1);
      if (at < F) big[at] = make_int4(f, x0 | (x1 << 16), y0 | (y1 << 16), 0);
    }
    return;
  }
  const size_t wp = (size_t)((W + 31) >> 5);
  for (int i = lane; i < n; i += 64) {
    const int col = x0 + i % bw, row = y0 + i / bw;
    float w[3];
    if (cover(X, Y, 256 * col + 128, 256 * row + 128, w)) atomicOr(&cov[row * wp + (col >> 5)], 1u << (col & 31));
  }
}

// Coverage build, pass 2: one workgroup per 16 x 16 texel tile, one thread per texel; the big faces stream through LDS CHUNK at a time, as
// in the backprojection.  A wave holds four rows of 16 texels: its ballot gives the 16 bits of each row, which lie in one word.
__global__ __launch_bounds__(256) void mesh_cover_tiles_kernel(const int4* __restrict__ big, const MeshState* st, int F, const float* __restrict__ uvs,
                                                               int H, int W, unsigned int* __restrict__ cov) {
  __shared__ int s_n, s_X[CHUNK][3], s_Y[CHUNK][3];
  const int n_big = min(st->n_big, F);
  if (n_big == 0) return;  // (uniform)
  const int t = threadIdx.x, col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
  const int col = col0 + (t & 15), row = row0 + (t >> 4);
  const bool live = col < W && row < H;
  const int px = 256 * col + 128, py = 256 * row + 128;
  bool in = false;
  for (int base = 0; base < n_big; base += CHUNK) {
    if (t == 0) s_n = 0;
    __syncthreads();
    if (base + t < n_big) {
      const int4 e = big[base + t];
      if (ranges_meet(e.y, col0, col0 + 15) && ranges_meet(e.z, row0, row0 + 15)) {
        const int slot = atomicAdd(&s_n, 1);
        snap_uvs(uvs + (size_t)6 * e.x, H, W, s_X[slot], s_Y[slot]);
      }
    }
    __syncthreads();
    const int n = s_n;
    if (live)
      for (int i = 0; i < n && !in; ++i) {
        float w[3];
        in = cover(s_X[i], s_Y[i], px, py, w);
      }
    __syncthreads();
  }
  const unsigned long long rows = __ballot(in);  // bit l: row (l >> 4) of the wave's four, column l & 15 of the tile
  if ((t & 63) == 0) {
    const size_t wp = (size_t)((W + 31) >> 5);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned int bits = (unsigned int)(rows >> (16 * r)) & 0xffffu;
      if (bits) atomicOr(&cov[(row + r) * wp + (col0 >> 5)], bits << (col0 & 31));  // (a texel outside the texture has no bit)
    }
  }
}

// the coverage as bytes 0 / 1 (dtp_op_mesh_coverage)
__global__ __launch_bounds__(256) void mesh_cover_bytes_kernel(const unsigned int* __restrict__ cov, int H, int W, unsigned char* __restrict__ out) {
  const size_t wp = (size_t)((W + 31) >> 5), n = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t row = i / W;
    const int col = (int)(i - row * W);
    out[i] = (unsigned char)((cov[row * wp + (col >> 5)] >> (col & 31)) & 1u);
  }
}

// The bleed pass: one workgroup per 16 x 16 texels of the whole texture; a tile that misses the rectangle leaves at once.  The rectangle
// is `rect` (x0, y0, x1, y1, clipped by the host), or with `st` the texel bounding box of the stamp backprojected last grown by k and
// clipped here (no valid face: no pass).  The coverage flags of the tile and a k-texel halo are staged in LDS (0 outside the texture:
// no wrap-around), with the first n_off offsets of the table; an uncovered texel takes the four bytes of the first covered candidate.
// Only covered texels are read and only uncovered ones written, so the launch needs no second buffer and no order.
__global__ __launch_bounds__(256) void mesh_bleed_kernel(const unsigned int* __restrict__ cov, const signed char* __restrict__ table, int n_off, int k,
                                                         const MeshState* st, int F, int4 rect, unsigned int* tex, int H, int W) {
  __shared__ unsigned char s_cov[(16 + 2 * MESH_MAX_BLEED) * (16 + 2 * MESH_MAX_BLEED)];
  __shared__ signed char s_off[2 * MESH_MAX_OFF];
  const int t = threadIdx.x, col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
  int x0 = rect.x, y0 = rect.y, x1 = rect.z, y1 = rect.w;
  if (st) {
    if (min(st->n_val, F) == 0) return;
    x0 = max(st->bb[0] - k, 0); y0 = max(st->bb[1] - k, 0); x1 = min(st->bb[2] + k, W - 1); y1 = min(st->bb[3] + k, H - 1);
  }
  if (col0 > x1 || col0 + 15 < x0 || row0 > y1 || row0 + 15 < y0) return;  // (uniform)
  const int n = 16 + 2 * k;
  const size_t wp = (size_t)((W + 31) >> 5);
  for (int i = t; i < n * n; i += 256) {
    const int r = row0 - k + i / n, c = col0 - k + i % n;
    s_cov[i] = (r >= 0 && r < H && c >= 0 && c < W) ? (unsigned char)((cov[r * wp + (c >> 5)] >> (c & 31)) & 1u) : (unsigned char)0;
  }
  for (int i = t; i < 2 * n_off; i += 256) s_off[i] = table[i];
  __syncthreads();
  const int col = col0 + (t & 15), row = row0 + (t >> 4);
  if (col < x0 || col > x1 || row < y0 || row > y1) return;  // (x1 < W, y1 < H)
  const int ly = (t >> 4) + k, lx = (t & 15) + k;
  if (s_cov[ly * n + lx]) return;
  for (int o = 0; o < n_off; ++o) {
    const int di = s_off[2 * o], dj = s_off[2 * o + 1];  // |di|, |dj| <= k: inside the staged square
    if (s_cov[(ly + di) * n + (lx + dj)]) {
      tex[(size_t)row * W + col] = tex[(size_t)(row + di) * W + (col + dj)];
      return;
    }
  }
}

// ---------------------------------------------------------------- device: picking
// A face against a ray: the camera-space vertices as mesh_project_kernel computes them, snapped on the ray's grid, the render's coverage
// at the single centre (0, 0).  true: the ray meets the face not behind its origin; w the weights, z the interpolated camera z (<= 0).
__device__ __forceinline__ bool pick_face(const PickRay& q, const float p[3][3], float w[3], float& z) {
  int X[3], Y[3];
  float cz[3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = ((q.m[0] * p[k][0] + q.m[1] * p[k][1]) + q.m[2] * p[k][2]) + q.m[3];
    const float y = ((q.m[4] * p[k][0] + q.m[5] * p[k][1]) + q.m[6] * p[k][2]) + q.m[7];
    cz[k] = ((q.m[8] * p[k][0] + q.m[9] * p[k][1]) + q.m[10] * p[k][2]) + q.m[11];
    finite = finite && isfinite(x) && isfinite(y) && isfinite(cz[k]);
    X[k] = snap(x * q.S);
    Y[k] = snap(y * q.S);
  }
  // three X or three Y of one strict sign: the centre lies outside the bounding box, no int64 work
  if (!finite || (X[0] > 0 && X[1] > 0 && X[2] > 0) || (X[0] < 0 && X[1] < 0 && X[2] < 0) || (Y[0] > 0 && Y[1] > 0 && Y[2] > 0) ||
      (Y[0] < 0 && Y[1] < 0 && Y[2] < 0))
    return false;
  if (!cover(X, Y, 0, 0, w)) return false;
  z = interp(w, cz[0], cz[1], cz[2]);
  if (z == 0.0f) z = 0.0f;  // (-0 is +0)
  return z <= 0.0f;
}

__device__ __forceinline__ void load_face(const float* __restrict__ verts, const int* __restrict__ faces, int f, float p[3][3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = verts + (size_t)3 * faces[(size_t)3 * f + k];
    p[k][0] = v[0]; p[k][1] = v[1]; p[k][2] = v[2];
  }
}

// One thread per face, which loads its nine vertex floats once, against a chunk of at most PICK_CHUNK rays staged in LDS (every lane
// reads the same frame: a broadcast); grid = (faces / 256, rays / PICK_CHUNK).  The winner of a ray is the largest key = (order-
// preserving bits of z) << 32 | ~face over all faces: the wave reduces its keys first (almost every wave has none for a ray and skips
// that), then one lane issues one 64-bit atomic max.  The slots were zeroed on the stream before the launch; 0 is below every key.
__global__ __launch_bounds__(256) void mesh_pick_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int F,
                                                        const PickRay* __restrict__ rays, int N, unsigned long long* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) PickRay s_ray[PICK_CHUNK];
  const int t = threadIdx.x, f = blockIdx.x * 256 + t, r0 = blockIdx.y * PICK_CHUNK, n = min(PICK_CHUNK, N - r0);
  const float4* src = (const float4*)(rays + r0);
  float4* dst = (float4*)s_ray;
  for (int i = t; i < 4 * n; i += 256) dst[i] = src[i];
  const bool live = f < F;
  float p[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  if (live) load_face(verts, faces, f, p);
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    float w[3], z;
    const bool hit = live && pick_face(s_ray[i], p, w, z);
    if (__ballot(hit) == 0ull) continue;  // (uniform in the wave)
    unsigned int hi = 0u, lo = 0u;
    if (hit) {
      const unsigned int u = __float_as_uint(z);
      hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      lo = ~(unsigned int)f;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned int ohi = __shfl_xor(hi, d, 64), olo = __shfl_xor(lo, d, 64);
      if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; }
    }
    if ((t & 63) == 0) atomicMax(&slots[r0 + i], ((unsigned long long)hi << 32) | lo);
  }
}

// One thread per ray: the record of the slot's winner, its weights recomputed by the same arithmetic; no hit: face -1 and zeros.
__global__ __launch_bounds__(256) void mesh_pick_record_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                               const float* __restrict__ uvs, int F, const PickRay* __restrict__ rays, int N,
                                                               const unsigned long long* __restrict__ slots, dtp_mesh_hit* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  dtp_mesh_hit h;
  memset(&h, 0, sizeof h);
  h.face = -1;
  const unsigned long long key = slots[i];
  const int f = (int)~(unsigned int)key;
  const PickRay q = rays[i];
  float p[3][3], w[3], z;
  if (key != 0ull && f >= 0 && f < F && (load_face(verts, faces, f, p), pick_face(q, p, w, z))) {
    h.face = f;
    const float e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const float e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    float n[3] = {e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);  // correctly rounded (__fsqrt_rn is the native instruction)
    const bool away = (n[0] * q.d[0] + n[1] * q.d[1]) + n[2] * q.d[2] > 0.0f;
    const float* uv = uvs + (size_t)6 * f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      h.w[c] = w[c];
      h.pos[c] = interp(w, p[0][c], p[1][c], p[2][c]);
      n[c] = n[c] / len;
      h.normal[c] = away ? -n[c] : n[c];
    }
    h.uv[0] = interp(w, uv[0], uv[2], uv[4]);
    h.uv[1] = interp(w, uv[1], uv[3], uv[5]);
    h.t = 0.0f - z;
  }
  out[i] = h;
}

// ---------------------------------------------------------------- host
inline int launch_ok() { return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP; }
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

bool mesh_alive(const Mesh* m) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_meshes.count(const_cast<Mesh*>(m)) != 0;
}

void mesh_free(Mesh* m) {
  (void)hipFree(m->verts); (void)hipFree(m->faces); (void)hipFree(m->uvs); (void)hipFree(m->rec); (void)hipFree(m->owned);
  (void)hipFree(m->win); (void)hipFree(m->val); (void)hipFree(m->state); (void)hipFree(m->cov);
  (void)hipFree(m->sel_poly);
  (void)hipFree(m->pick_rays); (void)hipFree(m->pick_slots); (void)hipFree(m->pick_out);
  if (m->pick_host) (void)hipHostFree(m->pick_host);
  view_free(m->view);
  delete m;
}

// ---- picking: every check and the frames of all rays, before any device call
int pick_check(const char* who, const Mesh* m, const dtp_ray* rays, int n, const void* out, std::vector<PickRay>& q) {
  if (!m || !rays || !out) { dtp_set_error("%s: NULL argument (mesh, rays and out are required)", who); return DTP_ERR_ARG; }
  if (n < 1 || n > PICK_MAX_RAYS) { dtp_set_error("%s: n=%d rays (1..%d)", who, n, PICK_MAX_RAYS); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("%s: the mesh is not a live mesh (destroyed?)", who); return DTP_ERR_ARG; }
  q.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const char* why = mesh_ray_frame(rays[i].origin, rays[i].dir, q[i].m);
    if (why) { dtp_set_error("%s: ray %d: %s", who, i, why); return DTP_ERR_ARG; }
    q[i].S = ldexpf(1.0f, mesh_pick_exponent(q[i].m, m->lo, m->hi));
    for (int c = 0; c < 3; ++c) q[i].d[c] = rays[i].dir[c];
  }
  return DTP_OK;
}

// the pick's own buffers, for at least n rays
int pick_reserve(Mesh* m, int n) {
  if (n <= m->pick_cap) return DTP_OK;
  (void)hipFree(m->pick_rays); (void)hipFree(m->pick_slots); (void)hipFree(m->pick_out);  // (waits for the work that still reads them)
  if (m->pick_host) (void)hipHostFree(m->pick_host);
  m->pick_rays = nullptr; m->pick_slots = nullptr; m->pick_out = nullptr; m->pick_host = nullptr; m->pick_cap = 0;
  const size_t cap = (size_t)(n + PICK_CHUNK - 1) / PICK_CHUNK * PICK_CHUNK;
  hipError_t e = hipMalloc((void**)&m->pick_rays, cap * sizeof(PickRay));
  if (e == hipSuccess) e = hipMalloc((void**)&m->pick_slots, cap * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&m->pick_out, cap * sizeof(dtp_mesh_hit));
  if (e == hipSuccess) e = hipHostMalloc((void**)&m->pick_host, cap * (sizeof(PickRay) + sizeof(dtp_mesh_hit)), hipHostMallocDefault);
  if (e != hipSuccess) { dtp_set_error("mesh pick: %s (buffers for %d rays)", hipGetErrorString(e), (int)cap); return DTP_ERR_HIP; }
  m->pick_cap = (int)cap;
  return DTP_OK;
}

// frames in -> slots zeroed -> pick -> records (-> the pinned copy), on s alone; waits for s.  out_dev null: the mesh's own records.
int pick_run(Mesh* m, const std::vector<PickRay>& q, dtp_mesh_hit* out_dev, dtp_mesh_hit* out_host, hipStream_t s) {
  const int n = (int)q.size();
  HIP_CHECK(hipSetDevice(m->ctx->device));
  RC(pick_reserve(m, n));
  dtp_mesh_hit* host_rec = (dtp_mesh_hit*)(m->pick_host + (size_t)m->pick_cap * sizeof(PickRay));
  dtp_mesh_hit* rec = out_dev ? out_dev : m->pick_out;
  memcpy(m->pick_host, q.data(), (size_t)n * sizeof(PickRay));
  HIP_CHECK(hipMemcpyAsync(m->pick_rays, m->pick_host, (size_t)n * sizeof(PickRay), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(m->pick_slots, 0, (size_t)n * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(mesh_pick_kernel, dim3((m->F + 255) / 256, (n + PICK_CHUNK - 1) / PICK_CHUNK), dim3(256), 0, s, m->verts, m->faces, m->F,
                     m->pick_rays, n, m->pick_slots);
  hipLaunchKernelGGL(mesh_pick_record_kernel, dim3((n + 255) / 256), dim3(256), 0, s, m->verts, m->faces, m->uvs, m->F, m->pick_rays, n,
                     m->pick_slots, rec);
  RC(launch_ok());
  if (out_host) HIP_CHECK(hipMemcpyAsync(host_rec, rec, (size_t)n * sizeof(dtp_mesh_hit), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (out_host) memcpy(out_host, host_rec, (size_t)n * sizeof(dtp_mesh_hit));
  return DTP_OK;
}

int check_texture(const char* who, const void* texture, int H, int W) {
  if (H < 1 || W < 1 || H > MAX_TEX || W > MAX_TEX) { dtp_set_error("%s: a %d x %d texture (each side 1..%d)", who, H, W, MAX_TEX); return DTP_ERR_ARG; }
  if (((uintptr_t)texture & 3) != 0) { dtp_set_error("%s: texture must be 4-byte aligned (one RGBA texel per load)", who); return DTP_ERR_ARG; }
  return DTP_OK;
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

// valid (-> journal) -> backproject of the window rendered last on this mesh; dec null: erase.  journal (or null): the one whose open record
// guards this texture; the tiles of the valid faces' texel box grown by `grow` (the bleed that follows) are saved before they are written.
// sel (or null): the face set outside which no face is valid.  tol (or null: the plain kernel): the occlusion test's tolerance.
int enqueue_backproject(Mesh* m, const float* dec, int finished, const unsigned char* mask, const int* face_idx, int R, unsigned char* texture, int H, int W,
                        hipStream_t s, Journal* journal = nullptr, int grow = 0, const unsigned int* sel = nullptr, const float* tol = nullptr) {
  hipLaunchKernelGGL(mesh_valid_kernel, dim3(std::min((m->F + 255) / 256, 1024)), dim3(256), 0, s, m->rec, m->owned, m->win, m->uvs, m->F, H,
                     W, m->val, m->state, sel);
  if (journal) RC(journal_save_box(journal, m->state->bb, grow, s));
  if (tol)
    hipLaunchKernelGGL(mesh_backproject_occluded_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, s, m->rec, m->val, m->state, m->F, m->uvs,
                       dec, finished, mask, face_idx, R, (unsigned int*)texture, H, W, *tol);
  else
    hipLaunchKernelGGL(mesh_backproject_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, s, m->rec, m->val, m->state, m->F, m->uvs, dec,
                       finished, mask, face_idx, R, (unsigned int*)texture, H, W);
  return launch_ok();
}

// the occlusion test's setting (or null: off), before anything else of a call is looked at
int check_occlude(const char* who, const float* occlude) {
  if (occlude && !mesh_occlude_ok(*occlude)) { dtp_set_error("%s: occlude=%g (a finite value >= 0, in stamp pixels)", who, (double)*occlude); return DTP_ERR_ARG; }
  return DTP_OK;
}

int check_bleed(const char* who, int bleed) {
  if (bleed < 0 || bleed > MESH_MAX_BLEED) { dtp_set_error("%s: bleed=%d outside 0..%d", who, bleed, MESH_MAX_BLEED); return DTP_ERR_ARG; }
  return DTP_OK;
}

// The coverage of an H x W texture by all faces of the mesh, built at the first use of the size: one allocation (the bits and the offset
// table behind them) and its kernels; the call waits for them once, so that every later use, on any stream, only reads.  Another size
// frees the mask and builds it again.  `val` holds the big faces meanwhile: the next backprojection rewrites it before it reads it.
int ensure_coverage(Mesh* m, int H, int W, hipStream_t s) {
  if (m->cov && m->cov_H == H && m->cov_W == W) return DTP_OK;
  if (m->cov) { (void)hipFree(m->cov); m->cov = nullptr; }  // (waits for the work that still reads it)
  const size_t bits = (size_t)((W + 31) >> 5) * H * 4;
  unsigned int* cov = nullptr;
  hipError_t e = hipMalloc((void**)&cov, bits + 2 * MESH_MAX_OFF);
  if (e == hipSuccess) e = hipMemsetAsync(cov, 0, bits, s);
  if (e == hipSuccess) e = hipMemsetAsync(&m->state->n_big, 0, sizeof(int), s);
  if (e == hipSuccess) e = hipMemcpyAsync((char*)cov + bits, mesh_bleed_table().d, 2 * MESH_MAX_OFF, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mesh_cover_faces_kernel, dim3((m->F + 3) / 4), dim3(256), 0, s, m->uvs, m->F, H, W, cov, m->val, m->state);
    hipLaunchKernelGGL(mesh_cover_tiles_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, s, m->val, m->state, m->F, m->uvs, H, W, cov);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    dtp_set_error("mesh coverage of a %d x %d texture: %s", H, W, hipGetErrorString(e));
    (void)hipFree(cov);
    return DTP_ERR_HIP;
  }
  m->cov = cov; m->cov_H = H; m->cov_W = W;
  return DTP_OK;
}

// the bleed pass at radius k over `rect` (clipped, not empty), or with rect null over the box of the stamp backprojected last on this mesh
int enqueue_bleed(Mesh* m, unsigned char* texture, int H, int W, int k, const int* rect, hipStream_t s) {
  const signed char* table = (const signed char*)m->cov + (size_t)((W + 31) >> 5) * H * 4;
  const int4 r = rect ? make_int4(rect[0], rect[1], rect[2], rect[3]) : make_int4(0, 0, -1, -1);
  hipLaunchKernelGGL(mesh_bleed_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, s, m->cov, table, mesh_bleed_table().count[k], k,
                     rect ? (const MeshState*)nullptr : m->state, m->F, r, (unsigned int*)texture, H, W);
  return launch_ok();
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

// dtp_mesh_stroke (bleed 0), dtp_mesh_stroke_bleed, dtp_mesh_stroke_masked (face_mask or null) and dtp_mesh_stroke_occluded (occlude or
// null: the plain backprojection): `who` names the entry point in a refusal
int mesh_stroke(const char* who, dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, dtp_stream s_, const uint32_t* face_mask = nullptr,
                int mask_words = 0, const float* occlude = nullptr) {
  Ctx* c = (Ctx*)ctx;
  Mesh* m = (Mesh*)mesh;
  hipStream_t s = (hipStream_t)s_;
  // ---- every check, before anything is enqueued
  RC(check_bleed(who, bleed));
  RC(check_occlude(who, occlude));
  if (!c || !m || !texture || !stamps || !st || !o) {
    dtp_set_error("%s: NULL argument (ctx, mesh, texture, stamps, st and o are required)", who);
    return DTP_ERR_ARG;
  }
  if (!c->finalized) { dtp_set_error("%s: weights not finalized", who); return DTP_ERR_STATE; }
  if (!mesh_alive(m)) { dtp_set_error("%s: the mesh is not a live mesh (destroyed?)", who); return DTP_ERR_ARG; }
  if (m->ctx != c) { dtp_set_error("%s: the mesh belongs to another handle", who); return DTP_ERR_ARG; }
  RC(check_face_mask(who, m, face_mask, mask_words));
  const unsigned int* sel = (const unsigned int*)face_mask;
  const int R = c->R;
  RC(check_texture(who, texture, H, W));
  if (n < 1) { dtp_set_error("%s: n=%d stamps (at least 1)", who, n); return DTP_ERR_ARG; }
  if (R > MAX_WIN) { dtp_set_error("%s: resolution %d above %d", who, R, MAX_WIN); return DTP_ERR_ARG; }
  if (o->margin < 0 || o->margin >= R / 2) { dtp_set_error("%s: margin=%d outside [0, %d)", who, o->margin, R / 2); return DTP_ERR_ARG; }
  std::vector<MeshStep> steps(n);
  int evals = 0;
  bool any_erase = false, any_stamp = false;
  for (int i = 0; i < n; ++i) {
    const dtp_mesh_stamp& t = stamps[i];
    MeshStep& q = steps[i];
    if (!known_mode(t.mode)) {
      dtp_set_error("%s: stamp %d has unknown mode %d (INPAINT = 0, ERASE = 1, OVERPAINT = 2)", who, i, t.mode);
      return DTP_ERR_ARG;
    }
    RC(check_over(who, i, t.mode, o->over_y, o->over_x, R));
    RC(make_camera(who, i, t.pos, t.normal, t.prev, t.fov, q.cam));
    if (occlude && !mesh_occlude_tol(*occlude, t.fov, R, &q.tol)) {
      dtp_set_error("%s: stamp %d: the tolerance of occlude=%g at fov=%g does not fit fp32", who, i, (double)*occlude, (double)t.fov);
      return DTP_ERR_ARG;
    }
    q.skip = !box_meets_window(m, q.cam, t.fov, R);
    if (t.mode == DTP_STROKE_ERASE) { any_erase = any_erase || !q.skip; continue; }  // (runs no stamp: its slot and seed are unused)
    if (t.slot < 0 || t.slot >= DTP_MAX_SLOTS) { dtp_set_error("%s: slot %d of stamp %d outside 0..%d", who, t.slot, i, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
    if (!c->slot_set[t.slot]) {
      dtp_set_error("%s: stamp %d: no brush set in slot %d (call dtp_set_brush / dtp_set_conditioning)", who, i, t.slot);
      return DTP_ERR_STATE;
    }
    // the stamp, as dtp_stamp_seeded would stage it, with the two hooks
    q.st = *st; q.seed = t.seed; q.slot = t.slot;
    StampPlan& p = q.plan;
    p.st = &q.st; p.B = 1; p.slot_ids = &q.slot; p.strength = o->strength;
    p.seeded = true; p.seeds = &q.seed; p.sample_vae = o->sample_vae != 0;
    p.canvas_staged = true;
    p.paste = [](const float*, int, int, hipStream_t) { return DTP_OK; };  // (set for the checks; the launcher proper follows below)
    const int rc = stamp_plan(c, p);
    if (rc) {  // dtp_stamp_seeded's refusal and code, with the stamp it is about
      const std::string why = dtp_last_error();
      dtp_set_error("%s: stamp %d: %s", who, i, why.c_str());
      return rc;
    }
    if (!q.skip) { evals += p.E; any_stamp = true; }
  }
  // ---- enqueue: per stamp reset -> project -> render -> stamp -> valid -> backproject (-> bleed); the stream orders the stamps
  HIP_CHECK(hipSetDevice(c->device));
  if (bleed && (any_stamp || any_erase)) RC(ensure_coverage(m, H, W, s));
  const unsigned char *square = paste_mask, *disc = paste_mask;
  if (!paste_mask && any_stamp) RC(stroke_default_mask(c, o->margin, s, &square));
  if (!paste_mask && any_erase) RC(disc_mask(c, s, &disc));
  int* face_idx = c->mesh_face_idx;
  Journal* journal = journal_armed(c, texture, H, W);
  for (int i = 0; i < n; ++i) {
    const dtp_mesh_stamp& t = stamps[i];
    MeshStep& q = steps[i];
    if (q.skip) continue;
    const bool occluded = occlude != nullptr;
    const float tol = q.tol;  // (by value: the paste hook below keeps its own copy)
    RC(enqueue_render(m, q.cam, t.fov, o->flip_normals != 0, texture, H, W, R, t.mode, o->over_y, o->over_x, c->canvas32, face_idx, s));
    if (t.mode == DTP_STROKE_ERASE) {
      RC(enqueue_backproject(m, nullptr, 0, disc, face_idx, R, texture, H, W, s, journal, bleed, sel, occluded ? &tol : nullptr));
      if (bleed) RC(enqueue_bleed(m, texture, H, W, bleed, nullptr, s));
      continue;
    }
    q.plan.paste = [=](const float* dec, int, int, hipStream_t q_s) {
      RC(enqueue_backproject(m, dec, 0, square, face_idx, R, texture, H, W, q_s, journal, bleed, sel, occluded ? &tol : nullptr));
      return bleed ? enqueue_bleed(m, texture, H, W, bleed, nullptr, q_s) : DTP_OK;
    };
    RC(stamp_enqueue(c, q.plan, s));
  }
  c->last_stroke_stamps = n; c->last_stroke_groups = n; c->last_stroke_evals = evals;
  return DTP_OK;
}

}  // namespace

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
  return mesh_stroke("dtp_mesh_stroke", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, 0, s);
}

int dtp_mesh_stroke_bleed(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                          const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, dtp_stream s) {
  return mesh_stroke("dtp_mesh_stroke_bleed", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, bleed, s);
}

int dtp_mesh_stroke_masked(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                           const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, const uint32_t* face_mask, int mask_words, dtp_stream s) {
  return mesh_stroke("dtp_mesh_stroke_masked", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, bleed, s, face_mask, mask_words);
}

int dtp_mesh_stroke_occluded(dtp_ctx* ctx, dtp_mesh* mesh, uint8_t* texture, int H, int W, const dtp_mesh_stamp* stamps, int n, const dtp_settings* st,
                             const dtp_mesh_stroke_opts* o, const uint8_t* paste_mask, int bleed, const uint32_t* face_mask, int mask_words, float occlude,
                             dtp_stream s) {
  return mesh_stroke("dtp_mesh_stroke_occluded", ctx, mesh, texture, H, W, stamps, n, st, o, paste_mask, bleed, s, face_mask, mask_words, &occlude);
}

int dtp_mesh_bleed_offsets(int radius, int* count, signed char* di_dj) {
  if (!count) { dtp_set_error("dtp_mesh_bleed_offsets: count is NULL"); return DTP_ERR_ARG; }
  if (radius < 1 || radius > MESH_MAX_BLEED) { dtp_set_error("dtp_mesh_bleed_offsets: radius=%d outside 1..%d", radius, MESH_MAX_BLEED); return DTP_ERR_ARG; }
  const MeshBleedTable& t = mesh_bleed_table();
  *count = t.count[radius];
  if (di_dj) memcpy(di_dj, t.d, (size_t)2 * t.count[radius]);
  return DTP_OK;
}

int dtp_mesh_bleed(dtp_mesh* mesh, uint8_t* texture, int H, int W, int bleed, const int* rect, dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  if (!m || !texture) { dtp_set_error("dtp_mesh_bleed: NULL argument (mesh and texture are required)"); return DTP_ERR_ARG; }
  RC(check_bleed("dtp_mesh_bleed", bleed));
  RC(check_texture("dtp_mesh_bleed", texture, H, W));
  int r[4];
  const int clipped = mesh_clip_rect(rect, H, W, r);
  if (clipped < 0) { dtp_set_error("dtp_mesh_bleed: rect (%d, %d, %d, %d) has x0 > x1 or y0 > y1", rect[0], rect[1], rect[2], rect[3]); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("dtp_mesh_bleed: the mesh is not a live mesh (destroyed?)"); return DTP_ERR_ARG; }
  if (bleed == 0 || clipped > 0) return DTP_OK;  // nothing to do
  HIP_CHECK(hipSetDevice(m->ctx->device));
  RC(ensure_coverage(m, H, W, (hipStream_t)s));
  return enqueue_bleed(m, texture, H, W, bleed, r, (hipStream_t)s);
}

int dtp_mesh_ray_frame(const float origin[3], const float dir[3], float out[12]) {
  if (!origin || !dir || !out) { dtp_set_error("dtp_mesh_ray_frame: NULL argument"); return DTP_ERR_ARG; }
  const char* why = mesh_ray_frame(origin, dir, out);
  if (why) { dtp_set_error("dtp_mesh_ray_frame: %s", why); return DTP_ERR_ARG; }
  return DTP_OK;
}

int dtp_mesh_pick(dtp_mesh* mesh, const dtp_ray* rays, int n, dtp_mesh_hit* out_host, dtp_stream s) {
  std::vector<PickRay> q;
  RC(pick_check("dtp_mesh_pick", (Mesh*)mesh, rays, n, out_host, q));
  return pick_run((Mesh*)mesh, q, nullptr, out_host, (hipStream_t)s);
}

int dtp_op_mesh_pick(dtp_mesh* mesh, const dtp_ray* rays, int n, dtp_mesh_hit* out, dtp_stream s) {
  std::vector<PickRay> q;
  RC(pick_check("dtp_op_mesh_pick", (Mesh*)mesh, rays, n, out, q));
  return pick_run((Mesh*)mesh, q, out, nullptr, (hipStream_t)s);
}

int dtp_mesh_path_plan(const dtp_mesh_hit* hits, int n, float stamp_distance, dtp_path_state* state, float* pos, float* normal, float* prev,
                       int cap, int* count) {
  if (!state || !count || (n > 0 && !hits) || (cap > 0 && (!pos || !normal || !prev))) {
    dtp_set_error("dtp_mesh_path_plan: NULL argument (state and count are required; hits with n > 0; pos, normal and prev with cap > 0)");
    return DTP_ERR_ARG;
  }
  if (n < 0 || cap < 0) { dtp_set_error("dtp_mesh_path_plan: n=%d, cap=%d (both >= 0)", n, cap); return DTP_ERR_ARG; }
  if (!(stamp_distance > 0.f) || !std::isfinite(stamp_distance)) {
    dtp_set_error("dtp_mesh_path_plan: stamp_distance=%g (a finite value > 0)", (double)stamp_distance);
    return DTP_ERR_ARG;
  }
  for (int i = 0; i < n; ++i)
    if (hits[i].face >= 0 && !(std::isfinite(hits[i].pos[0]) && std::isfinite(hits[i].pos[1]) && std::isfinite(hits[i].pos[2]))) {
      dtp_set_error("dtp_mesh_path_plan: hit %d has a non-finite position", i);
      return DTP_ERR_ARG;
    }
  const long long need = mesh_path_plan(hits, n, stamp_distance, state, pos, normal, prev, cap);
  if (need < 0) { dtp_set_error("dtp_mesh_path_plan: a chord of more than %d stamps", PATH_MAX_CHORD); return DTP_ERR_ARG; }
  if (need > 0x7fffffffLL) { dtp_set_error("dtp_mesh_path_plan: more than 2^31 - 1 stamps"); return DTP_ERR_ARG; }
  *count = (int)need;
  if (need > cap) { dtp_set_error("dtp_mesh_path_plan: %d stamps planned, capacity %d", (int)need, cap); return DTP_ERR_ARG; }
  return DTP_OK;
}

int dtp_op_mesh_coverage(dtp_mesh* mesh, int H, int W, uint8_t* out, dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  if (!m || !out) { dtp_set_error("dtp_op_mesh_coverage: NULL argument"); return DTP_ERR_ARG; }
  if (H < 1 || W < 1 || H > MAX_TEX || W > MAX_TEX) { dtp_set_error("dtp_op_mesh_coverage: a %d x %d texture (each side 1..%d)", H, W, MAX_TEX); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("dtp_op_mesh_coverage: the mesh is not a live mesh (destroyed?)"); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(m->ctx->device));
  RC(ensure_coverage(m, H, W, (hipStream_t)s));
  const size_t n = (size_t)H * W;
  hipLaunchKernelGGL(mesh_cover_bytes_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)s, m->cov, H, W, out);
  return launch_ok();
}

int dtp_op_mesh_render(dtp_mesh* mesh, const float cam[12], float fov, int flip_normals, const uint8_t* texture, int H, int W, int R, int mode,
                       int over_y, int over_x, float* canvas, int* face_idx, dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  if (!m || !cam || !texture || !canvas || !face_idx) { dtp_set_error("dtp_op_mesh_render: NULL argument"); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("dtp_op_mesh_render: the mesh is not a live mesh (destroyed?)"); return DTP_ERR_ARG; }
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
  Mesh* m = (Mesh*)mesh;
  if (!m || !mask || !face_idx || !texture) { dtp_set_error("dtp_op_mesh_backproject: NULL argument (dec alone may be NULL: erase)"); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("dtp_op_mesh_backproject: the mesh is not a live mesh (destroyed?)"); return DTP_ERR_ARG; }
  if (R < 1 || R > MAX_WIN) { dtp_set_error("dtp_op_mesh_backproject: R=%d (1..%d)", R, MAX_WIN); return DTP_ERR_ARG; }
  RC(check_texture("dtp_op_mesh_backproject", texture, H, W));
  HIP_CHECK(hipSetDevice(m->ctx->device));
  return enqueue_backproject(m, dec, dec_finished != 0, mask, face_idx, R, texture, H, W, (hipStream_t)s);
}

int dtp_op_mesh_backproject_masked(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R, uint8_t* texture,
                                   int H, int W, const uint32_t* face_mask, int mask_words, dtp_stream s) {
  const char* who = "dtp_op_mesh_backproject_masked";
  Mesh* m = (Mesh*)mesh;
  if (!m || !mask || !face_idx || !texture) { dtp_set_error("%s: NULL argument (dec alone may be NULL: erase; face_mask: no set)", who); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("%s: the mesh is not a live mesh (destroyed?)", who); return DTP_ERR_ARG; }
  RC(check_face_mask(who, m, face_mask, mask_words));
  if (R < 1 || R > MAX_WIN) { dtp_set_error("%s: R=%d (1..%d)", who, R, MAX_WIN); return DTP_ERR_ARG; }
  RC(check_texture(who, texture, H, W));
  HIP_CHECK(hipSetDevice(m->ctx->device));
  return enqueue_backproject(m, dec, dec_finished != 0, mask, face_idx, R, texture, H, W, (hipStream_t)s, nullptr, 0, (const unsigned int*)face_mask);
}

int dtp_op_mesh_backproject_occluded(dtp_mesh* mesh, const float* dec, int dec_finished, const uint8_t* mask, const int* face_idx, int R, uint8_t* texture,
                                     int H, int W, const uint32_t* face_mask, int mask_words, float fov, float occlude, dtp_stream s) {
  const char* who = "dtp_op_mesh_backproject_occluded";
  Mesh* m = (Mesh*)mesh;
  RC(check_occlude(who, &occlude));
  if (R < 1 || R > MAX_WIN) { dtp_set_error("%s: R=%d (1..%d)", who, R, MAX_WIN); return DTP_ERR_ARG; }
  if (!(fov > 0.f) || !std::isfinite(fov)) { dtp_set_error("%s: fov=%g (a finite value > 0)", who, (double)fov); return DTP_ERR_ARG; }
  float tol;
  if (!mesh_occlude_tol(occlude, fov, R, &tol)) {
    dtp_set_error("%s: the tolerance of occlude=%g at fov=%g does not fit fp32", who, (double)occlude, (double)fov);
    return DTP_ERR_ARG;
  }
  if (!m || !mask || !face_idx || !texture) { dtp_set_error("%s: NULL argument (dec alone may be NULL: erase; face_mask: no set)", who); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("%s: the mesh is not a live mesh (destroyed?)", who); return DTP_ERR_ARG; }
  RC(check_face_mask(who, m, face_mask, mask_words));
  RC(check_texture(who, texture, H, W));
  HIP_CHECK(hipSetDevice(m->ctx->device));
  return enqueue_backproject(m, dec, dec_finished != 0, mask, face_idx, R, texture, H, W, (hipStream_t)s, nullptr, 0, (const unsigned int*)face_mask, &tol);
}

}  // extern "C"
