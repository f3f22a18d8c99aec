// A view of a textured mesh (dtp_mesh_view): the whole mesh through a perspective camera into an H x W RGBA frame on the
// device, so that a client without Omniverse sees what it painted (in the reference the viewport is Omniverse RTX reading the texture
// through update_material_texture, kit_app/.../python/manager.py:349-354).  Written from the contract of include/dtp.h: the projection in
// fp32 one rounded operation at a time, the strokes' integer coverage (mesh_dev.h), the inverse depth interpolated on the screen, a winner
// per pixel that does not depend on the order in which faces are visited.  The stamp's own render streams its whole window list through
// every tile, which suits the 8 600 faces of a stamp window; a frame of 10^5..10^6 faces is binned instead: faces are counted into bins of
// 64 x 64 pixels, the counts are scanned, the faces written into their bins' segments, and a tile of 16 x 16 pixels streams its bin's
// segment alone -- plus the short list of faces too large to bin.  No capacity to choose, no overflow, no read-back.  The kernels read
// the mesh's vertices, faces and UVs and write buffers of their own: nothing a stroke or a pick in flight uses.  Plain HIP: vector loads,
// stores and atomics only.  dtp_mesh_view_mips is the same frame with a trilinear sample from the texture's mip pyramid
// (mips.hip): the raster kernel is a template on the filter.  dtp_mesh_view_clip also draws the faces that CROSS the
// near plane, in homogeneous form: per face the cross products of its camera-space vertices, per pixel their edge functions against the
// pixel's ray (cross_q), which give the same q_k and d the rest of the raster kernel consumes.  It is a second template parameter.
// dtp_mesh_view_aa draws the same frames with s x s samples per pixel: project, scan and fill run for the frame of
// s H x s W, and a raster kernel of its own (view_raster_aa_kernel) keeps a winner per sample in registers and sums the samples' bytes
// in LDS: the larger frame is never stored.  dtp_mesh_view_aniso is a third value of the filter parameter of both
// raster kernels: the two footprint vectors are kept apart, the level comes from the shorter one, and up to 16 trilinear taps along the
// longer one are averaged in a rolled loop.  Both raster kernels shade their winner through view_shade, and a face across the near
// plane is weighted through cross_q everywhere but in the plain kernel's face loop, which keeps its own text for a measured reason.
#pragma clang fp contract(off)
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "engine.h"
#include "mesh_dev.h"
#include "mips_host.h"
#include "view_host.h"

namespace {

enum { VF_SMALL = 1, VF_LARGE = 2 };  // drawn, and binned / on the list every tile streams; 0: not drawn
enum { VF_CROSS = 4 };                // with VF_LARGE: a face across the near plane, whose record holds the homogeneous form
constexpr int CROSS_SLOT = 1 << 30;   // a staged slot of such a face: this bit of s_face (a face index is below 2^20)

// what a view's projection leaves per face, 64 bytes: screen position snapped to 1/256 pixel, 1 / depth per vertex, the unit normal's z,
// the pixel ranges x0 | x1 << 16, y0 | y1 << 16.  A face across the near plane (VF_CROSS): X, Y, iw hold the bits of sign(D) n_0,
// sign(D) n_1, sign(D) n_2 (three floats each) and pad[0] those of 1 / |D|
struct ViewRec { int X[3], Y[3]; float iw[3], nzu; int flags, px, py, pad[3]; };
static_assert(sizeof(ViewRec) == 64, "one record per 64-byte line");
// the counters of a frame: count and n_large are zeroed on the stream before every projection
struct ViewState { int count[VIEW_MAX_BINS], n_large, offset[VIEW_MAX_BINS + 1], cursor[VIEW_MAX_BINS]; };
struct ViewBufs {
  ViewRec* rec = nullptr;     // [F]
  int* items = nullptr;       // [4 F]: the bins' segments of face indices (a small face has at most 4 entries)
  int* large = nullptr;       // [F]
  ViewState* st = nullptr;
};
struct ViewShade { int shade; float ambient, unpainted[3]; unsigned int background; };  // travels as a kernel argument
// what the raster kernel needs of the filter it is instantiated for; travels as a kernel argument.  0: one bilinear sample of level 0
// (dtp_mesh_view); 1: trilinear between two levels of the pyramid (dtp_mesh_view_mips): levels 1 .. levels - 1 as dtp_texture_mips lays
// them out, and the map of lod (or null)
template <int FILTER> struct ViewFilter {};
template <> struct ViewFilter<1> { const unsigned int* mips; float* lod; int levels; };
// 2: up to max_aniso trilinear taps along the longer axis of the footprint, the level from the shorter one (dtp_mesh_view_aniso, DESIGN.md
// 3.29); the map of the number of taps (or null)
template <> struct ViewFilter<2> { const unsigned int* mips; float* lod; int levels, max_aniso; unsigned char* taps; };
// and of the near-plane clip: what the ray of a pixel and the clip itself need of the camera
template <int CLIP> struct ViewClip {};
template <> struct ViewClip<1> { float fx, fy, near; };
// the ray of the centre of pixel column j (row i) of a W (H) pixel frame, without its z = -1: ndc / f
__device__ __forceinline__ float ray_x(int j, int W, float fx) { return ((float)(2 * j + 1) / (float)W - 1.0f) / fx; }
__device__ __forceinline__ float ray_y(int i, int H, float fy) { return (1.0f - (float)(2 * i + 1) / (float)H) / fy; }

// counter[key] += 1 for every lane of the wave whose key is >= 0, with ONE atomic per distinct key: the lanes that share a key elect a
// leader, which adds their number; -> the lane's slot, the counter's value before its own add.  Neighbouring faces of a mesh mostly share
// a bin, and a frame seen from afar has few bins: one atomic per face on the same few words serialises the whole launch.  Every lane that
// has not left the kernel calls it, from converged code.
__device__ __forceinline__ int wave_add(int* counter, int key) {
  const int lane = threadIdx.x & 63;
  int slot = 0;
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k) & todo;
    int base = 0;
    if (lane == leader) base = atomicAdd(&counter[k], __popcll(same));
    base = __shfl(base, leader, 64);
    if ((same >> lane) & 1ull) slot = base + __popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  return slot;
}
// entry e = 0 .. 3 of a small face: the bin (by0 + e / 2, bx0 + e % 2) if the face meets it, else -1
__device__ __forceinline__ int bin_key(int e, int bx0, int bx1, int by0, int by1, int nbx) {
  const int bx = bx0 + (e & 1), by = by0 + (e >> 1);
  return (bx <= bx1 && by <= by1) ? by * nbx + bx : -1;
}

// the z of the unit normal of the camera-space triangle c, correctly rounded (a zero area: 0 / 0)
__device__ __forceinline__ float unit_normal_z(const float c[3][3]) {
  const float e1x = c[1][0] - c[0][0], e1y = c[1][1] - c[0][1], e1z = c[1][2] - c[0][2];
  const float e2x = c[2][0] - c[0][0], e2y = c[2][1] - c[0][1], e2z = c[2][2] - c[0][2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  return nz / sqrtf((nx * nx + ny * ny) + nz * nz);
}

// One thread per face: camera space, the unit normal's z, the perspective division, the snapped screen position; a face that is drawn
// (in front of the near plane, not culled, with an area and a pixel centre in its box) is counted into its bins or appended to `large`.
// clip: a face with vertices on both sides of the near plane is drawn too: its record is the homogeneous form, its pixel range the box
// of view_clip_box (the whole frame when not binned), and it goes on `large`.  clip 0 writes what the kernel always wrote.
__global__ __launch_bounds__(256) void view_project_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int F, dtp_view_cam cam,
                                                           int H, int W, int cull, int flip, int binned, int nbx, ViewRec* __restrict__ rec,
                                                           int* __restrict__ large, ViewState* st, int clip) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  float c[3][3];
  bool draw = f < F, finite = f < F;
  int ahead = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = verts + (size_t)3 * (draw ? faces[(size_t)3 * f + k] : 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      c[k][r] = ((cam.m[4 * r] * v[0] + cam.m[4 * r + 1] * v[1]) + cam.m[4 * r + 2] * v[2]) + cam.m[4 * r + 3];
      finite = finite && isfinite(c[k][r]);
    }
    ahead += c[k][2] <= -cam.near ? 1 : 0;
  }
  draw = finite && ahead == 3;
  const bool cross = clip && finite && ahead > 0 && ahead < 3;
  ViewRec r;
  memset(&r, 0, sizeof r);
  if (cross) {
    float n[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* a = c[(k + 1) % 3];
      const float* b = c[(k + 2) % 3];
      n[k][0] = a[1] * b[2] - a[2] * b[1]; n[k][1] = a[2] * b[0] - a[0] * b[2]; n[k][2] = a[0] * b[1] - a[1] * b[0];
    }
    const float D = (c[0][0] * n[0][0] + c[0][1] * n[0][1]) + c[0][2] * n[0][2];
    const bool front = (D < 0.f) != (flip != 0);
    int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
    if (isfinite(D) && D != 0.f && (front || !cull) && (view_clip_box(c, cam.fx, cam.fy, cam.near, H, W, x0, x1, y0, y1) || !binned)) {
      if (!binned) { x0 = 0; x1 = W - 1; y0 = 0; y1 = H - 1; }
      r.nzu = unit_normal_z(c);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        r.X[k] = __float_as_int(D < 0.f ? -n[0][k] : n[0][k]);
        r.Y[k] = __float_as_int(D < 0.f ? -n[1][k] : n[1][k]);
        r.iw[k] = D < 0.f ? -n[2][k] : n[2][k];
      }
      r.pad[0] = __float_as_int(1.0f / fabsf(D));
      r.px = x0 | (x1 << 16); r.py = y0 | (y1 << 16);
      r.flags = VF_LARGE | VF_CROSS;
    }
  }
  if (draw) {
    r.nzu = unit_normal_z(c);
    const float wx = 128.0f * (float)W, wy = 128.0f * (float)H;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r.iw[k] = 1.0f / (0.0f - c[k][2]);
      r.X[k] = snap((((c[k][0] * cam.fx) * r.iw[k]) + 1.0f) * wx);
      r.Y[k] = snap((1.0f - ((c[k][1] * cam.fy) * r.iw[k])) * wy);
    }
    const long long A = orient(r.X[0], r.Y[0], r.X[1], r.Y[1], r.X[2], r.Y[2]);
    const bool front = (A < 0) != (flip != 0);
    int x0, x1, y0, y1;
    centre_range(min3(r.X[0], r.X[1], r.X[2]), max3(r.X[0], r.X[1], r.X[2]), W, x0, x1);
    centre_range(min3(r.Y[0], r.Y[1], r.Y[2]), max3(r.Y[0], r.Y[1], r.Y[2]), H, y0, y1);
    draw = A != 0 && (front || !cull) && x0 <= x1 && y0 <= y1;
    if (draw) { r.px = x0 | (x1 << 16); r.py = y0 | (y1 << 16); }
  }
  int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
  if (draw) r.flags = (view_bins(r.px, r.py, bx0, bx1, by0, by1) && binned) ? VF_SMALL : VF_LARGE;
  if (f < F) rec[f] = r;
#pragma unroll
  for (int e = 0; e < 4; ++e) wave_add(st->count, r.flags == VF_SMALL ? bin_key(e, bx0, bx1, by0, by1, nbx) : -1);
  const int at = wave_add(&st->n_large, (r.flags & VF_LARGE) ? 0 : -1);
  if ((r.flags & VF_LARGE) && at < F) large[at] = f;  // (always, unless two views of one mesh race)
}

// One workgroup: the exclusive prefix of the bins' counts -> where each bin's segment starts, and its cursor for the fill.
__global__ __launch_bounds__(256) void view_scan_kernel(ViewState* st) {
  constexpr int PER = VIEW_MAX_BINS / 256;
  __shared__ int s_sum[256];
  const int t = threadIdx.x;
  int local[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { local[i] = st->count[PER * t + i]; sum += local[i]; }
  s_sum[t] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int v = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  int run = s_sum[t] - sum;
#pragma unroll
  for (int i = 0; i < PER; ++i) { st->offset[PER * t + i] = run; st->cursor[PER * t + i] = run; run += local[i]; }
  if (t == 255) st->offset[VIEW_MAX_BINS] = run;
}

// One thread per face: a small face writes its index into the segment of every bin it was counted in (in any order).
__global__ __launch_bounds__(256) void view_fill_kernel(const ViewRec* __restrict__ rec, int F, int nbx, int* __restrict__ items, ViewState* st) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const bool small = f < F && rec[f].flags == VF_SMALL;
  if (__ballot(small) == 0ull) return;  // (uniform in the wave)
  int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
  if (small) view_bins(rec[f].px, rec[f].py, bx0, bx1, by0, by1);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int key = small ? bin_key(e, bx0, bx1, by0, by1, nbx) : -1;
    const int slot = wave_add(st->cursor, key);
    if (key >= 0 && slot < 4 * F) items[slot] = f;  // (always, unless two views of one mesh race)
  }
}

// A face across the near plane (VF_CROSS) against the ray (gx, gy).  Its ten words -- X, Y: the float bits of n_0, n_1; iw: n_2; inv: the
// bits of 1 / |D| -- come from a record or from a staged slot as they are, and this is the one place that unpacks them.
// -> E_k = (n_k,x gx + n_k,y gy) - n_k,z; qk = E_k / |D|
__device__ __forceinline__ float cross_edge(const int X[3], const int Y[3], const float iw[3], int inv, int k, float gx, float gy, float& qk) {
  const float nx = k == 0 ? __int_as_float(X[0]) : k == 1 ? __int_as_float(Y[0]) : iw[0];
  const float ny = k == 0 ? __int_as_float(X[1]) : k == 1 ? __int_as_float(Y[1]) : iw[1];
  const float nz = k == 0 ? __int_as_float(X[2]) : k == 1 ? __int_as_float(Y[2]) : iw[2];
  const float E = (nx * gx + ny * gy) - nz;
  qk = E * __int_as_float(inv);
  return E;
}
// the three q_k; -> the ray passes inside all three edges (E_k >= 0)
__device__ __forceinline__ bool cross_q(const int X[3], const int Y[3], const float iw[3], int inv, float gx, float gy, float q[3]) {
  const float E0 = cross_edge(X, Y, iw, inv, 0, gx, gy, q[0]), E1 = cross_edge(X, Y, iw, inv, 1, gx, gy, q[1]), E2 = cross_edge(X, Y, iw, inv, 2, gx, gy, q[2]);
  return E0 >= 0.f && E1 >= 0.f && E2 >= 0.f;
}
// d = (q_0 + q_1) + q_2 of such a face lies on this side of its plane's horizon and not nearer than the near plane: the clip itself
__device__ __forceinline__ bool cross_ahead(float d, float near) { return isfinite(d) && d > 0.f && 1.0f / d >= near; }

// The texel of a covered centre: `best` won pixel (row, col) of an H x W frame, centre (px, py), ray (gx, gy) (CLIP alone), with q_k = bq
// and their sum best_d.  The perspective-correct UV, the sample (FILTER 1: the footprint from the face at the two neighbouring centres,
// the level walk, two levels blended; lod is written.  FILTER 2: the two footprint vectors kept apart, the level from the shorter one,
// ntap trilinear taps along the longer one in a rolled loop, their plain mean; lod and ntap are written), the shade, the bytes with
// alpha 255.  Both raster kernels shade through it: a pixel of the plain frame and a sample of the anti-aliased one are the same code.
template <int FILTER, int CLIP>
__device__ __forceinline__ unsigned int view_shade(const ViewRec* __restrict__ rec, const float* __restrict__ uvs, const unsigned int* __restrict__ tex,
                                                   int TH, int TW, int H, int W, ViewShade sh, ViewFilter<FILTER> fl,
                                                   ViewClip<CLIP> cl, int best, const float bq[3], float best_d, int col, int row, int px,
                                                   int py, float gx, float gy, float& lod, int& ntap) {
  const float* uv = uvs + (size_t)6 * best;
  const float u = interp(bq, uv[0], uv[2], uv[4]) / best_d, v = interp(bq, uv[1], uv[3], uv[5]) / best_d;
  float tc[4];
  if constexpr (FILTER == 0) {
    sample_bilinear(tex, TH, TW, u, v, tc);
  } else {
    const ViewRec& r = rec[best];
    float qx[3], qy[3];
    bool crossing = false;
    if constexpr (CLIP != 0) crossing = (r.flags & VF_CROSS) != 0;
    if (crossing) {
      if constexpr (CLIP != 0) {  // the same q_k at the two neighbouring centres, no inside test
        const float gx1 = ray_x(col + 1, W, cl.fx), gy1 = ray_y(row + 1, H, cl.fy);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          cross_edge(r.X, r.Y, r.iw, r.pad[0], k, gx1, gy, qx[k]);
          cross_edge(r.X, r.Y, r.iw, r.pad[0], k, gx, gy1, qy[k]);
        }
      }
    } else {
      float wx[3], wy[3];
      weights_at(r.X, r.Y, px + 256, py, wx);
      weights_at(r.X, r.Y, px, py + 256, wy);
#pragma unroll
      for (int k = 0; k < 3; ++k) { qx[k] = wx[k] * r.iw[k]; qy[k] = wy[k] * r.iw[k]; }
    }
    const float dx = (qx[0] + qx[1]) + qx[2], dy = (qy[0] + qy[1]) + qy[2];
    float rho2 = INFINITY;  // beyond the horizon, or a footprint that is not finite: the last level
    [[maybe_unused]] float du = 0.f, dv = 0.f;  // FILTER 2: the longer axis of the footprint in UV, along which the taps lie
    [[maybe_unused]] int n_taps = 1;
    if (isfinite(dx) && dx > 0.f && isfinite(dy) && dy > 0.f) {
      const float fw = (float)TW, fh = (float)TH;
      if constexpr (FILTER == 1) {
        const float ax = (interp(qx, uv[0], uv[2], uv[4]) / dx - u) * fw, ay = (interp(qx, uv[1], uv[3], uv[5]) / dx - v) * fh;
        const float bx = (interp(qy, uv[0], uv[2], uv[4]) / dy - u) * fw, by = (interp(qy, uv[1], uv[3], uv[5]) / dy - v) * fh;
        rho2 = fmaxf(ax * ax + ay * ay, bx * bx + by * by);
        if (!isfinite(rho2)) rho2 = INFINITY;
      } else {
        const float dua = interp(qx, uv[0], uv[2], uv[4]) / dx - u, dva = interp(qx, uv[1], uv[3], uv[5]) / dx - v;
        const float dub = interp(qy, uv[0], uv[2], uv[4]) / dy - u, dvb = interp(qy, uv[1], uv[3], uv[5]) / dy - v;
        const float ax = dua * fw, ay = dva * fh, bx = dub * fw, by = dvb * fh;
        const float la2 = ax * ax + ay * ay, lb2 = bx * bx + by * by;
        if (isfinite(la2) && isfinite(lb2)) {
          const float pmax2 = fmaxf(la2, lb2), pmin2 = fminf(la2, lb2), m = (float)(fl.max_aniso * fl.max_aniso);
          du = la2 >= lb2 ? dua : dub; dv = la2 >= lb2 ? dva : dvb;
          rho2 = fminf(pmax2, fmaxf(fmaxf(pmin2, 1.0f), pmax2 / m));  // the shorter axis; no finer than a texel, nor than max_aniso taps span
          while (n_taps < fl.max_aniso && !(pmax2 <= (float)(n_taps * n_taps) * rho2)) ++n_taps;
        }
      }
    }
    // level l of hl x wl texels at `at` of the pyramid (l >= 1), level l + 1 at `next`; p4 = 4^l
    int l = 0, hl = TH, wl = TW;
    size_t at = 0, next = 0;
    float p4 = 1.0f;
    while (l + 1 < fl.levels && p4 * 4.0f <= rho2) {
      at = next; hl = mip_half(hl); wl = mip_half(wl); next = at + (size_t)hl * wl;
      p4 *= 4.0f; ++l;
    }
    const float f = (l + 1 == fl.levels || rho2 <= p4) ? 0.f : ((rho2 / p4) - 1.0f) / 3.0f;
    lod = (float)l + f;
    if constexpr (FILTER == 1) {
      sample_bilinear(l == 0 ? tex : fl.mips + at, hl, wl, u, v, tc);
      if (f > 0.f) {
        float tn[4];
        sample_bilinear(fl.mips + next, mip_half(hl), mip_half(wl), u, v, tn);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) tc[ch] = tc[ch] + (tn[ch] - tc[ch]) * f;
      }
    } else {  // n_taps trilinear samples of this l and f, spread along (du, dv) about (u, v); their plain average
      const unsigned int* here = l == 0 ? tex : fl.mips + at;
      const float twice = (float)(2 * n_taps);
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int i = 0; i < n_taps; ++i) {
        const float o = (float)(2 * i + 1) / twice - 0.5f;
        const float ui = u + du * o, vi = v + dv * o;
        sample_bilinear(here, hl, wl, ui, vi, tc);
        if (f > 0.f) {
          float tn[4];
          sample_bilinear(fl.mips + next, mip_half(hl), mip_half(wl), ui, vi, tn);
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) tc[ch] = tc[ch] + (tn[ch] - tc[ch]) * f;
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) sum[ch] = sum[ch] + tc[ch];
      }
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) tc[ch] = sum[ch] / (float)n_taps;
      ntap = n_taps;
    }
  }
  const float s = sh.shade ? sh.ambient + (1.0f - sh.ambient) * fabsf(rec[best].nzu) : 1.0f;
  const float rest = 1.0f - tc[3];
  unsigned int out = 0xff000000u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float cc = (tc[ch] * tc[3] + sh.unpainted[ch] * rest) * s;
    out |= (unsigned int)(unsigned char)(fminf(cc, 1.0f) * 255.0f + 0.5f) << (8 * ch);
  }
  return out;
}

// One workgroup per 16 x 16 pixel tile, one thread per pixel.  The tile's bin segment, then the large list, stream through LDS CHUNK at a
// time; a face whose pixel range misses the tile is dropped on the way in.  Winner: the largest (inverse depth d, -face index) among
// the faces that cover the centre.  Then the perspective-correct UV, the sample, the shade and the stores.  FILTER 1: the winner face
// alone is evaluated again at the two neighbouring centres, the footprint of the pixel in the texture picks a level of the pyramid by
// compares against powers of four (walking the layout on the way), and the sample is blended from that level and the next.  CLIP 1: a
// staged slot may hold a face across the near plane (CROSS_SLOT in s_face): its nine record words travel through s_X, s_Y, s_iw as they
// are, 1 / |D| beside them, and the pixel tests the edge functions of its ray instead of cover(); the winner update is the same.
template <int FILTER, int CLIP>
__global__ __launch_bounds__(256) void view_raster_kernel(const ViewRec* __restrict__ rec, const int* __restrict__ items, const int* __restrict__ large,
                                                          const ViewState* st, int F, int nbx, const float* __restrict__ uvs,
                                                          const unsigned int* __restrict__ tex, int TH, int TW, int H, int W, ViewShade sh,
                                                          unsigned int* __restrict__ image, int* __restrict__ face_idx, float* __restrict__ depth,
                                                          ViewFilter<FILTER> fl, ViewClip<CLIP> cl) {
  __shared__ int s_n, s_face[CHUNK], s_X[CHUNK][3], s_Y[CHUNK][3];
  __shared__ float s_iw[CHUNK][3];
  __shared__ int s_inv[CLIP ? CHUNK : 1];  // (CLIP 0 never names it: no LDS)
  const int t = threadIdx.x, col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
  const int col = col0 + (t & 15), row = row0 + (t >> 4);
  const bool live = col < W && row < H;
  const int px = 256 * col + 128, py = 256 * row + 128;
  const int bin = (row0 >> VIEW_BIN_SHIFT) * nbx + (col0 >> VIEW_BIN_SHIFT);
  const int cap = 4 * F;
  const int seg0 = min(max(st->offset[bin], 0), cap), n_seg = min(max(st->offset[bin + 1], seg0), cap) - seg0;
  const int total = n_seg + min(max(st->n_large, 0), F);
  int best = -1;
  float best_d = 0.f, bq[3] = {0.f, 0.f, 0.f};
  float gx = 0.f, gy = 0.f;
  if constexpr (CLIP != 0) { gx = ray_x(col, W, cl.fx); gy = ray_y(row, H, cl.fy); }
  for (int base = 0; base < total; base += CHUNK) {
    if (t == 0) s_n = 0;
    __syncthreads();
    if (base + t < total) {
      const int i = base + t, f = i < n_seg ? items[seg0 + i] : large[i - n_seg];
      if ((unsigned int)f < (unsigned int)F) {
        const ViewRec& r = rec[f];
        if (ranges_meet(r.px, col0, col0 + 15) && ranges_meet(r.py, row0, row0 + 15)) {
          const int slot = atomicAdd(&s_n, 1);
          if constexpr (CLIP != 0) {
            s_face[slot] = (r.flags & VF_CROSS) ? f | CROSS_SLOT : f;
            s_inv[slot] = r.pad[0];
          } else {
            s_face[slot] = f;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) { s_X[slot][k] = r.X[k]; s_Y[slot][k] = r.Y[k]; s_iw[slot][k] = r.iw[k]; }
        }
      }
    }
    __syncthreads();
    const int n = s_n;
    if (live)
      for (int i = 0; i < n; ++i) {
        if constexpr (CLIP == 0) {
          float w[3];
          if (!cover(s_X[i], s_Y[i], px, py, w)) continue;
          const float q0 = w[0] * s_iw[i][0], q1 = w[1] * s_iw[i][1], q2 = w[2] * s_iw[i][2];
          const float d = (q0 + q1) + q2;
          const int f = s_face[i];
          if (best < 0 || d > best_d || (d == best_d && f < best)) { best = f; best_d = d; bq[0] = q0; bq[1] = q1; bq[2] = q2; }
        } else {
          // Own text, not cross_q / cross_ahead: through them height_field_225_far_trilinear_clip_on_samples_1 took 1.2010 ms against the
          // parent's 1.1563 ms (spread 0.0445 ms; profiles/view_refactor_ab.json): three more moves in every round of this loop.
          float q0, q1, q2, d;
          int f = s_face[i];
          if (f & CROSS_SLOT) {
            f ^= CROSS_SLOT;
            const float E0 = (__int_as_float(s_X[i][0]) * gx + __int_as_float(s_X[i][1]) * gy) - __int_as_float(s_X[i][2]);
            const float E1 = (__int_as_float(s_Y[i][0]) * gx + __int_as_float(s_Y[i][1]) * gy) - __int_as_float(s_Y[i][2]);
            const float E2 = (s_iw[i][0] * gx + s_iw[i][1] * gy) - s_iw[i][2];
            if (!(E0 >= 0.f && E1 >= 0.f && E2 >= 0.f)) continue;
            const float inv = __int_as_float(s_inv[i]);
            q0 = E0 * inv; q1 = E1 * inv; q2 = E2 * inv;
            d = (q0 + q1) + q2;
            if (!(isfinite(d) && d > 0.f && 1.0f / d >= cl.near)) continue;  // the plane's horizon, and the clip itself
          } else {
            float w[3];
            if (!cover(s_X[i], s_Y[i], px, py, w)) continue;
            q0 = w[0] * s_iw[i][0]; q1 = w[1] * s_iw[i][1]; q2 = w[2] * s_iw[i][2];
            d = (q0 + q1) + q2;
          }
          if (best < 0 || d > best_d || (d == best_d && f < best)) { best = f; best_d = d; bq[0] = q0; bq[1] = q1; bq[2] = q2; }
        }
      }
    __syncthreads();
  }
  if (!live) return;
  const size_t pix = (size_t)row * W + col;
  unsigned int out = sh.background;
  float dist = 0.f, lod = 0.f;
  [[maybe_unused]] int ntap = 0;
  if (best >= 0) {
    out = view_shade<FILTER, CLIP>(rec, uvs, tex, TH, TW, H, W, sh, fl, cl, best, bq, best_d, col, row, px, py, gx, gy, lod, ntap);
    dist = 1.0f / best_d;
  }
  image[pix] = out;
  if (face_idx) face_idx[pix] = best;
  if (depth) depth[pix] = dist;
  if constexpr (FILTER != 0) {
    if (fl.lod) fl.lod[pix] = lod;
  }
  if constexpr (FILTER == 2) {
    if (fl.taps) fl.taps[pix] = (unsigned char)ntap;
  }
}

// The anti-aliased frame (dtp_mesh_view_aa): the raster kernel above for the FINE frame of S H x S W pixels that project,
// scan and fill have binned, resolved on the chip.  One workgroup per 16 x 16 OUTPUT pixels = 16 S x 16 S fine ones, which lie in one
// bin (view_aa_tile_bin).  The fine tile is S x S SUB-TILES of 16 x 16 fine pixels.  A round stages a chunk of the bin's segment (then
// of the large list) ONCE for all of them -- the plain kernel at S x the size stages it once per 16 x 16 tile -- and while staging, a
// face is entered into the list of every sub-tile its pixel range meets.  S > 1 runs 1024 threads, four groups of 256, and stages 1024
// (S = 2) or 512 (S = 4) faces a round; group g draws the sub-tiles g, g + 4, ... in turns (one turn at S = 2, four at S = 4), thread
// (ty, tx) of the group owning fine pixel (ty, tx) of each of them and keeping that sample's winner (d, face) in registers.  In a turn
// the group walks that sub-tile's list with cover() (or the rays of a crossing face): the plain kernel's loop on the faces the plain
// kernel's tile would have staged, so the lanes of a wave look at neighbouring samples of the same few faces, and a frame that covers
// few tiles keeps some of the plain kernel's parallelism.  (A first version gave each thread the S x S samples of ONE output pixel and
// stepped the edge functions between them: with faces of a fine pixel or two, nearly every face was then evaluated at all S^2 samples
// for the sake of one or two lanes, and the frame took 3 to 18 times as long as the plain kernel at S x the size; 3.28 has the
// figures.)  After the last round each sample is weighted again at its centre (the same operations: the same q_k, d), shaded by
// view_shade as a pixel of the fine frame, and its bytes, the background's where no face is, are added to the sums of its output
// pixel in LDS (integer adds: the order does not matter); the sample (S / 2, S / 2) of a pixel stores face_idx, depth and lod.  Last,
// thread (ty, tx) of the first group stores the rounded average and the count of output pixel (ty, tx).  The turns are rolled loops
// (copies of the body would crowd the instruction cache): a turn's winner is picked out of the registers and put back by compares with
// the turn, never by an index.  S = 1 is the kernel above with a count.
constexpr int view_aa_threads(int S) { return S == 1 ? 256 : 1024; }
constexpr int view_aa_chunk(int S) { return S == 1 ? CHUNK : S == 2 ? 1024 : 512; }  // faces staged per round (56 and 42 KB of LDS)
template <int FILTER, int CLIP, int S>
__global__ __launch_bounds__(view_aa_threads(S)) void view_raster_aa_kernel(const ViewRec* __restrict__ rec, const int* __restrict__ items,
                                                             const int* __restrict__ large, const ViewState* st, int F, int nbx, const float* __restrict__ uvs,
                                                             const unsigned int* __restrict__ tex, int TH, int TW, int H, int W, ViewShade sh,
                                                             unsigned int* __restrict__ image, int* __restrict__ face_idx, float* __restrict__ depth,
                                                             unsigned char* __restrict__ coverage, ViewFilter<FILTER> fl, ViewClip<CLIP> cl) {
  constexpr int N = S * S, LOG2N = S == 1 ? 0 : S == 2 ? 2 : 4;
  constexpr int GROUPS = view_aa_threads(S) / 256, P = N / GROUPS;  // 256 threads a group; group g takes the sub-tiles g, g + GROUPS, ...: P turns
  constexpr int CH = view_aa_chunk(S);
  __shared__ int s_n, s_cnt[N], s_face[CH], s_X[CH][3], s_Y[CH][3];
  __shared__ float s_iw[CH][3];
  __shared__ int s_inv[CLIP ? CH : 1];
  __shared__ unsigned short s_list[N][CH];    // per sub-tile: the staged slots whose pixel range meets it
  __shared__ unsigned int s_sum[256][2];      // per output pixel: the sums of R | G << 16 and of B | A << 16 (at most 16 x 255 each)
  __shared__ int s_cov[256];                  // and the number of samples that a face covers
  const int t = threadIdx.x & 255, tx = t & 15, ty = t >> 4, col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
  const int group = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);  // (the same in every lane of a wave)
  const bool first = group == 0;                                            // the group that stores the pixels
  const int FH = S * H, FW = S * W;              // the fine frame
  const int fcol0 = S * col0, frow0 = S * row0;  // the tile's first fine pixel
  const int bin = view_aa_tile_bin(S, row0, col0, nbx);
  const int cap = 4 * F;
  const int seg0 = min(max(st->offset[bin], 0), cap), n_seg = min(max(st->offset[bin + 1], seg0), cap) - seg0;
  const int total = n_seg + min(max(st->n_large, 0), F);
  int best[P];
  float best_d[P];
#pragma unroll
  for (int p = 0; p < P; ++p) { best[p] = -1; best_d[p] = 0.f; }
  if (first) { s_sum[t][0] = 0u; s_sum[t][1] = 0u; s_cov[t] = 0; }
  for (int base = 0; base < total; base += CH) {
    if (first && t == 0) s_n = 0;
    if (first && t < N) s_cnt[t] = 0;
    __syncthreads();
    if ((int)threadIdx.x < CH && base + (int)threadIdx.x < total) {
      const int i = base + (int)threadIdx.x, f = i < n_seg ? items[seg0 + i] : large[i - n_seg];
      if ((unsigned int)f < (unsigned int)F) {
        const ViewRec& r = rec[f];
        if (ranges_meet(r.px, fcol0, fcol0 + 16 * S - 1) && ranges_meet(r.py, frow0, frow0 + 16 * S - 1)) {
          const int slot = atomicAdd(&s_n, 1);  // (below CH: at most one per staging thread)
          if constexpr (CLIP != 0) {
            s_face[slot] = (r.flags & VF_CROSS) ? f | CROSS_SLOT : f;
            s_inv[slot] = r.pad[0];
          } else {
            s_face[slot] = f;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) { s_X[slot][k] = r.X[k]; s_Y[slot][k] = r.Y[k]; s_iw[slot][k] = r.iw[k]; }
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const int x = fcol0 + 16 * (k % S), y = frow0 + 16 * (k / S);
            if (ranges_meet(r.px, x, x + 15) && ranges_meet(r.py, y, y + 15)) s_list[k][atomicAdd(&s_cnt[k], 1)] = (unsigned short)slot;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
      const int k = group + GROUPS * p, n = s_cnt[k];
      const int col = fcol0 + 16 * (k % S) + tx, row = frow0 + 16 * (k / S) + ty;  // this thread's sample of sub-tile k
      if (n == 0 || !(col < FW && row < FH)) continue;
      const int px = 256 * col + 128, py = 256 * row + 128;
      float gx = 0.f, gy = 0.f;
      if constexpr (CLIP != 0) { gx = ray_x(col, FW, cl.fx); gy = ray_y(row, FH, cl.fy); }
      int cur = -1;
      float cur_d = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) { cur = j == p ? best[j] : cur; cur_d = j == p ? best_d[j] : cur_d; }
      for (int at = 0; at < n; ++at) {
        const int i = s_list[k][at];
        int f = s_face[i];
        float d;
        bool crossing = false;
        if constexpr (CLIP != 0) { crossing = (f & CROSS_SLOT) != 0; f &= ~CROSS_SLOT; }
        if (crossing) {
          if constexpr (CLIP != 0) {
            float q[3];
            if (!cross_q(s_X[i], s_Y[i], s_iw[i], s_inv[i], gx, gy, q)) continue;
            d = (q[0] + q[1]) + q[2];
            if (!cross_ahead(d, cl.near)) continue;
          }
        } else {
          float w[3];
          if (!cover(s_X[i], s_Y[i], px, py, w)) continue;
          d = (w[0] * s_iw[i][0] + w[1] * s_iw[i][1]) + w[2] * s_iw[i][2];
        }
        if (cur < 0 || d > cur_d || (d == cur_d && f < cur)) { cur = f; cur_d = d; }
      }
#pragma unroll
      for (int j = 0; j < P; ++j) { best[j] = j == p ? cur : best[j]; best_d[j] = j == p ? cur_d : best_d[j]; }
    }
    __syncthreads();
  }
  __syncthreads();  // (the sums were zeroed above; without a chunk nothing has waited yet)
#pragma unroll 1
  for (int p = 0; p < P; ++p) {
    const int k = group + GROUPS * p;
    const int sy = 16 * (k / S) + ty, sx = 16 * (k % S) + tx;  // the sample's place in the fine tile
    const int col = fcol0 + sx, row = frow0 + sy;
    if (!(col < FW && row < FH)) continue;
    int f = -1;
#pragma unroll
    for (int j = 0; j < P; ++j) f = j == p ? best[j] : f;
    unsigned int out = sh.background;
    float dist = 0.f, lod = 0.f;
    int ntap = 0;
    if (f >= 0) {
      const ViewRec& r = rec[f];
      const int px = 256 * col + 128, py = 256 * row + 128;
      float q[3] = {0.f, 0.f, 0.f}, gx = 0.f, gy = 0.f;
      bool crossing = false;
      if constexpr (CLIP != 0) {
        crossing = (r.flags & VF_CROSS) != 0;
        gx = ray_x(col, FW, cl.fx); gy = ray_y(row, FH, cl.fy);
      }
      if (crossing) {
        if constexpr (CLIP != 0) cross_q(r.X, r.Y, r.iw, r.pad[0], gx, gy, q);
      } else {
        float w[3] = {0.f, 0.f, 0.f};
        weights_at(r.X, r.Y, px, py, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = w[c] * r.iw[c];
      }
      const float d = (q[0] + q[1]) + q[2];
      out = view_shade<FILTER, CLIP>(rec, uvs, tex, TH, TW, FH, FW, sh, fl, cl, f, q, d, col, row, px, py, gx, gy, lod, ntap);
      dist = 1.0f / d;
    }
    const int at = (sy / S) * 16 + sx / S;  // the output pixel of the tile that this sample belongs to
    atomicAdd(&s_sum[at][0], (out & 0xffu) | ((out & 0xff00u) << 8));
    atomicAdd(&s_sum[at][1], ((out >> 16) & 0xffu) | ((out >> 24) << 16));
    if (f >= 0) atomicAdd(&s_cov[at], 1);
    if (sy % S == S / 2 && sx % S == S / 2) {  // (inside the frame, as its sample is)
      const size_t pix = (size_t)(row0 + sy / S) * W + (col0 + sx / S);
      if (face_idx) face_idx[pix] = f;
      if (depth) depth[pix] = dist;
      if constexpr (FILTER != 0) {
        if (fl.lod) fl.lod[pix] = lod;
      }
      if constexpr (FILTER == 2) {
        if (fl.taps) fl.taps[pix] = (unsigned char)ntap;
      }
    }
  }
  __syncthreads();
  if (!(first && col0 + tx < W && row0 + ty < H)) return;
  const size_t pix = (size_t)(row0 + ty) * W + (col0 + tx);
  const unsigned int rg = s_sum[t][0], ba = s_sum[t][1];
  image[pix] = (((rg & 0xffffu) + N / 2) >> LOG2N) | ((((rg >> 16) + N / 2) >> LOG2N) << 8) | ((((ba & 0xffffu) + N / 2) >> LOG2N) << 16) |
               ((((ba >> 16) + N / 2) >> LOG2N) << 24);
  if (coverage) coverage[pix] = (unsigned char)s_cov[t];
}

int view_reserve(const MeshGeom& g) {
  if (*g.view) return DTP_OK;
  ViewBufs* b = new ViewBufs();
  const size_t nf = (size_t)g.F;
  hipError_t e = hipMalloc((void**)&b->rec, nf * sizeof(ViewRec));
  if (e == hipSuccess) e = hipMalloc((void**)&b->items, nf * 4 * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&b->large, nf * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&b->st, sizeof(ViewState));
  if (e != hipSuccess) {
    dtp_set_error("mesh view: %s (buffers for %d faces)", hipGetErrorString(e), g.F);
    view_free(b);
    return DTP_ERR_HIP;
  }
  *g.view = b;
  return DTP_OK;
}

// One view, as its entry point fills it in: the arguments every entry point has, then what only some have, with the values of a
// dtp_mesh_view.  filter: 0 = one bilinear sample of level 0; 1 = trilinear from `mips`, with the map of lod (or null); 2 = up to max_aniso
// trilinear taps along the footprint, with the maps of lod and of taps (or null); clip: the faces across the near plane are drawn too;
// samples: 0 = the plain raster kernel, else the anti-aliased one with that many samples a side, and the map of coverage (or null)
struct ViewCall {
  const char* who; dtp_mesh* mesh; const uint8_t* texture; int TH, TW; const dtp_view_cam* cam; int H, W; const dtp_view_opts* o;
  uint8_t* image; int* face_idx; float* depth; int binned; dtp_stream s;
  int filter = 0; const uint8_t* mips = nullptr; float* lod = nullptr;
  int clip = 0, samples = 0; uint8_t* coverage = nullptr;
  int max_aniso = 1; uint8_t* taps = nullptr;
};

// what the _clip, _aa and _aniso entry points refuse of their own arguments before view_run sees them, in this order; `what`: which of them
// the entry point has
enum { OWN_FILTER = 1, OWN_CLIP = 2, OWN_SAMPLES = 4, OWN_ANISO = 8 };
int view_refuse(const ViewCall& c, int what) {
  const char* who = c.who;
  if ((what & OWN_ANISO) && (c.max_aniso < 1 || c.max_aniso > VIEW_MAX_ANISO)) {
    dtp_set_error("%s: max_aniso must lie in 1..%d", who, VIEW_MAX_ANISO);
    return DTP_ERR_ARG;
  }
  if ((what & OWN_FILTER) && c.filter != 0 && c.filter != 1) { dtp_set_error("%s: filter is 0 (bilinear) or 1 (trilinear)", who); return DTP_ERR_ARG; }
  if ((what & OWN_CLIP) && c.clip != 0 && c.clip != 1) { dtp_set_error("%s: clip is 0 or 1", who); return DTP_ERR_ARG; }
  if ((what & OWN_FILTER) && !c.filter && (c.mips || c.lod)) { dtp_set_error("%s: mips and lod need filter 1", who); return DTP_ERR_ARG; }
  if ((what & OWN_SAMPLES) && c.samples != 1 && c.samples != 2 && c.samples != 4) {
    dtp_set_error("%s: %s", who, view_aa_check(c.samples, 1, 1));
    return DTP_ERR_ARG;
  }
  return DTP_OK;
}

// every check, then zero the counters -> project -> scan -> fill -> raster on the stream; nothing waits
int view_run(const ViewCall& c) {
  const char* who = c.who;
  const int TH = c.TH, TW = c.TW, H = c.H, W = c.W;
  const hipStream_t s = (hipStream_t)c.s;
  if (!c.mesh) { dtp_set_error("%s: NULL argument (mesh, texture, cam, opts and image are required)", who); return DTP_ERR_ARG; }
  if (const char* why = view_check(c.texture, TH, TW, c.cam, H, W, c.o, c.image, c.face_idx, c.depth)) { dtp_set_error("%s: %s", who, why); return DTP_ERR_ARG; }
  if (c.samples)
    if (const char* why = view_aa_check(c.samples, H, W)) { dtp_set_error("%s: %s", who, why); return DTP_ERR_ARG; }
  dtp_mip_levels lay;
  if (c.filter) {
    (void)mip_layout(TH, TW, &lay);  // (the sides were checked above)
    if (lay.levels > 1 && !c.mips) { dtp_set_error("%s: NULL argument (mips is required for a texture larger than 1 x 1)", who); return DTP_ERR_ARG; }
    if (((uintptr_t)c.mips & 3) != 0 || ((uintptr_t)c.lod & 3) != 0) { dtp_set_error("%s: mips and lod must be 4-byte aligned", who); return DTP_ERR_ARG; }
  }
  MeshGeom g;
  if (!mesh_geom(c.mesh, &g)) { dtp_set_error("%s: the mesh is not a live mesh (destroyed?)", who); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(g.ctx->device));
  RC(view_reserve(g));
  const ViewBufs* b = (const ViewBufs*)*g.view;
  const dtp_view_opts* o = c.o;
  ViewShade sh;
  sh.shade = o->shade; sh.ambient = o->ambient;
  for (int ch = 0; ch < 3; ++ch) sh.unpainted[ch] = (float)o->unpainted[ch] / 255.0f;
  sh.background = (unsigned int)o->background[0] | ((unsigned int)o->background[1] << 8) | ((unsigned int)o->background[2] << 16) |
                  ((unsigned int)o->background[3] << 24);
  const int fine = c.samples ? c.samples : 1;  // project, scan and fill see the frame the samples are the pixels of
  const int nbx = view_bins_across(fine * W), blocks = (g.F + 255) / 256;
  HIP_CHECK(hipMemsetAsync(b->st, 0, offsetof(ViewState, offset), s));
  hipLaunchKernelGGL(view_project_kernel, dim3(blocks), dim3(256), 0, s, g.verts, g.faces, g.F, *c.cam, fine * H, fine * W, o->cull, o->flip_normals,
                     c.binned ? 1 : 0, nbx, b->rec, b->large, b->st, c.clip ? 1 : 0);
  hipLaunchKernelGGL(view_scan_kernel, dim3(1), dim3(256), 0, s, b->st);
  hipLaunchKernelGGL(view_fill_kernel, dim3(blocks), dim3(256), 0, s, b->rec, g.F, nbx, b->items, b->st);
  const dim3 tiles((W + 15) / 16, (H + 15) / 16);
  ViewFilter<1> fl;
  fl.mips = (const unsigned int*)c.mips; fl.lod = c.lod; fl.levels = c.filter ? lay.levels : 1;
  ViewFilter<2> fa;
  fa.mips = fl.mips; fa.lod = c.lod; fa.levels = fl.levels; fa.max_aniso = c.max_aniso; fa.taps = c.taps;
  ViewClip<1> cl;
  cl.fx = c.cam->fx; cl.fy = c.cam->fy; cl.near = c.cam->near;
#define RASTER(FILTER, CLIP, fl, cl)                                                                                                   \
  hipLaunchKernelGGL((view_raster_kernel<FILTER, CLIP>), tiles, dim3(256), 0, s, b->rec, b->items, b->large, b->st, g.F, nbx, g.uvs, \
                     (const unsigned int*)c.texture, TH, TW, H, W, sh, (unsigned int*)c.image, c.face_idx, c.depth, fl, cl)
#define RASTER_AA(FILTER, CLIP, S, fl, cl)                                                                                                    \
  hipLaunchKernelGGL((view_raster_aa_kernel<FILTER, CLIP, S>), tiles, dim3(view_aa_threads(S)), 0, s, b->rec, b->items, b->large, b->st, g.F, nbx, g.uvs, \
                     (const unsigned int*)c.texture, TH, TW, H, W, sh, (unsigned int*)c.image, c.face_idx, c.depth, c.coverage, fl, cl)
#define RASTER_S(FILTER, CLIP, fl, cl)                 \
  do {                                                 \
    if (c.samples == 0) RASTER(FILTER, CLIP, fl, cl);  \
    else if (c.samples == 1) RASTER_AA(FILTER, CLIP, 1, fl, cl); \
    else if (c.samples == 2) RASTER_AA(FILTER, CLIP, 2, fl, cl); \
    else RASTER_AA(FILTER, CLIP, 4, fl, cl);           \
  } while (0)
  if (c.filter == 2 && c.clip) RASTER_S(2, 1, fa, cl);
  else if (c.filter == 2) RASTER_S(2, 0, fa, ViewClip<0>());
  else if (c.filter && c.clip) RASTER_S(1, 1, fl, cl);
  else if (c.filter) RASTER_S(1, 0, fl, ViewClip<0>());
  else if (c.clip) RASTER_S(0, 1, ViewFilter<0>(), cl);
  else RASTER_S(0, 0, ViewFilter<0>(), ViewClip<0>());
#undef RASTER_S
#undef RASTER_AA
#undef RASTER
  if (hipGetLastError() != hipSuccess) { dtp_set_error("%s: a kernel launch failed", who); return DTP_ERR_HIP; }
  return DTP_OK;
}

}  // namespace

void view_free(void* view) {
  ViewBufs* b = (ViewBufs*)view;
  if (!b) return;
  (void)hipFree(b->rec); (void)hipFree(b->items); (void)hipFree(b->large); (void)hipFree(b->st);  // (waits for the work that still reads them)
  delete b;
}

extern "C" {

int dtp_view_camera(const float eye[3], const float at[3], const float up[3], float fov_y_degrees, int H, int W, float near, dtp_view_cam* out) {
  if (!eye || !at || !up || !out) { dtp_set_error("dtp_view_camera: NULL argument"); return DTP_ERR_ARG; }
  if (const char* why = view_camera(eye, at, up, fov_y_degrees, H, W, near, out)) { dtp_set_error("dtp_view_camera: %s", why); return DTP_ERR_ARG; }
  return DTP_OK;
}

int dtp_view_rays(const dtp_view_cam* cam, int H, int W, const float* pixels_xy, int n, dtp_ray* out) {
  if (!cam || !pixels_xy || !out) { dtp_set_error("dtp_view_rays: NULL argument"); return DTP_ERR_ARG; }
  int bad = -1;
  if (const char* why = view_rays(cam, H, W, pixels_xy, n, out, &bad)) {
    if (bad >= 0) dtp_set_error("dtp_view_rays: pixel %d: %s", bad, why);
    else dtp_set_error("dtp_view_rays: %s", why);
    return DTP_ERR_ARG;
  }
  return DTP_OK;
}

int dtp_mesh_view(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const dtp_view_cam* cam, int H, int W, const dtp_view_opts* opts,
                  uint8_t* image, int* face_idx, float* depth, dtp_stream s) {
  return view_run(ViewCall{"dtp_mesh_view", mesh, texture, TH, TW, cam, H, W, opts, image, face_idx, depth, 1, s});
}

int dtp_mesh_view_mips(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                       const dtp_view_opts* opts, uint8_t* image, int* face_idx, float* depth, float* lod, dtp_stream s) {
  return view_run(ViewCall{"dtp_mesh_view_mips", mesh, texture, TH, TW, cam, H, W, opts, image, face_idx, depth, 1, s, 1, mips, lod});
}

int dtp_op_mesh_view(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const dtp_view_cam* cam, int H, int W, const dtp_view_opts* opts,
                     uint8_t* image, int* face_idx, float* depth, int binned, dtp_stream s) {
  return view_run(ViewCall{"dtp_op_mesh_view", mesh, texture, TH, TW, cam, H, W, opts, image, face_idx, depth, binned, s});
}

int dtp_mesh_view_clip(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                       const dtp_view_opts* opts, int filter, uint8_t* image, int* face_idx, float* depth, float* lod, dtp_stream s) {
  return dtp_op_mesh_view_clip(mesh, texture, TH, TW, mips, cam, H, W, opts, filter, image, face_idx, depth, lod, 1, s);
}

int dtp_op_mesh_view_clip(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                          const dtp_view_opts* opts, int filter, uint8_t* image, int* face_idx, float* depth, float* lod, int binned, dtp_stream s) {
  const ViewCall c{binned == 1 ? "dtp_mesh_view_clip" : "dtp_op_mesh_view_clip", mesh, texture, TH, TW, cam, H, W, opts, image, face_idx, depth, binned, s,
                   filter, mips, lod, 1};
  RC(view_refuse(c, OWN_FILTER));
  return view_run(c);
}

int dtp_mesh_view_aa(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                     const dtp_view_opts* opts, int filter, int clip, int samples, uint8_t* image, int* face_idx, float* depth, float* lod,
                     uint8_t* coverage, dtp_stream s) {
  return dtp_op_mesh_view_aa(mesh, texture, TH, TW, mips, cam, H, W, opts, filter, clip, samples, image, face_idx, depth, lod, coverage, 1, s);
}

int dtp_op_mesh_view_aa(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                        const dtp_view_opts* opts, int filter, int clip, int samples, uint8_t* image, int* face_idx, float* depth, float* lod,
                        uint8_t* coverage, int binned, dtp_stream s) {
  const ViewCall c{binned == 1 ? "dtp_mesh_view_aa" : "dtp_op_mesh_view_aa", mesh, texture, TH, TW, cam, H, W, opts, image, face_idx, depth, binned, s,
                   filter, mips, lod, clip, samples, coverage};
  RC(view_refuse(c, OWN_FILTER | OWN_CLIP | OWN_SAMPLES));
  return view_run(c);
}

int dtp_mesh_view_aniso(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                        const dtp_view_opts* opts, int clip, int samples, int max_aniso, uint8_t* image, int* face_idx, float* depth, float* lod,
                        uint8_t* taps, uint8_t* coverage, dtp_stream s) {
  return dtp_op_mesh_view_aniso(mesh, texture, TH, TW, mips, cam, H, W, opts, clip, samples, max_aniso, image, face_idx, depth, lod, taps, coverage, 1, s);
}

// samples 1 without a coverage map runs the plain raster kernel, as dtp_mesh_view_mips does; every other call the anti-aliased one
int dtp_op_mesh_view_aniso(dtp_mesh* mesh, const uint8_t* texture, int TH, int TW, const uint8_t* mips, const dtp_view_cam* cam, int H, int W,
                           const dtp_view_opts* opts, int clip, int samples, int max_aniso, uint8_t* image, int* face_idx, float* depth, float* lod,
                           uint8_t* taps, uint8_t* coverage, int binned, dtp_stream s) {
  ViewCall c{binned == 1 ? "dtp_mesh_view_aniso" : "dtp_op_mesh_view_aniso", mesh, texture, TH, TW, cam, H, W, opts, image, face_idx, depth, binned, s,
             2, mips, lod, clip, samples, coverage, max_aniso, taps};
  RC(view_refuse(c, OWN_ANISO | OWN_CLIP | OWN_SAMPLES));
  if (samples == 1 && !coverage) c.samples = 0;
  return view_run(c);
}

}  // extern "C"
