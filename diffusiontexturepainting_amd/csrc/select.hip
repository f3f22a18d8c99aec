// Face sets (include/dtp.h "face sets: a lasso, masked strokes, a tint"): the lasso that makes one from what a frame
// shows (dtp_mesh_select) and the tint that shows one on a finished frame (dtp_view_tint).  The stroke that respects one is mesh.hip's
// (dtp_mesh_stroke_masked: one more condition in mesh_valid_kernel).  Integers only: the polygon is snapped on the host by the raster's
// snap, and the inside test is select_host.h's, the code the stand-alone host check runs.  Plain HIP: vector loads, stores and atomics.
#include <string.h>
#include <algorithm>

#include "engine.h"
#include "mesh_dev.h"
#include "select_host.h"

namespace {

constexpr int STAGE_VERTS = 384;            // vertices one staging launch carries in its arguments (3 KB of the 4 KB a launch may pass)
struct PolyChunk { int xy[2 * STAGE_VERTS]; };

// The snapped polygon travels to the mesh's buffer as kernel arguments, which the launch copies before it returns: the call only
// enqueues, needs no pinned buffer, and the caller's array is free at once.  At most three launches.
__global__ __launch_bounds__(128) void select_stage_kernel(PolyChunk chunk, int count, int* __restrict__ dst) {
  for (int i = threadIdx.x; i < 2 * count; i += 128) dst[i] = chunk.xy[i];
}

// One workgroup per 16 x 16 pixels of the polygon's pixel box [x0, x1] x [y0, y1] (clipped to the frame by the host; the tiles start at
// multiples of 16), one thread per pixel.  The polygon is staged in LDS whole (8 KB), and with it the list of the edges that can count
// for a centre of THIS tile (2 KB): an edge counts only for rows in [min y, max y) and only left of its larger x, so an edge that
// misses the tile's 16 rows or lies left of its first column is dropped on the way in (the parity does not depend on the order).  A
// pixel inside sets (clear: clears) the bit of its face, one atomic per distinct face of a wave: the lanes that share a face elect a
// leader, as view.hip's wave_add does for its bin counters.  A face_idx value outside 0 .. F - 1 is skipped, never used as an index.
__global__ __launch_bounds__(256) void select_kernel(const int* __restrict__ face_idx, int W, int F, const int* __restrict__ poly, int n, int x0,
                                                     int x1, int y0, int y1, int clear, unsigned int* __restrict__ out) {
  __shared__ int s_xy[2 * SELECT_MAX_VERTS];
  __shared__ unsigned short s_edge[SELECT_MAX_VERTS];
  __shared__ int s_n;
  const int t = threadIdx.x, lane = t & 63;
  const int col0 = (x0 & ~15) + 16 * blockIdx.x, row0 = (y0 & ~15) + 16 * blockIdx.y;
  if (t == 0) s_n = 0;
  for (int i = t; i < 2 * n; i += 256) s_xy[i] = poly[i];
  __syncthreads();
  const int py_first = 256 * row0 + 128, py_last = py_first + 256 * 15, px_first = 256 * col0 + 128;
  for (int i = t; i < n; i += 256) {
    const int j = i + 1 == n ? 0 : i + 1;
    const int ax = s_xy[2 * i], ay = s_xy[2 * i + 1], bx = s_xy[2 * j], by = s_xy[2 * j + 1];
    if (min(ay, by) <= py_last && max(ay, by) > py_first && max(ax, bx) > px_first) s_edge[atomicAdd(&s_n, 1)] = (unsigned short)i;
  }
  __syncthreads();
  const int col = col0 + (t & 15), row = row0 + (t >> 4);
  const bool live = col >= x0 && col <= x1 && row >= y0 && row <= y1;  // (x1 < W and y1 < H: inside the frame)
  const int px = 256 * col + 128, py = 256 * row + 128, m = s_n;
  bool in = false;
  if (live)
    for (int e = 0; e < m; ++e) {
      const int i = s_edge[e], j = i + 1 == n ? 0 : i + 1;
      if (select_edge_counts(s_xy[2 * i], s_xy[2 * i + 1], s_xy[2 * j], s_xy[2 * j + 1], px, py)) in = !in;
    }
  int f = -1;
  if (in) {
    f = face_idx[(size_t)row * W + col];
    if (f < 0 || f >= F) f = -1;
  }
  // (converged again: every lane of the wave takes part in the ballots)
  unsigned long long todo = __ballot(f >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(f, leader, 64);
    if (lane == leader) {
      if (clear) atomicAnd(&out[k >> 5], ~(1u << (k & 31)));
      else atomicOr(&out[k >> 5], 1u << (k & 31));
    }
    todo &= ~__ballot(f == k);
  }
}

// One thread per pixel: where face_idx is a selected face, R, G, B become (c (255 - a) + t a + 127) / 255; alpha and every other pixel
// are neither read nor written.
__global__ __launch_bounds__(256) void view_tint_kernel(unsigned int* __restrict__ frame, const int* __restrict__ face_idx, size_t pixels, int F,
                                                        const unsigned int* __restrict__ sel, unsigned int tint, unsigned int a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const int f = face_idx[i];
  if (f < 0 || f >= F || !((sel[f >> 5] >> (f & 31)) & 1u)) return;
  const unsigned int c = frame[i];
  unsigned int o = c & 0xff000000u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned int v = (((c >> (8 * ch)) & 0xffu) * (255u - a) + ((tint >> (8 * ch)) & 0xffu) * a + 127u) / 255u;
    o |= v << (8 * ch);
  }
  frame[i] = o;
}

}  // namespace

extern "C" {

int dtp_mesh_select(dtp_mesh* mesh, const int* face_idx, int H, int W, const float* polygon, int n, int op, uint32_t* out, int words, dtp_stream s_) {
  hipStream_t s = (hipStream_t)s_;
  // ---- every check, before anything is enqueued
  if (!polygon) { dtp_set_error("dtp_mesh_select: NULL argument (mesh, face_idx, polygon and out are required)"); return DTP_ERR_ARG; }
  char why[160];
  if (select_check(polygon, n, op, H, W, why)) { dtp_set_error("dtp_mesh_select: %s", why); return DTP_ERR_ARG; }
  if (!mesh || !face_idx || !out) { dtp_set_error("dtp_mesh_select: NULL argument (mesh, face_idx, polygon and out are required)"); return DTP_ERR_ARG; }
  MeshGeom g;
  if (!mesh_geom(mesh, &g)) { dtp_set_error("dtp_mesh_select: the mesh is not a live mesh (destroyed?)"); return DTP_ERR_ARG; }
  if (select_check_set(out, words, g.F, why)) { dtp_set_error("dtp_mesh_select: %s", why); return DTP_ERR_ARG; }
  if (((uintptr_t)face_idx & 3) != 0) { dtp_set_error("dtp_mesh_select: face_idx must be 4-byte aligned"); return DTP_ERR_ARG; }
  PolyChunk chunk;
  int xy[2 * SELECT_MAX_VERTS], x0, x1, y0, y1;
  select_snap_polygon(polygon, n, xy);
  const bool any = select_box(xy, n, H, W, x0, x1, y0, y1);
  // ---- enqueue
  HIP_CHECK(hipSetDevice(g.ctx->device));
  if (op == DTP_SELECT_REPLACE) HIP_CHECK(hipMemsetAsync(out, 0, (size_t)words * 4, s));
  if (!any) return DTP_OK;  // no centre of the frame lies in the polygon's box: no tile is launched
  for (int base = 0; base < n; base += STAGE_VERTS) {
    const int count = std::min(STAGE_VERTS, n - base);
    memcpy(chunk.xy, xy + 2 * base, (size_t)count * 8);
    hipLaunchKernelGGL(select_stage_kernel, dim3(1), dim3(128), 0, s, chunk, count, g.sel_poly + 2 * base);
  }
  const dim3 tiles((x1 >> 4) - (x0 >> 4) + 1, (y1 >> 4) - (y0 >> 4) + 1);
  hipLaunchKernelGGL(select_kernel, tiles, dim3(256), 0, s, face_idx, W, g.F, g.sel_poly, n, x0, x1, y0, y1, op == DTP_SELECT_SUBTRACT ? 1 : 0,
                     (unsigned int*)out);
  if (hipGetLastError() != hipSuccess) { dtp_set_error("dtp_mesh_select: a kernel launch failed"); return DTP_ERR_HIP; }
  return DTP_OK;
}

int dtp_view_tint(dtp_ctx* ctx, uint8_t* frame, const int* face_idx, int H, int W, const uint32_t* set, int words, int F, const uint8_t color[3],
                  int opacity, dtp_stream s) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !frame || !face_idx || !set || !color) { dtp_set_error("dtp_view_tint: NULL argument"); return DTP_ERR_ARG; }
  if (H < 1 || W < 1 || H > SELECT_MAX_SIDE || W > SELECT_MAX_SIDE) {
    dtp_set_error("dtp_view_tint: a %d x %d frame (each side 1..%d)", H, W, SELECT_MAX_SIDE);
    return DTP_ERR_ARG;
  }
  if (F < 1 || F > MAX_FACES) { dtp_set_error("dtp_view_tint: F=%d faces (1..%d)", F, MAX_FACES); return DTP_ERR_ARG; }
  char why[160];
  if (select_check_set(set, words, F, why)) { dtp_set_error("dtp_view_tint: %s", why); return DTP_ERR_ARG; }
  if (opacity < 0 || opacity > 255) { dtp_set_error("dtp_view_tint: opacity=%d outside 0..255", opacity); return DTP_ERR_ARG; }
  if ((((uintptr_t)frame | (uintptr_t)face_idx) & 3) != 0) { dtp_set_error("dtp_view_tint: frame and face_idx must be 4-byte aligned"); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(c->device));
  const size_t pixels = (size_t)H * W;
  const unsigned int tint = (unsigned int)color[0] | ((unsigned int)color[1] << 8) | ((unsigned int)color[2] << 16);
  hipLaunchKernelGGL(view_tint_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)s, (unsigned int*)frame, face_idx, pixels, F,
                     (const unsigned int*)set, tint, (unsigned int)opacity);
  if (hipGetLastError() != hipSuccess) { dtp_set_error("dtp_view_tint: a kernel launch failed"); return DTP_ERR_HIP; }
  return DTP_OK;
}

}  // extern "C"
