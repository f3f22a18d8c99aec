// Coverage and the bleed pass of the mesh strokes (dtp_mesh_stroke_bleed, dtp_mesh_bleed): the bleed pads the UV charts
// after a backprojection (mesh.hip): the texels no face of the mesh covers take the nearest covered texel, by the same integer coverage
// as the strokes'.  The coverage of a texture size is built once per mesh; the offset table and the rectangle's clipping are mesh_host.h's.
#pragma clang fp contract(off)
#include <string.h>
#include <algorithm>

#include "mesh_obj.h"

namespace {

constexpr int SMALL_BOX = 1024;  // coverage build: a face whose texel box holds at most this many centres is rasterised by one wave

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
      if (at < F) big[at] = pack_box(f, x0, x1, y0, y1);
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
  stream_faces(big, n_big, col0, row0, live, s_n, [&](int slot, const int4& e) { snap_uvs(uvs + (size_t)6 * e.x, H, W, s_X[slot], s_Y[slot]); },
      [&](int i) {
        float w[3];
        if (!in) in = cover(s_X[i], s_Y[i], px, py, w);
      });
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

}  // namespace

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

extern "C" {

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
  RC(check_mesh("dtp_mesh_bleed", m));
  if (bleed == 0 || clipped > 0) return DTP_OK;  // nothing to do
  HIP_CHECK(hipSetDevice(m->ctx->device));
  RC(ensure_coverage(m, H, W, (hipStream_t)s));
  return enqueue_bleed(m, texture, H, W, bleed, r, (hipStream_t)s);
}

int dtp_op_mesh_coverage(dtp_mesh* mesh, int H, int W, uint8_t* out, dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  if (!m || !out) { dtp_set_error("dtp_op_mesh_coverage: NULL argument"); return DTP_ERR_ARG; }
  if (H < 1 || W < 1 || H > MAX_TEX || W > MAX_TEX) { dtp_set_error("dtp_op_mesh_coverage: a %d x %d texture (each side 1..%d)", H, W, MAX_TEX); return DTP_ERR_ARG; }
  RC(check_mesh("dtp_op_mesh_coverage", m));
  HIP_CHECK(hipSetDevice(m->ctx->device));
  RC(ensure_coverage(m, H, W, (hipStream_t)s));
  const size_t n = (size_t)H * W;
  hipLaunchKernelGGL(mesh_cover_bytes_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)s, m->cov, H, W, out);
  return launch_ok();
}

}  // extern "C"
