// The device arithmetic that the mesh strokes (mesh.hip, mesh_bleed.hip, mesh_pick.hip) and the view of a mesh (view.hip) share, so that
// there is ONE coverage rule: vertices snapped to 1/256 pixel, edge functions in int64 with the top-left fill rule and both windings,
// interpolation and the bilinear taps in fp32 one rounded operation at a time.  Every file that includes this is compiled with contraction
// off; the pragma below holds for the rest of the including file as well.  Below it: what view.hip needs of a mesh, which lives in mesh.hip.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "../../include/dtp.h"

constexpr int SNAP_MAX = 1 << 26;  // snapped coordinates are clamped to +-2^26: every edge function fits an int64 with room to spare
constexpr int CHUNK = 256;         // faces staged in LDS per round of a tile
constexpr int MAX_FACES = 1 << 20, MAX_TEX = 32768, MAX_WIN = 4096;  // (the pixel and texel ranges of a face are packed in 16 bits)

__device__ __forceinline__ int snap(float t) { return (int)fminf(fmaxf(rintf(t), -(float)SNAP_MAX), (float)SNAP_MAX); }

__device__ __forceinline__ long long orient(int ax, int ay, int bx, int by, int cx, int cy) {
  return (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
}
// y points down and the edges are taken in the order that makes the area positive: a top edge runs right, a left edge runs up
__device__ __forceinline__ bool top_left(long long dx, long long dy) { return dy < 0 || (dy == 0 && dx > 0); }

// Does the triangle cover the centre (px, py)?  Both windings (s = the area's sign), top-left fill rule; w: the barycentric weights.
__device__ __forceinline__ bool cover(const int X[3], const int Y[3], int px, int py, float w[3]) {
  const long long A = orient(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (A == 0) return false;
  const long long s = A > 0 ? 1 : -1;
  long long E[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;  // the edge opposite vertex k
    E[k] = s * orient(X[a], Y[a], X[b], Y[b], px, py);
    if (E[k] < 0 || (E[k] == 0 && !top_left(s * (X[b] - X[a]), s * (Y[b] - Y[a])))) return false;
  }
  const float fa = (float)(s * A);
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = (float)E[k] / fa;
  return true;
}
// The barycentric weights of cover() at (px, py) with NO inside test: the same sign-normalised edge functions over the same |A|, for a
// point that may lie outside the triangle (a weight is then negative).  false: a triangle of zero area (w untouched).
__device__ __forceinline__ bool weights_at(const int X[3], const int Y[3], int px, int py, float w[3]) {
  const long long A = orient(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (A == 0) return false;
  const long long s = A > 0 ? 1 : -1;
  const float fa = (float)(s * A);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    w[k] = (float)(s * orient(X[a], Y[a], X[b], Y[b], px, py)) / fa;
  }
  return true;
}
__device__ __forceinline__ float interp(const float w[3], float a0, float a1, float a2) { return (w[0] * a0 + w[1] * a1) + w[2] * a2; }

// grid_sample(align_corners=False, padding_mode="border") at pixel position (x, y) of an Hs x Ws image: the four taps and their weights
struct Taps { int x0, x1, y0, y1; float w00, w01, w10, w11; };
__device__ __forceinline__ Taps taps(float x, float y, int Hs, int Ws) {
  x = fminf(fmaxf(x, 0.f), (float)(Ws - 1));
  y = fminf(fmaxf(y, 0.f), (float)(Hs - 1));
  const float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf, gx = 1.0f - fx, gy = 1.0f - fy;
  Taps t;
  t.x0 = (int)xf; t.y0 = (int)yf;
  t.x1 = min(t.x0 + 1, Ws - 1); t.y1 = min(t.y0 + 1, Hs - 1);
  t.w00 = gx * gy; t.w01 = fx * gy; t.w10 = gx * fy; t.w11 = fx * fy;
  return t;
}
__device__ __forceinline__ float blend(const Taps& t, float v00, float v01, float v10, float v11) {
  return ((v00 * t.w00 + v01 * t.w01) + v10 * t.w10) + v11 * t.w11;
}
// the bilinear sample of an h x w RGBA8 image (a texture, or a level of its pyramid) at (u, v): the four taps of grid_sample, byte / 255
// per channel
__device__ __forceinline__ void sample_bilinear(const unsigned int* __restrict__ tex, int h, int w, float u, float v, float tc[4]) {
  const Taps tp = taps(u * (float)w - 0.5f, (1.0f - v) * (float)h - 0.5f, h, w);
  const unsigned int t00 = tex[(size_t)tp.y0 * w + tp.x0], t01 = tex[(size_t)tp.y0 * w + tp.x1];
  const unsigned int t10 = tex[(size_t)tp.y1 * w + tp.x0], t11 = tex[(size_t)tp.y1 * w + tp.x1];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    const int s8 = 8 * ch;
    tc[ch] = blend(tp, (float)((t00 >> s8) & 0xffu) / 255.0f, (float)((t01 >> s8) & 0xffu) / 255.0f,
                   (float)((t10 >> s8) & 0xffu) / 255.0f, (float)((t11 >> s8) & 0xffu) / 255.0f);
  }
}

// the range [lo, hi] of pixel (texel) indices 0 .. n - 1 whose centres 256 i + 128 lie in [a, b]; empty: lo > hi
__device__ __forceinline__ void centre_range(int a, int b, int n, int& lo, int& hi) {
  lo = max((a - 128 + 255) >> 8, 0);
  hi = min((b - 128) >> 8, n - 1);
}
__device__ __forceinline__ int min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int max3(int a, int b, int c) { return max(a, max(b, c)); }
// a range packed as lo | hi << 16 against [lo, hi]
__device__ __forceinline__ bool ranges_meet(int packed, int lo, int hi) { return (packed & 0xffff) <= hi && (packed >> 16) >= lo; }

// an entry of a face list: the face and its pixel (texel) ranges, 16 bits a bound
__device__ __forceinline__ int4 pack_box(int f, int x0, int x1, int y0, int y1) { return make_int4(f, x0 | (x1 << 16), y0 | (y1 << 16), 0); }

// texture-space position of a face's three UVs, snapped to 1/256 texel
__device__ __forceinline__ void snap_uvs(const float* __restrict__ uv, int H, int W, int X[3], int Y[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    X[k] = snap((uv[2 * k] * (float)W) * 256.0f);
    Y[k] = snap(((1.0f - uv[2 * k + 1]) * (float)H) * 256.0f);
  }
}
// a face in texture space: false for a zero area or a texel box without a centre
__device__ __forceinline__ bool face_texels(const float* __restrict__ uv, int H, int W, int X[3], int Y[3], int& x0, int& x1, int& y0, int& y1) {
  snap_uvs(uv, H, W, X, Y);
  if (orient(X[0], Y[0], X[1], Y[1], X[2], Y[2]) == 0) return false;
  centre_range(min3(X[0], X[1], X[2]), max3(X[0], X[1], X[2]), W, x0, x1);
  centre_range(min3(Y[0], Y[1], Y[2]), max3(Y[0], Y[1], Y[2]), H, y0, y1);
  return x0 <= x1 && y0 <= y1;
}

// A 16 x 16 tile at (col0, row0), one thread per pixel (texel), against a list of n_list pack_box entries: the list streams through LDS
// CHUNK entries at a time; an entry whose ranges miss the tile is dropped on the way in, any other takes a slot, which stage(slot, entry)
// fills in the caller's own shared arrays; then every `live` thread calls visit(i) for the slots in turn.  s_n: the caller's shared
// counter.  Every thread of the workgroup must call this (three barriers a round).
template <typename Stage, typename Visit>
__device__ __forceinline__ void stream_faces(const int4* __restrict__ list, int n_list, int col0, int row0, bool live, int& s_n, Stage stage, Visit visit) {
  const int t = threadIdx.x;
  for (int base = 0; base < n_list; base += CHUNK) {
    if (t == 0) s_n = 0;
    __syncthreads();
    if (base + t < n_list) {
      const int4 e = list[base + t];
      if (ranges_meet(e.y, col0, col0 + 15) && ranges_meet(e.z, row0, row0 + 15)) stage(atomicAdd(&s_n, 1), e);
    }
    __syncthreads();
    const int n = s_n;
    if (live)
      for (int i = 0; i < n; ++i) visit(i);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- a mesh, as the view sees it
struct Ctx;
// what a view reads of a mesh (vertices [V][3], faces [F][3], UVs [F][3][2]: never written after dtp_mesh_create), and the slot in which
// the mesh keeps the view's own buffers; sel_poly: the mesh's buffer for the snapped polygon of a lasso (select.hip), 2 x 1024 ints
struct MeshGeom {
  Ctx* ctx;
  int F;
  const float* verts;
  const int* faces;
  const float* uvs;
  void** view;
  int* sel_poly;
};
bool mesh_geom(dtp_mesh* mesh, MeshGeom* out);  // mesh.hip: false = not a live mesh (nothing is followed)
void view_free(void* view);                     // view.hip: frees what *MeshGeom::view holds (null: nothing); called when the mesh is freed
void topo_free(void* topo);                     // topology.hip: the same for the mesh's topology
