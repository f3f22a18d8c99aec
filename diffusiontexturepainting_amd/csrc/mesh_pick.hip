// Picking on a mesh (dtp_mesh_pick): the render's visibility rule at one sample per ray: the closest hit of N rays, from
// the vertices, faces and UVs alone, so that it runs on a stream of its own beside a stroke.  It touches no stroke state of the mesh
// (mesh.hip), only its own five fields of it.  The ray frame, the grid's exponent and the path planner are mesh_host.h's.
#pragma clang fp contract(off)
#include <string.h>
#include <vector>

#include "mesh_obj.h"

constexpr int PICK_CHUNK = 256;            // ray frames staged in LDS per workgroup of the pick
struct PickRay { float m[12], S, d[3]; };  // 64 B: the ray's frame, its grid S = 2^e, its direction
static_assert(sizeof(PickRay) == 64 && sizeof(dtp_mesh_hit) == 52, "the pick's records are copied as bytes");

namespace {

// ---------------------------------------------------------------- device
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
// every check and the frames of all rays, before any device call
int pick_check(const char* who, const Mesh* m, const dtp_ray* rays, int n, const void* out, std::vector<PickRay>& q) {
  if (!m || !rays || !out) { dtp_set_error("%s: NULL argument (mesh, rays and out are required)", who); return DTP_ERR_ARG; }
  if (n < 1 || n > PICK_MAX_RAYS) { dtp_set_error("%s: n=%d rays (1..%d)", who, n, PICK_MAX_RAYS); return DTP_ERR_ARG; }
  RC(check_mesh(who, m));
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

}  // namespace

extern "C" {

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

}  // extern "C"
