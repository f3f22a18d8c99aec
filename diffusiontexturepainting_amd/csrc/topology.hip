// Growing a face set (include/dtp.h "growing a face set"): the topology of a mesh on the device -- built once, on the host,
// by topo_host.h, the code the stand-alone host check runs -- and the steps that grow a set by it: rings, shrink, linked parts, UV charts.
// It reads what dtp_mesh_create copied and nothing a stroke, a pick, a view or a lasso writes, and touches one field of the mesh, its own.
// Integers only.  Plain HIP: vector loads, stores and atomicOr; no kernel waits for another workgroup or loops until nothing changes.
#include <string.h>
#include <algorithm>
#include <vector>

#include "mesh_obj.h"
#include "select_host.h"
#include "topo_host.h"

static_assert(TOPO_MAX_FACES == MAX_FACES, "topo_host.h restates dtp_mesh_create's bound");

namespace {

// per mesh, one allocation: point [F][3], part [F], chart [F], the mark bitset ((max(V, F) + 31) / 32 words), two scratch face sets
struct Topo {
  int* point = nullptr;
  int* part = nullptr;
  int* chart = nullptr;
  unsigned int* marks = nullptr;
  unsigned int* set[2] = {nullptr, nullptr};
  int counts[3] = {0, 0, 0};
};

enum { POINTS = 3, LABEL = 1 };  // the labels a face carries: its three points, or its part / its chart

__device__ __forceinline__ bool bit_of(const unsigned int* set, int i) { return (set[i >> 5] >> (i & 31)) & 1u; }
// test before the atomic: a set bit stays set until the next clear, so a stale read costs an atomic and never loses one
__device__ __forceinline__ void mark(unsigned int* marks, int label) {
  if (!bit_of(marks, label)) atomicOr(&marks[label >> 5], 1u << (label & 31));
}

// One thread per face.  A face of the source -- outside != 0: a face (< F) NOT of the source -- ORs the bits of its labels into the marks.
// PER = POINTS: the three points of a face, which few lanes share.  PER = LABEL: the part or chart, which most lanes of a wave share (a
// hundred thousand faces of one part would all hit one word): the lanes that carry one label elect a leader, as select_kernel does per
// face, and the leader tests the bit first.
template <int PER>
__global__ __launch_bounds__(256) void topo_mark_kernel(const unsigned int* src, int F, const int* __restrict__ labels, int outside,
                                                        unsigned int* marks) {
  const int f = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool on = f < F && bit_of(src, f) != (outside != 0);
  if (PER == POINTS) {
    if (on)
#pragma unroll
      for (int k = 0; k < 3; ++k) mark(marks, labels[3 * (size_t)f + k]);
    return;
  }
  const int label = on ? labels[f] : -1;
  // (converged again: every lane of the wave takes part in the ballots)
  unsigned long long todo = __ballot(label >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(label, leader, 64);
    if (lane == leader) mark(marks, k);
    todo &= ~__ballot(label == k);
  }
}

// One thread per face, no atomics.  keep == 0: the face's bit is "any of its labels is marked" (RINGS, LINKED, CHARTS); keep != 0: "it is
// in the source and none of its labels is marked" (SHRINK).  A thread at f >= F contributes 0.  The 64 bits of a wave leave as two word
// stores from a ballot, after every lane has read the source word of its own face: src == dst is safe.
template <int PER>
__global__ __launch_bounds__(256) void topo_gather_kernel(const unsigned int* src, int F, const int* __restrict__ labels, int keep,
                                                          const unsigned int* __restrict__ marks, unsigned int* dst, int words) {
  const int f = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool bit = false;
  if (f < F) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < PER; ++k) any = any || bit_of(marks, labels[PER * (size_t)f + k]);
    bit = keep ? bit_of(src, f) && !any : any;
  }
  const unsigned long long wave = __ballot(bit);
  const int w = (f - lane) >> 5;  // the first of the wave's two words
  if (lane == 0 && w < words) dst[w] = (unsigned int)wave;
  if (lane == 1 && w + 1 < words) dst[w + 1] = (unsigned int)(wave >> 32);
}

// ---------------------------------------------------------------- host
// The first use of a mesh: copy back, build, allocate, upload -- on s alone, which it waits for.  Pageable memory on both sides: the
// copies are staged on s and the call returns from each when it is done, so nothing here meets the null stream.
int topo_ensure(Mesh* m, const char* who, hipStream_t s, Topo** out) {
  if (m->topo) { *out = (Topo*)m->topo; return DTP_OK; }
  HIP_CHECK(hipSetDevice(m->ctx->device));
  const size_t F = (size_t)m->F, V = (size_t)m->V;
  std::vector<float> verts(3 * V), uvs(6 * F);
  std::vector<int> faces(3 * F), labels(5 * F);
  HIP_CHECK(hipMemcpyAsync(verts.data(), m->verts, V * 12, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(faces.data(), m->faces, F * 12, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(uvs.data(), m->uvs, F * 24, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  Topo* t = new Topo();
  topo_build(verts.data(), m->V, faces.data(), m->F, uvs.data(), labels.data(), labels.data() + 3 * F, labels.data() + 4 * F, t->counts);
  const size_t mark_words = (std::max(V, F) + 31) / 32, set_words = (F + 31) / 32;
  hipError_t e = hipMalloc((void**)&t->point, (5 * F + mark_words + 2 * set_words) * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(t->point, labels.data(), 5 * F * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    dtp_set_error("%s: %s (the topology of V=%d, F=%d)", who, hipGetErrorString(e), m->V, m->F);
    topo_free(t);
    return DTP_ERR_HIP;
  }
  t->part = t->point + 3 * F;
  t->chart = t->part + F;
  t->marks = (unsigned int*)(t->chart + F);
  t->set[0] = t->marks + mark_words;
  t->set[1] = t->set[0] + set_words;
  m->topo = t;
  *out = t;
  return DTP_OK;
}

template <int PER>
void enqueue_step(const Mesh* m, const Topo* t, const int* labels, const unsigned int* src, unsigned int* dst, int words, bool shrink, hipStream_t s) {
  const dim3 grid((unsigned)((m->F + 255) / 256));
  const size_t mark_words = ((size_t)(PER == POINTS ? m->V : m->F) + 31) / 32;
  (void)hipMemsetAsync(t->marks, 0, mark_words * 4, s);
  hipLaunchKernelGGL(topo_mark_kernel<PER>, grid, dim3(256), 0, s, src, m->F, labels, shrink ? 1 : 0, t->marks);
  hipLaunchKernelGGL(topo_gather_kernel<PER>, grid, dim3(256), 0, s, src, m->F, labels, shrink ? 1 : 0, (const unsigned int*)t->marks, dst, words);
}

}  // namespace

void topo_free(void* topo) {
  Topo* t = (Topo*)topo;
  if (!t) return;
  (void)hipFree(t->point);  // (the one allocation; waits for the work that still reads it)
  delete t;
}

extern "C" {

int dtp_topology_build(const float* vertices, int V, const int* faces, int F, const float* face_uvs, int* point, int* part, int* chart,
                       int counts[3]) {
  if (!point || !part || !chart || !counts) {
    dtp_set_error("dtp_topology_build: NULL argument (vertices, faces, face_uvs, point, part, chart and counts are required)");
    return DTP_ERR_ARG;
  }
  char why[160];
  if (topo_check_mesh(vertices, V, faces, F, face_uvs, why)) { dtp_set_error("dtp_topology_build: %s", why); return DTP_ERR_ARG; }
  topo_build(vertices, V, faces, F, face_uvs, point, part, chart, counts);
  return DTP_OK;
}

int dtp_mesh_topology(dtp_mesh* mesh, int counts[3], dtp_stream s) {
  Mesh* m = (Mesh*)mesh;
  RC(check_mesh("dtp_mesh_topology", m));
  Topo* t;
  RC(topo_ensure(m, "dtp_mesh_topology", (hipStream_t)s, &t));
  if (counts) memcpy(counts, t->counts, sizeof t->counts);
  return DTP_OK;
}

int dtp_mesh_topology_labels(dtp_mesh* mesh, int* point, int* part, int* chart, dtp_stream s_) {
  Mesh* m = (Mesh*)mesh;
  hipStream_t s = (hipStream_t)s_;
  RC(check_mesh("dtp_mesh_topology_labels", m));
  Topo* t;
  RC(topo_ensure(m, "dtp_mesh_topology_labels", s, &t));
  HIP_CHECK(hipSetDevice(m->ctx->device));
  const size_t F = (size_t)m->F;
  if (point) HIP_CHECK(hipMemcpyAsync(point, t->point, F * 12, hipMemcpyDeviceToHost, s));
  if (part) HIP_CHECK(hipMemcpyAsync(part, t->part, F * 4, hipMemcpyDeviceToHost, s));
  if (chart) HIP_CHECK(hipMemcpyAsync(chart, t->chart, F * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return DTP_OK;
}

int dtp_mesh_select_extend(dtp_mesh* mesh, const uint32_t* in, uint32_t* out, int words, int how, int rings, dtp_stream s_) {
  hipStream_t s = (hipStream_t)s_;
  Mesh* m = (Mesh*)mesh;
  // ---- every check, before anything is enqueued
  char why[160];
  if (topo_check_how(how, rings, why)) { dtp_set_error("dtp_mesh_select_extend: %s", why); return DTP_ERR_ARG; }
  RC(check_mesh("dtp_mesh_select_extend", m, in && out, " (mesh, in and out are required)"));
  if (select_check_set(in, words, m->F, why) || select_check_set(out, words, m->F, why)) {
    dtp_set_error("dtp_mesh_select_extend: %s", why);
    return DTP_ERR_ARG;
  }
  if (topo_sets_overlap(in, out, words)) {
    dtp_set_error("dtp_mesh_select_extend: in and out overlap without being equal (in place is in == out)");
    return DTP_ERR_ARG;
  }
  Topo* t;
  RC(topo_ensure(m, "dtp_mesh_select_extend", s, &t));  // (the first use of the mesh builds its topology; later calls only enqueue)
  // ---- enqueue: the steps before the last write the mesh's two scratch sets in turn, the last writes out
  HIP_CHECK(hipSetDevice(m->ctx->device));
  const unsigned int* src = (const unsigned int*)in;
  if (how == DTP_EXTEND_LINKED) enqueue_step<LABEL>(m, t, t->part, src, (unsigned int*)out, words, false, s);
  else if (how == DTP_EXTEND_CHARTS) enqueue_step<LABEL>(m, t, t->chart, src, (unsigned int*)out, words, false, s);
  else
    for (int i = 0; i < rings; ++i) {
      unsigned int* dst = i + 1 == rings ? (unsigned int*)out : t->set[i & 1];
      enqueue_step<POINTS>(m, t, t->point, src, dst, words, how == DTP_EXTEND_SHRINK, s);
      src = dst;
    }
  if (hipGetLastError() != hipSuccess) { dtp_set_error("dtp_mesh_select_extend: a kernel launch failed"); return DTP_ERR_HIP; }
  return DTP_OK;
}

}  // extern "C"
