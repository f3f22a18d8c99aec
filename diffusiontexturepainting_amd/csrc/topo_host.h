// The host-only arithmetic of growing a face set (include/dtp.h "growing a face set"): the topology of a mesh -- the points
// its vertices weld to, the parts its faces are linked in, its UV charts -- and every argument check of dtp_mesh_select_extend and
// dtp_topology_build that needs no mesh object.  Everything is exact: keys are bit patterns, classes come from a union-find whose root is
// the lowest index, so no label depends on the order in which anything is met.  No device call, so the stand-alone sanitizer program
// (tools/topo_host_check.cpp) drives it directly, built by a plain C++ compiler.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/dtp.h"

constexpr int TOPO_MAX_FACES = 1 << 20;  // MAX_FACES of mesh_dev.h: dtp_mesh_create's bound
constexpr int TOPO_MAX_RINGS = 64;       // a call of RINGS or SHRINK launches 3 x rings times at most

// nullptr, or what dtp_mesh_select_extend refuses before it looks at the mesh; `why` holds the message
inline const char* topo_check_how(int how, int rings, char why[160]) {
  if (how != DTP_EXTEND_RINGS && how != DTP_EXTEND_SHRINK && how != DTP_EXTEND_LINKED && how != DTP_EXTEND_CHARTS) {
    snprintf(why, 160, "unknown how %d (RINGS = 0, SHRINK = 1, LINKED = 2, CHARTS = 3)", how);
    return why;
  }
  if ((how == DTP_EXTEND_RINGS || how == DTP_EXTEND_SHRINK) && (rings < 1 || rings > TOPO_MAX_RINGS)) {
    snprintf(why, 160, "rings=%d (1..%d)", rings, TOPO_MAX_RINGS);
    return why;
  }
  return nullptr;
}

// are the `words` 32-bit words at a and at b neither the same array nor disjoint?
inline bool topo_sets_overlap(const void* a, const void* b, int words) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, n = (uintptr_t)words * 4;
  return x != y && x < y + n && y < x + n;
}

// the argument checks of dtp_mesh_create, on the data alone; nullptr or the message
inline const char* topo_check_mesh(const float* vertices, int V, const int* faces, int F, const float* face_uvs, char why[160]) {
  if (!vertices || !faces || !face_uvs) {
    snprintf(why, 160, "NULL argument (vertices, faces and face_uvs are required)");
    return why;
  }
  if (V < 1 || F < 1 || F > TOPO_MAX_FACES) {
    snprintf(why, 160, "V=%d vertices, F=%d faces (V >= 1, 1 <= F <= %d)", V, F, TOPO_MAX_FACES);
    return why;
  }
  for (size_t i = 0; i < (size_t)3 * V; ++i)
    if (!std::isfinite(vertices[i])) {
      snprintf(why, 160, "vertex %d is not finite", (int)(i / 3));
      return why;
    }
  for (int f = 0; f < F; ++f) {
    for (int k = 0; k < 3; ++k)
      if (faces[3 * (size_t)f + k] < 0 || faces[3 * (size_t)f + k] >= V) {
        snprintf(why, 160, "face %d refers to vertex %d (0..%d)", f, faces[3 * (size_t)f + k], V - 1);
        return why;
      }
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(face_uvs[6 * (size_t)f + k])) {
        snprintf(why, 160, "face %d has a UV that is not finite", f);
        return why;
      }
  }
  return nullptr;
}

// the bit pattern of a finite float with -0.0 taken as +0.0: equal floats, equal keys
inline uint32_t topo_key(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u == 0x80000000u ? 0u : u;
}

// classes of 0 .. n - 1 whose root is the lowest member: the larger root always goes under the smaller, so find(i) IS the label
struct TopoClasses {
  std::vector<int> up;
  explicit TopoClasses(int n) : up((size_t)n) {
    for (int i = 0; i < n; ++i) up[(size_t)i] = i;
  }
  int find(int i) {
    while (up[(size_t)i] != i) {
      up[(size_t)i] = up[(size_t)up[(size_t)i]];  // (path halving: a parent is never larger than its child)
      i = up[(size_t)i];
    }
    return i;
  }
  void unite(int a, int b) {
    a = find(a); b = find(b);
    if (a < b) up[(size_t)b] = a;
    else up[(size_t)a] = b;
  }
};

// one side of a face that joins two different points: the points in ascending order and the UVs the face carries at them
struct TopoEdge {
  uint64_t pts, uv_lo, uv_hi;  // lo << 32 | hi; the keys of (u, v) at lo; at hi
  int face;
  bool same_uvs(const TopoEdge& o) const { return pts == o.pts && uv_lo == o.uv_lo && uv_hi == o.uv_hi; }
  bool operator<(const TopoEdge& o) const {
    if (pts != o.pts) return pts < o.pts;
    if (uv_lo != o.uv_lo) return uv_lo < o.uv_lo;
    return uv_hi < o.uv_hi;
  }
};

// The topology of checked data.  point [F][3]: the lowest vertex index with the key of faces[f][k]; part [F], chart [F]: the lowest face
// index of the class; counts: the distinct values of each.
inline void topo_build(const float* vertices, int V, const int* faces, int F, const float* face_uvs, int* point, int* part, int* chart,
                       int counts[3]) {
  // ---- points: the vertices sorted by key, then index; the first of a run names it
  std::vector<int> name((size_t)V), order((size_t)V);
  {
    std::vector<uint32_t> key((size_t)3 * V);
    for (size_t i = 0; i < (size_t)3 * V; ++i) key[i] = topo_key(vertices[i]);
    for (int i = 0; i < V; ++i) order[(size_t)i] = i;
    auto less = [&](int a, int b) {
      const int c = memcmp(&key[(size_t)3 * a], &key[(size_t)3 * b], 12);  // (any total order of the keys will do: only equality names a point)
      return c != 0 ? c < 0 : a < b;
    };
    std::sort(order.begin(), order.end(), less);
    for (int i = 0, first = 0; i < V; ++i) {
      if (i > 0 && memcmp(&key[(size_t)3 * order[(size_t)i]], &key[(size_t)3 * order[(size_t)first]], 12) != 0) first = i;
      name[(size_t)order[(size_t)i]] = order[(size_t)first];
    }
  }
  for (size_t i = 0; i < (size_t)3 * F; ++i) point[i] = name[(size_t)faces[i]];
  // ---- parts: every face joins the first face met at each of its points
  std::vector<int>& first_face = order;  // (reused: V entries)
  std::fill(first_face.begin(), first_face.end(), -1);
  int n_points = 0;
  {
    TopoClasses cls(F);
    for (int f = 0; f < F; ++f)
      for (int k = 0; k < 3; ++k) {
        int& seen = first_face[(size_t)point[3 * (size_t)f + k]];
        if (seen < 0) { seen = f; ++n_points; }
        else cls.unite(seen, f);
      }
    for (int f = 0; f < F; ++f) part[f] = cls.find(f);
  }
  // ---- charts: the sides sorted by edge, then UVs; the faces of a run of equal records are one class
  {
    std::vector<TopoEdge> edges;
    edges.reserve((size_t)3 * F);
    for (int f = 0; f < F; ++f)
      for (int k = 0; k < 3; ++k) {
        const int j = k == 2 ? 0 : k + 1;
        int a = point[3 * (size_t)f + k], b = point[3 * (size_t)f + j];
        if (a == b) continue;  // a side of zero length is no edge
        const float* ua = face_uvs + 6 * (size_t)f + 2 * k;
        const float* ub = face_uvs + 6 * (size_t)f + 2 * j;
        if (a > b) { std::swap(a, b); std::swap(ua, ub); }
        edges.push_back(TopoEdge{(uint64_t)(uint32_t)a << 32 | (uint32_t)b, (uint64_t)topo_key(ua[0]) << 32 | topo_key(ua[1]),
                                 (uint64_t)topo_key(ub[0]) << 32 | topo_key(ub[1]), f});
      }
    std::sort(edges.begin(), edges.end());
    TopoClasses cls(F);
    for (size_t i = 1; i < edges.size(); ++i)
      if (edges[i].same_uvs(edges[i - 1])) cls.unite(edges[i - 1].face, edges[i].face);
    for (int f = 0; f < F; ++f) chart[f] = cls.find(f);
  }
  int n_parts = 0, n_charts = 0;
  for (int f = 0; f < F; ++f) { n_parts += part[f] == f; n_charts += chart[f] == f; }
  counts[0] = n_points; counts[1] = n_parts; counts[2] = n_charts;
}
