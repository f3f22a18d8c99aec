// Stand-alone host check of the host arithmetic of growing a face set (csrc/topo_host.h) for a sanitizer build: the
// topology of a mesh -- points, parts, charts -- against a brute-force O(F^2) evaluation of the definitions of include/dtp.h with float
// comparisons (topo_host.h compares bit patterns), on meshes known by hand (a quad, a table on a floor, a two-chart grid with shared and
// with duplicated seam vertices and -0.0 against +0.0, a fan of three faces on one edge, two triangles that touch in one point, a face
// with a repeated vertex) and on seeded random small meshes whose vertices come from a small grid, so that coincident points, shared
// edges and non-manifold edges all occur; and the refusals of dtp_mesh_select_extend and dtp_topology_build.  Build and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \
//       tools/topo_host_check.cpp -o topo_host_check && ./topo_host_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <limits>
#include <set>
#include <vector>

#include "topo_host.h"

static int g_checks = 0;
#define EXPECT(cond)                                                                              \
  do {                                                                                            \
    ++g_checks;                                                                                   \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}

struct MeshData {
  std::vector<float> v;   // [V][3]
  std::vector<int> f;     // [F][3]
  std::vector<float> uv;  // [F][3][2]
  int V() const { return (int)v.size() / 3; }
  int F() const { return (int)f.size() / 3; }
  void vertex(float x, float y, float z) { v.push_back(x); v.push_back(y); v.push_back(z); }
  void face(int a, int b, int c, const float (&t)[6]) {
    f.push_back(a); f.push_back(b); f.push_back(c);
    uv.insert(uv.end(), t, t + 6);
  }
};
struct Labels { std::vector<int> point, part, chart; int counts[3]; };

// ---------------------------------------------------------------- the definitions, by brute force
// the classes of "adjacent" closed transitively, each labelled by its lowest face: a flood from every face not yet reached, in ascending order
template <typename Adjacent>
static std::vector<int> classes(int F, Adjacent adjacent) {
  std::vector<int> label((size_t)F, -1), todo;
  for (int f = 0; f < F; ++f) {
    if (label[(size_t)f] >= 0) continue;
    label[(size_t)f] = f;
    todo.assign(1, f);
    while (!todo.empty()) {
      const int a = todo.back();
      todo.pop_back();
      for (int b = 0; b < F; ++b)
        if (label[(size_t)b] < 0 && adjacent(a, b)) { label[(size_t)b] = f; todo.push_back(b); }
    }
  }
  return label;
}

static Labels brute(const MeshData& m) {
  const int V = m.V(), F = m.F();
  Labels r;
  std::vector<int> name((size_t)V);
  for (int i = 0; i < V; ++i)
    for (int j = 0; j <= i; ++j)
      if (m.v[3 * (size_t)j] == m.v[3 * (size_t)i] && m.v[3 * (size_t)j + 1] == m.v[3 * (size_t)i + 1] && m.v[3 * (size_t)j + 2] == m.v[3 * (size_t)i + 2]) {
        name[(size_t)i] = j;  // (float ==: -0.0 equals +0.0; every value is finite)
        break;
      }
  r.point.resize((size_t)3 * F);
  for (size_t i = 0; i < (size_t)3 * F; ++i) r.point[i] = name[(size_t)m.f[i]];
  const int* p = r.point.data();
  const float* uv = m.uv.data();
  r.part = classes(F, [&](int a, int b) {
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l)
        if (p[3 * a + k] == p[3 * b + l]) return true;
    return false;
  });
  auto same_uv = [&](int a, int k, int b, int l) { return uv[6 * a + 2 * k] == uv[6 * b + 2 * l] && uv[6 * a + 2 * k + 1] == uv[6 * b + 2 * l + 1]; };
  r.chart = classes(F, [&](int a, int b) {
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) {
        const int k1 = (k + 1) % 3, l1 = (l + 1) % 3;
        if (p[3 * a + k] == p[3 * a + k1]) continue;  // a side of zero length is no edge
        if (p[3 * a + k] == p[3 * b + l] && p[3 * a + k1] == p[3 * b + l1] && same_uv(a, k, b, l) && same_uv(a, k1, b, l1)) return true;
        if (p[3 * a + k] == p[3 * b + l1] && p[3 * a + k1] == p[3 * b + l] && same_uv(a, k, b, l1) && same_uv(a, k1, b, l)) return true;
      }
    return false;
  });
  r.counts[0] = (int)std::set<int>(r.point.begin(), r.point.end()).size();
  r.counts[1] = (int)std::set<int>(r.part.begin(), r.part.end()).size();
  r.counts[2] = (int)std::set<int>(r.chart.begin(), r.chart.end()).size();
  return r;
}

static Labels build(const MeshData& m) {
  Labels r;
  r.point.resize(m.f.size()); r.part.resize((size_t)m.F()); r.chart.resize((size_t)m.F());
  topo_build(m.v.data(), m.V(), m.f.data(), m.F(), m.uv.data(), r.point.data(), r.part.data(), r.chart.data(), r.counts);
  return r;
}

// topo_build against the brute force; true when every label and count agrees
static bool agrees(const MeshData& m, Labels* out = nullptr) {
  char why[160];
  if (topo_check_mesh(m.v.data(), m.V(), m.f.data(), m.F(), m.uv.data(), why)) return false;
  const Labels a = build(m), b = brute(m);
  if (out) *out = a;
  return a.point == b.point && a.part == b.part && a.chart == b.chart && memcmp(a.counts, b.counts, sizeof a.counts) == 0;
}

// ---------------------------------------------------------------- meshes known by hand
// nx x ny vertices over the unit square, two faces a cell; the cells left of column `mid` carry u = x / 2, the others u = 1 - x / 2, so the
// UVs differ along column mid.  split: that column's vertices exist twice, one copy per side, and the copies write 0.0 as -0.0.
static MeshData grid(int nx, int ny, int mid, bool split) {
  MeshData m;
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) m.vertex((float)(i - mid), (float)j, 0.0f);  // (column mid lies at x = 0)
  std::vector<int> copy((size_t)ny, 0);
  if (split)
    for (int j = 0; j < ny; ++j) {
      copy[(size_t)j] = m.V();
      m.vertex(-0.0f, (float)j, j & 1 ? -0.0f : 0.0f);
    }
  for (int j = 0; j + 1 < ny; ++j)
    for (int i = 0; i + 1 < nx; ++i) {
      const bool left = i < mid;
      auto id = [&](int col, int row) { return split && !left && col == mid ? copy[(size_t)row] : row * nx + col; };
      auto u = [&](int col) { return left ? 0.5f * (float)col / (float)nx : 1.0f - 0.5f * (float)col / (float)nx; };
      const float v0 = (float)j / (float)ny, v1 = (float)(j + 1) / (float)ny;
      m.face(id(i, j), id(i + 1, j), id(i + 1, j + 1), {u(i), v0, u(i + 1), v0, u(i + 1), v1});
      m.face(id(i, j), id(i + 1, j + 1), id(i, j + 1), {u(i), v0, u(i + 1), v1, u(i), v1});
    }
  return m;
}

static MeshData random_mesh(int F) {
  MeshData m;
  const int V = 4 + (int)(rnd() % 60);
  auto coord = [&]() {
    const float c = (float)(rnd() % 3);
    return c == 0.0f && (rnd() & 1) ? -0.0f : c;
  };
  for (int i = 0; i < V; ++i) m.vertex(coord(), coord(), rnd() % 4 ? 0.0f : 1.0f);
  for (int f = 0; f < F; ++f) {
    int id[3];
    for (int k = 0; k < 3; ++k) id[k] = (int)(rnd() % (uint32_t)V);
    if (rnd() % 16 == 0) id[1] = id[0];  // a repeated vertex
    // the UV of a corner is a function of its position, in one of two charts; now and then a corner is moved, or a zero written as -0.0
    const float shift = rnd() % 4 ? 0.0f : 0.5f;
    float t[6];
    for (int k = 0; k < 3; ++k) {
      t[2 * k] = 0.125f * m.v[3 * (size_t)id[k]] + shift;
      t[2 * k + 1] = 0.125f * m.v[3 * (size_t)id[k] + 1] + 0.0625f * m.v[3 * (size_t)id[k] + 2];
      if (rnd() % 32 == 0) t[2 * k] += 0.03125f;
      if (t[2 * k + 1] == 0.0f && (rnd() & 1)) t[2 * k + 1] = -0.0f;
    }
    m.face(id[0], id[1], id[2], t);
  }
  return m;
}

int main() {
  char why[160];
  // ---- keys and classes
  EXPECT(topo_key(0.0f) == 0u && topo_key(-0.0f) == 0u && topo_key(1.0f) == 0x3f800000u && topo_key(-1.0f) == 0xbf800000u);
  EXPECT(topo_key(std::numeric_limits<float>::denorm_min()) == 1u && topo_key(-std::numeric_limits<float>::denorm_min()) == 0x80000001u);
  {
    TopoClasses c(6);
    c.unite(5, 3); c.unite(4, 5); c.unite(1, 2);
    EXPECT(c.find(5) == 3 && c.find(4) == 3 && c.find(3) == 3 && c.find(2) == 1 && c.find(0) == 0);
    c.unite(2, 4);
    EXPECT(c.find(5) == 1 && c.find(3) == 1 && c.find(4) == 1);
  }
  // ---- the refusals of dtp_mesh_select_extend that need no mesh
  EXPECT(topo_check_how(DTP_EXTEND_RINGS, 1, why) == nullptr && topo_check_how(DTP_EXTEND_SHRINK, 64, why) == nullptr);
  EXPECT(topo_check_how(DTP_EXTEND_LINKED, 0, why) == nullptr && topo_check_how(DTP_EXTEND_CHARTS, -7, why) == nullptr);  // (rings is ignored)
  EXPECT(topo_check_how(4, 1, why) && strstr(why, "unknown how 4"));
  EXPECT(topo_check_how(-1, 1, why) && strstr(why, "unknown how -1"));
  EXPECT(topo_check_how(DTP_EXTEND_RINGS, 0, why) && strstr(why, "rings=0 (1..64)"));
  EXPECT(topo_check_how(DTP_EXTEND_SHRINK, 65, why) && strstr(why, "rings=65 (1..64)"));
  EXPECT(topo_check_how(DTP_EXTEND_RINGS, -3, why) != nullptr);
  {
    uint32_t w[8] = {0};
    EXPECT(!topo_sets_overlap(w, w, 4) && !topo_sets_overlap(w, w + 4, 4) && !topo_sets_overlap(w + 4, w, 4));
    EXPECT(topo_sets_overlap(w, w + 3, 4) && topo_sets_overlap(w + 1, w, 4) && topo_sets_overlap(w, (const char*)w + 2, 1));
  }
  // ---- the refusals of dtp_topology_build
  {
    MeshData q = grid(2, 2, 1, false);
    EXPECT(topo_check_mesh(q.v.data(), q.V(), q.f.data(), q.F(), q.uv.data(), why) == nullptr);
    EXPECT(topo_check_mesh(nullptr, q.V(), q.f.data(), q.F(), q.uv.data(), why) && strstr(why, "NULL"));
    EXPECT(topo_check_mesh(q.v.data(), q.V(), nullptr, q.F(), q.uv.data(), why) && topo_check_mesh(q.v.data(), q.V(), q.f.data(), q.F(), nullptr, why));
    EXPECT(topo_check_mesh(q.v.data(), 0, q.f.data(), q.F(), q.uv.data(), why) && strstr(why, "V=0"));
    EXPECT(topo_check_mesh(q.v.data(), q.V(), q.f.data(), 0, q.uv.data(), why) && strstr(why, "F=0"));
    EXPECT(topo_check_mesh(q.v.data(), q.V(), q.f.data(), TOPO_MAX_FACES + 1, q.uv.data(), why) && strstr(why, "F=1048577"));  // (before a face is read)
    MeshData bad = q;
    bad.f[4] = q.V();
    EXPECT(topo_check_mesh(bad.v.data(), bad.V(), bad.f.data(), bad.F(), bad.uv.data(), why) && strstr(why, "face 1 refers to vertex 4 (0..3)"));
    bad.f[4] = -1;
    EXPECT(topo_check_mesh(bad.v.data(), bad.V(), bad.f.data(), bad.F(), bad.uv.data(), why) && strstr(why, "vertex -1"));
    bad = q;
    bad.v[7] = std::numeric_limits<float>::infinity();
    EXPECT(topo_check_mesh(bad.v.data(), bad.V(), bad.f.data(), bad.F(), bad.uv.data(), why) && strstr(why, "vertex 2 is not finite"));
    bad = q;
    bad.uv[9] = std::numeric_limits<float>::quiet_NaN();
    EXPECT(topo_check_mesh(bad.v.data(), bad.V(), bad.f.data(), bad.F(), bad.uv.data(), why) && strstr(why, "face 1 has a UV"));
  }
  // ---- meshes known by hand
  Labels t;
  {
    MeshData quad = grid(2, 2, 1, false);  // one cell, left of the seam column: a quad of two faces
    EXPECT(agrees(quad, &t) && t.counts[0] == 4 && t.counts[1] == 1 && t.counts[2] == 1 && t.part == std::vector<int>({0, 0}));
  }
  {
    MeshData m;  // a table top over a floor: two pieces that share no point
    for (int piece = 0; piece < 2; ++piece) {
      const float s = piece ? 0.4f : 1.0f, z = piece ? 0.5f : 0.0f, u0 = piece ? 0.5f : 0.0f;
      const int b = m.V();
      m.vertex(-s, -s, z); m.vertex(s, -s, z); m.vertex(s, s, z); m.vertex(-s, s, z);
      m.face(b, b + 1, b + 2, {u0, 0.f, u0 + 0.4f, 0.f, u0 + 0.4f, 1.f});
      m.face(b, b + 2, b + 3, {u0, 0.f, u0 + 0.4f, 1.f, u0, 1.f});
    }
    EXPECT(agrees(m, &t) && t.counts[0] == 8 && t.counts[1] == 2 && t.counts[2] == 2);
    EXPECT(t.part == std::vector<int>({0, 0, 2, 2}) && t.chart == std::vector<int>({0, 0, 2, 2}));
  }
  {
    MeshData shared = grid(6, 6, 2, false), split = grid(6, 6, 2, true);
    Labels a, b;
    EXPECT(agrees(shared, &a) && agrees(split, &b));
    EXPECT(shared.F() == 50 && a.counts[0] == 36 && a.counts[1] == 1 && a.counts[2] == 2);
    int left = 0;
    for (int f = 0; f < 50; ++f) left += a.chart[(size_t)f] == 0;
    EXPECT(left == 20 && a.chart[4] == 4);  // two columns of cells left of the seam; the first face right of it names the other chart
    // the seam's vertices twice, a zero of some copies written as -0.0: the same parts and charts, and fewer points than vertices
    EXPECT(split.V() == 42 && b.counts[0] == 36 && b.part == a.part && b.chart == a.chart);
    for (size_t i = 0; i < b.point.size(); ++i) EXPECT(b.point[i] < 36);  // a copy is named by the lower, original index
  }
  {
    MeshData m;  // a fan of three faces on the edge (0, 1): faces 0 and 2 agree in UV along it, face 1 does not
    m.vertex(0, 0, 0); m.vertex(1, 0, 0); m.vertex(0, 1, 0); m.vertex(0, -1, 0); m.vertex(0, 0, 1);
    m.face(0, 1, 2, {0.1f, 0.1f, 0.3f, 0.1f, 0.1f, 0.3f});
    m.face(1, 0, 3, {0.8f, 0.1f, 0.6f, 0.1f, 0.6f, 0.3f});
    m.face(0, 1, 4, {0.1f, 0.1f, 0.3f, 0.1f, 0.2f, 0.0f});
    EXPECT(agrees(m, &t) && t.counts[1] == 1 && t.counts[2] == 2 && t.chart == std::vector<int>({0, 1, 0}));
    // the same with the agreeing pair listed around the other one and the edge reversed: still united
    m.f[6] = 1; m.f[7] = 0;
    std::swap(m.uv[12], m.uv[14]); std::swap(m.uv[13], m.uv[15]);
    EXPECT(agrees(m, &t) && t.chart == std::vector<int>({0, 1, 0}));
  }
  {
    MeshData m;  // two triangles that touch in one point only: one part, two charts, though the UVs at the point agree
    m.vertex(0, 0, 0); m.vertex(1, 0, 0); m.vertex(0, 1, 0); m.vertex(-1, 0, 0); m.vertex(0, -1, 0);
    m.face(0, 1, 2, {0.5f, 0.5f, 0.7f, 0.5f, 0.5f, 0.7f});
    m.face(0, 3, 4, {0.5f, 0.5f, 0.3f, 0.5f, 0.5f, 0.3f});
    EXPECT(agrees(m, &t) && t.counts[1] == 1 && t.counts[2] == 2 && t.chart == std::vector<int>({0, 1}));
    // a third face with a repeated vertex (0, 0, 1): its side of zero length joins nothing, its real edge (0, 1) joins face 0
    m.face(0, 0, 1, {0.5f, 0.5f, 0.5f, 0.5f, 0.7f, 0.5f});
    EXPECT(agrees(m, &t) && t.chart == std::vector<int>({0, 1, 0}));
    // a face that is one point three times has no edge at all: a chart of its own, in the part of the faces at that point
    m.face(0, 0, 0, {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f});
    EXPECT(agrees(m, &t) && t.chart == std::vector<int>({0, 1, 0, 3}) && t.part == std::vector<int>({0, 0, 0, 0}));
  }
  // ---- seeded random small meshes
  long meshes = 0, welded = 0, charts = 0, parts = 0;
  for (int trial = 0; trial < 300; ++trial) {
    const MeshData m = random_mesh(1 + (int)(rnd() % 200));
    EXPECT(agrees(m, &t));
    for (int f = 0; f < m.F(); ++f) {  // a label is the lowest face of its class, and a chart lies in one part
      EXPECT(t.part[(size_t)f] <= f && t.chart[(size_t)f] <= f && t.part[(size_t)t.chart[(size_t)f]] == t.part[(size_t)f]);
    }
    welded += t.counts[0] < m.V();
    parts += t.counts[1]; charts += t.counts[2];
    ++meshes;
  }
  EXPECT(welded > 100 && charts > parts && parts > meshes);  // points coincided, charts split parts, some meshes fell into several parts
  printf("topo_host_check: %d checks passed over %ld random meshes\n", g_checks, meshes);
  return 0;
}
