// Stand-alone host check of picking on a mesh (csrc/mesh_pick.hip, csrc/mesh_host.h) for a sanitizer build: the part of it
// that needs no device -- the ray frame, the exponent of a ray's grid, the stamp spacing of a pointer path and its state, and the
// argument checks of dtp_mesh_pick, dtp_op_mesh_pick and dtp_mesh_path_plan, all of which return before their first HIP call -- driven
// from its own main().  mesh_pick.hip needs one thing of the rest of the library, the live set of csrc/mesh.hip: here no mesh is live.
// Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I diffusiontexturepainting_amd/csrc diffusiontexturepainting_amd/csrc/mesh_pick.hip tools/mesh_pick_host_check.cpp \
//         -o mesh_pick_host_check
//   ./mesh_pick_host_check
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mesh_host.h"

static char g_err[1024];
void dtp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
struct Mesh;
bool mesh_alive(const Mesh*) { return false; }

static int g_checks = 0;
#define EXPECT(cond)                                                                      \
  do {                                                                                    \
    ++g_checks;                                                                           \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_err); return 1; } \
  } while (0)

static dtp_mesh_hit hit_at(float x, float y, float z, float nx) {
  dtp_mesh_hit h = {};
  h.face = 3; h.pos[0] = x; h.pos[1] = y; h.pos[2] = z; h.normal[0] = nx; h.normal[2] = 1.f;
  return h;
}
static dtp_mesh_hit miss() {
  dtp_mesh_hit h = {};
  h.face = -1;
  return h;
}

int main() {
  // ---- the ray frame: orthonormal rows, the origin at 0, the direction along -z, into a buffer of exactly 12 floats
  std::vector<float> frame(12);
  const float rays[][6] = {{0.25f, 0.5f, 2.f, 0, 0, -1}, {1, 2, -3, 0, 0, 2.5f}, {5, -1, 0.5f, 1, 0, 0}, {0.3f, 0.2f, 0.1f, 0.5f, -0.5f, 1},
                           {1, 1, 1, -1, 1, -1}, {0.3f, -1.7f, 2.9f, 0.2f, 0.5f, -0.84f}, {1234.5f, -987.25f, 400.125f, -0.6f, 0.1f, 0.79f},
                           {0, 0, 1, 1e-30f, -2e-30f, -3e-30f}};
  for (const auto& r : rays) {
    EXPECT(dtp_mesh_ray_frame(r, r + 3, frame.data()) == DTP_OK);
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) {
        double dot = 0;
        for (int i = 0; i < 3; ++i) dot += (double)frame[4 * k + i] * frame[4 * j + i];
        EXPECT(fabs(dot - (k == j ? 1.0 : 0.0)) < 1e-6);
      }
    const double len = sqrt((double)r[3] * r[3] + (double)r[4] * r[4] + (double)r[5] * r[5]);
    const double scale = fmax(1.0, fmax(fabs(r[0]), fmax(fabs(r[1]), fabs(r[2]))));
    for (int k = 0; k < 3; ++k) {
      double at_o = frame[4 * k + 3], along = 0;
      for (int i = 0; i < 3; ++i) { at_o += (double)frame[4 * k + i] * r[i]; along += (double)frame[4 * k + i] * r[3 + i] / len; }
      EXPECT(fabs(at_o) < 2e-6 * scale && fabs(along - (k == 2 ? -1.0 : 0.0)) < 1e-6);
    }
  }
  const float o[3] = {1, 2, 3}, down[3] = {0, 0, -1}, zero[3] = {0, 0, 0}, nanv[3] = {NAN, 0, 1}, infv[3] = {0, INFINITY, 1};
  const float huge[3] = {3e38f, 3e38f, 3e38f}, ones[3] = {1, 1, 1};
  EXPECT(dtp_mesh_ray_frame(o, down, frame.data()) == DTP_OK);
  const float want[12] = {0, -1, 0, 2, 1, 0, 0, -1, 0, 0, 1, -3};
  for (int i = 0; i < 12; ++i) EXPECT(frame[i] == want[i]);
  std::vector<float> keep(frame);
  EXPECT(dtp_mesh_ray_frame(o, zero, frame.data()) == DTP_ERR_ARG && strstr(g_err, "direction is zero"));
  EXPECT(dtp_mesh_ray_frame(o, nanv, frame.data()) == DTP_ERR_ARG && strstr(g_err, "non-finite direction"));
  EXPECT(dtp_mesh_ray_frame(o, infv, frame.data()) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_ray_frame(nanv, down, frame.data()) == DTP_ERR_ARG && strstr(g_err, "non-finite origin"));
  EXPECT(dtp_mesh_ray_frame(huge, ones, frame.data()) == DTP_ERR_ARG && strstr(g_err, "fit fp32"));
  EXPECT(dtp_mesh_ray_frame(nullptr, down, frame.data()) == DTP_ERR_ARG && dtp_mesh_ray_frame(o, nullptr, frame.data()) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_ray_frame(o, down, nullptr) == DTP_ERR_ARG);
  EXPECT(frame == keep);  // a refused call writes nothing

  // ---- the grid's exponent: 2^e max(|x|, |y|) <= 2^25 < 2^(e + 1) max, clamped
  const float above[3] = {0, 0, 2};
  EXPECT(dtp_mesh_ray_frame(above, down, frame.data()) == DTP_OK);
  struct { double lo[3], hi[3]; int e; } boxes[] = {
      {{0, 0, 0}, {1, 1, 0}, 25}, {{0, 0, 0}, {1.5, 1, 0}, 24}, {{-4, 0, 0}, {1, 1, 0}, 23}, {{0, 0, -5}, {0, 0, 7}, PICK_E_MAX},
      {{0, 0, 0}, {ldexp(1.0, -60), 0, 0}, PICK_E_MAX}, {{0, 0, 0}, {ldexp(1.0, 100), 0, 0}, PICK_E_MIN}, {{-0.3, -0.2, 0}, {0.7, 0.1, 3}, 25},
      {{0, 0, 0}, {INFINITY, 0, 0}, PICK_E_MIN}};
  for (const auto& b : boxes) EXPECT(mesh_pick_exponent(frame.data(), b.lo, b.hi) == b.e);
  for (const auto& r : rays) {  // the defining inequality on a box that is not aligned with the frame
    const double lo[3] = {-1.0, -0.75, -0.4}, hi[3] = {1.0, 0.75, 0.45};
    EXPECT(dtp_mesh_ray_frame(r, r + 3, frame.data()) == DTP_OK);
    const int e = mesh_pick_exponent(frame.data(), lo, hi);
    double m = 0;
    for (int c = 0; c < 8; ++c)
      for (int k = 0; k < 2; ++k) {
        const double v[3] = {c & 1 ? hi[0] : lo[0], c & 2 ? hi[1] : lo[1], c & 4 ? hi[2] : lo[2]};
        m = fmax(m, fabs((((double)frame[4 * k] * v[0] + (double)frame[4 * k + 1] * v[1]) + (double)frame[4 * k + 2] * v[2]) + (double)frame[4 * k + 3]));
      }
    EXPECT(e > PICK_E_MIN && e < PICK_E_MAX && ldexp(m, e) <= ldexp(1.0, 25) && ldexp(m, e + 1) > ldexp(1.0, 25));
  }

  // ---- the planner, into arrays of exactly the capacity
  {
    const dtp_mesh_hit hits[] = {hit_at(0, 0, 0, 0), miss(), hit_at(5, 0, 0, 1), hit_at(5, 0.5f, 0, 2), hit_at(5, 3, 0, 3)};
    dtp_path_state st = {};
    int count = -1;
    EXPECT(dtp_mesh_path_plan(hits, 1, 2.f, &st, nullptr, nullptr, nullptr, 0, &count) == DTP_OK && count == 0);
    EXPECT(st.has_prev == 1 && st.prev[0] == 0.f);  // the first hit only starts the path
    st = {};
    EXPECT(dtp_mesh_path_plan(hits, 5, 2.f, &st, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG && count == 3 && strstr(g_err, "capacity 0"));
    EXPECT(st.has_prev == 0);  // too small: the state stays
    std::vector<float> pos(6), nrm(6), prev(6);
    EXPECT(dtp_mesh_path_plan(hits, 5, 2.f, &st, pos.data(), nrm.data(), prev.data(), 2, &count) == DTP_ERR_ARG && count == 3 && st.has_prev == 0);
    pos.assign(9, 7.f); nrm.assign(9, 7.f); prev.assign(9, 7.f);
    EXPECT(dtp_mesh_path_plan(hits, 5, 2.f, &st, pos.data(), nrm.data(), prev.data(), 3, &count) == DTP_OK && count == 3);
    const float want_pos[9] = {2.5f, 0, 0, 5, 0, 0, 5, 3, 0}, want_prev[9] = {0, 0, 0, 2.5f, 0, 0, 5, 0, 0}, want_nrm[9] = {1, 0, 1, 1, 0, 1, 3, 0, 1};
    for (int i = 0; i < 9; ++i) EXPECT(pos[i] == want_pos[i] && prev[i] == want_prev[i] && nrm[i] == want_nrm[i]);
    EXPECT(st.has_prev == 1 && st.prev[0] == 5.f && st.prev[1] == 3.f && st.prev[2] == 0.f);
    // the same path in two calls that carry the state
    for (int cut = 1; cut < 5; ++cut) {
      dtp_path_state s2 = {};
      std::vector<float> p2(9, 7.f), n2(9, 7.f), v2(9, 7.f);
      int c1 = -1, c2 = -1;
      EXPECT(dtp_mesh_path_plan(hits, cut, 2.f, &s2, p2.data(), n2.data(), v2.data(), 3, &c1) == DTP_OK);
      EXPECT(dtp_mesh_path_plan(hits + cut, 5 - cut, 2.f, &s2, p2.data() + 3 * c1, n2.data() + 3 * c1, v2.data() + 3 * c1, 3 - c1, &c2) == DTP_OK);
      EXPECT(c1 + c2 == 3 && p2 == pos && n2 == nrm && v2 == prev && memcmp(&s2, &st, sizeof st) == 0);
    }
    // refusals leave the state and the count alone
    dtp_path_state s3 = {1, {1, 1, 1}};
    count = -7;
    const float bad[] = {0.f, -1.f, NAN, INFINITY};
    for (float sd : bad) EXPECT(dtp_mesh_path_plan(hits, 5, sd, &s3, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG && strstr(g_err, "stamp_distance"));
    EXPECT(dtp_mesh_path_plan(hits, 5, 1e-9f, &s3, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG && strstr(g_err, "chord"));
    EXPECT(dtp_mesh_path_plan(nullptr, 5, 1.f, &s3, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG);
    EXPECT(dtp_mesh_path_plan(hits, 5, 1.f, nullptr, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG);
    EXPECT(dtp_mesh_path_plan(hits, 5, 1.f, &s3, nullptr, nullptr, nullptr, 0, nullptr) == DTP_ERR_ARG);
    EXPECT(dtp_mesh_path_plan(hits, 5, 1.f, &s3, nullptr, nrm.data(), prev.data(), 3, &count) == DTP_ERR_ARG);
    EXPECT(dtp_mesh_path_plan(hits, -1, 1.f, &s3, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG);
    EXPECT(dtp_mesh_path_plan(hits, 5, 1.f, &s3, pos.data(), nrm.data(), prev.data(), -1, &count) == DTP_ERR_ARG);
    dtp_mesh_hit nan_hit = hit_at(NAN, 0, 0, 0);
    EXPECT(dtp_mesh_path_plan(&nan_hit, 1, 1.f, &s3, nullptr, nullptr, nullptr, 0, &count) == DTP_ERR_ARG && strstr(g_err, "hit 0"));
    EXPECT(count == -7 && s3.has_prev == 1 && s3.prev[0] == 1.f && s3.prev[1] == 1.f && s3.prev[2] == 1.f);
    EXPECT(dtp_mesh_path_plan(nullptr, 0, 1.f, &s3, nullptr, nullptr, nullptr, 0, &count) == DTP_OK && count == 0);  // no hit: nothing
  }

  // ---- the two entry points: every refusal comes before the mesh is followed or a device is touched
  int not_a_mesh[64] = {0};
  std::vector<dtp_ray> two(2);
  two[0] = {{0, 0, 1}, {0, 0, -1}};
  two[1] = {{0, 0, 1}, {0, 0, 0}};
  std::vector<dtp_mesh_hit> out(2);
  memset(out.data(), 0x5a, 2 * sizeof(dtp_mesh_hit));
  const std::vector<dtp_mesh_hit> before(out);
  int (*entries[2])(dtp_mesh*, const dtp_ray*, int, dtp_mesh_hit*, dtp_stream) = {dtp_mesh_pick, dtp_op_mesh_pick};
  for (auto fn : entries) {
    EXPECT(fn(nullptr, two.data(), 1, out.data(), nullptr) == DTP_ERR_ARG && strstr(g_err, "NULL"));
    EXPECT(fn((dtp_mesh*)not_a_mesh, nullptr, 1, out.data(), nullptr) == DTP_ERR_ARG && strstr(g_err, "NULL"));
    EXPECT(fn((dtp_mesh*)not_a_mesh, two.data(), 1, nullptr, nullptr) == DTP_ERR_ARG && strstr(g_err, "NULL"));
    EXPECT(fn((dtp_mesh*)not_a_mesh, two.data(), 0, out.data(), nullptr) == DTP_ERR_ARG && strstr(g_err, "n=0"));
    EXPECT(fn((dtp_mesh*)not_a_mesh, two.data(), PICK_MAX_RAYS + 1, out.data(), nullptr) == DTP_ERR_ARG && strstr(g_err, "n=4097"));
    EXPECT(fn((dtp_mesh*)not_a_mesh, two.data(), -3, out.data(), nullptr) == DTP_ERR_ARG);
    EXPECT(fn((dtp_mesh*)not_a_mesh, two.data(), 2, out.data(), nullptr) == DTP_ERR_ARG && strstr(g_err, "not a live mesh"));
    EXPECT(memcmp(out.data(), before.data(), 2 * sizeof(dtp_mesh_hit)) == 0);
  }
  printf("mesh_pick_host_check: %d checks passed\n", g_checks);
  return 0;
}
