// Stand-alone host check of csrc/mesh.hip and csrc/mesh_bleed.hip for a sanitizer build: the part of it that needs no device -- dtp_mesh_camera, the argument
// checks of dtp_mesh_create, dtp_mesh_destroy, dtp_mesh_stroke and the two ops, all of which return before their first HIP call, and
// the host side of the bleed pass (the offset table, the rectangle clipping of csrc/mesh_host.h, the argument checks), and of the
// occlusion test (the setting, the rounding of its tolerance, the refusals of the two occluded entry points) -- driven from its own main().  The rest of the library is replaced by the stubs below; none of them may be reached.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I diffusiontexturepainting_amd/csrc diffusiontexturepainting_amd/csrc/mesh.hip \
//         diffusiontexturepainting_amd/csrc/mesh_bleed.hip tools/mesh_host_check.cpp -o mesh_host_check
//   ./mesh_host_check
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mesh_host.h"
#include "stamp.h"

static char g_err[1024];
void dtp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" const char* dtp_last_error(void) { return g_err; }
static int unreachable(const char* what) { fprintf(stderr, "reached %s: a check let a bad call through\n", what); abort(); }
int stamp_plan(Ctx*, StampPlan&) { return unreachable("stamp_plan"); }
int stamp_enqueue(Ctx*, const StampPlan&, hipStream_t) { return unreachable("stamp_enqueue"); }
int ctx_persistent(Ctx*, size_t, void**, bool) { return unreachable("ctx_persistent"); }
int stroke_default_mask(Ctx*, int, hipStream_t, const unsigned char**) { return unreachable("stroke_default_mask"); }
Journal* journal_armed(Ctx*, const void*, int, int) { unreachable("journal_armed"); return nullptr; }
int journal_save_box(Journal*, const int*, int, hipStream_t) { return unreachable("journal_save_box"); }
void view_free(void*) {}  // (a mesh that never had a view holds nothing)

static int g_checks = 0;
#define EXPECT(cond)                                                                      \
  do {                                                                                    \
    ++g_checks;                                                                           \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_err); return 1; } \
  } while (0)

int main() {
  float out[12];
  const float pos[3] = {0.3f, -1.7f, 2.9f}, normal[3] = {0.2f, 0.5f, 0.84f}, prev[3] = {0.1f, -1.2f, 2.6f}, zero[3] = {0, 0, 0};
  EXPECT(dtp_mesh_camera(pos, normal, prev, 0.37f, out) == DTP_OK);
  for (int k = 0; k < 3; ++k) {  // orthonormal rows
    double n = 0;
    for (int i = 0; i < 3; ++i) n += (double)out[4 * k + i] * out[4 * k + i];
    EXPECT(fabs(n - 1.0) < 1e-6);
  }
  const float nanv[3] = {NAN, 0, 0}, p2[3] = {1.f, 2.f, 3.f}, n2[3] = {0.25f, 0.5f, 0.75f}, par[3] = {1.5f, 3.f, 4.5f}, huge[3] = {3e38f, 3e38f, 3e38f};
  EXPECT(dtp_mesh_camera(pos, zero, prev, 1.f, out) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_camera(pos, normal, pos, 1.f, out) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_camera(p2, n2, par, 1.f, out) == DTP_ERR_ARG);  // prev = pos + 2 normal, exactly
  EXPECT(dtp_mesh_camera(nanv, normal, prev, 1.f, out) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_camera(pos, normal, prev, 0.f, out) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_camera(pos, normal, prev, INFINITY, out) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_camera(huge, normal, prev, 1.f, out) == DTP_ERR_ARG || isfinite(out[3]));
  EXPECT(dtp_mesh_camera(nullptr, normal, prev, 1.f, out) == DTP_ERR_ARG);

  // dtp_mesh_create: every byte of the arrays is read before the refusal at the end (ctx NULL), at the exact sizes
  const int V = 1000, F = 1998;
  std::vector<float> verts(3 * V), uvs(6 * F);
  std::vector<int> faces(3 * F);
  for (int i = 0; i < 3 * V; ++i) verts[i] = (float)(i % 17) * 0.25f;
  for (int i = 0; i < 6 * F; ++i) uvs[i] = (float)(i % 11) / 11.f;
  for (int i = 0; i < 3 * F; ++i) faces[i] = i % V;
  dtp_mesh* mesh = nullptr;
  EXPECT(dtp_mesh_create(nullptr, verts.data(), V, faces.data(), F, uvs.data(), &mesh) == DTP_ERR_ARG && strstr(g_err, "ctx is NULL"));
  faces[3 * F - 1] = V;
  EXPECT(dtp_mesh_create(nullptr, verts.data(), V, faces.data(), F, uvs.data(), &mesh) == DTP_ERR_ARG && strstr(g_err, "face 1997"));
  faces[3 * F - 1] = 0;
  uvs[6 * F - 1] = NAN;
  EXPECT(dtp_mesh_create(nullptr, verts.data(), V, faces.data(), F, uvs.data(), &mesh) == DTP_ERR_ARG && strstr(g_err, "face 1997"));
  uvs[6 * F - 1] = 0.f;
  verts[3 * V - 1] = INFINITY;
  EXPECT(dtp_mesh_create(nullptr, verts.data(), V, faces.data(), F, uvs.data(), &mesh) == DTP_ERR_ARG && strstr(g_err, "vertex 999"));
  EXPECT(dtp_mesh_create(nullptr, verts.data(), 0, faces.data(), F, uvs.data(), &mesh) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_create(nullptr, verts.data(), V, faces.data(), (1 << 20) + 1, uvs.data(), &mesh) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_create(nullptr, nullptr, V, faces.data(), F, uvs.data(), &mesh) == DTP_ERR_ARG);
  EXPECT(mesh == nullptr);

  // handles that are not live meshes are refused without being followed
  int not_a_mesh[64] = {0};
  EXPECT(dtp_mesh_destroy(nullptr) == DTP_OK);
  EXPECT(dtp_mesh_destroy((dtp_mesh*)not_a_mesh) == DTP_ERR_ARG);
  float canvas[4];
  int face_idx[1];
  unsigned char tex[4], mask[1];
  EXPECT(dtp_op_mesh_render((dtp_mesh*)not_a_mesh, out, 1.f, 0, tex, 1, 1, 1, 0, 0, 0, canvas, face_idx, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_op_mesh_render(nullptr, out, 1.f, 0, tex, 1, 1, 1, 0, 0, 0, canvas, face_idx, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_op_mesh_backproject((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr) == DTP_ERR_ARG);
  dtp_settings st = {};
  dtp_mesh_stroke_opts o = {};
  dtp_mesh_stamp stamp = {};
  EXPECT(dtp_mesh_stroke(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, nullptr) == DTP_ERR_ARG);

  // ---- the bleed pass: the offset table at every radius into a buffer of exactly its size, against the definition
  std::vector<signed char> last;
  for (int k = 1; k <= 16; ++k) {
    int want = 0;
    for (int di = -k; di <= k; ++di)
      for (int dj = -k; dj <= k; ++dj) want += (di * di + dj * dj > 0 && di * di + dj * dj <= k * k);
    int count = -1;
    EXPECT(dtp_mesh_bleed_offsets(k, &count, nullptr) == DTP_OK && count == want);
    std::vector<signed char> d(2 * (size_t)count);
    EXPECT(dtp_mesh_bleed_offsets(k, &count, d.data()) == DTP_OK && count == want);
    for (int o = 0; o < count; ++o) {
      const int di = d[2 * o], dj = d[2 * o + 1], d2 = di * di + dj * dj;
      EXPECT(d2 > 0 && d2 <= k * k);
      if (o > 0) {  // the key (d2, di, dj) rises strictly
        const int pi = d[2 * o - 2], pj = d[2 * o - 1], p2 = pi * pi + pj * pj;
        EXPECT(p2 < d2 || (p2 == d2 && (pi < di || (pi == di && pj < dj))));
      }
    }
    EXPECT(last.size() <= d.size() && (last.empty() || memcmp(last.data(), d.data(), last.size()) == 0));  // a prefix of the next
    last = d;
  }
  EXPECT(last.size() == 2 * (size_t)MESH_MAX_OFF);
  EXPECT(last[0] == -1 && last[1] == 0 && last[2] == 0 && last[3] == -1 && last[4] == 0 && last[5] == 1 && last[6] == 1 && last[7] == 0);
  int count = -5;
  signed char one[2] = {9, 9};
  EXPECT(dtp_mesh_bleed_offsets(0, &count, one) == DTP_ERR_ARG && dtp_mesh_bleed_offsets(17, &count, one) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_bleed_offsets(-3, &count, one) == DTP_ERR_ARG && dtp_mesh_bleed_offsets(4, nullptr, one) == DTP_ERR_ARG);
  EXPECT(count == -5 && one[0] == 9 && one[1] == 9);

  // the rectangle of dtp_mesh_bleed
  int r[4];
  EXPECT(mesh_clip_rect(nullptr, 96, 160, r) == 0 && r[0] == 0 && r[1] == 0 && r[2] == 159 && r[3] == 95);
  const int inside[4] = {70, 30, 90, 47}, over[4] = {-7, -3, 11, 200}, right[4] = {160, 0, 300, 10}, above[4] = {0, -9, 10, -1};
  const int inverted_x[4] = {5, 0, 4, 9}, inverted_y[4] = {0, 9, 9, 8}, texel[4] = {159, 95, 159, 95};
  const int far[4] = {-2147483647 - 1, -2147483647 - 1, 2147483647, 2147483647};
  EXPECT(mesh_clip_rect(inside, 96, 160, r) == 0 && r[0] == 70 && r[1] == 30 && r[2] == 90 && r[3] == 47);
  EXPECT(mesh_clip_rect(over, 96, 160, r) == 0 && r[0] == 0 && r[1] == 0 && r[2] == 11 && r[3] == 95);
  EXPECT(mesh_clip_rect(right, 96, 160, r) == 1 && mesh_clip_rect(above, 96, 160, r) == 1);
  EXPECT(mesh_clip_rect(inverted_x, 96, 160, r) == -1 && mesh_clip_rect(inverted_y, 96, 160, r) == -1);
  EXPECT(mesh_clip_rect(texel, 96, 160, r) == 0 && r[0] == 159 && r[1] == 95 && r[2] == 159 && r[3] == 95);
  EXPECT(mesh_clip_rect(far, 1, 1, r) == 0 && r[0] == 0 && r[1] == 0 && r[2] == 0 && r[3] == 0);

  // the entry points: every refusal comes before the mesh is followed or a device is touched
  EXPECT(dtp_mesh_bleed(nullptr, tex, 1, 1, 1, nullptr, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, nullptr, 1, 1, 1, nullptr, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, tex, 1, 1, 17, nullptr, nullptr) == DTP_ERR_ARG && strstr(g_err, "bleed=17"));
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, tex, 1, 1, -1, nullptr, nullptr) == DTP_ERR_ARG && strstr(g_err, "bleed=-1"));
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, tex, 0, 1, 1, nullptr, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, tex, 1, 1, 1, inverted_x, nullptr) == DTP_ERR_ARG && strstr(g_err, "x0 > x1"));
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, tex, 1, 1, 1, nullptr, nullptr) == DTP_ERR_ARG && strstr(g_err, "not a live mesh"));
  EXPECT(dtp_mesh_bleed((dtp_mesh*)not_a_mesh, tex, 1, 1, 0, right, nullptr) == DTP_ERR_ARG && strstr(g_err, "not a live mesh"));
  EXPECT(dtp_op_mesh_coverage(nullptr, 1, 1, tex, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_op_mesh_coverage((dtp_mesh*)not_a_mesh, 1, 1, nullptr, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_op_mesh_coverage((dtp_mesh*)not_a_mesh, 1, 32769, tex, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_op_mesh_coverage((dtp_mesh*)not_a_mesh, 1, 1, tex, nullptr) == DTP_ERR_ARG && strstr(g_err, "not a live mesh"));
  EXPECT(dtp_mesh_stroke_bleed(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 17, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "dtp_mesh_stroke_bleed: bleed=17"));
  EXPECT(dtp_mesh_stroke_bleed(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, -1, nullptr) == DTP_ERR_ARG);
  EXPECT(dtp_mesh_stroke_bleed(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 2, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "NULL"));

  // ---- the occlusion test: the setting, the tolerance it becomes, and the refusals that come before everything else
  EXPECT(mesh_occlude_ok(0.f) && mesh_occlude_ok(1.f) && mesh_occlude_ok(3.4e38f) && mesh_occlude_ok(-0.f));
  EXPECT(!mesh_occlude_ok(-1e-30f) && !mesh_occlude_ok(NAN) && !mesh_occlude_ok(INFINITY) && !mesh_occlude_ok(-INFINITY));
  float tol = -7.f;
  EXPECT(mesh_occlude_tol(1.f, 1.f, 32, &tol) && tol == 0.0625f);
  EXPECT(mesh_occlude_tol(0.f, 3e38f, 1, &tol) && tol == 0.f);
  EXPECT(mesh_occlude_tol(0.25f, 0.45f, 64, &tol) && tol == (float)((0.25 * 2.0) * (double)0.45f / 64.0));
  // rounded ONCE: the product in double, not in float (0.1f * 2 * 0.3f / 7 rounds differently when each step is rounded to fp32)
  EXPECT(mesh_occlude_tol(0.1f, 0.3f, 7, &tol) && tol == (float)((((double)0.1f * 2.0) * (double)0.3f) / 7.0));
  EXPECT(mesh_occlude_tol(3e38f, 3e38f, 4096, &tol) == false && mesh_occlude_tol(3.4e38f, 1.f, 1, &tol) == false);  // (2 x 3.4e38: above fp32)
  EXPECT(tol == (float)((((double)0.1f * 2.0) * (double)0.3f) / 7.0));  // a refusal leaves *tol alone
  EXPECT(mesh_occlude_tol(3.4e38f, 1.f, 2, &tol) && tol == 3.4e38f);
  EXPECT(mesh_occlude_tol(1e-30f, 1e-30f, 4096, &tol) && tol == 0.f);  // an underflow is a tolerance of 0, not a refusal
  EXPECT(dtp_mesh_stroke_occluded(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 0, nullptr, 0, -1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "dtp_mesh_stroke_occluded: occlude=-1"));
  EXPECT(dtp_mesh_stroke_occluded(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 0, nullptr, 0, NAN, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "occlude=nan"));
  EXPECT(dtp_mesh_stroke_occluded(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 0, nullptr, 0, INFINITY, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "occlude=inf"));
  EXPECT(dtp_mesh_stroke_occluded(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 17, nullptr, 0, 1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "dtp_mesh_stroke_occluded: bleed=17"));
  EXPECT(dtp_mesh_stroke_occluded(nullptr, (dtp_mesh*)not_a_mesh, tex, 1, 1, &stamp, 1, &st, &o, nullptr, 2, nullptr, 0, 1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "NULL"));
  EXPECT(dtp_op_mesh_backproject_occluded((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr, 0, 1.f, -0.5f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "occlude=-0.5"));
  EXPECT(dtp_op_mesh_backproject_occluded((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr, 0, 0.f, 1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "fov=0"));
  EXPECT(dtp_op_mesh_backproject_occluded((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr, 0, NAN, 1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "fov=nan"));
  EXPECT(dtp_op_mesh_backproject_occluded((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 4097, tex, 1, 1, nullptr, 0, 1.f, 1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "R=4097"));
  EXPECT(dtp_op_mesh_backproject_occluded((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr, 0, 3e38f, 3e38f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "does not fit fp32"));
  EXPECT(dtp_op_mesh_backproject_occluded(nullptr, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr, 0, 1.f, 1.f, nullptr) == DTP_ERR_ARG && strstr(g_err, "NULL"));
  EXPECT(dtp_op_mesh_backproject_occluded((dtp_mesh*)not_a_mesh, nullptr, 0, mask, face_idx, 1, tex, 1, 1, nullptr, 0, 1.f, 1.f, nullptr) == DTP_ERR_ARG &&
         strstr(g_err, "not a live mesh"));
  printf("mesh_host_check: %d checks passed\n", g_checks);
  return 0;
}
