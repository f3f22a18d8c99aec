// Stand-alone host check of the view of a textured mesh (csrc/view_host.h) for a sanitizer build: everything of it that
// needs no device -- the perspective camera, the rays of its pixels, the argument checks of dtp_mesh_view that come before the mesh is
// looked up, and the bins a face's pixel range meets -- driven from its own main().  Build and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \
//       tools/view_host_check.cpp -o view_host_check && ./view_host_check
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "view_host.h"

static int g_checks = 0;
#define EXPECT(cond)                                                                 \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static bool has(const char* why, const char* word) { return why && strstr(why, word); }

int main() {
  // ---- the camera: an orthonormal frame, the eye at 0, `at` straight ahead; into a struct that the heap guards on both sides
  std::vector<dtp_view_cam> cams(1);
  dtp_view_cam& cam = cams[0];
  const float poses[][9] = {{0, 0, 3, 0, 0, 0, 0, 1, 0},       {2, -3, 1.5f, 0.25f, 0.5f, 0, 0, 0, 1}, {-1, 0.5f, -4, 0, 0, 0, 0.3f, 1, 0.2f},
                            {100.5f, 200, 50, 99, 198, 49, 0, 0, 5}, {0, 2, 0, 0, 0, 0, 1, 0, 0}};
  for (const auto& p : poses) {
    EXPECT(view_camera(p, p + 3, p + 6, 45.f, 720, 1280, 0.01f, &cam) == nullptr);
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) {
        double dot = 0;
        for (int i = 0; i < 3; ++i) dot += (double)cam.m[4 * k + i] * cam.m[4 * j + i];
        EXPECT(fabs(dot - (k == j ? 1.0 : 0.0)) < 1e-6);
      }
    double len = 0;
    for (int i = 0; i < 3; ++i) len += ((double)p[i] - p[3 + i]) * ((double)p[i] - p[3 + i]);
    len = sqrt(len);
    const double scale = fmax(1.0, fmax(fabs(p[0]), fmax(fabs(p[1]), fabs(p[2]))));
    for (int k = 0; k < 3; ++k) {
      double at_eye = cam.m[4 * k + 3], at_at = cam.m[4 * k + 3];
      for (int i = 0; i < 3; ++i) { at_eye += (double)cam.m[4 * k + i] * p[i]; at_at += (double)cam.m[4 * k + i] * p[3 + i]; }
      EXPECT(fabs(at_eye) < 4e-6 * scale && fabs(at_at - (k == 2 ? -len : 0.0)) < 4e-6 * scale);
    }
    EXPECT(fabs(cam.fy - 1.0 / tan(M_PI / 8)) < 1e-6 && fabs(cam.fx - cam.fy * 720.0 / 1280.0) < 1e-6 && cam.near == 0.01f);
  }
  const float eye[3] = {0, 0, 3}, at[3] = {0, 0, 0}, up[3] = {0, 1, 0}, zero[3] = {0, 0, 0}, along[3] = {0, 0, -2}, nanv[3] = {NAN, 0, 0};
  const float huge[3] = {3e38f, 3e38f, 3e38f};
  EXPECT(view_camera(eye, at, up, 90.f, 64, 64, 0.5f, &cam) == nullptr);
  const float want[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -3};
  for (int i = 0; i < 12; ++i) EXPECT(cam.m[i] == want[i]);
  EXPECT(fabs(cam.fx - 1.0) < 1e-7 && cam.fx == cam.fy);
  const dtp_view_cam keep = cam;
  EXPECT(has(view_camera(nanv, at, up, 45.f, 64, 64, 0.1f, &cam), "non-finite"));
  EXPECT(has(view_camera(eye, eye, up, 45.f, 64, 64, 0.1f, &cam), "eye == at"));
  EXPECT(has(view_camera(eye, at, zero, 45.f, 64, 64, 0.1f, &cam), "up is zero"));
  EXPECT(has(view_camera(eye, at, along, 45.f, 64, 64, 0.1f, &cam), "parallel"));
  const float fovs[] = {0.f, -1.f, 180.f, 200.f, NAN, INFINITY};
  for (float fov : fovs) EXPECT(has(view_camera(eye, at, up, fov, 64, 64, 0.1f, &cam), "fov_y"));
  const float nears[] = {0.f, -0.5f, NAN, INFINITY};
  for (float nr : nears) EXPECT(has(view_camera(eye, at, up, 45.f, 64, 64, nr, &cam), "near"));
  EXPECT(has(view_camera(eye, at, up, 45.f, 64, 64, 1e-45f, &cam), "fit fp32"));  // 1 / near is not finite
  EXPECT(has(view_camera(huge, at, up, 45.f, 64, 64, 0.1f, &cam), "fit fp32"));
  const int sides[][2] = {{0, 64}, {64, 0}, {4097, 64}, {64, 4097}, {-1, -1}};
  for (const auto& hw : sides) EXPECT(has(view_camera(eye, at, up, 45.f, hw[0], hw[1], 0.1f, &cam), "1..4096"));
  EXPECT(view_camera(eye, at, up, 45.f, 4096, 1, 0.1f, &cam) == nullptr && view_camera(eye, at, up, 179.99f, 1, 4096, 0.1f, &cam) == nullptr);
  cam = keep;
  EXPECT(has(view_camera(eye, eye, up, 45.f, 64, 64, 0.1f, &cam), "eye == at") && memcmp(&cam, &keep, sizeof cam) == 0);  // nothing written

  // ---- the rays, into an array of exactly n: the centre pixel looks down -b; the corners of the frame reach ndc = +-1
  {
    EXPECT(view_camera(eye, at, up, 90.f, 64, 128, 0.5f, &cam) == nullptr);
    const float px[] = {64, 32, 0, 0, 128, 64, 64.5f, 31.5f};
    std::vector<dtp_ray> out(4);
    int bad = 0;
    EXPECT(view_rays(&cam, 64, 128, px, 4, out.data(), &bad) == nullptr && bad == -1);
    for (int k = 0; k < 4; ++k) EXPECT(out[k].origin[0] == 0.f && out[k].origin[1] == 0.f && out[k].origin[2] == 3.f);
    EXPECT(out[0].dir[0] == 0.f && out[0].dir[1] == 0.f && out[0].dir[2] == -1.f);
    EXPECT(out[1].dir[0] == -2.f && out[1].dir[1] == 1.f && out[1].dir[2] == -1.f);  // fx = 0.5, fy = 1
    EXPECT(out[2].dir[0] == 2.f && out[2].dir[1] == -1.f && out[2].dir[2] == -1.f);
    EXPECT(out[3].dir[0] == 2.f * (1.f / 128.f) && out[3].dir[1] == 1.f / 64.f);
    const std::vector<dtp_ray> before(out);
    const float bad_px[] = {1, 2, 3, NAN, 5, 6, INFINITY, 8};
    EXPECT(has(view_rays(&cam, 64, 128, bad_px, 4, out.data(), &bad), "non-finite pixel") && bad == 1);
    EXPECT(has(view_rays(&cam, 64, 128, px, 0, out.data(), &bad), "at least 1") && has(view_rays(&cam, 64, 128, px, -5, out.data(), &bad), "at least 1"));
    EXPECT(has(view_rays(&cam, 0, 128, px, 4, out.data(), &bad), "1..4096"));
    dtp_view_cam broken = cam;
    broken.fx = 0.f;
    EXPECT(has(view_rays(&broken, 64, 128, px, 4, out.data(), &bad), "fx and fy"));
    broken = cam; broken.m[5] = NAN;
    EXPECT(has(view_rays(&broken, 64, 128, px, 4, out.data(), &bad), "matrix"));
    broken = cam; broken.near = 0.f;
    EXPECT(has(view_rays(&broken, 64, 128, px, 4, out.data(), &bad), "near"));
    broken = cam; broken.m[3] = broken.m[7] = broken.m[11] = 3e38f; broken.m[0] = broken.m[4] = broken.m[8] = 1.f;
    EXPECT(has(view_rays(&broken, 64, 128, px, 4, out.data(), &bad), "eye does not fit"));
    EXPECT(memcmp(out.data(), before.data(), 4 * sizeof(dtp_ray)) == 0);  // a refused call writes nothing
    std::vector<dtp_ray> one(1);
    EXPECT(view_rays(&cam, 64, 128, px + 6, 1, one.data(), &bad) == nullptr && one[0].dir[2] == -1.f);
  }

  // ---- the argument checks of a view
  {
    EXPECT(view_camera(eye, at, up, 45.f, 720, 1280, 0.01f, &cam) == nullptr);
    alignas(16) static unsigned char tex[64], img[64];
    static int fidx[4];
    static float dep[4];
    dtp_view_opts o = {0, 0, 1, 0.25f, {128, 128, 128}, {0, 0, 0, 0}};
    EXPECT(view_check(tex, 4, 4, &cam, 2, 2, &o, img, fidx, dep) == nullptr && view_check(tex, 4, 4, &cam, 2, 2, &o, img, nullptr, nullptr) == nullptr);
    EXPECT(has(view_check(nullptr, 4, 4, &cam, 2, 2, &o, img, fidx, dep), "NULL") && has(view_check(tex, 4, 4, nullptr, 2, 2, &o, img, fidx, dep), "NULL"));
    EXPECT(has(view_check(tex, 4, 4, &cam, 2, 2, nullptr, img, fidx, dep), "NULL") && has(view_check(tex, 4, 4, &cam, 2, 2, &o, nullptr, fidx, dep), "NULL"));
    EXPECT(has(view_check(tex, 4, 4, &cam, 0, 2, &o, img, fidx, dep), "1..4096") && has(view_check(tex, 4, 4, &cam, 2, 4097, &o, img, fidx, dep), "1..4096"));
    EXPECT(has(view_check(tex, 0, 4, &cam, 2, 2, &o, img, fidx, dep), "1..32768") && has(view_check(tex, 4, 32769, &cam, 2, 2, &o, img, fidx, dep), "1..32768"));
    EXPECT(has(view_check(tex + 1, 4, 4, &cam, 2, 2, &o, img, fidx, dep), "aligned") && has(view_check(tex, 4, 4, &cam, 2, 2, &o, img + 2, fidx, dep), "aligned"));
    EXPECT(has(view_check(tex, 4, 4, &cam, 2, 2, &o, img, (char*)fidx + 1, dep), "aligned") && has(view_check(tex, 4, 4, &cam, 2, 2, &o, img, fidx, (char*)dep + 3), "aligned"));
    dtp_view_cam broken = cam;
    broken.fy = -1.f;
    EXPECT(has(view_check(tex, 4, 4, &broken, 2, 2, &o, img, fidx, dep), "fx and fy"));
    dtp_view_opts b = o;
    b.cull = 2;
    EXPECT(has(view_check(tex, 4, 4, &cam, 2, 2, &b, img, fidx, dep), "0 or 1"));
    b = o; b.flip_normals = -1;
    EXPECT(has(view_check(tex, 4, 4, &cam, 2, 2, &b, img, fidx, dep), "0 or 1"));
    b = o; b.shade = 7;
    EXPECT(has(view_check(tex, 4, 4, &cam, 2, 2, &b, img, fidx, dep), "0 or 1"));
    const float ambients[] = {-0.1f, 1.5f, NAN, INFINITY};
    for (float a : ambients) { b = o; b.ambient = a; EXPECT(has(view_check(tex, 4, 4, &cam, 2, 2, &b, img, fidx, dep), "ambient")); }
    b = o; b.ambient = 0.f;
    EXPECT(view_check(tex, 4, 4, &cam, 2, 2, &b, img, fidx, dep) == nullptr);
    b.ambient = 1.f;
    EXPECT(view_check(tex, 4, 4, &cam, 2, 2, &b, img, fidx, dep) == nullptr);
  }

  // ---- the bins of a pixel range: every bin index stays inside the grid of the frame, a small face meets at most 2 x 2
  {
    int bx0, bx1, by0, by1;
    EXPECT(view_bins(0 | (63 << 16), 0 | (63 << 16), bx0, bx1, by0, by1) && bx0 == 0 && bx1 == 0 && by0 == 0 && by1 == 0);
    EXPECT(view_bins(63 | (64 << 16), 127 | (128 << 16), bx0, bx1, by0, by1) && bx0 == 0 && bx1 == 1 && by0 == 1 && by1 == 2);
    EXPECT(!view_bins(63 | (128 << 16), 5 | (5 << 16), bx0, bx1, by0, by1) && bx1 == 2);
    EXPECT(!view_bins(5 | (5 << 16), 0 | (4095 << 16), bx0, bx1, by0, by1) && by0 == 0 && by1 == 63);
    EXPECT(view_bins(4095 | (4095 << 16), 4032 | (4095 << 16), bx0, bx1, by0, by1) && bx0 == 63 && bx1 == 63 && by0 == 63 && by1 == 63);
    EXPECT(view_bins_across(1) == 1 && view_bins_across(64) == 1 && view_bins_across(65) == 2 && view_bins_across(4096) == 64);
    EXPECT(view_bins_across(VIEW_MAX) * view_bins_across(VIEW_MAX) == VIEW_MAX_BINS);
    const int sizes[] = {1, 24, 64, 136, 200, 4096};
    for (int H : sizes)
      for (int W : sizes) {
        const int nbx = view_bins_across(W), nby = view_bins_across(H);
        for (int x0 = 0; x0 < W; x0 += (W > 256 ? 61 : 7))
          for (int x1 = x0; x1 < W; x1 += (W > 256 ? 977 : 13))
            for (int y0 = 0; y0 < H; y0 += (H > 256 ? 1021 : 11)) {
              const int y1 = H - 1;
              const bool small = view_bins(x0 | (x1 << 16), y0 | (y1 << 16), bx0, bx1, by0, by1);
              EXPECT(0 <= bx0 && bx0 <= bx1 && bx1 < nbx && 0 <= by0 && by0 <= by1 && by1 < nby && by1 * nbx + bx1 < VIEW_MAX_BINS);
              EXPECT(small == ((bx1 - bx0 + 1) * (by1 - by0 + 1) <= 4 && bx1 - bx0 <= 1 && by1 - by0 <= 1));
              EXPECT(bx0 * VIEW_BIN <= x0 && x1 < (bx1 + 1) * VIEW_BIN && by0 * VIEW_BIN <= y0 && y1 < (by1 + 1) * VIEW_BIN);
            }
      }
  }
  printf("view_host_check: %d checks passed\n", g_checks);
  return 0;
}
