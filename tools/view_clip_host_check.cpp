// Stand-alone host check of the pixel range of a face that crosses the near plane (view_clip_box, csrc/view_host.h) for a
// sanitizer build.  The view rasterises such a face in homogeneous form and uses the range for the reject and the bins alone, so the range
// only has to be conservative: over random crossing faces and cameras -- vertices on the eye plane, exactly on the near plane, behind the
// eye, coordinates from 1e-3 to 3e38 -- no pixel centre that the face covers, computed here in double from the contract of include/dtp.h
// ("a view clipped at the near plane"), lies outside the box, and the box lies inside the frame.  Build and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \
//       tools/view_clip_host_check.cpp -o view_clip_host_check && ./view_clip_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "view_host.h"

static int g_checks = 0;
#define EXPECT(cond)                                                                 \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (case %d)\n", __FILE__, __LINE__, #cond, g_case); return 1; } \
  } while (0)

static int g_case = -1;
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // [0, 1)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}
static float between(double lo, double hi) { return (float)(lo + (hi - lo) * uniform()); }

// does the crossing face cover the centre of pixel (i, j)?  The contract's per-pixel rule, in double.
static bool covers(const float c[3][3], double fx, double fy, double near, int H, int W, int i, int j) {
  double n[3][3];
  for (int k = 0; k < 3; ++k) {
    const float* a = c[(k + 1) % 3];
    const float* b = c[(k + 2) % 3];
    n[k][0] = (double)a[1] * b[2] - (double)a[2] * b[1];
    n[k][1] = (double)a[2] * b[0] - (double)a[0] * b[2];
    n[k][2] = (double)a[0] * b[1] - (double)a[1] * b[0];
  }
  const double D = (c[0][0] * n[0][0] + c[0][1] * n[0][1]) + c[0][2] * n[0][2];
  if (D == 0.0 || !std::isfinite(D)) return false;
  const double s = D < 0 ? -1.0 : 1.0;
  const double gx = ((2.0 * j + 1.0) / W - 1.0) / fx, gy = (1.0 - (2.0 * i + 1.0) / H) / fy;
  double sum = 0;
  for (int k = 0; k < 3; ++k) {
    const double E = s * ((n[k][0] * gx + n[k][1] * gy) - n[k][2]);
    if (!(E >= 0)) return false;
    sum += E;
  }
  const double d = sum / fabs(D);
  return std::isfinite(d) && d > 0 && 1.0 / d >= near;
}

int main() {
  const int frames[][2] = {{36, 64}, {9, 9}, {1, 1}, {24, 200}, {136, 40}, {3, 4096}};
  const double scales[] = {1e-3, 1.0, 1.0, 1.0, 30.0, 1e4, 1e12, 1e30, 3e38};
  long covered_total = 0, whole = 0, empty = 0;
  for (g_case = 0; g_case < 6000; ++g_case) {
    const int H = frames[g_case % 6][0], W = frames[g_case % 6][1];
    const float near = (float)pow(10.0, -3.0 + 3.0 * uniform());
    const float fy = (float)(1.0 / tan((5.0 + 150.0 * uniform()) * M_PI / 360.0)), fx = fy * (float)H / (float)W;
    const double sc = scales[(g_case / 6) % 9];
    std::vector<float> heap(9);  // (the heap guards both ends of what the helper reads)
    float(*c)[3] = (float(*)[3])heap.data();
    for (int k = 0; k < 3; ++k) {
      c[k][0] = between(-sc, sc); c[k][1] = between(-sc, sc); c[k][2] = between(-sc, sc * 0.25);
    }
    // special vertices: on the eye plane, exactly on the near plane, just nearer than it, far behind the eye
    const int special = (g_case / 54) % 6;
    if (special == 1) c[1][2] = 0.f;
    if (special == 2) c[2][2] = -near;
    if (special == 3) c[0][2] = nextafterf(-near, 0.f);
    if (special == 4) { c[0][2] = (float)sc; c[1][2] = (float)sc * 2.f; }
    if (special == 5) { c[1][0] = 0.f; c[1][1] = 0.f; }  // (a vertex on the view axis)
    int ahead = 0;
    for (int k = 0; k < 3; ++k) ahead += c[k][2] <= -near;
    if (ahead == 0) { c[0][2] = -near - (float)fabs(between(0, sc)); ahead = 1; }  // make it cross
    if (ahead == 3) c[2][2] = between(0, sc);
    ahead = 0;
    for (int k = 0; k < 3; ++k) ahead += c[k][2] <= -near;
    EXPECT(ahead > 0 && ahead < 3);
    int x0 = -7, x1 = -7, y0 = -7, y1 = -7;
    const bool any = view_clip_box(c, fx, fy, near, H, W, x0, x1, y0, y1);
    if (any) {
      EXPECT(0 <= x0 && x0 <= x1 && x1 < W && 0 <= y0 && y0 <= y1 && y1 < H);
      whole += x0 == 0 && y0 == 0 && x1 == W - 1 && y1 == H - 1;
    } else {
      EXPECT(x0 == -7 && x1 == -7 && y0 == -7 && y1 == -7);  // nothing written
      ++empty;
    }
    const int step = W > 1024 ? 3 : 1;
    for (int i = 0; i < H; ++i)
      for (int j = (i * 7) % step; j < W; j += step) {
        if (any && x0 <= j && j <= x1 && y0 <= i && i <= y1) continue;
        if (covers(c, fx, fy, near, H, W, i, j)) {
          fprintf(stderr, "case %d: pixel (%d, %d) of %d x %d is covered outside the box [%d, %d] x [%d, %d] (drawn %d)\n", g_case, i, j, H, W, x0, x1, y0,
                  y1, (int)any);
          return 1;
        }
        ++g_checks;
      }
    if (any)
      for (int i = y0; i <= y1; ++i)
        for (int j = x0; j <= x1; j += step) covered_total += covers(c, fx, fy, near, H, W, i, j);
  }
  // the scenes of the tests by hand: a floor under the eye covers the rows below the horizon, and its box says so
  {
    g_case = -2;
    const float floor_c[3][3] = {{-10.f, -1.f, -10.f}, {10.f, -1.f, 10.f}, {10.f, -1.f, -10.f}};
    int x0, x1, y0, y1;
    EXPECT(view_clip_box(floor_c, 1.f, 1.f, 0.01f, 36, 64, x0, x1, y0, y1));
    EXPECT(x0 == 0 && x1 == 63 && y1 == 35 && y0 <= 18 && y0 >= 14);
    const float nan_c[3][3] = {{NAN, 0.f, -1.f}, {1.f, 0.f, 1.f}, {0.f, 1.f, -1.f}};
    EXPECT(view_clip_box(nan_c, 1.f, 1.f, 0.01f, 36, 64, x0, x1, y0, y1) && x0 == 0 && x1 == 63 && y0 == 0 && y1 == 35);  // the whole frame
    const float off_c[3][3] = {{50.f, 0.f, -1.f}, {60.f, 0.f, 1.f}, {55.f, 1.f, -1.f}};
    EXPECT(!view_clip_box(off_c, 1.f, 1.f, 0.01f, 36, 64, x0, x1, y0, y1));  // far to the right of the frame
  }
  EXPECT(covered_total > 20000 && whole > 100 && empty > 100);  // the cases are not all trivial
  printf("view_clip_host_check: %d checks passed (%ld covered centres inside their boxes, %ld whole-frame boxes, %ld empty)\n", g_checks,
         covered_total, whole, empty);
  return 0;
}
