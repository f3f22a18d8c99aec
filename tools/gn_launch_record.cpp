// Host-only record of what the GroupNorm launchers of csrc/norm.hip do, for a cmp of two trees (a change of the launchers' host code must
// leave it alone): norm.hip is included with hipLaunchKernelGGL replaced by a recorder, so no kernel runs and no GPU is needed.  Per call
// it writes the return code, whether an error was set, and per launch the kernel, grid, block and every argument -- over groups x channel
// counts x map sizes x batches x pitches x every launcher and its options, then the claim predicate of Builder::claim_reduce.
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -DGN_NORM_HIP='"<tree>/diffusiontexturepainting_amd/csrc/norm.hip"' \
//         -I<tree>/diffusiontexturepainting_amd/csrc tools/gn_launch_record.cpp -o rec && ./rec out.txt       (once per tree; cmp the two files)
// -DGN_POSITIONAL_API: the tree is older than GnParams (positional launcher arguments, the claim rule written out in builder.hip).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <type_traits>
#include <string>
static FILE* OUT;
template <class T> static void pr(const T& v) {
  if constexpr (std::is_pointer<T>::value) fprintf(OUT, " p%lx", (unsigned long)(uintptr_t)v);
  else if constexpr (std::is_floating_point<T>::value) fprintf(OUT, " %a", (double)v);
  else fprintf(OUT, " %lld", (long long)v);
}
template <class K, class... A> static void record(const char* name, K, dim3 g, dim3 b, int shm, hipStream_t, A... a) {
  fprintf(OUT, "  L %s g%u,%u,%u b%u,%u,%u", name, g.x, g.y, g.z, b.x, b.y, b.z);
  (pr(a), ...);
  fprintf(OUT, "\n");
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, shm, s, ...) record(#k, k, g, b, shm, s, __VA_ARGS__)
#define hipGetLastError() hipSuccess
#include GN_NORM_HIP
void dtp_set_error(const char* fmt, ...) { fprintf(OUT, "  E\n"); }

#define P(n) ((const float*)(uintptr_t)(0x1000 * n))
static const f16* X = (const f16*)0x100000; static f16* Y = (f16*)0x200000; static float* WS = (float*)0x300000;
static const f16* R = (const f16*)0x400000;
#ifndef GN_POSITIONAL_API
static GnParams gp(int ldx, int ldy, int B, int HW, int C, int g, float eps, int silu) { return {X, ldx, Y, ldy, P(1), P(2), B, HW, C, g, eps, silu}; }
#endif
int main(int, char** argv) {
  OUT = fopen(argv[1], "w");
  const int Gs[] = {1, 7, 8, 9, 16, 32, 33, 64, 65};
  const int Cs[] = {8, 16, 32, 36, 48, 64, 96, 128, 130, 256, 320, 512, 520, 640, 960, 1280, 1920, 2048, 2056, 2560, 4096, 8192, 8320, 8448, 16384};
  const int HWs[] = {1, 4, 16, 31, 32, 64, 100, 255, 256, 257, 1000, 1024, 1600, 4096, 16384};
  const int Bs[] = {1, 3, 300};
  const float eps = 1e-5f;
  for (int g : Gs) for (int C : Cs) for (int HW : HWs) for (int B : Bs) {
    fprintf(OUT, "g=%d C=%d HW=%d B=%d sup=%d ws=%zu ch=%d\n", g, C, HW, B, (int)dtp_reduce_groupnorm_supported(HW, C, g), dtp_groupnorm_ws_bytes(B, HW, C, g), dtp_groupnorm_stat_chunks(HW));
    for (int dx : {0, 4, 8}) for (int dy : {0, 4, 8}) {
      const int ldx = C + dx, ldy = C + dy, silu = (dx + dy) & 8 ? 1 : 0;
      int rc;
#ifndef GN_POSITIONAL_API
      rc = dtp_launch_groupnorm(gp(ldx, ldy, B, HW, C, g, eps, silu), WS, 0);
#else
      rc = dtp_launch_groupnorm(X, ldx, Y, ldy, P(1), P(2), WS, B, HW, C, g, eps, silu, 0);
#endif
      fprintf(OUT, " gn %d %d rc=%d\n", dx, dy, rc);
      for (int nchunk : {0, 1, 5}) {
#ifndef GN_POSITIONAL_API
        rc = dtp_launch_groupnorm_apply(gp(ldx, ldy, B, HW, C, g, eps, silu), P(3), nchunk, 0);
#else
        rc = dtp_launch_groupnorm_apply(X, ldx, Y, ldy, P(1), P(2), P(3), nchunk, B, HW, C, g, eps, silu, 0);
#endif
        fprintf(OUT, " ap %d rc=%d\n", nchunk, rc);
      }
      for (int dp : {0, 2, 4}) for (int dr : {-1, 0, 4}) for (int Cx : {0, C, C / 2, C - 4}) for (int ws : {0, 1}) {
        const int ldp = (Cx > 0 ? Cx : C) + dp;
        const GnReduceSrc rd = {P(4), 3, 12345, ldp, P(5), dr < 0 ? nullptr : R, C + (dr < 0 ? 3 : dr)};
#ifndef GN_POSITIONAL_API
        rc = dtp_launch_reduce_groupnorm(gp(ldx, ldy, B, HW, C, g, eps, silu), rd, Cx, ws ? WS : nullptr, 0);
#else
        rc = dtp_launch_reduce_groupnorm(rd.part, rd.splits, rd.slab, rd.ldp, rd.bias, rd.R, rd.ldr, (f16*)X, ldx, Y, ldy, P(1), P(2), B, HW, C, g, eps, silu, ws ? WS : nullptr, 0, Cx);
#endif
        fprintf(OUT, " rg %d %d %d %d rc=%d\n", dp, dr, Cx, ws, rc);
      }
      if (dy) continue;
      for (int dp : {-1, 0, 2, 4}) for (int dr : {-1, 0, 4}) {
        const GnReduceSrc rd = {P(4), 3, 12345, C + dp, P(5), dr < 0 ? nullptr : R, C + (dr < 0 ? 3 : dr)};
#ifndef GN_POSITIONAL_API
        rc = dtp_launch_groupnorm_stats(gp(ldx, 0, B, HW, C, g, eps, 0), WS, dp < 0 ? nullptr : &rd, 0);
#else
        rc = dtp_launch_groupnorm_stats(X, ldx, WS, B, HW, C, g, dp < 0 ? nullptr : &rd, 0);
#endif
        fprintf(OUT, " st %d %d rc=%d\n", dp, dr, rc);
      }
      for (int nchunk : {0, 3}) for (int Nout : {320, 5}) {
#ifndef GN_POSITIONAL_API
        rc = dtp_launch_gn_fold_weights(gp(0, 0, B, HW, C, g, eps, 0), P(3), nchunk, X, ldx, P(6), Nout, Y, 777, (float*)P(7), 128, 0);
#else
        rc = dtp_launch_gn_fold_weights(X, ldx, P(6), P(1), P(2), P(3), B, HW, C, Nout, g, eps, Y, 777, (float*)P(7), 128, 0, nchunk);
#endif
        fprintf(OUT, " fw %d %d rc=%d\n", nchunk, Nout, rc);
      }
    }
  }
  // the claim predicate of Builder::claim_reduce (32 groups; the caller has checked C % 8 == 0)
  for (int C = 8; C <= 20000; C += 8) for (int N : {C, C / 2, C - 2, C - 4}) for (int ld : {C, C + 4}) for (int ldr : {0, C, C + 4}) {
    bool ok;
#ifndef GN_POSITIONAL_API
    ok = dtp_groupnorm_reduce_accepts(C, 32, ld, N, ldr);
#else
    const int cpg = C / 32;
    ok = !((C % 32) || cpg < 4 || (cpg < 8 && cpg != 4) || (N & 3) || C / 8 > 1024 || (ld & 7) || (ldr && (ldr & 7)));
#endif
    fprintf(OUT, "claim %d %d %d %d %d\n", C, N, ld, ldr, (int)ok);
  }
  fclose(OUT);
}
