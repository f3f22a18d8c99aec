// Shared device/host declarations for the gfx950 (MI355X, CDNA4) kernels of libdtp.
// Wave = 64 lanes everywhere in this code base; activations are NHWC fp16
// ("tokens x channels", row stride `ld` in elements), accumulation is fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dtp.h"

typedef _Float16 f16;
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- hand-scheduled LDS fragment reads (GEMM-style kernels).  With global_load_lds in a loop the compiler treats every
// LDS-DMA as a possible out-of-order LGKM event and only ever emits s_waitcnt lgkmcnt(0); these untracked reads plus
// hand-counted waits let the MFMAs of k-step s run while the reads of steps s+1.. are still in flight.
// LDS byte address of a pointer into the dynamic shared segment
static __device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
// ds_read_b128 the compiler does not track: pair every use with wait_lds_frags<>
static __device__ __forceinline__ f16x8 lds_read16(uint32_t addr) {
  f16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
// s_waitcnt lgkmcnt(N) that the NF fragments "pass through", so their consumers cannot be scheduled above the wait
template <int N, int NF>
static __device__ __forceinline__ void wait_lds_frags(f16x8 (&f)[NF]) {
  static_assert(NF == 2 || NF == 3 || NF == 4 || NF == 5 || NF == 6 || NF == 7 || NF == 8, "fragment count");
  if constexpr (NF == 2) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(f[0]), "+v"(f[1]) : "n"(N));
  else if constexpr (NF == 3) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]) : "n"(N));
  else if constexpr (NF == 4) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) : "n"(N));
  else if constexpr (NF == 5)
    asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]) : "n"(N));
  else if constexpr (NF == 6)
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]) : "n"(N));
  else if constexpr (NF == 7)
    asm volatile("s_waitcnt lgkmcnt(%7)"
                 : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6])
                 : "n"(N));
  else
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7])
                 : "n"(N));
}



// 1 / x by v_rcp_f32 alone (1 ulp).  `1.0f / x` and __frcp_rn are the correctly rounded division: v_div_scale x 2, v_rcp, four FMAs,
// v_div_fmas, v_div_fixup -- ten VALU instructions per element, a third of the GEGLU epilogue of lnlin_kernel before round 5 noticed.
#ifndef DTP_IEEE_DIV
static __device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#else  // (A/B builds only: tools/ab_build.sh)
static __device__ __forceinline__ float fast_rcp(float x) { return 1.0f / x; }
#endif
// x * sigmoid(x) (x -> -inf: exp overflows to inf, rcp gives 0, the product -0 like the division's)
static __device__ __forceinline__ float silu_f(float x) { return x * fast_rcp(1.0f + __expf(-x)); }
static __device__ __forceinline__ float quick_gelu_f(float x) { return x * fast_rcp(1.0f + __expf(-1.702f * x)); }

// exact (erf) GELU.  erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far below the fp16 output): one v_rcp, one v_exp and
// a degree-5 Horner chain instead of the ~3x longer libm erff, which showed up in the GEGLU epilogues (2.6 G evaluations / stamp)
#ifndef DTP_GELU_POLY
static __device__ __forceinline__ float gelu_erf(float x) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = fast_rcp(fmaf(0.3275911f, z, 1.0f));
  float pl = fmaf(1.061405429f, t, -1.453152027f);
  pl = fmaf(pl, t, 1.421413741f);
  pl = fmaf(pl, t, -0.284496736f);
  pl = fmaf(pl, t, 0.254829592f);
  const float e = 1.0f - pl * t * __expf(-z * z);  // erf(|x| / sqrt 2)
  return 0.5f * x * (1.0f + copysignf(e, x));
}
#else
// (A/B builds only: tools/ab_build.sh gelu_poly -DDTP_GELU_POLY.)  erf(z) = z P(z^2) on [0, 3], degree 8 in z^2 (minimax fit, |error| <=
// 1.7e-5; z clamped at 3): no transcendental, 215 instead of 255 VALU instructions per lnlin chunk -- measured round 5: the GEGLU
// launches -1 ... -3 %, the stamp within noise (profiles/r05_lnlin_ablation.txt); not worth 5e-5 of absolute error, not shipped.
static __device__ __forceinline__ float gelu_erf(float x) {
  const float z = fminf(fabsf(x) * 0.70710678118654752f, 3.0f);
  const float u = z * z;
  float p = fmaf(4.074155537e-08f, u, -1.944803169e-06f);
  p = fmaf(p, u, 4.106023957e-05f);
  p = fmaf(p, u, -5.110346811e-04f);
  p = fmaf(p, u, 4.235417930e-03f);
  p = fmaf(p, u, -2.510283806e-02f);
  p = fmaf(p, u, 1.110793054e-01f);
  p = fmaf(p, u, -3.753148582e-01f);
  p = fmaf(p, u, 1.128268424e+00f);
  const float h = 0.5f * x;
  return fmaf(fabsf(h), p * z, h);  // 0.5 x (1 + sign(x) erf(|x| / sqrt 2))
}
#endif

// Sum n (value, value) pairs spaced `stride` floats apart, IN ORDER, with the loads issued eight at a time before their additions.
// A `for (q) s += p[q * stride]` loop chains one memory round trip per term (hipcc does not pipeline a runtime trip count): with
// 5-20 partial sums per row that chain was microseconds of pure latency in front of every LayerNorm-folded GEMM and GroupNorm apply.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <class T>  // T = the accumulator type
static __device__ __forceinline__ void sum_pairs_strided_t(const float* __restrict__ p, size_t stride, int n, T& s1, T& s2) {
  s1 = 0; s2 = 0;
  int q = 0;
  for (; q + 8 <= n; q += 8) {
    f32x2 t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = *(const f32x2*)(p + (size_t)(q + e) * stride);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1 += (T)t[e][0]; s2 += (T)t[e][1]; }
  }
  if (q < n) {
    f32x2 t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = *(const f32x2*)(p + (size_t)(q + (q + e < n ? e : 0)) * stride);  // clamped: always a valid address
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (q + e < n) { s1 += (T)t[e][0]; s2 += (T)t[e][1]; }
  }
}
static __device__ __forceinline__ void sum_pairs_strided(const float* __restrict__ p, size_t stride, int n, float& s1, float& s2) {
  sum_pairs_strided_t(p, stride, n, s1, s2);
}
// The same walk with the partial sums added in DOUBLE (round 6, GroupNorm statistics): every partial is an accurately rounded fp32
// (sum, sum of squares) of one chunk; their total and the final E[x^2] - mean^2 are formed in fp64, so the variance of a group whose
// mean is hundreds of standard deviations away from zero does not drown in the rounding of fp32 sums (tests/test_gpu_ops.py
// test_groupnorm_large_group_means; fp64 adds run at the fp32 rate on this chip and there are <= 16 per lane).
static __device__ __forceinline__ void sum_pairs_strided_d(const float* __restrict__ p, size_t stride, int n, double& s1, double& s2) {
  sum_pairs_strided_t(p, stride, n, s1, s2);
}
// LayerNorm fold, the mean term: out = rstd * (x W^T - mean * lns) + bias.  The kernels that stage their accumulators through an fp16
// tile (gemm_kernel, gemm_wide, xattn) subtract mean * lns from the fp32 accumulator BEFORE that rounding and multiply by rstd behind it:
// rounded first, the two terms of a row whose mean is not small against its sigma cancel only to 2^-11 of |x W^T|, and rstd (up to
// eps^-1/2 = 1000 on a constant row) multiplies what is left -- 1.1 at eps = 1e-5, 3.5 at 1e-6 on a constant -3 row
// (tests/test_gpu_norm_eps.py).  col4: four per-column fp32 values (weight row sums, biases) of columns n .. n + 3 (n % 4 == 0), zeros beyond N.
static __device__ __forceinline__ f32x4 col4(const float* __restrict__ v, int n, int N) {
  if (n + 4 <= N) return *(const f32x4*)(v + n);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (n + e < N) r[e] = v[n + e];
  return r;
}
static __device__ __forceinline__ double shfl_xor_d(double v, int o) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, o); hi = __shfl_xor(hi, o);
  return __hiloint2double(hi, lo);
}
// ---- all-reduce over aligned groups of W lanes WITHOUT the LDS: __shfl_xor compiles to ds_bpermute_b32 (an LDS round trip per level, and it
// enters the hand-counted lgkmcnt of the kernels that issue their fragment reads by hand); these are VALU moves.  Levels 1 and 2: DPP quad_perm;
// 4 and 8: row_half_mirror / row_mirror (every lane of a quad / half row holds the same partial by then, so "the mirrored lane" is a lane of the
// other quad / half: the same pairs, in the same order, as the xor butterfly taken from the small offsets up); 16 and 32: v_permlane16_swap /
// v_permlane32_swap of gfx950 (inline asm: this hipcc's builtins return their first result twice, attn_dma.hip).  All lanes of the group must be
// active.  Bit-identical to the ASCENDING butterfly `for (o = 1; o < W; o <<= 1) v = op(v, __shfl_xor(v, o))` -- which is NOT the order of the
// descending loops (o = W / 2 down to 1) it replaced in most kernels: a sum's last bits depend on the order, and every kernel's order is part
// of its output bytes (gemm_fp8 / gemm_f8f8 still reduce their row statistics from W / 2 down: rowstats_emit, tile_epilogue.h).
template <int CTRL>
static __device__ __forceinline__ float dpp_get_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
static __device__ __forceinline__ void swap16_f(float x, float& a, float& b) {  // a + b = x + x of the lane 16 away (xor 16)
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
static __device__ __forceinline__ void swap32_f(float x, float& a, float& b) {  // a = x of lane (l & 31), b = x of lane (l & 31) + 32
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
template <int W>
static __device__ __forceinline__ float group_allsum(float v) {
  static_assert(W == 2 || W == 4 || W == 8 || W == 16 || W == 32 || W == 64, "group width");
  v += dpp_get_f<0xb1>(v);
  if constexpr (W >= 4) v += dpp_get_f<0x4e>(v);
  if constexpr (W >= 8) v += dpp_get_f<0x141>(v);
  if constexpr (W >= 16) v += dpp_get_f<0x140>(v);
  if constexpr (W >= 32) { float a, b; swap16_f(v, a, b); v = a + b; }
  if constexpr (W >= 64) { float a, b; swap32_f(v, a, b); v = a + b; }
  return v;
}
template <int W>
static __device__ __forceinline__ float group_allmax(float v) {
  static_assert(W == 2 || W == 4 || W == 8 || W == 16, "group width");
  v = fmaxf(v, dpp_get_f<0xb1>(v));
  if constexpr (W >= 4) v = fmaxf(v, dpp_get_f<0x4e>(v));
  if constexpr (W >= 8) v = fmaxf(v, dpp_get_f<0x141>(v));
  if constexpr (W >= 16) v = fmaxf(v, dpp_get_f<0x140>(v));
  return v;
}
static __device__ __forceinline__ float xhalf_sum(float v) { float a, b; swap32_f(v, a, b); return a + b; }   // v + v of lane ^ 32
static __device__ __forceinline__ float xhalf_max(float v) { float a, b; swap32_f(v, a, b); return fmaxf(a, b); }

// fp64 sum over aligned groups of 8 lanes, result in all 8 -- three DPP steps (quad_perm xor 1, xor 2, row_half_mirror) instead of three
// ds_bpermute round trips per word
template <int CTRL>
static __device__ __forceinline__ double dpp_add8_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
static __device__ __forceinline__ double sum8_d(double v) {
  v = dpp_add8_d<0xb1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add8_d<0x4e>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_add8_d<0x141>(v);  // row_half_mirror: lane i <- lane 7 - i of its half row (the other quad)
  return v;
}
// (mean, rstd) of a group from its fp64 totals
static __device__ __forceinline__ void gn_mean_rstd(double s, double q, float inv_count, float eps, float& mean, float& rstd) {
  // the element count is an integer below 2^22: recovered exactly from its fp32 reciprocal.  (Multiplying by the ROUNDED reciprocal scales
  // E[x^2] and mean^2 by (1 + 6e-8) and (1 + 6e-8)^2: the difference is off by 6e-8 E[x^2] -- 0.5 % of the variance at |mean| = 300 sigma,
  // which is what the first fp64 version of this function still showed: 1e-2 in the normalised output.)  No fp64 DIVISION here: hipcc expands
  // one into ~40 instructions and this sits, single-lane, in front of the barrier of every GroupNorm launch (three of them cost a 256^2 stamp
  // 0.4 ms): the fp64 reciprocal of the count is the fp32 one refined by one Newton step (relative error 4e-15).
  const float nf = rintf(1.0f / inv_count);
  const double n = (double)nf;
  double inv = (double)(1.0f / nf);
  inv = inv * (2.0 - n * inv);
  const double m = s * inv;
  const double var = q * inv - m * m;
  mean = (float)m;
  rstd = rsqrtf(fmaxf((float)var, 0.f) + eps);
}

#define DTP_WAVE 64

#define HIP_CHECK(x)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) {                                                                 \
      dtp_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
      return DTP_ERR_HIP;                                                                   \
    }                                                                                       \
  } while (0)

// error codes: include/dtp.h (DTP_OK, DTP_ERR_*)

void dtp_set_error(const char* fmt, ...);

// ---------------------------------------------------------------- implicit GEMM (gemm_conv.hip)
enum {
  GF_BIAS = 1,       // += bias[n] (fp32)
  GF_BIAS_M = 2,     // += bias[m] (fp32) -- operand-swapped calls (V^T = Wv X^T)
  GF_RESID = 4,      // += R[m][n]
  GF_GEGLU = 8,      // out[m][f] = a * gelu(g); W rows packed [a(BN/2) | g(BN/2)] per 128-col tile
  GF_CONV3 = 16,     // A is an im2col view of an NHWC tensor (3x3 taps)
  GF_UPS2 = 32,      // conv input is the nearest-2x upsample of A (fused gather)
  GF_GELU = 64,      // out = gelu_erf(x)
  GF_QUICKGELU = 128,// out = x * sigmoid(1.702 x)
  GF_OUT_F32 = 256,  // C is fp32 (ldc in floats)
  GF_SILU = 512,     // out = x * sigmoid(x)
  GF_LNFOLD = 1024,  // A is the RAW pre-LayerNorm tensor; W carries gamma, bias carries W.beta; row statistics come from
                     // the producer (st_in) or are computed in-kernel; out = rstd*(acc - mean*lns[n]) + bias[n]
  GF_ROWSTATS = 2048,// also emit per-row (sum, sum of squares) of the fp16 output, one partial per N tile -> st_out
  GF_SOFTMAX16 = 4096,// epilogue: softmax over each aligned group of 16 output columns (first sm_valid of them; the rest -> 0)
  GF_MFAST = 1 << 20,// internal: tile_m varies fastest (neighbouring workgroups share the W panel)
  GF_NOREDUCE = 1 << 21,// internal: a split launch leaves its fp32 slabs for the consumer (fused reduce + GroupNorm)
  GF_XCDSPLIT = 1 << 23,// internal (set by the launcher): 1-D grid of tiles x splits blocks, K-slice z pinned to XCD z % 8 (see dtp_xcd_split)
  GF_GNSTATS = 1 << 24, // convws_kernel only (unsplit, two-n-tile builds): also emit the per-(pixel tile, group) sums / sums of squares of the
                        // rounded output for the GroupNorm that consumes it -> st_out [image][2 * tiles][N / gn_cpg][2] (conv_ws.hip)
  GF_RAGGED = 1 << 25,  // convws_kernel variants 2 / 3 may cover a map whose size is not a multiple of the 8 x 16 tile (and take the
                        // GF_UPS2 window cropped to 2 Hi - 1); set by the builder at resolutions that are not multiples of 64 only
  GF_GNAPPLY = 1 << 22, // conv_halo_kernel only: A is the RAW pre-GroupNorm tensor; the staged input patch is normalised (+ SiLU) in LDS
                        // from the statistics partials gn_part (GemmParams::gn_*): no apply launch, no normalised tensor
};

struct GemmParams {
  const f16* A;      // activations: dense [M][lda] or NHWC image for CONV3
  const f16* W;      // weights [N_pad][ldw], K contiguous, zero padded to k-block multiples
  const f16* Wcb;    // same 3x3 weights packed channel-block-major (k' = (cb*9+tap)*64 + c) for conv_halo_kernel; may be null
  const f16* Wfr;    // same 3x3 weights (+ the fused shortcut's 1x1 weights behind them) in MFMA fragment order for convws_kernel (conv_ws.hip), or the
                     // dense weights in fragment order for gemmws_kernel (gemm_ws.hip); may be null
  const f16* Wfr4;   // GF_UPS2 convs: the four phase sets of collapsed 2x2 weights for the phase build of convws_kernel (tile ids 56 / 57,
                     // pack_conv_ws_ups4_kernel in conv_ws.hip); may be null
  void* C;           // fp16 [M][ldc] (or fp32 with GF_OUT_F32)
  float* part;       // split-K partial slabs [splits][M][N] fp32 (when splits > 1)
  const float* bias; // fp32
  const f16* R;      // residual [M][ldr]
  const f16* zero;   // >= 16 bytes of zeros in device memory (source for padded taps)
  const float* lns;  // GF_LNFOLD: lns[n] = sum_k W'[n][k] (fp32, over the packed fp16 weights)
  float ln_eps;
  const float* st_in;  // GF_LNFOLD: [st_parts][M][2] partial (sum, sumsq) of the rows of A; null = compute in-kernel
  int st_parts;
  float* st_out;       // GF_ROWSTATS: [tiles_n][M][2]
  int M, N, K;
  int lda, ldw, ldc, ldr;
  int nkb;           // number of 64-wide k-blocks in total
  int splits;        // grid.z
  int kb_per_split;
  int col_ranges;    // tile DTP_TILE_LNLIN only: column ranges per row block (set by the tuner / caller)
  int Hi, Wi, Ho, Wo, Cin, stride, pad;  // CONV3 geometry (Hi/Wi are the stored input dims)
  const f16* A2;     // CONV3: a 10th, dense "tap" appended to K -- the ResBlock's 1x1 shortcut conv, read from the block input
  int lda2, Cin2;    // [M][lda2] (Cin2 channels, multiple of 64); dense GEMM: a second activation matrix supplying the LAST Cin2
                     // columns of the contraction (K - Cin2 from A, then Cin2 from A2; both multiples of 64); null / 0 = none
  int flags;
  // batched (grouped) problems: grid.y = batch; problem b uses A + b*a_bs, W + b*w_bs, C + b*c_bs, R + b*r_bs (elements),
  // bias + b*bias_bs, lns + b*lns_bs.  Row statistics stay indexed by the global row b*M + m of a [parts][st_rows][2] array.
  int batch;         // 0/1 = plain GEMM
  long long a_bs, w_bs, c_bs, r_bs;
  int bias_bs, lns_bs, st_rows;
  int sm_valid;      // GF_SOFTMAX16: valid columns per group of 16
  // GF_GNAPPLY: GroupNorm of the conv input applied on the staged patch.  gn_part = per-chunk (sum, sumsq) partials of the statistics
  // pass [B][gn_nchunk][groups][2] (groups = Cin / gn_cpg <= 32), gn_gamma / gn_beta fp32 [Cin]
  const float *gn_part, *gn_gamma, *gn_beta;
  int gn_nchunk, gn_cpg, gn_silu;
  float gn_eps;
  // fp8 (e4m3) variant (gemm_fp8.hip, tile ids 24..27): W8 = per-tensor quantised copy of W, [N_pad][ldw8] bytes (K padded to 128)
  const unsigned char* W8;
  int ldw8;
  float a_scale, w_scale;  // A8 = e4m3(A / a_scale), W8 = e4m3(W / w_scale); powers of two
  // host-side only (builder.hip make_gemm_op): the calibrated activation scale of this fp8 problem lives at *a_scale_host (read at
  // enqueue time, i.e. before graph capture); amax_slot1 - 1 = its slot in the context's amax table (0: none)
  const float* a_scale_host;
  int amax_slot1;
  // two-operand e4m3 GEMM (gemm_f8f8.hip): A8 = e4m3(A / a_scale) [M][lda8] bytes, A2_8 the same for the A2 columns (one scale for
  // both unless a2_scale is set); C8 (or null) = e4m3(out / c_scale) [M][ldc8] next to / instead of the fp16 C
  const unsigned char* A8;
  int lda8;
  const unsigned char* A2_8;
  int lda2_8;
  unsigned char* C8;
  int ldc8;
  float c_scale;
  float a2_scale;  // scale of A2_8 (0 = a_scale); another power of two needs (K - Cin2) % 128 == 0: applied as the MFMA's E8M0 block scale
};

// ---------------------------------------------------------------- e4m3 activation operands (gemm_f8f8.hip)
// quantise pass: up to two row-parallel jobs over the same M rows; job j writes y = e4m3(x / scale) or, with ln, e4m3(LN(x) / scale)
// where LN(x) = (x - mean) * rstd (no gamma / beta) from the producer's row-statistic partials st_in [st_parts][st_rows][2] (null:
// computed here).  Values beyond +-448 * scale saturate.
struct Quant8Job {
  const f16* x; int ld, K;
  unsigned char* y; int ldy;
  float scale;
  int ln;
};
struct Quant8Params {
  int M, njobs;
  Quant8Job job[2];
  const float* st_in; int st_parts, st_rows;
  float eps;
};
bool dtp_quant8_supported(const Quant8Params& q);
int dtp_launch_quant8(const Quant8Params& q, hipStream_t s);
// tile: 0 = 128x128, 1 = 64x128 (M x N), four waves each; -1 = heuristic (dtp_gemm_f8f8_pick)
bool dtp_gemm_f8f8_supported(const GemmParams& p);
int dtp_gemm_f8f8_pick(const GemmParams& p, int num_cu);
int dtp_launch_gemm_f8f8(const GemmParams& p, int tile, hipStream_t s);
void dtp_gemm_f8f8_init();

// K-slices pinned to XCDs.  Block b of a launch runs on XCD b % 8 and every XCD has its own L2: with the split index on grid.z the
// tiles of one K-slice are spread over all XCDs, so each slice's operand panels are fetched from the Infinity Cache / HBM into up to
// eight L2s (the shared panels of a level-2 conv: ~6x its weights).  With a 1-D grid and slice z on XCD z % 8 (S >= 8) -- or a slice
// on 8 / S XCDs (S = 2, 4) -- a panel crosses into exactly the L2(s) of its slice.  Applies when S is a power of two and the
// blocks divide evenly; otherwise the launcher keeps grid.z.
static inline bool dtp_xcd_split_ok(int tiles, int splits) {
  if (splits < 2 || (splits & (splits - 1)) || splits > 32) return false;
  return splits >= 8 || (tiles % (8 / splits)) == 0;
}
static __device__ __forceinline__ void dtp_xcd_split(int id, int tiles, int splits, int& tile, int& z) {
  const int xcd = id & 7, idx = id >> 3;
  if (splits >= 8) { const int r = splits >> 3; z = xcd + 8 * (idx % r); tile = idx / r; }
  else { const int g = 8 / splits; z = xcd % splits; tile = idx * g + xcd / splits; }
}

// gemm_kernel tile ids only (dtp_tile(tile).fam == TF_GEMM); dtp_launch_tile takes every family
int dtp_launch_gemm(const GemmParams& p, int tile, hipStream_t s);
void dtp_gemm_init();  // raises the dynamic-LDS limit once, outside any stream capture
int dtp_launch_tile(const GemmParams& p, int tile, hipStream_t s);
int dtp_launch_splitk_reduce(const GemmParams& p, hipStream_t s);
size_t dtp_gemm_workspace_bytes(const GemmParams& p);
void dtp_gemm_pick(GemmParams& p, int* tile, int num_cu);  // sets splits/kb_per_split

// ---------------------------------------------------------------- norms (norm.hip)
// GroupNorm over NHWC [B][HW][C] (row strides ldx / ldy), optional fused SiLU, fp32 statistics: the problem every launcher takes.
// (x is const for all but the two launches with a GnReduceSrc: those sum the slabs and WRITE x before they normalise it)
struct GnParams {
  const f16* x; int ldx; f16* y; int ldy; const float *gamma, *beta; int B, HW, C, groups; float eps; int silu;
};
// the split-K slabs of the conv that produced a GroupNorm's input: the GroupNorm-side kernel sums them (+ bias, + residual R) and writes x
struct GnReduceSrc {
  const float* part; int splits; long long slab; int ldp; const float* bias; const f16* R; int ldr;
};
int dtp_launch_groupnorm(const GnParams& p, float* stats_ws, hipStream_t s);
size_t dtp_groupnorm_ws_bytes(int B, int HW, int C, int groups);
int dtp_groupnorm_stat_chunks(int HW);  // pixel chunks per sample of dtp_launch_groupnorm_stats (partials [B][chunks][groups][2])
// the apply pass alone, on partial sums [B][nchunk][groups][2] that somebody else produced (a convws_kernel launch with GF_GNSTATS)
int dtp_launch_groupnorm_apply(const GnParams& p, const float* partial, int nchunk, hipStream_t s);
// the statistics pass alone (partial sums -> ws; y, gamma, beta unused), with rd the producing conv's split-K reduce rides in it
int dtp_launch_groupnorm_stats(const GnParams& p, float* ws, const GnReduceSrc* rd, hipStream_t s);
// split-K reduce (+ bias, + residual) of a conv output fused with the GroupNorm (+SiLU) that consumes it: writes the fp16 conv
// output p.x AND the normalised tensor p.y -- in one launch where dtp_reduce_groupnorm_supported() (HW <= 256), otherwise the
// reduce rides in the statistics pass of the two-launch GroupNorm (needs stats_ws, dtp_groupnorm_ws_bytes).  Cx: channels [0, Cx)
// come from the slabs, the rest (a concatenation's other half) are already in p.x; 0 = all
bool dtp_reduce_groupnorm_supported(int HW, int C, int groups);
int dtp_launch_reduce_groupnorm(const GnParams& p, const GnReduceSrc& rd, int Cx, float* stats_ws, hipStream_t s);
// may a GroupNorm over [..][C] rows of pitch ldx take over the reduce of slabs of pitch ldp (residual pitch ldr, 0 = none)?  What BOTH
// launchers with a reduce source accept: a claim (Builder::claim_reduce) may end in either
bool dtp_groupnorm_reduce_accepts(int C, int groups, int ldx, int ldp, int ldr);
// GroupNorm (no activation) folded into the Linear that consumes it: per-sample weights W diag(a_b) / biases bias + W d_b for a grouped
// GEMM on the raw tensor, from the partial sums of the statistics pass (p: gamma, beta, B, HW, C, groups, eps; norm.hip
// gn_fold_weights_kernel).  nchunk: partials per sample in `partial`, 0 = the statistics pass's own count
int dtp_launch_gn_fold_weights(const GnParams& p, const float* partial, int nchunk, const f16* W, int ldw, const float* bias, int Nout, f16* Wout,
                               long long w_bs, float* bias_out, int bias_bs, hipStream_t s);
int dtp_launch_layernorm(const f16* x, int ldx, f16* y, int ldy, const float* gamma, const float* beta, int rows, int C,
                         float eps, hipStream_t s);
int dtp_launch_softmax_rows(const f16* x, int ldx, f16* y, int ldy, int rows, int cols, float scale, hipStream_t s);

// ---------------------------------------------------------------- attention (attention.hip)
struct AttnParams {
  const f16 *Q, *K, *V;
  f16* O;
  int ldq, ldk, ldv, ldo;       // row strides (elements)
  int B, H, Sq, Skv, D;         // head h reads columns [h*D, (h+1)*D)
  long long qbs, kbs, vbs, obs; // batch strides (elements)
  float scale;
  int prio;  // $DTP_ATTN_PRIO: raise the wave priority around the MFMA clusters
  int skew;  // experiment ($DTP_ATTN_SKEW): start delay of every other workgroup, in units of 64 cycles
};
int dtp_launch_attention(const AttnParams& p, hipStream_t s);
// attn_dma.hip: K / V by LDS-DMA, V^T fragments by transpose reads (d = 40 / 80, Skv a multiple of 64); dtp_launch_attention dispatches
bool dtp_attention_uses_dma(const AttnParams& p);  // dtp_launch_attention hands p to attn_dma_kernel
bool dtp_attention_dma_supported(const AttnParams& p);
int dtp_launch_attention_dma(const AttnParams& p, hipStream_t s, int nw_force = 0);
// attention_fp8.hip: the same contraction on the fp8 (e4m3) MX MFMA; q_scale / v_scale = per-tensor scales (powers of two)
int dtp_launch_attention_fp8(const AttnParams& p, float q_scale, float v_scale, hipStream_t s);

// ---------------------------------------------------------------- fused cross-attention GEMM pair (xattn.hip)
// Y = softmax_16(LN(X) W1^T + b1) W2^T + b2 + R per sample, X / R / Y [N*S][C] fp16; see xattn.hip
struct XattnParams {
  const f16* X; int ldx;             // LayerNorm input (raw), rows smp*S + m
  const f16* W1; long long w1_bs;    // per sample [128][C] (LayerNorm gamma folded in), K contiguous
  const float *b1, *lns1;            // per sample [128]: bias (+ W.beta), row sums of W1
  const float* st_in; int st_parts, st_rows; float ln_eps;  // producer's per-row (sum, sumsq) partials [parts][st_rows][2]
  const f16* W2; long long w2_bs;    // per sample [roundup(C,128)][128]
  const float* b2;                   // [C] (shared) or null
  const f16* R; int ldr;             // residual rows
  f16* Y; int ldy;
  float* st_out;                     // [ceil(C/128)][st_rows][2] partials of the stored rows, or null
  int S, C, N, sm_valid;             // rows per sample, channels, samples, valid columns per 16-group
  const f16* zero;                   // >= 16 bytes of zeros
  int ct;                            // consecutive 128-column tiles per workgroup (the probability tile is computed once per workgroup); 0 = the launcher chooses
};
int dtp_xattn_tiles_per_wg(int S, int C, int N);
bool dtp_xattn_supported(const XattnParams& p);
int dtp_launch_xattn(const XattnParams& p, hipStream_t s);
void dtp_xattn_init();

// ---------------------------------------------------------------- register-chained out-projection + cross-attention (xchain.hip)
// Y3 = softmax_16(LN(Y2) W1^T + b1) W2^T + b2 + Y2 with Y2 = A Wo^T + bo + Y, per sample; C = 320, S % 128 == 0; Y2 stays in registers
struct XchainParams {
  const f16* A; int lda;             // self-attention output, rows smp * S + m
  const f16* Wo; int ldwo;           // attn1.to_out.0 weights, packed [C][ldwo] (pack_linear)
  const float* bo;                   // [C] or null
  const f16* Y; int ldy;             // residual of the projection (the block's proj_in output)
  const f16* W1; long long w1_bs;    // per sample [128][C] (LayerNorm-2 gamma folded in)
  const float *b1, *lns1;            // per sample [128]
  const f16* W2; long long w2_bs;    // per sample [roundup(C, 128)][128]
  const float* b2;                   // [C] or null
  f16* Y3; int ldy3;
  float* st_out;                     // [N * S][2] per-row (sum, sumsq) of the stored rows (ONE partial per row), or null
  int S, C, N, sm_valid;
  float ln_eps;
  int dup;                           // de-duplicated UNet prefix (unet.hip Dup): A and Y hold samples [dup, N) only and samples [0, dup) read the
                                     // rows of sample + dup (identical inputs up to here); 0 = A and Y hold all N samples
};
bool dtp_xchain_supported(const XchainParams& p);
int dtp_launch_xchain(const XchainParams& p, hipStream_t s);
void dtp_xchain_init();

// ---------------------------------------------------------------- register-chained feed-forward (ffchain.hip)
// Out = [GEGLU(LN(X) W1^T + b1) | X] Wm^T + bm + R, C = 320 (hidden 1280); the hidden tensor stays in registers
struct FfchainParams {
  const f16* X; int ldx;             // y3 rows [M][C] (raw: LayerNorm-3 folded into W1 / lns1 / b1)
  const f16* W1; int ldw1;           // ff.net.0.proj packed [2 H][ldw1] in the GEGLU row packing (a(64) | gate(64) per 128 rows), gamma folded in
  const float *lns1, *b1;            // [2 H] row sums of W1 and bias (+ W beta), indexed by packed row
  const f16* Wm; int ldwm;           // merged [ff.net.2 | proj_out] weights packed [>= C][ldwm], K = H + C (unet.hip load_linear_pair)
  const float* bm;                   // [C] or null
  const f16* R; int ldr;             // residual rows (the block input) or null
  f16* Out; int ldo;
  int M, C;
  float ln_eps;
};
bool dtp_ffchain_supported(const FfchainParams& p);
int dtp_launch_ffchain(const FfchainParams& p, hipStream_t s);
void dtp_ffchain_init();

// ---------------------------------------------------------------- elementwise / layout (elementwise.hip)
int dtp_launch_concat_channels(const f16* a, int lda, int Ca, const f16* b, int ldb, int Cb, f16* y, int ldy, long long rows,
                               hipStream_t s);
// several strided row copies in one launch (rows of row_bytes bytes; everything 16-byte aligned)
#define DTP_COPY_SEGS 8
struct CopySegs {
  int n;
  const char* src[DTP_COPY_SEGS];
  char* dst[DTP_COPY_SEGS];
  long long rows[DTP_COPY_SEGS], row_bytes[DTP_COPY_SEGS], src_stride[DTP_COPY_SEGS], dst_stride[DTP_COPY_SEGS];
  long long chunks[DTP_COPY_SEGS], total;  // filled by the launcher
};
int dtp_launch_copy_rows(CopySegs segs, hipStream_t s);
int dtp_launch_f32_to_f16(const float* x, f16* y, long long n, hipStream_t s);
int dtp_launch_nchw_f32_to_nhwc_f16(const float* x, f16* y, int B, int C, int HW, int Cpad, hipStream_t s);
int dtp_launch_nhwc_f16_to_nchw_f32(const f16* x, int ldx, float* y, int B, int C, int HW, hipStream_t s);
int dtp_launch_pack_conv_weight(const float* w, f16* out, int Cout, int Cin, int Cin_pad, int taps, int ldw, hipStream_t s);
int dtp_launch_pack_linear_weight(const float* w, f16* out, int N, int K, int ldw, const int* row_map, hipStream_t s);
int dtp_launch_rowdot(const float* w, const float* v, float* out, int N, int K, hipStream_t s);
int dtp_launch_scale_cols(float* w, const float* g, int N, int K, hipStream_t s);
int dtp_launch_rowsum_f16(const f16* w, int ld, int K, float* out, int rows, hipStream_t s);
int dtp_launch_matmul_f32(const float* A, const float* B, float* C, int M, int N, int K, hipStream_t s);
int dtp_launch_expand_kv(const f16* kv, f16* kexp, f16* vexp, int N, int T, int C, int H, float scale, hipStream_t s);
int dtp_launch_transpose_f16(const f16* src, int lds_, f16* dst, int ldd, int rows, int cols, hipStream_t s);
int dtp_launch_rowdot_f16(const f16* a, int ld, const float* v, float* out, int rows, int K, hipStream_t s);
// gemm_fp8.hip: dense GEMM on the fp8 MX MFMA (tile ids 24..27 of dtp_launch_gemm = 128x128 / 128x64 / 64x64 / 64x128)
bool dtp_gemm_fp8_supported(const GemmParams& p);
int dtp_launch_gemm_fp8(const GemmParams& p, int tile, hipStream_t s);
void dtp_gemm_fp8_init();
int dtp_quantize_weights_fp8(const f16* w, int ldw, int K, int rows, unsigned char* out, int ldw8, float* scale_out, hipStream_t s);
// gemm_wide.hip: 8-wave wide tiles; variant 0 = 256x256, 1 = 256x320 (tile ids 20 / 21 of dtp_launch_gemm)
bool dtp_gemm_wide_supported(const GemmParams& p, int variant);
int dtp_launch_gemm_wide(const GemmParams& p, int variant, hipStream_t s);
void dtp_gemm_wide_init();
// conv_halo.hip: variant 0..3 = (8x16|8x8 pixel tile) x (64|128 output channels); kb_per_split counts 64-channel blocks
constexpr int DTP_TILE_LNLIN = 50;  // lnlin_kernel (lnlin.hip): the "splits" of a tune entry are its column ranges, K is not split
constexpr int DTP_TILE_WS0 = 51;    // convws_kernel (conv_ws.hip): 51 = three 8 x 8 images, 52 = one 16 x 16 image, 53 = an 8 x 16 pixel tile x 64 channels per workgroup, 54 = the same for two co-resident workgroups per CU; splits = K-slices
constexpr int DTP_WS_VARIANTS = 6;  // convws variants: 0..3 = tile ids 51..54, 4 / 5 = tile ids 56 / 57
constexpr int DTP_TILE_GEMMWS = 55; // gemmws_kernel (gemm_ws.hip): dense problems with the fragment-order packing; splits = K-slices
constexpr int DTP_TILE_WSUPS4 = 56; // convws_kernel, phase build for GF_UPS2 (four 2x2 phase convs over the stored map, needs Wfr4): 56 / 57 = the geometry of 53 / 54; unsplit
constexpr int DTP_TILE_IDS = 58;    // tile ids are 0 .. DTP_TILE_IDS - 1

// profiling classes (dtp_profile_rows): 0-11 = gemm_kernel<BM,BN,NS> variants (id = shape + 4*(NS-2)), then the rest
enum { PK_GEMM0 = 0, PK_ATTN = 12, PK_GN = 13, PK_LN = 14, PK_ELEM = 15, PK_SOFTMAX = 16, PK_HALO0 = 17, PK_BIG0 = 21, PK_WIDE0 = 25, PK_FP8 = 27, PK_KH2 = 28, PK_LW = 36, PK_XATTN = 44, PK_HALO3 = 45, PK_LNLIN = 47, PK_WS0 = 48, PK_GEMMWS = 52, PK_F8F8 = 53, PK_QUANT8 = 54, PK_COUNT = 55 };

// ---- tile ids.  Every GEMM / conv launch of the engine is named by one id: the value of a tune table entry, of dtp_gemm_desc.tile
// and of LastGemm.  dtp_tile(id) is the only decoder: which kernel family runs the id, the variant that family's launcher takes,
// the tile shape, the profiling class, and what the "splits" of a configuration (tile, splits) mean.
enum DtpFamily : unsigned char { TF_NONE, TF_GEMM, TF_HALO, TF_WIDE, TF_FP8, TF_LNLIN, TF_CONVWS, TF_GEMMWS };
enum DtpSplit : unsigned char {
  SPLIT_K,       // K-slices of 64-wide k-blocks (the fp32 slabs are reduced by dtp_launch_splitk_reduce)
  SPLIT_HALO,    // K-slices of whole channel blocks: conv_halo_kernel unrolls the nine taps of a block, so a slice is a multiple of 9
  SPLIT_BLOCKS,  // K-slices that are ranges of whole channel / k-blocks (conv_ws.hip, gemm_ws.hip): every factor is realised
  SPLIT_COLS,    // column ranges per 128-row block (lnlin.hip); K is not split
  SPLIT_NONE,    // unsplit only (gemm_wide.hip, gemm_fp8.hip)
};
struct DtpTile {
  DtpFamily fam;
  int var;              // the variant the family's launcher takes: halo 0..5, wide 0..1, fp8 0..4, convws 0..5
  int bm, bn, ns;       // output tile and pipeline depth (0: the family has none)
  int kh, lw;           // gemm_kernel: 1 / 2 k-halves (4 / 8 waves), loader waves (0 = none)
  DtpSplit split;
  int pk;               // PK_* profiling class
};
// 0..11: gemm_kernel, shape (id & 3) of {128x128, 128x64, 64x64, 64x128} at depth 2 + id / 4.  12..15: conv_halo_kernel variants
// 0..3.  16..19: gemm_kernel {256x128, 256x128, 128x256, 128x256} at depth {2, 3, 2, 3}.  20 / 21: gemm_wide_kernel 256 x 256 /
// 256 x 320 (8 waves).  24..27: gemm_fp8_kernel, the shapes of ids 0..3; 28: its 8-wave 256 x 256.  32..39: gemm_kernel with 8 waves
// (KH = 2), shape (id & 3) at depth 2 + (id - 32) / 4.  40..47: gemm_kernel at depth 3 with 4 (40..43) or 8 loader waves.
// 48 / 49: conv_halo_kernel variants 4 / 5 (three images per workgroup).  50 / 51..54 / 55 / 56..57: see DTP_TILE_*.  22, 23 and 29..31 are
// holes: TF_NONE, as is any id outside 0 .. DTP_TILE_IDS - 1.
inline DtpTile dtp_tile(int id) {
  static constexpr int sm[4] = {128, 128, 64, 64}, sn[4] = {128, 64, 64, 128};
  const int s = id & 3;
  if (id >= 0 && id < 12) return {TF_GEMM, 0, sm[s], sn[s], 2 + id / 4, 1, 0, SPLIT_K, PK_GEMM0 + id};
  if (id >= 12 && id < 16) return {TF_HALO, id - 12, 0, 0, 0, 0, 0, SPLIT_HALO, PK_HALO0 + id - 12};
  if (id >= 16 && id < 20) return {TF_GEMM, 0, id < 18 ? 256 : 128, id < 18 ? 128 : 256, 2 + (id & 1), 1, 0, SPLIT_K, PK_BIG0 + id - 16};
  if (id == 20 || id == 21) return {TF_WIDE, id - 20, 256, id == 20 ? 256 : 320, 2, 0, 0, SPLIT_NONE, PK_WIDE0 + id - 20};
  if (id >= 24 && id < 28) return {TF_FP8, id - 24, sm[s], sn[s], 2, 0, 0, SPLIT_NONE, PK_FP8};
  if (id == 28) return {TF_FP8, 4, 256, 256, 2, 0, 0, SPLIT_NONE, PK_FP8};
  if (id >= 32 && id < 40) return {TF_GEMM, 0, sm[s], sn[s], 2 + (id - 32) / 4, 2, 0, SPLIT_K, PK_KH2 + id - 32};
  if (id >= 40 && id < 48) return {TF_GEMM, 0, sm[s], sn[s], 3, 1, id < 44 ? 4 : 8, SPLIT_K, PK_LW + id - 40};
  if (id == 48 || id == 49) return {TF_HALO, id - 44, 0, 0, 0, 0, 0, SPLIT_HALO, PK_HALO3 + id - 48};
  if (id == DTP_TILE_LNLIN) return {TF_LNLIN, 0, 0, 0, 0, 0, 0, SPLIT_COLS, PK_LNLIN};
  if (id >= DTP_TILE_WS0 && id < DTP_TILE_WS0 + 4) return {TF_CONVWS, id - DTP_TILE_WS0, 0, 0, 0, 0, 0, SPLIT_BLOCKS, PK_WS0 + id - DTP_TILE_WS0};
  if (id == DTP_TILE_WSUPS4 || id == DTP_TILE_WSUPS4 + 1)  // variants 4 / 5, profiled with the classes of the builds they share a geometry with
    return {TF_CONVWS, 4 + id - DTP_TILE_WSUPS4, 0, 0, 0, 0, 0, SPLIT_BLOCKS, PK_WS0 + 2 + id - DTP_TILE_WSUPS4};
  if (id == DTP_TILE_GEMMWS) return {TF_GEMMWS, 0, 64, 64, 0, 0, 0, SPLIT_BLOCKS, PK_GEMMWS};
  return {};
}
// Apply the configuration (tile, sp) -- a tune table entry -- to p: the K-slices (kb_per_split / splits) or the column ranges, and
// the halo kernels' channel-block-major weights (W = Wcb).  False when the tile cannot realise sp: p then holds the split it would take.
inline bool dtp_tile_apply(GemmParams& p, int tile, int sp) {
  const DtpTile t = dtp_tile(tile);
  if (sp < 1) sp = 1;
  if (t.fam == TF_HALO) p.W = p.Wcb;
  if (t.split == SPLIT_NONE || t.split == SPLIT_COLS) {
    p.kb_per_split = p.nkb; p.splits = 1;
    if (t.split == SPLIT_COLS) p.col_ranges = sp;
    return t.split == SPLIT_COLS || sp == 1;
  }
  p.kb_per_split = (p.nkb + sp - 1) / sp;
  if (t.split == SPLIT_BLOCKS) { p.splits = sp; return true; }
  if (t.split == SPLIT_HALO && sp > 1) p.kb_per_split = (((p.nkb + 8) / 9 + sp - 1) / sp) * 9;
  p.splits = (p.nkb + p.kb_per_split - 1) / p.kb_per_split;
  return p.splits == sp;
}
// Row-statistics partials per row that p on tile writes (GF_ROWSTATS): one per column range (lnlin), one when K is split (the
// reduce writes them), else one per N tile.  0 for the tile-less halo and convws kernels, whose launchers refuse GF_ROWSTATS.
inline int dtp_tile_row_parts(const GemmParams& p, int tile) {
  const DtpTile t = dtp_tile(tile);
  if (t.split == SPLIT_COLS) return p.col_ranges;
  if (!t.bn) return 0;
  return p.splits > 1 ? 1 : (p.N + t.bn - 1) / t.bn;
}
// lnlin.hip: activation-stationary LayerNorm-folded Linear (+ GEGLU) for K = 320 / 640; nsplit = column ranges per 128-row block
bool dtp_lnlin_supported(const GemmParams& p, int nsplit);
int dtp_launch_lnlin(const GemmParams& p, int nsplit, hipStream_t s);
void dtp_lnlin_init();
// conv_ws.hip: weight-streaming 3x3 conv (variant 0: three 8 x 8 images, 1: one 16 x 16 image, 2: an 8 x 16 tile x 64 channels per workgroup,
// 3: 2 for two co-resident workgroups, 4 / 5: the phase builds of 2 / 3 for GF_UPS2)
bool dtp_conv_ws_supported(const GemmParams& p, int variant, int nsplit);
int dtp_launch_conv_ws(const GemmParams& p, int variant, hipStream_t s);
void dtp_conv_ws_init();
size_t dtp_conv_ws_packed_elems(int Cout, int Cin, int Cin2);
int dtp_conv_ws_gn_chunks(int Ho, int Wo);  // GF_GNSTATS partials per image (two per 8 x 16 pixel tile, partial tiles included)
int dtp_launch_pack_conv_ws(const float* w, const float* w1, f16* out, int Cout, int Cin, int Cin2, hipStream_t s);
size_t dtp_conv_ws_ups4_packed_elems(int Cout, int Cin);  // the four phase sets of a GF_UPS2 conv (variants 4 / 5)
int dtp_launch_pack_conv_ws_ups4(const float* w, f16* out, int Cout, int Cin, hipStream_t s);
// gemm_ws.hip: weight-streaming dense GEMM (64 x 64 per workgroup, the waves split the contraction by k-blocks)
bool dtp_gemm_ws_supported(const GemmParams& p, int nsplit);
int dtp_launch_gemm_ws(const GemmParams& p, hipStream_t s);
void dtp_gemm_ws_init();
size_t dtp_gemm_ws_packed_elems(int N, int K);
int dtp_launch_pack_linear_ws(const f16* w, int ldw, f16* out, int N, int K, hipStream_t s);
bool dtp_conv_halo_supported(const GemmParams& p);
bool dtp_conv_halo3_supported(const GemmParams& p);  // variants 4 / 5 (tile ids 48 / 49): three images per workgroup
int dtp_launch_conv_halo(const GemmParams& p, int variant, hipStream_t s);
void dtp_conv_halo_init();
int dtp_launch_pack_conv_weight_cb(const float* w, f16* out, int Cout, int Cin, int ldw, hipStream_t s);
int dtp_launch_touch(const void* p, size_t bytes, float* sink, hipStream_t s);
// max |x| over a [rows][cols] fp16 matrix (row stride ld) -> atomicMax on the float bits at *slot (non-negative floats order like
// unsigned integers): the amax pass of the fp8 calibration
int dtp_launch_amax_f16(const f16* x, long long rows, int cols, int ld, unsigned int* slot, hipStream_t s);
int dtp_launch_lora_merge(float* w, const float* up, const float* down, int N, int K, int rank, float scale, hipStream_t s);
