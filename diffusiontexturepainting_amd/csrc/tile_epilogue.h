// Pieces of the staged-tile epilogue: the kernels that round their accumulators into an fp16 tile in LDS and finish from there, in this
// order: (1) what must leave or join the accumulator in fp32 does so, then it is rounded into the tile; (2) a thread
// walks the 8-column chunks it owns: * rstd, + bias[n], + bias[m], activation, 16-wide softmax; (3) + residual, rounding to fp16, the 16-byte
// store; (4) row statistics = sums of the ROUNDED values, reduced over the lanes of a row.  The GEGLU tiles replace (2) and (3) by geglu_chunk.
// Who calls what: gemm_fp8_kernel and gemm_f8f8_kernel everything below (they have bias only in step 2); gemm_wide_kernel stage_tile,
// cols8 + geglu_chunk and rowstats_emit; gemm_kernel rowstats_emit; xattn_kernel stage_block.  gemm_kernel, conv_halo_kernel and the plain
// chunk loop of gemm_wide_kernel hold the same steps as their OWN text (DESIGN.md section 4 says why): a change of the order of operations
// has to be made there too.  Device code only, forced inline.  tools/epilogue_digest.py A/Bs the callers' outputs byte for byte.
#pragma once
#include "common.h"

// D layout of a 32x32 MFMA block: the lane holds token (lane & 31), registers r -> channel (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
// One block -> the staging tile; dst = the lane's row at the block's first column + 4 * (lane >> 5).  pre(q, e, a) is applied to accumulator
// 4 * q + e before it is rounded -- element by element, as scalar expressions: hipcc contracts `(f16)(a * s)` and `(f16)(a - m * l)` into
// v_fma_mixlo_f16 (ONE rounding, straight to fp16) where it finds them, and which elements it finds is part of the output's last bits.
template <class F>
static __device__ __forceinline__ void stage_block(f16* dst, const f32x16& a, F&& pre) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f16x4 v = {(f16)pre(q, 0, a[4 * q]), (f16)pre(q, 1, a[4 * q + 1]), (f16)pre(q, 2, a[4 * q + 2]), (f16)pre(q, 3, a[4 * q + 3])};
    *(f16x4*)(dst + 8 * q) = v;
  }
}
// What happens to accumulator (j, q, e) of n-block i before the rounding.  cols(i) runs once per n-block, BEFORE that block's stores (which
// the compiler must assume alias whatever it reads).
struct StageAsIs {
  __device__ __forceinline__ void cols(int) {}
  __device__ __forceinline__ float pre(int, int, int, float a) const { return a; }
};
struct StageScaled {  // the fp8 kernels: a_scale * w_scale
  float sc;
  __device__ __forceinline__ void cols(int) {}
  __device__ __forceinline__ float pre(int, int, int, float a) const { return a * sc; }
};
struct StageLnFold {  // - mean * lns: the mean term of the LayerNorm fold (common.h, col4)
  const float* mean;  // [TM] this lane's rows
  const float* lns;   // the tile's weight row sums in LDS, at this lane's first column
  f32x4 l[4];         // this lane's 16 columns of the n-block
  __device__ __forceinline__ void cols(int i) {
#pragma unroll
    for (int q = 0; q < 4; ++q) l[q] = *(const f32x4*)(lns + i * 32 + 8 * q);
  }
  __device__ __forceinline__ float pre(int j, int q, int e, float a) const { return a - mean[j] * l[q][e]; }
};
// A wave's acc[TN][TM] -> rows row0 + j * 32, columns col0 + i * 32 + 8 * q of the tile (row0 = wm0 + frow less the row offset of a
// multi-pass epilogue, col0 = wn0 + 4 * fhalf)
template <int TN, int TM, int SLD, class F>
static __device__ __forceinline__ void stage_tile(f16* stg, const f32x16 (&acc)[TN][TM], int row0, int col0, F f) {
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    f.cols(i);
#pragma unroll
    for (int j = 0; j < TM; ++j)
      stage_block(stg + (row0 + j * 32) * SLD + col0 + i * 32, acc[i][j], [&](int q, int e, float a) { return f.pre(j, q, e, a); });
  }
}

// Eight per-column fp32 values (bias) of the complete chunk at column n, as two 16-byte loads (VEC = false: the fp8 kernels' element loads)
template <bool VEC = true>
static __device__ __forceinline__ void cols8(const float* __restrict__ v, int n, float (&o)[8]) {
  if constexpr (VEC) {
    const f32x4 t0 = *(const f32x4*)(v + n), t1 = *(const f32x4*)(v + n + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = t0[e]; o[4 + e] = t1[e]; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = v[n + e];
  }
}

// x[8] = the staged chunk v + bv (step 2 of the kernels that have bias only)
static __device__ __forceinline__ void chunk_bias(float (&x)[8], const f16x8 v, const float (&bv)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = (float)v[e];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] += bv[e];
}

// + residual row (or not), round to fp16; x[] is left holding the ROUNDED values and (s1, s2) gain their sums: statistics of what the
// consumer will actually read
static __device__ __forceinline__ f16x8 chunk_round(float (&x)[8], bool resid, const f16x8 r, float& s1, float& s2) {
  if (resid) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += (float)r[e];
  }
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    o[e] = (f16)x[e];
    x[e] = (float)o[e];
    s1 += x[e]; s2 += x[e] * x[e];
  }
  return o;
}

// o = (rstd * a + ba) * gelu_erf(rstd * g + bg); x[] = the rounded values
static __device__ __forceinline__ f16x8 geglu_chunk(const f16x8 a, const f16x8 g, float rstd, const float (&ba)[8], const float (&bg)[8], float (&x)[8]) {
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float av = rstd * (float)a[e] + ba[e];
    const float gv = rstd * (float)g[e] + bg[e];
    o[e] = (f16)(av * gelu_erf(gv));
    x[e] = (float)o[e];
  }
  return o;
}

// GF_ROWSTATS: NC consecutive lanes hold one row of this N tile (every lane of the group active): fixed-order reduce, the lane with `lead`
// stores the pair.  The ORDER is part of each kernel's output bytes: ascending butterfly (group_allsum) for the fp16 kernels, from offset
// NC / 2 down for the two fp8 kernels.
template <int NC, bool DESCENDING = false>
static __device__ __forceinline__ void rowstats_emit(float s1, float s2, bool lead, float* st) {
  if constexpr (DESCENDING) {
#pragma unroll
    for (int o = NC / 2; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
  } else {
    s1 = group_allsum<NC>(s1); s2 = group_allsum<NC>(s2);
  }
  if (lead) { st[0] = s1; st[1] = s2; }
}
