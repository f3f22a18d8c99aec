// Two-operand e4m3 GEMM for gfx950 and the quantise pass that produces its activation operand (option fp8_operands: q/k/v, to_out and
// FF1 of the C = 1280 transformer blocks, unet.hip; kernel level: dtp_op_gemm_f8f8, dtp_op_quant_e4m3).
//
//   C[m][n] = epilogue( a_scale * w_scale * sum_k A8(m,k) * W8[n][k] )       A8 = e4m3(A / a_scale), W8 = e4m3(W / w_scale)
//
// Unlike gemm_fp8_kernel (gemm_fp8.hip), which converts fp16 activations in registers on their way into LDS, BOTH operands sit in
// HBM as OCP e4m3 bytes and travel by direct-to-LDS DMA at one byte per element: A8 [M][lda8] (+ A2_8 [M][lda2_8] supplying the
// last Cin2 columns of the contraction, as in gemm_kernel; its own power-of-two scale a2_scale enters as the MFMA's E8M0 block scale
// of those k-blocks) and the per-tensor weight copy W8 [N_pad][ldw8] (K padded to 128, rows to a multiple of 128, zero beyond N / K).
// The structure is that of tools/micro/fp8_linear_probe.hip: a three-stage ring of 128-byte LDS rows for both operands (same
// XOR swizzle as every DMA GEMM here), one counted vmcnt and one barrier per 128-wide k-block, hand-issued ds_read_b128
// fragments with counted lgkmcnt, two v_mfma_scale_f32_32x32x64_f8f6f4 per 32 x 32 block and k-block with unit block scales.
// `a_scale * w_scale` is applied when the accumulators are staged; the epilogues are gemm_kernel's (bias, fp16 residual, GEGLU,
// row statistics) plus an e4m3 output C8 = e4m3(out / c_scale), quantised from the fp16-rounded output value (the value the fp16
// output C would hold: with both written, C8 is exactly the quantisation of C).
// Rows past M and k-chunks past K read the zero page, so M is arbitrary; N is a multiple of 64 (GEGLU: of 128).
//
// The quantise pass (quant8_kernel) writes e4m3(x / scale) of fp16 rows, optionally after the LayerNorm (x - mean) * rstd with the
// producer's row-statistic partials (the layout GF_LNFOLD reads; no gamma / beta: those are folded into the consumer's packed
// weights and bias, so the consumer of a normalised copy is a plain GF_BIAS GEMM).  One wave per row and job; up to two jobs
// (e.g. a raw and a normalised copy of the same rows) per launch.
// Both kernels SATURATE: values beyond +-448 * scale are clamped to +-448 before the conversion (the hardware conversion is
// round-to-nearest-even on the clamped value).
#include <math.h>

#include <algorithm>

#include "common.h"
#include "tile_epilogue.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
constexpr unsigned UNIT_SCALES = 0x7f7f7f7fu;
constexpr int NSTAGE = 3;

__device__ __forceinline__ void glds16(const void* src, void* lds_uniform) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_uniform, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// +-lim saturation that lets NaN through (fminf / fmaxf would turn it into -lim and hide it from a finiteness check)
__device__ __forceinline__ float sat(float x, float lim) { return x == x ? fminf(fmaxf(x, -lim), lim) : x; }
// four fp32 values / scale -> four e4m3 bytes, saturating at +-448
__device__ __forceinline__ unsigned q8x4(float a, float b, float c, float d, float scale) {
  const float lim = 448.0f * scale;
  a = sat(a, lim); b = sat(b, lim); c = sat(c, lim); d = sat(d, lim);
  s16x2 r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(s16x2{0, 0}, a, b, scale, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, c, d, scale, true);
  return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ u32x2 q8x8(const float (&x)[8], float scale) {
  return u32x2{q8x4(x[0], x[1], x[2], x[3], scale), q8x4(x[4], x[5], x[6], x[7], scale)};
}

__device__ __forceinline__ v8i frag8(f16x8 lo, f16x8 hi) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const i32x4 a = __builtin_bit_cast(i32x4, lo), b = __builtin_bit_cast(i32x4, hi);
  return v8i{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// BM x 128 tile, four waves in a 2 x 2 grid (BM / 2 x 64 each)
template <int BM>
__global__ __launch_bounds__(256) void gemm_f8f8_kernel(const GemmParams p) {
  constexpr int BN = 128, NT = 256, WTM = BM / 2, WTN = BN / 2;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int RPR = 32;                     // LDS rows filled per staging round (4 waves x 8 rows)
  constexpr int AR = BM / RPR, WR = BN / RPR;
  constexpr int LOADS = AR + WR;              // DMA pieces per thread and stage
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int SLD = BN + 8;
  constexpr int NF = 2 * (TN + TM);           // ds_read_b128 per K = 64 step
  static_assert(BM * SLD * 2 <= NSTAGE * STAGE, "the epilogue's staging tile fits in the ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int nwg = tiles_m * tiles_n;
  int wg;
  {  // consecutive tiles on one XCD (blocks are dealt to the eight XCDs round-robin)
    const int q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  int tile_m, tile_n;
  if (p.flags & GF_MFAST) { tile_n = wg / tiles_m; tile_m = wg - tile_n * tiles_m; }
  else { tile_m = wg / tiles_n; tile_n = wg - tile_m * tiles_n; }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nk = (p.K + 127) >> 7;

  // ---- DMA geometry: piece i of a thread = LDS row i * 32 + lrow, 16-byte slot lane & 7 holds source chunk slot ^ ((row >> 1) & 7)
  const int lrow = wave * 8 + (lane >> 3);
  const int chunk = (lane & 7) ^ ((lrow >> 1) & 7);
  const int dense_k1 = p.A2_8 ? p.K - p.Cin2 : p.K;
  int a_m[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = m0 + i * RPR + lrow;
    a_m[i] = (m < p.M) ? m : -1;
  }
  const int n_rows_packed = (p.N + 127) & ~127;
  const unsigned char* w_row[WR];
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    const int n = n0 + i * RPR + lrow;
    w_row[i] = (n < n_rows_packed) ? p.W8 + (size_t)n * p.ldw8 + chunk * 16 : nullptr;
  }
  auto issue = [&](int stage, int t) {
    char* As = smem + stage * STAGE;
    char* Ws = As + BM * 128;
    const int k0 = t * 128 + chunk * 16;
    const bool tail = k0 >= dense_k1;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const void* src = p.zero;
      if (k0 < p.K && a_m[i] >= 0) src = tail ? p.A2_8 + (size_t)a_m[i] * p.lda2_8 + (k0 - dense_k1) : p.A8 + (size_t)a_m[i] * p.lda8 + k0;
      glds16(src, As + (i * RPR + wave * 8) * 128);
    }
#pragma unroll
    for (int i = 0; i < WR; ++i) glds16(w_row[i] ? (const void*)(w_row[i] + (size_t)t * 128) : (const void*)p.zero, Ws + (i * RPR + wave * 8) * 128);
  };

  f32x16 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int wn0 = (wave & 1) * WTN, wm0 = (wave >> 1) * WTM;
  const int frow = lane & 31, fhalf = lane >> 5;

  // activation block scale (E8M0, 127 = 1): 2^e = a2_scale / a_scale on the k-blocks of A2 (whole k-blocks: supported() checks)
  unsigned tail_sc = UNIT_SCALES;
  if (p.A2_8 && p.a2_scale > 0.f && p.a2_scale != p.a_scale) {
    const unsigned b = (unsigned)(127 + ilogbf(p.a2_scale) - ilogbf(p.a_scale));
    tail_sc = b * 0x01010101u;
  }

  issue(0, 0);
  if (nk > 1) issue(1, 1);
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) wait_vmcnt<LOADS>(); else wait_vmcnt<0>();  // this thread's pieces of k-block t have landed
    __syncthreads();  // ... everybody's; and every wave is done with the stage k-block t + 2 overwrites (read in iteration t - 1)
    if (t + 2 < nk) issue((t + 2) % NSTAGE, t + 2);
    const uint32_t a_lds = lds_addr(smem + (t % NSTAGE) * STAGE), w_lds = a_lds + BM * 128;
    const unsigned a_sc = t * 128 >= dense_k1 ? tail_sc : UNIT_SCALES;
    f16x8 fr[2][NF];  // both K = 64 steps of the k-block: [step][weight fragments (2 halves each) | activation fragments]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c0 = 4 * j + 2 * fhalf;  // lane half h of step j supplies chunks c0, c0 + 1 of both operands
#pragma unroll
      for (int q = 0; q < TN; ++q) {
        const int row = wn0 + q * 32 + frow, key = (row >> 1) & 7;
        fr[j][2 * q] = lds_read16(w_lds + row * 128 + ((c0 ^ key) << 4));
        fr[j][2 * q + 1] = lds_read16(w_lds + row * 128 + (((c0 + 1) ^ key) << 4));
      }
#pragma unroll
      for (int q = 0; q < TM; ++q) {
        const int row = wm0 + q * 32 + frow, key = (row >> 1) & 7;
        fr[j][2 * (TN + q)] = lds_read16(a_lds + row * 128 + ((c0 ^ key) << 4));
        fr[j][2 * (TN + q) + 1] = lds_read16(a_lds + row * 128 + (((c0 + 1) ^ key) << 4));
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j == 0) wait_lds_frags<NF, NF>(fr[0]);  // step 0's reads are done while step 1's are still in flight
      else wait_lds_frags<0, NF>(fr[1]);
#pragma unroll
      for (int q = 0; q < TM; ++q) {
        const v8i af = frag8(fr[j][2 * (TN + q)], fr[j][2 * (TN + q) + 1]);
#pragma unroll
        for (int i = 0; i < TN; ++i)
          acc[i][q] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(frag8(fr[j][2 * i], fr[j][2 * i + 1]), af, acc[i][q], 0, 0, 0, UNIT_SCALES, 0, a_sc);
      }
    }
  }
  __syncthreads();  // the ring becomes the epilogue's staging tile

  // ---------------------------------------------------------------- epilogue (layout and fusions as in gemm_fp8_kernel)
  const float sc = p.a_scale * p.w_scale;
  f16* stg = (f16*)smem;
  const int fl = p.flags;
  stage_tile<TN, TM, SLD>(stg, acc, wm0 + frow, wn0 + 4 * fhalf, StageScaled{sc});
  __syncthreads();
  if (fl & GF_GEGLU) {  // W rows packed [a (64) | gate (64)] per 128-column tile -> 64 output columns
    const int nc = tid & 7;
    const int ca = nc * 8, cg = ca + 64, col = (n0 / 128) * 64 + nc * 8;
    float ba[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (fl & GF_BIAS) {
      cols8<false>(p.bias, n0 + ca, ba);
      cols8<false>(p.bias, n0 + cg, bg);
    }
    const bool col_ok = (n0 + cg + 8 <= p.N);
    for (int idx = tid; idx < BM * 8; idx += NT) {
      const int ml = idx >> 3, m = m0 + ml;
      if (m >= p.M || !col_ok) continue;
      const f16x8 a = *(const f16x8*)(stg + ml * SLD + ca), gt = *(const f16x8*)(stg + ml * SLD + cg);
      float x[8];
      const f16x8 o = geglu_chunk(a, gt, 1.f, ba, bg, x);
      if (p.C) *(f16x8*)((f16*)p.C + (size_t)m * p.ldc + col) = o;
      if (p.C8) *(u32x2*)(p.C8 + (size_t)m * p.ldc8 + col) = q8x8(x, p.c_scale);
    }
  } else {
    constexpr int NC = BN / 8;
    const int st_rows = p.st_rows > 0 ? p.st_rows : p.M;
    const int nc = tid % NC, n = n0 + nc * 8;
    const bool col_ok = (n + 8 <= p.N);
    float bv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col_ok && (fl & GF_BIAS)) cols8<false>(p.bias, n, bv);
    for (int idx = tid; idx < BM * NC; idx += NT) {  // BM * NC is a multiple of NT: every lane runs every iteration
      const int ml = idx / NC, m = m0 + ml;
      const bool active = col_ok && m < p.M;
      float s1 = 0.f, s2 = 0.f;
      if (active) {
        float x[8];
        chunk_bias(x, *(const f16x8*)(stg + ml * SLD + nc * 8), bv);
        f16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fl & GF_RESID) r = *(const f16x8*)(p.R + (size_t)m * p.ldr + n);
        const f16x8 o = chunk_round(x, fl & GF_RESID, r, s1, s2);
        if (p.C) *(f16x8*)((f16*)p.C + (size_t)m * p.ldc + n) = o;
        if (p.C8) *(u32x2*)(p.C8 + (size_t)m * p.ldc8 + n) = q8x8(x, p.c_scale);
      }
      if (fl & GF_ROWSTATS) rowstats_emit<NC, true>(s1, s2, nc == 0 && m < p.M, p.st_out + ((size_t)tile_n * st_rows + m) * 2);
    }
  }
}

template <int BM>
constexpr int f8f8_lds() { return NSTAGE * (BM + 128) * 128; }

template <int BM>
int launch_f8f8(const GemmParams& p, hipStream_t s) {
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + 127) / 128);
  static_assert(f8f8_lds<BM>() <= 160 * 1024, "LDS budget");
  hipLaunchKernelGGL(gemm_f8f8_kernel<BM>, dim3(tiles), dim3(256), f8f8_lds<BM>(), s, p);
  return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP;
}

// ---------------------------------------------------------------- quantise pass
__global__ __launch_bounds__(256) void quant8_kernel(const Quant8Params q) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= q.M) return;  // wave-uniform
  const Quant8Job j = blockIdx.y ? q.job[1] : q.job[0];
  const f16* row = j.x + (size_t)m * j.ld;
  unsigned char* out = j.y + (size_t)m * j.ldy;
  const int nch = j.K >> 3;
  float mean = 0.f, rstd = 1.f;
  if (j.ln) {
    if (q.st_in) {  // the producer's partials: the statistics every LayerNorm-folded GEMM of this code base forms
      float s1, s2;
      sum_pairs_strided(q.st_in + (size_t)m * 2, (size_t)q.st_rows * 2, q.st_parts, s1, s2);
      mean = s1 / (float)j.K;
      rstd = rsqrtf(fmaxf(s2 / (float)j.K - mean * mean, 0.f) + q.eps);
    } else {  // two passes over the row (mean, then the centred sum of squares)
      float s1 = 0.f;
      for (int c = lane; c < nch; c += 64) {
        const f16x8 v = *(const f16x8*)(row + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) s1 += (float)v[e];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s1 += __shfl_xor(s1, o);
      mean = s1 / (float)j.K;
      float s2 = 0.f;
      for (int c = lane; c < nch; c += 64) {
        const f16x8 v = *(const f16x8*)(row + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = (float)v[e] - mean; s2 += d * d; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
      rstd = rsqrtf(s2 / (float)j.K + q.eps);
    }
  }
  for (int c = lane; c < nch; c += 64) {
    const f16x8 v = *(const f16x8*)(row + c * 8);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = ((float)v[e] - mean) * rstd;  // fp32: no cancellation when |mean| >> sigma
    *(u32x2*)(out + c * 8) = q8x8(x, j.scale);
  }
}

}  // namespace

void dtp_gemm_f8f8_init() {
  (void)hipFuncSetAttribute((const void*)gemm_f8f8_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, f8f8_lds<128>());
  (void)hipFuncSetAttribute((const void*)gemm_f8f8_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, f8f8_lds<64>());
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the scales are powers of two (exact division in the conversions, an exact E8M0 ratio between A and A2)
static bool pow2(float s) { int e; return s > 0.f && isfinite(s) && frexpf(s, &e) == 0.5f; }

bool dtp_gemm_f8f8_supported(const GemmParams& p) {
  if (!p.A8 || !p.W8 || !p.zero || (!p.C && !p.C8)) return false;
  if (p.flags & ~(GF_BIAS | GF_RESID | GF_GEGLU | GF_ROWSTATS | GF_MFAST)) return false;
  if (p.splits > 1 || p.batch > 1 || p.M <= 0 || p.N <= 0 || (p.N & 63) || p.K <= 0 || (p.K & 15) || (p.ldw8 & 127) || p.ldw8 < p.K) return false;
  if ((p.lda8 & 15) || !al16(p.A8) || !al16(p.W8)) return false;
  if (p.C && ((p.ldc & 7) || !al16(p.C))) return false;
  if (p.C8 && ((p.ldc8 & 7) || ((uintptr_t)p.C8 & 7) || !pow2(p.c_scale))) return false;
  if ((p.flags & GF_BIAS) && !p.bias) return false;
  if ((p.flags & GF_RESID) && (!p.R || (p.ldr & 7) || !al16(p.R))) return false;
  if ((p.flags & GF_GEGLU) && ((p.N & 127) || (p.flags & (GF_RESID | GF_ROWSTATS)))) return false;
  if ((p.flags & GF_ROWSTATS) && !p.st_out) return false;
  if (p.A2_8 && (p.Cin2 <= 0 || p.Cin2 >= p.K || (p.Cin2 & 15) || (p.lda2_8 & 15) || !al16(p.A2_8))) return false;
  if (p.A2_8 && p.a2_scale > 0.f && p.a2_scale != p.a_scale) {
    if (!pow2(p.a2_scale) || ((p.K - p.Cin2) & 127)) return false;
    const int e = ilogbf(p.a2_scale) - ilogbf(p.a_scale);
    if (e < -127 || e > 127) return false;
  }
  return pow2(p.a_scale) && pow2(p.w_scale);
}

// 128 x 128 when that tile alone gives every CU a workgroup, the 64-row tile otherwise (ragged / small-M problems)
int dtp_gemm_f8f8_pick(const GemmParams& p, int num_cu) {
  const long long big = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128);
  return big >= num_cu ? 0 : 1;
}

int dtp_launch_gemm_f8f8(const GemmParams& p, int tile, hipStream_t s) {
  if (!dtp_gemm_f8f8_supported(p) || tile < 0 || tile > 1) {
    dtp_set_error("gemm_f8f8: unsupported problem (M %d N %d K %d flags %d) / tile %d", p.M, p.N, p.K, p.flags, tile);
    return DTP_ERR_ARG;
  }
  const int rc = tile == 0 ? launch_f8f8<128>(p, s) : launch_f8f8<64>(p, s);
  if (rc != DTP_OK) dtp_set_error("gemm_f8f8 launch failed: %s", hipGetErrorString(hipGetLastError()));
  return rc;
}

bool dtp_quant8_supported(const Quant8Params& q) {
  if (q.M <= 0 || q.njobs < 1 || q.njobs > 2) return false;
  bool ln = false;
  for (int i = 0; i < q.njobs; ++i) {
    const Quant8Job& j = q.job[i];
    if (!j.x || !j.y || j.K <= 0 || (j.K & 7) || (j.ld & 7) || (j.ldy & 7) || j.ld < j.K || j.ldy < j.K || !al16(j.x) || ((uintptr_t)j.y & 7) || !pow2(j.scale)) return false;
    ln = ln || j.ln;
  }
  return !(ln && q.st_in && (q.st_parts < 1 || q.st_rows < q.M));
}

int dtp_launch_quant8(const Quant8Params& q, hipStream_t s) {
  if (!dtp_quant8_supported(q)) { dtp_set_error("quant8: unsupported problem (M %d, %d jobs)", q.M, q.njobs); return DTP_ERR_ARG; }
  hipLaunchKernelGGL(quant8_kernel, dim3((q.M + 3) / 4, q.njobs), dim3(256), 0, s, q);
  return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP;
}
