// Arithmetic of the weight path that the load-time kernels (elementwise.hip) and the LoRA refit (lora_refit.hip) both run: a refitted
// handle holds bit for bit what dtp_finalize_weights packs from the same tensors because both go through THESE functions, in this
// association, with the contractions spelled out (fmaf) instead of left to the compiler's per-kernel choice.
#pragma once
#include "common.h"

// acc + sum_r up_row[r] * down[r * ldd], r ascending, one fused multiply-add per r (trt_inference/models.py:1083: up @ down)
static __device__ __forceinline__ float lora_accumulate(float acc, const float* up_row, const float* down, int ldd, int n) {
  for (int r = 0; r < n; ++r) acc = fmaf(up_row[r], down[(size_t)r * ldd], acc);
  return acc;
}
// W + scale * (up @ down), one fused multiply-add
static __device__ __forceinline__ float lora_merged(float w, float scale, float delta) { return fmaf(scale, delta, w); }
// LayerNorm fold of a Linear's weight (load_linear): W' = W diag(gamma); and the fp16 the packed layouts hold
static __device__ __forceinline__ float ln_fold_gamma(float w, float g) { return w * g; }
static __device__ __forceinline__ f16 pack_weight_f16(float w) { return (f16)w; }

// One wave per row: sum_k w(k) * v[k], lane-strided in k with one fused multiply-add per term, then a butterfly over the 64 lanes
// (every lane returns the sum).  w(k) is a callable: a load for the load path, the merged LoRA weight for the refit.
template <class WAt>
static __device__ __forceinline__ float wave_rowdot(WAt w_at, const float* __restrict__ v, int K, int lane) {
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = fmaf(w_at(k), v[k], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}
// One wave per packed fp16 row: sum_k w[k] (the `lns` vector of a LayerNorm-folded GEMM)
static __device__ __forceinline__ float wave_rowsum_f16(const f16* __restrict__ w_row, int K, int lane) {
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc += (float)w_row[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}
// One 32 x 32 tile of dst[c][r] = src[r][c] by a 256-thread workgroup through `t` (the workgroup's 32 x 33 LDS tile)
static __device__ __forceinline__ void transpose_tile_f16(f16 (*t)[33], const f16* __restrict__ src, int lds_, f16* __restrict__ dst, int ldd,
                                                          int rows, int cols, int bx, int by) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    t[r][tx] = (by + r < rows && bx + tx < cols) ? src[(size_t)(by + r) * lds_ + bx + tx] : (f16)0.f;
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (bx + r < cols && by + tx < rows) dst[(size_t)(bx + r) * ldd + by + tx] = t[tx][r];
}
