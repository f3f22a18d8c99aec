// Seeded stamp noise (dtp_stamp_seeded): standard normals as a pure function of (seed, draw, element) -- Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers) followed by Box-Muller.  One
// launch fills every draw of a stamp call straight into the stamp's staging buffers.  The bit generator is ONE __host__ __device__
// function: dtp_philox4x32 runs it on the CPU, the kernel on the GPU.
#include "engine.h"

namespace {

// One Philox round: (c0,c1,c2,c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped before rounds 2..10
__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ln u(w), u(w) = ((w >> 8) + 0.5) 2^-24.  k + 0.5 needs 25 significant bits from k = 2^23 on, where fp32 would round it (k = 2^24 - 1
// to u = 1, i.e. r = 0): that half goes through 1 - u = ((2^24 - k) - 0.5) 2^-24, which IS exact, and log1pf.  Both arguments are exact
// fp32 values, so the result is within the libm error of the real logarithm for every word.
__device__ __forceinline__ float log_u(uint32_t w) {
  const uint32_t k = w >> 8;
  if (k < (1u << 23)) return logf(((float)k + 0.5f) * 0x1p-24f);
  return log1pf(-(((float)((1u << 24) - k) - 0.5f) * 0x1p-24f));
}

// two words -> two normals: r cos(theta), r sin(theta), r = sqrt(-2 ln u(w0)), theta = 2 pi u(w1)
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * log_u(w0));
  const float theta = 6.283185307179586f * (((float)(w1 >> 8) + 0.5f) * 0x1p-24f);
  float sn, cs;
  sincosf(theta, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

// elements 4q .. 4q+3 of draw `draw` of the stamp seeded `seed`
__device__ __forceinline__ f32x4 stamp_noise4(uint64_t seed, uint32_t draw, uint64_t q) {
  const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32), draw, 0u}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  f32x4 z;
  float a, b;
  box_muller(w[0], w[1], a, b);
  z[0] = a; z[1] = b;
  box_muller(w[2], w[3], a, b);
  z[2] = a; z[3] = b;
  return z;
}

// Thread = one counter = four consecutive floats, one 16-byte store.  Job j < nd fills draw a.draw[j] of all B stamps at a.dst[j]
// ([B][4 Q] floats, dense): the counter index is the quad WITHIN the stamp, so neither b nor B reaches the generator.
__global__ __launch_bounds__(256) void philox_normal_kernel(NoiseArgs a, int nd, int B, long long Q) {
  const long long total = (long long)nd * B * Q;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long q = i % Q, jb = i / Q;
    const int b = (int)(jb % B), j = (int)(jb / B);
    *(f32x4*)(a.dst[j] + ((long long)b * Q + q) * 4) = stamp_noise4(a.seed[b], (uint32_t)a.draw[j], (uint64_t)q);
  }
}

}  // namespace

int dtp_launch_stamp_noise(const NoiseArgs& a, int nd, int B, long long Q, hipStream_t s) {
  const long long total = (long long)nd * B * Q;
  const int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(philox_normal_kernel, dim3(blocks), dim3(256), 0, s, a, nd, B, Q);
  return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP;
}

extern "C" {

int dtp_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) { dtp_set_error("dtp_philox4x32: null argument"); return DTP_ERR_ARG; }
  philox4x32_10(ctr, key, out);
  return DTP_OK;
}

int dtp_op_stamp_noise(uint64_t seed, int draw, float* out, long long n, dtp_stream s) {
  if (!out || n <= 0 || n % 4 != 0 || draw < 0 || draw > 3) {
    dtp_set_error("dtp_op_stamp_noise: bad argument (draw=%d outside 0..3, or n=%lld not a positive multiple of 4, or out is NULL)", draw, n);
    return DTP_ERR_ARG;
  }
  NoiseArgs a = {};
  a.seed[0] = seed;
  a.dst[0] = out;
  a.draw[0] = draw;
  return dtp_launch_stamp_noise(a, 1, 1, n / 4, (hipStream_t)s);
}

}  // extern "C"
