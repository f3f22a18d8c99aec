// The mip pyramid of a painted texture (dtp_mip_layout, dtp_texture_mips), written from the contract of include/dtp.h:
// alpha-weighted, in exact integers, so that unpainted texels (0,0,0,0) do not drag black into chart borders and the CPU restatement
// equals it byte for byte.  One pass takes 64 x 64-texel tiles of its source level: a workgroup loads its tile into LDS and writes that
// tile's part of up to six levels, reducing in LDS with a barrier between levels.  That works because the clamp rule keeps every deeper
// texel inside its 64-aligned tile: texel i of level l + 1 reads rows 2 i and min(2 i + 1, h - 1).  The passes start from levels 0, 6
// and 12: at most three launches.  Plain HIP: vector loads and stores only.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "engine.h"
#include "mips_host.h"

namespace {

// one pass: the source level and the levels it writes (n of them, 1..6); travels as a kernel argument
struct MipPass {
  const uint32_t* src;
  int hs, ws, n;
  uint32_t* dst[MIP_PASS_LEVELS];
  int w[MIP_PASS_LEVELS];  // their row pitches in texels
};

// where the levels of a tile lie in LDS: 64^2 at 0, then 32^2, 16^2, 8^2, 4^2, 2^2, 1
constexpr int MIP_LDS = 4096 + 1024 + 256 + 64 + 16 + 4 + 1;

__global__ __launch_bounds__(256) void mips_pass_kernel(MipPass p) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tex[MIP_LDS];
  const int t = threadIdx.x, col0 = blockIdx.x * MIP_TILE, row0 = blockIdx.y * MIP_TILE;
  // the tile: 64 rows of 16 groups of 4 texels; a row past the last is the last (any texel in bounds would do: every reduction clamps)
  const bool vec = (((uintptr_t)p.src & 15) == 0) && ((p.ws & 3) == 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = 256 * r + t, i = e >> 4, j = 4 * (e & 15);
    const int row = min(row0 + i, p.hs - 1), col = col0 + j;
    const uint32_t* line = p.src + (size_t)row * p.ws;
    uint4 v;
    if (vec && col + 3 < p.ws) {
      v = *(const uint4*)(line + col);
    } else {
      v.x = line[min(col, p.ws - 1)]; v.y = line[min(col + 1, p.ws - 1)];
      v.z = line[min(col + 2, p.ws - 1)]; v.w = line[min(col + 3, p.ws - 1)];
    }
    *(uint4*)&s_tex[64 * i + j] = v;
  }
  __syncthreads();
  int from = 0, side = MIP_TILE;               // the level being read: where it starts in LDS, its side there
  int lh = min(MIP_TILE, p.hs - row0), lw = min(MIP_TILE, p.ws - col0);  // ... and how much of it lies inside the texture
#pragma unroll
  for (int k = 0; k < MIP_PASS_LEVELS; ++k) {
    if (k >= p.n) break;  // (uniform)
    const int to = from + side * side, half = side >> 1;
    const int nh = mip_half(lh), nw = mip_half(lw);
    const int r0 = row0 >> (k + 1), c0 = col0 >> (k + 1);
    for (int e = t; e < half * half; e += 256) {
      const int i = e / half, j = e - i * half;
      if (i < nh && j < nw) {
        const int i0 = 2 * i, i1 = min(2 * i + 1, lh - 1), j0 = 2 * j, j1 = min(2 * j + 1, lw - 1);
        const uint32_t* s = s_tex + from;
        const uint32_t v = mip_texel(s[side * i0 + j0], s[side * i0 + j1], s[side * i1 + j0], s[side * i1 + j1]);
        s_tex[to + half * i + j] = v;
        p.dst[k][(size_t)(r0 + i) * p.w[k] + (c0 + j)] = v;
      }
    }
    __syncthreads();
    from = to; side = half; lh = nh; lw = nw;
  }
}

}  // namespace

extern "C" {

int dtp_mip_layout(int TH, int TW, dtp_mip_levels* out) {
  if (const char* why = mip_layout(TH, TW, out)) { dtp_set_error("dtp_mip_layout: %s", why); return DTP_ERR_ARG; }
  return DTP_OK;
}

int dtp_texture_mips(const uint8_t* texture, int TH, int TW, uint8_t* mips, uint64_t mips_bytes, dtp_stream s) {
  dtp_mip_levels lay;
  if (const char* why = mips_check(texture, TH, TW, mips, mips_bytes, &lay)) { dtp_set_error("dtp_texture_mips: %s", why); return DTP_ERR_ARG; }
  if (lay.levels == 1) return DTP_OK;  // a 1 x 1 texture is its own pyramid: nothing to launch
  for (int from = 0; from + 1 < lay.levels; from += MIP_PASS_LEVELS) {
    MipPass p;
    memset(&p, 0, sizeof p);
    p.src = from == 0 ? (const uint32_t*)texture : (const uint32_t*)(mips + lay.offset[from]);
    p.hs = lay.h[from]; p.ws = lay.w[from];
    p.n = lay.levels - 1 - from < MIP_PASS_LEVELS ? lay.levels - 1 - from : MIP_PASS_LEVELS;
    for (int k = 0; k < p.n; ++k) {
      p.dst[k] = (uint32_t*)(mips + lay.offset[from + 1 + k]);
      p.w[k] = lay.w[from + 1 + k];
    }
    hipLaunchKernelGGL(mips_pass_kernel, dim3((p.ws + MIP_TILE - 1) / MIP_TILE, (p.hs + MIP_TILE - 1) / MIP_TILE), dim3(256), 0, (hipStream_t)s, p);
  }
  if (hipGetLastError() != hipSuccess) { dtp_set_error("dtp_texture_mips: a kernel launch failed"); return DTP_ERR_HIP; }
  return DTP_OK;
}

}  // extern "C"
