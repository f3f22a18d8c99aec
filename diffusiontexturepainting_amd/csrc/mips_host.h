// The host-only arithmetic of the mip pyramid of a texture (include/dtp.h "the mip pyramid of a texture and a trilinear-filtered view":
// dtp_mip_layout, dtp_texture_mips): where the levels lie in their one buffer, every argument check of a build, and the
// texel rule in plain integers.  No device call, so the stand-alone sanitizer program (tools/mip_host_check.cpp) drives it directly,
// built by a plain C++ compiler.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/dtp.h"

#ifdef __HIPCC__
#define MIP_HD __host__ __device__
#else
#define MIP_HD
#endif

constexpr int MIP_MAX_TEX = 32768;   // as the strokes and the view: a texture side
constexpr int MIP_MAX_LEVELS = 16;   // 32768 -> 1 in 15 halvings, and level 0
constexpr int MIP_TILE = 64;         // a pass takes 64 x 64 source tiles ...
constexpr int MIP_PASS_LEVELS = 6;   // ... and writes 32^2, 16^2, 8^2, 4^2, 2^2, 1^2 of each

MIP_HD inline int mip_half(int n) { return (n + 1) / 2; }

// nullptr and *out written, or what is wrong (nothing written)
inline const char* mip_layout(int TH, int TW, dtp_mip_levels* out) {
  if (!out) return "NULL argument";
  if (TH < 1 || TW < 1 || TH > MIP_MAX_TEX || TW > MIP_MAX_TEX) return "the texture's TH and TW must lie in 1..32768";
  dtp_mip_levels m;
  memset(&m, 0, sizeof m);
  m.h[0] = TH; m.w[0] = TW;
  int l = 0;
  uint64_t at = 0;
  while (m.h[l] > 1 || m.w[l] > 1) {
    m.h[l + 1] = mip_half(m.h[l]); m.w[l + 1] = mip_half(m.w[l]);
    ++l;
    m.offset[l] = at;
    at += (uint64_t)4 * (uint64_t)m.h[l] * (uint64_t)m.w[l];
  }
  m.levels = l + 1;
  m.bytes = at;
  *out = m;
  return nullptr;
}

// Every check of dtp_texture_mips: nullptr and *lay written, or what is wrong.
inline const char* mips_check(const void* texture, int TH, int TW, const void* mips, uint64_t mips_bytes, dtp_mip_levels* lay) {
  if (!texture) return "NULL argument (texture is required)";
  if (const char* why = mip_layout(TH, TW, lay)) return why;
  if (lay->levels > 1 && !mips) return "NULL argument (mips is required for a texture larger than 1 x 1)";
  if (((uintptr_t)texture & 3) != 0 || ((uintptr_t)mips & 3) != 0) return "texture and mips must be 4-byte aligned";
  if (mips_bytes < lay->bytes) return "mips_bytes is smaller than the layout's bytes (dtp_mip_layout)";
  return nullptr;
}

// The texel rule: four RGBA texels (R in the low byte) of level l -> one of level l + 1.  Integers only.
MIP_HD inline uint32_t mip_texel(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
  const uint32_t a0 = t0 >> 24, a1 = t1 >> 24, a2 = t2 >> 24, a3 = t3 >> 24;
  const uint32_t A = (a0 + a1) + (a2 + a3);
  if (A == 0) return 0u;
  uint32_t out = ((A + 2u) >> 2) << 24;
  for (int ch = 0; ch < 3; ++ch) {
    const int s = 8 * ch;
    const uint32_t sum = ((t0 >> s) & 0xffu) * a0 + ((t1 >> s) & 0xffu) * a1 + ((t2 >> s) & 0xffu) * a2 + ((t3 >> s) & 0xffu) * a3;
    out |= ((sum + (A >> 1)) / A) << s;
  }
  return out;
}
