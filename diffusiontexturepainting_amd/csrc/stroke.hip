// Strokes on a device-resident texture (dtp_stroke): what the reference's Kit app does on the host around every stamp
// (kit_app/.../python/manager.py:229-271: crop the texture, u8 / 255, generate_raw, * 255 truncated, write where the stamp mask is > 0;
// the brush modes of :37-45,70) as two kernels around the existing stamp path, plus the host-only planner that finds the stamps of a
// stroke that may share one batched stamp.  Plain HIP, vector loads and stores only.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "stamp.h"

namespace {

__device__ __forceinline__ int pmod(long long a, int L) {  // a mod L reduced to 0 .. L - 1
  const int r = (int)(a % L);
  return r < 0 ? r + L : r;
}

// texel (ty, tx) of pixel (r, col) of window b: wrapped, or clipped (false: outside the texture)
__device__ __forceinline__ bool window_texel(const StrokeWins& w, int b, int r, int col, int H, int W, int wrap, int& ty, int& tx) {
  const long long y = (long long)w.y[b] + r, x = (long long)w.x[b] + col;
  if (wrap) { ty = pmod(y, H); tx = pmod(x, W); return true; }
  ty = (int)y; tx = (int)x;
  return y >= 0 && y < H && x >= 0 && x < W;
}

// texture u8 [H][W][4] -> canvas f32 [B][4][R][R] = texel / 255 (renderable_texture, manager.py:229-230; a real fp32 division).  A texel
// outside a non-wrapping texture gives 0 in all four channels (alpha 0 = unknown: inpainted, never pasted); in mode Overpaint rows
// [over_y, R - over_y) x columns [over_x, R - over_x) are 0 as well (overpaint_canvas, manager.py:37-39).  Thread = one texel: one 4-byte
// load, four stores that are contiguous across the wave.
__global__ __launch_bounds__(256) void stroke_gather_kernel(const unsigned int* __restrict__ tex, int H, int W, float* __restrict__ canvas,
                                                            int R, int B, StrokeWins w, int wrap, int over_y, int over_x) {
  const int HW = R * R;
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / HW), pix = (int)(i - (long long)b * HW);
    const int r = pix / R, col = pix - r * R;
    int ty, tx;
    bool take = window_texel(w, b, r, col, H, W, wrap, ty, tx);
    if (w.mode[b] == DTP_STROKE_OVERPAINT && r >= over_y && r < R - over_y && col >= over_x && col < R - over_x) take = false;
    const unsigned int t = take ? tex[(size_t)ty * W + tx] : 0u;
    float* cb = canvas + (size_t)b * 4 * HW + pix;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) cb[(size_t)ch * HW] = (float)((t >> (8 * ch)) & 0xffu) / 255.0f;
  }
}

// decoder output f32 [B][R][R][4] -> the texture, where mask[i][j] > 0 and the texel exists: RGB = the truncated u8 of the clamped value
// (finish_kernel's, composite = 0), A = 255 (manager.py:254,266-268); an Erase window (or dec == null) writes 0 to all four channels
// (:270).  One 4-byte store per texel; texels outside the mask are neither read nor written.
__global__ __launch_bounds__(256) void stroke_paste_kernel(const float* __restrict__ dec, const unsigned char* __restrict__ mask,
                                                           unsigned int* __restrict__ tex, int H, int W, int R, int B, StrokeWins w, int wrap) {
  const int HW = R * R;
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / HW), pix = (int)(i - (long long)b * HW);
    if (mask[pix] == 0) continue;
    const int r = pix / R, col = pix - r * R;
    int ty, tx;
    if (!window_texel(w, b, r, col, H, W, wrap, ty, tx)) continue;
    unsigned int t = 0u;
    if (dec && w.mode[b] != DTP_STROKE_ERASE) {
      t = 0xff000000u;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) t |= (unsigned int)finish_u8(finish_value(dec[i * 4 + ch])) << (8 * ch);
    }
    tex[(size_t)ty * W + tx] = t;
  }
}

// make_stamp_mask(R, margin), manager.py:42-45: 1 on [margin, R - margin)^2; every byte is written
__global__ void stroke_mask_kernel(unsigned char* __restrict__ mask, int R, int margin) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < R * R; i += gridDim.x * 256) {
    const int r = i / R, col = i - r * R;
    mask[i] = (r >= margin && r < R - margin && col >= margin && col < R - margin) ? 1 : 0;
  }
}

inline int nblk(long long total) { return (int)std::min<long long>((total + 255) / 256, 4096); }
inline int launch_ok() { return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP; }

bool known_mode(int m) { return m == DTP_STROKE_INPAINT || m == DTP_STROKE_ERASE || m == DTP_STROKE_OVERPAINT; }

// the planner's disjointness rule on one axis: windows [a, a + R) and [b, b + R) of an axis of length L
bool axis_disjoint(long long a, long long b, int R, int L, int wrap) {
  if (!wrap) return (a > b ? a - b : b - a) >= R;
  long long d = (a - b) % L;
  if (d < 0) d += L;
  return d >= R && d <= (long long)L - R;
}
bool windows_disjoint(const dtp_stroke_stamp& p, const dtp_stroke_stamp& q, int H, int W, int R, int wrap) {
  return axis_disjoint(p.x, q.x, R, W, wrap) || axis_disjoint(p.y, q.y, R, H, wrap);
}

// ONE implementation of the grouping rule for dtp_stroke_plan and dtp_stroke (arguments already checked)
void plan_groups(int H, int W, int R, int wrap, const dtp_stroke_stamp* st, int n, int max_group, int* group_of, int* n_groups) {
  int g = -1, first = 0;  // the current group and its first stamp
  for (int i = 0; i < n; ++i) {
    bool join = g >= 0 && i - first < max_group && st[i].mode != DTP_STROKE_ERASE && st[first].mode != DTP_STROKE_ERASE;
    for (int j = first; join && j < i; ++j) join = windows_disjoint(st[i], st[j], H, W, R, wrap);
    if (!join) { ++g; first = i; }
    group_of[i] = g;
  }
  if (n_groups) *n_groups = g + 1;
}

// the checks the planner and the stroke share; `who`: the entry point's name
int check_stamps(const char* who, int H, int W, int R, const dtp_stroke_stamp* st, int n) {
  if (!st) { dtp_set_error("%s: stamps is NULL", who); return DTP_ERR_ARG; }
  if (n < 1) { dtp_set_error("%s: n=%d stamps (at least 1)", who, n); return DTP_ERR_ARG; }
  if (R < 1 || H < R || W < R) { dtp_set_error("%s: a %d x %d texture is smaller than the %d x %d window", who, H, W, R, R); return DTP_ERR_ARG; }
  for (int i = 0; i < n; ++i)
    if (!known_mode(st[i].mode)) {
      dtp_set_error("%s: stamp %d has unknown mode %d (INPAINT = 0, ERASE = 1, OVERPAINT = 2)", who, i, st[i].mode);
      return DTP_ERR_ARG;
    }
  return DTP_OK;
}

// what the two op-level entry points check of their windows
int check_op_windows(const char* who, const void* a, const void* b, int H, int W, int R, int B, const int* xs, const int* ys, const int* modes,
                     StrokeWins& w) {
  if (!a || !b || !xs || !ys || B < 1 || B > DTP_STAMP_MAXB || R < 1 || H < R || W < R) {
    dtp_set_error("%s: bad argument (B=%d, max %d; H=%d W=%d R=%d)", who, B, DTP_STAMP_MAXB, H, W, R);
    return DTP_ERR_ARG;
  }
  for (int i = 0; i < B; ++i) {
    w.x[i] = xs[i]; w.y[i] = ys[i]; w.mode[i] = modes ? modes[i] : DTP_STROKE_INPAINT;
    if (!known_mode(w.mode[i])) { dtp_set_error("%s: window %d has unknown mode %d", who, i, w.mode[i]); return DTP_ERR_ARG; }
  }
  return DTP_OK;
}

}  // namespace

int dtp_launch_stroke_gather(const unsigned char* texture, int H, int W, float* canvas, int R, int B, const StrokeWins& wins, int wrap,
                             int over_y, int over_x, hipStream_t s) {
  hipLaunchKernelGGL(stroke_gather_kernel, dim3(nblk((long long)B * R * R)), dim3(256), 0, s, (const unsigned int*)texture, H, W, canvas, R, B,
                     wins, wrap, over_y, over_x);
  return launch_ok();
}

int dtp_launch_stroke_paste(const float* dec, const StrokePaste& p, int R, int B, hipStream_t s) {
  hipLaunchKernelGGL(stroke_paste_kernel, dim3(nblk((long long)B * R * R)), dim3(256), 0, s, dec, p.mask, (unsigned int*)p.texture, p.H, p.W, R,
                     B, p.wins, p.wrap);
  return launch_ok();
}

namespace {

// one group of a planned stroke: the storage its StampPlan points into
struct StrokeGroup {
  int first = 0, k = 0;
  bool erase = false;
  std::vector<uint64_t> seeds;
  std::vector<int> slots;
  std::vector<dtp_settings> st;
  StrokePaste paste;
  StampPlan plan;
};

}  // namespace

int stroke_default_mask(Ctx* c, int margin, hipStream_t s, const unsigned char** out) {
  auto it = c->stroke_masks.find(margin);
  if (it == c->stroke_masks.end()) {
    void* p;
    RC(ctx_persistent(c, (size_t)c->R * c->R, &p, false));
    hipLaunchKernelGGL(stroke_mask_kernel, dim3(nblk((long long)c->R * c->R)), dim3(256), 0, s, (unsigned char*)p, c->R, margin);
    RC(launch_ok());
    it = c->stroke_masks.emplace(margin, (unsigned char*)p).first;
  }
  *out = it->second;
  return DTP_OK;
}

extern "C" {

int dtp_stroke_plan(int H, int W, int R, int wrap, const dtp_stroke_stamp* stamps, int n, int max_group, int* group_of, int* n_groups) {
  RC(check_stamps("dtp_stroke_plan", H, W, R, stamps, n));
  if (!group_of) { dtp_set_error("dtp_stroke_plan: group_of is NULL (int[n])"); return DTP_ERR_ARG; }
  plan_groups(H, W, R, wrap != 0, stamps, n, max_group, group_of, n_groups);
  return DTP_OK;
}

int dtp_stroke(dtp_ctx* ctx, uint8_t* texture, int H, int W, const dtp_stroke_stamp* stamps, int n, const dtp_settings* st,
               const dtp_stroke_opts* o, const uint8_t* paste_mask, dtp_stream s_) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  // ---- every check, before anything is enqueued
  if (!c || !texture || !stamps || !st || !o) { dtp_set_error("dtp_stroke: NULL argument (ctx, texture, stamps, st and o are required)"); return DTP_ERR_ARG; }
  if (!c->finalized) { dtp_set_error("dtp_stroke: weights not finalized"); return DTP_ERR_STATE; }
  const int R = c->R, wrap = o->wrap != 0;
  RC(check_stamps("dtp_stroke", H, W, R, stamps, n));
  if (((uintptr_t)texture & 3) != 0) { dtp_set_error("dtp_stroke: texture must be 4-byte aligned (one RGBA texel per load)"); return DTP_ERR_ARG; }
  if (o->margin < 0 || o->margin >= R / 2) { dtp_set_error("dtp_stroke: margin=%d outside [0, %d)", o->margin, R / 2); return DTP_ERR_ARG; }
  for (int i = 0; i < n; ++i) {
    const dtp_stroke_stamp& t = stamps[i];
    if (t.mode == DTP_STROKE_OVERPAINT && (o->over_y < 1 || o->over_y >= R / 2 || o->over_x < 1 || o->over_x >= R / 2)) {
      dtp_set_error("dtp_stroke: stamp %d is an Overpaint stamp and over_y=%d / over_x=%d lie outside [1, %d)", i, o->over_y, o->over_x, R / 2);
      return DTP_ERR_ARG;
    }
    if (!wrap && (t.x <= -R || t.x >= W || t.y <= -R || t.y >= H)) {
      dtp_set_error("dtp_stroke: the window of stamp %d at (x=%d, y=%d) lies entirely outside the %d x %d texture", i, t.x, t.y, H, W);
      return DTP_ERR_ARG;
    }
    if (t.mode == DTP_STROKE_ERASE) continue;  // (runs no stamp: its slot and seed are unused)
    if (t.slot < 0 || t.slot >= DTP_MAX_SLOTS) { dtp_set_error("dtp_stroke: slot %d of stamp %d outside 0..%d", t.slot, i, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
    if (!c->slot_set[t.slot]) {
      dtp_set_error("dtp_stroke: stamp %d: no brush set in slot %d (call dtp_set_brush / dtp_set_conditioning)", i, t.slot);
      return DTP_ERR_STATE;
    }
  }
  std::vector<int> group_of(n);
  int n_groups = 0;
  plan_groups(H, W, R, wrap, stamps, n, std::min(o->max_group, c->maxB), group_of.data(), &n_groups);
  std::vector<StrokeGroup> groups(n_groups);
  for (int i = 0; i < n; ++i) {
    StrokeGroup& g = groups[group_of[i]];
    if (g.k++ == 0) g.first = i;
  }
  int evals = 0;
  for (StrokeGroup& g : groups) {
    g.erase = stamps[g.first].mode == DTP_STROKE_ERASE;
    g.paste.texture = texture; g.paste.H = H; g.paste.W = W; g.paste.wrap = wrap;
    for (int b = 0; b < g.k; ++b) {
      const dtp_stroke_stamp& t = stamps[g.first + b];
      g.paste.wins.x[b] = t.x; g.paste.wins.y[b] = t.y; g.paste.wins.mode[b] = t.mode;
      g.seeds.push_back(t.seed);
      g.slots.push_back(t.slot);
      g.st.push_back(*st);
    }
    if (g.erase) continue;
    // the stamp of the group, as dtp_stamp_seeded would stage it, with the two hooks
    StampPlan& p = g.plan;
    p.st = g.st.data(); p.B = g.k; p.slot_ids = g.slots.data(); p.strength = o->strength;
    p.seeded = true; p.seeds = g.seeds.data(); p.sample_vae = o->sample_vae != 0;
    p.canvas_staged = true;
    p.paste = [&g](const float* dec, int R, int B, hipStream_t q) { return dtp_launch_stroke_paste(dec, g.paste, R, B, q); };
    const int rc = stamp_plan(c, p);
    if (rc) {  // dtp_stamp_seeded's refusal and code, with the stamps it is about
      const std::string why = dtp_last_error();
      dtp_set_error("dtp_stroke: stamps %d..%d: %s", g.first, g.first + g.k - 1, why.c_str());
      return rc;
    }
    evals += p.E;
  }
  // ---- enqueue: per group gather -> one stamp of B = k -> paste; an Erase stamp only pastes.  The stream orders the groups.
  HIP_CHECK(hipSetDevice(c->device));
  const unsigned char* mask = paste_mask;
  if (!mask) RC(stroke_default_mask(c, o->margin, s, &mask));
  Journal* journal = journal_armed(c, texture, H, W);  // an open record guards this texture: the group's tiles are saved before its paste
  for (StrokeGroup& g : groups) {
    g.paste.mask = mask;
    if (journal) RC(journal_save_windows(journal, R, g.paste.wins.x, g.paste.wins.y, g.k, wrap, s));
    if (g.erase) { RC(dtp_launch_stroke_paste(nullptr, g.paste, R, g.k, s)); continue; }
    RC(dtp_launch_stroke_gather(texture, H, W, c->canvas32, R, g.k, g.paste.wins, wrap, o->over_y, o->over_x, s));
    RC(stamp_enqueue(c, g.plan, s));
  }
  c->last_stroke_stamps = n; c->last_stroke_groups = n_groups; c->last_stroke_evals = evals;
  return DTP_OK;
}

int dtp_last_stroke_info(dtp_ctx* ctx, int* stamps, int* groups, int* unet_evals) {
  Ctx* c = (Ctx*)ctx;
  if (!c || c->last_stroke_stamps < 0) { dtp_set_error("dtp_last_stroke_info: no stroke has run on this handle"); return DTP_ERR_STATE; }
  if (stamps) *stamps = c->last_stroke_stamps;
  if (groups) *groups = c->last_stroke_groups;
  if (unet_evals) *unet_evals = c->last_stroke_evals;
  return DTP_OK;
}

int dtp_op_stroke_gather(const uint8_t* texture, int H, int W, float* canvas, int R, int B, const int* xs, const int* ys, const int* modes,
                         int wrap, int over_y, int over_x, dtp_stream s) {
  StrokeWins w = {};
  RC(check_op_windows("dtp_op_stroke_gather", texture, canvas, H, W, R, B, xs, ys, modes, w));
  if (((uintptr_t)texture & 3) != 0) { dtp_set_error("dtp_op_stroke_gather: texture must be 4-byte aligned"); return DTP_ERR_ARG; }
  for (int i = 0; i < B; ++i)
    if (w.mode[i] == DTP_STROKE_OVERPAINT && (over_y < 1 || over_y >= R / 2 || over_x < 1 || over_x >= R / 2)) {
      dtp_set_error("dtp_op_stroke_gather: window %d is Overpaint and over_y=%d / over_x=%d lie outside [1, %d)", i, over_y, over_x, R / 2);
      return DTP_ERR_ARG;
    }
  return dtp_launch_stroke_gather(texture, H, W, canvas, R, B, w, wrap != 0, over_y, over_x, (hipStream_t)s);
}

int dtp_op_stroke_paste(const float* dec, const uint8_t* mask, uint8_t* texture, int H, int W, int R, int B, const int* xs, const int* ys,
                        const int* modes, int wrap, dtp_stream s) {
  StrokePaste p;
  RC(check_op_windows("dtp_op_stroke_paste", texture, mask, H, W, R, B, xs, ys, modes, p.wins));
  if (((uintptr_t)texture & 3) != 0) { dtp_set_error("dtp_op_stroke_paste: texture must be 4-byte aligned"); return DTP_ERR_ARG; }
  for (int i = 0; i < B; ++i)
    if (!dec && p.wins.mode[i] != DTP_STROKE_ERASE) {
      dtp_set_error("dtp_op_stroke_paste: dec is NULL and window %d is not an Erase window", i);
      return DTP_ERR_ARG;
    }
  p.texture = texture; p.mask = mask; p.H = H; p.W = W; p.wrap = wrap != 0;
  return dtp_launch_stroke_paste(dec, p, R, B, (hipStream_t)s);
}

}  // extern "C"
