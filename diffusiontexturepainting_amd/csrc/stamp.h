// What the stamp path (stamp.hip) shares with the stroke layer on top of it (stroke.hip): the plan of one stamp call, the kernel-argument
// records, and the device functions of the output conversion.
#pragma once
#include <functional>
#include <vector>

#include "engine.h"

// per-stamp values that travel as kernel ARGUMENTS (no host staging buffer to keep alive, no sync, nothing captured)
struct PadArgs { int lo[DTP_STAMP_MAXB], hi[DTP_STAMP_MAXB]; };
struct SlotArgs { int s[64]; };
// the windows of one stroke group: top-left texel (row y, column x) and DTP_STROKE_* mode of window b
struct StrokeWins { int x[DTP_STAMP_MAXB], y[DTP_STAMP_MAXB], mode[DTP_STAMP_MAXB]; };
// "paste instead of finish": where the decoded stamps of a group go (stroke_paste_kernel)
struct StrokePaste {
  unsigned char* texture = nullptr;     // u8 [H][W][4]
  const unsigned char* mask = nullptr;  // u8 [R][R]
  int H = 0, W = 0, wrap = 0;
  StrokeWins wins = {};
};

// inpaint_pipeline.py:148: the decoder's output as a clamped 0..1 value, and the truncating u8 conversion of handler.py:55-56.  ONE
// definition for finish_kernel (stamp.hip) and stroke_paste_kernel (stroke.hip).
__device__ __forceinline__ float finish_value(float dec) { return fminf(fmaxf(dec / 2.0f + 0.5f, 0.f), 1.f); }
__device__ __forceinline__ unsigned char finish_u8(float v) { return (unsigned char)(v * 255.0f); }

// ---------------------------------------------------------------- one plan per stamp call
// The entry points fill the first part; stamp_plan, which owns every argument check, resolves the rest; the stages only read it.
struct StampPlan {
  // the call (st, slot_ids: [B]; slot_ids null: slot 0 for every stamp)
  const float* canvas = nullptr;
  const dtp_settings* st = nullptr;
  void* out = nullptr;
  int B = 0;
  const int* slot_ids = nullptr;
  double strength = 1.0;
  // ... and its noise source: the caller's tensors (vae_eps / init_eps null: the distribution means), or with `seeded` one host seed per
  // stamp, from which the call's draws are generated into the staging buffers (noise.hip), and one switch for all the VAE draws
  const float *latents = nullptr, *vae_eps = nullptr, *init_eps = nullptr;
  const uint64_t* seeds = nullptr;
  bool seeded = false, sample_vae = false;
  // the two hooks of a stroke (dtp_stroke, dtp_mesh_stroke): the canvas is already in Ctx::canvas32 (the stroke's gather or render kernel
  // wrote it: `canvas` is unused), and the decoded stamps are pasted into a texture instead of converted into `out` (unused; composite and
  // output_u8 must be 0).  paste: a paste launcher, called with the decoder's output f32 [B][R][R][4], R, B and the stream
  bool canvas_staged = false;
  std::function<int(const float* dec, int R, int B, hipStream_t s)> paste;
  // resolved by stamp_plan
  bool use_eps = false, use_init = false;  // the encode stage samples the two VAE encodes / the init image's
  SlotArgs slots = {};
  PadArgs pads = {};
  int steps = 0, sched = 0, composite = 0, output_u8 = 0;
  // the start point: with `init` (strength < 1) x = a z0 + b latents from the init image, and the loop runs rows [row0, row0 + E) of
  // the (scheduler, steps) tables (the reference index t_start + i, minus steps_offset); E_full: the rows of the whole table
  bool init = false;
  float a = 0.f, b = 0.f;
  int row0 = 0, E = 0, E_full = 0;
  int tg_evals[DTP_STAMP_MAXB];
  StampCoefs coef = {};
  std::vector<int> ks;  // k_i: tg rows of evaluation i
};

// ---- stamp.hip: stamp_plan checks and resolves a plan without touching the device; stamp_enqueue puts a resolved plan on the stream
int stamp_plan(Ctx* c, StampPlan& p);
int stamp_enqueue(Ctx* c, const StampPlan& p, hipStream_t s);

// ---- stroke.hip: the two kernels of a stroke group, B <= DTP_STAMP_MAXB windows per launch (arguments checked by the callers)
int dtp_launch_stroke_gather(const unsigned char* texture, int H, int W, float* canvas, int R, int B, const StrokeWins& wins, int wrap,
                             int over_y, int over_x, hipStream_t s);
// dec f32 [B][R][R][4] (the VAE decoder's output, 3 channels used); null: every window is erased
int dtp_launch_stroke_paste(const float* dec, const StrokePaste& p, int R, int B, hipStream_t s);
// make_stamp_mask(R, margin) of the handle, u8 [R][R] on the device; the first use of a margin allocates and fills it
int stroke_default_mask(Ctx* c, int margin, hipStream_t s, const unsigned char** out);
