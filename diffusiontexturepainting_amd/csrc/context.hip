// The handle: its lifetime, weight staging and finalisation, the conditioning slots, options, profiling and the last stamp's records.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "engine.h"

int stamp_init(Ctx* c) {
  void* p;
  const size_t hw = (size_t)c->h * c->h, RR = (size_t)c->R * c->R;
  RC(ctx_persistent(c, c->maxB * hw * 4 * 4, &p, true)); c->x32 = (float*)p;
  RC(ctx_persistent(c, 3 * c->maxB * hw * 4 * 4, &p, true)); c->hist32 = (float*)p;
  RC(ctx_persistent(c, c->maxB * 4 * RR * 4, &p, true)); c->canvas32 = (float*)p;
  RC(ctx_persistent(c, 2 * c->maxB * RR * 4, &p, true)); c->alpha_tmp = (float*)p;
  RC(ctx_persistent(c, sizeof(StampParams), &p, true)); c->stamp_params = (StampParams*)p;
  RC(ctx_persistent(c, (size_t)DTP_MAX_SLOTS * 2 * 14 * 768 * 4, &p, true)); c->cond32 = (float*)p;
  RC(ctx_persistent(c, (size_t)DTP_MAX_SLOTS * 3 * RR * 4, &p, true)); c->brush32 = (float*)p;
  RC(ctx_persistent(c, 64 * sizeof(int), &p, true)); c->slot_map = (int*)p;
  RC(ctx_persistent(c, 256, &p, true)); c->finite_flag = (int*)p;
  RC(ctx_persistent(c, RR * 4, &p, true)); c->mesh_face_idx = (int*)p;
  return DTP_OK;
}

extern "C" {

int dtp_create(int device, int resolution, int max_batch, dtp_ctx** out) {
  if (!out || resolution < 64 || resolution % 8 || max_batch < 1 || max_batch > 64) {
    dtp_set_error("dtp_create: resolution must be a multiple of 8 and at least 64, 1 <= max_batch <= 64 (got resolution %d, max_batch %d)", resolution, max_batch);
    return DTP_ERR_ARG;
  }
  HIP_CHECK(hipSetDevice(device));
  Ctx* c = new Ctx();
  c->device = device; c->R = resolution; c->h = resolution / 8; c->maxB = max_batch;
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  c->num_cu = prop.multiProcessorCount;
  void* z;
  HIP_CHECK(hipMalloc(&z, 4096));
  HIP_CHECK(hipMemset(z, 0, 4096));
  c->zero = (f16*)z;
  for (int i = 0; i < 4; ++i) HIP_CHECK(hipEventCreate(&c->ev[i]));
  tune_cache_load(c);
  // the switches that shape a launch program (engine.h), read per context: set, and not "0"
  auto on = [](const char* name) { const char* e = getenv(name); return e && e[0] && e[0] != '0'; };
  c->fuse_reduce_gn = !on("DTP_NO_FUSE_REDUCE_GN"); c->dedupe_prefix = !on("DTP_NO_DEDUPE");
#ifdef DTP_EXPERIMENTAL
  c->fuse_gn_conv = on("DTP_GN_CONV");
#endif
  c->fuse_xattn = !on("DTP_NO_XATTN"); c->fold_gn_linear = !on("DTP_NO_FOLD_GN");
  c->conv_ws = !on("DTP_NO_WS"); c->conv_ws_vae = !on("DTP_NO_WS_VAE"); c->gemm_ws = on("DTP_GEMMWS");
  c->gn_epilogue = !on("DTP_NO_GN_EPILOGUE"); c->reduce_in_concat_gn = !on("DTP_NO_REDUCE_IN_CONCAT_GN"); c->gna_lnlin = !on("DTP_NO_GNA_LNLIN");
  c->tune_lnlin = !on("DTP_NO_LNLIN"); c->tune_halo3 = !on("DTP_NO_HALO3");
  c->xchain = !on("DTP_NO_XCHAIN"); c->xattn_tiles = !on("DTP_XATTN_CT1");
  if (const char* e = getenv("DTP_FFCHAIN")) c->ffchain = atoi(e);
  if (const char* e = getenv("DTP_UPS_PHASE")) c->ups_phase = std::min(std::max(atoi(e), 0), 3);
  *out = (dtp_ctx*)c;
  return DTP_OK;
}

void dtp_destroy(dtp_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  graphs_drop_all(c);
  journal_drop_ctx(c);
  delta_drop_ctx(c);
  mesh_drop_ctx(c);
  for (auto& s : c->staged) (void)hipFree(s.second.d);
  for (auto& s : c->refit_staged) (void)hipFree(s.second.d);
  for (int i = 0; i < 2; ++i) if (c->refit_ev[i]) (void)hipEventDestroy(c->refit_ev[i]);
  for (void* p : c->chunks) (void)hipFree(p);
  for (auto& b : c->pool.blocks) (void)hipFree(b.p);
  for (void* p : c->persistent) (void)hipFree(p);
  if (c->ws) (void)hipFree(c->ws);
  if (c->zero) (void)hipFree(c->zero);
  if (c->tune_thrash) (void)hipFree(c->tune_thrash);
  for (int i = 0; i < 4; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  delete c;
}

int dtp_load_tensor(dtp_ctx* ctx, const char* name, const float* data, int is_device, const int64_t* shape, int ndim) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !name || !data || ndim < 1 || ndim > 4) { dtp_set_error("dtp_load_tensor: bad argument"); return DTP_ERR_ARG; }
  if (c->finalized) { dtp_set_error("dtp_load_tensor: weights already finalized"); return DTP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(c->device));
  Staged s;
  s.n = 1;
  for (int i = 0; i < ndim; ++i) { s.shape.push_back(shape[i]); s.n *= (size_t)shape[i]; }
  HIP_CHECK(hipMalloc(&s.d, std::max<size_t>(s.n * 4, 16)));
  HIP_CHECK(hipMemcpy(s.d, data, s.n * 4, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  auto it = c->staged.find(name);
  if (it != c->staged.end()) { (void)hipFree(it->second.d); c->staged.erase(it); }
  c->staged.emplace(name, std::move(s));
  return DTP_OK;
}

int dtp_finalize_weights(dtp_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { dtp_set_error("dtp_finalize_weights: null handle"); return DTP_ERR_ARG; }
  if (c->finalized) { dtp_set_error("dtp_finalize_weights: already finalized"); return DTP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(c->device));
  dtp_gemm_init();
  dtp_conv_halo_init();
  dtp_gemm_wide_init();
  dtp_gemm_fp8_init();
  dtp_gemm_f8f8_init();
  dtp_xattn_init();
  dtp_lnlin_init();
  dtp_xchain_init();
  dtp_ffchain_init();
  dtp_conv_ws_init();
  dtp_gemm_ws_init();
  RC(load_unet_weights(c));
  RC(load_vae_weights(c));
  bool has_clip = false;
  for (auto& kv : c->staged)
    if (kv.first.rfind("clip.", 0) == 0) { has_clip = true; break; }
  if (has_clip) RC(load_imgenc_weights(c));
  HIP_CHECK(hipDeviceSynchronize());
  for (auto& s : c->staged) (void)hipFree(s.second.d);
  c->staged.clear();
  RC(stamp_init(c));
  c->finalized = true;
  return DTP_OK;
}

int dtp_set_conditioning_slot(dtp_ctx* ctx, int slot, const float* cond, const float* uncond, const float* brush, dtp_stream s_) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  if (!c || !c->finalized || !cond || !uncond || !brush) { dtp_set_error("dtp_set_conditioning: bad state/argument"); return DTP_ERR_STATE; }
  if (slot < 0 || slot >= DTP_MAX_SLOTS) { dtp_set_error("dtp_set_conditioning: slot %d outside 0..%d", slot, DTP_MAX_SLOTS - 1); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(c->device));
  float* dst = c->cond32 + (size_t)slot * 2 * 14 * 768;
  HIP_CHECK(hipMemcpyAsync(dst, cond, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dst + 14 * 768, uncond, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(c->brush32 + (size_t)slot * 3 * c->R * c->R, brush, (size_t)3 * c->R * c->R * 4, hipMemcpyDeviceToDevice, s));
  c->slot_set[slot] = true;
  c->slot_version[slot] = ++c->cond_version;
  return DTP_OK;
}

int dtp_set_conditioning(dtp_ctx* ctx, const float* cond, const float* uncond, const float* brush, dtp_stream s) {
  return dtp_set_conditioning_slot(ctx, 0, cond, uncond, brush, s);
}

int dtp_get_conditioning_slot(dtp_ctx* ctx, int slot, float* cond, float* uncond, dtp_stream s_) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  if (!c || slot < 0 || slot >= DTP_MAX_SLOTS || !c->slot_set[slot]) { dtp_set_error("dtp_get_conditioning: no brush set in slot %d", slot); return DTP_ERR_STATE; }
  const float* src = c->cond32 + (size_t)slot * 2 * 14 * 768;
  HIP_CHECK(hipMemcpyAsync(cond, src, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(uncond, src + 14 * 768, 14 * 768 * 4, hipMemcpyDeviceToDevice, s));
  return DTP_OK;
}

int dtp_get_conditioning(dtp_ctx* ctx, float* cond, float* uncond, dtp_stream s) { return dtp_get_conditioning_slot(ctx, 0, cond, uncond, s); }

int dtp_last_stamp_finite(dtp_ctx* ctx, int* finite) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !finite) return DTP_ERR_ARG;
  if (!c->finite_pending) { dtp_set_error("dtp_last_stamp_finite: the last stamp ran without the \"check_finite\" option"); return DTP_ERR_STATE; }
  HIP_CHECK(hipEventSynchronize(c->ev[3]));
  int flag = 0;
  HIP_CHECK(hipMemcpy(&flag, c->finite_flag, sizeof(int), hipMemcpyDeviceToHost));
  *finite = flag ? 0 : 1;
  return DTP_OK;
}

int dtp_last_stamp_times(dtp_ctx* ctx, float ms[3]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !ms) return DTP_ERR_ARG;
  HIP_CHECK(hipEventSynchronize(c->ev[3]));
  for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
  return DTP_OK;
}

int dtp_profile(dtp_ctx* ctx, int enable) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return DTP_ERR_ARG;
  HIP_CHECK(hipDeviceSynchronize());
  for (ProfRec& r : c->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  c->prof.clear();
  c->profile = enable != 0;
  return DTP_OK;
}

int dtp_profile_rows(dtp_ctx* ctx, dtp_prof_row* rows, int max_rows, int* n_rows) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rows || !n_rows) return DTP_ERR_ARG;
  HIP_CHECK(hipDeviceSynchronize());
  dtp_prof_row acc[PK_COUNT] = {};  // PK_COUNT kinds, see include/dtp.h
  for (int k = 0; k < PK_COUNT; ++k) acc[k].kind = k;
  for (const ProfRec& r : c->prof) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
    dtp_prof_row& a = acc[r.kind];
    a.launches += 1; a.ms += ms; a.flops += r.flops; a.bytes += r.bytes;
  }
  int n = 0;
  for (int k = 0; k < PK_COUNT && n < max_rows; ++k)
    if (acc[k].launches) rows[n++] = acc[k];
  *n_rows = n;
  return DTP_OK;
}

int dtp_profile_dump(dtp_ctx* ctx, const char* path) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !path) return DTP_ERR_ARG;
  HIP_CHECK(hipDeviceSynchronize());
  FILE* f = fopen(path, "w");
  if (!f) { dtp_set_error("dtp_profile_dump: cannot open %s", path); return DTP_ERR_ARG; }
  fprintf(f, "kind,us,tflops,algo_GBps,label\n");
  for (const ProfRec& r : c->prof) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    fprintf(f, "%d,%.2f,%.1f,%.1f,%s\n", r.kind, ms * 1e3, r.flops / (ms * 1e-3) / 1e12, r.bytes / (ms * 1e-3) / 1e9, r.label ? r.label : "");
  }
  fclose(f);
  return DTP_OK;
}

int dtp_set_option(dtp_ctx* ctx, const char* name, int value) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !name) return DTP_ERR_ARG;
  if (!strcmp(name, "scheduler")) {  // takes effect from the next stamp, which rebuilds the schedule tables
    if (value != DTP_SCHED_DDIM && value != DTP_SCHED_DPM && value != DTP_SCHED_LMSD) {
      dtp_set_error("dtp_set_option: scheduler %d is not one of DDIM = 0, DPM = 1, LMSD = 2", value);
      return DTP_ERR_ARG;
    }
    c->scheduler = value;
    return DTP_OK;
  }
  if (!strcmp(name, "use_graph")) { c->use_graph = value != 0; return DTP_OK; }
  if (!strcmp(name, "autotune")) { c->autotune = value != 0; return DTP_OK; }
  if (!strcmp(name, "check_finite")) { c->check_finite = value != 0; return DTP_OK; }
  if (!strcmp(name, "ups_phase")) {  // 1 = the tuner decides, 2 / 3 = tile 56 / 57 wherever it applies, 0 = never (the packing itself is chosen at dtp_create: $DTP_UPS_PHASE)
    if (value < 0 || value > 3) { dtp_set_error("dtp_set_option: ups_phase %d is not 0 .. 3", value); return DTP_ERR_ARG; }
    if (!c->unet_progs.empty() || !c->enc_progs.empty() || !c->dec_progs.empty()) {
      dtp_set_error("dtp_set_option: ups_phase must be chosen before the first launch program is built");
      return DTP_ERR_STATE;
    }
    if (value && !c->ups_phase && c->finalized) { dtp_set_error("dtp_set_option: ups_phase was 0 when the weights were packed"); return DTP_ERR_STATE; }
    c->ups_phase = value;
    return DTP_OK;
  }
  if (!strcmp(name, "fuse_gn_conv")) {
#ifndef DTP_EXPERIMENTAL
    if (value) { dtp_set_error("dtp_set_option: fuse_gn_conv is an experiment (slower: DESIGN.md 3.6) -- build with DTP_EXPERIMENTAL=1"); return DTP_ERR_ARG; }
#endif
    if (!c->unet_progs.empty() || !c->enc_progs.empty() || !c->dec_progs.empty()) {
      dtp_set_error("dtp_set_option: fuse_gn_conv must be chosen before the first launch program is built");
      return DTP_ERR_STATE;
    }
    c->fuse_gn_conv = value != 0;
    return DTP_OK;
  }
  if (!strcmp(name, "dedupe_prefix")) {  // programs are keyed by it: switching only affects which (cached) program a stamp uses
    c->dedupe_prefix = value != 0;
    graphs_drop_all(c);  // captured stages hold the old program's launches
    return DTP_OK;
  }
  // the fp8 options are parity-only (inside the 1e-2 gate at multiples of 64) and were never measured at the ragged
  // maps of a resolution that is a multiple of 8 but not of 64: refused there
  if (value && c->R % 64 && (!strcmp(name, "fp8_linear") || !strcmp(name, "fp8_operands") || !strcmp(name, "fp8_attention"))) {
    dtp_set_error("dtp_set_option: %s is parity-only and not offered at resolution %d (a multiple of 8 that is not a multiple of 64)", name, c->R);
    return DTP_ERR_STATE;
  }
  const struct { const char* name; bool Ctx::*flag; } fp8[] = {
      {"fp8_linear", &Ctx::fp8_linear}, {"fp8_operands", &Ctx::fp8_operands}, {"fp8_attention", &Ctx::fp8_attention}};
  for (const auto& o : fp8) {
    if (strcmp(name, o.name)) continue;
    if (!c->unet_progs.empty() && c->*o.flag != (value != 0)) {
      dtp_set_error("dtp_set_option: %s must be chosen before the first UNet program is built", o.name);
      return DTP_ERR_STATE;
    }
    c->*o.flag = value != 0;
    return DTP_OK;
  }
  dtp_set_error("dtp_set_option: unknown option '%s'", name);
  return DTP_ERR_ARG;
}

int dtp_last_stamp_info(dtp_ctx* ctx, int* unet_evals, int* graph_nodes) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return DTP_ERR_ARG;
  if (unet_evals) *unet_evals = c->last_evals;
  if (graph_nodes) *graph_nodes = c->last_nodes;
  return DTP_OK;
}

int dtp_last_stamp_unet_rows(dtp_ctx* ctx, int* rows) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rows) return DTP_ERR_ARG;
  *rows = c->last_unet_rows;
  return DTP_OK;
}

}  // extern "C"
