// Kernel-level C-ABI entry points (include/dtp.h, "kernel-level entry points") and the error slot.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

#include "../../include/dtp.h"
#include "common.h"

static thread_local char g_err[1024] = "";

void dtp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {
struct OpsScratch {
  f16* zero = nullptr;
  float* ws = nullptr;
  size_t ws_bytes = 0;
  int* geglu_map = nullptr;
  int geglu_map_n = 0;
  int num_cu = 256;
  bool init = false;
};
OpsScratch g_ops;
std::mutex g_ops_mu;

int ops_init() {
  if (g_ops.init) return DTP_OK;
  HIP_CHECK(hipMalloc(&g_ops.zero, 256));
  HIP_CHECK(hipMemset(g_ops.zero, 0, 256));
  hipDeviceProp_t prop;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  g_ops.num_cu = prop.multiProcessorCount;
  g_ops.init = true;
  return DTP_OK;
}

int ops_ws(size_t bytes) {
  if (bytes <= g_ops.ws_bytes) return DTP_OK;
  HIP_CHECK(hipDeviceSynchronize());
  if (g_ops.ws) HIP_CHECK(hipFree(g_ops.ws));
  g_ops.ws = nullptr;
  g_ops.ws_bytes = 0;
  HIP_CHECK(hipMalloc(&g_ops.ws, bytes));
  g_ops.ws_bytes = bytes;
  return DTP_OK;
}
}  // namespace

extern "C" {

int dtp_abi_version(void) { return DTP_ABI_VERSION; }
const char* dtp_last_error(void) { return g_err; }

// the problem a dtp_gemm_desc describes (dtp_op_gemm, dtp_op_conv_ups4, dtp_op_conv_ws_supported); the tile and the split are applied by the
// caller.  wfr4: the phase sets of an upsample2x conv (the descriptor has no field for them: it only grows by a new ABI version)
static GemmParams desc_params(const dtp_gemm_desc* d, const void* wfr4) {
  GemmParams p = {};
  p.A = (const f16*)d->A; p.W = (const f16*)d->W; p.C = d->C; p.bias = d->bias; p.R = (const f16*)d->R;
  p.zero = g_ops.zero;
  p.M = d->M; p.N = d->N; p.K = d->K;
  p.lda = d->lda; p.ldw = d->ldw; p.ldc = d->ldc; p.ldr = d->ldr;
  p.nkb = (d->K + 63) / 64;
  p.Hi = d->Hi; p.Wi = d->Wi; p.Ho = d->Ho; p.Wo = d->Wo; p.Cin = d->Cin; p.stride = d->stride; p.pad = d->pad;
  p.flags = d->flags | (d->conv ? GF_CONV3 : 0) | (d->upsample2x ? GF_UPS2 : 0);
  p.lns = d->lns; p.ln_eps = d->ln_eps;
  p.A2 = (const f16*)d->A2; p.lda2 = d->lda2; p.Cin2 = d->Cin2;
  p.batch = d->batch; p.a_bs = d->a_bs; p.w_bs = d->w_bs; p.c_bs = d->c_bs; p.r_bs = d->r_bs;
  p.bias_bs = d->bias_bs; p.lns_bs = d->lns_bs; p.sm_valid = d->sm_valid;
  p.st_out = d->st_out; p.st_in = d->st_in; p.st_parts = d->st_parts;
  if (p.batch > 1) p.st_rows = p.batch * p.M;  // statistics tables are [parts][batch * M][2]
  p.W8 = (const unsigned char*)d->W8; p.ldw8 = d->ldw8; p.a_scale = d->a_scale; p.w_scale = d->w_scale;
  p.Wfr = (const f16*)d->Wfr; p.Wfr4 = (const f16*)wfr4;
  p.gn_cpg = d->gn_cpg;
  return p;
}

static int op_gemm(dtp_gemm_desc* d, const void* wfr4, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  static bool halo_init = false;
  if (!halo_init) { dtp_conv_halo_init(); dtp_gemm_wide_init(); dtp_lnlin_init(); dtp_conv_ws_init(); dtp_gemm_ws_init(); halo_init = true; }
  GemmParams p = desc_params(d, wfr4);
  static bool fp8_init = false;
  if (!fp8_init) { dtp_gemm_fp8_init(); fp8_init = true; }
  if (p.ldw < p.nkb * 64) { dtp_set_error("gemm: ldw=%d smaller than padded K=%d", p.ldw, p.nkb * 64); return DTP_ERR_ARG; }
  int tile = 0;
  dtp_gemm_pick(p, &tile, g_ops.num_cu);
  if (d->tile >= 0) tile = d->tile;
  const DtpTile t = dtp_tile(tile);
  // the caller's splits; without them: the pick's K-slices for gemm_kernel tiles (batched problems always take those), four
  // column ranges for lnlin, unsplit for the rest
  int sp = t.split == SPLIT_COLS ? 4 : t.split == SPLIT_K ? p.splits : 1;
  if (d->splits >= 1 && (d->batch <= 1 || t.split != SPLIT_K)) sp = d->splits;
  if ((t.fam == TF_FP8) != (p.W8 != nullptr)) { dtp_set_error("gemm: tiles 24..28 and W8 go together"); return DTP_ERR_ARG; }
  if (t.fam == TF_HALO && !d->Wcb) { dtp_set_error("conv_halo: Wcb missing"); return DTP_ERR_ARG; }
  p.Wcb = (const f16*)d->Wcb;
  (void)dtp_tile_apply(p, tile, sp);  // an unrealisable split takes the nearest the tile has; wide and fp8 tiles stay unsplit
  rc = ops_ws(dtp_gemm_workspace_bytes(p));
  if (rc) return rc;
  p.part = g_ops.ws;
  if (p.flags & GF_ROWSTATS) d->st_parts_out = dtp_tile_row_parts(p, tile);
  return dtp_launch_tile(p, tile, (hipStream_t)s);
}

int dtp_op_gemm(dtp_gemm_desc* d, dtp_stream s) { return op_gemm(d, nullptr, s); }
int dtp_op_conv_ups4(dtp_gemm_desc* d, const void* wfr4, dtp_stream s) {
  if (!d || !d->conv || !d->upsample2x || !wfr4) { dtp_set_error("conv_ups4: a 3x3 conv over the 2x upsample and its phase weights"); return DTP_ERR_ARG; }
  return op_gemm(d, wfr4, s);
}

int dtp_op_gemm_f8f8(dtp_gemm_desc* d, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  static bool f8f8_init = false;
  if (!f8f8_init) { dtp_gemm_f8f8_init(); f8f8_init = true; }
  GemmParams p = {};
  p.A8 = (const unsigned char*)d->A8; p.lda8 = d->lda8;
  p.A2_8 = (const unsigned char*)d->A2_8; p.lda2_8 = d->lda2_8; p.Cin2 = d->A2_8 ? d->Cin2 : 0;
  p.W8 = (const unsigned char*)d->W8; p.ldw8 = d->ldw8;
  p.C = d->C; p.ldc = d->ldc; p.C8 = (unsigned char*)d->C8; p.ldc8 = d->ldc8;
  p.bias = d->bias; p.R = (const f16*)d->R; p.ldr = d->ldr;
  p.zero = g_ops.zero;
  p.M = d->M; p.N = d->N; p.K = d->K;
  p.flags = d->flags;
  p.st_out = d->st_out;
  p.a_scale = d->a_scale; p.w_scale = d->w_scale; p.c_scale = d->c_scale; p.a2_scale = d->a2_scale;
  p.splits = 1;
  const int tile = d->tile >= 0 ? d->tile : dtp_gemm_f8f8_pick(p, g_ops.num_cu);
  if (p.flags & GF_ROWSTATS) d->st_parts_out = (p.N + 127) / 128;
  return dtp_launch_gemm_f8f8(p, tile, (hipStream_t)s);
}

int dtp_op_quant_e4m3(const void* x, int ldx, void* y, int ldy, int K, float scale, int ln, const void* x2, int ldx2, void* y2, int ldy2,
                      int K2, float scale2, int ln2, int M, const float* st_in, int st_parts, float eps, dtp_stream s) {
  Quant8Params q = {};
  q.M = M; q.njobs = x2 ? 2 : 1;
  q.job[0] = Quant8Job{(const f16*)x, ldx, K, (unsigned char*)y, ldy, scale, ln};
  if (x2) q.job[1] = Quant8Job{(const f16*)x2, ldx2, K2, (unsigned char*)y2, ldy2, scale2, ln2};
  q.st_in = st_in; q.st_parts = st_parts; q.st_rows = M; q.eps = eps;
  return dtp_launch_quant8(q, (hipStream_t)s);
}

int dtp_op_pack_linear(const float* w, void* out, int N, int K, int ldw, int geglu, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  const int* map = nullptr;
  if (geglu) {
    if (N % 256) { dtp_set_error("pack_linear: GEGLU needs N %% 256 == 0"); return DTP_ERR_ARG; }
    // source row f (a-part) / N/2+f (gate) -> tile t=f/64: rows [128t, 128t+64) = a, [128t+64, 128t+128) = gate
    std::vector<int> h(N);
    for (int f = 0; f < N / 2; ++f) {
      h[f] = (f / 64) * 128 + (f % 64);
      h[N / 2 + f] = (f / 64) * 128 + 64 + (f % 64);
    }
    if (g_ops.geglu_map_n < N) {
      if (g_ops.geglu_map) HIP_CHECK(hipFree(g_ops.geglu_map));
      HIP_CHECK(hipMalloc(&g_ops.geglu_map, sizeof(int) * N));
      g_ops.geglu_map_n = N;
    }
    HIP_CHECK(hipMemcpyAsync(g_ops.geglu_map, h.data(), sizeof(int) * N, hipMemcpyHostToDevice, (hipStream_t)s));
    HIP_CHECK(hipStreamSynchronize((hipStream_t)s));
    map = g_ops.geglu_map;
  }
  return dtp_launch_pack_linear_weight(w, (f16*)out, N, K, ldw, map, (hipStream_t)s);
}

int dtp_op_quantize_w8(const void* w, int ldw, int K, int rows, void* out, int ldw8, float* w_scale, dtp_stream s) {
  if (!w || !out || !w_scale || (ldw8 & 127) || ldw8 < K) { dtp_set_error("quantize_w8: bad argument"); return DTP_ERR_ARG; }
  return dtp_quantize_weights_fp8((const f16*)w, ldw, K, rows, (unsigned char*)out, ldw8, w_scale, (hipStream_t)s);
}

int dtp_op_rowsum(const void* w, int ld, int K, float* out, int rows, dtp_stream s) {
  return dtp_launch_rowsum_f16((const f16*)w, ld, K, out, rows, (hipStream_t)s);
}

int dtp_op_pack_conv(const float* w, void* out, int Cout, int Cin, int Cin_pad, int taps, int ldw, dtp_stream s) {
  return dtp_launch_pack_conv_weight(w, (f16*)out, Cout, Cin, Cin_pad, taps, ldw, (hipStream_t)s);
}

int dtp_op_pack_conv_cb(const float* w, void* out, int Cout, int Cin, int ldw, dtp_stream s) {
  return dtp_launch_pack_conv_weight_cb(w, (f16*)out, Cout, Cin, ldw, (hipStream_t)s);
}

int dtp_op_pack_conv_ws(const float* w, const float* w1, void* out, int Cout, int Cin, int Cin2, dtp_stream s) {
  return dtp_launch_pack_conv_ws(w, w1, (f16*)out, Cout, Cin, Cin2, (hipStream_t)s);
}
int dtp_op_pack_linear_ws(const void* w, int ldw, void* out, int N, int K, dtp_stream s) {
  return dtp_launch_pack_linear_ws((const f16*)w, ldw, (f16*)out, N, K, (hipStream_t)s);
}
long long dtp_op_pack_linear_ws_elems(int N, int K) { return (long long)dtp_gemm_ws_packed_elems(N, K); }
long long dtp_op_pack_conv_ws_elems(int Cout, int Cin, int Cin2) { return (long long)dtp_conv_ws_packed_elems(Cout, Cin, Cin2); }
int dtp_op_pack_conv_ws_ups4(const float* w, void* out, int Cout, int Cin, dtp_stream s) {
  return dtp_launch_pack_conv_ws_ups4(w, (f16*)out, Cout, Cin, (hipStream_t)s);
}
long long dtp_op_pack_conv_ws_ups4_elems(int Cout, int Cin) { return (long long)dtp_conv_ws_ups4_packed_elems(Cout, Cin); }
int dtp_op_conv_ws_supported(const dtp_gemm_desc* d, const void* wfr4, int tile, int splits) {
  const DtpTile t = dtp_tile(tile);
  if (!d || t.fam != TF_CONVWS) return 0;
  return dtp_conv_ws_supported(desc_params(d, wfr4), t.var, splits < 1 ? 1 : splits) ? 1 : 0;
}

int dtp_op_groupnorm(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta, int B, int HW, int C,
                     int groups, float eps, int silu, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  rc = ops_ws(dtp_groupnorm_ws_bytes(B, HW, C, groups));
  if (rc) return rc;
  return dtp_launch_groupnorm(GnParams{(const f16*)x, ldx, (f16*)y, ldy, gamma, beta, B, HW, C, groups, eps, silu}, g_ops.ws, (hipStream_t)s);
}

int dtp_op_groupnorm_apply(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta, const float* partial, int nchunk,
                           int B, int HW, int C, int groups, float eps, int silu, dtp_stream s) {
  return dtp_launch_groupnorm_apply(GnParams{(const f16*)x, ldx, (f16*)y, ldy, gamma, beta, B, HW, C, groups, eps, silu}, partial, nchunk, (hipStream_t)s);
}

int dtp_op_reduce_groupnorm_cx(const float* part, int splits, const float* bias, const void* resid, void* conv_out, void* y, const float* gamma,
                               const float* beta, int B, int HW, int C, int groups, float eps, int silu, int cx, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  rc = ops_ws(dtp_groupnorm_ws_bytes(B, HW, C, groups));
  if (rc) return rc;
  // cx < C: the slabs hold the FIRST cx channels ([splits][B*HW][cx]); channels >= cx are already in conv_out (the other half of a
  // zero-copy concatenation) -- the round-5 form of the launch (engine.hip Builder::claim_reduce)
  if (cx <= 0 || cx > C) { dtp_set_error("reduce_groupnorm: cx %d outside (0, C = %d]", cx, C); return DTP_ERR_ARG; }
  const GnReduceSrc rd = {part, splits, (long long)B * HW * cx, cx, bias, (const f16*)resid, cx};
  return dtp_launch_reduce_groupnorm(GnParams{(const f16*)conv_out, C, (f16*)y, C, gamma, beta, B, HW, C, groups, eps, silu}, rd, cx, g_ops.ws, (hipStream_t)s);
}

int dtp_op_reduce_groupnorm(const float* part, int splits, const float* bias, const void* resid, void* conv_out, void* y, const float* gamma,
                            const float* beta, int B, int HW, int C, int groups, float eps, int silu, dtp_stream s) {
  return dtp_op_reduce_groupnorm_cx(part, splits, bias, resid, conv_out, y, gamma, beta, B, HW, C, groups, eps, silu, C, s);
}

int dtp_op_gn_fold_weights(const void* x, const void* W, int ldw, const float* bias, const float* gamma, const float* beta, int B, int HW, int C,
                           int Nout, int groups, float eps, void* Wout, float* bias_out, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  rc = ops_ws(dtp_groupnorm_ws_bytes(B, HW, C, groups));
  if (rc) return rc;
  const GnParams gp = {(const f16*)x, C, nullptr, 0, gamma, beta, B, HW, C, groups, eps, 0};
  rc = dtp_launch_groupnorm_stats(gp, g_ops.ws, nullptr, (hipStream_t)s);
  if (rc) return rc;
  const int rows = (Nout + 127) / 128 * 128;
  return dtp_launch_gn_fold_weights(gp, g_ops.ws, 0, (const f16*)W, ldw, bias, Nout, (f16*)Wout, (long long)rows * ldw, bias_out, rows, (hipStream_t)s);
}

// The statistics pass with the producing conv's split-K reduce riding in it (part: fp32 slabs [splits][B*HW][C], + bias, + residual; it
// writes x) or over x as it is (part == nullptr), then the apply pass from its partials: what gn_linear / gn_conv3 run on a claim
int dtp_op_groupnorm_stats_apply(const float* part, int splits, const float* bias, const void* resid, void* x, void* y, const float* gamma,
                                 const float* beta, int B, int HW, int C, int groups, float eps, int silu, dtp_stream s) {
  if (part && splits < 1) { dtp_set_error("groupnorm_stats_apply: %d slabs", splits); return DTP_ERR_ARG; }
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  rc = ops_ws(dtp_groupnorm_ws_bytes(B, HW, C, groups));
  if (rc) return rc;
  const GnParams gp = {(const f16*)x, C, (f16*)y, C, gamma, beta, B, HW, C, groups, eps, silu};
  const GnReduceSrc rd = {part, splits, (long long)B * HW * C, C, bias, (const f16*)resid, C};
  rc = dtp_launch_groupnorm_stats(gp, g_ops.ws, part ? &rd : nullptr, (hipStream_t)s);
  if (rc) return rc;
  return dtp_launch_groupnorm_apply(gp, g_ops.ws, dtp_groupnorm_stat_chunks(HW), (hipStream_t)s);
}

int dtp_op_gn_linear(const void* x, const void* W, int ldw, const float* bias, const float* gamma, const float* beta, int B, int HW, int C,
                     int Nout, int groups, float eps, void* y, float* st_out, int col_ranges, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  static bool init = false;
  if (!init) { dtp_lnlin_init(); init = true; }
  if (groups != 32) { dtp_set_error("gn_linear: 32 groups (got %d)", groups); return DTP_ERR_ARG; }
  rc = ops_ws(dtp_groupnorm_ws_bytes(B, HW, C, groups));
  if (rc) return rc;
  rc = dtp_launch_groupnorm_stats(GnParams{(const f16*)x, C, nullptr, 0, gamma, beta, B, HW, C, groups, eps, 0}, g_ops.ws, nullptr, (hipStream_t)s);
  if (rc) return rc;
  GemmParams p = {};
  p.A = (const f16*)x; p.lda = C; p.W = (const f16*)W; p.ldw = ldw; p.nkb = ldw / 64;
  p.M = HW; p.N = Nout; p.K = C; p.C = y; p.ldc = Nout;
  p.bias = bias; p.flags = (bias ? GF_BIAS : 0) | GF_GNAPPLY | (st_out ? GF_ROWSTATS : 0);
  p.batch = B; p.a_bs = (long long)HW * C; p.c_bs = (long long)HW * Nout; p.w_bs = 0; p.bias_bs = 0;
  p.st_out = st_out; p.st_rows = B * HW;
  p.gn_part = g_ops.ws; p.gn_gamma = gamma; p.gn_beta = beta; p.gn_nchunk = dtp_groupnorm_stat_chunks(HW); p.gn_cpg = C / groups; p.gn_eps = eps;
  p.zero = g_ops.zero;
  return dtp_launch_lnlin(p, col_ranges >= 1 ? col_ranges : 4, (hipStream_t)s);
}

int dtp_op_ffchain(const void* X, const void* W1, int ldw1, const float* lns1, const float* b1, const void* Wm, int ldwm, const float* bm,
                   const void* R, void* Out, int M, int C, float ln_eps, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  static bool init = false;
  if (!init) { dtp_ffchain_init(); init = true; }
  FfchainParams p = {};
  p.X = (const f16*)X; p.ldx = C; p.W1 = (const f16*)W1; p.ldw1 = ldw1; p.lns1 = lns1; p.b1 = b1;
  p.Wm = (const f16*)Wm; p.ldwm = ldwm; p.bm = bm; p.R = (const f16*)R; p.ldr = C; p.Out = (f16*)Out; p.ldo = C;
  p.M = M; p.C = C; p.ln_eps = ln_eps;
  return dtp_launch_ffchain(p, (hipStream_t)s);
}

int dtp_op_xchain(const void* A, const void* Wo, int ldwo, const float* bo, const void* Y, const void* W1, const float* b1, const float* lns1,
                  const void* W2, const float* b2, void* Y3, float* st_out, int S, int C, int N, int sm_valid, float ln_eps, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  static bool init = false;
  if (!init) { dtp_xchain_init(); init = true; }
  XchainParams p = {};
  p.A = (const f16*)A; p.lda = C; p.Wo = (const f16*)Wo; p.ldwo = ldwo; p.bo = bo; p.Y = (const f16*)Y; p.ldy = C;
  p.W1 = (const f16*)W1; p.w1_bs = (long long)128 * C; p.b1 = b1; p.lns1 = lns1;
  p.W2 = (const f16*)W2; p.w2_bs = (long long)((C + 127) / 128 * 128) * 128; p.b2 = b2;
  p.Y3 = (f16*)Y3; p.ldy3 = C; p.st_out = st_out; p.S = S; p.C = C; p.N = N; p.sm_valid = sm_valid; p.ln_eps = ln_eps;
  return dtp_launch_xchain(p, (hipStream_t)s);
}

int dtp_op_xattn_ct(const void* X, const void* W1, const float* b1, const float* lns1, const float* st_in, int st_parts, const void* W2, const float* b2,
                    const void* R, void* Y, float* st_out, int S, int C, int N, int sm_valid, float ln_eps, int ct, dtp_stream s) {
  std::lock_guard<std::mutex> lk(g_ops_mu);
  int rc = ops_init();
  if (rc) return rc;
  static bool init = false;
  if (!init) { dtp_xattn_init(); init = true; }
  XattnParams p = {};
  p.X = (const f16*)X; p.ldx = C; p.W1 = (const f16*)W1; p.w1_bs = (long long)128 * C; p.b1 = b1; p.lns1 = lns1;
  p.st_in = st_in; p.st_parts = st_parts; p.st_rows = N * S; p.ln_eps = ln_eps;
  p.W2 = (const f16*)W2; p.w2_bs = (long long)((C + 127) / 128 * 128) * 128; p.b2 = b2; p.R = (const f16*)R; p.ldr = C;
  p.Y = (f16*)Y; p.ldy = C; p.st_out = st_out; p.S = S; p.C = C; p.N = N; p.sm_valid = sm_valid; p.zero = (const f16*)g_ops.zero;
  p.ct = ct;  // column tiles per workgroup; < 1: the launcher's rule
  return dtp_launch_xattn(p, (hipStream_t)s);
}

int dtp_op_xattn(const void* X, const void* W1, const float* b1, const float* lns1, const float* st_in, int st_parts, const void* W2, const float* b2,
                 const void* R, void* Y, float* st_out, int S, int C, int N, int sm_valid, float ln_eps, dtp_stream s) {
  return dtp_op_xattn_ct(X, W1, b1, lns1, st_in, st_parts, W2, b2, R, Y, st_out, S, C, N, sm_valid, ln_eps, 0, s);
}

int dtp_op_layernorm(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta, int rows, int C,
                     float eps, dtp_stream s) {
  return dtp_launch_layernorm((const f16*)x, ldx, (f16*)y, ldy, gamma, beta, rows, C, eps, (hipStream_t)s);
}

int dtp_op_attention(const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo, int B, int H,
                     int Sq, int Skv, int D, int64_t qbs, int64_t kbs, int64_t vbs, int64_t obs, float scale, dtp_stream s) {
  AttnParams p;
  p.Q = (const f16*)Q; p.K = (const f16*)K; p.V = (const f16*)V; p.O = (f16*)O;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.B = B; p.H = H; p.Sq = Sq; p.Skv = Skv; p.D = D;
  p.qbs = qbs; p.kbs = kbs; p.vbs = vbs; p.obs = obs;
  p.scale = scale;
  return dtp_launch_attention(p, (hipStream_t)s);
}

int dtp_op_attention_dma(const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo, int B, int H,
                         int Sq, int Skv, int D, int64_t qbs, int64_t kbs, int64_t vbs, int64_t obs, float scale, int nw, dtp_stream s) {
  AttnParams p;
  p.Q = (const f16*)Q; p.K = (const f16*)K; p.V = (const f16*)V; p.O = (f16*)O;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.B = B; p.H = H; p.Sq = Sq; p.Skv = Skv; p.D = D;
  p.qbs = qbs; p.kbs = kbs; p.vbs = vbs; p.obs = obs;
  p.scale = scale;
  if (nw != 0 && nw != 4 && nw != 8) { dtp_set_error("attention_dma: nw %d (0 = the launcher's rule, 4, 8)", nw); return DTP_ERR_ARG; }
  if (!Q && !K && !V && !O) return dtp_attention_dma_supported(p) ? DTP_OK : DTP_ERR_ARG;  // a query: would the kernel take this problem?
  return dtp_launch_attention_dma(p, (hipStream_t)s, nw);
}

int dtp_op_attention_fp8(const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo, int B, int H,
                         int Sq, int Skv, int D, int64_t qbs, int64_t kbs, int64_t vbs, int64_t obs, float scale, float q_scale,
                         float v_scale, dtp_stream s) {
  AttnParams p;
  p.Q = (const f16*)Q; p.K = (const f16*)K; p.V = (const f16*)V; p.O = (f16*)O;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.B = B; p.H = H; p.Sq = Sq; p.Skv = Skv; p.D = D;
  p.qbs = qbs; p.kbs = kbs; p.vbs = vbs; p.obs = obs;
  p.scale = scale;
  return dtp_launch_attention_fp8(p, q_scale, v_scale, (hipStream_t)s);
}

int dtp_op_softmax_rows(const void* x, int ldx, void* y, int ldy, int rows, int cols, float scale, dtp_stream s) {
  return dtp_launch_softmax_rows((const f16*)x, ldx, (f16*)y, ldy, rows, cols, scale, (hipStream_t)s);
}

}  // extern "C"
