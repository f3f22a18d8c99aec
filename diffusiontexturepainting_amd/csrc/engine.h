// Host-side engine of libdtp: weight staging/packing, static activation planning and the
// launch programs of the three networks.  One Ctx = one GPU; not thread-safe (include/dtp.h).
#pragma once
#include <deque>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/dtp.h"
#include "common.h"

#define RC(x)            \
  do {                   \
    int rc_ = (x);       \
    if (rc_) return rc_; \
  } while (0)

struct Staged {
  float* d = nullptr;  // device fp32
  std::vector<int64_t> shape;
  size_t n = 0;
};

struct ConvW {  // 3x3 (taps = 9) or 1x1 (taps = 1) convolution / any Linear (taps = 1)
  f16* w = nullptr;
  f16* wcb = nullptr;  // 3x3 only: channel-block-major packing for conv_halo_kernel (Cin % 64 == 0, no fused shortcut)
  f16* wfr = nullptr;  // UNet only: MFMA-fragment-order packing -- of a 3x3 conv for convws_kernel (conv_ws.hip; Cin % 64 == 0, + the fused shortcut),
                       // of a Linear for gemmws_kernel (gemm_ws.hip; K % 64 == 0)
  f16* wfr4 = nullptr; // upsampler convs (GF_UPS2) only: the four phase sets of collapsed 2x2 weights (load_conv_ups4; conv_ws.hip tile ids 56 / 57)
  float* b = nullptr;  // fp32 bias (may be null)
  float* lns = nullptr;  // LayerNorm folded in: row sums of the packed weights (GF_LNFOLD)
  int cout = 0, cin = 0 /* padded */, cin_true = 0, taps = 1, K = 0, ldw = 0;
  int cin2 = 0;  // >0: a 1x1 shortcut conv over cin2 channels is fused as a 10th tap (K = 9*cin + cin2)
  unsigned char* w8 = nullptr;  // Linear only, option fp8_linear: per-tensor e4m3 copy of `w` [rows][ldw8] (K padded to 128)
  int ldw8 = 0;
  float w8_scale = 1.f;
};
struct NormW {
  float *g = nullptr, *b = nullptr;
  int c = 0;
};

// NHWC fp16 view
struct T {
  f16* p = nullptr;
  int B = 0, H = 0, W = 0, C = 0, ld = 0;
  long long rows() const { return (long long)B * H * W; }
};

// e4m3 view [rows][ld] bytes (option fp8_operands): value = byte * scale, scale = *scale_host when calibrated (read at enqueue time,
// like every fp8 scale), `scale` otherwise; amax_slot1 - 1 = the calibration slot its producer measures into (0: fixed scale)
struct T8 {
  unsigned char* p = nullptr;
  int B = 0, H = 0, W = 0, C = 0, ld = 0;
  const float* scale_host = nullptr;
  float scale = 1.f;
  int amax_slot1 = 0;
  long long rows() const { return (long long)B * H * W; }
  float now() const { return scale_host ? *scale_host : scale; }
};

struct Ctx;

// A launch program: a flat list of closures bound to statically planned buffers.
using Op = std::function<int(hipStream_t, int /*step*/)>;
struct ProfRec {
  int kind;
  double flops, bytes;
  hipEvent_t e0, e1;
  const char* label;  // owned by the closure's std::string (lives as long as the program)
};
// the split-K GEMM pushed last (if nothing was pushed after it): a GroupNorm consuming its output folds the reduce in
struct LastGemm {
  bool valid = false;
  GemmParams p;
  int tile = 0, bias_step_off = -1;
  size_t op_index = 0;
  int kind = 0;
  double flops = 0, bytes = 0;
  std::string label;
};
struct Prog {
  std::vector<Op> ops;
  LastGemm last_gemm;
  int run(hipStream_t s, int step) const {
    for (const Op& o : ops) RC(o(s, step));
    return DTP_OK;
  }
};

struct ResW {
  NormW n1, n2;
  ConvW c1, c2, sc;
  bool has_sc = false;
  int temb_off = -1;  // offset of this block's (conv1.bias + time_emb_proj(...)) slice in the step-bias table
};
struct XfW {
  NormW gn, ln1, ln2, ln3;
  ConvW proj_in, qkv, out1, q2, kv2, out2, ff1;
  ConvW ff2_proj;  // ff.net.2 and proj_out merged (load_linear_pair): [f | y3] -> block output in one GEMM
  int kv_index = -1;  // which cross-attention K/V buffer
  f16* q2T = nullptr; // LayerNorm-folded to_q of the cross-attention, transposed and packed: [up(C,128)][C] (rows = input channel)
};
struct VaeAttnW {
  NormW gn;
  ConvW qk, out;
  f16* wv = nullptr;  // [512][512] plain fp16 (used as the activation-side operand: V^T = Wv x^T)
  float* bv = nullptr;
};

// ---- LoRA refit (lora_refit.hip).  The three job records are what the grouped kernels read from a device table.
struct LoraRefitJob {  // one target matrix: dst rows [row0, row0 + N) x columns [0, K) = f16((base + scale * up @ down) * gamma[k])
  const float *base, *up, *down;  // f32 [N][K], [N][rank], [rank][K]; rank == 0: up / down unused (the matrix becomes its base)
  const float* gamma;             // LayerNorm gain folded into the columns, or null
  const float* beta;              // LayerNorm bias: wbeta[n] = 0 + sum_k (base + scale * up @ down)[n][k] * beta[k] (the folded bias b'), or null
  float* wbeta;                   // [N], the rows of the stacked bias this matrix owns
  f16* dst;                       // the packed buffer [>= roundup(row0 + N, 128)][ldw]
  int rank, N, K, row0, ldw;
};
struct RowsumJob { const f16* w; float* out; int ld, K, rows; };                    // out[r] = sum_k w[r][k] (`lns`)
struct TransposeJob { const f16* src; f16* dst; int lds, ldd, rows, cols; };        // dst[c][r] = src[r][c] (`q2T`)
struct RefitTarget {  // host side: a LoRA-targetable matrix and where every program reads it from
  std::string name;   // staged name of its weight, "unet.<module>.<proj>.weight"
  LoraRefitJob job;   // base / gamma / beta / wbeta / dst / N / K / row0 / ldw filled at finalize; up / down / rank per refit
};

struct UNetW {
  ConvW conv_in, conv_out, t1, t2, tproj;  // tproj: all 22 time_emb_proj stacked
  NormW norm_out;
  ResW down_res[4][2], mid_res[2], up_res[4][3];
  XfW down_xf[3][2], mid_xf, up_xf[4][3];
  ConvW down_conv[3], up_conv[3];
  int temb_total = 0;
};
struct VaeW {
  ConvW enc_in, enc_out, dec_in, dec_out;
  ResW enc_res[4][2], enc_mid[2], dec_mid[2], dec_res[4][3];
  ConvW enc_down[3], dec_up[3];
  VaeAttnW enc_attn, dec_attn;
  NormW enc_norm_out, dec_norm_out;
  float *quant_w = nullptr, *quant_b = nullptr, *pquant_w = nullptr, *pquant_b = nullptr;  // fp32 8x8 / 4x4
};
struct ClipLayerW {
  NormW ln1, ln2;
  ConvW qkv, out, fc1, fc2;
};
struct PencBlockW {
  NormW n1, n3;
  ConvW qkv, out, ff1, ff2;
};
struct ImgEncW {
  ConvW patch;  // 32x32 s32 conv as a [768][3072] GEMM
  float *cls_pos = nullptr;   // class_embedding + pos[0]   fp32 [768]
  float *pos = nullptr;       // pos[1..49] fp32 [49][768]
  NormW pre_ln, post_ln, final_ln;
  ClipLayerW layers[12];
  PencBlockW blocks[3][4];
  ConvW proj_out;
  float* uncond = nullptr;    // [14][768]
  float* pos_emb = nullptr;   // [14][768] (image_encoder.py:54-56)
  bool present = false;
};

struct Pool {
  struct Block { char* p; size_t bytes; bool free; };
  std::vector<Block> blocks;
  size_t total = 0;
};

// fp8 calibration (configs[4]): every fp8 problem whose activation operand is not LayerNorm'd gets its scale from the absolute maximum
// its operand reached in one evaluation of the program (Ctx::calibrating: the ops also launch dtp_launch_amax_f16 on their inputs)
struct Fp8Cal {
  int kind = 0;            // 0: Linear / 1x1 conv (slot0 = A [| A2]), 1: self-attention (slot0 .. slot0 + 2 = Q, K, V)
  int slot0 = 0;
  float* s0 = nullptr;     // Linear: a_scale; attention: q_scale
  float* s1 = nullptr;     // attention: v_scale
  float softmax_scale = 1.f;
};
constexpr int DTP_FP8_SLOTS = 2048;
constexpr float DTP_FP8_LN_A_SCALE = 0.125f;  // LayerNorm'd operands: |x| <= sqrt(K - 1) < 36 -> x * 8 < 448 never clips, three more octaves above the subnormals
constexpr float DTP_FP8_MARGIN = 2.0f;        // head-room over the calibration evaluation's absolute maximum
constexpr int DTP_FP8_OPERANDS_MIN_K = 1280;  // option fp8_operands: transformer Linears with K >= this contract two e4m3 operands (gemm_f8f8.hip)

struct UNetProg {
  int N = 0;          // UNet batch (2B + k: k texture-guided rows, 0 <= k <= B)
  size_t cal_begin = 0, cal_end = 0;  // this program's records in Ctx::fp8_cals
  bool fp8_calibrated = false;
  Prog kv, main;
  f16* in16 = nullptr;     // [N][h][w][16] input (latent 0-3, mask 4, masked latents 5-8, zero 9-15)
  f16* ctx16 = nullptr;    // [N][14][768]
  float* out32 = nullptr;  // [N][h][w][4]
  std::vector<f16*> kvbuf; // 16 x [N*14][2C]
  // Cross-attention against the 14 context tokens, fused algebraically: per sample n and block i
  //   xW1[i][n] [8*16][C]   = (scale * K_n,h,j restricted to head h) . Wq'      scores = LN2(x) . xW1^T   (+ xb1, LN fold via xl1)
  //   xW2[i][n] [C][8*16]   = Wo . (V_n,h,j restricted to head h)^T              out    = softmax_j(scores) . xW2^T + bo + x
  // both recomputed once per stamp by the `kv` program; the per-evaluation work is two small grouped GEMMs per block.
  std::vector<f16*> xW1, xW2;
  std::vector<float*> xb1, xl1;
  f16 *kexp = nullptr, *vexp = nullptr;  // scratch [N*128][1280]
  // validity of ctx16 / the per-stamp cross-attention matrices: the layout [uncond x B | cond x B | cond x k] depends on the
  // (B, k) split, not only on N = 2B + k (B=2,k=2 and B=3,k=0 share a program when the prefix is not de-duplicated)
  unsigned long long kv_ver = 0;
  int kv_B = 0, kv_k = 0;
  std::vector<int> kv_slots;                       // conditioning slot of every cond row [B + n] the K/V were built for (B + k entries)
  std::vector<unsigned long long> kv_slot_ver;     // ... and the version of that slot at the time
};
struct VaeEncProg {
  int B = 0;
  Prog main;
  f16* in8 = nullptr;       // [B][R][R][8]
  float* moments = nullptr; // [B][h][w][8] (conv_out output, before quant_conv)
};
struct VaeDecProg {
  int B = 0;
  Prog main;
  f16* in8 = nullptr;     // [B][h][w][8] (after post_quant_conv)
  float* out32 = nullptr; // [B][R][R][4] (3 used)
};

struct StampBufs {  // per-batch persistent staging of dtp_stamp
  float *masks = nullptr, *ml = nullptr, *lat = nullptr, *eps = nullptr;
  bool three = false;  // ml / eps hold three slabs (the init-image rows of a strength < 1 stamp), not two
};
struct IencBufs {  // brush-encoder program + buffers (built on the first dtp_set_brush)
  float* img224 = nullptr;
  f16* patchA = nullptr;
  Prog prog;
  f16* out16 = nullptr;  // [14][768] final embeddings (f16)
  bool built = false;
};

struct StampGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int nodes = 0;
  unsigned long long used = 0;  // Ctx::graph_clock at the last replay (LRU of the denoise-loop graphs)
};
// What a captured stage of a stamp depends on: two calls replay the same graph exactly when every field agrees.  The encode key carries
// neither the strength value nor the scheduler (read from the parameter block); the fields a stage does not use stay 0.
struct StageKey {
  int stage = 0;  // 1 = encode, 2 = denoise loop, 3 = decode
  int B = 0;
  int k0 = 0;                                                   // encode: tg rows of the first program
  bool vae_eps = false, init_image = false, init_eps = false;   // encode: VAE draws used, init-image slab (strength < 1) and its draw
  int sched = 0, steps = 0, row0 = 0;                           // loop
  std::vector<int> tg_profile;                                  // loop: tg_evals by rank
  bool operator<(const StageKey& o) const {
    return std::tie(stage, B, k0, vae_eps, init_image, init_eps, sched, steps, row0, tg_profile) <
           std::tie(o.stage, o.B, o.k0, o.vae_eps, o.init_image, o.init_eps, o.sched, o.steps, o.row0, o.tg_profile);
  }
};
// Batches of stamps with different guidance settings produce many loop profiles: beyond this many captured loop graphs per context the
// least recently replayed one is destroyed.
constexpr int DTP_LOOP_GRAPH_CAP = 16;

// Device parameter block the captured stamp kernels read.  The per-stamp part is written by a kernel whose ARGUMENTS carry the
// values (set_header_kernel): dtp_stamp never stages through host memory, and a captured loop is replayed for any cfg / tg values.
constexpr int DTP_STAMP_MAXB = 64;  // = the largest max_batch dtp_create accepts
struct StampCoefs {
  float cfg[DTP_STAMP_MAXB], tg[DTP_STAMP_MAXB];  // per stamp: cfg_weight, tg_weight
  int order[DTP_STAMP_MAXB];  // the UNet's texture-guided row 2B + j belongs to stamp order[j] (stamps by descending tg_evals)
  int rank[DTP_STAMP_MAXB];   // inverse of order: stamp b owns tg row 2B + rank[b] while rank[b] < k (k = tg rows of the program)
};
// the start point of a strength < 1 stamp (dtp_stamp_strength): x = a z0 + b latents, then scale_model_input of row `row`
struct StampStrength {
  float a, b;
  int row;  // start row in the schedule tables: t_start - steps_offset
  int pad_;
};
struct StampParams {
  StampCoefs coef;
  StampStrength strength;
  float sched[DTP_SCHED_ROW * 1000];  // per evaluation: the scheduler's coefficient row (dtp_scheduler_tables, include/dtp.h)
  float in_scale[1001];               // per evaluation: scale_model_input of the latent channels (entry E: 1)
  float init_sigma;                   // init_noise_sigma: the initial latent is latents * init_sigma
};

struct Ctx {
  int device = 0, R = 0, h = 0, maxB = 1, num_cu = 256;
  bool finalized = false;
  std::unordered_map<std::string, Staged> staged;

  // weight arena (zero-initialised chunks, bump allocated)
  std::vector<void*> chunks;
  char* cur = nullptr;
  size_t cur_left = 0, arena_total = 0;
  Pool pool;
  std::vector<void*> persistent;  // dedicated buffers (freed at destroy)
  f16* zero = nullptr;
  float* ws = nullptr;            // shared split-K / GroupNorm workspace
  size_t ws_bytes = 0, ws_need = 0;

  UNetW unet;
  VaeW vae;
  ImgEncW ienc;

  // programs keyed by batch
  std::map<int, UNetProg> unet_progs;  // key = N * 128 + dupB (dupB = samples filled by duplication, 0 = none)
  std::map<int, VaeEncProg> enc_progs;
  std::map<int, VaeDecProg> dec_progs;

  // step-bias table for the current step set: fp32 [nsteps][temb_total]
  float* temb_table = nullptr;
  int temb_rows = 0;         // capacity
  f16* temb_sin = nullptr;   // [rows][320]
  f16 *temb_h1 = nullptr, *temb_h2 = nullptr;  // [rows][1280]
  int sched_steps = -1;      // step count the table/coefficients were built for
  int sched_kind = -1;       // ... and scheduler (DTP_SCHED_*)
  int scheduler = DTP_SCHED_DDIM;  // option "scheduler": the sampler of the next stamp

  // conditioning
  // conditioning SLOTS: one brush per slot (a client of the multi-client server); slot 0 is what the single-brush entry
  // points use.  cond32 [DTP_MAX_SLOTS][2][14][768] (cond, uncond), brush32 [DTP_MAX_SLOTS][3][R][R]
  float* cond32 = nullptr;
  float* brush32 = nullptr;
  bool slot_set[DTP_MAX_SLOTS] = {};
  unsigned long long slot_version[DTP_MAX_SLOTS] = {};  // bumped by every (re)definition of the slot
  unsigned long long cond_version = 0;                  // bumped by every change of any slot
  int* slot_map = nullptr;   // device int[maxB]: conditioning slot of stamp b of the stamp batch being processed

  // stamp state
  float* x32 = nullptr;       // [maxB][h][w][4] current latent (fp32, NHWC)
  float* hist32 = nullptr;    // [3][B][h][w][4] sampler history of a B-stamp batch (DPM: previous x0; LMSD: the last three derivatives)
  float* canvas32 = nullptr;  // [maxB][4][R][R] copy of the canvas (for compositing inside the graph-free tail)
  float* alpha_tmp = nullptr; // dilation scratch [2][maxB][R][R]
  StampParams* stamp_params = nullptr;  // device: per-stamp guidance weights + row map, per-step DDIM coefficients
  std::map<int, StampBufs> stamp_bufs;  // keyed by stamp batch B; the buffers live in `persistent` and die with the context
  IencBufs ienc_bufs;
  int* finite_flag = nullptr;     // device: set to 1 by the post-loop finiteness check ("check_finite" option)
  bool check_finite = false;
  bool dedupe_prefix = true;      // uncond and cond branches share the UNet prefix up to the first cross-attention ($DTP_NO_DEDUPE=1: off, A/B)
  bool fuse_gn_conv = false;      // GroupNorm + SiLU applied on the halo conv's staged input patch (GF_GNAPPLY).  OFF: measured +4.9 ms per
                                  // stamp (the normalisation costs every workgroup ~40 % -- DESIGN.md 3.6); option "fuse_gn_conv" / $DTP_GN_CONV=1
  bool fuse_xattn = true;         // the two grouped GEMMs of a cross-attention as one launch (xattn.hip; $DTP_NO_XATTN=1: off, A/B)
  bool fold_gn_linear = true;     // transformer GroupNorm folded into per-sample proj_in weights at HW >= 1024 ($DTP_NO_FOLD_GN=1: off, A/B)
  bool fuse_reduce_gn = true;     // fold a split-K conv's reduce into the GroupNorm that consumes it ($DTP_NO_FUSE_REDUCE_GN=1: off, A/B)
  bool pack_ws = false;           // load_conv also builds the fragment-order packing (set while the UNet's / VAE's weights load, from the two below)
  bool conv_ws = true, conv_ws_vae = true;  // weight-streaming conv: packing + tuner candidates / the VAE's packing ($DTP_NO_WS=1 / $DTP_NO_WS_VAE=1: off, A/B)
  int ups_phase = 1;              // phase form of the upsampler convs: 0 = no phase packing, 1 = packed, a tuner candidate, 2 / 3 = tile 56 / 57 forced
                                  // wherever it applies ($DTP_UPS_PHASE, option "ups_phase": tests, A/B)
  bool gemm_ws = false;           // fragment-order packing of the Linears for gemmws_kernel, tile 55 ($DTP_GEMMWS=1: on, A/B)
  bool gn_epilogue = true;        // GroupNorm statistics from the producing conv's epilogue (Builder::claim_stats; $DTP_NO_GN_EPILOGUE=1: off, A/B)
  bool reduce_in_concat_gn = true;  // ... the split-K reduce folded into a GroupNorm over a concatenation too ($DTP_NO_REDUCE_IN_CONCAT_GN=1: off, A/B)
  bool gna_lnlin = true;          // GroupNorm applied on lnlin_kernel's resident fragments (Builder::gn_linear; $DTP_NO_GNA_LNLIN=1: off, A/B)
  bool tune_lnlin = true, tune_halo3 = true;  // lnlin_kernel / the three-image halo tiles among the tuner's candidates ($DTP_NO_LNLIN=1 / $DTP_NO_HALO3=1: off, A/B)
  bool xchain = true;             // level-0 to_out + cross-attention as one register-chained launch (xchain.hip; $DTP_NO_XCHAIN=1: off, A/B)
  bool xattn_tiles = true;        // xattn: several column tiles per workgroup where that is one round ($DTP_XATTN_CT1=1: off, A/B)
  int ffchain = -1;               // FF1 + FF2 + proj_out as one launch (ffchain.hip): < 0 by the row-count gate ($DTP_FFCHAIN=0 / 1: off / on, A/B)
  bool fp8_linear = false;        // UNet transformer Linears / 1x1 convs on the fp8 MX MFMA (configs[4]); fixed once a UNet program exists
  bool fp8_attention = false;     // UNet self-attention on the fp8 MX MFMA (BASELINE configs[4]); fixed once a UNet program exists
  bool fp8_operands = false;      // transformer Linears with K >= DTP_FP8_OPERANDS_MIN_K on e4m3 activations in memory (gemm_f8f8.hip); fixed once a UNet program exists
  std::deque<float> fp8_scales;   // host copies of the calibrated scales (stable addresses: the ops read them at enqueue time)
  std::deque<Fp8Cal> fp8_cals;
  unsigned int* fp8_amax = nullptr;  // device: DTP_FP8_SLOTS float bit patterns
  int fp8_nslots = 0;
  bool calibrating = false;
  bool finite_pending = false;    // the last stamp ran the check; dtp_last_stamp_finite reads the flag
  std::map<StageKey, StampGraph> graphs;  // captured stamp stages (graph_run / graphs_drop below)
  unsigned long long graph_clock = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int last_evals = 0, last_nodes = 0, last_unet_rows = 0;
  std::map<int, unsigned char*> stroke_masks;  // dtp_stroke: the default paste mask make_stamp_mask(R, margin) by margin, u8 [R][R]
  int last_stroke_stamps = -1, last_stroke_groups = 0, last_stroke_evals = 0;  // of the last dtp_stroke / dtp_mesh_stroke (-1: none yet)
  int* mesh_face_idx = nullptr;            // dtp_mesh_stroke: i32 [R][R], the face that won each pixel of the current stamp's render (-1: none)
  unsigned char* mesh_disc = nullptr;      // dtp_mesh_stroke: the Erase stamp's default mask, u8 [R][R] (built at its first use)
  struct Journal* journal_open = nullptr;  // the journal with an open record on this handle (dtp_journal_begin .. dtp_journal_end), or null
  bool use_graph = true;
  bool exec_imgenc_ready = false;
  bool profile = false;
  std::vector<ProfRec> prof;
  bool autotune = true;            // time every (tile, split-K) candidate of each distinct GEMM shape at build time
  std::map<std::string, std::pair<int, int>> tuned;  // shape key -> (tile, splits)
  std::map<std::string, std::pair<float, float>> tune_ms;  // $DTP_TUNE_REPORT: (cold, hot) ms of the chosen configuration
  double rep_cold_ms = 0, rep_hot_ms = 0;            // ... summed over every GEMM pushed into a program
  hipEvent_t tune_ev[2] = {nullptr, nullptr};
  void* tune_thrash = nullptr;     // 512 MiB scratch written before every timed tuning launch (cold weights)
  std::string tune_cache_path;     // $DTP_TUNE_CACHE: persisted (shape -> tile, splits) table
  size_t tune_saved = 0;

  // LoRA refit: the fp32 pre-merge copy of the 128 attention matrices (taken before merge_lora, ~0.37 GB), every packed buffer derived
  // from them, and the tensors staged for the next dtp_refit_lora
  std::unordered_map<std::string, float*> refit_base;  // staged weight name -> base copy (arena)
  std::vector<RefitTarget> refit_targets;
  std::vector<RowsumJob> refit_rowsums;                // qkv.lns, q2.lns of every block
  std::vector<TransposeJob> refit_transposes;          // q2T of every block
  std::unordered_map<std::string, Staged> refit_staged;
  void* refit_tables = nullptr;                        // device copy of the three job tables
  hipEvent_t refit_ev[2] = {nullptr, nullptr};
  int refit_matrices = -1, refit_launches = 0;         // of the last successful refit (-1: none yet)
  float refit_ms = 0.f;
};

// ---- engine.hip: memory, staging, weight loaders
int ctx_arena_alloc(Ctx* c, size_t bytes, void** out);
int ctx_pool_get(Ctx* c, size_t bytes, void** out);
void ctx_pool_put(Ctx* c, void* p);
int ctx_persistent(Ctx* c, size_t bytes, void** out, bool zero);
void mesh_drop_ctx(Ctx* c);  // mesh.hip: frees the meshes created on this handle (dtp_destroy)
// ---- journal.hip: the undo / redo journal of a texture.  The stroke calls ask for the journal whose open record guards
// (texture, H, W) on this handle -- null: none, and then they enqueue nothing more -- and save the tiles they are about to write.
void journal_drop_ctx(Ctx* c);  // frees the journals created on this handle (dtp_destroy)
struct Journal* journal_armed(Ctx* c, const void* texture, int H, int W);
// the tiles that meet the k windows of a 2D stroke group (clipped, or the wrapped pieces), each tile once per record
int journal_save_windows(struct Journal* j, int R, const int* xs, const int* ys, int k, int wrap, hipStream_t s);
// the tiles that meet the device-side texel box bb = {x0, y0, x1, y1} grown by `grow` and clipped (an empty box: none)
int journal_save_box(struct Journal* j, const int* bb, int grow, hipStream_t s);
// ---- delta.hip: the changed-tile trackers of images
void delta_drop_ctx(Ctx* c);  // frees the trackers created on this handle (dtp_destroy)
const Staged* ctx_find(Ctx* c, const std::string& name);
int ctx_fetch_host(Ctx* c, const std::string& name, std::vector<float>& out);
int ctx_upload_f32(Ctx* c, const std::vector<float>& v, float** out);
int load_norm(Ctx* c, const std::string& name, NormW& n);
// conv weight [Cout][Cin][k][k] -> packed; cin_pad = padded input channels (>= Cin, multiple of 8)
int load_conv(Ctx* c, const std::string& name, ConvW& w, int cin_pad = 0, bool bias = true);
int load_conv_ups4(Ctx* c, const std::string& name, ConvW& w);  // after load_conv of a conv that runs over a nearest-2x upsample: its phase sets (ConvW::wfr4)
// ResBlock tail: conv2 (3x3) and the 1x1 shortcut conv packed as ONE contraction [W2 | Wsc], bias = b2 + bsc
int load_conv_with_shortcut(Ctx* c, const std::string& conv, const std::string& shortcut, ConvW& w);
// two Linears in a row with only a residual between them, out = Wb (Wa f + ba + r) + bb, merged into ONE contraction over
// [f | r]: W = [Wb Wa | Wb] (product in fp32 at load time), bias = Wb ba + bb.  K = Ka + Kb.
int load_linear_pair(Ctx* c, const std::string& first, const std::string& second, ConvW& w);
// stacked linear: rows of several [n_i][K] matrices one after another; geglu packs the [a|gate] tile order
int load_linear(Ctx* c, const std::vector<std::string>& names, ConvW& w, bool bias, bool geglu = false,
                const std::string& fold_ln = std::string());  // fold_ln: name of the LayerNorm feeding this Linear
int load_plain_f16(Ctx* c, const std::string& name, f16** out);  // unpadded fp16 copy of a matrix

// ---- lora_refit.hip
// jobs: device table of njobs records.  One launch rewrites every job's rows of its packed buffer; the second writes the folded bias
// rows of the jobs that carry a beta; max_n / max_k: the largest N / K of the table (grid size)
int dtp_launch_lora_refit(const LoraRefitJob* jobs, int njobs, int max_n, int max_k, float scale, hipStream_t s);
int dtp_launch_lora_wbeta(const LoraRefitJob* jobs, int njobs, int max_n, float scale, hipStream_t s);
int dtp_launch_rowsum_f16_grouped(const RowsumJob* jobs, int njobs, int max_rows, hipStream_t s);
int dtp_launch_transpose_f16_grouped(const TransposeJob* jobs, int njobs, int max_rows, int max_cols, hipStream_t s);

// per-row (sum, sumsq) partials handed from a producer GEMM (GF_ROWSTATS) to the LayerNorm-folded consumer
struct RowStats {
  float* buf = nullptr;  // [parts][M][2]
  int parts = 0, M = 0;
  // the producer covers only rows [row_off, row_off + its M) of a rows_total-row table (de-duplicated prefix, unet.hip)
  int rows_total = 0, row_off = 0;
};

// ---- builder.hip: every function appends ops to `prog` and returns planned buffers
void prog_push(Ctx* c, Prog* prog, int kind, double flops, double bytes, Op fn, const std::string& label);
int push_gemm(Ctx* c, Prog* prog, GemmParams p, int bias_step_off, double k_alg, RowStats* emit = nullptr);  // emit (with a buffer): the launch writes its row statistics there (GF_ROWSTATS) and fills in parts / M
bool dtp_conv_output_can_carry_gn_stats(const GemmParams& p);  // the UNSPLIT conv problem p: may its epilogue emit its consumer GroupNorm's statistics?

struct MemRange { const void* p; size_t bytes; };

// A split-K producer whose reduce the GroupNorm-side launch that consumes its output has taken over (Builder::claim_reduce)
struct ReduceClaim {
  bool claimed = false;
  GemmParams p = {};       // the producer as it was re-pushed (GF_NOREDUCE)
  int bias_step_off = -1;  // >= 0: its bias is this slice of the step-bias table
  explicit operator bool() const { return claimed; }
  size_t slab_bytes() const;           // the producer's fp32 slabs at the head of the shared workspace, 256-byte aligned (0: nothing claimed)
  std::vector<MemRange> busy() const;  // what the taken-over reduce still reads besides the slabs: the producer's residual, or nothing
  GnReduceSrc src(const Ctx* c, int step) const;  // the reduce as the GroupNorm kernels take it, the bias resolved for `step` (at enqueue time)
};

// GroupNorm (+ SiLU) applied on a conv's staged input (GF_GNAPPLY): the statistics partials and the affine parameters
struct GnOnLoad { const float *part = nullptr, *gamma = nullptr, *beta = nullptr; float eps = 0.f; int nchunk = 0, cpg = 0; };
// what only some conv3() calls need
struct Conv3Opts {
  int extra_flags = 0;
  void* out_override = nullptr; int ldc_override = 0;  // write here with this row pitch (the fp32 outputs) instead of a planned fp16 buffer
  const T* tail = nullptr;       // the operand of the 1x1 shortcut fused as a 10th tap (w.cin2 channels)
  const T* dst = nullptr;        // write into this (possibly strided) view instead of a fresh buffer
  GnOnLoad gn;                   // with GF_GNAPPLY among extra_flags
  static Conv3Opts into(const T& view) { Conv3Opts o; o.dst = &view; return o; }
  static Conv3Opts f32_out(float* out, int ldc) { Conv3Opts o; o.extra_flags = GF_OUT_F32; o.out_override = out; o.ldc_override = ldc; return o; }
};

struct Builder {
  Ctx* c;
  Prog* prog;
  bool fp8 = false;  // dense Linears pushed through linear() / the transformer tail run on gemm_fp8_kernel when they can
  bool f8ops = false;  // option fp8_operands: linear_f8ops() runs the K >= DTP_FP8_OPERANDS_MIN_K Linears through quant8 / linear8
  // append an op; when profiling is on, every launch is bracketed by HIP events on its own stream
  void push(int kind, double flops, double bytes, Op fn, const std::string& label = std::string());
  T alloc(int B, int H, int W, int C);
  void release(const T& t);
  int gn(const T& x, const NormW& n, float eps, bool silu, T& y);
  ReduceClaim claim_reduce(const T& x, bool allow_concat = false);
  bool claim_stats(const T& x, float** partials, int* nchunk);
  bool gn_linear_supported(const T& x, const ConvW& w) const;
  int gn_linear(const T& x, const NormW& n, float eps, const ConvW& w, T& y, RowStats* emit);
  // GroupNorm + SiLU + 3x3 conv (stride 1, pad 1); the apply pass rides on the conv's staged input where the halo kernel can take it
  int gn_conv3(const T& x, const NormW& n, float eps, const ConvW& w, const T* resid, int bias_step_off, T& y, const T* tail, const T* dst);
  int ln(const T& x, const NormW& n, T& y);
  // conv3x3; bias_step_off >= 0 selects the per-step bias slice from the temb table instead of w.b
  int conv3(const T& x, const ConvW& w, int stride, int pad, bool ups, int Ho, int Wo, const T* resid, int bias_step_off, T& y,
            const Conv3Opts& o = Conv3Opts());
  int linear(const T& x, const ConvW& w, const T* resid, int flags, T& y, RowStats* emit = nullptr, const RowStats* use = nullptr,
             const T* dst = nullptr);
  // option fp8_operands: an e4m3 tensor from the pool shaped like `like` with C columns and a calibrated (a new calibration slot) or
  // fixed scale; the quantise pass x -> y (ln: (x - mean) * rstd with the statistics `st` when they cover x); a Linear over the e4m3 x
  T8 alloc8(const T& like, int C, bool calibrated, float fixed_scale = 1.f);
  void release8(const T8& t);
  int quant8(const T& x, const T8& y, bool ln, const RowStats* st);
  int linear8(const T8& x, const ConvW& w, const T* resid, int flags, T& y, RowStats* emit);
  // linear() -- or, where option fp8_operands covers w, quant8 + linear8: x quantised after its LayerNorm (statistics `ln`, fixed scale)
  // or, without `ln`, with a calibrated scale.  release_ln: `ln` goes back to the pool once its last reader is pushed.
  int linear_f8ops(const T& x, const ConvW& w, const T* resid, int flags, T& y, RowStats* emit, RowStats* ln, bool release_ln);
  int alloc_stats(long long rows, int C, RowStats& st);  // room for one partial per 64-column tile
  void release_stats(RowStats& st);
  int attention(const T& q, const T& k, const T& v, int heads, int Sq, int Skv, int Bn, T& o);
  int concat(const T& a, const T& b, T& y);
  int resnet(const T& x, const ResW& w, float eps, bool temb, T& y, const T* dst = nullptr);
};

int build_unet_prog(Ctx* c, int N, int dupB, UNetProg& up);
int build_vae_enc_prog(Ctx* c, int B, VaeEncProg& p);
int build_vae_dec_prog(Ctx* c, int B, VaeDecProg& p);
int load_unet_weights(Ctx* c);
int load_vae_weights(Ctx* c);
int load_imgenc_weights(Ctx* c);
// the cached program of a batch, built on first use (unet.hip, vae.hip)
int get_unet_prog(Ctx* c, int N, int dupB, UNetProg** out);
int get_enc_prog(Ctx* c, int B, VaeEncProg** out);
int get_dec_prog(Ctx* c, int B, VaeDecProg** out);
int launch_vae_sample(Ctx* c, const float* mom, const float* eps, float* out, int B, float scale, hipStream_t s, const float* eps3 = nullptr,
                      int n_eps = -1);
int launch_post_quant(Ctx* c, const float* z, int nhwc, float in_scale, f16* out, int B, hipStream_t s);
int ensure_ws(Ctx* c);              // engine.hip
int ensure_w8(Ctx* c, ConvW& w);    // engine.hip: build the e4m3 copy of a Linear's packed weights (once)
// fp8 calibration (builder.hip): new scale / amax-slot pair for a Linear (returns the scale's address, sets *slot1), and the pass itself
float* fp8_new_linear_scale(Ctx* c, int* slot1);
int fp8_calibrate(Ctx* c, UNetProg* up, hipStream_t s, int step);
// ---- tune.hip: the persisted (shape -> tile, splits) table; tune_gemm: (*tile, *sp) is the caller's configuration on entry, the one to use on return
void tune_cache_load(Ctx* c);
void tune_cache_save(Ctx* c);
int tune_gemm(Ctx* c, const GemmParams& p, int* tile, int* sp);
int ensure_temb(Ctx* c, const std::vector<float>& timesteps);  // fills temb_table rows 0..n-1

// ---- context.hip
int stamp_init(Ctx* c);

// ---- schedule.hip
int sched_evals(int scheduler, int steps);  // UNet evaluations of a full (strength 1) stamp

// ---- the captured stages of a stamp (Ctx::graphs).  Neither drop waits for the device: a caller whose graphs may still be replaying
// synchronises first.
template <class P>
void graphs_drop(Ctx* c, P pred) {
  for (auto g = c->graphs.begin(); g != c->graphs.end();) {
    if (!pred(g->first)) { ++g; continue; }
    if (g->second.exec) (void)hipGraphExecDestroy(g->second.exec);
    if (g->second.graph) (void)hipGraphDestroy(g->second.graph);
    g = c->graphs.erase(g);
  }
}
inline void graphs_drop_all(Ctx* c) { graphs_drop(c, [](const StageKey&) { return true; }); }

// run `body` on stream s, replaying a captured hipGraph when possible.  Of the denoise-loop graphs the context keeps the
// DTP_LOOP_GRAPH_CAP most recently replayed
template <class F>
int graph_run(Ctx* c, const StageKey& key, hipStream_t s, F body) {
  if (!c->use_graph || c->profile || s == nullptr) return body(s);
  auto it = c->graphs.find(key);
  if (it == c->graphs.end()) {
    if (key.stage == 2) {
      int n = 0;
      const std::pair<const StageKey, StampGraph>* lru = nullptr;
      for (const auto& g : c->graphs) {
        if (g.first.stage != 2) continue;
        ++n;
        if (!lru || g.second.used < lru->second.used) lru = &g;
      }
      if (n >= DTP_LOOP_GRAPH_CAP) {  // (rare: a new profile; its capture costs far more than this wait)
        HIP_CHECK(hipDeviceSynchronize());  // the evicted graph may still be replaying
        graphs_drop(c, [lru](const StageKey& k) { return &k == &lru->first; });
      }
    }
    StampGraph g;
    HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = body(s);
    hipError_t e = hipStreamEndCapture(s, &g.graph);
    if (rc != DTP_OK) { if (g.graph) (void)hipGraphDestroy(g.graph); return rc; }
    if (e != hipSuccess) { dtp_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return DTP_ERR_HIP; }
    size_t n = 0;
    (void)hipGraphGetNodes(g.graph, nullptr, &n);
    g.nodes = (int)n;
    HIP_CHECK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    it = c->graphs.emplace(key, g).first;
  }
  it->second.used = ++c->graph_clock;
  c->last_nodes += it->second.nodes;
  HIP_CHECK(hipGraphLaunch(it->second.exec, s));
  return DTP_OK;
}

// ---- noise.hip: the draws of a seeded stamp call (dtp_stamp_seeded).  Job j < nd writes draw `draw[j]` of every stamp b < B, generated
// from seed[b], to dst[j] + b * 4 Q (Q = h w counters of four floats each); the seeds travel as a kernel argument, like PadArgs.
struct NoiseArgs {
  uint64_t seed[DTP_STAMP_MAXB];
  float* dst[4];
  int draw[4];
};
int dtp_launch_stamp_noise(const NoiseArgs& a, int nd, int B, long long Q, hipStream_t s);
