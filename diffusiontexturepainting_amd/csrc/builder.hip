// Launch-program builder: every Builder method, the GEMM / conv push with its tile choice, and the fp8 calibration pass.
#include "engine.h"

#include <math.h>
#include <stdio.h>

#include <algorithm>

static Op make_gemm_op(Ctx* c, GemmParams p, int tile, int bias_step_off);

// the bias of a launch at denoising step `step`: its slice of the step-bias table (conv1.bias + time_emb_proj, ensure_temb), or `fallback`
static const float* step_bias(const Ctx* c, int bias_step_off, int step, const float* fallback) {
  return bias_step_off >= 0 ? c->temb_table + (size_t)step * c->unet.temb_total + bias_step_off : fallback;
}
// the flags a producer may carry for a GroupNorm to take over its split-K reduce (claim_reduce) or get its statistics from its epilogue
// (claim_stats): nothing that changes what the stored output means
static constexpr int GF_CLAIMABLE = GF_BIAS | GF_RESID | GF_CONV3 | GF_UPS2 | GF_MFAST | GF_RAGGED;

// ---------------------------------------------------------------- builder
void prog_push(Ctx* c, Prog* prog, int kind, double flops, double bytes, Op fn, const std::string& label) {
  prog->last_gemm.valid = false;
  prog->ops.push_back([=](hipStream_t s, int step) -> int {
    if (!c->profile) return fn(s, step);
    ProfRec r;
    r.kind = kind; r.flops = flops; r.bytes = bytes; r.label = label.c_str();
    HIP_CHECK(hipEventCreate(&r.e0));
    HIP_CHECK(hipEventCreate(&r.e1));
    HIP_CHECK(hipEventRecord(r.e0, s));
    const int rc = fn(s, step);
    HIP_CHECK(hipEventRecord(r.e1, s));
    c->prof.push_back(r);
    return rc;
  });
}
void Builder::push(int kind, double flops, double bytes, Op fn, const std::string& label) { prog_push(c, prog, kind, flops, bytes, fn, label); }

T Builder::alloc(int B, int H, int W, int C) {
  T t;
  t.B = B; t.H = H; t.W = W; t.C = C; t.ld = C;
  void* p = nullptr;
  if (ctx_pool_get(c, (size_t)B * H * W * C * sizeof(f16), &p) != DTP_OK) p = nullptr;
  t.p = (f16*)p;
  return t;
}
void Builder::release(const T& t) { ctx_pool_put(c, t.p); }

// Column ranges of an lnlin_kernel launch when no tuner picks them: the LARGEST count the kernel accepts within one partial per 64
// output columns -- independent of the row count, so that the row-statistics partials (one per range) are summed in the same grouping
// whatever the batch (the de-duplicated UNet prefix evaluates two of three samples and must stay bit-identical with the tuner off).
static int lnlin_default_ranges(const GemmParams& p) {
  for (int r = (p.N + 63) / 64; r >= 1; --r)
    if (dtp_lnlin_supported(p, r)) return r;
  return 0;
}

// Which conv outputs can carry their consumer GroupNorm's statistics (GF_GNSTATS of the two-n-tile convws builds)?  ONE predicate for
// Builder::claim_stats (which re-pushes the conv with the flag) and for tune_gemm (which credits such a candidate with the statistics
// pass it saves) -- round-5 advisor: the two had repeated parts of each other's conditions (chunk cap, channels-per-group range) and
// could drift apart.  `p` is the UNSPLIT problem.  What the shape cannot tell is the consumer: an output view inside a concatenation
// buffer (ldc > N) is claimed when the next GroupNorm runs over that view alone (down path: the skip slot IS the layer output) and not
// when it runs over the whole concatenation (up path); the tuner's credit stays a shape-level estimate.
bool dtp_conv_output_can_carry_gn_stats(const GemmParams& p) {
  if ((p.flags & ~GF_CLAIMABLE) || !(p.flags & GF_CONV3) || p.batch > 1) return false;
  if ((p.N % 32) || p.N / 32 < 4 || p.N / 32 > 64) return false;
  // every block of the consumer re-reads its image's whole partials table (chunks x 32 x 8 bytes): beyond ~1k chunks (the VAE's 512^2 and
  // 256^2 maps: 1 MB per image) that is more traffic than the statistics pass it replaces (round-4 advisor) -- those keep the pass
  if (!(p.flags & GF_RAGGED) && ((p.Ho & 7) || (p.Wo & 15))) return false;
  if (dtp_conv_ws_gn_chunks(p.Ho, p.Wo) > 1024) return false;
  return true;
}

// A pool block that overlaps none of `ranges` (operands some launch still reads while the block is being written).  The pool hands out
// whatever fits -- also a block an operand was released from a moment ago, because the Builder releases tensors as soon as their last
// consumer is PUSHED, not run; a launch that both reads such an operand and writes the new block would race with itself (round-4 / 5
// advisor: GroupNorm output vs the claimed reduce's residual, statistics partials vs the conv's operands).  Overlapping blocks are set
// aside for the duration of the search and returned.
static void* pool_get_clear_of(Ctx* c, size_t need, const std::vector<MemRange>& ranges, int attempts = 6) {
  std::vector<void*> aside;
  void* got = nullptr;
  for (int attempt = 0; attempt < attempts; ++attempt) {
    void* pp = nullptr;
    if (ctx_pool_get(c, need, &pp) != DTP_OK) break;
    bool hit = false;
    for (const MemRange& r : ranges)
      if (r.p && r.bytes && (const char*)pp < (const char*)r.p + r.bytes && (const char*)r.p < (const char*)pp + need) { hit = true; break; }
    if (!hit) { got = pp; break; }
    aside.push_back(pp);
  }
  for (void* q : aside) ctx_pool_put(c, q);
  return got;
}
// the operands a (re-pushed) GEMM / conv launch reads
static std::vector<MemRange> gemm_operand_ranges(const GemmParams& gp, long long images) {
  const size_t in_bytes = (gp.flags & GF_CONV3) ? (size_t)images * gp.Hi * gp.Wi * gp.lda * sizeof(f16) : (size_t)gp.M * gp.lda * sizeof(f16);
  return {{gp.A, in_bytes}, {gp.A2, gp.A2 ? (size_t)gp.M * gp.lda2 * sizeof(f16) : 0}, {gp.R, gp.R ? (size_t)gp.M * gp.ldr * sizeof(f16) : 0}};
}

// The producer of x was a split-K conv whose reduce has not run yet: take the reduce over (the GroupNorm-side kernel sums the slabs
// and writes x itself).  Re-pushes the conv with GF_NOREDUCE and returns the claim (unclaimed: the separate reduce stays).
ReduceClaim Builder::claim_reduce(const T& x, bool allow_concat) {
  const LastGemm lg = prog->last_gemm;
  // round 5 (allow_concat): x may be a zero-copy concatenation [producer's N channels | skip] -- the split producer wrote (will write) the
  // FIRST lg.p.N channels of x's rows; the single-launch reduce + GroupNorm sums those from the slabs and reads the rest from x itself
  const bool whole = lg.p.N == x.C;
  const bool front = allow_concat && lg.p.N < x.C && (lg.p.N & 7) == 0 && x.H * x.W <= 256 && dtp_reduce_groupnorm_supported(x.H * x.W, x.C, 32);
  if (!(c->fuse_reduce_gn && lg.valid && lg.p.splits > 1 && (f16*)lg.p.C == x.p && lg.p.ldc == x.ld && lg.p.M == (int)x.rows() && (whole || front) &&
        !(lg.p.flags & ~GF_CLAIMABLE) && lg.p.batch <= 1 && (x.C & 7) == 0))
    return ReduceClaim();
  // what the GroupNorm-side launches accept, asked here, where the separate reduce is still the fallback
  if (!dtp_groupnorm_reduce_accepts(x.C, 32, x.ld, lg.p.N, (lg.p.flags & GF_RESID) ? lg.p.ldr : 0)) return ReduceClaim();
  ReduceClaim claim = {true, lg.p, lg.bias_step_off};
  claim.p.flags |= GF_NOREDUCE;
  prog->ops[lg.op_index] = Op();  // rebuilt below through the profiling wrapper
  prog->ops.pop_back();
  prog_push(c, prog, lg.kind, lg.flops, lg.bytes, make_gemm_op(c, claim.p, lg.tile, lg.bias_step_off), lg.label + " (reduce in gn)");
  return claim;
}

size_t ReduceClaim::slab_bytes() const { return claimed ? ((dtp_gemm_workspace_bytes(p) + 255) & ~(size_t)255) : 0; }
std::vector<MemRange> ReduceClaim::busy() const {
  return claimed && (p.flags & GF_RESID) ? std::vector<MemRange>{{p.R, (size_t)p.M * p.ldr * sizeof(f16)}} : std::vector<MemRange>();
}
GnReduceSrc ReduceClaim::src(const Ctx* c, int step) const {
  const float* bias = (p.flags & GF_BIAS) ? step_bias(c, bias_step_off, step, p.bias) : nullptr;
  return {c->ws, p.splits, (long long)p.M * p.N, p.N, bias, (p.flags & GF_RESID) ? p.R : nullptr, p.ldr};  // the slabs sit at the head of the workspace
}

// A pool block for what the launch that ALSO runs the claimed reduce writes (a GroupNorm's output, its statistics partials).  That launch
// adds the producer's residual -- a transformer block's input, normally back in the pool by now -- so the pool may hand out the residual's
// own block: one workgroup would write where another still reads (rounds 4-5: a whole tensor laid out like the residual never showed it,
// over a concatenation the pitches differ and stamps differed run to run).  Every consumer of a claim takes its block here.
static void* block_clear_of_claim(Ctx* c, size_t bytes, const ReduceClaim& claim, const char* who, const char* what) {
  void* p = pool_get_clear_of(c, bytes, claim.busy());
  if (!p) dtp_set_error("%s: no %s block clear of the claimed reduce's residual", who, what);
  return p;
}

// The 32-group GroupNorm over x as the launchers take it (y: the normalised tensor, if the launch writes one), and its launch label
static GnParams gn_params(const T& x, const NormW& n, float eps, bool silu, const T* y = nullptr) {
  return {x.p, x.ld, y ? y->p : nullptr, y ? y->ld : 0, n.g, n.b, x.B, x.H * x.W, x.C, 32, eps, silu ? 1 : 0};
}
static std::string gn_label(const GnParams& gp) { return " B=" + std::to_string(gp.B) + " HW=" + std::to_string(gp.HW) + " C=" + std::to_string(gp.C); }

// The statistics pass of the two-launch GroupNorm over x, the claimed reduce riding in it.  `part`: a planned partials buffer that outlives
// the launch, or null: the shared workspace behind the claim's slabs (good until the next split launch).
static void push_gn_stats(Builder& b, const GnParams& gp, float* part, const ReduceClaim& claim, const char* label_suffix) {
  Ctx* cc = b.c;
  const size_t slab_bytes = claim.slab_bytes();
  b.push(PK_GN, 0.0, 2.0 * (double)gp.B * gp.HW * gp.C, [=](hipStream_t s, int step) {
    const GnReduceSrc rd = claim.src(cc, step);
    return dtp_launch_groupnorm_stats(gp, part ? part : (float*)((char*)cc->ws + slab_bytes), claim ? &rd : nullptr, s);
  }, (claim ? "reduce+gn-stats" : "gn-stats") + gn_label(gp) + label_suffix);
}

// Let the GEMM p emit the per-row (sum, sumsq) partials of its output into `emit` (GF_ROWSTATS); false: nothing to emit into.  The table
// has rows_total rows when the launch covers only a slice of it, otherwise the launch's own (all groups of a grouped problem).  push_gemm
// applies it to its own copy of the problem (never in an argument of a call that also takes p by value: the copy is made first).
static bool emit_rowstats(GemmParams& p, const RowStats* emit) {
  if (!emit || !emit->buf) return false;
  p.flags |= GF_ROWSTATS;
  p.st_out = emit->buf; p.st_rows = (p.batch > 1 ? p.batch : 1) * p.M;
  if (emit->rows_total > 0) { p.st_out = emit->buf + (size_t)emit->row_off * 2; p.st_rows = emit->rows_total; }
  return true;
}

// The producer of x was an UNSPLIT two-n-tile convws launch (tile 53 / 54): let its epilogue emit the GroupNorm partial sums of x (GF_GNSTATS,
// conv_ws.hip) -- the consumer then needs no statistics pass over x.  Re-pushes the conv with the flag and a planned partials buffer
// [B][nchunk][32][2]; the caller returns the buffer to the pool once its consumer is pushed.
bool Builder::claim_stats(const T& x, float** partials, int* nchunk) {
  const LastGemm lg = prog->last_gemm;
  const DtpTile t = dtp_tile(lg.tile);
  if (!c->gn_epilogue || !lg.valid || t.fam != TF_CONVWS || t.var < 2 || lg.p.splits != 1 || (f16*)lg.p.C != x.p || lg.p.ldc != x.ld ||
      lg.p.M != (int)x.rows() || lg.p.N != x.C || !dtp_conv_output_can_carry_gn_stats(lg.p))
    return false;
  GemmParams gp = lg.p;
  const int chunks = dtp_conv_ws_gn_chunks(gp.Ho, gp.Wo);
  // The conv's input (and residual / shortcut operand) may already be back in the pool -- gn_conv3 releases it before its consumer is
  // built -- and the pool would happily hand that very block out for the partials, which the re-pushed conv WRITES while other
  // workgroups still read the operand (round-4 advisor: a latent aliasing race): pool_get_clear_of.
  const size_t need = (size_t)x.B * chunks * 32 * 2 * sizeof(float);
  void* pp = pool_get_clear_of(c, need, gemm_operand_ranges(gp, x.B), 4);
  if (!pp) return false;
  gp.flags |= GF_GNSTATS;
  gp.st_out = (float*)pp;
  gp.gn_cpg = x.C / 32;
  if (!dtp_conv_ws_supported(gp, t.var, 1)) { ctx_pool_put(c, pp); return false; }
  prog->ops.pop_back();
  prog_push(c, prog, lg.kind, lg.flops, lg.bytes, make_gemm_op(c, gp, lg.tile, lg.bias_step_off), lg.label + " (+gn stats)");
  *partials = (float*)pp;
  *nchunk = chunks;
  return true;
}

int Builder::gn(const T& x, const NormW& n, float eps, bool silu, T& y) {
  Ctx* cc = c;
  const ReduceClaim claim = claim_reduce(x, cc->reduce_in_concat_gn);
  y = T();
  y.B = x.B; y.H = x.H; y.W = x.W; y.C = x.C; y.ld = x.C;
  y.p = (f16*)block_clear_of_claim(cc, (size_t)x.B * x.H * x.W * x.C * sizeof(f16), claim, "gn", "output");
  if (!y.p) return DTP_ERR_HIP;
  const size_t slab_bytes = claim.slab_bytes();
  cc->ws_need = std::max(cc->ws_need, slab_bytes + dtp_groupnorm_ws_bytes(x.B, x.H * x.W, x.C, 32));
  const GnParams gp = gn_params(x, n, eps, silu, &y);
  const double bytes = 4.0 * (double)x.rows() * x.C;
  if (claim) {
    // small maps: one launch does it all; large maps: the reduce rides in the statistics pass, whose partial sums live behind the slabs
    const int Cx = claim.p.N;  // the producer wrote channels [0, Cx) of x (fewer than x.C: a concatenation's front)
    push(PK_GN, 0.0, bytes, [=](hipStream_t s, int step) {
      return dtp_launch_reduce_groupnorm(gp, claim.src(cc, step), Cx, (float*)((char*)cc->ws + slab_bytes), s);
    }, (Cx < x.C ? "reduce(front " + std::to_string(Cx) + ")+gn" : std::string("reduce+gn")) + gn_label(gp) + " splits=" + std::to_string(claim.p.splits));
    return DTP_OK;
  }
  float* partials = nullptr;
  int nchunk = 0;
  if (claim_stats(x, &partials, &nchunk)) {  // statistics from the producing conv's epilogue: the apply pass alone
    push(PK_GN, 0.0, bytes, [=](hipStream_t s, int) { return dtp_launch_groupnorm_apply(gp, partials, nchunk, s); }, "gn-apply" + gn_label(gp));
    ctx_pool_put(cc, partials);
    return DTP_OK;
  }
  push(PK_GN, 0.0, bytes, [=](hipStream_t s, int) { return dtp_launch_groupnorm(gp, cc->ws, s); }, "gn" + gn_label(gp));
  return DTP_OK;
}

// GroupNorm (no activation) + the Linear / 1x1 conv that consumes it, with the normalisation folded into per-sample weights
// (norm.hip gn_fold_weights_kernel): statistics pass (+ the producer's split-K reduce) -> fold -> ONE grouped GEMM on the raw tensor.
// The apply pass and the normalised tensor do not exist.  Same three launches as stats + apply + GEMM, but the middle one touches
// N * C * C weights instead of reading and writing the whole activation tensor.
bool Builder::gn_linear_supported(const T& x, const ConvW& w) const {
  const int HW = x.H * x.W, C = x.C;
  return c->fold_gn_linear && HW >= 1024 && w.taps == 1 && w.K == C && w.ldw == C && (C % 64) == 0 && C <= 2048 && (C % 32) == 0 && !w.lns &&
         !(fp8 && w.w8) && C / 32 >= 8;
}

int Builder::gn_linear(const T& x, const NormW& n, float eps, const ConvW& w, T& y, RowStats* emit) {
  Ctx* cc = c;
  const int HW = x.H * x.W, C = x.C, N = x.B, Cp = (w.cout + 127) / 128 * 128;
  const GnParams gp = gn_params(x, n, eps, false);
  const ReduceClaim claim = claim_reduce(x);
  float* ep_part = nullptr;  // statistics emitted by the producing conv's epilogue (claim_stats): no statistics launch at all
  int ep_chunks = 0;
  const bool from_epilogue = !claim && claim_stats(x, &ep_part, &ep_chunks);
  const size_t slab_bytes = claim.slab_bytes();
  cc->ws_need = std::max(cc->ws_need, slab_bytes + dtp_groupnorm_ws_bytes(N, HW, C, 32));
  // Round 6: where the activation-stationary Linear takes the problem (K = C in {320, 640}: UNet levels 0-1), the GroupNorm is applied to
  // its RESIDENT activation fragments (lnlin_kernel GNA) -- [statistics ->] ONE launch on the raw tensor with the shared weights; the fold
  // launch (190 per batch-1 stamp), the per-sample weight copies and the grouped problem disappear.  Ctx::gna_lnlin off: the fold (A/B).
  GemmParams lin = {};  // what both forms share: one problem per sample over the raw tensor
  lin.A = x.p; lin.lda = x.ld; lin.ldw = w.ldw; lin.nkb = w.ldw / 64;
  lin.M = HW; lin.N = w.cout; lin.K = w.K;
  lin.batch = N; lin.a_bs = (long long)HW * x.ld;
  if (cc->gna_lnlin && (C == 320 || C == 640) && (HW & 127) == 0 && !fp8) {
    GemmParams g = lin;  // the shared weights and bias (w_bs = bias_bs = 0)
    g.W = w.w; g.bias = w.b; g.flags = (w.b ? GF_BIAS : 0) | GF_GNAPPLY;
    g.c_bs = (long long)HW * w.cout;
    g.gn_gamma = n.g; g.gn_beta = n.b; g.gn_eps = eps; g.gn_cpg = C / 32;
    g.gn_nchunk = from_epilogue ? ep_chunks : dtp_groupnorm_stat_chunks(HW);
    g.gn_part = (const float*)x.p;  // (a non-null placeholder for the support check: the partials block is planned below)
    g.ldc = w.cout;
    if (lnlin_default_ranges(g) > 0) {
      // the partial sums outlive the statistics launch inside the shared workspace only until the next split launch: own planned buffer
      float* part = ep_part;
      if (!from_epilogue) {
        part = (float*)block_clear_of_claim(cc, dtp_groupnorm_ws_bytes(N, HW, C, 32), claim, "gn_linear", "partials");
        if (!part) return DTP_ERR_HIP;
        push_gn_stats(*this, gp, part, claim, " (apply in proj_in)");
      }
      g.gn_part = part;
      y = alloc(x.B, x.H, x.W, w.cout);
      if (!y.p) return DTP_ERR_HIP;
      g.C = y.p; g.ldc = y.ld; g.c_bs = (long long)HW * y.ld;
      RC(push_gemm(cc, prog, g, -1, (double)w.K, emit));
      ctx_pool_put(cc, part);
      return DTP_OK;
    }
  }
  void *pw = nullptr, *pb = nullptr;
  RC(ctx_pool_get(cc, (size_t)N * Cp * w.ldw * sizeof(f16), &pw));
  RC(ctx_pool_get(cc, (size_t)N * Cp * sizeof(float), &pb));
  f16* Wf = (f16*)pw;
  float* bf = (float*)pb;
  const ConvW ww = w;
  if (!from_epilogue) push_gn_stats(*this, gp, nullptr, claim, "");  // into the shared workspace behind the slabs: the fold below reads them next
  push(PK_GN, 0.0, 2.0 * (double)N * w.cout * C * 2, [=](hipStream_t s, int) {
    const float* part = from_epilogue ? ep_part : (const float*)((char*)cc->ws + slab_bytes);
    return dtp_launch_gn_fold_weights(gp, part, from_epilogue ? ep_chunks : 0, ww.w, ww.ldw, ww.b, ww.cout, Wf, (long long)Cp * ww.ldw, bf, Cp, s);
  }, std::string(from_epilogue ? "gn-fold (stats from conv) B=" : "gn-fold B=") + std::to_string(N) + " C=" + std::to_string(C) + " N=" + std::to_string(w.cout));
  if (from_epilogue) ctx_pool_put(cc, ep_part);
  y = alloc(x.B, x.H, x.W, w.cout);
  if (!y.p) return DTP_ERR_HIP;
  GemmParams g = lin;  // per-sample weights and biases
  g.W = Wf; g.w_bs = (long long)Cp * w.ldw; g.bias = bf; g.bias_bs = Cp; g.flags = GF_BIAS;
  g.C = y.p; g.ldc = y.ld; g.c_bs = (long long)HW * y.ld;
  RC(push_gemm(cc, prog, g, -1, (double)w.K, emit));
  ctx_pool_put(cc, pw);
  ctx_pool_put(cc, pb);
  return DTP_OK;
}

int Builder::ln(const T& x, const NormW& n, T& y) {
  y = alloc(x.B, x.H, x.W, x.C);
  if (!y.p) return DTP_ERR_HIP;
  const T xx = x, yy = y;
  const NormW nn = n;
  push(PK_LN, 0.0, 4.0 * (double)xx.rows() * xx.C, [=](hipStream_t s, int) {
    return dtp_launch_layernorm(xx.p, xx.ld, yy.p, yy.ld, nn.g, nn.b, (int)xx.rows(), xx.C, 1e-5f, s);
  });
  return DTP_OK;
}

float* fp8_new_linear_scale(Ctx* c, int* slot1) {
  if (c->fp8_nslots + 1 > DTP_FP8_SLOTS) {  // (round-4 advisor: this fallback to the default scale used to be silent)
    static bool warned = false;
    if (!warned) { fprintf(stderr, "[dtp] fp8: the %d calibration slots are used up -- further fp8 operands keep the default activation scale\n", DTP_FP8_SLOTS); warned = true; }
    *slot1 = 0;
    return nullptr;
  }
  c->fp8_scales.push_back(1.0f);
  Fp8Cal r;
  r.kind = 0; r.slot0 = c->fp8_nslots; r.s0 = &c->fp8_scales.back();
  c->fp8_cals.push_back(r);
  *slot1 = ++c->fp8_nslots;
  return r.s0;
}

// One evaluation of the program with every fp8 op also measuring the absolute maximum of its operands, then power-of-two scales:
// amax * margin / scale <= 448 (the largest e4m3 value), as large a mantissa use as that allows.  Synchronises the stream once.
int fp8_calibrate(Ctx* c, UNetProg* up, hipStream_t s, int step) {
  if (up->fp8_calibrated || up->cal_begin == up->cal_end) { up->fp8_calibrated = true; return DTP_OK; }
  if (!c->fp8_amax) { void* p; RC(ctx_persistent(c, DTP_FP8_SLOTS * sizeof(unsigned int), &p, true)); c->fp8_amax = (unsigned int*)p; }
  HIP_CHECK(hipMemsetAsync(c->fp8_amax, 0, DTP_FP8_SLOTS * sizeof(unsigned int), s));
  c->calibrating = true;
  const int rc = up->main.run(s, step);
  c->calibrating = false;
  RC(rc);
  std::vector<float> amax(DTP_FP8_SLOTS);
  HIP_CHECK(hipMemcpyAsync(amax.data(), c->fp8_amax, DTP_FP8_SLOTS * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  auto pow2_for = [](float a) { return a > 0.f ? exp2f(ceilf(log2f(a * DTP_FP8_MARGIN / 448.0f))) : 1.0f; };
  for (size_t i = up->cal_begin; i < up->cal_end; ++i) {
    Fp8Cal& r = c->fp8_cals[i];
    if (r.kind == 0) {
      *r.s0 = pow2_for(amax[r.slot0]);
    } else {
      // Q' = Q * (softmax_scale * log2 e * q_scale), K' = K / q_scale: balance the two absolute maxima (their product is fixed)
      const float aq = amax[r.slot0] * r.softmax_scale * 1.4426950408889634f, ak = amax[r.slot0 + 1], av = amax[r.slot0 + 2];
      *r.s0 = (aq > 0.f && ak > 0.f) ? exp2f(roundf(0.5f * log2f(ak / aq))) : 1.0f;
      *r.s1 = pow2_for(av);
    }
  }
  up->fp8_calibrated = true;
  return DTP_OK;
}

static Op make_gemm_op(Ctx* c, GemmParams p, int tile, int bias_step_off) {
  return [=](hipStream_t s, int step) -> int {
    GemmParams q = p;
    q.part = c->ws;
    if (p.a_scale_host) {  // fp8 with a calibrated activation scale
      if (c->calibrating && p.amax_slot1 > 0) {
        const int ka = p.A2 ? p.K - p.Cin2 : p.K;
        RC(dtp_launch_amax_f16(p.A, p.M, ka, p.lda, c->fp8_amax + p.amax_slot1 - 1, s));
        if (p.A2) RC(dtp_launch_amax_f16(p.A2, p.M, p.Cin2, p.lda2, c->fp8_amax + p.amax_slot1 - 1, s));
      }
      q.a_scale = *p.a_scale_host;
    }
    q.bias = step_bias(c, bias_step_off, step, q.bias);
    return dtp_launch_tile(q, tile, s);
  };
}

int push_gemm(Ctx* c, Prog* prog, GemmParams p, int bias_step_off, double k_alg, RowStats* emit) {
  if (!emit_rowstats(p, emit)) emit = nullptr;  // (before the tile is picked: the flag is part of the problem)
  int tile = 0;
  dtp_gemm_pick(p, &tile, c->num_cu);
  int sp = p.splits;
  if (p.W8) { tile = 24 + ((p.flags & GF_GEGLU) ? (p.M >= 512 ? 0 : 3) : (p.M >= 512 ? 0 : 2)); sp = 1; }  // fp8: unsplit, one of the four fp8 tiles
  if ((p.flags & GF_GNAPPLY) && (p.flags & GF_CONV3)) { tile = (p.Hi * p.Wi <= 256) ? 14 : 12; sp = 1; }  // halo kernel only
  if ((p.flags & GF_GNAPPLY) && !(p.flags & GF_CONV3)) {  // dense: GroupNorm on the resident fragments of lnlin_kernel, nothing else applies it
    tile = DTP_TILE_LNLIN;
    sp = lnlin_default_ranges(p);
    if (!sp) { dtp_set_error("push_gemm: no lnlin configuration for the GroupNorm-on-load Linear (M %d N %d K %d)", p.M, p.N, p.K); return DTP_ERR_ARG; }
  }
  if (c->autotune) RC(tune_gemm(c, p, &tile, &sp));
  if (c->ups_phase >= 2 && dtp_conv_ws_supported(p, 2 + c->ups_phase, 1)) { tile = DTP_TILE_WSUPS4 + c->ups_phase - 2; sp = 1; }  // forced (tests, A/B)
  (void)dtp_tile_apply(p, tile, sp);
  const DtpTile t = dtp_tile(tile);
  if (emit) {  // the consumer must know how many partials this launch configuration writes per row
    emit->parts = dtp_tile_row_parts(p, tile);
    emit->M = p.M * (p.batch > 1 ? p.batch : 1);
  }
  c->ws_need = std::max(c->ws_need, dtp_gemm_workspace_bytes(p));
  p.zero = c->zero;
  // algorithmic work: 2*M*N*K on the UNPADDED contraction; bytes = A once + W once + C once (fp16)
  const double n_out = (p.flags & GF_GEGLU) ? p.N / 2.0 : (double)p.N;
  const double a_elems = (p.flags & GF_CONV3) ? (double)p.M * (k_alg / 9.0) * ((p.flags & GF_UPS2) ? 0.25 : (double)(p.stride * p.stride))
                                               : (double)p.M * k_alg;
  const double nb = p.batch > 1 ? (double)p.batch : 1.0;
  const double bytes = 2.0 * nb * (a_elems + (double)p.N * k_alg + (double)p.M * n_out);
  char lab[160];
  const bool f8tile = t.fam == TF_FP8;  // an fp8 problem may have kept an fp16 tile (tune_gemm)
  snprintf(lab, sizeof(lab), "%s M=%d N=%d K=%d tile=%d splits=%d%s%s%s%s", (p.flags & GF_CONV3) ? "conv3" : "gemm", p.M, p.N, p.K, tile,
           t.split == SPLIT_COLS ? p.col_ranges : p.splits, (p.flags & GF_UPS2) ? (t.fam == TF_CONVWS && t.var >= 4 ? " ups4" : " ups") : "", (p.flags & GF_GEGLU) ? (f8tile ? " geglu fp8" : " geglu") : (f8tile ? " fp8" : ""), p.stride == 2 ? " s2" : "",
           p.batch > 1 ? (" x" + std::to_string(p.batch)).c_str() : "");
  const double flops = 2.0 * nb * p.M * (double)p.N * k_alg;
  prog_push(c, prog, t.pk, flops, bytes, make_gemm_op(c, p, tile, bias_step_off), lab);
  if (p.splits > 1 || (t.fam == TF_CONVWS && t.var >= 2)) {  // a GroupNorm pushed next may take over the reduce (Builder::gn) -- or, behind an unsplit
    LastGemm& lg = prog->last_gemm;                // two-n-tile convws launch, get its statistics from the conv's epilogue (claim_stats)
    lg.valid = true; lg.p = p; lg.tile = tile; lg.bias_step_off = bias_step_off; lg.op_index = prog->ops.size() - 1;
    lg.kind = t.pk; lg.flops = flops; lg.bytes = bytes; lg.label = lab;
  }
  return DTP_OK;
}

int Builder::conv3(const T& x, const ConvW& w, int stride, int pad, bool ups, int Ho, int Wo, const T* resid, int bias_step_off, T& y,
                   const Conv3Opts& o) {
  if ((w.cin2 > 0) != (o.tail != nullptr) || (o.tail && o.tail->C != w.cin2)) { dtp_set_error("conv3: shortcut tail mismatch"); return DTP_ERR_ARG; }
  if (x.C != w.cin || w.taps != 9) { dtp_set_error("conv3: channel mismatch %d vs %d", x.C, w.cin); return DTP_ERR_ARG; }
  GemmParams p = {};
  p.A = x.p; p.W = w.w;
  p.M = x.B * Ho * Wo; p.N = w.cout; p.K = w.K;
  p.lda = x.ld; p.ldw = w.ldw;
  p.nkb = w.ldw / 64;
  p.Hi = x.H; p.Wi = x.W; p.Ho = Ho; p.Wo = Wo; p.Cin = w.cin; p.stride = stride; p.pad = pad;
  p.flags = GF_CONV3 | (ups ? GF_UPS2 : 0) | o.extra_flags;
  if (c->R % 64) p.flags |= GF_RAGGED;  // ragged maps: convws_kernel may cover them with partial 8 x 16 tiles
  if (o.tail) { p.A2 = o.tail->p; p.lda2 = o.tail->ld; p.Cin2 = w.cin2; }
  p.Wcb = w.wcb;
  p.Wfr = w.wfr;
  if (ups && c->ups_phase) p.Wfr4 = w.wfr4;
  if (o.extra_flags & GF_GNAPPLY) {
    if (!o.gn.part) { dtp_set_error("conv3: GF_GNAPPLY without GroupNorm parameters"); return DTP_ERR_ARG; }
    p.gn_part = o.gn.part; p.gn_gamma = o.gn.gamma; p.gn_beta = o.gn.beta; p.gn_eps = o.gn.eps;
    p.gn_nchunk = o.gn.nchunk; p.gn_cpg = o.gn.cpg; p.gn_silu = 1;
  }
  if (o.out_override) {
    y = T();
    y.p = (f16*)o.out_override; y.B = x.B; y.H = Ho; y.W = Wo; y.C = w.cout; y.ld = o.ldc_override;
  } else if (o.dst) {
    if (o.dst->C != w.cout || o.dst->rows() != (long long)x.B * Ho * Wo) { dtp_set_error("conv3: destination view mismatch"); return DTP_ERR_ARG; }
    y = *o.dst;
  } else {
    y = alloc(x.B, Ho, Wo, w.cout);
    if (!y.p) return DTP_ERR_HIP;
  }
  p.C = y.p; p.ldc = y.ld;
  if (w.b || bias_step_off >= 0) { p.flags |= GF_BIAS; p.bias = w.b; }
  if (resid) { p.flags |= GF_RESID; p.R = resid->p; p.ldr = resid->ld; }
  return push_gemm(c, prog, p, bias_step_off, 9.0 * w.cin_true + w.cin2);
}

// GroupNorm (+ SiLU) followed by a 3x3 conv.  Where the conv can run on the halo kernel and the GroupNorm is the two-launch kind
// (maps of >= 1024 pixels), the apply pass is folded into the conv (GF_GNAPPLY, conv_halo.hip): statistics pass (+ the producer's
// split-K reduce) -> conv on the RAW tensor.  Otherwise: gn() + conv3().
int Builder::gn_conv3(const T& x, const NormW& n, float eps, const ConvW& w, const T* resid, int bias_step_off, T& y, const T* tail, const T* dst) {
  Ctx* cc = c;
  const int HW = x.H * x.W, C = x.C;
  Conv3Opts opts;
  opts.tail = tail; opts.dst = dst;
  // (bigger problems -- batched stamps, the VAE at 512^2 -- are not launch-bound: there the apply pass costs less than what the
  // normalisation adds to every workgroup of the conv, and their tuned tiles are not the halo kernel's)
  const bool fuse = cc->fuse_gn_conv && HW >= 1024 && x.rows() <= 16384 && w.wcb && w.taps == 9 && (C & 63) == 0 && C <= 1024 && x.C == w.cin && (C % 32) == 0 && C / 32 >= 8 &&
                    (w.cout & 7) == 0 && (x.ld & 7) == 0;
  if (!fuse) {
    T t;
    RC(gn(x, n, eps, true, t));
    RC(conv3(t, w, 1, 1, false, x.H, x.W, resid, bias_step_off, y, opts));
    release(t);
    return DTP_OK;
  }
  const ReduceClaim claim = claim_reduce(x);
  // the partial sums outlive the statistics launch (the conv's workgroups read them while other workgroups may already write
  // split-K slabs into the shared workspace): they get their own planned buffer
  float* partials = (float*)block_clear_of_claim(cc, dtp_groupnorm_ws_bytes(x.B, HW, C, 32), claim, "gn_conv3", "partials");
  if (!partials) return DTP_ERR_HIP;
  cc->ws_need = std::max(cc->ws_need, claim.slab_bytes());
  push_gn_stats(*this, gn_params(x, n, eps, true), partials, claim, " (apply in conv)");  // (the statistics pass reads x and the shape alone)
  opts.extra_flags = GF_GNAPPLY; opts.gn = {partials, n.g, n.b, eps, dtp_groupnorm_stat_chunks(HW), C / 32};
  const int rc = conv3(x, w, 1, 1, false, x.H, x.W, resid, bias_step_off, y, opts);
  ctx_pool_put(cc, partials);
  return rc;
}

int Builder::alloc_stats(long long rows, int C, RowStats& st) {
  void* p = nullptr;
  RC(ctx_pool_get(c, (size_t)((C + 63) / 64) * rows * 2 * sizeof(float), &p));
  st.buf = (float*)p;
  st.parts = 0;
  st.M = (int)rows;
  return DTP_OK;
}
void Builder::release_stats(RowStats& st) { ctx_pool_put(c, st.buf); st.buf = nullptr; }

int Builder::linear(const T& x, const ConvW& w, const T* resid, int flags, T& y, RowStats* emit, const RowStats* use, const T* dst) {
  if (x.C != w.K || w.taps != 1) { dtp_set_error("linear: K mismatch %d vs %d", x.C, w.K); return DTP_ERR_ARG; }
  GemmParams p = {};
  p.A = x.p; p.W = w.w; p.Wfr = w.wfr;
  p.M = (int)x.rows(); p.N = w.cout; p.K = w.K;
  p.lda = x.ld; p.ldw = w.ldw; p.nkb = w.ldw / 64;
  p.flags = flags;
  if (dst) {
    if (dst->C != w.cout || (flags & GF_GEGLU) || dst->rows() != x.rows()) { dtp_set_error("linear: destination view mismatch"); return DTP_ERR_ARG; }
    y = *dst;
  } else {
    y = alloc(x.B, x.H, x.W, (flags & GF_GEGLU) ? w.cout / 2 : w.cout);
    if (!y.p) return DTP_ERR_HIP;
  }
  p.C = y.p; p.ldc = y.ld;
  if (w.b) { p.flags |= GF_BIAS; p.bias = w.b; }
  if (w.lns) {  // x is the raw pre-LayerNorm tensor
    p.flags |= GF_LNFOLD; p.lns = w.lns; p.ln_eps = 1e-5f;
    if (use && use->buf && use->parts > 0 && use->M == p.M) { p.st_in = use->buf; p.st_parts = use->parts; }
  }
  if (resid) { p.flags |= GF_RESID; p.R = resid->p; p.ldr = resid->ld; }
  if (fp8 && w.w8) {
    GemmParams q = p;
    q.W8 = w.w8; q.ldw8 = w.ldw8; q.w_scale = w.w8_scale; q.splits = 1;
    // activation scale: a LayerNorm'd operand is bounded (fixed scale); anything else is calibrated (fp8_calibrate)
    q.a_scale = (p.flags & GF_LNFOLD) ? DTP_FP8_LN_A_SCALE : DTP_FP8_LN_A_SCALE * 8.0f;
    if (dtp_gemm_fp8_supported(q)) {
      if (!(p.flags & GF_LNFOLD) && (q.K & 7) == 0) q.a_scale_host = fp8_new_linear_scale(c, &q.amax_slot1);
      p = q;  // otherwise the fp16 kernel takes it
    }
  }
  return push_gemm(c, prog, p, -1, (double)w.K, emit);
}

// ---------------------------------------------------------------- option fp8_operands: e4m3 activations in memory (gemm_f8f8.hip)
T8 Builder::alloc8(const T& like, int C, bool calibrated, float fixed_scale) {
  T8 t;
  t.B = like.B; t.H = like.H; t.W = like.W; t.C = C; t.ld = (C + 15) & ~15;
  void* p = nullptr;
  if (ctx_pool_get(c, (size_t)t.rows() * t.ld, &p) != DTP_OK) p = nullptr;
  t.p = (unsigned char*)p;
  t.scale = fixed_scale;
  if (calibrated) {
    t.scale_host = fp8_new_linear_scale(c, &t.amax_slot1);
    if (!t.scale_host) t.scale = DTP_FP8_LN_A_SCALE * 8.0f;  // calibration slots used up: the default scale of fp8_linear
  }
  return t;
}
void Builder::release8(const T8& t) { ctx_pool_put(c, t.p); }

int Builder::quant8(const T& x, const T8& y, bool ln, const RowStats* st) {
  if (!y.p) return DTP_ERR_HIP;
  if (x.C != y.C || x.rows() != y.rows()) { dtp_set_error("quant8: shape mismatch"); return DTP_ERR_ARG; }
  Quant8Params q = {};
  q.M = (int)x.rows(); q.njobs = 1; q.eps = 1e-5f;
  q.job[0] = Quant8Job{x.p, x.ld, x.C, y.p, y.ld, y.scale, ln ? 1 : 0};
  if (ln && st && st->buf && st->parts > 0 && st->M == q.M) { q.st_in = st->buf; q.st_parts = st->parts; q.st_rows = q.M; }
  if (!dtp_quant8_supported(q)) { dtp_set_error("quant8: unsupported problem (M %d, K %d)", q.M, x.C); return DTP_ERR_ARG; }
  const T8 ya = y;
  Ctx* cc = c;
  push(PK_QUANT8, 0.0, 3.0 * q.M * x.C, [=](hipStream_t s, int) -> int {
    Quant8Params r = q;
    r.job[0].scale = ya.now();
    if (cc->calibrating && ya.amax_slot1 > 0 && !ln)  // a raw operand with a calibrated scale: measure it once
      RC(dtp_launch_amax_f16(r.job[0].x, r.M, r.job[0].K, r.job[0].ld, cc->fp8_amax + ya.amax_slot1 - 1, s));
    return dtp_launch_quant8(r, s);
  }, "quant8 M=" + std::to_string(q.M) + " K=" + std::to_string(x.C) + (ln ? " ln" : ""));
  return DTP_OK;
}

int Builder::linear8(const T8& x, const ConvW& w, const T* resid, int flags, T& y, RowStats* emit) {
  if (x.C != w.K || w.taps != 1 || !w.w8) { dtp_set_error("linear8: operand mismatch (K %d vs %d)", x.C, w.K); return DTP_ERR_ARG; }
  const int n_out = (flags & GF_GEGLU) ? w.cout / 2 : w.cout;
  GemmParams p = {};
  p.A8 = x.p; p.lda8 = x.ld;
  p.W8 = w.w8; p.ldw8 = w.ldw8; p.w_scale = w.w8_scale;
  p.M = (int)x.rows(); p.N = w.cout; p.K = x.C;
  p.flags = flags;
  p.zero = c->zero; p.splits = 1;
  p.a_scale = x.scale; p.a_scale_host = x.scale_host;  // (the producer of x measured its range: no amax slot here)
  y = alloc(x.B, x.H, x.W, n_out);
  if (!y.p) return DTP_ERR_HIP;
  p.C = y.p; p.ldc = y.ld;
  if (w.b) { p.flags |= GF_BIAS; p.bias = w.b; }
  if (resid) { p.flags |= GF_RESID; p.R = resid->p; p.ldr = resid->ld; }
  if (emit_rowstats(p, emit)) { emit->parts = (p.N + 127) / 128; emit->M = p.M; }  // (no push_gemm here: one partial per 128-column tile)
  if (!dtp_gemm_f8f8_supported(p)) { dtp_set_error("linear8: unsupported problem (M %d N %d K %d)", p.M, p.N, p.K); return DTP_ERR_ARG; }
  const int tile = dtp_gemm_f8f8_pick(p, c->num_cu);
  char lab[160];
  snprintf(lab, sizeof(lab), "f8f8 M=%d N=%d K=%d tile=%d%s", p.M, p.N, p.K, tile, (flags & GF_GEGLU) ? " geglu" : "");
  // algorithmic work: 2*M*N*K; bytes = both e4m3 operands once + the fp16 output once
  const double bytes = (double)p.M * p.K + (double)p.N * p.K + 2.0 * p.M * n_out;
  push(PK_F8F8, 2.0 * p.M * (double)p.N * p.K, bytes, [=](hipStream_t s, int) -> int {
    GemmParams q = p;
    if (p.a_scale_host) q.a_scale = *p.a_scale_host;
    return dtp_launch_gemm_f8f8(q, tile, s);
  }, lab);
  return DTP_OK;
}

int Builder::linear_f8ops(const T& x, const ConvW& w, const T* resid, int flags, T& y, RowStats* emit, RowStats* ln, bool release_ln) {
  if (f8ops && w.K >= DTP_FP8_OPERANDS_MIN_K && w.w8) {
    const T8 x8 = ln ? alloc8(x, x.C, false, DTP_FP8_LN_A_SCALE) : alloc8(x, x.C, true);
    RC(quant8(x, x8, ln != nullptr, ln));
    if (ln && release_ln) release_stats(*ln);
    RC(linear8(x8, w, resid, flags, y, emit));
    release8(x8);
    return DTP_OK;
  }
  RC(linear(x, w, resid, flags, y, emit, ln));
  if (ln && release_ln) release_stats(*ln);
  return DTP_OK;
}

int Builder::attention(const T& q, const T& k, const T& v, int heads, int Sq, int Skv, int Bn, T& o) {
  o = alloc(Bn, 1, Sq, q.C);
  if (!o.p) return DTP_ERR_HIP;
  AttnParams a;
  a.Q = q.p; a.K = k.p; a.V = v.p; a.O = o.p;
  a.ldq = q.ld; a.ldk = k.ld; a.ldv = v.ld; a.ldo = o.ld;
  a.B = Bn; a.H = heads; a.Sq = Sq; a.Skv = Skv; a.D = q.C / heads;
  a.qbs = (long long)Sq * q.ld; a.kbs = (long long)Skv * k.ld; a.vbs = (long long)Skv * v.ld; a.obs = (long long)Sq * o.ld;
  a.scale = 1.0f / sqrtf((float)a.D);
  const bool fp8 = c->fp8_attention && (a.D % 64) != 0 && a.D <= 184 && Skv >= 64;  // the brush encoder's tiny attentions stay f16
  const float *qs = nullptr, *vs = nullptr;
  int slot0 = -1;
  if (fp8 && c->fp8_nslots + 3 <= DTP_FP8_SLOTS && (q.C & 7) == 0) {  // calibrated Q / K and V scales (fp8_calibrate)
    Ctx* cc0 = c;
    cc0->fp8_scales.push_back(1.0f); float* s0 = &cc0->fp8_scales.back();
    cc0->fp8_scales.push_back(1.0f); float* s1 = &cc0->fp8_scales.back();
    Fp8Cal r;
    r.kind = 1; r.slot0 = cc0->fp8_nslots; r.s0 = s0; r.s1 = s1; r.softmax_scale = a.scale;
    cc0->fp8_cals.push_back(r);
    slot0 = cc0->fp8_nslots;
    cc0->fp8_nslots += 3;
    qs = s0; vs = s1;
  }
  Ctx* cc = c;
  const T qq = q, kk = k, vv = v;
  push(PK_ATTN, 4.0 * Bn * heads * (double)Sq * Skv * a.D, 2.0 * Bn * q.C * (2.0 * Sq + 2.0 * Skv),
       [=](hipStream_t s, int) {
         if (!fp8) return dtp_launch_attention(a, s);
         if (cc->calibrating && slot0 >= 0) {
           RC(dtp_launch_amax_f16(qq.p, (long long)Bn * Sq, qq.C, qq.ld, cc->fp8_amax + slot0, s));
           RC(dtp_launch_amax_f16(kk.p, (long long)Bn * Skv, kk.C, kk.ld, cc->fp8_amax + slot0 + 1, s));
           RC(dtp_launch_amax_f16(vv.p, (long long)Bn * Skv, vv.C, vv.ld, cc->fp8_amax + slot0 + 2, s));
         }
         return dtp_launch_attention_fp8(a, qs ? *qs : 1.0f, vs ? *vs : 1.0f, s);
       },
       "attn B=" + std::to_string(Bn) + " Sq=" + std::to_string(Sq) + " Skv=" + std::to_string(Skv) + " D=" + std::to_string(a.D) +
           (!fp8 && dtp_attention_uses_dma(a) ? " dma" : ""));
  return DTP_OK;
}

int Builder::concat(const T& a, const T& b, T& y) {
  y = alloc(a.B, a.H, a.W, a.C + b.C);
  if (!y.p) return DTP_ERR_HIP;
  const T aa = a, bb = b, yy = y;
  push(PK_ELEM, 0.0, 4.0 * (double)aa.rows() * (aa.C + bb.C), [=](hipStream_t s, int) {
    return dtp_launch_concat_channels(aa.p, aa.ld, aa.C, bb.p, bb.ld, bb.C, yy.p, yy.ld, aa.rows(), s);
  });
  return DTP_OK;
}

int Builder::resnet(const T& x, const ResW& w, float eps, bool temb, T& y, const T* dst) {
  T h;
  RC(gn_conv3(x, w.n1, eps, w.c1, nullptr, temb ? w.temb_off : -1, h, nullptr, nullptr));
  if (w.has_sc) {  // conv2 and the 1x1 shortcut are one contraction: [im2col(GN(h)) | x] . [W2 | Wsc]^T
    RC(gn_conv3(h, w.n2, eps, w.c2, nullptr, -1, y, &x, dst));
  } else {
    RC(gn_conv3(h, w.n2, eps, w.c2, &x, -1, y, nullptr, dst));
  }
  release(h);
  return DTP_OK;
}
