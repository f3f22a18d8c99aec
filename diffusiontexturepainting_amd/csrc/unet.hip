// SD-1.5-inpainting UNet on the libdtp kernels: weight loading (with LoRA merge), the static
// launch program, and the `unet` engine entry point.
// Reference: trt_inference/models.py:1017-1139 (model + LoRA merge + engine I/O); topology
// SURVEY.md Appendix A.1.
#include <math.h>

#include "engine.h"

static const int CH[4] = {320, 640, 1280, 1280};

static int load_res(Ctx* c, const std::string& p, ResW& w, bool temb, int& temb_off_acc, std::vector<std::string>* tnames) {
  RC(load_norm(c, p + ".norm1", w.n1));
  RC(load_conv(c, p + ".conv1", w.c1));
  RC(load_norm(c, p + ".norm2", w.n2));
  w.has_sc = ctx_find(c, p + ".conv_shortcut.weight") != nullptr;
  if (w.has_sc) RC(load_conv_with_shortcut(c, p + ".conv2", p + ".conv_shortcut", w.c2));
  else RC(load_conv(c, p + ".conv2", w.c2));
  if (temb) {
    w.temb_off = temb_off_acc;
    temb_off_acc += w.c1.cout;
    tnames->push_back(p);
  }
  return DTP_OK;
}

static int load_xf(Ctx* c, const std::string& p, XfW& w, int& kv_counter) {
  const std::string t = p + ".transformer_blocks.0";
  RC(load_norm(c, p + ".norm", w.gn));
  RC(load_conv(c, p + ".proj_in", w.proj_in));
  RC(load_norm(c, t + ".norm1", w.ln1));
  RC(load_norm(c, t + ".norm2", w.ln2));
  RC(load_norm(c, t + ".norm3", w.ln3));
  // the three LayerNorms are folded into the Linear that consumes them (GF_LNFOLD): no LN kernel, no LN tensor
  RC(load_linear(c, {t + ".attn1.to_q", t + ".attn1.to_k", t + ".attn1.to_v"}, w.qkv, false, false, t + ".norm1"));
  RC(load_linear(c, {t + ".attn1.to_out.0"}, w.out1, true));
  RC(load_linear(c, {t + ".attn2.to_q"}, w.q2, false, false, t + ".norm2"));
  RC(load_linear(c, {t + ".attn2.to_k", t + ".attn2.to_v"}, w.kv2, false));
  RC(load_linear(c, {t + ".attn2.to_out.0"}, w.out2, true));
  RC(load_linear(c, {t + ".ff.net.0.proj"}, w.ff1, true, true, t + ".norm3"));
  RC(load_linear_pair(c, t + ".ff.net.2", p + ".proj_out", w.ff2_proj));
  w.kv_index = kv_counter++;
  {  // transposed copy of the folded to_q for the per-stamp score-matrix GEMM (rows = input channel, K = output channel)
    const int C = w.q2.K, rows = (C + 127) / 128 * 128, ld = (C + 63) / 64 * 64;
    void* pq;
    RC(ctx_arena_alloc(c, (size_t)rows * ld * 2, &pq));
    HIP_CHECK(hipMemsetAsync(pq, 0, (size_t)rows * ld * 2, 0));
    w.q2T = (f16*)pq;
    RC(dtp_launch_transpose_f16(w.q2.w, w.q2.ldw, w.q2T, ld, w.q2.cout, C, 0));
    c->refit_transposes.push_back({w.q2.w, w.q2T, w.q2.ldw, ld, w.q2.cout, C});
  }
  // LoRA refit targets (lora_refit.hip): the eight attention matrices, each with the packed buffer, the row offset inside a stack and the
  // LayerNorm fold it was loaded with above -- every copy a program reads (xchain_kernel reads out1.w itself; q2T, lns and the folded
  // biases are derived from the rewritten rows by the kernels that made them here)
  auto target = [&](const std::string& name, ConvW& cw, int row0, const NormW* fold) -> int {
    const std::string key = name + ".weight";
    auto it = c->refit_base.find(key);
    const Staged* s = ctx_find(c, key);
    if (it == c->refit_base.end() || !s) { dtp_set_error("LoRA refit: no base copy of '%s'", key.c_str()); return DTP_ERR_MISSING; }
    RefitTarget rt;
    rt.name = key;
    rt.job = LoraRefitJob{};
    rt.job.base = it->second; rt.job.N = (int)s->shape[0]; rt.job.K = (int)s->shape[1];
    rt.job.dst = cw.w; rt.job.ldw = cw.ldw; rt.job.row0 = row0;
    if (fold) { rt.job.gamma = fold->g; rt.job.beta = fold->b; rt.job.wbeta = cw.b + row0; }
    c->refit_targets.push_back(rt);
    return DTP_OK;
  };
  const int C = w.q2.K;
  RC(target(t + ".attn1.to_q", w.qkv, 0, &w.ln1));
  RC(target(t + ".attn1.to_k", w.qkv, C, &w.ln1));
  RC(target(t + ".attn1.to_v", w.qkv, 2 * C, &w.ln1));
  RC(target(t + ".attn1.to_out.0", w.out1, 0, nullptr));
  RC(target(t + ".attn2.to_q", w.q2, 0, &w.ln2));
  RC(target(t + ".attn2.to_k", w.kv2, 0, nullptr));
  RC(target(t + ".attn2.to_v", w.kv2, C, nullptr));
  RC(target(t + ".attn2.to_out.0", w.out2, 0, nullptr));
  c->refit_rowsums.push_back({w.qkv.w, w.qkv.lns, w.qkv.ldw, w.qkv.K, (w.qkv.cout + 127) / 128 * 128});
  c->refit_rowsums.push_back({w.q2.w, w.q2.lns, w.q2.ldw, w.q2.K, (w.q2.cout + 127) / 128 * 128});
  return DTP_OK;
}

// fp32 copies of the LoRA-targetable matrices as staged, i.e. BEFORE merge_lora adds to them: what dtp_refit_lora rebuilds from
static int keep_refit_bases(Ctx* c) {
  for (auto& kv : c->staged) {
    const std::string& k = kv.first;
    if (k.rfind("unet.", 0) != 0 || k.find(".transformer_blocks.0.attn") == std::string::npos || kv.second.shape.size() != 2) continue;
    const size_t n = k.size();
    const bool proj = (n > 12 && (k.compare(n - 12, 12, ".to_q.weight") == 0 || k.compare(n - 12, 12, ".to_k.weight") == 0 ||
                                  k.compare(n - 12, 12, ".to_v.weight") == 0)) ||
                      (n > 16 && k.compare(n - 16, 16, ".to_out.0.weight") == 0);
    if (!proj) continue;
    void* p;
    RC(ctx_arena_alloc(c, kv.second.n * 4, &p));
    HIP_CHECK(hipMemcpy(p, kv.second.d, kv.second.n * 4, hipMemcpyDeviceToDevice));
    c->refit_base[k] = (float*)p;
  }
  return DTP_OK;
}

// W += 1.0 * up @ down for q/k/v/out of every attention module that has LoRA tensors staged
// (trt_inference/models.py:1070-1086).  Operates on the staged fp32 tensors, before packing.
static int merge_lora(Ctx* c) {
  std::vector<std::string> keys;
  for (auto& kv : c->staged)
    if (kv.first.rfind("lora.", 0) == 0 && kv.first.find("_lora.down.weight") != std::string::npos) keys.push_back(kv.first);
  for (const std::string& k : keys) {
    // lora.<module>.processor.<proj>_lora.down.weight
    const size_t pp = k.find(".processor.");
    if (pp == std::string::npos) continue;
    const std::string module = k.substr(5, pp - 5);
    const size_t ps = pp + 11, pe = k.find("_lora.down.weight");
    const std::string proj = k.substr(ps, pe - ps);
    const std::string upk = "lora." + module + ".processor." + proj + "_lora.up.weight";
    const std::string tgt = "unet." + module + (proj == "to_out" ? ".to_out.0.weight" : "." + proj + ".weight");
    const Staged *dn = ctx_find(c, k), *up = ctx_find(c, upk), *w = ctx_find(c, tgt);
    if (!up || !w) { dtp_set_error("LoRA: missing '%s' or target '%s'", upk.c_str(), tgt.c_str()); return DTP_ERR_MISSING; }
    const int rank = (int)dn->shape[0], K = (int)dn->shape[1], N = (int)up->shape[0];
    if ((int)w->shape[0] != N || (int)w->shape[1] != K || (int)up->shape[1] != rank) {
      dtp_set_error("LoRA: shape mismatch for '%s'", tgt.c_str());
      return DTP_ERR_ARG;
    }
    RC(dtp_launch_lora_merge(w->d, up->d, dn->d, N, K, rank, 1.0f, 0));
  }
  HIP_CHECK(hipDeviceSynchronize());
  return DTP_OK;
}

int load_unet_weights(Ctx* c) {
  RC(keep_refit_bases(c));
  RC(merge_lora(c));
  struct WsScope {  // the UNet's 3x3 convs also get the fragment-order packing (conv_ws.hip)
    Ctx* c;
    explicit WsScope(Ctx* cc) : c(cc) { c->pack_ws = c->conv_ws; }
    ~WsScope() { c->pack_ws = false; }
  } ws_scope(c);
  UNetW& u = c->unet;
  const std::string P = "unet.";
  int toff = 0, kvn = 0;
  std::vector<std::string> tn;
  RC(load_conv(c, P + "conv_in", u.conv_in, 16));
  RC(load_linear(c, {P + "time_embedding.linear_1"}, u.t1, true));
  RC(load_linear(c, {P + "time_embedding.linear_2"}, u.t2, true));
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) {
      RC(load_res(c, P + "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), u.down_res[i][j], true, toff, &tn));
      if (i < 3) RC(load_xf(c, P + "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), u.down_xf[i][j], kvn));
    }
    if (i < 3) RC(load_conv(c, P + "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", u.down_conv[i]));
  }
  RC(load_res(c, P + "mid_block.resnets.0", u.mid_res[0], true, toff, &tn));
  RC(load_xf(c, P + "mid_block.attentions.0", u.mid_xf, kvn));
  RC(load_res(c, P + "mid_block.resnets.1", u.mid_res[1], true, toff, &tn));
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) {
      RC(load_res(c, P + "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), u.up_res[i][j], true, toff, &tn));
      if (i > 0) RC(load_xf(c, P + "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), u.up_xf[i][j], kvn));
    }
    if (i < 3) {
      RC(load_conv(c, P + "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", u.up_conv[i]));
      RC(load_conv_ups4(c, P + "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", u.up_conv[i]));
    }
  }
  RC(load_norm(c, P + "conv_norm_out", u.norm_out));
  RC(load_conv(c, P + "conv_out", u.conv_out));
  // all time_emb_proj stacked into one [temb_total][1280] GEMM; its bias also carries conv1.bias so the
  // per-step table row is directly the conv1 bias of every ResBlock
  u.temb_total = toff;
  std::vector<std::string> names;
  for (auto& p : tn) names.push_back(p + ".time_emb_proj");
  RC(load_linear(c, names, u.tproj, false));
  std::vector<float> bias;
  for (auto& p : tn) {
    std::vector<float> a, b;
    RC(ctx_fetch_host(c, p + ".time_emb_proj.bias", a));
    RC(ctx_fetch_host(c, p + ".conv1.bias", b));
    for (size_t i = 0; i < a.size(); ++i) bias.push_back(a[i] + b[i]);
  }
  bias.resize((bias.size() + 127) / 128 * 128, 0.f);
  RC(ctx_upload_f32(c, bias, &u.tproj.b));
  return DTP_OK;
}

// timestep embedding -> per-step conv1 bias rows.  Host sinusoid (flip_sin_to_cos, shift 0), then
// three GEMMs: linear_1+SiLU, linear_2+SiLU (every consumer applies SiLU first), stacked projections.
int ensure_temb(Ctx* c, const std::vector<float>& timesteps) {
  const int n = (int)timesteps.size();
  if (n > 1000) { dtp_set_error("temb: too many timesteps"); return DTP_ERR_ARG; }
  if (n > c->temb_rows) {
    const int rows = 1000;  // fixed capacity: captured graphs keep pointers into this table
    void* p;
    RC(ctx_persistent(c, (size_t)rows * c->unet.temb_total * 4, &p, true)); c->temb_table = (float*)p;
    RC(ctx_persistent(c, (size_t)rows * 320 * 2, &p, true)); c->temb_sin = (f16*)p;
    RC(ctx_persistent(c, (size_t)rows * 1280 * 2, &p, true)); c->temb_h1 = (f16*)p;
    RC(ctx_persistent(c, (size_t)rows * 1280 * 2, &p, true)); c->temb_h2 = (f16*)p;
    c->temb_rows = rows;
  }
  std::vector<f16> sin_tab((size_t)n * 320);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 160; ++j) {
      const float f = expf(-logf(10000.0f) * (float)j / 160.0f);
      const float a = timesteps[i] * f;
      sin_tab[(size_t)i * 320 + j] = (f16)cosf(a);
      sin_tab[(size_t)i * 320 + 160 + j] = (f16)sinf(a);
    }
  HIP_CHECK(hipMemcpy(c->temb_sin, sin_tab.data(), sin_tab.size() * 2, hipMemcpyHostToDevice));
  auto gemm = [&](const f16* A, const ConvW& w, void* C, int flags) -> int {
    GemmParams p = {};
    p.A = A; p.W = w.w; p.C = C; p.bias = w.b; p.zero = c->zero;
    p.M = n; p.N = w.cout; p.K = w.K; p.lda = w.K; p.ldw = w.ldw; p.ldc = w.cout; p.nkb = w.ldw / 64;
    p.flags = flags | GF_BIAS;
    p.splits = 1; p.kb_per_split = p.nkb;
    return dtp_launch_gemm(p, p.M > 64 ? 0 : 3, 0);
  };
  RC(gemm(c->temb_sin, c->unet.t1, c->temb_h1, GF_SILU));
  RC(gemm(c->temb_h1, c->unet.t2, c->temb_h2, GF_SILU));
  RC(gemm(c->temb_h2, c->unet.tproj, c->temb_table, GF_OUT_F32));
  HIP_CHECK(hipDeviceSynchronize());
  return DTP_OK;
}

// sub-batch view: samples [first, first + count) of an NHWC tensor
static T samples(const T& t, int first, int count) {
  T v = t;
  v.p += (size_t)first * t.H * t.W * t.ld;
  v.B = count;
  return v;
}

// De-duplicated prefix (Dup): the uncond and cond branches of a stamp feed the UNet IDENTICAL samples (inpaint_pipeline.py:115,136,
// stable_diffusion_pipeline.py:423: cat([latents] * 3), cat([mask, mask, ctx_mask]), cat([ml, ml, ctx_ml])) and first differ in
// encoder_hidden_states, i.e. at the first cross-attention.  Everything before it -- conv_in, down_blocks.0.resnets.0, the first
// transformer's GroupNorm / proj_in / self-attention -- is evaluated for samples [dupB, N) only (batch order [uncond | cond | tg]:
// one contiguous range) and the uncond rows [0, dupB) of the three tensors that live on (the conv_in skip, the transformer input,
// the self-attention output with its LayerNorm statistics) are filled by ONE row-copy launch: bit-identical results.
struct Dup {
  int B = 0;       // samples filled by duplication (0 = off)
  T x_full;        // the transformer input for all N samples (x below is its [B, N) view)
  T skip_full;     // the conv_in skip view for all N samples (channel slice of a concat buffer)
};

// One row-copy launch of the de-duplicated prefix: uncond rows <- cond rows of the conv_in skip and the block input, and of the
// self-attention output y2 and its row statistics st2 where the caller has those in memory
static void push_dup_copy(Builder& b, const Dup& d, int S, const T* y2 = nullptr, const RowStats* st2 = nullptr) {
  const long long rB = (long long)d.B * S;
  CopySegs cs = {};
  auto seg = [&](const void* src, void* dstp, long long rows, long long row_bytes, long long stride) {
    cs.src[cs.n] = (const char*)src; cs.dst[cs.n] = (char*)dstp; cs.rows[cs.n] = rows; cs.row_bytes[cs.n] = row_bytes;
    cs.src_stride[cs.n] = cs.dst_stride[cs.n] = stride; ++cs.n;
  };
  auto rows = [&](const T& t) { seg(t.p + rB * t.ld, t.p, rB, (long long)t.C * 2, (long long)t.ld * 2); };
  rows(d.skip_full); rows(d.x_full);
  if (y2) rows(*y2);
  if (st2) seg(st2->buf + rB * 2, st2->buf, st2->parts, rB * 8, (long long)st2->M * 8);
  double bytes = 0;
  for (int k = 0; k < cs.n; ++k) bytes += 2.0 * cs.rows[k] * cs.row_bytes[k];
  b.push(PK_ELEM, 0.0, bytes, [=](hipStream_t s, int) { return dtp_launch_copy_rows(cs, s); }, "dup uncond<-cond rows=" + std::to_string(rB));
}

// the block output: the caller's destination view, or a fresh buffer -- shaped like `like`
static int block_out(Builder& b, const T* dst, const T& like, T& out) {
  if (dst) {
    if (dst->C != like.C || dst->rows() != like.rows()) { dtp_set_error("transformer: destination view mismatch"); return DTP_ERR_ARG; }
    out = *dst;
    return DTP_OK;
  }
  out = b.alloc(like.B, like.H, like.W, like.C);
  return out.p ? DTP_OK : DTP_ERR_HIP;
}

// One SD transformer block in three stages.  LayerNorms are folded into their consumer GEMMs; the row statistics ride on the producer's
// epilogue.  Option fp8_operands: q/k/v, to_out and FF1 with K >= DTP_FP8_OPERANDS_MIN_K (the C = 1280 blocks; no de-duplicated prefix
// reaches them) contract two e4m3 operands (gemm_f8f8.hip, Builder::linear_f8ops).  A LayerNorm'd operand is quantised AFTER the
// normalisation (fixed scale; gamma / beta stay folded into the packed weights / bias, so its consumer is a plain GF_BIAS GEMM); the
// attention output gets a calibrated scale.

// Stage 1: GroupNorm + proj_in -> y (with the LayerNorm-1 statistics), q/k/v (LN1 folded), self-attention -> a
static int self_attention(Builder& b, const T& x, const XfW& w, T& y, T& a) {
  const int C = x.C, S = x.H * x.W;
  const bool fold_gn = b.gn_linear_supported(x, w.proj_in);  // levels 0-1: the GroupNorm becomes per-sample proj_in weights (Builder::gn_linear)
  RowStats st1;
  RC(b.alloc_stats(x.rows(), C, st1));
  if (fold_gn) {
    RC(b.gn_linear(x, w.gn, 1e-6f, w.proj_in, y, &st1));
  } else {
    T t;
    RC(b.gn(x, w.gn, 1e-6f, false, t));
    RC(b.linear(t, w.proj_in, nullptr, 0, y, &st1));
    b.release(t);
  }
  T qkv;
  RC(b.linear_f8ops(y, w.qkv, nullptr, 0, qkv, nullptr, &st1, false));  // LN1 folded (e4m3: quantised after LN1)
  b.release_stats(st1);
  T q = qkv, k = qkv, v = qkv;
  q.C = k.C = v.C = C;
  k.p += C; v.p += 2 * C;
  RC(b.attention(q, k, v, 8, S, S, x.B, a));
  b.release(qkv);
  a.B = x.B; a.H = x.H; a.W = x.W;
  return DTP_OK;
}

// Stage 2: to_out (+ y), LayerNorm-2 and the cross-attention over the 14 context tokens (+ its residual) -> y3 with the LayerNorm-3
// statistics st3, for all N samples.  a and y go back to the pool.
static int cross_attention(Builder& b, const T& x, const XfW& w, const UNetProg& up, const Dup* dup, const T& a, const T& y, T& y3, RowStats& st3) {
  const int dB = dup ? dup->B : 0;
  const int C = x.C, S = x.H * x.W, N = x.B + dB, i = w.kv_index, Cp = (C + 127) / 128 * 128;  // x holds the samples evaluated so far
  // Round 6: at level 0 (C = 320) the output projection, its residual, LayerNorm-2 and the whole fused cross-attention run as ONE
  // register-chained launch (xchain.hip): y2 and its row statistics never reach memory.  With a de-duplicated prefix the uncond samples
  // read the cond samples' rows of a and y (the kernel's `dup`): their y2 is recomputed instead of copied.  The launch has one workgroup
  // per 128 rows: it is used where that is at least a quarter of the CUs (512^2: 96 at batch 1; not the 24 of a 256^2 stamp, where the
  // two well-parallelised launches it replaces are faster: +2 % per stamp measured).  (Ctx::xchain off: the two launches, A/B.)
  XchainParams xc = {};
  xc.A = a.p; xc.lda = a.ld; xc.Wo = w.out1.w; xc.ldwo = w.out1.ldw; xc.bo = w.out1.b; xc.Y = y.p; xc.ldy = y.ld;
  xc.W1 = up.xW1[i]; xc.w1_bs = (long long)128 * C; xc.b1 = up.xb1[i]; xc.lns1 = up.xl1[i];
  xc.W2 = up.xW2[i]; xc.w2_bs = (long long)Cp * 128; xc.b2 = w.out2.b;
  xc.S = S; xc.C = C; xc.N = N; xc.sm_valid = 14; xc.ln_eps = 1e-5f; xc.dup = dB;
  xc.Y3 = a.p; xc.ldy3 = C;  // (placeholder for the support check)
  const bool chain = b.c->xchain && b.c->fuse_xattn && !b.fp8 && w.out1.K == C && w.out1.cout == C && !w.out1.lns &&
                     (long long)(S / 128) * N >= b.c->num_cu / 4 && dtp_xchain_supported(xc);
  RowStats st2;
  RC(b.alloc_stats((long long)N * S, C, st2));
  if (chain) {
    b.release_stats(st2);
    RC(b.alloc_stats((long long)N * S, C, st3));
    y3 = b.alloc(N, x.H, x.W, C);
    if (!y3.p) return DTP_ERR_HIP;
    xc.Y3 = y3.p; xc.ldy3 = y3.ld; xc.st_out = st3.buf;
    st3.parts = 1; st3.M = N * S;
    b.push(PK_XATTN, 2.0 * N * S * ((double)C * C + 2.0 * 128.0 * C), 2.0 * N * (3.0 * S * C + (double)C * C + 2.0 * 128 * C),
           [=](hipStream_t s, int) { return dtp_launch_xchain(xc, s); }, "xchain M=" + std::to_string(S) + " C=" + std::to_string(C) + " x" + std::to_string(N));
    if (dB > 0) push_dup_copy(b, *dup, S);  // the other two tensors the branches share
    b.release(a); b.release(y);
    return DTP_OK;
  }
  T y2;
  if (dB > 0) {  // to_out over the evaluated samples, then the uncond rows of everything the branches share by one row copy
    y2 = b.alloc(N, x.H, x.W, C);
    if (!y2.p) return DTP_ERR_HIP;
    const T y2s = samples(y2, dB, x.B);
    st2.rows_total = N * S; st2.row_off = dB * S;
    T y2v;
    RC(b.linear(a, w.out1, &y, 0, y2v, &st2, nullptr, &y2s));
    st2.M = N * S;
    push_dup_copy(b, *dup, S, &y2, &st2);
  } else {
    RC(b.linear_f8ops(a, w.out1, &y, 0, y2, &st2, nullptr, false));  // (e4m3: the attention output, calibrated)
  }
  b.release(a); b.release(y);
  // Cross-attention over 14 context tokens: softmax_j(LN2(y2) Wq'^T K^T) V Wo^T collapses to two grouped GEMMs against
  // per-sample matrices prepared once per stamp (UNetProg::xW1 / xW2): scores + group softmax, then the value-output product.
  XattnParams xp = {};
  xp.X = y2.p; xp.ldx = y2.ld; xp.W1 = up.xW1[i]; xp.w1_bs = (long long)128 * C; xp.b1 = up.xb1[i]; xp.lns1 = up.xl1[i];
  xp.st_in = st2.buf; xp.st_parts = st2.parts; xp.st_rows = N * S; xp.ln_eps = 1e-5f;
  xp.W2 = up.xW2[i]; xp.w2_bs = (long long)Cp * 128; xp.b2 = w.out2.b; xp.R = y2.p; xp.ldr = y2.ld;
  xp.S = S; xp.C = C; xp.N = N; xp.sm_valid = 14; xp.zero = b.c->zero;
  // The fused kernel recomputes the score tile once per 128-column tile of the output: it pays where the pair is launch-bound (few
  // workgroups: levels 1-3 of a batch-1 stamp, every level at 256^2) and loses where the grid already fills the chip several times
  // (level 0 at 512^2: +1.3 ms per stamp; batch 8: +17 ms per batch with everything fused -- same-box A/B).
  // Round 5: a workgroup may take several column tiles (one probability tile, no recomputation) -- taken when the whole launch is then a
  // single round of workgroups (level 0 at batch 1: 64 row blocks x 3 samples x all three tiles = 192 workgroups, one launch instead of
  // two grouped GEMMs); otherwise one tile per workgroup under the old gate (and always with Ctx::xattn_tiles off, A/B).
  const int nt = (C + 127) / 128;
  int ct = dtp_xattn_tiles_per_wg(S, C, N);
  if (!b.c->xattn_tiles || (long long)((S + 63) / 64) * ((nt + ct - 1) / ct) * N > b.c->num_cu) ct = 1;
  xp.ct = ct;
  const long long xa_wgs = (long long)((S + 63) / 64) * ((nt + ct - 1) / ct) * N;
  const bool fused = b.c->fuse_xattn && xa_wgs <= 2LL * b.c->num_cu && st2.buf && st2.parts > 0 && st2.M == N * S && dtp_xattn_supported(xp);
  if (fused) {
    // one launch: scores + group softmax + value-output product + residual (xattn.hip); the probabilities never leave LDS
    RC(b.alloc_stats((long long)N * S, C, st3));
    y3 = b.alloc(N, x.H, x.W, C);
    if (!y3.p) return DTP_ERR_HIP;
    xp.Y = y3.p; xp.ldy = y3.ld; xp.st_out = st3.buf;
    st3.parts = (C + 127) / 128; st3.M = N * S;
    const double tiles = (double)((nt + ct - 1) / ct);  // the scores are computed once per workgroup
    b.push(PK_XATTN, 2.0 * N * S * 128.0 * C * (tiles + 1.0), 2.0 * N * (3.0 * S * C + 2.0 * 128 * C),
           [=](hipStream_t s, int) { return dtp_launch_xattn(xp, s); }, "xattn M=" + std::to_string(S) + " C=" + std::to_string(C) + " x" + std::to_string(N) + (ct > 1 ? " ct=" + std::to_string(ct) : ""));
    b.release_stats(st2);
    b.release(y2);
    return DTP_OK;
  }
  T pm = b.alloc(N, x.H, x.W, 128);  // probabilities [rows][8 heads x 16 (14 valid)]
  if (!pm.p) return DTP_ERR_HIP;
  GemmParams g = {};
  g.A = y2.p; g.W = up.xW1[i]; g.C = pm.p;
  g.M = S; g.N = 128; g.K = C; g.lda = y2.ld; g.ldw = C; g.ldc = pm.ld; g.nkb = C / 64;
  g.bias = up.xb1[i]; g.lns = up.xl1[i]; g.ln_eps = 1e-5f;
  g.flags = GF_BIAS | GF_LNFOLD | GF_SOFTMAX16; g.sm_valid = 14;
  g.batch = N; g.a_bs = (long long)S * y2.ld; g.w_bs = (long long)128 * C; g.c_bs = (long long)S * pm.ld; g.bias_bs = 128; g.lns_bs = 128;
  if (st2.buf && st2.parts > 0 && st2.M == N * S) { g.st_in = st2.buf; g.st_parts = st2.parts; g.st_rows = N * S; }
  RC(push_gemm(b.c, b.prog, g, -1, (double)C, nullptr));
  b.release_stats(st2);
  RC(b.alloc_stats((long long)N * S, C, st3));
  y3 = b.alloc(N, x.H, x.W, C);
  if (!y3.p) return DTP_ERR_HIP;
  GemmParams h = {};
  h.A = pm.p; h.W = up.xW2[i]; h.C = y3.p;
  h.M = S; h.N = C; h.K = 128; h.lda = pm.ld; h.ldw = 128; h.ldc = y3.ld; h.nkb = 2;
  h.bias = w.out2.b; h.R = y2.p; h.ldr = y2.ld;
  h.flags = (w.out2.b ? GF_BIAS : 0) | GF_RESID | (st3.buf ? GF_ROWSTATS : 0);
  h.st_out = st3.buf; h.st_rows = N * S;
  h.batch = N; h.a_bs = (long long)S * pm.ld; h.w_bs = (long long)Cp * 128; h.c_bs = (long long)S * y3.ld; h.r_bs = (long long)S * y2.ld;
  RC(push_gemm(b.c, b.prog, h, -1, 128.0, st3.buf ? &st3 : nullptr));
  b.release(pm); b.release(y2);
  return DTP_OK;
}

// Stage 3: the feed-forward (LN3 folded, GEGLU), ff.net.2 and proj_out with their residuals -> out.  y3 and st3 go back to the pool.
static int feed_forward(Builder& b, const XfW& w, const T& y3, RowStats& st3, const T& xin, T& out, const T* dst) {
  const int C = y3.C, N = y3.B, S = y3.H * y3.W;
  const ConvW& wm = w.ff2_proj;
  // Round 6: at level 0 (C = 320) with enough rows to give every CU several 128-row workgroups (batched stamps), FF1 (GEGLU), FF2 and
  // proj_out run as ONE register-chained launch (ffchain.hip): the [rows][1280] hidden tensor is never written.  At batch 1 its 96
  // workgroups (one per CU, ~400 registers) tie the two launches they replace, so the gate is the row count; Ctx::ffchain forces it
  // off / on (A/B).
  FfchainParams fc = {};
  fc.X = y3.p; fc.ldx = y3.ld; fc.W1 = w.ff1.w; fc.ldw1 = w.ff1.ldw; fc.lns1 = w.ff1.lns; fc.b1 = w.ff1.b;
  fc.Wm = wm.w; fc.ldwm = wm.ldw; fc.bm = wm.b; fc.R = xin.p; fc.ldr = xin.ld;
  fc.M = N * S; fc.C = C; fc.ln_eps = 1e-5f;
  fc.Out = y3.p; fc.ldo = C;  // (placeholder for the support check)
  const bool want = b.c->ffchain >= 0 ? b.c->ffchain != 0 : (long long)N * S / 128 >= 2LL * b.c->num_cu;
  const bool chain = want && !b.fp8 && wm.K == 5 * C && wm.cout == C && w.ff1.cout == 8 * C && w.ff1.K == C && w.ff1.lns && dtp_ffchain_supported(fc);
  if (chain) {
    RC(block_out(b, dst, y3, out));
    fc.Out = out.p; fc.ldo = out.ld;
    b.release_stats(st3);
    b.push(PK_LNLIN, 2.0 * N * S * (8.0 * C * C + 5.0 * C * C), 2.0 * (3.0 * N * S * C + 13.0 * C * C),
           [=](hipStream_t s, int) { return dtp_launch_ffchain(fc, s); }, "ffchain M=" + std::to_string(N * S) + " C=" + std::to_string(C));
    b.release(y3);
    return DTP_OK;
  }
  T f;
  RC(b.linear_f8ops(y3, w.ff1, nullptr, GF_GEGLU, f, nullptr, &st3, true));  // LN3 folded (e4m3: st3 released before the GEMM)
  // (fp8_operands leaves the merged GEMM below in fp16 although its K is 1600 .. 6400: its A2 operand y3 is the residual stream, and
  // rounding THAT to e4m3 costs 2.6e-2 of pixel error on its own -- measured by emulation in the fp32 oracle)
  // ff.net.2 (+ y3) and proj_out (+ x) are two Linears with only a residual add between them: one GEMM over [f | y3]
  // with the merged weights [Wp W2 | Wp] (load_linear_pair) -- no y4 tensor, one launch fewer per block
  if (wm.K != f.C + y3.C || wm.cout != C) { dtp_set_error("transformer: merged ff2/proj_out weight mismatch"); return DTP_ERR_ARG; }
  RC(block_out(b, dst, y3, out));
  GemmParams g = {};
  g.A = f.p; g.lda = f.ld; g.A2 = y3.p; g.lda2 = y3.ld; g.Cin2 = y3.C;
  g.W = wm.w; g.Wfr = wm.wfr; g.ldw = wm.ldw; g.nkb = wm.ldw / 64;
  g.M = N * S; g.N = C; g.K = wm.K;
  g.C = out.p; g.ldc = out.ld;
  g.bias = wm.b; g.R = xin.p; g.ldr = xin.ld;
  g.flags = GF_BIAS | GF_RESID;
  if (b.fp8 && wm.w8) {
    GemmParams q = g;
    q.W8 = wm.w8; q.ldw8 = wm.ldw8; q.w_scale = wm.w8_scale; q.a_scale = DTP_FP8_LN_A_SCALE * 8.0f; q.splits = 1;
    if (dtp_gemm_fp8_supported(q)) {  // [GEGLU output | residual stream]: un-normalised operands, calibrated scale (fp8_calibrate)
      q.a_scale_host = fp8_new_linear_scale(b.c, &q.amax_slot1);
      g = q;
    }
  }
  RC(push_gemm(b.c, b.prog, g, -1, (double)wm.K, nullptr));
  b.release(f); b.release(y3);
  return DTP_OK;
}

static int transformer(Builder& b, const T& x, const XfW& w, const UNetProg& up, T& out, const T* dst = nullptr, const Dup* dup = nullptr) {
  const T& xin = dup && dup->B > 0 ? dup->x_full : x;  // the block input for all N samples (residual of the last GEMM)
  T y, a, y3; RowStats st3;
  RC(self_attention(b, x, w, y, a));
  RC(cross_attention(b, x, w, up, dup, a, y, y3, st3));
  return feed_forward(b, w, y3, st3, xin, out, dst);
}

// the 16 transformer blocks in kv_index order (the order load_unet_weights numbers them)
static std::vector<XfW*> xf_blocks(UNetW& u) {
  std::vector<XfW*> all;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 2; ++j) all.push_back(&u.down_xf[i][j]);
  all.push_back(&u.mid_xf);
  for (int i = 1; i < 4; ++i) for (int j = 0; j < 3; ++j) all.push_back(&u.up_xf[i][j]);
  return all;
}

int build_unet_prog(Ctx* c, int N, int dupB, UNetProg& up) {
  const UNetW& u = c->unet;
  const int h = c->h;
  up.N = N;
  void* p;
  RC(ctx_persistent(c, (size_t)N * h * h * 16 * 2, &p, true)); up.in16 = (f16*)p;
  RC(ctx_persistent(c, (size_t)N * 14 * 768 * 2, &p, true)); up.ctx16 = (f16*)p;
  RC(ctx_persistent(c, (size_t)N * h * h * 4 * 4, &p, true)); up.out32 = (float*)p;
  // ---- cross-attention K/V of the 16 transformer blocks (depends only on the conditioning)
  const std::vector<XfW*> xfs = xf_blocks(c->unet);
  up.kvbuf.assign(xfs.size(), nullptr);
  up.xW1.assign(xfs.size(), nullptr); up.xW2.assign(xfs.size(), nullptr);
  up.xb1.assign(xfs.size(), nullptr); up.xl1.assign(xfs.size(), nullptr);
  RC(ctx_persistent(c, (size_t)N * 128 * 1280 * 2, &p, true)); up.kexp = (f16*)p;
  RC(ctx_persistent(c, (size_t)N * 128 * 1280 * 2, &p, true)); up.vexp = (f16*)p;
  {
    Builder b{c, &up.kv};
    T ctx;
    ctx.p = up.ctx16; ctx.B = N; ctx.H = 1; ctx.W = 14; ctx.C = 768; ctx.ld = 768;
    auto plain = [&](GemmParams g, int tile) {
      g.zero = c->zero; g.splits = 1; g.kb_per_split = g.nkb;
      const double nb = g.batch > 1 ? g.batch : 1;
      b.push(dtp_tile(tile).pk, 2.0 * nb * g.M * (double)g.N * g.K, 2.0 * nb * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N),
             [=](hipStream_t s, int) { return dtp_launch_gemm(g, tile, s); });
    };
    for (const XfW* w : xfs) {
      const int C = w->q2.K, Cp = (C + 127) / 128 * 128, i = w->kv_index;
      if (w->kv2.cout != 2 * C || w->out2.K != C || (C % 64) || !w->q2.b || !w->q2T) { dtp_set_error("cross-attention: unexpected weight shapes"); return DTP_ERR_ARG; }
      RC(ctx_persistent(c, (size_t)N * 14 * 2 * C * 2, &p, true)); up.kvbuf[i] = (f16*)p;
      RC(ctx_persistent(c, (size_t)N * 128 * C * 2, &p, true)); up.xW1[i] = (f16*)p;
      RC(ctx_persistent(c, (size_t)N * Cp * 128 * 2, &p, true)); up.xW2[i] = (f16*)p;
      RC(ctx_persistent(c, (size_t)N * 128 * 4, &p, true)); up.xb1[i] = (float*)p;
      RC(ctx_persistent(c, (size_t)N * 128 * 4, &p, true)); up.xl1[i] = (float*)p;
      GemmParams g = {};  // K | V of the 14 context tokens
      g.A = ctx.p; g.W = w->kv2.w; g.C = up.kvbuf[i];
      g.M = N * 14; g.N = 2 * C; g.K = 768; g.lda = 768; g.ldw = w->kv2.ldw; g.ldc = 2 * C; g.nkb = w->kv2.ldw / 64;
      plain(g, 3);
      f16 *kvb = up.kvbuf[i], *kexp = up.kexp, *vexp = up.vexp, *W1 = up.xW1[i];
      float *b1 = up.xb1[i], *l1 = up.xl1[i];
      const float* bq = w->q2.b;
      const float scale = 1.0f / sqrtf((float)(C / 8));
      b.push(PK_ELEM, 0.0, 0.0, [=](hipStream_t s, int) { return dtp_launch_expand_kv(kvb, kexp, vexp, N, 14, C, 8, scale, s); });
      GemmParams g1 = {};  // score matrix: rows (n, h, j), K = to_q output channel
      g1.A = kexp; g1.W = w->q2T; g1.C = W1;
      g1.M = N * 128; g1.N = C; g1.K = C; g1.lda = C; g1.ldw = C; g1.ldc = C; g1.nkb = C / 64;
      plain(g1, 3);
      b.push(PK_ELEM, 0.0, 0.0, [=](hipStream_t s, int) {
        RC(dtp_launch_rowsum_f16(W1, C, C, l1, N * 128, s));
        return dtp_launch_rowdot_f16(kexp, C, bq, b1, N * 128, C, s);
      });
      GemmParams g2 = {};  // value-output matrix per sample: [C][128] = Wo . Vexp_n^T, stored as packed weights of the 2nd GEMM
      g2.A = w->out2.w; g2.W = vexp; g2.C = up.xW2[i];
      g2.M = C; g2.N = 128; g2.K = C; g2.lda = w->out2.ldw; g2.ldw = C; g2.ldc = 128; g2.nkb = C / 64;
      g2.batch = N; g2.a_bs = 0; g2.w_bs = (long long)128 * C; g2.c_bs = (long long)Cp * 128;
      plain(g2, 3);
    }
  }
  // ---- main program
  if (c->fp8_linear) {  // e4m3 copies of the transformer Linears (once per context)
    for (XfW* x : xfs)
      for (ConvW* w : {&x->proj_in, &x->qkv, &x->out1, &x->ff1, &x->ff2_proj}) RC(ensure_w8(c, *w));
    // the quantise kernels run on the null stream, the program on the caller's (non-blocking) stream: order them once, here
    HIP_CHECK(hipDeviceSynchronize());
  }
  if (c->fp8_operands) {  // e4m3 copies of the Linears fp8_operands covers (transformer(): q/k/v, to_out, FF1 with K >= DTP_FP8_OPERANDS_MIN_K)
    for (XfW* x : xfs)
      for (ConvW* w : {&x->qkv, &x->out1, &x->ff1})
        if (w->K >= DTP_FP8_OPERANDS_MIN_K) RC(ensure_w8(c, *w));
    HIP_CHECK(hipDeviceSynchronize());  // (null-stream quantise kernels before the caller's stream, as above)
  }
  up.cal_begin = c->fp8_cals.size();
  Builder b{c, &up.main};
  b.fp8 = c->fp8_linear;
  b.f8ops = c->fp8_operands;
  T x0;
  x0.p = up.in16; x0.B = N; x0.H = h; x0.W = h; x0.C = 16; x0.ld = 16;
  // Zero-copy skip connections: every up-path ResBlock consumes cat([x, skip], C).  The 12 concat buffers are
  // planned up front; the skip's producer (down path) writes channels [Cx, Cx+Cs) and the x producer (up path)
  // writes channels [0, Cx) of the same buffer through the row stride, so no concat kernel ever runs.
  const int Cs[12] = {320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280};   // skip k, in push order
  const int Cx[12] = {1280, 1280, 1280, 1280, 1280, 1280, 1280, 640, 640, 640, 320, 320};  // x at up position p = 11-k
  // Level sizes: each stride-2, pad-1 downsampler gives ceil(n / 2) (R a multiple of 8 but not of 64 leaves odd levels).
  // Every up-block upsampler then writes its skip's size, 2 n or 2 n - 1 (the reference's interpolate(size=skip)); for h % 8 == 0
  // this is the exact halving / doubling it always was.
  const int L1 = (h + 1) / 2, L2 = (L1 + 1) / 2, L3 = (L2 + 1) / 2;
  const int Hs[12] = {h, h, h, L1, L1, L1, L2, L2, L2, L3, L3, L3};
  T cat[12], skipv[12], xslot[12];
  for (int k = 0; k < 12; ++k) {
    const int cx = Cx[11 - k];
    cat[k] = b.alloc(N, Hs[k], Hs[k], cx + Cs[k]);
    if (!cat[k].p) return DTP_ERR_HIP;
    skipv[k] = cat[k]; skipv[k].p += cx; skipv[k].C = Cs[k];
    xslot[k] = cat[k]; xslot[k].C = cx;
  }
  int sk = 0;  // next skip to produce
  T x;
  if (dupB > 0) {  // de-duplicated prefix: conv_in on samples [dupB, N) only (struct Dup)
    const T x0s = samples(x0, dupB, N - dupB), sk0s = samples(skipv[sk], dupB, N - dupB);
    RC(b.conv3(x0s, u.conv_in, 1, 1, false, h, h, nullptr, -1, x, Conv3Opts::into(sk0s)));
    ++sk;
  } else {
    RC(b.conv3(x0, u.conv_in, 1, 1, false, h, h, nullptr, -1, x, Conv3Opts::into(skipv[sk++])));
  }
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) {
      T y;
      if (i < 3) {
        T z;
        if (dupB > 0 && i == 0 && j == 0) {
          Dup dup;
          dup.B = dupB;
          dup.skip_full = skipv[0];
          dup.x_full = b.alloc(N, x.H, x.W, u.down_res[0][0].c2.cout);
          if (!dup.x_full.p) return DTP_ERR_HIP;
          const T ys = samples(dup.x_full, dupB, N - dupB);
          RC(b.resnet(x, u.down_res[i][j], 1e-5f, true, y, &ys));
          RC(transformer(b, y, u.down_xf[i][j], up, z, &skipv[sk++], &dup));
          y = dup.x_full;  // released below
        } else {
          RC(b.resnet(x, u.down_res[i][j], 1e-5f, true, y));
          RC(transformer(b, y, u.down_xf[i][j], up, z, &skipv[sk++]));
        }
        b.release(y);
        x = z;
      } else {
        RC(b.resnet(x, u.down_res[i][j], 1e-5f, true, y, &skipv[sk++]));
        x = y;
      }
    }
    if (i < 3) {
      T y;
      RC(b.conv3(x, u.down_conv[i], 2, 1, false, (x.H + 1) / 2, (x.W + 1) / 2, nullptr, -1, y, Conv3Opts::into(skipv[sk++])));
      x = y;
    }
  }
  int pk = 11;  // concat buffer consumed next
  {
    T y, z, w2;
    RC(b.resnet(x, u.mid_res[0], 1e-5f, true, y));  // x is a skip view: stays alive
    RC(transformer(b, y, u.mid_xf, up, z));
    b.release(y);
    RC(b.resnet(z, u.mid_res[1], 1e-5f, true, w2, &xslot[pk]));
    b.release(z);
  }
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) {
      const T in = cat[pk];
      // where this layer's output goes: the x slot of the next concat buffer, unless an upsampler (or the end) follows
      const T* dst = (j < 2) ? &xslot[pk - 1] : nullptr;
      T y;
      if (i > 0) {
        RC(b.resnet(in, u.up_res[i][j], 1e-5f, true, y));
        T z;
        RC(transformer(b, y, u.up_xf[i][j], up, z, dst));
        b.release(y);
        x = z;
      } else {
        RC(b.resnet(in, u.up_res[i][j], 1e-5f, true, y, dst));
        x = y;
      }
      b.release(in);
      --pk;
    }
    if (i < 3) {
      T y;
      // nearest upsample to the skip's size (2 n or 2 n - 1): the x2 window of GF_UPS2, cropped by the output size
      RC(b.conv3(x, u.up_conv[i], 1, 1, true, xslot[pk].H, xslot[pk].W, nullptr, -1, y, Conv3Opts::into(xslot[pk])));
      b.release(x);
      x = y;
    }
  }
  T t, o;
  RC(b.gn(x, u.norm_out, 1e-5f, true, t));
  b.release(x);
  RC(b.conv3(t, u.conv_out, 1, 1, false, h, h, nullptr, -1, o, Conv3Opts::f32_out(up.out32, 4)));
  b.release(t);
  up.cal_end = c->fp8_cals.size();
  tune_cache_save(c);
  return ensure_ws(c);
}

__global__ void nhwc4_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int HW, int ldx) {
  const long long total = (long long)B * C * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int hw = (int)(i % HW);
    const long long bc = i / HW;
    const int ch = (int)(bc % C), b = (int)(bc / C);
    y[i] = x[((size_t)b * HW + hw) * ldx + ch];
  }
}

int launch_nhwc_f32_to_nchw(const float* x, float* y, int B, int C, int HW, int ldx, hipStream_t s) {
  long long total = (long long)B * C * HW;
  int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(nhwc4_to_nchw_kernel, dim3(blocks), dim3(256), 0, s, x, y, B, C, HW, ldx);
  return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP;
}

int get_unet_prog(Ctx* c, int N, int dupB, UNetProg** out) {
  // (the prefix's one row-copy launch moves 16-byte aligned segments: the level-0 row statistics -- dupB * h^2 rows at a pitch of N * h^2
  // rows, 8 bytes each -- are that only when both counts are even; an odd latent size (R a multiple of 8 but not of 16)
  // with an odd dupB or N evaluates every sample)
  const long long hw = (long long)c->h * c->h;
  if (!c->dedupe_prefix || dupB >= N || (dupB * hw) % 2 || (N * hw) % 2) dupB = 0;
  const int key = N * 128 + dupB;  // dupB <= max_batch <= 64: unique
  auto it = c->unet_progs.find(key);
  if (it == c->unet_progs.end()) {
    UNetProg& up = c->unet_progs[key];
    RC(build_unet_prog(c, N, dupB, up));
    *out = &up;
    return DTP_OK;
  }
  *out = &it->second;
  return DTP_OK;
}

extern "C" int dtp_unet(dtp_ctx* ctx, const float* sample, float timestep, const void* ctx_f16, float* out, int N,
                        dtp_stream s_) {
  Ctx* c = (Ctx*)ctx;
  hipStream_t s = (hipStream_t)s_;
  if (!c || !c->finalized) { dtp_set_error("dtp_unet: weights not finalized"); return DTP_ERR_STATE; }
  if (N < 1 || N > 3 * c->maxB) { dtp_set_error("dtp_unet: batch %d outside 1..%d", N, 3 * c->maxB); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(c->device));
  UNetProg* up;
  RC(get_unet_prog(c, N, 0, &up));  // engine-level call: arbitrary samples, nothing to de-duplicate
  const int hw = c->h * c->h;
  HIP_CHECK(hipStreamSynchronize(s));
  RC(ensure_temb(c, {timestep}));
  c->sched_steps = -1;  // the table no longer holds a stamp schedule
  RC(dtp_launch_nchw_f32_to_nhwc_f16(sample, up->in16, N, 9, hw, 16, s));
  HIP_CHECK(hipMemcpyAsync(up->ctx16, ctx_f16, (size_t)N * 14 * 768 * 2, hipMemcpyDeviceToDevice, s));
  up->kv_ver = 0;  // K/V now belong to the caller's conditioning
  up->kv_slots.clear();
  RC(up->kv.run(s, 0));
  RC(fp8_calibrate(c, up, s, 0));  // (first call of an fp8 context only)
  RC(up->main.run(s, 0));
  return launch_nhwc_f32_to_nchw(up->out32, out, N, 4, hw, 4, s);
}
