// Engine core: device memory (weight arena, activation pool, shared workspace), weight staging + packing.
// The launch-program builder is builder.hip, the build-time tuner tune.hip.
#include "engine.h"

#include <algorithm>

static size_t up_to(size_t x, size_t m) { return (x + m - 1) / m * m; }

// ---------------------------------------------------------------- memory
int ctx_arena_alloc(Ctx* c, size_t bytes, void** out) {
  bytes = up_to(bytes, 256);
  if (bytes > c->cur_left) {
    const size_t chunk = std::max(bytes, (size_t)512 << 20);
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, chunk));
    HIP_CHECK(hipMemset(p, 0, chunk));
    c->chunks.push_back(p);
    c->cur = (char*)p;
    c->cur_left = chunk;
    c->arena_total += chunk;
  }
  *out = c->cur;
  c->cur += bytes;
  c->cur_left -= bytes;
  return DTP_OK;
}

int ctx_pool_get(Ctx* c, size_t bytes, void** out) {
  bytes = up_to(bytes, 4096);
  int best = -1;
  for (size_t i = 0; i < c->pool.blocks.size(); ++i) {
    const Pool::Block& b = c->pool.blocks[i];
    if (b.free && b.bytes >= bytes && b.bytes <= bytes + bytes / 2 + (1 << 20) &&
        (best < 0 || b.bytes < c->pool.blocks[best].bytes))
      best = (int)i;
  }
  if (best < 0) {
    // +256 KiB slack: operand tiles may over-read up to 127 rows past the last valid row
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes + (256 << 10)));
    HIP_CHECK(hipMemset(p, 0, bytes + (256 << 10)));
    c->pool.blocks.push_back({(char*)p, bytes, false});
    c->pool.total += bytes;
    *out = p;
    return DTP_OK;
  }
  c->pool.blocks[best].free = false;
  *out = c->pool.blocks[best].p;
  return DTP_OK;
}

void ctx_pool_put(Ctx* c, void* p) {
  for (auto& b : c->pool.blocks)
    if (b.p == (char*)p) { b.free = true; return; }
}

int ctx_persistent(Ctx* c, size_t bytes, void** out, bool zero) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes + (256 << 10)));
  if (zero) HIP_CHECK(hipMemset(p, 0, bytes + (256 << 10)));
  c->persistent.push_back(p);
  *out = p;
  return DTP_OK;
}

const Staged* ctx_find(Ctx* c, const std::string& name) {
  auto it = c->staged.find(name);
  return it == c->staged.end() ? nullptr : &it->second;
}

int ctx_fetch_host(Ctx* c, const std::string& name, std::vector<float>& out) {
  const Staged* s = ctx_find(c, name);
  if (!s) { dtp_set_error("missing tensor '%s'", name.c_str()); return DTP_ERR_MISSING; }
  out.resize(s->n);
  HIP_CHECK(hipMemcpy(out.data(), s->d, s->n * sizeof(float), hipMemcpyDeviceToHost));
  return DTP_OK;
}

int ctx_upload_f32(Ctx* c, const std::vector<float>& v, float** out) {
  void* p;
  RC(ctx_arena_alloc(c, v.size() * sizeof(float), &p));
  HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = (float*)p;
  return DTP_OK;
}

// ---------------------------------------------------------------- weight loaders
int load_norm(Ctx* c, const std::string& name, NormW& n) {
  const Staged *g = ctx_find(c, name + ".weight"), *b = ctx_find(c, name + ".bias");
  if (!g || !b) { dtp_set_error("missing norm '%s'", name.c_str()); return DTP_ERR_MISSING; }
  void *pg, *pb;
  RC(ctx_arena_alloc(c, g->n * 4, &pg));
  RC(ctx_arena_alloc(c, b->n * 4, &pb));
  HIP_CHECK(hipMemcpy(pg, g->d, g->n * 4, hipMemcpyDeviceToDevice));
  HIP_CHECK(hipMemcpy(pb, b->d, b->n * 4, hipMemcpyDeviceToDevice));
  n.g = (float*)pg; n.b = (float*)pb; n.c = (int)g->n;
  return DTP_OK;
}

int load_conv(Ctx* c, const std::string& name, ConvW& w, int cin_pad, bool bias) {
  const Staged* s = ctx_find(c, name + ".weight");
  if (!s) { dtp_set_error("missing weight '%s.weight'", name.c_str()); return DTP_ERR_MISSING; }
  const int cout = (int)s->shape[0], cin = (int)s->shape[1];
  const int taps = s->shape.size() == 4 ? (int)(s->shape[2] * s->shape[3]) : 1;
  if (cin_pad <= 0) cin_pad = (int)up_to(cin, 8);
  w.cout = cout; w.cin = cin_pad; w.cin_true = cin; w.taps = taps; w.K = taps * cin_pad; w.ldw = (int)up_to(w.K, 64);
  void* p;
  RC(ctx_arena_alloc(c, up_to(cout, 128) * (size_t)w.ldw * 2, &p));
  w.w = (f16*)p;
  RC(dtp_launch_pack_conv_weight(s->d, w.w, cout, cin, cin_pad, taps, w.ldw, 0));
  if (taps == 9 && (cin & 63) == 0) {  // second packing for the halo-tiled kernel
    void* p2;
    RC(ctx_arena_alloc(c, up_to(cout, 128) * (size_t)w.ldw * 2, &p2));
    w.wcb = (f16*)p2;
    RC(dtp_launch_pack_conv_weight_cb(s->d, w.wcb, cout, cin, w.ldw, 0));
  }
  if (c->pack_ws && taps == 9 && (cin & 63) == 0 && cout >= 32) {  // third packing: fragment order for the weight-streaming kernel
    void* p3;
    RC(ctx_arena_alloc(c, dtp_conv_ws_packed_elems(cout, cin, 0) * 2, &p3));
    w.wfr = (f16*)p3;
    RC(dtp_launch_pack_conv_ws(s->d, nullptr, w.wfr, cout, cin, 0, 0));
  }
  w.b = nullptr;
  if (bias) {
    const Staged* b = ctx_find(c, name + ".bias");
    if (!b) { dtp_set_error("missing bias '%s.bias'", name.c_str()); return DTP_ERR_MISSING; }
    void* pb;
    RC(ctx_arena_alloc(c, b->n * 4, &pb));
    HIP_CHECK(hipMemcpy(pb, b->d, b->n * 4, hipMemcpyDeviceToDevice));
    w.b = (float*)pb;
  }
  return DTP_OK;
}

// The four phase sets of an upsampler conv (conv_ws.hip, pack_conv_ws_ups4_kernel), next to its nine-tap fragment packing: 16/9 of that
// packing's bytes.  Only where load_conv built the fragment packing (Ctx::pack_ws, Cin % 64 == 0): without it no weight-streaming tile runs.
int load_conv_ups4(Ctx* c, const std::string& name, ConvW& w) {
  if (!c->ups_phase || !w.wfr || w.taps != 9 || w.cin2) return DTP_OK;
  const Staged* s = ctx_find(c, name + ".weight");
  if (!s) { dtp_set_error("missing weight '%s.weight'", name.c_str()); return DTP_ERR_MISSING; }
  void* p;
  RC(ctx_arena_alloc(c, dtp_conv_ws_ups4_packed_elems(w.cout, w.cin_true) * 2, &p));
  w.wfr4 = (f16*)p;
  return dtp_launch_pack_conv_ws_ups4(s->d, w.wfr4, w.cout, w.cin_true, 0);
}

int load_conv_with_shortcut(Ctx* c, const std::string& conv, const std::string& shortcut, ConvW& w) {
  const Staged *s = ctx_find(c, conv + ".weight"), *t = ctx_find(c, shortcut + ".weight");
  const Staged *sb = ctx_find(c, conv + ".bias"), *tb = ctx_find(c, shortcut + ".bias");
  if (!s || !t || !sb || !tb) { dtp_set_error("missing tensors for '%s' + '%s'", conv.c_str(), shortcut.c_str()); return DTP_ERR_MISSING; }
  const int cout = (int)s->shape[0], cin = (int)s->shape[1], cin2 = (int)t->shape[1];
  if ((int)t->shape[0] != cout || ((9 * cin) & 63) || (cin2 & 63)) { dtp_set_error("shortcut fusion: unsupported shape at '%s'", conv.c_str()); return DTP_ERR_ARG; }
  w.cout = cout; w.cin = cin; w.cin_true = cin; w.taps = 9; w.cin2 = cin2;
  w.K = 9 * cin + cin2; w.ldw = (int)up_to(w.K, 64);
  void* p;
  RC(ctx_arena_alloc(c, up_to(cout, 128) * (size_t)w.ldw * 2, &p));
  w.w = (f16*)p;
  RC(dtp_launch_pack_conv_weight(s->d, w.w, cout, cin, cin, 9, w.ldw, 0));
  RC(dtp_launch_pack_conv_weight(t->d, w.w + 9 * cin, cout, cin2, cin2, 1, w.ldw, 0));
  void* p2;  // halo-kernel packing: channel-block-major 3x3 part, same shortcut columns
  RC(ctx_arena_alloc(c, up_to(cout, 128) * (size_t)w.ldw * 2, &p2));
  w.wcb = (f16*)p2;
  RC(dtp_launch_pack_conv_weight_cb(s->d, w.wcb, cout, cin, w.ldw, 0));
  RC(dtp_launch_pack_conv_weight(t->d, w.wcb + 9 * cin, cout, cin2, cin2, 1, w.ldw, 0));
  if (c->pack_ws && (cin & 63) == 0 && cout >= 32) {  // fragment order for the weight-streaming kernel: 3x3 part, then the shortcut
    void* p3;
    RC(ctx_arena_alloc(c, dtp_conv_ws_packed_elems(cout, cin, cin2) * 2, &p3));
    w.wfr = (f16*)p3;
    RC(dtp_launch_pack_conv_ws(s->d, t->d, w.wfr, cout, cin, cin2, 0));
  }
  std::vector<float> b1, b2;
  RC(ctx_fetch_host(c, conv + ".bias", b1));
  RC(ctx_fetch_host(c, shortcut + ".bias", b2));
  for (size_t i = 0; i < b1.size(); ++i) b1[i] += b2[i];
  b1.resize(up_to(b1.size(), 128), 0.f);
  return ctx_upload_f32(c, b1, &w.b);
}

// fragment-order copy of a packed Linear for gemmws_kernel (gemm_ws.hip) -- while the UNet's weights load (Ctx::pack_ws)
static int pack_linear_ws(Ctx* c, ConvW& w) {
  // opt-in (Ctx::gemm_ws): measured in round 4, the kernel matches the tiled ones within +-10 % on the single-round launches and loses
  // on the multi-round ones -- without the packing no problem carries Wfr and the tuner never sees tile 55
  if (!c->pack_ws || !c->gemm_ws || w.taps != 1 || (w.K & 63) || w.K < 128 || w.cout < 32 || (w.cout & 3)) return DTP_OK;
  void* p;
  RC(ctx_arena_alloc(c, dtp_gemm_ws_packed_elems(w.cout, w.K) * 2, &p));
  w.wfr = (f16*)p;
  return dtp_launch_pack_linear_ws(w.w, w.ldw, w.wfr, w.cout, w.K, 0);
}

int load_linear_pair(Ctx* c, const std::string& first, const std::string& second, ConvW& w) {
  const Staged *wa = ctx_find(c, first + ".weight"), *wb = ctx_find(c, second + ".weight");
  const Staged *ba = ctx_find(c, first + ".bias"), *bb = ctx_find(c, second + ".bias");
  if (!wa || !wb || !ba || !bb) { dtp_set_error("linear pair: missing '%s' / '%s'", first.c_str(), second.c_str()); return DTP_ERR_MISSING; }
  const int Na = (int)wa->shape[0], Ka = (int)(wa->n / Na), Nb = (int)wb->shape[0], Kb = (int)(wb->n / Nb);  // wb may be a 1x1 conv
  if (Kb != Na || (Ka & 63) || (Kb & 63)) { dtp_set_error("linear pair: shapes [%d,%d] then [%d,%d] do not chain", Na, Ka, Nb, Kb); return DTP_ERR_ARG; }
  const int K = Ka + Kb;
  float *prod = nullptr, *cat = nullptr, *bias = nullptr;
  HIP_CHECK(hipMalloc(&prod, (size_t)Nb * Ka * 4));
  HIP_CHECK(hipMalloc(&cat, (size_t)Nb * K * 4));
  HIP_CHECK(hipMalloc(&bias, (size_t)Nb * 4));
  RC(dtp_launch_matmul_f32(wb->d, wa->d, prod, Nb, Ka, Kb, 0));  // Wb . Wa  [Nb][Ka]
  HIP_CHECK(hipMemcpy2DAsync(cat, (size_t)K * 4, prod, (size_t)Ka * 4, (size_t)Ka * 4, Nb, hipMemcpyDeviceToDevice, 0));
  HIP_CHECK(hipMemcpy2DAsync(cat + Ka, (size_t)K * 4, wb->d, (size_t)Kb * 4, (size_t)Kb * 4, Nb, hipMemcpyDeviceToDevice, 0));
  RC(dtp_launch_rowdot(wb->d, ba->d, bias, Nb, Kb, 0));  // Wb . ba
  w = ConvW();
  w.cout = Nb; w.cin = K; w.cin_true = K; w.taps = 1; w.K = K; w.ldw = (int)up_to(K, 64);
  void* p;
  RC(ctx_arena_alloc(c, up_to(Nb, 128) * (size_t)w.ldw * 2, &p));
  w.w = (f16*)p;
  RC(dtp_launch_pack_linear_weight(cat, w.w, Nb, K, w.ldw, nullptr, 0));
  RC(pack_linear_ws(c, w));
  std::vector<float> hb(Nb), hb2;
  HIP_CHECK(hipMemcpy(hb.data(), bias, (size_t)Nb * 4, hipMemcpyDeviceToHost));
  RC(ctx_fetch_host(c, second + ".bias", hb2));
  for (int i = 0; i < Nb; ++i) hb[i] += hb2[i];
  hb.resize(up_to(hb.size(), 128), 0.f);
  RC(ctx_upload_f32(c, hb, &w.b));
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipFree(prod)); HIP_CHECK(hipFree(cat)); HIP_CHECK(hipFree(bias));
  return DTP_OK;
}

int load_linear(Ctx* c, const std::vector<std::string>& names, ConvW& w, bool bias, bool geglu, const std::string& fold_ln) {
  int N = 0, K = -1;
  for (const auto& nm : names) {
    const Staged* s = ctx_find(c, nm + ".weight");
    if (!s) { dtp_set_error("missing weight '%s.weight'", nm.c_str()); return DTP_ERR_MISSING; }
    const int k = (int)(s->n / s->shape[0]);
    if (K >= 0 && k != K) { dtp_set_error("stacked linear '%s': K mismatch", nm.c_str()); return DTP_ERR_ARG; }
    K = k;
    N += (int)s->shape[0];
  }
  w.cout = N; w.cin = K; w.cin_true = K; w.taps = 1; w.K = K; w.ldw = (int)up_to(K, 64);
  void* p;
  RC(ctx_arena_alloc(c, up_to(N, 128) * (size_t)w.ldw * 2, &p));
  w.w = (f16*)p;
  std::vector<int> map;
  int* dmap = nullptr;
  if (geglu) {
    if (names.size() != 1 || N % 256) { dtp_set_error("geglu pack: bad shape"); return DTP_ERR_ARG; }
    map.resize(N);
    for (int f = 0; f < N / 2; ++f) {
      map[f] = (f / 64) * 128 + (f % 64);
      map[N / 2 + f] = (f / 64) * 128 + 64 + (f % 64);
    }
    HIP_CHECK(hipMalloc(&dmap, N * sizeof(int)));
    HIP_CHECK(hipMemcpy(dmap, map.data(), N * sizeof(int), hipMemcpyHostToDevice));
  }
  // LayerNorm fold: LN(x) W^T + b = rstd * (x W'^T - mean * rowsum(W')) + (b + W beta), W' = W diag(gamma)
  std::vector<float> wbeta;  // (W beta)[n] over the stacked rows
  if (!fold_ln.empty()) {
    const Staged *g = ctx_find(c, fold_ln + ".weight"), *be = ctx_find(c, fold_ln + ".bias");
    if (!g || !be || (int)g->n != K) { dtp_set_error("LN fold: missing or mismatched norm '%s'", fold_ln.c_str()); return DTP_ERR_MISSING; }
    float* tmp = nullptr;
    HIP_CHECK(hipMalloc(&tmp, (size_t)N * 4));
    int r0 = 0;
    for (const auto& nm : names) {
      const Staged* s = ctx_find(c, nm + ".weight");
      const int n = (int)s->shape[0];
      RC(dtp_launch_rowdot(s->d, be->d, tmp + r0, n, K, 0));
      RC(dtp_launch_scale_cols(s->d, g->d, n, K, 0));
      r0 += n;
    }
    wbeta.resize(N);
    HIP_CHECK(hipMemcpy(wbeta.data(), tmp, (size_t)N * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(tmp));
  }
  int row = 0;
  for (const auto& nm : names) {
    const Staged* s = ctx_find(c, nm + ".weight");
    const int n = (int)s->shape[0];
    RC(dtp_launch_pack_linear_weight(s->d, w.w + (size_t)row * w.ldw, n, K, w.ldw, dmap, 0));
    row += n;
  }
  if (!fold_ln.empty()) {
    void* pl;
    const int rows = (int)up_to(N, 128);
    RC(ctx_arena_alloc(c, (size_t)rows * 4, &pl));
    w.lns = (float*)pl;
    RC(dtp_launch_rowsum_f16(w.w, w.ldw, K, w.lns, rows, 0));
  }
  if (dmap) { HIP_CHECK(hipDeviceSynchronize()); HIP_CHECK(hipFree(dmap)); }
  if (!geglu) RC(pack_linear_ws(c, w));
  w.b = nullptr;
  if (bias || !fold_ln.empty()) {
    std::vector<float> all;
    for (const auto& nm : names) {
      std::vector<float> b;
      if (bias && ctx_find(c, nm + ".bias")) RC(ctx_fetch_host(c, nm + ".bias", b));
      else b.assign((size_t)ctx_find(c, nm + ".weight")->shape[0], 0.f);
      all.insert(all.end(), b.begin(), b.end());
    }
    for (size_t i = 0; i < wbeta.size(); ++i) all[i] += wbeta[i];
    if (geglu) {
      std::vector<float> perm(all.size());
      for (size_t i = 0; i < all.size(); ++i) perm[map[i]] = all[i];
      all.swap(perm);
    }
    all.resize(up_to(all.size(), 128), 0.f);
    RC(ctx_upload_f32(c, all, &w.b));
  }
  return DTP_OK;
}

int load_plain_f16(Ctx* c, const std::string& name, f16** out) {
  const Staged* s = ctx_find(c, name);
  if (!s) { dtp_set_error("missing tensor '%s'", name.c_str()); return DTP_ERR_MISSING; }
  void* p;
  RC(ctx_arena_alloc(c, s->n * 2, &p));
  RC(dtp_launch_f32_to_f16(s->d, (f16*)p, (long long)s->n, 0));
  *out = (f16*)p;
  return DTP_OK;
}

int ensure_w8(Ctx* c, ConvW& w) {
  if (w.w8 || w.taps != 1 || !w.w) return DTP_OK;
  const size_t rows = up_to(w.cout, 128);
  w.ldw8 = (int)up_to(w.K, 128);
  void* p;
  RC(ctx_arena_alloc(c, rows * (size_t)w.ldw8, &p));  // arena chunks are zero-initialised: padded rows / columns stay 0
  w.w8 = (unsigned char*)p;
  return dtp_quantize_weights_fp8(w.w, w.ldw, w.K, (int)rows, w.w8, w.ldw8, &w.w8_scale, 0);
}

int ensure_ws(Ctx* c) {
  if (c->ws_need <= c->ws_bytes) return DTP_OK;
  HIP_CHECK(hipDeviceSynchronize());
  if (c->ws) HIP_CHECK(hipFree(c->ws));
  c->ws = nullptr;
  HIP_CHECK(hipMalloc(&c->ws, c->ws_need));
  c->ws_bytes = c->ws_need;
  // captured graphs hold the old workspace pointer: drop them, they are re-captured on next use
  graphs_drop_all(c);
  return DTP_OK;
}
