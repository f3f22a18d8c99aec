// Build-time tuner: the persisted (shape -> tile, split-K) table and the timing of every candidate configuration of a contraction.
#include "engine.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

static void tune_read_file(Ctx* c, const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return;
  char key[256];
  int tile, splits;
  while (fscanf(f, "%255s %d %d", key, &tile, &splits) == 3)
    if (tile >= 0 && tile < DTP_TILE_IDS && splits >= 1 && splits <= 64) c->tuned[key] = std::make_pair(tile, splits);  // shape-level checks: tune_entry_valid()
  fclose(f);
}

// $DTP_TUNE_SEED: a read-only table shipped with the package (the choices measured on the build's own MI355X), read first;
// $DTP_TUNE_CACHE: the per-user table this process may extend.  Entries are only trusted after tune_entry_valid().
void tune_cache_load(Ctx* c) {
  const char* seed = getenv("DTP_TUNE_SEED");
  if (seed && *seed) tune_read_file(c, seed);
  const char* e = getenv("DTP_TUNE_CACHE");
  if (!e || !*e) return;
  c->tune_cache_path = e;
  tune_read_file(c, e);
  c->tune_saved = c->tuned.size();
}

// Is (tile, splits) a configuration the launcher accepts for THIS problem?  A persisted table can be stale (older build,
// different packing) or hand-edited: a halo tile without the channel-block-major packing, a GEGLU problem on a tile that is
// not 128 wide, or a split LayerNorm-fold would otherwise reach the kernels.
static bool tune_entry_valid(const GemmParams& p, int tile, int sp) {
  const DtpTile t = dtp_tile(tile);
  GemmParams q = p;
  if (sp < 1 || (sp > p.nkb && t.fam != TF_LNLIN) || !dtp_tile_apply(q, tile, sp)) return false;  // not a factor this tile can realise
  switch (t.fam) {
    case TF_NONE: return false;
    case TF_GEMMWS: return dtp_gemm_ws_supported(p, sp);
    case TF_LNLIN: return dtp_lnlin_supported(p, sp);
    case TF_CONVWS: return dtp_conv_ws_supported(p, t.var, sp);
    case TF_HALO: return p.Wcb && (t.var >= 4 ? dtp_conv_halo3_supported(p) : dtp_conv_halo_supported(p)) && p.batch <= 1;
    default: break;
  }
  if (p.flags & GF_GNAPPLY) return false;  // only the halo kernel normalises its staged input
  if (t.fam == TF_FP8) return dtp_gemm_fp8_supported(q) && !((p.flags & GF_GEGLU) && (t.bn % 128));
  if (t.fam == TF_WIDE) return dtp_gemm_wide_supported(q, t.var);
  if ((p.flags & GF_GEGLU) && (t.bn != 128 || sp != 1)) return false;
  if (sp > 1 && ((p.flags & (GF_LNFOLD | GF_SOFTMAX16)) || p.batch > 1)) return false;
  if (sp > 1 && (size_t)sp * p.M * p.N * sizeof(float) > ((size_t)512 << 20)) return false;  // the fp32 slabs of a split
  return true;
}

void tune_cache_save(Ctx* c) {
  if (c->rep_cold_ms > 0) fprintf(stderr, "[tune] sum over pushed GEMMs: cold %.2f ms, hot %.2f ms\n", c->rep_cold_ms, c->rep_hot_ms);
  if (c->tune_thrash) { (void)hipDeviceSynchronize(); (void)hipFree(c->tune_thrash); c->tune_thrash = nullptr; }
  if (c->tune_cache_path.empty() || c->tuned.size() == c->tune_saved) return;
  // several ranks may share the path: write a private file and rename it into place (atomic)
  const std::string tmp = c->tune_cache_path + ".tmp." + std::to_string((long long)getpid());
  FILE* f = fopen(tmp.c_str(), "w");
  if (!f) return;
  for (auto& kv : c->tuned) fprintf(f, "%s %d %d\n", kv.first.c_str(), kv.second.first, kv.second.second);
  fclose(f);
  (void)rename(tmp.c_str(), c->tune_cache_path.c_str());
  c->tune_saved = c->tuned.size();
}

// The first-round candidates of a problem, as configurations (tile id, splits) in the order they are timed.  ws_ok[v]: the
// weight-streaming conv variant v takes the problem; gw_ok: the weight-streaming GEMM does.
struct TuneCfg { int tile, sp; };
static std::vector<TuneCfg> tune_candidates(const Ctx* c, const GemmParams& p, const bool* ws_ok, bool gw_ok) {
  static const int cand_splits[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
  const bool geglu = (p.flags & GF_GEGLU) != 0;
  std::vector<TuneCfg> out;
  auto add = [&](int tile, int sp) {  // a split the tile cannot realise, or fp32 slabs over 512 MiB, is not a candidate
    GemmParams q = p;
    if (dtp_tile_apply(q, tile, sp) && dtp_gemm_workspace_bytes(q) <= ((size_t)512 << 20)) out.push_back({tile, sp});
  };
  // gemm_kernel in all its shapes, depths and wave layouts, the 8-wave wide tiles and fp8
  for (int tile = 0; tile < DTP_TILE_IDS && !(p.flags & GF_GNAPPLY); ++tile) {
    const DtpTile t = dtp_tile(tile);
    if (t.fam != TF_GEMM && t.fam != TF_WIDE && t.fam != TF_FP8) continue;
    // fp8 tiles need the e4m3 weight copy.  An fp8 problem keeps the choice of an fp16 tile while it is small (the register-
    // staged activation operand costs latency-bound launches more than the MX MFMA returns: 256^2 / 8 steps 32.6 -> 27.5 ms);
    // from M = 6144 on (every level-0..2 Linear of a batch-8 stamp) it runs on the fp8 tiles only -- there the cold single-launch
    // timing of the tuner under-rates them (batch 8: 588 ms with fp8 tiles throughout, 606 ms with the tuner's mix, 605 ms in fp16)
    if (t.fam == TF_FP8 ? !p.W8 : (p.W8 && p.M >= 6144)) continue;
    const long long ntiles = (long long)((p.M + t.bm - 1) / t.bm) * ((p.N + t.bn - 1) / t.bn);
    if (t.fam == TF_FP8) {
      if (!(geglu && (t.bn % 128)) && !(t.var == 4 && ntiles < 96)) add(tile, 1);
      continue;
    }
    if (t.fam == TF_WIDE) {  // gemm_wide_kernel: unsplit big-M problems only (at least half a wave of 256 CUs worth of tiles)
      GemmParams q = p;
      q.splits = 1;
      if (!dtp_gemm_wide_supported(q, t.var) || ntiles < 96) continue;
      if (t.var == 1 && (p.N % 320) > 0 && (p.N % 320) <= 192) continue;  // a mostly empty last column tile: 256 x 256 covers it better
      add(tile, 1);
      continue;
    }
    if (geglu && t.bn != 128) continue;
    if (p.nkb < 3 && t.ns > 2) continue;
    if ((t.bm == 256 && p.M < 192) || (t.bn == 256 && p.N < 192)) continue;
    for (int sp : cand_splits) {
      if (sp > 1 && (geglu || (p.flags & GF_LNFOLD) || p.batch > 1 || p.nkb / sp < 2)) break;
      add(tile, sp);
    }
  }
  {  // the activation-stationary kernel of the short LayerNorm-folded contractions: column ranges per 128-row block
    static const int ranges[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40};
    for (int sp : ranges)
      if (c->tune_lnlin && dtp_lnlin_supported(p, sp)) add(DTP_TILE_LNLIN, sp);
  }
  for (int tile = 0; tile < DTP_TILE_IDS && p.Wcb && dtp_conv_halo_supported(p); ++tile) {  // the halo-tiled conv kernels (Wcb packing)
    const DtpTile t = dtp_tile(tile);
    if (t.fam != TF_HALO) continue;
    const bool small = p.Hi * p.Wi <= 256;
    // 8x8 pixel tiles for small feature maps, 8x16 otherwise; three images per workgroup: the small maps of a batch-1 stamp, where
    // the weight slices are most of the LDS fill
    if (t.var < 4 ? (t.var >= 2) != small : (!c->tune_halo3 || !small || !dtp_conv_halo3_supported(p))) continue;
    for (int sp : cand_splits) {
      if (sp > 1 && p.nkb / sp < 9) break;
      add(tile, sp);
    }
  }
  for (int tile = 0; tile < DTP_TILE_IDS; ++tile) {  // the weight-streaming conv: K-slices = ranges of whole channel blocks
    const DtpTile t = dtp_tile(tile);
    static const int slices[] = {1, 2, 3, 4, 5, 6, 8, 10};
    if (t.fam != TF_CONVWS) continue;
    for (int sp : slices) {
      if (!c->conv_ws || !ws_ok[t.var] || !dtp_conv_ws_supported(p, t.var, sp)) continue;
      if (t.var >= 2 && sp > 4) continue;
      add(tile, sp);
    }
  }
  if (gw_ok) {  // the weight-streaming GEMM: K-slices = ranges of whole k-blocks
    static const int slices[] = {1, 2, 3, 4, 5, 6, 8};
    for (int sp : slices)
      if (dtp_gemm_ws_supported(p, sp) && !(sp > 1 && p.nkb / sp < 4)) add(DTP_TILE_GEMMWS, sp);
  }
  return out;
}

// Build-time autotuning: the stamp path has ~100 distinct contraction shapes, most of them far from
// "large square GEMM" (M from 192 to 524288, N from 3 to 10240).  Each distinct shape is timed once
// with every tile variant x split-K factor on the real buffers and the fastest pair is kept.
// (*tile, *sp) is the caller's configuration on entry, the one to use on return.
int tune_gemm(Ctx* c, const GemmParams& p, int* tile, int* sp) {
  char key[200];
  // "k8|": bump when tile ids or pipelines change, so that a persisted table written by an older build is ignored
  int kl = snprintf(key, sizeof(key), "k8|%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", p.M, p.N, p.K, p.flags & ~GF_MFAST, p.Hi, p.Wi, p.Cin,
                    p.stride, p.lda, p.ldc, p.ldw, p.st_parts, p.Cin2, p.lda2);
  if (p.batch > 1) kl += snprintf(key + kl, sizeof(key) - kl, ",b%d", p.batch);
  if (p.W8) kl += snprintf(key + kl, sizeof(key) - kl, ",f8");
  // problems the weight-streaming conv can take were tuned without it by older tables: their key carries a marker
  bool ws_ok[DTP_WS_VARIANTS];
  bool ws_any = false;
  for (int v = 0; v < DTP_WS_VARIANTS; ++v) { ws_ok[v] = p.Wfr && (p.flags & GF_CONV3) && dtp_conv_ws_supported(p, v, 1); ws_any = ws_any || ws_ok[v]; }
  if (ws_any) kl += snprintf(key + kl, sizeof(key) - kl, ",ws2");
  // ... and the upsampler convs the phase build takes (variants 4 / 5 = tile ids 56 / 57) were tuned without it: theirs carries another
  if (ws_ok[4] || ws_ok[5]) kl += snprintf(key + kl, sizeof(key) - kl, ",u4");
  // ... and so do the plain problems the activation-stationary Linear takes since round 4 (attention output projection, grouped proj_in)
  if (!(p.flags & GF_LNFOLD)) {
    bool ll = false;
    for (int r = 1; r <= 40 && !ll; ++r) ll = dtp_lnlin_supported(p, r);
    if (ll) snprintf(key + kl, sizeof(key) - kl, ",ll");
  }
  // ... and the dense problems the weight-streaming GEMM takes (gemm_ws.hip)
  const bool gw_ok = dtp_gemm_ws_supported(p, 1);
  if (gw_ok) { kl = (int)strlen(key); snprintf(key + kl, sizeof(key) - kl, ",gw"); }
  auto it = c->tuned.find(key);
  if (it != c->tuned.end() && !tune_entry_valid(p, it->second.first, it->second.second)) {
    fprintf(stderr, "[dtp] tune table entry '%s' -> (%d, %d) does not fit the problem; re-tuning\n", key, it->second.first, it->second.second);
    c->tuned.erase(it);
    it = c->tuned.end();
  }
  if (it == c->tuned.end()) {
    if (!c->tune_ev[0]) { HIP_CHECK(hipEventCreate(&c->tune_ev[0])); HIP_CHECK(hipEventCreate(&c->tune_ev[1])); }
    constexpr size_t THRASH_BYTES = (size_t)512 << 20;
    if (!c->tune_thrash) HIP_CHECK(hipMalloc(&c->tune_thrash, THRASH_BYTES));
    const size_t a_bytes = (p.flags & GF_CONV3) ? (size_t)(p.M / (p.Ho * p.Wo)) * p.Hi * p.Wi * p.lda * 2 : (size_t)p.M * p.lda * 2;
    // Timed the way the stamp sees it (cold): weights COLD (1.7 GB of them stream through the 256 MiB Infinity Cache every UNet
    // evaluation), activations warm (just written by the previous kernel); minimum over `reps` runs (a single cold run is noisy:
    // DVFS, thrash write-back still draining).  Hot: nothing evicted, the first run not counted.
    auto time_cfg = [&](int cfg_tile, int cfg_sp, int reps, bool cold, float* out_ms) -> int {
      GemmParams q = p;
      (void)dtp_tile_apply(q, cfg_tile, cfg_sp);
      const size_t need = dtp_gemm_workspace_bytes(q);
      if (need > c->ws_bytes) { c->ws_need = std::max(c->ws_need, need); RC(ensure_ws(c)); }
      q.part = c->ws;
      q.zero = c->zero;
      float ms = 1e30f;
      for (int rep = 0; rep < reps; ++rep) {
        if (cold) {
          HIP_CHECK(hipMemsetAsync(c->tune_thrash, rep, THRASH_BYTES, 0));
          RC(dtp_launch_touch(q.A, a_bytes, (float*)c->tune_thrash, 0));
          if (q.R) RC(dtp_launch_touch(q.R, (size_t)q.M * q.ldr * 2, (float*)c->tune_thrash, 0));
        }
        HIP_CHECK(hipEventRecord(c->tune_ev[0], 0));
        RC(dtp_launch_tile(q, cfg_tile, 0));
        HIP_CHECK(hipEventRecord(c->tune_ev[1], 0));
        HIP_CHECK(hipEventSynchronize(c->tune_ev[1]));
        float ev = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ev, c->tune_ev[0], c->tune_ev[1]));
        if (cold || rep) ms = std::min(ms, ev);
      }
      *out_ms = ms;
      return DTP_OK;
    };
    struct Cand { float ms; int tile, sp; };
    std::vector<Cand> cands;
    for (const TuneCfg& cfg : tune_candidates(c, p, ws_ok, gw_ok)) {
      float ms;
      RC(time_cfg(cfg.tile, cfg.sp, 5, true, &ms));
      cands.push_back({ms, cfg.tile, cfg.sp});
    }
    // second round: the three fastest candidates are usually within the measurement noise of each other -- time them again,
    // longer, and keep the minimum over both rounds
    std::sort(cands.begin(), cands.end(), [](const Cand& x, const Cand& y) { return x.ms < y.ms; });
    for (size_t i = 0; i < cands.size() && i < 3; ++i) {
      float ms;
      RC(time_cfg(cands[i].tile, cands[i].sp, 8, true, &ms));
      cands[i].ms = std::min(cands[i].ms, ms);
    }
    float best = 1e30f;
    int bt = *tile, bs = *sp;
    for (size_t i = 0; i < cands.size() && i < 3; ++i)
      if (cands[i].ms < best) { best = cands[i].ms; bt = cands[i].tile; bs = cands[i].sp; }
    // A conv is ranked by its own launch, but an UNSPLIT two-n-tile convws launch (tile 53 / 54) also delivers the GroupNorm statistics of
    // its output (Builder::claim_stats), i.e. it saves its consumer a statistics pass: one dispatch floor plus one read of the tensor.
    // Round 5 found the level-0 long-shortcut convs on the halo kernel by 1-2 us -- and 76 statistics launches per stamp behind them
    // (switched by hand in the shipped table: -0.4 % at batch 1; at batch 8 the halo kernel's lead is larger than the pass).  The
    // statistics-capable candidate is credited with that pass when its output is one claim_stats would take.
    // (the tune key does not know the consumer: an output of such a shape is followed by a GroupNorm everywhere in these networks --
    // conv_out has N = 4 / 3, which the predicate excludes -- but in the up path that GroupNorm runs over a concatenation and cannot claim)
    if (ws_any && dtp_tile(bt).fam != TF_CONVWS && dtp_conv_output_can_carry_gn_stats(p)) {
      const float stats_ms = 0.005f + (float)((double)p.M * p.N * 2.0 / 4.0e12 * 1e3);  // dispatch floor + the tensor once at ~4 TB/s
      for (const Cand& cd : cands) {
        const DtpTile t = dtp_tile(cd.tile);
        if (cd.sp == 1 && t.fam == TF_CONVWS && t.var >= 2 && cd.ms - stats_ms < best) { best = cd.ms - stats_ms; bt = cd.tile; bs = 1; }
      }
    }
    it = c->tuned.emplace(key, std::make_pair(bt, bs)).first;
    if (getenv("DTP_TUNE_REPORT")) {  // how much of the chosen configuration's time is the cold operands?
      float hot;
      RC(time_cfg(bt, bs, 4, false, &hot));
      c->tune_ms[key] = std::make_pair(best, hot);
    }
  }
  {
    auto m = c->tune_ms.find(key);
    if (m != c->tune_ms.end()) {
      c->rep_cold_ms += m->second.first;
      c->rep_hot_ms += m->second.second;
      fprintf(stderr, "[tune] %s tile=%d sp=%d cold %.1f us hot %.1f us\n", key, it->second.first, it->second.second, m->second.first * 1e3,
              m->second.second * 1e3);
    }
  }
  *tile = it->second.first;
  *sp = it->second.second;
  return DTP_OK;
}
