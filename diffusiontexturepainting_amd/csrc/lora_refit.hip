// LoRA refit of a finalized handle (include/dtp.h: dtp_refit_stage / dtp_refit_lora): every LoRA-targetable matrix is
// rebuilt as base + scale * up @ down from its fp32 pre-merge copy and written over the packed fp16 rows the launch programs read, in
// place -- programs, tune entries and captured graphs keep their pointers.  Reference: Engine.refit (trt_inference/utilities.py:88-189)
// and the scaled merge of trt_inference/models.py:1034,1083.
// The arithmetic is weight_math.h's, the functions the load path (lora_merge_kernel, scale_cols_kernel, pack_linear_kernel, rowdot_kernel,
// rowsum_f16_kernel, transpose_f16_kernel) runs: a refitted handle equals a fresh one bit for bit by construction.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "engine.h"
#include "weight_math.h"

namespace {

constexpr int RF_KC = 512;   // columns per workgroup: 64 lanes x 8 consecutive k
constexpr int RF_IT = 4;     // rows per wave
constexpr int RF_ROWS = 4 * RF_IT;  // rows per workgroup
constexpr int RF_RC = 16;    // rows of `down` staged per pass: 16 x 512 floats = 32 KB of LDS; a larger rank takes several passes

// grid (row blocks, column chunks, jobs), sized by the largest job; a workgroup outside its job's matrix leaves at once.
// A thread owns 8 consecutive k of RF_IT rows: the rank reduction continues one fused-multiply-add chain per element across the passes
// (lora_accumulate: r ascending, as lora_merge_kernel), then merge, fold, round and ONE 16-byte store per row.
__global__ __launch_bounds__(256) void lora_refit_kernel(const LoraRefitJob* __restrict__ jobs, float scale) {
  __shared__ __attribute__((aligned(16))) float dn[RF_RC][RF_KC];
  const LoraRefitJob j = jobs[blockIdx.z];
  const int k0 = blockIdx.y * RF_KC, n0 = blockIdx.x * RF_ROWS;
  if (k0 >= j.K || n0 >= j.N) return;  // (uniform over the workgroup)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int kl = lane * 8, k = k0 + kl;
  const bool kin = k < j.K;  // K % 8 == 0: a thread's 8 columns are all inside or all outside
  float acc[RF_IT][8];
#pragma unroll
  for (int it = 0; it < RF_IT; ++it)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[it][e] = 0.f;
  for (int r0 = 0; r0 < j.rank; r0 += RF_RC) {
    const int nr = min(RF_RC, j.rank - r0);
    if (r0) __syncthreads();
    for (int i = threadIdx.x; i < nr * (RF_KC / 4); i += 256) {  // down rows [r0, r0 + nr), columns [k0, k0 + RF_KC): once per workgroup
      const int r = i / (RF_KC / 4), c4 = (i % (RF_KC / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + c4 < j.K) v = *(const f32x4*)(j.down + (size_t)(r0 + r) * j.K + k0 + c4);
      *(f32x4*)&dn[r][c4] = v;
    }
    __syncthreads();
    if (kin) {
#pragma unroll
      for (int it = 0; it < RF_IT; ++it) {
        const int n = n0 + it * 4 + wv;
        if (n >= j.N) continue;
        const float* up_row = j.up + (size_t)n * j.rank + r0;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[it][e] = lora_accumulate(acc[it][e], up_row, &dn[0][kl + e], RF_KC, nr);
      }
    }
  }
  if (!kin) return;
  float g[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
  if (j.gamma) {
    const f32x4 g0 = *(const f32x4*)(j.gamma + k), g1 = *(const f32x4*)(j.gamma + k + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[e] = g0[e]; g[4 + e] = g1[e]; }
  }
#pragma unroll
  for (int it = 0; it < RF_IT; ++it) {
    const int n = n0 + it * 4 + wv;
    if (n >= j.N) continue;
    const float* b = j.base + (size_t)n * j.K + k;
    const f32x4 b0 = *(const f32x4*)b, b1 = *(const f32x4*)(b + 4);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float w = lora_merged(e < 4 ? b0[e] : b1[e - 4], scale, acc[it][e]);
      if (j.gamma) w = ln_fold_gamma(w, g[e]);
      o[e] = pack_weight_f16(w);
    }
    *(f16x8*)(j.dst + (size_t)(j.row0 + n) * j.ldw + k) = o;
  }
}

// The folded bias rows b'[n] = 0 + sum_k W[n][k] beta[k] over the merged, un-folded fp32 W (load_linear: rowdot_kernel on the merged
// tensor, added to a zero bias on the host): one wave per row, the merged weight recomputed per element instead of read back.
__global__ __launch_bounds__(256) void lora_wbeta_kernel(const LoraRefitJob* __restrict__ jobs, float scale) {
  const LoraRefitJob j = jobs[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (!j.beta || row >= j.N) return;
  const float* br = j.base + (size_t)row * j.K;
  const float* ur = j.up + (size_t)row * j.rank;
  const float acc = wave_rowdot([&](int k) { return lora_merged(br[k], scale, lora_accumulate(0.f, ur, j.down + k, j.K, j.rank)); }, j.beta, j.K, lane);
  if (lane == 0) j.wbeta[row] = 0.f + acc;
}

__global__ __launch_bounds__(256) void rowsum_f16_grouped_kernel(const RowsumJob* __restrict__ jobs) {
  const RowsumJob j = jobs[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= j.rows) return;
  const float acc = wave_rowsum_f16(j.w + (size_t)row * j.ld, j.K, lane);
  if (lane == 0) j.out[row] = acc;
}

__global__ __launch_bounds__(256) void transpose_f16_grouped_kernel(const TransposeJob* __restrict__ jobs) {
  __shared__ f16 t[32][33];
  const TransposeJob j = jobs[blockIdx.z];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  if (bx >= j.cols || by >= j.rows) return;  // (uniform over the workgroup)
  transpose_tile_f16(t, j.src, j.lds, j.dst, j.ldd, j.rows, j.cols, bx, by);
}

int launch_ok() { return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP; }

}  // namespace

int dtp_launch_lora_refit(const LoraRefitJob* jobs, int njobs, int max_n, int max_k, float scale, hipStream_t s) {
  if (njobs < 1 || njobs > 65535 || max_n < 1 || max_k < 1) { dtp_set_error("lora_refit: bad job table (%d jobs, N <= %d, K <= %d)", njobs, max_n, max_k); return DTP_ERR_ARG; }
  const dim3 grid((max_n + RF_ROWS - 1) / RF_ROWS, (max_k + RF_KC - 1) / RF_KC, njobs);
  hipLaunchKernelGGL(lora_refit_kernel, grid, dim3(256), 0, s, jobs, scale);
  return launch_ok();
}
int dtp_launch_lora_wbeta(const LoraRefitJob* jobs, int njobs, int max_n, float scale, hipStream_t s) {
  if (njobs < 1 || njobs > 65535 || max_n < 1) { dtp_set_error("lora_wbeta: bad job table"); return DTP_ERR_ARG; }
  hipLaunchKernelGGL(lora_wbeta_kernel, dim3((max_n + 3) / 4, njobs), dim3(256), 0, s, jobs, scale);
  return launch_ok();
}
int dtp_launch_rowsum_f16_grouped(const RowsumJob* jobs, int njobs, int max_rows, hipStream_t s) {
  if (njobs < 1 || njobs > 65535 || max_rows < 1) { dtp_set_error("rowsum_f16_grouped: bad job table"); return DTP_ERR_ARG; }
  hipLaunchKernelGGL(rowsum_f16_grouped_kernel, dim3((max_rows + 3) / 4, njobs), dim3(256), 0, s, jobs);
  return launch_ok();
}
int dtp_launch_transpose_f16_grouped(const TransposeJob* jobs, int njobs, int max_rows, int max_cols, hipStream_t s) {
  if (njobs < 1 || njobs > 65535 || max_rows < 1 || max_cols < 1) { dtp_set_error("transpose_f16_grouped: bad job table"); return DTP_ERR_ARG; }
  hipLaunchKernelGGL(transpose_f16_grouped_kernel, dim3((max_cols + 31) / 32, (max_rows + 31) / 32, njobs), dim3(256), 0, s, jobs);
  return launch_ok();
}

// ---------------------------------------------------------------- C ABI
static void refit_clear_staged(Ctx* c) {
  for (auto& s : c->refit_staged) (void)hipFree(s.second.d);
  c->refit_staged.clear();
}

// what a refit cannot follow: weights not packed yet; e4m3 copies calibrated per program; the fragment-order copy of $DTP_GEMMWS
static int refit_state_check(Ctx* c, const char* who) {
  if (!c->finalized) { dtp_set_error("%s: weights not finalized (before dtp_finalize_weights the LoRA goes through dtp_load_tensor)", who); return DTP_ERR_STATE; }
  if (c->fp8_linear || c->fp8_attention || c->fp8_operands) {
    dtp_set_error("%s: a LoRA refit is not offered under the fp8 options (parity-only, calibrated per program)", who);
    return DTP_ERR_STATE;
  }
  if (c->gemm_ws) { dtp_set_error("%s: a LoRA refit is not offered with the fragment-order Linear packing (DTP_GEMMWS)", who); return DTP_ERR_STATE; }
  return DTP_OK;
}

static bool ends_with(const std::string& s, const char* tail) {
  const size_t n = strlen(tail);
  return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

// "lora.<module>.processor.<proj>_lora.{down,up}.weight" -> the target's staged name and the name of the other half of the pair
static bool refit_parse(const std::string& name, bool* is_down, std::string* target, std::string* other) {
  const bool dn = ends_with(name, "_lora.down.weight"), up = ends_with(name, "_lora.up.weight");
  const size_t pp = name.find(".processor.");
  if (name.rfind("lora.", 0) != 0 || (!dn && !up) || pp == std::string::npos || pp <= 5) return false;
  const size_t tail = dn ? strlen("_lora.down.weight") : strlen("_lora.up.weight"), ps = pp + strlen(".processor.");
  if (name.size() < ps + tail + 1) return false;
  const std::string module = name.substr(5, pp - 5), proj = name.substr(ps, name.size() - tail - ps);
  *is_down = dn;
  *target = "unet." + module + (proj == "to_out" ? ".to_out.0.weight" : "." + proj + ".weight");
  *other = "lora." + module + ".processor." + proj + (dn ? "_lora.up.weight" : "_lora.down.weight");
  return true;
}

extern "C" {

int dtp_refit_stage(dtp_ctx* ctx, const char* name, const float* data, int is_device, const int64_t* shape, int ndim) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !name || !data || !shape || ndim < 1 || ndim > 4) { dtp_set_error("dtp_refit_stage: bad argument (null handle, name, data or shape; ndim 1..4)"); return DTP_ERR_ARG; }
  RC(refit_state_check(c, "dtp_refit_stage"));
  HIP_CHECK(hipSetDevice(c->device));
  Staged s;
  s.n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 1) { dtp_set_error("dtp_refit_stage: '%s' has an empty dimension", name); return DTP_ERR_ARG; }
    s.shape.push_back(shape[i]);
    s.n *= (size_t)shape[i];
  }
  HIP_CHECK(hipMalloc(&s.d, std::max<size_t>(s.n * 4, 16)));
  const hipError_t e = hipMemcpy(s.d, data, s.n * 4, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(s.d); dtp_set_error("dtp_refit_stage: copy of '%s' failed: %s", name, hipGetErrorString(e)); return DTP_ERR_HIP; }
  auto it = c->refit_staged.find(name);
  if (it != c->refit_staged.end()) { (void)hipFree(it->second.d); c->refit_staged.erase(it); }
  c->refit_staged.emplace(name, std::move(s));
  return DTP_OK;
}

// everything is checked against the target table before the first byte is written
static int refit_plan(Ctx* c, std::vector<LoraRefitJob>& jobs) {
  std::unordered_map<std::string, size_t> index;
  for (size_t i = 0; i < c->refit_targets.size(); ++i) index[c->refit_targets[i].name] = i;
  jobs.clear();
  for (const RefitTarget& t : c->refit_targets) jobs.push_back(t.job);  // rank 0: the matrix becomes its base
  for (auto& kv : c->refit_staged) {
    const std::string& name = kv.first;
    bool is_down;
    std::string target, other;
    if (!refit_parse(name, &is_down, &target, &other)) {
      dtp_set_error("dtp_refit_lora: '%s' is not a LoRA tensor name (lora.<module>.processor.<proj>_lora.{down,up}.weight)", name.c_str());
      return DTP_ERR_ARG;
    }
    auto ti = index.find(target);
    if (ti == index.end()) { dtp_set_error("dtp_refit_lora: '%s' has no target: the UNet has no '%s'", name.c_str(), target.c_str()); return DTP_ERR_ARG; }
    auto oi = c->refit_staged.find(other);
    if (oi == c->refit_staged.end()) { dtp_set_error("dtp_refit_lora: '%s' is staged without '%s'", name.c_str(), other.c_str()); return DTP_ERR_MISSING; }
    LoraRefitJob& j = jobs[ti->second];
    const Staged& s = kv.second;
    if (is_down) {  // [rank][K]
      if (s.shape.size() != 2 || s.shape[1] != j.K || s.shape[0] > 65536) {
        dtp_set_error("dtp_refit_lora: shape of '%s' does not fit its target '%s' [%d, %d] (want [rank, %d])", name.c_str(), target.c_str(), j.N, j.K, j.K);
        return DTP_ERR_ARG;
      }
      j.down = s.d;
      j.rank = (int)s.shape[0];
    } else {  // [N][rank], the rank of its down
      const Staged& d = oi->second;
      if (s.shape.size() != 2 || s.shape[0] != j.N || (d.shape.size() == 2 && s.shape[1] != d.shape[0])) {
        dtp_set_error("dtp_refit_lora: shape of '%s' does not fit its target '%s' [%d, %d] (want [%d, rank of its down])", name.c_str(), target.c_str(), j.N, j.K, j.N);
        return DTP_ERR_ARG;
      }
      j.up = s.d;
    }
  }
  for (const LoraRefitJob& j : jobs)
    if ((j.K & 7) || (j.ldw & 7) || j.K > j.ldw) { dtp_set_error("dtp_refit_lora: a target with K = %d, ldw = %d is not supported (multiples of 8)", j.K, j.ldw); return DTP_ERR_ARG; }
  return DTP_OK;
}

int dtp_refit_lora(dtp_ctx* ctx, float scale) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { dtp_set_error("dtp_refit_lora: null handle"); return DTP_ERR_ARG; }
  struct Clear {  // success or failure, nothing stays staged
    Ctx* c;
    ~Clear() { refit_clear_staged(c); }
  } clear{c};
  (void)hipSetDevice(c->device);
  RC(refit_state_check(c, "dtp_refit_lora"));
  if (!isfinite(scale)) { dtp_set_error("dtp_refit_lora: scale must be finite"); return DTP_ERR_ARG; }
  if (c->refit_targets.empty()) { dtp_set_error("dtp_refit_lora: the handle has no refit targets"); return DTP_ERR_STATE; }
  std::vector<LoraRefitJob> jobs;
  RC(refit_plan(c, jobs));
  // ---- nothing was written up to here
  HIP_CHECK(hipDeviceSynchronize());  // the work already enqueued on the handle reads the old weights
  const size_t nj = jobs.size(), nr = c->refit_rowsums.size(), nt = c->refit_transposes.size();
  const size_t off_r = nj * sizeof(LoraRefitJob), off_t = off_r + nr * sizeof(RowsumJob), total = off_t + nt * sizeof(TransposeJob);
  if (!c->refit_tables) {
    RC(ctx_persistent(c, total, &c->refit_tables, true));
    for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventCreate(&c->refit_ev[i]));
  }
  char* tab = (char*)c->refit_tables;
  HIP_CHECK(hipMemcpy(tab, jobs.data(), off_r, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(tab + off_r, c->refit_rowsums.data(), nr * sizeof(RowsumJob), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(tab + off_t, c->refit_transposes.data(), nt * sizeof(TransposeJob), hipMemcpyHostToDevice));
  int max_n = 0, max_k = 0, max_rows = 0, max_tr = 0, max_tc = 0;
  for (const LoraRefitJob& j : jobs) { max_n = std::max(max_n, j.N); max_k = std::max(max_k, j.K); }
  for (const RowsumJob& j : c->refit_rowsums) max_rows = std::max(max_rows, j.rows);
  for (const TransposeJob& j : c->refit_transposes) { max_tr = std::max(max_tr, j.rows); max_tc = std::max(max_tc, j.cols); }
  hipStream_t s = 0;
  HIP_CHECK(hipEventRecord(c->refit_ev[0], s));
  RC(dtp_launch_lora_refit((const LoraRefitJob*)tab, (int)nj, max_n, max_k, scale, s));          // the packed rows of all targets
  RC(dtp_launch_lora_wbeta((const LoraRefitJob*)tab, (int)nj, max_n, scale, s));                 // b' of the LayerNorm-folded stacks
  RC(dtp_launch_rowsum_f16_grouped((const RowsumJob*)(tab + off_r), (int)nr, max_rows, s));      // lns, from the rewritten rows
  RC(dtp_launch_transpose_f16_grouped((const TransposeJob*)(tab + off_t), (int)nt, max_tr, max_tc, s));  // q2T, likewise
  HIP_CHECK(hipEventRecord(c->refit_ev[1], s));
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipEventElapsedTime(&c->refit_ms, c->refit_ev[0], c->refit_ev[1]));
  c->refit_matrices = (int)nj;
  c->refit_launches = 4;
  // the per-stamp cross-attention matrices (UNetProg::xW1 / xW2) were built from the old attn2 weights: the next stamp rebuilds them
  for (auto& p : c->unet_progs) { p.second.kv_ver = 0; p.second.kv_slots.clear(); p.second.kv_slot_ver.clear(); }
  return DTP_OK;
}

int dtp_last_refit_info(dtp_ctx* ctx, int* matrices, int* launches, float* ms) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { dtp_set_error("dtp_last_refit_info: null handle"); return DTP_ERR_ARG; }
  if (c->refit_matrices < 0) { dtp_set_error("dtp_last_refit_info: no refit has run on this handle"); return DTP_ERR_STATE; }
  if (matrices) *matrices = c->refit_matrices;
  if (launches) *launches = c->refit_launches;
  if (ms) *ms = c->refit_ms;
  return DTP_OK;
}

int dtp_op_lora_refit(const float* w0, const float* up, const float* down, int rank, float scale, const float* gamma, void* out, int row0,
                      int N, int K, int ldw, dtp_stream s_) {
  static std::mutex mu;
  static LoraRefitJob* slot = nullptr;  // one device job record, reused (the call waits for its launch)
  if (!w0 || !out || rank < 0 || (rank > 0 && (!up || !down)) || row0 < 0 || N < 1 || K < 8 || (K & 7) || (ldw & 7) || ldw < K || !isfinite(scale)) {
    dtp_set_error("dtp_op_lora_refit: bad argument (rank=%d row0=%d N=%d K=%d ldw=%d; K and ldw multiples of 8, ldw >= K, finite scale)", rank, row0, N, K, ldw);
    return DTP_ERR_ARG;
  }
  if (((uintptr_t)w0 | (uintptr_t)down | (uintptr_t)gamma | (uintptr_t)out) & 15) { dtp_set_error("dtp_op_lora_refit: w0, down, gamma and out must be 16-byte aligned"); return DTP_ERR_ARG; }
  std::lock_guard<std::mutex> lk(mu);
  hipStream_t s = (hipStream_t)s_;
  if (!slot) HIP_CHECK(hipMalloc(&slot, sizeof(LoraRefitJob)));
  LoraRefitJob j = {};
  j.base = w0; j.up = up; j.down = down; j.gamma = gamma; j.dst = (f16*)out;
  j.rank = rank; j.N = N; j.K = K; j.row0 = row0; j.ldw = ldw;
  HIP_CHECK(hipMemcpy(slot, &j, sizeof(j), hipMemcpyHostToDevice));
  RC(dtp_launch_lora_refit(slot, 1, N, K, scale, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return DTP_OK;
}

}  // extern "C"
