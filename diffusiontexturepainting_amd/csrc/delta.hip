// The changed tiles of an image (include/dtp.h: "changed tiles of an image").  The reference pushes the whole texture to
// the viewport after every stamp (kit_app/.../python/manager.py:349-354).  Here a tracker keeps a shadow copy of what a client already
// has; a scan compares the image with it 16 x 16 texels at a time and emits the tiles that differ, in ascending order, at their rank.
// Three launches in stream order, and no workgroup waits for another: flag + count per group of 64 tiles, one workgroup that scans the
// counts, gather.  Plain HIP: wave64, vector loads and stores, no atomics.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "engine.h"
#include "delta_host.h"

namespace {

constexpr int WAVE_TILES = DELTA_GROUP / 4;  // a workgroup is four waves; each takes 16 consecutive tiles of the group, one at a time
constexpr int SCAN_THREADS = 1024;

// what the kernels need of a tracker; travels as a kernel argument
struct DDev {
  unsigned int* shadow;    // [H][W], one u32 per texel: what the client has
  unsigned char* stale;    // [n_tiles]: 1 = the client's copy of the tile is unknown
  unsigned char* flag;     // [n_tiles]: the last flag pass found the tile changed
  int* group_count;        // [n_groups]: the flagged tiles of a group
  int* group_base;         // [n_groups]: the flagged tiles of all groups before it
  int* ids;                // [capacity]
  unsigned int* tiles;     // [capacity][256]
  int* counts;             // {emitted, remaining}
  int H, W, tiles_x, n_tiles, n_groups, capacity;
};

}  // namespace

struct Delta {
  Ctx* ctx = nullptr;
  DDev d = {};
  dtp_delta_sizes lay = {};
  unsigned char* host = nullptr;  // the pinned block: counts, ids, tiles
};

namespace {

DeltaLive g_live;

// ---------------------------------------------------------------- device
// Pass 1.  One workgroup per group of 64 tiles, one wave per tile: lane l holds texel (l / 16 + 4 q, l % 16) of the tile for q = 0 .. 3,
// one u32 of the image against one of the shadow; texels outside the image are not read.  The tile's flag is its stale mark or any lane's
// difference; the group's count goes through shared memory, in a fixed order.
__global__ __launch_bounds__(256) void delta_flag_kernel(DDev d, const unsigned int* __restrict__ image) {
  __shared__ int s_cnt[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int t0 = blockIdx.x * DELTA_GROUP + wave * WAVE_TILES;
  int cnt = 0;
#pragma unroll 4
  for (int i = 0; i < WAVE_TILES; ++i) {
    const int t = t0 + i;
    const bool valid = t < d.n_tiles;  // (uniform)
    bool differs = false;
    if (valid) {
      const int ty = t / d.tiles_x, tx = t - ty * d.tiles_x;
      const int col = tx * JOURNAL_TILE + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = ty * JOURNAL_TILE + 4 * q + (lane >> 4);
        if (row < d.H && col < d.W) {
          const size_t at = (size_t)row * d.W + col;
          differs |= image[at] != d.shadow[at];
        }
      }
    }
    const bool changed = valid && (__ballot(differs) != 0ull || d.stale[t] != 0);
    if (valid && lane == 0) d.flag[t] = changed ? 1 : 0;
    cnt += changed ? 1 : 0;
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) d.group_count[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// Pass 2.  ONE workgroup: thread i sums a run of ceil(n_groups / 1024) consecutive counts (at most 16 for 1024 x 1024 tiles), the 1024
// sums are scanned in shared memory, and the thread writes the exclusive bases of its run.  The last thread knows the total.
__global__ __launch_bounds__(SCAN_THREADS) void delta_scan_kernel(DDev d) {
  __shared__ int s[SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (d.n_groups + SCAN_THREADS - 1) / SCAN_THREADS;
  const int g0 = min(tid * per, d.n_groups), g1 = min(g0 + per, d.n_groups);
  int sum = 0;
  for (int g = g0; g < g1; ++g) sum += d.group_count[g];
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {
    const int v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int run = s[tid] - sum;
  for (int g = g0; g < g1; ++g) {
    d.group_base[g] = run;
    run += d.group_count[g];
  }
  if (tid == SCAN_THREADS - 1) {
    const int total = s[tid], emitted = min(total, d.capacity);
    d.counts[0] = emitted;
    d.counts[1] = total - emitted;
  }
}

// Pass 3.  The workgroups of pass 1 again.  Every wave ballots the 64 flags of its group; tile k of the group has the rank base + the
// flagged tiles below k.  A tile with a rank below the capacity writes its id and its payload (zero outside the image), takes the
// image's texels into the shadow and clears its stale mark.  Ranks are distinct, so no two waves write one slot.
__global__ __launch_bounds__(256) void delta_gather_kernel(DDev d, const unsigned int* __restrict__ image) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int g = blockIdx.x;
  const int base = d.group_base[g];
  if (d.group_count[g] == 0 || base >= d.capacity) return;  // (uniform)
  const int tl = g * DELTA_GROUP + lane;
  const unsigned long long mask = __ballot(tl < d.n_tiles && d.flag[tl] != 0);
  for (int i = 0; i < WAVE_TILES; ++i) {
    const int k = wave * WAVE_TILES + i;
    if (((mask >> k) & 1ull) == 0ull) continue;  // (uniform)
    const int rank = base + __popcll(mask & ((1ull << k) - 1ull));
    if (rank >= d.capacity) return;  // (ranks ascend with k)
    const int t = g * DELTA_GROUP + k;
    const int ty = t / d.tiles_x, tx = t - ty * d.tiles_x;
    const int col = tx * JOURNAL_TILE + (lane & 15);
    unsigned int* out = d.tiles + (size_t)rank * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = ty * JOURNAL_TILE + 4 * q + (lane >> 4);
      unsigned int v = 0u;
      if (row < d.H && col < d.W) {
        const size_t at = (size_t)row * d.W + col;
        v = image[at];
        d.shadow[at] = v;
      }
      out[64 * q + lane] = v;
    }
    if (lane == 0) {
      d.ids[rank] = t;
      d.stale[t] = 0;
    }
  }
}

// ---------------------------------------------------------------- host
inline int launch_ok() { return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP; }

// the live tracker behind a caller's pointer, or null with the refusal set
Delta* live(const char* who, dtp_delta* p) {
  if (!p) { dtp_set_error("%s: the tracker is NULL", who); return nullptr; }
  if (!g_live.owner(p)) { dtp_set_error("%s: not a live tracker (destroyed?)", who); return nullptr; }
  return (Delta*)p;
}

void delta_free(Delta* t) {
  DDev& d = t->d;
  (void)hipFree(d.shadow); (void)hipFree(d.stale); (void)hipFree(d.flag); (void)hipFree(d.group_count);
  (void)hipFree(d.ids); (void)hipFree(d.tiles); (void)hipFree(d.counts);
  if (t->host) (void)hipHostFree(t->host);
  delete t;
}

// every check of a scan; null with the refusal set
Delta* scan_checked(const char* who, dtp_ctx* ctx, dtp_delta* p, const uint8_t* image, int H, int W) {
  if (!ctx) { dtp_set_error("%s: ctx is NULL", who); return nullptr; }
  Delta* t = live(who, p);
  if (!t) return nullptr;
  if ((const void*)t->ctx != (const void*)ctx) { dtp_set_error("%s: the tracker belongs to another handle", who); return nullptr; }
  char why[160];
  if (!delta_check_image(image, H, W, t->d.H, t->d.W, why, sizeof why)) { dtp_set_error("%s: %s", who, why); return nullptr; }
  return t;
}

int enqueue_scan(Delta* t, const uint8_t* image, hipStream_t s) {
  const DDev& d = t->d;
  const unsigned int* img = (const unsigned int*)image;
  hipLaunchKernelGGL(delta_flag_kernel, dim3(d.n_groups), dim3(256), 0, s, d, img);
  hipLaunchKernelGGL(delta_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, d);
  hipLaunchKernelGGL(delta_gather_kernel, dim3(d.n_groups), dim3(256), 0, s, d, img);
  return launch_ok();
}

}  // namespace

void delta_drop_ctx(Ctx* c) {
  for (const void* p : g_live.take_owner(c)) delta_free((Delta*)p);
}

extern "C" {

int dtp_delta_layout(int H, int W, int capacity_tiles, dtp_delta_sizes* out) {
  char why[160];
  if (!delta_layout(H, W, capacity_tiles, out, why, sizeof why)) { dtp_set_error("dtp_delta_layout: %s", why); return DTP_ERR_ARG; }
  return DTP_OK;
}

int dtp_delta_create(dtp_ctx* ctx, int H, int W, int capacity_tiles, dtp_delta** out) {
  Ctx* c = (Ctx*)ctx;
  char why[160];
  // ---- the arguments, before the first HIP call
  if (!out) { dtp_set_error("dtp_delta_create: out is NULL"); return DTP_ERR_ARG; }
  dtp_delta_sizes lay;
  if (!delta_layout(H, W, capacity_tiles, &lay, why, sizeof why)) { dtp_set_error("dtp_delta_create: %s", why); return DTP_ERR_ARG; }
  if (!c) { dtp_set_error("dtp_delta_create: ctx is NULL"); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(c->device));
  Delta* t = new Delta();
  t->ctx = c;
  t->lay = lay;
  DDev& d = t->d;
  d.H = H; d.W = W; d.tiles_x = lay.tiles_x; d.n_tiles = lay.n_tiles; d.n_groups = lay.n_groups; d.capacity = capacity_tiles;
  hipError_t e = hipMalloc((void**)&d.shadow, lay.shadow_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d.stale, lay.stale_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d.flag, lay.flag_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d.group_count, lay.group_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d.ids, lay.ids_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d.tiles, lay.tiles_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d.counts, lay.counts_bytes);
  if (e == hipSuccess) e = hipHostMalloc((void**)&t->host, lay.host_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemset(d.shadow, 0, lay.shadow_bytes);
  if (e == hipSuccess) e = hipMemset(d.stale, 1, lay.stale_bytes);
  if (e == hipSuccess) e = hipMemset(d.flag, 0, lay.flag_bytes);
  if (e == hipSuccess) e = hipMemset(d.group_count, 0, lay.group_bytes);
  if (e == hipSuccess) e = hipMemset(d.ids, 0, lay.ids_bytes);
  if (e == hipSuccess) e = hipMemset(d.tiles, 0, lay.tiles_bytes);
  if (e == hipSuccess) e = hipMemset(d.counts, 0, lay.counts_bytes);
  if (e != hipSuccess) {
    dtp_set_error("dtp_delta_create: %s (%d x %d, %d tiles, capacity %d)", hipGetErrorString(e), H, W, lay.n_tiles, capacity_tiles);
    delta_free(t);
    return DTP_ERR_HIP;
  }
  d.group_base = d.group_count + lay.n_groups;
  memset(t->host, 0, lay.host_tiles_offset);
  g_live.add(t, c);
  *out = (dtp_delta*)t;
  return DTP_OK;
}

int dtp_delta_destroy(dtp_delta* p) {
  if (!p) return DTP_OK;
  if (!g_live.remove(p)) { dtp_set_error("dtp_delta_destroy: not a live tracker"); return DTP_ERR_ARG; }
  Delta* t = (Delta*)p;
  (void)hipSetDevice(t->ctx->device);
  delta_free(t);  // (hipFree waits for the work that still reads it)
  return DTP_OK;
}

int dtp_delta_reset(dtp_delta* p, dtp_stream s) {
  Delta* t = live("dtp_delta_reset", p);
  if (!t) return DTP_ERR_ARG;
  HIP_CHECK(hipSetDevice(t->ctx->device));
  HIP_CHECK(hipMemsetAsync(t->d.stale, 1, t->lay.stale_bytes, (hipStream_t)s));
  return DTP_OK;
}

int dtp_delta_scan(dtp_ctx* ctx, dtp_delta* p, const uint8_t* image, int H, int W, dtp_stream s) {
  Delta* t = scan_checked("dtp_delta_scan", ctx, p, image, H, W);
  if (!t) return DTP_ERR_ARG;
  HIP_CHECK(hipSetDevice(t->ctx->device));
  return enqueue_scan(t, image, (hipStream_t)s);
}

int dtp_delta_device(dtp_delta* p, int** ids, uint8_t** tiles, int** counts) {
  if (!ids || !tiles || !counts) { dtp_set_error("dtp_delta_device: NULL argument"); return DTP_ERR_ARG; }
  Delta* t = live("dtp_delta_device", p);
  if (!t) return DTP_ERR_ARG;
  *ids = t->d.ids; *tiles = (uint8_t*)t->d.tiles; *counts = t->d.counts;
  return DTP_OK;
}

int dtp_delta_host(dtp_delta* p, int** ids, uint8_t** tiles) {
  if (!ids || !tiles) { dtp_set_error("dtp_delta_host: NULL argument"); return DTP_ERR_ARG; }
  Delta* t = live("dtp_delta_host", p);
  if (!t) return DTP_ERR_ARG;
  *ids = (int*)(t->host + t->lay.host_ids_offset); *tiles = t->host + t->lay.host_tiles_offset;
  return DTP_OK;
}

int dtp_delta_pull(dtp_ctx* ctx, dtp_delta* p, const uint8_t* image, int H, int W, dtp_stream s_, int* host_ids, uint8_t* host_tiles,
                   int max_tiles, int* count, int* remaining) {
  Delta* t = scan_checked("dtp_delta_pull", ctx, p, image, H, W);
  if (!t) return DTP_ERR_ARG;
  char why[160];
  if (!delta_check_pull(host_ids, host_tiles, count, remaining, max_tiles, t->d.capacity, why, sizeof why)) {
    dtp_set_error("dtp_delta_pull: %s", why);
    return DTP_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)s_;
  HIP_CHECK(hipSetDevice(t->ctx->device));
  RC(enqueue_scan(t, image, s));
  int* head = (int*)t->host;
  HIP_CHECK(hipMemcpyAsync(head, t->d.counts, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  const int n = std::min(std::max(head[0], 0), t->d.capacity);
  if (n > 0) {
    HIP_CHECK(hipMemcpyAsync(host_ids, t->d.ids, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(host_tiles, t->d.tiles, (size_t)n * DELTA_TILE_BYTES, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  *count = n;
  *remaining = head[1];
  return DTP_OK;
}

int dtp_op_delta_state(dtp_delta* p, uint8_t* shadow_host, uint8_t* stale_host, dtp_stream s_) {
  Delta* t = live("dtp_op_delta_state", p);
  if (!t) return DTP_ERR_ARG;
  hipStream_t s = (hipStream_t)s_;
  HIP_CHECK(hipSetDevice(t->ctx->device));
  if (shadow_host) HIP_CHECK(hipMemcpyAsync(shadow_host, t->d.shadow, t->lay.shadow_bytes, hipMemcpyDeviceToHost, s));
  if (stale_host) HIP_CHECK(hipMemcpyAsync(stale_host, t->d.stale, t->lay.stale_bytes, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return DTP_OK;
}

}  // extern "C"
