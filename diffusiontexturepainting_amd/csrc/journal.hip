// The undo / redo journal of a texture (include/dtp.h: "undo / redo journal of a texture").  The reference copies the whole
// texture to the host before every stroke and uploads a copy on Ctrl+Z (kit_app/.../python/ui/brush.py:52-77,131-137).  Here the first
// write of a record into a 16 x 16-texel tile is preceded by a copy of the tile's old texels into a ring of 1 KiB slots on the device; undo
// and redo swap slots and tiles.  Everything is in stream order; the painting path reads nothing back.  Plain HIP: vector loads and
// stores and device atomics only.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <set>
#include <vector>

#include "engine.h"
#include "journal_host.h"

namespace {

constexpr int RECTS_PER_LAUNCH = 32;  // tile rectangles that travel as one kernel argument
constexpr int N_COUNTERS = 1 + 2 * JOURNAL_MAX_DEPTH;  // head, then (start, end) of every record row

// what the kernels need of a journal; travels as a kernel argument
struct JDev {
  unsigned int* tex;         // the guarded texture, one u32 per texel
  unsigned int* slots;       // [capacity][256]
  int* tile_gen;             // [n_tiles]: the gen of the record that saved the tile last (0: none)
  int* slot_tile;            // [capacity]: the tile a slot holds (-1: never taken)
  unsigned long long* head;  // the slots ever taken
  int H, W, tiles_x, n_tiles, capacity;
};
struct JRects { int n, r[RECTS_PER_LAUNCH][4]; };  // tile rectangles {tx0, ty0, tx1, ty1}, inclusive, inside the texture

}  // namespace

struct Journal {
  Ctx* ctx = nullptr;
  JDev d = {};
  JournalList list;
  unsigned long long* counters = nullptr;  // device [N_COUNTERS]; d.head = counters
  unsigned long long* host = nullptr;      // pinned [N_COUNTERS]: where undo / redo / info read them back
  hipStream_t last = nullptr;              // the stream the journal was used on last
};

namespace {

std::mutex g_mu;
std::set<Journal*> g_journals;  // the live journals: a destroyed handle is refused, not followed

// ---------------------------------------------------------------- device
// The whole workgroup, uniformly: thread 0 claims tile t for the record `gen` (the first exchange that finds another value wins, so a
// tile is saved once per record whoever else asks in this launch or a later one) and takes the next slot of the ring; then thread i
// copies texel (i / 16, i % 16) of the tile, one u32, rows of 64 bytes.  Texels outside the texture are not read and their slot words
// not written.
__device__ __forceinline__ void save_tile(const JDev& d, int gen, int t, int* s_slot) {
  if (threadIdx.x == 0) {
    int slot = -1;
    if (atomicExch(&d.tile_gen[t], gen) != gen) {
      const unsigned long long k = atomicAdd(d.head, 1ull);
      slot = (int)(k % (unsigned long long)d.capacity);
      d.slot_tile[slot] = t;
    }
    *s_slot = slot;
  }
  __syncthreads();
  const int slot = *s_slot;
  __syncthreads();  // (the next tile of this workgroup rewrites s_slot)
  if (slot < 0) return;
  const int ty = t / d.tiles_x, tx = t - ty * d.tiles_x;
  const int row = ty * JOURNAL_TILE + (threadIdx.x >> 4), col = tx * JOURNAL_TILE + (threadIdx.x & 15);
  if (row < d.H && col < d.W) d.slots[(size_t)slot * 256 + threadIdx.x] = d.tex[(size_t)row * d.W + col];
}

// begin: start = end = head; end: end = head.  One thread.
__global__ void journal_mark_kernel(unsigned long long* counters, int row, int begin) {
  const unsigned long long head = counters[0];
  if (begin) counters[1 + 2 * row] = head;
  counters[2 + 2 * row] = head;
}

// The tiles of a list of tile rectangles, one workgroup per tile in a grid-stride loop over the concatenated rectangles.  Rectangles may
// overlap: the claim sorts it out.
__global__ __launch_bounds__(256) void journal_save_rects_kernel(JDev d, int gen, JRects rs) {
  __shared__ int s_slot;
  long long total = 0;
  for (int q = 0; q < rs.n; ++q) total += (long long)(rs.r[q][2] - rs.r[q][0] + 1) * (rs.r[q][3] - rs.r[q][1] + 1);
  for (long long i = blockIdx.x; i < total; i += gridDim.x) {
    long long k = i;
    int q = 0;
    for (; q < rs.n - 1; ++q) {
      const long long cnt = (long long)(rs.r[q][2] - rs.r[q][0] + 1) * (rs.r[q][3] - rs.r[q][1] + 1);
      if (k < cnt) break;
      k -= cnt;
    }
    const int w = rs.r[q][2] - rs.r[q][0] + 1;
    const int tx = rs.r[q][0] + (int)(k % w), ty = rs.r[q][1] + (int)(k / w);
    save_tile(d, gen, ty * d.tiles_x + tx, &s_slot);
  }
}

// The tiles that meet the device-side texel box bb grown by `grow` and clipped: a grid over all tiles of the texture, and a tile that
// misses the box leaves at once (as mesh_backproject_kernel does); bb empty (x0 > x1): every tile leaves.
__global__ __launch_bounds__(256) void journal_save_box_kernel(JDev d, int gen, const int* __restrict__ bb, int grow) {
  __shared__ int s_slot;
  const int b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
  if (b0 > b2 || b1 > b3) return;  // (uniform)
  const int x0 = max(b0 - grow, 0), y0 = max(b1 - grow, 0), x1 = min(b2 + grow, d.W - 1), y1 = min(b3 + grow, d.H - 1);
  const int col0 = blockIdx.x * JOURNAL_TILE, row0 = blockIdx.y * JOURNAL_TILE;
  if (col0 > x1 || col0 + JOURNAL_TILE - 1 < x0 || row0 > y1 || row0 + JOURNAL_TILE - 1 < y0) return;  // (uniform)
  save_tile(d, gen, blockIdx.y * d.tiles_x + blockIdx.x, &s_slot);
}

// Slots start .. start + n - 1 of the ring against their tiles, one workgroup per slot: texel and slot word change places.  The tiles of
// one record are distinct, so no two workgroups meet.
__global__ __launch_bounds__(256) void journal_swap_kernel(JDev d, unsigned long long start, unsigned int n) {
  for (unsigned int i = blockIdx.x; i < n; i += gridDim.x) {
    const int slot = (int)((start + i) % (unsigned long long)d.capacity);
    const int t = d.slot_tile[slot];
    if (t < 0 || t >= d.n_tiles) continue;  // (uniform; a restorable record's slots all name a tile)
    const int ty = t / d.tiles_x, tx = t - ty * d.tiles_x;
    const int row = ty * JOURNAL_TILE + (threadIdx.x >> 4), col = tx * JOURNAL_TILE + (threadIdx.x & 15);
    if (row >= d.H || col >= d.W) continue;
    unsigned int* a = d.slots + (size_t)slot * 256 + threadIdx.x;
    unsigned int* b = d.tex + (size_t)row * d.W + col;
    const unsigned int va = *a, vb = *b;
    *a = vb; *b = va;
  }
}

// ---------------------------------------------------------------- host
inline int launch_ok() { return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP; }

bool journal_alive(const Journal* j) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_journals.count(const_cast<Journal*>(j)) != 0;
}
// the live journal behind a caller's pointer, or null with the refusal set
Journal* live(const char* who, dtp_journal* p) {
  Journal* j = (Journal*)p;
  if (!j) { dtp_set_error("%s: the journal is NULL", who); return nullptr; }
  if (!journal_alive(j)) { dtp_set_error("%s: not a live journal (destroyed?)", who); return nullptr; }
  return j;
}

void journal_free(Journal* j) {
  if (j->ctx && j->ctx->journal_open == j) j->ctx->journal_open = nullptr;
  (void)hipFree(j->d.slots); (void)hipFree(j->d.tile_gen); (void)hipFree(j->d.slot_tile); (void)hipFree(j->counters);
  if (j->host) (void)hipHostFree(j->host);
  delete j;
}

// clipped texel rectangles -> the save launches, RECTS_PER_LAUNCH rectangles each
int save_rects(Journal* j, const int (*rects)[4], int n, hipStream_t s) {
  const int gen = j->list.recs.back().gen;
  for (int base = 0; base < n; base += RECTS_PER_LAUNCH) {
    JRects rs;
    rs.n = std::min(n - base, RECTS_PER_LAUNCH);
    long long total = 0;
    for (int q = 0; q < rs.n; ++q) {
      journal_tile_rect(rects[base + q], rs.r[q]);
      total += (long long)(rs.r[q][2] - rs.r[q][0] + 1) * (rs.r[q][3] - rs.r[q][1] + 1);
    }
    hipLaunchKernelGGL(journal_save_rects_kernel, dim3((unsigned)std::min<long long>(total, 16384)), dim3(256), 0, s, j->d, gen, rs);
  }
  j->last = s;
  return launch_ok();
}

// the counters, read back on s; waits for s
int read_counters(Journal* j, hipStream_t s) {
  HIP_CHECK(hipMemcpyAsync(j->host, j->counters, N_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return DTP_OK;
}

// undo (dir = -1) and redo (dir = +1): the same swap
int step(const char* who, dtp_journal* p, int dir, hipStream_t s) {
  Journal* j = live(who, p);
  if (!j) return DTP_ERR_ARG;
  const char* what = dir < 0 ? "undo" : "redo";
  if (j->list.open) { dtp_set_error("%s: a record is open (close it with dtp_journal_end first)", who); return DTP_ERR_STATE; }
  const int i = dir < 0 ? j->list.undo_pick() : j->list.redo_pick();
  if (i < 0) { dtp_set_error("%s: nothing to %s", who, what); return DTP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(j->ctx->device));
  RC(read_counters(j, s));
  const int row = j->list.recs[i].row;
  const unsigned long long head = j->host[0], start = j->host[1 + 2 * row], end = j->host[2 + 2 * row];
  if (!journal_restorable(head, start, (uint64_t)j->d.capacity) || end < start || end - start > (unsigned long long)j->d.capacity) {
    dtp_set_error("%s: record %d was overwritten in the ring and cannot be %s: it saved %llu tiles and %llu slots were taken since its begin, "
                  "capacity %d tiles; it and every older record are dropped", who, i, dir < 0 ? "undone" : "redone", end - start, head - start,
                  j->d.capacity);
    j->list.drop_through(i);
    return DTP_ERR_STATE;
  }
  const unsigned long long n = end - start;
  if (n > 0) {
    hipLaunchKernelGGL(journal_swap_kernel, dim3((unsigned)std::min<unsigned long long>(n, 16384)), dim3(256), 0, s, j->d, start, (unsigned int)n);
    RC(launch_ok());
  }
  if (dir < 0) j->list.undo_done(); else j->list.redo_done();
  j->last = s;
  return DTP_OK;
}

}  // namespace

void journal_drop_ctx(Ctx* c) {
  std::vector<Journal*> mine;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    for (Journal* j : g_journals)
      if (j->ctx == c) mine.push_back(j);
    for (Journal* j : mine) g_journals.erase(j);
  }
  for (Journal* j : mine) journal_free(j);
}

Journal* journal_armed(Ctx* c, const void* texture, int H, int W) {
  Journal* j = c->journal_open;
  return j && (const void*)j->d.tex == texture && j->d.H == H && j->d.W == W ? j : nullptr;
}

int journal_save_windows(Journal* j, int R, const int* xs, const int* ys, int k, int wrap, hipStream_t s) {
  int rects[4 * DTP_STAMP_MAXB][4], n = 0;
  for (int b = 0; b < k && b < DTP_STAMP_MAXB; ++b) n += journal_window_rects(j->d.H, j->d.W, R, wrap != 0, xs[b], ys[b], rects + n);
  return n ? save_rects(j, rects, n, s) : DTP_OK;
}

int journal_save_box(Journal* j, const int* bb, int grow, hipStream_t s) {
  hipLaunchKernelGGL(journal_save_box_kernel, dim3(j->d.tiles_x, journal_tiles_x(j->d.H)), dim3(256), 0, s, j->d, j->list.recs.back().gen, bb, grow);
  j->last = s;
  return launch_ok();
}

extern "C" {

int dtp_journal_create(dtp_ctx* ctx, uint8_t* texture, int H, int W, int capacity_tiles, int depth, dtp_journal** out) {
  Ctx* c = (Ctx*)ctx;
  char why[160];
  // ---- the arguments, before the first HIP call
  if (!out) { dtp_set_error("dtp_journal_create: out is NULL"); return DTP_ERR_ARG; }
  if (!journal_check_create(texture, H, W, capacity_tiles, depth, why, sizeof why)) { dtp_set_error("dtp_journal_create: %s", why); return DTP_ERR_ARG; }
  if (!c) { dtp_set_error("dtp_journal_create: ctx is NULL"); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(c->device));
  Journal* j = new Journal();
  j->ctx = c;
  j->list.depth = depth;
  JDev& d = j->d;
  d.tex = (unsigned int*)texture;
  d.H = H; d.W = W; d.tiles_x = journal_tiles_x(W); d.n_tiles = journal_tile_count(H, W); d.capacity = capacity_tiles;
  hipError_t e = hipMalloc((void**)&d.slots, (size_t)capacity_tiles * 1024);
  if (e == hipSuccess) e = hipMalloc((void**)&d.tile_gen, (size_t)d.n_tiles * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&d.slot_tile, (size_t)capacity_tiles * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&j->counters, N_COUNTERS * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipHostMalloc((void**)&j->host, N_COUNTERS * sizeof(unsigned long long), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemset(d.tile_gen, 0, (size_t)d.n_tiles * 4);
  if (e == hipSuccess) e = hipMemset(d.slot_tile, 0xff, (size_t)capacity_tiles * 4);
  if (e == hipSuccess) e = hipMemset(j->counters, 0, N_COUNTERS * sizeof(unsigned long long));
  if (e != hipSuccess) {
    dtp_set_error("dtp_journal_create: %s (%d slots, %d tiles)", hipGetErrorString(e), capacity_tiles, d.n_tiles);
    journal_free(j);
    return DTP_ERR_HIP;
  }
  d.head = j->counters;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    g_journals.insert(j);
  }
  *out = (dtp_journal*)j;
  return DTP_OK;
}

int dtp_journal_destroy(dtp_journal* p) {
  Journal* j = (Journal*)p;
  if (!j) return DTP_OK;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (!g_journals.erase(j)) { dtp_set_error("dtp_journal_destroy: not a live journal"); return DTP_ERR_ARG; }
  }
  (void)hipSetDevice(j->ctx->device);
  journal_free(j);  // (hipFree waits for the work that still reads it)
  return DTP_OK;
}

int dtp_journal_begin(dtp_journal* p, dtp_stream s_) {
  Journal* j = live("dtp_journal_begin", p);
  if (!j) return DTP_ERR_ARG;
  hipStream_t s = (hipStream_t)s_;
  if (j->list.open) { dtp_set_error("dtp_journal_begin: a record is open already"); return DTP_ERR_STATE; }
  if (j->ctx->journal_open) { dtp_set_error("dtp_journal_begin: another journal of this handle has a record open (one at a time)"); return DTP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(j->ctx->device));
  JournalRec r;
  j->list.begin(&r);
  j->ctx->journal_open = j;
  hipLaunchKernelGGL(journal_mark_kernel, dim3(1), dim3(1), 0, s, j->counters, r.row, 1);
  j->last = s;
  return launch_ok();
}

int dtp_journal_end(dtp_journal* p, dtp_stream s_) {
  Journal* j = live("dtp_journal_end", p);
  if (!j) return DTP_ERR_ARG;
  hipStream_t s = (hipStream_t)s_;
  if (!j->list.open) { dtp_set_error("dtp_journal_end: no record is open"); return DTP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(j->ctx->device));
  j->list.end();
  j->ctx->journal_open = nullptr;
  hipLaunchKernelGGL(journal_mark_kernel, dim3(1), dim3(1), 0, s, j->counters, j->list.recs.back().row, 0);
  j->last = s;
  return launch_ok();
}

int dtp_journal_touch(dtp_journal* p, const int* rects, int n, dtp_stream s) {
  char why[160];
  if (!journal_check_rects(rects, n, why, sizeof why)) { dtp_set_error("dtp_journal_touch: %s", why); return DTP_ERR_ARG; }
  Journal* j = live("dtp_journal_touch", p);
  if (!j) return DTP_ERR_ARG;
  if (!j->list.open) { dtp_set_error("dtp_journal_touch: no record is open"); return DTP_ERR_STATE; }
  std::vector<int> clipped;
  for (int i = 0; i < n; ++i) {
    int r[4];
    if (journal_clip_rect(rects + 4 * (size_t)i, j->d.H, j->d.W, r)) clipped.insert(clipped.end(), r, r + 4);
  }
  if (clipped.empty()) return DTP_OK;
  HIP_CHECK(hipSetDevice(j->ctx->device));
  return save_rects(j, (const int(*)[4])clipped.data(), (int)(clipped.size() / 4), (hipStream_t)s);
}

int dtp_journal_undo(dtp_journal* j, dtp_stream s) { return step("dtp_journal_undo", j, -1, (hipStream_t)s); }
int dtp_journal_redo(dtp_journal* j, dtp_stream s) { return step("dtp_journal_redo", j, +1, (hipStream_t)s); }

int dtp_journal_info(dtp_journal* p, int* records, int* cursor, int* open, uint64_t* head) {
  Journal* j = live("dtp_journal_info", p);
  if (!j) return DTP_ERR_ARG;
  if (head) {
    HIP_CHECK(hipSetDevice(j->ctx->device));
    RC(read_counters(j, j->last));
    *head = j->host[0];
  }
  if (records) *records = (int)j->list.recs.size();
  if (cursor) *cursor = j->list.cursor;
  if (open) *open = j->list.open ? 1 : 0;
  return DTP_OK;
}

int dtp_journal_record_info(dtp_journal* p, int record, uint64_t* start, uint64_t* end, int* restorable) {
  Journal* j = live("dtp_journal_record_info", p);
  if (!j) return DTP_ERR_ARG;
  const int n = (int)j->list.recs.size();
  if (record < 0 || record >= n) { dtp_set_error("dtp_journal_record_info: record %d outside 0..%d", record, n - 1); return DTP_ERR_ARG; }
  HIP_CHECK(hipSetDevice(j->ctx->device));
  RC(read_counters(j, j->last));
  const int row = j->list.recs[record].row;
  const bool is_open = j->list.open && record == n - 1;
  const unsigned long long head = j->host[0], a = j->host[1 + 2 * row], b = is_open ? head : j->host[2 + 2 * row];
  if (start) *start = a;
  if (end) *end = b;
  if (restorable) *restorable = journal_restorable(head, a, (uint64_t)j->d.capacity) ? 1 : 0;
  return DTP_OK;
}

int dtp_op_journal_tiles(dtp_journal* p, int record, int* tiles_host, int max, int* n_out) {
  Journal* j = live("dtp_op_journal_tiles", p);
  if (!j) return DTP_ERR_ARG;
  if (!n_out || max < 0 || (max > 0 && !tiles_host)) { dtp_set_error("dtp_op_journal_tiles: NULL argument (n is required; tiles_host with max > 0)"); return DTP_ERR_ARG; }
  uint64_t a = 0, b = 0;
  int ok = 0;
  RC(dtp_journal_record_info(p, record, &a, &b, &ok));
  if (!ok) { dtp_set_error("dtp_op_journal_tiles: record %d was overwritten in the ring (%llu tiles, capacity %d)", record, (unsigned long long)(b - a), j->d.capacity); return DTP_ERR_STATE; }
  const uint64_t n = b - a, cap = (uint64_t)j->d.capacity;
  *n_out = (int)n;
  if (n > (uint64_t)max) { dtp_set_error("dtp_op_journal_tiles: record %d saved %d tiles, room for %d", record, (int)n, max); return DTP_ERR_ARG; }
  const uint64_t at = a % cap, first = std::min(n, cap - at);  // (the stream was waited for: plain copies)
  if (first) HIP_CHECK(hipMemcpy(tiles_host, j->d.slot_tile + at, first * 4, hipMemcpyDeviceToHost));
  if (n > first) HIP_CHECK(hipMemcpy(tiles_host + first, j->d.slot_tile, (n - first) * 4, hipMemcpyDeviceToHost));
  return DTP_OK;
}

int dtp_journal_window_tiles(int H, int W, int R, int wrap, int x, int y, int* tiles, int max, int* n) {
  if (!n || max < 0 || (max > 0 && !tiles)) { dtp_set_error("dtp_journal_window_tiles: NULL argument (n is required; tiles with max > 0)"); return DTP_ERR_ARG; }
  if (H < 1 || W < 1 || H > JOURNAL_MAX_TEX || W > JOURNAL_MAX_TEX) { dtp_set_error("dtp_journal_window_tiles: a %d x %d texture (each side 1..%d)", H, W, JOURNAL_MAX_TEX); return DTP_ERR_ARG; }
  if (R < 1 || R > H || R > W) { dtp_set_error("dtp_journal_window_tiles: R=%d outside 1..min(H, W)=%d", R, std::min(H, W)); return DTP_ERR_ARG; }
  const std::vector<int> t = journal_window_tiles(H, W, R, wrap != 0, x, y);
  *n = (int)t.size();
  if ((int)t.size() > max) { dtp_set_error("dtp_journal_window_tiles: %d tiles, room for %d", (int)t.size(), max); return DTP_ERR_ARG; }
  if (!t.empty()) memcpy(tiles, t.data(), t.size() * sizeof(int));
  return DTP_OK;
}

}  // extern "C"
