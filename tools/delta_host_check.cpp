// Stand-alone host check of csrc/delta_host.h for a sanitizer build: everything of the changed-tile tracker that needs no device -- the
// argument checks, the layout, the set of live trackers, and the CPU scan (the kernels' three passes with their grouping) against a
// tile-by-tile restatement written here: key frames, single bytes, random tile sets, capped scans that continue, change and change
// back -- driven from its own main().  Plain C++, no HIP.
// Build and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \
//       tools/delta_host_check.cpp -o delta_host_check
//   ./delta_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "delta_host.h"

static int g_checks = 0;
static char g_why[200];
#define EXPECT(cond)                                                                                          \
  do {                                                                                                        \
    ++g_checks;                                                                                               \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_why); return 1; } \
  } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// a tracker's state in exactly-sized heap blocks, so that the sanitizer sees every byte past an end
struct State {
  int H, W, cap, n;
  std::vector<uint8_t> image, shadow, stale, tiles;
  std::vector<int> ids;
  int counts[2];
  State(int H_, int W_, int cap_) : H(H_), W(W_), cap(cap_), n(journal_tile_count(H_, W_)), image((size_t)H_ * W_ * 4), shadow((size_t)H_ * W_ * 4, 0),
                                     stale((size_t)n, 1), tiles((size_t)cap_ * DELTA_TILE_BYTES, 0xEE), ids((size_t)cap_, -7) {
    counts[0] = counts[1] = -1;
    for (auto& b : image) b = (uint8_t)rnd();
  }
  void scan() { delta_scan_host(image.data(), shadow.data(), stale.data(), H, W, cap, ids.data(), tiles.data(), counts); }
  // one byte of texel (r, c) takes another value
  void poke(int r, int c, int ch) { image[((size_t)r * W + c) * 4 + ch] ^= 0x5A; }
};

// the changed tiles, texel by texel, before a scan
static std::vector<int> brute_changed(const State& s) {
  std::vector<char> hit((size_t)s.n, 0);
  for (int t = 0; t < s.n; ++t) hit[t] = s.stale[t] != 0;
  for (int r = 0; r < s.H; ++r)
    for (int c = 0; c < s.W; ++c)
      if (memcmp(&s.image[((size_t)r * s.W + c) * 4], &s.shadow[((size_t)r * s.W + c) * 4], 4) != 0)
        hit[(size_t)(r / 16) * journal_tiles_x(s.W) + (size_t)(c / 16)] = 1;
  std::vector<int> out;
  for (int t = 0; t < s.n; ++t)
    if (hit[t]) out.push_back(t);
  return out;
}

// one scan against the restatement: ids, payloads (zero outside the image), counts, the shadow and the stale marks afterwards, and
// the slots past `emitted` untouched.  0: all held.
static int check_scan(State& s) {
  const std::vector<int> want = brute_changed(s);
  const State before = s;
  s.scan();
  const int emitted = std::min((int)want.size(), s.cap);
  snprintf(g_why, sizeof g_why, "%d x %d, capacity %d, %d changed", s.H, s.W, s.cap, (int)want.size());
  EXPECT(s.counts[0] == emitted && s.counts[1] == (int)want.size() - emitted);
  const int tw = journal_tiles_x(s.W);
  std::vector<char> sent((size_t)s.n, 0);
  for (int k = 0; k < emitted; ++k) {
    const int t = want[k];
    EXPECT(s.ids[k] == t);
    sent[t] = 1;
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        const int r = (t / tw) * 16 + i, c = (t % tw) * 16 + j;
        const uint8_t* got = &s.tiles[(size_t)k * 1024 + ((size_t)i * 16 + j) * 4];
        static const uint8_t zero[4] = {0, 0, 0, 0};
        EXPECT(memcmp(got, r < s.H && c < s.W ? &s.image[((size_t)r * s.W + c) * 4] : zero, 4) == 0);
      }
  }
  for (int k = emitted; k < s.cap; ++k) {
    EXPECT(s.ids[k] == before.ids[k]);
    EXPECT(memcmp(&s.tiles[(size_t)k * 1024], &before.tiles[(size_t)k * 1024], 1024) == 0);
  }
  for (int r = 0; r < s.H; ++r)
    for (int c = 0; c < s.W; ++c) {
      const int t = (r / 16) * tw + c / 16;
      const size_t at = ((size_t)r * s.W + c) * 4;
      EXPECT(memcmp(&s.shadow[at], sent[t] ? &s.image[at] : &before.shadow[at], 4) == 0);
    }
  for (int t = 0; t < s.n; ++t) EXPECT(s.stale[t] == (sent[t] ? 0 : before.stale[t]));
  EXPECT(s.image == before.image);
  return 0;
}

int main() {
  // ---- argument checks
  alignas(16) static unsigned char img[64];
  int a = 0, b = 0;
  EXPECT(delta_check_create(1, 1, 1, g_why, sizeof g_why));
  EXPECT(delta_check_create(16384, 16384, 1 << 20, g_why, sizeof g_why));
  EXPECT(!delta_check_create(0, 150, 1, g_why, sizeof g_why) && strstr(g_why, "0 x 150"));
  EXPECT(!delta_check_create(90, 16385, 1, g_why, sizeof g_why) && strstr(g_why, "16385"));
  EXPECT(!delta_check_create(-3, 150, 1, g_why, sizeof g_why) && strstr(g_why, "-3 x 150"));
  EXPECT(!delta_check_create(90, 150, 0, g_why, sizeof g_why) && strstr(g_why, "capacity_tiles=0"));
  EXPECT(!delta_check_create(90, 150, -4, g_why, sizeof g_why) && strstr(g_why, "capacity_tiles=-4"));
  EXPECT(delta_check_image(img, 90, 150, 90, 150, g_why, sizeof g_why));
  EXPECT(delta_check_image(img + 4, 90, 150, 90, 150, g_why, sizeof g_why));
  EXPECT(!delta_check_image(nullptr, 90, 150, 90, 150, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!delta_check_image(img, 90, 151, 90, 150, g_why, sizeof g_why) && strstr(g_why, "90 x 151") && strstr(g_why, "90 x 150"));
  EXPECT(!delta_check_image(img, 150, 90, 90, 150, g_why, sizeof g_why) && strstr(g_why, "created for"));
  EXPECT(!delta_check_image(img, 0, 150, 90, 150, g_why, sizeof g_why) && strstr(g_why, "0 x 150"));
  EXPECT(!delta_check_image(img + 1, 90, 150, 90, 150, g_why, sizeof g_why) && strstr(g_why, "aligned"));
  EXPECT(!delta_check_image(img + 2, 90, 150, 90, 150, g_why, sizeof g_why) && strstr(g_why, "aligned"));
  EXPECT(delta_check_pull(img, img, &a, &b, 8, 8, g_why, sizeof g_why) && delta_check_pull(img, img, &a, &b, 9, 8, g_why, sizeof g_why));
  EXPECT(!delta_check_pull(img, img, &a, &b, 7, 8, g_why, sizeof g_why) && strstr(g_why, "max_tiles=7") && strstr(g_why, "8 tiles"));
  EXPECT(!delta_check_pull(nullptr, img, &a, &b, 8, 8, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!delta_check_pull(img, nullptr, &a, &b, 8, 8, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!delta_check_pull(img, img, nullptr, &b, 8, 8, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!delta_check_pull(img, img, &a, nullptr, 8, 8, g_why, sizeof g_why) && strstr(g_why, "NULL"));

  // ---- the layout
  dtp_delta_sizes L;
  memset(&L, 0x77, sizeof L);
  const dtp_delta_sizes untouched = L;
  EXPECT(!delta_layout(90, 150, 5, nullptr, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!delta_layout(90, 0, 5, &L, g_why, sizeof g_why) && memcmp(&L, &untouched, sizeof L) == 0);
  EXPECT(!delta_layout(90, 150, 0, &L, g_why, sizeof g_why) && memcmp(&L, &untouched, sizeof L) == 0);
  EXPECT(delta_layout(90, 150, 5, &L, g_why, sizeof g_why));
  EXPECT(L.tiles_x == 10 && L.tiles_y == 6 && L.n_tiles == 60 && L.n_groups == 1 && L.capacity == 5);
  EXPECT(L.shadow_bytes == 90u * 150u * 4u && L.stale_bytes == 60 && L.flag_bytes == 60 && L.group_bytes == 8 && L.ids_bytes == 20);
  EXPECT(L.tiles_bytes == 5 * 1024 && L.counts_bytes == 8 && L.host_ids_offset == 16 && L.host_tiles_offset == 48 && L.host_bytes == 48 + 5 * 1024);
  EXPECT(delta_layout(1, 1, 1, &L, g_why, sizeof g_why) && L.n_tiles == 1 && L.n_groups == 1 && L.shadow_bytes == 4 && L.host_bytes == 32 + 1024);
  EXPECT(delta_layout(2048, 2064, 16512, &L, g_why, sizeof g_why) && L.n_tiles == 128 * 129 && L.n_groups == 258);
  EXPECT(delta_layout(16384, 16384, 1 << 20, &L, g_why, sizeof g_why));
  EXPECT(L.n_tiles == 1 << 20 && L.n_groups == 1 << 14 && L.shadow_bytes == (uint64_t)1 << 30 && L.tiles_bytes == (uint64_t)1 << 30);
  EXPECT(L.host_bytes == 16 + ((uint64_t)4 << 20) + ((uint64_t)1 << 30));
  EXPECT(delta_groups(64) == 1 && delta_groups(65) == 2 && delta_groups(1) == 1);

  // ---- the live set
  {
    DeltaLive live;
    int t1, t2, t3, c1, c2;
    unsigned char junk[64];
    memset(junk, 0xAB, sizeof junk);
    EXPECT(live.owner(&t1) == nullptr && live.owner(junk) == nullptr && live.owner(nullptr) == nullptr && !live.remove(&t1));
    live.add(&t1, &c1); live.add(&t2, &c1); live.add(&t3, &c2);
    EXPECT(live.size() == 3 && live.owner(&t1) == &c1 && live.owner(&t2) == &c1 && live.owner(&t3) == &c2 && live.owner(junk) == nullptr);
    EXPECT(live.remove(&t1) && !live.remove(&t1) && live.owner(&t1) == nullptr && live.size() == 2);
    const std::vector<const void*> mine = live.take_owner(&c1);
    EXPECT(mine.size() == 1 && mine[0] == &t2 && live.size() == 1 && live.owner(&t2) == nullptr && live.owner(&t3) == &c2);
    EXPECT(live.take_owner(&c1).empty() && live.take_owner(&c2).size() == 1 && live.size() == 0);
  }

  // ---- the scan
  const int sizes[][2] = {{1, 1}, {16, 16}, {17, 33}, {90, 150}, {96, 160}, {130, 1040}};  // the last: 9 x 65 = 585 tiles, 10 groups
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1], n = journal_tile_count(H, W);
    State s(H, W, n);
    // a key frame, then nothing
    if (check_scan(s)) return 1;
    EXPECT(s.counts[0] == n && s.counts[1] == 0 && s.shadow == s.image);
    if (check_scan(s)) return 1;
    EXPECT(s.counts[0] == 0 && s.counts[1] == 0);
    // single bytes: red of (0, 0), alpha only, the image's last texel
    s.poke(0, 0, 0);
    if (check_scan(s)) return 1;
    EXPECT(s.counts[0] == 1 && s.ids[0] == 0);
    s.poke(H / 2, W / 2, 3);
    if (check_scan(s)) return 1;
    EXPECT(s.counts[0] == 1 && s.ids[0] == (H / 2 / 16) * journal_tiles_x(W) + W / 2 / 16);
    s.poke(H - 1, W - 1, 2);
    if (check_scan(s)) return 1;
    EXPECT(s.counts[0] == 1 && s.ids[0] == n - 1);
    // changed and changed back: nothing
    s.poke(H - 1, 0, 1); s.poke(H - 1, 0, 1);
    if (check_scan(s)) return 1;
    EXPECT(s.counts[0] == 0);
    // random sets: about 1 %, half, all
    for (int pct : {1, 50, 100}) {
      for (int t = 0; t < n; ++t)
        if ((int)(rnd() % 100) < pct) {
          const int r0 = (t / journal_tiles_x(W)) * 16, c0 = (t % journal_tiles_x(W)) * 16;
          s.poke(r0 + (int)(rnd() % (unsigned)std::min(16, H - r0)), c0 + (int)(rnd() % (unsigned)std::min(16, W - c0)), (int)(rnd() % 4));
        }
      if (check_scan(s)) return 1;
    }
    // capped: capacity 7 and 1 from a fresh tracker; the scans continue in order until nothing remains
    for (int cap : {7, 1}) {
      if (cap == 1 && n > 100) continue;  // (a tile per scan: the small sizes say it all)
      State c(H, W, cap);
      int left = n, rounds = 0;
      while (true) {
        if (check_scan(c)) return 1;
        left -= c.counts[0];
        EXPECT(c.counts[1] == left);
        ++rounds;
        if (c.counts[1] == 0) break;
        if (rounds == 2) c.poke(0, 0, 0);  // tile 0 was emitted already: it comes again
        if (rounds == 2) ++left;
        EXPECT(rounds < 2 * n + 4);
      }
      EXPECT(c.shadow == c.image);
      // reset: everything again
      std::fill(c.stale.begin(), c.stale.end(), 1);
      if (check_scan(c)) return 1;
      EXPECT(c.counts[0] == std::min(cap, n) && c.counts[1] == n - std::min(cap, n));
    }
  }
  printf("delta_host_check: %d checks passed\n", g_checks);
  return 0;
}
