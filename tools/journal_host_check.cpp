// Stand-alone host check of csrc/journal_host.h for a sanitizer build: everything of the undo / redo journal that needs no device -- the
// argument checks, rectangle clipping, the pieces of a wrapped window, window -> tiles against a texel-by-texel count, the record list
// with cursor, depth eviction and row reuse, and the ring's restorability rule -- driven from its own main().  Plain C++, no HIP.
// Build and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I diffusiontexturepainting_amd/csrc \
//       tools/journal_host_check.cpp -o journal_host_check
//   ./journal_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <vector>

#include "journal_host.h"

static int g_checks = 0;
static char g_why[200];
#define EXPECT(cond)                                                                                          \
  do {                                                                                                        \
    ++g_checks;                                                                                               \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_why); return 1; } \
  } while (0)

// the tiles of a window, texel by texel
static std::vector<int> brute(int H, int W, int R, bool wrap, int x, int y) {
  std::vector<char> hit((size_t)journal_tile_count(H, W), 0);
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < R; ++c) {
      long long ty = (long long)y + r, tx = (long long)x + c;
      if (wrap) { ty = ((ty % H) + H) % H; tx = ((tx % W) + W) % W; }
      else if (ty < 0 || ty >= H || tx < 0 || tx >= W) continue;
      hit[(size_t)(ty / 16) * journal_tiles_x(W) + (size_t)(tx / 16)] = 1;
    }
  std::vector<int> t;
  for (size_t i = 0; i < hit.size(); ++i)
    if (hit[i]) t.push_back((int)i);
  return t;
}

int main() {
  // ---- argument checks
  alignas(16) static unsigned char tex[64];
  EXPECT(journal_check_create(tex, 90, 150, 1, 1, g_why, sizeof g_why));
  EXPECT(journal_check_create(tex, 32768, 32768, 1 << 30, 64, g_why, sizeof g_why));
  EXPECT(!journal_check_create(nullptr, 90, 150, 1, 1, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!journal_check_create(tex, 0, 150, 1, 1, g_why, sizeof g_why) && strstr(g_why, "0 x 150"));
  EXPECT(!journal_check_create(tex, 90, 32769, 1, 1, g_why, sizeof g_why) && strstr(g_why, "32769"));
  EXPECT(!journal_check_create(tex + 2, 90, 150, 1, 1, g_why, sizeof g_why) && strstr(g_why, "aligned"));
  EXPECT(!journal_check_create(tex, 90, 150, 0, 1, g_why, sizeof g_why) && strstr(g_why, "capacity_tiles=0"));
  EXPECT(!journal_check_create(tex, 90, 150, 1, 0, g_why, sizeof g_why) && strstr(g_why, "depth=0"));
  EXPECT(!journal_check_create(tex, 90, 150, 1, 65, g_why, sizeof g_why) && strstr(g_why, "depth=65"));
  const int good[8] = {0, 0, 5, 5, 7, 7, 7, 7}, bad_x[8] = {0, 0, 5, 5, 9, 0, 8, 0}, bad_y[4] = {0, 3, 0, 2};
  EXPECT(journal_check_rects(good, 2, g_why, sizeof g_why));
  EXPECT(!journal_check_rects(nullptr, 2, g_why, sizeof g_why) && strstr(g_why, "NULL"));
  EXPECT(!journal_check_rects(good, 0, g_why, sizeof g_why) && strstr(g_why, "n=0"));
  EXPECT(!journal_check_rects(bad_x, 2, g_why, sizeof g_why) && strstr(g_why, "rectangle 1"));
  EXPECT(!journal_check_rects(bad_y, 1, g_why, sizeof g_why) && strstr(g_why, "rectangle 0"));
  g_why[0] = 0;

  // ---- clipping and tiles
  int out[4];
  const int r0[4] = {-7, -3, 11, 200}, r1[4] = {150, 0, 160, 5}, r2[4] = {0, -9, 5, -1};
  EXPECT(journal_clip_rect(r0, 90, 150, out) && out[0] == 0 && out[1] == 0 && out[2] == 11 && out[3] == 89);
  EXPECT(!journal_clip_rect(r1, 90, 150, out));
  EXPECT(!journal_clip_rect(r2, 90, 150, out));
  EXPECT(journal_tiles_x(150) == 10 && journal_tile_count(90, 150) == 60 && journal_tile_count(32768, 32768) == 2048 * 2048);
  EXPECT(journal_tile_count(1, 1) == 1 && journal_tile_count(16, 17) == 2);

  // ---- window -> tiles against the texel count
  const int sizes[][3] = {{96, 160, 64}, {90, 150, 64}, {64, 64, 64}, {64, 72, 64}, {72, 64, 64}, {90, 150, 1}, {17, 17, 16}, {33, 40, 24}};
  const int at[] = {-200, -65, -64, -63, -17, -16, -1, 0, 1, 7, 8, 15, 16, 17, 31, 40, 63, 64, 86, 89, 90, 95, 96, 149, 150, 159, 160, 161, 1000};
  for (const auto& sz : sizes)
    for (int wrap = 0; wrap < 2; ++wrap)
      for (int x : at)
        for (int y : at) {
          const std::vector<int> got = journal_window_tiles(sz[0], sz[1], sz[2], wrap != 0, x, y);
          snprintf(g_why, sizeof g_why, "H=%d W=%d R=%d wrap=%d x=%d y=%d", sz[0], sz[1], sz[2], wrap, x, y);
          EXPECT(got == brute(sz[0], sz[1], sz[2], wrap != 0, x, y));
          int rects[4][4];
          const int n = journal_window_rects(sz[0], sz[1], sz[2], wrap != 0, x, y, rects);
          EXPECT(n >= 0 && n <= 4 && (wrap ? n >= 1 : n <= 1));
          long long texels = 0;  // the pieces are disjoint and hold the window's texels inside the texture
          for (int i = 0; i < n; ++i) {
            EXPECT(rects[i][0] >= 0 && rects[i][1] >= 0 && rects[i][2] < sz[1] && rects[i][3] < sz[0] && rects[i][0] <= rects[i][2] && rects[i][1] <= rects[i][3]);
            texels += (long long)(rects[i][2] - rects[i][0] + 1) * (rects[i][3] - rects[i][1] + 1);
          }
          if (wrap) EXPECT(texels == (long long)sz[2] * sz[2]);
        }
  g_why[0] = 0;
  // W = R + 8 with wrap: the two pieces of a window that starts inside tile column 0 share it
  {
    int rects[4][4];
    EXPECT(journal_window_rects(64, 72, 64, true, 16, 0, rects) == 2);
    int a[4], b[4];
    journal_tile_rect(rects[0], a); journal_tile_rect(rects[1], b);
    EXPECT(a[0] == 1 && a[2] == 4 && b[0] == 0 && b[2] == 0);
    EXPECT(journal_window_rects(64, 72, 64, true, 12, 0, rects) == 2);
    journal_tile_rect(rects[0], a); journal_tile_rect(rects[1], b);
    EXPECT(a[0] == 0 && b[0] == 0 && b[2] == 0);  // column 12 .. 71 and 0 .. 3: tile column 0 twice
    EXPECT(journal_window_tiles(64, 72, 64, true, 12, 0).size() == 20);
  }
  // a huge texture: the largest window's tile list
  EXPECT(journal_window_tiles(32768, 32768, 4096, false, 32768 - 4096, 32768 - 4096).size() == 256u * 256u);
  EXPECT(journal_window_tiles(32768, 32768, 4096, true, 2147483647, -2147483647 - 1).size() > 0);

  // ---- the ring
  EXPECT(journal_restorable(0, 0, 1) && journal_restorable(5, 0, 5) && !journal_restorable(6, 0, 5));
  EXPECT(journal_restorable((1ull << 40) + 7, 1ull << 40, 7) && !journal_restorable((1ull << 40) + 8, 1ull << 40, 7));

  // ---- the records
  {
    JournalList l;
    l.depth = 3;
    JournalRec r;
    EXPECT(l.undo_pick() == -1 && l.redo_pick() == -1 && !l.end());
    EXPECT(l.begin(&r) && r.row == 0 && r.gen == 1 && l.open && !l.begin(&r));
    EXPECT(l.undo_pick() == 0);
    EXPECT(l.end() && !l.end());
    EXPECT(l.begin(&r) && r.row == 1 && r.gen == 2 && l.end());
    EXPECT(l.begin(&r) && r.row == 2 && r.gen == 3 && l.end());
    EXPECT(l.recs.size() == 3 && l.cursor == 3);
    EXPECT(l.begin(&r) && r.row == 0 && r.gen == 4 && l.end());  // depth: the oldest went and its row is taken again
    EXPECT(l.recs.size() == 3 && l.recs[0].gen == 2 && l.cursor == 3);
    EXPECT(l.undo_pick() == 2); l.undo_done();
    EXPECT(l.undo_pick() == 1); l.undo_done();
    EXPECT(l.redo_pick() == 1 && l.cursor == 1);
    l.redo_done();
    EXPECT(l.redo_pick() == 2 && l.undo_pick() == 1);
    EXPECT(l.begin(&r) && l.end());  // the undone record (gen 4, row 0) goes; its row is free for the new one
    EXPECT(l.recs.size() == 3 && r.row == 0 && r.gen == 5 && l.redo_pick() == -1 && l.cursor == 3);
    l.undo_done();
    l.drop_through(0);  // record 0 was overwritten
    EXPECT(l.recs.size() == 2 && l.cursor == 1 && l.recs[0].gen == 3);
    l.drop_through(1);
    EXPECT(l.recs.empty() && l.cursor == 0 && l.rows_used == 0);
    std::set<int> gens;
    JournalList m;
    m.depth = JOURNAL_MAX_DEPTH;
    for (int i = 0; i < 300; ++i) {
      EXPECT(m.begin(&r) && m.end() && r.row >= 0 && r.row < JOURNAL_MAX_DEPTH && r.gen > 0 && gens.insert(r.gen).second);
      std::set<int> rows;
      for (const JournalRec& q : m.recs) EXPECT(rows.insert(q.row).second);
      if (i % 7 == 3 && m.undo_pick() >= 0) m.undo_done();
    }
    EXPECT((int)m.recs.size() <= JOURNAL_MAX_DEPTH);
    m.next_gen = 0x7fffffff;
    EXPECT(m.begin(&r) && r.gen == 0x7fffffff && m.end() && m.begin(&r) && r.gen == 1);
  }
  printf("journal_host_check: %d checks passed\n", g_checks);
  return 0;
}
