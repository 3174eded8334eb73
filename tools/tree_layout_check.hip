// Host-only check of the combine tree's workspace layout (gram.hpp) over a grid of shapes, for
// the counter stride the build sets:
//   hipcc -std=c++17 -I include -I cc-mpc_amd/csrc [-DCCMPC_CTR_STRIDE=64] \
//         tools/tree_layout_check.hip -o tools/tree_layout_check && tools/tree_layout_check
// For every (items, cells, slab size): the size function's answer lays out; the counters fit the
// counter region and the slabs what is left; levels do not overlap; and a larger shared buffer
// (another shape's, or a grown one) lays out as well.  (A buffer shorter than the size function's
// answer is refused by the entry points themselves, before tree_layout is asked.)
#include <cstdio>
#include <vector>

#include "gram.hpp"

using namespace ccmpc;

static long bad = 0;
#define EXPECT(c)                                                                   \
  do {                                                                              \
    if (!(c) && bad++ < 20) std::printf("FAILED %s (items %lld cells %lld E %d)\n", #c, \
                                        (long long)items, (long long)cells, E);     \
  } while (0)

int main() {
  const int Es[] = {176, 260, 272, 800, 1648, 3904};
  const int64_t item_counts[] = {1, 2, 9, 16, 17, 79, 88, 256, 257, 4097, 65537, 1 << 20};
  const int64_t cell_counts[] = {1, 2, 9, 67, 512, 4096, 100000};
  long n = 0;
  std::vector<size_t> sizes;
  for (int E : Es)
    for (int64_t cells : cell_counts)
      for (int64_t extra : item_counts) {
        const int64_t items = extra + cells;  // max_items: at least one per cell
        const size_t c = tree_counter_bytes(items, cells), s = tree_slab_bytes(items, cells, E);
        const size_t ws = tree_bytes(items, cells, E);
        sizes.push_back(ws);
        EXPECT(ws % kCounterAlign == 0);
        EXPECT(ctr_region(ws) >= c);
        EXPECT(ws - ctr_region(ws) >= s);
        TreeLayout L;
        char *base = reinterpret_cast<char *>(uintptr_t(1) << 20);  // never dereferenced
        EXPECT(tree_layout(base, ws, items, cells, E, L));
        for (int l = 0; l < kMaxLevels; ++l) {
          const char *c0 = reinterpret_cast<char *>(L.counters[l]);
          const char *c1 = c0 + level_capacity(items, cells, l + 1) * kCounterStride * 4;
          EXPECT(c0 >= base && c1 <= base + ctr_region(ws));
          if (l + 1 < kMaxLevels) EXPECT(c1 <= reinterpret_cast<char *>(L.counters[l + 1]));
          const char *s0 = reinterpret_cast<char *>(L.slabs[l]);
          const char *s1 = s0 + level_capacity(items, cells, l) * E * 8;
          EXPECT(s0 >= base + ctr_region(ws) && s1 <= base + ws);
          if (l + 1 < kMaxLevels) EXPECT(s1 <= reinterpret_cast<char *>(L.slabs[l + 1]));
        }
        ++n;
      }
  // every shape on every buffer at least as large as its own (a grow-only workspace: + 4096)
  size_t k = 0;
  for (int E : Es)
    for (int64_t cells : cell_counts)
      for (int64_t extra : item_counts) {
        const int64_t items = extra + cells;
        const size_t own = sizes[k++];
        for (size_t other : sizes) {
          TreeLayout L;
          if (other + 4096 >= own)
            EXPECT(tree_layout(reinterpret_cast<void *>(uintptr_t(1) << 20), other + 4096, items,
                               cells, E, L));
        }
      }
  std::printf("stride %d words, counter region 1/%zu of the buffer: %ld shapes, %ld failures\n",
              kCounterStride, kCtrShare, n, bad);
  return bad ? 1 : 0;
}
