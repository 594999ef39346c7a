// TEST INFRASTRUCTURE: the integer rules of the contraction kernel (renormalizer_amd/csrc/mpse_gemm_tiles.h) behind a C
// interface, composed in the order k_gemm composes them (tests/test_gemm_tiles_host.py).  Never linked into
// libmpsengine.so.
#include <cstddef>
#include <vector>

#include "../../renormalizer_amd/csrc/mpse_gemm_tiles.h"

using namespace mpse_tiles;

namespace {
// what the rules read of the launch arguments (GemmArgs of mpse_gemm.hip)
struct Launch {
  int tiles_m, tiles_n, ksplit, slice_fast, die_group, skew;
  const int* perm;
  struct {
    int split2, cpd, tiles_m_grp;
  } gg;
};
}  // namespace

// Walks launch positions 0 .. nwg - 1 as the kernel does - launch_position, the launch order, the dead mark, tile_coords,
// the group of the tile row - and checks that they reach every (batch x K slice or half, group's tile row, tile column)
// exactly once.
// in: tiles_m, tiles_n, batch, ksplit, slice_fast, die_group, skew, grouped, split2, cpd, tiles_m_grp
// perm: launch order (entries tile or ~tile), or null.  Returns 0, or the line of the check that failed; *dead_out
// receives the number of positions marked dead.
extern "C" int emu_positions_cover(const long long* in, const int* perm, long long nwg, long long* dead_out) {
  Launch g{(int)in[0], (int)in[1], (int)in[3], (int)in[4], (int)in[5], (int)in[6], perm, {(int)in[8], (int)in[9], (int)in[10]}};
  const int batch = (int)in[2];
  const bool grouped = in[7] != 0;
  const int ntile = g.tiles_m * g.tiles_n;
  const int rows = grouped && g.gg.split2 ? 2 : batch * g.ksplit;
  if (nwg != (long long)rows * ntile) return __LINE__;
  std::vector<char> seen((size_t)nwg, 0);
  long long ndead = 0;
  for (int bid = 0; bid < (int)nwg; ++bid) {
    int bs, t, half;
    launch_position(g, grouped, bid, ntile, bs, t, half);
    if (bs < 0 || bs >= rows || t < 0 || t >= ntile || half < 0 || half > 1) return __LINE__;
    if (grouped && g.gg.split2 ? bs != half : half != 0) return __LINE__;
    const int b = bs / g.ksplit, ks_id = bs - b * g.ksplit;
    if (!(grouped && g.gg.split2) && b >= batch) return __LINE__;   // (halved launches: bs is the half, no batch)
    bool dead = false;
    if (g.perm) {
      t = g.perm[order_index(t, ks_id, ntile)];
      if (grouped) order_decode(t, t, dead);
    }
    if (t < 0 || t >= ntile) return __LINE__;
    ndead += dead;
    int tm, tn;
    tile_coords(g, t, tm, tn);
    if (tm < 0 || tm >= g.tiles_m || tn < 0 || tn >= g.tiles_n) return __LINE__;
    if (grouped) {
      const int grp = group_of_row(tm, g.gg.tiles_m_grp), tml = tm - grp * g.gg.tiles_m_grp;
      if (grp < 0 || grp * g.gg.tiles_m_grp >= g.tiles_m || tml < 0 || tml >= g.gg.tiles_m_grp) return __LINE__;
    }
    const size_t key = ((size_t)bs * g.tiles_m + tm) * g.tiles_n + tn;
    if (seen[key]) return __LINE__;
    seen[key] = 1;
  }
  if (dead_out) *dead_out = ndead;
  return 0;
}

// launch_position alone: (bs, t, half) of every position, 3 ints each
extern "C" void emu_launch_positions(const long long* in, long long nwg, int* out) {
  Launch g{(int)in[0], (int)in[1], (int)in[3], (int)in[4], (int)in[5], (int)in[6], nullptr, {(int)in[8], (int)in[9], (int)in[10]}};
  for (int bid = 0; bid < (int)nwg; ++bid)
    launch_position(g, in[7] != 0, bid, g.tiles_m * g.tiles_n, out[3 * bid], out[3 * bid + 1], out[3 * bid + 2]);
}

// The K tiles the K loop visits in [kt_begin, kt_end): next_flagged from kt_begin, then from one past each tile found,
// on the flag words of both operands (b may be null) combined as the kernel combines them.  Returns their number.
extern "C" int emu_flag_walk(const unsigned long long* a, const unsigned long long* b, int kt_begin, int kt_end, int* out) {
  auto word_at = [&](int w) {
    unsigned long long word = FLAGS_ALL;
    word &= a[w];
    if (b) word &= b[w];
    return word;
  };
  int n = 0;
  for (int kt = next_flagged(kt_begin, kt_end, word_at); kt < kt_end; kt = next_flagged(kt + 1, kt_end, word_at)) out[n++] = kt;
  return n;
}

// The K range of one half of a halved tile, composed as in the kernel: count, FlaggedPos, the two ranges
extern "C" void emu_half_range(const unsigned long long* words, int nkw, int nkt, int half, int* kt_begin, int* kt_end) {
  auto word_at = [&](int w) { return trim_flags(words[w], w, nkt); };
  int n = 0;
  for (int w = 0; w < nkw; ++w) n += __builtin_popcountll(word_at(w));
  const FlaggedPos<decltype(word_at)> pos_of{n, nkw, nkt, word_at};
  *kt_begin = half == 0 ? 0 : pos_of(n / 2);
  *kt_end = half == 0 ? pos_of(n / 2) : nkt;
}

// tile_coords alone: (tile row, tile column) of linear tile t without a launch order
extern "C" void emu_tile_coords(const long long* in, int t, int* tm, int* tn) {
  Launch g{(int)in[0], (int)in[1], (int)in[3], (int)in[4], (int)in[5], (int)in[6], nullptr, {(int)in[8], (int)in[9], (int)in[10]}};
  tile_coords(g, t, *tm, *tn);
}

// next_flagged alone, on one operand's flag words
extern "C" int emu_next_flagged(const unsigned long long* a, int from, int kt_end) {
  return next_flagged(from, kt_end, [&](int w) { return a[w] & FLAGS_ALL; });
}
