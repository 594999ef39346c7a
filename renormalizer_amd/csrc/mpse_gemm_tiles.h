// The integer rules of the contraction kernel (k_gemm, mpse_gemm.hip): which tile a launch position works on and which
// K tiles it visits.  No HIP dependency: the kernel calls these, and tests/test_gemm_tiles_host.py runs them on a CPU.
// G: the launch arguments - GemmArgs on the device, any struct with the fields read here on the host; taken whole, so
// that the kernel loads each field where the rule uses it.  The forms are those that leave every instantiation's device
// code as it was (profiles/gemm_stages_refactor.md): no struct returned, every out-parameter stored once from a local.
#pragma once

#if defined(__HIPCC__)
#define MPSE_TILES_FN __host__ __device__ __forceinline__
#else
#define MPSE_TILES_FN inline
#endif

namespace mpse_tiles {

constexpr unsigned long long FLAGS_ALL = 0x0101010101010101ull;   // eight byte flags per word, all set

// Launch position -> (bs, t, half): bs = batch * ksplit + K slice (the slot row of the dot partials), t = position in
// the launch order (or the linear tile), half = which half of the tile's K tiles (split2).  Die = position mod 8:
//   * tile-fastest, or - split products of one batch element (slice_fast) - slice-fastest: a die then works on one (or
//     a few) K slices of every tile and its L2 sees 1/8 of both operands instead of most of them;
//   * split2 (grouped launches, two workgroups per tile).  On a die the first cpd positions get a compute unit each, the
//     next cpd join them: of the die's 2 m halves, by decreasing weight, the unit that receives the q-th heaviest in
//     the first round receives the q-th lightest in the second.
template <class G>
MPSE_TILES_FN void launch_position(const G& g, bool grouped, int bid, int ntile, int& bs_out, int& t_out, int& half_out) {
  int bs = bid / ntile;
  int t = bid - bs * ntile;
  int half = 0;
  if (grouped && g.gg.split2) {
    if ((ntile & 7) == 0) {
      const int m2 = 2 * (ntile >> 3), r = bid >> 3, cpd = g.gg.cpd;
      const int q = (r < cpd || m2 <= cpd) ? r : (m2 - 1) - (r - cpd);
      half = q & 1;
      t = ((q >> 1) << 3) | (bid & 7);
    } else {
      half = bid & 1;
      t = bid >> 1;
    }
    bs = half;       // (slot of the dot partials: half * tiles + tile)
  }
  if (g.slice_fast) {
    t = bid / g.ksplit;
    bs = bid - t * g.ksplit;
  }
  bs_out = bs, t_out = t, half_out = half;
}

// Index into the launch order (heaviest tiles first): the odd slices of a split product run through it backwards - the
// compute unit that receives a heavy tile's slice in one round receives a light one in the next
MPSE_TILES_FN int order_index(int t, int ks_id, int ntile) { return (ks_id & 1) ? ntile - 1 - t : t; }

// An entry of the launch order, as k_tile_order writes it: the linear tile, or ~tile for one that nobody reads
MPSE_TILES_FN void order_decode(int entry, int& tile, bool& dead) {
  dead = entry < 0;
  tile = dead ? ~entry : entry;
}

// Linear tile -> (tile row, tile column): row major, then
//   * die_group (unsplit products without a launch order): all tiles of a tile row (1) or tile column (2) on one die -
//     die x takes rows x, x + 8, .. with every column: the larger operand's panels go into one L2, not into all eight;
//   * else, without a launch order, the column skewed by the row: tile columns come in multiples of eight, so a die
//     would own whole columns - with block-sparse operands three times the K tiles of others (tools/gemm_balance.py).
// A macro that the kernel expands in place: a function is simplified on its own before it is inlined, and these
// branches then come out as other scalar code in every instantiation.  tile_coords is the whole rule.
#define MPSE_TILES_PLACE(g, t, tm, tn)                                         \
  do {                                                                         \
    if ((g).die_group == 1) {                                                  \
      const int x = (t) & 7, j = (t) >> 3;                                     \
      tm = x + 8 * (j / (g).tiles_n);                                          \
      tn = j % (g).tiles_n;                                                    \
    } else if ((g).die_group == 2) {                                           \
      const int x = (t) & 7, j = (t) >> 3;                                     \
      tn = x + 8 * (j / (g).tiles_m);                                          \
      tm = j % (g).tiles_m;                                                    \
    }                                                                          \
    if ((g).skew && !(g).perm && !(g).die_group) tn = (tn + tm) % (g).tiles_n; \
  } while (0)
template <class G>
MPSE_TILES_FN void tile_coords(const G& g, int t, int& tm_out, int& tn_out) {
  int tm = t / g.tiles_n;
  int tn = t - tm * g.tiles_n;
  MPSE_TILES_PLACE(g, t, tm, tn);
  tm_out = tm, tn_out = tn;
}

// Grouped launch: the tile row picks the group; the group's own row is tm - group * tiles_m_grp
MPSE_TILES_FN int group_of_row(int tm, int tiles_m_grp) { return tm / tiles_m_grp; }

// Flag word w of a K range of nkt tiles without the bytes past the last K tile (never written)
MPSE_TILES_FN unsigned long long trim_flags(unsigned long long x, int w, int nkt) {
  x &= FLAGS_ALL;
  const int valid = nkt - 8 * w;
  if (valid < 8) x &= valid > 0 ? (1ull << (8 * valid)) - 1ull : 0ull;
  return x;
}

// Next K tile >= from (and < kt_end) whose flag is set; kt_end if there is none.  word_at(w): flag word w, the flags of
// both operands combined.  Flags at or beyond kt_end are never looked at.
template <class Words>
MPSE_TILES_FN int next_flagged(int from, int kt_end, Words word_at) {
  while (from < kt_end) {
    const int w = from >> 3;                      // 8 byte flags per word
    unsigned long long word = word_at(w);
    word &= ~0ull << ((from & 7) * 8);
    if (word) {
      const int kt = (w << 3) + (__builtin_ctzll(word) >> 3);
      return kt < kt_end ? kt : kt_end;
    }
    from = (w + 1) << 3;
  }
  return kt_end;
}

// Position of the i-th of the n flagged K tiles of a tile (word_at: trimmed words; i >= n: the end, nkt).  split2:
// workgroup `half` takes the K range [0, pos(n / 2)) or [pos(n / 2), nkt) - n / 2 and n - n / 2 occupied tiles.
// (A functor with reference members, as a lambda of the kernel body is: as a plain function it cost scalar instructions.)
template <class Words>
struct FlaggedPos {
  const int &n, &nkw, &nkt;
  const Words& word_at;
  MPSE_TILES_FN int operator()(int i) const {
    if (i >= n) return nkt;
    int seen = 0;
    for (int w = 0; w < nkw; ++w) {
      unsigned long long x = word_at(w);
      const int c = __builtin_popcountll(x);
      if (seen + c > i) {
        for (int skip = i - seen; skip > 0; --skip) x &= x - 1;
        return (w << 3) + (__builtin_ctzll(x) >> 3);
      }
      seen += c;
    }
    return nkt;
  }
};

}  // namespace mpse_tiles
