// Host export of the result-tile liveness rule (mpse_plans.h out_tile_live) for tests/test_plans_outmask_host.py, and of
// grouped_plan with its out_mask argument.
#include "../../renormalizer_amd/csrc/mpse_plans.h"

using namespace mpse_plan;

// live[tm * tiles_n + tn] for every 64 x 64 tile of the (M = Dl * d) x Dr result
extern "C" void emu_out_tiles_live(const unsigned char* mask, int pitch, int d, int Dr, int M, unsigned char* live) {
  const int tiles_m = (M + 63) / 64, tiles_n = (Dr + 63) / 64;
  for (int tm = 0; tm < tiles_m; ++tm)
    for (int tn = 0; tn < tiles_n; ++tn) live[tm * tiles_n + tn] = out_tile_live(mask, pitch, d, Dr, M, tm, tn) ? 1 : 0;
}

// out: order, die_group, wide, nwg
extern "C" void emu_grouped_plan_outmask(long long M, long long N, int nkt_max, int split2, int n_cu, int out_mask,
                                         long long* out) {
  const GroupedPlan p = grouped_plan(M, N, 1, nkt_max, true, split2 != 0, true, n_cu, out_mask != 0);
  out[0] = p.order, out[1] = p.die_group, out[2] = p.wide, out[3] = p.nwg;
}
