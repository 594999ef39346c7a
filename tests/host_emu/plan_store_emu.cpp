// Host build of the plan store's slot table and match rules (renormalizer_amd/csrc/mpse_plan_store.h) for
// tests/test_plan_reuse_host.py: a table with an int payload, driven through a flat C interface.
#include "../../renormalizer_amd/csrc/mpse_plan_store.h"

#include <vector>

namespace {
using Tab = mpse_store::Table<int>;
Tab g_tab;
std::vector<int> g_released;
int g_evicted = 0;     // slots evicted by the last emu_put, also when it found no room
}  // namespace

extern "C" {

void emu_reset(long long budget) {
  g_tab = Tab();
  g_tab.budget = (size_t)budget;
  g_released.clear();
}

// 1: found (and touched), 0: not there
int emu_find(long long key) { return g_tab.find(key) ? 1 : 0; }

// looks the key up, inserts it when missing, and gives it `bytes` device bytes and the payload `tag`; borrowed != 0: the
// slot stays borrowed.  Returns the number of slots evicted to make room, -1 when the budget could not be met (the slot
// then owns nothing).
int emu_put(long long key, long long bytes, int tag, int borrowed) {
  Tab::Slot* s = g_tab.find(key);
  if (!s) s = g_tab.insert(key);
  g_tab.charge(s, 0);
  const bool room = g_tab.make_room((size_t)bytes, s, [](int& t) { g_released.push_back(t); }, &g_evicted);
  if (room) {
    g_tab.charge(s, (size_t)bytes);
    s->data = tag;
  }
  s->borrowed = borrowed != 0;
  return room ? g_evicted : -1;
}

void emu_release(long long key) {
  for (auto& s : g_tab.slots)      // (not find(): handing a slot back is no use of it)
    if (s.key == key) s.borrowed = false;
}

int emu_last_evicted() { return g_evicted; }
long long emu_total() { return (long long)g_tab.total; }
int emu_count() { return (int)g_tab.slots.size(); }
int emu_released(int* out, int cap) {
  int n = 0;
  for (int t : g_released)
    if (n < cap) out[n++] = t;
  return (int)g_released.size();
}

// F0Match of a kept (sig, terms) against a new one; sig: 11 ints in the order of F0Sig
int emu_f0_match(int have, const int* kept, const char* kept_terms, int kept_n, const int* now, const char* terms, int n) {
  auto sig = [](const int* v) { return mpse_store::F0Sig{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]}; };
  const std::vector<char> kt(kept_terms, kept_terms + kept_n);
  return (int)mpse_store::f0_match(have != 0, sig(kept), kt, sig(now), terms, (size_t)n);
}

}  // extern "C"
