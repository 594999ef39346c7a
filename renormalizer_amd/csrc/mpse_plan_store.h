// Slot table of the context's plan store (mpse_ctx::plan_store) and the host-side match rules of a slot - host code
// only, no HIP: tests/host_emu/plan_store_emu.cpp compiles this header with g++.
//
// A slot is named by the caller's key (mpse_solve_slot) and owns device data that a later solve under the same key may
// find unchanged: the plan data of the fused matvec (mpse_heff0.hip).  What is compared on the HOST before a slot's
// data is used is here (F0Sig + the term table); what is compared on the DEVICE (tile flags, centre mask) rides on the
// scan kernels.  The table itself knows keys, sizes and ages only: the payload P is the engine's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <list>
#include <vector>

namespace mpse_store {

// Everything about a fused-matvec plan that the host can compare: two solves whose signatures and term tables are
// equal run k_f0_plan on the same arguments, and differ at most in the flag bytes the device compares.
struct F0Sig {
  int Dl = 0, Dr = 0, wl = 0, wr = 0, d = 0, nsite = -1, n_cu = 0, compact = 0, fc_pitch = 0, fc_bytes = 0, order_on = 0;
};
inline bool f0_sig_equal(const F0Sig& a, const F0Sig& b) {
  return a.Dl == b.Dl && a.Dr == b.Dr && a.wl == b.wl && a.wr == b.wr && a.d == b.d && a.nsite == b.nsite &&
         a.n_cu == b.n_cu && a.compact == b.compact && a.fc_pitch == b.fc_pitch && a.fc_bytes == b.fc_bytes &&
         a.order_on == b.order_on;
}
// What a keyed solve finds in its slot
enum F0Match {
  F0_FRESH = 0,    // no plan of this kind in the slot yet: allocate, upload, force the planner
  F0_SHAPE = 1,    // another signature: the buffer is replaced, upload, force
  F0_TERMS = 2,    // same signature, another term table (another MPO site): the buffer stays, upload, force
  F0_HIT = 3       // equal: no upload, the planner runs only if the device saw another flag byte
};
inline F0Match f0_match(bool have, const F0Sig& kept, const std::vector<char>& kept_terms, const F0Sig& now,
                        const void* terms, size_t term_bytes) {
  if (!have) return F0_FRESH;
  if (!f0_sig_equal(kept, now)) return F0_SHAPE;
  if (kept_terms.size() != term_bytes || (term_bytes && memcmp(kept_terms.data(), terms, term_bytes) != 0)) return F0_TERMS;
  return F0_HIT;
}

template <class P>
struct Table {
  struct Slot {
    int64_t key = 0;
    unsigned long long age = 0;   // value of the table's clock at the last lookup
    size_t bytes = 0;             // device bytes the slot owns (charge())
    bool borrowed = false;        // a solve is using it: never evicted
    P data{};
  };
  std::list<Slot> slots;          // (a list: slots keep their address while others come and go)
  size_t budget = size_t(64) << 20;
  size_t total = 0;
  unsigned long long clock = 0;

  Slot* find(int64_t key) {
    for (auto& s : slots)
      if (s.key == key) {
        s.age = ++clock;
        return &s;
      }
    return nullptr;
  }
  Slot* insert(int64_t key) {
    slots.emplace_back();
    Slot& s = slots.back();
    s.key = key;
    s.age = ++clock;
    return &s;
  }
  // the slot's device bytes become `bytes`
  void charge(Slot* s, size_t bytes) {
    total = total - s->bytes + bytes;
    s->bytes = bytes;
  }
  // Makes room for `need` more bytes: evicts the least recently used slots that nobody borrows (never `keep`) until
  // total + need <= budget; release(data) frees a slot's device memory.  *evicted = number of slots that went.  False:
  // the budget cannot be met (the caller then goes without a slot; what was evicted on the way stays evicted and counted).
  template <class F>
  bool make_room(size_t need, const Slot* keep, F&& release, int* evicted) {
    int& n = *evicted;
    n = 0;
    while (total + need > budget) {
      auto lru = slots.end();
      for (auto it = slots.begin(); it != slots.end(); ++it)
        if (!it->borrowed && &*it != keep && it->bytes > 0 && (lru == slots.end() || it->age < lru->age)) lru = it;
      if (lru == slots.end()) return false;
      release(lru->data);
      total -= lru->bytes;
      slots.erase(lru);
      ++n;
    }
    return true;
  }
  template <class F>
  void clear(F&& release) {
    for (auto& s : slots) release(s.data);
    slots.clear();
    total = 0;
  }
};

}  // namespace mpse_store
