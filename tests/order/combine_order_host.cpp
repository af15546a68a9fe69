// TEST HARNESS ONLY (tests/test_combine_order_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and
// runs the pieces of the G2 launch order that tc_jobs.h holds: the predicted cost of a tuple, the descending order of the
// groups, the fold of a single resident round and the slot of a job -- fed by the serial model of k_combine_group /
// k_combine_plan / k_combine_place (one thread after the other; a barrier is the end of a loop).  Never linked into
// libtc_amd.so.  With -DCO_MAIN a stand-alone program over fixed inputs (for a sanitizer build:
// g++ -fsanitize=address,undefined -DCO_MAIN) that prints "combine_order_host: ok".
#include "tc_jobs.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
uint32_t co_tuple_macs(int t, const uint64_t* idx) { return combine_tuple_macs(idx, t); }
uint32_t co_key_macs(int t, uint64_t key) { return combine_key_macs(key, t); }
uint32_t co_divide_macs(uint64_t d_abs) { return combine_divide_macs(d_abs); }
// the same without the shortcut for small denominators: the cheaper of the two forms, as combine_divide_cheapest chooses
uint32_t co_divide_macs_by_comparison(uint64_t d_abs) {
  const uint32_t ladder = combine_divide_uniform_macs(d_abs);
  uint64_t q = 0;
  int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
  if (combine_denominator_class(d_abs) != kCombineClassGeneric || !combine_quotient_decompose(d_abs, &q, T, E)) return ladder;
  const uint32_t planned = combine_quotient_plan(q, T, E).macs;
  return planned < ladder ? planned : ladder;
}
uint32_t co_mixed_generic_macs() { return kMacsMixedGeneric; }
uint32_t co_group_slots(size_t B) { return (uint32_t)(B + (size_t)kSubsetMaxGroups * (kSubsetPad - 1)); }
int co_aligned(uint32_t waves, uint32_t seats) { return combine_order_aligned(waves, seats); }
uint32_t co_fold_wave(uint32_t d, uint32_t fold_seats) { return combine_fold_wave(d, fold_seats); }

// The grouping of B jobs as the three kernels build it.  perm: co_group_slots(B) words; cost / start_wave: kSubsetSlots words
// (start_wave 0xffffffff for an empty entry); *fold = the seats the order folds at (0: plain descending cost).  Returns the
// mode (1 = subset), -1 when a position falls outside perm, -2 when two jobs get one position.
int co_plan(int t, const uint64_t* idx, size_t n_per_job, size_t B, uint32_t seats, uint32_t* perm, uint32_t* cost_out, uint32_t* start_wave,
            uint32_t* fold, uint32_t* waves_out) {
  std::vector<uint64_t> ws64((kGwsZeroWords + 1) / 2, 0);
  uint32_t* ws = reinterpret_cast<uint32_t*>(ws64.data());
  std::vector<uint32_t> rank(B, 0xffffffffu), crank(B, 0);
  std::vector<uint16_t> grp(B, 0xffffu);
  std::vector<uint8_t> cls(B, 0);
  const size_t slots = co_group_slots(B);
  // k_combine_group
  for (size_t j0 = 0; j0 < B; j0 += kGroupWgJobs) {
    const uint32_t n = (uint32_t)(B - j0 < kGroupWgJobs ? B - j0 : kGroupWgJobs);
    std::vector<uint64_t> wkey(kGroupWgSlots, 0);
    std::vector<uint32_t> wcount(kGroupWgSlots, 0), wbase(kGroupWgSlots, 0), slot(n), lrank(n);
    std::vector<uint16_t> wentry(kGroupWgSlots, 0xffffu);
    std::vector<uint8_t> made(n);
    for (uint32_t i = 0; i < n; i++) {
      int c;
      const uint64_t key = combine_tuple_key(idx + (j0 + i) * n_per_job, t, &c);
      cls[j0 + i] = (uint8_t)c;
      crank[j0 + i] = ws[kGwsClassCount + c]++;
      bool m;
      slot[i] = combine_wg_insert(wkey.data(), wcount.data(), key, &lrank[i], &m);
      made[i] = m;
    }
    for (uint32_t i = 0; i < n; i++)
      if (made[i]) combine_wg_publish(slot[i], wkey.data(), wcount.data(), wentry.data(), wbase.data(), ws);
    for (uint32_t i = 0; i < n; i++)
      if (wentry[slot[i]] < kSubsetSlots) {
        grp[j0 + i] = wentry[slot[i]];
        rank[j0 + i] = wbase[slot[i]] + lrank[i];
      }
  }
  // k_combine_plan
  const uint64_t* keys = ws64.data();
  const bool subset = combine_subset_mode(ws[kGwsOverflow] != 0, ws[kGwsGroups], B);
  std::vector<uint32_t> count(kSubsetSlots), cost(kSubsetSlots), start(kSubsetSlots);
  for (uint32_t s = 0; s < kSubsetSlots; s++) {
    count[s] = ws[kGwsCount + s];
    cost[s] = subset && count[s] ? combine_key_macs(keys[s], t) : 0;
  }
  uint32_t waves = 0;
  for (uint32_t s = 0; s < kSubsetSlots; s++) start[s] = combine_order_start(cost.data(), count.data(), kSubsetSlots, s, kSubsetPad, &waves);
  const uint32_t fold_seats = subset && combine_order_aligned(waves, seats) ? seats : 0;
  uint8_t corder[kCombineClasses];
  uint32_t ccount[kCombineClasses], cstart[kCombineClasses];
  for (int c = 0; c < kCombineClasses; c++) {
    corder[c] = (uint8_t)combine_class_order(c);
    ccount[c] = ws[kGwsClassCount + c];
  }
  for (int c = 0; c < kCombineClasses; c++) cstart[c] = combine_group_start(ccount, corder, kCombineClasses, (uint32_t)c, kClassPad);
  for (uint32_t s = 0; s < kSubsetSlots; s++) {
    cost_out[s] = cost[s];
    start_wave[s] = subset && count[s] ? start[s] : 0xffffffffu;
  }
  *fold = fold_seats;
  *waves_out = waves;
  // k_combine_place
  for (size_t i = 0; i < slots; i++) perm[i] = 0xffffffffu;
  for (size_t j = 0; j < B; j++) {
    if (subset && grp[j] >= kSubsetSlots) return -1;
    const size_t pos = subset ? combine_order_slot(start[grp[j]], rank[j], kSubsetPad, fold_seats) : (size_t)cstart[cls[j]] + crank[j];
    if (pos >= slots) return -1;
    if (perm[pos] != 0xffffffffu) return -2;
    perm[pos] = (uint32_t)j;
  }
  return subset ? 1 : 0;
}
}

#if defined(CO_MAIN)
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return (uint32_t)(g_seed >> 16);
}
static int fail(const char* what, long a, long b) {
  printf("combine_order_host: FAILED %s (%ld, %ld)\n", what, a, b);
  return 1;
}
int main() {
  for (size_t B : {(size_t)1, (size_t)255, (size_t)4096, (size_t)4127, (size_t)9000}) {
    for (uint32_t tuples : {1u, 16u, 17u, 35u, 700u}) {
      for (uint32_t seats : {0u, 2u, 64u, 100u, 4096u}) {
        const size_t n = 4;
        std::vector<uint64_t> idx(B * n);
        for (size_t j = 0; j < B; j++) {
          const uint32_t k = rnd32() % tuples;
          for (size_t i = 0; i < n; i++) idx[j * n + i] = (uint64_t)(k % 27) + 3 * i + (i ? k / 27 : 0);
          if (rnd32() % 97 == 0) idx[j * n + 3] = 65535;
        }
        const size_t slots = co_group_slots(B);
        std::vector<uint32_t> perm(slots), cost(kSubsetSlots), start(kSubsetSlots);
        std::vector<uint8_t> seen(B, 0);
        uint32_t fold = 0, waves = 0;
        const int mode = co_plan(3, idx.data(), n, B, seats, perm.data(), cost.data(), start.data(), &fold, &waves);
        if (mode < 0) return fail("plan", (long)B, mode);
        for (size_t i = 0; i < slots; i++) {
          if (perm[i] == 0xffffffffu) continue;
          if (perm[i] >= B || seen[perm[i]]) return fail("placed twice", (long)B, (long)i);
          seen[perm[i]] = 1;
        }
        for (size_t j = 0; j < B; j++)
          if (!seen[j]) return fail("not placed", (long)B, (long)j);
      }
    }
  }
  printf("combine_order_host: ok\n");
  return 0;
}
#endif
