// TEST HARNESS ONLY (tests/test_combine_group_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and
// runs the pieces of the G2 grouping kernels (k_combine.hip k_combine_group / k_combine_plan) that tc_jobs.h holds: the
// workgroup's own table, the step of the one lane per distinct key on the call's table, and the prefix-sum starts.  On the host
// a workgroup is a loop over its jobs and a barrier is the end of that loop.  Never linked into libtc_amd.so.  With -DCG_MAIN
// it is a stand-alone program (for a sanitizer build: g++ -fsanitize=address,undefined -DCG_MAIN) over fixed inputs in
// exactly-sized heap arrays that prints "combine_group_host: ok".
#include "tc_jobs.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
uint32_t cg_wg_jobs() { return kGroupWgJobs; }
uint32_t cg_wg_slots() { return kGroupWgSlots; }
uint32_t cg_wg_hash(uint64_t key) { return combine_wg_hash(key); }
uint32_t cg_table_hash(uint64_t key) { return combine_key_hash(key) & (kSubsetSlots - 1); }
uint32_t cg_probe_step(uint64_t key) { return combine_probe_step(key); }
uint64_t cg_key(int t, const uint64_t* idx) {
  int c;
  return combine_tuple_key(idx, t, &c);
}
uint32_t cg_group_slots(size_t B) { return (uint32_t)(B + (size_t)kSubsetMaxGroups * (kSubsetPad - 1)); }

// the starts of n groups: by the scan (steps of n threads, a barrier after each) and by n walks
void cg_scan_starts(const uint32_t* count, const uint8_t* order, uint32_t n, uint32_t pad, uint32_t* start) {
  std::vector<uint32_t> buf((size_t)2 * n * kGroupOrders, 0xdeadbeefu);
  for (int step = 0; step < combine_scan_steps(n); step++)
    for (uint32_t s = 0; s < n; s++) combine_scan_step(step, s, n, count, order, pad, buf.data());
  for (uint32_t s = 0; s < n; s++) start[s] = combine_scan_start(s, n, count, order, pad, buf.data());
}
void cg_walk_starts(const uint32_t* count, const uint8_t* order, uint32_t n, uint32_t pad, uint32_t* start) {
  for (uint32_t s = 0; s < n; s++) start[s] = combine_group_start(count, order, n, s, pad);
}

// One workgroup's aggregation alone: n <= kGroupWgJobs keys.  slot / lrank / made per job, wkey / wcount: the table
// (kGroupWgSlots entries).  Returns the number of entries made.
int cg_wg_aggregate(const uint64_t* keys, uint32_t n, uint32_t* slot, uint32_t* lrank, uint8_t* made, uint64_t* wkey, uint32_t* wcount) {
  if (n > kGroupWgJobs) return -1;
  memset(wkey, 0, kGroupWgSlots * sizeof(uint64_t));
  memset(wcount, 0, kGroupWgSlots * sizeof(uint32_t));
  int entries = 0;
  for (uint32_t i = 0; i < n; i++) {
    bool m;
    slot[i] = combine_wg_insert(wkey, wcount, keys[i], &lrank[i], &m);
    made[i] = m;
    entries += m;
  }
  return entries;
}

// The grouping of B jobs as k_combine_group / k_combine_plan / k_combine_place build it: workgroup after workgroup (insert,
// barrier, publish, barrier, ranks), the plan by the scan, the placement.  perm: cg_group_slots(B) words.  Returns the mode
// (1 = subset), -1 when a position falls outside perm, -2 when two jobs get one position; *groups = distinct keys seen before
// the table closed, *need = the jobs the fast path leaves.
int cg_plan(int t, const uint64_t* idx, size_t n_per_job, size_t B, uint32_t* perm, uint32_t* starts, uint8_t* orders, uint32_t* groups,
            uint32_t* need) {
  std::vector<uint64_t> ws64((kGwsZeroWords + 1) / 2, 0);  // (8-byte aligned: the keys are read as 64-bit words)
  uint32_t* ws = reinterpret_cast<uint32_t*>(ws64.data());
  std::vector<uint32_t> rank(B, 0xffffffffu), crank(B, 0);
  std::vector<uint16_t> grp(B, 0xffffu);
  std::vector<uint8_t> cls(B, 0);
  const size_t slots = cg_group_slots(B);
  for (size_t j0 = 0; j0 < B; j0 += kGroupWgJobs) {
    const uint32_t n = (uint32_t)(B - j0 < kGroupWgJobs ? B - j0 : kGroupWgJobs);
    std::vector<uint64_t> wkey(kGroupWgSlots, 0);
    std::vector<uint32_t> wcount(kGroupWgSlots, 0), wbase(kGroupWgSlots, 0xdeadbeefu), slot(n), lrank(n);
    std::vector<uint16_t> wentry(kGroupWgSlots, 0xbeefu);
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
    for (uint32_t i = 0; i < n; i++) {
      if (wentry[slot[i]] < kSubsetSlots) {
        grp[j0 + i] = wentry[slot[i]];
        rank[j0 + i] = wbase[slot[i]] + lrank[i];
      }
    }
  }
  *groups = ws[kGwsGroups];
  *need = ws[kGwsNeed];
  // k_combine_plan
  const uint64_t* keys = ws64.data();
  std::vector<uint32_t> count(kSubsetSlots), start(kSubsetSlots);
  std::vector<uint8_t> order(kSubsetSlots);
  for (uint32_t s = 0; s < kSubsetSlots; s++) {
    count[s] = ws[kGwsCount + s];
    order[s] = keys[s] ? (uint8_t)combine_key_order(keys[s], t) : (uint8_t)(kGroupOrders - 1);
  }
  const bool subset = combine_subset_mode(ws[kGwsOverflow] != 0, ws[kGwsGroups], B);
  cg_scan_starts(count.data(), order.data(), kSubsetSlots, kSubsetPad, start.data());
  uint8_t corder[kCombineClasses];
  uint32_t ccount[kCombineClasses], cstart[kCombineClasses];
  for (int c = 0; c < kCombineClasses; c++) {
    corder[c] = (uint8_t)combine_class_order(c);
    ccount[c] = ws[kGwsClassCount + c];
  }
  for (int c = 0; c < kCombineClasses; c++) cstart[c] = combine_group_start(ccount, corder, kCombineClasses, (uint32_t)c, kClassPad);
  for (uint32_t s = 0; s < kSubsetSlots; s++) {
    starts[s] = subset && count[s] ? start[s] : 0xffffffffu;
    orders[s] = order[s];
  }
  // k_combine_place
  for (size_t i = 0; i < slots; i++) perm[i] = 0xffffffffu;
  for (size_t j = 0; j < B; j++) {
    if (subset && grp[j] >= kSubsetSlots) return -1;  // (subset mode: no key was turned away)
    const size_t pos = subset ? (size_t)start[grp[j]] + rank[j] : (size_t)cstart[cls[j]] + crank[j];
    if (pos >= slots) return -1;
    if (perm[pos] != 0xffffffffu) return -2;
    perm[pos] = (uint32_t)j;
  }
  return subset ? 1 : 0;
}
}

#if defined(CG_MAIN)
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return (uint32_t)(g_seed >> 16);
}
static int fail(const char* what, long a, long b) {
  printf("combine_group_host: FAILED %s (%ld, %ld)\n", what, a, b);
  return 1;
}
int main() {
  // starts: the scan against the walks
  for (uint32_t n : {1u, 3u, 64u, 512u}) {
    for (int round = 0; round < 4; round++) {
      std::vector<uint32_t> count(n), a(n), b(n);
      std::vector<uint8_t> order(n);
      for (uint32_t s = 0; s < n; s++) {
        count[s] = round == 0 ? 0 : (rnd32() % 3 == 0 ? 0 : rnd32() % 1000);
        order[s] = (uint8_t)(rnd32() % kGroupOrders);
      }
      cg_scan_starts(count.data(), order.data(), n, kSubsetPad, a.data());
      cg_walk_starts(count.data(), order.data(), n, kSubsetPad, b.data());
      for (uint32_t s = 0; s < n; s++)
        if (a[s] != b[s]) return fail("starts", n, s);
    }
  }
  // placement: few tuples (subset mode), many (class mode), more than the table admits; ragged sizes; some jobs the fast path leaves
  for (size_t B : {(size_t)1, (size_t)255, (size_t)4096, (size_t)4097, (size_t)4127}) {
    for (uint32_t tuples : {1u, 16u, 17u, 210u, 700u}) {
      const size_t n = 4;
      std::vector<uint64_t> idx(B * n);
      for (size_t j = 0; j < B; j++) {
        const uint32_t k = rnd32() % tuples;
        for (size_t i = 0; i < n; i++) idx[j * n + i] = (uint64_t)(k % 27) + 3 * i + (i ? k / 27 : 0);
        if (rnd32() % 97 == 0) idx[j * n + 3] = 65535;
      }
      const size_t slots = cg_group_slots(B);
      std::vector<uint32_t> perm(slots), starts(kSubsetSlots);
      std::vector<uint8_t> orders(kSubsetSlots), seen(B, 0);
      uint32_t groups = 0, need = 0, general = 0;
      const int mode = cg_plan(3, idx.data(), n, B, perm.data(), starts.data(), orders.data(), &groups, &need);
      if (mode < 0) return fail("plan", (long)B, mode);
      for (size_t i = 0; i < slots; i++) {
        if (perm[i] == 0xffffffffu) continue;
        if (perm[i] >= B || seen[perm[i]]) return fail("placed twice", (long)B, (long)i);
        seen[perm[i]] = 1;
      }
      for (size_t j = 0; j < B; j++) {
        if (!seen[j]) return fail("not placed", (long)B, (long)j);
        general += !combine_small_applies(idx.data() + j * n, 3);
      }
      if (need != general) return fail("need", need, general);
    }
  }
  printf("combine_group_host: ok\n");
  return 0;
}
#endif
