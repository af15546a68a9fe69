// TEST HARNESS ONLY (tests/test_fallback_host.py).  Compiles tc_fallback.h -- the group cut, the jobs of the failed groups and the
// record / job / slot maps the combined entries of tc_api.hip share -- with g++.  Never linked into libtc_amd.so.  With
// -DFALLBACK_MAIN it is a stand-alone program (the sanitizer build: g++ -fsanitize=address,undefined -DFALLBACK_MAIN) that walks
// the same arithmetic over exactly-sized heap arrays and prints "fallback_host: ok".
#include "tc_fallback.h"
#include <stdio.h>
#include <vector>
using namespace tc;

extern "C" {
// out: four values (group, G, tail, NG)
void fh_group_cut(size_t B, size_t group, size_t* out) {
  const GroupCut c = group_cut(B, group);
  out[0] = c.group;
  out[1] = c.G;
  out[2] = c.tail;
  out[3] = c.NG;
}
// bad_group: group_cut(B, group).NG bytes; out: room for B values; returns how many were written
size_t fh_failed_jobs(const uint8_t* bad_group, size_t B, size_t group, uint32_t* out) {
  std::vector<uint32_t> jobs;
  failed_jobs_of_groups(bad_group, group_cut(B, group), B, jobs);
  for (size_t i = 0; i < jobs.size(); i++) out[i] = jobs[i];
  return jobs.size();
}
// record / job / slot: F * N values each
void fh_slot_maps(const uint32_t* failed, size_t F, size_t N, uint32_t* record, uint32_t* job, uint32_t* slot) {
  const SlotMaps m = slot_maps(failed, F, N);
  for (size_t r = 0; r < F * N; r++) {
    record[r] = m.record[r];
    job[r] = m.job[r];
    slot[r] = m.slot[r];
  }
}
}

#if defined(FALLBACK_MAIN)
int main() {
  int rc = 0;
  const size_t Bs[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 1025}, groups[] = {0, 1, 2, 3, 64, 1024, 2000};
  for (size_t B : Bs)
    for (size_t group : groups) {
      const GroupCut c = group_cut(B, group);
      size_t want = group ? group : 64;
      if (want > 1024) want = 1024;
      if (want > B) want = B;
      rc |= (c.group == want && c.G == B / want && c.tail == B % want && c.NG == (B + want - 1) / want) ? 0 : 1;
      // all groups, no group, every single group: the jobs lo .. hi of each, in order, never one past B
      for (size_t pick = 0; pick < c.NG + 2; pick++) {
        std::vector<uint8_t> bad(c.NG, pick == c.NG ? 1 : 0);
        if (pick < c.NG) bad[pick] = 1;
        std::vector<uint32_t> jobs;
        failed_jobs_of_groups(bad.data(), c, B, jobs);
        size_t n = 0;
        for (size_t g = 0; g < c.NG; g++)
          for (size_t j = g * want; bad[g] && j < B && j < (g + 1) * want; j++) rc |= (n < jobs.size() && jobs[n++] == j) ? 0 : 1;
        rc |= n == jobs.size() ? 0 : 1;
      }
    }
  for (size_t F : {(size_t)1, (size_t)3})
    for (size_t N : {(size_t)1, (size_t)4}) {
      const std::vector<uint32_t> failed = {7, 2, 40};  // not contiguous, not sorted
      const SlotMaps m = slot_maps(failed.data(), F, N);
      rc |= (m.record.size() == F * N && m.job.size() == F * N && m.slot.size() == F * N) ? 0 : 1;
      for (size_t f = 0; f < F; f++)
        for (size_t i = 0; i < N; i++)
          rc |= (m.record[f * N + i] == failed[f] * N + i && m.job[f * N + i] == failed[f] && m.slot[f * N + i] == i) ? 0 : 1;
    }
  printf("fallback_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
