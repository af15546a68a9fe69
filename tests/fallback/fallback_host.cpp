// TEST HARNESS ONLY (tests/test_fallback_host.py).  Compiles tc_fallback.h -- the group cut, the bad-group rule (BadGroups), the jobs
// of the failed groups, the record / job / slot maps and the records of the failed jobs that the combined entries of tc_api.hip
// share -- with g++.  Never linked into libtc_amd.so.  With
// -DFALLBACK_MAIN it is a stand-alone program (the sanitizer build: g++ -fsanitize=address,undefined -DFALLBACK_MAIN) that walks
// the same arithmetic over exactly-sized heap arrays and prints "fallback_host: ok".
#include "tc_fallback.h"
#include <stdio.h>
#include <vector>
using namespace tc;

// BadGroups with the caller's bad[] (NG bytes) as its state: one kind of evidence is ORed in, and the state goes back
template <class F>
static void with_bad(size_t B, size_t group, uint8_t* bad, F evidence) {
  BadGroups a(group_cut(B, group), B);
  for (size_t g = 0; g < a.cut.NG; g++) a.bad[g] = bad[g];
  evidence(a);
  for (size_t g = 0; g < a.cut.NG; g++) bad[g] = a.bad[g];
}

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
// v: NG bytes or null
void fh_bad_per_group(size_t B, size_t group, uint8_t* bad, const uint8_t* v, int zero_bad) {
  with_bad(B, group, bad, [&](BadGroups& a) { a.per_group(v, zero_bad != 0); });
}
void fh_bad_all(size_t B, size_t group, uint8_t* bad) {
  with_bad(B, group, bad, [&](BadGroups& a) { a.all(); });
}
// first: NG + 1 values; v: first[NG] bytes or null
void fh_bad_spans(size_t B, size_t group, uint8_t* bad, const uint64_t* first, const uint8_t* v, int zero_bad) {
  with_bad(B, group, bad, [&](BadGroups& a) { a.spans(first, v, zero_bad != 0); });
}
// v1, v2: B bytes or null
void fh_bad_jobs(size_t B, size_t group, uint8_t* bad, const uint8_t* v1, const uint8_t* v2, int zero_bad) {
  with_bad(B, group, bad, [&](BadGroups& a) { a.jobs({v1, v2}, zero_bad != 0); });
}
// rec_first: NG + 1 values; key_idx: rec_first[NG] values or null; key_ok: K bytes or null
void fh_bad_named_keys(size_t B, size_t group, uint8_t* bad, const uint64_t* rec_first, const uint64_t* key_idx, size_t K, const uint8_t* key_ok) {
  with_bad(B, group, bad, [&](BadGroups& a) { a.named_keys(rec_first, key_idx, K, key_ok); });
}
// BadGroups::failed_jobs over the caller's bad[]; out: room for B values; returns how many were written
size_t fh_bad_failed_jobs(size_t B, size_t group, uint8_t* bad, uint32_t* out) {
  size_t n = 0;
  with_bad(B, group, bad, [&](BadGroups& a) {
    for (uint32_t j : a.failed_jobs()) out[n++] = j;
  });
  return n;
}
// record / job: room for every record of the n jobs; returns how many were written ((size_t)-1: the maps differ in length, or the
// slot map is not empty)
size_t fh_records_of_jobs(const uint64_t* rec_off, const uint32_t* jobs, size_t n, uint32_t* record, uint32_t* job) {
  const SlotMaps m = records_of_jobs(rec_off, std::vector<uint32_t>(jobs, jobs + n));
  if (m.job.size() != m.record.size() || !m.slot.empty()) return (size_t)-1;
  for (size_t r = 0; r < m.record.size(); r++) {
    record[r] = m.record[r];
    job[r] = m.job[r];
  }
  return m.record.size();
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
  // the bad-group rule: one bad byte at every place of every kind of evidence, each polarity, over heap arrays of the exact sizes
  for (size_t B : {(size_t)1, (size_t)2, (size_t)3, (size_t)5})
    for (size_t group : {(size_t)1, (size_t)2, (size_t)3})
      for (int zero_bad = 0; zero_bad < 2; zero_bad++) {
        const GroupCut c = group_cut(B, group);
        const uint8_t good = zero_bad ? 1 : 0, wrong = zero_bad ? 0 : 7;
        // job j owns j % 3 records (so some jobs, and with them some groups, own none)
        std::vector<uint64_t> rec_off(B + 1, 0), grp(c.NG + 1);
        for (size_t j = 0; j < B; j++) rec_off[j + 1] = rec_off[j] + j % 3;
        for (size_t g = 0; g <= c.NG; g++) grp[g] = rec_off[g * c.group < B ? g * c.group : B];
        const size_t R = (size_t)rec_off[B], K = 3;
        for (size_t at = 0; at <= B; at++) {  // at == B: nothing is bad
          std::vector<uint8_t> v(B, good);
          if (at < B) v[at] = wrong;
          BadGroups a(c, B), none(c, B);
          a.jobs({nullptr, v.data()}, zero_bad != 0);
          none.jobs({nullptr}, zero_bad != 0);
          none.spans(grp.data(), nullptr, zero_bad != 0);
          none.per_group(nullptr, zero_bad != 0);
          none.named_keys(grp.data(), nullptr, K, nullptr);
          for (size_t g = 0; g < c.NG; g++) rc |= (a.bad[g] == (at < B && at / c.group == g) && !none.bad[g]) ? 0 : 1;
          std::vector<uint32_t> want;
          for (size_t j = 0; at < B && j < B; j++)
            if (j / c.group == at / c.group) want.push_back((uint32_t)j);
          rc |= a.failed_jobs() == want ? 0 : 1;
          const SlotMaps m = records_of_jobs(rec_off.data(), want);
          size_t n = 0;
          for (uint32_t j : want)
            for (uint64_t r = rec_off[j]; r < rec_off[j + 1]; r++, n++) rc |= (n < m.record.size() && m.record[n] == r && m.job[n] == j) ? 0 : 1;
          rc |= (n == m.record.size() && n == m.job.size() && m.slot.empty()) ? 0 : 1;
        }
        for (size_t at = 0; at < c.NG; at++) {
          std::vector<uint8_t> v(c.NG, good);
          v[at] = wrong;
          BadGroups a(c, B);
          a.per_group(v.data(), zero_bad != 0);
          for (size_t g = 0; g < c.NG; g++) rc |= a.bad[g] == (g == at) ? 0 : 1;
          a.all();
          rc |= a.failed_jobs().size() == B ? 0 : 1;
        }
        for (size_t at = 0; at < R; at++) {  // one bad record; then one bad key, record r naming key (r * 2) % K but for one index out of range
          std::vector<uint8_t> v(R, good), key_ok(K, 1);
          v[at] = wrong;
          std::vector<uint64_t> key_idx(R);
          for (size_t r = 0; r < R; r++) key_idx[r] = (r * 2) % K;
          key_ok[key_idx[at]] = 0;
          key_idx[(at + 1) % R] = at % 2 ? K : ~(uint64_t)0;
          BadGroups a(c, B), b(c, B);
          a.spans(grp.data(), v.data(), zero_bad != 0);
          b.named_keys(grp.data(), key_idx.data(), K, key_ok.data());
          for (size_t g = 0; g < c.NG; g++) {
            bool named = false;
            for (uint64_t r = grp[g]; r < grp[g + 1]; r++) named = named || (key_idx[r] < K && !key_ok[key_idx[r]]);
            rc |= (a.bad[g] == (grp[g] <= at && at < grp[g + 1]) && b.bad[g] == named) ? 0 : 1;
          }
        }
      }
  printf("fallback_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
