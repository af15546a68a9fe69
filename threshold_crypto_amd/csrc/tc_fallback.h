// Host arithmetic of the combined entries of tc_api.hip -- "check a whole group with one pairing, re-check the failures one by
// one": how a batch is cut into groups, which groups the evidence a call has read back sends to the per-job checks (BadGroups,
// the ONE copy of that rule) and which jobs those are, and the index maps that compact the N slots (ragged calls: the records)
// of every failed job.  Plain host C++, no HIP: tc_api.hip and tests/fallback/fallback_host.cpp (g++) share it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <vector>

namespace tc {

// B jobs in groups of `group` consecutive jobs: G full groups, then `tail` < group jobs in a group of their own; NG groups in all
struct GroupCut {
  size_t group, G, tail, NG;
};
// the caller's `group` as the entries take it: 0 = the default of 64, at most 1024, at most B
inline GroupCut group_cut(size_t B, size_t group) {
  if (group == 0) group = 64;
  if (group > 1024) group = 1024;
  if (group > B) group = B;
  GroupCut c{group, 0, 0, 0};
  if (group) {
    c.G = B / group;
    c.tail = B % group;
    c.NG = c.G + (c.tail ? 1 : 0);
  }
  return c;
}

// appends to `out` every job of the groups g < cut.NG with bad_group[g] != 0, in order
inline void failed_jobs_of_groups(const uint8_t* bad_group, const GroupCut& cut, size_t B, std::vector<uint32_t>& out) {
  for (size_t g = 0; g < cut.NG; g++) {
    if (!bad_group[g]) continue;
    const size_t lo = g * cut.group, hi = (lo + cut.group < B) ? lo + cut.group : B;
    for (size_t j = lo; j < hi; j++) out.push_back((uint32_t)j);
  }
}

// Which of cut.NG groups of B jobs go to the per-item checks.  Every group starts good and evidence is ORed in, so the order of
// the calls does not matter.  zero_bad says which byte is the bad one: 0 (ok bytes, membership verdicts) or non-zero (status
// bytes).  A null array is no evidence: a verdict that nobody registered (Call::take_verdicts, tc_api.hip).
inline bool has_zero(const uint8_t* v, size_t n) { return v && n && memchr(v, 0, n) != nullptr; }
struct BadGroups {
  GroupCut cut;
  size_t B;
  std::vector<uint8_t> bad;         // NG bytes
  std::vector<uint64_t> job_first;  // NG + 1 values: group g holds the jobs job_first[g] .. job_first[g + 1]
  BadGroups(const GroupCut& c, size_t jobs) : cut(c), B(jobs), bad(c.NG, 0), job_first(c.NG + 1) {
    for (size_t g = 0; g <= cut.NG; g++) job_first[g] = g * cut.group < B ? g * cut.group : B;
  }
  void all() { bad.assign(cut.NG, 1); }  // (the one key of every job is no member)
  void per_group(const uint8_t* v, bool zero_bad) {  // v[g] speaks for group g
    for (size_t g = 0; v && g < cut.NG; g++) bad[g] |= (v[g] == 0) == zero_bad;
  }
  // v[first[g] .. first[g + 1]] speak for group g (first: NG + 1 non-decreasing values -- its jobs, its records, its pieces)
  void spans(const uint64_t* first, const uint8_t* v, bool zero_bad) {
    for (size_t g = 0; v && g < cut.NG; g++)
      for (uint64_t i = first[g]; i < first[g + 1] && !bad[g]; i++) bad[g] = (v[i] == 0) == zero_bad;
  }
  void jobs(std::initializer_list<const uint8_t*> vs, bool zero_bad) {  // v[j] speaks for the group of job j
    for (const uint8_t* v : vs) spans(job_first.data(), v, zero_bad);
  }
  // record r of group g (rec_first[g] .. rec_first[g + 1]) names key key_idx[r] (null: key r) of K keys with the verdicts key_ok: a
  // named key with verdict 0 marks the group.  An index >= K is not this rule's business: the record's segment has failed its sum.
  void named_keys(const uint64_t* rec_first, const uint64_t* key_idx, size_t K, const uint8_t* key_ok) {
    if (!has_zero(key_ok, K)) return;
    for (size_t g = 0; g < cut.NG; g++)
      for (uint64_t r = rec_first[g]; r < rec_first[g + 1] && !bad[g]; r++) {
        const uint64_t i = key_idx ? key_idx[r] : r;
        bad[g] = i < K && key_ok[i] == 0;
      }
  }
  std::vector<uint32_t> failed_jobs() const {  // every job of the bad groups, in order
    std::vector<uint32_t> out;
    failed_jobs_of_groups(bad.data(), cut, B, out);
    return out;
  }
};

// The rows f * N + i of F failed jobs x N slots: the record (failed[f], i) of the call's B x N arrays, its job, its slot
struct SlotMaps {
  std::vector<uint32_t> record, job, slot;
};
inline SlotMaps slot_maps(const uint32_t* failed, size_t F, size_t N) {
  SlotMaps m;
  m.record.resize(F * N);
  m.job.resize(F * N);
  m.slot.resize(F * N);
  for (size_t f = 0; f < F; f++)
    for (size_t i = 0; i < N; i++) {
      m.record[f * N + i] = (uint32_t)(failed[f] * N + i);
      m.job[f * N + i] = failed[f];
      m.slot[f * N + i] = (uint32_t)i;
    }
  return m;
}
// The ragged form: job j owns the records rec_off[j] .. rec_off[j + 1].  For each of `jobs` in order, its records in order: the
// record and its job (no slot map)
inline SlotMaps records_of_jobs(const uint64_t* rec_off, const std::vector<uint32_t>& jobs) {
  SlotMaps m;
  for (uint32_t j : jobs)
    for (uint64_t r = rec_off[j]; r < rec_off[j + 1]; r++) {
      m.record.push_back((uint32_t)r);
      m.job.push_back(j);
    }
  return m;
}

}  // namespace tc
