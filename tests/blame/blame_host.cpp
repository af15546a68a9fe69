// Host harness of the blame-by-bisection search (tests/test_blame_host.py): threshold_crypto_amd/csrc/tc_blame.h compiled by
// g++ and driven with a TRUTHFUL range oracle -- a range passes iff it holds no slot that is live and bad -- the way
// tc_api.hip drives it with pairing checks.  With -DBH_MAIN it is a stand-alone program over a fixed case list (what a
// g++ -fsanitize=address,undefined build runs).  Test code only: never linked into libtc_amd.so.
#include "tc_blame.h"

#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" {
// present / live / truth (1 = the share is bad): N bytes each; out_bad: N bytes; out2 = {checks, rounds}; returns the number of
// plan() calls that asked for checks with an empty answer list (0 when the engine is consistent)
int bh_search(uint32_t N, const uint8_t* present, const uint8_t* live, const uint8_t* truth, uint8_t* out_bad, uint64_t* out2) {
  tc::BlameSearch s;
  s.start(N, present, live, out_bad);
  std::vector<tc::BlameRange> r;
  std::vector<uint8_t> pass;
  int odd = 0;
  uint64_t rounds = 0, checks = 0;
  for (;;) {
    r.clear();
    const size_t n = s.plan(r);
    if (n != r.size()) odd++;
    if (n == 0) break;
    rounds++;
    checks += n;
    pass.assign(n, 1);
    for (size_t i = 0; i < n; i++) {
      if (r[i].lo >= r[i].hi || r[i].hi > N) odd++;
      for (uint32_t k = r[i].lo; k < r[i].hi && k < N; k++)
        if (present[k] && live[k] && truth[k]) pass[i] = 0;
    }
    s.apply(pass.data());
    if (rounds > 4 * (uint64_t)N + 8) return -1;  // (would never end)
  }
  if (rounds != s.rounds || checks != s.checks) odd++;
  out2[0] = s.checks;
  out2[1] = s.rounds;
  return odd;
}
}

#if defined(BH_MAIN)
static int run(uint32_t N, const std::vector<uint32_t>& bad, uint64_t max_checks, uint64_t max_rounds) {
  std::vector<uint8_t> present(N, 1), live(N, 1), truth(N, 0), out(N, 7);
  for (uint32_t b : bad) truth[b] = 1;
  uint64_t st[2] = {0, 0};
  int rc = bh_search(N, present.data(), live.data(), truth.data(), out.data(), st);
  rc |= memcmp(out.data(), truth.data(), N) ? 1 : 0;
  rc |= (st[0] <= max_checks && st[1] <= max_rounds) ? 0 : 1;
  return rc;
}
int main() {
  int rc = 0;
  rc |= run(1, {}, 1, 1);
  rc |= run(1, {0}, 1, 1);
  rc |= run(10, {3}, 9, 9);
  rc |= run(13, {0, 12}, 17, 9);
  rc |= run(200, {0}, 17, 17);
  rc |= run(200, {199}, 17, 17);
  rc |= run(200, {5, 100, 101}, 49, 17);
  rc |= run(1000, {999}, 21, 21);
  {
    std::vector<uint32_t> all;
    for (uint32_t i = 0; i < 200; i++) all.push_back(i);
    rc |= run(200, all, 399, 17);
  }
  // a present slot that is not live is bad without a check; an absent one is ignored whatever it holds
  {
    const uint32_t N = 6;
    uint8_t present[N] = {1, 0, 1, 1, 0, 1}, live[N] = {1, 0, 0, 1, 1, 1}, truth[N] = {0, 1, 1, 0, 1, 0}, out[N];
    uint64_t st[2];
    rc |= bh_search(N, present, live, truth, out, st);
    const uint8_t want[N] = {0, 0, 1, 0, 0, 0};
    rc |= memcmp(out, want, N) ? 1 : 0;
    rc |= (st[0] == 1 && st[1] == 1) ? 0 : 1;
  }
  printf("blame_host: %s\n", rc ? "FAILED" : "ok");
  return rc ? 1 : 0;
}
#endif
