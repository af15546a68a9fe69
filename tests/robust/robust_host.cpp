// TEST HARNESS ONLY (tests/test_robust_host.py).  Compiles tc_robust.h -- the share selection of the robust combiners, the
// routine every lane of k_select_shares runs -- with g++.  Never linked into libtc_amd.so.  With -DRH_MAIN it is a stand-alone
// program (for a sanitizer build: g++ -fsanitize=address,undefined -DRH_MAIN) that runs the routine once over fixed inputs.
#include "tc_robust.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
// The masks are copied to `offset` bytes past an 8-byte boundary (separately for the two rows), so that the word loads of
// select_first are exercised at every alignment.  idx_out / slot_out hold cap entries each; the caller pre-fills them and
// checks that nothing past the returned count changed.
size_t rh_select_first(const uint8_t* present, size_t present_offset, const uint8_t* bad, size_t bad_offset, size_t N, size_t need,
                       uint64_t* idx_out, uint32_t* slot_out) {
  std::vector<uint64_t> pbuf((N + 31) / 8 + 2), bbuf((N + 31) / 8 + 2);
  uint8_t* p = present ? reinterpret_cast<uint8_t*>(pbuf.data()) + (present_offset & 7) : nullptr;
  uint8_t* b = bad ? reinterpret_cast<uint8_t*>(bbuf.data()) + (bad_offset & 7) : nullptr;
  // bytes around the row are all ones / all zeros the wrong way round: a read outside the row would change the answer
  memset(pbuf.data(), 0xff, pbuf.size() * 8);
  memset(bbuf.data(), 0x00, bbuf.size() * 8);
  if (p) memcpy(p, present, N);
  if (b) memcpy(b, bad, N);
  return select_first(p, b, N, need, idx_out, slot_out);
}
}

#if defined(RH_MAIN)
int main() {
  int rc = 0;
  for (size_t N : {1, 7, 8, 9, 10, 64, 65, 200})
    for (size_t off = 0; off < 8; off++) {
      std::vector<uint8_t> present(N), bad(N);
      for (size_t i = 0; i < N; i++) {
        present[i] = (i * 7 + off) % 3 ? 1 : 0;
        bad[i] = (i * 5 + off) % 4 ? 0 : 1;
      }
      for (size_t need : {(size_t)1, N, N + 1}) {
        std::vector<uint64_t> idx(need + 1, ~0ull);
        std::vector<uint32_t> slot(need + 1, ~0u);
        const size_t got = rh_select_first(present.data(), off, bad.data(), (off + N) & 7, N, need, idx.data(), slot.data());
        size_t want = 0;
        for (size_t i = 0; i < N && want < need; i++)
          if (present[i] && !bad[i]) {
            rc |= (want < got && idx[want] == i && slot[want] == i) ? 0 : 1;
            want++;
          }
        rc |= got == want ? 0 : 1;
        rc |= (idx[got] == ~0ull && slot[got] == ~0u) ? 0 : 1;
      }
    }
  printf("robust_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
