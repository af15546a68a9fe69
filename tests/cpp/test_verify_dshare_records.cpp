// Decryption-share verification under many key shares through the C++ mirror (include/threshold_crypto.hpp):
// PublicKeyShare::verify_decryption_share_records_batch over a fixture written by tests/test_gpu_cpp_verify_dshare_records.py --
// a number of cases, each: per ciphertext its (u, v, w) and its (key share, decryption share, expected answer) records, then the
// expected fallback count.  Prints CPP-VERIFY-DSHARE-RECORDS-OK.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include "threshold_crypto.hpp"

using namespace threshold_crypto;

struct Reader {
  std::vector<std::uint8_t> b;
  std::size_t pos = 0;
  std::uint32_t u32() {
    std::uint32_t v;
    std::memcpy(&v, &b.at(pos), 4);
    pos += 4;
    return v;
  }
  std::uint8_t u8() { return b.at(pos++); }
  Bytes bytes(std::size_t n) {
    if (pos + n > b.size()) throw std::runtime_error("short fixture");
    Bytes out(b.begin() + pos, b.begin() + pos + n);
    pos += n;
    return out;
  }
};

#define EXPECT(c)                                                                        \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      std::printf("FAILED line %d: %s (case %zu, ciphertext %zu)\n", __LINE__, #c, t, m); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

using Records = std::vector<std::vector<std::pair<PublicKeyShare, DecryptionShare>>>;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  Reader r;
  r.b.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  std::array<std::uint8_t, 32> seed{};
  for (int i = 0; i < 32; i++) seed[i] = (std::uint8_t)(11 * i + 3);
  const std::size_t cases = r.u32();
  std::size_t t = 0, m = 0;
  std::vector<Ciphertext> last_cts;
  for (t = 0; t < cases; t++) {
    const std::size_t M = r.u32(), group = r.u32();
    Records records(M);
    std::vector<std::vector<bool>> want(M);
    std::vector<Ciphertext> cts(M);
    for (m = 0; m < M; m++) {
      std::memcpy(cts[m].u.data(), r.bytes(96).data(), 96);
      cts[m].v = r.bytes(r.u32());
      std::memcpy(cts[m].w.data(), r.bytes(192).data(), 192);
      const std::size_t n = r.u32();
      for (std::size_t k = 0; k < n; k++) {
        PublicKeyShare pk;
        DecryptionShare sh;
        std::memcpy(pk.pk.g1.data(), r.bytes(96).data(), 96);
        std::memcpy(sh.g1.data(), r.bytes(96).data(), 96);
        records[m].emplace_back(pk, sh);
        want[m].push_back(r.u8() != 0);
      }
    }
    const std::uint32_t want_fallback = r.u32();
    std::uint64_t fallback = 77;
    const auto got = PublicKeyShare::verify_decryption_share_records_batch(records, cts, seed, group, &fallback);
    m = 0;
    EXPECT(got.size() == M);
    for (m = 0; m < M; m++) EXPECT(got[m] == want[m]);
    m = 0;
    EXPECT(fallback == want_fallback);
    last_cts = cts;
  }
  // no record at all: nothing to launch, one empty row per ciphertext; no ciphertext at all; a row count that does not match
  m = 0;
  std::uint64_t fallback = 77;
  const auto none = PublicKeyShare::verify_decryption_share_records_batch(Records(last_cts.size()), last_cts, seed, 3, &fallback);
  EXPECT(none.size() == last_cts.size() && fallback == 0);
  for (m = 0; m < none.size(); m++) EXPECT(none[m].empty());
  m = 0;
  fallback = 77;
  EXPECT(PublicKeyShare::verify_decryption_share_records_batch(Records(), std::vector<Ciphertext>(), seed, 0, &fallback).empty() && fallback == 0);
  bool threw = false;
  try {
    PublicKeyShare::verify_decryption_share_records_batch(Records(1), last_cts, seed);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw && last_cts.size() != 1);
  std::printf("CPP-VERIFY-DSHARE-RECORDS-OK\n");
  return 0;
}
