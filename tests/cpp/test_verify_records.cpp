// Batch verification under many keys through the C++ mirror (include/threshold_crypto.hpp): PublicKey::verify_records_batch over
// a fixture written by tests/test_gpu_cpp_verify_records.py -- per message its text and its (key, signature, expected answer)
// records, then the expected fallback count.  Prints CPP-VERIFY-RECORDS-OK.
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

#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAILED line %d: %s (message %zu)\n", __LINE__, #c, m); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  Reader r;
  r.b.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  const std::size_t M = r.u32(), group = r.u32();
  std::vector<std::vector<std::pair<PublicKey, Signature>>> records(M);
  std::vector<std::vector<bool>> want(M);
  Messages msgs;
  for (std::size_t m = 0; m < M; m++) {
    msgs.push(r.bytes(r.u32()));
    const std::size_t n = r.u32();
    for (std::size_t k = 0; k < n; k++) {
      PublicKey pk;
      Signature sig;
      std::memcpy(pk.g1.data(), r.bytes(96).data(), 96);
      std::memcpy(sig.g2.data(), r.bytes(192).data(), 192);
      records[m].emplace_back(pk, sig);
      want[m].push_back(r.u8() != 0);
    }
  }
  const std::uint32_t want_fallback = r.u32();
  std::array<std::uint8_t, 32> seed{};
  for (int i = 0; i < 32; i++) seed[i] = (std::uint8_t)(11 * i + 3);
  std::uint64_t fallback = 77;
  const auto got = PublicKey::verify_records_batch(records, msgs, seed, group, &fallback);
  std::size_t m = 0;
  EXPECT(got.size() == M);
  for (m = 0; m < M; m++) EXPECT(got[m] == want[m]);
  m = 0;
  EXPECT(fallback == want_fallback);
  // no record at all: nothing to launch, one empty row per message
  const auto none = PublicKey::verify_records_batch(std::vector<std::vector<std::pair<PublicKey, Signature>>>(M), msgs, seed, group, &fallback);
  EXPECT(none.size() == M && fallback == 0);
  for (m = 0; m < M; m++) EXPECT(none[m].empty());
  std::printf("CPP-VERIFY-RECORDS-OK\n");
  return 0;
}
