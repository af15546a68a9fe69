// The decryption shares of many holders through the C++ host mirror (include/threshold_crypto.hpp decrypt_shares_batch), built and
// run by tests/test_gpu_cpp_decrypt_shares.py, which writes the fixture: u32 S, B; S secret key shares (32 B); per ciphertext u
// (96 B), u32 length of v, v, w (192 B); then B expected ok bytes and, for every valid ciphertext, its S expected shares (96 B).
#include <cstdio>
#include <fstream>
#include <iterator>
#include "threshold_crypto.hpp"

using namespace threshold_crypto;

struct Reader {
  std::vector<std::uint8_t> d;
  std::size_t pos = 0;
  std::uint32_t u32() {
    std::uint32_t v;
    std::memcpy(&v, &d.at(pos + 3) - 3, 4);
    pos += 4;
    return v;
  }
  template <std::size_t N>
  std::array<std::uint8_t, N> take() {
    std::array<std::uint8_t, N> a;
    std::memcpy(a.data(), &d.at(pos + N - 1) - (N - 1), N);
    pos += N;
    return a;
  }
};

#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #c); \
      return 1;                                           \
    }                                                     \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  Reader r;
  r.d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  const std::size_t S = r.u32(), B = r.u32();
  std::vector<SecretKeyShare> keys;
  for (std::size_t s = 0; s < S; s++) keys.emplace_back(r.take<32>());
  std::vector<Ciphertext> cts(B);
  for (auto& ct : cts) {
    ct.u = r.take<96>();
    const std::size_t len = r.u32();
    for (std::size_t i = 0; i < len; i++) ct.v.push_back(r.take<1>()[0]);
    ct.w = r.take<192>();
  }
  std::vector<bool> want_ok(B);
  for (std::size_t j = 0; j < B; j++) want_ok[j] = r.take<1>()[0] != 0;
  std::vector<std::vector<G1Bytes>> want(B);
  for (std::size_t j = 0; j < B; j++)
    if (want_ok[j])
      for (std::size_t s = 0; s < S; s++) want[j].push_back(r.take<96>());
  EXPECT(r.pos == r.d.size());

  std::vector<const SecretKeyShare*> holders;
  for (auto& k : keys) holders.push_back(&k);
  const auto rows = decrypt_shares_batch(holders, cts);
  EXPECT(rows.size() == B);
  std::size_t valid = 0;
  for (std::size_t j = 0; j < B; j++) {
    EXPECT(rows[j].has_value() == want_ok[j]);
    if (!want_ok[j]) continue;
    valid++;
    EXPECT(rows[j]->size() == S);
    for (std::size_t s = 0; s < S; s++) EXPECT((*rows[j])[s].g1 == want[j][s]);
  }
  EXPECT(valid > 0 && valid < B);
  // the same holder by holder: SecretKeyShare::decrypt_share
  for (std::size_t j = 0; j < B && j < 3; j++)
    for (std::size_t s = 0; s < S; s++) {
      const auto one = keys[s].decrypt_share(cts[j]);
      EXPECT(one.has_value() == want_ok[j]);
      if (one) EXPECT(one->g1 == (*rows[j])[s].g1);
    }
  // nothing to do: no holders, no ciphertexts
  EXPECT(decrypt_shares_batch({}, cts).size() == B && !decrypt_shares_batch({}, cts)[0].has_value());
  EXPECT(decrypt_shares_batch(holders, {}).empty());
  std::printf("CPP-DECRYPT-SHARES-OK\n");
  return 0;
}
