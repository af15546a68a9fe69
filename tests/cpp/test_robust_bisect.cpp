// Blame by bisection through the C++ mirror (include/threshold_crypto.hpp): set_blame_bisect / blame_bisect / last_blame_stats
// around PublicKeySet::combine_signatures_robust_batch and ::decrypt_robust_batch, over a fixture written by
// tests/test_gpu_cpp_robust_bisect.py (key set, shares with planted faults, the statuses / used / bad indices / results the rules
// of include/tc_amd.h demand, and the pairing checks / rounds the rule of csrc/tc_blame.h demands).  Every half runs with the mode
// off, then on: the same results, the stats of each mode.  Prints CPP-ROBUST-BISECT-OK.
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
  std::vector<std::uint64_t> indices(std::size_t N) {
    std::vector<std::uint64_t> out;
    for (std::size_t i = 0; i < N; i++)
      if (u8()) out.push_back(i);
    return out;
  }
};

#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAILED line %d: %s (job %zu)\n", __LINE__, #c, j); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  Reader r;
  r.b.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  const std::size_t t = r.u32(), N = r.u32(), B = r.u32();
  std::vector<G1Bytes> commit(t + 1);
  for (auto& c : commit) std::memcpy(c.data(), r.bytes(96).data(), 96);
  PublicKeySet pks(commit);
  std::array<std::uint8_t, 32> seed{}, key{};
  for (int i = 0; i < 32; i++) seed[i] = (std::uint8_t)(7 * i + 1), key[i] = (std::uint8_t)(11 * i + 3);
  {
    std::size_t j = 0;
    EXPECT(!blame_bisect());
  }

  // signatures
  {
    std::vector<std::map<std::uint64_t, SignatureShare>> jobs(B);
    Messages msgs;
    std::vector<PublicKeySet::RobustResult> want(B);
    std::vector<Bytes> want_sig(B);
    for (std::size_t j = 0; j < B; j++) {
      msgs.push(r.bytes(r.u32()));
      for (std::size_t i = 0; i < N; i++) {
        const bool present = r.u8() != 0;
        const Bytes s = r.bytes(192);
        if (present) std::memcpy(jobs[j][i].sig.g2.data(), s.data(), 192);
      }
      want[j].status = r.u8();
      want[j].used = r.indices(N);
      want[j].bad = r.indices(N);
      want_sig[j] = r.bytes(192);
    }
    const std::uint32_t want_fallback = r.u32(), want_checks = r.u32(), want_rounds = r.u32();
    for (int mode = 0; mode < 2; mode++) {
      set_blame_bisect(mode ? &key : nullptr);
      std::vector<PublicKeySet::RobustResult> got;
      std::uint64_t fallback = 0;
      auto sigs = pks.combine_signatures_robust_batch(jobs, msgs, N, seed, got, &fallback);
      for (std::size_t j = 0; j < B; j++) {
        EXPECT(got[j].status == want[j].status);
        EXPECT(got[j].used == want[j].used);
        EXPECT(got[j].bad == want[j].bad);
        EXPECT(std::memcmp(sigs[j].g2.data(), want_sig[j].data(), 192) == 0);
      }
      std::size_t j = (std::size_t)mode;
      EXPECT(blame_bisect() == (mode != 0));
      EXPECT(fallback == want_fallback);
      const BlameStats s = last_blame_stats();
      EXPECT(s.pairing_checks == (mode ? want_checks : want_fallback * N));
      EXPECT(s.rounds == (mode ? want_rounds : (want_fallback ? 1u : 0u)));
    }
  }
  // decryption
  {
    std::vector<std::map<std::uint64_t, DecryptionShare>> jobs(B);
    std::vector<Ciphertext> cts(B);
    std::vector<PublicKeySet::RobustResult> want(B);
    std::vector<Bytes> want_plain(B);
    for (std::size_t j = 0; j < B; j++) {
      std::memcpy(cts[j].u.data(), r.bytes(96).data(), 96);
      cts[j].v = r.bytes(r.u32());
      std::memcpy(cts[j].w.data(), r.bytes(192).data(), 192);
      for (std::size_t i = 0; i < N; i++) {
        const bool present = r.u8() != 0;
        const Bytes s = r.bytes(96);
        if (present) std::memcpy(jobs[j][i].g1.data(), s.data(), 96);
      }
      want[j].status = r.u8();
      want[j].used = r.indices(N);
      want[j].bad = r.indices(N);
      want_plain[j] = r.bytes(r.u32());
    }
    const std::uint32_t want_fallback = r.u32(), want_checks = r.u32(), want_rounds = r.u32();
    for (int mode = 1; mode >= 0; mode--) {
      set_blame_bisect(mode ? &key : nullptr);
      std::vector<PublicKeySet::RobustResult> got;
      std::uint64_t fallback = 0;
      auto plain = pks.decrypt_robust_batch(jobs, cts, N, got, &fallback);
      for (std::size_t j = 0; j < B; j++) {
        EXPECT(got[j].status == want[j].status);
        EXPECT(got[j].used == want[j].used);
        EXPECT(got[j].bad == want[j].bad);
        EXPECT(plain[j] == (want[j].status == TC_JOB_OK ? want_plain[j] : Bytes()));
      }
      std::size_t j = (std::size_t)mode;
      EXPECT(fallback == want_fallback);
      const BlameStats s = last_blame_stats();
      EXPECT(s.pairing_checks == (mode ? want_checks : want_fallback * N));
      EXPECT(s.rounds == (mode ? want_rounds : (want_fallback ? 1u : 0u)));
    }
  }
  std::printf("CPP-ROBUST-BISECT-OK\n");
  return 0;
}
