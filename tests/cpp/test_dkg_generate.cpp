// The DKG finalisation through the C++ host mirror (include/threshold_crypto.hpp commitment_sum, dkg_generate), built and run
// by tests/test_gpu_dkg_generate.py, which writes the fixture: u32 degree, P, n_v; P accept bytes; P commitments of
// (degree+1)(degree+2)/2 points; P x n_v u64 abscissae; P x n_v values; the expected commitment (degree+1 points) and share;
// then P commitments as (u32 length, points) and their expected masked sum (degree+1 points).
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
  const std::size_t degree = r.u32(), P = r.u32(), nv = r.u32(), n = degree + 1, nco = n * (n + 1) / 2;
  std::vector<bool> accept(P);
  for (std::size_t p = 0; p < P; p++) accept[p] = r.take<1>()[0] != 0;
  std::vector<std::vector<G1Bytes>> commits(P, std::vector<G1Bytes>(nco));
  for (auto& c : commits)
    for (auto& pt : c) pt = r.take<96>();
  std::vector<std::vector<std::uint64_t>> xs(P, std::vector<std::uint64_t>(nv));
  for (auto& row : xs)
    for (auto& x : row) {
      auto b = r.take<8>();
      std::memcpy(&x, b.data(), 8);
    }
  std::vector<std::vector<FrBytes>> vals(P, std::vector<FrBytes>(nv));
  for (auto& row : vals)
    for (auto& v : row) v = r.take<32>();
  std::vector<G1Bytes> want_commit(n);
  for (auto& pt : want_commit) pt = r.take<96>();
  const FrBytes want_share = r.take<32>();

  FrBytes share;
  EXPECT(dkg_generate(commits, degree, accept, &xs, &vals, &share) == want_commit);
  EXPECT(share == want_share);
  EXPECT(dkg_generate(commits, degree, accept) == want_commit);  // an observer without a secret
  // a rejected dealer's commitment is never used; accepted, the same bytes fail the call
  std::vector<std::vector<G1Bytes>> junk = commits;
  for (std::size_t p = 0; p < P; p++)
    if (!accept[p])
      for (auto& pt : junk[p]) pt.fill(0xA5);
  EXPECT(dkg_generate(junk, degree, accept, &xs, &vals, &share) == want_commit && share == want_share);
  bool threw = false;
  try {
    dkg_generate(junk, degree);
  } catch (const FromBytesError&) {
    threw = true;
  }
  EXPECT(threw);
  // a repeated abscissa in an accepted part
  std::vector<std::vector<std::uint64_t>> dup = xs;
  for (std::size_t p = 0; p < P; p++)
    if (accept[p]) {
      dup[p][nv - 1] = dup[p][0];
      break;
    }
  threw = false;
  try {
    dkg_generate(commits, degree, accept, &dup, &vals, &share);
  } catch (const ErrorException&) {
    threw = true;
  }
  EXPECT(threw);

  std::vector<std::vector<G1Bytes>> rows(P);
  for (auto& row : rows) {
    row.resize(r.u32());
    for (auto& pt : row) pt = r.take<96>();
  }
  std::vector<G1Bytes> want_sum(n);
  for (auto& pt : want_sum) pt = r.take<96>();
  EXPECT(r.pos == r.d.size());
  EXPECT(commitment_sum(rows, accept) == want_sum);
  EXPECT(commitment_sum({}).empty());
  std::printf("CPP-DKG-OK\n");
  return 0;
}
