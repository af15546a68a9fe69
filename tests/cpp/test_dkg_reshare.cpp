// The DKG resharing through the C++ host mirror (include/threshold_crypto.hpp dkg_reshare), built and run by
// tests/test_gpu_cpp_dkg_reshare.py, which writes the fixture: u32 t_old, degree, P, n_v; the old commitment (t_old+1 points); P u64
// dealer indices; P accept bytes; P commitments of (degree+1)(degree+2)/2 points; P x n_v u64 abscissae; P x n_v values; the
// expected commitment (degree+1 points), share and P used bytes.
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
  std::uint64_t u64() {
    auto b = take<8>();
    std::uint64_t v;
    std::memcpy(&v, b.data(), 8);
    return v;
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
  const std::size_t t_old = r.u32(), degree = r.u32(), P = r.u32(), nv = r.u32(), n = degree + 1, nco = n * (n + 1) / 2;
  std::vector<G1Bytes> old_commit(t_old + 1);
  for (auto& pt : old_commit) pt = r.take<96>();
  std::vector<std::uint64_t> idx(P);
  for (auto& i : idx) i = r.u64();
  std::vector<bool> accept(P);
  for (std::size_t p = 0; p < P; p++) accept[p] = r.take<1>()[0] != 0;
  std::vector<std::vector<G1Bytes>> commits(P, std::vector<G1Bytes>(nco));
  for (auto& c : commits)
    for (auto& pt : c) pt = r.take<96>();
  std::vector<std::vector<std::uint64_t>> xs(P, std::vector<std::uint64_t>(nv));
  for (auto& row : xs)
    for (auto& x : row) x = r.u64();
  std::vector<std::vector<FrBytes>> vals(P, std::vector<FrBytes>(nv));
  for (auto& row : vals)
    for (auto& v : row) v = r.take<32>();
  std::vector<G1Bytes> want_commit(n);
  for (auto& pt : want_commit) pt = r.take<96>();
  const FrBytes want_share = r.take<32>();
  std::vector<bool> want_used(P);
  for (std::size_t p = 0; p < P; p++) want_used[p] = r.take<1>()[0] != 0;
  EXPECT(r.pos == r.d.size());

  FrBytes share;
  std::vector<bool> used;
  EXPECT(dkg_reshare(old_commit, idx, commits, degree, accept, &xs, &vals, &share, &used) == want_commit);
  EXPECT(share == want_share && used == want_used);
  EXPECT(want_commit[0] == old_commit[0]);                                              // the master key does not move
  EXPECT(dkg_reshare(old_commit, idx, commits, degree, accept) == want_commit);         // an observer without a secret
  // a rejected dealer's commitment is never used; accepted, the same bytes fail the call
  std::vector<std::vector<G1Bytes>> junk = commits;
  for (std::size_t p = 0; p < P; p++)
    if (!accept[p])
      for (auto& pt : junk[p]) pt.fill(0xA5);
  EXPECT(dkg_reshare(old_commit, idx, junk, degree, accept, &xs, &vals, &share) == want_commit && share == want_share);
  bool threw = false;
  try {
    dkg_reshare(old_commit, idx, junk, degree);
  } catch (const FromBytesError&) {
    threw = true;
  }
  EXPECT(threw);
  // a dealer whose constant term is another node's share
  std::vector<std::vector<G1Bytes>> swapped = commits;
  std::size_t a = P, b = P;
  for (std::size_t p = 0; p < P; p++)
    if (accept[p]) (a == P ? a : b) = p;
  EXPECT(a != P && b != P);
  std::swap(swapped[a][0], swapped[b][0]);
  threw = false;
  try {
    dkg_reshare(old_commit, idx, swapped, degree, accept);
  } catch (const ShareMismatch&) {
    threw = true;
  }
  EXPECT(threw);
  // the same dealer twice
  std::vector<std::uint64_t> twice = idx;
  twice[b] = twice[a];
  threw = false;
  try {
    dkg_reshare(old_commit, twice, commits, degree, accept);
  } catch (const ErrorException& e) {
    threw = e.code == Error::DuplicateEntry;
  }
  EXPECT(threw);
  // too few accepted parts
  std::vector<bool> one(P, false);
  one[a] = true;
  threw = false;
  try {
    dkg_reshare(old_commit, idx, commits, degree, one);
  } catch (const ErrorException& e) {
    threw = e.code == Error::NotEnoughShares;
  }
  EXPECT(threw);
  std::printf("CPP-RESHARE-OK\n");
  return 0;
}
