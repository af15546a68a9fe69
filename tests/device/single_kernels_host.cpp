// Host leg of the single-point kernel conformance harness (tests/single_conformance.py): the header routines the kernels of
// k_mul.hip, k_hash.hip, k_check.hip and k_robust.hip call -- job_point_mul, job_g1_mul_arena, job_g2_mul_shared,
// job_g2_mul_gather, job_compress, job_decompress and its _x2 form, job_decompress_selected and its _x2 form, the cofactor
// scalings, job_commitment_evaluate, the hashes and their _x2 forms, job_xor_with_hash, job_encrypt, point_in_subgroup, select_first -- run by
// g++ with -DTC_BOUND_CHECK over the same buffers, in the layout of tests/device/single_kernels.hip / single_kernels_mul.hip.
// Each kernel's index map is written here as a plain loop over the lane number round the same body, so the case tables, the
// models and the checkers are proven before any GPU time is spent.  What it cannot see is the kernels' own text (lane pairs,
// the arena, the launch geometry); share / form = 0 (the launcher's rule) exist on the device only and run here as 1.  The
// kernels whose body lives in the __global__ function (k_rlc_scalars*, k_invalidate_jobs, k_ok_and_status, the gather, scatter
// and take kernels, k_robust_mark, k_robust_finish, k_gather_selected) have no header routine and no entry here.
// With -DSK_MAIN it is a stand-alone program over a short fixed case list (for a g++ -fsanitize=address,undefined build).
// Test code only: never linked into libtc_amd.so.
#include "../../threshold_crypto_amd/csrc/tc_jobs.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tc;

namespace {
// record (i / take, i % take) of records that hold n_per_job samples each
size_t take_source(size_t i, size_t n_per_job, size_t take) { return (i / take) * n_per_job + i % take; }
// mask bytes at `off` bytes behind an 8-byte boundary
const uint8_t* place(std::vector<uint64_t>& store, const uint8_t* p, size_t bytes, size_t off) {
  if (!p) return nullptr;
  store.assign((bytes + 16) / 8 + 2, 0x5A5A5A5A5A5A5A5Aull);
  uint8_t* at = reinterpret_cast<uint8_t*>(store.data()) + off;
  memcpy(at, p, bytes);
  return at;
}
}  // namespace

extern "C" {
int skh_point_mul(int kernel, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  if (kernel < 0 || kernel > 5 || !S || !B) return 1;
  const bool g2 = kernel >= 3;
  const bool shared = kernel == 5 || (kernel == 3 && S > 1);
  if (shared) {
    const size_t chunks = (S + kMulShare - 1) / kMulShare;
    for (size_t tid = 0; tid < chunks * B; tid++) {
      const size_t c = tid / B, j = tid % B;
      const size_t s0 = c * kMulShare;
      const int n = (int)((S - s0 < (size_t)kMulShare) ? S - s0 : (size_t)kMulShare);
      const size_t o = j * S + s0;
      job_g2_mul_shared(fr + s0 * 32, n, pts + j * 192, out + o * 192, with_status ? status + o : nullptr, true);
    }
    return 0;
  }
  for (size_t tid = 0; tid < S * B; tid++) {
    const size_t s = tid / B, j = tid % B;
    const size_t o = j * S + s;
    uint8_t st;
    if (g2) st = job_point_mul<Fq2>(fr + s * 32, pts + j * 192, out + o * 192);
    else if (kernel == 2) st = job_g1_mul_arena(fr + s * 32, pts + j * 96, out + o * 96);
    else st = job_point_mul<Fq>(fr + s * 32, pts + j * 96, out + o * 96);
    if (with_status) status[o] = st;
  }
  return 0;
}

int skh_g2_mul_gather(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, size_t share, int with_status,
                      uint8_t* out, uint8_t* status) {
  if (!n || !B || !N || share > (size_t)kGatherShare) return 1;
  if (!share) share = 1;
  const size_t chunks = (n + share - 1) / share;
  for (size_t tid = 0; tid < chunks * B; tid++) {
    const size_t c = tid / B, j = tid % B;
    const size_t s0 = c * share;
    const int cnt = (int)((n - s0 < share) ? n - s0 : share);
    const size_t o = j * n + s0;
    job_g2_mul_gather(sk, N, idx + o, cnt, pts + j * 192, out + o * 192, with_status ? status + o : nullptr, true);
  }
  return 0;
}

int skh_compress(int g2, const uint8_t* in, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  for (size_t j = 0; j < B; j++) {
    const uint8_t st = g2 ? job_compress<Fq2>(in + j * 192, out + j * 96) : job_compress<Fq>(in + j * 96, out + j * 48);
    if (with_status) status[j] = st;
  }
  return 0;
}

int skh_decompress(int g2, int form, const uint8_t* in, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  if (!B || form < 0 || form > 2 || (form == 2 && !g2)) return 1;
  if (form == 2) {
    for (size_t p = 0; 2 * p < B; p++) {
      const size_t ja = 2 * p, jb = 2 * p + 1;
      const bool has_b = jb < B;
      uint8_t sa, sb;
      job_decompress_g2_x2(in + ja * 96, in + (has_b ? jb : ja) * 96, out + ja * 192, has_b ? out + jb * 192 : nullptr, sa, sb);
      if (with_status) {
        status[ja] = sa;
        if (has_b) status[jb] = sb;
      }
    }
    return 0;
  }
  for (size_t j = 0; j < B; j++) {
    const uint8_t st = g2 ? job_decompress<Fq2>(in + j * 96, out + j * 192) : job_decompress<Fq>(in + j * 48, out + j * 96);
    if (with_status) status[j] = st;
  }
  return 0;
}

int skh_decompress_take(int g2, int form, const uint8_t* in, size_t n_per_job, size_t take, size_t B, uint8_t* out, uint8_t* valid) {
  if (!B || !take || take > n_per_job || form < 0 || form > 2 || (form == 2 && !g2)) return 1;
  const size_t n = B * take;
  if (form == 2) {
    for (size_t p = 0; 2 * p < n; p++) {
      const size_t ia = 2 * p;
      const bool has_b = ia + 1 < n;
      const size_t ib = has_b ? ia + 1 : ia;
      uint8_t sa, sb;
      job_decompress_g2_x2(in + take_source(ia, n_per_job, take) * 96, in + take_source(ib, n_per_job, take) * 96, out + ia * 192,
                           has_b ? out + ib * 192 : nullptr, sa, sb);
      valid[ia] = sa == TC_JOB_OK ? 1 : 0;
      if (has_b) valid[ib] = sb == TC_JOB_OK ? 1 : 0;
    }
    return 0;
  }
  for (size_t i = 0; i < n; i++) {
    const size_t src = take_source(i, n_per_job, take);
    const uint8_t st = g2 ? job_decompress<Fq2>(in + src * 96, out + i * 192) : job_decompress<Fq>(in + src * 48, out + i * 96);
    valid[i] = st == TC_JOB_OK ? 1 : 0;
  }
  return 0;
}

int skh_decompress_selected(int g2, int form, const uint8_t* in, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough, size_t jobs,
                            uint8_t* out, uint8_t* ok) {
  if (!jobs || !need || form < 0 || form > 2 || (form == 2 && !g2)) return 1;
  const size_t n = jobs * need;
  if (form == 2) {
    for (size_t p = 0; 2 * p < n; p++) {
      const size_t ia = 2 * p;
      const bool has_b = ia + 1 < n;
      const size_t ib = has_b ? ia + 1 : ia;
      bool oka, okb;
      job_decompress_selected_g2_x2(in, N, need, slot, enough, ia, ib, out + ia * 192, has_b ? out + ib * 192 : nullptr, oka, okb);
      ok[ia] = oka ? 1 : 0;
      if (has_b) ok[ib] = okb ? 1 : 0;
    }
    return 0;
  }
  for (size_t i = 0; i < n; i++) {
    const bool good = g2 ? job_decompress_selected<Fq2>(in, N, need, slot, enough, i, out + i * 192)
                         : job_decompress_selected<Fq>(in, N, need, slot, enough, i, out + i * 96);
    ok[i] = good ? 1 : 0;
  }
  return 0;
}

int skh_small(int what, const uint8_t* in, size_t in_bytes, size_t stride, size_t n, uint8_t* out) {
  if (what < 0 || what > 1) return 1;
  for (size_t j = 0; j < n; j++) {
    if (what == 0) job_fr_scale_cofactor_fix(in + j * 32, out + j * 32);
    else job_g1_scale_cofactor_fix(in + j * stride, out + j * 96);
  }
  return 0;
}

int skh_commitment_evaluate(const uint8_t* commit, size_t t, const uint64_t* idx, size_t M, int with_status, uint8_t* out, uint8_t* status) {
  for (size_t j = 0; j < M; j++) {
    const uint8_t st = job_commitment_evaluate(commit, (int)t, idx[j], out + j * 96);
    if (with_status) status[j] = st;
  }
  return 0;
}

int skh_hash(const uint8_t* g1, const uint8_t* msgs, const uint64_t* off, size_t B, int fix, int form, int with_status, uint8_t* out, uint8_t* status) {
  if (!B || form < 0 || form > 2) return 1;
  if (form == 2) {
    for (size_t p = 0; 2 * p < B; p++) {
      const size_t ja = 2 * p;
      const bool has_b = ja + 1 < B;
      const size_t jb = has_b ? ja + 1 : ja;
      uint8_t sa = 0, sb = 0;
      if (g1)
        job_hash_g1_g2_x2(g1 + ja * 96, msgs + off[ja], (size_t)(off[ja + 1] - off[ja]), g1 + jb * 96, msgs + off[jb], (size_t)(off[jb + 1] - off[jb]),
                          out + ja * 192, has_b ? out + jb * 192 : nullptr, fix != 0, sa, sb);
      else
        job_hash_g2_x2(msgs + off[ja], (size_t)(off[ja + 1] - off[ja]), msgs + off[jb], (size_t)(off[jb + 1] - off[jb]), out + ja * 192,
                       has_b ? out + jb * 192 : nullptr, fix != 0);
      if (g1 && with_status) {
        status[ja] = sa;
        if (has_b) status[jb] = sb;
      }
    }
    return 0;
  }
  for (size_t j = 0; j < B; j++) {
    const size_t len = (size_t)(off[j + 1] - off[j]);
    if (g1) {
      const uint8_t st = job_hash_g1_g2(g1 + j * 96, msgs + off[j], len, out + j * 192, fix != 0);
      if (with_status) status[j] = st;
    } else {
      job_hash_g2(msgs + off[j], len, out + j * 192, fix != 0);
    }
  }
  return 0;
}

int skh_xor_with_hash(const uint8_t* g1, const uint8_t* data, const uint64_t* off, size_t B, uint8_t* status, uint8_t* out) {
  for (size_t j = 0; j < B; j++) {
    if (status && status[j] != TC_JOB_OK) continue;
    const uint8_t st = job_xor_with_hash(g1 + j * 96, data + off[j], (size_t)(off[j + 1] - off[j]), out + off[j]);
    if (status) status[j] = st;
  }
  return 0;
}

int skh_encrypt(const uint8_t* pk, size_t pk_stride, const uint8_t* r, const uint8_t* msgs, const uint64_t* off, size_t B, int with_status, uint8_t* u,
                uint8_t* v, uint8_t* w, uint8_t* status) {
  for (size_t j = 0; j < B; j++) {
    const uint8_t st = job_encrypt(pk + j * pk_stride, r + j * 32, msgs + off[j], (size_t)(off[j + 1] - off[j]), u + j * 96, v + off[j], w + j * 192);
    if (with_status) status[j] = st;
  }
  return 0;
}

int skh_subgroup_check(int g2, const uint8_t* pts, size_t pts_bytes, size_t stride, size_t n_per_job, size_t take, size_t n, uint8_t* valid) {
  if (!n || !take || take > n_per_job) return 1;
  for (size_t i = 0; i < n; i++) {
    const uint8_t* at = pts + take_source(i, n_per_job, take) * stride;
    bool ok;
    if (g2) {
      G2Affine p;
      ok = g2_decode_uncompressed(at, p);
      if (!ok) p = G2Affine::infinity();
      ok = ok && point_in_subgroup(p);
    } else {
      G1Affine p;
      ok = g1_decode_uncompressed(at, p);
      if (!ok) p = G1Affine::infinity();
      ok = ok && point_in_subgroup(p);
    }
    valid[i] = ok ? 1 : 0;
  }
  return 0;
}

int skh_select_shares(const uint8_t* present, const uint8_t* bad, size_t off_p, size_t off_b, size_t N, size_t need, size_t jobs, const uint32_t* map,
                      size_t used_rows, uint64_t* idx, uint32_t* slot, uint8_t* used, uint8_t* enough) {
  if (off_p > 15 || off_b > 15 || need > N || (used && !map && used_rows < jobs)) return 1;
  std::vector<uint64_t> sp, sb;
  const uint8_t* p = place(sp, present, jobs * N, off_p);
  const uint8_t* b = place(sb, bad, jobs * N, off_b);
  for (size_t j = 0; j < jobs; j++) {
    uint64_t* my_idx = idx + j * need;
    uint32_t* my_slot = slot + j * need;
    const size_t count = select_first(p ? p + j * N : nullptr, b ? b + j * N : nullptr, N, need, my_idx, my_slot);
    for (size_t k = count; k < need; k++) {
      my_idx[k] = (uint64_t)(N + k);
      my_slot[k] = 0xffffffffu;
    }
    const bool full = count == need;
    enough[j] = full ? 1 : 0;
    if (used && full) {
      uint8_t* row = used + (size_t)(map ? map[j] : (uint32_t)j) * N;
      for (size_t k = 0; k < need; k++) row[my_slot[k]] = 1;
    }
  }
  return 0;
}
}  // extern "C"

#if defined(SK_MAIN)
static void le32(uint64_t v, uint8_t* out) {
  memset(out, 0, 32);
  for (int b = 0; b < 8; b++) out[b] = (uint8_t)(v >> (8 * b));
}
// [k] g1 by plain double-and-add (k >= 1), not by the GLV ladder under test
static void gen1(uint64_t k, uint8_t* out96) {
  const G1Jac base = G1Jac::from_affine(g1_generator());
  G1Jac acc = base;
  int bit = 63;
  while (!((k >> bit) & 1)) bit--;
  for (bit--; bit >= 0; bit--) {
    acc = jac_dbl(acc);
    if ((k >> bit) & 1) acc = jac_add(acc, base);
  }
  g1_encode_uncompressed(jac_to_affine(acc), out96);
}
// a point of G2: the hash of a one-byte message
static void some_g2(uint8_t* out192) {
  const uint8_t msg[1] = {7};
  job_hash_g2(msg, 1, out192, true);
}
static bool poison(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (p[i] != 0x5A) return false;
  return true;
}
int main() {
  int rc = 0, seen = 0;
  auto mark = [&](const char* what) {
    if (rc != seen) printf("single_kernels_host: %s failed\n", what);
    seen = rc;
  };
  // G1 products: S = 2 signers x B = 3 points, the register and the arena form agree with the 64-bit ladder; a bad scalar fails
  // its column
  {
    const size_t S = 3, B = 3, n = S * B;
    const uint64_t k[S] = {5, 0xffffffffffffull, 0}, m[B] = {1, 7, 11};
    std::vector<uint8_t> fr(S * 32), pts(B * 96), a((n + 1) * 96, 0x5A), b((n + 1) * 96, 0x5A), sa(n + 1, 0x5A), sb(n + 1, 0x5A), want(96);
    for (size_t s = 0; s < S; s++) le32(k[s], fr.data() + s * 32);
    memset(fr.data() + 2 * 32, 0xff, 32);
    for (size_t j = 0; j < B; j++) gen1(m[j], pts.data() + j * 96);
    rc |= skh_point_mul(1, fr.data(), pts.data(), S, B, 1, a.data(), sa.data());
    rc |= skh_point_mul(2, fr.data(), pts.data(), S, B, 1, b.data(), sb.data());
    rc |= (a == b && sa == sb && poison(a.data() + n * 96, 96) && sa[n] == 0x5A) ? 0 : 1;
    for (size_t j = 0; j < B; j++)
      for (size_t s = 0; s < 2; s++) {
        gen1(m[j] * k[s], want.data());
        rc |= (memcmp(want.data(), a.data() + (j * S + s) * 96, 96) == 0 && sa[j * S + s] == TC_JOB_OK) ? 0 : 1;
      }
    for (size_t j = 0; j < B; j++) rc |= (sa[j * S + 2] == TC_JOB_INVALID_ENCODING && a[(j * S + 2) * 96] == 0x40) ? 0 : 1;
  }
  mark("G1 products");
  // G2: the shared form at S = 5 (a full and a ragged chunk) and the gather at every share leave the bytes of k_point_mul<Fq2>
  {
    const size_t S = 5, B = 2, n = S * B;
    std::vector<uint8_t> fr(S * 32), pts(B * 192), a((n + 1) * 192, 0x5A), b((n + 1) * 192, 0x5A), sa(n + 1, 0x5A), sb(n + 1, 0x5A);
    for (size_t s = 0; s < S; s++) le32(3 + 1000003ull * s, fr.data() + s * 32);
    memset(fr.data() + 32, 0, 32);        // a scalar 0: an identity inside the shared inversion
    memset(fr.data() + 4 * 32, 0xff, 32);  // a non-canonical one in the ragged chunk
    some_g2(pts.data());
    {
      uint8_t two[32];
      le32(2, two);
      rc |= job_point_mul<Fq2>(two, pts.data(), pts.data() + 192) == TC_JOB_OK ? 0 : 1;
    }
    rc |= skh_point_mul(4, fr.data(), pts.data(), S, B, 1, a.data(), sa.data());
    rc |= skh_point_mul(5, fr.data(), pts.data(), S, B, 1, b.data(), sb.data());
    rc |= (a == b && sa == sb && sa[1] == TC_JOB_OK && a[192] == 0x40 && sa[4] == TC_JOB_INVALID_ENCODING) ? 0 : 1;
    std::vector<uint64_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = i % S;
    idx[3] = S;  // an index >= N
    std::vector<uint8_t> first;
    for (size_t share = 1; share <= (size_t)kGatherShare; share++) {
      std::vector<uint8_t> g((n + 1) * 192, 0x5A), sg(n + 1, 0x5A);
      rc |= skh_g2_mul_gather(fr.data(), S, idx.data(), pts.data(), S, B, share, 1, g.data(), sg.data());
      if (first.empty()) first = g;
      rc |= (g == first && poison(g.data() + n * 192, 192) && sg[n] == 0x5A && sg[3] == TC_JOB_INVALID_ENCODING) ? 0 : 1;
      rc |= (memcmp(g.data(), a.data(), 3 * 192) == 0 && memcmp(g.data() + 5 * 192, a.data() + 5 * 192, 3 * 192) == 0) ? 0 : 1;
    }
  }
  mark("G2 products");
  // decoders: compress, decompress (both forms), take (5, 3) with garbage behind `take`, the selected decode with a job without shares
  {
    const size_t npj = 5, take = 3, B = 3, n = B * take;
    std::vector<uint8_t> p1(96), p2(192), c1(B * npj * 48, 0xEE), c2(B * npj * 96, 0xEE), st(2, 0x5A);
    for (size_t i = 0; i < B * npj; i++) {
      if (i % npj >= take) continue;
      gen1(i + 2, p1.data());
      rc |= skh_compress(0, p1.data(), 1, 1, c1.data() + i * 48, st.data());
      uint8_t k[32];
      le32(i + 2, k);
      std::vector<uint8_t> g(192);
      some_g2(g.data());
      rc |= job_point_mul<Fq2>(k, g.data(), p2.data()) == TC_JOB_OK ? 0 : 1;
      rc |= skh_compress(1, p2.data(), 1, 1, c2.data() + i * 96, st.data());
    }
    std::vector<uint8_t> o1((n + 1) * 96, 0x5A), o2((n + 1) * 192, 0x5A), o3((n + 1) * 192, 0x5A), v1(n + 1, 0x5A), v2(n + 1, 0x5A), v3(n + 1, 0x5A);
    rc |= skh_decompress_take(0, 1, c1.data(), npj, take, B, o1.data(), v1.data());
    rc |= skh_decompress_take(1, 1, c2.data(), npj, take, B, o2.data(), v2.data());
    rc |= skh_decompress_take(1, 2, c2.data(), npj, take, B, o3.data(), v3.data());
    rc |= (o2 == o3 && v2 == v3 && v1 == v2 && poison(o1.data() + n * 96, 96) && poison(o3.data() + n * 192, 192) && v3[n] == 0x5A) ? 0 : 1;
    for (size_t i = 0; i < n; i++) rc |= v1[i] == 1 ? 0 : 1;
    gen1(5 + 2, p1.data());  // record 1, sample 0 = source 5
    rc |= memcmp(p1.data(), o1.data() + 3 * 96, 96) ? 1 : 0;
    // selected: N = 5 (the same arrays), need = 2; job 1 has no shares
    const uint32_t slot[6] = {2, 0, 0xffffffffu, 0xffffffffu, 1, 2};
    const uint8_t enough[3] = {1, 0, 1};
    std::vector<uint8_t> s1(7 * 96, 0x5A), s2(7 * 192, 0x5A), s3(7 * 192, 0x5A), k1(7, 0x5A), k2(7, 0x5A), k3(7, 0x5A);
    rc |= skh_decompress_selected(0, 1, c1.data(), npj, 2, slot, enough, 3, s1.data(), k1.data());
    rc |= skh_decompress_selected(1, 1, c2.data(), npj, 2, slot, enough, 3, s2.data(), k2.data());
    rc |= skh_decompress_selected(1, 2, c2.data(), npj, 2, slot, enough, 3, s3.data(), k3.data());
    rc |= (s2 == s3 && k2 == k3 && k1 == k2 && s1[2 * 96] == 0x40 && s1[3 * 96] == 0x40 && poison(s1.data() + 6 * 96, 96)) ? 0 : 1;
    gen1(2 + 2, p1.data());
    rc |= memcmp(p1.data(), s1.data(), 96) ? 1 : 0;
  }
  mark("decoders");
  // selection: both paths of select_first over rows at odd offsets, used rows through a map
  {
    const size_t N = 17, need = 3, jobs = 4;
    std::vector<uint8_t> present(jobs * N, 1), bad(jobs * N, 0);
    present[0] = 0;
    bad[1] = 1;
    for (size_t i = 0; i < N; i++) present[2 * N + i] = i == 16;  // job 2: one share
    const uint32_t map[jobs] = {3, 2, 1, 0};
    std::vector<uint8_t> first;
    for (size_t off_b = 3; off_b <= 4; off_b++) {
      std::vector<uint64_t> idx(jobs * need + 1, 0x5A5A5A5A5A5A5A5Aull);
      std::vector<uint32_t> slot(jobs * need + 1, 0x5A5A5A5Au);
      std::vector<uint8_t> used(jobs * N + 1, 0), enough(jobs + 1, 0x5A);
      rc |= skh_select_shares(present.data(), bad.data(), 3, off_b, N, need, jobs, map, jobs, idx.data(), slot.data(), used.data(), enough.data());
      rc |= (slot[0] == 2 && slot[2] == 4 && enough[2] == 0 && slot[6] == 16 && slot[7] == 0xffffffffu && idx[8] == N + 2 && used[3 * N + 2] == 1 &&
             used[1 * N + 16] == 0 && slot[jobs * need] == 0x5A5A5A5Au && used[jobs * N] == 0 && enough[jobs] == 0x5A)
                ? 0
                : 1;
      if (first.empty()) first = used;
      rc |= first == used ? 0 : 1;
    }
  }
  mark("selection");
  // Commitment::evaluate at t = 2: c0 + c1 x + c2 x^2 with c = (3, 5, 7) g1 at x = 1, 2; idx = 2^64 - 1 is invalid
  {
    std::vector<uint8_t> c(3 * 96), out(4 * 96, 0x5A), st(4, 0x5A), want(96);
    gen1(3, c.data());
    gen1(5, c.data() + 96);
    gen1(7, c.data() + 192);
    const uint64_t idx[3] = {0, 1, ~0ull};
    rc |= skh_commitment_evaluate(c.data(), 2, idx, 3, 1, out.data(), st.data());
    gen1(15, want.data());
    rc |= memcmp(want.data(), out.data(), 96) ? 1 : 0;
    gen1(3 + 10 + 28, want.data());
    rc |= (memcmp(want.data(), out.data() + 96, 96) == 0 && st[2] == TC_JOB_INVALID_ENCODING && out[192] == 0x40 && poison(out.data() + 288, 96)) ? 0 : 1;
  }
  mark("commitment evaluation");
  // hashes: the two-job form leaves the one-job bytes; the keystream XOR is an involution
  {
    const size_t B = 3;
    const uint64_t off[B + 1] = {0, 0, 1, 138};
    std::vector<uint8_t> msgs(138), g1(B * 96), a((B + 1) * 192, 0x5A), b((B + 1) * 192, 0x5A), sa(B + 1, 0x5A), sb(B + 1, 0x5A);
    for (size_t i = 0; i < msgs.size(); i++) msgs[i] = (uint8_t)(i * 7 + 1);
    for (size_t j = 0; j < B; j++) gen1(j + 9, g1.data() + j * 96);
    g1[96] = 0x1f;  // x >= q: the operand does not decode
    for (int with_g1 = 0; with_g1 < 2; with_g1++) {
      rc |= skh_hash(with_g1 ? g1.data() : nullptr, msgs.data(), off, B, 1, 1, 1, a.data(), sa.data());
      rc |= skh_hash(with_g1 ? g1.data() : nullptr, msgs.data(), off, B, 1, 2, 1, b.data(), sb.data());
      rc |= (a == b && sa == sb && poison(a.data() + B * 192, 192)) ? 0 : 1;
    }
    rc |= sa[1] == TC_JOB_INVALID_ENCODING ? 0 : 1;
    std::vector<uint8_t> x(139, 0x5A), y(139, 0x5A), st(B + 1, 0);
    rc |= skh_xor_with_hash(g1.data(), msgs.data(), off, B, st.data(), x.data());
    rc |= (st[1] == TC_JOB_INVALID_ENCODING && st[2] == TC_JOB_OK && x[138] == 0x5A) ? 0 : 1;
    st[1] = 0;
    g1[96] = 0;
    gen1(10, g1.data() + 96);
    rc |= skh_xor_with_hash(g1.data(), x.data(), off, B, st.data(), y.data());
    rc |= memcmp(y.data() + 1, msgs.data() + 1, 137) ? 1 : 0;
  }
  mark("hashes");
  printf(rc ? "single_kernels_host: FAILED\n" : "single_kernels_host: ok\n");
  return rc;
}
#endif
