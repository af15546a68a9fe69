// Job-level routines of blame by bisection (k_blame.hip; the search itself is tc_blame.h): the LEAVES [r] share and
// [r] pk_share of every examined slot, and the sums of leaves over a range of slots.  TC_HD like the other job headers: g++
// compiles them for tests/blame/ (with -DTC_BOUND_CHECK: the interval analysis of the limb arithmetic).
//
// r = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3 with four 16-bit digits, d0 odd, from ChaCha20(key = the call's pass-2 seed, block
// counter = the leaf's number) -- the scalar of k_rlc_scalars (k_check.hip), 2^63 equally likely values.
//   G2: psi = [x] on the subgroup, so [r] P = d0 P + d1 (-psi P) + d2 psi^2 P + d3 (-psi^3 P): the sign-aligned joint ladder of
//       tc_gls.h over 16 columns (sac_recode4(d, 16): the short-scalar mode of the two-stage MSM), 16 doublings.
//   G1: phi' = [x^2], so [r] P = [d0 + d1 |x|] P + [d2 + d3 |x|] phi' P: the base-4 sign-aligned GLV ladder of tc_gls.h over two
//       80-bit halves, 40 steps (tc_msm.h msm_g1_recode's short form).
// A leaf is kept as a Jacobian point in the limb (Montgomery) form of the field code -- no inversion per leaf: 3 (G1) / 6 (G2)
// rows of 16 words, every coordinate multiplied by one first so that its value is a product's (below 2.1 p, what
// tbl_load_fq promises).  A slot that is not live stores the identity (Z = 0).
#pragma once
#include "tc_jobs.h"

namespace tc {

constexpr int kBlameLeafWordsG1 = 3 * kTblCoordWords;  // x, y, z: 192 B
constexpr int kBlameLeafWordsG2 = 6 * kTblCoordWords;  // x, y, z of the even (c0) and the odd (c1) lane: 384 B

TC_HD void blame_store_fq(int32_t* w, const Fq& v) {
  const Fq n = (v * Fq::one()).norm();
#if defined(TC_BOUND_CHECK)
  if (n.val() > 2.1f) tc_bound_fail(n.val(), 0.f);
#endif
  TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) w[i] = n.l[i];
  w[14] = w[15] = 0;
}
TC_HD Fq blame_load_fq(const int32_t* w) { return tbl_load_fq((const tbl_word*)w); }

TC_HD void blame_store_leaf(int32_t* e, const G1Jac& p) {
  blame_store_fq(e, p.x);
  blame_store_fq(e + kTblCoordWords, p.y);
  blame_store_fq(e + 2 * kTblCoordWords, p.z);
}
TC_HD void blame_load_leaf(const int32_t* e, G1Jac& p) {
  p = G1Jac{blame_load_fq(e), blame_load_fq(e + kTblCoordWords), blame_load_fq(e + 2 * kTblCoordWords)};
}
// G2: coordinate c at rows 2c (the even lane's coefficient) and 2c + 1 (the odd lane's)
TC_HD void blame_store_leaf(int32_t* e, const G2Jac& p) {
#if TC_PAIR
  const int o = pair_odd() * kTblCoordWords;
  blame_store_fq(e + o, p.x.m);
  blame_store_fq(e + 2 * kTblCoordWords + o, p.y.m);
  blame_store_fq(e + 4 * kTblCoordWords + o, p.z.m);
#else
  blame_store_fq(e, p.x.c0);
  blame_store_fq(e + kTblCoordWords, p.x.c1);
  blame_store_fq(e + 2 * kTblCoordWords, p.y.c0);
  blame_store_fq(e + 3 * kTblCoordWords, p.y.c1);
  blame_store_fq(e + 4 * kTblCoordWords, p.z.c0);
  blame_store_fq(e + 5 * kTblCoordWords, p.z.c1);
#endif
}
TC_HD void blame_load_leaf(const int32_t* e, G2Jac& p) {
#if TC_PAIR
  const int o = pair_odd() * kTblCoordWords;
  p = G2Jac{Fq2{blame_load_fq(e + o)}, Fq2{blame_load_fq(e + 2 * kTblCoordWords + o)}, Fq2{blame_load_fq(e + 4 * kTblCoordWords + o)}};
#else
  p = G2Jac{Fq2::make(blame_load_fq(e), blame_load_fq(e + kTblCoordWords)),
            Fq2::make(blame_load_fq(e + 2 * kTblCoordWords), blame_load_fq(e + 3 * kTblCoordWords)),
            Fq2::make(blame_load_fq(e + 4 * kTblCoordWords), blame_load_fq(e + 5 * kTblCoordWords))};
#endif
}
template <class F>
struct BlameLeaf;
template <>
struct BlameLeaf<Fq> {
  static constexpr int WORDS = kBlameLeafWordsG1;
};
template <>
struct BlameLeaf<Fq2> {
  static constexpr int WORDS = kBlameLeafWordsG2;
};

// the four digits of leaf number `leaf` under the pass-2 seed (8 key words): k_rlc_scalars' draw
TC_HD void blame_digits(const uint32_t* key8, uint64_t leaf, uint64_t* d) {
  ChaChaRng rng;
  rng.init(key8);
  rng.counter = leaf;
  const uint32_t w0 = rng.next_u32(), w1 = rng.next_u32();
  d[0] = (uint64_t)(w0 & 0xffffu) | 1ull;
  d[1] = (uint64_t)(w0 >> 16);
  d[2] = (uint64_t)(w1 & 0xffffu);
  d[3] = (uint64_t)(w1 >> 16);
}
// The seed of one call's pass 2: the first 32 bytes of ChaCha20(key = the context's key, block counter = the context's call
// counter).  No two calls share a block, so no two calls share a scalar; the caller's seed32 (pass 1) never enters.
TC_HD void blame_call_seed(const uint32_t* ctx_key8, uint64_t call, uint32_t* seed8) {
  ChaChaRng rng;
  rng.init(ctx_key8);
  rng.counter = call;
  TC_UNROLL for (int i = 0; i < 8; i++) seed8[i] = rng.next_u32();
}

// [d0 + d1 |x| + d2 |x|^2 + d3 |x|^3] p in G2 for 16-bit digits (d0 odd): the table of g2_sac_table in this lane pair's arena
// table (the kernel holds a slot), then 16 doublings and 16 mixed additions with every special case handled.  `live` = false
// (or p the identity): the ladder runs over a stand-in -- the table stores and loads are the whole wave's -- and the identity
// is returned.
TC_HD G2Jac blame_leaf_g2(const G2Affine& p_in, bool live, const uint64_t* d) {
  const bool dead = !live || p_in.inf;
  const G2Affine gen{Fq2::make(Fq::from_mont384(G2_GEN_X0), Fq::from_mont384(G2_GEN_X1)),
                     Fq2::make(Fq::from_mont384(G2_GEN_Y0), Fq::from_mont384(G2_GEN_Y1)), false};
  const G2Affine p{Fq2::select(dead, gen.x, p_in.x), Fq2::select(dead, gen.y, p_in.y), false};
  G2Affine base[4];
  g2_gls_bases(p, base);
  G2SacTable t;
  g2_sac_table_call(base, t);
  const SacDigits sd = sac_recode4(d, 16);
  G2Jac acc = G2Jac::from_affine(t.entry(sd.top));
  TC_NOUNROLL for (int bit = 15; bit >= 0; bit--) {
    acc = jac_dbl(acc);
    const uint32_t m = (uint32_t)((sd.u[0] >> bit) & 1) | ((uint32_t)((sd.u[1] >> bit) & 1) << 1) | ((uint32_t)((sd.u[2] >> bit) & 1) << 2);
    G2Affine e = t.entry(m);
    e.y = Fq2::select((sd.neg >> bit) & 1, -e.y, e.y).norm();
    acc = jac_add_mixed(acc, e);
  }
  acc.z = coord_norm(acc.z * t.zc);
  return G2Jac::select(dead, G2Jac::infinity(), acc);
}

// the same scalar on a G1 point: k1 + k2 x^2 with k1 = d0 + d1 |x| (odd) and k2 = d2 + d3 |x|, both below 2^80; the base-4
// sign-aligned ladder of g1_mul_glv_impl (tc_gls.h) cut to 40 steps, its table in this lane's arena table
TC_HD G1Jac blame_leaf_g1(const G1Affine& p_in, bool live, const uint64_t* d) {
  constexpr int kBits = 80;
  const bool dead = !live || p_in.inf;
  const G1Affine g = g1_generator();
  const G1Affine b{Fq::select(dead, g.x, p_in.x), Fq::select(dead, g.y, p_in.y), false};
  const tc_u128 k1 = (tc_u128)d[1] * BLS_X_ABS + d[0];
  tc_u128 k2 = (tc_u128)d[3] * BLS_X_ABS + d[2];
  const tc_u128 neg = ~((k1 | 1) >> 1);
  tc_u128 u = 0;
  TC_NOUNROLL for (int i = 0; i < kBits; i++) {
    const tc_u128 odd = k2 & 1;
    u |= odd << i;
    k2 = (k2 >> 1) + (odd & (neg >> i));
  }
  const bool top = k2 != 0;
  const G1Jac p2 = jac_dbl(G1Jac::from_affine(b));
  const G1Jac p3 = jac_add_mixed(p2, b);
  const Fq beta = Fq::from_limbs(G1_BETA);
  const G1Affine m1{b.x * beta, b.y, false};          // phi(P) = -phi'(P)
  const G1Affine f1{m1.x, (-b.y).norm(), false};      // phi'(P)
  const G1Jac f2{p2.x * beta, (-p2.y).norm(), p2.z};  // phi'(2P)
  const G1Jac f3{p3.x * beta, (-p3.y).norm(), p3.z};  // phi'(3P)
  G1Jac e[7];
  e[0] = jac_add_affine(b, m1);  // 1: P - phi'
  e[1] = jac_add_mixed(f2, b);   // 2: P + 2 phi'
  e[2] = jac_add_affine(b, f1);  // 3: P + phi'
  e[3] = p3;                     // 4: 3P
  e[4] = jac_add_mixed(p3, f1);  // 5: 3P + phi'
  e[5] = jac_add(p3, f2);        // 6: 3P + 2 phi'
  e[6] = jac_add(p3, f3);        // 7: 3P + 3 phi'
  G1Affine tbl[8];
  const Fq zc = jac_batch_to_common_z<Fq, 8>(e, tbl + 1, 7);
  const Fq zc2 = zc.sqr();
  tbl[0] = affine_scale_z(b, zc2, zc2 * zc);
  tbl_word* mem = lane_table();
  TC_UNROLL for (int m = 0; m < 8; m++) tbl_store_g1(mem + m * kG1EntryWords, tbl[m]);
  G1Jac acc = G1Jac::from_affine(tbl_load_g1(mem + (top ? 3 : 0) * kG1EntryWords));
  TC_NOUNROLL for (int c = kBits / 2 - 1; c >= 0; c--) {
    acc = jac_dbl(jac_dbl(acc));
    const uint32_t n = (uint32_t)(neg >> (2 * c)) & 3u, w = (uint32_t)(u >> (2 * c)) & 3u;  // bit 1: column 2c+1, bit 0: column 2c
    const bool sub = (n >> 1) != 0;
    const uint32_t m = w | ((((n >> 1) ^ n) & 1u) ? 0u : 4u);
    G1Affine t = tbl_load_g1(mem + m * kG1EntryWords);
    t.y = Fq::select(sub, -t.y, t.y).norm();
    acc = jac_add_mixed(acc, t);
  }
  acc.z = coord_norm(acc.z * zc);
  return G1Jac::select(dead, G1Jac::infinity(), acc);
}

// leaf `leaf` of the call from the affine encoding at `pt`.  *live (may be null: a key share, always valid): read, and cleared
// by the leader when the point does not decode -- such a share is bad without a check.  Every lane (pair) of the wave runs the
// ladder; the leaf of a slot that is not live is the identity.
template <class F>
TC_HD void job_blame_leaf(const uint32_t* key8, uint64_t leaf, const uint8_t* pt, uint8_t* live, bool leader, int32_t* out);
template <>
TC_HD void job_blame_leaf<Fq2>(const uint32_t* key8, uint64_t leaf, const uint8_t* pt, uint8_t* live, bool leader, int32_t* out) {
  uint64_t d[4];
  blame_digits(key8, leaf, d);
  G2Affine p = G2Affine::infinity();
  bool ok = !live || *live != 0;
  if (ok) ok = g2_decode_uncompressed(pt, p);
  if (!ok && live && leader) *live = 0;
  blame_store_leaf(out, blame_leaf_g2(p, ok, d));
}
template <>
TC_HD void job_blame_leaf<Fq>(const uint32_t* key8, uint64_t leaf, const uint8_t* pt, uint8_t* live, bool leader, int32_t* out) {
  uint64_t d[4];
  blame_digits(key8, leaf, d);
  G1Affine p = G1Affine::infinity();
  bool ok = !live || *live != 0;
  if (ok) ok = g1_decode_uncompressed(pt, p);
  if (!ok && live && leader) *live = 0;
  blame_store_leaf(out, blame_leaf_g1(p, ok, d));
}

// one lane's (lane pair's) share of the sum of the leaves [lo, hi) of one job: the terms sum_part (tc_dkg.h) gives part g of
// `parts`.  The loop is wave-uniform (tc_common.h): a lane whose part is shorter adds nothing in its last trips -- it reloads
// leaf `lo`, always a leaf of the range.  Complete additions: identities (slots that are not live) and equal terms are inputs.
template <class F>
TC_HD Jac<F> job_blame_range_part(const int32_t* leaves, size_t lo, size_t hi, size_t g, size_t parts) {
  const size_t n = hi - lo;
  const size_t k0 = lo + g * n / parts, k1 = lo + (g + 1) * n / parts;
  Jac<F> acc = Jac<F>::infinity();
  size_t k = k0;
  TC_NOUNROLL while (wave_any(k < k1)) {
    const bool take = k < k1;
    Jac<F> t;
    blame_load_leaf(leaves + (take ? k : lo) * BlameLeaf<F>::WORDS, t);
    const Jac<F> s = jac_add(acc, t);
    acc = Jac<F>::select(take, s, acc);
    k++;
  }
  return acc;
}

}  // namespace tc
