// Conformance ops: ONE shipped primitive of threshold_crypto_amd/csrc per op, applied to operands handed in as raw
// signed limbs (14 x int32, radix 2^28, Montgomery R = 2^392), so that lazy, non-canonical representations reach the
// primitive exactly as the caller built them and the output representation can be checked, not only its residue.
//
// Written once as TC_HD code: tests/device/conformance.hip compiles it with hipcc for gfx950 (the lane-pair Fq2 of the
// product, TC_PAIR = 1), tests/device_conformance.py compiles it with g++ -DTC_BOUND_CHECK (the host Fq2, with the
// declared input intervals loaded into the interval bookkeeping).  Test code only: never part of libtc_amd.so.
//
// Per job:  in    CONF_IN  Fq slots (14 limbs each; a canonical integer in 12 u32 words, or 13 x 30-bit limbs, where an
//                  op says so)
//           aux   CONF_AUX int32 parameters (point-at-infinity flags, the Frobenius power, "also compare")
//           out   CONF_OUT Fq slots
//           flags CONF_FLAGS int32: slots [4 l, 4 l + 4) written by lane l of the job (the one-lane and host forms write
//                  [0, 8) as a lane pair would; a host quad writes all four lanes), so lanes that disagree on a predicate show
//           range CONF_IN x {lo, hi, val}: the declared interval of every input slot (units of 2^28 for limbs, of p for
//                  the value), read by the bound-check build only
//
// The scalar block (ops 100 on, one lane per job) applies the integer and Fr code that decides WHICH multiple of a point
// is computed.  Its operands are raw u32 words, not limbs: a scalar fills the first 8 words of a slot (little-endian), a
// u64 two words, and an index list runs across consecutive slots as raw words (in words(0)); t, i, K and nbits go in aux.
//
// The pairing block (ops 80 on) applies the Miller steps, loops, exponentiations and checks of tc_pairing.h (a lane pair
// per job) and tc_quad.h (ops 90 on: a quad of four lanes per job, pair A lanes 0, 1 and pair B lanes 2, 3).  A check's
// operands: G1 point k at slots 6 k, 6 k + 1 and G2 point k at slots 6 k + 2 .. 6 k + 5 (k = 0, 1), aux[2 k] and
// aux[2 k + 1] their point-at-infinity flags.  MILLER_LINES also hands back the row block of miller_prepare_lines.
//
// The point-multiplication block (ops 140 on: G1, one lane per job; ops 160 on: G2, a lane pair per job) applies the code
// that turns digits and group operations into a multiple: table builders, common-Z bookkeeping, the branch-free ladders with
// their safe twins, GLS / GLV multiplication, cofactor clearing, the Straus combiners and the [1 / D] step of the share
// combiner.  Points go in as limbs (affine: x, y; Jacobian: x, y, z; infinity flags as bit masks in aux), scalars as raw
// words in the slot after the points.  An op hands back the Jacobian result as the routine returns it (slot 0 on), then
// jac_to_affine of it (what every shipped job body does next) with the infinity bit in flag 0.  Ops whose routine keeps
// a table in the arena of tc_table.h (conf_needs_table) run with a table slot held, as the product's kernels do.
//
// The wave-uniform forms of the G2 share combination (scalar ops 128 on, point ops 172 on, byte op 214) read K, the
// coefficients, D or (q, T, E) from the wave's first active lane: their case tables give one such key to every aligned block
// of 32 jobs, and an op hands back the routine's exception flag (flag 1) beside its result, so that a lane which met a
// special case shows exactly there and its 31 wave-mates show untouched.
//
// The byte layer (ops 180 on: hash primitives and G1, one lane per job; ops 200 on: everything that holds Fq2 or calls
// duo_each, a lane pair per job) applies the code on either side of the arithmetic: SHA3-256, the ChaCha20 word stream,
// the rejection samplers and the hash onto G2 of tc_hash.h, the wire codecs of tc_codec.h / tc_sqrt.h and the job_*
// wrappers of tc_jobs.h around them.  Byte operands go in as raw words (in_bytes: byte k of the job's input row,
// little-endian), a length in aux.  Byte results are written by the shipped routine itself, through Ctx::bytes (the
// job's output row as bytes) from EVERY lane of the job -- in the lane-pair build each lane stores its own 48-byte half
// --, so lanes past the end of the batch get a spare row from the launcher.  Status bytes and verdicts go in flags.
#pragma once
#include "../../threshold_crypto_amd/csrc/tc_codec.h"  // (tc_quad.h job_pairing_check_quad_io decodes)
#include "../../threshold_crypto_amd/csrc/tc_quad.h"
#include "../../threshold_crypto_amd/csrc/tc_sqrt.h"
#include "../../threshold_crypto_amd/csrc/tc_msm.h"
#include "../../threshold_crypto_amd/csrc/tc_dkg.h"
#include "../../threshold_crypto_amd/csrc/tc_hash.h"
#include "../../threshold_crypto_amd/csrc/tc_jobs.h"

namespace tc {
namespace conf {

// (CONF_IN and CONF_OUT hold the 68 abscissae / coefficients of t = 67 as 8-word scalars: 544 words)
constexpr int CONF_IN = 40, CONF_OUT = 40, CONF_AUX = 4, CONF_FLAGS = 16;
constexpr int CONF_MAX_N = 68;  // t + 1 of the scalar block's index lists

enum Op {
  // Fq, one lane per job
  FQ_MUL = 0, FQ_SQR, FQ_REDC_FULL, FQ_FROM_CANONICAL, FQ_TO_CANONICAL, FQ_FROM_MONT384, FQ_GT_HALF, FQ_NORM,
  FQ_REDUCE_VALUE, FQ_ZERO, FQ_INV, FQ_INV_FERMAT, FQ_INV30, FQ_LEGENDRE, FQ_SQRT,
  // Fq2 (lane pair on the device)
  FQ2_MUL = 20, FQ2_SQR, FQ2_CONJ, FQ2_MUL_XI, FQ2_NORM_FQ, FQ2_INV, FQ2_ZERO, FQ2_SQRT, FQ2_SQRT_X2, FQ2_INV_X2,
  // Fq6 / Fq12 (lane pair)
  FQ6_MUL = 40, FQ6_SQR, FQ6_INV, FQ12_MUL, FQ12_SQR, FQ12_INV, FQ12_FROB, FQ12_CONJ, FQ12_LINE_PRODUCT,
  FQ12_CYCLO_SQR, CYCLO_CHAIN,
  // G1, one lane per job
  G1_DBL = 60, G1_ADD_MIXED, G1_ADD, G1_ADD_MIXED_GENERIC, G1_ADD_GENERIC, G1_TO_AFFINE, G1_ON_CURVE, G1_IN_SUBGROUP,
  // G2 (lane pair)
  G2_DBL = 70, G2_ADD_MIXED, G2_ADD, G2_ADD_MIXED_GENERIC, G2_ADD_GENERIC, G2_TO_AFFINE, G2_TO_AFFINE_X2, G2_ON_CURVE,
  G2_IN_SUBGROUP, G2_PSI,
  // the pairing (lane pair)
  MILLER_DBL_STEP = 80, MILLER_ADD_STEP, MILLER_LOOP2, MILLER_LINES, CYCLO_EXP_BY_X, CYCLO_EXP_BY_X_HALF, FINAL_EXP,
  PAIRING_CHECK,
  // the pairing on a quad (four lanes)
  Q_MILLER_LOOP = 90, Q_EXP_BY_X, Q_EXP_BY_X_HALF, Q_FINAL_EXP, Q_PAIRING_CHECK,
  // Fr and the scalar layer, one lane per job
  FR_ADD = 100, FR_SUB, FR_MUL, FR_SQR, FR_INV, FR_FROM_CANONICAL, FR_TO_CANONICAL, FR_FROM_U64, FR_FROM_LE32,
  FR_SCALE_COFACTOR_FIX,
  DIV_BY_X_ABS = 110, GLS_DECOMPOSE, GLS_DECOMPOSE_ODD, SAC_RECODE4, GLV_DECOMPOSE, GLV_RECODE_SIGN_ALIGNED, MSM_G1_RECODE,
  LAGRANGE_COEFF = 120, LAGRANGE_COEFF_FR, LAGRANGE_ALL, LAGRANGE_SPLIT, LAGRANGE_SMALL_COEFFS, COMBINE_CLASS,
  FR_INVERSE_OF_SMALL, GCD_U64, WNAF_RECODE, COMBINE_QUOTIENT_DECOMPOSE, COMBINE_DIVIDE_CHOICE,
  // point multiplication on G1, one lane per job
  G1_ADD_AFFINE = 140, G1_COMMON_Z, G1_MUL_BY_X_ABS, G1_MUL_GLV, G1_MUL_GLV_JAC, G1_MUL_GLV_ARENA, G1_LINCOMB_CHUNK4,
  G1_STRAUS_SMALL, G1_STRAUS_SMALL_INLINE, G1_COMBINE_DIVIDE, G1_COMBINE_DIVIDE_ARENA, G1_MUL_U64,
  // point multiplication on G2 (lane pair)
  G2_ADD_AFFINE = 160, G2_COMMON_Z, G2_MUL_BY_X_ABS, G2_PSI_JAC, G2_GLS_BASES, G2_SAC_TABLE, G2_JOINT_MUL4, G2_MUL_GLS,
  G2_MUL_GLS_JAC, G2_CLEAR_COFACTOR, G2_STRAUS_SMALL, G2_COMBINE_DIVIDE,
  // the wave-uniform forms of the G2 share combination (lane pair; the parameters named in each op are the WAVE's)
  G2_STRAUS_SMALL_UNIFORM, G2_WNAF_TABLE, G2_COMBINE_DIVIDE_UNIFORM, G2_COMBINE_DIVIDE_QUOTIENT, G2_QUOTIENT_MUL,
  G2_COMBINE_UNIFORM_WAVE,
  // the byte layer: hash primitives and G1, one lane per job
  SHA3_256 = 180, CHACHA_WORDS, FQ_RANDOM, XOR_WITH_HASH, FQ_FROM_BE48, FQ_TO_BE48, FQ_LEX_LARGEST, G1_DECODE_UNCOMPRESSED,
  G1_ENCODE_UNCOMPRESSED, G1_ENCODE_COMPRESSED, G1_DECODE_COMPRESSED,
  // the byte layer on Fq2 / two jobs per pair (lane pair)
  G2_RANDOM_FROM_SEED = 200, G2_RANDOM_FROM_SEED_X2, HASH_G2, HASH_G2_X2, HASH_G1_G2, HASH_G1_G2_X2, FQ2_FROM_BE96,
  FQ2_TO_BE96, FQ2_LEX_LARGEST, G2_DECODE_UNCOMPRESSED, G2_ENCODE_UNCOMPRESSED, G2_ENCODE_COMPRESSED, G2_DECODE_COMPRESSED,
  G2_DECODE_COMPRESSED_X2, JOB_COMBINE_SMALL_G2,
};

// the quad ops (tc_quad.h): four lanes per job on the device, two threads per job on the host
TC_HD constexpr bool conf_quad(int op) { return op >= Q_MILLER_LOOP && op < FR_ADD; }
// lanes per job on the device: Fq, G1 and the scalar block one, everything that holds Fq2 values a lane pair
TC_HD constexpr int conf_lanes(int op) {
  return conf_quad(op) ? kQuadLanes
         : (op >= FQ2_MUL && op < G1_DBL) || (op >= G2_DBL && op < FR_ADD) || (op >= G2_ADD_AFFINE && op < SHA3_256) ||
                 op >= G2_RANDOM_FROM_SEED
             ? kG2Lanes
             : 1;
}
// ops whose routine keeps a table in the arena (tc_table.h): the kernel holds a table slot while the op runs
TC_HD constexpr bool conf_needs_table(int op) {
  return op == G1_MUL_GLV_ARENA || op == G1_COMBINE_DIVIDE_ARENA || op == G2_SAC_TABLE || op == G2_JOINT_MUL4 ||
         op == G2_MUL_GLS || op == G2_MUL_GLS_JAC || op == G2_COMBINE_DIVIDE || (op >= G2_STRAUS_SMALL_UNIFORM && op < SHA3_256) ||
         op == JOB_COMBINE_SMALL_G2;
}
// ops that take a row block (tc_pairing.h Fq2Rows): device, kConfLineWords words per lane in the row layout of
// k_miller_lines; host, kMillerRowSlots Fq2 per job
TC_HD constexpr bool conf_needs_rows(int op) { return op == MILLER_LINES; }
constexpr int kConfLineWords = kMillerRowSlots * FQ_LIMBS;

struct Ctx {
  const int32_t* in;
  const int32_t* aux;
  int32_t* out;
  int32_t* flags;
  const float* range;  // bound-check build: declared input intervals
  bool live;           // a real job (lanes past the end of the batch run a copy of the last job and store nothing)
  int lane;            // 0 .. 3 within the job's lanes (a host quad thread: 0 for pair A, 2 for pair B)
  bool pair;           // every lane of the job runs on its own lane (device lane-pair and quad forms)
  void* rows = nullptr;  // conf_needs_rows: this lane's column of the row block (device) / the job's Fq2 rows (host)

  TC_HD Fq fq(int s) const {
    Fq r;
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) r.l[i] = in[s * FQ_LIMBS + i];
#if defined(TC_BOUND_CHECK)
    r.set_range(range[3 * s], range[3 * s + 1]);
    r.set_val(range[3 * s + 2]);
#endif
    return r;
  }
  TC_HD Fq2 fq2(int s) const { return Fq2::make(fq(s), fq(s + 1)); }
  TC_HD Fq6 fq6(int s) const { return Fq6{fq2(s), fq2(s + 2), fq2(s + 4)}; }
  TC_HD Fq12 fq12(int s) const { return Fq12{fq6(s), fq6(s + 6)}; }
  template <class F>
  TC_HD F field(int s) const;
  TC_HD const uint32_t* words(int s) const { return (const uint32_t*)(in + s * FQ_LIMBS); }
  // the byte layer: byte k of the job's input row (raw words, little-endian) / of its output row.  The shipped routines
  // store through bytes() from every lane of the job; a lane past the end of the batch has a spare row behind `out`
  TC_HD const uint8_t* in_bytes(int k) const { return (const uint8_t*)in + k; }
  TC_HD uint8_t* bytes(int k) const { return (uint8_t*)out + k; }
  // the scalar block: u64 k of the raw words from slot 0 on (two words each, low word first)
  TC_HD uint64_t u64(int k) const {
    const uint32_t* w = words(0);
    return (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
  }
  TC_HD uint64_t u64_at(int s, int k) const {  // u64 k of the raw words from slot s on
    const uint32_t* w = words(s);
    return (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
  }
  TC_HD Fr fr(int s) const {  // a Montgomery-form Fr, raw words
    Fr r;
    TC_UNROLL for (int i = 0; i < 8; i++) r.v.l[i] = words(s)[i];
    return r;
  }

  TC_HD bool writer() const { return live && lane == 0; }
  TC_HD void put_raw(int s, const int32_t* v, int n) {
    if (writer()) TC_UNROLL for (int i = 0; i < n; i++) out[s * FQ_LIMBS + i] = v[i];
  }
  TC_HD void put(int s, const Fq& v) { put_raw(s, v.l, FQ_LIMBS); }
  TC_HD void put_words(int s, const uint32_t* v, int n) { put_raw(s, (const int32_t*)v, n); }
  TC_HD void put(int s, const Fr& v) { put_words(s, v.v.l, 8); }
  TC_HD void put_u64(int s, int k, uint64_t v) {  // word pair k of slot s (and on)
    const uint32_t w[2] = {(uint32_t)v, (uint32_t)(v >> 32)};
    if (writer()) TC_UNROLL for (int i = 0; i < 2; i++) out[s * FQ_LIMBS + 2 * k + i] = (int32_t)w[i];
  }
  TC_HD void put_u128(int s, int k, tc_u128 v) {  // words 4 k .. 4 k + 3 of slot s (and on)
    put_u64(s, 2 * k, (uint64_t)v);
    put_u64(s, 2 * k + 1, (uint64_t)(v >> 64));
  }
  // (both coefficients are gathered by both lanes first: re() / im() exchange values over the pair)
  TC_HD void put(int s, const Fq2& v) {
    const Fq re = v.re(), im = v.im();
    put(s, re);
    put(s + 1, im);
  }
  TC_HD void put(int s, const Fq6& v) {
    put(s, v.c0);
    put(s + 2, v.c1);
    put(s + 4, v.c2);
  }
  TC_HD void put(int s, const Fq12& v) {
    put(s, v.c0);
    put(s + 6, v.c1);
  }
  TC_HD void flag(int i, int v) {
    if (!live) return;
    flags[lane * 4 + i] = v;
    if (!pair) flags[(lane + 1) * 4 + i] = v;  // one lane, or a host thread that stands for a lane pair: both halves
  }
};
template <>
TC_HD Fq Ctx::field<Fq>(int s) const { return fq(s); }
template <>
TC_HD Fq2 Ctx::field<Fq2>(int s) const { return fq2(s); }

// coordinates per field element: 1 slot (Fq) or 2 (Fq2)
template <class F>
struct Width;
template <>
struct Width<Fq> { static constexpr int n = 1; };
template <>
struct Width<Fq2> { static constexpr int n = 2; };

template <class F>
TC_HD Jac<F> jac_at(const Ctx& c, int s) {
  constexpr int w = Width<F>::n;
  return Jac<F>{c.field<F>(s), c.field<F>(s + w), c.field<F>(s + 2 * w)};
}
template <class F>
TC_HD Affine<F> aff_at(const Ctx& c, int s, int inf) {
  constexpr int w = Width<F>::n;
  return Affine<F>{c.field<F>(s), c.field<F>(s + w), inf != 0};
}
template <class F>
TC_HD void put_jac(Ctx& c, int s, const Jac<F>& p) {
  constexpr int w = Width<F>::n;
  c.put(s, p.x);
  c.put(s + w, p.y);
  c.put(s + 2 * w, p.z);
}
template <class F>
TC_HD void put_aff(Ctx& c, int s, const Affine<F>& p) {
  constexpr int w = Width<F>::n;
  c.put(s, p.x);
  c.put(s + w, p.y);
}

template <class F>
TC_HD F curve_b();
template <>
TC_HD Fq curve_b<Fq>() { return g1_b(); }
template <>
TC_HD Fq2 curve_b<Fq2>() { return g2_b(); }

// the group ops, for F = Fq (G1) and F = Fq2 (G2): slots P = [0, 3w), Q = [3w, 6w) (affine Q: [3w, 5w), aux[0] = Q at infinity)
template <class F, int K>
TC_HD void conf_curve(Ctx& c) {
  constexpr int w = Width<F>::n;
  if constexpr (K == 0) {
    put_jac(c, 0, jac_dbl(jac_at<F>(c, 0)));
  } else if constexpr (K == 1) {
    put_jac(c, 0, jac_add_mixed(jac_at<F>(c, 0), aff_at<F>(c, 3 * w, c.aux[0])));
  } else if constexpr (K == 2) {
    put_jac(c, 0, jac_add(jac_at<F>(c, 0), jac_at<F>(c, 3 * w)));
  } else if constexpr (K == 3) {
    bool exc = false;
    const Jac<F> r = jac_add_mixed_generic(jac_at<F>(c, 0), aff_at<F>(c, 3 * w, c.aux[0]), exc);
    put_jac(c, 0, r);
    c.flag(0, exc);
  } else if constexpr (K == 4) {
    bool exc = false;
    const Jac<F> r = jac_add_generic(jac_at<F>(c, 0), jac_at<F>(c, 3 * w), exc);
    put_jac(c, 0, r);
    c.flag(0, exc);
  } else if constexpr (K == 5) {
    const Affine<F> a = jac_to_affine(jac_at<F>(c, 0));
    put_aff(c, 0, a);
    c.flag(0, a.inf);
  } else if constexpr (K == 6) {
    c.flag(0, affine_on_curve(aff_at<F>(c, 0, c.aux[0]), curve_b<F>()));
  }
}

// ---- the pairing: Miller steps and loops, the cyclotomic exponentiation, the final exponentiation, the check ----------
// G1 / G2 operand k of a check (slots 6 k .. 6 k + 5, aux[2 k], aux[2 k + 1])
TC_HD G1Affine conf_g1(const Ctx& c, int k) { return aff_at<Fq>(c, 6 * k, c.aux[2 * k]); }
TC_HD G2Affine conf_g2(const Ctx& c, int k) { return aff_at<Fq2>(c, 6 * k + 2, c.aux[2 * k + 1]); }

template <int OP>
TC_HD void conf_pairing(Ctx& c) {
  if constexpr (OP == MILLER_DBL_STEP || OP == MILLER_ADD_STEP) {
    // T = (X : Y : zt) at slots 0 .. 5, the affine Q at 6 .. 9; out: T' at 0 .. 5, the line (c0, c1, c2) at 6 .. 11
    G2Jac t = jac_at<Fq2>(c, 0);
    LineCoeffs l;
    if constexpr (OP == MILLER_DBL_STEP) {
      l = miller_doubling_step(t);
    } else {
      l = miller_addition_step(t, aff_at<Fq2>(c, 6, 0));
    }
    put_jac(c, 0, t);
    c.put(6, l.c0);
    c.put(8, l.c1);
    c.put(10, l.c2);
  } else if constexpr (OP == MILLER_LOOP2 || OP == MILLER_LINES || OP == PAIRING_CHECK) {
    const G1Affine ps[2] = {conf_g1(c, 0), conf_g1(c, 1)};
    const G2Affine qs[2] = {conf_g2(c, 0), conf_g2(c, 1)};
    if constexpr (OP == MILLER_LOOP2) {
      c.put(0, miller_loop<2>(ps, qs));
    } else if constexpr (OP == MILLER_LINES) {  // k_miller_lines, then k_miller_accumulate on the same rows
      const bool skip[2] = {ps[0].inf || qs[0].inf, ps[1].inf || qs[1].inf};
#if TC_PAIR
      const Fq2Rows rows = Fq2Rows::at(static_cast<int32_t*>(c.rows));
#else
      const Fq2Rows rows = Fq2Rows::at(static_cast<Fq2*>(c.rows));
#endif
      miller_prepare_lines(ps, qs, skip, rows);
      c.put(0, miller_accumulate(rows));
    } else {  // (a, b, c, d) = (P0, Q0, P1, Q1): pairing_check negates c itself
      c.flag(0, pairing_check(ps[0], qs[0], ps[1], qs[1]));
    }
  } else if constexpr (OP == CYCLO_EXP_BY_X || OP == CYCLO_EXP_BY_X_HALF) {
    // (the exponent is fixed per op: cyclotomic_exp_by_x reads it from the wave's first lane)
    c.put(0, cyclotomic_exp_by_x(c.fq12(0), OP == CYCLO_EXP_BY_X ? BLS_X_ABS : BLS_X_ABS >> 1));
  } else if constexpr (OP == FINAL_EXP) {
    const Fq12 r = final_exponentiation(c.fq12(0));
    c.put(0, r);
    c.flag(0, r == Fq12::one());  // the comparison of pairing_check / job_final_exp_is_one
  // ---- the quad forms: pair A (lanes 0, 1) gets pair 0 of the operands, pair B (lanes 2, 3) pair 1 ----
  } else if constexpr (OP == Q_MILLER_LOOP) {
    const int k = quad_hi() ? 1 : 0;
    c.put(0, q_miller_loop(conf_g1(c, k), conf_g2(c, k)).gather());
  } else if constexpr (OP == Q_EXP_BY_X || OP == Q_EXP_BY_X_HALF) {
    c.put(0, q_exp_by_x(QFq12::from(c.fq12(0)), OP == Q_EXP_BY_X ? BLS_X_ABS : BLS_X_ABS >> 1).gather());
  } else if constexpr (OP == Q_FINAL_EXP) {
    const QFq12 r = q_final_exponentiation(QFq12::from(c.fq12(0)));
    c.put(0, r.gather());
    c.flag(0, r.is_one());
  } else if constexpr (OP == Q_PAIRING_CHECK) {  // pair A brings (a, b), pair B (c, d)
    const int k = quad_hi() ? 1 : 0;
    c.flag(0, q_pairing_check(conf_g1(c, k), conf_g2(c, k)));
  }
}

// ---- the scalar block: Fr, the base-|x| / GLV decompositions and their recodings, Lagrange coefficients ------------------
template <int OP>
TC_HD void conf_scalar(Ctx& c) {
  if constexpr (OP == FR_ADD) {
    c.put(0, c.fr(0) + c.fr(1));
  } else if constexpr (OP == FR_SUB) {
    c.put(0, c.fr(0) - c.fr(1));
  } else if constexpr (OP == FR_MUL) {
    c.put(0, c.fr(0) * c.fr(1));
  } else if constexpr (OP == FR_SQR) {
    c.put(0, c.fr(0).sqr());
  } else if constexpr (OP == FR_INV) {
    c.put(0, c.fr(0).inv());
  } else if constexpr (OP == FR_FROM_CANONICAL) {
    c.put(0, Fr::from_canonical(c.words(0)));
  } else if constexpr (OP == FR_TO_CANONICAL) {
    uint32_t w[8];
    c.fr(0).to_canonical(w);
    c.put_words(0, w, 8);
  } else if constexpr (OP == FR_FROM_U64) {
    c.put(0, fr_from_u64(c.u64(0)));
  } else if constexpr (OP == FR_FROM_LE32) {
    uint32_t w[8];
    const bool ok = fr_from_le32((const uint8_t*)c.words(0), w);
    c.put_words(0, w, 8);
    c.flag(0, ok);
  } else if constexpr (OP == FR_SCALE_COFACTOR_FIX) {
    uint8_t b[32];
    job_fr_scale_cofactor_fix((const uint8_t*)c.words(0), b);
    uint32_t w[8];
    TC_UNROLL for (int i = 0; i < 8; i++)
      w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
    c.put_words(0, w, 8);
  } else if constexpr (OP == DIV_BY_X_ABS) {
    uint64_t rem = 0;
    const uint64_t q = div_by_x_abs(c.u64(0), c.u64(1), &rem);  // (u1 : u0)
    c.put_u64(0, 0, q);
    c.put_u64(0, 1, rem);
  } else if constexpr (OP == GLS_DECOMPOSE || OP == GLS_DECOMPOSE_ODD) {
    uint64_t d[4];
    if constexpr (OP == GLS_DECOMPOSE) {
      gls_decompose(c.words(0), d);
    } else {
      c.flag(0, gls_decompose_odd(c.words(0), d));
    }
    TC_UNROLL for (int j = 0; j < 4; j++) c.put_u64(0, j, d[j]);
  } else if constexpr (OP == SAC_RECODE4) {
    const uint64_t d[4] = {c.u64(0), c.u64(1), c.u64(2), c.u64(3)};
    const SacDigits sd = sac_recode4(d, c.aux[0]);
    c.put_u64(0, 0, sd.neg);
    TC_UNROLL for (int j = 0; j < 3; j++) c.put_u64(0, j + 1, sd.u[j]);
    c.flag(0, (int)sd.top);
    c.flag(1, sd.fix);
  } else if constexpr (OP == GLV_DECOMPOSE) {
    tc_u128 k1, k2;
    glv_decompose(c.words(0), &k1, &k2);
    c.put_u128(0, 0, k1);
    c.put_u128(0, 1, k2);
  } else if constexpr (OP == GLV_RECODE_SIGN_ALIGNED) {
    tc_u128 neg, u;
    bool top = false;
    const bool flip = glv_recode_sign_aligned(c.words(0), &neg, &u, &top);
    c.put_u128(0, 0, neg);
    c.put_u128(0, 1, u);
    c.flag(0, flip);
    c.flag(1, top);
  } else if constexpr (OP == MSM_G1_RECODE) {
    uint8_t codes[65];
    TC_UNROLL for (int i = 0; i < 65; i++) codes[i] = 0xee;  // (a column the recoding leaves alone keeps this)
    bool fits = false;
    const bool flip = msm_g1_recode(c.words(0), codes, 1, c.aux[0], &fits);
    uint32_t w[65];
    TC_UNROLL for (int i = 0; i < 65; i++) w[i] = codes[i];
    c.put_words(0, w, 65);
    c.flag(0, flip);
    c.flag(1, fits);
  } else if constexpr (OP == LAGRANGE_COEFF || OP == LAGRANGE_ALL || OP == LAGRANGE_SPLIT) {
    const int t = c.aux[0], n = t + 1;
    uint64_t idx[CONF_MAX_N];
    TC_NOUNROLL for (int j = 0; j < n; j++) idx[j] = c.u64(j);
    if constexpr (OP == LAGRANGE_COEFF) {
      uint32_t w[8];
      c.flag(0, job_lagrange(idx, t, c.aux[1], w));
      c.put_words(0, w, 8);
    } else {
      uint32_t ws[4 * CONF_MAX_N * 8], w[CONF_MAX_N * 8];
      uint8_t st;
      if constexpr (OP == LAGRANGE_ALL) {
        st = lagrange_all_at_zero(idx, t, w, ws);
      } else {  // k_lagrange_den (every i), then k_lagrange_finish
        uint32_t* xm = ws;
        uint32_t* den = ws + CONF_MAX_N * 8;
        TC_NOUNROLL for (int i = 0; i < n; i++) {
          const Fr x = fr_from_u64(idx[i]) + Fr::one();
          TC_UNROLL for (int k = 0; k < 8; k++) xm[i * 8 + k] = x.v.l[k];
        }
        TC_NOUNROLL for (int i = 0; i < n; i++) {
          const Fr d = lagrange_denominator(idx, n, i);
          TC_UNROLL for (int k = 0; k < 8; k++) den[i * 8 + k] = d.v.l[k];
        }
        st = lagrange_finish(n, xm, den, ws + 2 * CONF_MAX_N * 8, w);
      }
      c.flag(0, st);
      c.put_words(0, w, 8 * n);
    }
  } else if constexpr (OP == LAGRANGE_COEFF_FR) {
    Fr lam = Fr::zero();
    const bool ok = lagrange_coeff_at_zero_fr(c.words(0), c.aux[0], c.aux[1], lam);
    uint32_t w[8];
    lam.to_canonical(w);
    c.put_words(0, w, 8);
    c.flag(0, ok);
  } else if constexpr (OP == LAGRANGE_SMALL_COEFFS || OP == COMBINE_CLASS) {
    const uint64_t idx[4] = {c.u64(0), c.u64(1), c.u64(2), c.u64(3)};
    if constexpr (OP == LAGRANGE_SMALL_COEFFS) {
      uint64_t c_abs[4] = {0, 0, 0, 0}, d_abs = 0;
      bool c_neg[4] = {false, false, false, false}, d_neg = false;
      bool ok = false;
      if (c.aux[0] == 2) ok = lagrange_small_coeffs<2>(idx, c_abs, c_neg, &d_abs, &d_neg);
      if (c.aux[0] == 3) ok = lagrange_small_coeffs<3>(idx, c_abs, c_neg, &d_abs, &d_neg);
      if (c.aux[0] == 4) ok = lagrange_small_coeffs<4>(idx, c_abs, c_neg, &d_abs, &d_neg);
      TC_UNROLL for (int k = 0; k < 4; k++) c.put_u64(0, k, c_abs[k]);
      c.put_u64(0, 4, d_abs);
      c.flag(0, ok);
      c.flag(1, d_neg);
      c.flag(2, (int)c_neg[0] | ((int)c_neg[1] << 1) | ((int)c_neg[2] << 2) | ((int)c_neg[3] << 3));
    } else {
      c.flag(0, combine_job_class(idx, c.aux[0]));
      c.flag(1, combine_small_applies(idx, c.aux[0]));
    }
  } else if constexpr (OP == FR_INVERSE_OF_SMALL) {
    uint32_t w[8];
    fr_inverse_of_small(c.u64(0), c.aux[0] != 0, w);
    c.put_words(0, w, 8);
  } else if constexpr (OP == GCD_U64) {
    c.put_u64(0, 0, gcd_u64(c.u64(0), c.u64(1)));
  } else if constexpr (OP == WNAF_RECODE) {
    // the u64 of slot 0; out: the 65 digits of width 4 (words 0 .. 64), of width kQuotWidth (65 .. 129), then pos and neg of
    // naf_recode (word pairs 65 and 66)
    int8_t d4[kWnafCols], dq[kWnafCols];
    wnaf_recode<4>(c.u64(0), d4);
    wnaf_recode<kQuotWidth>(c.u64(0), dq);
    uint32_t w[2 * kWnafCols];
    TC_NOUNROLL for (int i = 0; i < kWnafCols; i++) {
      w[i] = (uint32_t)(int32_t)d4[i];
      w[kWnafCols + i] = (uint32_t)(int32_t)dq[i];
    }
    c.put_words(0, w, 2 * kWnafCols);
    uint64_t pos = 0, neg = 0;
    naf_recode(c.u64(0), &pos, &neg);
    c.put_u64(0, kWnafCols, pos);
    c.put_u64(0, kWnafCols + 1, neg);
  } else if constexpr (OP == COMBINE_QUOTIENT_DECOMPOSE || OP == COMBINE_DIVIDE_CHOICE) {
    // D = the u64 of slot 0.  DECOMPOSE: out q, T[4], E[4] (word pairs 0 .. 8), flag 0 = the verdict.  CHOICE: flag 0 =
    // combine_divide_takes_quotient, flag 1 = the decomposition exists, and then both predictions (word pairs 0, 1)
    const uint64_t D = c.u64(0);
    uint64_t q = 0;
    int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
    const bool ok = combine_quotient_decompose(D, &q, T, E);
    if constexpr (OP == COMBINE_QUOTIENT_DECOMPOSE) {
      c.put_u64(0, 0, q);
      TC_UNROLL for (int j = 0; j < 4; j++) {
        c.put_u64(0, 1 + j, (uint64_t)T[j]);
        c.put_u64(0, 5 + j, (uint64_t)E[j]);
      }
      c.flag(0, ok);
    } else {
      c.flag(0, combine_divide_takes_quotient(D));
      c.flag(1, ok);
      if (ok) {
        c.put_u64(0, 0, combine_divide_uniform_macs(D));
        c.put_u64(0, 1, combine_divide_quotient_macs(q, T, E));
      }
    }
  }
}

// ---- the point-multiplication block: table builders, ladders, GLS / GLV, cofactor clearing, Straus, [1 / D] ----------
// the Jacobian result as the routine returns it (slots 0 .. 3w), jac_to_affine of it (3w .. 5w), flag 0 = infinity
template <class F>
TC_HD void put_result(Ctx& c, const Jac<F>& r) {
  constexpr int w = Width<F>::n;
  put_jac(c, 0, r);
  const Affine<F> a = jac_to_affine(r);
  put_aff(c, 3 * w, a);
  c.flag(0, a.inf);
}
// N affine points at slots 2w k, bit k of mask = point k at infinity
template <class F, int N>
TC_HD void affs_at(const Ctx& c, int mask, Affine<F>* pts) {
  constexpr int w = Width<F>::n;
  TC_UNROLL for (int k = 0; k < N; k++) pts[k] = aff_at<F>(c, 2 * w * k, (mask >> k) & 1);
}
// a point (x, y) of the curve scaled by zc, back on the original curve and affine
template <class F>
TC_HD Affine<F> conf_unscale(const Affine<F>& p, const F& zc) {
  Jac<F> j{p.x, p.y, zc};
  if (p.inf) j = Jac<F>::infinity();
  return jac_to_affine(j);
}

// jac_batch_to_common_z on aux[0] = n Jacobian points (slots 3w i) + affine_scale_z of one more affine point (slot 3w NMAX,
// aux[1] = at infinity).  out: (x_i, y_i) at 2w i, zc at 2w NMAX, the scaled point after it, then point n - 1 and the scaled
// point brought back to the original curve; flag 0 = the infinity bits of the n points, flag 1 = the extra point's
// (G2: n <= 6 -- seven Jacobian points would need 42 input slots; G2_SAC_TABLE runs the routine at n = 7)
template <class F>
TC_HD void conf_common_z(Ctx& c) {
  constexpr int w = Width<F>::n, NMAX = w == 1 ? 7 : 6;
  const int n = c.aux[0];
  Jac<F> in[NMAX];
  Affine<F> out[NMAX];
  TC_NOUNROLL for (int i = 0; i < n; i++) in[i] = jac_at<F>(c, 3 * w * i);
  const F zc = jac_batch_to_common_z(in, out, n);
  const F zc2 = zc.sqr();
  const Affine<F> e = affine_scale_z(aff_at<F>(c, 3 * w * NMAX, c.aux[1]), zc2, zc2 * zc);
  int inf = 0;
  TC_NOUNROLL for (int i = 0; i < n; i++) {
    put_aff(c, 2 * w * i, out[i]);
    inf |= (int)out[i].inf << i;
  }
  c.put(2 * w * NMAX, zc);
  put_aff(c, 2 * w * NMAX + w, e);
  put_aff(c, 2 * w * NMAX + 3 * w, conf_unscale(out[n - 1], zc));
  put_aff(c, 2 * w * NMAX + 5 * w, conf_unscale(e, zc));
  c.flag(0, inf);
  c.flag(1, e.inf);
}

// straus_small on aux[0] = K points (slots 2w k, aux[1] their infinity bits) and K u64 (the words of slot 8w); G2 through
// straus_small_call, as job_combine_small_io calls it
template <class F, int K, bool INLINE_SAFE>
TC_HD Jac<F> conf_straus_k(const Ctx& c) {
  constexpr int w = Width<F>::n;
  Affine<F> pts[K];
  uint64_t cs[K];
  affs_at<F, K>(c, c.aux[1], pts);
  TC_UNROLL for (int k = 0; k < K; k++) cs[k] = c.u64_at(8 * w, k);
  if constexpr (w > 1) {
    return straus_small_call<F, K>(pts, cs);
  } else {
    return straus_small<F, K, INLINE_SAFE>(pts, cs);
  }
}
template <class F, bool INLINE_SAFE>
TC_HD void conf_straus(Ctx& c) {
  Jac<F> r = Jac<F>::infinity();
  if (c.aux[0] == 2) r = conf_straus_k<F, 2, INLINE_SAFE>(c);
  if (c.aux[0] == 3) r = conf_straus_k<F, 3, INLINE_SAFE>(c);
  if (c.aux[0] == 4) r = conf_straus_k<F, 4, INLINE_SAFE>(c);
  put_result(c, r);
}

// straus_small_uniform / combine_uniform_wave on K G2 points (slots 4 k) and the u64 words of slot 16
template <int K>
TC_HD void conf_straus_uniform(Ctx& c) {
  G2Affine pts[K];
  uint64_t cs[K];
  affs_at<Fq2, K>(c, c.aux[1], pts);
  TC_UNROLL for (int k = 0; k < K; k++) cs[k] = c.u64_at(16, k);
  bool exc = false;
  const G2Jac r = straus_small_uniform<Fq2, K>(pts, cs, exc);
  put_result(c, r);
  c.flag(1, exc);
}
template <int K>
TC_HD void conf_uniform_wave(Ctx& c) {
  G2Affine pts[K];
  uint64_t cs[K];
  affs_at<Fq2, K>(c, c.aux[1], pts);
  TC_UNROLL for (int k = 0; k < K; k++) cs[k] = c.u64_at(16, k);
  put_result(c, combine_uniform_wave<K>(pts, cs, c.u64_at(16, 4), c.aux[2] != 0));
}

template <int OP>
TC_HD void conf_mul(Ctx& c) {
  if constexpr (OP == G1_ADD_AFFINE) {
    put_result(c, jac_add_affine(aff_at<Fq>(c, 0, c.aux[0]), aff_at<Fq>(c, 2, c.aux[1])));
  } else if constexpr (OP == G2_ADD_AFFINE) {
    put_result(c, jac_add_affine(aff_at<Fq2>(c, 0, c.aux[0]), aff_at<Fq2>(c, 4, c.aux[1])));
  } else if constexpr (OP == G1_COMMON_Z) {
    conf_common_z<Fq>(c);
  } else if constexpr (OP == G2_COMMON_Z) {
    conf_common_z<Fq2>(c);
  } else if constexpr (OP == G1_MUL_BY_X_ABS) {
    put_result(c, g1_mul_by_x_abs(jac_at<Fq>(c, 0)));
  } else if constexpr (OP == G2_MUL_BY_X_ABS) {
    put_result(c, g2_mul_by_x_abs(jac_at<Fq2>(c, 0)));
  } else if constexpr (OP == G2_PSI_JAC) {
    put_result(c, g2_psi(jac_at<Fq2>(c, 0)));
  } else if constexpr (OP == G2_GLS_BASES) {  // out: the four bases at 4 k, flag 0 = their infinity bits
    G2Affine base[4];
    g2_gls_bases(aff_at<Fq2>(c, 0, c.aux[0]), base);
    int inf = 0;
    TC_UNROLL for (int k = 0; k < 4; k++) {
      put_aff(c, 4 * k, base[k]);
      inf |= (int)base[k].inf << k;
    }
    c.flag(0, inf);
  } else if constexpr (OP == G2_SAC_TABLE) {
    // four affine bases (slots 4 k, aux[0] their infinity bits); out: entry m at 4 m, read back through entry(m), zc at 32,
    // entry 7 brought back to the original curve at 34; flag 0 = the entries' infinity bits
    G2Affine base[4];
    affs_at<Fq2, 4>(c, c.aux[0], base);
    G2SacTable t;
    g2_sac_table(base, t);
    int inf = 0;
    TC_NOUNROLL for (int m = 0; m < 8; m++) {
      const G2Affine e = t.entry(m);
      put_aff(c, 4 * m, e);
      inf |= (int)e.inf << m;
    }
    c.put(32, t.zc);
    put_aff(c, 34, conf_unscale(t.entry(7), t.zc));
    c.flag(0, inf);
  } else if constexpr (OP == G2_JOINT_MUL4) {  // four independent bases, four u64 digits (the words of slot 16)
    G2Affine base[4];
    affs_at<Fq2, 4>(c, c.aux[0], base);
    const uint64_t d[4] = {c.u64_at(16, 0), c.u64_at(16, 1), c.u64_at(16, 2), c.u64_at(16, 3)};
    put_result(c, g2_joint_mul4(base, d));
  } else if constexpr (OP == G2_MUL_GLS) {
    put_result(c, g2_mul_gls(aff_at<Fq2>(c, 0, c.aux[0]), c.words(4)));
  } else if constexpr (OP == G2_MUL_GLS_JAC) {
    put_result(c, g2_mul_gls(jac_at<Fq2>(c, 0), c.words(6)));
  } else if constexpr (OP == G2_CLEAR_COFACTOR) {
    put_result(c, g2_clear_cofactor(aff_at<Fq2>(c, 0, c.aux[0]), c.aux[1] != 0));
  } else if constexpr (OP == G1_MUL_GLV) {
    put_result(c, g1_mul_glv(aff_at<Fq>(c, 0, c.aux[0]), c.words(2)));
  } else if constexpr (OP == G1_MUL_GLV_JAC) {
    put_result(c, g1_mul_glv(jac_at<Fq>(c, 0), c.words(3)));
  } else if constexpr (OP == G1_MUL_GLV_ARENA) {
    put_result(c, g1_mul_glv_arena(aff_at<Fq>(c, 0, c.aux[0]), c.words(2)));
  } else if constexpr (OP == G1_LINCOMB_CHUNK4) {  // four points (aux[0] their infinity bits), scalar k in slot 8 + k
    G1Affine pts[4];
    affs_at<Fq, 4>(c, c.aux[0], pts);
    uint32_t sc[4][8];
    TC_UNROLL for (int k = 0; k < 4; k++)
      TC_UNROLL for (int i = 0; i < 8; i++) sc[k][i] = c.words(8 + k)[i];
    put_result(c, lincomb_chunk4(pts, sc));
  } else if constexpr (OP == G1_STRAUS_SMALL) {
    conf_straus<Fq, false>(c);
  } else if constexpr (OP == G1_STRAUS_SMALL_INLINE) {
    conf_straus<Fq, true>(c);
  } else if constexpr (OP == G2_STRAUS_SMALL) {
    conf_straus<Fq2, false>(c);
  } else if constexpr (OP == G1_COMBINE_DIVIDE) {  // Q, D in the words of the next slot, aux[0] = d_neg
    put_result(c, combine_divide(jac_at<Fq>(c, 0), c.u64_at(3, 0), c.aux[0] != 0));
  } else if constexpr (OP == G1_COMBINE_DIVIDE_ARENA) {
    put_result(c, combine_divide_arena(jac_at<Fq>(c, 0), c.u64_at(3, 0), c.aux[0] != 0));
  } else if constexpr (OP == G2_COMBINE_DIVIDE) {
    put_result(c, combine_divide(jac_at<Fq2>(c, 0), c.u64_at(6, 0), c.aux[0] != 0));
  } else if constexpr (OP == G1_MUL_U64) {
    put_result(c, g1_mul_u64(jac_at<Fq>(c, 0), c.u64_at(3, 0)));
  // ---- the wave-uniform forms: K, the coefficients, D and (q, T, E) are read from the wave's first lane by the routines, so
  // the case tables give one value to every job of a wave (tests/device_conformance.py uniform_table) ----
  } else if constexpr (OP == G2_STRAUS_SMALL_UNIFORM) {  // operands as G2_STRAUS_SMALL; flag 1 = exc
    if (c.aux[0] == 2) conf_straus_uniform<2>(c);
    if (c.aux[0] == 3) conf_straus_uniform<3>(c);
    if (c.aux[0] == 4) conf_straus_uniform<4>(c);
  } else if constexpr (OP == G2_WNAF_TABLE) {
    // a Jacobian point; out: entry m at 4 m, read back through entry(m), zn at 32; flag 0 = the entries' infinity bits, flag 1 = exc
    G2WnafTable t;
    bool exc = false;
    g2_wnaf_table(jac_at<Fq2>(c, 0), t, exc);
    int inf = 0;
    TC_NOUNROLL for (int m = 0; m < 8; m++) {
      const G2Affine e = t.entry(m);
      put_aff(c, 4 * m, e);
      inf |= (int)e.inf << m;
    }
    c.put(32, t.zn);
    c.flag(0, inf);
    c.flag(1, exc);
  } else if constexpr (OP == G2_COMBINE_DIVIDE_UNIFORM || OP == G2_COMBINE_DIVIDE_QUOTIENT) {  // Q, D in the words of slot 6; flag 1 = exc
    bool exc = false;
    const G2Jac q = jac_at<Fq2>(c, 0);
    const uint64_t D = c.u64_at(6, 0);
    const G2Jac r = OP == G2_COMBINE_DIVIDE_UNIFORM ? combine_divide_uniform(q, D, exc) : combine_divide_quotient(q, D, exc);
    put_result(c, r);
    c.flag(1, exc);
  } else if constexpr (OP == G2_QUOTIENT_MUL) {  // P; q, T[4], E[4] as nine u64 from slot 6 on; flag 1 = exc
    int64_t T[4], E[4];
    TC_UNROLL for (int j = 0; j < 4; j++) {
      T[j] = (int64_t)c.u64_at(6, 1 + j);
      E[j] = (int64_t)c.u64_at(6, 5 + j);
    }
    bool exc = false;
    const G2Jac r = g2_quotient_mul(jac_at<Fq2>(c, 0), c.u64_at(6, 0), T, E, exc);
    put_result(c, r);
    c.flag(1, exc);
  } else if constexpr (OP == G2_COMBINE_UNIFORM_WAVE) {
    // aux[0] = K points (aux[1] their infinity bits), K u64 coefficients and D (the words of slot 16), aux[2] = d_neg
    if (c.aux[0] == 2) conf_uniform_wave<2>(c);
    if (c.aux[0] == 3) conf_uniform_wave<3>(c);
    if (c.aux[0] == 4) conf_uniform_wave<4>(c);
  }
}

// ---- the byte layer: SHA3, ChaCha20, the samplers and the hash onto G2; the wire codecs and their job_* wrappers --------
// byte offsets inside the job's rows (the case tables of tests/device_conformance.py use the same)
constexpr int kConfG1B = 96, kConfMsg = 96;                    // HASH_G1_G2 / XOR_WITH_HASH: g1 at 0, the message at 96
constexpr int kConfMsgB2 = 1120;                               // HASH_G2_X2: message A at 0, B at 1120
constexpr int kConfMsgA4 = 192, kConfMsgB4 = 1216;             // HASH_G1_G2_X2: g1 A at 0, g1 B at 96, messages at 192 / 1216
constexpr int kConfWrap = 10 * FQ_LIMBS * 4;                   // decode ops: the wrapper's output bytes, from slot 10 on

// the stream words an rng has handed out so far (ChaChaRng: `counter` blocks refilled, `idx` words of the last one used)
TC_HD uint32_t conf_words_used(const ChaChaRng& rng) { return (uint32_t)rng.counter * 16u + (uint32_t)rng.idx - 16u; }

template <class F>
TC_HD void put_decoded(Ctx& c, bool ok, const Affine<F>& p) {
  put_aff(c, 0, p);
  c.flag(0, ok);
  c.flag(1, p.inf);
}

constexpr int kConfIdx = 4 * 192;  // JOB_COMBINE_SMALL_G2: the index tuple behind four shares
template <int K>
TC_HD void conf_combine_small(Ctx& c) {
  uint64_t idx[K];
  TC_UNROLL for (int k = 0; k < K; k++) {
    const uint32_t* w = (const uint32_t*)c.in_bytes(kConfIdx + 8 * k);
    idx[k] = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  }
  DirectIO io{c.in_bytes(0), (size_t)192, c.bytes(0)};
  uint8_t status = 0xee;
  const bool took = job_combine_small_io<Fq2, K, DirectIO>(idx, true, io, &status);
  c.flag(0, status);
  c.flag(1, took);
}

template <int OP>
TC_HD void conf_bytes(Ctx& c) {
  if constexpr (OP == SHA3_256) {  // aux[0] = len, aux[1]: the out-of-line form
    uint32_t w[8];
    if (c.aux[1]) {
      sha3_256_words_call(c.in_bytes(0), (size_t)c.aux[0], w);
    } else {
      sha3_256_words(c.in_bytes(0), (size_t)c.aux[0], w);
    }
    c.put_words(0, w, 8);
  } else if constexpr (OP == CHACHA_WORDS) {
    // key = the words of slot 0; aux[1]: start at the counter in the words of slot 1; aux[0] <= 64 words, then idx and counter
    ChaChaRng rng;
    rng.init(c.words(0));
    if (c.aux[1]) rng.counter = c.u64_at(1, 0);
    const int n = c.aux[0];
    TC_NOUNROLL for (int i = 0; i < 64; i++) {
      if (i < n) {
        const uint32_t w = rng.next_u32();
        if (c.writer()) c.out[i] = (int32_t)w;
      }
    }
    const uint32_t tail[3] = {(uint32_t)rng.idx, (uint32_t)rng.counter, (uint32_t)(rng.counter >> 32)};
    c.put_words(5, tail, 3);
  } else if constexpr (OP == FQ_RANDOM) {
    // seed = the words of slot 0; aux[0] <= 8 draws (slot k), the stream words used after each (the words of slot 8)
    ChaChaRng rng;
    rng.init(c.words(0));
    const int n = c.aux[0];
    TC_NOUNROLL for (int k = 0; k < 8; k++) {  // (every lane draws eight times: fq_random decides per wave)
      const Fq v = fq_random(rng);
      const uint32_t used = conf_words_used(rng);
      if (k < n) {
        c.put(k, v);
        if (c.writer()) c.out[8 * FQ_LIMBS + k] = (int32_t)used;
      }
    }
  } else if constexpr (OP == XOR_WITH_HASH) {
    c.flag(0, job_xor_with_hash(c.in_bytes(0), c.in_bytes(kConfMsg), (size_t)c.aux[0], c.bytes(0)));
  } else if constexpr (OP == FQ_FROM_BE48) {
    Fq v;
    const bool ok = fq_from_be48(c.in_bytes(0), c.aux[0] != 0, v);
    c.put(0, v);
    c.flag(0, ok);
  } else if constexpr (OP == FQ_TO_BE48) {
    fq_to_be48(c.fq(0), c.bytes(0));
  } else if constexpr (OP == FQ_LEX_LARGEST) {
    c.flag(0, fq_lex_largest(c.fq(0)));
  } else if constexpr (OP == FQ2_FROM_BE96) {
    Fq2 v;
    const bool ok = fq2_from_be96(c.in_bytes(0), c.aux[0] != 0, v);
    c.put(0, v);
    c.flag(0, ok);
  } else if constexpr (OP == FQ2_TO_BE96) {
    fq2_to_be96(c.fq2(0), c.bytes(0));
  } else if constexpr (OP == FQ2_LEX_LARGEST) {
    c.flag(0, fq2_lex_largest(c.fq2(0)));
  // ---- decode: the routine (point at slot 0, flag 0 = verdict, flag 1 = infinity), then its wrapper (bytes from slot 10 on,
  // flag 2 = status) ----
  } else if constexpr (OP == G1_DECODE_UNCOMPRESSED) {
    G1Affine p = G1Affine::infinity();
    const bool ok = g1_decode_uncompressed(c.in_bytes(0), p);
    put_decoded(c, ok, p);
    c.flag(2, job_compress<Fq>(c.in_bytes(0), c.bytes(kConfWrap)));
  } else if constexpr (OP == G2_DECODE_UNCOMPRESSED) {
    G2Affine p = G2Affine::infinity();
    const bool ok = g2_decode_uncompressed(c.in_bytes(0), p);
    put_decoded(c, ok, p);
    c.flag(2, job_compress<Fq2>(c.in_bytes(0), c.bytes(kConfWrap)));
  } else if constexpr (OP == G1_DECODE_COMPRESSED) {
    G1Affine p = G1Affine::infinity();
    const bool ok = g1_decode_compressed(c.in_bytes(0), p);
    put_decoded(c, ok, p);
    c.flag(2, job_decompress<Fq>(c.in_bytes(0), c.bytes(kConfWrap)));
  } else if constexpr (OP == G2_DECODE_COMPRESSED) {
    G2Affine p = G2Affine::infinity();
    const bool ok = g2_decode_compressed(c.in_bytes(0), p);
    put_decoded(c, ok, p);
    c.flag(2, job_decompress<Fq2>(c.in_bytes(0), c.bytes(kConfWrap)));
  } else if constexpr (OP == G2_DECODE_COMPRESSED_X2) {
    // encodings at bytes 0 and 96; points at slots 0 and 4, flags 0 / 1 = verdict + 2 * infinity of A / B; the wrapper's
    // outputs from slot 10 on (A, then B unless aux[0]: out_b null), flags 2 / 3 = its statuses
    G2Affine pa, pb;
    bool oka, okb;
    g2_decode_compressed_x2(c.in_bytes(0), c.in_bytes(96), pa, pb, oka, okb);
    put_aff(c, 0, pa);
    put_aff(c, 4, pb);
    c.flag(0, (int)oka | ((int)pa.inf << 1));
    c.flag(1, (int)okb | ((int)pb.inf << 1));
    uint8_t sa = 0xee, sb = 0xee;
    job_decompress_g2_x2(c.in_bytes(0), c.in_bytes(96), c.bytes(kConfWrap), c.aux[0] ? nullptr : c.bytes(kConfWrap + 192), sa, sb);
    c.flag(2, sa);
    c.flag(3, sb);
  // ---- encode: an affine point in limbs (aux[0] = at infinity) to bytes ----
  } else if constexpr (OP == G1_ENCODE_UNCOMPRESSED) {
    g1_encode_uncompressed(aff_at<Fq>(c, 0, c.aux[0]), c.bytes(0));
  } else if constexpr (OP == G1_ENCODE_COMPRESSED) {
    g1_encode_compressed(aff_at<Fq>(c, 0, c.aux[0]), c.bytes(0));
  } else if constexpr (OP == G2_ENCODE_UNCOMPRESSED) {
    g2_encode_uncompressed(aff_at<Fq2>(c, 0, c.aux[0]), c.bytes(0));
  } else if constexpr (OP == G2_ENCODE_COMPRESSED) {
    g2_encode_compressed(aff_at<Fq2>(c, 0, c.aux[0]), c.bytes(0));
  // ---- the hash onto G2 ----
  } else if constexpr (OP == G2_RANDOM_FROM_SEED || OP == G2_RANDOM_FROM_SEED_X2) {
    // seed(s) = the words of slot 0 (and 1); aux[0] = fix; aux[1] = outer rounds to force (a build with TC_TEST_HOOKS only:
    // the last flag says how many were forced, so the check knows which candidate it is looking at)
    int forced = 0;
#if defined(TC_TEST_HOOKS)
    forced = g_tc_force_extra_rounds = c.aux[1];
#endif
    if constexpr (OP == G2_RANDOM_FROM_SEED) {
      put_result(c, g2_random_from_seed(c.words(0), c.aux[0] != 0));
      c.flag(1, forced);
    } else {
      Seed8 sa, sb;
      TC_UNROLL for (int i = 0; i < 8; i++) {
        sa.w[i] = c.words(0)[i];
        sb.w[i] = c.words(1)[i];
      }
      G2Jac ra, rb;
      g2_random_from_seed_x2(duo_pick(sa, sb), c.aux[0] != 0, ra, rb);
      put_jac(c, 0, ra);
      put_jac(c, 6, rb);
      G2Affine pa, pb;
      jac_to_affine_x2(ra, rb, pa, pb);
      put_aff(c, 12, pa);
      put_aff(c, 16, pb);
      c.flag(0, pa.inf);
      c.flag(1, pb.inf);
      c.flag(2, forced);
    }
#if defined(TC_TEST_HOOKS)
    g_tc_force_extra_rounds = 0;
#endif
  } else if constexpr (OP == HASH_G2) {  // aux[0] = len, aux[1] = fix
    job_hash_g2(c.in_bytes(0), (size_t)c.aux[0], c.bytes(0), c.aux[1] != 0);
  } else if constexpr (OP == HASH_G2_X2) {  // aux[0], aux[1] = lengths, aux[2] = fix + 2 * (out_b null)
    job_hash_g2_x2(c.in_bytes(0), (size_t)c.aux[0], c.in_bytes(kConfMsgB2), (size_t)c.aux[1], c.bytes(0),
                   (c.aux[2] & 2) ? nullptr : c.bytes(192), (c.aux[2] & 1) != 0);
  } else if constexpr (OP == HASH_G1_G2) {
    c.flag(0, job_hash_g1_g2(c.in_bytes(0), c.in_bytes(kConfMsg), (size_t)c.aux[0], c.bytes(0), c.aux[1] != 0));
  } else if constexpr (OP == HASH_G1_G2_X2) {
    uint8_t sa = 0xee, sb = 0xee;
    job_hash_g1_g2_x2(c.in_bytes(0), c.in_bytes(kConfMsgA4), (size_t)c.aux[0], c.in_bytes(kConfG1B), c.in_bytes(kConfMsgB4),
                      (size_t)c.aux[1], c.bytes(0), (c.aux[2] & 2) ? nullptr : c.bytes(192), (c.aux[2] & 1) != 0, sa, sb);
    c.flag(0, sa);
    c.flag(1, sb);
  } else if constexpr (OP == JOB_COMBINE_SMALL_G2) {
    // aux[0] = K uncompressed shares at bytes 192 k, the K indices as u64 at byte kConfIdx; out: the 192 bytes of the
    // combination (nothing where the fast path does not take the job); flag 0 = the status, flag 1 = the return value
    if (c.aux[0] == 2) conf_combine_small<2>(c);
    if (c.aux[0] == 3) conf_combine_small<3>(c);
    if (c.aux[0] == 4) conf_combine_small<4>(c);
  }
}

template <int OP>
TC_HD void conf_op(Ctx& c) {
  // ---- Fq ---------------------------------------------------------------------------------------------------------
  if constexpr (OP == FQ_MUL) {
    c.put(0, c.fq(0) * c.fq(1));
  } else if constexpr (OP == FQ_SQR) {
    c.put(0, c.fq(0).sqr());
  } else if constexpr (OP == FQ_REDC_FULL) {
    int32_t t[FQ_LIMBS];
    fq_redc_full(c.fq(0), t);
    c.put_raw(0, t, FQ_LIMBS);
  } else if constexpr (OP == FQ_FROM_CANONICAL) {
    c.put(0, Fq::from_canonical(c.words(0)));
  } else if constexpr (OP == FQ_TO_CANONICAL) {
    uint32_t w[12];
    c.fq(0).to_canonical(w);
    c.put_raw(0, (const int32_t*)w, 12);
  } else if constexpr (OP == FQ_FROM_MONT384) {
    c.put(0, Fq::from_mont384(c.words(0)));
  } else if constexpr (OP == FQ_GT_HALF) {
    c.flag(0, fq_canonical_gt_half(c.words(0)));
  } else if constexpr (OP == FQ_NORM) {
    c.put(0, c.fq(0).norm());
  } else if constexpr (OP == FQ_REDUCE_VALUE) {
    c.put(0, c.fq(0).reduce_value());
  } else if constexpr (OP == FQ_ZERO) {
    const Fq a = c.fq(0), b = c.fq(1);
    c.flag(0, a.maybe_zero());
    c.flag(1, a.maybe_zero56());
    c.flag(2, a.is_zero());
    if (c.aux[0]) c.flag(3, a == b);  // (only where a - b is inside the input contract)
  } else if constexpr (OP == FQ_INV) {
    c.put(0, c.fq(0).inv());
  } else if constexpr (OP == FQ_INV_FERMAT) {
    c.put(0, fq_inv_fermat(c.fq(0)));
  } else if constexpr (OP == FQ_INV30) {
    int32_t r[FQ_INV_LIMBS];
    fq_inv_limbs30(c.in, r);
    c.put_raw(0, r, FQ_INV_LIMBS);
  } else if constexpr (OP == FQ_LEGENDRE) {
    c.flag(0, fq_legendre(c.fq(0)));
  } else if constexpr (OP == FQ_SQRT) {
    Fq root, inv_root;
    const bool ok = fq_sqrt(c.fq(0), root, &inv_root);
    c.put(0, root);
    c.put(1, inv_root);
    c.flag(0, ok);
  // ---- Fq2 --------------------------------------------------------------------------------------------------------
  } else if constexpr (OP == FQ2_MUL) {
    c.put(0, c.fq2(0) * c.fq2(2));
  } else if constexpr (OP == FQ2_SQR) {
    c.put(0, c.fq2(0).sqr());
  } else if constexpr (OP == FQ2_CONJ) {
    c.put(0, c.fq2(0).conj());
  } else if constexpr (OP == FQ2_MUL_XI) {
    c.put(0, c.fq2(0).mul_xi());
  } else if constexpr (OP == FQ2_NORM_FQ) {
    c.put(0, c.fq2(0).norm_fq());
  } else if constexpr (OP == FQ2_INV) {
    c.put(0, c.fq2(0).inv());
  } else if constexpr (OP == FQ2_ZERO) {
    const Fq2 a = c.fq2(0), b = c.fq2(2);
    c.flag(0, a.is_zero());
    c.flag(1, maybe_zero56(a));
    if (c.aux[0]) c.flag(2, a == b);
  } else if constexpr (OP == FQ2_SQRT) {
    const Fq2 a = c.fq2(0);
    Fq2 r = Fq2::zero();
    c.flag(1, fq2_is_square(a, a.norm_fq()));
    const bool ok = fq2_sqrt(a, r);
    c.put(0, r);
    c.flag(0, ok);
  } else if constexpr (OP == FQ2_SQRT_X2) {
    Fq2 ya, yb;
    bool oka, okb;
    fq2_sqrt_x2(c.fq2(0), c.fq2(2), ya, yb, oka, okb);
    c.put(0, ya);
    c.put(2, yb);
    c.flag(0, oka);
    c.flag(1, okb);
  } else if constexpr (OP == FQ2_INV_X2) {
    Fq2 ia, ib;
    fq2_inv_x2(c.fq2(0), c.fq2(2), ia, ib);
    c.put(0, ia);
    c.put(2, ib);
  // ---- Fq6 / Fq12 -------------------------------------------------------------------------------------------------
  } else if constexpr (OP == FQ6_MUL) {
    c.put(0, c.fq6(0) * c.fq6(6));
  } else if constexpr (OP == FQ6_SQR) {
    c.put(0, c.fq6(0).sqr());
  } else if constexpr (OP == FQ6_INV) {
    c.put(0, c.fq6(0).inv());
  } else if constexpr (OP == FQ12_MUL) {
    c.put(0, c.fq12(0) * c.fq12(12));
  } else if constexpr (OP == FQ12_SQR) {
    c.put(0, c.fq12(0).sqr());
  } else if constexpr (OP == FQ12_INV) {
    c.put(0, c.fq12(0).inv());
  } else if constexpr (OP == FQ12_FROB) {
    c.put(0, c.fq12(0).frobenius(c.aux[0]));
  } else if constexpr (OP == FQ12_CONJ) {
    c.put(0, c.fq12(0).conj());
  } else if constexpr (OP == FQ12_LINE_PRODUCT) {
    c.put(0, Fq12::line_product(c.fq2(0), c.fq2(2), c.fq2(4), c.fq2(6), c.fq2(8), c.fq2(10)));
  } else if constexpr (OP == FQ12_CYCLO_SQR) {
    c.put(0, c.fq12(0).cyclotomic_sqr());
  } else if constexpr (OP == CYCLO_CHAIN) {
    // three compressed elements (z2, z3, z4, z5 at slots 8 i), kCycloReduceEvery squarings each -- the last one reducing,
    // as in the chain of cyclotomic_exp_by_x --, then decompressed together
    CycloCompressed z[3];
    TC_UNROLL for (int i = 0; i < 3; i++) {
      CycloCompressed t{c.fq2(8 * i), c.fq2(8 * i + 2), c.fq2(8 * i + 4), c.fq2(8 * i + 6)};
      TC_NOUNROLL for (int s = 0; s < kCycloReduceEvery - 1; s++) t = t.sqr_t<false>();
      z[i] = t.sqr_t<true>();
    }
    Fq12 f[3];
    cyclotomic_decompress3(z, f);
    TC_UNROLL for (int i = 0; i < 3; i++) c.put(12 * i, f[i]);
  // ---- G1 / G2 ----------------------------------------------------------------------------------------------------
  } else if constexpr (OP >= G1_DBL && OP <= G1_ON_CURVE) {
    conf_curve<Fq, OP - G1_DBL>(c);
  } else if constexpr (OP == G1_IN_SUBGROUP) {
    c.flag(0, g1_in_subgroup(aff_at<Fq>(c, 0, c.aux[0])));
  } else if constexpr (OP >= G2_DBL && OP <= G2_TO_AFFINE) {
    conf_curve<Fq2, OP - G2_DBL>(c);
  } else if constexpr (OP == G2_TO_AFFINE_X2) {
    G2Affine pa, qa;
    jac_to_affine_x2(jac_at<Fq2>(c, 0), jac_at<Fq2>(c, 6), pa, qa);
    put_aff(c, 0, pa);
    put_aff(c, 4, qa);
    c.flag(0, pa.inf);
    c.flag(1, qa.inf);
  } else if constexpr (OP == G2_ON_CURVE) {
    conf_curve<Fq2, 6>(c);
  } else if constexpr (OP == G2_IN_SUBGROUP) {
    c.flag(0, g2_in_subgroup(aff_at<Fq2>(c, 0, c.aux[0])));
  } else if constexpr (OP == G2_PSI) {
    put_aff(c, 0, g2_psi(aff_at<Fq2>(c, 0, c.aux[0])));
  // ---- the pairing ------------------------------------------------------------------------------------------------
  } else if constexpr (OP >= MILLER_DBL_STEP && OP < FR_ADD) {
    conf_pairing<OP>(c);
  // ---- the scalar block -------------------------------------------------------------------------------------------
  } else if constexpr (OP >= FR_ADD && OP < G1_ADD_AFFINE) {
    conf_scalar<OP>(c);
  // ---- the point-multiplication block -------------------------------------------------------------------------------
  } else if constexpr (OP >= G1_ADD_AFFINE && OP < SHA3_256) {
    conf_mul<OP>(c);
  // ---- the byte layer -------------------------------------------------------------------------------------------------
  } else if constexpr (OP >= SHA3_256) {
    conf_bytes<OP>(c);
  }
}

// every op, for the launchers' switch
#define TC_CONF_OPS(X)                                                                                                  \
  X(FQ_MUL) X(FQ_SQR) X(FQ_REDC_FULL) X(FQ_FROM_CANONICAL) X(FQ_TO_CANONICAL) X(FQ_FROM_MONT384) X(FQ_GT_HALF)          \
  X(FQ_NORM) X(FQ_REDUCE_VALUE) X(FQ_ZERO) X(FQ_INV) X(FQ_INV_FERMAT) X(FQ_INV30) X(FQ_LEGENDRE) X(FQ_SQRT)            \
  X(FQ2_MUL) X(FQ2_SQR) X(FQ2_CONJ) X(FQ2_MUL_XI) X(FQ2_NORM_FQ) X(FQ2_INV) X(FQ2_ZERO) X(FQ2_SQRT) X(FQ2_SQRT_X2)     \
  X(FQ2_INV_X2) X(FQ6_MUL) X(FQ6_SQR) X(FQ6_INV) X(FQ12_MUL) X(FQ12_SQR) X(FQ12_INV) X(FQ12_FROB) X(FQ12_CONJ)         \
  X(FQ12_LINE_PRODUCT) X(FQ12_CYCLO_SQR) X(CYCLO_CHAIN) X(G1_DBL) X(G1_ADD_MIXED) X(G1_ADD) X(G1_ADD_MIXED_GENERIC)    \
  X(G1_ADD_GENERIC) X(G1_TO_AFFINE) X(G1_ON_CURVE) X(G1_IN_SUBGROUP) X(G2_DBL) X(G2_ADD_MIXED) X(G2_ADD)               \
  X(G2_ADD_MIXED_GENERIC) X(G2_ADD_GENERIC) X(G2_TO_AFFINE) X(G2_TO_AFFINE_X2) X(G2_ON_CURVE) X(G2_IN_SUBGROUP) X(G2_PSI) \
  X(MILLER_DBL_STEP) X(MILLER_ADD_STEP) X(MILLER_LOOP2) X(MILLER_LINES) X(CYCLO_EXP_BY_X) X(CYCLO_EXP_BY_X_HALF)           \
  X(FINAL_EXP) X(PAIRING_CHECK) X(Q_MILLER_LOOP) X(Q_EXP_BY_X) X(Q_EXP_BY_X_HALF) X(Q_FINAL_EXP) X(Q_PAIRING_CHECK)     \
  X(FR_ADD) X(FR_SUB) X(FR_MUL) X(FR_SQR) X(FR_INV) X(FR_FROM_CANONICAL) X(FR_TO_CANONICAL) X(FR_FROM_U64) X(FR_FROM_LE32)   \
  X(FR_SCALE_COFACTOR_FIX) X(DIV_BY_X_ABS) X(GLS_DECOMPOSE) X(GLS_DECOMPOSE_ODD) X(SAC_RECODE4) X(GLV_DECOMPOSE)              \
  X(GLV_RECODE_SIGN_ALIGNED) X(MSM_G1_RECODE) X(LAGRANGE_COEFF) X(LAGRANGE_COEFF_FR) X(LAGRANGE_ALL) X(LAGRANGE_SPLIT)      \
  X(LAGRANGE_SMALL_COEFFS) X(COMBINE_CLASS) X(FR_INVERSE_OF_SMALL) X(GCD_U64) X(WNAF_RECODE)                            \
  X(COMBINE_QUOTIENT_DECOMPOSE) X(COMBINE_DIVIDE_CHOICE)                                                                \
  X(G1_ADD_AFFINE) X(G1_COMMON_Z) X(G1_MUL_BY_X_ABS) X(G1_MUL_GLV) X(G1_MUL_GLV_JAC) X(G1_MUL_GLV_ARENA)                \
  X(G1_LINCOMB_CHUNK4) X(G1_STRAUS_SMALL) X(G1_STRAUS_SMALL_INLINE) X(G1_COMBINE_DIVIDE) X(G1_COMBINE_DIVIDE_ARENA)     \
  X(G1_MUL_U64) X(G2_ADD_AFFINE) X(G2_COMMON_Z) X(G2_MUL_BY_X_ABS) X(G2_PSI_JAC) X(G2_GLS_BASES) X(G2_SAC_TABLE)        \
  X(G2_JOINT_MUL4) X(G2_MUL_GLS) X(G2_MUL_GLS_JAC) X(G2_CLEAR_COFACTOR) X(G2_STRAUS_SMALL) X(G2_COMBINE_DIVIDE)      \
  X(G2_STRAUS_SMALL_UNIFORM) X(G2_WNAF_TABLE) X(G2_COMBINE_DIVIDE_UNIFORM) X(G2_COMBINE_DIVIDE_QUOTIENT) X(G2_QUOTIENT_MUL) \
  X(G2_COMBINE_UNIFORM_WAVE)                                                                                            \
  X(SHA3_256) X(CHACHA_WORDS) X(FQ_RANDOM) X(XOR_WITH_HASH) X(FQ_FROM_BE48) X(FQ_TO_BE48) X(FQ_LEX_LARGEST)             \
  X(G1_DECODE_UNCOMPRESSED) X(G1_ENCODE_UNCOMPRESSED) X(G1_ENCODE_COMPRESSED) X(G1_DECODE_COMPRESSED)                   \
  X(G2_RANDOM_FROM_SEED) X(G2_RANDOM_FROM_SEED_X2) X(HASH_G2) X(HASH_G2_X2) X(HASH_G1_G2) X(HASH_G1_G2_X2)              \
  X(FQ2_FROM_BE96) X(FQ2_TO_BE96) X(FQ2_LEX_LARGEST) X(G2_DECODE_UNCOMPRESSED) X(G2_ENCODE_UNCOMPRESSED)                \
  X(G2_ENCODE_COMPRESSED) X(G2_DECODE_COMPRESSED) X(G2_DECODE_COMPRESSED_X2) X(JOB_COMBINE_SMALL_G2)

}  // namespace conf
}  // namespace tc
