// gfx950 kernels: batched pairing-product check  e(a,b) == e(c,d).
#include "tc_jobs.h"
#include "tc_launch.h"
#include "tc_stage.h"
#include "tc_quad.h"

#include <stdlib.h>

namespace tc {

// One lane pair per check.  The four operands of the wave's 32 checks are moved through ONE LDS row buffer with
// coalesced 8-byte loads (tc_stage.h), one operand after the other; a stride of 0 broadcasts one record.
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_pairing_check(const uint8_t* __restrict__ a, size_t sa,
                                                          const uint8_t* __restrict__ b, size_t sb,
                                                          const uint8_t* __restrict__ c, size_t sc,
                                                          const uint8_t* __restrict__ d, size_t sd, size_t B,
                                                          uint8_t* __restrict__ ok) {
  using IO1 = WaveRowIO<96, kG2Lanes>;
  using IO2 = WaveRowIO<192, kG2Lanes>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[IO2::BYTES];
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const bool live = j < B;
  const size_t jj = live ? j : 0;
  IO1 ia{lds, live ? a + jj * sa : nullptr, 0, nullptr}, ic{lds, live ? c + jj * sc : nullptr, 0, nullptr};
  IO2 ib{lds, live ? b + jj * sb : nullptr, 0, nullptr}, id{lds, live ? d + jj * sd : nullptr, 0, nullptr};
  const uint8_t r = job_pairing_check_io(live, ia, ib, ic, id);
  if (live && pair_leader()) ok[j] = r;
}

// ---- the same check as two kernels --------------------------------------------------------------------------
// The Miller loop and the final exponentiation have disjoint live sets (point arithmetic + sparse products against a
// running Fq12 / cyclotomic chains on three or four Fq12 values): compiled as ONE kernel the register allocator
// serves the union (1 994 spilled registers, 9.6 KB of scratch per lane).  As two kernels each half gets its own
// allocation; the Miller value travels through HBM in the lane-pair row layout: word w of lane l of wave v at
// fbuf[(v * kFq12Words + w) * 64 + l] -- every store / load instruction moves one full 256-byte row.
constexpr int kFq12Words = 6 * FQ_LIMBS;  // per lane: one coefficient of each of the six Fq2
#if TC_PAIR
__device__ __forceinline__ void fq12_store_rows(int32_t* __restrict__ rows, const Fq12& f) {
  const Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  TC_UNROLL for (int k = 0; k < 6; k++) {
    const Fq v = c[k]->m.reduce_value();
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) rows[(k * FQ_LIMBS + i) * 64] = v.l[i];
  }
}
__device__ __forceinline__ Fq12 fq12_load_rows(const int32_t* __restrict__ rows) {
  Fq12 f;
  Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  TC_UNROLL for (int k = 0; k < 6; k++) {
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) c[k]->m.l[i] = rows[(k * FQ_LIMBS + i) * 64];
  }
  return f;
}
#else
__device__ __forceinline__ void fq12_store_rows(int32_t*, const Fq12&) {}
__device__ __forceinline__ Fq12 fq12_load_rows(const int32_t*) { return Fq12::one(); }
#endif

__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_miller_loop(const uint8_t* __restrict__ a, size_t sa,
                                                        const uint8_t* __restrict__ b, size_t sb,
                                                        const uint8_t* __restrict__ c, size_t sc,
                                                        const uint8_t* __restrict__ d, size_t sd, size_t B,
                                                        int32_t* __restrict__ fbuf, uint8_t* __restrict__ ok) {
  using IO1 = WaveRowIO<96, kG2Lanes>;
  using IO2 = WaveRowIO<192, kG2Lanes>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[IO2::BYTES];
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const bool live = j < B;
  const size_t jj = live ? j : 0;
  IO1 ia{lds, live ? a + jj * sa : nullptr, 0, nullptr}, ic{lds, live ? c + jj * sc : nullptr, 0, nullptr};
  IO2 ib{lds, live ? b + jj * sb : nullptr, 0, nullptr}, id{lds, live ? d + jj * sd : nullptr, 0, nullptr};
  Fq12 f = Fq12::one();
  const bool good = job_miller_io(live, ia, ib, ic, id, f);
  fq12_store_rows(fbuf + (size_t)blockIdx.x * kFq12Words * 64 + threadIdx.x, f);
  if (live && pair_leader()) ok[j] = good ? 1 : 0;  // 0: an operand did not decode; the second kernel keeps it
}

__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_final_exp(const int32_t* __restrict__ fbuf, size_t B, uint8_t* __restrict__ ok) {
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const Fq12 f = fq12_load_rows(fbuf + (size_t)blockIdx.x * kFq12Words * 64 + threadIdx.x);
  const uint8_t r = job_final_exp_is_one(f);
  if (j < B && pair_leader() && ok[j]) ok[j] = r;
}

// ---- the Miller loop as two kernels: prepared line products in HBM (tc_pairing.h) ---------------------------------------
// k_miller_lines (stage P: the two Miller points, their lines, the product of the two lines of a step) writes 68 x 5 Fq2
// coefficients per check into the wave's row block -- word w of lane l of wave v at lines[(v * kLineWords + w) * 64 + l],
// 256-byte rows, 39 KB per check --, k_miller_accumulate (stage M: the Fq12 accumulator) streams them back and leaves the
// Miller value for k_final_exp.
constexpr int kLineWords = kMillerRowSlots * FQ_LIMBS;  // per lane: operands, one parked line, 68 x 5 product coefficients
#ifndef TC_WAVES_MILLER_P
#define TC_WAVES_MILLER_P TC_WAVES_G2
#endif
#ifndef TC_WAVES_MILLER_M
#define TC_WAVES_MILLER_M TC_WAVES_G2
#endif
#if TC_PAIR
__global__ __launch_bounds__(kBlock, TC_WAVES_MILLER_P) void k_miller_lines(const uint8_t* __restrict__ a, size_t sa,
                                                         const uint8_t* __restrict__ b, size_t sb,
                                                         const uint8_t* __restrict__ c, size_t sc,
                                                         const uint8_t* __restrict__ d, size_t sd, size_t B,
                                                         int32_t* lines, uint8_t* __restrict__ ok) {  // (lines: read back through laundered pointers, tc_pairing.h rows_after: no restrict)
  using IO1 = WaveRowIO<96, kG2Lanes>;
  using IO2 = WaveRowIO<192, kG2Lanes>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[IO2::BYTES];
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const bool live = j < B;
  const size_t jj = live ? j : 0;
  IO1 ia{lds, live ? a + jj * sa : nullptr, 0, nullptr}, ic{lds, live ? c + jj * sc : nullptr, 0, nullptr};
  IO2 ib{lds, live ? b + jj * sb : nullptr, 0, nullptr}, id{lds, live ? d + jj * sd : nullptr, 0, nullptr};
  const bool good = job_miller_lines_io(live, ia, ib, ic, id, Fq2Rows::at(lines + (size_t)blockIdx.x * kLineWords * 64 + threadIdx.x));
  if (live && pair_leader()) ok[j] = good ? 1 : 0;  // 0: an operand did not decode; the later kernels keep it
}

__global__ __launch_bounds__(kBlock, TC_WAVES_MILLER_M) void k_miller_accumulate(const int32_t* lines, int32_t* __restrict__ fbuf) {
  const Fq12 f = miller_accumulate(Fq2Rows::at(const_cast<int32_t*>(lines) + (size_t)blockIdx.x * kLineWords * 64 + threadIdx.x));
  fq12_store_rows(fbuf + (size_t)blockIdx.x * kFq12Words * 64 + threadIdx.x, f);
}
#else
__global__ void k_miller_lines(const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*, size_t, size_t, int32_t*, uint8_t*) {}
__global__ void k_miller_accumulate(const int32_t*, int32_t*) {}
#endif

// ---- four lanes per check (tc_quad.h) -----------------------------------------------------------------------------------
// Pair A of a quad stages and decodes (a, b), pair B (c, d): two passes through the LDS row buffer with a PAIR as the
// staging unit (32 rows per wave), each pair parses one G1 and one G2 record.
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_pairing_quad(const uint8_t* __restrict__ a, size_t sa,
                                                         const uint8_t* __restrict__ b, size_t sb,
                                                         const uint8_t* __restrict__ c, size_t sc,
                                                         const uint8_t* __restrict__ d, size_t sd, size_t B,
                                                         uint8_t* __restrict__ ok) {
  using IO1 = WaveRowIO<96, kG2Lanes>;
  using IO2 = WaveRowIO<192, kG2Lanes>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[IO2::BYTES];
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kQuadLanes;
  const bool live = j < B;
  const size_t jj = live ? j : 0;
  const bool hi = quad_hi();
  IO1 i1{lds, live ? (hi ? c + jj * sc : a + jj * sa) : nullptr, 0, nullptr};
  IO2 i2{lds, live ? (hi ? d + jj * sd : b + jj * sb) : nullptr, 0, nullptr};
  const uint8_t r = job_pairing_check_quad_io(live, i1, i2);
  if (live && (threadIdx.x & (kQuadLanes - 1)) == 0) ok[j] = r;
}

// Which form runs (Tuning::pairing_form, from TC_PAIRING_FORM = quad | lines | pair | fused when the context was created, overrides
// the choice for experiments):
//   four lanes per check (k_pairing_quad) up to kQuadMaxBatch checks -- the batch alone cannot give every SIMD two waves of
//     the lane-pair kernels, and a check finishes in about 0.6 of the time (6.9 instead of 10.9 ms at 4 096 checks, 8.5
//     instead of 11.4 ms at 16 384: profiles/r03_pairing_forms.txt);
//   above it the PREPARED form: k_miller_lines -> k_miller_accumulate -> k_final_exp (r04; 206 / 142 / 4 spilled registers,
//     12.99 ms for the two Miller kernels against 13.1-13.2 ms for the one loop with its 2 238: profiles/r04_pairing_*);
//   `pair` = r03's k_miller_loop + k_final_exp, `fused` = r02's single kernel.
constexpr size_t kQuadMaxBatch = 16384;
enum PairingForm { kFormQuad, kFormLines, kFormPair, kFormFused };
int pairing_form(size_t B, const Tuning& tn) {
  if (tn.pairing_form >= 1 && tn.pairing_form <= 4) return tn.pairing_form - 1;
  return B <= kQuadMaxBatch ? kFormQuad : kFormLines;
}
bool pairing_form_needs_lines(int form) { return form == kFormLines; }
// checks per pass of the prepared form: its line buffer (kLineWords = 552 x 14 words per lane: 61.8 KB per check, 4.05 GB for
// 65 536 checks) is sized for one tile, larger batches run tile by tile.  The tile shrinks to what the caller's budget holds
// (a third of the free HBM: several contexts on one GPU, a smaller card), in whole rounds of 2 048 waves down to 16 384
// checks; below that the one-loop form (k_miller_loop + k_final_exp, no line buffer) runs instead of failing an allocation.
constexpr size_t kPreparedTile = 65536;
constexpr size_t kPreparedMinTile = 16384;
size_t pairing_tile(size_t B, size_t budget_bytes) {
  const size_t per_check = (size_t)kG2Lanes * kLineWords * sizeof(int32_t);
  size_t tile = kPreparedTile;
  while (tile > kPreparedMinTile && tile * per_check > budget_bytes) tile /= 2;
  if (tile * per_check > budget_bytes) return 0;
  return B < tile ? B : tile;
}
size_t pairing_ws_words(size_t B, size_t tile) {
  return (size_t)grid_for(B * kG2Lanes) * kFq12Words * 64 + (tile ? (size_t)grid_for(tile * kG2Lanes) * kLineWords * 64 : 0);
}

void launch_pairing_check(hipStream_t st, const uint8_t* a, size_t sa, const uint8_t* b, size_t sb, const uint8_t* c,
                          size_t sc, const uint8_t* d, size_t sd, size_t B, uint8_t* ok, PairingWs pws) {
  if (!B) return;
  int32_t* ws = pws.p;
  int form = pws.form;
  if (form == kFormLines && !pws.tile) form = kFormPair;  // no room for the line buffer
  if (form == kFormQuad) {
    hipLaunchKernelGGL(k_pairing_quad, dim3(grid_for(B * kQuadLanes)), dim3(kBlock), 0, st, a, sa, b, sb, c, sc, d, sd, B, ok);
    return;
  }
  if (form == kFormFused || !ws) {
    hipLaunchKernelGGL(k_pairing_check, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, a, sa, b, sb, c, sc, d, sd, B, ok);
    return;
  }
  if (form == kFormPair) {
    hipLaunchKernelGGL(k_miller_loop, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, a, sa, b, sb, c, sc, d, sd, B, ws, ok);
    hipLaunchKernelGGL(k_final_exp, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, (const int32_t*)ws, B, ok);
    return;
  }
  // prepared form: lines (stage P) -> accumulator (stage M) tile by tile through one line buffer, then ONE final exponentiation launch
  int32_t* lines = ws + (size_t)grid_for(B * kG2Lanes) * kFq12Words * 64;
  for (size_t lo = 0; lo < B; lo += pws.tile) {
    const size_t cnt = (B - lo < pws.tile) ? B - lo : pws.tile;
    const unsigned grid = grid_for(cnt * kG2Lanes);
    int32_t* fb = ws + (size_t)grid_for(lo * kG2Lanes) * kFq12Words * 64;
    hipLaunchKernelGGL(k_miller_lines, dim3(grid), dim3(kBlock), 0, st, a + lo * sa, sa, b + lo * sb, sb, c + lo * sc, sc, d + lo * sd, sd, cnt,
                       lines, ok + lo);
    hipLaunchKernelGGL(k_miller_accumulate, dim3(grid), dim3(kBlock), 0, st, (const int32_t*)lines, fb);
  }
  hipLaunchKernelGGL(k_final_exp, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, (const int32_t*)ws, B, ok);
}

// ---- product of n pairings per job:  prod_k e(a_k, b_k) == 1  (optionally == e(c, d)) --------------------------------------------
// Miller stage: one lane pair takes two CONSECUTIVE pairs of a job (miller_loop<2>: the two share the accumulator's squarings);
// lane pair p = j * H + h, H = ceil(n / 2), works on pairs 2h and 2h + 1 of job j -- an odd last pair has an empty partner -- and
// leaves its value in the row layout of k_miller_loop, value p in the lane pair p % 32 of wave p / 32.  NEG: the G1 operands are
// negated (the right-hand side of "== e(c, d)", one pair per job).  An operand that does not decode marks its JOB failed
// (ok[j] = 0, preset to 1 by the launcher; several lane pairs of a job may store the same 0) and contributes the empty product.
template <bool NEG>
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_miller_pairs(const uint8_t* __restrict__ a, size_t sa, const uint8_t* __restrict__ b,
                                                                      size_t sb, size_t n, size_t B, int32_t* __restrict__ fbuf,
                                                                      uint8_t* __restrict__ ok) {
  using IO1 = WaveRowIO<96, kG2Lanes>;
  using IO2 = WaveRowIO<192, kG2Lanes>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[IO2::BYTES];
  const size_t H = (n + 1) / 2;
  const size_t p = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const size_t j = p / H, k0 = 2 * (p % H);
  const bool live0 = j < B, live1 = live0 && k0 + 1 < n;
  const size_t r0 = live0 ? j * n + k0 : 0;
  IO1 ia0{lds, live0 ? a + r0 * sa : nullptr, 0, nullptr}, ia1{lds, live1 ? a + (r0 + 1) * sa : nullptr, 0, nullptr};
  IO2 ib0{lds, live0 ? b + r0 * sb : nullptr, 0, nullptr}, ib1{lds, live1 ? b + (r0 + 1) * sb : nullptr, 0, nullptr};
  Fq12 f = Fq12::one();
  const bool good = job_miller_pairs_io<NEG>(live0, live1, ia0, ib0, ia1, ib1, f);
  fq12_store_rows(fbuf + (size_t)blockIdx.x * kFq12Words * 64 + threadIdx.x, f);
  if (live0 && !good && pair_leader()) ok[j] = 0;
}

// Product stage: `hin` values per job (value j * hin + h in the lane pair (j * hin + h) % 32 of wave (j * hin + h) / 32 of `in`)
// are multiplied down to hout = ceil(hin / S) values per job, S (a power of two, at most 32) adjacent lane pairs per product:
// log2(S) rounds of one exchange over the wave's crossbar (ds_bpermute, msm_from_partner's pattern) and one Fq12 multiplication,
// every lane pair of the S ending with the whole product; the first one stores it as value j * hout + c of `out`.  hout == 1 is
// the last pass: its output is what k_final_exp reads (job j in lane pair j % 32 of wave j / 32), times the job's value of
// `extra` (the same layout) when there is one.  Slots past the last job get the value 1, so the final exponentiation of a
// partial wave runs on defined data.  A job that spans waves (hin > 32) takes more than one pass, through HBM.
#if TC_PAIR
__device__ __forceinline__ Fq12 fq12_from_lane_xor(const Fq12& f, int lanes) {
  Fq12 r;
  const Fq2* s[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  Fq2* d[6] = {&r.c0.c0, &r.c0.c1, &r.c0.c2, &r.c1.c0, &r.c1.c1, &r.c1.c2};
  TC_UNROLL for (int k = 0; k < 6; k++) {
    TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) d[k]->m.l[i] = __shfl_xor(s[k]->m.l[i], lanes, 64);
  }
  return r;
}
__device__ __forceinline__ size_t fq12_row_slot(size_t value, unsigned odd) {  // first word of `value`'s column, this lane's half
  return (value / 32) * kFq12Words * 64 + 2 * (value % 32) + odd;
}
// (one wave per SIMD: two Fq12 values and the temporaries of their product do not fit 256 registers, and the kernel is short)
__global__ __launch_bounds__(kBlock, 1) void k_fq12_product(const int32_t* __restrict__ in, size_t hin, unsigned S, size_t hout, size_t B,
                                                                      const int32_t* __restrict__ extra, int32_t* __restrict__ out) {
  const size_t p = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const unsigned odd = threadIdx.x & 1u;
  const size_t g = p / S, t = p % S;     // product g = (job, chunk), this lane pair's place in it
  const size_t j = g / hout, c = g % hout, h = c * S + t;
  const bool live = j < B;
  Fq12 f = Fq12::one();
  if (live && h < hin) f = fq12_load_rows(in + fq12_row_slot(j * hin + h, odd));
  TC_NOUNROLL for (unsigned d = 1; d < S; d <<= 1) f = f * fq12_from_lane_xor(f, (int)(d * kG2Lanes));
  if (extra && hout == 1) {  // (kernel-uniform)
    Fq12 e = Fq12::one();
    if (live && t == 0) e = fq12_load_rows(extra + fq12_row_slot(j, odd));
    f = f * e;
  }
  if (t == 0) fq12_store_rows(out + fq12_row_slot(g, odd), f);
}
#else
__global__ void k_fq12_product(const int32_t*, size_t, unsigned, size_t, size_t, const int32_t*, int32_t*) {}
#endif

// lane pairs per product of a pass over `hin` values per job, and the passes a job of n pairs needs
static unsigned product_slots(size_t hin) {
  unsigned s = 1;
  while (s < 32 && s < hin) s <<= 1;
  return s;
}
static size_t fq12_rows_words(size_t values) { return (size_t)grid_for(values * kG2Lanes) * kFq12Words * 64; }
// Workspace (words): the Miller values (B * ceil(n / 2)), the values of the right-hand side (B, when there is one), and the
// output of the product passes (the first pass's is the largest; later passes alternate between it and the Miller buffer).
// Every pass writes whole waves: its value count is rounded up to 32.
size_t pairing_product_ws_words(size_t n, size_t B, bool rhs) {
  const size_t H = (n + 1) / 2;
  const size_t first = B * ((H + product_slots(H) - 1) / product_slots(H));
  return fq12_rows_words(B * H) + (rhs ? fq12_rows_words(B) : 0) + fq12_rows_words(first > B ? first : B);
}
// ok[j] = ( prod_{k < n} e(a[(j n + k) sa], b[(j n + k) sb]) == e(c[j sc], d[j sd]) ), or == 1 when c is null.  A stride of 0
// broadcasts one operand.  ws: pairing_product_ws_words(n, B, c != nullptr) words.
void launch_pairing_product_check(hipStream_t st, const uint8_t* a, size_t sa, const uint8_t* b, size_t sb, size_t n, size_t B, const uint8_t* c,
                                  size_t sc, const uint8_t* d, size_t sd, uint8_t* ok, int32_t* ws) {
  if (!B || !n || !ws) return;
  const size_t H = (n + 1) / 2;
  int32_t* cur = ws;
  int32_t* rhs = c ? ws + fq12_rows_words(B * H) : nullptr;
  int32_t* nxt = ws + fq12_rows_words(B * H) + (c ? fq12_rows_words(B) : 0);
  (void)hipMemsetAsync(ok, 1, B, st);
  hipLaunchKernelGGL(k_miller_pairs<false>, dim3(grid_for(B * H * kG2Lanes)), dim3(kBlock), 0, st, a, sa, b, sb, n, B, cur, ok);
  if (c) hipLaunchKernelGGL(k_miller_pairs<true>, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, c, sc, d, sd, (size_t)1, B, rhs, ok);
  // (one value per job and no right-hand side: the Miller stage's output already is what k_final_exp reads)
  for (size_t hin = H, hout = (H > 1 || rhs) ? 0 : 1; hout != 1; hin = hout) {
    const unsigned S = product_slots(hin);
    hout = (hin + S - 1) / S;
    const size_t products = (B * hout + 31) / 32 * 32;  // whole waves of output values
    hipLaunchKernelGGL(k_fq12_product, dim3(grid_for(products * S * kG2Lanes)), dim3(kBlock), 0, st, (const int32_t*)cur, hin, S, hout, B,
                       (const int32_t*)rhs, nxt);
    int32_t* o = cur;
    cur = nxt;
    nxt = o;
  }
  hipLaunchKernelGGL(k_final_exp, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, (const int32_t*)cur, B, ok);
}

}  // namespace tc
