// Many-point conformance harness of the blame-by-bisection kernels (test code only: never linked into libtc_amd.so, never run by
// bench.py).  Includes the product's kernel unit k_blame.hip as it is (-fno-gpu-rdc: every unit is self-contained), so
// k_blame_seed, k_blame_leaves and k_blame_range_sum and their launchers are the product's own text, compiled with the product's
// flags.  A harness file of its own beside manypoint.hip (two kernel units there already; this one builds in a fraction of the
// time), by the same recipe.  Entries: the leaves (mp_blame_leaves), the range sums over a leaf buffer written by the caller
// (mp_blame_range_sum), leaves and range sums kernel to kernel without the leaves leaving the device in between
// (mp_blame_chain), the leaf ladders blame_leaf_g1 / blame_leaf_g2 at digits given by the caller (mp_blame_ladder: the one
// kernel of this file, k_blame_leaves' frame around the ladder), and blame_sum_parts.  Each allocates, copies in, launches,
// synchronises once, copies out, frees and returns the first HIP error.  Leaves, sums and the rows / bytes behind them are filled
// with 0x5A before the launch.
//   build: tests/manypoint_conformance.py (hipcc, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "../../threshold_crypto_amd/csrc/k_blame.hip"

#include "manypoint_dev.h"  // Dev, arena, arena_result, kMpSlotLeak, kMpPoison

using namespace tc;

namespace {
size_t leaf_words(bool g2) { return g2 ? kBlameLeafWordsG2 : kBlameLeafWordsG1; }
size_t point_bytes(bool g2) { return g2 ? 192 : 96; }

// launch_blame_seed + launch_blame_leaves into a fresh leaf buffer of n rows and a guard row; returns the device buffer
int32_t* run_leaves(Dev& d, const TableArena& ta, bool g2, const uint8_t* key32, uint64_t call, uint64_t leaf0, const uint8_t* pts, size_t n_pts,
                    size_t period, const uint8_t* live_in, size_t n, uint8_t* seed_out, uint8_t* live_out) {
  const uint8_t* dkey = (const uint8_t*)d.upload(key32, 32);
  uint8_t* dseed = (uint8_t*)d.alloc(32, kMpPoison);
  const uint8_t* dpts = (const uint8_t*)d.upload(pts, n_pts * point_bytes(g2));
  uint8_t* dlive = live_in ? (uint8_t*)d.upload(live_in, n + 1) : nullptr;
  int32_t* dleaves = (int32_t*)d.alloc((n + 1) * leaf_words(g2) * 4, kMpPoison);
  int32_t* dsink = (int32_t*)d.alloc(blame_sink_bytes(), kMpPoison);
  if (d.e == hipSuccess) {
    launch_blame_seed(0, dkey, call, dseed);
    launch_blame_leaves(0, ta, g2, dseed, leaf0, dpts, period, dlive, n, dleaves, dsink);
    d.after_launch();
  }
  d.sync();
  d.download(seed_out, dseed, 32);
  if (live_in) d.download(live_out, dlive, n + 1);
  return dleaves;
}
// the range sums over a device leaf buffer: out gets n_items rows and two guard rows.  parts = 0: blame_sum_parts' choice.
void run_sums(Dev& d, bool g2, const int32_t* dleaves, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi, size_t n_items,
              size_t parts, uint8_t* out) {
  const size_t ob = (n_items + 2) * point_bytes(g2);
  const uint32_t* djob = (const uint32_t*)d.upload(job, n_items * 4);
  const uint32_t* dlo = (const uint32_t*)d.upload(lo, n_items * 4);
  const uint32_t* dhi = (const uint32_t*)d.upload(hi, n_items * 4);
  uint8_t* dout = (uint8_t*)d.alloc(ob, kMpPoison);
  if (parts == 0) {
    size_t longest = 0;
    for (size_t i = 0; i < n_items; i++) longest = hi[i] - lo[i] > longest ? hi[i] - lo[i] : longest;
    parts = blame_sum_parts(g2, n_items, longest, 0);
  }
  if (d.e == hipSuccess) {
    launch_blame_range_sum(0, g2, dleaves, N, djob, dlo, dhi, n_items, parts, dout);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, ob);
}
// every item inside its job's N leaves and not empty (an empty range is outside the kernel's contract)
bool items_ok(size_t F, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi, size_t n_items) {
  for (size_t i = 0; i < n_items; i++)
    if (job[i] >= F || lo[i] >= hi[i] || hi[i] > N) return false;
  return true;
}

// leaves[i] = blame_store_leaf([d0 + d1 |x| + d2 |x|^2 + d3 |x|^3] pts[i]) for the digits d = digits[4 i ..], live[i] as the
// ladder's `live`: k_blame_leaves' frame (one lane / lane pair per row, the wave's arena slot held, lanes past the end run row
// 0 into the sink) around blame_leaf_g1 / blame_leaf_g2
template <class F>
__global__ __launch_bounds__(kBlock, 2) void k_mp_blame_ladder(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ live,
                                                               const uint64_t* __restrict__ digits, size_t n, int32_t* __restrict__ leaves,
                                                               int32_t* __restrict__ sink, TableArena ta) {
  constexpr int L = JobLanes<F>::N;
  const uint32_t tslot = table_slot_acquire(ta);
  const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) / L;
  const bool mine = i < n;
  const size_t r = mine ? i : 0;
  uint64_t d[4];
  for (int k = 0; k < 4; k++) d[k] = digits[4 * r + k];
  Affine<F> p = Affine<F>::infinity();
  const bool ok = PointIO<F>::decode(pts + r * PointIO<F>::BYTES, p) && live[r] != 0;
  int32_t* out = mine ? leaves + r * BlameLeaf<F>::WORDS : sink + (size_t)(threadIdx.x / L) * BlameLeaf<F>::WORDS;
  if constexpr (L > 1) blame_store_leaf(out, blame_leaf_g2(p, ok, d));
  else blame_store_leaf(out, blame_leaf_g1(p, ok, d));
  table_slot_release(ta, tslot);
}
}  // namespace

// seed_out (32), leaves (n rows and a guard row), live_out (n bytes and a guard byte; live_in: the same n + 1 bytes, or null: no
// live array, live_out is not written).  pts: n_pts points (period, or n when period = 0).
extern "C" int mp_blame_leaves(int g2, const uint8_t* key32, uint64_t call, uint64_t leaf0, const uint8_t* pts, size_t n_pts, size_t period,
                               const uint8_t* live_in, size_t n, uint8_t* seed_out, int32_t* leaves, uint8_t* live_out) {
  if (!n || n_pts != (period ? period : n)) return (int)hipErrorInvalidValue;
  Dev d;
  TableArena ta = arena(d);
  const int32_t* dleaves = run_leaves(d, ta, g2 != 0, key32, call, leaf0, pts, n_pts, period, live_in, n, seed_out, live_out);
  d.download(leaves, dleaves, (n + 1) * leaf_words(g2 != 0) * 4);
  return arena_result(d, ta);
}

// leaves: F jobs of N leaves in limb form, as the caller wrote them; out: n_items rows and two guard rows
extern "C" int mp_blame_range_sum(int g2, const int32_t* leaves, size_t F, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi,
                                  size_t n_items, size_t parts, uint8_t* out) {
  if (!n_items || !items_ok(F, N, job, lo, hi, n_items)) return (int)hipErrorInvalidValue;
  Dev d;
  const int32_t* dleaves = (const int32_t*)d.upload(leaves, F * N * leaf_words(g2 != 0) * 4);
  run_sums(d, g2 != 0, dleaves, N, job, lo, hi, n_items, parts, out);
  return (int)d.e;
}

// mp_blame_leaves, then the range sums over its leaves (one job of N = n leaves) where k_blame_leaves left them
extern "C" int mp_blame_chain(int g2, const uint8_t* key32, uint64_t call, uint64_t leaf0, const uint8_t* pts, size_t n_pts, size_t period,
                              const uint8_t* live_in, size_t n, const uint32_t* lo, const uint32_t* hi, size_t n_items, size_t parts,
                              uint8_t* seed_out, uint8_t* live_out, uint8_t* out) {
  std::vector<uint32_t> job(n_items, 0);
  if (!n || n_pts != (period ? period : n) || !n_items || !items_ok(1, n, job.data(), lo, hi, n_items)) return (int)hipErrorInvalidValue;
  Dev d;
  TableArena ta = arena(d);
  const int32_t* dleaves = run_leaves(d, ta, g2 != 0, key32, call, leaf0, pts, n_pts, period, live_in, n, seed_out, live_out);
  run_sums(d, g2 != 0, dleaves, n, job.data(), lo, hi, n_items, parts, out);
  return arena_result(d, ta);
}

// pts (n points), live (n), digits (n x 4); leaves: n rows and a guard row
extern "C" int mp_blame_ladder(int g2, const uint8_t* pts, const uint8_t* live, const uint64_t* digits, size_t n, int32_t* leaves) {
  if (!n) return (int)hipErrorInvalidValue;
  Dev d;
  TableArena ta = arena(d);
  const uint8_t* dpts = (const uint8_t*)d.upload(pts, n * point_bytes(g2 != 0));
  const uint8_t* dlive = (const uint8_t*)d.upload(live, n);
  const uint64_t* ddig = (const uint64_t*)d.upload(digits, n * 4 * 8);
  int32_t* dleaves = (int32_t*)d.alloc((n + 1) * leaf_words(g2 != 0) * 4, kMpPoison);
  int32_t* dsink = (int32_t*)d.alloc(blame_sink_bytes(), kMpPoison);
  if (d.e == hipSuccess) {
    if (g2) hipLaunchKernelGGL(k_mp_blame_ladder<Fq2>, dim3(grid_for(n * kG2Lanes)), dim3(kBlock), 0, 0, dpts, dlive, ddig, n, dleaves, dsink, ta);
    else hipLaunchKernelGGL(k_mp_blame_ladder<Fq>, dim3(grid_for(n)), dim3(kBlock), 0, 0, dpts, dlive, ddig, n, dleaves, dsink, ta);
    d.after_launch();
  }
  d.sync();
  d.download(leaves, dleaves, (n + 1) * leaf_words(g2 != 0) * 4);
  return arena_result(d, ta);
}

// blame_sum_parts (a host function of k_blame.hip) and the sizes the kernels' callers allocate by
extern "C" size_t mp_blame_sum_parts(int g2, size_t n_items, size_t longest, int cus) { return blame_sum_parts(g2 != 0, n_items, longest, cus); }
extern "C" size_t mp_blame_leaf_bytes(int g2) { return blame_leaf_bytes(g2 != 0); }
