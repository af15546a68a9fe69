// gfx950 kernels: blame by bisection for pass 2 of the robust combiners (tc_blame_jobs.h; the search is tc_blame.h, driven by
// the host in tc_api.hip).
#include "tc_blame_jobs.h"
#include "tc_launch.h"

namespace tc {

// seed_out (32 B) = the pass-2 seed of call number `call` under the context's key (32 B)
__global__ void k_blame_seed(const uint8_t* __restrict__ key32, uint64_t call, uint8_t* __restrict__ seed_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t key[8], seed[8];
  for (int w = 0; w < 8; w++)
    key[w] = (uint32_t)key32[4 * w] | ((uint32_t)key32[4 * w + 1] << 8) | ((uint32_t)key32[4 * w + 2] << 16) | ((uint32_t)key32[4 * w + 3] << 24);
  blame_call_seed(key, call, seed);
  for (int w = 0; w < 8; w++)
    for (int b = 0; b < 4; b++) seed_out[4 * w + b] = (uint8_t)(seed[w] >> (8 * b));
}

// leaves[i] = [r_(leaf0 + i)] pts[i % period] (period 0: pts[i]) for i < n: one lane (G1) / one lane pair (G2) per leaf, the
// ladder's table in the wave's arena slot.  live: n bytes, or null (every point counts); a point that does not decode clears
// its byte.  Lanes past the end run leaf 0 again into a sink of their own: the table traffic is the whole wave's.
template <class F>
__global__ __launch_bounds__(kBlock, 2) void k_blame_leaves(const uint8_t* __restrict__ seed32, uint64_t leaf0, const uint8_t* __restrict__ pts,
                                                            size_t period, uint8_t* __restrict__ live, size_t n, int32_t* __restrict__ leaves,
                                                            int32_t* __restrict__ sink, TableArena ta) {
  constexpr int L = JobLanes<F>::N;
  constexpr int PB = PointIO<F>::BYTES;
  const uint32_t tslot = table_slot_acquire(ta);
  const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) / L;
  const bool mine = i < n;
  const size_t r = mine ? i : 0;
  uint32_t key[8];
  for (int w = 0; w < 8; w++)
    key[w] = (uint32_t)seed32[4 * w] | ((uint32_t)seed32[4 * w + 1] << 8) | ((uint32_t)seed32[4 * w + 2] << 16) | ((uint32_t)seed32[4 * w + 3] << 24);
  const bool leader = L == 1 || pair_leader();
  // (a lane past the end never writes a live byte: leader = false for it)
  job_blame_leaf<F>(key, leaf0 + r, pts + (period ? r % period : r) * PB, live ? live + r : nullptr, leader && mine,
                    mine ? leaves + r * BlameLeaf<F>::WORDS : sink + (size_t)(threadIdx.x / L) * BlameLeaf<F>::WORDS);
  table_slot_release(ta, tslot);
}

// out[it] = the affine encoding of sum_{lo[it] <= k < hi[it]} leaves[job[it] * N + k]: `parts` (a power of two; at most 64 lanes
// for G1, 32 lane pairs for G2) adjacent lanes (pairs) per item, so an item never spans two waves; their partial sums meet in
// log2(parts) rounds of one __shfl_xor exchange of the limbs + one complete addition (k_g1_sum, k_msm_ladder_split), the first
// one inverts once and writes.  No lane of a live item leaves before the last round; the lanes of items >= n_items leave as
// whole groups.  A range may be longer than a wave and start anywhere: a lane takes sum_part's share of it.
template <class F>
__global__ __launch_bounds__(kBlock, 2) void k_blame_range_sum(const int32_t* __restrict__ leaves, size_t N, const uint32_t* __restrict__ job,
                                                               const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, size_t n_items,
                                                               size_t parts, uint8_t* __restrict__ out) {
  constexpr int L = JobLanes<F>::N;
  const size_t lp = ((size_t)blockIdx.x * kBlock + threadIdx.x) / L;
  const size_t it = lp / parts, g = lp % parts;
  if (it >= n_items) return;
  Jac<F> r = job_blame_range_part<F>(leaves + (size_t)job[it] * N * BlameLeaf<F>::WORDS, lo[it], hi[it], g, parts);
  TC_NOUNROLL for (size_t d = 1; d < parts; d <<= 1) {
    const int lanes = (int)(d * L);
    Jac<F> o = r;
    if constexpr (L > 1) {
      TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) {
        o.x.m.l[i] = __shfl_xor(r.x.m.l[i], lanes, 64);
        o.y.m.l[i] = __shfl_xor(r.y.m.l[i], lanes, 64);
        o.z.m.l[i] = __shfl_xor(r.z.m.l[i], lanes, 64);
      }
    } else {
      TC_UNROLL for (int i = 0; i < FQ_LIMBS; i++) {
        o.x.l[i] = __shfl_xor(r.x.l[i], lanes, 64);
        o.y.l[i] = __shfl_xor(r.y.l[i], lanes, 64);
        o.z.l[i] = __shfl_xor(r.z.l[i], lanes, 64);
      }
    }
    r = jac_add(r, o);
  }
  if (g == 0) PointIO<F>::encode(jac_to_affine(r), out + it * PointIO<F>::BYTES);
}

size_t blame_leaf_bytes(bool g2) { return (size_t)(g2 ? kBlameLeafWordsG2 : kBlameLeafWordsG1) * sizeof(int32_t); }
size_t blame_sink_bytes() { return (size_t)kBlock * kBlameLeafWordsG2 * sizeof(int32_t); }

void launch_blame_seed(hipStream_t st, const uint8_t* key32, uint64_t call, uint8_t* seed_out) {
  hipLaunchKernelGGL(k_blame_seed, dim3(1), dim3(kBlock), 0, st, key32, call, seed_out);
}
void launch_blame_leaves(hipStream_t st, TableArena ta, bool g2, const uint8_t* seed32, uint64_t leaf0, const uint8_t* pts, size_t period, uint8_t* live,
                         size_t n, int32_t* leaves, int32_t* sink) {
  if (!n || !ta.mem || !ta.flags) return;
  if (g2)
    hipLaunchKernelGGL(k_blame_leaves<Fq2>, dim3(grid_for(n * kG2Lanes)), dim3(kBlock), 0, st, seed32, leaf0, pts, period, live, n, leaves, sink, ta);
  else
    hipLaunchKernelGGL(k_blame_leaves<Fq>, dim3(grid_for(n)), dim3(kBlock), 0, st, seed32, leaf0, pts, period, live, n, leaves, sink, ta);
}
// lanes (G2: lane pairs) per item: the smallest power of two that gives the launch one wave per SIMD, at most half the
// longest range of the round and at most a wave
size_t blame_sum_parts(bool g2, size_t n_items, size_t longest, int cus) {
  const size_t want = (size_t)(cus > 0 ? cus : 256) * 4 * kBlock / (g2 ? kG2Lanes : 1);
  const size_t most = (size_t)kBlock / (g2 ? kG2Lanes : 1);
  size_t parts = 1;
  while (parts < most && n_items * parts < want && parts * 2 * 2 <= longest) parts *= 2;
  return parts;
}
void launch_blame_range_sum(hipStream_t st, bool g2, const int32_t* leaves, size_t N, const uint32_t* job, const uint32_t* lo, const uint32_t* hi,
                            size_t n_items, size_t parts, uint8_t* out) {
  if (!n_items) return;
  const size_t most = (size_t)kBlock / (g2 ? kG2Lanes : 1);
  if (parts < 1 || parts > most || (parts & (parts - 1))) parts = 1;
  if (g2)
    hipLaunchKernelGGL(k_blame_range_sum<Fq2>, dim3(grid_for(n_items * parts * kG2Lanes)), dim3(kBlock), 0, st, leaves, N, job, lo, hi, n_items, parts, out);
  else
    hipLaunchKernelGGL(k_blame_range_sum<Fq>, dim3(grid_for(n_items * parts)), dim3(kBlock), 0, st, leaves, N, job, lo, hi, n_items, parts, out);
}

}  // namespace tc
