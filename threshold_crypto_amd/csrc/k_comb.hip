// gfx950 kernels: the shares of a message by many signers through a per-message comb (tc_comb.h), and the decryption shares of
// a ciphertext by many key holders through a per-ciphertext comb in G1 (tc_comb_g1.h).
#include "tc_comb.h"
#include "tc_comb_g1.h"
#include "tc_launch.h"

namespace tc {

// stage T: one lane pair per message; ok[j] = the hash point decoded
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_comb_tables(const uint8_t* __restrict__ pts, size_t B, int32_t* __restrict__ tbl,
                                                                   uint8_t* __restrict__ ok) {
  const size_t j = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  if (j >= B) return;
  const bool good = job_comb_tables(pts + j * 192, (tbl_word*)(tbl + j * (size_t)kCombTableWords));
  if (pair_leader()) ok[j] = good ? 1 : 0;
}

// stage S: a lane pair takes one message and up to kCombShare of its n signers (chunk-major lane order)
__global__ __launch_bounds__(kBlock, TC_WAVES_G2) void k_comb_sign(const uint8_t* __restrict__ sk, size_t N, const uint64_t* __restrict__ idx,
                                                                 const int32_t* __restrict__ tbl, const uint8_t* __restrict__ ok, size_t n,
                                                                 size_t B, uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                                 TableArena ta, size_t share) {
  const uint32_t tslot = table_slot_acquire(ta);  // (the guarded fallback ladder reads column 0 in place: no table is built here)
  const size_t tid = ((size_t)blockIdx.x * kBlock + threadIdx.x) / kG2Lanes;
  const size_t chunks = (n + share - 1) / share;  // share <= kCombShare signers per lane pair (launch_comb_sign)
  if (tid < chunks * B) {
    const size_t c = tid / B, j = tid % B;
    const size_t s0 = c * share;
    const int cnt = (int)((n - s0 < share) ? n - s0 : share);
    const size_t o = j * n + s0;
    job_comb_sign(sk, N, idx + o, cnt, (const tbl_word*)(tbl + j * (size_t)kCombTableWords), ok[j] != 0, out + o * 192,
                  status ? status + o : nullptr, pair_leader());
  }
  table_slot_release(ta, tslot);
}

size_t comb_table_bytes(size_t B) { return B * (size_t)kCombTableWords * sizeof(int32_t); }
void launch_comb_sign(hipStream_t st, TableArena ta, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B,
                      int32_t* tbl, uint8_t* ok, uint8_t* out, uint8_t* status) {
  if (!(n * B) || !ta.mem || !ta.flags) return;
  hipLaunchKernelGGL(k_comb_tables, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, st, pts, B, tbl, ok);
  const size_t share = signers_per_lane_pair(n, B, kCombShare);
  const size_t chunks = (n + share - 1) / share;
  hipLaunchKernelGGL(k_comb_sign, dim3(grid_for(chunks * B * kG2Lanes)), dim3(kBlock), 0, st, sk, N, idx, (const int32_t*)tbl, (const uint8_t*)ok, n, B,
                     out, status, ta, share);
}

// ---- G1: decryption shares (tc_comb_g1.h) ---------------------------------------------------------------------------------
// stage T: one lane per ciphertext; ok[j] = u decoded
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_comb_tables_g1(const uint8_t* __restrict__ pts, size_t B, int32_t* __restrict__ tbl,
                                                                          uint8_t* __restrict__ ok) {
  const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= B) return;
  ok[j] = job_comb_tables_g1(pts + j * 96, tbl + j * (size_t)kCombG1TableWords) ? 1 : 0;
}

// stage S: a lane takes one ciphertext and up to kCombG1Share of its n holders (chunk-major lane order).  A lane past the end
// takes none of ciphertext 0's: the holder loop is the wave's (tc_comb_g1.h job_comb_decrypt).
__global__ __launch_bounds__(kBlock, TC_WAVES_G1_AUX) void k_comb_decrypt(const uint8_t* __restrict__ sk, size_t N, const uint64_t* __restrict__ idx,
                                                                        const int32_t* __restrict__ tbl, const uint8_t* __restrict__ ok, size_t n,
                                                                        size_t B, uint8_t* __restrict__ out, uint8_t* __restrict__ status,
                                                                        size_t share) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t chunks = (n + share - 1) / share;  // share <= kCombG1Share holders per lane (launch_comb_decrypt)
  const bool live = tid < chunks * B;
  const size_t c = live ? tid / B : 0, j = live ? tid % B : 0;
  const size_t s0 = c * share;
  const int cnt = live ? (int)((n - s0 < share) ? n - s0 : share) : 0;
  const size_t o = j * n + s0;
  job_comb_decrypt(sk, N, idx + o, cnt, tbl + j * (size_t)kCombG1TableWords, ok[j] != 0, out + o * 96, status ? status + o : nullptr);
}

// one ladder per (ciphertext, selected holder), holder-major lane order (tid = k * B + j); the ladder's table in the wave's arena slot
__global__ __launch_bounds__(kBlock, 2) void k_g1_mul_gather(const uint8_t* __restrict__ sk, size_t N, const uint64_t* __restrict__ idx,
                                                           const uint8_t* __restrict__ pts, size_t n, size_t B, uint8_t* __restrict__ out,
                                                           uint8_t* __restrict__ status, TableArena ta) {
  const uint32_t tslot = table_slot_acquire(ta);
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = tid < n * B;
  const size_t k = live ? tid / B : 0, j = live ? tid % B : 0;
  const size_t o = j * n + k;
  // (a lane past the end multiplies job 0 again and drops the result: the ladder's loads and stores are the whole wave's)
  uint8_t sink[96];
  const uint8_t st = job_g1_mul_gather(sk, N, idx[o], pts + j * 96, live ? out + o * 96 : sink);
  if (live && status) status[o] = st;
  table_slot_release(ta, tslot);
}

size_t comb_table_bytes_g1(size_t B) { return B * (size_t)kCombG1TableWords * sizeof(int32_t); }
void launch_comb_decrypt(hipStream_t st, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, int32_t* tbl,
                         uint8_t* ok, uint8_t* out, uint8_t* status) {
  if (!(n * B)) return;
  hipLaunchKernelGGL(k_comb_tables_g1, dim3(grid_for(B)), dim3(kBlock), 0, st, pts, B, tbl, ok);
  const size_t share = holders_per_lane(n, B, kCombG1Share);
  const size_t chunks = (n + share - 1) / share;
  hipLaunchKernelGGL(k_comb_decrypt, dim3(grid_for(chunks * B)), dim3(kBlock), 0, st, sk, N, idx, (const int32_t*)tbl, (const uint8_t*)ok, n, B, out,
                     status, share);
}
void launch_g1_mul_gather(hipStream_t st, TableArena ta, const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B,
                          uint8_t* out, uint8_t* status) {
  if (!(n * B) || !ta.mem || !ta.flags) return;
  hipLaunchKernelGGL(k_g1_mul_gather, dim3(grid_for(n * B)), dim3(kBlock), 0, st, sk, N, idx, pts, n, B, out, status, ta);
}

}  // namespace tc
