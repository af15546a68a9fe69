// Device probe of the planned quotient form (test code only: never linked into libtc_amd.so, never run by bench.py).
//   k_plan          one wave per denominator: tc_jobs.h combine_quotient_plan of its decomposition, as the wave of the product runs it
//   k_plan_divide   one wave per (denominator, m, width): 32 jobs, [1 / D] of [6] P by tc_jobs.h combine_divide_planned at that
//                   candidate (width 0: the wave's own plan) -- the result's canonical bytes and the lane's exception flag
//   build: tests/test_gpu_combine_plan.py (hipcc with the product's flags, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "tc_jobs.h"

using namespace tc;

constexpr int kBlock = 64, kWaveJobs = kBlock / kG2Lanes;

// out: 4 words per denominator -- decomposed?, m, width, multiply-adds
__global__ __launch_bounds__(kBlock) void k_plan(const uint64_t* __restrict__ ds, int64_t* __restrict__ out) {
  const uint64_t D = wave_uniform(ds[blockIdx.x]);
  uint64_t q = 0;
  int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
  const bool ok = combine_quotient_decompose(D, &q, T, E);
  QuotPlan plan{0, 0, 0};
  if (ok) {
    q = wave_uniform(q);
    TC_UNROLL for (int j = 0; j < 4; j++) {
      T[j] = (int64_t)wave_uniform((uint64_t)T[j]);
      E[j] = (int64_t)wave_uniform((uint64_t)E[j]);
    }
    plan = combine_quotient_plan(q, T, E);
  }
  if (threadIdx.x == 0) {
    int64_t* o = out + (size_t)blockIdx.x * 4;
    o[0] = ok ? 1 : 0;
    o[1] = plan.m;
    o[2] = plan.width;
    o[3] = plan.macs;
  }
}

// cand: 3 words per wave -- D, m, width.  pts: kWaveJobs encoded points, the same for every wave.  out: 192 bytes per job;
// flags: 2 words per job -- the point decoded?, exc
__global__ __launch_bounds__(kBlock, 2) void k_plan_divide(const int64_t* __restrict__ cand, const uint8_t* __restrict__ pts,
                                                                   uint8_t* __restrict__ out, int32_t* __restrict__ flags, TableArena ta) {
  const uint32_t tslot = table_slot_acquire(ta);
  const int local = threadIdx.x / kG2Lanes;
  const size_t job = (size_t)blockIdx.x * kWaveJobs + local;
  const uint64_t D = wave_uniform((uint64_t)cand[(size_t)blockIdx.x * 3]);
  const int m = (int)wave_uniform((uint64_t)cand[(size_t)blockIdx.x * 3 + 1]), width = (int)wave_uniform((uint64_t)cand[(size_t)blockIdx.x * 3 + 2]);
  G2Affine p;
  const bool decoded = PointIO<Fq2>::decode(pts + (size_t)local * 192, p);
  // (a Z that is neither one nor real, as the short ladder leaves it)
  const G2Jac a = jac_dbl(jac_add_mixed(jac_dbl(G2Jac::from_affine(p)), p));
  uint64_t q = 0;
  int64_t T[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
  bool exc = !combine_quotient_decompose(D, &q, T, E);
  q = wave_uniform(q);
  TC_UNROLL for (int j = 0; j < 4; j++) {
    T[j] = (int64_t)wave_uniform((uint64_t)T[j]);
    E[j] = (int64_t)wave_uniform((uint64_t)E[j]);
  }
  const QuotPlan plan = width ? QuotPlan{m, width, 0} : combine_quotient_plan(q, T, E);
  const G2Jac r = combine_divide_planned(a, q, T, E, plan, exc);
  PointIO<Fq2>::encode(jac_to_affine(r), out + job * 192);
  if (pair_leader()) {
    flags[job * 2] = decoded ? 1 : 0;
    flags[job * 2 + 1] = exc ? 1 : 0;
  }
  table_slot_release(ta, tslot);
}

// n denominators -> out (n x 4).  Returns the first HIP error (0 = none).
extern "C" int tc_plan_probe(int n, const uint64_t* ds, int64_t* out) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  uint64_t* dds = nullptr;
  int64_t* dout = nullptr;
  hipError_t e = hipMalloc(&dds, (size_t)n * 8);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * 32);
  if (e == hipSuccess) e = hipMemcpy(dds, ds, (size_t)n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_plan, dim3(n), dim3(kBlock), 0, 0, dds, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 32, hipMemcpyDeviceToHost);
  hipFree(dds);
  hipFree(dout);
  return (int)e;
}

// n waves of (D, m, width) over the kWaveJobs points of pts -> out (n x kWaveJobs x 192 bytes), flags (n x kWaveJobs x 2).  A table
// arena of the product's geometry (tc_arena.h), flags zeroed, as the context allocates it.  Returns the first HIP error.
extern "C" int tc_plan_divide_probe(int n, const int64_t* cand, const uint8_t* pts, uint8_t* out, int32_t* flags) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  const size_t jobs = (size_t)n * kWaveJobs;
  int64_t* dcand = nullptr;
  uint8_t *dpts = nullptr, *dout = nullptr;
  int32_t* dfl = nullptr;
  TableArena ta{nullptr, nullptr};
  hipError_t e = hipMalloc(&dcand, (size_t)n * 24);
  if (e == hipSuccess) e = hipMalloc(&dpts, (size_t)kWaveJobs * 192);
  if (e == hipSuccess) e = hipMalloc(&dout, jobs * 192);
  if (e == hipSuccess) e = hipMalloc(&dfl, jobs * 8);
  if (e == hipSuccess) e = hipMalloc(&ta.mem, kTableArenaWords * 4);
  if (e == hipSuccess) e = hipMalloc(&ta.flags, kTableArenaFlags * 4);
  if (e == hipSuccess) e = hipMemset(ta.flags, 0, kTableArenaFlags * 4);
  if (e == hipSuccess) e = hipMemset(dout, 0, jobs * 192);
  if (e == hipSuccess) e = hipMemset(dfl, 0xff, jobs * 8);
  if (e == hipSuccess) e = hipMemcpy(dcand, cand, (size_t)n * 24, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dpts, pts, (size_t)kWaveJobs * 192, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_plan_divide, dim3(n), dim3(kBlock), 0, 0, dcand, dpts, dout, dfl, ta);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, jobs * 192, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, dfl, jobs * 8, hipMemcpyDeviceToHost);
  if (ta.mem) hipFree(ta.mem);
  if (ta.flags) hipFree(ta.flags);
  hipFree(dcand);
  hipFree(dpts);
  hipFree(dout);
  hipFree(dfl);
  return (int)e;
}
