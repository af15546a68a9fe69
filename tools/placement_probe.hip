// Where does the dispatcher put the workgroups of a launch shaped like k_combine_fast<Fq2>'s?  (whether a
// launch ORDER can choose which two waves share a SIMD.)  One wave per workgroup, 256 registers and the product kernel's LDS,
// so that two waves fit a SIMD and eight a CU.  Every wave writes its hardware identity (XCC, SE, CU, SIMD, wave slot), the
// constant-rate clock at its start and at its end, and stays resident for a fixed time by reading that clock; it waits for
// nothing else, so a launch ends after ceil(grid / resident) x hold whatever the placement.
//   build: hipcc --offload-arch=gfx950 -O3 tools/placement_probe.hip -o tools/placement_probe
//   run:   tools/placement_probe [hold_us] [repeats] [grid ...]      (tools/placement_probe.py runs and reads it)
// One line per workgroup: grid repeat block xcc se cu simd slot start end   (clock ticks of 10 ns from the launch's first start)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

constexpr int kProbeLds = 6672;  // profiles/kernel_resources.json: k_combine_fast<Fq2>

struct Rec {
  uint32_t block, hw_id, xcc, pad;
  uint64_t start, end;
};

__global__ __launch_bounds__(64, 2) void k_probe(Rec* out, uint64_t hold_ticks, uint32_t seed) {
  __shared__ uint32_t lds[kProbeLds / 4];
  const uint64_t t0 = wall_clock64();  // 100 MHz, one counter for the whole device
  asm volatile("v_mov_b32 v255, 0" ::: "v255");  // 256 registers: two waves per SIMD, as the product kernel
  lds[threadIdx.x] = seed + threadIdx.x;
  const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));   // HW_REG_HW_ID, all 32 bits
  const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));  // HW_REG_XCC_ID [3:0]
  uint64_t t1 = t0;
  uint32_t spin = 0;
  // (the clock always advances: the loop ends after hold_ticks; the trip bound is a second, independent end)
  while (t1 - t0 < hold_ticks && spin < (1u << 24)) {
    __builtin_amdgcn_s_sleep(8);
    t1 = wall_clock64();
    spin++;
  }
  if (threadIdx.x == 0) {
    Rec r;
    r.block = blockIdx.x;
    r.hw_id = hw;
    r.xcc = xcc;
    r.pad = lds[(spin + seed) & 63];  // (keeps the LDS allocation alive)
    r.start = t0;
    r.end = t1;
    out[blockIdx.x] = r;
  }
}

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                      \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(int argc, char** argv) {
  const double hold_us = argc > 1 ? atof(argv[1]) : 200.0;
  const int repeats = argc > 2 ? atoi(argv[2]) : 3;
  std::vector<int> grids;
  for (int i = 3; i < argc; i++) grids.push_back(atoi(argv[i]));
  if (grids.empty()) grids = {2296, 2048, 4592};
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    fprintf(stderr, "no HIP device\n");
    return 1;
  }
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  int per_cu = 0;
  CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_probe, 64, 0));
  printf("# device %s cus %d workgroups_per_cu %d resident %d hold_us %.1f\n", p.gcnArchName, p.multiProcessorCount, per_cu,
         per_cu * p.multiProcessorCount, hold_us);
  int max_grid = 0;
  for (int g : grids) {
    if (g < 1 || g > (1 << 16)) {
      fprintf(stderr, "grid %d out of range\n", g);
      return 1;
    }
    if (g > max_grid) max_grid = g;
  }
  Rec* d = nullptr;
  CHECK(hipMalloc(&d, sizeof(Rec) * (size_t)max_grid));
  std::vector<Rec> h((size_t)max_grid);
  const uint64_t hold_ticks = (uint64_t)(hold_us * 100.0);
  for (int g : grids)
    for (int r = 0; r < repeats; r++) {
      CHECK(hipMemset(d, 0, sizeof(Rec) * (size_t)max_grid));
      hipLaunchKernelGGL(k_probe, dim3(g), dim3(64), 0, 0, d, hold_ticks, 17u * r + g);
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(h.data(), d, sizeof(Rec) * (size_t)g, hipMemcpyDeviceToHost));
      uint64_t first = ~0ull;
      for (int b = 0; b < g; b++)
        if (h[b].start < first) first = h[b].start;
      for (int b = 0; b < g; b++) {
        const uint32_t hw = h[b].hw_id;
        // HW_ID: WAVE_ID [3:0], SIMD_ID [5:4], CU_ID [11:8], SH_ID [12], SE_ID [15:13]
        printf("%d %d %u %u %u %u %u %u %llu %llu\n", g, r, h[b].block, h[b].xcc & 15u, (hw >> 13) & 7u, ((hw >> 12) & 1u) * 16u + ((hw >> 8) & 15u),
               (hw >> 4) & 3u, hw & 15u, (unsigned long long)(h[b].start - first), (unsigned long long)(h[b].end - first));
      }
    }
  CHECK(hipFree(d));
  return 0;
}
