// Device conformance kernels (test code only: never linked into libtc_amd.so, never run by bench.py).
// One kernel per op of conformance.h, each applying one shipped primitive of threshold_crypto_amd/csrc as the product
// compiles it (gfx950, the product's flags, lane-pair Fq2), in 64-lane workgroups like the product's kernels.
//   build: tests/device_conformance.py (hipcc, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "conformance.h"

#include <vector>

using namespace tc;
using namespace tc::conf;

constexpr int kBlock = 64;

static int conf_grid(int op, int n) { return (n * conf_lanes(op) + kBlock - 1) / kBlock; }

// rows (conf_needs_rows ops): the row block of the workgroup, laid out as k_pairing.hip k_miller_lines lays out its lines
// ta (conf_needs_table ops): the table arena; the wave holds a slot of it while the op runs, as in k_mul.hip
template <int OP>
__global__ __launch_bounds__(kBlock) void k_conf(const int32_t* in, const int32_t* aux, int32_t* out, int32_t* flags,
                                                 int32_t* rows, TableArena ta, int n) {
  constexpr int lanes = conf_lanes(OP);
  uint32_t tslot = 0;
  if constexpr (conf_needs_table(OP)) tslot = table_slot_acquire(ta);
  const int t = blockIdx.x * kBlock + threadIdx.x;
  int job = t / lanes;
  const bool live = job < n;
  if (!live) job = n - 1;  // lanes past the end run a copy of the last job (the pair exchanges and ballots need every lane)
  // (the byte layer's routines store through the output row from every lane: a lane past the end gets the spare row n)
  Ctx c{in + (size_t)job * CONF_IN * FQ_LIMBS, aux + (size_t)job * CONF_AUX, out + (size_t)(live ? job : n) * CONF_OUT * FQ_LIMBS,
        flags + (size_t)job * CONF_FLAGS, nullptr, live, t % lanes, lanes >= 2};
  if (rows) c.rows = rows + (size_t)blockIdx.x * kConfLineWords * 64 + threadIdx.x;
  conf_op<OP>(c);
  if constexpr (conf_needs_table(OP)) table_slot_release(ta, tslot);
}

template <int OP>
static hipError_t launch(const int32_t* in, const int32_t* aux, int32_t* out, int32_t* flags, int32_t* rows, TableArena ta,
                         int n) {
  hipLaunchKernelGGL(k_conf<OP>, dim3(conf_grid(OP, n)), dim3(kBlock), 0, 0, in, aux, out, flags, rows, ta, n);
  return hipGetLastError();
}

static hipError_t dispatch(int op, const int32_t* in, const int32_t* aux, int32_t* out, int32_t* flags, int32_t* rows,
                           TableArena ta, int n) {
  switch (op) {
#define TC_CONF_CASE(name) \
  case name:               \
    return launch<name>(in, aux, out, flags, rows, ta, n);
    TC_CONF_OPS(TC_CONF_CASE)
#undef TC_CONF_CASE
  }
  return hipErrorInvalidValue;
}

// n jobs of op `op` on the current device.  Host buffers in (n x CONF_IN x 14), aux (n x CONF_AUX), out (n x CONF_OUT x 14)
// and flags (n x CONF_FLAGS); out and flags are copied in first, so entries an op does not write keep the caller's value.
// The device's out has one row more than the host's: the spare row that lanes past the end of the batch store into.
// rows (conf_needs_rows ops, else unused): n x kMillerRowSlots x 2 x 14 -- slot k of job j as (re, im) limbs, gathered
// from the device row block (re on the even lane of the pair, im on the odd one), which is filled with a poison pattern
// before the launch so that a row read before it is written gives a wrong result.  conf_needs_table ops get a table arena
// of the product's geometry (tc_arena.h), its flags zeroed and its memory filled with the same pattern; after the run every
// slot flag must be clear again.  Returns the first HIP error (0 = none), or kConfSlotLeak when a slot stayed marked in use.
constexpr int kConfSlotLeak = -2;
extern "C" int tc_conf_run(int op, int n, const int32_t* in, const int32_t* aux, int32_t* out, int32_t* flags, int32_t* rows) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  const size_t sin = (size_t)n * CONF_IN * FQ_LIMBS * 4, saux = (size_t)n * CONF_AUX * 4;
  const size_t srow = (size_t)CONF_OUT * FQ_LIMBS * 4, sout = (size_t)n * srow, sfl = (size_t)n * CONF_FLAGS * 4;
  const size_t nrow = conf_needs_rows(op) ? (size_t)conf_grid(op, n) * kConfLineWords * 64 : 0;
  int32_t *din = nullptr, *daux = nullptr, *dout = nullptr, *dfl = nullptr, *drows = nullptr;
  TableArena ta{nullptr, nullptr};
  const bool table = conf_needs_table(op);
  bool leak = false;
  hipError_t e = hipMalloc(&din, sin);
  if (e == hipSuccess) e = hipMalloc(&daux, saux);
  if (e == hipSuccess) e = hipMalloc(&dout, sout + srow);
  if (e == hipSuccess) e = hipMalloc(&dfl, sfl);
  if (e == hipSuccess && nrow) e = hipMalloc(&drows, nrow * 4);
  if (e == hipSuccess && nrow) e = hipMemset(drows, 0x5A, nrow * 4);
  if (e == hipSuccess && table) e = hipMalloc(&ta.mem, kTableArenaWords * 4);
  if (e == hipSuccess && table) e = hipMalloc(&ta.flags, kTableArenaFlags * 4);
  if (e == hipSuccess && table) e = hipMemset(ta.mem, 0x5A, kTableArenaWords * 4);
  if (e == hipSuccess && table) e = hipMemset(ta.flags, 0, kTableArenaFlags * 4);
  if (e == hipSuccess) e = hipMemcpy(din, in, sin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(daux, aux, saux, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dout, out, sout, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dfl, flags, sfl, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = dispatch(op, din, daux, dout, dfl, drows, ta, n);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, sout, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, dfl, sfl, hipMemcpyDeviceToHost);
  if (e == hipSuccess && nrow && rows) {
    std::vector<int32_t> raw(nrow);
    e = hipMemcpy(raw.data(), drows, nrow * 4, hipMemcpyDeviceToHost);
    for (int j = 0; e == hipSuccess && j < n; j++)
      for (int part = 0; part < 2; part++) {
        const int t = kG2Lanes * j + part;  // the job's lane pair
        const int32_t* col = raw.data() + (size_t)(t / kBlock) * kConfLineWords * 64 + t % kBlock;
        for (int k = 0; k < kMillerRowSlots; k++)
          for (int i = 0; i < FQ_LIMBS; i++)
            rows[(((size_t)j * kMillerRowSlots + k) * 2 + part) * FQ_LIMBS + i] = col[(size_t)(k * FQ_LIMBS + i) * 64];
      }
  }
  if (e == hipSuccess && table) {
    std::vector<uint32_t> fl(kTableArenaFlags);
    e = hipMemcpy(fl.data(), ta.flags, kTableArenaFlags * 4, hipMemcpyDeviceToHost);
    for (size_t i = 0; e == hipSuccess && i < fl.size(); i++) leak = leak || fl[i] != 0;
  }
  if (ta.mem) hipFree(ta.mem);
  if (ta.flags) hipFree(ta.flags);
  hipFree(din);
  hipFree(daux);
  hipFree(dout);
  hipFree(dfl);
  if (drows) hipFree(drows);
  return e == hipSuccess && leak ? kConfSlotLeak : (int)e;
}
