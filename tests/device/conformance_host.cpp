// Host form of the conformance ops (g++, the host Fq2 of tc_tower.h): the same op bodies and case tables as
// conformance.hip, built with -DTC_BOUND_CHECK so that every case runs under the interval analysis with its declared input
// intervals (tests/device_conformance.py).  A bound violation aborts the process.
//   quad ops (tc_quad.h): the two pairs of a job's quad as two threads that meet at every exchange (tests/hostsim
//     hs_pairing_check_quad); the thread of pair B stands for lanes 2, 3
//   rows (conf_needs_rows ops): kMillerRowSlots Fq2 per job, poisoned before the job, handed back in the device leg's
//     per-job layout (n x kMillerRowSlots x 2 x 14 limbs)
//   tables (conf_needs_table ops): tc_table.h gives the thread a table; it is poisoned before every job
#include "conformance.h"

#include <string.h>
#include <thread>
#include <vector>

using namespace tc;
using namespace tc::conf;

template <int OP>
static void run(int n, const int32_t* in, const float* range, const int32_t* aux, int32_t* out, int32_t* flags,
                int32_t* rows) {
  std::vector<Fq2> mem(conf_needs_rows(OP) ? kMillerRowSlots : 0);
  for (int j = 0; j < n; j++) {
    auto job = [&](int lane) {
      Ctx c{in + (size_t)j * CONF_IN * FQ_LIMBS, aux + (size_t)j * CONF_AUX, out + (size_t)j * CONF_OUT * FQ_LIMBS,
            flags + (size_t)j * CONF_FLAGS, range + (size_t)j * CONF_IN * 3, true, lane, false};
      c.rows = mem.data();
      conf_op<OP>(c);
    };
    if (!mem.empty()) memset((void*)mem.data(), 0x5A, mem.size() * sizeof(Fq2));
    if (conf_needs_table(OP)) {
      memset(pair_table(), 0x5A, kPairTableWords * sizeof(tbl_word));
      memset(lane_table(), 0x5A, kLaneTableWords * sizeof(tbl_word));
    }
    if constexpr (conf_quad(OP)) {
      QuadSim sim;
      auto pair = [&](int hi) {
        tl_quad_sim = &sim;
        tl_quad_hi = hi;
        job(2 * hi);
      };
      std::thread tb(pair, 1);
      pair(0);
      tb.join();
    } else {
      job(0);
    }
    if (rows && !mem.empty())
      for (int k = 0; k < kMillerRowSlots; k++)
        for (int i = 0; i < FQ_LIMBS; i++) {
          int32_t* r = rows + (((size_t)j * kMillerRowSlots + k) * 2) * FQ_LIMBS + i;
          r[0] = mem[k].c0.l[i];
          r[FQ_LIMBS] = mem[k].c1.l[i];
        }
  }
}

extern "C" int tc_conf_host_run(int op, int n, const int32_t* in, const float* range, const int32_t* aux, int32_t* out,
                                int32_t* flags, int32_t* rows) {
  switch (op) {
#define TC_CONF_CASE(name)                            \
  case name:                                          \
    run<name>(n, in, range, aux, out, flags, rows);   \
    return 0;
    TC_CONF_OPS(TC_CONF_CASE)
#undef TC_CONF_CASE
  }
  return -1;
}
