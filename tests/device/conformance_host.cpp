// Host form of the conformance ops (g++, the host Fq2 of tc_tower.h): the same op bodies and case tables as
// conformance.hip, built with -DTC_BOUND_CHECK so that every case runs under the interval analysis with its declared input
// intervals (tests/device_conformance.py).  A bound violation aborts the process.
#include "conformance.h"

using namespace tc;
using namespace tc::conf;

template <int OP>
static void run(int n, const int32_t* in, const float* range, const int32_t* aux, int32_t* out, int32_t* flags) {
  for (int j = 0; j < n; j++) {
    Ctx c{in + (size_t)j * CONF_IN * FQ_LIMBS, aux + (size_t)j * CONF_AUX, out + (size_t)j * CONF_OUT * FQ_LIMBS,
          flags + (size_t)j * CONF_FLAGS, range + (size_t)j * CONF_IN * 3, true, 0, false};
    conf_op<OP>(c);
  }
}

extern "C" int tc_conf_host_run(int op, int n, const int32_t* in, const float* range, const int32_t* aux, int32_t* out,
                                int32_t* flags) {
  switch (op) {
#define TC_CONF_CASE(name)                      \
  case name:                                    \
    run<name>(n, in, range, aux, out, flags);   \
    return 0;
    TC_CONF_OPS(TC_CONF_CASE)
#undef TC_CONF_CASE
  }
  return -1;
}
