// What the device harnesses of the many-point conformance suite share (manypoint.hip, manypoint_blame.hip; test code only):
// device buffers that remember the first HIP error, and a table arena of the product's geometry.  Included AFTER the product's
// kernel units (TableArena, kTableArenaWords).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

constexpr int kMpSlotLeak = -2;  // a table slot was still marked in use after the run
constexpr int kMpPoison = 0x5A;

namespace {
struct Dev {
  std::vector<void*> owned;
  hipError_t e = hipSuccess;
  void* alloc(size_t bytes, int fill = -1) {
    void* p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) owned.push_back(p);
    if (e == hipSuccess && fill >= 0 && bytes) e = hipMemset(p, fill, bytes);
    return e == hipSuccess ? p : nullptr;
  }
  void* upload(const void* src, size_t bytes) {
    void* p = alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return p;
  }
  void download(void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  }
  void after_launch() {
    if (e == hipSuccess) e = hipGetLastError();
  }
  void sync() {
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  ~Dev() {
    for (void* p : owned) hipFree(p);
  }
};
// a table arena of the product's geometry, every slot free
tc::TableArena arena(Dev& d) {
  tc::TableArena ta;
  ta.mem = (int32_t*)d.alloc(tc::kTableArenaWords * 4, kMpPoison);
  ta.flags = (uint32_t*)d.alloc(tc::kTableArenaFlags * 4, 0);
  return ta;
}
// the entry's return value after a run with an arena: the first HIP error, else kMpSlotLeak when a slot flag is still set
int arena_result(Dev& d, const tc::TableArena& ta) {
  std::vector<uint32_t> fl(tc::kTableArenaFlags);
  d.download(fl.data(), ta.flags, tc::kTableArenaFlags * 4);
  bool leak = false;
  for (size_t i = 0; d.e == hipSuccess && i < fl.size(); i++) leak = leak || fl[i] != 0;
  return d.e == hipSuccess && leak ? kMpSlotLeak : (int)d.e;
}
}  // namespace
