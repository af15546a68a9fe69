// What tests/call/call_host.cpp sees of the fake runtime (fake_runtime.cpp) beyond the HIP functions themselves.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

namespace fake {

// Allocations made while a Quiet lives are the runtime's own (its queues, the closures of deferred work): the counting
// allocator neither counts nor fails them.
struct Quiet {
  Quiet();
  ~Quiet();
};
// deferred work of a stub launcher: runs, in submission order, when its stream is synchronised or waited for
void enqueue(hipStream_t st, std::function<void()> fn);
size_t pending();  // operations still queued on any stream

// The counting allocator (global operator new / delete are replaced): arm() starts counting at 0 and makes allocation number
// fail_at throw std::bad_alloc (-1: none); disarm() stops and returns the count; injected(): the failure was delivered.
void arm(long fail_at);
long disarm();
bool injected();

// watch(): every `window` (>= 2) consecutive bytes of marker[0 .. n) are looked for from now on; device_holds_watched(): one of
// them occurs in a live device block (the table arena, which no stub writes, is left out by its size)
void watch(const uint8_t* marker, size_t n, size_t window);
bool device_holds_watched();

}  // namespace fake
