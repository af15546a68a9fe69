// A HIP runtime for the host: "device" memory is malloc'ed, and NOTHING asynchronous runs when it is submitted.  Every
// hipMemcpyAsync, hipMemsetAsync, their 2D forms and every stub launcher (call_host.cpp) is queued on its stream and runs, in
// submission order, only at hipStreamSynchronize -- or when another stream that waits on an event behind it is synchronised.  A
// real runtime may do exactly that, so host memory that a caller frees before it synchronises is read or written after the free:
// under AddressSanitizer, a report.  That is the point of this file.  (hipFree drains everything first, as the real one does.)
// Also here: the counting allocator the harness fails allocations with.
#include "fake_runtime.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <map>
#include <new>
#include <set>
#include <string>
#include <vector>

namespace {

thread_local int g_quiet = 0;
bool g_armed = false, g_injected = false;
long g_count = 0, g_fail_at = -1;

void* counted_alloc(size_t n) {
  if (g_armed && g_quiet == 0 && g_count++ == g_fail_at) {
    g_injected = true;
    throw std::bad_alloc();
  }
  void* p = malloc(n ? n : 1);
  if (!p) throw std::bad_alloc();
  return p;
}

struct Op {
  uint64_t seq;
  std::function<void()> fn;        // empty: a marker (event record)
  fakeStream* wait_st = nullptr;   // a wait: everything of wait_st up to wait_seq runs first
  uint64_t wait_seq = 0;
};

}  // namespace

void* operator new(size_t n) { return counted_alloc(n); }
void* operator new[](size_t n) { return counted_alloc(n); }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }

struct fakeStream {
  std::deque<Op> q;
};
struct fakeEvent {
  fakeStream* st = nullptr;  // where it was last recorded
  uint64_t seq = 0;
};

namespace {

uint64_t g_seq = 0;
std::vector<fakeStream*> g_streams;
std::map<void*, size_t> g_blocks;
fakeStream g_null_stream;
std::set<std::string> g_windows;  // fake::watch
std::vector<bool> g_first2(65536, false);
size_t g_window = 0;

fakeStream* stream_of(hipStream_t st) { return st ? st : &g_null_stream; }

void run_until(fakeStream* s, uint64_t limit) {
  while (!s->q.empty() && s->q.front().seq <= limit) {
    Op op = std::move(s->q.front());
    s->q.pop_front();
    if (op.wait_st) run_until(op.wait_st, op.wait_seq);
    if (op.fn) op.fn();
  }
}
void drain_all() {
  run_until(&g_null_stream, g_seq);
  for (fakeStream* s : g_streams) run_until(s, g_seq);
}
void push(hipStream_t st, std::function<void()> fn) {
  Op op;
  op.seq = ++g_seq;
  op.fn = std::move(fn);
  stream_of(st)->q.push_back(std::move(op));
}

}  // namespace

namespace fake {

Quiet::Quiet() { g_quiet++; }
Quiet::~Quiet() { g_quiet--; }
void enqueue(hipStream_t st, std::function<void()> fn) {
  Quiet q;
  push(st, std::move(fn));
}
size_t pending() {
  size_t n = g_null_stream.q.size();
  for (fakeStream* s : g_streams) n += s->q.size();
  return n;
}
void arm(long fail_at) {
  g_count = 0;
  g_fail_at = fail_at;
  g_injected = false;
  g_armed = true;
}
long disarm() {
  g_armed = false;
  return g_count;
}
bool injected() { return g_injected; }
void watch(const uint8_t* marker, size_t n, size_t window) {
  Quiet q;
  for (size_t w = 0; w + window <= n; w++) {
    g_windows.insert(std::string((const char*)marker + w, window));
    g_first2[marker[w] | (marker[w + 1] << 8)] = true;
  }
  g_window = window;
}
bool device_holds_watched() {
  Quiet q;
  for (auto& b : g_blocks) {
    if (b.second > ((size_t)64 << 20) || b.second < g_window) continue;
    const uint8_t* p = (const uint8_t*)b.first;
    for (size_t i = 0; i + g_window <= b.second; i++)
      if (g_first2[p[i] | (p[i + 1] << 8)] && g_windows.count(std::string((const char*)p + i, g_window))) return true;
  }
  return false;
}

}  // namespace fake

using fake::Quiet;

const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake runtime error"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
  prop->multiProcessorCount = 256;
  return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) {
  *least = 0;
  *greatest = -1;
  return hipSuccess;
}
hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) {
  *free_b = *total_b = (size_t)64 << 30;
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  Quiet q;
  *p = calloc(bytes ? bytes : 1, 1);
  if (!*p) return hipErrorOutOfMemory;
  g_blocks[*p] = bytes;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  Quiet q;
  drain_all();
  if (p && g_blocks.erase(p)) free(p);
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned) {
  Quiet q;
  *st = new fakeStream();
  g_streams.push_back(*st);
  return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* st, unsigned flags, int) { return hipStreamCreateWithFlags(st, flags); }
hipError_t hipStreamDestroy(hipStream_t st) {
  Quiet q;
  run_until(st, g_seq);
  for (size_t i = 0; i < g_streams.size(); i++)
    if (g_streams[i] == st) g_streams.erase(g_streams.begin() + i);
  delete st;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st) {
  Quiet q;
  run_until(stream_of(st), g_seq);
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned) {
  Quiet q;
  if (!ev->st) return hipSuccess;  // never recorded: nothing to wait for
  Op op;
  op.seq = ++g_seq;
  op.wait_st = ev->st;
  op.wait_seq = ev->seq;
  stream_of(st)->q.push_back(std::move(op));
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* ev) {
  Quiet q;
  *ev = new fakeEvent();
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) { return hipEventCreate(ev); }
hipError_t hipEventDestroy(hipEvent_t ev) {
  Quiet q;
  delete ev;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
  Quiet q;
  push(st, nullptr);
  ev->st = stream_of(st);
  ev->seq = g_seq;
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 0.f;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t st) {
  Quiet q;
  push(st, [=] { memmove(dst, src, bytes); });
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t st) {
  Quiet q;
  push(st, [=] {
    for (size_t r = 0; r < height; r++) memmove((uint8_t*)dst + r * dpitch, (const uint8_t*)src + r * spitch, width);
  });
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t st) {
  Quiet q;
  push(st, [=] { memset(dst, value, bytes); });
  return hipSuccess;
}
hipError_t hipMemset2DAsync(void* dst, size_t pitch, int value, size_t width, size_t height, hipStream_t st) {
  Quiet q;
  push(st, [=] {
    for (size_t r = 0; r < height; r++) memset((uint8_t*)dst + r * pitch, value, width);
  });
  return hipSuccess;
}
