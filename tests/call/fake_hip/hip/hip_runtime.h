// A stand-in for <hip/hip_runtime.h>: the types and the runtime functions threshold_crypto_amd/csrc/tc_api.hip uses, so that g++
// compiles that unit unchanged for tests/call/call_host.cpp (a test harness -- not a product path).  tests/call/fake_runtime.cpp
// implements them: "device" memory is host memory, and every copy, memset and launch is DEFERRED until somebody synchronises.
#pragma once
#include <stddef.h>
#include <stdint.h>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
struct fakeStream;
struct fakeEvent;
typedef fakeStream* hipStream_t;
typedef fakeEvent* hipEvent_t;
struct hipDeviceProp_t {
  int multiProcessorCount;
};
constexpr unsigned hipStreamNonBlocking = 1;
constexpr unsigned hipEventDisableTiming = 2;

const char* hipGetErrorString(hipError_t e);
hipError_t hipGetLastError();
hipError_t hipGetDeviceCount(int* n);
hipError_t hipSetDevice(int device);
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int device);
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest);
hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b);
hipError_t hipMalloc(void** p, size_t bytes);
hipError_t hipFree(void* p);
hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned flags);
hipError_t hipStreamCreateWithPriority(hipStream_t* st, unsigned flags, int priority);
hipError_t hipStreamDestroy(hipStream_t st);
hipError_t hipStreamSynchronize(hipStream_t st);
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned flags);
hipError_t hipEventCreate(hipEvent_t* ev);
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t ev);
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st);
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b);
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st);
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t st);
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t st);
hipError_t hipMemset2DAsync(void* dst, size_t pitch, int value, size_t width, size_t height, hipStream_t st);
