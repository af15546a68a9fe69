// Single-point kernel conformance harness, part 1 (test code only: never linked into libtc_amd.so, never run by bench.py).
// Includes the product's kernel units k_check.hip and k_robust.hip as they are (every unit of the product is self-contained:
// -fno-gpu-rdc), so the __global__ kernels launched here are the product's own text, compiled with the product's flags.  Every
// entry allocates, fills each written buffer with 0x5A (or copies in what the kernel reads AND writes, guard included), copies
// in, launches THROUGH THE PRODUCT'S LAUNCHER, synchronises once, copies out, frees and returns the first HIP error.  Every
// written buffer carries one guard row / byte / entry behind it.  Where the launcher derives a geometry (the 16-byte or 8-byte
// form of k_gather_selected) the entry takes it by value: 0 goes through the launcher, another value launches the kernel
// directly.  The other half (k_mul.hip, k_hash.hip): single_kernels_mul.hip; the host leg: single_kernels_host.cpp.
//   build: tests/single_conformance.py (hipcc, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "../../threshold_crypto_amd/csrc/k_check.hip"
#include "../../threshold_crypto_amd/csrc/k_robust.hip"

#include "manypoint_dev.h"  // Dev, kMpPoison

using namespace tc;

namespace {
const uint8_t* up(Dev& d, const void* p, size_t bytes) { return p ? (const uint8_t*)d.upload(p, bytes) : nullptr; }
uint8_t* io(Dev& d, const void* p, size_t bytes) { return p ? (uint8_t*)d.upload(p, bytes) : nullptr; }
uint8_t* fresh(Dev& d, size_t bytes) { return (uint8_t*)d.alloc(bytes, kMpPoison); }
// `bytes` of p at `off` (0 .. 15) bytes behind a 16-byte boundary of an allocation of its own
uint8_t* up_at(Dev& d, const void* p, size_t bytes, size_t off) {
  if (!p) return nullptr;
  uint8_t* base = (uint8_t*)d.alloc(bytes + 16, kMpPoison);
  if (d.e == hipSuccess && bytes) d.e = hipMemcpy(base + off, p, bytes, hipMemcpyHostToDevice);
  return d.e == hipSuccess ? base + off : nullptr;
}
}  // namespace

// g1 = 0: k_rlc_scalars, 1: k_rlc_scalars_g1.  out: (n + 1) x 32
extern "C" int sk_rlc_scalars(int g1, const uint8_t* seed32, size_t n, uint8_t* out) {
  Dev d;
  const uint8_t* ds = up(d, seed32, 32);
  uint8_t* dout = fresh(d, (n + 1) * 32);
  if (d.e == hipSuccess) {
    if (g1) launch_rlc_scalars_g1(0, ds, n, dout);
    else launch_rlc_scalars(0, ds, n, dout);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (n + 1) * 32);
  return (int)d.e;
}

// pts: pts_bytes >= ((n - 1) / take * n_per_job + take) * stride bytes; valid: n + 1
extern "C" int sk_subgroup_check(int g2, const uint8_t* pts, size_t pts_bytes, size_t stride, size_t n_per_job, size_t take, size_t n,
                                 uint8_t* valid) {
  if (!n || !take || take > n_per_job || stride < (g2 ? 192u : 96u) || pts_bytes < ((n - 1) / take * n_per_job + (n - 1) % take + 1) * stride)
    return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dp = up(d, pts, pts_bytes);
  uint8_t* dv = fresh(d, n + 1);
  if (d.e == hipSuccess) {
    if (g2) launch_subgroup_check_g2(0, dp, stride, n_per_job, take, n, dv);
    else launch_subgroup_check_g1(0, dp, stride, n_per_job, take, n, dv);
    d.after_launch();
  }
  d.sync();
  d.download(valid, dv, n + 1);
  return (int)d.e;
}

// valid: valid_len bytes (checked against what `group` makes the kernel read); status, ok: B + 1 bytes in and out, or null;
// out: (B + 1) x out_bytes in and out, or null
extern "C" int sk_invalidate_jobs(const uint8_t* valid, size_t valid_len, size_t per_job, size_t group, size_t B, uint8_t* status, uint8_t* out,
                                  size_t out_bytes, uint8_t* ok) {
  const size_t g = group ? group : 1;
  if (!B || valid_len < ((B - 1) / g + 1) * per_job) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dv = up(d, valid, valid_len);
  uint8_t* dst = io(d, status, B + 1);
  uint8_t* dok = io(d, ok, B + 1);
  uint8_t* dout = io(d, out, (B + 1) * out_bytes);
  if (d.e == hipSuccess) {
    launch_invalidate_jobs(0, dv, per_job, group, B, dst, dout, out_bytes, dok);
    d.after_launch();
  }
  d.sync();
  if (status) d.download(status, dst, B + 1);
  if (ok) d.download(ok, dok, B + 1);
  if (out) d.download(out, dout, (B + 1) * out_bytes);
  return (int)d.e;
}

// ok: B + 1 bytes in and out
extern "C" int sk_ok_and_status(const uint8_t* status, size_t B, uint8_t* ok) {
  Dev d;
  const uint8_t* dst = up(d, status, B);
  uint8_t* dok = io(d, ok, B + 1);
  if (d.e == hipSuccess) {
    launch_ok_and_status(0, dst, B, dok);
    d.after_launch();
  }
  d.sync();
  d.download(ok, dok, B + 1);
  return (int)d.e;
}

// src: src_rows x row_bytes; map: `rows` entries below src_rows; dst: (rows + 1) x row_bytes
extern "C" int sk_gather_rows(const uint8_t* src, size_t src_rows, size_t row_bytes, const uint32_t* map, size_t rows, uint8_t* dst) {
  if (row_bytes % 8) return (int)hipErrorInvalidValue;
  for (size_t r = 0; r < rows; r++)
    if (map[r] >= src_rows) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* ds = up(d, src, src_rows * row_bytes);
  const uint32_t* dm = (const uint32_t*)up(d, map, rows * 4);
  uint8_t* dd = fresh(d, (rows + 1) * row_bytes);
  if (d.e == hipSuccess) {
    launch_gather_rows(0, ds, row_bytes, dm, rows, dd);
    d.after_launch();
  }
  d.sync();
  d.download(dst, dd, (rows + 1) * row_bytes);
  return (int)d.e;
}

// scatter = 1: k_scatter_bytes, dst[map[r]] = src[r] (src: rows, dst: other + 1 bytes); 0: k_gather_bytes, dst[r] = src[map[r]]
// (src: other, dst: rows + 1 bytes).  map: `rows` entries below `other`.
extern "C" int sk_move_bytes(int scatter, const uint8_t* src, const uint32_t* map, size_t rows, size_t other, uint8_t* dst) {
  for (size_t r = 0; r < rows; r++)
    if (map[r] >= other) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t out_len = (scatter ? other : rows) + 1;
  const uint8_t* ds = up(d, src, scatter ? rows : other);
  const uint32_t* dm = (const uint32_t*)up(d, map, rows * 4);
  uint8_t* dd = fresh(d, out_len);
  if (d.e == hipSuccess) {
    if (scatter) launch_scatter_bytes(0, ds, dm, rows, dd);
    else launch_gather_bytes(0, ds, dm, rows, dd);
    d.after_launch();
  }
  d.sync();
  d.download(dst, dd, out_len);
  return (int)d.e;
}

// present, bad: jobs x N bytes or null, placed off_p / off_b bytes behind a 16-byte boundary; map: jobs entries below used_rows, or
// null (then used_rows >= jobs); idx, slot: jobs x need + 1 entries; used: used_rows x N + 1 bytes in and out, or null; enough:
// jobs + 1
extern "C" int sk_select_shares(const uint8_t* present, const uint8_t* bad, size_t off_p, size_t off_b, size_t N, size_t need, size_t jobs,
                                const uint32_t* map, size_t used_rows, uint64_t* idx, uint32_t* slot, uint8_t* used, uint8_t* enough) {
  if (off_p > 15 || off_b > 15 || need > N || (used && !map && used_rows < jobs)) return (int)hipErrorInvalidValue;
  for (size_t j = 0; map && j < jobs; j++)
    if (map[j] >= used_rows) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dp = up_at(d, present, jobs * N, off_p);
  const uint8_t* db = up_at(d, bad, jobs * N, off_b);
  const uint32_t* dm = (const uint32_t*)up(d, map, jobs * 4);
  uint64_t* didx = (uint64_t*)fresh(d, (jobs * need + 1) * 8);
  uint32_t* dslot = (uint32_t*)fresh(d, (jobs * need + 1) * 4);
  uint8_t* dused = io(d, used, used_rows * N + 1);
  uint8_t* den = fresh(d, jobs + 1);
  if (d.e == hipSuccess) {
    launch_select_shares(0, dp, db, N, need, jobs, dm, didx, dslot, dused, den);
    d.after_launch();
  }
  d.sync();
  d.download(idx, didx, (jobs * need + 1) * 8);
  d.download(slot, dslot, (jobs * need + 1) * 4);
  if (used) d.download(used, dused, used_rows * N + 1);
  d.download(enough, den, jobs + 1);
  return (int)d.e;
}

// shares: jobs x N x point_bytes at off_s (0 or 8) behind a 16-byte boundary; dst: (jobs x need + 1) x point_bytes, written at
// off_d (0 or 8) behind one.  form 0: the launcher's choice (16-byte words when both are 16-byte aligned), 16 / 8: the uint4 /
// uint2 kernel directly.  Every slot of a job with enough shares is checked to lie below N.
extern "C" int sk_gather_selected(const uint8_t* shares, size_t N, size_t need, size_t point_bytes, const uint32_t* slot, const uint8_t* enough,
                                  size_t jobs, int form, size_t off_s, size_t off_d, uint8_t* dst) {
  if ((form != 0 && form != 8 && form != 16) || (off_s != 0 && off_s != 8) || (off_d != 0 && off_d != 8) || point_bytes % 16 || !point_bytes ||
      (form == 16 && (off_s || off_d)))
    return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < jobs; j++)
    for (size_t k = 0; enough[j] && k < need; k++)
      if (slot[j * need + k] >= N) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t out_bytes = (jobs * need + 1) * point_bytes;
  const uint8_t* ds = up_at(d, shares, jobs * N * point_bytes, off_s);
  const uint32_t* dsl = (const uint32_t*)up(d, slot, jobs * need * 4);
  const uint8_t* den = up(d, enough, jobs);
  uint8_t* base = fresh(d, out_bytes + 16);
  uint8_t* dd = base ? base + off_d : nullptr;
  if (d.e == hipSuccess && jobs && need) {
    if (form == 0) {
      launch_gather_selected(0, ds, N, need, point_bytes, dsl, den, jobs, dd);
    } else if (form == 16) {
      const size_t rw = point_bytes / 16;
      hipLaunchKernelGGL(k_gather_selected<uint4>, dim3(grid_for(jobs * need * rw)), dim3(kBlock), 0, 0, ds, N, need, rw, dsl, den, jobs, dd);
    } else {
      const size_t rw = point_bytes / 8;
      hipLaunchKernelGGL(k_gather_selected<uint2>, dim3(grid_for(jobs * need * rw)), dim3(kBlock), 0, 0, ds, N, need, rw, dsl, den, jobs, dd);
    }
    d.after_launch();
  }
  d.sync();
  d.download(dst, dd, out_bytes);
  return (int)d.e;
}

// present: `total` bytes or null; rec: `rows` entries below total; ok: rows; c_present, c_bad: rows + 1; bad: total + 1 in and out,
// or null
extern "C" int sk_robust_mark(const uint8_t* present, const uint32_t* rec, const uint8_t* ok, size_t rows, size_t total, uint8_t* c_present,
                              uint8_t* c_bad, uint8_t* bad) {
  for (size_t r = 0; r < rows; r++)
    if (rec[r] >= total) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dp = up(d, present, total);
  const uint32_t* dr = (const uint32_t*)up(d, rec, rows * 4);
  const uint8_t* dok = up(d, ok, rows);
  uint8_t* dcp = fresh(d, rows + 1);
  uint8_t* dcb = fresh(d, rows + 1);
  uint8_t* dbad = io(d, bad, total + 1);
  if (d.e == hipSuccess) {
    launch_robust_mark(0, dp, dr, dok, rows, dcp, dcb, dbad);
    d.after_launch();
  }
  d.sync();
  d.download(c_present, dcp, rows + 1);
  d.download(c_bad, dcb, rows + 1);
  if (bad) d.download(bad, dbad, total + 1);
  return (int)d.e;
}

// map: `jobs` entries below `total`, or null (then total >= jobs); enough, st: jobs; ok: jobs or null; member: jobs x need or null;
// comb: jobs x point_bytes; out: (total + 1) x point_bytes, status: total + 1, used: total x N + 1 (or null), all three in and out;
// verdict: jobs + 1 or null
extern "C" int sk_robust_finish(const uint32_t* map, size_t N, size_t need, size_t point_bytes, size_t jobs, size_t total, const uint8_t* enough,
                                const uint8_t* st, const uint8_t* ok, const uint8_t* member, const uint8_t* comb, uint8_t* out, uint8_t* status,
                                uint8_t* used, uint8_t* verdict) {
  if (point_bytes % 8 || !point_bytes || (!map && total < jobs)) return (int)hipErrorInvalidValue;
  for (size_t j = 0; map && j < jobs; j++)
    if (map[j] >= total) return (int)hipErrorInvalidValue;
  Dev d;
  const uint32_t* dm = (const uint32_t*)up(d, map, jobs * 4);
  const uint8_t* den = up(d, enough, jobs);
  const uint8_t* dst = up(d, st, jobs);
  const uint8_t* dok = up(d, ok, jobs);
  const uint8_t* dmem = up(d, member, jobs * need);
  const uint8_t* dcomb = up(d, comb, jobs * point_bytes);
  uint8_t* dout = io(d, out, (total + 1) * point_bytes);
  uint8_t* dstatus = io(d, status, total + 1);
  uint8_t* dused = io(d, used, total * N + 1);
  uint8_t* dver = verdict ? fresh(d, jobs + 1) : nullptr;
  if (d.e == hipSuccess) {
    launch_robust_finish(0, dm, N, need, point_bytes, jobs, den, dst, dok, dmem, dcomb, dout, dstatus, dused, dver);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (total + 1) * point_bytes);
  d.download(status, dstatus, total + 1);
  if (used) d.download(used, dused, total * N + 1);
  if (verdict) d.download(verdict, dver, jobs + 1);
  return (int)d.e;
}
