// Single-point kernel conformance harness, part 2 (test code only: never linked into libtc_amd.so, never run by bench.py).
// Includes the product's kernel units k_mul.hip and k_hash.hip as they are; see single_kernels.hip for the rules every entry
// follows (0x5A fill, one guard row / byte / entry behind every written buffer, the product's launcher, the first HIP error).
// Where the launcher derives a geometry -- the register or the arena form of the G1 multiplication, the shared form in G2,
// `share` of k_g2_mul_gather, the two-jobs-per-lane-pair forms of the decoders and hashes -- the entry takes it by value: 0 goes
// through the launcher, another value launches that kernel directly.  Entries that use the table arena return kMpSlotLeak
// unless every slot flag is clear afterwards.
//   build: tests/single_conformance.py (hipcc, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "../../threshold_crypto_amd/csrc/k_mul.hip"
#include "../../threshold_crypto_amd/csrc/k_hash.hip"

#include "manypoint_dev.h"  // Dev, arena, arena_result, kMpSlotLeak, kMpPoison

using namespace tc;

namespace {
const uint8_t* up(Dev& d, const void* p, size_t bytes) { return p ? (const uint8_t*)d.upload(p, bytes) : nullptr; }
uint8_t* fresh(Dev& d, size_t bytes) { return (uint8_t*)d.alloc(bytes, kMpPoison); }
uint8_t* io(Dev& d, const void* p, size_t bytes) { return p ? (uint8_t*)d.upload(p, bytes) : nullptr; }
}  // namespace

// out[j * S + s] = fr[s] * pts[j].  kernel 0: launch_g1_mul, 1: k_point_mul<Fq>, 2: k_g1_mul_arena, 3: launch_g2_mul,
// 4: k_point_mul<Fq2>, 5: k_g2_mul_shared.  out: (S B + 1) points, status: S B + 1 (stays as filled when with_status == 0)
extern "C" int sk_point_mul(int kernel, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  if (kernel < 0 || kernel > 5 || !S || !B) return (int)hipErrorInvalidValue;
  const size_t PB = kernel >= 3 ? 192 : 96, n = S * B;
  Dev d;
  const uint8_t* dfr = up(d, fr, S * 32);
  const uint8_t* dp = up(d, pts, B * PB);
  uint8_t* dout = fresh(d, (n + 1) * PB);
  uint8_t* dst = fresh(d, n + 1);
  uint8_t* st = with_status ? dst : nullptr;
  TableArena ta = arena(d);
  if (d.e == hipSuccess) {
    if (kernel == 0) launch_g1_mul(0, ta, dfr, dp, S, B, dout, st);
    else if (kernel == 1) hipLaunchKernelGGL(k_point_mul<Fq>, dim3(grid_for(n)), dim3(kBlock), 0, 0, dfr, dp, S, B, dout, st, TableArena{nullptr, nullptr});
    else if (kernel == 2) hipLaunchKernelGGL(k_g1_mul_arena, dim3(grid_for(n)), dim3(kBlock), 0, 0, dfr, dp, S, B, dout, st, ta);
    else if (kernel == 3) launch_g2_mul(0, ta, dfr, dp, S, B, dout, st);
    else if (kernel == 4) hipLaunchKernelGGL(k_point_mul<Fq2>, dim3(grid_for(n * kG2Lanes)), dim3(kBlock), 0, 0, dfr, dp, S, B, dout, st, ta);
    else hipLaunchKernelGGL(k_g2_mul_shared, dim3(grid_for((S + kMulShare - 1) / kMulShare * B * kG2Lanes)), dim3(kBlock), 0, 0, dfr, dp, S, B, dout, st, ta);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (n + 1) * PB);
  d.download(status, dst, n + 1);
  return arena_result(d, ta);
}

// out[j * n + k] = sk[idx[j * n + k]] * pts[j]; share 0: launch_g2_mul_gather, 1 .. kGatherShare: k_g2_mul_gather with that share.
// out: (n B + 1) x 192, status: n B + 1
extern "C" int sk_g2_mul_gather(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, size_t share, int with_status,
                                uint8_t* out, uint8_t* status) {
  if (!n || !B || !N || share > (size_t)kGatherShare) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dsk = up(d, sk, N * 32);
  const uint64_t* didx = (const uint64_t*)up(d, idx, n * B * 8);
  const uint8_t* dp = up(d, pts, B * 192);
  uint8_t* dout = fresh(d, (n * B + 1) * 192);
  uint8_t* dst = fresh(d, n * B + 1);
  uint8_t* st = with_status ? dst : nullptr;
  TableArena ta = arena(d);
  if (d.e == hipSuccess) {
    if (share == 0) {
      launch_g2_mul_gather(0, ta, dsk, N, didx, dp, n, B, dout, st);
    } else {
      const size_t chunks = (n + share - 1) / share;
      hipLaunchKernelGGL(k_g2_mul_gather, dim3(grid_for(chunks * B * kG2Lanes)), dim3(kBlock), 0, 0, dsk, N, didx, dp, n, B, dout, st, ta, share);
    }
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (n * B + 1) * 192);
  d.download(status, dst, n * B + 1);
  return arena_result(d, ta);
}

// g2 = 0: k_compress<Fq> (96 -> 48 bytes), 1: k_compress<Fq2> (192 -> 96).  out: (B + 1) encodings, status: B + 1
extern "C" int sk_compress(int g2, const uint8_t* in, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  const size_t PB = g2 ? 192 : 96, CB = PB / 2;
  Dev d;
  const uint8_t* din = up(d, in, B * PB);
  uint8_t* dout = fresh(d, (B + 1) * CB);
  uint8_t* dst = fresh(d, B + 1);
  if (d.e == hipSuccess) {
    if (g2) launch_g2_compress(0, din, B, dout, with_status ? dst : nullptr);
    else launch_g1_compress(0, din, B, dout, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B + 1) * CB);
  d.download(status, dst, B + 1);
  return (int)d.e;
}

// form 0: the launcher (default Tuning), 1: k_decompress<F>, 2: k_decompress_g2_x2 (g2 only).  out: (B + 1) points, status: B + 1
extern "C" int sk_decompress(int g2, int form, const uint8_t* in, size_t B, int with_status, uint8_t* out, uint8_t* status) {
  if (!B || form < 0 || form > 2 || (form == 2 && !g2)) return (int)hipErrorInvalidValue;
  const size_t PB = g2 ? 192 : 96, CB = PB / 2;
  Dev d;
  const uint8_t* din = up(d, in, B * CB);
  uint8_t* dout = fresh(d, (B + 1) * PB);
  uint8_t* dst = fresh(d, B + 1);
  uint8_t* st = with_status ? dst : nullptr;
  if (d.e == hipSuccess) {
    if (form == 0 && g2) launch_g2_decompress(Tuning{}, 0, din, B, dout, st);
    else if (form == 0) launch_g1_decompress(0, din, B, dout, st);
    else if (form == 2) hipLaunchKernelGGL(k_decompress_g2_x2, dim3(grid_for((B + 1) / 2 * kG2Lanes)), dim3(kBlock), 0, 0, din, B, dout, st);
    else if (g2) hipLaunchKernelGGL(k_decompress<Fq2>, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, 0, din, B, dout, st);
    else hipLaunchKernelGGL(k_decompress<Fq>, dim3(grid_for(B)), dim3(kBlock), 0, 0, din, B, dout, st);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B + 1) * PB);
  d.download(status, dst, B + 1);
  return (int)d.e;
}

// in: B x n_per_job compressed samples; form as above (2: k_decompress_take_g2_x2).  out: (B take + 1) points, valid: B take + 1
extern "C" int sk_decompress_take(int g2, int form, const uint8_t* in, size_t n_per_job, size_t take, size_t B, uint8_t* out, uint8_t* valid) {
  if (!B || !take || take > n_per_job || form < 0 || form > 2 || (form == 2 && !g2)) return (int)hipErrorInvalidValue;
  const size_t PB = g2 ? 192 : 96, CB = PB / 2, n = B * take;
  Dev d;
  const uint8_t* din = up(d, in, B * n_per_job * CB);
  uint8_t* dout = fresh(d, (n + 1) * PB);
  uint8_t* dv = fresh(d, n + 1);
  if (d.e == hipSuccess) {
    if (form == 0) launch_decompress_take(Tuning{}, 0, g2 != 0, din, n_per_job, take, B, dout, dv);
    else if (form == 2) hipLaunchKernelGGL(k_decompress_take_g2_x2, dim3(grid_for((n + 1) / 2 * kG2Lanes)), dim3(kBlock), 0, 0, din, n_per_job, take, n, dout, dv);
    else if (g2) hipLaunchKernelGGL(k_decompress_take<Fq2>, dim3(grid_for(n * kG2Lanes)), dim3(kBlock), 0, 0, din, n_per_job, take, n, dout, dv);
    else hipLaunchKernelGGL(k_decompress_take<Fq>, dim3(grid_for(n)), dim3(kBlock), 0, 0, din, n_per_job, take, n, dout, dv);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (n + 1) * PB);
  d.download(valid, dv, n + 1);
  return (int)d.e;
}

// out[j * take + k] = in[j * n_per_job + k]; out: B take + 1 words
extern "C" int sk_take_u64(const uint64_t* in, size_t n_per_job, size_t take, size_t B, uint64_t* out) {
  if (!take || take > n_per_job) return (int)hipErrorInvalidValue;
  Dev d;
  const uint64_t* din = (const uint64_t*)up(d, in, B * n_per_job * 8);
  uint64_t* dout = (uint64_t*)fresh(d, (B * take + 1) * 8);
  if (d.e == hipSuccess) {
    launch_take_u64(0, din, n_per_job, take, B, dout);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B * take + 1) * 8);
  return (int)d.e;
}

// in: jobs x N compressed shares; slot: jobs x need, every slot of a job with enough shares checked to lie below N; form as
// above (2: k_decompress_selected_g2_x2).  out: (jobs need + 1) points, ok: jobs need + 1
extern "C" int sk_decompress_selected(int g2, int form, const uint8_t* in, size_t N, size_t need, const uint32_t* slot, const uint8_t* enough,
                                      size_t jobs, uint8_t* out, uint8_t* ok) {
  if (!jobs || !need || form < 0 || form > 2 || (form == 2 && !g2)) return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < jobs; j++)
    for (size_t k = 0; enough[j] && k < need; k++)
      if (slot[j * need + k] >= N) return (int)hipErrorInvalidValue;
  const size_t PB = g2 ? 192 : 96, CB = PB / 2, n = jobs * need;
  Dev d;
  const uint8_t* din = up(d, in, jobs * N * CB);
  const uint32_t* dsl = (const uint32_t*)up(d, slot, n * 4);
  const uint8_t* den = up(d, enough, jobs);
  uint8_t* dout = fresh(d, (n + 1) * PB);
  uint8_t* dok = fresh(d, n + 1);
  if (d.e == hipSuccess) {
    if (form == 0) launch_decompress_selected(Tuning{}, 0, g2 != 0, din, N, need, dsl, den, jobs, dout, dok);
    else if (form == 2)
      hipLaunchKernelGGL(k_decompress_selected_g2_x2, dim3(grid_for((n + 1) / 2 * kG2Lanes)), dim3(kBlock), 0, 0, din, N, need, dsl, den, n, dout, dok);
    else if (g2) hipLaunchKernelGGL(k_decompress_selected<Fq2>, dim3(grid_for(n * kG2Lanes)), dim3(kBlock), 0, 0, din, N, need, dsl, den, n, dout, dok);
    else hipLaunchKernelGGL(k_decompress_selected<Fq>, dim3(grid_for(n)), dim3(kBlock), 0, 0, din, N, need, dsl, den, n, dout, dok);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (n + 1) * PB);
  d.download(ok, dok, n + 1);
  return (int)d.e;
}

// what 0: k_fr_scale_cofactor_fix (in: n x 32, out: (n + 1) x 32); 1: k_g1_scale_cofactor_fix (in: in_bytes >= (n - 1) stride + 96,
// out: (n + 1) x 96); 2: k_fill_g1_generator (out: two rows of 96 bytes, each with a guard row behind it: 4 x 96)
extern "C" int sk_small(int what, const uint8_t* in, size_t in_bytes, size_t stride, size_t n, uint8_t* out) {
  if (what < 0 || what > 2 || (what == 0 && in_bytes < n * 32) || (what == 1 && (!n || in_bytes < (n - 1) * stride + 96))) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* din = up(d, in, in_bytes);
  const size_t ob = what == 0 ? (n + 1) * 32 : what == 1 ? (n + 1) * 96 : 4 * 96;
  uint8_t* dout = fresh(d, ob);
  if (d.e == hipSuccess) {
    if (what == 0) launch_fr_scale_cofactor_fix(0, din, n, dout);
    else if (what == 1) launch_g1_scale_cofactor_fix(0, din, stride, n, dout);
    else launch_fill_g1_generator(0, dout, dout + 2 * 96);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, ob);
  return (int)d.e;
}

// commit: (t + 1) x 96; idx: M; out: (M + 1) x 96, status: M + 1
extern "C" int sk_commitment_evaluate(const uint8_t* commit, size_t t, const uint64_t* idx, size_t M, int with_status, uint8_t* out, uint8_t* status) {
  Dev d;
  const uint8_t* dc = up(d, commit, (t + 1) * 96);
  const uint64_t* di = (const uint64_t*)up(d, idx, M * 8);
  uint8_t* dout = fresh(d, (M + 1) * 96);
  uint8_t* dst = fresh(d, M + 1);
  if (d.e == hipSuccess) {
    launch_commitment_evaluate(0, dc, t, di, M, dout, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (M + 1) * 96);
  d.download(status, dst, M + 1);
  return (int)d.e;
}

// g1: null (k_hash_g2 / _x2) or B x 96 (k_hash_g1_g2 / _x2); off: B + 1 offsets into msgs (off[B] bytes); form 0: the launcher
// (default Tuning), 1: the one-job kernel, 2: the _x2 kernel.  out: (B + 1) x 192, status: B + 1 (written by the g1 forms only)
extern "C" int sk_hash(const uint8_t* g1, const uint8_t* msgs, const uint64_t* off, size_t B, int fix, int form, int with_status, uint8_t* out,
                       uint8_t* status) {
  if (!B || form < 0 || form > 2) return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < B; j++)
    if (off[j] > off[j + 1]) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dg = up(d, g1, B * 96);
  const uint8_t* dm = (const uint8_t*)d.upload(msgs, off[B]);
  const uint64_t* doff = (const uint64_t*)up(d, off, (B + 1) * 8);
  uint8_t* dout = fresh(d, (B + 1) * 192);
  uint8_t* dst = fresh(d, B + 1);
  uint8_t* st = with_status ? dst : nullptr;
  const unsigned g1job = grid_for(B * kG2Lanes), g2job = grid_for((B + 1) / 2 * kG2Lanes);
  if (d.e == hipSuccess) {
    if (form == 0 && g1) launch_hash_g1_g2(Tuning{}, 0, dg, dm, doff, B, dout, st, fix != 0);
    else if (form == 0) launch_hash_g2(Tuning{}, 0, dm, doff, B, dout, fix != 0);
    else if (form == 1 && g1) hipLaunchKernelGGL(k_hash_g1_g2, dim3(g1job), dim3(kBlock), 0, 0, dg, dm, doff, B, dout, st, fix);
    else if (form == 1) hipLaunchKernelGGL(k_hash_g2, dim3(g1job), dim3(kBlock), 0, 0, dm, doff, B, dout, fix);
    else if (g1) hipLaunchKernelGGL(k_hash_g1_g2_x2, dim3(g2job), dim3(kBlock), 0, 0, dg, dm, doff, B, dout, st, fix);
    else hipLaunchKernelGGL(k_hash_g2_x2, dim3(g2job), dim3(kBlock), 0, 0, dm, doff, B, dout, fix);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, (B + 1) * 192);
  d.download(status, dst, B + 1);
  return (int)d.e;
}

// g1: B x 96; data: off[B] bytes; status: B + 1 in and out, or null; out: off[B] + 1 bytes
extern "C" int sk_xor_with_hash(const uint8_t* g1, const uint8_t* data, const uint64_t* off, size_t B, uint8_t* status, uint8_t* out) {
  if (!B) return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < B; j++)
    if (off[j] > off[j + 1]) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dg = up(d, g1, B * 96);
  const uint8_t* dd = (const uint8_t*)d.upload(data, off[B]);
  const uint64_t* doff = (const uint64_t*)up(d, off, (B + 1) * 8);
  uint8_t* dst = io(d, status, B + 1);
  uint8_t* dout = fresh(d, off[B] + 1);
  if (d.e == hipSuccess) {
    launch_xor_with_hash(0, dg, dd, doff, B, dout, dst);
    d.after_launch();
  }
  d.sync();
  if (status) d.download(status, dst, B + 1);
  d.download(out, dout, off[B] + 1);
  return (int)d.e;
}

// pk: 96 bytes (pk_stride 0: one key for every job) or B x 96; r: B x 32; off: B + 1 offsets into msgs.  u: (B + 1) x 96,
// v: off[B] + 1 bytes, w: (B + 1) x 192, status: B + 1
extern "C" int sk_encrypt(const uint8_t* pk, size_t pk_stride, const uint8_t* r, const uint8_t* msgs, const uint64_t* off, size_t B, int with_status,
                          uint8_t* u, uint8_t* v, uint8_t* w, uint8_t* status) {
  if (!B || (pk_stride != 0 && pk_stride != 96)) return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < B; j++)
    if (off[j] > off[j + 1]) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dpk = up(d, pk, pk_stride ? B * 96 : 96);
  const uint8_t* dr = up(d, r, B * 32);
  const uint8_t* dm = (const uint8_t*)d.upload(msgs, off[B]);
  const uint64_t* doff = (const uint64_t*)up(d, off, (B + 1) * 8);
  uint8_t* du = fresh(d, (B + 1) * 96);
  uint8_t* dv = fresh(d, off[B] + 1);
  uint8_t* dw = fresh(d, (B + 1) * 192);
  uint8_t* dst = fresh(d, B + 1);
  TableArena ta = arena(d);
  if (d.e == hipSuccess) {
    launch_encrypt(0, ta, dpk, pk_stride, dr, dm, doff, B, du, dv, dw, with_status ? dst : nullptr);
    d.after_launch();
  }
  d.sync();
  d.download(u, du, (B + 1) * 96);
  d.download(v, dv, off[B] + 1);
  d.download(w, dw, (B + 1) * 192);
  d.download(status, dst, B + 1);
  return arena_result(d, ta);
}
