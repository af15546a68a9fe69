// Many-point conformance harness (test code only: never linked into libtc_amd.so, never run by bench.py).
// Includes the product's kernel units k_msm.hip and k_comb.hip as they are (every unit of the product is self-contained:
// -fno-gpu-rdc), so the __global__ kernels launched here are the product's own text, compiled with the product's flags.
// Eight entries (the two-stage sums in G2 and G1, the comb signer, the ragged sums and their key gather, the paired ragged sums,
// the G1 comb of the decryption shares and the arena ladders beside it); each allocates, copies in, launches, synchronises once, copies out, frees and returns the first HIP
// error.  `parts` / `share` = 0 goes through the product's launcher (its own rule for the launch geometry); another value
// launches the stage kernels directly with that value.  Tables, codes, outputs and written-only status bytes are filled
// with 0x5A before the launch, so the caller sees what the kernels left in memory -- and what they did not touch.
// The blame-by-bisection kernels (k_blame.hip) have a harness file of their own beside this one: manypoint_blame.hip.
//   build: tests/manypoint_conformance.py (hipcc, keyed by a hash of the sources)
#include <hip/hip_runtime.h>
#include "../../threshold_crypto_amd/csrc/k_msm.hip"
#include "../../threshold_crypto_amd/csrc/k_comb.hip"

#include "manypoint_dev.h"  // Dev, arena, arena_result, kMpSlotLeak, kMpPoison

#include <string.h>
#include <vector>

using namespace tc;

namespace {
bool legal_parts(size_t parts, size_t n, size_t most) {
  return parts <= most && (parts & (parts - 1)) == 0 && (parts <= 1 || 4 * parts <= n);
}
size_t points_bytes(size_t n, size_t B, size_t stride, size_t point) { return (B - 1) * stride + n * point; }
}  // namespace

// G2: out (B x 192), status (B, copied in from status_in first), tbl (msm_table_bytes(n, B)), codes (msm_code_bytes(n, B)).
// idx: null, or B x n_per_job indices for the MsmFilter with threshold t; need_value < 0: no `need` word, else its value.
extern "C" int mp_msm_g2(size_t n, size_t B, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, const uint8_t* status_in,
                         int nbits, size_t parts, const uint64_t* idx, size_t n_per_job, size_t t, int need_value, uint8_t* out,
                         uint8_t* status, int32_t* tbl, uint8_t* codes) {
  if (!n || !B || nbits < 1 || nbits > 64 || !legal_parts(parts, n, 32)) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t tb = msm_table_bytes(n, B), cb = msm_code_bytes(n, B);
  const uint8_t* dpts = (const uint8_t*)d.upload(points, points_bytes(n, B, pts_stride, 192));
  const uint32_t* dsc = (const uint32_t*)d.upload(scalars, B * n * 32);
  uint8_t* dst = (uint8_t*)d.upload(status_in, B);
  uint8_t* dout = (uint8_t*)d.alloc(B * 192, kMpPoison);
  int32_t* dtbl = (int32_t*)d.alloc(tb, kMpPoison);
  uint8_t* dcodes = (uint8_t*)d.alloc(cb, kMpPoison);
  MsmFilter f;
  if (idx) {
    f.idx = (const uint64_t*)d.upload(idx, B * n_per_job * 8);
    f.n_per_job = n_per_job;
    f.t = t;
  }
  if (need_value >= 0) {
    const uint32_t v = (uint32_t)need_value;
    f.need = (const uint32_t*)d.upload(&v, 4);
  }
  if (d.e == hipSuccess) {
    if (parts == 0) {
      launch_msm_g2(0, n, pts_stride, dpts, dsc, B, dtbl, dcodes, dout, dst, nbits, f);
    } else {
      hipLaunchKernelGGL(k_msm_tables, dim3(grid_for(B * msm_chunks(n) * kG2Lanes)), dim3(kBlock), 0, 0, n, pts_stride, dpts, dsc, B, dtbl,
                         dcodes, dst, nbits, f);
      if (parts == 1)
        hipLaunchKernelGGL(k_msm_ladder, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, 0, n, B, (const int32_t*)dtbl, (const uint8_t*)dcodes,
                           dout, (const uint8_t*)dst, nbits, f);
      else
        hipLaunchKernelGGL(k_msm_ladder_split, dim3(grid_for(B * parts * kG2Lanes)), dim3(kBlock), 0, 0, n, B, (const int32_t*)dtbl,
                           (const uint8_t*)dcodes, dout, (const uint8_t*)dst, nbits, f, parts);
    }
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, B * 192);
  d.download(status, dst, B);
  d.download(tbl, dtbl, tb);
  d.download(codes, dcodes, cb);
  return (int)d.e;
}

// G1: out (B x 96), status (B), tbl (msm_table_bytes_g1(n, B): B table sets in shared mode too), codes (msm_code_bytes).
// pts_stride = 0 with nbits < 128: the shared table set.
extern "C" int mp_msm_g1(size_t n, size_t B, size_t pts_stride, const uint8_t* points, const uint32_t* scalars, const uint8_t* status_in,
                         int nbits, size_t parts, uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes) {
  if (!n || !B || nbits < 2 || nbits > 128 || (nbits & 1) || !legal_parts(parts, n, 64)) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t tb = msm_table_bytes_g1(n, B), cb = msm_code_bytes(n, B);
  const uint8_t* dpts = (const uint8_t*)d.upload(points, points_bytes(n, B, pts_stride, 96));
  const uint32_t* dsc = (const uint32_t*)d.upload(scalars, B * n * 32);
  uint8_t* dst = (uint8_t*)d.upload(status_in, B);
  uint8_t* dout = (uint8_t*)d.alloc(B * 96, kMpPoison);
  int32_t* dtbl = (int32_t*)d.alloc(tb, kMpPoison);
  uint8_t* dcodes = (uint8_t*)d.alloc(cb, kMpPoison);
  if (d.e == hipSuccess) {
    if (parts == 0) {
      launch_msm_g1(0, n, pts_stride, dpts, dsc, B, dtbl, dcodes, dout, dst, nbits);
    } else {
      const int top = nbits / 2;
      const int shared = msm_g1_shared_tables(pts_stride, nbits) ? 1 : 0;
      hipLaunchKernelGGL(k_msm_tables_g1, dim3(grid_for(B * msm_chunks(n))), dim3(kBlock), 0, 0, n, pts_stride, dpts, dsc, B, dtbl, dcodes, dst,
                         nbits);
      if (parts == 1)
        hipLaunchKernelGGL(k_msm_ladder_g1<false>, dim3(grid_for(B)), dim3(kBlock), 0, 0, n, B, (const int32_t*)dtbl, (const uint8_t*)dcodes, dout,
                           (const uint8_t*)dst, parts, top, shared);
      else
        hipLaunchKernelGGL(k_msm_ladder_g1<true>, dim3(grid_for(B * parts)), dim3(kBlock), 0, 0, n, B, (const int32_t*)dtbl,
                           (const uint8_t*)dcodes, dout, (const uint8_t*)dst, parts, top, shared);
    }
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, B * 96);
  d.download(status, dst, B);
  d.download(tbl, dtbl, tb);
  d.download(codes, dcodes, cb);
  return (int)d.e;
}

// Comb: sk (N x 32), idx (B x n), pts (B x 192); out (B x n x 192), status (B x n), ok (B), tbl (comb_table_bytes(B)).
// Runs with a table arena of the product's geometry; every slot flag must be clear again afterwards (kMpSlotLeak).
extern "C" int mp_comb(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, size_t share, uint8_t* out,
                       uint8_t* status, uint8_t* ok, int32_t* tbl) {
  if (!n || !B || !N || share > (size_t)kCombShare) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t tb = comb_table_bytes(B);
  const uint8_t* dsk = (const uint8_t*)d.upload(sk, N * 32);
  const uint64_t* didx = (const uint64_t*)d.upload(idx, B * n * 8);
  const uint8_t* dpts = (const uint8_t*)d.upload(pts, B * 192);
  uint8_t* dout = (uint8_t*)d.alloc(B * n * 192, kMpPoison);
  uint8_t* dst = (uint8_t*)d.alloc(B * n, kMpPoison);
  uint8_t* dok = (uint8_t*)d.alloc(B, kMpPoison);
  int32_t* dtbl = (int32_t*)d.alloc(tb, kMpPoison);
  TableArena ta = arena(d);
  if (d.e == hipSuccess) {
    if (share == 0) {
      launch_comb_sign(0, ta, dsk, N, didx, dpts, n, B, dtbl, dok, dout, dst);
    } else {
      hipLaunchKernelGGL(k_comb_tables, dim3(grid_for(B * kG2Lanes)), dim3(kBlock), 0, 0, dpts, B, dtbl, dok);
      const size_t chunks = (n + share - 1) / share;
      hipLaunchKernelGGL(k_comb_sign, dim3(grid_for(chunks * B * kG2Lanes)), dim3(kBlock), 0, 0, dsk, N, didx, (const int32_t*)dtbl,
                         (const uint8_t*)dok, n, B, dout, dst, ta, share);
    }
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, B * n * 192);
  d.download(status, dst, B * n);
  d.download(ok, dok, B);
  d.download(tbl, dtbl, tb);
  return arena_result(d, ta);
}

// The ragged sums (k_rec_tables_g2 / k_rec_ladder_g2, w = 2; k_rec_tables_g1 / k_rec_ladder_g1, w = 1) through their launchers, the
// only route to these kernels: `parts` goes in by value, legal or not.  J segments of one record array (seg_first: J + 1
// values); first_chunk_out (J + 1) is rec_chunk_ranges' answer.  out: (J + 1) rows, status: J bytes, tbl: rec_table_bytes and
// codes: rec_code_bytes of the launch's chunks AND ONE MORE (the guard rows / chunk behind them come back as they were filled).
extern "C" int mp_rec_sum(int w, size_t J, const uint64_t* seg_first, const uint8_t* points, const uint32_t* scalars, const uint8_t* status_in,
                          int nbits, size_t parts, uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes, uint64_t* first_chunk_out) {
  const bool g2 = w == 2;
  if ((w != 1 && w != 2) || nbits < 2 || nbits > (g2 ? 64 : 128) || (!g2 && (nbits & 1))) return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < J; j++)
    if (seg_first[j + 1] < seg_first[j]) return (int)hipErrorInvalidValue;
  std::vector<uint64_t> fc(J + 1);
  const uint64_t chunks = rec_chunk_ranges(seg_first, J, fc.data());
  memcpy(first_chunk_out, fc.data(), (J + 1) * 8);
  const size_t R = (size_t)seg_first[J], pt = g2 ? 192 : 96;
  const size_t tb = rec_table_bytes(g2, chunks + 1), cb = rec_code_bytes(chunks + 1), ob = (J + 1) * pt;
  Dev d;
  const uint8_t* dpts = (const uint8_t*)d.upload(points, R * pt);
  const uint32_t* dsc = (const uint32_t*)d.upload(scalars, R * 32);
  const uint64_t* dseg = (const uint64_t*)d.upload(seg_first, (J + 1) * 8);
  const uint64_t* dfc = (const uint64_t*)d.upload(fc.data(), (J + 1) * 8);
  uint8_t* dst = (uint8_t*)d.upload(status_in, J);
  uint8_t* dout = (uint8_t*)d.alloc(ob, kMpPoison);
  int32_t* dtbl = (int32_t*)d.alloc(tb, kMpPoison);
  uint8_t* dcodes = (uint8_t*)d.alloc(cb, kMpPoison);
  if (d.e == hipSuccess) {
    if (g2) launch_rec_sum_g2(0, dpts, dsc, dseg, dfc, J, chunks, parts, dtbl, dcodes, dout, dst, nbits);
    else launch_rec_sum_g1(0, dpts, dsc, dseg, dfc, J, chunks, parts, dtbl, dcodes, dout, dst, nbits);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, ob);
  d.download(status, dst, J);
  d.download(tbl, dtbl, tb);
  d.download(codes, dcodes, cb);
  return (int)d.e;
}

// The PAIRED ragged sums (k_rec_tables_g1_pair / k_rec_ladder_g1_pair) through launch_rec_sum_g1_pair, the only route: segment j
// over points_a and over points_b with the same scalars.  out: 2 J + 2 rows (A_j, -B_j interleaved, two guard rows), status: J bytes,
// tbl / codes: 2 x the launch's chunks AND ONE MORE (the guard chunk behind half 1).
extern "C" int mp_rec_sum_pair(size_t J, const uint64_t* seg_first, const uint8_t* points_a, const uint8_t* points_b, const uint32_t* scalars,
                               const uint8_t* status_in, int nbits, size_t parts, uint8_t* out, uint8_t* status, int32_t* tbl, uint8_t* codes,
                               uint64_t* first_chunk_out) {
  if (nbits < 2 || nbits > 128 || (nbits & 1)) return (int)hipErrorInvalidValue;
  for (size_t j = 0; j < J; j++)
    if (seg_first[j + 1] < seg_first[j]) return (int)hipErrorInvalidValue;
  std::vector<uint64_t> fc(J + 1);
  const uint64_t chunks = rec_chunk_ranges(seg_first, J, fc.data());
  memcpy(first_chunk_out, fc.data(), (J + 1) * 8);
  const size_t R = (size_t)seg_first[J];
  const size_t tb = rec_table_bytes(false, 2 * chunks + 1), cb = rec_code_bytes(2 * chunks + 1), ob = (2 * J + 2) * 96;
  Dev d;
  const uint8_t* dpa = (const uint8_t*)d.upload(points_a, R * 96);
  const uint8_t* dpb = (const uint8_t*)d.upload(points_b, R * 96);
  const uint32_t* dsc = (const uint32_t*)d.upload(scalars, R * 32);
  const uint64_t* dseg = (const uint64_t*)d.upload(seg_first, (J + 1) * 8);
  const uint64_t* dfc = (const uint64_t*)d.upload(fc.data(), (J + 1) * 8);
  uint8_t* dst = (uint8_t*)d.upload(status_in, J);
  uint8_t* dout = (uint8_t*)d.alloc(ob, kMpPoison);
  int32_t* dtbl = (int32_t*)d.alloc(tb, kMpPoison);
  uint8_t* dcodes = (uint8_t*)d.alloc(cb, kMpPoison);
  if (d.e == hipSuccess) {
    launch_rec_sum_g1_pair(0, dpa, dpb, dsc, dseg, dfc, J, chunks, parts, dtbl, dcodes, dout, dst, nbits);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, ob);
  d.download(status, dst, J);
  d.download(tbl, dtbl, tb);
  d.download(codes, dcodes, cb);
  return (int)d.e;
}

// G1 comb: sk (N x 32), idx (B x n), pts (B x 96); out (B n + 1 rows of 96), status (B n + 1), ok (B + 1), tbl (comb_table_bytes_g1(B)
// and one entry of 128 bytes): the last row / byte / entry of each is a guard.  share = 0: launch_comb_decrypt.
extern "C" int mp_comb_g1(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, size_t share, uint8_t* out,
                          uint8_t* status, uint8_t* ok, int32_t* tbl) {
  if (!n || !B || !N || share > (size_t)kCombG1Share) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t tb = comb_table_bytes_g1(B) + kMsmEntryWordsG1 * sizeof(int32_t), rows = B * n + 1;
  const uint8_t* dsk = (const uint8_t*)d.upload(sk, N * 32);
  const uint64_t* didx = (const uint64_t*)d.upload(idx, B * n * 8);
  const uint8_t* dpts = (const uint8_t*)d.upload(pts, B * 96);
  uint8_t* dout = (uint8_t*)d.alloc(rows * 96, kMpPoison);
  uint8_t* dst = (uint8_t*)d.alloc(rows, kMpPoison);
  uint8_t* dok = (uint8_t*)d.alloc(B + 1, kMpPoison);
  int32_t* dtbl = (int32_t*)d.alloc(tb, kMpPoison);
  if (d.e == hipSuccess) {
    if (share == 0) {
      launch_comb_decrypt(0, dsk, N, didx, dpts, n, B, dtbl, dok, dout, dst);
    } else {
      hipLaunchKernelGGL(k_comb_tables_g1, dim3(grid_for(B)), dim3(kBlock), 0, 0, dpts, B, dtbl, dok);
      const size_t chunks = (n + share - 1) / share;
      hipLaunchKernelGGL(k_comb_decrypt, dim3(grid_for(chunks * B)), dim3(kBlock), 0, 0, dsk, N, didx, (const int32_t*)dtbl, (const uint8_t*)dok, n, B,
                         dout, dst, share);
    }
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, rows * 96);
  d.download(status, dst, rows);
  d.download(ok, dok, B + 1);
  d.download(tbl, dtbl, tb);
  return (int)d.e;
}

// k_g1_mul_gather through its launcher, with a table arena of the product's geometry: out (B n + 1 rows), status (B n + 1), the
// last of each a guard; every slot flag must be clear again afterwards (kMpSlotLeak)
extern "C" int mp_g1_mul_gather(const uint8_t* sk, size_t N, const uint64_t* idx, const uint8_t* pts, size_t n, size_t B, uint8_t* out,
                                uint8_t* status) {
  if (!n || !B || !N) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t rows = B * n + 1;
  const uint8_t* dsk = (const uint8_t*)d.upload(sk, N * 32);
  const uint64_t* didx = (const uint64_t*)d.upload(idx, B * n * 8);
  const uint8_t* dpts = (const uint8_t*)d.upload(pts, B * 96);
  uint8_t* dout = (uint8_t*)d.alloc(rows * 96, kMpPoison);
  uint8_t* dst = (uint8_t*)d.alloc(rows, kMpPoison);
  TableArena ta = arena(d);
  if (d.e == hipSuccess) {
    launch_g1_mul_gather(0, ta, dsk, N, didx, dpts, n, B, dout, dst);
    d.after_launch();
  }
  d.sync();
  d.download(out, dout, rows * 96);
  d.download(status, dst, rows);
  return arena_result(d, ta);
}

// k_rec_gather_keys through its launcher: pks (K x 96), key_idx (R), keys (R x 96 and 96 guard bytes behind them)
extern "C" int mp_rec_gather_keys(const uint8_t* pks, size_t K, const uint64_t* key_idx, size_t R, uint8_t* keys) {
  Dev d;
  const uint8_t* dpk = (const uint8_t*)d.upload(pks, K * 96);
  const uint64_t* didx = (const uint64_t*)d.upload(key_idx, R * 8);
  uint8_t* dkeys = (uint8_t*)d.alloc(R * 96 + 96, kMpPoison);
  if (d.e == hipSuccess) {
    launch_rec_gather_keys(0, dpk, K, didx, R, dkeys);
    d.after_launch();
  }
  d.sync();
  d.download(keys, dkeys, R * 96 + 96);
  return (int)d.e;
}
