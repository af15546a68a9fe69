// The call frame of the C ABI on the CPU (tests/test_call_host.py; a test harness -- not a product path):
// threshold_crypto_amd/csrc/tc_api.hip compiled unchanged by g++ against tests/call/fake_hip, linked with the deferring runtime
// of fake_runtime.cpp and the stub launchers below, which compute nothing cryptographic: checks answer from a switch of the
// harness, scalar and MSM stubs carry the SECRET bytes they are given into their outputs, the row movers really move rows.
// main() drives the entries whose host decides in mid-call -- clean and with the last job failing, host and device I/O -- and
// fails the k-th host allocation of each for k = 0, 1, 2, ... (see sweep()).  Built with the address and undefined-behaviour
// sanitizers: a copy that runs after its host side was freed is a report.
//
//   call_host            the sweep over every case; prints "call_host: ok"
//   call_host --counts   host allocations per call of an uninjected run, one line per case
#include "../../include/tc_amd.h"
#include "../../threshold_crypto_amd/csrc/tc_launch.h"
#include "../../threshold_crypto_amd/csrc/tc_robust.h"
#include "fake_runtime.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

// ---- what the stubs answer --------------------------------------------------------------------------------------------------
static bool g_fail_last = false;  // every check launch answers 0 for its LAST row (job, group, share, range)
static size_t g_bad_key_n = 0;    // a G1 membership test over exactly this many points answers 0 for the last one (0: never)

// (the closure is the fake runtime's, like the queue it goes into: a launcher of the product allocates nothing on the host)
#define DEFER(st, ...)                       \
  do {                                       \
    fake::Quiet quiet_;                      \
    fake::enqueue(st, [=] { __VA_ARGS__; }); \
  } while (0)

namespace tc {

static void answer(hipStream_t st, uint8_t* ok, size_t rows) {
  const bool fail = g_fail_last;
  DEFER(st, memset(ok, 1, rows); if (fail && rows) ok[rows - 1] = 0);
}
static void spread(hipStream_t st, const uint8_t* seed32, uint8_t* out, size_t bytes) {
  DEFER(st, for (size_t i = 0; i < bytes; i++) out[i] = seed32[i % 32]);
}

// sizes: small, and whole words where the unit divides by sizeof(int32_t)
size_t msm_table_bytes(size_t n, size_t B) { return n * B * 64; }
size_t msm_table_bytes_g1(size_t n, size_t B) { return n * B * 64; }
size_t msm_code_bytes(size_t n, size_t B) { return n * B * 32; }
size_t msm_table_jobs_g1(size_t pts_stride, int nbits, size_t B) { return pts_stride == 0 && nbits < 128 ? 1 : B; }
size_t rec_table_bytes(bool, uint64_t chunks) { return (size_t)(chunks + 1) * 64; }
size_t rec_code_bytes(uint64_t chunks) { return (size_t)(chunks + 1) * 32; }
int pairing_form(size_t, const Tuning&) { return 0; }
bool pairing_form_needs_lines(int) { return false; }
size_t pairing_tile(size_t, size_t) { return 0; }
size_t pairing_ws_words(size_t B, size_t) { return B * 4; }
size_t pairing_product_ws_words(size_t n, size_t B, bool) { return n * B * 4; }
size_t blame_leaf_bytes(bool g2) { return g2 ? 576 : 384; }
size_t blame_sink_bytes() { return 64; }
size_t blame_sum_parts(bool, size_t, size_t, int) { return 1; }
size_t fixed_base_table_bytes() { return 64; }
size_t lagrange_all_ws_words(size_t, size_t) { return 8; }

// checks: the switch of the harness
void launch_pairing_check(hipStream_t st, const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*, size_t, size_t B,
                          uint8_t* ok, PairingWs) {
  answer(st, ok, B);
}
void launch_pairing_product_check(hipStream_t st, const uint8_t*, size_t, const uint8_t*, size_t, size_t, size_t B, const uint8_t*, size_t, const uint8_t*,
                                  size_t, uint8_t* ok, int32_t*) {
  answer(st, ok, B);
}
void launch_g1_is_identity(hipStream_t st, const uint8_t*, const uint8_t*, const uint8_t*, size_t B, uint8_t* ok) { answer(st, ok, B); }
void launch_g1_equal(hipStream_t st, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, size_t, size_t B, uint8_t* ok) { answer(st, ok, B); }
void launch_robust_finish(hipStream_t st, const uint32_t* map, size_t, size_t, size_t point_bytes, size_t jobs, const uint8_t*, const uint8_t*, const uint8_t*,
                          const uint8_t*, const uint8_t*, uint8_t* out, uint8_t* status, uint8_t*, uint8_t* verdict) {
  const bool fail = g_fail_last;
  DEFER(st, for (size_t f = 0; f < jobs; f++) {
    const size_t j = map ? map[f] : f;
    status[j] = TC_JOB_OK;
    memset(out + j * point_bytes, 0, point_bytes);
    if (verdict) verdict[f] = fail && f == jobs - 1 ? kRobustRetry : kRobustGood;
  });
}
void launch_subgroup_check_g1(hipStream_t st, const uint8_t*, size_t, size_t, size_t, size_t n, uint8_t* valid) {
  const bool bad = g_bad_key_n && n == g_bad_key_n;
  DEFER(st, memset(valid, 1, n); if (bad) valid[n - 1] = 0);
}
void launch_subgroup_check_g2(hipStream_t st, const uint8_t*, size_t, size_t, size_t, size_t n, uint8_t* valid) { DEFER(st, memset(valid, 1, n)); }

// secrets: the seed's bytes go into the scalars, the scalars' bytes into the digit codes
void launch_rlc_scalars(hipStream_t st, const uint8_t* seed32, size_t n, uint8_t* out_fr) { spread(st, seed32, out_fr, n * 32); }
void launch_rlc_scalars_g1(hipStream_t st, const uint8_t* seed32, size_t n, uint8_t* out_fr) { spread(st, seed32, out_fr, n * 32); }
void launch_dkg_rlc_scalars(hipStream_t st, const uint8_t* seed32, const uint64_t*, const uint8_t*, size_t, size_t degree, size_t B, uint32_t* scalars,
                            uint8_t* valid) {
  spread(st, seed32, (uint8_t*)scalars, B * (degree + 2) * 32);
  DEFER(st, memset(valid, 1, B));
}
void launch_blame_seed(hipStream_t st, const uint8_t* key32, uint64_t, uint8_t* seed_out) { DEFER(st, memcpy(seed_out, key32, 32)); }
void launch_msm_g2(hipStream_t st, size_t n, size_t, const uint8_t*, const uint32_t* scalars, size_t B, int32_t*, uint8_t* codes, uint8_t*, uint8_t*, int,
                   MsmFilter) {
  DEFER(st, memcpy(codes, scalars, n * B * 32));
}
void launch_msm_g1(hipStream_t st, size_t n, size_t, const uint8_t*, const uint32_t* scalars, size_t B, int32_t*, uint8_t* codes, uint8_t*, uint8_t*, int) {
  DEFER(st, memcpy(codes, scalars, n * B * 32));
}
// (the ragged sums are not told how many records there are: the first scalar stands for all of them)
void launch_rec_sum_g2(hipStream_t st, const uint8_t*, const uint32_t* scalars, const uint64_t*, const uint64_t*, size_t, uint64_t, size_t, int32_t*,
                       uint8_t* codes, uint8_t*, uint8_t*, int) {
  DEFER(st, memcpy(codes, scalars, 32));
}
void launch_rec_sum_g1(hipStream_t st, const uint8_t*, const uint32_t* scalars, const uint64_t*, const uint64_t*, size_t, uint64_t, size_t, int32_t*,
                       uint8_t* codes, uint8_t*, uint8_t*, int) {
  DEFER(st, memcpy(codes, scalars, 32));
}
void launch_rec_sum_g1_pair(hipStream_t st, const uint8_t*, const uint8_t*, const uint32_t* scalars, const uint64_t*, const uint64_t*, size_t, uint64_t,
                            size_t, int32_t*, uint8_t* codes, uint8_t*, uint8_t*, int) {
  DEFER(st, memcpy(codes, scalars, 32));
}

// the row movers of the fallbacks: real
void launch_gather_rows(hipStream_t st, const uint8_t* src, size_t row_bytes, const uint32_t* map, size_t rows, uint8_t* dst) {
  DEFER(st, for (size_t r = 0; r < rows; r++) memcpy(dst + r * row_bytes, src + (size_t)map[r] * row_bytes, row_bytes));
}
void launch_scatter_bytes(hipStream_t st, const uint8_t* src, const uint32_t* map, size_t rows, uint8_t* dst) {
  DEFER(st, for (size_t r = 0; r < rows; r++) dst[map[r]] = src[r]);
}
void launch_gather_bytes(hipStream_t st, const uint8_t* src, const uint32_t* map, size_t rows, uint8_t* dst) {
  DEFER(st, for (size_t r = 0; r < rows; r++) dst[r] = src[map[r]]);
}
void launch_ok_and_status(hipStream_t st, const uint8_t* status, size_t B, uint8_t* ok) {
  DEFER(st, for (size_t j = 0; j < B; j++) ok[j] = ok[j] && status[j] == TC_JOB_OK);
}
void launch_g2_compress(hipStream_t st, const uint8_t*, size_t B, uint8_t* out, uint8_t*) { DEFER(st, memset(out, 0, B * 96)); }
void launch_g1_decompress(hipStream_t st, const uint8_t*, size_t B, uint8_t*, uint8_t* status) { DEFER(st, memset(status, 0, B)); }
void launch_g2_decompress(const Tuning&, hipStream_t st, const uint8_t*, size_t B, uint8_t*, uint8_t* status) { DEFER(st, memset(status, 0, B)); }

// everything else the driven entries reach: nothing to do (status bytes are zeroed by the unit, every operand "decodes")
void launch_invalidate_jobs(hipStream_t, const uint8_t*, size_t, size_t, size_t, uint8_t*, uint8_t*, size_t, uint8_t*) {}
void launch_hash_g2(const Tuning&, hipStream_t, const uint8_t*, const uint64_t*, size_t, uint8_t*, bool) {}
void launch_hash_g1_g2(const Tuning&, hipStream_t, const uint8_t*, const uint8_t*, const uint64_t*, size_t, uint8_t*, uint8_t*, bool) {}
void launch_lincomb_g1(hipStream_t, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, bool) {}
void launch_g1_scale_cofactor_fix(hipStream_t, const uint8_t*, size_t, size_t, uint8_t*) {}
void launch_xor_with_hash(hipStream_t, const uint8_t*, const uint8_t*, const uint64_t*, size_t, uint8_t*, uint8_t*) {}
void launch_commitment_evaluate(hipStream_t, const uint8_t*, size_t, const uint64_t*, size_t, uint8_t*, uint8_t*) {}
void launch_commitment_evaluate_jobs(hipStream_t, const uint8_t*, size_t, const uint64_t*, size_t, size_t, uint8_t*, uint8_t*) {}
void launch_fixed_base_table(hipStream_t, int32_t*) {}
void launch_g1_fixed_base(hipStream_t, const int32_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, int) {}
void launch_dkg_rlc_points(hipStream_t, const uint8_t*, size_t, const uint8_t*, size_t, uint8_t*) {}
void launch_fill_g1_generator(hipStream_t, uint8_t*, uint8_t*) {}
void launch_rec_gather_keys(hipStream_t, const uint8_t*, size_t, const uint64_t*, size_t, uint8_t*) {}
void launch_select_shares(hipStream_t, const uint8_t*, const uint8_t*, size_t, size_t, size_t, const uint32_t*, uint64_t*, uint32_t*, uint8_t*, uint8_t*) {}
void launch_gather_selected(hipStream_t, const uint8_t*, size_t, size_t, size_t, const uint32_t*, const uint8_t*, size_t, uint8_t*) {}
void launch_decompress_selected(const Tuning&, hipStream_t, bool, const uint8_t*, size_t, size_t, const uint32_t*, const uint8_t*, size_t, uint8_t*, uint8_t*) {}
void launch_robust_mark(hipStream_t, const uint8_t*, const uint32_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint8_t*) {}
void launch_blame_leaves(hipStream_t, TableArena, bool, const uint8_t*, uint64_t, const uint8_t*, size_t, uint8_t*, size_t, int32_t*, int32_t*) {}
void launch_blame_range_sum(hipStream_t, bool, const int32_t*, size_t, const uint32_t*, const uint32_t*, const uint32_t*, size_t, size_t, uint8_t*) {}
void launch_lagrange(hipStream_t, const uint64_t*, size_t, size_t, size_t, uint32_t*, uint8_t*, uint32_t*, bool) {}
void launch_combine_g2(hipStream_t, TableArena, size_t, size_t, const uint64_t*, const uint8_t*, uint32_t*, size_t, uint8_t*, uint8_t*, uint32_t*, uint32_t*,
                       const uint32_t*, hipEvent_t) {}
void launch_combine_g1(hipStream_t, size_t, size_t, const uint64_t*, const uint8_t*, const uint32_t*, size_t, uint8_t*, uint8_t*, const uint32_t*, TableArena,
                       uint8_t*, uint32_t*, uint32_t*, hipEvent_t) {}

}  // namespace tc

// ---- the cases --------------------------------------------------------------------------------------------------------------
static int g_errors = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      g_errors++;                    \
      printf("FAIL %s: ", #cond);    \
      printf(__VA_ARGS__);           \
      printf("\n");                  \
    }                                \
  } while (0)

// The secret markers: every 8-byte window of each is distinct and occurs in no other input (those are all 0x11).
static uint8_t g_seed[32], g_blame_key[32];
static std::vector<uint8_t> g_vals;
static void make_markers(size_t vals) {
  for (int i = 0; i < 32; i++) g_seed[i] = (uint8_t)(0xA0 + i), g_blame_key[i] = (uint8_t)(0xC0 + i);
  g_vals.resize(vals * 32);
  for (size_t i = 0; i < g_vals.size() / 4; i++) {
    const uint8_t w[4] = {0xE5, (uint8_t)(0x80 | (i & 0x7f)), (uint8_t)(0x80 | (i >> 7)), 0x5E};  // (no zero, no 0x11: the search skips those fast)
    memcpy(&g_vals[4 * i], w, 4);
  }
  fake::watch(g_seed, 32, 8);
  fake::watch(g_blame_key, 32, 8);
  fake::watch(g_vals.data(), g_vals.size(), 8);
}
static bool secrets_on_device() { return fake::device_holds_watched(); }

// One call: operands and results live in buffers made before the allocator is armed; in the fake, host memory is as good a
// "device" pointer as any, so both I/O modes use the same ones (kept out of hipMalloc: the marker search is for what the LIBRARY holds)
struct Case {
  std::string name;
  std::function<int()> run;
  std::vector<uint8_t> out;  // every result of the call, one buffer
  uint64_t n_fallback = 0;
  bool bisect = false;
  size_t bad_key_n = 0;
};

static std::vector<uint8_t> g_in(1 << 20, 0x11);  // operand bytes nobody interprets
static std::vector<uint64_t> g_off, g_idx;        // offsets 0, 1, 2, ...; indices 0, 1, 0, 1, ...

static void add_cases(std::vector<Case>& cs, tc_ctx* ctx, size_t B) {
  const uint8_t* in = g_in.data();
  const uint64_t* off = g_off.data();
  auto add = [&](const char* name, size_t out_bytes, std::function<int(Case&)> body, bool bisect = false) {
    cs.emplace_back();
    Case* c = &cs.back();
    c->name = name;
    c->out.assign(out_bytes, 0xEE);
    c->bisect = bisect;
    c->run = [c, body] { return body(*c); };
  };
  const size_t N = 3, t = 1;
  add("verify_shares_rlc", B * N, [=](Case& c) { return tc_verify_shares_rlc_batch(ctx, in, N, in, in, off, B, g_seed, c.out.data(), &c.n_fallback); });
  add("verify_decryption_shares_rlc", B * N,
      [=](Case& c) { return tc_verify_decryption_shares_rlc_batch(ctx, in, N, in, in, in, off, in, B, g_seed, c.out.data(), &c.n_fallback); });
  const size_t GB = B == 3 ? 5 : B;  // the grouped entries: B = 5 in groups of 2, so that a tail group exists
  add("verify_g2_rlc", GB, [=](Case& c) { return tc_verify_g2_rlc_batch(ctx, in, in, in, GB, 2, g_seed, c.out.data(), &c.n_fallback); });
  add("verify_sig_rlc", GB, [=](Case& c) { return tc_verify_sig_rlc_batch(ctx, in, in, in, off, GB, 2, g_seed, c.out.data(), &c.n_fallback); });
  add("ciphertext_verify_rlc", GB, [=](Case& c) { return tc_ciphertext_verify_rlc_batch(ctx, in, in, off, in, GB, 2, g_seed, c.out.data(), &c.n_fallback); });
  // ragged: M messages with 2, 0, 1, 2, 0, 1, ... records, K = 2 keys through key_idx, groups of 2
  const size_t M = B, K = 2;
  static std::vector<std::vector<uint64_t>> rec_offs;  // (one per batch size, alive as long as the cases)
  rec_offs.emplace_back(M + 1, 0);
  std::vector<uint64_t>& rec_off = rec_offs.back();
  for (size_t m = 0; m < M; m++) rec_off[m + 1] = rec_off[m] + (m % 3 == 0 ? 2 : m % 3 == 1 ? 0 : 1);
  const size_t R = (size_t)rec_off[M];
  const uint64_t *ro = rec_off.data(), *kidx = g_idx.data();
  add("verify_g2_records_rlc", R, [=](Case& c) { return tc_verify_g2_records_rlc_batch(ctx, in, K, kidx, in, ro, in, M, 2, g_seed, c.out.data(), &c.n_fallback); });
  add("verify_sig_records_rlc", R,
      [=](Case& c) { return tc_verify_sig_records_rlc_batch(ctx, in, K, kidx, in, ro, in, off, M, 2, g_seed, c.out.data(), &c.n_fallback); });
  add("verify_dshare_records_rlc", R, [=](Case& c) {
    return tc_verify_decryption_share_records_rlc_batch(ctx, in, K, kidx, in, ro, in, in, off, in, M, 2, g_seed, c.out.data(), &c.n_fallback);
  });
  add("verify_dshare_records_prehashed_rlc", R, [=](Case& c) {
    return tc_verify_decryption_share_records_prehashed_rlc_batch(ctx, in, K, kidx, in, ro, in, in, M, 2, g_seed, c.out.data(), &c.n_fallback);
  });
  // robust: out | used | bad | status
  for (int bisect = 0; bisect < 2; bisect++) {
    const size_t so = B * 192, pl = B;  // signature bytes; plaintext bytes (off = 0, 1, 2, ...)
    add(bisect ? "combine_signatures_robust/bisect" : "combine_signatures_robust", so + 2 * B * N + B, [=](Case& c) {
      uint8_t* o = c.out.data();
      return tc_combine_signatures_robust_batch(ctx, in, t, N, in, in, in, nullptr, nullptr, B, 2, g_seed, o, o + so, o + so + B * N, o + so + 2 * B * N,
                                                &c.n_fallback);
    }, bisect);
    add(bisect ? "combine_signatures_robust_wire/bisect" : "combine_signatures_robust_wire", B * 96 + 2 * B * N + B, [=](Case& c) {
      uint8_t* o = c.out.data();
      return tc_combine_signatures_robust_wire_batch(ctx, in, t, N, in, in, in, nullptr, nullptr, B, 2, g_seed, o, o + B * 96, o + B * 96 + B * N,
                                                     o + B * 96 + 2 * B * N, &c.n_fallback);
    }, bisect);
    add(bisect ? "decrypt_robust/bisect" : "decrypt_robust", pl + 2 * B * N + B, [=](Case& c) {
      uint8_t* o = c.out.data();
      return tc_decrypt_robust_batch(ctx, in, t, N, in, in, in, in, off, in, B, o, o + pl, o + pl + B * N, o + pl + 2 * B * N, &c.n_fallback);
    }, bisect);
    add(bisect ? "decrypt_robust_wire/bisect" : "decrypt_robust_wire", pl + 2 * B * N + B, [=](Case& c) {
      uint8_t* o = c.out.data();
      return tc_decrypt_robust_wire_batch(ctx, in, t, N, in, in, in, in, off, in, B, o, o + pl, o + pl + B * N, o + pl + 2 * B * N, &c.n_fallback);
    }, bisect);
  }
  const size_t n = 2, degree = 1;
  add("dkg_verify_values_rlc", B * n,
      [=](Case& c) { return tc_dkg_verify_values_rlc_batch(ctx, in, degree, g_idx.data(), g_vals.data(), n, B, g_seed, c.out.data(), &c.n_fallback); });
}

// the two entries WITHOUT a host decision, for the allocation counts only
static void add_plain_cases(std::vector<Case>& cs, tc_ctx* ctx, size_t B) {
  const uint8_t* in = g_in.data();
  auto add = [&](const char* name, size_t out_bytes, std::function<int(Case&)> body) {
    cs.emplace_back();
    Case* c = &cs.back();
    c->name = name;
    c->out.assign(out_bytes, 0xEE);
    c->run = [c, body] { return body(*c); };
  };
  add("verify_g2 (no host decision)", B, [=](Case& c) { return tc_verify_g2_batch(ctx, in, 0, in, in, B, c.out.data()); });
  add("combine_g2 (no host decision)", B * 192 + B, [=](Case& c) { return tc_combine_g2_batch(ctx, 1, 3, g_idx.data(), in, B, c.out.data(), c.out.data() + B * 192); });
}

struct Result {
  int rc;
  long allocs;
  bool injected;
};
// one call of the case under the switches of the run; fail_at < 0: uninjected.  The stream is drained afterwards (a device-I/O
// call may return with its work queued: here is where a copy against freed memory would run) and the device searched.
static Result run_case(tc_ctx* ctx, Case& c, bool device_io, bool fail_last, long fail_at) {
  tc_ctx_set_device_io(ctx, device_io);
  tc_ctx_set_blame_bisect(ctx, c.bisect ? g_blame_key : nullptr);
  g_fail_last = fail_last;
  g_bad_key_n = c.bad_key_n;
  memset(c.out.data(), 0xEE, c.out.size());
  c.n_fallback = 77;
  fake::arm(fail_at);
  const int rc = c.run();
  Result r{rc, fake::disarm(), fake::injected()};
  EXPECT(tc_sync(ctx) == TC_OK && fake::pending() == 0, "%s: work left queued", c.name.c_str());
  EXPECT(!secrets_on_device(), "%s: secret bytes on the device after rc = %d (io %d, fail %d, allocation %ld)", c.name.c_str(), rc, device_io, fail_last,
         fail_at);
  return r;
}

// Fails allocation k of the call for k = 0, 1, 2, ... until the call gets through: every injected run answers TC_ERR_HOST with a
// message, leaves no secret behind and a context that answers the next call like a fresh one; the run that gets through answers
// what the uninjected run answered.
static void sweep(tc_ctx* ctx, Case& c, bool device_io, bool fail_last) {
  const Result base = run_case(ctx, c, device_io, fail_last, -1);
  EXPECT(base.rc == TC_OK, "%s: uninjected rc = %d (%s)", c.name.c_str(), base.rc, tc_last_error(ctx));
  const std::vector<uint8_t> want = c.out;
  const uint64_t want_fb = c.n_fallback;
  EXPECT((fail_last || c.bad_key_n) ? want_fb > 0 : want_fb == 0, "%s: n_fallback = %llu with fail_last = %d", c.name.c_str(),
         (unsigned long long)want_fb, fail_last);
  long k = 0;
  for (; k < 10000; k++) {
    const Result r = run_case(ctx, c, device_io, fail_last, k);
    if (!r.injected) {
      EXPECT(r.rc == TC_OK && c.out == want && c.n_fallback == want_fb, "%s: the run behind the sweep differs (rc = %d)", c.name.c_str(), r.rc);
      break;
    }
    EXPECT(r.rc == TC_ERR_HOST, "%s: allocation %ld failed, rc = %d", c.name.c_str(), k, r.rc);
    EXPECT(tc_last_error(ctx)[0] != 0, "%s: no message after allocation %ld failed", c.name.c_str(), k);
    const Result again = run_case(ctx, c, device_io, fail_last, -1);
    EXPECT(again.rc == TC_OK && c.out == want && c.n_fallback == want_fb, "%s: the call after allocation %ld failed differs (rc = %d)", c.name.c_str(), k,
           again.rc);
    if (g_errors > 20) return;
  }
  EXPECT(k < 10000, "%s: the sweep did not end", c.name.c_str());
  printf("  %-44s io %d fail %d: %ld allocations swept, n_fallback %llu\n", c.name.c_str(), device_io, fail_last, k, (unsigned long long)want_fb);
}

int main(int argc, char** argv) {
  const bool counts = argc > 1 && !strcmp(argv[1], "--counts");
  tc_ctx* ctx = nullptr;
  if (tc_ctx_create(&ctx, 0) != TC_OK) {
    printf("tc_ctx_create failed\n");
    return 1;
  }
  make_markers(50 * 2);
  g_off.resize(4096);
  g_idx.resize(4096);
  for (size_t i = 0; i < 4096; i++) g_off[i] = i, g_idx[i] = i % 2;
  std::vector<Case> small, large, plain;
  small.reserve(64), large.reserve(64), plain.reserve(8);
  add_cases(small, ctx, 3);
  if (counts) {
    // host allocations of one uninjected call (the second of its kind: the staging slots exist), at the small shapes and at B = 50
    add_cases(large, ctx, 50);
    add_plain_cases(plain, ctx, 3);
    for (auto& c : plain) {
      run_case(ctx, c, false, false, -1);
      printf("allocs %-44s host %ld\n", c.name.c_str(), run_case(ctx, c, false, false, -1).allocs);
    }
    for (size_t i = 0; i < small.size(); i++)
      for (int fail = 0; fail < 2; fail++) {
        run_case(ctx, small[i], false, fail, -1);
        const long a3 = run_case(ctx, small[i], false, fail, -1).allocs;
        run_case(ctx, large[i], false, fail, -1);
        const long a50 = run_case(ctx, large[i], false, fail, -1).allocs;
        printf("allocs %-44s fail %d: small %ld  B=50 %ld\n", small[i].name.c_str(), fail, a3, a50);
      }
  } else {
    for (auto& c : small)
      for (int io = 0; io < 2; io++)
        for (int fail = 0; fail < 2; fail++) sweep(ctx, c, io, fail);
    // device I/O with a bad key-table entry in checked-input mode: key_idx is read back in mid-call (Records::host_key_idx)
    for (auto& c : small)
      if (c.name.find("records") != std::string::npos) {
        c.bad_key_n = 2;
        sweep(ctx, c, true, false);
        c.bad_key_n = 0;
      }
  }
  tc_ctx_destroy(ctx);
  if (g_errors) {
    printf("call_host: %d error(s)\n", g_errors);
    return 1;
  }
  printf("call_host: ok\n");
  return 0;
}
