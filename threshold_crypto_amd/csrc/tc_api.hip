// C ABI of libtc_amd.so (declared in include/tc_amd.h): context, device staging and the
// batch entry points.  Host code only; every computation is a gfx950 kernel launch (see
// tc_launch.h).  There is no CPU compute path: without a HIP device tc_ctx_create fails.
#include "tc_launch.h"
#include "tc_robust.h"
#include "tc_blame.h"
#include "tc_records.h"
#include "tc_fallback.h"
#include "../../include/tc_amd.h"

#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

struct Slot {
  void* p = nullptr;
  size_t cap = 0;
};

}  // namespace

struct tc_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  bool device_io = false;
  bool timing = false;
  // validate uncompressed point operands (order-r subgroup) before using them: ON unless the caller opts out
  // (tc_ctx_set_input_checks(ctx, 0)) for operands it knows to be group members -- outputs of this library, values that
  // passed the checked decode
  bool input_checks = true;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // the membership tests of checked-input mode run on a SECOND stream beside the call's main kernels (Call::run_checks): a
  // LOW-priority stream, created by the first call that needs it -- a context whose caller opted out of the tests never has
  // one (HIP multiplexes its streams onto a few hardware queues: a stream nobody uses must not take a queue from the main
  // streams of several contexts that run side by side, bench.py `streaming`) -- and the two ordering events
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  double last_ms = 0.0;
  std::string err;
  std::vector<Slot> slots;  // grow-only device staging buffers, reused across calls
  size_t next_slot = 0;
  uint8_t* g1_gen = nullptr;  // 96 B uncompressed G1 generator on the device
  // [3 (x^2 - 1)] g1: the generator side of a pairing check whose other side holds a hash point without
  // its last constant multiplication (tc_gls.h g2_clear_cofactor): e(pk, [c] Q') == e(g1, sig)  <=>
  // e(pk, Q') == e([1/c] g1, sig)
  uint8_t* g1_gen_unfix = nullptr;
  int32_t* fb_table = nullptr;  // signed 4-bit window table of the G1 generator (tc_dkg.h), built on first use
  // per-job ladder tables of the G2 kernels (tc_table.h): 256 MB + one flag word per wave slot, allocated on first use
  int32_t* tbl_mem = nullptr;
  uint32_t* tbl_flags = nullptr;
  bool tbl_reset = false;  // a call failed: a kernel may have died holding slots, clear the flags before the next use
  int cus = 0;
  tc::Tuning tuning;  // form choices, fixed when the context is created (tc_launch.h)
  uint64_t h2d_bytes = 0, d2h_bytes = 0;  // bytes this context's staging copies moved over PCIe (tc_ctx_transfer_bytes)
  // pass 2 of the robust combiners by bisection (tc_ctx_set_blame_bisect; tc_blame.h): the secret key the pass-2 scalars of
  // every call derive from, the number of the next call under it, and what pass 2 of the last robust call spent
  bool blame_bisect = false;
  uint8_t blame_key[32] = {};
  uint64_t blame_calls = 0;
  uint64_t blame_checks = 0, blame_rounds = 0;
};

namespace {

struct Call {
  tc_ctx* c;
  bool failed = false;
  bool arg_error = false;
  struct CopyBack {
    void* host;
    const void* dev;
    size_t n;
  };
  std::vector<CopyBack> outs;
  struct Pending {
    const uint8_t* valid;
    size_t per_job, group;
    // the membership-test launch that will fill `valid` (pts == nullptr: already filled, e.g. by a checked decode)
    bool g2 = false;
    const uint8_t* pts = nullptr;
    size_t stride = 0, n_per_job = 0, take = 0, n = 0;
    size_t bytes = 0;  // extent of the operand the deferred test reads (records * n_per_job * stride)
  };
  std::vector<Pending> checks;  // checked-input mode: validity bytes waiting to be applied to the jobs
  // device-io mode: the caller's output buffers.  A deferred membership test reads its operand WHILE the main kernels write
  // their results, so an operand that overlaps an output (an in-place call) keeps the order of a one-stream context: test first.
  std::vector<std::pair<const uint8_t*, size_t>> out_ranges;
  static bool ranges_overlap(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
  }
  bool overlaps_output(const uint8_t* p, size_t n) const {
    for (auto& r : out_ranges)
      if (ranges_overlap(p, n, r.first, r.second)) return true;
    return false;
  }

  explicit Call(tc_ctx* ctx) : c(ctx) {
    c->next_slot = 0;
    c->err.clear();
    if (hipSetDevice(c->device) != hipSuccess) fail("hipSetDevice failed");
    // hipGetLastError() is how finish() learns of a failed kernel LAUNCH, and the runtime keeps the last error of this host thread
    // until somebody reads it: a hipMalloc that failed in an EARLIER call (HBM full) would otherwise be reported, as "kernel
    // launch: out of memory", by the first call that runs after the memory came back
    // (tests/test_gpu_tables.py::test_failed_device_allocation_is_an_error_and_the_context_survives).  A call starts clean.
    (void)hipGetLastError();
  }
  Call(const Call&) = delete;
  Call& operator=(const Call&) = delete;
  // A call that ends without finish() -- a TC_REQUIRE behind the frame, or an exception on its way to on_exception -- ends HERE,
  // while everything its copies touch is still alive: both streams are drained (a deferred test may not have been joined), the
  // secrets zeroed like finish() zeroes them, the stream drained again.  Nothing here allocates or throws.
  ~Call() {
    if (ended) return;
    failed = true;
    c->tbl_reset = true;
    (void)hipStreamSynchronize(c->stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    close(/*copy_back=*/false, /*drain=*/true);
  }
  void fail(const std::string& m) {
    if (!failed) c->err = m;
    failed = true;
  }
  bool check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
      fail(std::string(what) + ": " + hipGetErrorString(e));
      return false;
    }
    return true;
  }
  // the table arena of the G2 ladder kernels (tc_table.h)
  tc::TableArena tables() {
    // (either half may be missing: an earlier call can have failed between the two allocations -- HBM full -- and a launcher
    // handed an arena without flags returns without doing anything)
    if ((!c->tbl_mem || !c->tbl_flags) && !failed) {
      if (!c->tbl_mem && !check(hipMalloc((void**)&c->tbl_mem, tc::kTableArenaWords * sizeof(int32_t)), "hipMalloc")) c->tbl_mem = nullptr;
      if (!failed && !c->tbl_flags) {
        if (check(hipMalloc((void**)&c->tbl_flags, tc::kTableArenaFlags * sizeof(uint32_t)), "hipMalloc"))
          check(hipMemsetAsync(c->tbl_flags, 0, tc::kTableArenaFlags * sizeof(uint32_t), c->stream), "memset");
        else
          c->tbl_flags = nullptr;
      }
    }
    if (c->tbl_flags && c->tbl_reset && !failed) {
      // stream-ordered after whatever ran before; nothing of this context is in flight beyond the stream
      if (check(hipMemsetAsync(c->tbl_flags, 0, tc::kTableArenaFlags * sizeof(uint32_t), c->stream), "memset")) c->tbl_reset = false;
    }
    return tc::TableArena{c->tbl_mem, c->tbl_flags};
  }
  void* scratch(size_t n) {
    if (n == 0) n = 8;
    if (c->next_slot >= c->slots.size()) c->slots.emplace_back();
    Slot& s = c->slots[c->next_slot++];
    if (s.cap < n) {
      if (s.p) (void)hipFree(s.p);
      s.p = nullptr;
      s.cap = 0;
      size_t cap = n + n / 4 + 256;
      if (!check(hipMalloc(&s.p, cap), "hipMalloc")) {
        s.p = nullptr;  // (whatever the failed call left in the slot is not a pointer to free later)
        return nullptr;
      }
      s.cap = cap;
    }
    return s.p;
  }
  // input operand: device pointer usable by kernels
  template <class T>
  const T* in(const T* p, size_t count, bool secret = false) {
    if (p) operand_bytes += count * sizeof(T);
    if (c->device_io || p == nullptr) return p;
    size_t n = count * sizeof(T);
    void* d = scratch(n);
    if (!d) return nullptr;
    if (secret) this->secret(d, n);  // (listed BEFORE the bytes arrive: a list that cannot grow ends the call with nothing to zero)
    if (n && !upload(d, p, n, "H2D copy")) return nullptr;
    return (const T*)d;
  }
  // output operand: device pointer the kernels write; copied back in finish()
  template <class T>
  T* out(T* p, size_t count, bool zero = false) {
    if (p == nullptr) return nullptr;
    size_t n = count * sizeof(T);
    operand_bytes += n;
    T* d = p;
    if (!c->device_io) {
      d = (T*)scratch(n);
      if (!d) return nullptr;
      outs.push_back({p, d, n});
    } else if (n) {
      out_ranges.emplace_back((const uint8_t*)d, n);
      // (an operand registered before this output and deferred already: test it now, on the main stream, before anything writes)
      for (auto& pc : checks)
        if (pc.pts && ranges_overlap(pc.pts, pc.bytes, (const uint8_t*)d, n)) launch_pending(pc, c->stream);
    }
    if (zero && n) check(hipMemsetAsync(d, 0, n, c->stream), "memset");
    return d;
  }
  template <class T>
  T* temp(size_t count, bool zero = false) {
    size_t n = count * sizeof(T);
    T* d = (T*)scratch(n);
    if (d && zero && n) check(hipMemsetAsync(d, 0, n, c->stream), "memset");
    return d;
  }
  // the staging copies of a call, on its stream: the ONLY places that count the bytes moved over PCIe (tc_ctx_transfer_bytes)
  bool upload(void* dst, const void* host_src, size_t bytes, const char* what) {
    if (!check(hipMemcpyAsync(dst, host_src, bytes, hipMemcpyHostToDevice, c->stream), what)) return false;
    c->h2d_bytes += bytes;
    return true;
  }
  bool readback(void* host_dst, const void* dev_src, size_t bytes, const char* what) {
    if (!check(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream), what)) return false;
    c->d2h_bytes += bytes;
    return true;
  }
  // HOST memory of the call.  Every host byte that an asynchronous copy of the call touches after the operands are staged -- verdict
  // and status bytes read back, job maps and descriptors uploaded -- belongs to the frame and lives until the call has ended,
  // however it ends: never a local of an entry, which an exception would free under the copy.  (The caller's operands and
  // results are the caller's; total_bytes and the one word of combine() read into a stack slot and wait at once.)
  template <class T>
  T* host(size_t count) {  // zero-initialised
    host_bufs.emplace_back((count * sizeof(T) + 7) / 8);
    return reinterpret_cast<T*>(host_bufs.back().data());
  }
  // `count` values of device memory, on the host after the next wait(): in a buffer of their own, or (fetch_into) in host()
  // memory the caller reuses from round to round
  template <class T>
  const T* fetch(const T* dev, size_t count, const char* what) {
    T* h = host<T>(count);
    fetch_into(h, dev, count, what);
    return h;
  }
  template <class T>
  void fetch_into(T* owned, const T* dev, size_t count, const char* what) {
    if (readback(owned, dev, count * sizeof(T), what)) host_in_flight = true;
  }
  // a map the host has built (tc_fallback.h returns them by value), handed to the frame; its entries stay where they are
  const uint32_t* keep(std::vector<uint32_t>&& v) {
    host_maps.push_back(std::move(v));
    return host_maps.back().data();
  }
  // upload() out of host() / keep() memory
  bool upload_owned(void* dst, const void* owned_src, size_t bytes, const char* what) {
    if (!upload(dst, owned_src, bytes, what)) return false;
    host_in_flight = true;
    return true;
  }
  // the main stream drained: what fetch() asked for is there.  false: the call has failed (now or earlier)
  bool wait() {
    const hipError_t e = hipStreamSynchronize(c->stream);
    host_in_flight = false;
    if (!failed) check(e, "stream sync");
    return !failed;
  }
  // the staging slots taken while a SlotScope lives are handed out again behind it -- the buffers of one round are the next
  // round's.  The round ends with wait(); on unwinding the frame drains the stream before anybody takes a slot again.
  struct SlotScope {
    tc_ctx* c;
    size_t mark;
    explicit SlotScope(Call& k) : c(k.c), mark(k.c->next_slot) {}
    ~SlotScope() { c->next_slot = mark; }
    SlotScope(const SlotScope&) = delete;
    SlotScope& operator=(const SlotScope&) = delete;
  };
  // device bytes that hold a secret (scalars, a lossless recoding of them): zeroed when the call ends.  after_copy: a secret
  // RESULT staged for the host, zeroed behind its D2H copy.  List the bytes before anything writes them.
  void secret(void* d, size_t bytes, bool after_copy = false) {
    if (d) (after_copy ? wipe_after_copy : wipe).emplace_back(d, bytes);
  }
  template <class T>
  T* secret_temp(size_t count) {
    T* d = temp<T>(count);
    secret(d, count * sizeof(T));
    return d;
  }
  // the seed of a combined entry on the device: host memory in both I/O modes (32 bytes; secret until the call returns)
  uint8_t* secret_seed(const uint8_t* seed32) {
    uint8_t* d = secret_temp<uint8_t>(32);
    if (d) upload(d, seed32, 32, "seed copy");
    return d;
  }
  // members only: ok[j] &= (row j of pts is a point of the order-r subgroup) for R rows of `stride` bytes -- stride 0: ONE point,
  // shared by every row.  v: R bytes of scratch.
  void require_members(bool g2, const uint8_t* pts, size_t stride, size_t R, uint8_t* v, uint8_t* ok) {
    const size_t n = stride ? R : 1;
    if (g2) tc::launch_subgroup_check_g2(c->stream, pts, stride, 1, 1, n, v);
    else tc::launch_subgroup_check_g1(c->stream, pts, stride, 1, 1, n, v);
    tc::launch_invalidate_jobs(c->stream, v, 1, stride ? 1 : (size_t)-1, R, nullptr, nullptr, 0, ok);
  }
  // the Miller values between the two kernels of a pairing check (k_pairing.hip)
  // (+ the line buffer of the prepared form, one tile of checks sized to the memory this call may spend: msm_table_budget)
  tc::PairingWs pairing_ws(size_t B);
  // the Miller values and the partial products of an n-pair product check (k_pairing.hip launch_pairing_product_check)
  int32_t* pairing_product_ws(size_t n, size_t B, bool rhs) { return temp<int32_t>(tc::pairing_product_ws_words(n, B, rhs)); }
  // Checked-input mode (tc_ctx_set_input_checks): validate the first `take` points of `records` records of
  // n_per_job points each (stride 0 = ONE point shared by every job); job j owns record j / group.
  // always: the test runs whatever the context's switch says (entries that multiply a SECRET by the operand)
  // Returns the handle of the verdict bytes (Call::take_verdicts), nullptr when nothing was registered.
  const uint8_t* check_points(bool g2, const uint8_t* d_pts, size_t stride, size_t n_per_job, size_t take, size_t records, size_t group,
                              bool always = false) {
    if (!(c->input_checks || always) || failed || !d_pts || !records || !take) return nullptr;
    const size_t PB = g2 ? 192 : 96;
    if (stride == 0) {
      stride = PB;
      records = 1;
      n_per_job = take = 1;
      group = (size_t)-1;
    }
    const size_t n = records * take;
    const size_t bytes = records * n_per_job * stride;
    uint8_t* v = temp<uint8_t>(n);
    if (!v) return nullptr;
    // The tests are NOT launched here.  They read operands only and nothing reads their verdict before apply_checks, so they
    // run on the context's second stream BESIDE the main kernels of the call, submitted after them (apply_checks): a launch
    // that ends with idle SIMDs -- the 65 536-job combination's last third, DESIGN.md 5.2 -- gets its tail filled (default-mode
    // combine_signatures 10.2 -> 9.3 ms per call, profiles/r06_checks_beside_ab.txt), and a small batch runs both at once.
    // ev_fork marks where the operands are ready in the main stream (every check_points call precedes the main kernels).
    const bool beside = c->tuning.checks_beside && !overlaps_output(d_pts, bytes) && side_stream_ready();
    if (beside && !check(hipEventRecord(c->ev_fork, c->stream), "event record")) return nullptr;
    checks.push_back({v, take, group, g2, d_pts, stride, n_per_job, take, n, bytes});
    if (!beside) launch_pending(checks.back(), c->stream);
    return v;
  }
  // the context's second stream, made on first use: non-blocking and of the LOWEST priority the device offers, so that its
  // kernels take the wave slots the main kernels leave idle instead of competing with them for the dispatcher, and so that it
  // draws its hardware queue from another pool than the normal-priority streams
  bool side_stream_ready() {
    if (c->side_stream) return true;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    if (hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, c->tuning.checks_beside == 2 ? 0 : least) != hipSuccess) {
      c->side_stream = nullptr;
      (void)hipGetLastError();
      return false;  // no second stream: the tests run before the main kernels, on the one stream (correct, just not overlapped)
    }
    return true;
  }
  // the event a launcher may re-record just before the call's one long kernel (k_combine.hip launch_combine_g2): the deferred
  // tests then start behind that kernel instead of beside the small kernels in front of it; nullptr when nothing is deferred
  hipEvent_t fork_event() const {
    for (auto& p : checks)
      if (p.pts) return c->ev_fork;
    return nullptr;
  }
  void launch_pending(Pending& p, hipStream_t st) {
    if (!p.pts) return;
    if (p.g2) tc::launch_subgroup_check_g2(st, p.pts, p.stride, p.n_per_job, p.take, p.n, const_cast<uint8_t*>(p.valid));
    else tc::launch_subgroup_check_g1(st, p.pts, p.stride, p.n_per_job, p.take, p.n, const_cast<uint8_t*>(p.valid));
    p.pts = nullptr;  // launched
  }
  // the tests check_points deferred: submitted now (after the call's main kernels) on the second stream, their verdicts
  // ordered before whatever the main stream does next.  Every reader of Pending::valid goes through here first.
  void run_checks() {
    if (failed) return;
    bool beside = false;
    for (auto& p : checks) beside = beside || p.pts != nullptr;
    if (!beside) return;
    // second stream: wait for the operands, run the tests, hand the verdicts back to the main stream
    if (!check(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0), "stream wait")) return;
    for (auto& p : checks) launch_pending(p, c->side_stream);
    if (check(hipEventRecord(c->ev_join, c->side_stream), "event record")) check(hipStreamWaitEvent(c->stream, c->ev_join, 0), "stream wait");
  }
  // after the main kernels: jobs that own an invalid point fail like undecodable ones
  void apply_checks(size_t B, uint8_t* status, uint8_t* out, size_t out_bytes, uint8_t* ok) {
    run_checks();
    if (!failed)
      for (auto& p : checks) tc::launch_invalidate_jobs(c->stream, p.valid, p.per_job, p.group, B, status, out, out_bytes, ok);
    checks.clear();
  }
  // For the entries whose HOST decides what falls back: the deferred tests run, and the verdict bytes behind each handle
  // (check_points' return value) are read back, as many as were registered, into memory of the frame (fetch): the host pointer
  // of each, null for a null handle -- nothing registered, no evidence.  The pending list ends empty; with nothing pending and
  // no handle this does nothing.
  void take_verdicts(std::initializer_list<std::pair<const uint8_t*, const uint8_t**>> want) {
    run_checks();
    for (auto& w : want) {
      *w.second = nullptr;
      for (auto& p : checks)
        if (w.first && p.valid == w.first) *w.second = fetch(p.valid, p.n, "valid readback");
    }
    checks.clear();
  }
  // Every entry calls begin_timing() after its allocations and before its first launch: the place to refuse a call the RUNTIME
  // could not survive.  The kernels' private segments (spilled registers, ladder tables: up to 11 KB per lane) are allocated by
  // the ROCm runtime when a dispatch needs them, per queue, for as many waves as the dispatch has (at most 32 per CU); when that
  // allocation fails the runtime's queue-error callback calls abort() -- the process dies on a runtime thread, no error code
  // reaches anybody (reproduced with ~0.4 GB of HBM free: DESIGN.md 7).  So a call whose size could ask for more than is free is
  // turned away HERE, as TC_ERR_HIP.  The bound is generous (operand bytes / 48 lanes, every lane at the largest private
  // segment of the library): it only ever bites with the HBM nearly full.
  size_t operand_bytes = 0;
  void guard_private() {
    if (failed || c->tuning.private_reserve == 0) return;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    size_t need = c->tuning.private_reserve;
    if (need == (size_t)-1) {
      const size_t device_waves = (size_t)(c->cus > 0 ? c->cus : 256) * 32;
      size_t waves = operand_bytes / 48 / 64 + 1;  // (no entry moves fewer than 97 operand bytes per job, no kernel runs more than two lanes per 97 bytes)
      if (waves > device_waves) waves = device_waves;
      need = waves * 64 * tc::kMaxPrivateBytesPerLane + ((size_t)64 << 20);
    }
    if (free_b < need)
      fail("out of memory: " + std::to_string(free_b >> 20) + " MB of HBM free, the kernels' private segments may need " + std::to_string(need >> 20) +
           " MB (the ROCm runtime aborts the process when it cannot allocate them; TC_PRIVATE_RESERVE overrides)");
  }
  void begin_timing() {
    guard_private();
    if (c->timing && !failed) check(hipEventRecord(c->ev0, c->stream), "event record");
  }
  void end_timing() {
    if (c->timing && !failed) check(hipEventRecord(c->ev1, c->stream), "event record");
  }
  int finish() {
    if (!failed) check(hipGetLastError(), "kernel launch");
    close(/*copy_back=*/!failed, /*drain=*/!c->device_io || c->timing);
    if (c->timing && !failed) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_ms = ms;
    }
    return failed ? (arg_error ? TC_ERR_INVALID_ARG : TC_ERR_HIP) : TC_OK;
  }

 private:
  std::vector<std::vector<uint64_t>> host_bufs;  // host(): 8-byte units, zeroed
  std::vector<std::vector<uint32_t>> host_maps;  // keep()
  // a copy that fetch() / upload_owned() queued may still be running: set by them, cleared by every synchronise of the main stream
  bool host_in_flight = false;
  bool ended = false;
  std::vector<std::pair<void*, size_t>> wipe;             // secret()
  std::vector<std::pair<void*, size_t>> wipe_after_copy;  // secret(.., after_copy)
  // The ONE ending of a call, behind finish() and behind the destructor: the secrets zeroed, the results copied back (a call that
  // is still good), the staged secret results zeroed behind their copies, and the stream drained -- always for a failed call and
  // for one with a copy running against the frame's host memory (a device-I/O call otherwise returns without waiting).  Without
  // copy_back, or once `failed` is set, nothing here allocates.
  void close(bool copy_back, bool drain) {
    for (auto& w : wipe) (void)hipMemsetAsync(w.first, 0, w.second, c->stream);
    if (copy_back)
      for (auto& o : outs)
        if (o.n) readback(o.host, o.dev, o.n, "D2H copy");
    for (auto& w : wipe_after_copy) (void)hipMemsetAsync(w.first, 0, w.second, c->stream);  // stream-ordered after the copies
    if (drain || failed || host_in_flight) wait();
    if (failed && !arg_error) c->tbl_reset = true;
    if (failed) (void)hipGetLastError();  // this call's own failure has been reported through `err`: do not leave it for the caller's next HIP check
    ended = true;
  }
};

// total message bytes = off[B]; in device-io mode read it back (8 bytes)
bool total_bytes(Call& k, const uint64_t* off, size_t B, uint64_t* total) {
  if (!k.c->device_io) {
    // host offsets are validated here (O(B)); in device-io mode the caller guarantees off[0] = 0 and a
    // non-decreasing array (the kernels read msgs + off[j] .. off[j+1] as they are)
    bool good = off[0] == 0;
    for (size_t j = 0; j < B && good; j++) good = off[j + 1] >= off[j];
    if (!good) {
      k.fail("invalid argument: offsets must start at 0 and be non-decreasing");
      k.arg_error = true;
      return false;
    }
    *total = off[B];
    return true;
  }
  // (eight bytes into the caller's stack slot, not into memory of the frame: the wait is the very next statement, nothing between
  // the copy and it can throw or return)
  if (!k.readback(total, off + B, 8, "offset readback")) return false;
  return k.wait();
}

// sum_i scalars[j][i] * points[j][i] in G2 for n >= kMsmMinPoints through the two-stage kernels (k_msm.hip);
// d_st must hold B zeroed-or-flagged status bytes.  The per-share tables live in HBM (2 KB per share): batches
// whose tables would exceed kMsmTableBudget run as consecutive tiles of jobs through ONE table buffer (the stream
// orders a tile's ladder before the next tile's table stage).
constexpr size_t kMsmTableBudget = (size_t)24 << 30;
// What a call may spend on table buffers: a third of the HBM that is free right now (plus whatever the context's staging
// slots already hold), at most 24 GiB, at least 1 GiB -- several contexts on one GPU, or a smaller card, tile their batches
// finer instead of failing an allocation.  tc_ctx_trim() gives the slots back.
size_t msm_table_budget(Call& k) {
  if (k.c->tuning.msm_budget) return k.c->tuning.msm_budget;  // (TC_MSM_BUDGET at context creation: the tile loops under test)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (size_t)1 << 30;
  size_t held = 0;
  for (auto& s : k.c->slots) held += s.cap;
  size_t b = (free_b + held) / 3;
  if (b > kMsmTableBudget) b = kMsmTableBudget;
  if (b < ((size_t)1 << 30)) b = (size_t)1 << 30;
  return b;
}
// What the line buffer of the prepared pairing form may take: a third of the HBM that is free right now (plus the context's own
// staging slots), at most 24 GiB -- and NO floor (the smallest tile's buffer is 1.013 GB, just under msm_table_budget's
// 1 GiB floor, so with the floor a card with less than that free still tried the allocation and failed; without it pairing_tile
// answers 0 and the one-loop form, which needs no line buffer, runs).
size_t pairing_line_budget(Call& k) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
  size_t held = 0;
  for (auto& s : k.c->slots) held += s.cap;
  const size_t b = (free_b + held) / 3;
  return b > kMsmTableBudget ? kMsmTableBudget : b;
}
tc::PairingWs Call::pairing_ws(size_t B) {
  const tc::Tuning& tn = c->tuning;
  const int form = tc::pairing_form(B, tn);
  // (the budget -- hipMemGetInfo and a walk over the slots -- is only looked up by the form that has a line buffer: small
  // batches, which run the four-lane form, pay nothing for it)
  const size_t tile = tc::pairing_form_needs_lines(form) ? tc::pairing_tile(B, tn.pairing_budget ? tn.pairing_budget : pairing_line_budget(*this)) : 0;
  return tc::PairingWs{temp<int32_t>(tc::pairing_ws_words(B, tile)), tile, form};
}
void msm_g2(Call& k, size_t n, size_t pts_stride, const uint8_t* d_pts, const uint32_t* d_scalars, size_t B, uint8_t* d_out,
            uint8_t* d_st, int nbits = 64, tc::MsmFilter filter = tc::MsmFilter(), bool secret_scalars = false) {
  const size_t per_job = tc::msm_table_bytes(n, 1);
  size_t tile = msm_table_budget(k) / (per_job ? per_job : 1);
  if (tile < 1) tile = 1;
  if (tile > B) tile = B;
  int32_t* d_tbl = k.temp<int32_t>(tc::msm_table_bytes(n, tile) / sizeof(int32_t));
  uint8_t* d_codes = k.temp<uint8_t>(tc::msm_code_bytes(n, tile));
  // the digit codes are a lossless recoding of the scalars: wiped like them when they are secret
  if (secret_scalars) k.secret(d_codes, tc::msm_code_bytes(n, tile));
  for (size_t lo = 0; lo < B && !k.failed; lo += tile) {
    const size_t cnt = (B - lo < tile) ? B - lo : tile;
    tc::MsmFilter f = filter;
    if (f.idx) f.idx += lo * f.n_per_job;
    tc::launch_msm_g2(k.c->stream, n, pts_stride, d_pts + lo * pts_stride, d_scalars + lo * n * 8, cnt, d_tbl, d_codes, d_out + lo * 192,
                      d_st + lo, nbits, f);
  }
}

// the same in G1 (k_msm.hip launch_msm_g1).  pts_stride 0 with short scalars: ONE table set for the whole call.
void msm_g1(Call& k, size_t n, size_t pts_stride, const uint8_t* d_pts, const uint32_t* d_scalars, size_t B, uint8_t* d_out, uint8_t* d_st,
            int nbits = 128, bool secret_scalars = false) {
  const bool shared = tc::msm_table_jobs_g1(pts_stride, nbits, B) == 1;
  const size_t per_job = shared ? tc::msm_code_bytes(n, 1) : tc::msm_table_bytes_g1(n, 1);
  size_t tile = msm_table_budget(k) / (per_job ? per_job : 1);
  if (tile < 1) tile = 1;
  if (tile > B) tile = B;
  int32_t* d_tbl = k.temp<int32_t>(tc::msm_table_bytes_g1(n, shared ? 1 : tile) / sizeof(int32_t));
  uint8_t* d_codes = k.temp<uint8_t>(tc::msm_code_bytes(n, tile));
  // the digit codes are a lossless recoding of the scalars: wiped like them when they are secret
  if (secret_scalars) k.secret(d_codes, tc::msm_code_bytes(n, tile));
  for (size_t lo = 0; lo < B && !k.failed; lo += tile) {
    const size_t cnt = (B - lo < tile) ? B - lo : tile;
    tc::launch_msm_g1(k.c->stream, n, pts_stride, d_pts + lo * pts_stride, d_scalars + lo * n * 8, cnt, d_tbl, d_codes, d_out + lo * 96, d_st + lo,
                      nbits);
  }
}

// The compacted operands of a fallback (the combined entries re-check what their one check per group rejected, item by item):
// row r of a gathered operand is row map[r] of the call's array, through one to four index maps the host has built; one verdict
// byte per row in c_ok, scattered through one of the maps into the call's ok[] at the end.  Which operands are gathered, which
// pairing equation runs over them and which of them are tested for membership is the entry's business, at its call site.
struct Compacted {
  Call& k;
  size_t R;  // rows of c_ok
  size_t maps = 0, first[5] = {0};     // map i = d_maps[first[i] .. first[i + 1])
  const uint32_t* h_map[4] = {nullptr};  // ... and where it lies on the host, in memory of the frame
  uint32_t* d_maps;
  uint8_t* c_ok;
  uint8_t* c_v = nullptr;
  // one to four maps, each HANDED OVER (std::move at the call site) to the frame, which holds it until its copy has run
  // (Call::keep); host_map() is where to read one again
  template <class... Maps>
  Compacted(Call& call, size_t rows, Maps&&... handed) : k(call), R(rows) {
    static_assert(sizeof...(Maps) >= 1 && sizeof...(Maps) <= 4 && (std::is_same<Maps, std::vector<uint32_t>>::value && ...),
                  "std::move every map into Compacted");
    (take(std::move(handed)), ...);
    d_maps = k.temp<uint32_t>(first[maps]);
    c_ok = k.temp<uint8_t>(R);
    for (size_t i = 0; i < maps && !k.failed; i++) k.upload_owned(d_maps + first[i], h_map[i], (first[i + 1] - first[i]) * 4, "map copy");
  }
  void take(std::vector<uint32_t>&& m) {
    first[maps + 1] = first[maps] + m.size();
    h_map[maps++] = k.keep(std::move(m));
  }
  const uint32_t* host_map(size_t which) const { return h_map[which]; }
  const uint32_t* map(size_t which) const { return d_maps + first[which]; }
  // the rows of src (stride bytes each) that map `which` names; secret: zeroed when the call ends (Call::secret)
  uint8_t* gather(const void* src, size_t stride, size_t which, bool secret = false) {
    const size_t n = first[which + 1] - first[which];
    uint8_t* d = k.temp<uint8_t>(n * stride);
    if (secret) k.secret(d, n * stride);
    if (!k.failed) tc::launch_gather_rows(k.c->stream, (const uint8_t*)src, stride, map(which), n, d);
    return d;
  }
  uint8_t* scratch() {  // R bytes
    if (!c_v) c_v = k.temp<uint8_t>(R);
    return c_v;
  }
  // c_ok[r] &= (row r of pts is a group member); stride 0: one point for every row (Call::require_members)
  void members(bool g2, const uint8_t* pts, size_t stride) {
    uint8_t* v = scratch();
    if (!k.failed) k.require_members(g2, pts, stride, R, v, c_ok);
  }
  void finish(uint8_t* d_ok, size_t which) {
    if (!k.failed) tc::launch_scatter_bytes(k.c->stream, c_ok, map(which), R, d_ok);
  }
};

// TC_DUO_MIN / TC_PAIRING_FORM / TC_PAIRING_BUDGET / TC_SUM_PARTS (tests, experiments): read here, once per context, never on the launch path
tc::Tuning tuning_from_env() {
  tc::Tuning tn;
  if (const char* e = getenv("TC_DUO_MIN")) tn.duo_min_decode = tn.duo_min_hash = (size_t)strtoull(e, nullptr, 10);
  if (const char* f = getenv("TC_PAIRING_FORM")) tn.pairing_form = f[0] == 'q' ? 1 : f[0] == 'l' ? 2 : f[0] == 'p' ? 3 : f[0] == 'f' ? 4 : 0;
  if (const char* b = getenv("TC_PAIRING_BUDGET")) tn.pairing_budget = (size_t)strtoull(b, nullptr, 10);
  if (const char* m = getenv("TC_MSM_BUDGET")) tn.msm_budget = (size_t)strtoull(m, nullptr, 10);
  if (const char* r = getenv("TC_PRIVATE_RESERVE")) tn.private_reserve = (size_t)strtoull(r, nullptr, 10);
  if (const char* q = getenv("TC_SUM_PARTS")) {
    const size_t v = (size_t)strtoull(q, nullptr, 10);
    if (v >= 1 && v <= 64 && (v & (v - 1)) == 0) tn.sum_parts = v;  // a power of two within one wave; anything else: the default rule
  }
  if (const char* q = getenv("TC_WSUM_SLICES")) {
    const size_t v = (size_t)strtoull(q, nullptr, 10);
    if (v >= 1 && v <= 64) tn.wsum_slices = v;  // (the launch takes at most as many as there are terms); anything else: the default rule
  }
  if (const char* q = getenv("TC_RECORDS_PARTS")) {
    const size_t v = (size_t)strtoull(q, nullptr, 10);
    if (v >= 1 && v <= 64 && (v & (v - 1)) == 0) tn.records_parts = v;  // (G2 takes at most 32: a larger value means 32 there)
  }
  if (const char* g = getenv("TC_COMB_G1_MIN")) {  // "<holders>,<batch>": both or neither
    char* end = nullptr;
    const unsigned long long h = strtoull(g, &end, 10);
    if (end && end != g && *end == ',') {
      const char* b = end + 1;
      const unsigned long long m = strtoull(b, &end, 10);
      if (end && end != b) {
        tn.comb_g1_min_holders = (size_t)h;
        tn.comb_g1_min_batch = (size_t)m;
      }
    }
  }
  if (const char* e = getenv("TC_COMBINE_SEATS")) tn.combine_seats = (uint32_t)strtoul(e, nullptr, 10);
  if (const char* o = getenv("TC_CHECKS_BESIDE")) tn.checks_beside = (o[0] >= '0' && o[0] <= '2') ? o[0] - '0' : 1;  // 0 one stream, 1 low priority, 2 normal
  return tn;
}

#define TC_REQUIRE(cond)            \
  do {                              \
    if (!(cond)) {                  \
      if (ctx) ctx->err = "invalid argument: " #cond; \
      return TC_ERR_INVALID_ARG;    \
    }                               \
  } while (0)

}  // namespace

// "never throws across the boundary" (include/tc_amd.h): every entry point below is a function-try-block that ends here.
// zeroes secret host bytes in a way the optimiser may not drop
static void wipe_host(uint8_t* p, size_t n) {
  volatile uint8_t* v = p;
  for (size_t i = 0; i < n; i++) v[i] = 0;
}

// The host code allocates (std::vector, std::string); under memory pressure that throws, and an exception that crossed the C ABI
// into Rust or ctypes would be undefined behaviour.  The handler of a function-try-block runs after the entry's locals are gone:
// the call itself has been ended by its frame by then (~Call: streams drained, secrets zeroed, arena flags marked for a reset),
// so the context stays usable and all that is left to do here is to name the failure.
static int on_exception(tc_ctx* ctx) noexcept {
  const char* what = "C++ exception";
  try {
    throw;
  } catch (const std::bad_alloc&) {
    what = "host allocation failed (std::bad_alloc)";
  } catch (const std::exception&) {
    what = "C++ exception in the host code";
  } catch (...) {
  }
  if (ctx) {
    try {
      ctx->err = what;
    } catch (...) {
    }
  }
  return TC_ERR_HOST;
}

extern "C" {

const char* tc_version(void) { return "tc_amd 0.1.0 (gfx950)"; }

int tc_ctx_create(tc_ctx** out, int device) try {
  if (!out) return TC_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TC_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return TC_ERR_INVALID_ARG;
  if (hipSetDevice(device) != hipSuccess) return TC_ERR_HIP;
  tc_ctx* c = new tc_ctx();
  c->device = device;
  c->tuning = tuning_from_env();
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipMalloc((void**)&c->g1_gen, 96) != hipSuccess || hipMalloc((void**)&c->g1_gen_unfix, 96) != hipSuccess) {
    tc_ctx_destroy(c);
    return TC_ERR_HIP;
  }
  c->stream = c->own_stream;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->cus = prop.multiProcessorCount;
  }
  (void)hipGetLastError();  // (whatever this thread's earlier HIP calls left behind is not this launch's)
  tc::launch_fill_g1_generator(c->stream, c->g1_gen, c->g1_gen_unfix);
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
    // typically: no gfx950 code object for this device
    tc_ctx_destroy(c);
    return TC_ERR_NO_DEVICE;
  }
  *out = c;
  return TC_OK;
} catch (...) {
  return on_exception(nullptr);
}

void tc_ctx_destroy(tc_ctx* c) try {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // device-I/O calls may still be running on the context's (or the caller's) stream: nothing is freed under them
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);  // (joined into the main stream by every call that completed; a call that FAILED between launch and join is the exception)
  for (auto& s : c->slots)
    if (s.p) (void)hipFree(s.p);
  if (c->g1_gen) (void)hipFree(c->g1_gen);
  if (c->g1_gen_unfix) (void)hipFree(c->g1_gen_unfix);
  if (c->fb_table) (void)hipFree(c->fb_table);
  if (c->tbl_mem) (void)hipFree(c->tbl_mem);
  if (c->tbl_flags) (void)hipFree(c->tbl_flags);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  wipe_host(c->blame_key, 32);
  delete c;
} catch (...) {
}

int tc_ctx_set_device_io(tc_ctx* ctx, int enabled) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  ctx->device_io = enabled != 0;
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_set_stream(tc_ctx* ctx, void* hip_stream) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_set_input_checks(tc_ctx* ctx, int enabled) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  ctx->input_checks = enabled != 0;
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_set_blame_bisect(tc_ctx* ctx, const uint8_t* key32) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  wipe_host(ctx->blame_key, 32);
  ctx->blame_bisect = key32 != nullptr;
  // (the call counter is the context's and never goes back: setting the same key again cannot repeat a scalar)
  if (key32) memcpy(ctx->blame_key, key32, 32);
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_get_blame_bisect(const tc_ctx* ctx) { return (ctx && ctx->blame_bisect) ? 1 : 0; }

int tc_ctx_last_blame_stats(const tc_ctx* ctx, uint64_t* pairing_checks, uint64_t* rounds) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  if (pairing_checks) *pairing_checks = ctx->blame_checks;
  if (rounds) *rounds = ctx->blame_rounds;
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// gives the context's grow-only staging / table buffers back to the device (they are allocated again on demand)
int tc_ctx_trim(tc_ctx* ctx) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return TC_ERR_HIP;
  for (auto& s : ctx->slots) {
    // staging slots may have held secret operands or their recodings: zeroed before they go back to the allocator
    if (s.p) (void)hipMemsetAsync(s.p, 0, s.cap, ctx->stream);
  }
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& s : ctx->slots) {
    if (s.p) (void)hipFree(s.p);
    s.p = nullptr;
    s.cap = 0;
  }
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_get_input_checks(const tc_ctx* ctx) { return (ctx && ctx->input_checks) ? 1 : 0; }
int tc_ctx_get_device_io(const tc_ctx* ctx) { return (ctx && ctx->device_io) ? 1 : 0; }
int tc_ctx_get_tuning(const tc_ctx* ctx, uint64_t* out8) try {
  if (!ctx || !out8) return TC_ERR_INVALID_ARG;
  out8[0] = ctx->tuning.duo_min_decode;
  out8[1] = ctx->tuning.duo_min_hash;
  out8[2] = (uint64_t)ctx->tuning.pairing_form;
  out8[3] = ctx->tuning.pairing_budget;
  out8[4] = (uint64_t)ctx->tuning.checks_beside;
  out8[5] = ctx->tuning.msm_budget;
  out8[6] = ctx->tuning.private_reserve;  // ~0 = by the size of the call
  out8[7] = 0;  // reserved
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_transfer_bytes(const tc_ctx* ctx, uint64_t* h2d_bytes, uint64_t* d2h_bytes) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  if (h2d_bytes) *h2d_bytes = ctx->h2d_bytes;
  if (d2h_bytes) *d2h_bytes = ctx->d2h_bytes;
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ctx_set_timing(tc_ctx* ctx, int enabled) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  ctx->timing = enabled != 0;
  return TC_OK;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

double tc_last_kernel_ms(const tc_ctx* ctx) { return ctx ? ctx->last_ms : 0.0; }

int tc_sync(tc_ctx* ctx) try {
  if (!ctx) return TC_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return TC_ERR_HIP;
  return hipStreamSynchronize(ctx->stream) == hipSuccess ? TC_OK : TC_ERR_HIP;
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

const char* tc_last_error(const tc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// ---- hashing ------------------------------------------------------------------------------
int tc_hash_g2_batch(tc_ctx* ctx, const uint8_t* msgs, const uint64_t* off, size_t B, uint8_t* out_g2) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && off && out_g2);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || msgs);
  const uint8_t* d_msgs = k.in(msgs, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_out = k.out(out_g2, B * 192);
  k.begin_timing();
  if (!k.failed) tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, B, d_out);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_hash_g1_g2_batch(tc_ctx* ctx, const uint8_t* g1, const uint8_t* msgs, const uint64_t* off, size_t B,
                        uint8_t* out_g2, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && g1 && off && out_g2);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || msgs);
  const uint8_t* d_g1 = k.in(g1, B * 96);
  const uint8_t* d_msgs = k.in(msgs, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_out = k.out(out_g2, B * 192);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  k.check_points(false, d_g1, 96, 1, 1, B, 1);
  if (!k.failed) tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_g1, d_msgs, d_off, B, d_out, d_st);
  k.apply_checks(B, d_st, d_out, 192, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- scalar multiplication -----------------------------------------------------------------
static int point_mul(tc_ctx* ctx, bool g2, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                     uint8_t* status) {
  TC_REQUIRE(ctx);
  if (S == 0 || B == 0) return TC_OK;
  TC_REQUIRE(ctx && fr && pts && out);
  const size_t PB = g2 ? 192 : 96;
  Call k(ctx);
  const uint8_t* d_fr = k.in(fr, S * 32, /*secret=*/true);
  const uint8_t* d_pts = k.in(pts, B * PB);
  uint8_t* d_out = k.out(out, S * B * PB);
  uint8_t* d_st = k.out(status, S * B);
  k.begin_timing();
  k.check_points(g2, d_pts, PB, 1, 1, B, S);
  if (!k.failed) {
    if (g2) tc::launch_g2_mul(ctx->stream, k.tables(), d_fr, d_pts, S, B, d_out, d_st);
    else tc::launch_g1_mul(ctx->stream, k.tables(), d_fr, d_pts, S, B, d_out, d_st);
  }
  k.apply_checks(S * B, d_st, d_out, PB, nullptr);
  k.end_timing();
  return k.finish();
}

int tc_g2_mul_batch(tc_ctx* ctx, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                    uint8_t* status) try {
  return point_mul(ctx, true, fr, pts, S, B, out, status);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_g1_mul_batch(tc_ctx* ctx, const uint8_t* fr, const uint8_t* pts, size_t S, size_t B, uint8_t* out,
                    uint8_t* status) try {
  return point_mul(ctx, false, fr, pts, S, B, out, status);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_sign_shares_g2_batch(tc_ctx* ctx, const uint8_t* sk_table, size_t N, const uint64_t* idx, const uint8_t* hashes, size_t n,
                            size_t B, uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (n == 0 || B == 0) return TC_OK;
  TC_REQUIRE(ctx && sk_table && idx && hashes && out && N > 0);
  Call k(ctx);
  const uint8_t* d_sk = k.in(sk_table, N * 32, /*secret=*/true);
  const uint64_t* d_idx = k.in(idx, B * n);
  const uint8_t* d_h = k.in(hashes, B * 192);
  uint8_t* d_out = k.out(out, B * n * 192);
  uint8_t* d_st = k.out(status, B * n);
  k.begin_timing();
  k.check_points(true, d_h, 192, 1, 1, B, n);
  if (!k.failed && n >= tc::kCombMinSigners && B >= tc::kCombMinBatch) {
    // many signers per message: the doublings are done once per message, on a comb of its table (k_comb.hip); the combs
    // (133 KB per message) live in one HBM buffer, messages run through it in tiles
    const size_t per_msg = tc::comb_table_bytes(1);
    size_t tile = msm_table_budget(k) / per_msg;
    if (tile < 1) tile = 1;
    if (tile > B) tile = B;
    int32_t* d_tbl = k.temp<int32_t>(tc::comb_table_bytes(tile) / sizeof(int32_t));
    uint8_t* d_ok = k.temp<uint8_t>(tile);
    const tc::TableArena ta = k.tables();
    for (size_t lo = 0; lo < B && !k.failed; lo += tile) {
      const size_t cnt = (B - lo < tile) ? B - lo : tile;
      tc::launch_comb_sign(ctx->stream, ta, d_sk, N, d_idx + lo * n, d_h + lo * 192, n, cnt, d_tbl, d_ok, d_out + lo * n * 192,
                           d_st ? d_st + lo * n : nullptr);
    }
  } else if (!k.failed) {
    tc::launch_g2_mul_gather(ctx->stream, k.tables(), d_sk, N, d_idx, d_h, n, B, d_out, d_st);
  }
  k.apply_checks(B * n, d_st, d_out, 192, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// out[j*n + k] = sk[idx[j*n + k]] * u[j] in G1 (the multiplication stage of both tc_decrypt_shares_* entries): the per-ciphertext
// comb (k_comb.hip, tc_comb_g1.h) from the context's thresholds on, one arena ladder per share below them.  The combs (66 KB per
// ciphertext) live in one HBM buffer, ciphertexts run through it in tiles.
static void decrypt_shares_mul(Call& k, const uint8_t* d_sk, size_t N, const uint64_t* d_idx, const uint8_t* d_u, size_t n, size_t B,
                               uint8_t* d_out, uint8_t* d_st) {
  if (k.failed) return;
  tc_ctx* ctx = k.c;
  if (n >= ctx->tuning.comb_g1_min_holders && B >= ctx->tuning.comb_g1_min_batch) {
    const size_t per_ct = tc::comb_table_bytes_g1(1);
    size_t tile = msm_table_budget(k) / per_ct;
    if (tile < 1) tile = 1;
    if (tile > B) tile = B;
    int32_t* d_tbl = k.temp<int32_t>(tc::comb_table_bytes_g1(tile) / sizeof(int32_t));
    uint8_t* d_tok = k.temp<uint8_t>(tile);
    for (size_t lo = 0; lo < B && !k.failed; lo += tile) {
      const size_t cnt = (B - lo < tile) ? B - lo : tile;
      tc::launch_comb_decrypt(ctx->stream, d_sk, N, d_idx + lo * n, d_u + lo * 96, n, cnt, d_tbl, d_tok, d_out + lo * n * 96,
                              d_st ? d_st + lo * n : nullptr);
    }
  } else {
    tc::launch_g1_mul_gather(ctx->stream, k.tables(), d_sk, N, d_idx, d_u, n, B, d_out, d_st);
  }
}

int tc_decrypt_shares_g1_batch(tc_ctx* ctx, const uint8_t* sk_table, size_t N, const uint64_t* idx, const uint8_t* u_g1, size_t n, size_t B,
                               uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (n == 0 || B == 0) return TC_OK;
  TC_REQUIRE(ctx && sk_table && idx && u_g1 && out && N > 0);
  Call k(ctx);
  const uint8_t* d_sk = k.in(sk_table, N * 32, /*secret=*/true);
  const uint64_t* d_idx = k.in(idx, B * n);
  const uint8_t* d_u = k.in(u_g1, B * 96);
  uint8_t* d_out = k.out(out, B * n * 96);
  uint8_t* d_st = k.out(status, B * n);
  k.begin_timing();
  k.check_points(false, d_u, 96, 1, 1, B, n);
  decrypt_shares_mul(k, d_sk, N, d_idx, d_u, n, B, d_out, d_st);
  k.apply_checks(B * n, d_st, d_out, 96, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_sign_batch(tc_ctx* ctx, const uint8_t* fr, const uint8_t* msgs, const uint64_t* off, size_t S, size_t B,
                  uint8_t* out_g2, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (S == 0 || B == 0) return TC_OK;
  TC_REQUIRE(ctx && fr && off && out_g2);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || msgs);
  const uint8_t* d_fr = k.in(fr, S * 32, true);
  const uint8_t* d_msgs = k.in(msgs, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_frc = k.temp<uint8_t>(S * 32);
  k.secret(d_frc, S * 32);
  uint8_t* d_out = k.out(out_g2, S * B * 192);
  uint8_t* d_st = k.out(status, S * B);
  k.begin_timing();
  if (!k.failed) {
    // sk * hash_g2(m) = (sk c) * Q': the hash skips its last constant multiplication, the scalars carry it
    tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, B, d_hash, /*fix=*/false);
    tc::launch_fr_scale_cofactor_fix(ctx->stream, d_fr, S, d_frc);
    tc::launch_g2_mul(ctx->stream, k.tables(), d_frc, d_hash, S, B, d_out, d_st);
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- combination -----------------------------------------------------------------------------
// The launches of one combination over device-resident operands: Lagrange stage + the group's kernels.  d_idx: B x n u64
// abscissae (IntoFr for u64); d_idx_fr != nullptr: B x n Fr abscissae (8 canonical words each) instead -- every job takes
// the general path then, coefficients from k_lagrange_fr.  d_st: B zeroed status bytes (or already flagged jobs).
static void combine_launch(Call& k, bool g2, size_t t, size_t n, const uint64_t* d_idx, const uint32_t* d_idx_fr, const uint8_t* d_sh, size_t B,
                           uint8_t* d_pt, uint8_t* d_st) {
  tc_ctx* ctx = k.c;
  const size_t PB = g2 ? 192 : 96;
  uint32_t* d_lam = k.temp<uint32_t>(B * (t + 1) * 8);
  // G2, t <= 3: jobs are grouped by the class of their Lagrange denominator so that whole waves take
  // the cheap forms of the final division (tc_jobs.h combine_divide); not worth three launches for a
  // batch that fills a fraction of the machine anyway
  const bool group = !d_idx_fr && t >= 1 && t <= 3 && (g2 ? B >= 4096 : B >= tc::kG1GroupMinJobs);
  // (G2 groups by index tuple, or by class where the tuples are too many: k_combine.hip k_combine_group)
  uint8_t* d_cls = group && !g2 ? k.temp<uint8_t>(B) : nullptr;
  uint32_t* d_counters = group && !g2 ? k.temp<uint32_t>(8) : nullptr;
  uint32_t* d_gws = group && g2 ? k.temp<uint32_t>(tc::combine_group_ws_words(B)) : nullptr;
  uint32_t* d_perm = group ? k.temp<uint32_t>(g2 ? tc::combine_group_slots_g2(B) : tc::combine_group_slots(B)) : nullptr;
  // the count of the jobs the fast path leaves: a word of the grouping's workspace where G2 groups (k_combine_group counts
  // them, and launch_combine_g2 runs the Lagrange stage behind it), a zeroed word the Lagrange stage counts in otherwise
  const bool counted = group && g2;
  uint32_t* d_need = counted ? tc::combine_group_need(d_gws) : (t > 0 && !d_idx_fr) ? k.temp<uint32_t>(1, /*zero=*/true) : nullptr;
  if (k.failed) return;
  if (d_idx_fr) {
    // `T: IntoFr` abscissae beyond u64 (src/into_fr.rs:10-14, 28-56): no small-index fast path, no integer differences
    if (t > 0) tc::launch_lagrange_fr(ctx->stream, d_idx_fr, n, t, B, d_lam, d_st);
    if (g2 && t >= 1) msm_g2(k, t + 1, n * PB, d_sh, d_lam, B, d_pt, d_st);
    else if (g2) tc::launch_combine_g2(ctx->stream, k.tables(), t, n, nullptr, d_sh, d_lam, B, d_pt, d_st, nullptr, nullptr, nullptr);
    else if (t + 1 >= tc::kMsmMinPoints) msm_g1(k, t + 1, n * PB, d_sh, d_lam, B, d_pt, d_st);
    else tc::launch_combine_g1(ctx->stream, t, n, nullptr, d_sh, d_lam, B, d_pt, d_st, nullptr);
    return;
  }
  if (t + 1 >= tc::kMsmMinPoints) {
    uint32_t* d_ws = k.temp<uint32_t>(tc::lagrange_all_ws_words(t, B));
    if (!k.failed) tc::launch_lagrange_all(ctx->stream, d_idx, n, t, B, d_lam, d_ws, d_st);
  } else if (t > 0 && !counted) {
    tc::launch_lagrange(ctx->stream, d_idx, n, t, B, d_lam, d_st, d_need);
  }
  if (g2 && t + 1 >= tc::kMsmMinPoints) {
    msm_g2(k, t + 1, n * PB, d_sh, d_lam, B, d_pt, d_st);  // large thresholds: every job, coefficients from the one-inversion kernels
  } else if (g2) {
    // t <= 3: small-index fast path first; then (t >= 1) the jobs it left, through the two-stage kernels
    tc::t_combine_seats = ctx->tuning.combine_seats;
    tc::launch_combine_g2(ctx->stream, k.tables(), t, n, d_idx, d_sh, d_lam, B, d_pt, d_st, d_gws, d_perm, d_need,
                          k.fork_event());
    if (t >= 1) {
      tc::MsmFilter f;
      f.need = d_need;
      f.idx = d_idx;
      f.n_per_job = n;
      f.t = t;
      msm_g2(k, t + 1, n * PB, d_sh, d_lam, B, d_pt, d_st, 64, f);
    }
  }
  else if (t + 1 >= tc::kMsmMinPoints) msm_g1(k, t + 1, n * PB, d_sh, d_lam, B, d_pt, d_st);  // large thresholds in G1: the same two stages
  else tc::launch_combine_g1(ctx->stream, t, n, d_idx, d_sh, d_lam, B, d_pt, d_st, d_need,
                             k.tables(), d_cls, d_counters, d_perm, k.fork_event());
}

// samples.len() <= t  =>  Err(NotEnoughShares) for every job        (src/lib.rs:731-733)
static int not_enough_shares(Call& k, size_t B, uint8_t* out, size_t out_bytes, uint8_t* status) {
  if (k.c->device_io) {
    k.check(hipMemsetAsync(status, TC_JOB_NOT_ENOUGH_SHARES, B, k.c->stream), "memset");
    if (out && out_bytes) k.check(hipMemsetAsync(out, 0, B * out_bytes, k.c->stream), "memset");
  } else {
    memset(status, TC_JOB_NOT_ENOUGH_SHARES, B);
    if (out && out_bytes) memset(out, 0, B * out_bytes);
  }
  return k.finish();
}

// idx_fr != nullptr: the abscissae as 32-byte Fr values (idx unused); wire: the shares arrive compressed (48 / 96 B, checked
// decode) and a G2 result leaves compressed
static int combine(tc_ctx* ctx, bool g2, size_t t, size_t n, const uint64_t* idx, const uint8_t* idx_fr, const uint8_t* shares, size_t B,
                   uint8_t* out, uint8_t* status, const uint8_t* v, const uint64_t* off, uint8_t* plain, bool wire = false,
                   bool plain_unbacked = false) {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && out && status);
  TC_REQUIRE(t < (1u << 20));
  const size_t PB = g2 ? 192 : 96, CB = PB / 2;
  const size_t OB = plain ? 0 : (wire ? CB : PB);  // bytes of a point result
  Call k(ctx);
  if (n <= t) return not_enough_shares(k, B, plain ? nullptr : out, OB, status);
  TC_REQUIRE((idx || idx_fr) && shares);
  uint64_t total = 0;
  if (plain) {
    TC_REQUIRE(off);
    if (!total_bytes(k, off, B, &total)) return k.finish();
    TC_REQUIRE(total == 0 || v);
    TC_REQUIRE(total == 0 || !plain_unbacked);  // (a null plaintext buffer is only acceptable when there is nothing to write)
  }
  const uint64_t* d_idx = idx_fr ? nullptr : k.in(idx, B * n);
  const uint32_t* d_idx_fr = idx_fr ? reinterpret_cast<const uint32_t*>(k.in(idx_fr, B * n * 32)) : nullptr;
  const uint8_t* d_sh = k.in(shares, B * n * (wire ? CB : PB));
  uint8_t* d_st = k.out(status, B, /*zero=*/true);
  uint8_t* d_pt = (plain || wire) ? k.temp<uint8_t>(B * PB) : k.out(out, B * PB);
  uint8_t* d_wire_out = (wire && !plain) ? k.out(out, B * CB) : nullptr;
  const uint8_t* d_v = nullptr;
  const uint64_t* d_off = nullptr;
  uint8_t* d_plain = nullptr;
  if (plain) {
    d_v = k.in(v, (size_t)total);
    d_off = k.in(off, B + 1);
    d_plain = k.out(plain, (size_t)total, /*zero=*/true);  // failed jobs leave zeros, never stale staging bytes
  }
  k.begin_timing();
  size_t n_eff = n;
  if (idx_fr && !k.failed) {
    // abscissae that merely ARRIVED as Fr but fit 64 bits take the u64 kernels (fast path included); one word comes back
    uint64_t* d_idx64 = k.temp<uint64_t>(B * n);
    uint32_t* d_wide = k.temp<uint32_t>(1, /*zero=*/true);
    uint8_t* d_canon = k.temp<uint8_t>(B);
    if (!k.failed) {
      k.check(hipMemsetAsync(d_canon, 1, B, ctx->stream), "memset");
      tc::launch_fr_idx_narrow(ctx->stream, d_idx_fr, n, t + 1, B, d_idx64, d_wide, d_canon);
      uint32_t wide = 0;  // (a stack slot, like total_bytes': the wait is the next statement)
      k.readback(&wide, d_wide, 4, "readback");
      k.wait();
      k.checks.push_back({d_canon, 1, 1});  // a job that owns a non-canonical abscissa (>= r) fails like an undecodable operand
      if (wide == 0) {
        d_idx = d_idx64;
        d_idx_fr = nullptr;
      }
    }
  }
  if (wire && !k.failed) {
    // the first t+1 samples of every job through the checked decode of from_bytes (src/lib.rs:140-146, 246-252), compactly
    uint8_t* d_dec = k.temp<uint8_t>(B * (t + 1) * PB);
    uint8_t* d_valid = k.temp<uint8_t>(B * (t + 1));
    if (!k.failed) {
      tc::launch_decompress_take(ctx->tuning, ctx->stream, g2, d_sh, n, t + 1, B, d_dec, d_valid);
      k.checks.push_back({d_valid, t + 1, 1});
      if (d_idx_fr) {
        uint32_t* d_fr2 = k.temp<uint32_t>(B * (t + 1) * 8);
        if (d_fr2) tc::launch_take_u64(ctx->stream, reinterpret_cast<const uint64_t*>(d_idx_fr), n * 4, (t + 1) * 4, B, reinterpret_cast<uint64_t*>(d_fr2));
        d_idx_fr = d_fr2;
      } else {
        uint64_t* d_idx2 = k.temp<uint64_t>(B * (t + 1));
        if (d_idx2) tc::launch_take_u64(ctx->stream, d_idx, n, t + 1, B, d_idx2);
        d_idx = d_idx2;
      }
      d_sh = d_dec;
      n_eff = t + 1;
    }
  } else {
    k.check_points(g2, d_sh, PB, n, t + 1, B, 1);  // exactly the first t+1 samples interpolate() takes
  }
  if (!k.failed) {
    combine_launch(k, g2, t, n_eff, d_idx, d_idx_fr, d_sh, B, d_pt, d_st);
    k.apply_checks(B, d_st, d_pt, PB, nullptr);
    if (plain) tc::launch_xor_with_hash(ctx->stream, d_pt, d_v, d_off, B, d_plain, d_st);
    else if (wire) {
      if (g2) tc::launch_g2_compress(ctx->stream, d_pt, B, d_wire_out, nullptr);   // Signature::to_bytes src/lib.rs:255-259
      else tc::launch_g1_compress(ctx->stream, d_pt, B, d_wire_out, nullptr);
    }
  }
  k.end_timing();
  return k.finish();
}

int tc_combine_g2_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares,
                        size_t B, uint8_t* out, uint8_t* status) try {
  return combine(ctx, true, t, n_per_job, idx, nullptr, shares, B, out, status, nullptr, nullptr, nullptr);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_combine_g1_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares,
                        size_t B, uint8_t* out, uint8_t* status) try {
  return combine(ctx, false, t, n_per_job, idx, nullptr, shares, B, out, status, nullptr, nullptr, nullptr);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// The plaintext buffer of a batch whose plaintexts are ALL empty has no address when it is device-resident (an empty tensor's
// data pointer is null): the decrypt entries then stand a private byte in for it -- never written, combine() insists that the
// total length is 0 -- so that `SecretKey::decrypt(encrypt(b""))` works with either residency.
static uint8_t g_no_plaintext_bytes;
int tc_decrypt_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares_g1,
                     const uint8_t* v, const uint64_t* off, size_t B, uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;  // (an empty batch is a no-op for every entry: a device-resident empty buffer has no address)
  TC_REQUIRE(ctx && status && off);
  const bool unbacked = out == nullptr;
  if (unbacked) out = &g_no_plaintext_bytes;
  return combine(ctx, false, t, n_per_job, idx, nullptr, shares_g1, B, out /*non-null marker*/, status, v, off, out, /*wire=*/false, unbacked);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// `T: IntoFr` beyond u64 (src/into_fr.rs:10-14, 28-56; combine_signatures / decrypt are generic over it, src/lib.rs:608-622)
int tc_combine_g2_fr_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint8_t* idx_fr, const uint8_t* shares, size_t B, uint8_t* out,
                           uint8_t* status) try {
  return combine(ctx, true, t, n_per_job, nullptr, idx_fr, shares, B, out, status, nullptr, nullptr, nullptr);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}
int tc_combine_g1_fr_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint8_t* idx_fr, const uint8_t* shares, size_t B, uint8_t* out,
                           uint8_t* status) try {
  return combine(ctx, false, t, n_per_job, nullptr, idx_fr, shares, B, out, status, nullptr, nullptr, nullptr);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}
int tc_decrypt_fr_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint8_t* idx_fr, const uint8_t* shares_g1, const uint8_t* v,
                        const uint64_t* off, size_t B, uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;  // (an empty batch is a no-op for every entry: a device-resident empty buffer has no address)
  TC_REQUIRE(ctx && status && off);
  const bool unbacked = out == nullptr;
  if (unbacked) out = &g_no_plaintext_bytes;
  return combine(ctx, false, t, n_per_job, nullptr, idx_fr, shares_g1, B, out, status, v, off, out, /*wire=*/false, unbacked);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// wire-level forms: shares as they travel (Signature::to_bytes / DecryptionShare's compressed G1, checked decode of
// from_bytes src/lib.rs:140-146, 246-252), the combined signature back as Signature::to_bytes (src/lib.rs:255-259)
int tc_combine_signatures_wire_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares96, size_t B,
                                     uint8_t* out96, uint8_t* status) try {
  return combine(ctx, true, t, n_per_job, idx, nullptr, shares96, B, out96, status, nullptr, nullptr, nullptr, /*wire=*/true);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}
int tc_decrypt_wire_batch(tc_ctx* ctx, size_t t, size_t n_per_job, const uint64_t* idx, const uint8_t* shares48, const uint8_t* v,
                          const uint64_t* off, size_t B, uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;  // (an empty batch is a no-op for every entry: a device-resident empty buffer has no address)
  TC_REQUIRE(ctx && status && off);
  const bool unbacked = out == nullptr;
  if (unbacked) out = &g_no_plaintext_bytes;
  return combine(ctx, false, t, n_per_job, idx, nullptr, shares48, B, out, status, v, off, out, /*wire=*/true, unbacked);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

static int lincomb(tc_ctx* ctx, bool g2, size_t n, const uint8_t* scalars, const uint8_t* points, size_t B, uint8_t* out,
                   uint8_t* status) {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && out && (n == 0 || (scalars && points)));
  const size_t PB = g2 ? 192 : 96;
  Call k(ctx);
  const uint8_t* d_sc = k.in(scalars, B * n * 32, /*secret=*/true);
  const uint8_t* d_pt = k.in(points, B * n * PB);
  uint8_t* d_out = k.out(out, B * PB);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  k.check_points(g2, d_pt, PB, n, n, B, 1);
  if (!k.failed) {
    if (g2 && n == 0) {
      // the empty sum: the identity (flag byte 0x40, then zeros) for every job
      k.check(hipMemsetAsync(d_out, 0, B * PB, ctx->stream), "memset");
      k.check(hipMemset2DAsync(d_out, PB, 0x40, 1, B, ctx->stream), "memset");
      if (d_st) k.check(hipMemsetAsync(d_st, 0, B, ctx->stream), "memset");
    } else if (g2) {
      uint8_t* st_buf = d_st ? d_st : k.temp<uint8_t>(B);
      if (st_buf) k.check(hipMemsetAsync(st_buf, 0, B, ctx->stream), "memset");
      msm_g2(k, n, n * PB, d_pt, reinterpret_cast<const uint32_t*>(d_sc), B, d_out, st_buf, 64, tc::MsmFilter(), /*secret_scalars=*/true);
    } else if (n >= tc::kMsmMinPoints) {
      uint8_t* st_buf = d_st ? d_st : k.temp<uint8_t>(B);
      if (st_buf) k.check(hipMemsetAsync(st_buf, 0, B, ctx->stream), "memset");
      msm_g1(k, n, n * PB, d_pt, reinterpret_cast<const uint32_t*>(d_sc), B, d_out, st_buf, 128, /*secret_scalars=*/true);
    } else tc::launch_lincomb_g1(ctx->stream, n, d_sc, d_pt, B, d_out, d_st);
  }
  k.apply_checks(B, d_st, d_out, PB, nullptr);
  k.end_timing();
  return k.finish();
}

int tc_g1_lincomb_batch(tc_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* points, size_t B, uint8_t* out,
                        uint8_t* status) try {
  return lincomb(ctx, false, n, scalars, points, B, out, status);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_g2_lincomb_batch(tc_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* points, size_t B, uint8_t* out,
                        uint8_t* status) try {
  return lincomb(ctx, true, n, scalars, points, B, out, status);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_xor_with_hash_batch(tc_ctx* ctx, const uint8_t* g1, const uint8_t* data, const uint64_t* off, size_t B,
                           uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && g1 && off);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || (data && out));  // (all-empty inputs: a device-resident empty buffer has no address)
  const uint8_t* d_g1 = k.in(g1, B * 96);
  const uint8_t* d_data = k.in(data, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_out = k.out(out, (size_t)total, /*zero=*/true);
  uint8_t* d_st = k.out(status, B, /*zero=*/true);
  k.begin_timing();
  k.check_points(false, d_g1, 96, 1, 1, B, 1);
  if (!k.failed) {
    k.apply_checks(B, d_st, nullptr, 0, nullptr);  // the keystream kernel skips jobs already flagged
    tc::launch_xor_with_hash(ctx->stream, d_g1, d_data, d_off, B, d_out, d_st);
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- pairing checks ---------------------------------------------------------------------------
int tc_pairing_check_batch(tc_ctx* ctx, const uint8_t* a, size_t sa, const uint8_t* b, size_t sb, const uint8_t* c,
                           size_t sc, const uint8_t* d, size_t sd, size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && a && b && c && d && ok);
  TC_REQUIRE((sa == 0 || sa >= 96) && (sc == 0 || sc >= 96) && (sb == 0 || sb >= 192) && (sd == 0 || sd >= 192));
  Call k(ctx);
  auto span = [&](size_t stride, size_t bytes) { return stride ? (B - 1) * stride + bytes : bytes; };
  const uint8_t* da = k.in(a, span(sa, 96));
  const uint8_t* db = k.in(b, span(sb, 192));
  const uint8_t* dc = k.in(c, span(sc, 96));
  const uint8_t* dd = k.in(d, span(sd, 192));
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  k.check_points(false, da, sa, 1, 1, B, 1);
  k.check_points(true, db, sb, 1, 1, B, 1);
  k.check_points(false, dc, sc, 1, 1, B, 1);
  k.check_points(true, dd, sd, 1, 1, B, 1);
  if (!k.failed) tc::launch_pairing_check(ctx->stream, da, sa, db, sb, dc, sc, dd, sd, B, d_ok, k.pairing_ws(B));
  k.apply_checks(B, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ok[j] = ( prod_{k < n} e(a[j n + k], b[j n + k]) == 1 ): the multi-pairing behind every check of the reference
// (src/lib.rs:109, :185, :511 are n = 2 with one G1 operand negated), n pairs sharing ONE final exponentiation.
int tc_pairing_product_check_batch(tc_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && a && b && ok && n >= 1);
  TC_REQUIRE(n < (1ull << 32) && B < (1ull << 32) && n * B < (1ull << 32));
  Call k(ctx);
  const uint8_t* da = k.in(a, B * n * 96);
  const uint8_t* db = k.in(b, B * n * 192);
  uint8_t* d_ok = k.out(ok, B);
  int32_t* ws = k.pairing_product_ws(n, B, false);
  k.begin_timing();
  k.check_points(false, da, 96, n, n, B, 1);
  k.check_points(true, db, 192, n, n, B, 1);
  if (!k.failed) tc::launch_pairing_product_check(ctx->stream, da, 96, db, 192, n, B, nullptr, 0, nullptr, 0, d_ok, ws);
  k.apply_checks(B, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_verify_g2_batch(tc_ctx* ctx, const uint8_t* pk, size_t pk_stride, const uint8_t* sig, const uint8_t* hash,
                       size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && pk && sig && hash && ok);
  TC_REQUIRE(pk_stride == 0 || pk_stride >= 96);
  Call k(ctx);
  const uint8_t* d_pk = k.in(pk, pk_stride ? (B - 1) * pk_stride + 96 : 96);
  const uint8_t* d_sig = k.in(sig, B * 192);
  const uint8_t* d_hash = k.in(hash, B * 192);
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  k.check_points(false, d_pk, pk_stride, 1, 1, B, 1);
  k.check_points(true, d_sig, 192, 1, 1, B, 1);
  k.check_points(true, d_hash, 192, 1, 1, B, 1);
  // e(pk, hash) == e(g1, sig)                                           (src/lib.rs:109)
  if (!k.failed) tc::launch_pairing_check(ctx->stream, d_pk, pk_stride, d_hash, 192, ctx->g1_gen, 0, d_sig, 192, B, d_ok, k.pairing_ws(B));
  k.apply_checks(B, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_verify_sig_batch(tc_ctx* ctx, const uint8_t* pk, size_t pk_stride, const uint8_t* sig, const uint8_t* msgs,
                        const uint64_t* off, size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && pk && sig && off && ok);
  TC_REQUIRE(pk_stride == 0 || pk_stride >= 96);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || msgs);
  const uint8_t* d_pk = k.in(pk, pk_stride ? (B - 1) * pk_stride + 96 : 96);
  const uint8_t* d_sig = k.in(sig, B * 192);
  const uint8_t* d_msgs = k.in(msgs, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  k.check_points(false, d_pk, pk_stride, 1, 1, B, 1);
  k.check_points(true, d_sig, 192, 1, 1, B, 1);
  if (!k.failed) {
    // e(pk, [c] Q') == e(g1, sig)  <=>  e(pk, Q') == e([1/c] g1, sig): the hash skips its last constant
    // multiplication and the generator side uses the context's pre-scaled generator
    tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, B, d_hash, /*fix=*/false);
    tc::launch_pairing_check(ctx->stream, d_pk, pk_stride, d_hash, 192, ctx->g1_gen_unfix, 0, d_sig, 192, B, d_ok, k.pairing_ws(B));
  }
  k.apply_checks(B, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Share validation by ONE random linear combination per message (opt-in fast path of the loop at
// examples/threshold_sig.rs:115-131): instead of N pairing checks  e(pk_i, H(m)) == e(g1, sig_i)  the device
// checks  e(sum_i r_i pk_i, H(m)) == e(g1, sum_i r_i sig_i)  with secret r_i (2^63 values), which holds whenever all N
// do and fails with probability >= 1 - 2^-63 otherwise; messages whose combined check fails are re-checked
// share by share, so ok[] equals the per-share path's (up to that 2^-63).
int tc_verify_shares_rlc_batch(tc_ctx* ctx, const uint8_t* pk_shares, size_t N, const uint8_t* sig_shares, const uint8_t* msgs,
                               const uint64_t* off, size_t B, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0 || N == 0) return TC_OK;
  TC_REQUIRE(ctx && pk_shares && sig_shares && off && seed32 && ok);
  TC_REQUIRE(B * N < (1ull << 32));
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || msgs);
  const uint8_t* d_pk = k.in(pk_shares, N * 96);
  const uint8_t* d_sig = k.in(sig_shares, B * N * 192);
  const uint8_t* d_msgs = k.in(msgs, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_seed = k.secret_seed(seed32);
  uint8_t* d_r = k.secret_temp<uint8_t>(B * N * 32);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_S = k.temp<uint8_t>(B * 192);
  uint8_t* d_P = k.temp<uint8_t>(B * 96);
  uint8_t* d_stS = k.temp<uint8_t>(B);
  uint8_t* d_okmsg = k.temp<uint8_t>(B);
  uint8_t* d_ok = k.out(ok, B * N);
  k.begin_timing();
  k.check_points(false, d_pk, 96, N, N, 1, (size_t)-1);
  k.check_points(true, d_sig, 192, N, N, B, 1);
  if (!k.failed) {
    tc::launch_rlc_scalars(ctx->stream, d_seed, B * N, d_r);
    // (the two-stage kernels' short-scalar mode: 16 doublings for the 64-bit random scalars)
    k.check(hipMemsetAsync(d_stS, 0, B, ctx->stream), "memset");
    msm_g2(k, N, N * 192, d_sig, reinterpret_cast<const uint32_t*>(d_r), B, d_S, d_stS, /*nbits=*/16, tc::MsmFilter(), /*secret_scalars=*/true);
    tc::launch_lincomb_g1(ctx->stream, N, d_r, d_pk, B, d_P, nullptr, /*shared_points=*/true);
    tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, B, d_hash, /*fix=*/false);
    // e(P, [c] Q') == e(g1, S)  <=>  e(P, Q') == e([1/c] g1, S)   (the folded hash constant of tc_verify_sig_batch)
    tc::launch_pairing_check(ctx->stream, d_P, 96, d_hash, 192, ctx->g1_gen_unfix, 0, d_S, 192, B, d_okmsg, k.pairing_ws(B));
    // a share that does not decode (status below) or, in checked-input mode, is no group member sends its
    // message to the per-share fallback
    k.apply_checks(B, nullptr, nullptr, 0, d_okmsg);
    k.check(hipMemsetAsync(d_ok, 1, B * N, ctx->stream), "memset");
    const uint8_t* h_okmsg = k.fetch(d_okmsg, B, "ok readback");
    const uint8_t* h_stS = k.fetch(d_stS, B, "status readback");
    std::vector<uint32_t> failed;
    if (k.wait())
      for (size_t j = 0; j < B; j++)
        if (!h_okmsg[j] || h_stS[j] != TC_JOB_OK) failed.push_back((uint32_t)j);
    if (!k.failed && !failed.empty()) {
      // per-share pairing checks for every share of the failed messages, on compacted operands
      const size_t F = failed.size(), R = F * N;
      tc::SlotMaps m = tc::slot_maps(failed.data(), F, N);
      Compacted c(k, R, std::move(m.record), std::move(m.job), std::move(m.slot));
      const uint8_t* c_sig = c.gather(d_sig, 192, 0);
      const uint8_t* c_hash = c.gather(d_hash, 192, 1);
      const uint8_t* c_pk = c.gather(d_pk, 96, 2);
      const tc::PairingWs pws = k.pairing_ws(R);
      if (!k.failed) tc::launch_pairing_check(ctx->stream, c_pk, 96, c_hash, 192, ctx->g1_gen_unfix, 0, c_sig, 192, R, c.c_ok, pws);
      if (ctx->input_checks) {  // members only, as the per-share path would require
        c.members(true, c_sig, 192);
        c.members(false, c_pk, 96);
      }
      c.finish(d_ok, 0);
      if (n_fallback) *n_fallback = F;
    }
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// The device temporaries of one pass of group checks over B jobs (seed32: HOST memory, copied here and wiped after the call);
// `group` is the caller's, cut: what it means for B jobs (tc_fallback.h).
struct RlcWs {
  tc::GroupCut cut;
  uint8_t *d_seed, *d_r, *d_S, *d_H, *d_st, *d_okg;
};
static RlcWs rlc_workspace(Call& k, size_t B, size_t group, const uint8_t* seed32) {
  RlcWs w{};
  w.cut = tc::group_cut(B, group);
  w.d_seed = k.secret_seed(seed32);
  w.d_r = k.secret_temp<uint8_t>(B * 32);
  w.d_S = k.temp<uint8_t>(w.cut.NG * 192);
  w.d_H = k.temp<uint8_t>(w.cut.NG * 192);
  w.d_st = k.temp<uint8_t>(2 * w.cut.NG);
  w.d_okg = k.temp<uint8_t>(w.cut.NG);
  return w;
}
// The group checks of verify_rlc over DEVICE operands, inside the caller's Call: d_ok[j] (B bytes) = e(pk, hash_j) ==
// e(g1, sig_j) up to the 2^-63 of a wrongly passing group.  d_g1 is the generator that matches the hash points (g1_gen, or
// g1_gen_unfix for hash points without their last constant multiplication).  v_key / v_sig / v_hash: the handles of the
// caller's pending membership tests (Call::check_points; null: not registered) -- one byte for the key, one per job for the
// others; they are consumed here and send their groups to the per-job checks.  member_checks: the per-job checks test sig
// (and the hash points when hash_is_operand) and the key for membership again, as tc_verify_g2_batch would.
// tc_combine_signatures_robust_batch runs this over the combinations it has just made, with no pending test and
// member_checks off.  *n_fallback (optional) = jobs that went through the per-job checks.
static void rlc_group_checks(Call& k, const RlcWs& w, const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_hash, const uint8_t* d_g1,
                             size_t B, const uint8_t* v_key, const uint8_t* v_sig, const uint8_t* v_hash, bool member_checks,
                             bool hash_is_operand, uint8_t* d_ok, uint64_t* n_fallback) {
  tc_ctx* ctx = k.c;
  const size_t group = w.cut.group, G = w.cut.G, tail = w.cut.tail, NG = w.cut.NG;
  uint8_t *d_seed = w.d_seed, *d_r = w.d_r, *d_S = w.d_S, *d_H = w.d_H, *d_st = w.d_st, *d_okg = w.d_okg;
  if (k.failed) return;
  tc::launch_rlc_scalars(ctx->stream, d_seed, B, d_r);
  k.check(hipMemsetAsync(d_st, 0, 2 * NG, ctx->stream), "memset");
  const uint32_t* rr = reinterpret_cast<const uint32_t*>(d_r);
  if (G) {
    msm_g2(k, group, group * 192, d_sig, rr, G, d_S, d_st, /*nbits=*/16, tc::MsmFilter(), /*secret_scalars=*/true);
    msm_g2(k, group, group * 192, d_hash, rr, G, d_H, d_st + NG, 16, tc::MsmFilter(), true);
  }
  if (tail) {
    msm_g2(k, tail, tail * 192, d_sig + G * group * 192, rr + G * group * 8, 1, d_S + G * 192, d_st + G, 16, tc::MsmFilter(), true);
    msm_g2(k, tail, tail * 192, d_hash + G * group * 192, rr + G * group * 8, 1, d_H + G * 192, d_st + NG + G, 16, tc::MsmFilter(), true);
  }
  tc::launch_pairing_check(ctx->stream, d_pk, 0, d_H, 192, d_g1, 0, d_S, 192, NG, d_okg, k.pairing_ws(NG));
  k.check(hipMemsetAsync(d_ok, 1, B, ctx->stream), "memset");
  const uint8_t* h_okg = k.fetch(d_okg, NG, "ok readback");
  const uint8_t* h_st = k.fetch(d_st, 2 * NG, "status readback");
  // checked-input mode: a group that owns a non-member operand goes to the per-job path as well
  // (the membership tests ran beside the two sums and the group checks)
  const uint8_t *h_vkey, *h_vsig, *h_vhash;
  k.take_verdicts({{v_key, &h_vkey}, {v_sig, &h_vsig}, {v_hash, &h_vhash}});
  if (!k.wait()) return;
  tc::BadGroups bad(w.cut, B);
  bad.per_group(h_okg, true);
  bad.per_group(h_st, false);       // the sums of the signatures
  bad.per_group(h_st + NG, false);  // and of the hash points
  if (h_vkey && h_vkey[0] == 0) bad.all();
  bad.jobs({h_vsig, h_vhash}, true);
  std::vector<uint32_t> failed = bad.failed_jobs();
  if (failed.empty()) return;
  // per-job pairing checks for every job of the failed groups, on compacted operands
  const size_t R = failed.size();
  Compacted c(k, R, std::move(failed));
  const uint8_t* c_sig = c.gather(d_sig, 192, 0);
  const uint8_t* c_hash = c.gather(d_hash, 192, 0);
  const tc::PairingWs pws = k.pairing_ws(R);
  if (!k.failed) tc::launch_pairing_check(ctx->stream, d_pk, 0, c_hash, 192, d_g1, 0, c_sig, 192, R, c.c_ok, pws);
  if (member_checks) {  // members only, as the per-job path would require
    c.members(true, c_sig, 192);
    if (hash_is_operand) c.members(true, c_hash, 192);
    c.members(false, d_pk, 0);  // the one key
  }
  c.finish(d_ok, 0);
  if (n_fallback) *n_fallback = R;
}

// Signature batches under ONE key (BASELINE config 3's shape: 65 536 verifies under the master key) by random linear
// combination, opt-in: the batch is cut into groups of `group` jobs, and a group passes with ONE check
//     e(pk, sum_j r_j H_j) == e(g1, sum_j r_j sig_j)          (bilinearity; r_j secret, 2^63 values each)
// instead of `group` checks of src/lib.rs:109; a group that fails (or holds an undecodable / non-member operand) is
// re-checked job by job, so ok[] equals tc_verify_g2_batch's up to the 2^-63 of a wrongly passing group.  The two sums
// are 16-column ladders over the psi-images (the two-stage kernels' short-scalar mode).  hash == nullptr: the hash points
// are made on the device from msgs / off first (tc_verify_sig_batch's composition, hash constant folded into g1).
static int verify_rlc(tc_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* hash, const uint8_t* msgs, const uint64_t* off,
                      size_t B, size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && pk && sig && (hash || off) && seed32 && ok);
  TC_REQUIRE(B < (1ull << 32));
  Call k(ctx);
  uint64_t total = 0;
  if (!hash) {
    if (!total_bytes(k, off, B, &total)) return k.finish();
    TC_REQUIRE(total == 0 || msgs);
  }
  const uint8_t* d_pk = k.in(pk, 96);
  const uint8_t* d_sig = k.in(sig, B * 192);
  const uint8_t* d_hash_in = hash ? k.in(hash, B * 192) : nullptr;
  const uint8_t* d_msgs = hash ? nullptr : k.in(msgs, (size_t)total);
  const uint64_t* d_off = hash ? nullptr : k.in(off, B + 1);
  uint8_t* d_hash_own = hash ? nullptr : k.temp<uint8_t>(B * 192);
  const uint8_t* d_hash = hash ? d_hash_in : d_hash_own;
  const uint8_t* d_g1 = hash ? ctx->g1_gen : ctx->g1_gen_unfix;
  const RlcWs ws = rlc_workspace(k, B, group, seed32);
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  const uint8_t* v_key = k.check_points(false, d_pk, 0, 1, 1, B, 1);
  const uint8_t* v_sig = k.check_points(true, d_sig, 192, 1, 1, B, 1);
  const uint8_t* v_hash = hash ? k.check_points(true, d_hash, 192, 1, 1, B, 1) : nullptr;
  if (!k.failed) {
    if (!hash) tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, B, d_hash_own, /*fix=*/false);
    rlc_group_checks(k, ws, d_pk, d_sig, d_hash, d_g1, B, v_key, v_sig, v_hash, ctx->input_checks, hash != nullptr, d_ok, n_fallback);
  }
  k.end_timing();
  return k.finish();
}

int tc_verify_g2_rlc_batch(tc_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* hash, size_t B, size_t group,
                           const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  if (ctx && !hash) {
    ctx->err = "invalid argument: hash";
    return TC_ERR_INVALID_ARG;
  }
  return verify_rlc(ctx, pk, sig, hash, nullptr, nullptr, B, group, seed32, ok, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_verify_sig_rlc_batch(tc_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs, const uint64_t* off, size_t B,
                            size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  if (ctx && !off) {
    ctx->err = "invalid argument: off";
    return TC_ERR_INVALID_ARG;
  }
  return verify_rlc(ctx, pk, sig, nullptr, msgs, off, B, group, seed32, ok, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// What the two ragged entries (verify_records, verify_dshare_records) share around their sums and their fallback: rec_off on the
// host, the inputs of the plan, the key of record r, the identity pairs that fill up the last group, and key_idx on the host.
struct Records {
  Call& k;
  const uint8_t* pks;
  const uint64_t* key_idx;  // the caller's, in the memory of the other operands; null: record r under pks[r]
  size_t K, M, R = 0, simd_lanes = 0;
  tc::GroupCut cut;              // groups of jobs (messages / ciphertexts)
  uint64_t longest = 0;          // the most records of one job
  const uint64_t *hr = nullptr, *d_kidx = nullptr;  // rec_off on the host; key_idx as an operand
  std::vector<uint64_t> h_grp;  // NG + 1 values, the first record of every group (host arithmetic only: never copied)
  const uint8_t *d_pk = nullptr, *d_keys = nullptr;  // the key table; the key of record r
  Records(Call& call, const uint8_t* pks_, size_t K_, const uint64_t* key_idx_, size_t M_, size_t group)
      : k(call), pks(pks_), key_idx(key_idx_), K(K_), M(M_), cut(tc::group_cut(M_, group)), h_grp(cut.NG + 1) {}
  bool require(bool cond, const char* what) {
    if (!cond) k.fail(std::string("invalid argument: ") + what);
    k.arg_error = k.arg_error || !cond;
    return cond;
  }
  // rec_off comes to the host in both I/O modes (device I/O: 8 (M + 1) bytes and one sync: the chunk ranges of the segments are host
  // arithmetic, tc_records.h) and is validated.  records / ok: the caller's per-record operand and output.  false: the call is
  // over -- an error, or no record at all -- and the entry returns k.finish()
  bool offsets(const uint64_t* rec_off, const void* records, const void* ok) {
    hr = k.c->device_io ? k.fetch(rec_off, M + 1, "offset readback") : rec_off;
    if (k.c->device_io && !k.wait()) return false;
    bool good = hr[0] == 0;
    for (size_t m = 0; m < M && good; m++) good = hr[m + 1] >= hr[m];
    if (!require(good, "offsets must start at 0 and be non-decreasing") || !require(hr[M] < (1ull << 32), "R < 2^32")) return false;
    R = (size_t)hr[M];
    if (R == 0 || !require(records && ok && (K == 0 || pks), "records && ok && (K == 0 || pks)") || !require(key_idx || K >= R, "key_idx || K >= R"))
      return false;
    simd_lanes = (size_t)(k.c->cus > 0 ? k.c->cus : 256) * 4 * tc::kBlock;  // one wave per SIMD
    for (size_t m = 0; m < M; m++) longest = hr[m + 1] - hr[m] > longest ? hr[m + 1] - hr[m] : longest;
    tc::rec_group_ranges(hr, M, cut.group, h_grp.data());
    return true;
  }
  bool tables_fit(size_t table_bytes) {  // false: the sums need more table memory than a call may spend; the entry returns k.finish()
    const bool fit = table_bytes <= msm_table_budget(k);
    if (!fit) k.fail("out of memory: the tables of " + std::to_string(R) + " records need " + std::to_string(table_bytes >> 20) + " MB; split the call");
    return fit;
  }
  void stage_keys() {  // the key table and the indices as operands; d_keys: the table itself, or the room that gather_keys() fills
    d_pk = k.in(pks, K * 96);
    d_kidx = k.in(key_idx, key_idx ? R : 0);
    d_keys = key_idx ? k.temp<uint8_t>(R * 96) : d_pk;
  }
  void gather_keys() { if (key_idx) tc::launch_rec_gather_keys(k.c->stream, d_pk, K, d_kidx, R, const_cast<uint8_t*>(d_keys)); }
  // the pairs that fill up the last group, so that ONE launch checks every group: `count` identities of G2 at g2_tail, of G1 at g1_tail
  void pad_identities(uint8_t* g2_tail, uint8_t* g1_tail, size_t count) {
    if (count == 0) return;
    uint8_t* h_pad = k.host<uint8_t>(count * (192 + 96));
    for (size_t i = 0; i < count; i++) h_pad[i * 192] = h_pad[count * 192 + i * 96] = 0x40;  // the identity of G2 / of G1
    k.upload_owned(g2_tail, h_pad, count * 192, "pad copy");
    k.upload_owned(g1_tail, h_pad + count * 192, count * 96, "pad copy");
  }
  // key_idx for BadGroups::named_keys: a bad key fails the groups of the records that NAME it, so the indices are needed on the
  // host only then, and only then does device I/O read them back (8 R bytes and one sync)
  const uint64_t* host_key_idx(const uint8_t* h_vkey) {  // h_vkey: the K verdicts of the key table, or null
    if (!key_idx || !k.c->device_io || !tc::has_zero(h_vkey, K)) return key_idx;
    const uint64_t* h_kidx = k.fetch(key_idx, R, "index readback");
    k.wait();
    return h_kidx;
  }
};

// Batch verification of ragged input: M messages, message m owning the records rec_off[m] .. rec_off[m + 1],
// record r = (sigs[r], pks[key_idx[r]]).  Groups of `group` consecutive messages pass with ONE product check
//     prod_{m in g} e(P_m, H_m) == e(g1, S_g),  P_m = sum_{r in m} rho_r pk_r (G1),  S_g = sum_{r in g} rho_r sig_r (G2)
// -- the two ragged sums of k_msm.hip (k_rec_*) over the 63-bit scalars of k_rlc_scalars, then launch_pairing_product_check with
// one pair per message; a group that fails, holds an operand that does not decode or (checked-input mode) is no member, is
// re-checked record by record on compacted operands like the failed messages of tc_verify_shares_rlc_batch.
static int verify_records(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* sigs, const uint64_t* rec_off,
                          const uint8_t* hashes, const uint8_t* msgs, const uint64_t* off, size_t M, size_t group, const uint8_t* seed32,
                          uint8_t* ok, uint64_t* n_fallback) {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (M == 0) return TC_OK;
  TC_REQUIRE(ctx && rec_off && (hashes || off) && seed32);
  Call k(ctx);
  Records f(k, pks, K, key_idx, M, group);  // groups of MESSAGES
  if (!f.offsets(rec_off, sigs, ok)) return k.finish();
  group = f.cut.group;
  const size_t R = f.R, NG = f.cut.NG, simd_lanes = f.simd_lanes;  // NG = tc::rec_groups(M, group)
  uint64_t total = 0;
  if (!hashes) {
    if (!total_bytes(k, off, M, &total)) return k.finish();
    TC_REQUIRE(total == 0 || msgs);
  }
  // the segments of the sums: messages (G1); in G2 the PIECES of the groups (tc_records.h: a group of many records would leave
  // the GPU to a few waves), then, when a group has several, the groups as segments over the sums of their pieces.  One
  // descriptor array: [rec_off | chunks of the messages | first records of the pieces | their chunks | first pieces of the
  // groups | their chunks]
  const size_t pairs_most = (size_t)tc::kBlock / tc::kG2Lanes;
  const uint64_t piece = tc::rec_piece_size(R, simd_lanes / tc::kG2Lanes, pairs_most);
  const size_t NP = (size_t)tc::rec_piece_total(f.h_grp.data(), NG, piece);
  const size_t desc_words = 2 * (M + 1) + 2 * (NP + 1) + 2 * (NG + 1);
  uint64_t *h_seg1 = k.host<uint64_t>(desc_words), *h_fc1 = h_seg1 + M + 1, *h_seg2 = h_fc1 + M + 1, *h_fc2 = h_seg2 + NP + 1, *h_seg3 = h_fc2 + NP + 1,
           *h_fc3 = h_seg3 + NG + 1;
  memcpy(h_seg1, f.hr, (M + 1) * 8);
  const uint64_t C1 = tc::rec_chunk_ranges(h_seg1, M, h_fc1);
  tc::rec_piece_ranges(f.h_grp.data(), NG, piece, h_seg2, h_seg3);
  const uint64_t C2 = tc::rec_chunk_ranges(h_seg2, NP, h_fc2);
  const uint64_t C3 = tc::rec_chunk_ranges(h_seg3, NG, h_fc3);
  uint64_t longest2 = 0, longest3 = 0;
  for (size_t q = 0; q < NP; q++) longest2 = h_seg2[q + 1] - h_seg2[q] > longest2 ? h_seg2[q + 1] - h_seg2[q] : longest2;
  for (size_t g = 0; g < NG; g++) longest3 = h_seg3[g + 1] - h_seg3[g] > longest3 ? h_seg3[g + 1] - h_seg3[g] : longest3;
  bool direct = true;  // every group is exactly one piece: the sums of the pieces ARE the sums of the groups
  for (size_t g = 0; g < NG; g++) direct = direct && h_seg3[g + 1] - h_seg3[g] == 1;
  const size_t forced = ctx->tuning.records_parts, forced2 = forced > pairs_most ? pairs_most : forced;
  const size_t parts1 = tc::rec_parts(M, f.longest, simd_lanes, tc::kBlock, forced);
  const size_t parts2 = tc::rec_parts(NP, longest2, simd_lanes / tc::kG2Lanes, pairs_most, forced2);
  const size_t parts3 = tc::rec_parts(NG, longest3, simd_lanes / tc::kG2Lanes, pairs_most, forced2);
  if (!f.tables_fit(tc::rec_table_bytes(false, C1) + tc::rec_table_bytes(true, C2) + tc::rec_table_bytes(true, C3))) return k.finish();
  f.stage_keys();
  const uint8_t* d_sig = k.in(sigs, R * 192);
  const uint8_t* d_hash_in = hashes ? k.in(hashes, M * 192) : nullptr;
  const uint8_t* d_msgs = hashes ? nullptr : k.in(msgs, (size_t)total);
  const uint64_t* d_off = hashes ? nullptr : k.in(off, M + 1);
  // the pairs of the product checks: `group` per group, the last group filled up with identity pairs (the factor 1), so that
  // ONE launch checks every group (a launch of one job takes as long as a launch of a thousand)
  const size_t MP = NG * group;
  uint8_t* d_hash = k.temp<uint8_t>(MP * 192);
  const uint8_t* d_g1 = hashes ? ctx->g1_gen : ctx->g1_gen_unfix;
  uint64_t* d_desc = k.temp<uint64_t>(desc_words);
  uint8_t* d_seed = k.secret_seed(seed32);
  uint8_t* d_r = k.secret_temp<uint8_t>(R * 32);
  uint8_t* d_P = k.temp<uint8_t>(MP * 96);
  uint8_t* d_S = k.temp<uint8_t>(NG * 192);
  uint8_t* d_Sp = direct ? d_S : k.temp<uint8_t>(NP * 192);  // the sums of the pieces
  uint8_t* d_ones = k.temp<uint8_t>(NP * 32);
  uint8_t* d_st = k.temp<uint8_t>(M + NG + NP);  // messages | groups | pieces
  uint8_t* d_okg = k.temp<uint8_t>(NG);
  int32_t* d_tbl1 = k.temp<int32_t>(tc::rec_table_bytes(false, C1) / sizeof(int32_t));
  int32_t* d_tbl2 = k.temp<int32_t>(tc::rec_table_bytes(true, C2) / sizeof(int32_t));
  int32_t* d_tbl3 = k.temp<int32_t>(tc::rec_table_bytes(true, C3) / sizeof(int32_t));
  // (the digit codes are a lossless recoding of the secret scalars: wiped like them; the third sum's scalars are all 1)
  uint8_t* d_codes1 = k.secret_temp<uint8_t>(tc::rec_code_bytes(C1));
  uint8_t* d_codes2 = k.secret_temp<uint8_t>(tc::rec_code_bytes(C2));
  uint8_t* d_codes3 = k.temp<uint8_t>(tc::rec_code_bytes(C3));
  uint8_t* d_ok = k.out(ok, R);
  int32_t* ws_groups = k.pairing_product_ws(group, NG, true);
  k.begin_timing();
  // checked-input mode: every key TABLE entry once (K tests, not R), every signature, every hash operand
  const uint8_t* v_key = k.check_points(false, f.d_pk, 96, K, K, 1, (size_t)-1);
  const uint8_t* v_sig = k.check_points(true, d_sig, 192, 1, 1, R, 1);
  const uint8_t* v_hash = hashes ? k.check_points(true, d_hash_in, 192, 1, 1, M, 1) : nullptr;
  if (!k.failed) {
    k.upload_owned(d_desc, h_seg1, desc_words * 8, "descriptor copy");
    k.check(hipMemsetAsync(d_st, 0, M + NG + NP, ctx->stream), "memset");
    if (!hashes) tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, M, d_hash, /*fix=*/false);
    else k.check(hipMemcpyAsync(d_hash, d_hash_in, M * 192, hipMemcpyDeviceToDevice, ctx->stream), "hash copy");
    f.pad_identities(d_hash + M * 192, d_P + M * 96, MP - M);
    tc::launch_rlc_scalars(ctx->stream, d_seed, R, d_r);
    const uint32_t* rr = reinterpret_cast<const uint32_t*>(d_r);
    f.gather_keys();
    const uint64_t *d_seg1 = d_desc, *d_fc1 = d_seg1 + M + 1, *d_seg2 = d_fc1 + M + 1, *d_fc2 = d_seg2 + NP + 1, *d_seg3 = d_fc2 + NP + 1,
                   *d_fc3 = d_seg3 + NG + 1;
    // (the short-scalar modes of the two-stage kernels: 40 two-half steps in G1, 16 columns in G2, as tc_ciphertext_verify_rlc_batch)
    tc::launch_rec_sum_g1(ctx->stream, f.d_keys, rr, d_seg1, d_fc1, M, C1, parts1, d_tbl1, d_codes1, d_P, d_st, /*nbits=*/80);
    tc::launch_rec_sum_g2(ctx->stream, d_sig, rr, d_seg2, d_fc2, NP, C2, parts2, d_tbl2, d_codes2, d_Sp, d_st + M + NG, /*nbits=*/16);
    // S_g = the sum of the group's pieces: the same kernels over the piece sums with the scalar 1 (short and odd).  A group
    // without records has no piece: its sum is the identity.
    if (!direct) {
      k.check(hipMemsetAsync(d_ones, 0, NP * 32, ctx->stream), "memset");
      k.check(hipMemset2DAsync(d_ones, 32, 1, 1, NP, ctx->stream), "memset");
      tc::launch_rec_sum_g2(ctx->stream, d_Sp, reinterpret_cast<const uint32_t*>(d_ones), d_seg3, d_fc3, NG, C3, parts3, d_tbl3, d_codes3, d_S,
                            d_st + M, 16);
    }
    // one pair per message (an empty message: P_m = identity, the factor 1), one final exponentiation per group
    tc::launch_pairing_product_check(ctx->stream, d_P, 96, d_hash, 192, group, NG, d_g1, 0, d_S, 192, d_okg, ws_groups);
    k.check(hipMemsetAsync(d_ok, 1, R, ctx->stream), "memset");
    const uint8_t* h_okg = k.fetch(d_okg, NG, "ok readback");
    const uint8_t* h_st = k.fetch(d_st, M + NG + NP, "status readback");
    // (the membership tests ran beside the sums and the group checks)
    const uint8_t *h_vkey, *h_vsig, *h_vhash;
    k.take_verdicts({{v_key, &h_vkey}, {v_sig, &h_vsig}, {v_hash, &h_vhash}});
    tc::SlotMaps maps;  // every record of the messages of the bad groups
    if (k.wait()) {
      tc::BadGroups bad(f.cut, M);
      bad.per_group(h_okg, true);
      bad.per_group(h_st + M, false);           // the sums of the groups,
      bad.spans(h_seg3, h_st + M + NG, false);  // of their pieces
      bad.jobs({h_st}, false);                  // and of their messages
      bad.jobs({h_vhash}, true);
      bad.spans(f.h_grp.data(), h_vsig, true);
      bad.named_keys(f.h_grp.data(), f.host_key_idx(h_vkey), K, h_vkey);
      maps = tc::records_of_jobs(f.hr, bad.failed_jobs());
    }
    if (!k.failed && !maps.record.empty()) {
      // the per-record check of tc_verify_g2_batch for every record of the failed groups, on compacted operands
      const size_t F = maps.record.size();
      Compacted c(k, F, std::move(maps.record), std::move(maps.job));
      const uint8_t* c_sig = c.gather(d_sig, 192, 0);
      const uint8_t* c_hash = c.gather(d_hash, 192, 1);
      const uint8_t* c_pk = c.gather(f.d_keys, 96, 0);
      const tc::PairingWs pws = k.pairing_ws(F);
      if (!k.failed) tc::launch_pairing_check(ctx->stream, c_pk, 96, c_hash, 192, d_g1, 0, c_sig, 192, F, c.c_ok, pws);  // src/lib.rs:109
      if (ctx->input_checks) {  // members only, as the per-record path would require
        c.members(false, c_pk, 96);
        c.members(true, c_sig, 192);
        if (hashes) c.members(true, c_hash, 192);
      }
      c.finish(d_ok, 0);
      if (n_fallback) *n_fallback = F;
    }
  }
  k.end_timing();
  return k.finish();
}

int tc_verify_g2_records_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* sigs,
                                   const uint64_t* rec_off, const uint8_t* hashes, size_t M, size_t group, const uint8_t* seed32, uint8_t* ok,
                                   uint64_t* n_fallback) try {
  if (ctx && M && !hashes) {
    ctx->err = "invalid argument: hashes";
    return TC_ERR_INVALID_ARG;
  }
  return verify_records(ctx, pks, K, key_idx, sigs, rec_off, hashes, nullptr, nullptr, M, group, seed32, ok, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_verify_sig_records_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* sigs,
                                    const uint64_t* rec_off, const uint8_t* msgs, const uint64_t* off, size_t M, size_t group,
                                    const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  if (ctx && M && !off) {
    ctx->err = "invalid argument: off";
    return TC_ERR_INVALID_ARG;
  }
  return verify_records(ctx, pks, K, key_idx, sigs, rec_off, nullptr, msgs, off, M, group, seed32, ok, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_ciphertext_verify_batch(tc_ctx* ctx, const uint8_t* u, const uint8_t* v, const uint64_t* off,
                               const uint8_t* w, size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && u && off && w && ok);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || v);
  const uint8_t* d_u = k.in(u, B * 96);
  const uint8_t* d_v = k.in(v, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  const uint8_t* d_w = k.in(w, B * 192);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  k.check_points(false, d_u, 96, 1, 1, B, 1);
  k.check_points(true, d_w, 192, 1, 1, B, 1);
  if (!k.failed) {
    // an undecodable u leaves an infinity hash; the pairing kernel then rejects u itself
    tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, B, d_hash, nullptr, /*fix=*/false);
    // e(g1, w) == e(u, [c] Q')  <=>  e([1/c] g1, w) == e(u, Q')         (src/lib.rs:511)
    tc::launch_pairing_check(ctx->stream, ctx->g1_gen_unfix, 0, d_w, 192, d_u, 96, d_hash, 192, B, d_ok, k.pairing_ws(B));
  }
  k.apply_checks(B, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Ciphertext::verify (src/lib.rs:508-512) for a batch by random linear combination, opt-in: the batch is cut into groups of
// `group` ciphertexts, and a group passes with ONE product check
//     e(g1, sum_j r_j w_j) == prod_j e(r_j u_j, H_j)          (H_j = hash_g1_g2(u_j, v_j); bilinearity; r_j secret)
// -- `group` pairs, two per Miller loop, and ONE final exponentiation instead of `group` checks of two pairs each.  u_j and
// H_j both differ per ciphertext, so nothing folds into a group sum on that side: the SAME r_j multiplies u_j in G1 and
// enters the sum over w_j in G2.  The scalars are k_rlc_scalars' (k_check.hip): d0 + d1 |x| + d2 |x|^2 + d3 |x|^3 with four
// 16-bit digits, d0 odd -- 2^63 values, pairwise distinct mod r, so for members of G1 / G2 a group holding an invalid
// ciphertext passes with probability <= 2^-63.  That shape keeps the G2 sum (per point the dearer of the two ladders: Fq2
// arithmetic on a lane pair, one table of psi-images per w_j) in its 16-column mode; in G1 the same value is
// (d0 + d1 |x|) + (d2 + d3 |x|) x^2, two 80-bit halves: the short-scalar mode of k_msm_*_g1 with 40 base-4 steps instead of 64.
// (k_rlc_scalars_g1's a + b x^2 would give G1 16 steps and G2 32 columns of 4 additions per chunk: more Fq2 additions than
// the G1 steps it saves -- an operation count, NOT a measurement; msm_g1 with one point per job also fills three of the four
// places of its chunk with the identity.)  A group that fails -- or whose sums report an error, or that holds an undecodable or, in
// checked-input mode, non-member operand -- is re-checked ciphertext by ciphertext, so ok[] equals
// tc_ciphertext_verify_batch's up to that 2^-63.
int tc_ciphertext_verify_rlc_batch(tc_ctx* ctx, const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w, size_t B,
                                   size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && u && off && w && seed32 && ok);
  TC_REQUIRE(B < (1ull << 32));
  const tc::GroupCut cut = tc::group_cut(B, group);
  group = cut.group;
  const size_t G = cut.G, tail = cut.tail, NG = cut.NG;
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || v);
  const uint8_t* d_u = k.in(u, B * 96);
  const uint8_t* d_v = k.in(v, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  const uint8_t* d_w = k.in(w, B * 192);
  uint8_t* d_seed = k.secret_seed(seed32);
  uint8_t* d_r = k.secret_temp<uint8_t>(B * 32);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_ru = k.temp<uint8_t>(B * 96);     // r_j u_j
  uint8_t* d_W = k.temp<uint8_t>(NG * 192);    // sum_j r_j w_j per group
  uint8_t* d_st = k.temp<uint8_t>(2 * B + NG); // hash | r_j u_j | group sums
  uint8_t* d_okg = k.temp<uint8_t>(NG);
  uint8_t* d_ok = k.out(ok, B);
  int32_t* ws_groups = G ? k.pairing_product_ws(group, G, true) : nullptr;
  int32_t* ws_tail = tail ? k.pairing_product_ws(tail, 1, true) : nullptr;
  k.begin_timing();
  const uint8_t* v_u = k.check_points(false, d_u, 96, 1, 1, B, 1);
  const uint8_t* v_w = k.check_points(true, d_w, 192, 1, 1, B, 1);
  if (!k.failed) {
    k.check(hipMemsetAsync(d_st, 0, 2 * B + NG, ctx->stream), "memset");
    // an undecodable u leaves a hash that does not decode either (and a status): its group falls back
    tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, B, d_hash, d_st, /*fix=*/false);
    tc::launch_rlc_scalars(ctx->stream, d_seed, B, d_r);
    const uint32_t* rr = reinterpret_cast<const uint32_t*>(d_r);
    msm_g1(k, 1, 96, d_u, rr, B, d_ru, d_st + B, /*nbits=*/80, /*secret_scalars=*/true);
    if (G) msm_g2(k, group, group * 192, d_w, rr, G, d_W, d_st + 2 * B, /*nbits=*/16, tc::MsmFilter(), /*secret_scalars=*/true);
    if (tail) msm_g2(k, tail, tail * 192, d_w + G * group * 192, rr + G * group * 8, 1, d_W + G * 192, d_st + 2 * B + G, 16, tc::MsmFilter(), true);
    // prod_j e(r_j u_j, [c] Q'_j) == e(g1, W)  <=>  prod_j e(r_j u_j, Q'_j) == e([1/c] g1, W)   (the folded hash constant of
    // tc_ciphertext_verify_batch)
    if (G) tc::launch_pairing_product_check(ctx->stream, d_ru, 96, d_hash, 192, group, G, ctx->g1_gen_unfix, 0, d_W, 192, d_okg, ws_groups);
    if (tail)
      tc::launch_pairing_product_check(ctx->stream, d_ru + G * group * 96, 96, d_hash + G * group * 192, 192, tail, 1, ctx->g1_gen_unfix, 0,
                                       d_W + G * 192, 192, d_okg + G, ws_tail);
    k.check(hipMemsetAsync(d_ok, 1, B, ctx->stream), "memset");
    const uint8_t* h_okg = k.fetch(d_okg, NG, "ok readback");
    const uint8_t* h_st = k.fetch(d_st, 2 * B + NG, "status readback");
    // checked-input mode: a group that owns a non-member operand goes to the per-ciphertext path as well
    // (the membership tests ran beside the sums and the group checks)
    const uint8_t *h_vu, *h_vw;
    k.take_verdicts({{v_u, &h_vu}, {v_w, &h_vw}});
    std::vector<uint32_t> failed;
    if (k.wait()) {
      tc::BadGroups bad(cut, B);
      bad.per_group(h_okg, true);
      bad.per_group(h_st + 2 * B, false);      // the sums of the groups
      bad.jobs({h_st, h_st + B}, false);       // the hashes and r_j u_j
      bad.jobs({h_vu, h_vw}, true);
      failed = bad.failed_jobs();
    }
    if (!k.failed && !failed.empty()) {
      // the per-ciphertext check of tc_ciphertext_verify_batch for every ciphertext of the failed groups, on compacted operands
      const size_t R = failed.size();
      Compacted c(k, R, std::move(failed));
      const uint8_t* c_u = c.gather(d_u, 96, 0);
      const uint8_t* c_hash = c.gather(d_hash, 192, 0);
      const uint8_t* c_w = c.gather(d_w, 192, 0);
      const tc::PairingWs pws = k.pairing_ws(R);
      if (!k.failed) tc::launch_pairing_check(ctx->stream, ctx->g1_gen_unfix, 0, c_w, 192, c_u, 96, c_hash, 192, R, c.c_ok, pws);  // src/lib.rs:511
      if (ctx->input_checks) {  // members only, as the per-ciphertext path would require
        c.members(false, c_u, 96);
        c.members(true, c_w, 192);
      }
      c.finish(d_ok, 0);
      if (n_fallback) *n_fallback = R;
    }
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Ciphertext::verify, then [sk] u for the ciphertexts that pass: SecretKeyShare::decrypt_share (src/lib.rs:452-457) when
// plain == nullptr, SecretKey::decrypt (src/lib.rs:384-391: the same, then xor_with_hash) otherwise
static int verified_decrypt(tc_ctx* ctx, const uint8_t* sk, const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w,
                            size_t B, uint8_t* out_g1, uint8_t* plain, uint8_t* ok, bool plain_unbacked = false) {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && sk && u && off && w && ok && (out_g1 || plain));
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || (v && !plain_unbacked));
  const uint8_t* d_sk = k.in(sk, 32, /*secret=*/true);
  const uint8_t* d_u = k.in(u, B * 96);
  const uint8_t* d_v = k.in(v, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  const uint8_t* d_w = k.in(w, B * 192);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_ok = k.out(ok, B);
  uint8_t* d_st = k.temp<uint8_t>(B, /*zero=*/true);
  uint8_t* d_pt = plain ? k.temp<uint8_t>(B * 96) : k.out(out_g1, B * 96);
  uint8_t* d_plain = plain ? k.out(plain, (size_t)total, /*zero=*/true) : nullptr;
  if (plain) k.secret(d_pt, B * 96, /*after_copy=*/true);  // g = [sk] u opens the ciphertext: not left in a staging slot
  k.begin_timing();
  // ALWAYS, whatever tc_ctx_set_input_checks says: the pairing check cannot see a small-order component of u
  // (u = u1 + T, T in E(Fq)[h1]: e(u, H) = e(u1, H)), and [sk] u would leak sk modulo the cofactor's small factors.  The
  // reference cannot reach that state: Ciphertext deserialisation always runs the subgroup test (src/lib.rs:140-146).
  k.check_points(false, d_u, 96, 1, 1, B, 1, /*always=*/true);
  k.check_points(true, d_w, 192, 1, 1, B, 1, /*always=*/true);
  if (!k.failed) {
    tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, B, d_hash, nullptr, /*fix=*/false);
    tc::launch_pairing_check(ctx->stream, ctx->g1_gen_unfix, 0, d_w, 192, d_u, 96, d_hash, 192, B, d_ok, k.pairing_ws(B));  // src/lib.rs:511
    k.apply_checks(B, nullptr, nullptr, 0, d_ok);
    tc::launch_g1_mul(ctx->stream, k.tables(), d_sk, d_u, 1, B, d_pt, d_st);
    // a multiplication that reported an error (a non-canonical secret key: >= r) is not a decryption: ok = 0, like the
    // reference, which cannot hold such an Fr
    tc::launch_ok_and_status(ctx->stream, d_st, B, d_ok);
    // `if !ct.verify() { return None; }` (src/lib.rs:385, 453): a ciphertext that fails the check gets the identity, never [sk] u
    tc::launch_invalidate_jobs(ctx->stream, d_ok, 1, 1, B, d_st, d_pt, 96, nullptr);
    if (plain) tc::launch_xor_with_hash(ctx->stream, d_pt, d_v, d_off, B, d_plain, d_st);  // skips flagged jobs: zeros
  }
  k.end_timing();
  return k.finish();
}

int tc_decrypt_share_batch(tc_ctx* ctx, const uint8_t* sk_fr, const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w,
                           size_t B, uint8_t* out_g1, uint8_t* ok) try {
  TC_REQUIRE(ctx && (B == 0 || out_g1));
  return verified_decrypt(ctx, sk_fr, u, v, off, w, B, out_g1, nullptr, ok);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// The same for n selected holders per ciphertext: Ciphertext::verify (the hash + pairing check of verified_decrypt) ONCE per
// ciphertext, then the n shares by decrypt_shares_mul.  ok[j] is the verdict on ciphertext j; a holder's own failure (index >= N,
// scalar >= r) is reported in its status byte and leaves ok[j] alone.
int tc_decrypt_shares_batch(tc_ctx* ctx, const uint8_t* sk_table, size_t N, const uint64_t* idx, const uint8_t* u, const uint8_t* v,
                            const uint64_t* off, const uint8_t* w, size_t n, size_t B, uint8_t* out, uint8_t* ok, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (n == 0 || B == 0) return TC_OK;
  TC_REQUIRE(ctx && sk_table && idx && u && off && w && out && ok && N > 0);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || v);
  const uint8_t* d_sk = k.in(sk_table, N * 32, /*secret=*/true);
  const uint64_t* d_idx = k.in(idx, B * n);
  const uint8_t* d_u = k.in(u, B * 96);
  const uint8_t* d_v = k.in(v, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  const uint8_t* d_w = k.in(w, B * 192);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_ok = k.out(ok, B);
  uint8_t* d_out = k.out(out, B * n * 96);
  uint8_t* d_st = status ? k.out(status, B * n) : k.temp<uint8_t>(B * n);
  k.begin_timing();
  // ALWAYS, as in verified_decrypt: [sk] u for a u with a small-order component would leak sk modulo the cofactor's factors
  k.check_points(false, d_u, 96, 1, 1, B, 1, /*always=*/true);
  k.check_points(true, d_w, 192, 1, 1, B, 1, /*always=*/true);
  if (!k.failed) {
    tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, B, d_hash, nullptr, /*fix=*/false);
    tc::launch_pairing_check(ctx->stream, ctx->g1_gen_unfix, 0, d_w, 192, d_u, 96, d_hash, 192, B, d_ok, k.pairing_ws(B));  // src/lib.rs:511
    k.apply_checks(B, nullptr, nullptr, 0, d_ok);
    decrypt_shares_mul(k, d_sk, N, d_idx, d_u, n, B, d_out, d_st);
    // `if !ct.verify() { return None; }` (src/lib.rs:453): a ciphertext that fails the check gets n identities, never [sk] u
    if (!k.failed) tc::launch_invalidate_jobs(ctx->stream, d_ok, 1, n, B * n, d_st, d_out, 96, nullptr);
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_secret_key_decrypt_batch(tc_ctx* ctx, const uint8_t* sk_fr, const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w,
                                size_t B, uint8_t* out, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  const bool unbacked = out == nullptr;  // (all-empty plaintexts, device-resident: see g_no_plaintext_bytes)
  if (unbacked) out = &g_no_plaintext_bytes;
  return verified_decrypt(ctx, sk_fr, u, v, off, w, B, nullptr, out, ok, unbacked);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_verify_decryption_share_batch(tc_ctx* ctx, const uint8_t* pk_share, size_t pk_stride, const uint8_t* share,
                                     const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w,
                                     size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && pk_share && share && u && off && w && ok);
  TC_REQUIRE(pk_stride == 0 || pk_stride >= 96);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || v);
  const uint8_t* d_pk = k.in(pk_share, pk_stride ? (B - 1) * pk_stride + 96 : 96);
  const uint8_t* d_share = k.in(share, B * 96);
  const uint8_t* d_u = k.in(u, B * 96);
  const uint8_t* d_v = k.in(v, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  const uint8_t* d_w = k.in(w, B * 192);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_st = k.temp<uint8_t>(B);
  uint8_t* d_sharec = k.temp<uint8_t>(B * 96);
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  k.check_points(false, d_pk, pk_stride, 1, 1, B, 1);
  k.check_points(false, d_share, 96, 1, 1, B, 1);
  k.check_points(false, d_u, 96, 1, 1, B, 1);
  k.check_points(true, d_w, 192, 1, 1, B, 1);
  if (!k.failed) {
    tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, B, d_hash, d_st, /*fix=*/false);
    tc::launch_g1_scale_cofactor_fix(ctx->stream, d_share, 96, B, d_sharec);
    // e(share, hash) = e([c] share, Q') == e(pk_share, w)               (src/lib.rs:185)
    tc::launch_pairing_check(ctx->stream, d_sharec, 96, d_hash, 192, d_pk, pk_stride, d_w, 192, B, d_ok, k.pairing_ws(B));
  }
  k.apply_checks(B, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Decryption-share validation by ONE random linear combination per ciphertext (opt-in fast path of the loop of
// examples/threshold_enc.rs over PublicKeyShare::verify_decryption_share, src/lib.rs:182-186): instead of N checks
// e(share_i, H) == e(pk_i, w) per ciphertext (H = hash_g1_g2(u, v)) the device checks
//     e(sum_i r_i share_i, H) == e(sum_i r_i pk_i, w)
// with secret r_i = a_i + b_i x^2 (2^63 values; a 16-step ladder through phi); ciphertexts whose combined check fails are
// re-checked share by share, so ok[] equals the per-share path's up to 2^-63.
int tc_verify_decryption_shares_rlc_batch(tc_ctx* ctx, const uint8_t* pk_shares, size_t N, const uint8_t* shares, const uint8_t* u,
                                          const uint8_t* v, const uint64_t* off, const uint8_t* w, size_t B, const uint8_t* seed32,
                                          uint8_t* ok, uint64_t* n_fallback) try {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0 || N == 0) return TC_OK;
  TC_REQUIRE(ctx && pk_shares && shares && u && off && w && seed32 && ok);
  TC_REQUIRE(B * N < (1ull << 32));
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || v);
  const uint8_t* d_pk = k.in(pk_shares, N * 96);
  const uint8_t* d_sh = k.in(shares, B * N * 96);
  const uint8_t* d_u = k.in(u, B * 96);
  const uint8_t* d_v = k.in(v, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  const uint8_t* d_w = k.in(w, B * 192);
  uint8_t* d_seed = k.secret_seed(seed32);
  uint8_t* d_r = k.secret_temp<uint8_t>(B * N * 32);
  uint8_t* d_hash = k.temp<uint8_t>(B * 192);
  uint8_t* d_D = k.temp<uint8_t>(B * 96);
  uint8_t* d_Dc = k.temp<uint8_t>(B * 96);
  uint8_t* d_P = k.temp<uint8_t>(B * 96);
  uint8_t* d_st = k.temp<uint8_t>(3 * B);
  uint8_t* d_okct = k.temp<uint8_t>(B);
  uint8_t* d_ok = k.out(ok, B * N);
  k.begin_timing();
  k.check_points(false, d_pk, 96, N, N, 1, (size_t)-1);
  k.check_points(false, d_sh, 96, N, N, B, 1);
  k.check_points(false, d_u, 96, 1, 1, B, 1);
  k.check_points(true, d_w, 192, 1, 1, B, 1);
  if (!k.failed) {
    tc::launch_rlc_scalars_g1(ctx->stream, d_seed, B * N, d_r);
    k.check(hipMemsetAsync(d_st, 0, 3 * B, ctx->stream), "memset");
    const uint32_t* rr = reinterpret_cast<const uint32_t*>(d_r);
    msm_g1(k, N, N * 96, d_sh, rr, B, d_D, d_st, /*nbits=*/32, /*secret_scalars=*/true);
    msm_g1(k, N, 0, d_pk, rr, B, d_P, d_st + B, 32, true);   // the N key shares are the same for every ciphertext: one table set
    tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, B, d_hash, d_st + 2 * B, /*fix=*/false);
    tc::launch_g1_scale_cofactor_fix(ctx->stream, d_D, 96, B, d_Dc);
    // e(D, [c] Q') = e([c] D, Q') == e(P, w)      (the folded hash constant of tc_verify_decryption_share_batch)
    tc::launch_pairing_check(ctx->stream, d_Dc, 96, d_hash, 192, d_P, 96, d_w, 192, B, d_okct, k.pairing_ws(B));
    k.apply_checks(B, nullptr, nullptr, 0, d_okct);  // checked-input mode: a ciphertext owning a non-member operand falls back
    k.check(hipMemsetAsync(d_ok, 1, B * N, ctx->stream), "memset");
    const uint8_t* h_okct = k.fetch(d_okct, B, "ok readback");
    const uint8_t* h_st = k.fetch(d_st, 3 * B, "status readback");
    std::vector<uint32_t> failed;
    if (k.wait())
      for (size_t j = 0; j < B; j++)
        if (!h_okct[j] || h_st[j] != TC_JOB_OK || h_st[B + j] != TC_JOB_OK || h_st[2 * B + j] != TC_JOB_OK) failed.push_back((uint32_t)j);
    if (!k.failed && !failed.empty()) {
      // per-share pairing checks for every share of the failed ciphertexts, on compacted operands
      const size_t F = failed.size(), R = F * N;
      tc::SlotMaps m = tc::slot_maps(failed.data(), F, N);
      Compacted c(k, R, std::move(m.record), std::move(m.job), std::move(m.slot));
      const uint8_t* c_sh = c.gather(d_sh, 96, 0);
      const uint8_t* c_hash = c.gather(d_hash, 192, 1);
      const uint8_t* c_w = c.gather(d_w, 192, 1);
      const uint8_t* c_pk = c.gather(d_pk, 96, 2);
      uint8_t* c_shc = k.temp<uint8_t>(R * 96);
      const tc::PairingWs pws = k.pairing_ws(R);
      if (!k.failed) {
        // e([c] share, Q') == e(pk, w), the cofactor constant on the share side as in the combined check above
        tc::launch_g1_scale_cofactor_fix(ctx->stream, c_sh, 96, R, c_shc);
        tc::launch_pairing_check(ctx->stream, c_shc, 96, c_hash, 192, c_pk, 96, c_w, 192, R, c.c_ok, pws);
      }
      if (ctx->input_checks) {  // members only, as the per-share path would require
        c.members(false, c_sh, 96);
        c.members(false, c_pk, 96);
        c.members(true, c_w, 192);
        // ... and u, which tc_verify_decryption_share_batch checks too (an on-curve u outside G1 used to
        // reach the bare pairing result here)
        c.members(false, c.gather(d_u, 96, 1), 96);
      }
      c.finish(d_ok, 0);
      if (n_fallback) *n_fallback = F;
    }
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Batch verification of ragged decryption shares: M ciphertexts, ciphertext c owning the records rec_off[c] ..
// rec_off[c + 1], record r = (shares[r], pks[key_idx[r]]).  Groups of `group` consecutive ciphertexts pass with ONE product check
//     prod_{c in g} e(A_c, H_c) e(-B_c, w_c) == 1,  A_c = sum_{r in c} rho_r share_r,  B_c = sum_{r in c} rho_r pk_r  (both G1)
// -- both ragged sums from ONE launch per stage (k_msm.hip k_rec_*_g1_pair) over the 63-bit scalars of k_rlc_scalars_g1, written
// straight into the interleaved operands [A_c, -B_c] of launch_pairing_product_check, two pairs per ciphertext, against [H_c, w_c].
// H_c is the FIXED hash (fix = true), so the hashing and the pre-hashed entry share every step behind it and no cofactor scaling
// stands between the sums and the check.  A group that fails, holds an operand that does not decode or (checked-input mode) is
// no member, is re-checked record by record on compacted operands like the failed ciphertexts of
// tc_verify_decryption_shares_rlc_batch.
static int verify_dshare_records(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* shares, const uint64_t* rec_off,
                                 const uint8_t* hashes, const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w, size_t M,
                                 size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (M == 0) return TC_OK;
  TC_REQUIRE(ctx && rec_off && (hashes || (u && off)) && w && seed32);
  Call k(ctx);
  Records f(k, pks, K, key_idx, M, group);  // groups of CIPHERTEXTS
  if (!f.offsets(rec_off, shares, ok)) return k.finish();
  group = f.cut.group;
  const size_t R = f.R, NG = f.cut.NG;
  uint64_t total = 0;
  if (!hashes) {
    if (!total_bytes(k, off, M, &total)) return k.finish();
    TC_REQUIRE(total == 0 || v);
  }
  // the segments of both sums: the ciphertexts.  One descriptor array: [rec_off | chunks of the ciphertexts]
  const size_t desc_words = 2 * (M + 1);
  uint64_t *h_seg = k.host<uint64_t>(desc_words), *h_fc = h_seg + M + 1;
  memcpy(h_seg, f.hr, (M + 1) * 8);
  const uint64_t C = tc::rec_chunk_ranges(h_seg, M, h_fc);
  const size_t parts = tc::rec_parts(2 * M, f.longest, f.simd_lanes, tc::kBlock, ctx->tuning.records_parts);  // lanes per SUM, two sums per ciphertext
  const size_t table_bytes = tc::rec_table_bytes(false, 2 * C);
  if (!f.tables_fit(table_bytes)) return k.finish();
  f.stage_keys();
  const uint8_t* d_sh = k.in(shares, R * 96);
  const uint8_t* d_hash_in = hashes ? k.in(hashes, M * 192) : nullptr;
  const uint8_t* d_u = hashes ? nullptr : k.in(u, M * 96);
  const uint8_t* d_v = hashes ? nullptr : k.in(v, (size_t)total);
  const uint64_t* d_off = hashes ? nullptr : k.in(off, M + 1);
  const uint8_t* d_w = k.in(w, M * 192);
  // the pairs of the product checks: 2 * group per group, the last group filled up with identity pairs (the factor 1), so that
  // ONE launch checks every group
  const size_t MP = NG * group;
  uint8_t* d_hash_own = hashes ? nullptr : k.temp<uint8_t>(M * 192);
  const uint8_t* d_hash = hashes ? d_hash_in : d_hash_own;
  uint8_t* d_ab = k.temp<uint8_t>(MP * 2 * 96);   // [A_c, -B_c]
  uint8_t* d_hw = k.temp<uint8_t>(MP * 2 * 192);  // [H_c, w_c]
  uint64_t* d_desc = k.temp<uint64_t>(desc_words);
  uint8_t* d_seed = k.secret_seed(seed32);
  uint8_t* d_r = k.secret_temp<uint8_t>(R * 32);
  uint8_t* d_st = k.temp<uint8_t>(2 * M);  // the sums of the ciphertexts | their hashes
  uint8_t* d_okg = k.temp<uint8_t>(NG);
  int32_t* d_tbl = k.temp<int32_t>(table_bytes / sizeof(int32_t));
  // (the digit codes are a lossless recoding of the secret scalars: wiped like them)
  uint8_t* d_codes = k.secret_temp<uint8_t>(tc::rec_code_bytes(2 * C));
  uint8_t* d_ok = k.out(ok, R);
  int32_t* ws_groups = k.pairing_product_ws(2 * group, NG, false);
  k.begin_timing();
  // checked-input mode: every key TABLE entry once (K tests, not R), every share, every u (or hash) and every w
  const uint8_t* v_key = k.check_points(false, f.d_pk, 96, K, K, 1, (size_t)-1);
  const uint8_t* v_sh = k.check_points(false, d_sh, 96, 1, 1, R, 1);
  const uint8_t* v_u = hashes ? k.check_points(true, d_hash_in, 192, 1, 1, M, 1) : k.check_points(false, d_u, 96, 1, 1, M, 1);
  const uint8_t* v_w = k.check_points(true, d_w, 192, 1, 1, M, 1);
  if (!k.failed) {
    k.upload_owned(d_desc, h_seg, desc_words * 8, "descriptor copy");
    k.check(hipMemsetAsync(d_st, 0, 2 * M, ctx->stream), "memset");
    if (!hashes) tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_v, d_off, M, d_hash_own, d_st + M, /*fix=*/true);
    k.check(hipMemcpy2DAsync(d_hw, 384, d_hash, 192, 192, M, hipMemcpyDeviceToDevice, ctx->stream), "hash copy");
    k.check(hipMemcpy2DAsync(d_hw + 192, 384, d_w, 192, 192, M, hipMemcpyDeviceToDevice, ctx->stream), "w copy");
    f.pad_identities(d_hw + M * 384, d_ab + M * 192, 2 * (MP - M));
    tc::launch_rlc_scalars_g1(ctx->stream, d_seed, R, d_r);
    f.gather_keys();
    const uint64_t *d_seg = d_desc, *d_fc = d_seg + M + 1;
    // (the short-scalar mode of the G1 two-stage kernels: 16 two-half steps, as tc_verify_decryption_shares_rlc_batch)
    tc::launch_rec_sum_g1_pair(ctx->stream, d_sh, f.d_keys, reinterpret_cast<const uint32_t*>(d_r), d_seg, d_fc, M, C, parts, d_tbl, d_codes, d_ab,
                               d_st, /*nbits=*/32);
    // two pairs per ciphertext (one lane pair of the Miller stage; an empty ciphertext: both sums the identity, the factor 1),
    // one final exponentiation per group                                                          (src/lib.rs:185)
    tc::launch_pairing_product_check(ctx->stream, d_ab, 96, d_hw, 192, 2 * group, NG, nullptr, 0, nullptr, 0, d_okg, ws_groups);
    k.check(hipMemsetAsync(d_ok, 1, R, ctx->stream), "memset");
    const uint8_t* h_okg = k.fetch(d_okg, NG, "ok readback");
    const uint8_t* h_st = k.fetch(d_st, 2 * M, "status readback");
    // (the membership tests ran beside the sums and the group checks)
    const uint8_t *h_vkey, *h_vsh, *h_vu, *h_vw;
    k.take_verdicts({{v_key, &h_vkey}, {v_sh, &h_vsh}, {v_u, &h_vu}, {v_w, &h_vw}});
    tc::SlotMaps maps;  // every record of the ciphertexts of the bad groups
    if (k.wait()) {
      tc::BadGroups bad(f.cut, M);
      bad.per_group(h_okg, true);
      bad.jobs({h_st, h_st + M}, false);  // the sums of the ciphertexts and their hashes
      bad.jobs({h_vu, h_vw}, true);
      bad.spans(f.h_grp.data(), h_vsh, true);
      bad.named_keys(f.h_grp.data(), f.host_key_idx(h_vkey), K, h_vkey);
      maps = tc::records_of_jobs(f.hr, bad.failed_jobs());
    }
    if (!k.failed && !maps.record.empty()) {
      // the per-record check of tc_verify_decryption_share_batch for every record of the failed groups, on compacted operands
      const size_t F = maps.record.size();
      // (the fixed hash of an undecodable u is the identity, which a pairing check would SKIP: the per-record path sees an
      // encoding that does not decode there and answers 0 -- so do these records)
      for (size_t m = 0; m < M && !hashes && !k.failed; m++)
        if (h_st[M + m] != TC_JOB_OK) k.check(hipMemsetAsync(d_hash_own + m * 192, 0xff, 192, ctx->stream), "memset");
      Compacted c(k, F, std::move(maps.record), std::move(maps.job));
      const uint8_t* c_sh = c.gather(d_sh, 96, 0);
      const uint8_t* c_pk = c.gather(f.d_keys, 96, 0);
      const uint8_t* c_hash = c.gather(d_hash, 192, 1);
      const uint8_t* c_w = c.gather(d_w, 192, 1);
      const tc::PairingWs pws = k.pairing_ws(F);
      // e(share, H) == e(pk, w)                                                                     (src/lib.rs:185)
      if (!k.failed) tc::launch_pairing_check(ctx->stream, c_sh, 96, c_hash, 192, c_pk, 96, c_w, 192, F, c.c_ok, pws);
      if (ctx->input_checks) {  // members only, as the per-record path would require
        c.members(false, c_sh, 96);
        c.members(false, c_pk, 96);
        c.members(true, c_w, 192);
        if (hashes) c.members(true, c_hash, 192);
        else c.members(false, c.gather(d_u, 96, 1), 96);
      }
      c.finish(d_ok, 0);
      if (n_fallback) *n_fallback = F;
    }
  }
  k.end_timing();
  return k.finish();
}

// PublicKeyShare::verify_decryption_share (src/lib.rs:182-186) over ragged records, the loop of examples/threshold_enc.rs:
// ok[r] for every received (key, share) record of every ciphertext, one final exponentiation per group of ciphertexts
int tc_verify_decryption_share_records_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx, const uint8_t* shares,
                                                 const uint64_t* rec_off, const uint8_t* u, const uint8_t* v, const uint64_t* off, const uint8_t* w,
                                                 size_t M, size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  if (ctx && M && !(u && off)) {
    ctx->err = "invalid argument: u, off";
    return TC_ERR_INVALID_ARG;
  }
  return verify_dshare_records(ctx, pks, K, key_idx, shares, rec_off, nullptr, u, v, off, w, M, group, seed32, ok, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// the same with hashes[c] = hash_g1_g2(u_c, v_c) made by the caller (tc_hash_g1_g2_batch): src/lib.rs:182-186 with its hash at
// hand, the loop of examples/threshold_enc.rs
int tc_verify_decryption_share_records_prehashed_rlc_batch(tc_ctx* ctx, const uint8_t* pks, size_t K, const uint64_t* key_idx,
                                                           const uint8_t* shares, const uint64_t* rec_off, const uint8_t* hashes, const uint8_t* w,
                                                           size_t M, size_t group, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  if (ctx && M && !hashes) {
    ctx->err = "invalid argument: hashes";
    return TC_ERR_INVALID_ARG;
  }
  return verify_dshare_records(ctx, pks, K, key_idx, shares, rec_off, hashes, nullptr, nullptr, nullptr, w, M, group, seed32, ok, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Pass 2 of robust_combine by bisection (tc_ctx_set_blame_bisect; rule, bounds and the 2^-63 argument: tc_blame.h, DESIGN.md
// 4.17): the returned bytes (memory of the frame) h_ok[f * N + i] = 0 exactly for the present shares of the failed jobs that per-share mode would answer ok = 0 for,
// found with range checks over leaves [r] share / [r] pk_share (k_blame.hip).  c_sh: the failed jobs' shares, uncompressed
// (F x N); c_dec: the status bytes of their checked decode (wire) or null; d_maps: the record / job maps of pass 2.  The host
// drives the rounds -- one batched pairing-check launch and one readback of verdict bytes each -- and builds the worklists
// (tc::BlameSearch, one per job).  The leaves of F x N slots take F N (576 B signatures / 384 B decryption): failed jobs
// go through in chunks under the budget the two-stage tables have (msm_table_budget; TC_MSM_BUDGET).  The engine knows
// nothing of the entry: the RLC fallbacks could drive it the same way.
static const uint8_t* blame_pass(Call& k, bool sig, bool wire, size_t N, const uint32_t* failed, size_t F, const uint32_t* d_maps, const uint8_t* c_sh,
                                 const uint8_t* c_dec, const uint8_t* d_present, const uint8_t* d_jvalid, const uint8_t* d_pks, const uint8_t* d_hash,
                                 const uint8_t* d_w, const uint8_t* d_g1) {
  tc_ctx* ctx = k.c;
  const size_t R = F * N, PB = sig ? 192 : 96;
  uint8_t* h_ok = k.host<uint8_t>(R);
  memset(h_ok, 1, R);
  uint8_t* c_pres = k.temp<uint8_t>(R);
  uint8_t* c_live = k.temp<uint8_t>(R);
  uint8_t* c_v = k.temp<uint8_t>(R);
  uint8_t* d_key = k.secret_temp<uint8_t>(32);
  uint8_t* d_seed = k.secret_temp<uint8_t>(32);
  const size_t leaf_s = tc::blame_leaf_bytes(sig), leaf_pk = tc::blame_leaf_bytes(false);
  size_t Fc = msm_table_budget(k) / (N * (leaf_s + leaf_pk));
  if (Fc < 1) Fc = 1;
  if (Fc > F) Fc = F;
  int32_t* d_leaf_s = k.temp<int32_t>(Fc * N * leaf_s / sizeof(int32_t));
  int32_t* d_leaf_pk = k.temp<int32_t>(Fc * N * leaf_pk / sizeof(int32_t));
  int32_t* d_sink = k.temp<int32_t>(tc::blame_sink_bytes() / sizeof(int32_t));
  const tc::TableArena ta = k.tables();
  if (k.failed) return h_ok;
  // live = present, decoded, a group member where that is tested, and the job's own operands valid
  if (d_present) tc::launch_gather_bytes(ctx->stream, d_present, d_maps, R, c_pres);
  else k.check(hipMemsetAsync(c_pres, 1, R, ctx->stream), "memset");
  k.check(hipMemcpyAsync(c_live, c_pres, R, hipMemcpyDeviceToDevice, ctx->stream), "live copy");
  if (wire) {
    tc::launch_ok_and_status(ctx->stream, c_dec, R, c_live);  // (the checked decode has tested membership)
  } else if (ctx->input_checks) {
    k.require_members(sig, c_sh, PB, R, c_v, c_live);
  }
  tc::launch_gather_bytes(ctx->stream, d_jvalid, d_maps + R, R, c_v);
  tc::launch_invalidate_jobs(ctx->stream, c_v, 1, 1, R, nullptr, nullptr, 0, c_live);
  // this call's scalars: ChaCha20 under a seed of its own, derived from the context's key and call counter
  k.upload(d_key, ctx->blame_key, 32, "key copy");
  tc::launch_blame_seed(ctx->stream, d_key, ctx->blame_calls++, d_seed);
  // memory of the frame, reused chunk after chunk and round after round (each ends with wait()): Fc * N bytes hold a chunk's
  // present / live bytes, and the items and verdicts of a round, which grow when a round has more ranges than the last
  uint8_t *h_pres = k.host<uint8_t>(Fc * N), *h_live = k.host<uint8_t>(Fc * N), *h_verdict = nullptr;
  uint32_t* items = nullptr;
  size_t items_room = 0;
  std::vector<uint8_t> h_bad;
  std::vector<tc::BlameSearch> search;
  std::vector<tc::BlameRange> ranges;
  std::vector<uint32_t> counts;
  for (size_t f0 = 0; f0 < F && !k.failed; f0 += Fc) {
    const size_t cnt = (F - f0 < Fc) ? F - f0 : Fc, rows = cnt * N;
    // (the share leaves first: a share that does not decode clears its live byte, and its key share's leaf is the identity too)
    tc::launch_blame_leaves(ctx->stream, ta, sig, d_seed, (uint64_t)(f0 * N), c_sh + f0 * N * PB, 0, c_live + f0 * N, rows, d_leaf_s, d_sink);
    tc::launch_blame_leaves(ctx->stream, ta, false, d_seed, (uint64_t)(f0 * N), d_pks, N, c_live + f0 * N, rows, d_leaf_pk, d_sink);
    h_bad.assign(rows, 0);
    k.fetch_into(h_pres, c_pres + f0 * N, rows, "present readback");
    k.fetch_into(h_live, c_live + f0 * N, rows, "live readback");
    if (!k.wait()) break;
    search.assign(cnt, tc::BlameSearch());
    for (size_t f = 0; f < cnt; f++) search[f].start((uint32_t)N, h_pres + f * N, h_live + f * N, h_bad.data() + f * N);
    while (!k.failed) {
      // one round: the pending checks of every job of the chunk in ONE launch
      ranges.clear();
      counts.assign(cnt, 0);
      for (size_t f = 0; f < cnt; f++) counts[f] = (uint32_t)search[f].plan(ranges);
      const size_t n = ranges.size();
      if (n == 0) break;
      if (n > items_room) {
        items = k.host<uint32_t>(4 * n);  // job of the chunk, lo, hi, job of the call
        h_verdict = k.host<uint8_t>(n);
        items_room = n;
      }
      size_t longest = 1;
      for (size_t f = 0, i = 0; f < cnt; f++)
        for (uint32_t c = 0; c < counts[f]; c++, i++) {
          items[i] = (uint32_t)f;
          items[n + i] = ranges[i].lo;
          items[2 * n + i] = ranges[i].hi;
          items[3 * n + i] = failed[f0 + f];
          if (ranges[i].hi - ranges[i].lo > longest) longest = ranges[i].hi - ranges[i].lo;
        }
      const Call::SlotScope round(k);  // the round's buffers are the next round's: it ends with wait()
      uint32_t* d_items = k.temp<uint32_t>(4 * n);
      uint8_t* s_sh = k.temp<uint8_t>(n * PB);
      uint8_t* s_shc = sig ? nullptr : k.temp<uint8_t>(n * 96);
      uint8_t* s_pk = k.temp<uint8_t>(n * 96);
      uint8_t* s_hash = k.temp<uint8_t>(n * 192);
      uint8_t* s_w = sig ? nullptr : k.temp<uint8_t>(n * 192);
      uint8_t* s_ok = k.temp<uint8_t>(n);
      const tc::PairingWs pws = k.pairing_ws(n);
      if (k.failed) break;
      k.upload_owned(d_items, items, 16 * n, "item copy");
      tc::launch_blame_range_sum(ctx->stream, sig, d_leaf_s, N, d_items, d_items + n, d_items + 2 * n, n, tc::blame_sum_parts(sig, n, longest, ctx->cus), s_sh);
      tc::launch_blame_range_sum(ctx->stream, false, d_leaf_pk, N, d_items, d_items + n, d_items + 2 * n, n, tc::blame_sum_parts(false, n, longest, ctx->cus),
                                 s_pk);
      tc::launch_gather_rows(ctx->stream, d_hash, 192, d_items + 3 * n, n, s_hash);
      if (sig) {
        // e(sum r_i pk_i, H) == e(g1, sum r_i sig_i)
        tc::launch_pairing_check(ctx->stream, s_pk, 96, s_hash, 192, d_g1, 0, s_sh, 192, n, s_ok, pws);
      } else {
        // e([c] sum r_i share_i, H') == e(sum r_i pk_i, w), the cofactor constant on the share side as in the per-share check
        tc::launch_gather_rows(ctx->stream, d_w, 192, d_items + 3 * n, n, s_w);
        tc::launch_g1_scale_cofactor_fix(ctx->stream, s_sh, 96, n, s_shc);
        tc::launch_pairing_check(ctx->stream, s_shc, 96, s_hash, 192, s_pk, 96, s_w, 192, n, s_ok, pws);
      }
      k.fetch_into(h_verdict, s_ok, n, "verdict readback");
      if (!k.wait()) break;
      for (size_t f = 0, i = 0; f < cnt; i += counts[f], f++) search[f].apply(h_verdict + i);
      ctx->blame_rounds++;
    }
    for (size_t f = 0; f < cnt; f++) ctx->blame_checks += search[f].checks;
    for (size_t r = 0; r < rows; r++) h_ok[f0 * N + r] = h_bad[r] ? 0 : 1;
  }
  return h_ok;
}

// ---- robust combination ------------------------------------------------------------------------------
// What a node runs per message: of up to N shares, some absent and some possibly forged, combine the first t+1 VALID ones and
// name the senders of bad ones -- the loop of examples/threshold_sig.rs:115-131 followed by combine_signatures
// (src/lib.rs:608-615), or the loop of examples/threshold_enc.rs followed by PublicKeySet::decrypt (src/lib.rs:618-626) --
// optimistically.  Pass 1 combines the first t+1 PRESENT shares of every job and checks the combination under the master key
// commit[0]; a BLS signature (a decryption share sum) is unique, so a combination that verifies is the answer and none of its
// shares needs a check of its own.  Only the jobs whose combination does not stand go through pass 2: every present share
// checked under its public key share, the first t+1 valid ones combined.  Selection, gather and re-selection run on the
// device (k_robust.hip); the host sees B verdict bytes between the passes and builds the job maps of pass 2, as the other
// combined entries do.  sig: G2 shares against hash points (hashes, or msgs / off hashed here); otherwise G1 decryption shares
// against the ciphertexts (u, msgs = v, off, w) and the plaintexts as output.
//
// wire: the shares are the COMPRESSED wire forms (96 / 48 bytes, always checked: from_bytes src/lib.rs:246-252, 140-146) and a
// signature leaves compressed.  Pass 1 decodes only the t+1 selected shares, straight out of the caller's array and only as far
// as the curve (k_decompress_selected); membership is tested ONCE per job, on the combination: a point of the order-r subgroup
// that satisfies the pairing equation under commit[0] is THE signature (THE sk u) whatever it was combined from.  A
// combination that is off the curve, outside the subgroup or does not verify sends its job to pass 2, where every present
// share goes through the full checked decode and its own pairing check.
static int robust_combine(tc_ctx* ctx, bool sig, bool wire, const uint8_t* commit, size_t t, size_t N, const uint8_t* present, const uint8_t* shares,
                          const uint8_t* hashes, const uint8_t* msgs, const uint64_t* off, const uint8_t* u, const uint8_t* w, size_t B,
                          size_t group, const uint8_t* seed32, uint8_t* out, bool out_unbacked, uint8_t* used, uint8_t* bad, uint8_t* status,
                          uint64_t* n_fallback) {
  TC_REQUIRE(ctx);
  ctx->blame_checks = ctx->blame_rounds = 0;
  if (n_fallback) *n_fallback = 0;
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && commit && shares && out && status);
  TC_REQUIRE(t < (1u << 20));
  TC_REQUIRE(t + 1 <= N);
  TC_REQUIRE(N < (1ull << 32) && B < (1ull << 32) && B * N < (1ull << 32));
  if (sig) TC_REQUIRE(seed32 && ((hashes != nullptr) != (off != nullptr)));
  else TC_REQUIRE(u && off && w);
  const size_t PB = sig ? 192 : 96, need = t + 1;
  const size_t SB = wire ? PB / 2 : PB;  // bytes per share in the caller's array
  Call k(ctx);
  uint64_t total = 0;
  if (off) {
    if (!total_bytes(k, off, B, &total)) return k.finish();
    TC_REQUIRE(total == 0 || msgs);
    TC_REQUIRE(sig || total == 0 || !out_unbacked);
  }
  const uint8_t* d_commit = k.in(commit, need * 96);
  const uint8_t* d_present = k.in(present, B * N);
  const uint8_t* d_sh = k.in(shares, B * N * SB);
  // (pass 2 expands the failed jobs' shares to the uncompressed form: guard_private sees the size the uncompressed entry has)
  if (wire) k.operand_bytes += B * N * SB;
  // (pass 2 by bisection multiplies the key share of every examined slot as well: lanes of its own, priced like an operand)
  const bool bisect = ctx->blame_bisect;
  if (bisect) k.operand_bytes += B * N * 96;
  const uint8_t* d_hash_in = hashes ? k.in(hashes, B * 192) : nullptr;
  const uint8_t* d_msgs = off ? k.in(msgs, (size_t)total) : nullptr;
  const uint64_t* d_off = off ? k.in(off, B + 1) : nullptr;
  const uint8_t* d_u = sig ? nullptr : k.in(u, B * 96);
  const uint8_t* d_w = sig ? nullptr : k.in(w, B * 192);
  uint8_t* d_status = k.out(status, B);
  uint8_t* d_used = k.out(used, B * N, /*zero=*/true);
  uint8_t* d_bad = k.out(bad, B * N, /*zero=*/true);
  // the point result: the caller's signatures, or the G1 value the plaintext is masked with
  // (wire signatures: compressed into the caller's B x 96 at the end)
  uint8_t* d_res = sig && !wire ? k.out(out, B * 192) : k.temp<uint8_t>(B * PB);
  uint8_t* d_out96 = sig && wire ? k.out(out, B * 96) : nullptr;
  uint8_t* d_plain = sig ? nullptr : k.out(out, (size_t)total, /*zero=*/true);  // failed jobs leave zeros
  // the N public key shares, made once per call: Commitment::evaluate(i + 1), src/lib.rs:570-573
  uint64_t* h_slots = k.host<uint64_t>(N);
  for (size_t i = 0; i < N; i++) h_slots[i] = i;
  uint64_t* d_pkidx = k.temp<uint64_t>(N);
  uint8_t* d_pks = k.temp<uint8_t>(N * 96);
  uint8_t* d_pkst = k.temp<uint8_t>(N, /*zero=*/true);
  uint8_t* d_cval = k.temp<uint8_t>(need);
  uint64_t* d_idx = k.temp<uint64_t>(B * need);
  uint32_t* d_slot = k.temp<uint32_t>(B * need);
  uint8_t* d_enough = k.temp<uint8_t>(B);
  uint8_t* d_packed = k.temp<uint8_t>(B * need * PB);
  uint8_t* d_comb = k.temp<uint8_t>(B * PB);
  uint8_t* d_combc = sig ? nullptr : k.temp<uint8_t>(B * 96);
  uint8_t* d_st1 = k.temp<uint8_t>(B, /*zero=*/true);
  uint8_t* d_ok1 = k.temp<uint8_t>(B);
  // what k_robust_finish requires of every selected share: membership (checked-input mode), or -- wire -- that it decoded
  uint8_t* d_member = (wire || ctx->input_checks) ? k.temp<uint8_t>(B * need) : nullptr;
  uint8_t* d_cmem = wire ? k.temp<uint8_t>(B) : nullptr;  // wire: the combination is on the curve and in the subgroup
  uint8_t* d_hash_chk = wire && sig ? k.temp<uint8_t>(B * 192) : nullptr;
  uint8_t* d_verdict = k.temp<uint8_t>(B);
  uint8_t* d_hash_own = hashes ? nullptr : k.temp<uint8_t>(B * 192);
  const uint8_t* d_hash = hashes ? d_hash_in : d_hash_own;
  // hash points made here lack their last constant multiplication: the generator side carries it (tc_verify_sig_batch)
  const uint8_t* d_g1 = hashes ? ctx->g1_gen : ctx->g1_gen_unfix;
  // what a job's own operands allow: 0 when its hash point / ciphertext is undecodable or, in checked-input mode, no group
  // member -- every check of that job then fails, as tc_verify_g2_batch / tc_verify_decryption_share_batch answer ok = 0
  uint8_t* d_jvalid = k.temp<uint8_t>(B);
  uint8_t* d_jtmp = k.temp<uint8_t>(B);
  RlcWs ws{};
  if (sig) ws = rlc_workspace(k, B, group, seed32);
  k.begin_timing();
  const uint8_t *h_verdict = nullptr, *h_pkst = nullptr, *h_cval = nullptr;  // h_cval: checked-input mode only
  std::vector<uint32_t> failed;
  if (!k.failed) {
    k.upload_owned(d_pkidx, h_slots, N * 8, "index copy");
    tc::launch_commitment_evaluate(ctx->stream, d_commit, t, d_pkidx, N, d_pks, d_pkst);
    if (ctx->input_checks) tc::launch_subgroup_check_g1(ctx->stream, d_commit, 96, need, need, need, d_cval);
    // pass 1: the first t+1 present shares, whatever they are
    tc::launch_select_shares(ctx->stream, d_present, nullptr, N, need, B, nullptr, d_idx, d_slot, d_used, d_enough);
    if (wire) tc::launch_decompress_selected(ctx->tuning, ctx->stream, sig, d_sh, N, need, d_slot, d_enough, B, d_packed, d_member);
    else tc::launch_gather_selected(ctx->stream, d_sh, N, need, PB, d_slot, d_enough, B, d_packed);
    combine_launch(k, sig, t, need, d_idx, nullptr, d_packed, B, d_comb, d_st1);
    // membership of the selected shares goes into bytes of our own: a non-member share sends its job to pass 2 and ends as a
    // bad bit there, never as a failed job
    if (wire) {
      // ONE test per job, on the combination (decodes as a curve point, lies in the subgroup) instead of need per job.  A
      // combination that fails becomes the identity -- and, for signatures, so does the job's hash point in the copy the group
      // checks read: the job drops out of both sums of its group instead of sending the whole group to the per-job checks
      if (sig) tc::launch_subgroup_check_g2(ctx->stream, d_comb, PB, 1, 1, B, d_cmem);
      else tc::launch_subgroup_check_g1(ctx->stream, d_comb, PB, 1, 1, B, d_cmem);
      tc::launch_invalidate_jobs(ctx->stream, d_member, need, 1, B, nullptr, nullptr, 0, d_cmem);  // (an undecodable share: pass 2 as well)
      tc::launch_invalidate_jobs(ctx->stream, d_cmem, 1, 1, B, nullptr, d_comb, PB, nullptr);
    } else if (d_member) {
      if (sig) tc::launch_subgroup_check_g2(ctx->stream, d_packed, PB, need, need, B * need, d_member);
      else tc::launch_subgroup_check_g1(ctx->stream, d_packed, PB, need, need, B * need, d_member);
    }
    k.check(hipMemsetAsync(d_jvalid, 1, B, ctx->stream), "memset");
    if (sig) {
      if (hashes) {
        if (ctx->input_checks) k.require_members(true, d_hash, 192, B, d_jtmp, d_jvalid);
      } else {
        tc::launch_hash_g2(ctx->tuning, ctx->stream, d_msgs, d_off, B, d_hash_own, /*fix=*/false);
      }
      // the combinations under the ONE master key, by random linear combination: about one pairing check per `group` jobs
      const uint8_t* d_hash_rlc = d_hash;
      if (wire) {
        k.check(hipMemcpyAsync(d_hash_chk, d_hash, B * 192, hipMemcpyDeviceToDevice, ctx->stream), "hash copy");
        tc::launch_invalidate_jobs(ctx->stream, d_cmem, 1, 1, B, nullptr, d_hash_chk, 192, nullptr);
        d_hash_rlc = d_hash_chk;
      }
      rlc_group_checks(k, ws, d_commit, d_comb, d_hash_rlc, d_g1, B, nullptr, nullptr, nullptr, /*member_checks=*/false, /*hash_is_operand=*/false,
                       d_ok1, nullptr);
    } else {
      tc::launch_hash_g1_g2(ctx->tuning, ctx->stream, d_u, d_msgs, d_off, B, d_hash_own, d_jtmp, /*fix=*/false);
      tc::launch_ok_and_status(ctx->stream, d_jtmp, B, d_jvalid);
      if (ctx->input_checks) {
        k.require_members(false, d_u, 96, B, d_jtmp, d_jvalid);
        k.require_members(true, d_w, 192, B, d_jtmp, d_jvalid);
      }
      // verify_decryption_share of the COMBINATION under the master key: e(g, H) = e([c] g, Q') == e(commit[0], w)
      tc::launch_g1_scale_cofactor_fix(ctx->stream, d_comb, 96, B, d_combc);
      tc::launch_pairing_check(ctx->stream, d_combc, 96, d_hash, 192, d_commit, 0, d_w, 192, B, d_ok1, k.pairing_ws(B));
    }
    tc::launch_invalidate_jobs(ctx->stream, d_jvalid, 1, 1, B, nullptr, nullptr, 0, d_ok1);
    if (wire) tc::launch_invalidate_jobs(ctx->stream, d_cmem, 1, 1, B, nullptr, nullptr, 0, d_ok1);
    tc::launch_robust_finish(ctx->stream, nullptr, N, need, PB, B, d_enough, d_st1, d_ok1, d_member, d_comb, d_res, d_status, d_used, d_verdict);
    h_verdict = k.fetch(d_verdict, B, "verdict readback");
    h_pkst = k.fetch(d_pkst, N, "status readback");
    if (ctx->input_checks) h_cval = k.fetch(d_cval, need, "valid readback");
    k.wait();
  }
  bool commit_bad = false;
  if (!k.failed) {
    for (size_t i = 0; i < N; i++) commit_bad = commit_bad || h_pkst[i] != TC_JOB_OK;
    for (size_t i = 0; h_cval && i < need; i++) commit_bad = commit_bad || h_cval[i] == 0;
  }
  if (!k.failed && commit_bad) {
    // no key set, no verdict on anything: every job fails with INVALID_ENCODING and the identity, used = bad = 0
    k.check(hipMemsetAsync(d_status, TC_JOB_INVALID_ENCODING, B, ctx->stream), "memset");
    k.check(hipMemsetAsync(d_jvalid, 0, 1, ctx->stream), "memset");
    tc::launch_invalidate_jobs(ctx->stream, d_jvalid, 1, (size_t)-1, B, nullptr, d_res, PB, nullptr);
    if (d_used) k.check(hipMemsetAsync(d_used, 0, B * N, ctx->stream), "memset");
  } else if (!k.failed) {
    for (size_t j = 0; j < B; j++)
      if (h_verdict[j] == tc::kRobustRetry) failed.push_back((uint32_t)j);
  }
  if (!k.failed && !failed.empty()) {
    // pass 2: every share of the jobs whose combination did not stand, checked under its public key share on compacted
    // operands (PublicKeyShare::verify src/lib.rs:177-179 / verify_decryption_share :182-186); the verdict of an absent slot
    // is dropped by k_robust_mark
    const size_t F = failed.size(), R = F * N;
    tc::SlotMaps m = tc::slot_maps(failed.data(), F, N);
    Compacted c(k, R, std::move(m.record), std::move(m.job), std::move(m.slot), std::move(failed));
    const uint32_t *d_maps = c.map(0), *d_fmap = c.map(3);  // (record | job | slot maps, R entries each, then the F failed jobs)
    uint8_t* c_ok = c.c_ok;
    // wire: the full checked decode of from_bytes (curve AND subgroup); a failure leaves the identity -- decodable input for the
    // pairing kernel -- and its verdict goes into c_ok below
    const uint8_t* c_wire = wire ? c.gather(d_sh, SB, 0) : nullptr;
    uint8_t* c_dec = wire ? k.temp<uint8_t>(R) : nullptr;
    uint8_t* c_sh = wire ? k.temp<uint8_t>(R * PB) : c.gather(d_sh, PB, 0);
    uint8_t* c_present = k.temp<uint8_t>(R);
    uint8_t* c_bad = k.temp<uint8_t>(R);
    uint64_t* d_idx2 = k.temp<uint64_t>(F * need);
    uint32_t* d_slot2 = k.temp<uint32_t>(F * need);
    uint8_t* d_enough2 = k.temp<uint8_t>(F);
    uint8_t* d_packed2 = k.temp<uint8_t>(F * need * PB);
    uint8_t* d_comb2 = k.temp<uint8_t>(F * PB);
    uint8_t* d_st2 = k.temp<uint8_t>(F, /*zero=*/true);
    if (wire && !k.failed) {
      if (sig) tc::launch_g2_decompress(ctx->tuning, ctx->stream, c_wire, R, c_sh, c_dec);
      else tc::launch_g1_decompress(ctx->stream, c_wire, R, c_sh, c_dec);
    }
    if (bisect) {
      // which checks run is the ONLY difference: ranges of slots, halved where they fail (blame_pass), instead of every slot
      // (the verdicts come from the host's search)
      const uint8_t* h_ok = k.failed ? nullptr : blame_pass(k, sig, wire, N, c.host_map(3), F, d_maps, c_sh, c_dec, d_present, d_jvalid, d_pks, d_hash, d_w, d_g1);
      if (!k.failed) k.upload_owned(c_ok, h_ok, R, "verdict copy");
    } else {
      // (the per-share checks read one hash point / w / key share per record; the range checks of the bisection gather theirs per round)
      const uint8_t* c_hash = c.gather(d_hash, 192, 1);
      const uint8_t* c_pk = c.gather(d_pks, 96, 2);
      const uint8_t* c_w = sig ? nullptr : c.gather(d_w, 192, 1);
      uint8_t* c_shc = sig ? nullptr : k.temp<uint8_t>(R * 96);
      const tc::PairingWs pws = k.pairing_ws(R);
      if (!k.failed) {
        if (sig) {
          tc::launch_pairing_check(ctx->stream, c_pk, 96, c_hash, 192, d_g1, 0, c_sh, 192, R, c_ok, pws);
        } else {
          tc::launch_g1_scale_cofactor_fix(ctx->stream, c_sh, 96, R, c_shc);
          tc::launch_pairing_check(ctx->stream, c_shc, 96, c_hash, 192, c_pk, 96, c_w, 192, R, c_ok, pws);
        }
      }
      if (wire) {
        if (!k.failed) tc::launch_ok_and_status(ctx->stream, c_dec, R, c_ok);  // (the checked decode has tested membership)
      } else if (ctx->input_checks) {  // members only (the key shares are sums of the commitment's points, tested above)
        c.members(sig, c_sh, PB);
      }
      uint8_t* c_v = c.scratch();
      if (!k.failed) {
        tc::launch_gather_bytes(ctx->stream, d_jvalid, c.map(1), R, c_v);
        tc::launch_invalidate_jobs(ctx->stream, c_v, 1, 1, R, nullptr, nullptr, 0, c_ok);
        ctx->blame_checks = R;
        ctx->blame_rounds = 1;
      }
    }
    if (!k.failed) {
      tc::launch_robust_mark(ctx->stream, d_present, d_maps, c_ok, R, c_present, c_bad, d_bad);
      // the first t+1 VALID shares: their combination needs no further check
      tc::launch_select_shares(ctx->stream, c_present, c_bad, N, need, F, d_fmap, d_idx2, d_slot2, d_used, d_enough2);
      tc::launch_gather_selected(ctx->stream, c_sh, N, need, PB, d_slot2, d_enough2, F, d_packed2);
      combine_launch(k, sig, t, need, d_idx2, nullptr, d_packed2, F, d_comb2, d_st2);
      tc::launch_robust_finish(ctx->stream, d_fmap, N, need, PB, F, d_enough2, d_st2, nullptr, nullptr, d_comb2, d_res, d_status, d_used, nullptr);
    }
    if (n_fallback) *n_fallback = F;
  }
  // the plaintext of a job that ended OK: xor_with_hash(g, v), src/lib.rs:625
  if (!k.failed && !sig) tc::launch_xor_with_hash(ctx->stream, d_res, d_msgs, d_off, B, d_plain, d_status);
  // Signature::to_bytes of the results (the identity of a job that did not end OK: 0xC0, then zeros)
  if (!k.failed && d_out96) tc::launch_g2_compress(ctx->stream, d_res, B, d_out96, nullptr);
  k.end_timing();
  return k.finish();
}

int tc_combine_signatures_robust_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present,
                                       const uint8_t* sig_shares, const uint8_t* hashes, const uint8_t* msgs, const uint64_t* off, size_t B,
                                       size_t group, const uint8_t* seed32, uint8_t* out_sig, uint8_t* used, uint8_t* bad, uint8_t* status,
                                       uint64_t* n_fallback) try {
  return robust_combine(ctx, true, false, commit, t, N, present, sig_shares, hashes, msgs, off, nullptr, nullptr, B, group, seed32, out_sig, false, used, bad,
                        status, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_decrypt_robust_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present, const uint8_t* shares_g1,
                            const uint8_t* u_g1, const uint8_t* v, const uint64_t* off, const uint8_t* w_g2, size_t B, uint8_t* out_plain,
                            uint8_t* used, uint8_t* bad, uint8_t* status, uint64_t* n_fallback) try {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0) return TC_OK;  // (an empty batch is a no-op for every entry: a device-resident empty buffer has no address)
  const bool unbacked = out_plain == nullptr;
  if (unbacked) out_plain = &g_no_plaintext_bytes;
  return robust_combine(ctx, false, false, commit, t, N, present, shares_g1, nullptr, v, off, u_g1, w_g2, B, 0, nullptr, out_plain, unbacked, used, bad,
                        status, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_combine_signatures_robust_wire_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present,
                                            const uint8_t* sig_shares96, const uint8_t* hashes, const uint8_t* msgs, const uint64_t* off, size_t B,
                                            size_t group, const uint8_t* seed32, uint8_t* out_sig96, uint8_t* used, uint8_t* bad, uint8_t* status,
                                            uint64_t* n_fallback) try {
  return robust_combine(ctx, true, true, commit, t, N, present, sig_shares96, hashes, msgs, off, nullptr, nullptr, B, group, seed32, out_sig96, false,
                        used, bad, status, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_decrypt_robust_wire_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, size_t N, const uint8_t* present, const uint8_t* shares48,
                                 const uint8_t* u_g1, const uint8_t* v, const uint64_t* off, const uint8_t* w_g2, size_t B, uint8_t* out_plain,
                                 uint8_t* used, uint8_t* bad, uint8_t* status, uint64_t* n_fallback) try {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0) return TC_OK;
  const bool unbacked = out_plain == nullptr;
  if (unbacked) out_plain = &g_no_plaintext_bytes;
  return robust_combine(ctx, false, true, commit, t, N, present, shares48, nullptr, v, off, u_g1, w_g2, B, 0, nullptr, out_plain, unbacked, used, bad,
                        status, n_fallback);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- DKG algebra -----------------------------------------------------------------------------------
int tc_g1_commitment_batch(tc_ctx* ctx, const uint8_t* coeff_fr, size_t M, uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (M == 0) return TC_OK;
  TC_REQUIRE(ctx && coeff_fr && out);
  Call k(ctx);
  if (!ctx->fb_table && !k.failed) {
    if (k.check(hipMalloc((void**)&ctx->fb_table, tc::fixed_base_table_bytes()), "hipMalloc"))
      tc::launch_fixed_base_table(ctx->stream, ctx->fb_table);
    else
      ctx->fb_table = nullptr;
  }
  const uint8_t* d_fr = k.in(coeff_fr, M * 32, /*secret=*/true);
  uint8_t* d_out = k.out(out, M * 96);
  uint8_t* d_st = k.out(status, M);
  k.begin_timing();
  if (!k.failed) tc::launch_g1_fixed_base(ctx->stream, ctx->fb_table, d_fr, M, d_out, d_st, ctx->cus);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_bivar_commitment_row_batch(tc_ctx* ctx, const uint8_t* commit, size_t degree, const uint64_t* xs, size_t M, uint8_t* out,
                                  uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (M == 0) return TC_OK;
  TC_REQUIRE(ctx && commit && xs && out);
  TC_REQUIRE(degree < (1u << 16));
  const size_t ncoeff = (degree + 1) * (degree + 2) / 2;
  Call k(ctx);
  const uint8_t* d_c = k.in(commit, ncoeff * 96);
  const uint64_t* d_x = k.in(xs, M);
  uint8_t* d_out = k.out(out, M * (degree + 1) * 96);
  uint8_t* d_st = k.out(status, M * (degree + 1));
  k.begin_timing();
  k.check_points(false, d_c, 96, ncoeff, ncoeff, 1, (size_t)-1);
  if (!k.failed) tc::launch_bivar_commitment_row(ctx->stream, d_c, degree, d_x, M, d_out, d_st);
  k.apply_checks(M * (degree + 1), d_st, d_out, 96, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_fr_interpolate_batch(tc_ctx* ctx, size_t n, const uint8_t* xs, const uint8_t* ys, size_t B, uint8_t* out_coeff, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0 || n == 0) return TC_OK;
  TC_REQUIRE(ctx && xs && ys && out_coeff);
  TC_REQUIRE(n < (1u << 16));
  Call k(ctx);
  const uint8_t* d_x = k.in(xs, B * n * 32);
  const uint8_t* d_y = k.in(ys, B * n * 32, /*secret=*/true);
  uint8_t* d_out = k.out(out_coeff, B * n * 32);
  // host-I/O mode: the interpolated (secret) coefficients pass through a staging slot that outlives the call: wiped after
  // the copy back, like every other secret operand
  if (!ctx->device_io) k.secret(d_out, B * n * 32, /*after_copy=*/true);
  uint32_t* d_ws = k.temp<uint32_t>(B * 2 * (n + 1) * 8);
  k.secret(d_ws, B * 2 * (n + 1) * 8 * sizeof(uint32_t));
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed)
    tc::launch_fr_interpolate(ctx->stream, n, (const uint32_t*)d_x, (const uint32_t*)d_y, B, (uint32_t*)d_out, d_ws, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- DKG verification: the secret side and the two checks of distributed_key_generation (src/poly.rs:838-878) ----------
// the fixed-base window table of the G1 generator, built by the first call that multiplies by it
static void need_fixed_base_table(Call& k) {
  tc_ctx* ctx = k.c;
  if (ctx->fb_table || k.failed) return;
  if (k.check(hipMalloc((void**)&ctx->fb_table, tc::fixed_base_table_bytes()), "hipMalloc"))
    tc::launch_fixed_base_table(ctx->stream, ctx->fb_table);
  else
    ctx->fb_table = nullptr;
}

int tc_fr_poly_evaluate_batch(tc_ctx* ctx, const uint8_t* coeff_fr, size_t n, const uint8_t* xs_fr, size_t M, size_t B, uint8_t* out_fr,
                              uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0 || M == 0) return TC_OK;
  TC_REQUIRE(ctx && xs_fr && out_fr && (n == 0 || coeff_fr));
  TC_REQUIRE(n < (1u << 20) && B * M < (1ull << 40));
  Call k(ctx);
  const uint8_t* d_c = k.in(coeff_fr, B * n * 32, /*secret=*/true);
  const uint8_t* d_x = k.in(xs_fr, M * 32);
  uint8_t* d_out = k.out(out_fr, B * M * 32);
  // host-I/O mode: the (secret) values pass through a staging slot that outlives the call: wiped after the copy back
  if (!ctx->device_io) k.secret(d_out, B * M * 32, /*after_copy=*/true);
  uint8_t* d_st = k.out(status, B * M);
  uint32_t* d_mont = k.temp<uint32_t>(B * n * 8);
  k.secret(d_mont, B * n * 8 * sizeof(uint32_t));
  uint8_t* d_valid = k.temp<uint8_t>(B * n);
  k.begin_timing();
  if (!k.failed) {
    tc::launch_fr_to_mont(ctx->stream, d_c, B * n, d_mont, d_valid);
    tc::launch_fr_poly_evaluate(ctx->stream, d_mont, d_valid, n, d_x, M, B, d_out, d_st);
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_bivar_poly_row_batch(tc_ctx* ctx, const uint8_t* coeff_fr, size_t degree, const uint64_t* xs, size_t M, uint8_t* out_fr,
                            uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (M == 0) return TC_OK;
  TC_REQUIRE(ctx && coeff_fr && xs && out_fr);
  TC_REQUIRE(degree < (1u << 12));
  const size_t n = degree + 1, ncoeff = n * (n + 1) / 2;
  Call k(ctx);
  const uint8_t* d_c = k.in(coeff_fr, ncoeff * 32, /*secret=*/true);
  const uint64_t* d_x = k.in(xs, M);
  uint8_t* d_out = k.out(out_fr, M * n * 32);
  if (!ctx->device_io) k.secret(d_out, M * n * 32, /*after_copy=*/true);
  uint8_t* d_st = k.out(status, M * n);
  uint32_t* d_mont = k.temp<uint32_t>(n * n * 8);
  k.secret(d_mont, n * n * 8 * sizeof(uint32_t));
  uint8_t* d_valid = k.temp<uint8_t>(n * n);
  k.begin_timing();
  if (!k.failed) {
    tc::launch_bivar_to_mont(ctx->stream, d_c, degree, d_mont, d_valid);
    tc::launch_bivar_poly_row(ctx->stream, d_mont, d_valid, degree, d_x, M, d_out, d_st);
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_dkg_verify_rows_batch(tc_ctx* ctx, const uint8_t* commits, size_t commit_stride, size_t degree, const uint64_t* xs,
                             const uint8_t* row_fr, size_t B, uint8_t* out_rows, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && commits && xs && row_fr && ok);
  TC_REQUIRE(degree < (1u << 12));
  const size_t n = degree + 1, ncoeff = n * (n + 1) / 2;
  TC_REQUIRE(commit_stride == 0 || (commit_stride % 96 == 0 && commit_stride >= ncoeff * 96));
  TC_REQUIRE(B * n < (1ull << 32));
  Call k(ctx);
  need_fixed_base_table(k);
  const uint8_t* d_c = k.in(commits, commit_stride ? (B - 1) * commit_stride + ncoeff * 96 : ncoeff * 96);
  const uint64_t* d_x = k.in(xs, B);
  const uint8_t* d_row = k.in(row_fr, B * n * 32, /*secret=*/true);
  uint8_t* d_R = out_rows ? k.out(out_rows, B * n * 96) : k.temp<uint8_t>(B * n * 96);
  uint8_t* d_ok = k.out(ok, B);
  uint8_t* d_G = k.temp<uint8_t>(B * n * 96);
  uint8_t* d_st = k.temp<uint8_t>(2 * B * n);
  k.begin_timing();
  // (job j * n + i of the row kernel owns commitment j: `group` = n row points per record)
  if (commit_stride) k.check_points(false, d_c, 96, commit_stride / 96, ncoeff, B, n);
  else k.check_points(false, d_c, 96, ncoeff, ncoeff, 1, (size_t)-1);
  if (!k.failed) {
    tc::launch_bivar_commitment_row_jobs(ctx->stream, d_c, commit_stride, degree, d_x, B, d_R, d_st);
    tc::launch_g1_fixed_base(ctx->stream, ctx->fb_table, d_row, B * n, d_G, d_st + B * n, ctx->cus);
  }
  k.apply_checks(B * n, d_st, d_R, 96, nullptr);
  if (!k.failed) tc::launch_g1_equal(ctx->stream, d_R, d_st, d_G, d_st + B * n, n, B, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ok[j * n + k] = Commitment(rows[j]).evaluate(xs[j * n + k]) == vals[j * n + k] * g1 on device operands: the exact form, and the
// per-value pass of the combined form's failed jobs.  `checked`: the row points are tested for membership here (the compacted
// operands of a fallback; the exact entry registers its operands with Call::check_points instead)
static void dkg_values_exact(Call& k, const uint8_t* d_rows, size_t degree, const uint64_t* d_x, const uint8_t* d_vals, size_t n, size_t B,
                             uint8_t* d_ok, bool checked) {
  tc_ctx* ctx = k.c;
  const size_t V = B * n;
  uint8_t* d_E = k.temp<uint8_t>(V * 96);
  uint8_t* d_G = k.temp<uint8_t>(V * 96);
  uint8_t* d_st = k.temp<uint8_t>(2 * V);
  uint8_t* d_member = checked ? k.temp<uint8_t>(B * (degree + 1)) : nullptr;
  if (k.failed) return;
  tc::launch_commitment_evaluate_jobs(ctx->stream, d_rows, degree, d_x, n, B, d_E, d_st);
  tc::launch_g1_fixed_base(ctx->stream, ctx->fb_table, d_vals, V, d_G, d_st + V, ctx->cus);
  tc::launch_g1_equal(ctx->stream, d_E, d_st, d_G, d_st + V, 1, V, d_ok);
  if (checked) {
    tc::launch_subgroup_check_g1(ctx->stream, d_rows, 96, degree + 1, degree + 1, B * (degree + 1), d_member);
    tc::launch_invalidate_jobs(ctx->stream, d_member, degree + 1, n, V, nullptr, nullptr, 0, d_ok);
  }
}

int tc_dkg_verify_values_batch(tc_ctx* ctx, const uint8_t* rows, size_t degree, const uint64_t* xs, const uint8_t* vals_fr, size_t n,
                               size_t B, uint8_t* ok) try {
  TC_REQUIRE(ctx);
  if (B == 0 || n == 0) return TC_OK;
  TC_REQUIRE(ctx && rows && xs && vals_fr && ok);
  TC_REQUIRE(degree < (1u << 20) && B * n < (1ull << 32));
  Call k(ctx);
  need_fixed_base_table(k);
  const uint8_t* d_rows = k.in(rows, B * (degree + 1) * 96);
  const uint64_t* d_x = k.in(xs, B * n);
  const uint8_t* d_vals = k.in(vals_fr, B * n * 32, /*secret=*/true);
  uint8_t* d_ok = k.out(ok, B * n);
  k.begin_timing();
  k.check_points(false, d_rows, 96, degree + 1, degree + 1, B, n);  // value j * n + k owns row commitment j
  dkg_values_exact(k, d_rows, degree, d_x, d_vals, n, B, d_ok, /*checked=*/false);
  k.apply_checks(B * n, nullptr, nullptr, 0, d_ok);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// The n value checks of a part by ONE G1 linear combination of degree + 2 points (tc_dkg.h dkg_rlc_scalar): the scalars
// c_0 .. c_degree, c_g of every job, the points R_j || g1, the existing linear-combination kernels, an is-identity test; jobs
// that do not pass run the exact kernels on compacted operands, as the fallbacks of the other combined entries do.
int tc_dkg_verify_values_rlc_batch(tc_ctx* ctx, const uint8_t* rows, size_t degree, const uint64_t* xs, const uint8_t* vals_fr, size_t n,
                                   size_t B, const uint8_t* seed32, uint8_t* ok, uint64_t* n_fallback) try {
  TC_REQUIRE(ctx);
  if (n_fallback) *n_fallback = 0;
  if (B == 0 || n == 0) return TC_OK;
  TC_REQUIRE(ctx && rows && xs && vals_fr && seed32 && ok);
  TC_REQUIRE(degree < (1u << 20) && B * n < (1ull << 32) && B * (degree + 2) < (1ull << 32));
  const size_t np = degree + 2, row_bytes = (degree + 1) * 96;
  Call k(ctx);
  need_fixed_base_table(k);
  const uint8_t* d_rows = k.in(rows, B * row_bytes);
  const uint64_t* d_x = k.in(xs, B * n);
  const uint8_t* d_vals = k.in(vals_fr, B * n * 32, /*secret=*/true);
  uint8_t* d_seed = k.secret_seed(seed32);
  uint32_t* d_sc = k.secret_temp<uint32_t>(B * np * 8);
  uint8_t* d_pts = k.temp<uint8_t>(B * np * 96);
  uint8_t* d_sum = k.temp<uint8_t>(B * 96);
  uint8_t* d_st = k.temp<uint8_t>(B);
  uint8_t* d_valid = k.temp<uint8_t>(B);
  uint8_t* d_okjob = k.temp<uint8_t>(B);
  uint8_t* d_ok = k.out(ok, B * n);
  k.begin_timing();
  k.check_points(false, d_rows, 96, degree + 1, degree + 1, B, 1);
  if (!k.failed) {
    tc::launch_dkg_rlc_scalars(ctx->stream, d_seed, d_x, d_vals, n, degree, B, d_sc, d_valid);
    tc::launch_dkg_rlc_points(ctx->stream, d_rows, degree, ctx->g1_gen, B, d_pts);
    k.check(hipMemsetAsync(d_st, 0, B, ctx->stream), "memset");
    if (np >= tc::kMsmMinPoints) msm_g1(k, np, np * 96, d_pts, d_sc, B, d_sum, d_st, 128, /*secret_scalars=*/true);
    else tc::launch_lincomb_g1(ctx->stream, np, reinterpret_cast<const uint8_t*>(d_sc), d_pts, B, d_sum, d_st);
    tc::launch_g1_is_identity(ctx->stream, d_sum, d_st, d_valid, B, d_okjob);
    // checked-input mode: a job owning a non-member row point falls back (and fails there)
    k.apply_checks(B, nullptr, nullptr, 0, d_okjob);
    k.check(hipMemsetAsync(d_ok, 1, B * n, ctx->stream), "memset");
    const uint8_t* h_okjob = k.fetch(d_okjob, B, "ok readback");
    std::vector<uint32_t> failed;
    if (k.wait())
      for (size_t j = 0; j < B; j++)
        if (!h_okjob[j]) failed.push_back((uint32_t)j);
    if (!k.failed && !failed.empty()) {
      // the exact kernels for every value of the failed jobs, on compacted operands: whole rows gathered by job, the verdicts
      // scattered by value
      const size_t F = failed.size(), R = F * n;
      tc::SlotMaps m = tc::slot_maps(failed.data(), F, n);
      Compacted c(k, R, std::move(failed), std::move(m.record));
      const uint8_t* c_rows = c.gather(d_rows, row_bytes, 0);
      const uint64_t* c_x = reinterpret_cast<const uint64_t*>(c.gather(d_x, n * 8, 0));
      const uint8_t* c_vals = c.gather(d_vals, n * 32, 0, /*secret=*/true);
      if (!k.failed) dkg_values_exact(k, c_rows, degree, c_x, c_vals, n, F, c.c_ok, /*checked=*/ctx->input_checks);
      c.finish(d_ok, 1);
      if (n_fallback) *n_fallback = F;
    }
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- DKG finalisation: the accepted parts summed into the key set (src/poly.rs:870-876, 895-898) --------------------------
// out[j] = sum over the included terms of one point per term, on device operands.  Checked-input mode: Call::check_points
// marks by record and cannot express the mask, so the membership test runs here and the sum kernel reads its verdicts for the
// INCLUDED terms only (as dkg_values_exact(checked = true) does for its compacted operands).  column0: the terms are bivariate
// commitments and output j is coefficient (j, 0); the test then reads a compact copy of the first columns.
// (the membership half, shared with the weighted sums: the verdict bytes, n x B, or null with the checks off; a column0 operand
// is replaced by the compact copy of its first columns)
static const uint8_t* g1_sum_members(Call& k, bool& column0, const uint8_t*& d_pts, size_t& term_stride, size_t n, size_t B) {
  tc_ctx* ctx = k.c;
  if (!ctx->input_checks || !n) return nullptr;
  uint8_t* d_valid = k.temp<uint8_t>(n * B);
  uint8_t* d_col = column0 ? k.temp<uint8_t>(n * B * 96) : nullptr;
  if (k.failed) return nullptr;
  if (column0) {
    tc::launch_bivar_column0(ctx->stream, d_pts, term_stride, B - 1, n, d_col);
    d_pts = d_col;
    term_stride = B * 96;
    column0 = false;
  }
  tc::launch_subgroup_check_g1(ctx->stream, d_pts, 96, term_stride / 96, B, n * B, d_valid);
  return d_valid;
}
static void g1_sum(Call& k, bool column0, const uint8_t* d_pts, size_t term_stride, size_t n, const uint8_t* d_mask, size_t B, uint8_t* d_out,
                   uint8_t* d_st, uint8_t* d_term_bad) {
  tc_ctx* ctx = k.c;
  const uint8_t* d_member = g1_sum_members(k, column0, d_pts, term_stride, n, B);
  if (k.failed) return;
  tc::launch_g1_sum(ctx->stream, column0, d_pts, term_stride, n, d_mask, d_member, B, tc::g1_sum_parts(B, n, ctx->cus, ctx->tuning.sum_parts), d_out,
                    d_st, d_term_bad);
}
// the weighted form: d_w = n x 32 B weights, recoded once per term; d_member as g1_sum_members left it.  d_sel (may be null):
// n_sel term numbers, the only terms the sum visits
static void g1_wsum(Call& k, bool column0, const uint8_t* d_pts, size_t term_stride, size_t n, const uint8_t* d_w, const uint8_t* d_mask,
                    const uint8_t* d_member, size_t B, uint8_t* d_out, uint8_t* d_st, const uint32_t* d_sel = nullptr, size_t n_sel = 0) {
  tc_ctx* ctx = k.c;
  uint32_t* d_rec = k.temp<uint32_t>(n * tc::wsum_rec_words());
  if (k.failed) return;
  tc::launch_wsum_recode(ctx->stream, d_w, n, d_rec);
  const size_t visited = d_sel ? n_sel : n;
  const size_t parts = tc::g1_wsum_parts(B, visited, ctx->cus, ctx->tuning.sum_parts);
  const size_t slices = tc::g1_wsum_slices(B, visited, parts, ctx->cus, ctx->tuning.wsum_slices);
  if (slices <= 1) {
    tc::launch_g1_wsum(ctx->stream, column0, d_pts, term_stride, visited, d_rec, d_mask, d_member, B, parts, 1, d_out, d_st, nullptr, d_sel);
    return;
  }
  // a long sum: `slices` partial sums per output, each by its own lanes, then the plain sum of those
  uint8_t* d_partial = k.temp<uint8_t>(B * slices * 96);
  uint8_t* d_pok = k.temp<uint8_t>(B * slices);
  if (k.failed) return;
  tc::launch_g1_wsum(ctx->stream, column0, d_pts, term_stride, visited, d_rec, d_mask, d_member, B, parts, slices, d_partial, nullptr, d_pok, d_sel);
  tc::launch_g1_sum(ctx->stream, false, d_partial, B * 96, slices, nullptr, d_pok, B, tc::g1_sum_parts(B, slices, ctx->cus, 0), d_out, d_st, nullptr);
}

int tc_g1_sum_batch(tc_ctx* ctx, const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* mask, size_t B, uint8_t* out,
                    uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && out && (n == 0 || pts));
  TC_REQUIRE(n == 0 || (term_stride % 96 == 0 && term_stride / 96 >= B));
  TC_REQUIRE(B < (1ull << 26) && n < (1ull << 32) && B * n < (1ull << 40));
  Call k(ctx);
  const uint8_t* d_pts = k.in(pts, n ? (n - 1) * term_stride + B * 96 : 0);
  const uint8_t* d_mask = k.in(mask, n);
  uint8_t* d_out = k.out(out, B * 96);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  g1_sum(k, false, d_pts, term_stride, n, d_mask, B, d_out, d_st, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_bivar_commitment_row0_sum_batch(tc_ctx* ctx, const uint8_t* commits, size_t commit_stride, size_t degree, size_t P, const uint8_t* mask,
                                       uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (P == 0) return TC_OK;
  TC_REQUIRE(ctx && commits && out);
  TC_REQUIRE(degree < (1u << 12) && P < (1ull << 26));
  const size_t n = degree + 1, ncoeff = n * (n + 1) / 2;
  TC_REQUIRE(commit_stride % 96 == 0 && commit_stride >= ncoeff * 96);
  Call k(ctx);
  const uint8_t* d_c = k.in(commits, (P - 1) * commit_stride + ncoeff * 96);
  const uint8_t* d_mask = k.in(mask, P);
  uint8_t* d_out = k.out(out, n * 96);
  uint8_t* d_st = k.out(status, n);
  k.begin_timing();
  g1_sum(k, true, d_c, commit_stride, P, d_mask, n, d_out, d_st, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_fr_sum_batch(tc_ctx* ctx, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* mask, size_t B, uint8_t* out_fr,
                    uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && out_fr && (n == 0 || vals_fr));
  TC_REQUIRE(n == 0 || (term_stride % 32 == 0 && term_stride / 32 >= B));
  TC_REQUIRE(B < (1ull << 32) && n < (1ull << 32));
  Call k(ctx);
  const uint8_t* d_v = k.in(vals_fr, n ? (n - 1) * term_stride + B * 32 : 0, /*secret=*/true);
  const uint8_t* d_mask = k.in(mask, n);
  uint8_t* d_out = k.out(out_fr, B * 32);
  // host-I/O mode: the (secret) sums pass through a staging slot that outlives the call: wiped after the copy back
  if (!ctx->device_io) k.secret(d_out, B * 32, /*after_copy=*/true);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed) tc::launch_fr_sum(ctx->stream, d_v, term_stride, n, d_mask, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// The public side is the first-column sum with the accept bytes as its mask; the sum kernel marks the parts that own a bad
// included point.  The secret side: every accepted part's interpolation at zero, then one Fr sum over the parts.  The verdict
// kernels write part_status and, when an accepted part failed, the identity / zero over both outputs.
int tc_dkg_generate_batch(tc_ctx* ctx, const uint8_t* commits, size_t commit_stride, size_t degree, size_t P, const uint8_t* accept,
                          const uint64_t* xs, const uint8_t* vals_fr, size_t n_v, uint8_t* out_commit, uint8_t* out_share_fr,
                          uint8_t* part_status) try {
  TC_REQUIRE(ctx);
  if (P == 0) return TC_OK;
  TC_REQUIRE(ctx && commits);
  TC_REQUIRE(degree < (1u << 12) && P < (1ull << 26) && n_v < (1u << 16));
  const size_t n = degree + 1, ncoeff = n * (n + 1) / 2;
  TC_REQUIRE(commit_stride % 96 == 0 && commit_stride >= ncoeff * 96);
  const bool share = out_share_fr != nullptr;
  TC_REQUIRE(!share || n_v == 0 || (xs && vals_fr));
  Call k(ctx);
  const uint8_t* d_c = k.in(commits, (P - 1) * commit_stride + ncoeff * 96);
  const uint8_t* d_acc = k.in(accept, P);
  const uint64_t* d_x = share ? k.in(xs, P * n_v) : nullptr;
  const uint8_t* d_v = share ? k.in(vals_fr, P * n_v * 32, /*secret=*/true) : nullptr;
  uint8_t* d_oc = out_commit ? k.out(out_commit, n * 96) : k.temp<uint8_t>(n * 96);
  uint8_t* d_os = k.out(out_share_fr, 32);
  if (!ctx->device_io) k.secret(d_os, 32, /*after_copy=*/true);
  uint8_t* d_ps = part_status ? k.out(part_status, P) : k.temp<uint8_t>(P);
  uint8_t* d_bad = k.temp<uint8_t>(P, /*zero=*/true);
  uint8_t* d_part = share ? k.temp<uint8_t>(P * 32) : nullptr;  // the parts' contributions to the share: secret
  k.secret(d_part, P * 32);
  uint8_t* d_sst = share ? k.temp<uint8_t>(P) : nullptr;
  k.begin_timing();
  g1_sum(k, true, d_c, commit_stride, P, d_acc, n, d_oc, nullptr, d_bad);
  if (!k.failed && share) {
    tc::launch_fr_interpolate_at_zero(ctx->stream, n_v, d_x, d_v, d_acc, P, d_part, d_sst);
    tc::launch_fr_sum(ctx->stream, d_part, 32, P, d_acc, 1, d_os, nullptr);
  }
  if (!k.failed) tc::launch_dkg_generate_verdict(ctx->stream, d_acc, d_bad, d_sst, P, degree, d_ps, d_oc, d_os);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- DKG resharing: the accepted parts summed with Lagrange weights, the master key unchanged ---------------------------------
// (`Poly * Fr` src/poly.rs:210-254, Commitment::add_assign :462-471, the finalisation :870-876 and :895-898, the coefficients of
// src/lib.rs:719-767)
int tc_g1_weighted_sum_batch(tc_ctx* ctx, const uint8_t* pts, size_t term_stride, size_t n, const uint8_t* weights_fr, const uint8_t* mask, size_t B,
                             uint8_t* out, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && out && (n == 0 || (pts && weights_fr)));
  TC_REQUIRE(n == 0 || (term_stride % 96 == 0 && term_stride / 96 >= B));
  TC_REQUIRE(B < (1ull << 26) && n < (1ull << 32) && B * n < (1ull << 40));
  Call k(ctx);
  const uint8_t* d_pts = k.in(pts, n ? (n - 1) * term_stride + B * 96 : 0);
  const uint8_t* d_w = k.in(weights_fr, n * 32);
  const uint8_t* d_mask = k.in(mask, n);
  uint8_t* d_out = k.out(out, B * 96);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  bool column0 = false;
  const uint8_t* d_member = g1_sum_members(k, column0, d_pts, term_stride, n, B);
  g1_wsum(k, false, d_pts, term_stride, n, d_w, d_mask, d_member, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_fr_weighted_sum_batch(tc_ctx* ctx, const uint8_t* vals_fr, size_t term_stride, size_t n, const uint8_t* weights_fr, const uint8_t* mask, size_t B,
                             uint8_t* out_fr, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && out_fr && (n == 0 || (vals_fr && weights_fr)));
  TC_REQUIRE(n == 0 || (term_stride % 32 == 0 && term_stride / 32 >= B));
  TC_REQUIRE(B < (1ull << 32) && n < (1ull << 32));
  Call k(ctx);
  const uint8_t* d_v = k.in(vals_fr, n ? (n - 1) * term_stride + B * 32 : 0, /*secret=*/true);
  const uint8_t* d_w = k.in(weights_fr, n * 32);
  const uint8_t* d_mask = k.in(mask, n);
  uint8_t* d_out = k.out(out_fr, B * 32);
  if (!ctx->device_io) k.secret(d_out, B * 32, /*after_copy=*/true);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed) tc::launch_fr_wsum(ctx->stream, d_v, term_stride, n, d_w, d_mask, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// Every accepted part is examined (k_reshare_check, the interpolations at zero), the verdict kernels pick S and its Lagrange
// weights, and the two weighted sums run with `used` as their mask -- the G1 sum over the t_old + 1 part numbers of S only, so its
// ladders spread evenly over the lanes wherever S sits among the P parts.  A failed verdict leaves used all zero (and the part
// numbers at their zero fill: part 0, masked out), so the sums are the identity and zero already; the guard writes them once more.
// Nothing of the selection passes through the host.
int tc_dkg_reshare_batch(tc_ctx* ctx, const uint8_t* old_commit, size_t t_old, const uint64_t* dealer_idx, const uint8_t* commits, size_t commit_stride,
                         size_t degree, size_t P, const uint8_t* accept, const uint64_t* xs, const uint8_t* vals_fr, size_t n_v, uint8_t* out_commit,
                         uint8_t* out_share_fr, uint8_t* used, uint8_t* part_status, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (P == 0) return TC_OK;
  TC_REQUIRE(ctx && old_commit && dealer_idx && commits);
  TC_REQUIRE(degree < (1u << 12) && t_old < (1u << 12) && P < (1ull << 16) && n_v < (1u << 16));
  const size_t n = degree + 1, ncoeff = n * (n + 1) / 2;
  TC_REQUIRE(commit_stride % 96 == 0 && commit_stride >= ncoeff * 96);
  const bool share = out_share_fr != nullptr;
  TC_REQUIRE(!share || n_v == 0 || (xs && vals_fr));
  Call k(ctx);
  const uint8_t* d_old = k.in(old_commit, (t_old + 1) * 96);
  const uint64_t* d_di = k.in(dealer_idx, P);
  const uint8_t* d_c = k.in(commits, (P - 1) * commit_stride + ncoeff * 96);
  const uint8_t* d_acc = k.in(accept, P);
  const uint64_t* d_x = share ? k.in(xs, P * n_v) : nullptr;
  const uint8_t* d_v = share ? k.in(vals_fr, P * n_v * 32, /*secret=*/true) : nullptr;
  uint8_t* d_oc = out_commit ? k.out(out_commit, n * 96) : k.temp<uint8_t>(n * 96);
  uint8_t* d_os = k.out(out_share_fr, 32);
  if (!ctx->device_io) k.secret(d_os, 32, /*after_copy=*/true);
  uint8_t* d_used = used ? k.out(used, P) : k.temp<uint8_t>(P);
  uint8_t* d_ps = part_status ? k.out(part_status, P) : k.temp<uint8_t>(P);
  uint8_t* d_status = status ? k.out(status, 1) : k.temp<uint8_t>(1);
  uint8_t* d_flags = k.temp<uint8_t>(3 * P + 1);  // const_st, point_bad, dup, old_bad
  uint8_t* d_part = share ? k.temp<uint8_t>(P * 32) : nullptr;  // the parts' contributions to the share: secret
  k.secret(d_part, P * 32);
  uint8_t* d_sst = share ? k.temp<uint8_t>(P) : nullptr;
  uint8_t* d_w = k.temp<uint8_t>(P * 32, /*zero=*/true);  // lambda_p on S: public
  uint32_t* d_sel = k.temp<uint32_t>(t_old + 1, /*zero=*/true);  // (read by the sum whatever the verdict: never uninitialised)
  uint64_t* d_sidx = k.temp<uint64_t>(t_old + 1);
  uint32_t* d_ws = k.temp<uint32_t>(tc::reshare_plan_ws_words(t_old));
  uint8_t* d_oldv = ctx->input_checks ? k.temp<uint8_t>(t_old + 1) : nullptr;
  k.begin_timing();
  if (!k.failed) {
    bool column0 = true;
    const uint8_t* d_pts = d_c;
    size_t term_stride = commit_stride;
    const uint8_t* d_member = g1_sum_members(k, column0, d_pts, term_stride, P, n);
    if (d_oldv && !k.failed) tc::launch_subgroup_check_g1(ctx->stream, d_old, 96, 1, 1, t_old + 1, d_oldv);
    if (!k.failed) {
      tc::launch_reshare_check(ctx->stream, d_old, d_oldv, t_old, d_di, d_c, commit_stride, degree, d_acc, d_member, P, d_flags, d_flags + P,
                               d_flags + 2 * P, d_flags + 3 * P);
      if (share) tc::launch_fr_interpolate_at_zero(ctx->stream, n_v, d_x, d_v, d_acc, P, d_part, d_sst);
      tc::launch_reshare_verdict(ctx->stream, d_acc, d_di, t_old, P, d_flags, d_flags + P, d_flags + 2 * P, d_sst, d_flags + 3 * P, d_ps, d_used, d_sel,
                                 d_sidx, d_ws, d_w, d_status);
      g1_wsum(k, column0, d_pts, term_stride, P, d_w, d_used, d_member, n, d_oc, nullptr, d_sel, t_old + 1);
      if (share && !k.failed) tc::launch_fr_wsum(ctx->stream, d_part, 32, P, d_w, d_used, 1, d_os, nullptr);
      if (!k.failed) tc::launch_reshare_guard(ctx->stream, d_status, degree, d_oc, d_os);
    }
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- membership tests ---------------------------------------------------------------------------
static int subgroup_check(tc_ctx* ctx, bool g2, const uint8_t* pts, size_t B, uint8_t* ok) {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && pts && ok);
  const size_t PB = g2 ? 192 : 96;
  Call k(ctx);
  const uint8_t* d_pts = k.in(pts, B * PB);
  uint8_t* d_ok = k.out(ok, B);
  k.begin_timing();
  if (!k.failed) {
    if (g2) tc::launch_subgroup_check_g2(ctx->stream, d_pts, PB, 1, 1, B, d_ok);
    else tc::launch_subgroup_check_g1(ctx->stream, d_pts, PB, 1, 1, B, d_ok);
  }
  k.end_timing();
  return k.finish();
}
int tc_g1_subgroup_check_batch(tc_ctx* ctx, const uint8_t* pts96, size_t B, uint8_t* ok) try {
  return subgroup_check(ctx, false, pts96, B, ok);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}
int tc_g2_subgroup_check_batch(tc_ctx* ctx, const uint8_t* pts192, size_t B, uint8_t* ok) try {
  return subgroup_check(ctx, true, pts192, B, ok);
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

// ---- wire formats ------------------------------------------------------------------------------
int tc_g1_compress_batch(tc_ctx* ctx, const uint8_t* in96, size_t B, uint8_t* out48, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && in96 && out48);
  Call k(ctx);
  const uint8_t* d_in = k.in(in96, B * 96);
  uint8_t* d_out = k.out(out48, B * 48);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed) tc::launch_g1_compress(ctx->stream, d_in, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_g2_compress_batch(tc_ctx* ctx, const uint8_t* in192, size_t B, uint8_t* out96, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && in192 && out96);
  Call k(ctx);
  const uint8_t* d_in = k.in(in192, B * 192);
  uint8_t* d_out = k.out(out96, B * 96);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed) tc::launch_g2_compress(ctx->stream, d_in, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_encrypt_batch(tc_ctx* ctx, const uint8_t* pk, size_t pk_stride, const uint8_t* r, const uint8_t* msgs,
                     const uint64_t* off, size_t B, uint8_t* out_u, uint8_t* out_v, uint8_t* out_w, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && pk && r && off && out_u && out_w);
  TC_REQUIRE(pk_stride == 0 || pk_stride >= 96);
  Call k(ctx);
  uint64_t total = 0;
  if (!total_bytes(k, off, B, &total)) return k.finish();
  TC_REQUIRE(total == 0 || (msgs && out_v));  // (all-empty messages: no v bytes, and a device-resident empty buffer has no address)
  const uint8_t* d_pk = k.in(pk, pk_stride ? (B - 1) * pk_stride + 96 : 96);
  const uint8_t* d_r = k.in(r, B * 32, /*secret=*/true);
  const uint8_t* d_msgs = k.in(msgs, (size_t)total);
  const uint64_t* d_off = k.in(off, B + 1);
  uint8_t* d_u = k.out(out_u, B * 96);
  uint8_t* d_v = k.out(out_v, (size_t)total);
  uint8_t* d_w = k.out(out_w, B * 192);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  k.check_points(false, d_pk, pk_stride, 1, 1, B, 1);
  if (!k.failed) tc::launch_encrypt(ctx->stream, k.tables(), d_pk, pk_stride, d_r, d_msgs, d_off, B, d_u, d_v, d_w, d_st);
  if (!k.checks.empty()) {
    // an invalid key fails the job: status + identity u and w (v keeps the kernel's bytes and must be ignored)
    auto pending = k.checks;
    for (auto& p : pending) p.pts = nullptr;  // (the first apply_checks launches the tests; the second only applies their verdicts)
    k.apply_checks(B, d_st, d_u, 96, nullptr);
    k.checks = pending;
    k.apply_checks(B, nullptr, d_w, 192, nullptr);
  }
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_public_key_share_batch(tc_ctx* ctx, const uint8_t* commit, size_t t, const uint64_t* idx, size_t M, uint8_t* out,
                              uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (M == 0) return TC_OK;
  TC_REQUIRE(ctx && commit && idx && out);
  TC_REQUIRE(t < (1u << 20));
  Call k(ctx);
  const uint8_t* d_c = k.in(commit, (t + 1) * 96);
  const uint64_t* d_idx = k.in(idx, M);
  uint8_t* d_out = k.out(out, M * 96);
  uint8_t* d_st = k.out(status, M);
  k.begin_timing();
  k.check_points(false, d_c, 96, t + 1, t + 1, 1, (size_t)-1);  // the t+1 coefficients, shared by every index
  if (!k.failed) tc::launch_commitment_evaluate(ctx->stream, d_c, t, d_idx, M, d_out, d_st);
  k.apply_checks(M, d_st, d_out, 96, nullptr);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_g1_decompress_batch(tc_ctx* ctx, const uint8_t* in48, size_t B, uint8_t* out96, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && in48 && out96);
  Call k(ctx);
  const uint8_t* d_in = k.in(in48, B * 48);
  uint8_t* d_out = k.out(out96, B * 96);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed) tc::launch_g1_decompress(ctx->stream, d_in, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

int tc_g2_decompress_batch(tc_ctx* ctx, const uint8_t* in96, size_t B, uint8_t* out192, uint8_t* status) try {
  TC_REQUIRE(ctx);
  if (B == 0) return TC_OK;
  TC_REQUIRE(ctx && in96 && out192);
  Call k(ctx);
  const uint8_t* d_in = k.in(in96, B * 96);
  uint8_t* d_out = k.out(out192, B * 192);
  uint8_t* d_st = k.out(status, B);
  k.begin_timing();
  if (!k.failed) tc::launch_g2_decompress(ctx->tuning, ctx->stream, d_in, B, d_out, d_st);
  k.end_timing();
  return k.finish();
} catch (...) {
  return on_exception((tc_ctx*)ctx);
}

}  // extern "C"
