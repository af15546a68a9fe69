"""Single-point kernel conformance: the kernels of k_mul.hip, k_hash.hip, k_check.hip and k_robust.hip, launched directly and
compared byte for byte.

The fourth kernel-level suite (after tests/device_conformance.py, tests/manypoint_conformance.py and tests/dkg_conformance.py,
whose helpers and build recipe it reuses).  tests/device/single_kernels.hip (k_check.hip, k_robust.hip) and
tests/device/single_kernels_mul.hip (k_mul.hip, k_hash.hip) include the kernel units as they are and launch every kernel THROUGH
THE PRODUCT'S LAUNCHER; where the launcher derives a geometry (the register / arena / shared form of a multiplication, `share` of
k_g2_mul_gather, the two-jobs-per-lane-pair forms, the 16-byte form of k_gather_selected) the test chooses it and the kernel is
launched directly.  Every buffer a kernel writes is filled with 0x5A first and carries one guard row / byte / entry behind it,
and everything comes back.  tests/device/single_kernels_host.cpp runs the same header routines with g++ -DTC_BOUND_CHECK over the
same buffers, each kernel's index map written as a plain loop.

Expected values come from the big-integer oracle (oracle/tc_oracle.py), from the shared table of encodings and the hash
references of tests/device_conformance.py (which are the oracle's), and from plain restatements of the header comments, never from
the code under test.  Points are known multiples of the generators, so a product costs one oracle multiplication per DISTINCT
output.  All comparisons are exact.

  legs   "sk_": the device harness (tests/test_gpu_single_kernels.py); "skh_": the host leg (tests/test_single_kernels_host.py).
         The host leg does not see lane pairing, the arena, the indexing or the launch geometry; the kernels whose body lives in
         the __global__ function (k_rlc_scalars*, k_invalidate_jobs, k_ok_and_status, the gather, scatter and take kernels,
         k_robust_mark, k_robust_finish, k_gather_selected) have no host entry: their models are plain Python.
"""
import ctypes
import os
import random
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dkg_conformance as dk  # noqa: E402
from dkg_conformance import fresh, u8, fr32, is_poison, rows, same  # noqa: E402,F401
from manypoint_conformance import enc, HipError, POISON  # noqa: E402

mp, dc, o = dk.mp, dk.dc, dk.o
R, P, X, X2, RF = o.R, o.Q, dc.X, dc.X2, 1 << 256
OK, NOT_ENOUGH, INVALID = 0, 1, 3  # tc_codec.h TC_JOB_*
NOT_ENOUGH_V, GOOD_V, RETRY_V = 0, 1, 2  # tc_robust.h RobustVerdict
PB = {1: 96, 2: 192}
IDENT = {1: enc(1, None), 2: enc(2, None)}
BAD = mp.BAD_POINT
NOSLOT = 0xffffffff
EDGE_SCALARS = [0, 1, R - 1, R, RF - 1]


# ---------------------------------------------------------------------------------------------------------------------
# builds and entries
# ---------------------------------------------------------------------------------------------------------------------
DEVICE_UNITS = ("single_kernels.hip", "single_kernels_mul.hip")


def build_device():
    """tests/device/single_kernels.hip and single_kernels_mul.hip -> two gfx950 shared objects, with the product's compiler
    flags (build.py FLAGS)."""
    from threshold_crypto_amd import build as tcb
    libs = []
    for unit in DEVICE_UNITS:
        src = os.path.join(mp.DEV, unit)
        libs.append(dc._build("libtc_" + unit[:-4], lambda out, src=src: [dc.hipcc()] + tcb.FLAGS + ["-w", "-shared", src, "-o", out], {unit}))
    return libs


def build_host():
    src = os.path.join(mp.DEV, "single_kernels_host.cpp")
    return dc._build("libtc_single_kernels_host_bc",
                     lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-shared", "-fPIC", src, "-o", out],
                     {"single_kernels_host.cpp"})


def build_host_main(extra=()):
    """The stand-alone program of single_kernels_host.cpp (its fixed short case list); extra: e.g. sanitizer flags."""
    src = os.path.join(mp.DEV, "single_kernels_host.cpp")
    return dc._build("single_kernels_host_main",
                     lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-DSK_MAIN"] + list(extra) + [src, "-o", out],
                     {"single_kernels_host.cpp"})


# i: int, z: size_t, p: pointer -- the arguments of the entries of single_kernels*.hip / single_kernels_host.cpp
SIG = {"point_mul": "ippzzipp", "g2_mul_gather": "pzppzzzipp", "compress": "ipzipp", "decompress": "iipzipp", "decompress_take": "iipzzzpp",
       "decompress_selected": "iipzzppzpp", "small": "ipzzzp", "commitment_evaluate": "pzpzipp", "hash": "pppziiipp", "xor_with_hash": "pppzpp",
       "encrypt": "pzpppzipppp", "subgroup_check": "ipzzzzzp", "select_shares": "ppzzzzzpzpppp"}
SIG_DEVICE_ONLY = {"rlc_scalars": "ipzp", "invalidate_jobs": "pzzzzppzp", "ok_and_status": "pzp", "gather_rows": "pzzpzp", "move_bytes": "ippzzp",
                   "gather_selected": "pzzzppzizzp", "robust_mark": "pppzzppp", "robust_finish": "pzzzzzppppppppp", "take_u64": "pzzzp"}
_CT = {"i": ctypes.c_int, "z": ctypes.c_size_t, "p": ctypes.c_void_p}


def load(paths, prefix):
    """paths: the device harness's two libraries, or the host leg's one."""
    libs = [ctypes.CDLL(p) for p in ([paths] if isinstance(paths, str) else paths)]
    host = prefix == "skh_"
    entries = {}
    for name, sig in list(SIG.items()) + ([] if host else list(SIG_DEVICE_ONLY.items())):
        f = next(getattr(lib, prefix + name) for lib in libs if hasattr(lib, prefix + name))
        f.argtypes = [_CT[c] for c in sig]
        f.restype = ctypes.c_int
        entries[name] = f
    return dict(entries, lib=libs, host=host)


def call(lib, name, *args):
    """One entry; numpy arrays go in as pointers.  A non-zero return (the first HIP error, or -2: a table slot left in use)
    raises HipError."""
    if lib.get("python"):  # KernelText: the arrays themselves
        rc = lib[name](*args)
    else:
        rc = lib[name](*[a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a for a in args])
    if rc != 0:
        raise HipError("%s: the harness returned %d%s" % (name, rc, " (a table slot stayed in use)" if rc == mp.SLOT_LEAK else ""))


def arr(vals, dtype):
    a = np.array(list(vals), dtype=dtype)
    return a if len(a) else np.zeros(1, dtype=dtype)


def guarded(vals, dtype=np.uint8):
    """An array a kernel reads AND writes, with its guard entry (0x5A bytes) behind it."""
    a = np.array(list(vals), dtype=dtype).reshape(-1)
    return np.concatenate([a, fresh(1, dtype)])


_PT = {1: {0: None}, 2: {0: None}}
_MULTS = {}


def gmul(w, m):
    """[m] G by the oracle's multiplication (cached)."""
    m %= R
    if m not in _PT[w]:
        _PT[w][m] = mp.E[w].mul(mp.GEN[w], m)
    return _PT[w][m]


def pool(w):
    """40 distinct non-zero multiples of the generator of group w."""
    if w not in _MULTS:
        rnd = random.Random("single-kernels-pool-%d" % w)
        _MULTS[w] = [rnd.randrange(1, R) for _ in range(40)]
    return _MULTS[w]


def prod(w, k, m):
    """[k] ([m] G) for k, m mod r."""
    return gmul(w, k * m % R)


def offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return np.array(off, dtype=np.uint64)


def message(n, salt=0):
    return bytes((37 * i + 11 * n + 101 * salt + 3) & 0xff for i in range(n))


def off_curve(w):
    b = bytearray(enc(w, gmul(w, 7)))
    b[-1] ^= 1
    return bytes(b)


# ---------------------------------------------------------------------------------------------------------------------
# 1. k_mul.hip: the multiplications
# ---------------------------------------------------------------------------------------------------------------------
MUL_SHAPES = [(1, 1), (1, 70), (3, 33), (5, 13), (2, 65)]  # (S, B): S B = 65 and 130 leave lanes past the end
MUL_KERNELS = {1: (0, 1, 2), 2: (3, 4)}  # launcher / k_point_mul<Fq> / k_g1_mul_arena; launcher (shared when S > 1) / k_point_mul<Fq2>
MUL_DISTINCT = {1: 35, 2: 13}
_PROPER = [random.Random("single-kernels-scalars").randrange(2, R) for _ in range(9)]


class MulCase:
    """S scalars x B points (multiples of the generator; 0: the identity, None: a point that does not decode):
    out[j S + s] = scalars[s] * points[j]."""

    def __init__(self, w, scalars, mults, tag, bad_bytes=None):
        self.w, self.scalars, self.mults, self.tag = w, list(scalars), list(mults), tag
        self.S, self.B = len(self.scalars), len(self.mults)
        self.bad_bytes = bad_bytes or BAD[w]
        self._want = None

    def want(self):
        if self._want is None:
            self._want = []
            for j, m in enumerate(self.mults):
                for k in self.scalars:
                    good = m is not None and k < R
                    self._want.append((enc(self.w, prod(self.w, k, m)) if good else IDENT[self.w], OK if good else INVALID))
        return self._want

    def points(self):
        return b"".join(self.bad_bytes if m is None else enc(self.w, gmul(self.w, m)) for m in self.mults)


MUL_VARIANTS = ["plain", "bad scalar first", "bad scalar last", "bad point first", "bad point last"]


def mul_case(w, S, B, variant):
    pl = pool(w)
    scalars = _PROPER[:S]
    mults = [pl[j % MUL_DISTINCT[w]] for j in range(B)]
    if B >= 3:
        mults[B // 2] = 0  # an identity point
    if variant == "bad scalar first":
        scalars[0] = R
    elif variant == "bad scalar last":
        scalars[S - 1] = RF - 1
    elif variant == "bad point first":
        mults[0] = None
    elif variant == "bad point last":
        mults[B - 1] = None
    elif variant.startswith("edge"):  # "edges": the five edge scalars side by side (S = 5); "edge k": edge k as the only scalar
        scalars = EDGE_SCALARS[:S] if variant == "edges" else [EDGE_SCALARS[int(variant[5:])]] * S
    elif variant != "plain":
        raise ValueError(variant)
    return MulCase(w, scalars, mults, "mul G%d S=%d B=%d %s" % (w, S, B, variant))


def mul_variants(S, B):
    v = list(MUL_VARIANTS)
    if (S, B) == (5, 13):
        v.append("edges")
    if (S, B) == (1, 70):
        v += ["edge %d" % k for k in range(5)]
    if B == 1:
        v = [x for x in v if x != "bad point last"]
    if S == 1:
        v = [x for x in v if x != "bad scalar last"]
    return v


def shared_case(S, B, rot):
    """k_g2_mul_shared: position p of every chunk holds a scalar 0, a non-canonical one and a proper one as rot goes 0, 1, 2, so the
    shared inversion sees identities first, last and in the middle; rot = 1 and B > 1: the last point does not decode."""
    kinds = lambda s: [0, R + 1 + s, _PROPER[s]][(s + rot) % 3]
    pl = pool(2)
    mults = [pl[j % 8] for j in range(B)]
    if rot == 1 and B > 1:
        mults[B - 1] = None
    if rot == 2 and B > 2:
        mults[1] = 0
    return MulCase(2, [kinds(s) for s in range(S)], mults, "shared S=%d B=%d rot=%d" % (S, B, rot))


SHARED_S, SHARED_B = [2, 3, 4, 5, 8, 9], [1, 7, 33]


def run_mul(lib, case, kernel, with_status=1):
    n = case.S * case.B
    out, status = fresh((n + 1) * PB[case.w]), fresh(n + 1)
    call(lib, "point_mul", kernel, u8(b"".join(fr32(k) for k in case.scalars)), u8(case.points()), case.S, case.B, with_status, out, status)
    return out, status


def check_points(what, w, want, with_status, res):
    """want: [(bytes, status)] per output of a kernel that writes points and status bytes."""
    out, status = res
    L, pb = len(want), len(want[0][0]) if want else PB[w]
    bad = []
    if not is_poison(out[L * pb:]) or status[L] != POISON:
        bad.append("%s: the guard row or byte was written" % what)
    if not with_status and not is_poison(status):
        bad.append("%s: status written though null was passed" % what)
    for t, (b, st) in enumerate(want):
        if bytes(out[t * pb:(t + 1) * pb]) != b or (with_status and status[t] != st):
            bad.append("%s output %d: wrong bytes or status %d, expected %d" % (what, t, status[t], st))
    return bad[:12]


def check_mul(case, with_status, res):
    return check_points(case.tag, case.w, case.want(), with_status, res)


# k_g2_mul_gather at the shapes of the G1 comb suite
GATHER_SHAPES = [(1, 5), (7, 5), (8, 5), (9, 5), (17, 5), (9, 70)]  # (n, B)
GATHER_SHARES = list(range(1, 9)) + [0]
_GATHER = {}


class GatherCase:
    """N = 40 keys (0, 1, r - 1, r and 2^256 - 1 among them), B messages (a multiple of G2's generator, 0 = the identity, None =
    undecodable), n signer indices each; an index >= N stands first, in the middle or last in a row, so that at one share or
    another it is the first and the last of a chunk."""

    def __init__(self, n, B):
        rnd = random.Random("single-kernels-gather-%d-%d" % (n, B))
        self.n, self.B, self.N, self.tag = n, B, 40, "gather n=%d B=%d" % (n, B)
        ks = [0, 1, 2, R - 1, R, 3, RF - 1, R - 2, X, X + 1, X ** 3 - 1, (R - 1) // 2]
        self.keys = ks + _PROPER + [rnd.randrange(R) for _ in range(self.N - len(ks) - len(_PROPER))]
        msgs = [pool(2)[0], 0, pool(2)[1], None, pool(2)[2]]
        self.msgs = [msgs[j % 5] for j in range(B)]
        self.idx = []
        for j in range(B):
            row = [(j * 7 + 3 * s) % 24 for s in range(n)] if j % 2 else [(s + 3 * j) % 12 for s in range(n)]
            if n > 1 or j % 2 == 0:
                row[(0, n // 2, n - 1)[j % 3]] = (self.N, self.N + j, 1 << 63)[j % 3]
            if j % 8 == 7:
                row = [(s + j) % 12 for s in range(n)]  # a row without a bad index
            self.idx.append(row)
        self._ref = None

    def ref(self):
        if self._ref is None:
            st, out = [], []
            for j in range(self.B):
                a = self.msgs[j]
                for i in self.idx[j]:
                    good = a is not None and i < self.N and self.keys[i] < R
                    st.append(OK if good else INVALID)
                    out.append(enc(2, prod(2, self.keys[i], a) if good else None))
            self._ref = (st, out)
        return self._ref


def gather_case(n, B):
    if (n, B) not in _GATHER:
        _GATHER[(n, B)] = GatherCase(n, B)
    return _GATHER[(n, B)]


def run_gather(lib, case, share, with_status=1):
    n, B = case.n, case.B
    out, status = fresh((n * B + 1) * 192), fresh(n * B + 1)
    pts = u8(b"".join(BAD[2] if a is None else enc(2, gmul(2, a)) for a in case.msgs))
    call(lib, "g2_mul_gather", u8(b"".join(fr32(k) for k in case.keys)), case.N, np.array(case.idx, dtype=np.uint64).reshape(-1), pts, n, B, share,
         with_status, out, status)
    return out, status


def check_gather(case, share, with_status, res):
    st, out = case.ref()
    return check_points("%s share=%d" % (case.tag, share), 2, list(zip(out, st)), with_status, res)


# ---------------------------------------------------------------------------------------------------------------------
# 2. k_mul.hip: the codecs
# ---------------------------------------------------------------------------------------------------------------------
CODEC_B = [1, 2, 63, 65]
CSIZE = {1: 48, 2: 96}


def codec_ref(g, form, b, member=True):
    """(ok, point) of an encoding: the shared table's reference (the oracle's checked decode / uncompressed parse), or with
    member = False the curve-level decode of a compressed form (no subgroup test)."""
    if member or form == "unc":
        return dc.byte_ref(g, form, b)

    def ref():
        try:
            return True, (o.g1_from_compressed if g == 1 else o.g2_from_compressed)(bytes(b), check=False)
        except o.DecodeError:
            return False, None
    return dc.cached("curveref", (g, bytes(b)), ref)


def codec_inputs(g, form, B, shift, tail=None):
    """B encodings dealt from the shared table of encodings, entry (j + shift) mod its length at position j; tail: the kind of the
    table the last position holds instead (the odd tail of a pair when B is odd)."""
    tbl = dc.byte_cases(g, form)
    ins = [tbl[(j + shift) % len(tbl)][2] for j in range(B)]
    if tail:
        ins[B - 1] = [b for _, k, b in tbl if k == tail][0]
    return ins


CODEC_TAILS = [None, "x out of range", "bad flags", "non-square", "outside subgroup", "identity"]


def codec_want(g, form, ins, member=True):
    """form "comp": the decoders (uncompressed point out), "unc": k_compress (compressed out)."""
    out_enc = {(1, "comp"): o.g1_uncompressed, (2, "comp"): o.g2_uncompressed, (1, "unc"): o.g1_compressed, (2, "unc"): o.g2_compressed}[(g, form)]
    want = []
    for b in ins:
        ok, p = codec_ref(g, form, b, member)
        want.append((out_enc(p if ok else None), OK if ok else INVALID))
    return want


def run_decompress(lib, g, form, ins, with_status=1):
    B = len(ins)
    out, status = fresh((B + 1) * PB[g]), fresh(B + 1)
    call(lib, "decompress", g - 1, form, u8(b"".join(ins)), B, with_status, out, status)
    return out, status


def run_compress(lib, g, ins, with_status=1):
    B = len(ins)
    out, status = fresh((B + 1) * CSIZE[g]), fresh(B + 1)
    call(lib, "compress", g - 1, u8(b"".join(ins)), B, with_status, out, status)
    return out, status


TAKE_SHAPES = [(5, 3), (4, 4), (3, 1)]  # (n_per_job, take)
TAKE_B = [1, 7, 43]
GARBAGE = bytes([0xEE])  # what the samples behind `take` hold: no decoder takes it (x >= q with all three flag bits set)


def take_inputs(g, npj, take, B):
    """B x n_per_job compressed samples; the first `take` of a record from the shared table, the rest garbage.  Returns (all bytes,
    the samples a kernel must read, in output order)."""
    tbl = dc.byte_cases(g, "comp")
    buf, used = [], []
    for j in range(B):
        for k in range(npj):
            if k < take:
                b = tbl[(j * take + k + 3 * j) % len(tbl)][2]
                used.append(b)
            else:
                b = GARBAGE * CSIZE[g]
            buf.append(b)
    return b"".join(buf), used


def run_take(lib, g, form, npj, take, B):
    data, _ = take_inputs(g, npj, take, B)
    n = B * take
    out, valid = fresh((n + 1) * PB[g]), fresh(n + 1)
    call(lib, "decompress_take", g - 1, form, u8(data), npj, take, B, out, valid)
    return out, valid


def check_take(g, npj, take, B, res):
    _, used = take_inputs(g, npj, take, B)
    want = [(b, 1 if st == OK else 0) for b, st in codec_want(g, "comp", used)]
    return check_points("take G%d (%d, %d) B=%d" % (g, npj, take, B), g, want, 1, res)


def run_take_u64(lib, npj, take, B):
    rnd = random.Random("single-kernels-take-%d-%d-%d" % (npj, take, B))
    src = [rnd.getrandbits(64) for _ in range(B * npj)]
    out = fresh(B * take + 1, np.uint64)
    call(lib, "take_u64", arr(src, np.uint64), npj, take, B, out)
    want = [src[j * npj + k] for j in range(B) for k in range(take)]
    bad = []
    if [int(v) for v in out[:B * take]] != want:
        bad.append("take_u64 (%d, %d) B=%d: wrong words" % (npj, take, B))
    if not is_poison(out[B * take:]):
        bad.append("take_u64 (%d, %d) B=%d: the guard word was written" % (npj, take, B))
    return bad


SELECTED_JOBS = {1: [], 5: [0, 3, 4], 22: [0, 7, 11, 21]}  # jobs -> the jobs without enough shares (need = 3: an odd job starts in slot b)
SEL_N, SEL_NEED = 7, 3


class SelectedCase:
    """jobs x N = 7 compressed shares from the shared table (malformed entries and an on-curve non-member among them), need = 3
    slots per job; the jobs of `lacking` have enough = 0 and slots 0xffffffff."""

    def __init__(self, g, jobs, lacking):
        rnd = random.Random("single-kernels-selected-%d-%d" % (g, jobs))
        tbl = dc.byte_cases(g, "comp")
        self.g, self.jobs, self.tag = g, jobs, "selected G%d jobs=%d lacking %s" % (g, jobs, lacking)
        self.shares = [tbl[(j * SEL_N + i + j) % len(tbl)][2] for j in range(jobs) for i in range(SEL_N)]
        outside = [b for _, k, b in tbl if k == "outside subgroup"][0]
        self.shares[min(jobs - 1, 1) * SEL_N + 2] = outside
        self.enough = [0 if j in lacking else 1 for j in range(jobs)]
        self.slot = []
        for j in range(jobs):
            pick = sorted(rnd.sample(range(SEL_N), SEL_NEED))
            if j == min(jobs - 1, 1):
                pick = [0, 2, 6]  # the non-member is selected
            self.slot += pick if self.enough[j] else [NOSLOT] * SEL_NEED
        self.nonmember_record = min(jobs - 1, 1) * SEL_NEED + 1 if self.enough[min(jobs - 1, 1)] else None

    def want(self):
        out = []
        for i, s in enumerate(self.slot):
            j = i // SEL_NEED
            if not self.enough[j]:
                out.append((IDENT[self.g], 1))
                continue
            ok, p = codec_ref(self.g, "comp", self.shares[j * SEL_N + s], member=False)
            out.append((enc(self.g, p if ok else None), int(ok)))
        return out


def run_selected(lib, case, form):
    n = case.jobs * SEL_NEED
    out, ok = fresh((n + 1) * PB[case.g]), fresh(n + 1)
    call(lib, "decompress_selected", case.g - 1, form, u8(b"".join(case.shares)), SEL_N, SEL_NEED, arr(case.slot, np.uint32), arr(case.enough, np.uint8),
         case.jobs, out, ok)
    return out, ok


def check_selected(case, res):
    return check_points(case.tag, case.g, case.want(), 1, res)


def small_cases():
    """(what, input bytes, stride, n, expected output rows)."""
    rnd = random.Random("single-kernels-small")
    ks = [0, 1, R - 1, R, RF - 1, dc.COFACTOR_FIX] + [rnd.randrange(R) for _ in range(64)]
    out = [(0, b"".join(fr32(k) for k in ks), 32, len(ks), [fr32(k * dc.COFACTOR_FIX % R) if k < R else b"\xff" * 32 for k in ks])]
    pl = pool(1)
    pts = [(enc(1, gmul(1, pl[j])), enc(1, prod(1, dc.COFACTOR_FIX, pl[j]))) for j in range(8)]
    bads = [BAD[1], off_curve(1)]
    items = [pts[j % 8] if j % 9 != 4 else (bads[j % 2], bads[j % 2]) for j in range(70)]
    items[7] = (IDENT[1], IDENT[1])
    out.append((1, b"".join(a for a, _ in items), 96, 70, [b for _, b in items]))
    out.append((1, pts[3][0], 0, 65, [pts[3][1]] * 65))                      # stride 0: one operand for every lane
    out.append((1, bads[1], 0, 3, [bads[1]] * 3))
    return out


def run_small(lib, what, data, stride, n):
    width = 32 if what == 0 else 96
    out = fresh(4 * 96 if what == 2 else (n + 1) * width)  # what = 2: two rows, a guard row behind each
    call(lib, "small", what, u8(data), len(data), stride, n, out)
    return out


def check_small(what, n, want, out):
    width = 32 if what == 0 else 96
    bad = []
    if not is_poison(out[n * width:]):
        bad.append("small kernel %d: the guard row was written" % what)
    for j in range(n):
        if bytes(out[j * width:(j + 1) * width]) != want[j]:
            bad.append("small kernel %d row %d: wrong bytes" % (what, j))
    return bad[:12]


def generator_want():
    unfix = pow(dc.COFACTOR_FIX, -1, R)
    return enc(1, o.G1_GEN), enc(1, o.E1.mul(o.G1_GEN, unfix))


# ---------------------------------------------------------------------------------------------------------------------
# 3. k_check.hip and k_robust.hip
# ---------------------------------------------------------------------------------------------------------------------
RLC_NS = [1, 64, 65, 130]
RLC_SEEDS = [bytes(range(32)), bytes((251 * i + 17) & 0xff for i in range(32))]


def rlc_model(g1, seed, i):
    """The header comments of k_rlc_scalars / k_rlc_scalars_g1 restated over the oracle's ChaCha20: key = seed, block counter = i,
    the first two words."""
    w0, w1 = o.chacha20_block(struct.unpack("<8I", seed), i)[:2]
    if g1:
        return (w0 | 1) + w1 * X2
    d = [(w0 & 0xffff) | 1, w0 >> 16, w1 & 0xffff, w1 >> 16]
    return d[0] + d[1] * X + d[2] * X ** 2 + d[3] * X ** 3


def run_rlc(lib, g1, seed, n):
    out = fresh((n + 1) * 32)
    call(lib, "rlc_scalars", g1, u8(seed), n, out)
    return out


def check_rlc(g1, seed, n, out):
    bad = []
    what = "rlc scalars%s n=%d" % (" g1" if g1 else "", n)
    if not is_poison(out[n * 32:]):
        bad.append("%s: the guard row was written" % what)
    vals = [int.from_bytes(bytes(out[i * 32:(i + 1) * 32]), "little") for i in range(n)]
    for i, v in enumerate(vals):
        if v != rlc_model(g1, seed, i):
            bad.append("%s row %d: %x, the restatement gives %x" % (what, i, v, rlc_model(g1, seed, i)))
        # what the soundness argument uses
        if not v & 1:
            bad.append("%s row %d: the low digit is even" % (what, i))
        if v >= (R if g1 else 1 << 208):
            bad.append("%s row %d: out of range" % (what, i))
    if len(set(vals)) != n:
        bad.append("%s: the scalars are not pairwise distinct" % what)
    return bad[:12]


SUBGROUP_SHAPES = [(5, 3), (1, 1)]
SUBGROUP_NS = [1, 33, 65]
_SUB = {}


def subgroup_points(g):
    """[(bytes, member)]: a member, an on-curve non-member, an off-curve point, x >= q, the identity, another member."""
    if g not in _SUB:
        rnd = random.Random("single-kernels-subgroup-%d" % g)
        q = dc.g1_point(rnd, False) if g == 1 else dc.g2_point(rnd, False)
        _SUB[g] = [(enc(g, gmul(g, pool(g)[0])), 1), (enc(g, q), 0), (off_curve(g), 0), (BAD[g], 0), (IDENT[g], 1), (enc(g, gmul(g, pool(g)[1])), 1)]
    return _SUB[g]


def run_subgroup(lib, g, npj, take, n, slack=0):
    kinds = subgroup_points(g)
    stride = PB[g] + slack
    recs = (n + take - 1) // take
    buf, want = [], []
    for r in range(recs):
        for k in range(npj):
            if k < take:
                b, m = kinds[(r * take + k + r) % len(kinds)]
                if r * take + k < n:
                    want.append(m)
            else:
                b = GARBAGE * PB[g]
            buf.append(b + b"\xEE" * slack)
    valid = fresh(n + 1)
    data = b"".join(buf)
    call(lib, "subgroup_check", g - 1, u8(data), len(data), stride, npj, take, n, valid)
    return valid, want


def check_subgroup(what, res):
    valid, want = res
    bad = []
    if valid[len(want)] != POISON:
        bad.append("%s: the guard byte was written" % what)
    if [int(v) for v in valid[:len(want)]] != want:
        bad.append("%s: verdicts %s, expected %s" % (what, [int(v) for v in valid[:len(want)]], want))
    return bad


INV_GROUPS = [0, 1, 4, (1 << 64) - 1]
INV_OUT_BYTES = [96, 192, 48, 0]


def invalidate_model(valid, per_job, group, B, status, out, out_bytes, ok):
    """The header comment of k_invalidate_jobs restated: (status, out, ok) afterwards (None stays None)."""
    g = group or 1
    status, ok = (None if status is None else list(status)), (None if ok is None else list(ok))
    out = None if out is None else bytearray(out)
    for j in range(B):
        if all(valid[(j // g) * per_job + k] for k in range(per_job)):
            continue
        if status is not None and status[j] == OK:
            status[j] = INVALID
        if ok is not None:
            ok[j] = 0
        if out is not None:
            out[j * out_bytes:(j + 1) * out_bytes] = bytes(out_bytes)
            if out_bytes in (96, 192):
                out[j * out_bytes] = 0x40
    return status, out, ok


def run_invalidate(lib, per_job, group, B, out_bytes, null=None):
    """(what came back, the model's answer); null: "status", "ok" or "out" passed as a null pointer."""
    rnd = random.Random("single-kernels-invalidate-%d-%d-%d" % (per_job, group % 97, B))
    g = group or 1
    nrec = (B - 1) // g + 1
    valid = [int(rnd.randrange(4) != 0) for _ in range(nrec * per_job)]
    valid[0] = 0
    valid[-1] = 0
    if nrec > 2:
        valid[per_job] = 1 if per_job == 1 else valid[per_job]
    status = [rnd.choice([OK, OK, OK, NOT_ENOUGH, 2]) for _ in range(B)]
    status[0] = NOT_ENOUGH  # already not OK: keeps its value
    ok = [1] * B
    out = bytes([0xC3]) * (B * out_bytes)
    a_st = None if null == "status" else guarded(status)
    a_ok = None if null == "ok" else guarded(ok)
    a_out = None if null == "out" else guarded(np.frombuffer(out, dtype=np.uint8)) if not out_bytes else np.concatenate([u8(out), fresh(out_bytes)])
    call(lib, "invalidate_jobs", arr(valid, np.uint8), len(valid), per_job, group, B, a_st, a_out, out_bytes, a_ok)
    want = invalidate_model(valid, per_job, group, B, None if null == "status" else status, None if null == "out" else out, out_bytes,
                            None if null == "ok" else ok)
    return (a_st, a_out, a_ok), want


def check_invalidate(what, B, out_bytes, got, want):
    bad = []
    for name, a, w_, width in (("status", got[0], want[0], 1), ("out", got[1], want[1], out_bytes), ("ok", got[2], want[2], 1)):
        if a is None:
            continue
        if bytes(a[:B * width]) != bytes(w_):
            bad.append("%s: %s differs from the restatement" % (what, name))
        if width and not is_poison(a[B * width:]):
            bad.append("%s: the guard behind %s was written" % (what, name))
    return bad


def run_select(lib, N, need, jobs, with_present, with_bad, off_p, off_b, with_map, with_used):
    """(idx, slot, used, enough), and the inputs (present, bad, map, used before)."""
    rnd = random.Random("single-kernels-select-%d-%d-%d" % (N, need, jobs))
    present = [int(rnd.randrange(8) != 0) for _ in range(jobs * N)]
    badm = [int(rnd.randrange(6) == 0) for _ in range(jobs * N)]
    for j in range(0, jobs, 3):  # every third job: sparse, so that some lack `need` eligible slots and the scan reaches the row's end
        for i in range(N):
            present[j * N + i] = int(rnd.randrange(N) < need)
    if jobs > 1:
        present[(jobs - 1) * N:jobs * N] = [0] * (N - 1) + [1]  # the last job: only its last slot
    used_rows = jobs + 2
    order = list(range(used_rows))
    rnd.shuffle(order)
    mapping = order[:jobs] if with_map else None
    used0 = [rnd.randrange(2) * 7 for _ in range(used_rows * N)]
    idx, slot, enough = fresh(jobs * need + 1, np.uint64), fresh(jobs * need + 1, np.uint32), fresh(jobs + 1)
    used = guarded(used0) if with_used else None
    call(lib, "select_shares", arr(present, np.uint8) if with_present else None, arr(badm, np.uint8) if with_bad else None, off_p, off_b, N, need, jobs,
         arr(mapping, np.uint32) if with_map else None, used_rows, idx, slot, used, enough)
    return (idx, slot, used, enough), (present if with_present else None, badm if with_bad else None, mapping, used0)


def check_select(what, N, need, jobs, res, inputs):
    idx, slot, used, enough = res
    present, badm, mapping, used0 = inputs
    bad = []
    want_used = list(used0)
    lacking = 0
    for j in range(jobs):
        el = [i for i in range(N) if (present is None or present[j * N + i]) and (badm is None or not badm[j * N + i])][:need]
        full = len(el) == need
        lacking += not full
        want_slot = el + [NOSLOT] * (need - len(el))
        want_idx = el + [N + k for k in range(len(el), need)]
        if [int(v) for v in slot[j * need:(j + 1) * need]] != want_slot or [int(v) for v in idx[j * need:(j + 1) * need]] != want_idx:
            bad.append("%s job %d: slots %s, expected %s (or the abscissae differ)" % (what, j, [int(v) for v in slot[j * need:(j + 1) * need]], want_slot))
        if enough[j] != int(full):
            bad.append("%s job %d: enough = %d" % (what, j, enough[j]))
        if full:
            row = mapping[j] if mapping is not None else j
            for s in el:
                want_used[row * N + s] = 1
    if not is_poison(idx[jobs * need:]) or not is_poison(slot[jobs * need:]) or enough[jobs] != POISON:
        bad.append("%s: a guard entry (idx, slot, enough) was written" % what)
    if used is not None:
        if [int(v) for v in used[:len(want_used)]] != want_used:
            bad.append("%s: `used` differs (a job without enough shares must leave its row alone)" % what)
        if used[len(want_used)] != POISON:
            bad.append("%s: the guard byte behind `used` was written" % what)
    return bad[:12], lacking


SELECT_NS = [1, 7, 8, 9, 16, 17, 200]
SELECT_JOBS = [1, 65, 130]


def gather_selected_case(point_bytes, jobs, N=7, need=3):
    rnd = random.Random("single-kernels-gather-selected-%d-%d" % (point_bytes, jobs))
    shares = bytes(rnd.getrandbits(8) for _ in range(jobs * N * point_bytes))
    enough = [int(j % 4 != 1) for j in range(jobs)]
    slot = []
    for j in range(jobs):
        slot += sorted(rnd.sample(range(N), need)) if enough[j] else [NOSLOT] * need
    want = b""
    for i, s in enumerate(slot):
        j = i // need
        want += shares[(j * N + s) * point_bytes:(j * N + s + 1) * point_bytes] if enough[j] else b"\x40" + bytes(point_bytes - 1)
    return shares, enough, slot, want


def run_gather_selected(lib, point_bytes, jobs, form, off_s, off_d, N=7, need=3):
    shares, enough, slot, want = gather_selected_case(point_bytes, jobs, N, need)
    dst = fresh((jobs * need + 1) * point_bytes)
    call(lib, "gather_selected", u8(shares), N, need, point_bytes, arr(slot, np.uint32), arr(enough, np.uint8), jobs, form, off_s, off_d, dst)
    bad = []
    if bytes(dst[:len(want)]) != want:
        bad.append("gather_selected %d B jobs=%d form=%d offsets (%d, %d): wrong rows" % (point_bytes, jobs, form, off_s, off_d))
    if not is_poison(dst[len(want):]):
        bad.append("gather_selected %d B jobs=%d form=%d offsets (%d, %d): the guard row was written" % (point_bytes, jobs, form, off_s, off_d))
    return bad, dst


def run_mark(lib, rows_, with_present, with_bad):
    rnd = random.Random("single-kernels-mark-%d" % rows_)
    total = rows_ + 9
    present = [rnd.randrange(3) % 2 * 5 for _ in range(total)]  # 0 or 5: any non-zero byte counts
    rec = rnd.sample(range(total), rows_)
    ok = [rnd.randrange(2) * 3 for _ in range(rows_)]
    bad0 = [9] * total
    c_present, c_bad = fresh(rows_ + 1), fresh(rows_ + 1)
    a_bad = guarded(bad0) if with_bad else None
    call(lib, "robust_mark", arr(present, np.uint8) if with_present else None, arr(rec, np.uint32), arr(ok, np.uint8), rows_, total, c_present, c_bad, a_bad)
    want_p = [1 if (not with_present or present[s]) else 0 for s in rec]
    want_b = [1 if p and not k else 0 for p, k in zip(want_p, ok)]
    want_bad = list(bad0)
    for s, b in zip(rec, want_b):
        want_bad[s] = b
    bad = []
    what = "robust_mark rows=%d present=%d bad=%d" % (rows_, with_present, with_bad)
    if [int(v) for v in c_present[:rows_]] != want_p or [int(v) for v in c_bad[:rows_]] != want_b:
        bad.append("%s: wrong compacted masks" % what)
    if c_present[rows_] != POISON or c_bad[rows_] != POISON:
        bad.append("%s: a guard byte was written" % what)
    if with_bad and ([int(v) for v in a_bad[:total]] != want_bad or a_bad[total] != POISON):
        bad.append("%s: the caller's bad mask differs (an untouched share keeps its byte) or its guard was written" % what)
    return bad


def finish_table(need):
    """Every row of the truth table of k_robust_finish: (enough, st, ok, member) with ok None (a null pointer's stand-in when the
    whole array is null), 0 or 1 and member "ones", "zero first", "zero last"."""
    t = []
    for enough in (0, 1):
        for st in (OK, INVALID):
            for ok in (0, 1):
                for member in ("ones", "zero first", "zero last"):
                    t.append((enough, st, ok, member))
    return t


def run_finish(lib, N, point_bytes, with_ok, with_member, with_map, with_used, with_verdict, need=3):
    table = finish_table(need)
    jobs = len(table) * 3  # 72 jobs: more than one workgroup at 12 or 24 lanes per job
    rnd = random.Random("single-kernels-finish-%d-%d" % (N, point_bytes))
    rows_ = [table[(f * 7) % len(table)] for f in range(jobs)]
    total = jobs + 3
    order = list(range(total))
    rnd.shuffle(order)
    mapping = order[:jobs] if with_map else None
    enough = [r[0] for r in rows_]
    st = [r[1] for r in rows_]
    ok = [r[2] for r in rows_]
    member = []
    for r in rows_:
        member += {"ones": [1] * need, "zero first": [0] + [1] * (need - 1), "zero last": [1] * (need - 1) + [0]}[r[3]]
    comb = bytes(rnd.getrandbits(8) | 1 for _ in range(jobs * point_bytes))
    out0, status0, used0 = bytes([0x77]) * (total * point_bytes), [0x66] * total, [1] * (total * N)
    a_out, a_status = np.concatenate([np.frombuffer(out0, dtype=np.uint8), fresh(point_bytes)]), guarded(status0)
    a_used = guarded(used0) if with_used else None
    verdict = fresh(jobs + 1) if with_verdict else None
    call(lib, "robust_finish", arr(mapping, np.uint32) if with_map else None, N, need, point_bytes, jobs, total, arr(enough, np.uint8), arr(st, np.uint8),
         arr(ok, np.uint8) if with_ok else None, arr(member, np.uint8) if with_member else None, u8(comb), a_out, a_status, a_used, verdict)
    # the header comment restated
    w_out, w_status, w_used, w_verdict = bytearray(out0), list(status0), list(used0), []
    for f in range(jobs):
        job = mapping[f] if with_map else f
        good = bool(enough[f]) and st[f] == OK and (not with_ok or ok[f]) and (not with_member or all(member[f * need:(f + 1) * need]))
        w_out[job * point_bytes:(job + 1) * point_bytes] = comb[f * point_bytes:(f + 1) * point_bytes] if good else b"\x40" + bytes(point_bytes - 1)
        w_status[job] = OK if good else NOT_ENOUGH
        if enough[f] and not good:
            w_used[job * N:(job + 1) * N] = [0] * N
        w_verdict.append(GOOD_V if good else RETRY_V if enough[f] else NOT_ENOUGH_V)
    what = "robust_finish N=%d %d B ok=%d member=%d map=%d used=%d verdict=%d" % (N, point_bytes, with_ok, with_member, with_map, with_used, with_verdict)
    bad = []
    if bytes(a_out[:total * point_bytes]) != bytes(w_out):
        bad.append("%s: wrong output rows (a failed job gets the identity, an unmapped row stays)" % what)
    if [int(v) for v in a_status[:total]] != w_status:
        bad.append("%s: wrong status codes" % what)
    if not is_poison(a_out[total * point_bytes:]) or a_status[total] != POISON:
        bad.append("%s: a guard (out row, status byte) was written" % what)
    if with_used and ([int(v) for v in a_used[:total * N]] != w_used or a_used[total * N] != POISON):
        bad.append("%s: `used` differs (cleared once for a job whose combination does not stand, untouched otherwise) or its guard was written" % what)
    if with_verdict and ([int(v) for v in verdict[:jobs]] != w_verdict or verdict[jobs] != POISON):
        bad.append("%s: wrong verdicts or guard" % what)
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# 4. k_hash.hip
# ---------------------------------------------------------------------------------------------------------------------
HASH_B = [1, 2, 63, 65]
HASH_LENS = [0, 1, 63, 64, 65, 135, 136, 137, 300]
# dealt so that the two messages of a pair differ widely: 300 beside 0, 1 beside 137, ...
HASH_DEAL = [300, 0, 1, 137, 136, 63, 64, 135, 65, 300, 65, 0, 137, 1, 63, 136, 135, 64]


def hash_case(B, with_g1, bad_at=None):
    """(g1 operands or None, messages).  Two G1 operands in turn; bad_at: the position of an operand that does not decode."""
    msgs = [message(HASH_DEAL[j % len(HASH_DEAL)]) for j in range(B)]
    if not with_g1:
        return None, msgs
    pl = pool(1)
    g1 = [enc(1, gmul(1, pl[j % 2])) for j in range(B)]
    if bad_at is not None:
        g1[bad_at] = BAD[1] if bad_at % 2 else off_curve(1)
    return g1, msgs


def hash_bad_ats(B, with_g1):
    """Where the operand that does not decode stands: nowhere; slot a, slot b and the odd tail of B = 65; the only job of B = 1."""
    if not with_g1:
        return [None]
    return {65: [None, 0, 1, 64], 1: [None, 0]}.get(B, [None])


def run_hash(lib, g1, msgs, fix, form, with_status=1):
    B = len(msgs)
    out, status = fresh((B + 1) * 192), fresh(B + 1)
    call(lib, "hash", u8(b"".join(g1)) if g1 else None, u8(b"".join(msgs)), offsets(len(m) for m in msgs), B, fix, form, with_status, out, status)
    return out, status


def check_hash(what, g1, msgs, fix, with_status, res):
    out, status = res
    B = len(msgs)
    bad = []
    if not is_poison(out[B * 192:]) or status[B] != POISON:
        bad.append("%s: the guard row or byte was written" % what)
    if (g1 is None or not with_status) and not is_poison(status):
        bad.append("%s: status written by a kernel that has none (or though null was passed)" % what)
    for j, m in enumerate(msgs):
        st, want = (OK, dc.hash_g2_ref(m, fix)) if g1 is None else dc.hash_g1_g2_ref(g1[j], m, fix)
        if bytes(out[j * 192:(j + 1) * 192]) != want or (g1 is not None and with_status and status[j] != st):
            bad.append("%s message %d (%d bytes): wrong point or status %d" % (what, j, len(m), status[j]))
    return bad[:12]


XOR_LENS = [0, 1, 63, 64, 65, 200]


def run_xor(lib, B, with_status):
    pl = pool(1)
    lens = [XOR_LENS[j % len(XOR_LENS)] for j in range(B)]
    data = [message(n, 1) for n in lens]
    pts = [gmul(1, pl[j % 3]) for j in range(B)]
    g1 = [enc(1, p) for p in pts]
    status0 = [OK] * B
    want_out = []
    for j in range(B):
        kind = j % 7
        if kind == 3:
            g1[j] = BAD[1]          # does not decode: status 3, nothing written
        if kind == 5 and with_status:
            status0[j] = NOT_ENOUGH  # flagged by an earlier stage: skipped
        want_out.append(bytes([POISON]) * lens[j] if kind == 3 or (kind == 5 and with_status) else o.xor_with_hash(pts[j], data[j]))
    status = guarded(status0) if with_status else None
    off = offsets(lens)
    out = fresh(int(off[B]) + 1)
    call(lib, "xor_with_hash", u8(b"".join(g1)), u8(b"".join(data)), off, B, status, out)
    bad = []
    if bytes(out[:int(off[B])]) != b"".join(want_out) or out[int(off[B])] != POISON:
        bad.append("xor_with_hash B=%d: wrong bytes (a failed or flagged job leaves its bytes as filled) or the guard byte was written" % B)
    if with_status:
        want_st = [INVALID if j % 7 == 3 else status0[j] for j in range(B)]
        if [int(v) for v in status[:B]] != want_st or status[B] != POISON:
            bad.append("xor_with_hash B=%d: wrong status bytes" % B)
    return bad


def run_encrypt(lib, B, pk_stride, with_status=1):
    pl = pool(1)
    rnd = random.Random("single-kernels-encrypt")
    rs = [rnd.randrange(1, R) for _ in range(3)]
    lens = [[0, 1, 33, 64, 65, 130][j % 6] for j in range(B)]
    msgs = [message(n, 2) for n in lens]
    pks = [pl[j % 2] if pk_stride else pl[0] for j in range(B)]
    r = [rs[j % 3] for j in range(B)]
    bad_pk = set()
    if B > 4:
        r[2] = R           # a non-canonical r
        r[B - 1] = RF - 1
        if pk_stride:
            bad_pk = {4}
    pk_bytes = b"".join(BAD[1] if j in bad_pk else enc(1, gmul(1, pks[j])) for j in range(B)) if pk_stride else enc(1, gmul(1, pks[0]))
    off = offsets(lens)
    u, v, w, status = fresh((B + 1) * 96), fresh(int(off[B]) + 1), fresh((B + 1) * 192), fresh(B + 1)
    call(lib, "encrypt", u8(pk_bytes), pk_stride, u8(b"".join(fr32(k) for k in r)), u8(b"".join(msgs)), off, B, with_status, u, v, w, status)
    bad = []
    what = "encrypt B=%d pk_stride=%d" % (B, pk_stride)
    if not is_poison(u[B * 96:]) or v[int(off[B])] != POISON or not is_poison(w[B * 192:]) or status[B] != POISON:
        bad.append("%s: a guard (u row, v byte, w row, status byte) was written" % what)
    if not with_status and not is_poison(status):
        bad.append("%s: status written though null was passed" % what)
    for j in range(B):
        if r[j] >= R or j in bad_pk:
            want = (IDENT[1], bytes(lens[j]), IDENT[2], INVALID)
        else:
            def ref(j=j):
                cu, cv, cw = o.encrypt_with_r(gmul(1, pks[j]), r[j], msgs[j])
                return enc(1, cu), cv, enc(2, cw), OK
            want = dc.cached("sk-encrypt", (pks[j], r[j], msgs[j]), ref)
        got = (bytes(u[j * 96:(j + 1) * 96]), bytes(v[int(off[j]):int(off[j + 1])]), bytes(w[j * 192:(j + 1) * 192]), status[j] if with_status else want[3])
        if got != want:
            bad.append("%s job %d: wrong %s" % (what, j, [n for n, a, b in zip(("u", "v", "w", "status"), got, want) if a != b]))
    return bad[:12]


EVAL_TS = [0, 1, 2, 7]
EVAL_IDX = [0, 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1]  # the last: x = idx + 1 = 0, INVALID


def eval_commits(t):
    """Commitments of degree t as multiples of g1 (None: off the curve): random, identity coefficients, an off-curve coefficient at
    the top and further down, and -- for x = 2 = idx 1 -- a Horner step whose `acc` equals the next coefficient and one whose `acc`
    equals its negative."""
    rnd = random.Random("single-kernels-eval-%d" % t)
    fresh_m = lambda: [rnd.randrange(1, R) for _ in range(t + 1)]
    out = [(fresh_m(), "random")]
    out.append(([0] * (t + 1), "all identity"))
    m = fresh_m()
    m[t] = 0
    out.append((m, "identity at the top"))
    m = fresh_m()
    m[t] = None
    out.append((m, "off-curve at the top"))
    if t >= 1:
        m = fresh_m()
        m[0] = 0
        out.append((m, "identity at the bottom"))
        m = fresh_m()
        m[t - 1] = 2 * m[t] % R
        out.append((m, "acc == c at x = 2"))
        m = fresh_m()
        m[t - 1] = (-2 * m[t]) % R
        out.append((m, "acc == -c at x = 2"))
        m = fresh_m()
        m[0] = None
        out.append((m, "off-curve further down"))
    if t >= 2:
        m = fresh_m()
        m[t - 2] = (2 * (2 * m[t] + m[t - 1])) % R
        out.append((m, "acc == c at the second step, x = 2"))
    return out


def eval_want(m, idx):
    x = (idx + 1) & dk.M64
    if x == 0 or any(c is None for c in m):
        return IDENT[1], INVALID
    res, events = dk.horner(m, x)
    return enc(1, gmul(1, res)), OK


def run_eval(lib, m, t, idxs, with_status=1):
    M = len(idxs)
    commit = b"".join(off_curve(1) if c is None else enc(1, gmul(1, c)) for c in m)
    out, status = fresh((M + 1) * 96), fresh(M + 1)
    call(lib, "commitment_evaluate", u8(commit), t, arr(idxs, np.uint64), M, with_status, out, status)
    return out, status


def eval_idxs(M):
    return [EVAL_IDX[j % len(EVAL_IDX)] if j < 10 else 2 + j % 7 for j in range(M)]


# ---------------------------------------------------------------------------------------------------------------------
# mode tables of the kernels above
# ---------------------------------------------------------------------------------------------------------------------
def select_modes(need, jobs):
    """(present, bad, off_p, off_b, map, used): both masks at the same offset from an 8-byte boundary (select_first's word path, with
    a bytewise head) and at different ones (its bytewise path), each mask null in turn, map / used null and given."""
    modes = [(1, 1, 3, 3, 1, 1), (1, 1, 3, 4, 1, 1), (1, 1, 1, 9, 0, 1)]
    if jobs == 65:
        modes += [(1, 0, 5, 0, 1, 1), (0, 1, 0, 2, 0, 1), (0, 0, 0, 0, 1, 1), (1, 1, 0, 0, 1, 0)]
    return modes


def invalidate_cases():
    """(per_job, group, B, out_bytes, null)"""
    cases = [(per_job, group, B, 96, None) for per_job in (1, 3) for group in INV_GROUPS for B in (1, 65, 130)]
    cases += [(3, 1, 65, ob, None) for ob in INV_OUT_BYTES[1:]]
    cases += [(1, 4, 65, 96, null) for null in ("status", "ok", "out")]
    return cases


GATHER_SELECTED_FORMS = [(0, 0, 0), (16, 0, 0), (8, 0, 0), (0, 8, 0), (0, 0, 8), (0, 8, 8), (8, 8, 8)]  # (form, off_shares, off_dst)
MARK_MODES = [(1, 1), (1, 0), (0, 1), (0, 0)]  # (present, bad) given


def finish_modes():
    """(ok, member, map, used, verdict) given: everything, then each null in turn, then nothing optional."""
    return [(1, 1, 1, 1, 1), (0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (0, 0, 0, 0, 0)]


def run_movers(lib):
    """k_ok_and_status, k_gather_rows (rows of 8, 96 and 192 bytes, repeated map entries), k_scatter_bytes, k_gather_bytes."""
    rnd = random.Random("single-kernels-movers")
    bad = []
    for B in (1, 65, 130):
        status = [rnd.choice([OK, OK, NOT_ENOUGH, INVALID]) for _ in range(B)]
        ok0 = [rnd.randrange(2) for _ in range(B)]
        ok = guarded(ok0)
        call(lib, "ok_and_status", arr(status, np.uint8), B, ok)
        if [int(v) for v in ok[:B]] != [a if s == OK else 0 for a, s in zip(ok0, status)] or ok[B] != POISON:
            bad.append("ok_and_status B=%d: wrong bytes or guard" % B)
    for row_bytes in (8, 96, 192):
        for rows_ in (1, 23, 70):
            src_rows = 9
            src = bytes(rnd.getrandbits(8) for _ in range(src_rows * row_bytes))
            m = [rnd.randrange(src_rows) for _ in range(rows_)]
            if rows_ > 2:
                m[1] = m[0]
                m[-1] = src_rows - 1
            dst = fresh((rows_ + 1) * row_bytes)
            call(lib, "gather_rows", u8(src), src_rows, row_bytes, arr(m, np.uint32), rows_, dst)
            if bytes(dst[:rows_ * row_bytes]) != b"".join(src[r * row_bytes:(r + 1) * row_bytes] for r in m) or not is_poison(dst[rows_ * row_bytes:]):
                bad.append("gather_rows %d B x %d: wrong rows or guard" % (row_bytes, rows_))
    for rows_ in (1, 65, 130):
        other = rows_ + 11
        src = [rnd.getrandbits(8) for _ in range(rows_)]
        m = rnd.sample(range(other), rows_)
        dst = fresh(other + 1)
        call(lib, "move_bytes", 1, arr(src, np.uint8), arr(m, np.uint32), rows_, other, dst)
        want = [POISON] * other
        for r in range(rows_):
            want[m[r]] = src[r]
        if [int(v) for v in dst[:other]] != want or dst[other] != POISON:
            bad.append("scatter_bytes rows=%d: wrong bytes or guard" % rows_)
        src = [rnd.getrandbits(8) for _ in range(other)]
        m = [rnd.randrange(other) for _ in range(rows_)]
        dst = fresh(rows_ + 1)
        call(lib, "move_bytes", 0, arr(src, np.uint8), arr(m, np.uint32), rows_, other, dst)
        if [int(v) for v in dst[:rows_]] != [src[i] for i in m] or dst[rows_] != POISON:
            bad.append("gather_bytes rows=%d: wrong bytes or guard" % rows_)
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the text of the kernels that have no header routine, transcribed lane by lane (CPU leg only)
# ---------------------------------------------------------------------------------------------------------------------
class KernelText:
    """k_rlc_scalars*, k_invalidate_jobs, k_ok_and_status, k_gather_rows, k_scatter_bytes, k_gather_bytes, k_take_u64,
    k_gather_selected, k_robust_mark and k_robust_finish as their text reads: a loop over the lanes of the launch (lanes past the end
    included), the arithmetic on machine words, behind their launchers' rules.  It stands in for the device harness in the CPU leg,
    so the restatements and checkers are proven against something that is not themselves.  fault: one of the faults the suite must
    notice -- "counter & 63", "no | 1", "used from w + row_words" -- or "used stride 1" (it leaves the same bytes)."""
    python, host = True, False

    def __init__(self, fault=None):
        self.fault = fault

    def get(self, key, default=None):
        return getattr(self, key, default)

    def __getitem__(self, name):
        return getattr(self, name)

    @staticmethod
    def _lanes(n):
        return range((n + 63) // 64 * 64)

    def rlc_scalars(self, g1, seed, n, out):
        M = (1 << 64) - 1
        key = [int.from_bytes(bytes(seed[4 * w:4 * w + 4]), "little") for w in range(8)]
        for i in self._lanes(n):
            if i >= n:
                continue
            block = o.chacha20_block(key, i & 63 if self.fault == "counter & 63" else i)
            w0, w1 = block[0], block[1]
            one = 0 if self.fault == "no | 1" else 1
            if g1:
                a, b = (w0 | one), w1
                x2lo, x2hi = X2 & M, X2 >> 64
                c = x2lo * b + a
                acc = [c & M, 0, 0, 0]
                c = (c >> 64) + x2hi * b
                acc[1], acc[2] = c & M, (c >> 64) & M
            else:
                d = [(w0 & 0xffff) | one, w0 >> 16, w1 & 0xffff, w1 >> 16]
                acc = [d[3], 0, 0, 0]
                for j in (2, 1, 0):
                    carry = d[j]
                    for w in range(4):
                        carry += acc[w] * X
                        acc[w] = carry & M
                        carry >>= 64
            for w in range(4):
                for b_ in range(8):
                    out[i * 32 + 8 * w + b_] = (acc[w] >> (8 * b_)) & 0xff
        return 0

    def invalidate_jobs(self, valid, valid_len, per_job, group, B, status, out, out_bytes, ok):
        group = group or 1
        for j in self._lanes(B):
            if j >= B:
                continue
            good = True
            for k in range(per_job):
                good = good and valid[(j // group) * per_job + k] != 0
            if good:
                continue
            if status is not None and status[j] == OK:
                status[j] = INVALID
            if ok is not None:
                ok[j] = 0
            if out is not None:
                for b in range(out_bytes):
                    out[j * out_bytes + b] = 0
                if out_bytes in (96, 192):
                    out[j * out_bytes] = 0x40
        return 0

    def ok_and_status(self, status, B, ok):
        for j in self._lanes(B):
            if j < B and status[j] != OK:
                ok[j] = 0
        return 0

    def gather_rows(self, src, src_rows, row_bytes, map_, rows_, dst):
        row_words = row_bytes // 8
        s64, d64 = src.view(np.uint64), dst.view(np.uint64)
        for t in self._lanes(rows_ * row_words):
            if t >= rows_ * row_words:
                continue
            r, w = t // row_words, t % row_words
            d64[t] = s64[int(map_[r]) * row_words + w]
        return 0

    def move_bytes(self, scatter, src, map_, rows_, other, dst):
        for r in self._lanes(rows_):
            if r < rows_:
                if scatter:
                    dst[int(map_[r])] = src[r]
                else:
                    dst[r] = src[int(map_[r])]
        return 0

    def take_u64(self, in_, npj, take, B, out):
        n = B * take
        for i in self._lanes(n):
            if i < n:
                out[i] = in_[(i // take) * npj + i % take]
        return 0

    def gather_selected(self, shares, N, need, point_bytes, slot, enough, jobs, form, off_s, off_d, dst):
        V = 16 if form == 16 or (form == 0 and (off_s | off_d) & 15 == 0) else 8
        rw = point_bytes // V
        for i in self._lanes(jobs * need * rw):
            if i >= jobs * need * rw:
                continue
            rec, w = i // rw, i % rw
            j = rec // need
            if enough[j]:
                at = ((j * N + int(slot[rec])) * rw + w) * V
                val = bytes(shares[at:at + V])
            else:
                val = (b"\x40" if w == 0 else b"\x00") + bytes(V - 1)
            dst[i * V:(i + 1) * V] = np.frombuffer(val, dtype=np.uint8)
        return 0

    def robust_mark(self, present, rec, ok, rows_, total, c_present, c_bad, bad):
        for r in self._lanes(rows_):
            if r >= rows_:
                continue
            src = int(rec[r])
            p = 1 if (present is None or present[src] != 0) else 0
            b = 1 if (p and ok[r] == 0) else 0
            c_present[r] = p
            c_bad[r] = b
            if bad is not None:
                bad[src] = b
        return 0

    def robust_finish(self, map_, N, need, point_bytes, jobs, total, enough, st, ok, member, comb, out, status, used, verdict):
        rw = point_bytes // 8
        for i in self._lanes(jobs * rw):
            if i >= jobs * rw:
                continue
            f, w = i // rw, i % rw
            job = int(map_[f]) if map_ is not None else f
            full = enough[f] != 0
            good = full and st[f] == OK and (ok is None or ok[f] != 0)
            if good and member is not None:
                for k in range(need):
                    good = good and member[f * need + k] != 0
            val = bytes(comb[i * 8:i * 8 + 8]) if good else (b"\x40" if w == 0 else b"\x00") + bytes(7)
            out[(job * rw + w) * 8:(job * rw + w) * 8 + 8] = np.frombuffer(val, dtype=np.uint8)
            if used is not None and full and not good:
                start, step = {"used stride 1": (w, 1), "used from w + row_words": (w + rw, rw)}.get(self.fault, (w, rw))
                for k in range(start, N, step):
                    used[job * N + k] = 0
            if w == 0:
                status[job] = OK if good else NOT_ENOUGH
                if verdict is not None:
                    verdict[f] = GOOD_V if good else (RETRY_V if full else NOT_ENOUGH_V)
        return 0
