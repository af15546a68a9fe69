"""DKG kernel conformance: the 36 kernels of threshold_crypto_amd/csrc/k_dkg.hip, launched directly and compared byte for byte.

The third kernel-level suite (after tests/device_conformance.py and tests/manypoint_conformance.py, whose helpers and build recipe it
reuses).  tests/device/dkg_kernels.hip includes k_dkg.hip as it is and launches every kernel THROUGH THE PRODUCT'S LAUNCHER with
`cus`, `parts` and `slices` chosen by the test; every buffer a kernel writes is filled with 0x5A first and carries one guard row /
byte / entry behind it, and everything comes back: outputs, statuses, the other one of status / part_ok, term_bad, the interpolation
workspaces, the Montgomery matrices, the recoded weights, the intermediate arrays of the resharing verdict.
tests/device/dkg_kernels_host.cpp runs the same header routines (tc_dkg.h) with g++ -DTC_BOUND_CHECK over the same buffers.

Expected values come from the big-integer oracle (oracle/tc_oracle.py) and from plain restatements of the header comments, never
from the code under test.  Points are known multiples a g1, so a sum, a weighted sum or a commitment row costs one oracle
multiplication per DISTINCT output; invalid encodings are ordinary data.  All comparisons are exact.

  legs   "dk_": the device harness (tests/test_gpu_dkg_kernels.py); "dkh_": the host leg (tests/test_dkg_kernels_host.py).  The host
         leg does not see lane pairing, the shuffle merge, the indexing or the launch geometry, and parts / slices = 0 (the
         launcher's rule) run on the device only; the word-copy kernels, the two comparisons and the generate verdict have no header
         routine, so they have no host entry: their models are plain Python.
"""
import ctypes
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import manypoint_conformance as mp  # noqa: E402
from manypoint_conformance import enc, pool, gmul, neg_mult, HipError, POISON  # noqa: E402

dc, o = mp.dc, mp.o
R, P, X2 = o.R, o.Q, mp.X2
OK, NOT_ENOUGH, DUPLICATE, INVALID, MISMATCH = 0, 1, 2, 3, 4  # tc_codec.h TC_JOB_*
IDENT = enc(1, None)
BAD = mp.BAD_POINT[1]  # x >= p
RF = 1 << 256
M64 = (1 << 64) - 1
PARTS = [0, 1, 2, 4, 8, 16, 32, 64, 3, 128]  # 0: the launcher's rule (device only); 3, 128: illegal, run as 1
KEEP = 0x11  # what out_commit / out_share hold before a guard kernel runs


def off_curve():
    """A point with a canonical x and a y that is not on the curve (y + 1)."""
    b = bytearray(enc(1, gmul(1, 7)))
    b[95] ^= 1
    return bytes(b)


# ---------------------------------------------------------------------------------------------------------------------
# builds and entries
# ---------------------------------------------------------------------------------------------------------------------
def build_device():
    """tests/device/dkg_kernels.hip -> a gfx950 shared object, with the product's compiler flags (build.py FLAGS)."""
    from threshold_crypto_amd import build as tcb
    src = os.path.join(mp.DEV, "dkg_kernels.hip")
    return dc._build("libtc_dkg_kernels", lambda out: [dc.hipcc()] + tcb.FLAGS + ["-w", "-shared", src, "-o", out], {"dkg_kernels.hip"})


def build_host():
    src = os.path.join(mp.DEV, "dkg_kernels_host.cpp")
    return dc._build("libtc_dkg_kernels_host_bc",
                     lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-shared", "-fPIC", src, "-o", out],
                     {"dkg_kernels_host.cpp"})


def build_host_main(extra=()):
    """The stand-alone program of dkg_kernels_host.cpp (its fixed short case list); extra: e.g. sanitizer flags."""
    src = os.path.join(mp.DEV, "dkg_kernels_host.cpp")
    return dc._build("dkg_kernels_host_main",
                     lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-DDK_MAIN"] + list(extra) + [src, "-o", out],
                     {"dkg_kernels_host.cpp"})


# i: int, z: size_t, p: pointer -- the arguments of the entries of dkg_kernels.hip / dkg_kernels_host.cpp
SIG = {"fixed_base_table": "p", "g1_fixed_base": "pziipp", "commitment_rows": "ipzzzpzzipp", "fr_interpolate": "zppzippp",
       "fr_interpolate_at_zero": "zpppzpp", "to_mont": "pzzipp", "fr_poly_evaluate": "pzpzzipp", "bivar_poly_row": "pzpzipp",
       "fr_sum": "pzzzppzipp", "g1_sum": "ipzzzppzziiipppp", "g1_wsum": "ipzzzpzppzzzipiz" + "p" * 7, "rlc_scalars": "pppzzzpp",
       "reshare_chain": "ppzppzzzpppz" + "p" * 13}
SIG_DEVICE_ONLY = {"copy_points": "ipzzzpzp", "g1_compare": "ppppzzp", "generate_verdict": "pppzzppp"}
_CT = {"i": ctypes.c_int, "z": ctypes.c_size_t, "p": ctypes.c_void_p}


def load(path, prefix):
    lib = ctypes.CDLL(path)
    host = prefix == "dkh_"
    entries = {}
    for name, sig in list(SIG.items()) + ([] if host else list(SIG_DEVICE_ONLY.items())):
        f = getattr(lib, prefix + name)
        f.argtypes = [_CT[c] for c in sig]
        f.restype = ctypes.c_int
        entries[name] = f
    if host:
        lib.dkh_sum_part.argtypes = [ctypes.c_size_t] * 5 + [ctypes.c_void_p]
        lib.dkh_sum_part.restype = None
    return dict(entries, lib=lib, host=host)


def call(lib, name, *args):
    """One entry; numpy arrays go in as pointers.  A non-zero return (the first HIP error) raises HipError."""
    conv = [a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    rc = lib[name](*conv)
    if rc != 0:
        raise HipError("%s: the harness returned %d" % (name, rc))


def fresh(count, dtype=np.uint8):
    return np.frombuffer(bytes([POISON]) * (count * np.dtype(dtype).itemsize), dtype=dtype).copy()


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, dtype=np.uint8)


def fr32(v):
    return int(v).to_bytes(32, "little")


def words8(v):
    return [(int(v) >> (32 * i)) & 0xffffffff for i in range(8)]


def is_poison(a):
    return bool((np.asarray(a).view(np.uint8) == POISON).all())


def same(res, ref):
    return all((a == b).all() for a, b in zip(res, ref))


def rows(a, width):
    return [bytes(a[i * width:(i + 1) * width]) for i in range(len(a) // width)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fixed-base table and multiplication
# ---------------------------------------------------------------------------------------------------------------------
def fb_digits(k):
    """g1_fixed_base_mul's signed windows restated: ([(magnitude, negative)] for windows 0 .. 63, the carry left over)."""
    carry, out = 0, []
    for w in range(64):
        v = ((k >> (4 * w)) & 15) + carry  # 0 .. 16
        neg = v > 8
        carry = 1 if neg else 0
        out.append((16 - v if neg else v, neg))
    return out, carry


def fb_value(digits, carry):
    return sum((-m if neg else m) << (4 * w) for w, (m, neg) in enumerate(digits)) + (carry << 256)


_FB = {}


def fb_table_model():
    """[m 16^w] g1 for w = 0 .. 63, m = 1 .. 8 by the oracle's additions and doublings."""
    if "tbl" not in _FB:
        pts, base = [], o.G1_GEN
        for _ in range(64):
            acc = None
            for _m in range(8):
                acc = o.E1.add(acc, base)
                pts.append(acc)
            for _d in range(4):
                base = o.E1.dbl(base)
        _FB["tbl"] = pts
    return _FB["tbl"]


def run_fb_table(lib):
    tbl = fresh(513 * 28, np.int32)
    call(lib, "fixed_base_table", tbl)
    return tbl.reshape(513, 28)


LIMB_TOP = int(mp.dc.NORM_HI * (1 << dc.RB))  # g1_fixed_base_mul reads every entry as limbs in [0, 1.001] 2^28, value <= 2.1 p


def check_fb_table(tbl, guard=True):
    bad = []
    if guard and not is_poison(tbl[512]):
        bad.append("the entry behind the table was written")
    want = fb_table_model()
    for e in range(512):
        for c, name in ((0, "x"), (1, "y")):
            l = [int(v) for v in tbl[e, 14 * c:14 * c + 14]]
            if not all(0 <= v <= LIMB_TOP for v in l):
                bad.append("entry %d %s: limbs outside [0, 1.001] 2^28: %s" % (e, name, l))
            v = dc.value(l)
            if v > 2.1 * P:
                bad.append("entry %d %s: value %.2f p" % (e, name, v / P))
            if v * dc.RINV % P != want[e][c]:
                bad.append("entry %d (window %d, m = %d): wrong %s" % (e, e // 8, e % 8 + 1, name))
        if len(bad) > 12:
            break
    return bad


def fb_directed():
    """(scalar, what it is for): every reachable digit at windows 0, 31 and 62, the all-0xF carry chain, the edges."""
    out = []
    for w in (0, 31, 62):
        for d in range(1, 9):
            out.append((d << (4 * w), "digit +%d at window %d" % (d, w)))
        for d in range(1, 8):
            out.append(((16 - d) << (4 * w), "digit -%d at window %d" % (d, w)))
    out += [(m << 252, "entry (63, %d)" % m) for m in range(1, 8)]
    out.append(((1 << 80) - 7, "nibble 9, then nineteen 0xF nibbles (v = 16: magnitude 0 with carry)"))
    out.append(((0xfff9 << 236), "a carry chain into window 63"))
    out += [(0, "0"), (1, "1"), (R - 1, "r - 1"), (R - 2, "r - 2"), (R, "r"), ((1 << 256) - 1, "2^256 - 1")]
    return out


class FbCase:
    def __init__(self):
        rnd = random.Random("dkg-kernels-fb")
        self.directed = fb_directed()
        self.scalars = [k for k, _ in self.directed] + [rnd.randrange(R) for _ in range(32)]
        self.tag = "fixed base"
        self._want = {}

    def fr(self, M):
        return [self.scalars[(5 * j) % len(self.scalars)] if M > len(self.scalars) else self.scalars[j] for j in range(M)]

    def want(self, k):
        if k not in self._want:
            self._want[k] = (IDENT, INVALID) if k >= R else (enc(1, gmul(1, k)), OK)
        return self._want[k]


def fb_case():
    if "case" not in _FB:
        _FB["case"] = FbCase()
    return _FB["case"]


FB_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (513, 1), (1061, 1), (1061, 0)]  # (M, cus); cus = 1: two workgroups
FB_ALL = len(fb_directed()) + 32


def run_fb(lib, case, M, cus, with_status):
    fr = u8(b"".join(fr32(k) for k in case.fr(M)))
    out, status = fresh((M + 1) * 96), fresh(M + 1)
    call(lib, "g1_fixed_base", fr, M, cus, with_status, out, status)
    return out, status


def check_fb(case, M, with_status, res, oracle_rows=None):
    out, status = res
    bad = []
    if not is_poison(out[M * 96:]) or status[M] != POISON:
        bad.append("M = %d: the guard row or byte was written" % M)
    if not with_status and not is_poison(status):
        bad.append("M = %d: status written though null was passed" % M)
    for j, k in enumerate(case.fr(M)):
        if oracle_rows is not None and j >= oracle_rows:
            break
        pt, st = case.want(k)
        if bytes(out[j * 96:(j + 1) * 96]) != pt or (with_status and status[j] != st):
            bad.append("M = %d row %d (k = %x): wrong product or status %d" % (M, j, k, status[j]))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# 2. rows and evaluations in G1
# ---------------------------------------------------------------------------------------------------------------------
XS = [0, 1, 2, 1 << 63, M64, 3, 0xd201000000010000, 5]  # cycled; the first five are the edges


def tri(degree):
    return (degree + 1) * (degree + 2) // 2


class Commit:
    """A bivariate commitment as multiples of g1 (None: an entry that does not decode), or a row (kind "row": degree + 1 entries)."""

    def __init__(self, mults, tag, bad_bytes=None):
        self.m, self.tag, self.bad_bytes = mults, tag, bad_bytes or BAD

    def bytes(self):
        return b"".join(self.bad_bytes if a is None else enc(1, gmul(1, a)) for a in self.m)


def horner(coeffs, x):
    """Horner over multiples as job_bivar_commitment_row / job_commitment_evaluate_at walk it: (result or None when a coefficient
    does not decode, the events "double" (c = [x] res, not the identity) and "cancel" (c = -[x] res))."""
    ok = all(c is not None for c in coeffs)
    cs = [0 if c is None else c for c in coeffs]
    res, ev = cs[-1], []
    for c in reversed(cs[:-1]):
        scaled = res * x % R
        if scaled and scaled == c:
            ev.append("double")
        if scaled and (scaled + c) % R == 0:
            ev.append("cancel")
        res = (scaled + c) % R
    return (res if ok else None), ev


def row_coeffs(commit, degree, i):
    return [commit.m[o.coeff_pos(i, j)] for j in range(degree + 1)]


def directed_commits(degree, rnd):
    """Bivariate commitments of one degree >= 2; the Horner events are for the abscissa 2."""
    n = tri(degree)

    def fresh_m():
        return [rnd.randrange(1, R) for _ in range(n)]
    out = []
    m = fresh_m()
    for i in range(degree + 1):
        m[o.coeff_pos(i, degree)] = 0
    out.append(Commit(m, "identity at the top"))
    m = fresh_m()
    for i in range(degree + 1):
        m[o.coeff_pos(i, degree // 2)] = 0
    out.append(Commit(m, "identity in the middle"))
    out.append(Commit([0] * n, "all identity"))
    m = fresh_m()
    m[o.coeff_pos(0, degree - 1)] = (-2 * m[o.coeff_pos(0, degree)]) % R  # row 0: the first step meets -[2] res, then goes on
    m[o.coeff_pos(1, degree - 1)] = 2 * m[o.coeff_pos(1, degree)] % R     # row 1: the first step meets [2] res
    out.append(Commit(m, "Horner meets c = -[x] res and c = [x] res at x = 2"))
    m = fresh_m()
    m[o.coeff_pos(1, degree)] = None
    out.append(Commit(m, "one off-curve coefficient", off_curve()))
    return out


class RowsCase:
    """form 0: one commitment, B abscissae; 1: B commitments `stride` apart, one abscissa each; 2: B rows, n abscissae each."""

    def __init__(self, form, degree, B, n=0, directed=False, slack=0, tag=""):
        rnd = random.Random("dkg-kernels-rows-%d-%d-%d-%d" % (form, degree, B, n))
        self.form, self.degree, self.B, self.n = form, degree, B, n
        per = degree + 1
        size = per if form == 2 else tri(degree)
        self.commit_size = size * 96
        self.stride = self.commit_size + slack * 96
        pl = pool(1)
        kinds = [Commit([pl[rnd.randrange(len(pl))] for _ in range(size)], "random %d" % i) for i in range(2)]
        if directed and form != 2:
            kinds += directed_commits(degree, rnd)
        if directed and form == 2:
            r = [rnd.randrange(1, R) for _ in range(per)]
            kinds.append(Commit([0 if i == degree else a for i, a in enumerate(r)], "identity at the top"))
            kinds.append(Commit([0] * per, "all identity"))
            kinds.append(Commit(r[:-2] + [2 * r[-1] % R, r[-1]], "Horner meets c = [x] res at x = 2"))
            kinds.append(Commit(r[:-2] + [(-2 * r[-1]) % R, r[-1]], "Horner meets c = -[x] res at x = 2"))
            kinds.append(Commit([None if i == 1 else a for i, a in enumerate(r)], "one off-curve coefficient", off_curve()))
        self.kinds = kinds
        self.jobs = [kinds[0]] if form == 0 else [kinds[j % len(kinds)] for j in range(B)]
        count = B * n if form == 2 else B
        self.xs = [XS[(t + t // len(XS)) % len(XS)] for t in range(count)]
        if form != 0:  # every kind of commitment meets the abscissa 2 (the Horner events) and 0
            for j in range(min(B, 2 * len(kinds))):
                self.xs[j * n if form == 2 else j] = 2 if j < len(kinds) else 0
        self.lanes = count if form == 2 else B * per
        self.tag = tag or "rows form %d degree %d B %d n %d%s" % (form, degree, B, n, " directed" if directed else "")
        self._ref = None

    def lane(self, t):
        """(coefficients low degree first, abscissa) of lane t."""
        per = self.degree + 1
        if self.form == 2:
            return self.jobs[t // self.n].m, self.xs[t]
        c = self.jobs[0 if self.form == 0 else t // per]
        return row_coeffs(c, self.degree, t % per), self.xs[t // per]

    def ref(self):
        if self._ref is None:
            out, st, events = [], [], []
            for t in range(self.lanes):
                coeffs, x = self.lane(t)
                res, ev = horner(coeffs, x)
                out.append(IDENT if res is None else enc(1, gmul(1, res)))
                st.append(INVALID if res is None else OK)
                events.append(ev)
            self._ref = (out, st, events)
        return self._ref

    def commits_bytes(self):
        if self.form == 0:
            return self.jobs[0].bytes()
        pad = bytes([0xEE]) * (self.stride - self.commit_size)  # bytes between two commitments: never a point
        return b"".join(c.bytes() + pad for c in self.jobs)


ROWS_SHAPES = [(0, 0, 1), (0, 1, 32), (0, 0, 65), (0, 0, 257), (0, 2, 22), (0, 7, 8), (0, 7, 33)]  # (form, degree, M): 1, 64, 65, 257, 66, 64, 264 lanes
_ROWS = {}


def rows_case(*key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _ROWS:
        _ROWS[k] = RowsCase(*key, **kw)
    return _ROWS[k]


def rows_directed_cases():
    """Every directed commitment of degree 2 and 7 in the three forms (form 0: one launch per commitment)."""
    out = []
    for degree in (2, 7):
        jobs = rows_case(1, degree, 23 if degree == 2 else 9, directed=True, slack=2)
        out.append(jobs)
        for ki in range(2, len(jobs.kinds)):
            c = RowsCase(0, degree, 5, tag="rows form 0 degree %d: %s" % (degree, jobs.kinds[ki].tag))
            c.jobs = [jobs.kinds[ki]]
            out.append(c)
        out.append(rows_case(2, degree, 14, n=5, directed=True))
    out.append(rows_case(1, 0, 65, slack=1))
    out.append(rows_case(1, 1, 32, slack=3))
    out.append(rows_case(2, 0, 1, n=1))
    out.append(rows_case(2, 1, 13, n=5))
    return out


def run_rows(lib, case, with_status=1):
    cb = u8(case.commits_bytes())
    xs = np.array(case.xs, dtype=np.uint64)
    out, status = fresh((case.lanes + 1) * 96), fresh(case.lanes + 1)
    call(lib, "commitment_rows", case.form, cb, len(cb), case.stride, case.degree, xs, case.B, case.n, with_status, out, status)
    return out, status


def check_rows(case, with_status, res):
    out, status = res
    want, st, _ = case.ref()
    bad = []
    if not is_poison(out[case.lanes * 96:]) or status[case.lanes] != POISON:
        bad.append("%s: the guard row or byte was written" % case.tag)
    if not with_status and not is_poison(status):
        bad.append("%s: status written though null was passed" % case.tag)
    for t in range(case.lanes):
        if bytes(out[t * 96:(t + 1) * 96]) != want[t] or (with_status and status[t] != st[t]):
            bad.append("%s lane %d (x = %d): wrong point or status %d, expected %d" % (case.tag, t, case.lane(t)[1], status[t], st[t]))
    return bad[:12]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Fr kernels
# ---------------------------------------------------------------------------------------------------------------------
class InterpCase:
    """B jobs of n samples (u64 abscissae, so that both interpolation kernels read the same samples).  Directed jobs: the abscissa 0;
    a repeated abscissa in the first, a middle and the last job at the sample positions (0, 1) and (n - 2, n - 1); a value >= r."""

    def __init__(self, n, B=70):
        rnd = random.Random("dkg-kernels-interp-%d" % n)
        self.n, self.B, self.tag = n, B, "interpolate n = %d" % n
        self.xs, self.ys, self.note = [], [], []
        for j in range(B):
            xs = rnd.sample(range(1, 200), n) if j % 3 else [rnd.randrange(1, 1 << 64) for _ in range(n)]
            if len(set(xs)) < n:
                xs = list(range(1, n + 1))
            ys = [rnd.randrange(R) for _ in range(n)]
            note = "random"
            if j % 7 == 1:
                xs[rnd.randrange(n)] = 0
                note = "abscissa 0"
            if j == 5:
                xs[0] = M64
                note = "abscissa 2^64 - 1"
            if n >= 2 and j in (0, B // 2, B - 1):
                a = 0 if j != B // 2 else n - 2
                xs[a + 1] = xs[a]
                note = "repeated abscissa at (%d, %d)" % (a, a + 1)
            if j == 3:
                ys[n - 1] = R
                note = "value r"
            if j == B - 2:
                ys[0] = RF - 1
                note = "value 2^256 - 1"
            if n >= 2 and j == 9:
                xs[1] = xs[0]
                ys[1] = R + 5
                note = "repeated abscissa and a value >= r"
            self.xs.append(xs)
            self.ys.append(ys)
            self.note.append(note)
        self.accept = [0 if j % 5 == 2 else 1 for j in range(B)]
        self._ref = None

    def ref(self):
        """[(status, coefficients)]"""
        if self._ref is None:
            out = []
            for xs, ys in zip(self.xs, self.ys):
                if any(y >= R for y in ys):
                    out.append((INVALID, [0] * self.n))
                elif len(set(xs)) < self.n:
                    out.append((DUPLICATE, [0] * self.n))
                else:
                    c = o.poly_interpolate(list(zip(xs, ys)))
                    out.append((OK, c + [0] * (self.n - len(c))))
            self._ref = out
        return self._ref


_INTERP = {}


def interp_case(n):
    if n not in _INTERP:
        _INTERP[n] = InterpCase(n)
    return _INTERP[n]


def _words(vals):
    return np.array([w for v in vals for w in words8(v)], dtype=np.uint32)


def run_interp(lib, case, with_status=1):
    n, B = case.n, case.B
    xs = _words([x for j in case.xs for x in j])
    ys = _words([y for j in case.ys for y in j])
    out, ws, status = fresh((B * n + 1) * 8, np.uint32), fresh((B + 1) * 2 * (n + 1) * 8, np.uint32), fresh(B + 1)
    call(lib, "fr_interpolate", n, xs, ys, B, with_status, out, ws, status)
    return out, ws, status


def check_interp(case, with_status, res):
    out, ws, status = res
    n, B = case.n, case.B
    blk = 2 * (n + 1) * 8
    bad = []
    if not is_poison(out[B * n * 8:]) or status[B] != POISON or not is_poison(ws[B * blk:]):
        bad.append("%s: a guard (out row, status byte or workspace block) was written" % case.tag)
    if not with_status and not is_poison(status):
        bad.append("%s: status written though null was passed" % case.tag)
    for j, (st, coeffs) in enumerate(case.ref()):
        what = "%s job %d (%s)" % (case.tag, j, case.note[j])
        if with_status and status[j] != st:
            bad.append("%s: status %d, expected %d" % (what, status[j], st))
        if [int(v) for v in out[j * n * 8:(j + 1) * n * 8]] != [w for c in coeffs for w in words8(c)]:
            bad.append("%s: wrong coefficients" % what)
        block = ws[j * blk:(j + 1) * blk]
        if st == INVALID and not is_poison(block):
            bad.append("%s: the workspace of a job that fails before it starts was written" % what)
        if st == OK:  # `poly` is the first half of the block, in Montgomery form
            if [int(v) for v in block[:n * 8]] != [w for c in coeffs for w in words8(c * RF % R)]:
                bad.append("%s: the workspace does not hold the polynomial in Montgomery form" % what)
            if not is_poison(block[n * 8:(n + 1) * 8]):
                bad.append("%s: word row n of `poly` was written (its length is n)" % what)
    return bad[:12]


def run_interp0(lib, case, with_accept):
    n, B = case.n, case.B
    xs = np.array([x for j in case.xs for x in j], dtype=np.uint64)
    vals = bytearray(b"".join(fr32(y) for j in case.ys for y in j))
    accept = None
    if with_accept:
        accept = np.array(case.accept, dtype=np.uint8)
        for j in range(B):
            if not case.accept[j]:
                vals[j * n * 32:(j + 1) * n * 32] = b"\xff" * (n * 32)  # a rejected part holds garbage: not read
    out, status = fresh((B + 1) * 32), fresh(B + 1)
    call(lib, "fr_interpolate_at_zero", n, xs, u8(vals), accept, B, out, status)
    return out, status


def check_interp0(case, with_accept, res):
    out, status = res
    bad = []
    if not is_poison(out[case.B * 32:]) or status[case.B] != POISON:
        bad.append("%s at zero: the guard row or byte was written" % case.tag)
    for j, (st, coeffs) in enumerate(case.ref()):
        if with_accept and not case.accept[j]:
            st, coeffs = OK, [0]
        if status[j] != st or bytes(out[j * 32:(j + 1) * 32]) != fr32(coeffs[0]):
            bad.append("%s at zero, job %d (%s): status %d (expected %d) or wrong value" % (case.tag, j, case.note[j], status[j], st))
    return bad[:12]


MONT_VALUES = [0, 1, 2, R - 1, R, R + 1, RF - 1, 1 << 255, RF % R, (1 << 128) - 1]


def mont_values():
    rnd = random.Random("dkg-kernels-mont")
    return MONT_VALUES + [rnd.randrange(R) for _ in range(60)]  # 70 lanes


def run_to_mont(lib, vals, degree=-1):
    count = len(vals) if degree < 0 else (degree + 1) ** 2
    fr = u8(b"".join(fr32(v) for v in vals))
    mont, valid = fresh((count + 1) * 8, np.uint32), fresh(count + 1)
    call(lib, "to_mont", fr, len(fr), count, degree, mont, valid)
    return mont, valid


def check_to_mont(vals, degree, res):
    mont, valid = res
    if degree >= 0:
        n = degree + 1
        vals = [vals[o.coeff_pos(t // n, t % n)] for t in range(n * n)]  # the symmetric expansion
    count = len(vals)
    bad = []
    if not is_poison(mont[count * 8:]) or valid[count] != POISON:
        bad.append("to_mont degree %d: the guard row or byte was written" % degree)
    for t, v in enumerate(vals):
        want = words8(v * RF % R) if v < R else [0] * 8
        if [int(x) for x in mont[t * 8:(t + 1) * 8]] != want or valid[t] != int(v < R):
            bad.append("to_mont degree %d entry %d (%x): wrong words or validity byte %d" % (degree, t, v, valid[t]))
    return bad[:12]


def bivar_coeffs(degree, variant=0):
    rnd = random.Random("dkg-kernels-bivar-%d" % degree)
    c = [rnd.randrange(R) for _ in range(tri(degree))]
    if variant:
        c[o.coeff_pos(1, degree)] = R + 3  # rows 1 and `degree` read it
    return c


def run_poly_evaluate(lib, polys, xs, with_status=1):
    B, n, M = len(polys), len(polys[0]), len(xs)
    coeff = u8(b"".join(fr32(c) for p in polys for c in p))
    out, status = fresh((B * M + 1) * 32), fresh(B * M + 1)
    call(lib, "fr_poly_evaluate", coeff, n, u8(b"".join(fr32(x) for x in xs)), M, B, with_status, out, status)
    return out, status


def check_fr_rows(what, want, res, with_status=1):
    """want: [(status, value)] per lane of an Fr kernel with 32-byte outputs."""
    out, status = res
    L = len(want)
    bad = []
    if not is_poison(out[L * 32:]) or status[L] != POISON:
        bad.append("%s: the guard row or byte was written" % what)
    if not with_status and not is_poison(status):
        bad.append("%s: status written though null was passed" % what)
    for t, (st, v) in enumerate(want):
        if bytes(out[t * 32:(t + 1) * 32]) != fr32(v) or (with_status and status[t] != st):
            bad.append("%s lane %d: status %d (expected %d) or wrong value" % (what, t, status[t], st))
    return bad[:12]


def poly_evaluate_case(n):
    rnd = random.Random("dkg-kernels-polyeval-%d" % n)
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
    if n:
        polys[3][n - 1] = R  # a non-canonical coefficient fails its whole row
    xs = [0, 1, R - 1, R, RF - 1] + [rnd.randrange(R) for _ in range(9)]  # 5 x 14 = 70 lanes
    want = [((INVALID, 0) if x >= R or any(c >= R for c in p) else (OK, o.poly_evaluate(p, x))) for p in polys for x in xs]
    return polys, xs, want


def run_bivar_row(lib, degree, coeffs, xs, with_status=1):
    L = len(xs) * (degree + 1)
    out, status = fresh((L + 1) * 32), fresh(L + 1)
    call(lib, "bivar_poly_row", u8(b"".join(fr32(c) for c in coeffs)), degree, np.array(xs, dtype=np.uint64), len(xs), with_status, out, status)
    return out, status


def bivar_row_want(degree, coeffs, xs):
    want = []
    for x in xs:
        for i in range(degree + 1):
            if any(coeffs[o.coeff_pos(i, j)] >= R for j in range(degree + 1)):
                want.append((INVALID, 0))
            else:
                want.append((OK, o.bivar_poly_row(degree, coeffs, x)[i]))
    return want


BIVAR_ROW_SHAPES = [(0, 65, 0), (2, 22, 0), (2, 22, 1), (7, 9, 0)]  # (degree, M, variant): 65, 66, 66, 72 lanes


class FrSumCase:
    """n terms x B outputs (B = 70).  mode 0: no mask; 1: the mask excludes every term that holds a non-canonical value or weight;
    2: the values are included, and so is the weight when n is even.  Non-canonical values sit in outputs 3 and 68 of term n // 2, the
    non-canonical weight at term n - 1."""

    def __init__(self, n, weighted, mode, B=70):
        rnd = random.Random("dkg-kernels-frsum-%d-%d-%d" % (n, weighted, mode))
        self.n, self.B, self.weighted, self.mode = n, B, weighted, mode
        self.stride = 32 * B if n % 2 else 32 * B + 64
        self.vals = [[rnd.randrange(R) for _ in range(B)] for _ in range(n)]
        self.w = [rnd.choice([0, 1, R - 1, rnd.randrange(R)]) for _ in range(n)] if weighted else None
        self.mask = None
        if mode and n:
            self.vals[n // 2][3] = R
            self.vals[n // 2][68] = RF - 1
            self.mask = [rnd.randrange(4) != 0 for _ in range(n)]
            self.mask[n // 2] = mode == 2
            if weighted and n >= 2:
                self.w[n - 1] = R + 1
                self.mask[n - 1] = mode == 2 and n % 2 == 0
        self.tag = "fr %ssum n = %d mode %d" % ("w" if weighted else "", n, mode)

    def want(self):
        out = []
        inc = [k for k in range(self.n) if self.mask is None or self.mask[k]]
        for j in range(self.B):
            ok = all(self.vals[k][j] < R and (not self.weighted or self.w[k] < R) for k in inc)
            v = sum(self.vals[k][j] * (self.w[k] if self.weighted else 1) for k in inc) % R
            out.append((OK, v) if ok else (INVALID, 0))
        return out


def run_fr_sum(lib, case, with_status=1):
    buf = bytearray([0xC3]) * (case.n * case.stride + 32)
    for k in range(case.n):
        for j in range(case.B):
            buf[k * case.stride + j * 32:k * case.stride + j * 32 + 32] = fr32(case.vals[k][j])
    vals = u8(buf)
    w = u8(b"".join(fr32(x) for x in case.w)) if case.weighted else None
    mask = np.array(case.mask, dtype=np.uint8) if case.mask is not None else None
    if mask is not None and not len(mask):
        mask = np.zeros(1, dtype=np.uint8)
    out, status = fresh((case.B + 1) * 32), fresh(case.B + 1)
    call(lib, "fr_sum", vals, len(vals), case.stride, case.n, w, mask, case.B, with_status, out, status)
    return out, status


# ---------------------------------------------------------------------------------------------------------------------
# 4. k_g1_sum
# ---------------------------------------------------------------------------------------------------------------------
def sum_part(n, g, parts):
    return g * n // parts, (g + 1) * n // parts


def slice_part(n, s, slices, g, parts):
    k0, k1 = sum_part(n, s, slices)
    a, b = sum_part(k1 - k0, g, parts)
    return k0 + a, k0 + b


def eff_parts(parts):
    return parts if 1 <= parts <= 64 and parts & (parts - 1) == 0 else 1


def g1_sum_parts_model(B, n, cus, forced):
    if forced:
        return forced
    want = (cus if cus > 0 else 256) * 4 * 64
    parts = 1
    while parts < 64 and B * parts < want and parts * 4 <= n:
        parts *= 2
    return parts


def g1_wsum_parts_model(B, n, cus, forced):
    if forced:
        return forced
    want = (cus if cus > 0 else 256) * 4 * 64
    parts = 1
    while parts < 64 and B * parts < want and parts * 2 <= n:
        parts *= 2
    return parts


def g1_wsum_slices_model(B, n, parts, cus, forced):
    slices = forced
    if not slices:
        if parts < 64 or n <= 64:
            return 1
        slices = min((n + 63) // 64, (cus if cus > 0 else 256) * 4 // max(B, 1))
    return max(1, min(slices, n))


def lane_of(n, k, parts):
    return next(g for g in range(parts) if sum_part(n, g, parts)[0] <= k < sum_part(n, g, parts)[1])


SUM_COLUMNS = ["random", "P, -P adjacent and mirrored across the split", "copies", "a term that does not decode", "member verdict 0",
               "identities", "random", "random", "random"]


class SumCase:
    """n terms x 9 columns of points as multiples of g1 (None: a term that does not decode), laid out term-major with
    term_stride = 9 x 96.  variant "masked": the mask excludes the term that does not decode (and a few more); "included": no mask,
    and a member array with one zero verdict in column 4."""

    def __init__(self, n, variant):
        rnd = random.Random("dkg-kernels-sum-%d" % n)
        pl = pool(1)
        self.n, self.variant, self.W = n, variant, 9
        self.tag = "g1 sum n = %d %s" % (n, variant)
        m = [[pl[rnd.randrange(len(pl))] for _ in range(9)] for _ in range(n)]
        p, q = pl[3], pl[4]
        self.pairs = []
        if n >= 2:
            m[0][1], m[1][1] = p, neg_mult(1, p)
            self.pairs.append((0, 1))
        if n >= 6:
            m[n // 2 - 1][1], m[n // 2][1] = q, neg_mult(1, q)
            self.pairs.append((n // 2 - 1, n // 2))
        for k in range(n):
            m[k][2] = pl[7]
            if k % 2 == 0 or k == n - 1:
                m[k][5] = 0
        self.k_bad, self.k_mem = n // 3, (2 * n) // 3
        m[self.k_bad][3] = None
        self.m = m
        self.mask = None
        if variant == "masked":
            self.mask = [rnd.randrange(5) != 0 for _ in range(n)]
            self.mask[self.k_bad] = False

    def B(self, parts):
        return 5 if parts == 64 else 9

    def member(self, B):
        if self.variant != "included":
            return None
        mem = np.ones(self.n * B, dtype=np.uint8)
        mem[self.k_mem * B + 4] = 0
        return mem

    def want(self, B):
        """(out rows, statuses, term_bad)"""
        inc = [k for k in range(self.n) if self.mask is None or self.mask[k]]
        out, st, tb = [], [], [0] * self.n
        for j in range(B):
            good = True
            for k in inc:
                if self.m[k][j] is None or (self.variant == "included" and j == 4 and k == self.k_mem):
                    good = False
                    tb[k] = 1
            out.append(enc(1, gmul(1, sum(self.m[k][j] for k in inc))) if good else IDENT)
            st.append(OK if good else INVALID)
        return out, st, tb

    def points(self):
        return b"".join(BAD if a is None else enc(1, gmul(1, a)) for row in self.m for a in row)


SUM_NS = [1, 2, 5, 67, 130]
_SUM = {}


def sum_case(n, variant):
    if (n, variant) not in _SUM:
        _SUM[(n, variant)] = SumCase(n, variant)
    return _SUM[(n, variant)]


def run_sum(lib, case, parts, cus=1, with_status=1, with_term_bad=1):
    """(out[:5 rows], status[:5], term_bad, rest of out, rest of status): the first three are the same for every parts (B = 5 at 64)."""
    B, n = case.B(parts), case.n
    pts = u8(case.points())
    mask = np.array(case.mask, dtype=np.uint8) if case.mask is not None else None
    out, status, term_bad = fresh((B + 1) * 96), fresh(B + 1), fresh(n + 1)
    used = np.zeros(2, dtype=np.uint64)
    call(lib, "g1_sum", 0, pts, len(pts), case.W * 96, n, mask, case.member(B), B, parts, cus, with_status, with_term_bad, out, status, term_bad, used)
    if used[0] != g1_sum_parts_model(B, n, cus, parts):
        raise AssertionError("%s: g1_sum_parts gave %d, the model %d" % (case.tag, used[0], g1_sum_parts_model(B, n, cus, parts)))
    return out[:5 * 96], status[:5], term_bad, out[5 * 96:], status[5:]


def check_sum(case, parts, res, with_status=1, with_term_bad=1):
    head, st_head, term_bad, tail, st_tail = res
    B = case.B(parts)
    want, st, tb = case.want(B)
    out = np.concatenate([head, tail])
    status = np.concatenate([st_head, st_tail])
    what = "%s parts = %d" % (case.tag, parts)
    bad = []
    if not is_poison(out[B * 96:]) or status[B] != POISON or term_bad[case.n] != POISON:
        bad.append("%s: a guard (out row, status byte, term_bad byte) was written" % what)
    if not with_status and not is_poison(status):
        bad.append("%s: status written though null was passed" % what)
    if with_term_bad and [int(x) for x in term_bad[:case.n]] != tb:
        bad.append("%s: term_bad %s, expected %s" % (what, [int(x) for x in term_bad[:case.n]], tb))
    if not with_term_bad and not is_poison(term_bad):
        bad.append("%s: term_bad written though null was passed" % what)
    for j in range(B):
        if bytes(out[j * 96:(j + 1) * 96]) != want[j] or (with_status and status[j] != st[j]):
            bad.append("%s output %d (%s): wrong sum or status %d, expected %d" % (what, j, SUM_COLUMNS[j], status[j], st[j]))
    return bad[:12]


def sum_head(res):
    return res[:3]


class Column0Case:
    """P = 3 bivariate commitments of one degree, `stride` bytes apart: out[j] = sum_p commits[p][pos(j, 0)] (SumOffColumn0 with
    term_stride = the commitment size)."""

    def __init__(self, degree, P=3):
        rnd = random.Random("dkg-kernels-column0-%d" % degree)
        pl = pool(1)
        self.degree, self.P, self.B = degree, P, degree + 1
        self.size = tri(degree) * 96
        self.m = [[pl[rnd.randrange(len(pl))] for _ in range(tri(degree))] for _ in range(P)]
        self.tag = "column 0 of %d commitments of degree %d" % (P, degree)

    def points(self):
        return b"".join(enc(1, gmul(1, a)) for c in self.m for a in c)

    def want(self):
        return [enc(1, gmul(1, sum(c[o.coeff_pos(j, 0)] for c in self.m))) for j in range(self.B)]


def run_column0_sum(lib, case, parts):
    pts = u8(case.points())
    B = case.B
    out, status, term_bad = fresh((B + 1) * 96), fresh(B + 1), fresh(case.P + 1)
    used = np.zeros(2, dtype=np.uint64)
    call(lib, "g1_sum", 1, pts, len(pts), case.size, case.P, None, None, B, parts, 1, 1, 1, out, status, term_bad, used)
    return out, status, term_bad


def check_column0_sum(case, parts, res):
    out, status, term_bad = res
    B = case.B
    bad = []
    if not is_poison(out[B * 96:]) or status[B] != POISON or term_bad[case.P] != POISON or term_bad[:case.P].any():
        bad.append("%s parts = %d: a guard was written or term_bad set" % (case.tag, parts))
    if rows(out[:B * 96], 96) != case.want() or status[:B].any():
        bad.append("%s parts = %d: wrong sums or statuses" % (case.tag, parts))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# 5. k_wsum_recode and k_g1_wsum
# ---------------------------------------------------------------------------------------------------------------------
REC_TOP, REC_FLIP, REC_ZERO, REC_VALID = 1, 2, 4, 8  # tc_dkg.h kWsum*


def rec_weights():
    rnd = random.Random("dkg-kernels-rec")
    edge = [0, 1, 2, R - 1, R - 2, R, R + 1, RF - 1, X2, X2 - 1, X2 + 1, 2 * X2, R - X2, (R // X2) * X2, 1 << 128, (1 << 128) - 1, 1 << 254]
    return edge + [rnd.randrange(R) for _ in range(70 - len(edge))]


def rec_value(rec):
    """The scalar nine recoded words stand for: (value mod r or None when invalid, flags).  k' = k1 + k2 x^2 with the 129 sign-aligned
    columns of glv_recode_sign_aligned; the ladder negates the base point when `flip` is set."""
    neg = sum(int(rec[i]) << (32 * i) for i in range(4))
    u = sum(int(rec[4 + i]) << (32 * i) for i in range(4))
    flags = int(rec[8])
    if not flags & REC_VALID:
        return None, flags
    if flags & REC_ZERO:
        return 0, flags
    k1 = sum((-1 if (neg >> i) & 1 else 1) << i for i in range(128)) + (1 << 128)
    k2 = sum((-1 if (neg >> i) & 1 else 1) * ((u >> i) & 1) << i for i in range(128)) + ((flags & REC_TOP) << 128)
    k = (k1 + k2 * X2) % R
    return ((R - k) % R if flags & REC_FLIP else k), flags


def check_rec(weights, rec):
    bad = []
    if not is_poison(rec[len(weights) * 9:]):
        bad.append("recode: the guard entry was written")
    for k, w in enumerate(weights):
        v, flags = rec_value(rec[k * 9:k * 9 + 9])
        if flags & ~15 or bool(flags & REC_VALID) != (w < R) or bool(flags & REC_ZERO) != (w % RF == 0):
            bad.append("recode weight %d (%x): flags %x" % (k, w, flags))
        elif (w >= R or w == 0) and any(int(x) for x in rec[k * 9:k * 9 + 8]):
            bad.append("recode weight %d (%x): digits stored for a weight that has none" % (k, w))
        elif w < R and v != w:
            bad.append("recode weight %d (%x): the words stand for %x" % (k, w, v))
        elif w < R and w and gmul(1, v) != gmul(1, w):
            bad.append("recode weight %d: [rec] g1 != [w] g1" % k)
    return bad[:12]


class WsumCase:
    """n_terms terms x B = 5 columns and one weight per term; the sum visits all terms, or the positions of `sel` (a permuted subset:
    the other terms then hold bytes that do not decode and non-canonical weights, to show that they are not read).
    Columns: 0 random; 1 two terms with w_a P_a = w_b P_b; 2 with w_a P_a = -w_b P_b; 3 a zero weight on a term that does not
    decode (variant "failing"); 4 random.  variant "masked": a non-canonical weight on a masked term; "failing": on an included one."""

    def __init__(self, n, variant, with_sel=False):
        rnd = random.Random("dkg-kernels-wsum-%d-%s-%d" % (n, variant, with_sel))
        pl = pool(1)
        self.B, self.variant = 5, variant
        self.tag = "g1 wsum n = %d %s%s" % (n, variant, " sel" if with_sel else "")
        if with_sel:
            self.n_terms = 12
            self.sel = rnd.sample(range(12), n)
        else:
            self.n_terms, self.sel = n, None
        self.n = n
        visited = self.sel if with_sel else list(range(n))
        nt = self.n_terms
        self.m = [[pl[rnd.randrange(len(pl))] for _ in range(5)] for _ in range(nt)]
        self.w = [rnd.choice([1, 2, R - 1, rnd.randrange(1, R), rnd.randrange(1, R)]) for _ in range(nt)]
        self.mask = [True] * nt
        if n >= 3:
            a, b, c = visited[0], visited[n // 2], visited[n - 1]
            self.w[c] = 0  # a zero weight: the term contributes nothing
            inv_b = pow(self.w[b], R - 2, R)
            self.m[b][1] = self.w[a] * self.m[a][1] * inv_b % R
            self.m[b][2] = (R - self.w[a] * self.m[a][2] % R) * inv_b % R
            if variant == "failing":
                self.m[c][3] = None  # the decode comes before the weight
            if n >= 5:
                d = visited[1]
                self.w[d] = R + 2
                self.mask[d] = variant == "failing"
                e = visited[3]
                self.m[e][0] = None  # masked out in both variants
                self.mask[e] = False
        elif variant == "failing":
            self.m[visited[0]][3] = None
        if with_sel:
            for k in range(nt):
                if k not in visited:
                    self.m[k] = [None] * 5
                    self.w[k] = RF - 1
        self.mask_arr = None if all(self.mask) else np.array(self.mask, dtype=np.uint8)

    def visited(self):
        return self.sel if self.sel is not None else list(range(self.n))

    def term_ok(self, k, j):
        return self.m[k][j] is not None and self.w[k] < R

    def want_range(self, j, k0, k1):
        """(bytes, good) of the positions k0 .. k1 of output j."""
        inc = [k for k in self.visited()[k0:k1] if self.mask[k]]
        if not all(self.term_ok(k, j) for k in inc):
            return IDENT, 0
        return enc(1, gmul(1, sum(self.m[k][j] * self.w[k] for k in inc))), 1

    def points(self):
        return b"".join(BAD if a is None else enc(1, gmul(1, a)) for row in self.m for a in row)


def recode_only(lib, weights):
    """k_wsum_recode over `weights` (the sum behind it runs over masked identities): the (n + 1) x 9 words."""
    nt = len(weights)
    rec = fresh((nt + 1) * 9, np.uint32)
    used = np.zeros(2, dtype=np.uint64)
    call(lib, "g1_wsum", 0, u8(IDENT * nt), nt * 96, 96, nt, u8(b"".join(fr32(w) for w in weights)), nt, np.zeros(nt, dtype=np.uint8), None, 1, 1, 1, 1,
         None, 0, 1, rec, fresh(2 * 96), fresh(2), fresh(2), fresh(2 * 96), fresh(2), used)
    return rec


_WSUM = {}


def wsum_case(n, variant, with_sel=False):
    key = (n, variant, with_sel)
    if key not in _WSUM:
        _WSUM[key] = WsumCase(*key)
    return _WSUM[key]


WSUM_NS = [1, 3, 67, 130]


def wsum_slices(n):
    return [0, 1, 2, 3, 5, 64, n + 3]


def run_wsum(lib, case, parts, slices, cus=1, chain=1):
    """(final out, final status, rec, partial out, status, part_ok, slices used): the first two are the same for every (parts, slices)."""
    B, n, nt = case.B, case.n, case.n_terms
    rows_cap = B * max(1, min(n, max(slices, (n + 63) // 64)))
    pts = u8(case.points())
    w = u8(b"".join(fr32(x) for x in case.w))
    sel = np.array(case.sel, dtype=np.uint32) if case.sel is not None else None
    rec = fresh((nt + 1) * 9, np.uint32)
    out, status, part_ok = fresh((rows_cap + 1) * 96), fresh(rows_cap + 1), fresh(rows_cap + 1)
    fout, fstatus = fresh((B + 1) * 96), fresh(B + 1)
    used = np.zeros(2, dtype=np.uint64)
    call(lib, "g1_wsum", 0, pts, len(pts), B * 96, nt, w, n, case.mask_arr, None, B, parts, slices, cus, sel, chain, rows_cap, rec, out, status, part_ok,
         fout, fstatus, used)
    p_model = g1_wsum_parts_model(B, n, cus, parts)
    s_model = g1_wsum_slices_model(B, n, p_model, cus, slices)
    if (int(used[0]), int(used[1])) != (p_model, s_model):
        raise AssertionError("%s: parts, slices = %s, the model %s" % (case.tag, used, (p_model, s_model)))
    S = s_model
    if S == 1:
        return out[:(B + 1) * 96], status[:B + 1], rec, out, status, part_ok, S
    return fout, fstatus, rec, out, status, part_ok, S


def check_wsum(case, parts, slices, res, chain=1):
    fout, fstatus, rec, out, status, part_ok, S = res
    B, n = case.B, case.n
    what = "%s parts = %d slices = %d (%d used)" % (case.tag, parts, slices, S)
    bad = []
    if not is_poison(out[B * S * 96:]) or not is_poison(status[B * S:]) or not is_poison(part_ok[B * S:]):
        bad.append("%s: rows or bytes behind the %d groups were written" % (what, B * S))
    if S > 1:
        if not is_poison(status):
            bad.append("%s: status written though part_ok is in use" % what)
        for s in range(S):
            k0, k1 = sum_part(n, s, S)
            for j in range(B):
                q = s * B + j
                pt, good = case.want_range(j, k0, k1)
                if bytes(out[q * 96:(q + 1) * 96]) != pt or part_ok[q] != good:
                    bad.append("%s: slice %d of output %d: wrong partial sum or part_ok %d" % (what, s, j, part_ok[q]))
    else:
        if not is_poison(part_ok):
            bad.append("%s: part_ok written though there is one slice" % what)
    if S == 1 or chain:
        if not is_poison(fout[B * 96:]) or fstatus[B] != POISON:
            bad.append("%s: the guard behind the final sums was written" % what)
        for j in range(B):
            pt, good = case.want_range(j, 0, n)
            if bytes(fout[j * 96:(j + 1) * 96]) != pt or fstatus[j] != (OK if good else INVALID):
                bad.append("%s: output %d: wrong sum or status %d" % (what, j, fstatus[j]))
    return bad[:12]


# ---------------------------------------------------------------------------------------------------------------------
# 6. the pieces of the combined values check
# ---------------------------------------------------------------------------------------------------------------------
RLC_SEED = bytes((7 * i + 3) & 0xff for i in range(32))


class RlcCase:
    def __init__(self, degree, n, B=70):
        rnd = random.Random("dkg-kernels-rlc-%d-%d" % (degree, n))
        self.degree, self.n, self.B = degree, n, B
        self.tag = "rlc scalars degree %d n %d" % (degree, n)
        self.xs = [[rnd.choice([0, 1, M64, rnd.randrange(1 << 64)]) for _ in range(n)] for _ in range(B)]
        self.vals = [[rnd.randrange(R) for _ in range(n)] for _ in range(B)]
        self.vals[2][n - 1] = R
        self.vals[B - 1][0] = RF - 1

    def want(self):
        """(scalars per job, valid): c_i = sum_k rho_k x_k^i, c_g = -sum_k rho_k v_k; rho: the first two words of ChaCha20 block
        j n + k, the low bit set."""
        key = [int.from_bytes(RLC_SEED[4 * i:4 * i + 4], "little") for i in range(8)]
        sc, valid = [], []
        for j in range(self.B):
            rho = []
            for k in range(self.n):
                blk = o.chacha20_block(key, j * self.n + k)
                rho.append((blk[1] << 32) | blk[0] | 1)
            ok = all(v < R for v in self.vals[j])
            row = [sum(r * pow(x, i, R) for r, x in zip(rho, self.xs[j])) % R for i in range(self.degree + 1)]
            row.append((-sum(r * v for r, v in zip(rho, self.vals[j]))) % R)
            sc.append(row if ok else [0] * (self.degree + 2))
            valid.append(int(ok))
        return sc, valid


RLC_SHAPES = [(0, 1), (2, 5), (7, 5), (7, 1)]


def run_rlc(lib, case):
    per = case.degree + 2
    xs = np.array([x for j in case.xs for x in j], dtype=np.uint64)
    vals = u8(b"".join(fr32(v) for j in case.vals for v in j))
    scalars, valid = fresh((case.B * per + 1) * 8, np.uint32), fresh(case.B + 1)
    call(lib, "rlc_scalars", u8(RLC_SEED), xs, vals, case.n, case.degree, case.B, scalars, valid)
    return scalars, valid


def check_rlc(case, res):
    scalars, valid = res
    per = case.degree + 2
    sc, va = case.want()
    bad = []
    if not is_poison(scalars[case.B * per * 8:]) or valid[case.B] != POISON:
        bad.append("%s: the guard row or byte was written" % case.tag)
    for j in range(case.B):
        got = [int(x) for x in scalars[j * per * 8:(j + 1) * per * 8]]
        if got != [w for v in sc[j] for w in words8(v)] or valid[j] != va[j]:
            bad.append("%s job %d: wrong scalars or valid %d" % (case.tag, j, valid[j]))
    return bad[:12]


def copy_points_case(column0, degree, B):
    """(src bytes, stride, extra, expected out): every 8-byte word of the source is distinct, so a wrong word shows."""
    rnd = random.Random("dkg-kernels-copy-%d-%d-%d" % (column0, degree, B))
    if column0:
        stride = tri(degree) * 96 + 96
        src = rnd.randbytes(B * stride)
        want = b"".join(src[p * stride + o.coeff_pos(i, 0) * 96:p * stride + o.coeff_pos(i, 0) * 96 + 96] for p in range(B) for i in range(degree + 1))
        return src, stride, None, want
    src = rnd.randbytes(B * (degree + 1) * 96)
    extra = rnd.randbytes(96)
    row = (degree + 1) * 96
    return src, 0, extra, b"".join(src[j * row:(j + 1) * row] + extra for j in range(B))


COPY_SHAPES = [(0, 0, 1), (0, 2, 3), (0, 7, 9), (1, 0, 1), (1, 2, 3), (1, 7, 9)]  # 24 .. 972 words: a ragged last wave in each


def run_copy_points(lib, column0, degree, B):
    src, stride, extra, want = copy_points_case(column0, degree, B)
    out = fresh(len(want) + 96)
    call(lib, "copy_points", column0, u8(src), len(src), stride, degree, u8(extra) if extra else None, B, out)
    return out, want


def compare_case(per_job, B=70):
    """k_g1_equal: (a, st_a, b, st_b, expected ok)."""
    rnd = random.Random("dkg-kernels-equal-%d" % per_job)
    a = bytearray(rnd.randbytes(B * per_job * 96))
    b = bytearray(a)
    sa, sb = bytearray(B * per_job), bytearray(B * per_job)
    want = [1] * B
    b[(1 * per_job) * 96] ^= 1                               # the first byte of job 1
    b[(3 * per_job + per_job - 1) * 96 + 95] ^= 0x80         # the last byte of the last word of job 3
    sa[5 * per_job + per_job - 1] = INVALID
    sb[6 * per_job] = DUPLICATE
    b[(B - 1) * per_job * 96 + 50] ^= 4
    for j in (1, 3, 5, 6, B - 1):
        want[j] = 0
    return bytes(a), bytes(sa), bytes(b), bytes(sb), want


def identity_case(B=70):
    """k_g1_is_identity: (pts, status, valid, expected ok)."""
    rnd = random.Random("dkg-kernels-identity")
    pts = bytearray(rnd.randbytes(B * 96))
    st, valid, want = bytearray(B), bytearray([1]) * B, []
    for j in range(B):
        pts[j * 96] = (pts[j * 96] & ~0x40) | (0x40 if j % 2 == 0 else 0)
        st[j] = INVALID if j % 5 == 4 else OK
        valid[j] = 0 if j % 7 == 6 else (1 if j % 3 else 0xff)
        want.append(int(j % 2 == 0 and st[j] == OK and valid[j] != 0))
    return bytes(pts), bytes(st), bytes(valid), want


def run_compare(lib, a, sa, b, sb, per_job, B):
    ok = fresh(B + 1)
    call(lib, "g1_compare", u8(a), u8(sa), u8(b) if b is not None else None, u8(sb), per_job, B, ok)
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# 7. the resharing verdict chain and the generate verdict
# ---------------------------------------------------------------------------------------------------------------------
class ReshareCase:
    """P parts dealing into a resharing of a polynomial of degree t_old (old_commit: its commitment, as multiples of g1).  Part p is a
    bivariate commitment of degree 1 whose constant is, for a right dealer, old_commit.evaluate(dealer_idx[p] + 1)."""

    def __init__(self, P, t_old, kind):
        rnd = random.Random("dkg-kernels-reshare-%d-%d-%s" % (P, t_old, kind))
        self.P, self.t_old, self.kind, self.degree = P, t_old, kind, 1
        self.tag = "reshare P = %d t_old = %d %s" % (P, t_old, kind)
        self.old = [rnd.randrange(1, R) for _ in range(t_old + 1)]
        base = [0, M64, 5, 9, 1 << 40, 7, 3]
        self.idx = [base[p] if p < len(base) else 100 + p for p in range(P)]
        self.accept = [1] * P
        self.wrong, self.undecodable, self.col_bad, self.member0 = set(), set(), set(), set()
        self.share_st = None
        self.old_bad = kind == "bad old_commit"
        self.old_member = None
        if kind == "mixed" and P >= 7:
            self.accept[1] = 0           # rejected: holds garbage, not read
            self.idx[4] = self.idx[0]    # a repeated index: the first claim is not marked
            self.idx[6] = self.idx[1]    # repeats a REJECTED part's index: no duplicate
            self.wrong.add(3)            # a mismatching constant
            self.undecodable.add(5)      # a constant that does not decode
            if P > 200:
                self.accept[P - 2] = 0
                self.wrong.add(P - 1)
                self.col_bad.add(P - 3)  # its second first-column point does not decode
                self.member0.add(P - 4)
                self.share_st = [OK] * P
                self.share_st[P - 5] = DUPLICATE
                self.share_st[P - 6] = INVALID
                self.share_st[1] = INVALID  # of a rejected part: ignored
        if kind == "mixed" and P == 1:
            self.wrong.add(0)
        if kind == "too few":
            for p in range(P):
                self.accept[p] = 1 if p < t_old else 0
        if kind == "rejected only bad":  # every failing part is rejected: the verdict is OK
            self.accept = [1] * P
            for p in range(min(P - t_old - 1, 3)):
                self.accept[2 * p + 1 if 2 * p + 1 < P else p] = 0
        if kind == "old member":
            self.old_member = [1] * (t_old + 1)
            self.old_member[t_old] = 0
            self.old_bad = True
        self.with_accept = kind != "all accepted"

    def accepted(self, p):
        return not self.with_accept or self.accept[p] != 0

    def const_mult(self, p):
        return o.poly_evaluate(self.old, (self.idx[p] + 1) % R)

    def commits(self):
        rnd = random.Random("dkg-kernels-reshare-commits")
        pl = pool(1)
        out = []
        for p in range(self.P):
            if not self.accepted(p):
                out.append(bytes([0xEE]) * (3 * 96))
                continue
            c0 = enc(1, gmul(1, (self.const_mult(p) + (1 if p in self.wrong else 0)) % R))
            if p in self.undecodable:
                c0 = BAD
            c1 = BAD if p in self.col_bad else enc(1, gmul(1, pl[p % len(pl)]))
            out.append(c0 + c1 + bytes(rnd.randrange(256) for _ in range(96)))  # coefficient (1, 1) is not read: garbage
        return b"".join(out)

    def old_commit(self):
        b = b"".join(enc(1, gmul(1, a)) for a in self.old)
        return (b[:-96] + off_curve()) if self.kind == "bad old_commit" else b

    def member(self):
        if not self.member0:
            return None
        m = np.ones(self.P * 2, dtype=np.uint8)
        for p in self.member0:
            m[p * 2 + 1] = 0
        return m

    def want(self):
        """The rules of the header comments restated: dicts of every array the chain leaves."""
        P, t = self.P, self.t_old
        const_st, point_bad, dup = [OK] * P, [0] * P, [0] * P
        for p in range(P):
            if not self.accepted(p):
                continue
            dup[p] = int(any(self.accepted(q) and self.idx[q] == self.idx[p] for q in range(p)))
            point_bad[p] = int(p in self.undecodable or p in self.col_bad or p in self.member0)
            const_st[p] = INVALID if p in self.undecodable else MISMATCH if p in self.wrong else OK
        part = [OK] * P
        for p in range(P):
            if self.old_bad or not self.accepted(p):
                continue
            ss = self.share_st[p] if self.share_st else OK
            if point_bad[p] or const_st[p] == INVALID or ss == INVALID:
                part[p] = INVALID
            elif dup[p] or ss == DUPLICATE:
                part[p] = DUPLICATE
            elif const_st[p] == MISMATCH:
                part[p] = MISMATCH
        status = INVALID if self.old_bad else next((s for s in part if s != OK), OK)
        used, sel_part, weights = [0] * P, [], [0] * P
        if status == OK:
            acc = [p for p in range(P) if self.accepted(p)]
            if len(acc) <= t:
                status = NOT_ENOUGH
            else:
                sel_part = acc[:t + 1]
                for p in sel_part:
                    used[p] = 1
                lam = o.lagrange_coeffs(t, [(self.idx[p] + 1) % R for p in sel_part])
                for p, l in zip(sel_part, lam):
                    weights[p] = l
        return dict(const_st=const_st, point_bad=point_bad, dup=dup, old_bad=int(self.old_bad), part_status=part, used=used, sel_part=sel_part,
                    sel_idx=[self.idx[p] for p in sel_part], weights=weights, status=status)


RESHARE_SHAPES = [(1, 0, "mixed"), (1, 0, "all accepted"), (7, 2, "mixed"), (7, 2, "all accepted"), (7, 6, "all accepted"), (7, 2, "too few"),
                  (7, 6, "too few"), (7, 2, "bad old_commit"), (7, 2, "old member"), (7, 2, "rejected only bad"), (257, 6, "mixed"),
                  (257, 6, "all accepted"), (257, 0, "all accepted")]
_RESHARE = {}


def reshare_case(P, t_old, kind):
    if (P, t_old, kind) not in _RESHARE:
        _RESHARE[(P, t_old, kind)] = ReshareCase(P, t_old, kind)
    return _RESHARE[(P, t_old, kind)]


def run_reshare(lib, case, with_outputs=(True, True)):
    P, t = case.P, case.t_old
    commits = u8(case.commits())
    a = dict(const_st=fresh(P + 1), point_bad=fresh(P + 1), dup=fresh(P + 1), old_bad=fresh(2), part_status=fresh(P + 1), used=fresh(P + 1),
             sel_part=fresh(t + 2, np.uint32), sel_idx=fresh(t + 2, np.uint64), ws=fresh(5 * (t + 1) * 8 + 8, np.uint32), weights=fresh((P + 1) * 32),
             status=fresh(2))
    a["out_commit"] = np.full((case.degree + 2) * 96, KEEP, dtype=np.uint8) if with_outputs[0] else None
    a["out_share"] = np.full(64, KEEP, dtype=np.uint8) if with_outputs[1] else None
    call(lib, "reshare_chain", u8(case.old_commit()), np.array(case.old_member, dtype=np.uint8) if case.old_member else None, t,
         np.array(case.idx, dtype=np.uint64), commits, len(commits), 3 * 96, case.degree, np.array(case.accept, dtype=np.uint8) if case.with_accept else None,
         case.member(), np.array(case.share_st, dtype=np.uint8) if case.share_st else None, P, a["const_st"], a["point_bad"], a["dup"], a["old_bad"],
         a["part_status"], a["used"], a["sel_part"], a["sel_idx"], a["ws"], a["weights"], a["status"], a["out_commit"], a["out_share"])
    return a


def check_guarded_outputs(what, failed, degree, out_commit, out_share, bad):
    """k_reshare_guard / k_dkg_generate_guard: the identity over out_commit[0 .. degree] and zero over the share on failure only."""
    if out_commit is not None:
        want = (IDENT * (degree + 1) if failed else bytes([KEEP]) * (96 * (degree + 1))) + bytes([KEEP]) * 96
        if bytes(out_commit) != want:
            bad.append("%s: out_commit is not %s with the row behind it untouched" % (what, "all identities" if failed else "as it was"))
    if out_share is not None:
        want = (bytes(32) if failed else bytes([KEEP]) * 32) + bytes([KEEP]) * 32
        if bytes(out_share) != want:
            bad.append("%s: out_share is not %s with the bytes behind it untouched" % (what, "zero" if failed else "as it was"))


def check_reshare(case, a):
    P, t = case.P, case.t_old
    w = case.want()
    bad = []
    for name in ("const_st", "point_bad", "dup", "part_status", "used"):
        if name == "const_st" and case.kind == "bad old_commit":
            pass  # (tc_dkg.h: against an old_commit that does not decode the answer is meaningless, and nobody reads it)
        elif [int(x) for x in a[name][:P]] != w[name]:
            diff = [p for p in range(P) if int(a[name][p]) != w[name][p]]
            bad.append("%s: %s differs at parts %s" % (case.tag, name, diff[:8]))
        if a[name][P] != POISON:
            bad.append("%s: the byte behind %s was written" % (case.tag, name))
    if (int(a["old_bad"][0]), int(a["old_bad"][1])) != (w["old_bad"], POISON):
        bad.append("%s: old_bad %s" % (case.tag, a["old_bad"]))
    if (int(a["status"][0]), int(a["status"][1])) != (w["status"], POISON):
        bad.append("%s: status %s, expected %d" % (case.tag, a["status"], w["status"]))
    n_sel = len(w["sel_part"])
    if [int(x) for x in a["sel_part"][:n_sel]] != w["sel_part"] or [int(x) for x in a["sel_idx"][:n_sel]] != w["sel_idx"]:
        bad.append("%s: sel_part / sel_idx %s / %s" % (case.tag, a["sel_part"], a["sel_idx"]))
    if not is_poison(a["sel_part"][n_sel:]) or not is_poison(a["sel_idx"][n_sel:]):
        bad.append("%s: sel_part / sel_idx written behind the %d selected parts" % (case.tag, n_sel))
    if not n_sel and not is_poison(a["ws"]):
        bad.append("%s: the plan's workspace written though nothing was selected" % case.tag)
    if not is_poison(a["ws"][5 * (t + 1) * 8:]):
        bad.append("%s: the words behind the plan's workspace were written" % case.tag)
    if n_sel and [int(x) for x in a["ws"][:(t + 1) * 8]] != [x for p in w["sel_part"] for x in words8(w["weights"][p])]:
        bad.append("%s: lam is not the Lagrange coefficients of the selected dealers" % case.tag)
    if rows(a["weights"][:P * 32], 32) != [fr32(x) for x in w["weights"]] or not is_poison(a["weights"][P * 32:]):
        bad.append("%s: weights differ from the oracle's Lagrange coefficients at the rows of sel_part (zero elsewhere), or the guard row was written" % case.tag)
    check_guarded_outputs(case.tag, w["status"] != OK, case.degree, a["out_commit"], a["out_share"], bad)
    return bad[:12]


def generate_verdict_case(P, kind):
    """k_dkg_part_status / k_dkg_generate_guard: (accept or None, point_bad, share_st or None, expected part_status)."""
    accept = [0 if p % 4 == 1 else 1 for p in range(P)] if kind != "no accept" else None
    point_bad, share_st = [0] * P, [OK] * P
    if kind in ("failing", "no accept"):
        for p in range(P):
            point_bad[p] = int(p % 5 == 0)
            share_st[p] = [OK, DUPLICATE, INVALID][p % 3]
    elif kind == "rejected only bad":
        for p in range(P):
            if p % 4 == 1:
                point_bad[p], share_st[p] = 1, DUPLICATE
    if kind == "observer":
        share_st = None
        point_bad[P - 1] = 1
    want = []
    for p in range(P):
        st = OK
        if accept is None or accept[p]:
            st = INVALID if point_bad[p] else (share_st[p] if share_st else OK)
        want.append(st)
    return accept, point_bad, share_st, want


GENERATE_SHAPES = [(P, kind) for P in (1, 7, 257) for kind in ("failing", "no accept", "rejected only bad", "observer", "clean")]


def run_generate_verdict(lib, P, kind, degree=2, with_outputs=(True, True)):
    accept, point_bad, share_st, want = generate_verdict_case(P, kind)
    part = fresh(P + 1)
    oc = np.full((degree + 2) * 96, KEEP, dtype=np.uint8) if with_outputs[0] else None
    osh = np.full(64, KEEP, dtype=np.uint8) if with_outputs[1] else None
    call(lib, "generate_verdict", np.array(accept, dtype=np.uint8) if accept else None, np.array(point_bad, dtype=np.uint8),
         np.array(share_st, dtype=np.uint8) if share_st else None, P, degree, part, oc, osh)
    bad = []
    if [int(x) for x in part[:P]] != want or part[P] != POISON:
        bad.append("generate verdict P = %d %s: part_status %s, expected %s" % (P, kind, part[:8], want[:8]))
    check_guarded_outputs("generate verdict P = %d %s" % (P, kind), any(s != OK for s in want), degree, oc, osh, bad)
    return bad
