"""Many-point conformance suite: the two-stage MSM kernels (k_msm.hip / tc_msm.h, G2 and G1) and the comb signer
(k_comb.hip / tc_comb.h) against Python big integers, beside the device conformance suite (tests/device_conformance.py), whose
oracle, psi, gls_bases, gls_digits, sac_model, limb helpers and NORM_LO / NORM_HI it reuses.

Two legs run THE SAME case tables through the same checkers:

  * tests/device/manypoint.hip (hipcc, the product's flags) launches the shipped kernels with launch parameters chosen by
    the test -- `parts` / `share` given, or 0 for the product's launcher --: tests/test_gpu_manypoint.py;
  * tests/device/manypoint_host.cpp (g++ -DTC_BOUND_CHECK) calls the header routines the kernels call, parts one after the
    other, then the kernel's xor tree of jac_add: tests/test_manypoint_host.py.

What is checked, all exact: output bytes (the oracle's uncompressed encoding of one multiplication by sum a_i s_i mod r --
every point is a known multiple [a_i] G), status bytes, the table entries the kernels leave in HBM (decoded from the raw
words of the tc_table.h / msm_store_entry_g1 layouts: the model's affine point, the infinity flag, every limb inside
[NORM_LO, NORM_HI] 2^28, |value| <= 2.1 p -- the contract tbl_load_fq declares --, padding words), the digit codes (the
model's for the columns in use, the 0x5A fill beyond the top column in short-scalar mode), that nothing else is written
(jobs the MsmFilter leaves to the fast path, *need == 0, table sets 1 .. B-1 of the shared set), and that every legal
`parts` / `share` and the launcher's own choice give the same bytes.

Models.  Stage T: per share the flip decision, the eight entries (G2: B0 + subsets of the psi-bases; G1: {P, P - phi',
P + 2 phi', P + phi', 3P, 3P + phi', 3P + 2 phi', 3P + 3 phi'}) from the oracle's affine group law, and the column codes.
Stage L: because every point is [a] G with known a, psi is [x] on G2 and phi' is [x^2] on G1, every table entry and every
accumulator value is a known multiple of G, and in a group of prime order r "P = +-Q" and "P = O" are statements about
these multiples mod r; walk_part walks the part's columns on them and reports the sum and whether the branch-free pass meets
a special case (an operand at infinity, P = +-Q).  walk_part_points is the same walk on the oracle's group law
(device_conformance._walk_add); test_manypoint_host.py shows that the two agree.  merge_events does the same for the xor
tree.  Every directed job carries a claim (which part meets a special case, which merge round doubles / cancels / meets the
identity) that the model must confirm, and random filler jobs must be shown to meet none.

Wave layout.  The kernels decide on the safe path once per wave (wave_any), so a batch opens with random jobs only (at the
larger `parts` they fill whole waves that stay on the fast path) and continues with directed jobs, three of them side by
side (whole waves on the safe path at the largest `parts`), then a random one (mixed waves).

Findings.  (1) job_msm_ladder_safe restarted an accumulator that had come back to the identity from a lazily negated y, which
the bound analysis rejects in the next addition ("merge opposite" in short-scalar mode at parts = 1: the whole job cancels);
the selected y is carried now.  (2) job_msm_tables_g1 wrote identities into the SHARED table set when job 0's own scalar was
bad (shared_case "job0 even" / "job0 >= r"); an entry depends on its point alone now.

The ragged sums of the records verifier (k_rec_tables_* / k_rec_ladder_* / k_rec_gather_keys, tc_records.h) run through the same
two legs, checkers and pool: RecCase and rec_case at the end of this file.  A launch is J segments of one record array; what is
new against the fixed-n kernels is where a lane finds its work (first_chunk[j], the segment's own column stride), one trip
count per WAVE, and parts without records.  Nothing was found there.

The PAIRED ragged sums of the decryption-share verifier (k_rec_tables_g1_pair / k_rec_ladder_g1_pair, tc_records.h rec_pair_*):
PairCase at the end of this file.  Their results never leave the device, and an error common to both halves -- a record dropped
from both, a wrong digit in both -- cancels in the product check that consumes them; here out[2 j] = A_j and out[2 j + 1] = -B_j are
compared byte for byte.  A launch is two RecCases, one per half, over the same scalars: the models, the claims and the table
checker are the unpaired ones, applied to half h at chunk offset h * chunks.  The halves of every segment are different samples of
the pool, and a directed segment has its special case in ONE half.

The G1 comb of the decryption shares (k_comb_tables_g1 / k_comb_decrypt, tc_comb_g1.h) and the arena ladders beside it
(k_g1_mul_gather): Comb1Case.  The launcher takes one holder per lane up to 131 072 (ciphertext, holder) pairs, so the suite
forces share = 1 .. 8: the wave's holder loop, lanes with fewer holders than their wave's longest, lanes past the end.  The 514
table entries per ciphertext are the model's, column by column (two doublings of the oracle's affine law per column).

Blame by bisection (k_blame_seed / k_blame_leaves / k_blame_range_sum, tc_blame_jobs.h), through a harness file of its own
(tests/device/manypoint_blame.hip; the host leg shares manypoint_host.cpp): LeavesCase, LadderCase, RangeCase and ChainCase at the end
of this file.  The leaves never leave the device and both sums of a bisection step are built from the same (job, lo, hi), so an
error common to both cancels in the pairing check; here every leaf is decoded from its raw words ([r_i] P_i with r from the
oracle's ChaCha20; the limb form, the padding words, the G2 row order), the leaf ladders run at digits ChaCha20 would give once
in 2^16 leaves or less, and every range sum is compared byte for byte at every parts -- parts beyond the length of a range
included, where most lanes run masked trips only (the one path the host leg cannot execute: there a lane is a wave).  Nothing was
found.
"""
import ctypes
import os
import random
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import device_conformance as dc  # noqa: E402

o = dc.o
R, X, X2, P = dc.R, dc.X, dc.X2, dc.P
OK, NOT_ENOUGH, INVALID = 0, 1, 3  # tc_codec.h TC_JOB_*
POISON = 0x5A
POISON_WORD = 0x5A5A5A5A
SLOT_LEAK = -2  # manypoint.hip kMpSlotLeak
COLS = 65       # tc_msm.h kMsmColumns / tc_comb.h kCombColumns
ENTRY = {1: 32, 2: 64}  # words per table entry: kMsmEntryWordsG1 / kTblEntryWords
PT_BYTES = {1: 96, 2: 192}
MAX_PARTS = {1: 64, 2: 32}
COMB_SHARE = 8  # tc_comb.h kCombShare
E = {1: o.E1, 2: o.E2}
GEN = {1: o.G1_GEN, 2: o.G2_GEN}
BAD_POINT = {w: bytes([0x1f]) + b"\xff" * (PT_BYTES[w] - 1) for w in (1, 2)}  # x >= p: no decoder takes it
DEV = dc.DEV


def enc(w, pt):
    return o.g1_uncompressed(pt) if w == 1 else o.g2_uncompressed(pt)


# ---------------------------------------------------------------------------------------------------------------------
# builds
# ---------------------------------------------------------------------------------------------------------------------
def build_device():
    """tests/device/manypoint.hip -> a gfx950 shared object, with the product's compiler flags (build.py FLAGS)."""
    from threshold_crypto_amd import build as tcb
    src = os.path.join(DEV, "manypoint.hip")
    return dc._build("libtc_manypoint", lambda out: [dc.hipcc()] + tcb.FLAGS + ["-w", "-shared", src, "-o", out], {"manypoint.hip"})


def build_host():
    src = os.path.join(DEV, "manypoint_host.cpp")
    return dc._build("libtc_manypoint_host_bc",
                     lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-shared", "-fPIC", src, "-o", out],
                     {"manypoint_host.cpp"})


def build_host_main(extra=()):
    """The stand-alone program of manypoint_host.cpp (its fixed short case list); extra: e.g. sanitizer flags."""
    src = os.path.join(DEV, "manypoint_host.cpp")
    return dc._build("manypoint_host_main",
                     lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-DMP_MAIN"] + list(extra) + [src, "-o", out],
                     {"manypoint_host.cpp"})


_SZ, _VP, _INT = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


def load(path, prefix):
    """prefix "mp_": the device harness; "mph_": the host leg.  The entries that both have take the same arguments in both."""
    lib = ctypes.CDLL(path)
    g2 = getattr(lib, prefix + "msm_g2")
    g2.argtypes = [_SZ, _SZ, _SZ, _VP, _VP, _VP, _INT, _SZ, _VP, _SZ, _SZ, _INT, _VP, _VP, _VP, _VP]
    g1 = getattr(lib, prefix + "msm_g1")
    g1.argtypes = [_SZ, _SZ, _SZ, _VP, _VP, _VP, _INT, _SZ, _VP, _VP, _VP, _VP]
    comb = getattr(lib, prefix + "comb")
    comb.argtypes = [_VP, _SZ, _VP, _VP, _SZ, _SZ, _SZ, _VP, _VP, _VP, _VP]
    rec = getattr(lib, prefix + "rec_sum")
    rec.argtypes = [_INT, _SZ, _VP, _VP, _VP, _VP, _INT, _SZ, _VP, _VP, _VP, _VP, _VP]
    gather = getattr(lib, prefix + "rec_gather_keys")
    gather.argtypes = [_VP, _SZ, _VP, _SZ, _VP]
    pair = getattr(lib, prefix + "rec_sum_pair")
    pair.argtypes = [_SZ, _VP, _VP, _VP, _VP, _VP, _INT, _SZ, _VP, _VP, _VP, _VP, _VP]
    comb1 = getattr(lib, prefix + "comb_g1")
    comb1.argtypes = [_VP, _SZ, _VP, _VP, _SZ, _SZ, _SZ, _VP, _VP, _VP, _VP]
    entries = {"g2": g2, "g1": g1, "comb": comb, "rec": rec, "gather": gather, "rec_pair": pair, "comb_g1": comb1}
    if prefix == "mp_":  # (the arena ladders of k_g1_mul_gather: the device leg only)
        entries["g1_mul_gather"] = lib.mp_g1_mul_gather
        entries["g1_mul_gather"].argtypes = [_VP, _SZ, _VP, _VP, _SZ, _SZ, _VP, _VP]
    for f in entries.values():
        f.restype = _INT
    return dict(entries, lib=lib, host=prefix == "mph_")


# ---------------------------------------------------------------------------------------------------------------------
# group elements as known multiples of the generator
# ---------------------------------------------------------------------------------------------------------------------
_POW2 = {}
_PT = {1: {0: None}, 2: {0: None}}  # multiple mod r -> affine point


def gmul(w, m):
    """[m] G (cached): the sum of the 2^i G of m's bits on the oracle's group law."""
    m %= R
    if m not in _PT[w]:
        if w not in _POW2:
            pw = [GEN[w]]
            for _ in range(254):
                pw.append(E[w].dbl(pw[-1]))
            _POW2[w] = pw
        acc = dc._jac_of(E[w], None)
        for i in range(255):
            if (m >> i) & 1:
                acc = E[w]._jadd_affine(acc, _POW2[w][i])
        _PT[w][m] = E[w]._to_affine(acc)
    return _PT[w][m]


POOL_SIZE = {1: 272, 2: 136}
_POOL = {}


def pool(w):
    """Distinct multiples a with their points: 24 random ones by multiplication, the rest by additions of those."""
    if w not in _POOL:
        rnd = random.Random("manypoint-pool-%d" % w)
        base = [rnd.randrange(1, R) for _ in range(24)]
        for a in base:
            _PT[w][a] = E[w].mul(GEN[w], a)
        mults = list(base)
        a = base[0]
        while len(mults) < POOL_SIZE[w]:
            b = base[rnd.randrange(24)]
            pt = E[w].add(_PT[w][a], _PT[w][b])
            a = (a + b) % R
            if a and a not in _PT[w]:
                _PT[w][a] = pt
                mults.append(a)
        _POOL[w] = mults
    return _POOL[w]


def neg_mult(w, a):
    """The multiple of -[a] G (its point goes into the cache without a multiplication)."""
    a %= R
    if a in _PT[w] and (R - a) % R not in _PT[w]:
        _PT[w][(R - a) % R] = E[w].neg(_PT[w][a])
    return (R - a) % R


# entry m of a share's table as a multiple of the share's (possibly negated) point
T2 = [1 + sum(X ** (j + 1) for j in range(3) if (m >> j) & 1) for m in range(8)]  # B0 + subsets of (|x|, |x|^2, |x|^3) B0
T1 = [(1, 0), (1, -1), (1, 2), (1, 1), (3, 0), (3, 1), (3, 2), (3, 3)]             # A P + B phi', phi' = [x^2] P
T1M = [A + B * X2 for A, B in T1]
TM = {1: T1M, 2: T2}


def entry_mults(w, a, flip):
    return [(-a if flip else a) * t % R for t in TM[w]]


def _phi_prime():
    """phi' = -phi on G1: (x, y) -> (beta x, -y) for the cube root of unity beta that makes it [x^2]."""
    want = o.E1.mul(o.G1_GEN, X2)
    g = pow(2, (P - 1) // 3, P)
    for beta in (g, g * g % P):
        if beta != 1 and (beta * o.G1_X % P, P - o.G1_Y) == want:
            return beta
    raise AssertionError("no cube root of unity gives [x^2]")


_BETA = []
_TBL = {1: {}, 2: {}}


def entry_points(w, a, flip=False):
    """The eight entries of a share with point [a] G by the oracle's AFFINE group law (cached per point)."""
    a %= R
    if a == 0:
        return [None] * 8
    if a not in _TBL[w]:
        Ec, p = E[w], gmul(w, a)
        if w == 2:
            tbl = dc.subset_table(o.E2, dc.gls_bases(p), True)
        else:
            if not _BETA:
                _BETA.append(_phi_prime())
            f1 = (_BETA[0] * p[0] % P, P - p[1])
            p3 = Ec.add(Ec.dbl(p), p)
            f2 = Ec.dbl(f1)
            f3 = Ec.add(f2, f1)
            tbl = [p, Ec.add(p, Ec.neg(f1)), Ec.add(p, f2), Ec.add(p, f1), p3, Ec.add(p3, f1), Ec.add(p3, f2), Ec.add(p3, f3)]
        _TBL[w][a] = tbl
    return [E[w].neg(e) for e in _TBL[w][a]] if flip else _TBL[w][a]


# ---------------------------------------------------------------------------------------------------------------------
# stage T: the recodings
# ---------------------------------------------------------------------------------------------------------------------
def sac_cols(d, nbits=64):
    """sac_recode4 over nbits columns: signs s_i (i < nbits; the leading +1 sits at column nbits), the bits u_j[i] and the
    top bits.  nbits = 64 is device_conformance.sac_model."""
    d0 = d[0] | 1
    s = [1 if (d0 >> (i + 1)) & 1 else -1 for i in range(nbits)]
    u, top = [], []
    for j in (1, 2, 3):
        k, uj = d[j], []
        for i in range(nbits):
            uj.append(k & 1)
            k = (k - s[i] * (k & 1)) >> 1
        u.append(uj)
        top.append(k)
    return s, u, top


def g2_codes(k, nbits=64, padding=False):
    """job_msm_tables' column codes of one share: (codes[0 .. nbits], flip, fits)."""
    if nbits == 64:
        flip, fits = k % 2 == 0, True
        d = dc.gls_digits(R - k if flip else k)
    else:
        flip = False
        d = dc.gls_digits(k)
        fits = padding or (k % 2 == 1 and all(x >> nbits == 0 for x in d))
        if padding or not fits:
            d = [1, 0, 0, 0]
    s, u, top = sac_cols(d, nbits)
    codes = [u[0][i] | u[1][i] << 1 | u[2][i] << 2 | (8 if s[i] < 0 else 0) for i in range(nbits)]
    return codes + [top[0] | top[1] << 1 | top[2] << 2], flip, fits


def g1_codes(k, nbits=128, padding=False):
    """msm_g1_recode's base-4 column codes of one share: (codes[0 .. nbits / 2], flip, fits)."""
    if nbits == 128:
        flip, fits = k % 2 == 0, True
        kp = R - k if flip else k
        k1, k2 = kp % X2, kp // X2
    else:
        flip = False
        if padding:
            k = 1
        k1, k2 = k % X2, k // X2
        fits = k1 % 2 == 1 and k1 >> nbits == 0 and k2 >> nbits == 0
        if not fits:
            k1, k2 = 1, 0
    k1 |= 1
    s = [1 if (k1 >> (i + 1)) & 1 else -1 for i in range(nbits)]
    u = []
    for i in range(nbits):
        u.append(k2 & 1)
        k2 = (k2 - s[i] * (k2 & 1)) >> 1
    codes = [u[2 * c] | u[2 * c + 1] << 1 | (4 if s[2 * c] == s[2 * c + 1] else 0) | (8 if s[2 * c + 1] < 0 else 0) for c in range(nbits // 2)]
    return codes + [3 if k2 else 0], flip, fits


def codes_of(w, k, nbits, padding=False):
    return g2_codes(k, nbits, padding) if w == 2 else g1_codes(k, nbits, padding)


def codes_value(w, codes):
    """The multiple of the share's (possibly negated) point that a column of codes stands for, in units of the point."""
    top = len(codes) - 1
    step = 2 if w == 2 else 4
    acc = TM[w][codes[top] & 7]
    for col in range(top - 1, -1, -1):
        c = codes[col]
        acc = acc * step + (-1 if c & 8 else 1) * TM[w][c & 7]
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# stage L: the walk, on multiples and on points
# ---------------------------------------------------------------------------------------------------------------------
def msm_part(n, g=0, parts=1):
    """tc_msm.h msm_part: (s0, s1, trips)."""
    return g * n // parts, (g + 1) * n // parts, -(-n // parts)


def legal_parts(w, n):
    """The values the launchers can produce: a power of two with at least four shares per part."""
    return [p for p in (1, 2, 4, 8, 16, 32, 64) if p <= MAX_PARTS[w] and (p == 1 or 4 * p <= n)]


def launcher_parts(w, n, B):
    """launch_msm_g2 / launch_msm_g1: the parts they pick."""
    parts, slots = 1, 65536 if w == 2 else 131072
    while parts < MAX_PARTS[w] and B * parts * 2 <= slots and parts * 2 * 4 <= n:
        parts *= 2
    return parts


def _rel(acc, e):
    """What the branch-free mixed addition cannot do: an operand at infinity, P = +-Q."""
    return e % R == 0 or acc % R == 0 or (acc - e) % R == 0 or (acc + e) % R == 0


def walk_part(w, mults, codes, s0, s1):
    """job_msm_ladder_part over the shares [s0, s1) on multiples of G: (the part's sum, a special case was met).
    mults[s]: the 8 entry multiples of share s; codes[s]: its column codes.  Masked look-ups are not visited: the kernel
    discards both their sum and their hit."""
    top = len(codes[s0]) - 1
    step = 2 if w == 2 else 4
    acc, special = None, False
    for col in range(top, -1, -1):
        if col != top:
            acc = acc * step % R
        for s in range(s0, s1):
            c = codes[s][col]
            e = mults[s][c & 7]
            if col != top and c & 8:
                e = -e % R
            if acc is None:
                acc, special = e, e == 0
            else:
                special |= _rel(acc, e)
                acc = (acc + e) % R
    return acc, special


def walk_part_points(w, points, codes, s0, s1):
    """The same walk on the oracle's group law (device_conformance._walk_add): (affine sum, special)."""
    Ec = E[w]
    top = len(codes[s0]) - 1
    acc, special = None, False
    for col in range(top, -1, -1):
        if col != top:
            acc = Ec._jdbl(acc)
            if w == 1:
                acc = Ec._jdbl(acc)
        for s in range(s0, s1):
            c = codes[s][col]
            e = points[s][c & 7]
            if col != top and c & 8:
                e = Ec.neg(e)
            if acc is None:
                acc, special = dc._jac_of(Ec, e), e is None
            else:
                acc, sp = dc._walk_add(Ec, acc, e)
                special |= sp
    return Ec._to_affine(acc), special


def merge_events(sums):
    """The xor tree of k_msm_ladder_split / k_msm_ladder_g1<true> over the parts' sums: (lane 0's result, the special
    operand pairs jac_add meets as (round, lane, kind))."""
    r, events, rnd_no, d = list(sums), [], 0, 1
    while d < len(r):
        nr = []
        for g in range(len(r)):
            a, b = r[g], r[g ^ d]
            kind = "identity" if a == 0 or b == 0 else "equal" if a == b else "opposite" if (a + b) % R == 0 else None
            if kind:
                events.append((rnd_no, g, kind))
            nr.append((a + b) % R)
        r, d, rnd_no = nr, d * 2, rnd_no + 1
    return r[0], events


# ---------------------------------------------------------------------------------------------------------------------
# MSM jobs and batches
# ---------------------------------------------------------------------------------------------------------------------
class Job:
    """a[i]: the multiple of share i's point (0: the identity; None: an undecodable encoding), k[i]: its scalar.
    claim: what the model must confirm -- "parts": p with "special": the parts (lane pairs) that meet a special case
    (exactly those), "special_at_1": whether the unsplit ladder meets one, "merge": (round, kind) an event of the tree.
    A random job claims that nothing special happens at any legal parts."""

    def __init__(self, a, k, tag, status_in=OK, claim=None, directed=(), idx=None):
        self.a, self.k, self.tag, self.status_in, self.claim, self.directed, self.idx = list(a), list(k), tag, status_in, claim, set(directed), idx
        self.random = False


class MsmCase:
    def __init__(self, w, n, B, nbits, jobs, parts, shared=False, filter_t=None, need=-1, tag=""):
        self.w, self.n, self.B, self.nbits, self.jobs, self.parts, self.shared = w, n, B, nbits, jobs, parts, shared
        self.filter_t, self.need, self.tag = filter_t, need, tag or "G%d n=%d nbits=%d B=%d%s" % (w, n, nbits, B, " shared" if shared else "")
        self.shares4 = 4 * ((n + 3) // 4)
        self.full = nbits == (64 if w == 2 else 128)
        self.top = nbits if w == 2 else nbits // 2
        assert len(jobs) == B
        self._ref = None

    # ---- inputs ----
    def points(self):
        jobs = self.jobs[:1] if self.shared else self.jobs
        return b"".join(BAD_POINT[self.w] if a is None else enc(self.w, gmul(self.w, a)) for j in jobs for a in j.a)

    def scalars(self):
        return np.array([dc.u32s(k) for j in self.jobs for k in j.k], dtype=np.uint32).reshape(-1)

    def pts_stride(self):
        return 0 if self.shared else self.n * PT_BYTES[self.w]

    def taken(self, j):
        """MsmFilter: the job belongs to the two-stage path."""
        if self.need == 0:
            return False
        t = self.filter_t
        return not (t is not None and 1 <= t <= 3 and dc.small_coeffs_model(self.jobs[j].idx[:t + 1]) is not None)

    # ---- the model of one job ----
    def share_codes(self, job):
        """Column codes of all shares4 shares, the flips and whether every scalar is one the mode takes."""
        out, flips, ok = [], [], True
        for s in range(self.shares4):
            pad = s >= self.n
            k = 0 if pad else job.k[s]
            if k >= R:
                ok = False
                k = 0
            c, flip, fits = codes_of(self.w, k, self.nbits, pad)
            ok &= fits
            out.append(c)
            flips.append(flip)
        return out, flips, ok

    def valid(self, job):
        return all(a is not None for a in job.a) and self.share_codes(job)[2]

    def job_model(self, job, parts):
        """(sum, per part: special, merge events) of a valid job on multiples of G."""
        codes, flips, _ = self.share_codes(job)
        mults = [entry_mults(self.w, job.a[s], flips[s]) for s in range(self.n)]
        sums, special = [], []
        for g in range(parts):
            s0, s1, _ = msm_part(self.n, g, parts)
            acc, sp = walk_part(self.w, mults, codes, s0, s1)
            sums.append(acc)
            special.append(sp)
        total, events = merge_events(sums)
        return total, special, events

    def ref(self):
        """Expected status and output bytes per job, computed once."""
        if self._ref is None:
            w, st, out = self.w, [], []
            for job in self.jobs:
                if job.status_in != OK:
                    st.append(job.status_in)
                    out.append(enc(w, None))
                elif not self.valid(job):
                    st.append(INVALID)
                    out.append(enc(w, None))
                else:
                    st.append(OK)
                    out.append(enc(w, gmul(w, sum(a * k for a, k in zip(job.a, job.k)) % R)))
            self._ref = (st, out)
        return self._ref

    def sample(self, job):
        """Shares whose table entries are decoded and compared: all of them up to n = 13, else the first and last share of
        every part of every legal parts, the padding shares and the job's directed shares."""
        if self.n <= 13:
            return list(range(self.shares4))
        s = set(range(self.n, self.shares4)) | {x for x in job.directed if x < self.n}
        for p in legal_parts(self.w, self.n):
            for g in range(p):
                s0, s1, _ = msm_part(self.n, g, p)
                s |= {s0, s1 - 1}
        return sorted(s)


# ---- scalars ----
def short_scalar(w, nbits, rnd):
    if w == 2:
        d = [rnd.getrandbits(nbits) | (1 if j == 0 else 0) for j in range(4)]
        return sum(x * X ** j for j, x in enumerate(d))
    return (rnd.getrandbits(nbits) | 1) + rnd.getrandbits(nbits) * X2


def rand_scalar(case_full, w, nbits, rnd):
    return rnd.randrange(1, R) if case_full else short_scalar(w, nbits, rnd)


def edge_scalars(w):
    ks = [0, 1, 2, R - 1, R - 2] + [X ** j + e for j in (1, 2, 3) for e in (0, 1, -1)] + [(1 << 64) - 1, 1 << 64, (1 << 64) + 1, (R - 1) // 2,
                                                                                         (R + 1) // 2]
    if w == 1:
        ks += [k for k in dc._g1_edges(None) if k < R and k not in ks]
        ks += [R - X2 * ((1 << 126) + 5) - 1]  # (k1 even: recoded as r - k)
    return ks


def _full(w, nbits):
    return nbits == (64 if w == 2 else 128)


def random_job(w, n, nbits, rnd, tag="random"):
    a = rnd.sample(pool(w), n)
    j = Job(a, [rand_scalar(_full(w, nbits), w, nbits, rnd) for _ in range(n)], tag)
    j.random = True
    return j


def _solve(job, shares, t, target):
    """Set the scalar of share t so that the shares' sum is `target` (multiples of G)."""
    rest = sum(job.a[s] * job.k[s] for s in shares if s != t) % R
    job.k[t] = (target - rest) * pow(job.a[t], -1, R) % R


def directed_jobs(w, n, nbits, rnd):
    """The directed jobs of one (group, n, nbits), each with the claim the model has to confirm (Job)."""
    full = _full(w, nbits)
    legal = legal_parts(w, n)
    split = [p for p in legal if p > 1]
    big = legal[-1]
    jobs = []

    def base(tag, **kw):
        j = random_job(w, n, nbits, rnd, tag)
        j.random = False
        j.__dict__.update(kw)
        jobs.append(j)
        return j

    def rng(p, g):
        return msm_part(n, g, p)[:2]

    # the identity
    for p, g in sorted({(big, big - 1), (big, 0)}):
        s0, _ = rng(p, g)
        j = base("identity first of part %d/%d" % (g, p), claim={"parts": p, "special": {g}}, directed={s0})
        j.a[s0] = 0
    if n >= 3:
        p = split[0] if split else 1
        s0, s1 = rng(p, p - 1)
        j = base("identity in the middle", claim={"parts": p, "special": {p - 1}}, directed={s0 + 1})
        j.a[s0 + 1] = 0
    if split:
        p = big
        g = 1
        s0, s1 = rng(p, g)
        j = base("identity: every share of part %d/%d" % (g, p), claim={"parts": p, "special": {g}, "merge": (0, "identity")}, directed=set(range(s0, s1)))
        for s in range(s0, s1):
            j.a[s] = 0
    j = base("identity: every share", claim={"parts": big, "special": set(range(big))}, directed=set(range(n)))
    j.a = [0] * n
    # scalar edges (full-scalar mode), spread over the shares of as many jobs as it takes
    if full:
        ks = edge_scalars(w)
        for i in range(0, len(ks), n):
            chunk = ks[i:i + n]
            j = base("scalar edges %d.." % i, directed=set(range(len(chunk))))
            j.k[:len(chunk)] = chunk
    # equal points with equal scalars, P and -P
    # (the branch-free addition meets P = +-Q when the SUM SO FAR is +-the entry: the first two shares of a part)
    p = split[-1] if split else 1
    g = p - 1
    s0, s1 = rng(p, g)
    if n >= 2:
        j = base("equal shares at the start of part %d/%d" % (g, p), claim={"parts": p, "special": {g}}, directed={s0, s0 + 1})
        j.a[s0 + 1], j.k[s0 + 1] = j.a[s0], j.k[s0]
        j = base("P and -P, equal scalars, at the start of part %d/%d" % (g, p), claim={"parts": p, "special": {g}}, directed={s0, s0 + 1})
        j.a[s0 + 1], j.k[s0 + 1] = neg_mult(w, j.a[s0]), j.k[s0]
        j = base("all shares equal", claim={"parts": big, "special": set(range(big))}, directed=set(range(n)))
        j.a, j.k = [j.a[0]] * n, [j.k[0]] * n
    if split:
        p = split[0]
        s0, s1 = rng(p, 0)
        # the last share of part 0 and the first of part 1 equal: at parts = 1 the second one meets a sum, at `p` it starts part 1
        j = base("equal shares across a part boundary", claim={"parts": p, "special": set()}, directed={s1 - 1, s1})
        j.a[s1], j.k[s1] = j.a[s1 - 1], j.k[s1 - 1]
        short = [(q, g) for q in split for g in range(q) if rng(q, g)[1] - rng(q, g)[0] < msm_part(n, g, q)[2] and rng(q, g)[1] < n]
        if short:  # n not divisible by parts: the masked look-up of a shorter part, next to the share it must not take
            q, g = short[-1]
            t0, t1 = rng(q, g)
            j = base("equal shares at the masked position of part %d/%d" % (g, q), claim={"parts": q, "special": set()}, directed={t0, t1 - 1, t1})
            j.a[t1], j.k[t1] = j.a[t1 - 1], j.k[t1 - 1]
            j.a[t0 + 1], j.k[t0 + 1] = neg_mult(w, j.a[t0 + 2]), j.k[t0 + 2]  # (... + Q - Q: sums that return to earlier values)
    # the merge: partial sums of two partners equal, opposite, one of them the identity; first and a later round
    for p, rd in ([(split[0], 0)] if split else []) + ([(big, big.bit_length() - 2)] if big >= 4 else []):
        d = 1 << rd
        sa = list(range(rng(p, 0)[0], rng(p, d - 1)[1]))
        sb = list(range(rng(p, d)[0], rng(p, 2 * d - 1)[1]))
        for kind in ("equal", "opposite", "identity"):
            j = base("merge %s at round %d of parts %d" % (kind, rd, p), claim={"parts": p, "merge": (rd, kind)}, directed={sb[-1]})
            if full:
                suma = sum(j.a[s] * j.k[s] for s in sa) % R
                _solve(j, sb, sb[-1], {"equal": suma, "opposite": -suma, "identity": 0}[kind])
            elif kind == "identity":
                for s in sb:
                    j.a[s] = 0
                j.directed |= set(sb)
            elif len(sa) == len(sb):  # short scalars cannot be solved for: the partner's content, or its negative
                for x, y in zip(sa, sb):
                    j.a[y], j.k[y] = (j.a[x] if kind == "equal" else neg_mult(w, j.a[x])), j.k[x]
                j.directed |= set(sb)
            else:
                jobs.pop()
    # failures and kept statuses
    base("status not OK on entry", status_in=NOT_ENOUGH)
    j = base("undecodable point", directed={n - 1})
    j.a[n - 1] = None
    j = base("scalar = r", directed={0})
    j.k[0] = R
    j = base("scalar = 2^256 - 1", directed={n // 2})
    j.k[n // 2] = (1 << 256) - 1
    if not full:
        top = (1 << nbits) - 1
        j = base("largest short digits", directed={0, n - 1})
        j.k[0] = j.k[n - 1] = sum(top * X ** i for i in range(4)) if w == 2 else top + top * X2
        j = base("even short scalar", directed={0})
        j.k[0] -= 1
        j = base("digit with bit nbits set", directed={n - 1})
        j.k[n - 1] = (1 + (1 << nbits) * X) if w == 2 else 1 + (1 << nbits) * X2
        if w == 1:
            j = base("k1 with bit nbits set", directed={0})
            j.k[0] = (1 << nbits) + 1
    return jobs


def check_claims(case):
    """The model confirms every directed job's claim, and shows the random jobs to meet no special case at all."""
    bad = []
    for ji, job in enumerate(case.jobs):
        if not case.valid(job):
            continue
        if job.random:
            for p in legal_parts(case.w, case.n):
                _, special, events = case.job_model(job, p)
                if any(special) or events:
                    bad.append("job %d (%s): random, but special at parts %d: %s %s" % (ji, job.tag, p, special, events))
        elif job.claim:
            c = job.claim
            _, special, events = case.job_model(job, c["parts"])
            if "special" in c and {g for g, sp in enumerate(special) if sp} != c["special"]:
                bad.append("job %d (%s): special parts %s, claimed %s" % (ji, job.tag, special, c["special"]))
            if "special_at_1" in c and case.job_model(job, 1)[1][0] != c["special_at_1"]:
                bad.append("job %d (%s): unsplit ladder special != %s" % (ji, job.tag, c["special_at_1"]))
            if "merge" in c and not any((r, k) == c["merge"] for r, _, k in events):
                bad.append("job %d (%s): merge events %s, claimed %s" % (ji, job.tag, events, c["merge"]))
    return bad


def lay_out(w, B, rnd_jobs, directed, head):
    """`head` random jobs, then directed jobs three at a time with a random one after them; random ones to the end."""
    jobs = [rnd_jobs() for _ in range(min(head, B))]
    d = list(directed)
    while len(jobs) < B:
        for _ in range(3):
            if d and len(jobs) < B:
                jobs.append(d.pop(0))
        if len(jobs) < B:
            jobs.append(rnd_jobs())
    return jobs, d


_CASES = {}


def msm_case(w, n, nbits, B, with_zero=True):
    """The batch of one shape row: own points, every legal parts and the launcher's choice (0)."""
    key = (w, n, nbits, B)
    if key not in _CASES:
        rnd = random.Random("manypoint-%d-%d-%d-%d" % key)

        def rj():
            for _ in range(50):
                j = random_job(w, n, nbits, rnd)
                one = MsmCase(w, n, 1, nbits, [j], [1])
                models = [one.job_model(j, p) for p in legal_parts(w, n)]
                if not any(any(sp) or ev for _, sp, ev in models):
                    return j
            raise AssertionError("no random job without a special case")
        directed = directed_jobs(w, n, nbits, rnd)
        head = {2: 8, 1: 32}[w] if B > 8 else 0
        jobs, left = lay_out(w, B, rj, directed, head)
        case = MsmCase(w, n, B, nbits, jobs, legal_parts(w, n) + [0])
        case.left_out = [j.tag for j in left]
        _CASES[key] = case
    return _CASES[key]


def top_case(w):
    """parts = 32 (G2, n = 128) / 64 (G1, n = 256) with B = 3: a random job, an identity at the start of the last part and
    merge partners that cancel at the last round."""
    n = {2: 128, 1: 256}[w]
    key = (w, n, "top")
    if key not in _CASES:
        nbits = 64 if w == 2 else 128
        rnd = random.Random("manypoint-top-%d" % w)
        d = directed_jobs(w, n, nbits, rnd)
        big = MAX_PARTS[w]
        pick = [j for j in d if j.tag.startswith("identity first of part %d/" % (big - 1)) or j.tag.startswith("merge opposite at round %d" % (big.bit_length() - 2))]
        assert len(pick) == 2, [j.tag for j in d]
        _CASES[key] = MsmCase(w, n, 3, nbits, [random_job(w, n, nbits, rnd)] + pick, [big, 0])
    return _CASES[key]


FILTER_IDS = [[0, 1, 2, 3], [70000, 1, 2, 3], [5, 2, 9, 7], [65535, 65536, 65537, 65538], [3, 4, 5, 6], [1 << 40, 2, 3, 4]]


def filter_case(n, need=-1):
    """The filter's shapes: one chunk with padding, t = n - 1, index lists the small-index fast path takes and leaves."""
    key = (2, n, "filter", need)
    if key not in _CASES:
        rnd = random.Random("manypoint-filter-%d" % n)
        B = 37
        d = [j for j in directed_jobs(2, n, 64, rnd) if "part boundary" not in j.tag]
        jobs, _ = lay_out(2, B, lambda: random_job(2, n, 64, rnd), d, 4)
        for i, j in enumerate(jobs):
            j.idx = FILTER_IDS[(i + i // 6) % len(FILTER_IDS)][:n]
            j.claim = None
            j.random = False
        _CASES[key] = MsmCase(2, n, B, 64, jobs, [1, 0], filter_t=n - 1, need=need, tag="G2 filter n=%d need=%d" % (n, need))
    return _CASES[key]


def shared_case(n, variant):
    """G1 short scalars over ONE point set (pts_stride = 0): every job's points are job 0's.  variant: "good" (failing jobs
    other than 0 among good ones), "job0 even", "job0 >= r" (a failing job 0: the table set it builds for everybody must
    not depend on its scalars)."""
    key = (1, n, "shared", variant)
    if key not in _CASES:
        rnd = random.Random("manypoint-shared-%d" % n)
        B, nbits = 70, 32
        a = rnd.sample(pool(1), n)
        jobs = []
        for i in range(B):
            j = Job(a, [short_scalar(1, nbits, rnd) for _ in range(n)], "shared %d" % i)
            jobs.append(j)
        top = (1 << nbits) - 1
        jobs[3].k[0] = jobs[3].k[n - 1] = top + top * X2
        jobs[3].tag = "largest short digits"
        jobs[5].k[1] -= 1
        jobs[5].tag = "even scalar in job 5"
        jobs[40].k[n - 1] = R
        jobs[40].tag = "scalar = r in job 40"
        jobs[66].status_in = NOT_ENOUGH
        jobs[67].k[2] = 1 + (1 << nbits) * X2
        jobs[67].tag = "k2 with bit nbits set"
        if variant == "job0 even":
            jobs[0].k[0] -= 1
        elif variant == "job0 >= r":
            jobs[0].k[0] = R + 2
        else:
            assert variant == "good"
        for j in jobs:
            j.directed = {0, 1, 2, 3}
        _CASES[key] = MsmCase(1, n, B, nbits, jobs, legal_parts(1, n) + [0], shared=True, tag="G1 shared n=%d %s" % (n, variant))
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------
# running and checking an MSM batch
# ---------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class HipError(AssertionError):
    pass


def run_msm(lib, case, parts):
    """(out, status, tbl, codes) as the leg left them; tbl as int32 (B x shares4 x 8 x entry words), codes (B x 65 x shares4)."""
    w, n, B = case.w, case.n, case.B
    pts = np.frombuffer(case.points(), dtype=np.uint8).copy()
    sc = case.scalars()
    st_in = np.array([j.status_in for j in case.jobs], dtype=np.uint8)
    out = np.full(B * PT_BYTES[w], POISON, dtype=np.uint8)
    status = np.full(B, POISON, dtype=np.uint8)
    tbl = np.full(B * case.shares4 * 8 * ENTRY[w], POISON_WORD, dtype=np.int32)
    codes = np.full(B * COLS * case.shares4, POISON, dtype=np.uint8)
    if w == 2:
        idx = None
        if case.filter_t is not None:
            idx = np.array([j.idx for j in case.jobs], dtype=np.uint64).reshape(-1)
        rc = lib["g2"](n, B, case.pts_stride(), _ptr(pts), _ptr(sc), _ptr(st_in), case.nbits, parts, _ptr(idx) if idx is not None else None,
                       n if idx is not None else 0, case.filter_t or 0, case.need, _ptr(out), _ptr(status), _ptr(tbl), _ptr(codes))
    else:
        rc = lib["g1"](n, B, case.pts_stride(), _ptr(pts), _ptr(sc), _ptr(st_in), case.nbits, parts, _ptr(out), _ptr(status), _ptr(tbl), _ptr(codes))
    if rc != 0:
        raise HipError("%s parts=%d: the harness returned %d" % (case.tag, parts, rc))
    return (out.reshape(B, -1), status, tbl.reshape(B, case.shares4, 8, ENTRY[w]), codes.reshape(B, COLS, case.shares4))


_LIMB_LO, _LIMB_HI = dc.NORM_LO * (1 << dc.RB), dc.NORM_HI * (1 << dc.RB)
_TOP_MAX = max(-_LIMB_LO, _LIMB_HI)
TBL_VAL = 2.1  # tc_table.h tbl_load_fq: |value| <= 2.1 p


def coord(words, what, bad):
    """One stored coordinate (16 words): limbs inside the normalised interval, |value| <= 2.1 p; returns the residue."""
    l = [int(x) for x in words[:14]]
    if not (all(_LIMB_LO <= x <= _LIMB_HI for x in l[:13]) and abs(l[13]) <= _TOP_MAX):
        bad.append("%s: limbs outside [%g, %g] 2^28: %s" % (what, dc.NORM_LO, dc.NORM_HI, l))
    v = dc.value(l)
    if abs(v) > TBL_VAL * P:
        bad.append("%s: |value| = %.3f p > 2.1 p" % (what, abs(v) / P))
    return v * dc.RINV % P


def check_entry(w, e, want, what, bad):
    """One table entry in the layout of tbl_store_g2 (x.c0, x.c1, y.c0, y.c1 rows of 16 words; word 15 of both x rows: the
    infinity flag) or msm_store_entry_g1 (x, y rows; word 15 of x: the flag), against the model's affine point."""
    e = [int(x) for x in e]
    rows = 4 if w == 2 else 2
    flag_rows = (0, 1) if w == 2 else (0,)
    for r in range(rows):
        if e[16 * r + 14] != 0 or e[16 * r + 15] != (int(want is None) if r in flag_rows else 0):
            bad.append("%s: padding words of row %d: %s (infinity expected: %s)" % (what, r, e[16 * r + 14:16 * r + 16], want is None))
    cs = [coord(e[16 * r:16 * r + 16], "%s row %d" % (what, r), bad) for r in range(rows)]
    if want is not None:
        got = ((cs[0], cs[1]), (cs[2], cs[3])) if w == 2 else (cs[0], cs[1])
        if got != want:
            bad.append("%s: wrong point" % what)


def check_msm(case, parts, res, max_report=12):
    """Every check of the suite on one run; returns the list of failures."""
    out, status, tbl, codes = res
    w, n, B = case.w, case.n, case.B
    want_st, want_out = case.ref()
    bad = []
    poison_pt = bytes([POISON]) * PT_BYTES[w]
    for ji, job in enumerate(case.jobs):
        what = "%s parts=%d job %d (%s)" % (case.tag, parts, ji, job.tag)
        if len(bad) > max_report:
            break
        if not case.taken(ji):  # left to the fast path / nothing to do: nothing is written
            if bytes(out[ji]) != poison_pt or status[ji] != job.status_in:
                bad.append("%s: not taken, but output or status written" % what)
            if not (tbl[ji] == POISON_WORD).all() or not (codes[ji] == POISON).all():
                bad.append("%s: not taken, but tables or codes written" % what)
            continue
        if status[ji] != want_st[ji]:
            bad.append("%s: status %d, expected %d" % (what, status[ji], want_st[ji]))
        if bytes(out[ji]) != want_out[ji]:
            bad.append("%s: wrong output bytes" % what)
        if not (codes[ji, case.top + 1:] == POISON).all():
            bad.append("%s: codes written past column %d" % (what, case.top))
        if case.shared and ji:
            if not (tbl[ji] == POISON_WORD).all():
                bad.append("%s: table set %d of the shared mode written" % (what, ji))
        points_ok = all(a is not None for a in job.a)
        if not case.valid(job) and not (case.shared and points_ok):
            continue  # (a failed job's tables and codes are not read by anybody)
        mcodes, flips, scal_ok = case.share_codes(job)
        if scal_ok:
            got = codes[ji, :case.top + 1, :].T.tolist()
            if got != mcodes:
                s = next(s for s in range(case.shares4) if got[s] != mcodes[s])
                bad.append("%s: codes of share %d: %s, expected %s" % (what, s, got[s], mcodes[s]))
        if case.shared and ji:
            continue
        for s in case.sample(job):
            want = entry_points(w, job.a[s] if s < n else 0, flips[s] and s < n and scal_ok)
            for m in range(8):
                check_entry(w, tbl[ji, s, m], want[m], "%s share %d entry %d" % (what, s, m), bad)
        # limb range of everything the job stored (the sampled entries also had their values checked)
        limbs = tbl[ji].reshape(case.shares4, 8, -1, 16)[..., :13]
        if limbs.min() < _LIMB_LO or limbs.max() > _LIMB_HI:
            bad.append("%s: a stored limb outside [%g, %g] 2^28" % (what, dc.NORM_LO, dc.NORM_HI))
    return bad


def sweep(lib, case, run, check, values, name, launch=None):
    """One run of `case` per value of the launch parameter `name`.  The first run, and every run whose bytes differ from it, goes
    through `check`; then all runs must have left the first run's bytes.  launch(run, lib, case, value): the caller's wrapper of a
    run (the GPU leg launches nothing after a HIP error).  Returns the first run's buffers."""
    first = v0 = None
    for v in values:
        res = launch(run, lib, case, v) if launch else run(lib, case, v)
        if first is None or not all((a == b).all() for a, b in zip(res, first)):  # (equal bytes need no second decoding)
            bad = check(case, v, res)
            assert not bad, "\n".join(bad[:12])
        if first is None:
            first, v0 = res, v
        assert all((a == b).all() for a, b in zip(res, first)), "%s: %s = %d and %s = %d leave different bytes" % (case.tag, name, v, name, v0)
    return first


# ---------------------------------------------------------------------------------------------------------------------
# the comb signer
# ---------------------------------------------------------------------------------------------------------------------
def comb_model(k):
    """job_comb_sign for the key k < r over a point [a] G, in units of a: (flip, fix, special of the doubling-free pass when
    a != 0, the multiple before the flip)."""
    flip = k % 2 == 0
    d = dc.gls_digits(R - k if flip else k)
    s, u, top, fix = dc.sac_model(d)
    acc = (T2[top[0] | top[1] << 1 | top[2] << 2] << 64) % R
    special = False
    for bit in range(63, -1, -1):
        e = s[bit] * (T2[u[0][bit] | u[1][bit] << 1 | u[2][bit] << 2] << bit) % R
        special |= _rel(acc, e)
        acc = (acc + e) % R
    if fix:
        acc = (acc - 1) % R
    return flip, fix, special, acc


class CombCase:
    """N keys, B messages (a multiple of G2's generator, 0 = the identity, None = undecodable), n signer indices each."""

    def __init__(self, n, B, shares, tag=""):
        rnd = random.Random("manypoint-comb-%d-%d" % (n, B))
        self.n, self.B, self.N, self.shares = n, B, 40, shares
        self.tag = tag or "comb n=%d B=%d" % (n, B)
        ks = [0, 1, 2, R - 1, R, 3, (1 << 256) - 1, R - 2, X, X + 1, X ** 3 - 1, (R - 1) // 2]
        self.keys = ks + [rnd.randrange(R) for _ in range(self.N - len(ks))]
        msgs = [pool(2)[0], 0, pool(2)[1], None, pool(2)[2]]
        self.msgs = [msgs[j % 5] for j in range(B)]
        self.idx = []
        for j in range(B):
            row = [(j * 7 + 3 * s) % self.N for s in range(n)] if j % 2 else [(s + 3 * j) % 12 for s in range(n)]  # (the directed keys: the even rows)
            if j % 3 == 0:
                row[n // 2] = self.N          # the first index out of range
            if j % 3 == 1:
                row[n - 1] = 1 << 63
            self.idx.append(row)
        self._ref = None
        self._tables = {}

    def ref(self):
        if self._ref is None:
            st, out = [], []
            for j in range(self.B):
                a = self.msgs[j]
                for i in self.idx[j]:
                    good = a is not None and i < self.N and self.keys[i] < R
                    st.append(OK if good else INVALID)
                    out.append(enc(2, gmul(2, a * self.keys[i] % R) if good else None))
            self._ref = (st, out)
        return self._ref

    def table(self, a):
        """The 65 x 8 comb of a message: entry (c, m) = 2^c T[m], by doublings on the oracle's affine group law."""
        if a not in self._tables:
            col = entry_points(2, a or 0)
            cols = [col]
            for _ in range(COLS - 1):
                col = [o.E2.dbl(e) for e in col]
                cols.append(col)
            self._tables[a] = cols
        return self._tables[a]


_COMB = {}


def comb_case(n, B):
    if (n, B) not in _COMB:
        _COMB[(n, B)] = CombCase(n, B, list(range(1, COMB_SHARE + 1)) + [0] if B <= 8 else [3, 0])
    return _COMB[(n, B)]


def run_comb(lib, case, share):
    n, B, N = case.n, case.B, case.N
    sk = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in case.keys), dtype=np.uint8).copy()
    idx = np.array(case.idx, dtype=np.uint64).reshape(-1)
    pts = np.frombuffer(b"".join(BAD_POINT[2] if a is None else enc(2, gmul(2, a)) for a in case.msgs), dtype=np.uint8).copy()
    out = np.full(B * n * 192, POISON, dtype=np.uint8)
    status = np.full(B * n, POISON, dtype=np.uint8)
    ok = np.full(B, POISON, dtype=np.uint8)
    tbl = np.full(B * COLS * 8 * 64, POISON_WORD, dtype=np.int32)
    rc = lib["comb"](_ptr(sk), N, _ptr(idx), _ptr(pts), n, B, share, _ptr(out), _ptr(status), _ptr(ok), _ptr(tbl))
    if rc != 0:
        raise HipError("%s share=%d: the harness returned %d%s" % (case.tag, share, rc, " (a table slot stayed in use)" if rc == SLOT_LEAK else ""))
    return out.reshape(B * n, 192), status, ok, tbl.reshape(B, COLS, 8, 64)


def check_comb(case, share, res, max_report=12):
    out, status, ok, tbl = res
    want_st, want_out = case.ref()
    bad = []
    for i in range(case.B * case.n):
        what = "%s share=%d message %d signer %d" % (case.tag, share, i // case.n, i % case.n)
        if status[i] != want_st[i]:
            bad.append("%s: status %d, expected %d" % (what, status[i], want_st[i]))
        if bytes(out[i]) != want_out[i]:
            bad.append("%s: wrong output bytes" % what)
        if len(bad) > max_report:
            return bad
    first = {}
    for j, a in enumerate(case.msgs):
        what = "%s share=%d message %d" % (case.tag, share, j)
        if ok[j] != int(a is not None):
            bad.append("%s: ok byte %d" % (what, ok[j]))
        if a in first:  # the same point: the same table, word for word (the first one is decoded)
            if not (tbl[j] == tbl[first[a]]).all():
                bad.append("%s: its comb differs from message %d's over the same point" % (what, first[a]))
            continue
        first[a] = j
        want = case.table(a)
        for c in range(COLS):
            for m in range(8):
                check_entry(2, tbl[j, c, m], want[c][m], "%s comb entry (%d, %d)" % (what, c, m), bad)
            if len(bad) > max_report:
                return bad
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the G1 comb of the decryption shares (k_comb_tables_g1 / k_comb_decrypt / k_g1_mul_gather; tc_comb_g1.h)
# ---------------------------------------------------------------------------------------------------------------------
# Stage S gives a lane one ciphertext and up to `share` of its n holders, chunk-major (lane = chunk * B + ciphertext), and the
# holder loop is the WAVE's: a lane with fewer holders than the longest of its wave repeats its first one and drops the result,
# a lane past the end has none.  The launcher takes share = 1 up to 131 072 (ciphertext, holder) pairs, so the suite forces it.
COMB1_COLS = 64                   # tc_comb_g1.h kCombG1Columns
COMB1_ENTRIES = COMB1_COLS * 8 + 2
COMB1_N = 16
COMB1_SHAPES = [(1, 5), (7, 5), (8, 5), (9, 5), (17, 5), (9, 70)]
COMB1_CHECKED = {5: [0, 1, 2, 3, 4], 70: [0, 63, 64, 69]}  # the ciphertexts whose 514 entries are decoded
K_ZERO, K_R, K_BIG = 0, 10, 11   # places in the key table: the scalar 0, r and 2^256 - 1
# what a case has to contain, per share, as comb1_events finds it
COMB1_CLAIMS = {
    (1, 5): {1: {"index out of range first of chunk"}},
    (7, 5): {2: {"zero first of short last chunk in a mixed wave"}, 7: {"zero in the middle of a full chunk"}},
    (8, 5): {8: {"zero in the middle of a full chunk", "index out of range first of chunk", "invalid scalar last of chunk"}},
    (9, 5): {8: {"zero first of short last chunk in a mixed wave", "zero in the middle of a full chunk", "index out of range first of chunk",
                 "index out of range last of chunk", "invalid scalar last of chunk"},
             4: {"zero first of short last chunk in a mixed wave", "invalid scalar first of chunk"}},
    (17, 5): {8: {"zero first of short last chunk in a mixed wave"}},
    (9, 70): {s: {"zero first of short last chunk in a mixed wave", "zero in the middle of a full chunk", "identity u in a mixed wave",
                  "undecodable u in a mixed wave", "invalid scalar first of chunk", "invalid scalar last of chunk",
                  "index out of range first of chunk", "index out of range last of chunk", "lanes past the end beside live ones"} for s in (4, 8)},
}


def comb1_model(k):
    """job_comb_decrypt for the scalar k < r over a point other than the identity, in units of the point: (the multiple, the
    doubling-free pass meets a special case).  The recoding is the ladder's (g1_codes); the comb is built over P, the result
    negated for an even k."""
    codes, flip, _ = g1_codes(k)
    acc = (T1M[codes[COMB1_COLS] & 7] << 128) % R
    special = False
    for c in range(COMB1_COLS - 1, -1, -1):
        e = (-1 if codes[c] & 8 else 1) * (T1M[codes[c] & 7] << (2 * c)) % R
        special |= _rel(acc, e)
        acc = (acc + e) % R
    return (R - acc if flip else acc) % R, special


class Comb1Case:
    """N keys, B ciphertexts (u a multiple of G1's generator, 0 = the identity, None = undecodable), n holder indices each."""

    def __init__(self, n, B):
        rnd = random.Random("manypoint-comb1-%d-%d" % (n, B))
        self.n, self.B, self.N, self.tag = n, B, COMB1_N, "comb G1 n=%d B=%d" % (n, B)
        self.shares = list(range(COMB_SHARE + 1))
        self.keys = [0, 1, 2, 3, 4, 5, X2, X2 - 1, X2 + 1, R - 1, R, (1 << 256) - 1] + [rnd.randrange(1, R) for _ in range(4)]
        good = [i for i, k in enumerate(self.keys) if 0 < k < R]
        N, last = self.N, n - 1
        self.u = [pool(1)[j % 3] for j in range(B)]
        if B == 5:
            self.u[3], self.u[4] = 0, None
            rows = {1: "descending", 2: "repeated"}
            put = {(0, last): K_ZERO, (0, 1): K_ZERO, (2, 7): (1 << 64) - 1, (2, 4): K_BIG, (2, last): K_R, (2, 0): N, (3, 0): 1 << 32}
        else:
            self.u[64], self.u[69] = 0, None
            rows = {60: "descending", 61: "repeated"}
            put = {(3, 8): K_ZERO, (66, 8): K_ZERO, (5, 2): K_ZERO, (7, 0): N, (7, 7): K_R, (9, 0): K_BIG, (9, 7): (1 << 64) - 1, (11, 4): 1 << 32,
                   (11, 3): K_R, (63, 5): N}
        self.idx = []
        for j in range(B):
            how = rows.get(j)
            self.idx.append([good[-1 - s % len(good)] if how == "descending" else 7 if how == "repeated" else good[(5 * j + 3 * s) % len(good)]
                             for s in range(n)])
        for (j, s), i in put.items():  # (a later entry wins where two fall on one place of a short row)
            if s < n and not (i == K_ZERO and s == 1 and n < 3):
                self.idx[j][s] = i
        self.checked = COMB1_CHECKED[B]
        self._ref = None
        self._tables = {}

    def ref(self):
        if self._ref is None:
            st, out = [], []
            for j in range(self.B):
                a = self.u[j]
                for i in self.idx[j]:
                    good = a is not None and i < self.N and self.keys[i] < R
                    st.append(OK if good else INVALID)
                    out.append(enc(1, gmul(1, a * self.keys[i] % R) if good else None))
            self._ref = (st, out)
        return self._ref

    def table(self, a):
        """The 514 entries over u = [a] G: entry c * 8 + m = 4^c T[m] column by column, two doublings of the oracle's affine
        group law per column; then the start entries 4^64 T[0] and 4^64 T[3]."""
        if a not in self._tables:
            col = entry_points(1, a or 0)
            ents = []
            for _ in range(COMB1_COLS):
                ents += col
                col = [o.E1.dbl(o.E1.dbl(e)) for e in col]
            self._tables[a] = ents + [col[0], col[3]]
        return self._tables[a]


def comb1_events(case, share):
    """What the lanes of k_comb_decrypt meet at `share` holders per lane, by the kernel's lane order: the kinds COMB1_CLAIMS names."""
    n, B, N = case.n, case.B, case.N
    chunks = -(-n // share)
    lanes = chunks * B
    cnt_of = lambda tid: min(share, n - tid // B * share) if tid < lanes else 0  # noqa: E731
    waves = [{cnt_of(t) for t in range(w0, w0 + 64)} for w0 in range(0, lanes, 64)]
    mixed = [share in cs and any(0 < c < share for c in cs) for cs in waves]
    found = set()
    if lanes % 64:
        found.add("lanes past the end beside live ones")
    for tid in range(lanes):
        c, j = tid // B, tid % B
        s0, cnt, u = c * share, cnt_of(tid), case.u[j]
        if mixed[tid // 64] and u in (0, None):
            found.add("identity u in a mixed wave" if u == 0 else "undecodable u in a mixed wave")
        for s in range(s0, s0 + cnt):
            i = case.idx[j][s]
            where = [w for w, hit in (("first", s == s0), ("last", s == s0 + cnt - 1)) if hit]
            if i >= N or case.keys[i] >= R:
                found |= {"%s %s of chunk" % ("index out of range" if i >= N else "invalid scalar", w) for w in where}
            elif u not in (0, None) and comb1_model(case.keys[i])[1]:  # (the scalar 0, test_manypoint_host.py shows)
                if s == s0 and cnt < share and c == chunks - 1 and mixed[tid // 64]:
                    found.add("zero first of short last chunk in a mixed wave")
                if cnt == share and not where:
                    found.add("zero in the middle of a full chunk")
    return found


_COMB1 = {}


def comb1_case(n, B):
    if (n, B) not in _COMB1:
        _COMB1[(n, B)] = Comb1Case(n, B)
    return _COMB1[(n, B)]


def _comb1_in(case):
    sk = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in case.keys), dtype=np.uint8).copy()
    idx = np.array(case.idx, dtype=np.uint64).reshape(-1)
    pts = np.frombuffer(b"".join(BAD_POINT[1] if a is None else enc(1, gmul(1, a)) for a in case.u), dtype=np.uint8).copy()
    out = np.full((case.B * case.n + 1) * 96, POISON, dtype=np.uint8)
    status = np.full(case.B * case.n + 1, POISON, dtype=np.uint8)
    return sk, idx, pts, out, status


def run_comb1(lib, case, share):
    """(out (B n + 1 rows), status (B n + 1), ok (B + 1), tbl (B x 514 entries and a guard entry)) as the leg left them."""
    sk, idx, pts, out, status = _comb1_in(case)
    ok = np.full(case.B + 1, POISON, dtype=np.uint8)
    tbl = np.full((case.B * COMB1_ENTRIES + 1) * ENTRY[1], POISON_WORD, dtype=np.int32)
    rc = lib["comb_g1"](_ptr(sk), case.N, _ptr(idx), _ptr(pts), case.n, case.B, share, _ptr(out), _ptr(status), _ptr(ok), _ptr(tbl))
    if rc != 0:
        raise HipError("%s share=%d: the harness returned %d" % (case.tag, share, rc))
    return out.reshape(-1, 96), status, ok, tbl.reshape(-1, ENTRY[1])


def run_g1_mul_gather(lib, case):
    """k_g1_mul_gather over the comb's case: (out (B n + 1 rows), status (B n + 1))."""
    sk, idx, pts, out, status = _comb1_in(case)
    rc = lib["g1_mul_gather"](_ptr(sk), case.N, _ptr(idx), _ptr(pts), case.n, case.B, _ptr(out), _ptr(status))
    if rc != 0:
        raise HipError("%s gather: the harness returned %d%s" % (case.tag, rc, " (a table slot stayed in use)" if rc == SLOT_LEAK else ""))
    return out.reshape(-1, 96), status


def check_comb1_out(case, what0, out, status, max_report=12):
    """Outputs and statuses of a run over a Comb1Case (the comb's or the gather ladders'), and the guards behind them."""
    want_st, want_out = case.ref()
    bad, rows = [], case.B * case.n
    if bytes(out[rows]) != bytes([POISON]) * 96 or status[rows] != POISON:
        bad.append("%s: output or status written behind the last share" % what0)
    for i in range(rows):
        what = "%s ciphertext %d holder %d" % (what0, i // case.n, i % case.n)
        if status[i] != want_st[i]:
            bad.append("%s: status %d, expected %d" % (what, status[i], want_st[i]))
        if bytes(out[i]) != want_out[i]:
            bad.append("%s: wrong output bytes" % what)
        if len(bad) > max_report:
            break
    return bad


def check_comb1(case, share, res, max_report=12):
    out, status, ok, tbl = res
    what0 = "%s share=%d" % (case.tag, share)
    bad = check_comb1_out(case, what0, out, status, max_report)
    if ok[case.B] != POISON or not (tbl[case.B * COMB1_ENTRIES] == POISON_WORD).all():
        bad.append("%s: the ok byte or the table entry behind the last ciphertext written" % what0)
    limbs = tbl[:case.B * COMB1_ENTRIES].reshape(-1, 2, 16)[..., :13]
    if limbs.min() < _LIMB_LO or limbs.max() > _LIMB_HI:
        bad.append("%s: a stored limb outside [%g, %g] 2^28" % (what0, dc.NORM_LO, dc.NORM_HI))
    first = {}
    for j, a in enumerate(case.u):
        what = "%s ciphertext %d" % (what0, j)
        t = tbl[j * COMB1_ENTRIES:(j + 1) * COMB1_ENTRIES]
        if ok[j] != int(a is not None):
            bad.append("%s: ok byte %d" % (what, ok[j]))
        if a in first and not (t == tbl[first[a] * COMB1_ENTRIES:(first[a] + 1) * COMB1_ENTRIES]).all():
            bad.append("%s: its comb differs from ciphertext %d's over the same point" % (what, first[a]))
        first.setdefault(a, j)
        if j not in case.checked or len(bad) > max_report:
            continue
        want = case.table(a)  # (None, an undecodable u: the identity's table)
        for e in range(COMB1_ENTRIES):
            check_entry(1, t[e], want[e], "%s comb entry %d (column %d)" % (what, e, e // 8), bad)
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the ragged sums (k_rec_tables_* / k_rec_ladder_* / k_rec_gather_keys; tc_records.h)
# ---------------------------------------------------------------------------------------------------------------------
# A launch is J SEGMENTS of one record array.  Segment j of len records keeps the tables and codes of a fixed-n job with n = len,
# at first_chunk[j] (the column stride of its codes is its OWN shares4); stage L gives it `parts` lanes / lane pairs, rec_part's
# ranges, of which some are EMPTY when len < parts, and every lane of a wave runs the trip count of the longest part in the wave.
# A segment is a Job (a[i], k[i], status_in); its claim is a LIST of claims, one per `parts` it speaks about.
REC_PARTS = {w: [p for p in (1, 2, 4, 8, 16, 32, 64) if p <= MAX_PARTS[w]] for w in (1, 2)}
REC_ILLEGAL = {w: [3, 2 * MAX_PARTS[w]] for w in (1, 2)}  # the launchers run them as parts = 1
REC_NBITS = {1: 80, 2: 16}                                # the modes tc_verify_*_records_rlc_batch ships
REC_FULL = {1: 128, 2: 64}
REC_J = 70
REC_HEAD = [0, 0, 130, 1, 65, 2, 64, 3, 33, 4, 5, 7, 8, 9, 1, 2]  # random segments: long and short ones side by side


def rec_part(length, g, parts):
    """tc_records.h rec_part and rec_part_trips: (s0, s1, trips); s0 == s1: the part is empty."""
    return g * length // parts, (g + 1) * length // parts, -(-length // parts)


class RecCase:
    def __init__(self, w, nbits, segs, tag, parts=None):
        self.w, self.nbits, self.segs, self.tag, self.J = w, nbits, segs, tag, len(segs)
        self.parts = list(parts) if parts else REC_PARTS[w] + REC_ILLEGAL[w]
        self.top = nbits if w == 2 else nbits // 2
        self.lens = [len(s.a) for s in segs]
        self.seg_first, self.first_chunk = [0], [0]
        for n in self.lens:
            self.seg_first.append(self.seg_first[-1] + n)
            self.first_chunk.append(self.first_chunk[-1] + (n + 3) // 4)
        self.records, self.chunks = self.seg_first[-1], self.first_chunk[-1]
        self.one = [MsmCase(w, len(s.a), 1, nbits, [s], [1]) for s in segs]  # the fixed-n model of a segment's stage T
        self._ref = None

    def valid(self, j):
        return self.one[j].valid(self.segs[j])

    def seg_model(self, j, parts):
        """(sum, per part: special, merge events) of a valid segment on multiples of G.  An empty part has the sum 0; what its
        lane computes before the kernel replaces it cannot be observed and is not described."""
        seg, n = self.segs[j], self.lens[j]
        codes, flips, _ = self.one[j].share_codes(seg)
        mults = [entry_mults(self.w, seg.a[s], flips[s]) for s in range(n)]
        sums, special = [], []
        for g in range(parts):
            s0, s1, _ = rec_part(n, g, parts)
            acc, sp = walk_part(self.w, mults, codes, s0, s1) if s0 < s1 else (0, False)
            sums.append(acc)
            special.append(sp)
        total, events = merge_events(sums)
        return total, special, events

    def ref(self):
        """Expected status and output bytes per segment, once.  A launch without a record returns before it writes anything."""
        if self._ref is None:
            w, st, out = self.w, [], []
            for j, seg in enumerate(self.segs):
                good = seg.status_in == OK and self.valid(j)
                st.append(seg.status_in if seg.status_in != OK else OK if good else INVALID)
                if self.chunks == 0:
                    out.append(bytes([POISON]) * PT_BYTES[w])
                else:
                    out.append(enc(w, gmul(w, sum(a * k for a, k in zip(seg.a, seg.k)) % R) if good else None))
            if self.chunks == 0:
                st = [seg.status_in for seg in self.segs]
            self._ref = (st, out)
        return self._ref


def check_rec_claims(case):
    """The model confirms every claim of every directed segment; a random segment meets no special case in any part at any
    parts, and its tree meets nothing but the identities that its EMPTY parts bring (parts > len)."""
    bad = []
    for j, seg in enumerate(case.segs):
        if not case.valid(j):
            continue
        what = "%s segment %d (%s, len %d)" % (case.tag, j, seg.tag, case.lens[j])
        if seg.random:
            for p in REC_PARTS[case.w]:
                _, special, events = case.seg_model(j, p)
                if any(special) or any(p <= case.lens[j] or k != "identity" for _, _, k in events):
                    bad.append("%s: random, but special at parts %d: %s %s" % (what, p, special, events))
            continue
        claims = seg.claim if isinstance(seg.claim, list) else [seg.claim] if seg.claim else []
        for c in claims:
            _, special, events = case.seg_model(j, c["parts"])
            if "special" in c and {g for g, sp in enumerate(special) if sp} != c["special"]:
                bad.append("%s: special parts %s at parts %d, claimed %s" % (what, special, c["parts"], c["special"]))
            if "merge" in c and not any((r, k) == c["merge"] for r, _, k in events):
                bad.append("%s: merge events %s at parts %d, claimed %s" % (what, events, c["parts"], c["merge"]))
    return bad


def _rec_scalar(w, nbits, rnd, unit):
    return 1 if unit else rand_scalar(_full(w, nbits), w, nbits, rnd)


def rec_random_seg(w, n, nbits, rnd, unit=False, tag="random"):
    """A random segment that the model shows to meet nothing (check_rec_claims' rule)."""
    for _ in range(50):
        seg = Job(rnd.sample(pool(w), n), [_rec_scalar(w, nbits, rnd, unit) for _ in range(n)], tag)
        seg.random = True
        if not check_rec_claims(RecCase(w, nbits, [seg], "probe")):
            return seg
    raise AssertionError("no random segment without a special case")


def rec_directed(w, nbits, rnd, unit=False):
    """The directed segments of the ragged forms: short ones, where parts > len leaves empty parts beside the special case."""
    full, most = _full(w, nbits), MAX_PARTS[w]
    last = most.bit_length() - 2  # the last round of the tree at the largest split
    segs = []

    def base(n, tag, claim=None, **kw):
        s = rec_random_seg(w, n, nbits, rnd, unit, tag)
        s.random, s.claim = False, claim
        s.__dict__.update(kw)
        segs.append(s)
        return s

    # two adjacent records with the same point and scalar: P = Q at the top column in one part, `equal` in the tree in two
    s = base(2, "equal neighbours", [{"parts": 1, "special": {0}}, {"parts": 2, "special": set(), "merge": (0, "equal")},
                                     {"parts": most, "special": set(), "merge": (last, "equal")}])
    s.a[1], s.k[1] = s.a[0], s.k[0]
    s = base(5, "equal neighbours at the start of 5", [{"parts": 1, "special": {0}}, {"parts": 2, "special": {0}}, {"parts": 8, "merge": (0, "identity")}])
    s.a[1], s.k[1] = s.a[0], s.k[0]
    # a record and its negative: the whole segment is the identity / the accumulator comes back to the identity in mid-ladder
    s = base(2, "P and -P", [{"parts": 1, "special": {0}}, {"parts": 2, "special": set(), "merge": (0, "opposite")},
                             {"parts": 4, "special": set(), "merge": (1, "opposite")}, {"parts": most, "special": set(), "merge": (last, "opposite")}])
    s.a[1], s.k[1] = neg_mult(w, s.a[0]), s.k[0]
    s = base(3, "P, -P, Q", [{"parts": 1, "special": {0}}, {"parts": 2, "special": set()}])
    s.a[1], s.k[1] = neg_mult(w, s.a[0]), s.k[0]
    # the identity as a record: alone, first of a part, in mid-part
    s = base(1, "identity alone", [{"parts": 1, "special": {0}}, {"parts": most, "special": {most - 1}, "merge": (0, "identity")}])
    s.a[0] = 0
    s = base(9, "identity first, and first of part 2/4", [{"parts": 1, "special": {0}}, {"parts": 4, "special": {0, 2}}])
    s.a[0] = s.a[4] = 0
    s = base(5, "identity in mid-part", [{"parts": 1, "special": {0}}, {"parts": 2, "special": {0}}, {"parts": 16, "special": {6}}])
    s.a[1] = 0
    # halves that cancel: the last round of the tree meets `opposite` at 2, 4 and 8 parts
    s = base(8, "opposite halves", [{"parts": p, "merge": (p.bit_length() - 2, "opposite")} for p in (2, 4, 8)])
    for i in range(4):
        s.a[4 + i], s.k[4 + i] = neg_mult(w, s.a[i]), s.k[i]
    # failures: the neighbours must stay exact
    s = base(5, "undecodable first record")
    s.a[0] = None
    s = base(5, "undecodable last record")
    s.a[4] = None
    base(3, "status not OK on entry", status_in=NOT_ENOUGH)
    if not unit:
        s = base(3, "scalar = r")
        s.k[1] = R
        if not full:
            s = base(3, "even scalar")
            s.k[2] -= 1
            s = base(2, "scalar that is not short")
            s.k[0] = (1 + (1 << nbits) * X) if w == 2 else 1 + (1 << nbits) * X2
    return segs


def rec_lay_out(w, nbits, rnd, head, directed, J, unit=False, make=None, failing=None):
    """lay_out for segments: random ones of the lengths `head`, then three directed ones and a short random one, to J.
    make(n, tag): a random segment, failing(s): a directed segment fails -- the paired form brings its own."""
    make = make or (lambda n, tag: rec_random_seg(w, n, nbits, rnd, unit, tag))
    failing = failing or (lambda s: s.status_in != OK or not MsmCase(w, len(s.a), 1, nbits, [s], [1]).valid(s))
    segs = [make(n, "random len %d" % n) for n in head]
    # a failing segment goes between two that are OK: both neighbours must stay exact
    fails = [s for s in directed if failing(s)]
    good = [s for s in directed if not any(s is f for f in fails)]
    d, fill = [], 0
    while good or fails:
        d += good[:1] + fails[:1]
        good, fails = good[1:], fails[1:]
    while len(segs) < J:
        for _ in range(3):
            if d and len(segs) < J:
                segs.append(d.pop(0))
        if len(segs) < J:
            fill += 1
            segs.append(make(1 + (fill % 3 == 0), "random filler"))
    return segs, d


def rec_small_segs(w, kind, nbits, rnd):
    """The segments of the small kinds (rec_case): fail first, no segment, all empty, one record."""
    if kind == "fail first":
        bad = rec_random_seg(w, 3, nbits, rnd, tag="undecodable first record of the launch")
        bad.random, bad.a[0] = False, None
        kept = rec_random_seg(w, 2, nbits, rnd, tag="status not OK on entry")
        kept.random, kept.status_in = False, NOT_ENOUGH
        return [rec_random_seg(w, n, nbits, rnd) if n is not None else s for n, s in
                ((0, None), (None, bad), (0, None), (5, None), (0, None), (2, None), (None, kept), (1, None), (0, None))]
    if kind == "no segment":
        return []
    if kind == "all empty":
        return [rec_random_seg(w, 0, nbits, rnd) for _ in range(5)]
    assert kind == "one record"
    return [rec_random_seg(w, 1, nbits, rnd)]


_REC = {}
REC_TABLES = [(1, "short"), (2, "short"), (2, "unit"), (1, "full"), (2, "full"), (1, "fail first"), (2, "fail first"), (1, "no segment"),
              (2, "no segment"), (1, "all empty"), (2, "all empty"), (1, "one record"), (2, "one record")]


def rec_case(w, kind):
    """short: the shipped mode, J = 70 (more than one wave of segments at parts = 1, a ragged last wave), the directed jobs of
    the fixed-n suite at n = 8 (their claims hold as they are: rec_part cuts as msm_part does) and rec_directed.  unit: every
    scalar 1 (the second-level launch over piece sums).  full: a small table at full width.  fail first: the first segment with
    records fails in stage T, between empty ones -- place 0 of the launch, on which empty parts fall back, is a failed segment's."""
    key = (w, kind)
    if key in _REC:
        return _REC[key]
    rnd = random.Random("manypoint-rec-%d-%s" % key)
    nbits = REC_FULL[w] if kind == "full" else REC_NBITS[w]
    tag = "rec G%d %s nbits=%d" % (w, kind, nbits)
    left = []
    if kind == "short":
        keep = ("merge", "equal shares", "identity in the middle", "largest short digits", "digit with bit", "k1 with bit")
        fixed = [j for j in directed_jobs(w, 8, nbits, rnd) if j.tag.startswith(keep)]  # (the rest has a shorter twin in rec_directed)
        segs, left = rec_lay_out(w, nbits, rnd, REC_HEAD, rec_directed(w, nbits, rnd) + fixed, REC_J)
    elif kind == "unit":
        segs, left = rec_lay_out(w, nbits, rnd, REC_HEAD, rec_directed(w, nbits, rnd, True), REC_J, True)
    elif kind == "full":
        segs, left = rec_lay_out(w, nbits, rnd, [0, 1, 33, 2, 9, 5, 3, 8], rec_directed(w, nbits, rnd), 27)
    else:
        segs = rec_small_segs(w, kind, nbits, rnd)
    case = RecCase(w, nbits, segs, tag)
    case.left_out = [s.tag for s in left]
    _REC[key] = case
    return case


def run_rec(lib, case, parts):
    """(out (J + 1 rows), status, tbl, codes (both with one guard chunk), first_chunk) as the leg left them."""
    w, J = case.w, case.J
    pts = np.frombuffer(b"".join(BAD_POINT[w] if a is None else enc(w, gmul(w, a)) for s in case.segs for a in s.a) + b"\0", dtype=np.uint8).copy()
    sc = np.array([dc.u32s(k) for s in case.segs for k in s.k] + [[0] * 8], dtype=np.uint32).reshape(-1)
    st_in = np.array([s.status_in for s in case.segs] + [0], dtype=np.uint8)
    seg_first = np.array(case.seg_first, dtype=np.uint64)
    out = np.full((J + 1) * PT_BYTES[w], POISON, dtype=np.uint8)
    status = np.full(J + 1, POISON, dtype=np.uint8)
    tbl = np.full((case.chunks + 1) * 4 * 8 * ENTRY[w], POISON_WORD, dtype=np.int32)
    codes = np.full((case.chunks + 1) * 4 * COLS, POISON, dtype=np.uint8)
    fc = np.full(J + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rc = lib["rec"](w, J, _ptr(seg_first), _ptr(pts), _ptr(sc), _ptr(st_in), case.nbits, parts, _ptr(out), _ptr(status), _ptr(tbl), _ptr(codes), _ptr(fc))
    if rc != 0:
        raise HipError("%s parts=%d: the harness returned %d" % (case.tag, parts, rc))
    return out.reshape(J + 1, -1), status, tbl, codes, fc


def check_rec(case, parts, res, max_report=12):
    """Every check of the ragged sums on one run; returns the list of failures."""
    out, status, tbl, codes, fc = res
    w, J, ew = case.w, case.J, ENTRY[case.w]
    want_st, want_out = case.ref()
    what0 = "%s parts=%d" % (case.tag, parts)
    bad = []
    if fc.tolist() != case.first_chunk:
        bad.append("%s: first_chunk %s, expected %s" % (what0, fc.tolist(), case.first_chunk))
    if bytes(out[J]) != bytes([POISON]) * PT_BYTES[w] or status[J] != POISON:
        bad.append("%s: output or status written behind the last segment" % what0)
    used_t, used_c = case.chunks * 4 * 8 * ew, case.chunks * 4 * COLS
    if not (tbl[used_t:] == POISON_WORD).all() or not (codes[used_c:] == POISON).all():
        bad.append("%s: the guard chunk behind the tables or the codes written" % what0)
    if case.chunks == 0 and (not (tbl == POISON_WORD).all() or not (codes == POISON).all()):
        bad.append("%s: a launch without records wrote tables or codes" % what0)
    for j, seg in enumerate(case.segs):
        if len(bad) > max_report:
            break
        what = "%s segment %d (%s, len %d)" % (what0, j, seg.tag, case.lens[j])
        if status[j] != want_st[j]:
            bad.append("%s: status %d, expected %d" % (what, status[j], want_st[j]))
        if bytes(out[j]) != want_out[j]:
            bad.append("%s: wrong output bytes" % what)
    check_rec_places(case, what0, tbl, codes, bad, max_report)
    return bad


def check_rec_places(case, what0, tbl, codes, bad, max_report=12):
    """The tables and digit codes of every segment of `case` in tbl / codes, which start at the segments' chunk 0 (the paired
    form hands in one half at a time)."""
    w, ew = case.w, ENTRY[case.w]
    for j, seg in enumerate(case.segs):
        if len(bad) > max_report:
            break
        n = case.lens[j]
        what = "%s segment %d (%s, len %d)" % (what0, j, seg.tag, n)
        if not n:
            continue
        p0, s4 = case.first_chunk[j] * 4, 4 * ((n + 3) // 4)
        assert s4 == case.one[j].shares4
        t = tbl[p0 * 8 * ew:(p0 + s4) * 8 * ew].reshape(s4, 8, ew)
        c = codes[p0 * COLS:(p0 + s4) * COLS].reshape(COLS, s4)  # (the column stride is this segment's)
        if not (c[case.top + 1:] == POISON).all():
            bad.append("%s: codes written past column %d" % (what, case.top))
        if not case.valid(j):
            continue  # (a failed segment's tables and codes are read by nobody: only where it wrote matters, and the
            #            neighbours' exact contents and the fill above show that)
        mcodes, flips, _ = case.one[j].share_codes(seg)
        got = c[:case.top + 1, :].T.tolist()
        if got != mcodes:
            s = next(s for s in range(s4) if got[s] != mcodes[s])
            bad.append("%s: codes of place %d: %s, expected %s" % (what, s, got[s], mcodes[s]))
        for s in range(s4):
            want = entry_points(w, seg.a[s] if s < n else 0, flips[s] and s < n)
            for m in range(8):
                check_entry(w, t[s, m], want[m], "%s place %d entry %d" % (what, s, m), bad)


# ---- the PAIRED ragged sums (k_rec_tables_g1_pair / k_rec_ladder_g1_pair; tc_records.h rec_pair_*) ----
# Segment j is summed over points_a and over points_b with the SAME scalars; out[2 j] = A_j, out[2 j + 1] = -B_j.  A pair is two
# segments (Jobs) that share k and status_in: half 0 over a, half 1 over b.  Each half of a launch is a RecCase of its own --
# the models, the claims and the table checker are the unpaired ones, run once per half.
PAIR_NBITS = 32  # tc_verify_decryption_share_records_rlc_batch ships G1 short scalars of 32 bits
PAIR_TABLES = ["short", "full", "fail first", "no segment", "all empty", "one record"]
# where the special case of a directed segment of rec_directed goes (the other half is a random sample of the pool)
PAIR_SIDE = {"equal neighbours": 0, "equal neighbours at the start of 5": 1, "P and -P": 1, "P, -P, Q": 0, "identity alone": 1,
             "identity first, and first of part 2/4": 0, "identity in mid-part": 1, "opposite halves": 0, "undecodable first record": 0,
             "undecodable last record": 1, "status not OK on entry": 0, "scalar = r": 0, "even scalar": 1, "scalar that is not short": 0}
PAIR_SECOND = {"P and -P": 0, "undecodable first record": 2}  # from a second draw of rec_directed; 2: both halves


class Pair:
    def __init__(self, a, b, tag, random):
        assert a.k == b.k and a.status_in == b.status_in
        self.half, self.tag, self.random, self.status_in = (a, b), tag, random, a.status_in


def pair_partner(seg, nbits, rnd):
    """The other half of `seg`: other points of the pool under seg's scalars, shown by the model to meet nothing."""
    for _ in range(50):
        p = Job(rnd.sample(pool(1), len(seg.a)), list(seg.k), "partner of " + seg.tag, status_in=seg.status_in)
        p.random = True
        if not check_rec_claims(RecCase(1, nbits, [p], "probe")):
            return p
    raise AssertionError("no partner without a special case")


def pair_random(n, nbits, rnd, tag="random"):
    a = rec_random_seg(1, n, nbits, rnd, tag=tag)
    return Pair(a, pair_partner(a, nbits, rnd), tag, True)


def pair_directed(nbits, rnd):
    """rec_directed with the special case in ONE half (PAIR_SIDE), then a second draw for the other side of two of them."""
    pairs = []
    for table, draw in ((PAIR_SIDE, rec_directed(1, nbits, rnd)), (PAIR_SECOND, rec_directed(1, nbits, rnd))):
        for d in draw:
            if d.tag not in table:
                continue
            side, p = table[d.tag], pair_partner(d, nbits, rnd)
            if side == 2:  # the same record undecodable in both halves
                p.a[d.a.index(None)] = None
            tag = "%s in %s" % (d.tag, ("a", "b", "both")[side])
            pairs.append(Pair(p, d, tag, False) if side == 1 else Pair(d, p, tag, False))
    return pairs


class PairCase:
    def __init__(self, nbits, pairs, tag):
        self.nbits, self.pairs, self.tag, self.J = nbits, pairs, tag, len(pairs)
        self.half = [RecCase(1, nbits, [p.half[h] for p in pairs], "%s half %d" % (tag, h)) for h in (0, 1)]
        self.parts = self.half[0].parts
        self.first_chunk, self.chunks, self.lens = self.half[0].first_chunk, self.half[0].chunks, self.half[0].lens
        self.left_out = []
        self._ref = None

    def failing(self, j):
        return self.pairs[j].status_in != OK or not (self.half[0].valid(j) and self.half[1].valid(j))

    def ref(self):
        """Expected status per segment and output bytes per ROW (2 J rows), once: [sum a_i k_i] G, then -[sum b_i k_i] G."""
        if self._ref is None:
            st, out = [], []
            for j, p in enumerate(self.pairs):
                st.append(p.status_in if p.status_in != OK or self.chunks == 0 else INVALID if self.failing(j) else OK)
                for h in (0, 1):
                    m = sum(a * k for a, k in zip(p.half[h].a, p.half[h].k)) % R if not self.failing(j) else 0
                    out.append(bytes([POISON]) * 96 if self.chunks == 0 else enc(1, gmul(1, neg_mult(1, m) if h else m)))
            self._ref = (st, out)
        return self._ref


_PAIR = {}


def pair_case(kind):
    """The kinds of rec_case at w = 1 with an independent b array.  short: nbits = 32, J = 70; full: nbits = 128, J = 27."""
    if kind in _PAIR:
        return _PAIR[kind]
    rnd = random.Random("manypoint-pair-%s" % kind)
    nbits = REC_FULL[1] if kind == "full" else PAIR_NBITS
    left = []
    if kind in ("short", "full"):
        head, J = (REC_HEAD, REC_J) if kind == "short" else ([0, 1, 33, 2, 9, 5, 3, 8], 27)
        probe = lambda p: PairCase(nbits, [p], "probe").failing(0)  # noqa: E731
        pairs, left = rec_lay_out(1, nbits, rnd, head, pair_directed(nbits, rnd), J, make=lambda n, tag: pair_random(n, nbits, rnd, tag), failing=probe)
    else:
        pairs = []
        for s in rec_small_segs(1, kind, nbits, rnd):
            pairs.append(Pair(s, pair_partner(s, nbits, rnd), s.tag + ("" if s.random else " in a"), s.random))
    case = PairCase(nbits, pairs, "pair %s nbits=%d" % (kind, nbits))
    case.left_out = [p.tag for p in left]
    _PAIR[kind] = case
    return case


def check_pair_claims(case):
    """check_rec_claims on both halves: the half that holds a directed segment confirms its claims, every random half -- the
    partner of a directed one too -- meets nothing."""
    return check_rec_claims(case.half[0]) + check_rec_claims(case.half[1])


def run_rec_pair(lib, case, parts):
    """(out (2 J + 2 rows), status (J + 1), tbl, codes (2 chunks + 1 chunks each), first_chunk) as the leg left them."""
    J = case.J
    pts = [np.frombuffer(b"".join(BAD_POINT[1] if a is None else enc(1, gmul(1, a)) for p in case.pairs for a in p.half[h].a) + b"\0",
                         dtype=np.uint8).copy() for h in (0, 1)]
    sc = np.array([dc.u32s(k) for p in case.pairs for k in p.half[0].k] + [[0] * 8], dtype=np.uint32).reshape(-1)
    st_in = np.array([p.status_in for p in case.pairs] + [0], dtype=np.uint8)
    seg_first = np.array(case.half[0].seg_first, dtype=np.uint64)
    out = np.full((2 * J + 2) * 96, POISON, dtype=np.uint8)
    status = np.full(J + 1, POISON, dtype=np.uint8)
    tbl = np.full((2 * case.chunks + 1) * 4 * 8 * ENTRY[1], POISON_WORD, dtype=np.int32)
    codes = np.full((2 * case.chunks + 1) * 4 * COLS, POISON, dtype=np.uint8)
    fc = np.full(J + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rc = lib["rec_pair"](J, _ptr(seg_first), _ptr(pts[0]), _ptr(pts[1]), _ptr(sc), _ptr(st_in), case.nbits, parts, _ptr(out), _ptr(status), _ptr(tbl),
                         _ptr(codes), _ptr(fc))
    if rc != 0:
        raise HipError("%s parts=%d: the harness returned %d" % (case.tag, parts, rc))
    return out.reshape(2 * J + 2, 96), status, tbl, codes, fc


def check_rec_pair(case, parts, res, max_report=12):
    """Every check of the paired sums on one run; returns the list of failures."""
    out, status, tbl, codes, fc = res
    J, C, ew = case.J, case.chunks, ENTRY[1]
    want_st, want_out = case.ref()
    what0 = "%s parts=%d" % (case.tag, parts)
    bad = []
    if fc.tolist() != case.first_chunk:
        bad.append("%s: first_chunk %s, expected %s" % (what0, fc.tolist(), case.first_chunk))
    if bytes(out[2 * J:].reshape(-1)) != bytes([POISON]) * 192 or status[J] != POISON:
        bad.append("%s: output or status written behind the last segment" % what0)
    if not (tbl[2 * C * 4 * 8 * ew:] == POISON_WORD).all() or not (codes[2 * C * 4 * COLS:] == POISON).all():
        bad.append("%s: the guard chunk behind half 1's tables or codes written" % what0)
    if C == 0 and (not (tbl == POISON_WORD).all() or not (codes == POISON).all()):
        bad.append("%s: a launch without records wrote tables or codes" % what0)
    for j, p in enumerate(case.pairs):
        what = "%s segment %d (%s, len %d)" % (what0, j, p.tag, case.lens[j])
        if status[j] != want_st[j]:
            bad.append("%s: status %d, expected %d" % (what, status[j], want_st[j]))
        for h in (0, 1):
            if bytes(out[2 * j + h]) != want_out[2 * j + h]:
                bad.append("%s: wrong output bytes in half %d" % (what, h))
        if len(bad) > max_report:
            return bad
    for h in (0, 1):  # half h's tables and codes: the layout of an unpaired launch, at chunk offset h * chunks
        check_rec_places(case.half[h], "%s half %d" % (what0, h), tbl[h * C * 4 * 8 * ew:(h + 1) * C * 4 * 8 * ew], codes[h * C * 4 * COLS:(h + 1) * C * 4 * COLS],
                         bad, max_report)
    for j in range(J):  # the same scalars: the same codes
        if case.half[0].valid(j) and case.half[1].valid(j):
            c0, c1 = (case.first_chunk[j] * 4 * COLS, case.first_chunk[j + 1] * 4 * COLS)
            if not (codes[c0:c1] == codes[C * 4 * COLS + c0:C * 4 * COLS + c1]).all():
                bad.append("%s segment %d: the codes of half 1 differ from half 0's" % (what0, j))
    return bad


# ---- k_rec_gather_keys ----
GATHER_K, GATHER_R = 5, 71  # 6 lanes per record: 426 lanes, no multiple of a workgroup


def gather_case():
    idx = [0, GATHER_K - 1, GATHER_K, 1 << 32, (1 << 64) - 1, 1, 2, 3]
    idx = [idx[(r + r // 8) % len(idx)] for r in range(GATHER_R)]
    pks = [enc(1, gmul(1, a)) for a in pool(1)[:GATHER_K]]
    want = b"".join(pks[i] if i < GATHER_K else b"\xff" * 96 for i in idx) + bytes([POISON]) * 96
    return pks, idx, want


def run_gather(lib):
    """The bytes the leg left in keys (R rows and the guard row), and the expected ones."""
    pks, idx, want = gather_case()
    pk = np.frombuffer(b"".join(pks), dtype=np.uint8).copy()
    ix = np.array(idx, dtype=np.uint64)
    keys = np.full(GATHER_R * 96 + 96, POISON, dtype=np.uint8)
    rc = lib["gather"](_ptr(pk), GATHER_K, _ptr(ix), GATHER_R, _ptr(keys))
    if rc != 0:
        raise HipError("gather keys: the harness returned %d" % rc)
    return bytes(keys), want


# ---- blame by bisection (k_blame.hip / tc_blame_jobs.h): the leaves, the leaf ladders at chosen digits, the range sums ----
# The leaves never leave the device and the two sums of a bisection step are built from the same (job, lo, hi), so an error common
# to both -- a term dropped by the partition of a range, a lane whose masked trips disturb its accumulator -- cancels in the
# pairing check that consumes them.  Here every leaf is decoded from its raw words and every sum is compared byte for byte.
# A leaf is a Jacobian point in limb form: rows of 16 words, X, Y, Z in G1; X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1 in G2.
BLAME_KEY = bytes((3 * i + 1) & 0xff for i in range(32))
LEAF_ROWS = {1: 3, 2: 6}   # kBlameLeafWordsG1 / G2 = 16 words per row
WAVE_LEAVES = {1: 64, 2: 32}  # leaves per wave: one lane / one lane pair each
BLAME_PARTS = {w: [0] + REC_PARTS[w] + REC_ILLEGAL[w] for w in (1, 2)}  # 0: blame_sum_parts' choice (the device leg only)
BLAME_F, BLAME_N = 4, 130
BLAME_HEAD = [1, 2, 3, 4, 5, 6, 7, 8, 9, 33, 64, 65, 130]


def build_device_blame():
    """tests/device/manypoint_blame.hip -> a gfx950 shared object, by the recipe of build_device."""
    from threshold_crypto_amd import build as tcb
    src = os.path.join(DEV, "manypoint_blame.hip")
    return dc._build("libtc_manypoint_blame", lambda out: [dc.hipcc()] + tcb.FLAGS + ["-w", "-shared", src, "-o", out], {"manypoint_blame.hip"})


def load_blame(path, prefix):
    """prefix "mp_": tests/device/manypoint_blame.hip; "mph_": the host leg (build_host).  The same arguments in both."""
    lib = ctypes.CDLL(path)
    u64 = ctypes.c_uint64
    sig = {"leaves": [_INT, _VP, u64, u64, _VP, _SZ, _SZ, _VP, _SZ, _VP, _VP, _VP],
           "range_sum": [_INT, _VP, _SZ, _SZ, _VP, _VP, _VP, _SZ, _SZ, _VP],
           "chain": [_INT, _VP, u64, u64, _VP, _SZ, _SZ, _VP, _SZ, _VP, _VP, _SZ, _SZ, _VP, _VP, _VP],
           "ladder": [_INT, _VP, _VP, _VP, _SZ, _VP]}
    entries = {}
    for name, args in sig.items():
        entries[name] = getattr(lib, prefix + "blame_" + name)
        entries[name].argtypes, entries[name].restype = args, _INT
    sizes = [getattr(lib, prefix + "blame_leaf_bytes")]
    sizes[0].argtypes = [_INT]
    if prefix == "mp_":  # (blame_sum_parts is a host function of k_blame.hip: the device harness only)
        sizes.append(lib.mp_blame_sum_parts)
        sizes[1].argtypes = [_INT, _SZ, _SZ, _INT]
        entries["sum_parts"] = sizes[1]
    for f in sizes:
        f.restype = _SZ
    assert [sizes[0](g2) for g2 in (0, 1)] == [LEAF_ROWS[1] * 64, LEAF_ROWS[2] * 64]
    return dict(entries, lib=lib, host=prefix == "mph_")


def blame_call_seed(key, call):
    """blame_call_seed: the first 32 bytes of the oracle's ChaCha20 block `call` under the context's key."""
    return struct.pack("<8I", *o.chacha20_block(struct.unpack("<8I", key), call)[:8])


def digits_scalar(d):
    return d[0] + d[1] * X + d[2] * X ** 2 + d[3] * X ** 3


def blame_scalar(seed, leaf):
    """blame_digits: (the four 16-bit digits of leaf number `leaf`, d0 odd; the scalar they stand for)."""
    w0, w1 = o.chacha20_block(struct.unpack("<8I", seed), leaf)[:2]
    d = [(w0 & 0xffff) | 1, w0 >> 16, w1 & 0xffff, w1 >> 16]
    return d, digits_scalar(d)


def _flat(w, v):
    return [v] if w == 1 else list(v)


def identity_leaf(w):
    """Jac::infinity() = (0, 1, 0) as blame_store_leaf writes it: zero rows, and the plain digits of the Montgomery one."""
    one = dc.encode(1).limbs + [0, 0]
    rows = [[0] * 16 for _ in range(LEAF_ROWS[w])]
    rows[w] = one  # Y (G2: Y.c0)
    return [x for r in rows for x in r]


def leaf_words(w, m, rnd):
    """[m] G as a leaf with a random Z: (x z^2, y z^3, z), every coordinate the plain digits of its Montgomery form or of that
    plus p -- the two representatives blame_store_fq's product below 2.1 p can have."""
    if m % R == 0:
        return identity_leaf(w)
    F, pt = E[w].F, gmul(w, m)
    z = rnd.randrange(1, P) if w == 1 else (rnd.randrange(P), rnd.randrange(1, P))
    z2 = F.sqr(z)
    coords = _flat(w, F.mul(pt[0], z2)) + _flat(w, F.mul(pt[1], F.mul(z2, z))) + _flat(w, z)
    return [x for v in coords for x in dc.encode(v, k=rnd.randrange(2)).limbs + [0, 0]]


def leaf_point(w, row, what, bad):
    """One stored leaf (48 / 96 words) -> the affine point X / Z^2, Y / Z^3 (None: Z = 0), with the representation checks: every
    limb inside [NORM_LO, NORM_HI] 2^28, |value| <= 2.1 p, words 14 and 15 of every row 0, c0 / c1 in rows 2 c / 2 c + 1."""
    row = [int(x) for x in row]
    for c in range(LEAF_ROWS[w]):
        if row[16 * c + 14] or row[16 * c + 15]:
            bad.append("%s: words 14, 15 of row %d: %s" % (what, c, row[16 * c + 14:16 * c + 16]))
    cs = [coord(row[16 * c:16 * c + 16], "%s row %d" % (what, c), bad) for c in range(LEAF_ROWS[w])]
    return E[w]._to_affine(tuple(cs) if w == 1 else ((cs[0], cs[1]), (cs[2], cs[3]), (cs[4], cs[5])))


def check_leaf_rows(w, rows, want, what0, bad, max_report=12):
    """rows: len(want) leaves and a guard row; want: the affine points (None: the identity, Z = 0)."""
    if not (rows[len(want)] == POISON_WORD).all():
        bad.append("%s: the guard row behind the leaves written" % what0)
    for i, pt in enumerate(want):
        if len(bad) > max_report:
            break
        what = "%s leaf %d" % (what0, i)
        if (rows[i] == POISON_WORD).all():
            bad.append("%s: not written" % what)
            continue
        got = leaf_point(w, rows[i], what, bad)
        if got != pt:
            bad.append("%s: %s" % (what, "Z != 0 in a dead slot" if pt is None else "Z = 0" if got is None else "wrong point"))
        if pt is None and [int(x) for x in rows[i]] != identity_leaf(w):
            bad.append("%s: the identity is not stored as (0, 1, 0)" % what)


class LeavesCase:
    """k_blame_leaves over n leaves: a[q]: the multiple of point q (0: the identity's encoding, None: BAD_POINT), live: n bytes or
    None.  Identity encodings, slots that are not live and undecodable points stand first, last and in the middle of the waves (G2:
    on both of a wave's last lane pairs), each kind in each place over the waves of n = 130."""
    KINDS = ("identity", "not live", "bad")

    def __init__(self, w, n, leaf0, period, with_live, call):
        self.w, self.n, self.leaf0, self.period, self.call = w, n, leaf0, period, call
        self.tag = "blame leaves w=%d n=%d leaf0=%d period=%d%s" % (w, n, leaf0, period, "" if with_live else " no live")
        rnd = random.Random("manypoint-" + self.tag)
        W = WAVE_LEAVES[w]
        self.a = [rnd.choice(pool(w)) for _ in range(period or n)]
        self.live = [1] * n if with_live else None
        if n > 4:
            for v in range(-(-n // W)):
                size = min(W, n - v * W)
                places = {0: v % 3, size - 1: (v + 1) % 3}
                if size > 16:
                    places.update({size // 2 - 3 + 3 * j: (v + 2 + j) % 3 for j in range(3)})
                    if w == 2:
                        places[size - 2] = (v + 2) % 3
                for p, kind in places.items():
                    self._place(v * W + p, self.KINDS[kind])
        if with_live and n > 40:
            self.live[20], self.live[21] = 0, 0xff     # (any non-zero byte marks a live slot)
            if not period:
                self.a[20] = None                    # not live AND undecodable: the byte stays as it is
        self._ref = None

    def _place(self, r, kind):
        q = r % self.period if self.period else r
        if kind == "not live" and self.live is not None:
            self.live[r] = 0
        else:
            self.a[q] = None if kind == "bad" else 0

    def kind(self, r):
        a = self.a[r % self.period if self.period else r]
        return "not live" if self.live is not None and not self.live[r] else "bad" if a is None else "identity" if a == 0 else "point"

    def points(self):
        return b"".join(BAD_POINT[self.w] if a is None else enc(self.w, gmul(self.w, a)) for a in self.a)

    def ref(self):
        """(seed, the multiple of every leaf, its affine point, the live bytes afterwards with the guard byte or None), once."""
        if self._ref is None:
            seed = blame_call_seed(BLAME_KEY, self.call)
            live_out = None if self.live is None else list(self.live) + [POISON]
            mults = []
            for r in range(self.n):
                a = self.a[r % self.period if self.period else r]
                marked = self.live is None or self.live[r] != 0
                if marked and a is None and live_out is not None:
                    live_out[r] = 0
                mults.append(a * blame_scalar(seed, self.leaf0 + r)[1] % R if marked and a is not None else 0)
            self._ref = (seed, mults, [gmul(self.w, m) for m in mults], live_out)
        return self._ref


LEAVES_SHAPES = [(1, 0, 0, True), (33, (1 << 32) - 3, 0, True), (64, 0, 0, True), (65, (1 << 32) - 3, 0, True), (130, (1 << 32) - 3, 0, True),
                 (130, 0, 52, False), (130, 7 * 52, 52, True)]  # n, leaf0, period, with live; 130 = two and a half rows of 52
LEAVES_CALLS = [0, 1, (1 << 40) + 3]
_LEAVES = {}


def leaves_case(w, n, leaf0, period, with_live):
    key = (w, n, leaf0, period, with_live)
    if key not in _LEAVES:
        _LEAVES[key] = LeavesCase(w, n, leaf0, period, with_live, LEAVES_CALLS[LEAVES_SHAPES.index(key[1:]) % 3])
    return _LEAVES[key]


def _leaves_in(case):
    pts = np.frombuffer(case.points(), dtype=np.uint8).copy()
    live_in = None if case.live is None else np.array(case.live + [POISON], dtype=np.uint8)
    key = np.frombuffer(BLAME_KEY, dtype=np.uint8).copy()
    return pts, live_in, key, np.full(32, POISON, dtype=np.uint8), np.full(case.n + 1, POISON, dtype=np.uint8)


def run_blame_leaves(lib, case):
    """(seed, leaves (n rows and the guard row), live (n bytes and the guard byte; all 0x5A without a live array)) as the leg left them."""
    w, n = case.w, case.n
    pts, live_in, key, seed, live_out = _leaves_in(case)
    leaves = np.full((n + 1) * LEAF_ROWS[w] * 16, POISON_WORD, dtype=np.int32)
    rc = lib["leaves"](w - 1, _ptr(key), case.call, case.leaf0, _ptr(pts), len(case.a), case.period, _ptr(live_in) if live_in is not None else None, n,
                       _ptr(seed), _ptr(leaves), _ptr(live_out))
    if rc != 0:
        raise HipError("%s: the harness returned %d" % (case.tag, rc))
    return seed, leaves.reshape(n + 1, -1), live_out


def check_blame_leaves(case, res, max_report=12):
    seed, leaves, live = res
    want_seed, _, want, want_live = case.ref()
    bad = []
    if bytes(seed) != want_seed:
        bad.append("%s: the seed is not the oracle's ChaCha20 block %d" % (case.tag, case.call))
    if live.tolist() != (want_live if want_live is not None else [POISON] * (case.n + 1)):
        diff = [i for i, (a, b) in enumerate(zip(live.tolist(), want_live or [POISON] * (case.n + 1))) if a != b]
        bad.append("%s: live bytes (guard byte: index %d) differ at %s" % (case.tag, case.n, diff[:8]))
    check_leaf_rows(case.w, leaves, want, case.tag, bad, max_report)
    return bad


# -- the leaf ladders at chosen digits --
LADDER_DIGITS = [(1, 0, 0, 0), (0xffff, 0xffff, 0xffff, 0xffff), (1, 0xffff, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1), (0xffff, 0, 0xfffe, 0), (3, 1, 2, 0xffff)]
LADDER_RANDOM = 48


class LadderCase:
    """blame_leaf_g1 / blame_leaf_g2 + blame_store_leaf over rows of (multiple of the point, live, four digits): every directed
    digit row with a random point, with the identity and with live = false, and random rows with d0 odd.  The directed rows stand
    at lane (pair) 0 and at the last one of the full waves, at lane 0 of the ragged wave and around the middle; the rows of a wave
    all differ."""

    def __init__(self, w):
        self.w, self.tag = w, "blame ladder w=%d" % w
        rnd = random.Random("manypoint-" + self.tag)
        W = WAVE_LEAVES[w]
        directed = [(a, live, d) for d in LADDER_DIGITS for a, live in ((rnd.choice(pool(w)), 1), (0, 1), (rnd.choice(pool(w)), 0))]
        T = len(directed) + LADDER_RANDOM
        full = T // W
        spots = [v * W + p for v in range(full) for p in (0, W - 1)] + [full * W]
        mids = [v * W + p for p in sorted(range(1, W - 1), key=lambda i: abs(i - W // 2)) for v in range(full)]
        self.spots = spots + mids[:len(directed) - len(spots)]
        rows = [(rnd.choice(pool(w)), 1, (rnd.randrange(1 << 16) | 1,) + tuple(rnd.randrange(1 << 16) for _ in range(3))) for _ in range(T)]
        for s, row in zip(self.spots, directed):
            rows[s] = row
        self.rows, self.T = rows, T
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = [gmul(self.w, a * digits_scalar(d) % R) if live else None for a, live, d in self.rows]
        return self._ref


_LADDER = {}


def ladder_case(w):
    if w not in _LADDER:
        _LADDER[w] = LadderCase(w)
    return _LADDER[w]


def run_blame_ladder(lib, case):
    w, T = case.w, case.T
    pts = np.frombuffer(b"".join(enc(w, gmul(w, a)) for a, _, _ in case.rows), dtype=np.uint8).copy()
    live = np.array([l for _, l, _ in case.rows], dtype=np.uint8)
    digits = np.array([d for _, _, d in case.rows], dtype=np.uint64).reshape(-1)
    leaves = np.full((T + 1) * LEAF_ROWS[w] * 16, POISON_WORD, dtype=np.int32)
    rc = lib["ladder"](w - 1, _ptr(pts), _ptr(live), _ptr(digits), T, _ptr(leaves))
    if rc != 0:
        raise HipError("%s: the harness returned %d" % (case.tag, rc))
    return leaves.reshape(T + 1, -1)


def check_blame_ladder(case, leaves, max_report=12):
    bad = []
    check_leaf_rows(case.w, leaves, case.ref(), case.tag, bad, max_report)
    return bad


# -- the range sums --
# Out of contract: an EMPTY range (lo == hi).  BlameSearch (tc_blame.h) splits at lo + ((hi - lo + 1) >> 1) and never produces
# one, and with lo == hi == N in the last job the masked reload of leaf `lo` would read past the leaf buffer; the harnesses
# refuse such an item instead of launching it, and no table holds one.
def blame_item_model(mults, lo, hi, parts):
    """job_blame_range_part (sum_part's share of [lo, hi) per part, one complete addition per term) and k_blame_range_sum's xor
    tree on multiples mod r: (the sum; the special operands the parts meet as (part, index in the part, kind) -- a term that is the
    identity, an accumulator back at the identity after the part's first term, equal, opposite --; merge_events' events of the
    tree; those of them that are NOT an identity that is the sum of a part (or block of parts) without a term)."""
    n, sums, counts, ev = hi - lo, [], [], []
    for g in range(parts):
        k0, k1, _ = msm_part(n, g, parts)
        acc = 0
        for i, k in enumerate(range(lo + k0, lo + k1)):
            t = mults[k] % R
            kind = "term identity" if t == 0 else None if i == 0 else "acc identity" if acc == 0 else "equal" if acc == t else \
                "opposite" if (acc + t) % R == 0 else None
            if kind:
                ev.append((g, i, kind))
            acc = (acc + t) % R
        sums.append(acc)
        counts.append(k1 - k0)
    total, mev = merge_events(sums)
    empty, d, rnd_no = set(), 1, 0
    while d < parts:
        empty |= {(rnd_no, g) for g in range(parts) if counts[g] == 0 or counts[g ^ d] == 0}
        counts, d, rnd_no = [counts[g] + counts[g ^ d] for g in range(parts)], d * 2, rnd_no + 1
    return total, ev, mev, [e for e in mev if not (e[2] == "identity" and e[:2] in empty)]


class Item:
    """One range [lo, hi) of job `job`.  claims: (parts, "part" / "merge", event) that blame_item_model must confirm; a random
    item claims that it meets nothing at any parts but the identities of its empty parts."""

    def __init__(self, job, lo, hi, tag, claims=None):
        self.job, self.lo, self.hi, self.tag, self.claims, self.random = job, lo, hi, tag, claims or [], claims is None


def _log2(p):
    return p.bit_length() - 1


class RangeCase:
    """F = 4 jobs of N = 130 leaves written by the test (leaf_words), about 100 items: ranges of 1 .. 9, 33, 64, 65 and 130
    leaves side by side in the first wave (lo even, odd, 0 and N - len; the jobs not in order), then directed items, three side
    by side and then a random one.  Jobs 0 and 1 hold random multiples and serve the random items; every directed item has slots
    of its own in jobs 2 and 3."""

    def __init__(self, w):
        self.w, self.tag, self.F, self.N = w, "blame range sums w=%d" % w, BLAME_F, BLAME_N
        rnd = random.Random("manypoint-" + self.tag)
        N = self.N
        self.m = self._slots(rnd, self.F * N)
        head = []
        for i, n in enumerate(BLAME_HEAD):
            lo = (2 * rnd.randrange((N - n) // 2 + 1), min(N - n, 2 * rnd.randrange((N - n) // 2 + 1) + 1), 0, N - n)[i % 4]
            head.append(Item((i + 1) % 2, lo, lo + n, "head"))
        while len(head) < 16:
            head.append(self._random(rnd))
        directed = [d for s in range(5) for d in self._directed(rnd, s)]
        items = head
        for i in range(0, len(directed) - 2, 3):
            items += directed[i:i + 3] + [self._random(rnd)]
        items += directed[len(directed) - len(directed) % 3:]
        while len(items) < 101 or len(items) % 2 == 0:
            items.append(self._random(rnd))
        self.items = items
        self.leaves = np.array([x for m in self.m for x in leaf_words(w, m, rnd)], dtype=np.int32)
        self._ref = None

    def _slots(self, rnd, count):
        """`count` distinct multiples with their points: additions of pool points (pool())"""
        w = self.w
        base, mults, a = pool(w)[:24], [], pool(w)[-1]
        while len(mults) < count:
            b = base[rnd.randrange(24)]
            pt = E[w].add(_PT[w][a], _PT[w][b])
            a = (a + b) % R
            if a and a not in _PT[w]:
                _PT[w][a] = pt
                mults.append(a)
        return mults

    def _random(self, rnd):
        n = rnd.choice([1, 2, 3, 5, 8, 13, 21, 40, 70, 100])
        lo = rnd.randrange(self.N - n + 1)
        return Item(rnd.randrange(2), lo, lo + n, "random")

    def _directed(self, rnd, s):
        """The directed items of set s, each over slots of its own (jobs 2 and 3), rewritten here."""
        self._cursor = 2 * self.N if s == 0 else self._cursor + 1  # (the sets start at even and at odd slots)
        w, N, m = self.w, self.N, self.m
        out = []

        def region(n):
            if self._cursor % N + n > N:
                self._cursor += N - self._cursor % N
            lo = self._cursor
            self._cursor += n
            assert self._cursor <= self.F * N
            return lo

        def item(vals, tag, claims):
            lo = region(len(vals))
            for i, v in enumerate(vals):
                if v is not None:                     # (None: the random multiple that is there)
                    m[lo + i] = v % R
            out.append(Item(lo // N, lo % N, lo % N + len(vals), tag, claims))
            return lo

        top = MAX_PARTS[w]
        p, q = rnd.choice(pool(w)), rnd.choice(pool(w))
        item([0] * 5, "all identities", [(1, "part", (0, 0, "term identity")), (top, "merge", (_log2(top) - 1, 0, "identity"))])
        item([None] + [0] * 6, "one live leaf, first", [(1, "part", (0, 1, "term identity")), (2, "merge", (0, 0, "identity"))])
        item([0] * 6 + [None], "one live leaf, last", [(1, "part", (0, 6, "acc identity")), (2, "merge", (0, 0, "identity"))])
        item([0] * 3 + [None] + [0] * 3, "one live leaf, in the middle", [(1, "part", (0, 3, "acc identity")), (1, "part", (0, 4, "term identity"))])
        item([p, p], "equal neighbours", [(1, "part", (0, 1, "equal")), (2, "merge", (0, 0, "equal"))])
        item([p, neg_mult(w, p)], "P, -P", [(1, "part", (0, 1, "opposite")), (2, "merge", (0, 0, "opposite"))])
        item([q, neg_mult(w, q), None], "P, -P, Q", [(1, "part", (0, 1, "opposite")), (1, "part", (0, 2, "acc identity"))])
        lo = region(8)
        m[lo + 7] = -sum(m[lo:lo + 7]) % R
        out.append(Item(lo // N, lo % N, lo % N + 8, "halves that cancel in the last round",
                        [(pp, "merge", (_log2(pp) - 1, 0, "opposite")) for pp in REC_PARTS[w][1:]]))
        lo = region(5)
        m[lo + 2] = -(m[lo] + m[lo + 1]) % R
        out.append(Item(lo // N, lo % N, lo % N + 5, "back at the identity in mid-part, and on", [(1, "part", (0, 2, "opposite")), (1, "part", (0, 3, "acc identity"))]))
        return out

    def mults(self, it):
        return self.m[it.job * self.N + it.lo:it.job * self.N + it.hi]

    def ref(self):
        """The expected bytes per item, once: the oracle's encoding of [sum a_k] G."""
        if self._ref is None:
            self._ref = [enc(self.w, gmul(self.w, sum(self.mults(it)) % R)) for it in self.items]
        return self._ref


_RANGE = {}


def range_case(w):
    if w not in _RANGE:
        _RANGE[w] = RangeCase(w)
    return _RANGE[w]


def check_blame_claims(case):
    """Every directed item meets what it claims, at the parts it names; every random item meets nothing at any parts but the
    identities of its empty parts.  Returns the list of failures."""
    bad = []
    for j, it in enumerate(case.items):
        ms = case.mults(it)
        what = "%s item %d (%s, [%d, %d) of job %d)" % (case.tag, j, it.tag, it.lo, it.hi, it.job)
        for parts in REC_PARTS[case.w]:
            total, ev, mev, unexplained = blame_item_model(ms, 0, len(ms), parts)
            if total != sum(ms) % R:
                bad.append("%s: the model's sum at parts=%d" % (what, parts))
            if it.random and (ev or unexplained):
                bad.append("%s: a random item meets %s at parts=%d" % (what, ev + unexplained, parts))
            for cp, where, event in it.claims:
                if cp == parts and event not in (ev if where == "part" else mev):
                    bad.append("%s: claims %s %s at parts=%d, the model meets %s / %s" % (what, where, event, parts, ev, mev))
    return bad


def _items_in(items):
    return [np.array([getattr(it, f) for it in items], dtype=np.uint32) for f in ("job", "lo", "hi")]


def run_blame_range(lib, case, parts):
    """(out: n_items rows and two guard rows) as the leg left them."""
    w, n = case.w, len(case.items)
    job, lo, hi = _items_in(case.items)
    out = np.full((n + 2) * PT_BYTES[w], POISON, dtype=np.uint8)
    rc = lib["range_sum"](w - 1, _ptr(case.leaves), case.F, case.N, _ptr(job), _ptr(lo), _ptr(hi), n, parts, _ptr(out))
    if rc != 0:
        raise HipError("%s parts=%d: the harness returned %d" % (case.tag, parts, rc))
    return (out.reshape(n + 2, -1),)


def check_sum_rows(case, what0, out, want, bad):
    """out: len(want) rows and two guard rows.  No item is skipped."""
    if not (out[len(want):] == POISON).all():
        bad.append("%s: the guard rows behind the sums written" % what0)
    for j, it in enumerate(case.items):
        if bytes(out[j]) != want[j]:
            bad.append("%s item %d (%s, [%d, %d) of job %d): wrong output bytes" % (what0, j, it.tag, it.lo, it.hi, it.job))


def check_blame_range(case, parts, res, max_report=12):
    bad = []
    check_sum_rows(case, "%s parts=%d" % (case.tag, parts), res[0], case.ref(), bad)
    return bad


# -- k_blame_leaves -> k_blame_range_sum, the leaves staying where the first kernel left them --
class ChainCase:
    def __init__(self, w):
        self.w, self.N = w, 130
        self.leaves = leaves_case(w, *LEAVES_SHAPES[4])
        assert self.leaves.n == self.N and self.leaves.period == 0
        self.tag = "blame chain w=%d" % w
        rnd = random.Random("manypoint-" + self.tag)
        spans = [(0, 130), (0, 1), (129, 130), (1, 66), (63, 129), (64, 128), (19, 23), (127, 130), (31, 33)]
        spans += [tuple(sorted(rnd.sample(range(131), 2))) for _ in range(12)]
        self.items = [Item(0, lo, hi, "chain") for lo, hi in spans]
        self.parts = [0, 1, 8, MAX_PARTS[w], 3]
        self._ref = None

    def mults(self, it):
        return self.leaves.ref()[1][it.lo:it.hi]

    def ref(self):
        if self._ref is None:
            self._ref = [enc(self.w, gmul(self.w, sum(self.mults(it)) % R)) for it in self.items]
        return self._ref


_CHAIN = {}


def chain_case(w):
    if w not in _CHAIN:
        _CHAIN[w] = ChainCase(w)
    return _CHAIN[w]


def run_blame_chain(lib, case, parts):
    """(out: n_items rows and two guard rows, seed, live bytes with the guard byte) as the leg left them."""
    w, lc, n = case.w, case.leaves, len(case.items)
    pts, live_in, key, seed, live_out = _leaves_in(lc)
    _, lo, hi = _items_in(case.items)
    out = np.full((n + 2) * PT_BYTES[w], POISON, dtype=np.uint8)
    rc = lib["chain"](w - 1, _ptr(key), lc.call, lc.leaf0, _ptr(pts), len(lc.a), lc.period, _ptr(live_in), lc.n, _ptr(lo), _ptr(hi), n, parts,
                      _ptr(seed), _ptr(live_out), _ptr(out))
    if rc != 0:
        raise HipError("%s parts=%d: the harness returned %d" % (case.tag, parts, rc))
    return out.reshape(n + 2, -1), seed, live_out


def check_blame_chain(case, parts, res, max_report=12):
    out, seed, live = res
    want_seed, _, _, want_live = case.leaves.ref()
    bad = []
    if bytes(seed) != want_seed or live.tolist() != want_live:
        bad.append("%s parts=%d: seed or live bytes" % (case.tag, parts))
    check_sum_rows(case, "%s parts=%d" % (case.tag, parts), out, case.ref(), bad)
    return bad


# -- blame_sum_parts --
SUM_PARTS_TABLE = [(w, n_items, longest, cus) for w in (1, 2) for n_items in (1, 65536) for longest in (1, 2, 3, 4, 127, 128, 200) for cus in (0, 1, 256)]


def blame_sum_parts_model(w, n_items, longest, cus):
    """The documented rule: the smallest power of two of lanes (G2: lane pairs) per item that gives the launch one wave per SIMD
    (4 SIMDs on each of `cus` CUs; 256 CUs when cus is not positive), at most half the longest range and at most a wave."""
    want = (cus if cus > 0 else 256) * 4 * MAX_PARTS[w]  # lanes (lane pairs) of one wave per SIMD
    need = 1
    while n_items * need < want:
        need *= 2
    half = 1
    while half * 2 * 2 <= longest:
        half *= 2
    return min(need, half, MAX_PARTS[w])
