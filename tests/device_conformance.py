"""Device conformance suite: builders, operand generator, references and case tables.

tests/device/conformance.h applies ONE shipped primitive of threshold_crypto_amd/csrc per op to operands given as raw
signed limbs (14 x int32, radix 2^28, Montgomery R = 2^392).  The same case tables run through

  * the gfx950 build (tests/device/conformance.hip, hipcc with the product's flags): tests/test_gpu_conformance.py, and
  * the host build (tests/device/conformance_host.cpp, g++ -DTC_BOUND_CHECK, the declared input intervals loaded into the
    interval bookkeeping): tests/test_conformance_host.py, in a child process per op (a bound violation aborts it).

Every result is compared with Python big integers (oracle/tc_oracle.py) AND checked against the primitive's output
contract (limb ranges, value bound), which is what the next operation relies on.

The scalar block (ops 100 on) takes its operands as raw u32 words instead (raw_words): scalars, u64 digits and index
lists, with t, i, K and nbits in aux.  Where the device makes a decision once per wave (wave_any), the op's table is laid
out by a hook (LAYOUTS): whole waves that take one path, then waves that mix them.

The pairing block (ops 80 on; 90 on run four lanes per job, tc_quad.h) checks Miller steps, loops, the cyclotomic and the
final exponentiation and the check itself against the oracle's pairing: a Miller value must equal the product's own
(dev_miller_loop: the shipped step formulas on residues) and differ from the oracle's by a factor in Fq2; GT values and
check bits must equal the oracle's exactly.  MILLER_LINES also hands back its row block (prepared lines, line products).

The point-multiplication block (ops 140 on: G1, one lane per job; 160 on: G2, a lane pair) checks the routines that turn
digits and group operations into a multiple -- table builders, common-Z bookkeeping, the branch-free ladders and their
safe twins, GLS / GLV, cofactor clearing, the Straus combiners, the [1 / D] step -- against E.mul / E.add of the oracle.
Which path a case takes (the branch-free pass alone, or the safe ladder after a special case) comes from a Python model
that walks the ladder's columns on the oracle's group law (the *_model functions); ops with a table in the arena of
tc_table.h (NEEDS_TABLE) run with a slot held, and the device leg fails if a slot stays marked in use.

The byte layer (ops 180 on: hash primitives and G1, one lane per job; 200 on: a lane pair) checks the code on either side of
the arithmetic -- SHA3-256, the ChaCha20 word stream, the rejection samplers, the hash onto G2, the wire codecs and the job_*
wrappers around them -- against hashlib, the oracle's ChaCha and samplers, and its decoders.  Byte operands go in as raw
words (raw_bytes), byte results are read back from the output row, which stays filled with the sentinel wherever the
routine's documented length ends (check_row).  byte_cases() is the one shared table of encodings, each with the oracle's verdict.

The wave-uniform forms of the G2 share combination (scalar ops 128 on, point ops 172 on, byte op 214) read their parameters
from the wave's first active lane.  Their tables are aligned blocks of 32 jobs with one key and a ragged tail (uniform_table),
the exceptional lanes first, last and in the middle of a block, and each routine's exception flag must equal what a Python
walk of the same ladder says (straus_uniform_model, wnaf_ladder_model, quotient_mul_model), lane by lane.

    python tests/device_conformance.py host OPNAME    (the host leg of one op; exit status 0 = every case passed)
"""
import ctypes
import hashlib
import itertools
import math
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import tc_oracle as o  # noqa: E402

DEV = os.path.join(HERE, "device")
CSRC = os.path.join(ROOT, "threshold_crypto_amd", "csrc")
BUILD = os.path.join(DEV, "_build")

P = o.Q
RB = 28
NL = 14
MASK = (1 << RB) - 1
RM = 1 << 392  # Montgomery R
RINV = pow(RM, -1, P)
CONF_IN, CONF_OUT, CONF_AUX, CONF_FLAGS = 40, 40, 4, 16
CONF_MAX_N = 68  # t + 1 of the scalar block's index lists
# input contract of the primitives (tc_field.h): |limb| <= 7.9 * 2^28, |value| <= 300 p, B_a * B_b <= 8.14 at a product
LIMB_MAX = 7.9
VAL_MAX = 300
PRODUCT_MAX = 8.14
NORM_LO, NORM_HI = -0.001, 1.001  # the limb interval of norm() / reduce_value() / point coordinates (units of 2^28)
CYCLO_REDUCE_EVERY = 3  # tc_tower.h kCycloReduceEvery (the product builds with the default)

# op ids: tests/device/conformance.h enum Op
OPS = dict(
    FQ_MUL=0, FQ_SQR=1, FQ_REDC_FULL=2, FQ_FROM_CANONICAL=3, FQ_TO_CANONICAL=4, FQ_FROM_MONT384=5, FQ_GT_HALF=6, FQ_NORM=7,
    FQ_REDUCE_VALUE=8, FQ_ZERO=9, FQ_INV=10, FQ_INV_FERMAT=11, FQ_INV30=12, FQ_LEGENDRE=13, FQ_SQRT=14,
    FQ2_MUL=20, FQ2_SQR=21, FQ2_CONJ=22, FQ2_MUL_XI=23, FQ2_NORM_FQ=24, FQ2_INV=25, FQ2_ZERO=26, FQ2_SQRT=27, FQ2_SQRT_X2=28,
    FQ2_INV_X2=29,
    FQ6_MUL=40, FQ6_SQR=41, FQ6_INV=42, FQ12_MUL=43, FQ12_SQR=44, FQ12_INV=45, FQ12_FROB=46, FQ12_CONJ=47,
    FQ12_LINE_PRODUCT=48, FQ12_CYCLO_SQR=49, CYCLO_CHAIN=50,
    G1_DBL=60, G1_ADD_MIXED=61, G1_ADD=62, G1_ADD_MIXED_GENERIC=63, G1_ADD_GENERIC=64, G1_TO_AFFINE=65, G1_ON_CURVE=66,
    G1_IN_SUBGROUP=67,
    G2_DBL=70, G2_ADD_MIXED=71, G2_ADD=72, G2_ADD_MIXED_GENERIC=73, G2_ADD_GENERIC=74, G2_TO_AFFINE=75, G2_TO_AFFINE_X2=76,
    G2_ON_CURVE=77, G2_IN_SUBGROUP=78, G2_PSI=79,
    MILLER_DBL_STEP=80, MILLER_ADD_STEP=81, MILLER_LOOP2=82, MILLER_LINES=83, CYCLO_EXP_BY_X=84, CYCLO_EXP_BY_X_HALF=85,
    FINAL_EXP=86, PAIRING_CHECK=87,
    Q_MILLER_LOOP=90, Q_EXP_BY_X=91, Q_EXP_BY_X_HALF=92, Q_FINAL_EXP=93, Q_PAIRING_CHECK=94,
    FR_ADD=100, FR_SUB=101, FR_MUL=102, FR_SQR=103, FR_INV=104, FR_FROM_CANONICAL=105, FR_TO_CANONICAL=106, FR_FROM_U64=107,
    FR_FROM_LE32=108, FR_SCALE_COFACTOR_FIX=109,
    DIV_BY_X_ABS=110, GLS_DECOMPOSE=111, GLS_DECOMPOSE_ODD=112, SAC_RECODE4=113, GLV_DECOMPOSE=114,
    GLV_RECODE_SIGN_ALIGNED=115, MSM_G1_RECODE=116,
    LAGRANGE_COEFF=120, LAGRANGE_COEFF_FR=121, LAGRANGE_ALL=122, LAGRANGE_SPLIT=123, LAGRANGE_SMALL_COEFFS=124,
    COMBINE_CLASS=125, FR_INVERSE_OF_SMALL=126, GCD_U64=127, WNAF_RECODE=128, COMBINE_QUOTIENT_DECOMPOSE=129,
    COMBINE_DIVIDE_CHOICE=130,
    G1_ADD_AFFINE=140, G1_COMMON_Z=141, G1_MUL_BY_X_ABS=142, G1_MUL_GLV=143, G1_MUL_GLV_JAC=144, G1_MUL_GLV_ARENA=145,
    G1_LINCOMB_CHUNK4=146, G1_STRAUS_SMALL=147, G1_STRAUS_SMALL_INLINE=148, G1_COMBINE_DIVIDE=149,
    G1_COMBINE_DIVIDE_ARENA=150, G1_MUL_U64=151,
    G2_ADD_AFFINE=160, G2_COMMON_Z=161, G2_MUL_BY_X_ABS=162, G2_PSI_JAC=163, G2_GLS_BASES=164, G2_SAC_TABLE=165,
    G2_JOINT_MUL4=166, G2_MUL_GLS=167, G2_MUL_GLS_JAC=168, G2_CLEAR_COFACTOR=169, G2_STRAUS_SMALL=170,
    G2_COMBINE_DIVIDE=171, G2_STRAUS_SMALL_UNIFORM=172, G2_WNAF_TABLE=173, G2_COMBINE_DIVIDE_UNIFORM=174,
    G2_COMBINE_DIVIDE_QUOTIENT=175, G2_QUOTIENT_MUL=176, G2_COMBINE_UNIFORM_WAVE=177,
    SHA3_256=180, CHACHA_WORDS=181, FQ_RANDOM=182, XOR_WITH_HASH=183, FQ_FROM_BE48=184, FQ_TO_BE48=185, FQ_LEX_LARGEST=186,
    G1_DECODE_UNCOMPRESSED=187, G1_ENCODE_UNCOMPRESSED=188, G1_ENCODE_COMPRESSED=189, G1_DECODE_COMPRESSED=190,
    G2_RANDOM_FROM_SEED=200, G2_RANDOM_FROM_SEED_X2=201, HASH_G2=202, HASH_G2_X2=203, HASH_G1_G2=204, HASH_G1_G2_X2=205,
    FQ2_FROM_BE96=206, FQ2_TO_BE96=207, FQ2_LEX_LARGEST=208, G2_DECODE_UNCOMPRESSED=209, G2_ENCODE_UNCOMPRESSED=210,
    G2_ENCODE_COMPRESSED=211, G2_DECODE_COMPRESSED=212, G2_DECODE_COMPRESSED_X2=213, JOB_COMBINE_SMALL_G2=214)


def lanes(op):
    i = OPS[op]
    return 4 if 90 <= i < 100 else 2 if (20 <= i < 60 or 70 <= i < 90 or 160 <= i < 180 or i >= 200) else 1


NEEDS_ROWS = {"MILLER_LINES"}  # conformance.h conf_needs_rows
# conformance.h conf_needs_table: the device leg runs these with a slot of a table arena held (tc_table.h)
NEEDS_TABLE = {"G1_MUL_GLV_ARENA", "G1_COMBINE_DIVIDE_ARENA", "G2_SAC_TABLE", "G2_JOINT_MUL4", "G2_MUL_GLS", "G2_MUL_GLS_JAC",
               "G2_COMBINE_DIVIDE", "G2_STRAUS_SMALL_UNIFORM", "G2_WNAF_TABLE", "G2_COMBINE_DIVIDE_UNIFORM", "G2_COMBINE_DIVIDE_QUOTIENT",
               "G2_QUOTIENT_MUL", "G2_COMBINE_UNIFORM_WAVE", "JOB_COMBINE_SMALL_G2"}
SLOT_LEAK = -2  # conformance.hip kConfSlotLeak: a table slot was still marked in use after the run


# ---------------------------------------------------------------------------------------------------------------------
# builds
# ---------------------------------------------------------------------------------------------------------------------
def _digest(extra, srcs):
    h = hashlib.sha256()
    for d in (CSRC, DEV):
        for name in sorted(os.listdir(d)):
            if name.endswith((".h", ".hip", ".cpp")) and (d == CSRC or name in srcs or name.endswith(".h")):
                with open(os.path.join(d, name), "rb") as f:
                    h.update(name.encode())
                    h.update(f.read())
    h.update(" ".join(extra).encode())
    return h.hexdigest()[:16]


def _build(name, cmd_of, srcs):
    os.makedirs(BUILD, exist_ok=True)
    probe = cmd_of("X")
    lib = os.path.join(BUILD, "%s-%s.so" % (name, _digest(probe, srcs)))
    if not os.path.exists(lib):
        subprocess.run(cmd_of(lib + ".tmp"), check=True, timeout=900)
        os.replace(lib + ".tmp", lib)
        for old in os.listdir(BUILD):  # stale builds of earlier sources
            if old.startswith(name + "-") and old != os.path.basename(lib):
                os.remove(os.path.join(BUILD, old))
    return lib


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def build_device():
    """tests/device/conformance.hip -> a gfx950 shared object, with the product's compiler flags (build.py FLAGS)."""
    from threshold_crypto_amd import build as tcb
    src = os.path.join(DEV, "conformance.hip")
    return _build("libtc_conformance", lambda out: [hipcc()] + tcb.FLAGS + ["-w", "-shared", src, "-o", out], {"conformance.hip"})


def build_host():
    """The same op bodies for the host (host Fq2 form), under the interval analysis."""
    src = os.path.join(DEV, "conformance_host.cpp")
    return _build("libtc_conformance_host_bc",
                  lambda out: ["g++", "-O1", "-std=c++17", "-w", "-DTC_BOUND_CHECK", "-DTC_TEST_HOOKS", "-shared", "-fPIC", "-pthread", src,
                               "-o", out],
                  {"conformance_host.cpp"})


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def value(limbs):
    """The integer a limb vector holds (limb i has weight 2^(28 i); limbs are signed)."""
    return sum(int(x) << (RB * i) for i, x in enumerate(limbs))


def residue(limbs):
    """The field element a Montgomery representation stands for."""
    return value(limbs) * RINV % P


def mont(v):
    return v * RM % P


class Operand:
    """One input slot: raw limbs plus the interval declared for them (lo, hi in units of 2^28; val: |value| <= val * p)."""

    def __init__(self, limbs, lo, hi, val):
        self.limbs, self.lo, self.hi, self.val = list(limbs), lo, hi, val

    @property
    def bound(self):
        return max(-self.lo, self.hi)


def encode(v, k=0, interval=(0.0, 1.0), push=None):
    """Limbs whose integer is  v R mod p + k p,  inside `interval` (units of 2^28).  push: None (plain digits), "hi" / "lo"
    (every limb moved toward that end of the interval by borrowing from its upper neighbour) or "alt" (alternating).
    The result is checked against the input contract before anything is launched."""
    x = mont(v % P) + k * P
    lo, hi = interval
    LO, HI = int(lo * (1 << RB)), int(hi * (1 << RB))
    l = [(x >> (RB * i)) & MASK for i in range(NL - 1)] + [x >> (RB * (NL - 1))]
    if hi < 1.0:  # balanced digits in [-2^27, 2^27) first
        for i in range(NL - 1):
            if l[i] >= 1 << (RB - 1):
                l[i] -= 1 << RB
                l[i + 1] += 1
    if push:
        for i in range(NL - 1):
            up = push == "hi" or (push == "alt" and i % 2 == 0)
            if up:
                c = (HI - l[i]) >> RB
                if c > 0:
                    l[i] += c << RB
                    l[i + 1] -= c
            else:
                c = (l[i] - LO) >> RB
                if c > 0:
                    l[i] -= c << RB
                    l[i + 1] += c
    assert value(l) == x
    val = max(1, -(-abs(x) // P))
    op = Operand(l, lo, hi, val)
    check_input(op)
    return op


def encode_int(x, interval=(0.0, 1.0)):
    """Plain digits of an integer (not a Montgomery form): the representative p of zero, R itself, ..."""
    l = [(x >> (RB * i)) & MASK for i in range(NL - 1)] + [x >> (RB * (NL - 1))]
    op = Operand(l, interval[0], interval[1], max(1, -(-abs(x) // P)))
    check_input(op)
    return op


def check_input(op):
    """The documented input contract (tc_field.h): every limb inside its declared interval, |limb| <= 7.9 * 2^28,
    |value| <= 300 p.  A case that violates it is a bug of the test, never a finding."""
    lo, hi = op.lo * (1 << RB), op.hi * (1 << RB)
    assert -LIMB_MAX <= op.lo <= op.hi <= LIMB_MAX, (op.lo, op.hi)
    assert all(lo <= x <= hi for x in op.limbs), ("limb outside its interval", op.lo, op.hi, op.limbs)
    assert all(-2 ** 31 <= x < 2 ** 31 for x in op.limbs)
    assert abs(value(op.limbs)) <= op.val * P and op.val <= VAL_MAX, op.val


def check_product_operands(a, b):
    assert a.bound * b.bound <= PRODUCT_MAX, ("operands beyond the column limit", a.bound, b.bound)


def words(x):
    """A canonical integer as the 12 little-endian u32 words the codecs use (in the first 12 ints of a slot)."""
    w = [(x >> (32 * i)) & 0xffffffff for i in range(12)]
    return Operand([c - (1 << 32) if c >= 1 << 31 else c for c in w] + [0, 0], 0, 1, 1)


def raw_words(ws):
    """Raw u32 words across consecutive slots (14 words each, zero-padded): scalars, u64 digits, index lists.  They are
    not limbs, so they are not held to the limb contract (check_input)."""
    ws = [int(w) & 0xffffffff for w in ws]
    assert len(ws) <= CONF_IN * NL
    ws += [0] * (-len(ws) % NL)
    return [Operand([c - (1 << 32) if c >= 1 << 31 else c for c in ws[k:k + NL]], 0, 1, 1) for k in range(0, len(ws), NL)]


def words_value(op):
    return sum((int(c) & 0xffffffff) << (32 * i) for i, c in enumerate(op.limbs[:12]))


def limbs30(x):
    return Operand([(x >> (30 * i)) & ((1 << 30) - 1) for i in range(13)] + [0], 0, 4, 1)


class Case:
    def __init__(self, slots, aux=(), tag=""):
        self.slots, self.aux, self.tag = slots, list(aux), tag


def eq_ok(a, b):
    """a - b (the first step of a == b) inside the input contract: declared limb intervals and value bound."""
    return a.lo - b.hi >= -LIMB_MAX and a.hi - b.lo <= LIMB_MAX and a.val + b.val <= VAL_MAX


def zero_case(slots, tag, eq_pairs):
    return Case(slots, aux=[int(all(eq_ok(slots[i], slots[j]) for i, j in eq_pairs))], tag=tag)


# ---------------------------------------------------------------------------------------------------------------------
# launching
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A
FLAG_SENTINEL = -77


def pack(cases):
    n = len(cases)
    inp = np.zeros((n, CONF_IN, NL), np.int32)
    rng = np.zeros((n, CONF_IN, 3), np.float32)
    rng[:, :, 1] = 1.0
    rng[:, :, 2] = 1.0
    aux = np.zeros((n, CONF_AUX), np.int32)
    for j, c in enumerate(cases):
        for s, op in enumerate(c.slots):
            inp[j, s] = op.limbs
            rng[j, s] = (op.lo, op.hi, op.val)
        aux[j, :len(c.aux)] = c.aux
    out = np.full((n, CONF_OUT, NL), SENTINEL, np.int32)
    flags = np.full((n, CONF_FLAGS), FLAG_SENTINEL, np.int32)
    return inp, rng, aux, out, flags


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rows_buf(op, n):
    """The row block of conf_needs_rows ops, per job: MILLER_ROW_SLOTS x (re, im) x 14 limbs (None for other ops)."""
    return np.zeros((n, MILLER_ROW_SLOTS, 2, NL), np.int32) if op in NEEDS_ROWS else None


def run_device(lib, op, cases):
    inp, _, aux, out, flags = pack(cases)
    rows = _rows_buf(op, len(cases))
    rc = lib.tc_conf_run(OPS[op], len(cases), _p(inp), _p(aux), _p(out), _p(flags), None if rows is None else _p(rows))
    assert rc != SLOT_LEAK, "op %s left a table slot marked in use" % op
    assert rc == 0, "HIP error %d in op %s" % (rc, op)
    return out, flags, rows


def run_host(lib, op, cases):
    inp, rng, aux, out, flags = pack(cases)
    rows = _rows_buf(op, len(cases))
    rc = lib.tc_conf_host_run(OPS[op], len(cases), _p(inp), _p(rng), _p(aux), _p(out), _p(flags),
                              None if rows is None else _p(rows))
    assert rc == 0
    return out, flags, rows


# ---------------------------------------------------------------------------------------------------------------------
# output contracts
# ---------------------------------------------------------------------------------------------------------------------
class Fail(AssertionError):
    pass


def expect(cond, case, what):
    if not cond:
        raise Fail("%s [case %s]" % (what, case.tag))


def out_limbs(out, s):
    return [int(x) for x in out[s]]


def check_carried(case, l, what):
    """A product's / redc's output: limbs 0..12 fully carried into [0, 2^28), the top limb holds the rest."""
    expect(all(0 <= x <= MASK for x in l[:NL - 1]), case, "%s: limbs not carried %s" % (what, l))


def check_product(case, l, x, what="product"):
    """The Montgomery product's contract: out = (x + m p) / R exactly, with 0 <= m < R (so the value lies in
    (x / R, x / R + p)), limbs carried."""
    check_carried(case, l, what)
    t = value(l) * RM - x
    expect(t % P == 0 and 0 <= t // P < RM, case, "%s: out R - x = %s p is not m p with 0 <= m < R" % (what, t / P))


def check_normed(case, l, what, val_bound=VAL_MAX, lo=NORM_LO, hi=NORM_HI):
    L, H = lo * (1 << RB), hi * (1 << RB)
    expect(all(L <= x <= H for x in l[:NL - 1]), case, "%s: limbs outside [%g, %g] 2^28: %s" % (what, lo, hi, l))
    expect(abs(l[NL - 1]) <= max(-L, H), case, "%s: top limb %d" % (what, l[NL - 1]))
    expect(abs(value(l)) <= val_bound * P, case, "%s: |value| = %.3f p > %g p" % (what, abs(value(l)) / P, val_bound))


def f2_res(out, s):
    return (residue(out[s]), residue(out[s + 1]))


def f6_res(out, s):
    return (f2_res(out, s), f2_res(out, s + 2), f2_res(out, s + 4))


def f12_res(out, s):
    return (f6_res(out, s), f6_res(out, s + 6))


def check_bounded(case, out, s, n, what, limb=NORM_HI, val_bound=VAL_MAX, lo=None):
    for i in range(n):
        check_normed(case, out_limbs(out, s + i), "%s[%d]" % (what, i), val_bound, -limb if lo is None else lo, limb)


def flags_agree(case, flags, nflags):
    """Both lanes of a pair hold the same predicate (the one-lane and host forms write both halves)."""
    expect(list(flags[:nflags]) == list(flags[4:4 + nflags]), case,
           "the lanes of the pair disagree: %s vs %s" % (list(flags[:nflags]), list(flags[4:4 + nflags])))


# ---------------------------------------------------------------------------------------------------------------------
# the edge values
# ---------------------------------------------------------------------------------------------------------------------
HALF = (P - 1) // 2


def fq_edges():
    """The field elements where carries, signs and reductions turn: 0, 1, 2, p-1, p-2, (p +- 1)/2, 2^k and p - 2^k for k
    around every multiple of 28 and up to 380, 2^381 mod p, R, R^-1, R^2 mod p."""
    e = [0, 1, 2, P - 1, P - 2, HALF, HALF + 1, HALF - 1, (1 << 381) % P, RM % P, RINV, RM * RM % P]
    for m in range(0, 392, 28):
        for k in (m - 1, m, m + 1):
            if 0 <= k <= 380:
                e += [(1 << k) % P, (P - (1 << k)) % P]
    e += [(1 << 380) % P, P - (1 << 380)]
    out = []
    for v in e:
        if v not in out:
            out.append(v)
    return out


def g1_point(rnd, in_group=True):
    if in_group:
        return o.E1.mul(o.G1_GEN, rnd.randrange(1, o.R))
    while True:
        x = rnd.randrange(P)
        y2 = (x ** 3 + 4) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            pt = (x, y)
            if o.E1.mul(pt, o.R) is not None:
                return pt


def g2_point(rnd, in_group=True):
    if in_group:
        return o.E2.mul(o.G2_GEN, rnd.randrange(1, o.R))
    while True:
        pt = o.g2_get_point_from_x((rnd.randrange(P), rnd.randrange(P)), rnd.random() < 0.5)
        if pt is not None and o.E2.mul(pt, o.R) is not None:
            return pt


# ---------------------------------------------------------------------------------------------------------------------
# op specs: cases(rnd) -> [Case], check(case, out, flags) raises Fail
# ---------------------------------------------------------------------------------------------------------------------
SPECS = {}


def spec(name, random_case, nflags=0):
    def deco(fn):
        SPECS[name] = (fn, random_case, nflags)
        return fn
    return deco


PRODUCT_PAIRS = [(1.0, 1.0), (1.03, 7.9), (7.9, 1.03), (2.0, 4.07), (4.07, 2.0), (2.85, 2.85)]
PUSHES = (None, "hi", "lo", "alt")


def _mul_case(a, b, tag, square=False):
    check_product_operands(a, b)
    return Case([a] if square else [a, b], tag=tag)


# ---- Fq -----------------------------------------------------------------------------------------------------------
def _fq_mul_cases(rnd, square):
    cases = []
    for v in fq_edges():
        w = rnd.choice(fq_edges())
        a = encode(v)
        cases.append(_mul_case(a, encode(w), "edge %x*%x" % (v, w), square))
    # the representative p of zero
    cases.append(_mul_case(encode_int(P), encode(rnd.randrange(P)), "p*x", square))
    # lazy inputs at k = +-300, +-299, +-1, limbs at their interval ends; operand pairs at the column limit
    for ba, bb in PRODUCT_PAIRS:
        for push in PUSHES:
            for k in (299, -300, -299, 1, -1, 0):
                if abs(k) > 30 and min(ba, bb) < 0.5:
                    continue
                va = 0 if abs(k) == 300 else rnd.choice(fq_edges() + [rnd.randrange(P)])
                a = encode(va, k, (-ba, ba), push)
                b = a if square else encode(rnd.randrange(P), -k if k != -300 else 3, (-bb, bb), push)
                if square and ba != bb:
                    continue
                cases.append(_mul_case(a, b, "lazy k=%d B=(%g,%g) %s" % (k, ba, bb, push), square))
    return cases


def _rand_mul(rnd, square):
    ba, bb = rnd.choice(PRODUCT_PAIRS)
    if square:
        ba = bb = rnd.choice([1.0, 2.0, 2.85])
    a = encode(rnd.randrange(P), rnd.randint(-3, 3), (-ba, ba), rnd.choice(PUSHES))
    b = a if square else encode(rnd.randrange(P), rnd.randint(-3, 3), (-bb, bb), rnd.choice(PUSHES))
    return _mul_case(a, b, "random", square)


def _check_mul(case, out, flags, square):
    a = value(case.slots[0].limbs)
    b = a if square else value(case.slots[1].limbs)
    l = out_limbs(out, 0)
    check_product(case, l, a * b)
    expect(residue(l) == residue(case.slots[0].limbs) * residue(case.slots[-1].limbs) % P, case, "residue")


@spec("FQ_MUL", lambda rnd: _rand_mul(rnd, False))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fq_mul_cases(rnd, False)
    _check_mul(case, out, flags, False)


@spec("FQ_SQR", lambda rnd: _rand_mul(rnd, True))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fq_mul_cases(rnd, True)
    _check_mul(case, out, flags, True)


def _lazy_value_cases(rnd, kinds=(299, -300, -299, 1, -1, 0, 150, -150)):
    cases = [Case([encode(v)], tag="edge %x" % v) for v in fq_edges()]
    cases.append(Case([encode_int(P)], tag="p"))
    for k in kinds:
        for push in PUSHES:
            for iv in ((-7.9, 7.9), (-1.0, 1.0), (-0.001, 1.001)):
                v = 0 if abs(k) == 300 else rnd.choice(fq_edges())
                try:
                    cases.append(Case([encode(v, k, iv, push)], tag="lazy k=%d %s %s" % (k, iv, push)))
                except AssertionError:
                    pass  # (a push that cannot keep the top limb inside a narrow interval)
    return cases


def _rand_lazy(rnd):
    return Case([encode(rnd.randrange(P), rnd.randint(-300, 299), (-7.9, 7.9), rnd.choice(PUSHES))], tag="random")


@spec("FQ_REDC_FULL", _rand_lazy)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _lazy_value_cases(rnd)
    l = out_limbs(out, 0)
    expect(all(0 <= x <= MASK for x in l), case, "redc_full: limbs not in [0, 2^28): %s" % l)
    v = value(l)
    expect(0 <= v <= P, case, "redc_full: value outside [0, p]")
    expect(v % P == residue(case.slots[0].limbs), case, "redc_full: residue")


@spec("FQ_FROM_CANONICAL", lambda rnd: Case([words(rnd.randrange(P))], tag="random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [Case([words(v)], tag="edge %x" % v) for v in fq_edges()]
    l = out_limbs(out, 0)
    x = words_value(case.slots[0])
    check_product(case, l, x * (RM * RM % P))
    expect(residue(l) == x, case, "from_canonical: residue")


@spec("FQ_FROM_MONT384", lambda rnd: Case([words(rnd.randrange(P))], tag="random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [Case([words(v)], tag="edge %x" % v) for v in fq_edges()]
    l = out_limbs(out, 0)
    x = words_value(case.slots[0])
    check_carried(case, l, "from_mont384")
    expect(residue(l) == x * pow(2, -384, P) % P, case, "from_mont384: residue")
    expect(-P // 4 < value(l) < 5 * P // 4, case, "from_mont384: value outside (-p/4, 5p/4)")


@spec("FQ_TO_CANONICAL", _rand_lazy)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _lazy_value_cases(rnd)
    w = sum((int(c) & 0xffffffff) << (32 * i) for i, c in enumerate(out[0][:12]))
    expect(w == residue(case.slots[0].limbs), case, "to_canonical: %x" % w)


@spec("FQ_GT_HALF", lambda rnd: Case([words(rnd.randrange(P))], tag="random"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        vs = fq_edges() + [HALF - 2, HALF + 2, P - 3]
        return [Case([words(v)], tag="%x" % v) for v in vs]
    x = words_value(case.slots[0])
    expect(flags[0] == int(x > HALF), case, "gt_half(%x) = %d" % (x, flags[0]))


@spec("FQ_NORM", _rand_lazy)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _lazy_value_cases(rnd)
    l = out_limbs(out, 0)
    expect(value(l) == value(case.slots[0].limbs), case, "norm changed the value")
    check_normed(case, l, "norm")


def _reduce_value_cases(rnd):
    cases = _lazy_value_cases(rnd)
    # values where floorf(top / p_top) in reduce_value sits at an integer boundary: k p + (small) and k p - (small), with
    # the top limb of the carried value exactly k * p_top, just below it and just above it
    ptop = P >> (RB * (NL - 1))
    for k in list(range(-300, 301, 23)) + [-300, -299, -1, 0, 1, 2, 3, 150, 299, 300]:
        for d in (-2, -1, 0, 1, 2):
            for x in (k * P + d, (k * ptop) << (RB * (NL - 1)), ((k * ptop) << (RB * (NL - 1))) - 1 + d,
                      ((k * ptop + 1) << (RB * (NL - 1))) + d):
                if abs(x) > 300 * P:
                    continue
                for push in (None, "hi", "lo"):
                    try:
                        cases.append(Case([_encode_raw(x, (-7.9, 7.9), push)], tag="floor k=%d d=%d %s" % (k, d, push)))
                    except AssertionError:
                        pass
    return cases


def _encode_raw(x, interval, push):
    """encode() for an integer given directly (not v R + k p)."""
    k, r = divmod(x, P)
    op = encode(r * RINV % P, k, interval, push)
    assert value(op.limbs) == x
    return op


@spec("FQ_REDUCE_VALUE", _rand_lazy)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _reduce_value_cases(rnd)
    l = out_limbs(out, 0)
    expect((value(l) - value(case.slots[0].limbs)) % P == 0, case, "reduce_value changed the residue")
    check_normed(case, l, "reduce_value", val_bound=2.1)
    expect(value(l) > -P // 64, case, "reduce_value: value %.4f p below 0" % (value(l) / P))


def _mz(limbs, bits):
    t = (value(limbs) % (1 << bits)) * (-pow(P, -1, 1 << bits)) % (1 << bits)
    return int(((t + 300) % (1 << bits)) <= 600)


def _zero_cases(rnd):
    cases = []
    # EVERY representation k p of zero, k in [-300, 300], with lazy limbs
    for k in range(-300, 301):
        push = PUSHES[k % 4]
        iv = (-7.9, 7.9) if k % 3 else (-1.0, 1.0)
        try:
            a = encode(0, k, iv, push)
        except AssertionError:
            a = encode(0, k, (-7.9, 7.9), push)
        b = encode(0, rnd.randint(-3, 3), (-1.0, 1.0), rnd.choice(PUSHES))
        cases.append(zero_case([a, b], "zero k=%d" % k, [(0, 1)]))
    # near misses: k p + 1, k p - 1, and the values the filter lets through (t within 300 of zero but not a multiple of p)
    for k in (-300, -299, -1, 0, 1, 299):
        for d in (1, -1, 2 ** 28, -(2 ** 28)):
            x = k * P + d
            if abs(x) <= 300 * P:
                cases.append(zero_case([_encode_raw(x, (-7.9, 7.9), "alt"), encode(1)], "near k=%d d=%d" % (k, d), [(0, 1)]))
    for j in (-300, -299, 299, 300, 301, -301):
        # value = j (mod 2^56) * ... : low bits equal those of j p, residue non-zero
        x = j * P + (1 << 60) * rnd.randrange(1, 1 << 100)
        if abs(x) <= 300 * P:
            cases.append(zero_case([_encode_raw(x, (-7.9, 7.9), None), encode(0)], "filter edge j=%d" % j, [(0, 1)]))
    # a == b with b a different representation of the same element
    for v in fq_edges()[:20]:
        cases.append(zero_case([encode(v, 5, (-2.0, 2.0), "hi"), encode(v, -7, (-2.0, 2.0), "lo")], "eq %x" % v, [(0, 1)]))
    return cases


@spec("FQ_ZERO", lambda rnd: zero_case([encode(rnd.randrange(P), rnd.randint(-290, 290), (-6.9, 6.9), "alt"),
                                        encode(rnd.randrange(P))], "random", [(0, 1)]), nflags=4)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _zero_cases(rnd)
    a, b = case.slots[0].limbs, case.slots[1].limbs
    z = residue(a) == 0
    if z:
        expect(flags[0] == 1 and flags[1] == 1, case, "the zero filter missed a zero: %s" % list(flags[:2]))
    expect(flags[0] == _mz(a, 28), case, "maybe_zero = %d" % flags[0])
    expect(flags[1] == _mz(a, 56), case, "maybe_zero56 = %d" % flags[1])
    expect(flags[2] == int(z), case, "is_zero = %d" % flags[2])
    if case.aux[0]:
        expect(flags[3] == int(residue(a) == residue(b)), case, "== gave %d" % flags[3])


# Operands whose binary GCD (tc_field.h fq_inv_limbs30) needs the most steps before b = 1, the point after which v holds
# the inverse: c 2^k mod p with a small odd c near the top (3 * 2^379: 760 exact steps, all 26 rounds of 30; random
# operands: 540-580 steps, about 20 rounds).  2^380 runs all 26 rounds too but is correct after 381 steps.  A lower round
# cap breaks the former, and only rare random operands.
SLOW_INV = [3 * 2 ** 379 % P, 7 * 2 ** 377 % P, 3 * 2 ** 378 % P, 45 * 2 ** 375 % P, 5 * 2 ** 336]


def _inv_edges(rnd):
    vs = [0, 1, 2, 3, P - 1, P - 2, HALF, HALF + 1] + SLOW_INV
    vs += [1 << k for k in (100, 200, 250, 300, 330, 350, 360, 370, 375, 378, 379, 380)]
    vs += [P - (1 << k) for k in (200, 300, 379, 380)]
    vs += [(1 << 381) % P, RM % P, RINV]
    return vs


def _inv_cases(rnd):
    cases = [Case([encode(v)], tag="inv %x" % v) for v in _inv_edges(rnd)]
    cases.append(Case([encode_int(P)], tag="inv of p (zero)"))
    for k in (-300, 300, -1, 7):
        cases.append(Case([encode(0, k, (-7.9, 7.9), "alt")], tag="inv of %d p" % k))
    for v in (1 << 380, 1, P - 1):
        cases.append(Case([encode(v, 250, (-7.9, 7.9), "hi")], tag="lazy inv %x" % v))
    return cases


def _check_inv(case, out, what):
    l = out_limbs(out, 0)
    v = residue(case.slots[0].limbs)
    check_carried(case, l, what)
    expect(residue(l) == (pow(v, P - 2, P)), case, "%s: residue" % what)
    expect(-P // 4 < value(l) < 5 * P // 4, case, "%s: value %.3f p" % (what, value(l) / P))


@spec("FQ_INV", _rand_lazy)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _inv_cases(rnd)
    _check_inv(case, out, "inv")


@spec("FQ_INV_FERMAT", lambda rnd: Case([encode(rnd.randrange(P), rnd.randint(0, 2), (0.0, 1.0))], tag="random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [Case([encode(v, k % 3, (0.0, 1.0))], tag="inv %x" % v) for k, v in enumerate(_inv_edges(rnd))] + [
            Case([encode_int(P)], tag="p")]
    _check_inv(case, out, "fq_inv_fermat")


@spec("FQ_INV30", lambda rnd: Case([limbs30(rnd.randrange(P))], tag="random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        # 2^380 needs all 26 rounds of 30 steps, random operands about 18; both kinds share the wave
        return [Case([limbs30(v)], tag="inv30 %x" % v) for v in _inv_edges(rnd)] + [
            Case([limbs30(1 << k)], tag="2^%d" % k) for k in range(181, 381, 11)]
    l = [int(x) for x in out[0][:13]]
    r = sum(x << (30 * i) for i, x in enumerate(l))
    y = sum(x << (30 * i) for i, x in enumerate(case.slots[0].limbs[:13]))
    expect(all(0 <= x < (1 << 30) for x in l[:12]), case, "inv30: limbs")
    expect(-2 * P < r < P, case, "inv30: value %.3f p outside (-2p, p)" % (r / P))
    expect(r % P == (pow(y, P - 2, P)), case, "inv30: residue")


@spec("FQ_LEGENDRE", lambda rnd: Case([encode(rnd.randrange(P), rnd.randint(-2, 2), (-1.0, 1.0), "alt")], tag="random"),
      nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = [Case([encode(v)], tag="%x" % v) for v in fq_edges()]
        cases += [Case([encode(0, k, (-7.9, 7.9), "alt")], tag="zero k=%d" % k) for k in (-300, -1, 1, 300)]
        cases += [Case([encode(rnd.randrange(1, 1 << (k + 1)))], tag="small %d" % k) for k in range(0, 380, 19)]
        return cases
    v = residue(case.slots[0].limbs)
    want = 0 if v == 0 else (1 if pow(v, HALF, P) == 1 else -1)
    expect(flags[0] == want, case, "legendre = %d, want %d" % (flags[0], want))


@spec("FQ_SQRT", lambda rnd: Case([encode(rnd.randrange(P), rnd.randint(0, 2), (0.0, 1.0))], tag="random"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = [Case([encode(v)], tag="%x" % v) for v in fq_edges()]
        cases += [Case([encode(rnd.randrange(P) ** 2 % P, 1, (0.0, 1.0), "hi")], tag="square")]
        return cases
    v = residue(case.slots[0].limbs)
    sq = v == 0 or pow(v, HALF, P) == 1
    expect(flags[0] == int(sq), case, "fq_sqrt ok = %d" % flags[0])
    if sq:
        r, w = residue(out[0]), residue(out[1])
        expect(r * r % P == v, case, "fq_sqrt: root^2 != a")
        expect(v == 0 or r * w % P == 1, case, "fq_sqrt: inv_root")
    check_bounded(case, out, 0, 2, "fq_sqrt", val_bound=2)


# ---- Fq2 ----------------------------------------------------------------------------------------------------------
def f2_operand(rnd, v=None, k=(0, 0), iv=(0.0, 1.0), push=(None, None)):
    v = v if v is not None else (rnd.randrange(P), rnd.randrange(P))
    return [encode(v[0], k[0], iv, push[0]), encode(v[1], k[1], iv, push[1])]


def f2_edges():
    e = fq_edges()
    out = [(v, 0) for v in e[:8]] + [(0, v) for v in e[:8]]
    out += [(v, w) for v, w in zip(e, reversed(e))]
    return out


def f2_val(case, s):
    return (value(case.slots[s].limbs), value(case.slots[s + 1].limbs))


def f2_in(case, s):
    return (residue(case.slots[s].limbs), residue(case.slots[s + 1].limbs))


def _f2_mul_cases(rnd, square):
    cases = []
    e = f2_edges()
    for i, v in enumerate(e):
        w = e[(i * 7 + 3) % len(e)]
        # only one lane holds an edge value: the other coefficient random
        a = f2_operand(rnd, v)
        b = f2_operand(rnd, w)
        cases.append(Case(a + ([] if square else b), tag="edge %s" % (v,)))
    for ba, bb in PRODUCT_PAIRS:
        # the lane pair's column bound is Bx By + Bz Bw <= 8.14: each coefficient product takes half
        ba2, bb2 = ba / 2 ** 0.5, bb / 2 ** 0.5
        if square:
            # c0 = (a0 + a1)(a0 - a1): sums of the two coefficients -> B (2 b)^2 <= 8.14
            ba2 = bb2 = 1.42
        for push in PUSHES:
            for k in (0, 1, -1, 100, -100):
                a = f2_operand(rnd, None, (k, -k), (-ba2, ba2), (push, "alt"))
                b = f2_operand(rnd, None, (-k, k), (-bb2, bb2), ("alt", push))
                cases.append(Case(a + ([] if square else b), tag="lazy k=%d B=%g,%g %s" % (k, ba2, bb2, push)))
    return cases


def _check_f2_mul(case, out, square):
    a0, a1 = f2_val(case, 0)
    if square:
        x0, x1 = (a0 + a1) * (a0 - a1), 2 * a1 * a0
        want = o.f2_sqr(f2_in(case, 0))
    else:
        b0, b1 = f2_val(case, 2)
        x0, x1 = a0 * b0 - a1 * b1, a1 * b0 + a0 * b1
        want = o.f2_mul(f2_in(case, 0), f2_in(case, 2))
    check_product(case, out_limbs(out, 0), x0, "c0")
    check_product(case, out_limbs(out, 1), x1, "c1")
    expect(f2_res(out, 0) == want, case, "fq2 residue")


def _rand_f2(rnd, n=1, iv=(-1.0, 1.0), kmax=2):
    ops = []
    for _ in range(n):
        ops += f2_operand(rnd, None, (rnd.randint(-kmax, kmax), rnd.randint(-kmax, kmax)), iv, (rnd.choice(PUSHES), rnd.choice(PUSHES)))
    return Case(ops, tag="random")


@spec("FQ2_MUL", lambda rnd: _rand_f2(rnd, 2, (-1.4, 1.4)))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_mul_cases(rnd, False)
    _check_f2_mul(case, out, False)


@spec("FQ2_SQR", lambda rnd: _rand_f2(rnd, 1, (-1.4, 1.4)))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_mul_cases(rnd, True)
    _check_f2_mul(case, out, True)


def _f2_lazy_cases(rnd, iv=(-3.9, 3.9), kmax=150):
    cases = [Case(f2_operand(rnd, v), tag="edge %s" % (v,)) for v in f2_edges()]
    for k in (0, 1, -1, kmax, -kmax):
        for push in PUSHES:
            cases.append(Case(f2_operand(rnd, None, (k, -k), iv, (push, "alt")), tag="lazy k=%d %s" % (k, push)))
    return cases


@spec("FQ2_CONJ", lambda rnd: _rand_f2(rnd, 1, (-3.9, 3.9), 100))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_lazy_cases(rnd)
    a0, a1 = case.slots[0].limbs, case.slots[1].limbs
    expect(out_limbs(out, 0) == a0 and out_limbs(out, 1) == [-x for x in a1], case, "conj is not (c0, -c1) limb for limb")


@spec("FQ2_MUL_XI", lambda rnd: _rand_f2(rnd, 1, (-3.9, 3.9), 100))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_lazy_cases(rnd)
    a0, a1 = case.slots[0].limbs, case.slots[1].limbs
    expect(out_limbs(out, 0) == [x - y for x, y in zip(a0, a1)] and out_limbs(out, 1) == [x + y for x, y in zip(a0, a1)],
           case, "mul_xi is not (c0 - c1, c0 + c1) limb for limb")


@spec("FQ2_NORM_FQ", lambda rnd: _rand_f2(rnd, 1, (-2.0, 2.0), 100))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_lazy_cases(rnd, (-2.0, 2.0), 100)
    a0, a1 = f2_in(case, 0)
    l = out_limbs(out, 0)
    expect(residue(l) == (a0 * a0 + a1 * a1) % P, case, "norm_fq residue")
    x0, x1 = f2_val(case, 0)
    t = value(l) * RM - x0 * x0 - x1 * x1
    expect(t % P == 0 and 0 <= t // P < 2 * RM, case, "norm_fq: not a sum of two products")


def _f2_inv_check(case, out, s_in, s_out, what):
    want = o.f2_inv(f2_in(case, s_in)) if f2_in(case, s_in) != (0, 0) else (0, 0)
    expect(f2_res(out, s_out) == want, case, "%s residue" % what)
    check_bounded(case, out, s_out, 2, what, limb=1.0, val_bound=1.25)


@spec("FQ2_INV", lambda rnd: _rand_f2(rnd, 1, (-1.0, 1.0), 2))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = [Case(f2_operand(rnd, v), tag="edge %s" % (v,)) for v in f2_edges()]
        cases += [Case([encode(0, 3, (-1.0, 1.0), "hi"), encode(0, -2, (-1.0, 1.0), "lo")], tag="zero")]
        cases += [Case(f2_operand(rnd, (1 << 380, 0)), tag="2^380"), Case(f2_operand(rnd, (0, 1 << 380)), tag="2^380 u")]
        # norms a0^2 + a1^2 equal to the slow operands of the inverse: (s, 0) with s^2 = v where v is a square
        for v in SLOW_INV:
            if pow(v, HALF, P) == 1:
                cases.append(Case(f2_operand(rnd, (pow(v, (P + 1) // 4, P), 0)), tag="slow norm"))
        return cases
    _f2_inv_check(case, out, 0, 0, "fq2 inv")


def _f2_zero_cases(rnd):
    cases = []
    for k in range(-300, 301, 3):
        a = [encode(0, k, (-7.9, 7.9), PUSHES[k % 4]), encode(0, -k, (-7.9, 7.9), PUSHES[(k + 1) % 4])]
        cases.append(zero_case(a + f2_operand(rnd, (0, 0)), "zero k=%d" % k, [(0, 2), (1, 3)]))
    # one zero coefficient and one non-zero in the same pair, both ways round; near misses k p + 1
    for k in (-300, -1, 0, 1, 300):
        for nz in (1, P - 1, rnd.randrange(P)):
            z = encode(0, k, (-7.9, 7.9), "alt")
            n = encode(nz, 0 if abs(k) == 300 else k, (-7.9, 7.9), "hi")
            cases.append(zero_case([z, n] + f2_operand(rnd, (0, nz)), "(0, x) k=%d" % k, [(0, 2), (1, 3)]))
            cases.append(zero_case([n, z] + f2_operand(rnd, (nz, 0)), "(x, 0) k=%d" % k, [(0, 2), (1, 3)]))
            if abs(k) < 300:
                near = _encode_raw(k * P + 1, (-7.9, 7.9), None)
                cases.append(zero_case([z, near] + f2_operand(rnd, (0, 0)), "(0, kp+1) k=%d" % k, [(0, 2), (1, 3)]))
                cases.append(zero_case([near, z] + f2_operand(rnd, (0, 0)), "(kp+1, 0) k=%d" % k, [(0, 2), (1, 3)]))
    for v in f2_edges()[:24]:
        cases.append(zero_case(f2_operand(rnd, v, (3, -4), (-2.0, 2.0), ("hi", "lo")) + f2_operand(rnd, v, (-5, 6), (-2.0, 2.0), ("lo", "hi")),
                               "eq %s" % (v,), [(0, 2), (1, 3)]))
    return cases


@spec("FQ2_ZERO", lambda rnd: _rand_zero2(rnd), nflags=3)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_zero_cases(rnd)
    flags_agree(case, flags, 3 if case.aux[0] else 2)
    a = f2_in(case, 0)
    z = a == (0, 0)
    expect(flags[0] == int(z), case, "fq2 is_zero = %d" % flags[0])
    mz = _mz(case.slots[0].limbs, 56) & _mz(case.slots[1].limbs, 56)
    expect(flags[1] == mz, case, "maybe_zero56(fq2) = %d, want %d" % (flags[1], mz))
    if z:
        expect(flags[1] == 1, case, "maybe_zero56(fq2) missed a zero")
    if case.aux[0]:
        expect(flags[2] == int(a == f2_in(case, 2)), case, "fq2 == gave %d" % flags[2])


def _rand_zero2(rnd):
    c = _rand_f2(rnd, 2, (-3.0, 3.0), 100)
    return zero_case(c.slots, "random", [(0, 2), (1, 3)])


def _f2_is_square(a):
    if a == (0, 0):
        return True
    n = (a[0] * a[0] + a[1] * a[1]) % P
    return n == 0 or pow(n, HALF, P) == 1


def _f2_sqrt_cases(rnd, n_ops=1):
    vals = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1), (2, 0), (0, 2), (HALF, 0), (0, HALF + 1), (4, 4)]
    vals += [o.f2_sqr((rnd.randrange(P), rnd.randrange(P))) for _ in range(6)]
    vals += [(rnd.randrange(P), rnd.randrange(P)) for _ in range(6)]
    vals += [(o.f2_sqr((rnd.randrange(P), 0))[0], 0), (0, rnd.randrange(P)), (rnd.randrange(P), 0)]
    cases = []
    for i, v in enumerate(vals):
        ops = f2_operand(rnd, v, (i % 2, 0), (NORM_LO, 1.0), ("hi" if i % 3 == 0 else None, None))
        if n_ops == 2:
            ops += f2_operand(rnd, vals[(i * 5 + 1) % len(vals)])
        cases.append(Case(ops, tag="sqrt %s" % (v,)))
    return cases


def _check_f2_root(case, out, s, ok, a, what):
    sq = _f2_is_square(a)
    expect(ok == int(sq), case, "%s: ok = %d, is square %s" % (what, ok, sq))
    if sq:
        expect(o.f2_sqr(f2_res(out, s)) == a, case, "%s: root^2 != a" % what)


@spec("FQ2_SQRT", lambda rnd: Case(f2_operand(rnd, None), tag="random"), nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_sqrt_cases(rnd)
    flags_agree(case, flags, 2)
    a = f2_in(case, 0)
    expect(flags[1] == int(_f2_is_square(a)), case, "fq2_is_square = %d" % flags[1])
    _check_f2_root(case, out, 0, flags[0], a, "fq2_sqrt")


@spec("FQ2_SQRT_X2", lambda rnd: Case(f2_operand(rnd, None) + f2_operand(rnd, o.f2_sqr((rnd.randrange(P), rnd.randrange(P)))),
                                      tag="random"), nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f2_sqrt_cases(rnd, 2)
    flags_agree(case, flags, 2)
    _check_f2_root(case, out, 0, flags[0], f2_in(case, 0), "fq2_sqrt_x2 a")
    _check_f2_root(case, out, 2, flags[1], f2_in(case, 2), "fq2_sqrt_x2 b")


@spec("FQ2_INV_X2", lambda rnd: _rand_f2(rnd, 2, (-1.0, 1.0), 2))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        e = f2_edges()
        return [Case(f2_operand(rnd, v) + f2_operand(rnd, e[(i * 3 + 5) % len(e)]), tag="edge %s" % (v,)) for i, v in enumerate(e)]
    _f2_inv_check(case, out, 0, 0, "fq2_inv_x2 a")
    _f2_inv_check(case, out, 2, 2, "fq2_inv_x2 b")


# ---- Fq6 / Fq12 ---------------------------------------------------------------------------------------------------
TOWER_IV = (-0.01, NORM_HI)  # a normalised coefficient (norm / reduce_value output; the top limb may be negative)


def _tower_operand(rnd, vals, kmax=1):
    ops = []
    for v in vals:
        k = rnd.randint(-kmax, kmax)
        ops.append(encode(v, k, TOWER_IV, rnd.choice(PUSHES)))
    return ops


def _flat6(a):
    return [c for f2 in a for c in f2]


def _flat12(a):
    return _flat6(a[0]) + _flat6(a[1])


def _rand_f12(rnd):
    return tuple(tuple((rnd.randrange(P), rnd.randrange(P)) for _ in range(3)) for _ in range(2))


def _cyclotomic(rnd):
    """An element of the cyclotomic subgroup: f^((p^6 - 1)(p^2 + 1))."""
    f = _rand_f12(rnd)
    g = o.f12_mul(o.f12_conj(f), o.f12_inv(f))
    return o.f12_mul(o.f12_frobenius(g, 2), g)


def _special_f12(rnd):
    z = (0, 0)
    one6 = ((1, 0), z, z)
    zero6 = (z, z, z)
    e = fq_edges()
    return [(one6, zero6), (((e[3], e[4]), z, z), (z, (1, 0), z)),
            (((P - 1, 0), (0, P - 1), (1, 1)), (((1 << 380) % P, 0), z, (HALF, HALF + 1)))]


def _check_tower(case, out, s, want, n, what, limb=NORM_HI, val_bound=VAL_MAX, lo=-0.05):
    got = [residue(out[s + i]) for i in range(n)]
    expect(got == want, case, "%s: residue mismatch" % what)
    check_bounded(case, out, s, n, what, limb=limb, val_bound=val_bound, lo=lo)


def _f6_cases(rnd, nops):
    cases = []
    z = (0, 0)
    specials = [((1, 0), z, z), (z, (1, 0), z), (z, z, (1, 0)), ((P - 1, P - 1), (P - 1, 0), (0, P - 1)),
                (((1 << 380) % P, HALF), (HALF + 1, 1), (2, P - 2))]
    for sp in specials:
        b = tuple((rnd.randrange(P), rnd.randrange(P)) for _ in range(3))
        cases.append(Case(_tower_operand(rnd, _flat6(sp)) + (_tower_operand(rnd, _flat6(b)) if nops == 2 else []), tag="special"))
    return cases


def _rand_f6(rnd, nops, kmax=1):
    ops = []
    for _ in range(nops):
        ops += _tower_operand(rnd, [rnd.randrange(P) for _ in range(6)], kmax)
    return Case(ops, tag="random")


def _f6_of(case, s):
    return tuple(f2_in(case, s + 2 * i) for i in range(3))


def _f12_of(case, s):
    return (_f6_of(case, s), _f6_of(case, s + 6))


@spec("FQ6_MUL", lambda rnd: _rand_f6(rnd, 2))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f6_cases(rnd, 2)
    _check_tower(case, out, 0, _flat6(o.f6_mul(_f6_of(case, 0), _f6_of(case, 6))), 6, "fq6 mul")


@spec("FQ6_SQR", lambda rnd: _rand_f6(rnd, 1))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f6_cases(rnd, 1)
    a = _f6_of(case, 0)
    _check_tower(case, out, 0, _flat6(o.f6_mul(a, a)), 6, "fq6 sqr")


@spec("FQ6_INV", lambda rnd: _rand_f6(rnd, 1))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f6_cases(rnd, 1)
    _check_tower(case, out, 0, _flat6(o.f6_inv(_f6_of(case, 0))), 6, "fq6 inv")


def _f12_cases(rnd, nops, cyclo=False):
    cases = []
    elems = [_cyclotomic(rnd) for _ in range(4)] + ([] if cyclo else _special_f12(rnd))
    for f in elems:
        g = _cyclotomic(rnd) if cyclo else _rand_f12(rnd)
        cases.append(Case(_tower_operand(rnd, _flat12(f)) + (_tower_operand(rnd, _flat12(g)) if nops == 2 else []), tag="special"))
    return cases


def _rand_f12_case(rnd, nops, cyclo=False):
    ops = []
    for _ in range(nops):
        ops += _tower_operand(rnd, _flat12(_cyclotomic(rnd) if cyclo else _rand_f12(rnd)))
    return Case(ops, tag="random")


@spec("FQ12_MUL", lambda rnd: _rand_f12_case(rnd, 2))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f12_cases(rnd, 2)
    _check_tower(case, out, 0, _flat12(o.f12_mul(_f12_of(case, 0), _f12_of(case, 12))), 12, "fq12 mul", val_bound=2.1)


@spec("FQ12_SQR", lambda rnd: _rand_f12_case(rnd, 1))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f12_cases(rnd, 1)
    _check_tower(case, out, 0, _flat12(o.f12_sqr(_f12_of(case, 0))), 12, "fq12 sqr")


@spec("FQ12_INV", lambda rnd: _rand_f12_case(rnd, 1))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f12_cases(rnd, 1)
    _check_tower(case, out, 0, _flat12(o.f12_inv(_f12_of(case, 0))), 12, "fq12 inv", limb=1.01, lo=-1.01)


def _frob_case(rnd, k):
    c = _rand_f12_case(rnd, 1)
    c.aux = [k]
    c.tag = "frobenius %d" % k
    return c


@spec("FQ12_FROB", lambda rnd: _frob_case(rnd, rnd.randint(1, 3)))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = []
        for k in (1, 2, 3):
            for c in _f12_cases(rnd, 1):
                c.aux = [k]
                c.tag = "frobenius %d" % k
                cases.append(c)
        return cases
    _check_tower(case, out, 0, _flat12(o.f12_frobenius(_f12_of(case, 0), case.aux[0])), 12, "fq12 frobenius", limb=1.01, lo=-1.01)


@spec("FQ12_CONJ", lambda rnd: _rand_f12_case(rnd, 1))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f12_cases(rnd, 1)
    _check_tower(case, out, 0, _flat12(o.f12_conj(_f12_of(case, 0))), 12, "fq12 conj", limb=1.01)


def _line_case(rnd, vals, tag):
    return Case(_tower_operand(rnd, vals), tag=tag)


@spec("FQ12_LINE_PRODUCT", lambda rnd: _line_case(rnd, [rnd.randrange(P) for _ in range(12)], "random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        e = fq_edges()
        return [_line_case(rnd, [e[(i * 5 + j) % len(e)] for j in range(12)], "edges %d" % i) for i in range(8)] + [
            _line_case(rnd, [0] * 12, "zero"), _line_case(rnd, [1, 0] * 6, "ones")]
    d0, d1, d4, e0, e1, e4 = (f2_in(case, 2 * i) for i in range(6))
    z = (0, 0)
    want = o.f12_mul(((d0, d1, z), (z, d4, z)), ((e0, e1, z), (z, e4, z)))
    # t2, u are lazy differences of products (limbs in about [-2, 1] 2^28); the rest carried or normalised
    _check_tower(case, out, 0, _flat12(want), 12, "line_product", limb=2.01, lo=-2.01)


@spec("FQ12_CYCLO_SQR", lambda rnd: _rand_f12_case(rnd, 1, True))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _f12_cases(rnd, 1, True) + [Case(_tower_operand(rnd, _flat12(_special_f12(rnd)[0])), tag="one")]
    _check_tower(case, out, 0, _flat12(o.f12_sqr(_f12_of(case, 0))), 12, "cyclotomic_sqr", val_bound=2.1)


def _compressed(f):
    # (z2, z3, z4, z5) = (c1.c0, c0.c2, c0.c1, c1.c2)
    return [f[1][0], f[0][2], f[0][1], f[1][2]]


def _cyclo_chain_case(rnd, fs, tag):
    vals = []
    for f in fs:
        vals += [c for f2 in _compressed(f) for c in f2]
    ops = [encode(v, rnd.randint(0, 1), TOWER_IV, rnd.choice(PUSHES)) for v in vals]
    for op in ops:
        op.val = 2.1 if op.val <= 2 else op.val  # the output bound of reduce_value, the step before
    c = Case(ops, tag=tag)
    c.fs = fs
    return c


@spec("CYCLO_CHAIN", lambda rnd: _cyclo_chain_case(rnd, [_cyclotomic(rnd) for _ in range(3)], "random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        one = _special_f12(rnd)[0]
        return [_cyclo_chain_case(rnd, [one, _cyclotomic(rnd), one], "with the identity"),
                _cyclo_chain_case(rnd, [one, one, one], "identities")]
    for i in range(3):
        want = case.fs[i]  # the full element behind compressed input i
        for _ in range(CYCLO_REDUCE_EVERY):
            want = o.f12_sqr(want)
        _check_tower(case, out, 12 * i, _flat12(want), 12, "cyclo chain %d" % i, limb=1.01)


# ---- points -------------------------------------------------------------------------------------------------------
PT_IV = (NORM_LO, NORM_HI)  # coord_out / coord_norm outputs; values up to ~14 p (the doubling's x3)


class Field:
    def __init__(self, w):
        self.w = w
        self.F = o._Fq if w == 1 else o._Fq2
        self.E = o.E1 if w == 1 else o.E2

    def enc(self, rnd, v, k=None, push=None):
        vs = [v] if self.w == 1 else list(v)
        out = []
        for c in vs:
            kk = rnd.randint(0, 13) if k is None else k
            out.append(encode(c, kk, PT_IV, push or rnd.choice(PUSHES)))
        return out

    def rand(self, rnd):
        return rnd.randrange(1, P) if self.w == 1 else (rnd.randrange(P), rnd.randrange(1, P))

    def dec(self, case, s):
        return residue(case.slots[s].limbs) if self.w == 1 else f2_in(case, s)

    def res(self, out, s):
        return residue(out[s]) if self.w == 1 else f2_res(out, s)

    def jac(self, rnd, pt, lam=None):
        """A point as Jacobian (x l^2, y l^3, l) in lazy limbs; None = infinity (Z a representation k p of zero)."""
        F = self.F
        if pt is None:
            x, y = self.rand(rnd), self.rand(rnd)
            return self.enc(rnd, x) + self.enc(rnd, y) + self.enc(rnd, F.zero)
        lam = lam if lam is not None else self.rand(rnd)
        l2 = F.sqr(lam)
        return self.enc(rnd, F.mul(pt[0], l2)) + self.enc(rnd, F.mul(pt[1], F.mul(l2, lam))) + self.enc(rnd, lam)

    def aff(self, rnd, pt):
        if pt is None:
            return self.enc(rnd, self.F.zero) + self.enc(rnd, self.F.one)
        return self.enc(rnd, pt[0]) + self.enc(rnd, pt[1])

    def jac_to_aff(self, case, out, s):
        F = self.F
        w = self.w
        X, Y, Z = self.res(out, s), self.res(out, s + w), self.res(out, s + 2 * w)
        if F.is_zero(Z):
            return None
        zi = F.inv(Z)
        return (F.mul(X, F.sqr(zi)), F.mul(Y, F.mul(F.sqr(zi), zi)))


G1F, G2F = Field(1), Field(2)


def _pt(fld, rnd, in_group=True):
    return g1_point(rnd, in_group) if fld.w == 1 else g2_point(rnd, in_group)


def _pair_cases(fld, rnd, mixed):
    """(P, Q) pairs at the exceptions of the addition: P = O, Q = O, P = Q, P = -Q, P = +-Q in different lazy
    representations, and Q = 2P / generic pairs."""
    E = fld.E
    out = []
    for _ in range(3):
        p = _pt(fld, rnd)
        q = _pt(fld, rnd)
        out += [(None, q, "P=O"), (p, None, "Q=O"), (p, p, "P=Q"), (p, E.neg(p), "P=-Q"), (p, q, "generic"),
                (p, E.dbl(p), "Q=2P"), (None, None, "P=Q=O")]
    cases = []
    for p, q, tag in out:
        slots = fld.jac(rnd, p) + (fld.aff(rnd, q) if mixed else fld.jac(rnd, q))
        cases.append(Case(slots, aux=[int(q is None)] if mixed else [], tag=tag))
        cases[-1].pts = (p, q)
    return cases


def _rand_pair(fld, rnd, mixed):
    p, q = _pt(fld, rnd), _pt(fld, rnd)
    c = Case(fld.jac(rnd, p) + (fld.aff(rnd, q) if mixed else fld.jac(rnd, q)), aux=[0] if mixed else [], tag="random")
    c.pts = (p, q)
    return c


def _check_point_out(fld, case, out, want, what):
    got = fld.jac_to_aff(case, out, 0)
    expect(got == want, case, "%s: wrong point" % what)
    check_bounded(case, out, 0, 3 * fld.w, what, lo=-0.05)


def _point_specs(prefix, fld):
    def dbl(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            cases = []
            for p in [None, _pt(fld, rnd), _pt(fld, rnd)]:
                for _ in range(2):
                    c = Case(fld.jac(rnd, p), tag="dbl %s" % ("O" if p is None else "P"))
                    c.pts = (p, None)
                    cases.append(c)
            return cases
        _check_point_out(fld, case, out, fld.E.dbl(case.pts[0]), "jac_dbl")

    def rand_dbl(rnd):
        p = _pt(fld, rnd)
        c = Case(fld.jac(rnd, p), tag="random")
        c.pts = (p, None)
        return c

    def add_mixed(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            return _pair_cases(fld, rnd, True)
        _check_point_out(fld, case, out, fld.E.add(*case.pts), "jac_add_mixed")

    def add(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            return _pair_cases(fld, rnd, False)
        _check_point_out(fld, case, out, fld.E.add(*case.pts), "jac_add")

    def generic(mixed):
        def fn(case=None, out=None, flags=None, rnd=None):
            if rnd is not None:
                return _pair_cases(fld, rnd, mixed)
            flags_agree(case, flags, 1)
            p, q = case.pts
            special = p is None or q is None or p[0] == q[0]
            if special:
                expect(flags[0] == 1, case, "the generic addition did not raise its exception flag")
            else:
                expect(flags[0] == 0, case, "exception flag raised for a generic pair")
                _check_point_out(fld, case, out, fld.E.add(p, q), "jac_add_generic")
        return fn

    def to_affine(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            return [dbl_case for dbl_case in dbl(rnd=rnd)]
        flags_agree(case, flags, 1)
        p = case.pts[0]
        expect(flags[0] == int(p is None), case, "to_affine inf flag")
        if p is not None:
            expect((fld.res(out, 0), fld.res(out, fld.w)) == p, case, "to_affine: wrong point")
            check_bounded(case, out, 0, 2 * fld.w, "to_affine", val_bound=1.25)

    def on_curve(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            cases = []
            for p in [None, _pt(fld, rnd), _pt(fld, rnd, False), (fld.rand(rnd), fld.rand(rnd))]:
                c = Case(fld.aff(rnd, p), aux=[int(p is None)], tag="on_curve")
                c.pts = (p, None)
                cases.append(c)
            return cases
        flags_agree(case, flags, 1)
        expect(flags[0] == int(fld.E.on_curve(case.pts[0])), case, "affine_on_curve")

    def rand_on_curve(rnd):
        p = _pt(fld, rnd) if rnd.random() < 0.5 else (fld.rand(rnd), fld.rand(rnd))
        c = Case(fld.aff(rnd, p), aux=[0], tag="random")
        c.pts = (p, None)
        return c

    def subgroup(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            cases = []
            for p in [None, _pt(fld, rnd), _pt(fld, rnd, False), _pt(fld, rnd, False)]:
                c = Case(fld.aff(rnd, p), aux=[int(p is None)], tag="subgroup")
                c.pts = (p, None)
                cases.append(c)
            return cases
        flags_agree(case, flags, 1)
        p = case.pts[0]
        expect(flags[0] == int(fld.E.mul(p, o.R) is None), case, "in_subgroup")

    def rand_subgroup(rnd):
        p = _pt(fld, rnd, rnd.random() < 0.5)
        c = Case(fld.aff(rnd, p), aux=[0], tag="random")
        c.pts = (p, None)
        return c

    spec(prefix + "_DBL", rand_dbl)(dbl)
    spec(prefix + "_ADD_MIXED", lambda rnd: _rand_pair(fld, rnd, True))(add_mixed)
    spec(prefix + "_ADD", lambda rnd: _rand_pair(fld, rnd, False))(add)
    spec(prefix + "_ADD_MIXED_GENERIC", lambda rnd: _rand_pair(fld, rnd, True), nflags=1)(generic(True))
    spec(prefix + "_ADD_GENERIC", lambda rnd: _rand_pair(fld, rnd, False), nflags=1)(generic(False))
    spec(prefix + "_TO_AFFINE", rand_dbl, nflags=1)(to_affine)
    spec(prefix + "_ON_CURVE", rand_on_curve, nflags=1)(on_curve)
    spec(prefix + "_IN_SUBGROUP", rand_subgroup, nflags=1)(subgroup)


_point_specs("G1", G1F)
_point_specs("G2", G2F)


def _x2_case(rnd, p, q, tag):
    c = Case(G2F.jac(rnd, p) + G2F.jac(rnd, q), tag=tag)
    c.pts = (p, q)
    return c


@spec("G2_TO_AFFINE_X2", lambda rnd: _x2_case(rnd, _pt(G2F, rnd), _pt(G2F, rnd), "random"), nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        p = _pt(G2F, rnd)
        return [_x2_case(rnd, None, p, "O, P"), _x2_case(rnd, p, None, "P, O"), _x2_case(rnd, None, None, "O, O"),
                _x2_case(rnd, p, p, "P, P")]
    flags_agree(case, flags, 2)
    for i, p in enumerate(case.pts):
        expect(flags[i] == int(p is None), case, "to_affine_x2 inf flag %d" % i)
        if p is not None:
            expect((G2F.res(out, 4 * i), G2F.res(out, 4 * i + 2)) == p, case, "to_affine_x2: wrong point %d" % i)


def _psi_ref(p):
    # psi(P) = [x] P on G2, x = -|x| (M. Scott's membership test, tc_sqrt.h g2_in_subgroup)
    return o.E2.neg(o.E2.mul(p, o.BLS_X))


@spec("G2_PSI", lambda rnd: _psi_case(rnd, _pt(G2F, rnd)))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_psi_case(rnd, _pt(G2F, rnd)) for _ in range(4)]
    p = case.pts[0]
    expect((G2F.res(out, 0), G2F.res(out, 2)) == _psi_ref(p), case, "g2_psi")


def _psi_case(rnd, p):
    c = Case(G2F.aff(rnd, p), aux=[0], tag="psi")
    c.pts = (p, None)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the scalar block: Fr, the base-|x| and GLV decompositions and their recodings, Lagrange coefficients
# ---------------------------------------------------------------------------------------------------------------------
R = o.R
X = o.BLS_X  # |x|
X2 = X * X
RF = 1 << 256  # Montgomery R of Fr
RF_INV = pow(RF, -1, R)
M64 = (1 << 64) - 1
X_RECIP = ((1 << 128) - 1) // X - (1 << 64)  # tc_constants.h BLS_X_RECIP
COFACTOR_FIX = pow(3 * (X2 - 1), -1, R)  # tc_constants.h FR_COFACTOR_FIX: (3 (x^2 - 1))^-1 mod r
LAYOUTS = {}  # op -> (path of a case, {path: random case of that path}): the wave layout of ops with per-wave decisions


def u32s(x, n=8):
    """x as n little-endian u32 words (a scalar: 8; n = NL pads it to a whole slot)."""
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def u64_words(vals):
    return [w for v in vals for w in u32s(v, 2)]


def out_words(out):
    return [int(x) & 0xffffffff for x in np.asarray(out).reshape(-1)]


def out_int(out, w0, nw):
    ws = out_words(out)[w0:w0 + nw]
    return sum(w << (32 * i) for i, w in enumerate(ws))


def out_u64(out, k):
    return out_int(out, 2 * k, 2)


def scase(words, aux=(), tag="", **kw):
    c = Case(raw_words(words), aux=aux, tag=tag)
    c.__dict__.update(kw)
    return c


def fr_edges():
    """Where carries and reductions turn in 8 x u32: 0, 1, 2, r-1, r-2, (r +- 1)/2, 2^k and r - 2^k around every word
    boundary, 2^254, R mod r, R^-1, R^2 mod r."""
    e = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, RF % R, RF_INV, RF * RF % R, 1 << 254, R - (1 << 254)]
    for m in range(0, 256, 32):
        for k in (m - 1, m, m + 1):
            if 0 <= k < 255:
                e += [(1 << k) % R, (R - (1 << k)) % R]
    out = []
    for v in e:
        if v not in out:
            out.append(v)
    return out


def _check_fr(case, out, want, what):
    got = out_int(out, 0, 8)
    expect(got < R, case, "%s: not canonical (%x)" % (what, got))
    expect(got == want % R, case, "%s: %x != %x" % (what, got, want % R))


# ---- Fr arithmetic: Montgomery words in, Montgomery words out -------------------------------------------------------
def _fr_pair_cases(rnd):
    cases = []
    e = fr_edges()
    for a in e:
        partners = rnd.sample(e, 4) + [(R - a) % R, a, (a + 1) % R, (R - 1 - a) % R]
        for b in partners:
            cases.append(scase(u32s(a, NL) + u32s(b), tag="%x, %x" % (a, b), a=a, b=b))
    return cases


def _rand_fr_pair(rnd):
    a, b = rnd.randrange(R), rnd.randrange(R)
    return scase(u32s(a, NL) + u32s(b), tag="random", a=a, b=b)


def _fr_unary_cases(rnd):
    return [scase(u32s(a), tag="%x" % a, a=a) for a in fr_edges()]


def _rand_fr(rnd):
    a = rnd.randrange(R)
    return scase(u32s(a), tag="random", a=a)


@spec("FR_ADD", _rand_fr_pair)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_pair_cases(rnd)
    _check_fr(case, out, case.a + case.b, "a + b")


@spec("FR_SUB", _rand_fr_pair)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_pair_cases(rnd)
    _check_fr(case, out, case.a - case.b, "a - b")


@spec("FR_MUL", _rand_fr_pair)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_pair_cases(rnd)
    _check_fr(case, out, case.a * case.b * RF_INV, "a b / R")


@spec("FR_SQR", _rand_fr)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_unary_cases(rnd)
    _check_fr(case, out, case.a * case.a * RF_INV, "a^2 / R")


@spec("FR_INV", _rand_fr)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_unary_cases(rnd)
    # residue a / R -> its inverse, in Montgomery form: R^2 / a  (0 -> 0)
    _check_fr(case, out, pow(case.a, -1, R) * RF * RF if case.a else 0, "inv")


@spec("FR_FROM_CANONICAL", _rand_fr)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_unary_cases(rnd)
    _check_fr(case, out, case.a * RF, "from_canonical")


@spec("FR_TO_CANONICAL", _rand_fr)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fr_unary_cases(rnd)
    _check_fr(case, out, case.a * RF_INV, "to_canonical")


def _u64_edges():
    e = [0, 1, 2, M64, M64 - 1, 1 << 63, (1 << 63) - 1]
    for k in (31, 32, 33, 62, 63):
        e += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    return sorted(set(x for x in e if 0 <= x <= M64))


@spec("FR_FROM_U64", lambda rnd: (lambda a: scase(u32s(a, 2), tag="random", a=a))(rnd.getrandbits(64)))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [scase(u32s(a, 2), tag="%x" % a, a=a) for a in _u64_edges()]
    _check_fr(case, out, case.a * RF, "fr_from_u64")


def _le32_cases():
    vs = [0, 1, R - 1, R, R + 1, R - 2, (1 << 255) - 1, (1 << 256) - 1, 1 << 255, 1 << 254]
    for i in range(8):  # r with one word moved by one, both ways (where the word does not wrap)
        w = u32s(R)
        for d in (-1, 1):
            if 0 <= w[i] + d <= 0xffffffff:
                vs.append(R + d * (1 << (32 * i)))
    return [scase(u32s(v), tag="%x" % v, a=v) for v in vs]


def _rand_le32(rnd):
    a = rnd.choice([rnd.randrange(R), rnd.randrange(R, 1 << 256), R + rnd.randrange(-(1 << 64), 1 << 64)])
    return scase(u32s(a), tag="random", a=a)


@spec("FR_FROM_LE32", _rand_le32, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _le32_cases()
    expect(flags[0] == int(case.a < R), case, "fr_from_le32 accepts %d" % flags[0])
    expect(out_int(out, 0, 8) == case.a, case, "fr_from_le32: words")


@spec("FR_SCALE_COFACTOR_FIX", _rand_le32)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _le32_cases() + [scase(u32s(v), tag="%x" % v, a=v) for v in fr_edges()]
    got = out_int(out, 0, 8)
    if case.a >= R:
        expect(got == (1 << 256) - 1, case, "non-canonical input: not all ones")
    else:
        expect(got == case.a * COFACTOR_FIX % R, case, "k c mod r")


# ---- the base-|x| division and decompositions ----------------------------------------------------------------------
def div_by_x_abs_model(u1, u0):
    """tc_gls.h div_by_x_abs step by step: (quotient, remainder, first correction taken, second correction taken).

    The second correction (r >= |x|) cannot fire for this |x|.  With v = floor((2^128 - 1) / |x|) - 2^64 the estimate
    q = v u1 + u1 2^64 + u0 satisfies  U / |x| - q / 2^64 = u0 (2^64 - |x|) / (|x| 2^64) + u1 / (|x| 2^64) + u1 e / 2^64
    (U = u1 2^64 + u0, e = the fraction dropped from (2^128 - 1) / |x|), which is below 0.39 for u1 < |x|, u0 < 2^64
    (div_second_correction_bound).  So floor(U / |x|) <= floor(q / 2^64) + 1 = q1: the candidate remainder is U - q1 |x|
    or U - (q1 - 1) |x| < |x|, and after the first correction it is always below |x|."""
    q = (X_RECIP * u1 + ((u1 << 64) | u0)) & ((1 << 128) - 1)
    q1 = ((q >> 64) + 1) & M64
    q0 = q & M64
    r = (u0 - q1 * X) & M64
    c1 = r > q0
    if c1:
        q1 = (q1 - 1) & M64
        r = (r + X) & M64
    c2 = r >= X
    if c2:
        q1 = (q1 + 1) & M64
        r -= X
    return q1, r, c1, c2


def div_second_correction_bound():
    """The largest U / |x| - q / 2^64 over u1 < |x|, u0 < 2^64 (see div_by_x_abs_model), exactly."""
    from fractions import Fraction
    B = 1 << 64
    e = Fraction(B * B - 1, X) - (B + X_RECIP)
    return Fraction((B - 1) * (B - X), X * B) + Fraction(X - 1, X * B) + Fraction(X - 1, B) * e


def _div_cases(rnd):
    u1s = [0, 1, 2, X - 1, X - 2, X // 2, X >> 16, (1 << 63) - 1, 1 << 63]
    u0s = [0, 1, 2, M64, M64 - 1, X - 1, X, X + 1, (1 << 63), 2 * X - (1 << 64) if 2 * X > 1 << 64 else 0]
    cases = [(a, b) for a in u1s for b in u0s if a < X]
    # quotients and remainders at their ends: U = q |x| + rem
    for q in [0, 1, 2, M64, M64 - 1, 1 << 63, (1 << 63) + 1, 1 << 32]:
        for rem in [0, 1, X - 1, X - 2, X // 2]:
            U = q * X + rem
            if U >> 64 < X:
                cases.append((U >> 64, U & M64))
    return [scase(u64_words([a, b]), tag="u1=%x u0=%x" % (a, b), u1=a, u0=b) for a, b in cases]


def _rand_div(rnd):
    a, b = rnd.randrange(X), rnd.getrandbits(64)
    return scase(u64_words([a, b]), tag="random", u1=a, u0=b)


@spec("DIV_BY_X_ABS", _rand_div)
def _(case=None, out=None, flags=None, rnd=None):
    """(u1 : u0) / |x| for u1 < |x|, against divmod.  The table holds divisions that take no correction and ones that
    take the first (r > q0); the second (r >= |x|) cannot fire for this |x| (div_by_x_abs_model)."""
    if rnd is not None:
        return _div_cases(rnd)
    q, rem = divmod((case.u1 << 64) | case.u0, X)
    expect((out_u64(out, 0), out_u64(out, 1)) == (q, rem), case, "div_by_x_abs: (%x, %x) != (%x, %x)" % (
        out_u64(out, 0), out_u64(out, 1), q, rem))


def _gls_edges(rnd):
    """tests/test_hostsim.py's edge list of gls_decompose."""
    ks = [0, 1, X - 1, X, X + 1, X2 - 1, X2, X ** 3 - 1, X ** 3, R - 1, R - 2, (1 << 255) - 19, (1 << 64) - 1, 1 << 64,
          (1 << 128) - 1, 1 << 128, (X - 1) * (1 + X + X2 + X ** 3) % (X ** 4)]
    ks += [(rnd.getrandbits(64) * X + rnd.choice([0, 1, X - 1])) % R for _ in range(20)]
    return ks


def _check_digits(case, out, k, what):
    d = [out_u64(out, j) for j in range(4)]
    expect(all(x < X for x in d[:3]), case, "%s: digit >= |x|: %s" % (what, [hex(x) for x in d]))
    expect(sum(x * X ** j for j, x in enumerate(d)) == k, case, "%s: sum d_i |x|^i != %x" % (what, k))


def _rand_k(rnd):
    k = rnd.randrange(R)
    return scase(u32s(k), tag="random", k=k)


@spec("GLS_DECOMPOSE", _rand_k)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [scase(u32s(k), tag="%x" % k, k=k) for k in _gls_edges(rnd) if k < X ** 4]
    _check_digits(case, out, case.k, "gls_decompose")


@spec("GLS_DECOMPOSE_ODD", _rand_k, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [scase(u32s(k), tag="%x" % k, k=k) for k in _gls_edges(rnd) if k < R]
    flip = case.k % 2 == 0
    expect(flags[0] == int(flip), case, "gls_decompose_odd: flip flag")
    _check_digits(case, out, R - case.k if flip else case.k, "gls_decompose_odd")


def _sac_cases(rnd):
    cases = []
    for nb in (64, 32, 16):
        top = (1 << nb) - 1
        vals = [0, 1, 2, top, top - 1, 1 << (nb - 1), (1 << (nb - 1)) - 1] + ([X - 1, X - 2] if nb == 64 else [])
        for d0 in vals:
            for rest in ([top, top, top], [0, 0, 0], [1, top, 0], [top - 1, 1, 1 << (nb - 1)]):
                cases.append(_sac_case([d0] + rest, nb, "d0=%x %s" % (d0, rest)))
        for _ in range(6):
            cases.append(_sac_case([rnd.choice(vals)] + [rnd.choice(vals + [rnd.getrandbits(nb)]) for _ in range(3)], nb, "mixed"))
    return cases


def _sac_case(d, nb, tag):
    return scase(u64_words(d), aux=[nb], tag="nbits=%d %s" % (nb, tag), d=d, nbits=nb)


def _rand_sac(rnd):
    nb = rnd.choice([64, 32, 16])
    return _sac_case([rnd.getrandbits(nb) for _ in range(4)], nb, "random")


@spec("SAC_RECODE4", _rand_sac, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """d0 | 1 = sum_{i < n} s_i 2^i + 2^n and d_j = sum_{i < n} s_i u_j[i] 2^i + top_j 2^n (s_i = -1 where neg has bit i)."""
    if rnd is not None:
        return _sac_cases(rnd)
    n, d = case.nbits, case.d
    neg = out_u64(out, 0)
    u = [out_u64(out, j) for j in (1, 2, 3)]
    s = [-1 if (neg >> i) & 1 else 1 for i in range(n)]
    expect(flags[1] == int(d[0] % 2 == 0), case, "sac_recode4: fix != (d0 even)")
    expect(sum(s[i] << i for i in range(n)) + (1 << n) == d[0] | 1, case, "sac_recode4: the signs do not give d0 | 1")
    for j in range(3):
        expect(u[j] >> n == 0, case, "sac_recode4: u_%d has bits above nbits" % (j + 1))
        topj = (int(flags[0]) >> j) & 1
        rec = sum(s[i] * ((u[j] >> i) & 1) << i for i in range(n)) + (topj << n)
        expect(rec == d[j + 1], case, "sac_recode4: d_%d = %x, recoded %x" % (j + 1, d[j + 1], rec))
    expect(flags[0] >> 3 == 0, case, "sac_recode4: top has bits above 2")


def _g1_edges(rnd):
    """tests/test_hostsim.py's edge list of the base-4 G1 ladder."""
    return [0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, R - 1, R - 2, R - 3, R - 4, X2 - 2, X2 - 1, X2, X2 + 1, X2 + 2, 2 * X2, 3 * X2,
            3 * X2 + 3, X2 * X2 % R, (1 << 128) - 1, 1 << 128, (1 << 128) + 1, 1 << 127, (1 << 127) - 1, X, X + 1, X - 1,
            (R - 1) // 2, (R + 1) // 2, R - X2, R - X2 - 1, R - X2 + 1]


@spec("GLV_DECOMPOSE", _rand_k)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [scase(u32s(k), tag="%x" % k, k=k) for k in _g1_edges(rnd) + _gls_edges(rnd) if k < R]
    k1, k2 = out_int(out, 0, 4), out_int(out, 4, 4)
    expect(k1 < X2 and k2 < X2, case, "glv_decompose: half >= x^2")
    expect(k1 + k2 * X2 == case.k, case, "glv_decompose: k1 + k2 x^2 != k")


def _glv_prime(k):
    flip = k % 2 == 0
    return flip, (R - k if flip else k)


def _check_glv_columns(case, k1, k2, kp, ncol, what):
    expect(k1 % 2 == 1, case, "%s: k1 even" % what)
    expect(k1 + k2 * X2 == kp, case, "%s: k1 + k2 x^2 != k' (= %x)" % (what, kp))
    if ncol == 128:
        expect((k1, k2) == (kp % X2, kp // X2), case, "%s: not the decomposition k' = (k' mod x^2) + (k' div x^2) x^2" % what)


@spec("GLV_RECODE_SIGN_ALIGNED", _rand_k, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """k1 = sum_{i < 128} s_i 2^i + 2^128 and k2 = sum_{i < 128} s_i u_i 2^i + top 2^128 (the 129 columns)."""
    if rnd is not None:
        return [scase(u32s(k), tag="%x" % k, k=k) for k in _g1_edges(rnd) + [R]]
    flip, kp = _glv_prime(case.k)
    expect(flags[0] == int(flip), case, "glv_recode_sign_aligned: flip")
    neg, u = out_int(out, 0, 4), out_int(out, 4, 4)
    k1 = sum((-1 if (neg >> i) & 1 else 1) << i for i in range(128)) + (1 << 128)
    k2 = sum((-1 if (neg >> i) & 1 else 1) * ((u >> i) & 1) << i for i in range(128)) + (int(flags[1]) << 128)
    _check_glv_columns(case, k1, k2, kp, 128, "glv_recode_sign_aligned")


def _msm_short(k1, k2, nb, tag):
    k = k1 + k2 * X2
    return scase(u32s(k), aux=[nb], tag="nbits=%d %s" % (nb, tag), k=k, nbits=nb)


def _msm_cases(rnd):
    cases = [scase(u32s(k), aux=[128], tag="nbits=128 %x" % k, k=k, nbits=128) for k in _g1_edges(rnd) + [R]]
    for nb in (32, 16):
        top = (1 << nb) - 1
        for k1, k2, tag in [(1, 0, "1"), (top, top, "all ones"), (top, 0, "k2 = 0"), (1, top, "k1 = 1"),
                            (2, 5, "k1 even"), (0, 1, "k1 = 0"), (top - 1, top, "k1 even, long"), ((1 << nb) + 1, 3, "k1 of nbits + 1 bits"),
                            (3, 1 << nb, "k2 of nbits + 1 bits"), ((1 << nb) + 1, 1 << nb, "both nbits + 1 bits"),
                            (1 << (nb - 1) | 1, 1 << (nb - 1), "top bits")]:
            cases.append(_msm_short(k1, k2, nb, tag))
        cases += [scase(u32s(k), aux=[nb], tag="nbits=%d full %x" % (nb, k), k=k, nbits=nb) for k in (R - 1, R - 2, X2 * X2 % R)]
    return cases


def _rand_msm(rnd):
    nb = rnd.choice([128, 32, 16])
    if nb == 128:
        k = rnd.randrange(R)
        return scase(u32s(k), aux=[128], tag="random", k=k, nbits=128)
    return _msm_short(rnd.getrandbits(nb) | 1, rnd.getrandbits(nb), nb, "random")


@spec("MSM_G1_RECODE", _rand_msm, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """The column codes decoded back to k1 and k2 (column c: bits 0, 1 = u_{2c}, u_{2c+1}; bit 2: s_{2c} = s_{2c+1}; bit 3:
    s_{2c+1} = -1), the starting entry (0: P, 3: P + phi') included."""
    if rnd is not None:
        return _msm_cases(rnd)
    n = case.nbits
    nc = n // 2
    codes = out_words(out)[:65]
    expect(all(c == 0xee for c in codes[nc + 1:]), case, "msm_g1_recode: codes written past column %d" % nc)
    k1, k2 = 1 << n, 0
    expect(codes[nc] in (0, 3), case, "msm_g1_recode: starting entry %d" % codes[nc])
    if codes[nc] == 3:
        k2 += 1 << n
    for c in range(nc):
        code = codes[c]
        expect(code < 16, case, "msm_g1_recode: code %x" % code)
        s1 = -1 if code & 8 else 1
        s0 = s1 if code & 4 else -s1
        k1 += (s0 << (2 * c)) + (s1 << (2 * c + 1))
        k2 += (s0 * (code & 1) << (2 * c)) + (s1 * ((code >> 1) & 1) << (2 * c + 1))
    if n == 128:
        flip, kp = _glv_prime(case.k)
        expect(flags[0] == int(flip) and flags[1] == 1, case, "msm_g1_recode: flip / fits")
        _check_glv_columns(case, k1, k2, kp, 128, "msm_g1_recode")
        return
    h1, h2 = case.k % X2, case.k // X2
    fits = h1 % 2 == 1 and h1 >> n == 0 and h2 >> n == 0
    expect(flags[0] == 0, case, "msm_g1_recode: short mode flipped")
    expect(flags[1] == int(fits), case, "msm_g1_recode: fits = %d" % flags[1])
    expect((k1, k2) == ((h1, h2) if fits else (1, 0)), case, "msm_g1_recode: codes give (%x, %x)" % (k1, k2))


# ---- Lagrange coefficients -----------------------------------------------------------------------------------------
_LAGRANGE_REF = {}


def lagrange_ref(ids):
    key = tuple(ids)
    if key not in _LAGRANGE_REF:
        _LAGRANGE_REF[key] = o.lagrange_coeffs(len(ids) - 1, [o.into_fr_plus_1(i) for i in ids])
    return _LAGRANGE_REF[key]


def _chunk_bits(ids):
    """True when lagrange_denominator closes a 64-bit chunk for some i (the product of the |differences| it has gathered
    would leave 64 bits)."""
    for i, vi in enumerate(ids):
        chunk = 1
        for vj in ids:
            m = abs(vj - vi) or 1
            if chunk.bit_length() + m.bit_length() > 64:
                return True
            chunk *= m
    return False


def lagrange_index_sets(rnd):
    """t = 0; t = 67 over range(200); repeated indices; 0, 2^63, 2^64 - 1; random 33- and 64-bit indices; and sets where a
    running chunk of lagrange_denominator and the next difference have bit lengths that sum to exactly 64 (no close), and
    to exactly 65 with a true product >= 2^64 (the chunk must close)."""
    a, b = 2 ** 32 - 1, 2 ** 32 + 5
    sets = [[5], [0], [M64], sorted(rnd.sample(range(200), 68)), rnd.sample(range(200), 68), [5, 9, 5, 7, 9, 11, 2, 40, 41],
            [3, 3], [0, 1 << 63, M64, 1, 3, 9, 27], [M64, 0], [M64 - 1, M64, 0, 1 << 63],
            [rnd.getrandbits(33) for _ in range(12)] + [7, 7], [rnd.getrandbits(64) for _ in range(10)],
            # (i = 0: the differences are the other indices themselves)
            [0, a, a],                       # a repeated difference (factor 1 for the equal pair)
            [0, a, M64 - a],                 # 32 + 64 bits
            [0, a, 2 ** 32 - 2],             # 32 + 32 = 64 bits: the chunk stays open, the product < 2^64
            [0, b, a],                       # 33 + 32 = 65 bits, product >= 2^64: the chunk must close
            [0, a, b],                       # 32 + 33 = 65, the other order
            [0, 2 ** 40 + 1, 2 ** 24 + 2 ** 23],  # 41 + 25 = 66
            [0, 2 ** 40 + 3, 2 ** 24 - 1],   # 41 + 24 = 65, product >= 2^64
            [0, 2 ** 40 + 3, 2 ** 23 + 1],   # 41 + 24 = 65, product < 2^64
            [10, 10 + b, 10 - 9, 10 + a], list(range(10)), [rnd.randrange(70000) for _ in range(40)]]
    return [s for s in sets if len(s) <= CONF_MAX_N]


def _idx_case(ids, aux, tag, **kw):
    return scase(u64_words(ids), aux=aux, tag=tag, ids=list(ids), **kw)


def _rand_ids(rnd, big=None):
    n = rnd.randint(1, 6)
    big = rnd.random() < 0.5 if big is None else big
    return [rnd.getrandbits(64) if big else rnd.randrange(300) for _ in range(n)]


def _coeff_case(ids, i, tag):
    return _idx_case(ids, [len(ids) - 1, i], "%s i=%d" % (tag, i), i=i)


@spec("LAGRANGE_COEFF", lambda rnd: (lambda ids: _coeff_case(ids, rnd.randrange(len(ids)), "random"))(_rand_ids(rnd)), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_coeff_case(ids, i, "set %d" % k) for k, ids in enumerate(lagrange_index_sets(rnd)) for i in range(len(ids))]
    expect(flags[0] == 0, case, "lagrange_coeff_at_zero: status %d" % flags[0])
    expect(out_int(out, 0, 8) == lagrange_ref(case.ids)[case.i], case, "lagrange_coeff_at_zero")


def _fr_abscissae(rnd):
    return [[rnd.randrange(R) for _ in range(4)], [R - 1, R - 2, 5, 1 << 64], [R - 1, 0, 1, 2], [3, 3, 9, 11], [0, 1, 2, 3],
            [rnd.randrange(R) for _ in range(9)], [R - (1 << 63), 1 << 63, 7], [R - 1], [R - 1, R - 1, 4],
            sorted(rnd.sample(range(200), 68))]


def _fr_coeff_case(xs, i, tag):
    c = scase([w for x in xs for w in u32s(x)], aux=[len(xs) - 1, i], tag="%s i=%d" % (tag, i), i=i)
    c.ids = list(xs)
    return c


@spec("LAGRANGE_COEFF_FR", lambda rnd: (lambda xs: _fr_coeff_case(xs, rnd.randrange(len(xs)), "random"))(
    [rnd.randrange(R) for _ in range(rnd.randint(1, 6))]), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_fr_coeff_case(xs, i, "set %d" % k) for k, xs in enumerate(_fr_abscissae(rnd)) for i in range(len(xs))]
    expect(flags[0] == 1, case, "lagrange_coeff_at_zero_fr: refused")
    expect(out_int(out, 0, 8) == lagrange_ref(case.ids)[case.i], case, "lagrange_coeff_at_zero_fr")


def _lagrange_all(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_idx_case(ids, [len(ids) - 1], "set %d" % k) for k, ids in enumerate(lagrange_index_sets(rnd))]
    expect(flags[0] == 0, case, "status %d" % flags[0])
    n = len(case.ids)
    got = [out_int(out, 8 * i, 8) for i in range(n)]
    want = lagrange_ref(case.ids)
    bad = [i for i in range(n) if got[i] != want[i]]
    expect(not bad, case, "coefficients %s wrong" % bad[:8])


def _lagrange_path(case):
    return "chunks" if _chunk_bits(case.ids) else "one chunk"


def _lagrange_random_of_path(path):
    def make(rnd):
        ids = _rand_ids(rnd, big=path == "chunks")
        if path == "chunks":
            ids += [rnd.getrandbits(64) for _ in range(2)]
        return _idx_case(ids, [len(ids) - 1], "random %s" % path)
    return make


for _name in ("LAGRANGE_ALL", "LAGRANGE_SPLIT"):
    spec(_name, lambda rnd: _idx_case(*(lambda ids: (ids, [len(ids) - 1], "random"))(_rand_ids(rnd))), nflags=1)(_lagrange_all)
    LAYOUTS[_name] = (_lagrange_path, {p: _lagrange_random_of_path(p) for p in ("one chunk", "chunks")})


# ---- the small-index fast path -------------------------------------------------------------------------------------
def small_coeffs_model(ids):
    """tc_threshold.h lagrange_small_coeffs step by step, with its overflow tests: (c_abs, c_neg, D) or None."""
    if any(i >= 65535 for i in ids):
        return None
    K = len(ids)
    x = [i + 1 for i in ids]
    den, den_neg = [], []
    for i in range(K):
        d = 1
        for j in range(K):
            if j == i:
                continue
            if x[j] == x[i]:
                return None
            d *= x[j] - x[i]
            if not -(1 << 63) <= d < 1 << 63:
                return None
        den_neg.append(d < 0)
        den.append(abs(d))
    D = 1
    for i in range(K):
        D = D // math.gcd(D, den[i]) * den[i]
        if D >> 62:
            return None
    c = []
    for i in range(K):
        v = D // den[i]
        for j in range(K):
            if j != i:
                v *= x[j]
                if v >> 64:
                    return None
        if v >> 63:
            return None
        c.append(v)
    g = D
    for v in c:
        g = math.gcd(g, v)
    return [v // g for v in c], den_neg, D // g


def small_index_sets(rnd):
    sets = [list(s) for K in (2, 3, 4) for s in itertools.combinations(range(10), K)]
    sets += [[65534, 3, 9, 11], [65535, 3, 9, 11], [3, 65535], [65534, 0], [65533, 65534], [0, 65534, 1, 65533],
             [60000, 61000, 62000, 63000], [4, 4, 6, 8], [7, 7], [1, 2, 1], [0, 1, 2, 65535], [2 ** 40, 1, 2, 3],
             [M64, 0, 1], [0, 30000, 65000, 1], [0, 1, 65533, 65534], [0, 20000, 40000, 60000], [1, 2, 64000, 65000]]
    return sets


def _small_case(ids, tag):
    return _idx_case(ids, [len(ids)], tag)


def _class_case(ids, tag):
    return _idx_case(ids, [len(ids) - 1], tag)


def _small_path(case):
    if any(i >= 65535 for i in case.ids):
        return "index"
    return "fast" if small_coeffs_model(case.ids) else "late"


def _small_random_of_path(path):
    def make(rnd):
        K = rnd.choice([2, 3, 4])
        if path == "index":
            ids = [rnd.randrange(65535, 1 << 64) if k == 0 else rnd.randrange(100) for k in range(K)]
            rnd.shuffle(ids)
        elif path == "fast":
            ids = rnd.sample(range(rnd.choice([12, 300, 5000])), K)
        else:
            ids = rnd.sample(range(200), K - 1)
            ids.append(rnd.choice(ids))
        return _small_case(ids, "random %s" % path)
    return make


@spec("LAGRANGE_SMALL_COEFFS", lambda rnd: _small_random_of_path(rnd.choice(["fast", "index", "late"]))(rnd), nflags=3)
def _(case=None, out=None, flags=None, rnd=None):
    """Returns false exactly where the model does (an index >= 65535, a repeated index, an overflow); when true,
    lambda_i = +-c_i / D (mod r) for every i, D < 2^62, and no common factor is left in the c_i and D."""
    if rnd is not None:
        return [_small_case(ids, "%s" % ids) for ids in small_index_sets(rnd)]
    K = len(case.ids)
    m = small_coeffs_model(case.ids)
    expect(flags[0] == int(m is not None), case, "lagrange_small_coeffs returned %d" % flags[0])
    if m is None:
        return
    c_abs = [out_u64(out, k) for k in range(K)]
    D = out_u64(out, 4)
    c_neg = [(flags[2] >> k) & 1 for k in range(K)]
    expect(flags[1] == 0, case, "d_neg set")
    expect((c_abs, [int(v) for v in m[1]], D) == (m[0], [int(v) for v in m[1]], m[2]), case,
           "c = %s %s, D = %d; model %s" % (c_abs, c_neg, D, m))
    expect(0 < D < 1 << 62, case, "D = %d" % D)
    g = D
    for v in c_abs:
        g = math.gcd(g, v)
    expect(g == 1, case, "common factor %d left" % g)
    lam = lagrange_ref(case.ids)
    for i in range(K):
        expect(lam[i] * D % R == (-c_abs[i] if c_neg[i] else c_abs[i]) % R, case, "lambda_%d != +-c_%d / D" % (i, i))


def _class_ref(ids, t):
    if not 1 <= t <= 3:
        return 0, False
    m = small_coeffs_model(ids[:t + 1])
    if m is None:
        return 0, False
    D = m[2]
    return (1 if D == 1 else 2 if D & (D - 1) == 0 and D <= 1 << 16 else 0), True


def _class_random_of_path(path):
    return lambda rnd: (lambda c: _class_case(c.ids, c.tag))(_small_random_of_path(path)(rnd))


@spec("COMBINE_CLASS", lambda rnd: _class_random_of_path(rnd.choice(["fast", "index", "late"]))(rnd), nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """combine_job_class / combine_small_applies: D = 1 -> 1, D = 2^a (a <= 16) -> 2, everything else -> 0 (generic)."""
    if rnd is not None:
        cases = [_class_case(ids, "%s" % ids) for ids in small_index_sets(rnd)]
        cases += [_idx_case([0, 1], [0], "t = 0"), _idx_case([0, 1, 2, 3], [4], "t = 4"), _idx_case([0, 1], [1], "D = 1"),
                  _idx_case([0, 2], [1], "D = 2"), _idx_case([0, 1 << 15], [1], "D = 2^15"), _idx_case([0, 1 << 16], [1], "D = 2^16"),
                  _idx_case([5, 5 + (1 << 16)], [1], "D = 2^16 (shifted)"), _idx_case([0, 3], [1], "D = 3")]
        return cases
    t = case.aux[0]
    cls, applies = _class_ref(case.ids, t)
    expect((flags[0], flags[1]) == (cls, int(applies)), case, "class %d applies %d, want %d %d" % (flags[0], flags[1], cls, applies))


def _inv_small_case(d, neg, tag=""):
    return scase(u32s(d, 2), aux=[int(neg)], tag="%s%d %s" % ("-" if neg else "", d, tag), d=d, neg=neg)


def _inv_small_path(case):
    return "word" if case.d < 1 << 32 else "bit"


def _inv_small_random_of_path(path):
    def make(rnd):
        d = rnd.randrange(2, 1 << 32) if path == "word" else rnd.randrange(1 << 32, 1 << 63)
        return _inv_small_case(d, rnd.random() < 0.5, "random")
    return make


@spec("FR_INVERSE_OF_SMALL", lambda rnd: _inv_small_random_of_path(rnd.choice(["word", "bit"]))(rnd))
def _(case=None, out=None, flags=None, rnd=None):
    """(+-D)^-1 mod r, 0 < D < 2^63.  The 32-bit word path runs only when every lane of the wave has D < 2^32."""
    if rnd is not None:
        ds = [1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 62 - 1, 2 ** 62, 2 ** 63 - 1, 2 ** 63 - 25, 65521, 4294967291,
              2 ** 61 - 1, 1000000007, 999999999989, 6, 255, 1 << 16, 3 ** 39]
        return [_inv_small_case(d, neg) for d in ds for neg in (False, True)]
    want = pow(-case.d if case.neg else case.d, -1, R)
    _check_fr(case, out, want, "fr_inverse_of_small")


LAYOUTS["FR_INVERSE_OF_SMALL"] = (_inv_small_path, {p: _inv_small_random_of_path(p) for p in ("word", "bit")})


def _fib(n):
    a, b = 0, 1
    for _ in range(n):
        a, b = b, a + b
    return a


def _gcd_case(a, b, tag):
    return scase(u64_words([a, b]), tag="%s (%x, %x)" % (tag, a, b), a=a, b=b)


def _gcd_steps(a, b):
    n = 0
    while b:
        a, b = b, a % b
        n += 1
    return n


def _gcd_path(case):
    return _gcd_steps(case.a, case.b)


def _gcd_random_of_path(steps):
    def make(rnd):
        if steps == 0:
            return _gcd_case(rnd.getrandbits(64), 0, "b = 0")
        # (F_{n+1} m, F_n m) takes n - 1 Euclid steps for every multiplier m
        n = steps + 1
        m = rnd.randrange(1, M64 // _fib(n + 1))
        return _gcd_case(_fib(n + 1) * m, _fib(n) * m, "fibonacci multiple")
    return make


@spec("GCD_U64", lambda rnd: _gcd_case(rnd.getrandbits(64), rnd.getrandbits(rnd.choice([8, 32, 64])), "random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        F = [_fib(n) for n in range(95) if _fib(n) <= M64]
        cases = [_gcd_case(0, 0, "zeros"), _gcd_case(0, 7, "a = 0"), _gcd_case(7, 0, "b = 0"), _gcd_case(M64, 0, "b = 0"),
                 _gcd_case(0, M64, "a = 0"), _gcd_case(M64, M64, "equal"), _gcd_case(12, 12, "equal"), _gcd_case(1, M64, "1"),
                 _gcd_case(M64, M64 - 1, "consecutive"), _gcd_case(1 << 63, 1 << 62, "powers of two")]
        cases += [_gcd_case(F[n + 1], F[n], "fibonacci") for n in range(len(F) - 1)]
        cases += [_gcd_case(F[n], F[n + 1], "fibonacci, swapped") for n in range(len(F) - 3, len(F) - 1)]
        return cases
    got = out_u64(out, 0)
    expect(got == math.gcd(case.a, case.b), case, "gcd_u64 = %x" % got)


# a wave where no lane enters the loop, and one where every lane runs 59 steps (on different values)
LAYOUTS["GCD_U64"] = (_gcd_path, {p: _gcd_random_of_path(p) for p in (0, 59)})
LAYOUTS["LAGRANGE_SMALL_COEFFS"] = (_small_path, {p: _small_random_of_path(p) for p in ("fast", "index", "late")})
LAYOUTS["COMBINE_CLASS"] = (_small_path, {p: _class_random_of_path(p) for p in ("fast", "index")})


# ---------------------------------------------------------------------------------------------------------------------
# the pairing: Miller steps and loops, the cyclotomic exponentiation, the final exponentiation, the check
# ---------------------------------------------------------------------------------------------------------------------
# A check's operands (conformance.h conf_g1 / conf_g2): G1 point k at slots 6 k, 6 k + 1, G2 point k at 6 k + 2 .. 6 k + 5,
# aux = (P0 at infinity, Q0 at infinity, P1 at infinity, Q1 at infinity).  A point at infinity travels as (0, 1).
BTW = o.f2_scale(o.XI, 4)  # the twist constant b' = 4 (1 + u)
F2Z, F2O = o.F2_ZERO, o.F2_ONE
# The Miller point T = (X : Y : zt) (tc_pairing.h: homogeneous, third coordinate doubled; affine (2 X / zt, 2 Y / zt)).
# Its declared interval is what the step functions leave in it (coord norm() outputs), so that consecutive steps compose.
MPT_IV, MPT_VAL = (NORM_LO, NORM_HI), 16
# The Miller loop's output contract (the operand of the final exponentiation): normalised limbs, |value| <= MF_VAL p.
MF_IV, MF_VAL = (NORM_LO, NORM_HI), 8
# The final exponentiation's output: the operand of "== Fq12::one()" (Fq2 ==: a difference inside the zero filter).
FE_LIMB, FE_VAL = 1.01, 2.1


def _line014(d0, d1, d4):
    """d0 + d1 v + d4 v w as an Fq12 (the sparse line of mul_by_014)."""
    return ((d0, d1, F2Z), (F2Z, d4, F2Z))


def dev_doubling_step(T):
    """tc_pairing.h miller_doubling_step on residues: (T', (c0, c1, c2))."""
    X, Y, Z = T
    B, C = o.f2_sqr(Y), o.f2_sqr(Z)
    E = o.f2_scale(o.f2_mul_xi(C), 3)
    F = o.f2_scale(E, 3)
    XY = o.f2_mul(X, Y)
    H = o.f2_sub(o.f2_sub(o.f2_sqr(o.f2_add(Y, Z)), B), C)
    J = o.f2_sqr(X)
    line = (H, o.f2_neg(o.f2_scale(J, 6)), o.f2_scale(o.f2_sub(B, E), 2))
    X3 = o.f2_scale(o.f2_mul(XY, o.f2_sub(B, F)), 2)
    Y3 = o.f2_sub(o.f2_sqr(o.f2_add(B, F)), o.f2_scale(o.f2_sqr(E), 12))
    Z3 = o.f2_scale(o.f2_mul(B, H), 4)
    return (X3, Y3, Z3), line


def dev_addition_step(T, q):
    """tc_pairing.h miller_addition_step on residues."""
    X, Y, Z = T
    X2, Y2 = o.f2_scale(X, 2), o.f2_scale(Y, 2)
    theta = o.f2_sub(Y2, o.f2_mul(q[1], Z))
    lam = o.f2_sub(X2, o.f2_mul(q[0], Z))
    C, D = o.f2_sqr(theta), o.f2_sqr(lam)
    E = o.f2_mul(lam, D)
    F = o.f2_mul(Z, C)
    G = o.f2_mul(X2, D)
    Hh = o.f2_sub(o.f2_add(E, F), o.f2_scale(G, 2))
    line = (lam, o.f2_neg(theta), o.f2_sub(o.f2_mul(theta, q[0]), o.f2_mul(lam, q[1])))
    X3 = o.f2_mul(lam, Hh)
    Y3 = o.f2_sub(o.f2_mul(theta, o.f2_sub(G, Hh)), o.f2_mul(E, Y2))
    Z3 = o.f2_scale(o.f2_mul(Z, E), 2)
    return (X3, Y3, Z3), line


def miller_affine(T):
    X, Y, Z = T
    zi = o.f2_inv(Z)
    return (o.f2_scale(o.f2_mul(X, zi), 2), o.f2_scale(o.f2_mul(Y, zi), 2))


def dev_scaled_lines(P, Qp):
    """The 68 lines of one pair as the product evaluates them, (c2, c1 xP, c0 yP); the unit line for a skipped pair."""
    if P is None or Qp is None:
        return [(F2O, F2Z, F2Z)] * 68
    T = (Qp[0], Qp[1], (2, 0))
    out = []

    def step(line):
        c0, c1, c2 = line
        out.append((c2, o.f2_scale(c1, P[0]), o.f2_scale(c0, P[1])))
    for bit in bin(X >> 1)[3:]:
        T, line = dev_doubling_step(T)
        step(line)
        if bit == "1":
            T, line = dev_addition_step(T, Qp)
            step(line)
    T, line = dev_doubling_step(T)
    step(line)
    return out


def oracle_scaled_lines(P, Qp):
    """The oracle's (g2_prepare) lines of one pair scaled at P, in the same (d0, d1, d4) order; unit lines if skipped."""
    if P is None or Qp is None:
        return [(F2O, F2Z, F2Z)] * 68
    return [(c2, o.f2_scale(c1, P[0]), o.f2_scale(c0, P[1])) for c0, c1, c2 in o.g2_prepare(Qp)]


def line_product5(d, e):
    """The five coefficients (a0, a1, a2, b1, b2) of (d0 + d1 v + d4 v w)(e0 + e1 v + e4 v w), as the rows hold them."""
    m = o.f12_mul(_line014(*d), _line014(*e))
    assert m[1][0] == F2Z
    return [m[0][0], m[0][1], m[0][2], m[1][1], m[1][2]]


def dev_miller_loop(pairs):
    """The product Miller loop of tc_pairing.h miller_loop<2> on residues: the same lines, line products and squarings
    (miller_prepare_lines + miller_accumulate and q_miller_loop compute the same value)."""
    lines = [dev_scaled_lines(P, Qp) for P, Qp in pairs]
    f = o.F12_ONE
    s = 0
    for bit in bin(X >> 1)[3:]:
        for _ in range(2 if bit == "1" else 1):
            for ls in lines:
                f = o.f12_mul(f, _line014(*ls[s]))
            s += 1
        f = o.f12_sqr(f)
    for ls in lines:
        f = o.f12_mul(f, _line014(*ls[s]))
    return o.f12_conj(f)


def f12_is_fq2(f):
    """f lies in Fq2 (every coefficient but c0.c0 zero)."""
    return f[0][1] == F2Z and f[0][2] == F2Z and f[1] == o.F6_ZERO


def f2_multiple(a, b):
    """a = mu b for some NONZERO mu in Fq2 (a, b: tuples of Fq2 values, b not all zero)."""
    k = next((i for i, v in enumerate(b) if v != F2Z), None)
    if k is None or a[k] == F2Z:
        return False
    mu = o.f2_mul(a[k], o.f2_inv(b[k]))
    return all(x == o.f2_mul(mu, y) for x, y in zip(a, b))


_REF = {}


def cached(kind, key, fn):
    """Each reference once per process (the GPU leg checks every table at four launch sizes)."""
    k = (kind, key)
    if k not in _REF:
        _REF[k] = fn()
    return _REF[k]


def g1_slots(P, neg_y=False):
    """A G1 operand as the decoder leaves it: canonical coordinates; neg_y: (x, -y) with -y the limb-wise negation of y,
    as pairing_check forms its second G1 operand (not normalised)."""
    if P is None:
        return [encode(0), encode(1)]
    y = encode(P[1])
    if neg_y:
        y = Operand([-x for x in y.limbs], -y.hi, -y.lo, y.val)
        check_input(y)
    return [encode(P[0]), y]


def g2_slots(Q):
    if Q is None:
        return [encode(0), encode(0), encode(1), encode(0)]
    return [encode(Q[0][0]), encode(Q[0][1]), encode(Q[1][0]), encode(Q[1][1])]


def check_case(pts, tag, neg1=False):
    """pts = (P0, Q0, P1, Q1).  neg1: P1's y given as the raw negation of the canonical y of -P1 (the oracle sees P1)."""
    P0, Q0, P1, Q1 = pts
    slots = g1_slots(P0) + g2_slots(Q0) + g1_slots(P1 if not neg1 or P1 is None else o.E1.neg(P1), neg1) + g2_slots(Q1)
    c = Case(slots, aux=[int(P0 is None), int(Q0 is None), int(P1 is None), int(Q1 is None)], tag=tag)
    c.pts = pts
    return c


def _skip_of(pts):
    return (pts[0] is None or pts[1] is None, pts[2] is None or pts[3] is None)


def loop_pairs(rnd):
    """Operand sets of the Miller loops: every skip pattern (either operand of pair 0, of pair 1, of both at infinity),
    P1 = -P0 with Q1 = Q0 (a trivial product pairing whose f is not 1), Q1 = psi(Q0), the generators, P next to -P
    (canonical y and p - y), and the negated y of pairing_check's second operand."""
    g1, g2 = (lambda: g1_point(rnd)), (lambda: g2_point(rnd))
    out = []
    for p0, p1 in [(True, True), (False, True), (True, False), (False, False)]:
        for which in ("P", "Q", "PQ"):
            a, b = g1(), g2()
            c, d = g1(), g2()
            if not p0:
                a = None if "P" in which else a
                b = None if "Q" in which else b
            if not p1:
                c = None if "P" in which else c
                d = None if "Q" in which else d
            if p0 and p1 and which != "P":
                continue
            out.append(((a, b, c, d), "skip %s%s %s" % ("" if p0 else "0", "" if p1 else "1", which), False))
    a, b = g1(), g2()
    out.append(((a, b, o.E1.neg(a), b), "P1 = -P0, Q1 = Q0", False))
    out.append(((a, b, g1(), _psi_ref(b)), "Q1 = psi(Q0)", False))
    out.append(((o.G1_GEN, o.G2_GEN, o.G1_GEN, o.G2_GEN), "generators", False))
    out.append(((o.G1_GEN, o.G2_GEN, o.E1.neg(o.G1_GEN), o.E2.neg(o.G2_GEN)), "-generators", False))
    out.append(((a, b, o.E1.neg(a), g2()), "P, -P", False))
    out.append(((a, b, a, b), "P1 = P0 negated as pairing_check does", True))
    out.append(((a, b, g1(), g2()), "negated c.y", True))
    return out


def _rand_loop_case(rnd):
    return check_case((g1_point(rnd), g2_point(rnd), g1_point(rnd), g2_point(rnd)), "random", rnd.random() < 0.3)


def _loop_cases(rnd):
    return [check_case(pts, tag, neg) for pts, tag, neg in loop_pairs(rnd)]


def _dev_ml(case):
    return cached("dev_ml", case.pts, lambda: dev_miller_loop([(case.pts[0], case.pts[1]), (case.pts[2], case.pts[3])]))


def _oracle_ml(case):
    return cached("o_ml", case.pts, lambda: o.miller_loop([(case.pts[0], case.pts[1]), (case.pts[2], case.pts[3])]))


def _check_miller_value(case, out, what):
    """f: the product's own Miller value exactly (dev_miller_loop), nonzero, an Fq2 multiple of the oracle's -- the
    lines differ from pairing 0.16's only by Fq2 factors (projective scalings by powers of the Miller points' Fq2
    coordinates), a factor the final exponentiation removes; no wider subfield: Fq2 is where those factors live --, and
    exactly 1 when both pairs are skipped.  Coefficients inside the Miller-output contract."""
    f = f12_res(out, 0)
    expect(f != ((F2Z,) * 3, (F2Z,) * 3), case, "%s: f = 0" % what)
    expect(f == _dev_ml(case), case, "%s: not the product's Miller value" % what)
    ratio = o.f12_mul(f, o.f12_inv(_oracle_ml(case)))
    expect(f12_is_fq2(ratio), case, "%s: f / oracle is not in Fq2" % what)
    if all(_skip_of(case.pts)):
        expect(f == o.F12_ONE, case, "%s: both pairs skipped, f != 1" % what)
    check_bounded(case, out, 0, 12, what, limb=MF_IV[1], val_bound=MF_VAL, lo=MF_IV[0])


@spec("MILLER_LOOP2", _rand_loop_case)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _loop_cases(rnd)
    _check_miller_value(case, out, "miller_loop<2>")


@spec("Q_MILLER_LOOP", _rand_loop_case)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _loop_cases(rnd)
    _check_miller_value(case, out, "q_miller_loop")


ROW_FIRST, ROW_PRODUCTS, MILLER_ROW_SLOTS = 8, 8 + 3 * 68, 8 + 3 * 68 + 68 * 5  # tc_pairing.h kRowFirst, ...


def _row(rows, k):
    return (residue(rows[k][0]), residue(rows[k][1]))


@spec("MILLER_LINES", _rand_loop_case)
def _(case=None, out=None, flags=None, rnd=None, rows=None):
    """The prepared form: f as MILLER_LOOP2; every parked first-pair line an Fq2 multiple of the oracle's line of that
    step at P0; every step's five product coefficients one Fq2 multiple of the product of the two oracle lines (a
    skipped pair: the unit line, and the product rows of a check with both pairs skipped exactly (1, 0, 0, 0, 0))."""
    if rnd is not None:
        return _loop_cases(rnd)
    _check_miller_value(case, out, "miller_prepare_lines + miller_accumulate")
    P0, Q0, P1, Q1 = case.pts
    l0 = cached("o_lines", (P0, Q0), lambda: oracle_scaled_lines(P0, Q0))
    l1 = cached("o_lines", (P1, Q1), lambda: oracle_scaled_lines(P1, Q1))
    skip = _skip_of(case.pts)
    for s in range(68):
        e = tuple(_row(rows, ROW_FIRST + 3 * s + i) for i in range(3))
        if skip[0]:
            expect(e == (F2O, F2Z, F2Z), case, "step %d: the skipped first pair's line is not the unit" % s)
        else:
            expect(f2_multiple(e, l0[s]), case, "step %d: parked line is not an Fq2 multiple of the oracle's" % s)
        prod = tuple(_row(rows, ROW_PRODUCTS + 5 * s + i) for i in range(5))
        want = line_product5(l0[s], l1[s])
        if all(skip):
            expect(prod == tuple(want), case, "step %d: product rows of an empty check are not 1" % s)
        else:
            expect(f2_multiple(prod, want), case, "step %d: product rows are not one Fq2 multiple of the oracle's" % s)
    for k, (pt, co) in enumerate([(P0, 0), (P0, 1), (P1, 0), (P1, 1)]):
        slot = (0 if co == 0 else 2) + (k >= 2)
        if pt is not None:
            expect(_row(rows, slot)[0] == pt[co], case, "row %d does not hold the G1 operand" % slot)


def _check_bit(case, flags, nlanes):
    want = cached("o_check", case.pts, lambda: int(o.pairing_check(*case.pts)))
    got = [flags[4 * l] for l in range(nlanes)]
    expect(all(g == want for g in got), case, "pairing check %s, oracle %d" % (got, want))


def check_relations(rnd):
    """True and false relations: e([s]P, Q) = e(P, [s]Q) and the same against s + 1; a or c at infinity; all four at
    infinity (true); the same pair on both sides (true)."""
    out = []
    for _ in range(2):
        s = rnd.randrange(1, R)
        p, q = g1_point(rnd), g2_point(rnd)
        sp, sq, s1q = o.E1.mul(p, s), o.E2.mul(q, s), o.E2.mul(q, s + 1)
        out += [((sp, q, p, sq), "[s]P, Q vs P, [s]Q"), ((sp, q, p, s1q), "[s]P, Q vs P, [s+1]Q"),
                ((None, q, p, sq), "a = O"), ((sp, q, None, sq), "c = O"), ((None, q, None, sq), "a = c = O"),
                ((p, q, p, q), "same pair"), ((p, None, p, q), "b = O"), ((p, q, o.E1.neg(p), o.E2.neg(q)), "-P, -Q")]
    out.append(((None, None, None, None), "all at infinity"))
    return [check_case(pts, tag) for pts, tag in out]


def _rand_check(rnd):
    s = rnd.randrange(1, R)
    p, q = g1_point(rnd), g2_point(rnd)
    return check_case((o.E1.mul(p, s), q, p, o.E2.mul(q, s + (rnd.random() < 0.5))), "random")


@spec("PAIRING_CHECK", _rand_check, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return check_relations(rnd)
    _check_bit(case, flags, 2)


@spec("Q_PAIRING_CHECK", _rand_check, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return check_relations(rnd)
    _check_bit(case, flags, 4)


# ---- the Miller steps -----------------------------------------------------------------------------------------------
def _enc_f2(v, k, iv, push):
    return [encode(v[0], k[0], iv, push[0]), encode(v[1], k[1], iv, push[1])]


def miller_point_slots(rnd, T, kind):
    """T = (X, Y, zt) residues in lazy limbs: kind "canonical", "hi" / "lo" / "alt" (every limb at that end of MPT_IV, the
    value at k = MPT_VAL - 1 or -MPT_VAL + 1), or "random"."""
    out = []
    for v in T:
        if kind == "canonical":
            out += _enc_f2(v, (0, 0), (0.0, 1.0), (None, None))
        elif kind == "random":
            out += _enc_f2(v, (rnd.randint(0, MPT_VAL - 1), rnd.randint(0, MPT_VAL - 1)), MPT_IV,
                           (rnd.choice(PUSHES), rnd.choice(PUSHES)))
        else:
            k = MPT_VAL - 1 if kind == "hi" else 0 if kind == "alt" else -1
            out += _enc_f2(v, (k, k), MPT_IV, (kind, kind))
    return out


def _lambdas(rnd):
    """Projective factors of T: random, 2 (zt = 2: the first step), 1, -1, u, 2^380, p - 1 + u, R^-1 (Montgomery form 1)."""
    return [("random", (rnd.randrange(P), rnd.randrange(P))), ("2", (2, 0)), ("1", (1, 0)), ("-1", (P - 1, 0)),
            ("u", (0, 1)), ("2^380", (1 << 380, 0)), ("p-1+u", (P - 1, 1)), ("R^-1", (RINV, RINV))]


def miller_T(pt, lam):
    """(lam x / 2 : lam y / 2 : lam) for the affine pt."""
    h = o.f2_scale(lam, (P + 1) // 2)
    return (o.f2_mul(pt[0], h), o.f2_mul(pt[1], h), lam)


def _step_case(rnd, pt, lam, kind, q, tag):
    T = miller_T(pt, lam)
    slots = miller_point_slots(rnd, T, kind) + (g2_slots(q) if q is not None else [])
    c = Case(slots, tag="%s %s" % (tag, kind))
    c.T, c.q = T, q
    return c


def _step_cases(rnd, add):
    cases = []
    for name, lam in _lambdas(rnd):
        for kind in ("canonical", "hi", "lo", "alt", "random"):
            pt = g2_point(rnd)
            q = g2_point(rnd) if add else None
            cases.append(_step_case(rnd, pt, lam, kind, q, "lambda %s" % name))
    # the first steps of a real loop: T = Q (zt = 2), then the points the loop reaches
    q = g2_point(rnd)
    T = (q[0], q[1], (2, 0))
    for s in range(6):
        T, _ = dev_doubling_step(T)
        c = Case(miller_point_slots(rnd, T, "random") + (g2_slots(q) if add else []), tag="loop point %d" % s)
        c.T, c.q = T, q if add else None
        cases.append(c)
    return cases


def _rand_step(rnd, add):
    return _step_case(rnd, g2_point(rnd), (rnd.randrange(P), rnd.randrange(P)), rnd.choice(("random", "hi", "lo")),
                      g2_point(rnd) if add else None, "random")


def _check_step(case, out, add):
    T2 = tuple(f2_res(out, 2 * i) for i in range(3))
    line = tuple(f2_res(out, 6 + 2 * i) for i in range(3))
    x, y = miller_affine(case.T)
    if add:
        x2, y2 = case.q
        want_pt = o.E2.add((x, y), case.q)
        dx, dy = o.f2_sub(x, x2), o.f2_sub(y, y2)
        want_line = (dx, o.f2_neg(dy), o.f2_sub(o.f2_mul(dy, x2), o.f2_mul(dx, y2)))
    else:
        want_pt = o.E2.dbl((x, y))
        want_line = (o.f2_scale(y, 2), o.f2_neg(o.f2_scale(o.f2_sqr(x), 3)), o.f2_sub(o.f2_sqr(y), o.f2_scale(BTW, 3)))
    expect(T2[2] != F2Z and miller_affine(T2) == want_pt, case, "T' is not the affine %s" % ("T + Q" if add else "2T"))
    expect(f2_multiple(line, want_line), case, "the line is not an Fq2 multiple of the reference line")
    # T' inside the interval declared for T: the next step takes it as it is
    check_bounded(case, out, 0, 6, "T'", limb=MPT_IV[1], val_bound=MPT_VAL, lo=MPT_IV[0])
    # the line goes into scale() by a canonical G1 coordinate (a product: limb bound <= PRODUCT_MAX) and into the line
    # products: limbs of -6 J (the doubling's c1) down to -6 2^28, values up to |2 X| + |x2 zt| (the addition's lambda)
    check_bounded(case, out, 6, 6, "line", limb=1.01, val_bound=2 * MPT_VAL + 2, lo=-6.01)


@spec("MILLER_DBL_STEP", lambda rnd: _rand_step(rnd, False))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _step_cases(rnd, False)
    _check_step(case, out, False)


@spec("MILLER_ADD_STEP", lambda rnd: _rand_step(rnd, True))
def _(case=None, out=None, flags=None, rnd=None):
    """T + Q for T != +-Q: T = +-Q is out of contract (for subgroup points the loop's T = [k] Q with 1 < k < r - 1)."""
    if rnd is not None:
        return _step_cases(rnd, True)
    _check_step(case, out, True)


# ---- the cyclotomic exponentiation and the final exponentiation -------------------------------------------------------
def f12_slots(rnd, f, k=None, iv=TOWER_IV, val=None):
    """An Fq12 in 12 slots: k None (random k in {0, 1}, random pushes) or an int (every coefficient v + k p, limbs pushed
    to alternating ends of iv)."""
    ops = []
    for i, v in enumerate(_flat12(f)):
        if k is None:
            ops.append(encode(v, rnd.randint(0, 1), iv, rnd.choice(PUSHES)))
        else:
            ops.append(encode(v, k, iv, ("hi", "lo", "alt")[i % 3]))
    return ops


def _cyclo_case(rnd, f, tag, k=None):
    c = Case(f12_slots(rnd, f, k), tag=tag)
    c.f = f
    return c


def _cyclo_elements(rnd):
    """Cyclotomic elements: 1, a random one and its conjugate, the easy part of a real Miller value and its Frobenius image.  (The z2 = 0, z3 != 0 branch of cyclotomic_decompress3 is
    still unexercised: no construction of a cyclotomic element with c1.c0 = 0 and c0.c2 != 0 is known here.)"""
    one = o.F12_ONE
    g = _cyclotomic(rnd)
    ml = o.miller_loop([(g1_point(rnd), g2_point(rnd))])
    e = _easy_part(ml)
    return [("one", one), ("random", g), ("conj", o.f12_conj(g)), ("easy part of a Miller value", e),
            ("frobenius", o.f12_frobenius(e, 1)), ("square of one", o.f12_sqr(one))]


def _easy_part(f):
    r = o.f12_mul(o.f12_conj(f), o.f12_inv(f))
    return o.f12_mul(o.f12_frobenius(r, 2), r)


def _expx_cases(rnd):
    cases = []
    for tag, f in _cyclo_elements(rnd):
        cases.append(_cyclo_case(rnd, f, tag))
        cases.append(_cyclo_case(rnd, f, tag + " k = 1", 1))
    return cases


def _expx_spec(name, e):
    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            return _expx_cases(rnd)
        want = cached("expx", (case.f, e), lambda: o.f12_conj(o.f12_pow(case.f, e)))
        _check_tower(case, out, 0, _flat12(want), 12, name, limb=FE_LIMB, val_bound=FE_VAL, lo=-FE_LIMB)
    spec(name, lambda rnd: _cyclo_case(rnd, _cyclotomic(rnd), "random"))(fn)


_expx_spec("CYCLO_EXP_BY_X", X)
_expx_spec("CYCLO_EXP_BY_X_HALF", X >> 1)
_expx_spec("Q_EXP_BY_X", X)
_expx_spec("Q_EXP_BY_X_HALF", X >> 1)


def _fe_case(rnd, f, tag, k=None, cube=False):
    """f at the Miller-output contract: k None (canonical), or every coefficient v + k p with limbs pushed to the ends of
    MF_IV."""
    if k is None:
        ops = [encode(v) for v in _flat12(f)]
    else:
        ops = [encode(v, k, MF_IV, ("hi", "lo", "alt")[i % 3]) for i, v in enumerate(_flat12(f))]
    c = Case(ops, tag=tag)
    c.f, c.cube = f, cube
    return c


def _fe_cases(rnd):
    z6 = o.F6_ZERO
    r6 = tuple((rnd.randrange(P), rnd.randrange(P)) for _ in range(3))
    ml = o.miller_loop([(g1_point(rnd), g2_point(rnd))])
    a, b = g1_point(rnd), g2_point(rnd)
    ml_trivial = dev_miller_loop([(a, b), (o.E1.neg(a), b)])
    fs = [("1", o.F12_ONE), ("-1", ((o.f2_neg(F2O), F2Z, F2Z), z6)), ("in Fq2", (((rnd.randrange(P), rnd.randrange(P)), F2Z, F2Z), z6)),
          ("in Fq", (((rnd.randrange(P), 0), F2Z, F2Z), z6)), ("in Fq6", (r6, z6)), ("c1 w", (z6, r6)),
          ("oracle Miller value", ml), ("product Miller value, P1 = -P0", ml_trivial),
          ("product Miller value", dev_miller_loop([(g1_point(rnd), g2_point(rnd)), (g1_point(rnd), g2_point(rnd))]))]
    cases = []
    for i, (tag, f) in enumerate(fs):
        cases.append(_fe_case(rnd, f, tag, cube=i in (6, 8)))
        for k in (MF_VAL - 1, 1):
            cases.append(_fe_case(rnd, f, "%s, v + %d p" % (tag, k), k))
    return cases


def _check_fe(case, out, flags, nlanes, what):
    want = cached("fe", case.f, lambda: o.final_exponentiation_chain(case.f))
    got = f12_res(out, 0)
    expect(got == want, case, "%s: not the oracle's chain" % what)
    if case.cube:  # the factor 3 of the source comment
        plain = cached("fe_plain", case.f, lambda: o.final_exponentiation(case.f))
        expect(got == o.f12_mul(plain, o.f12_sqr(plain)), case, "%s: not the pairing cubed" % what)
    check_bounded(case, out, 0, 12, what, limb=FE_LIMB, val_bound=FE_VAL, lo=-FE_LIMB)
    is_one = [flags[4 * l] for l in range(nlanes)]
    expect(all(v == int(want == o.F12_ONE) for v in is_one), case, "%s: == 1 gave %s" % (what, is_one))


def _rand_fe(rnd):
    return _fe_case(rnd, _rand_f12(rnd), "random", rnd.choice([None, 1, MF_VAL - 1]))


@spec("FINAL_EXP", _rand_fe, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fe_cases(rnd)
    _check_fe(case, out, flags, 2, "final_exponentiation")


@spec("Q_FINAL_EXP", _rand_fe, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return _fe_cases(rnd)
    _check_fe(case, out, flags, 4, "q_final_exponentiation")


# ---------------------------------------------------------------------------------------------------------------------
# the point-multiplication block: table builders, ladders, GLS / GLV, cofactor clearing, Straus, the [1 / D] step
# ---------------------------------------------------------------------------------------------------------------------
H1, H2 = o.H1, o.H2
SMALL_ORDERS = {1: (3, 11, 10177, 859267, 52437899), 2: (13, 23, 2713, 11953, 262069)}  # small prime factors of the cofactors
assert all(H1 % l == 0 for l in SMALL_ORDERS[1]) and all(H2 % l == 0 for l in SMALL_ORDERS[2])
PSI_CX = o.f2_inv(o.f2_pow(o.XI, (P - 1) // 3))  # tc_constants.h PSI_CX / PSI_CY
PSI_CY = o.f2_inv(o.f2_pow(o.XI, (P - 1) // 2))
COFACTOR_FIX_SHORT = (X + 1) // 3  # tc_constants.h G2_COFACTOR_FIX_SHORT
CLEAR_NOFIX = 3 * (X2 - 1) * H2  # g2_clear_cofactor(fix = false) = [3 (x^2 - 1) h2] P


def psi(p):
    """psi on ALL of E'(Fq2) (untwist, Frobenius, twist); on G2 it is [x] (_psi_ref)."""
    return None if p is None else (o.f2_mul(o.f2_conj(p[0]), PSI_CX), o.f2_mul(o.f2_conj(p[1]), PSI_CY))


def curve_point(fld, rnd):
    """A point of the curve outside the order-r subgroup."""
    return _pt(fld, rnd, False)


def small_order_point(fld, rnd, l):
    """A point of prime order l (l a factor of the cofactor): a random point's l-primary part, brought down to order l."""
    n = (H1 if fld.w == 1 else H2) * R
    while n % l == 0:
        n //= l
    while True:
        p = fld.E.mul(curve_point(fld, rnd), n)
        while p is not None and fld.E.mul(p, l) is not None:
            p = fld.E.mul(p, l)
        if p is not None:
            return p


_SMALL = {}


def small_points(fld):
    """One point of every small order (cached), and for G1 the order-3 points (0, +-2)."""
    if fld.w not in _SMALL:
        rnd = random.Random("small-%d" % fld.w)
        pts = [small_order_point(fld, rnd, l) for l in SMALL_ORDERS[fld.w]]
        if fld.w == 1:
            pts += [(0, 2), (0, P - 2)]
        _SMALL[fld.w] = pts
    return _SMALL[fld.w]


def whole_curve_points(fld, rnd):
    """Operands of the routines defined on the whole curve: infinity, subgroup, outside it, small order."""
    return [None, _pt(fld, rnd), curve_point(fld, rnd), curve_point(fld, rnd)] + small_points(fld)


def aff_slots(fld, rnd, pt, canon=False):
    """An affine operand: canonical (a decoded point) or lazy inside the coordinate contract (values up to 2 p + v, what
    products and table loads hand on); infinity as (0, 1) with its flag in aux."""
    pt = pt if pt is not None else (fld.F.zero, fld.F.one)
    cs = [pt[0], pt[1]] if fld.w == 1 else list(pt[0]) + list(pt[1])
    if canon:
        return [encode(c) for c in cs]
    return [encode(c, rnd.randint(0, 2), PT_IV, rnd.choice(PUSHES)) for c in cs]


def inf_mask(pts):
    return sum(1 << i for i, p in enumerate(pts) if p is None)


def mcase(slots, words=(), aux=(), tag="", **kw):
    c = Case(list(slots) + (raw_words(list(words)) if words else []), aux=aux, tag=tag)
    c.__dict__.update(kw)
    return c


def check_result(fld, case, out, flags, want, what):
    """The Jacobian result (slot 0 on) is `want` as residues -- Z = 0 exactly when want is infinity --, and jac_to_affine of it
    (slot 3w on) is want's coordinates inside the normalised-coordinate contract, with the infinity bit in flag 0."""
    w = fld.w
    flags_agree(case, flags, 1)
    expect(fld.jac_to_aff(case, out, 0) == want, case, "%s: wrong point" % what)
    check_bounded(case, out, 0, 3 * w, what + " (Jacobian)")
    expect(flags[0] == int(want is None), case, "%s: infinity flag %d" % (what, flags[0]))
    if want is not None:
        expect((fld.res(out, 3 * w), fld.res(out, 4 * w)) == want, case, "%s: wrong affine point" % what)
        check_bounded(case, out, 3 * w, 2 * w, what + " (affine)", val_bound=1.25)


# ---- the path models: a ladder's columns walked on the oracle's group law -------------------------------------------------
def _walk_add(E, acc, e):
    """acc (Jacobian, the oracle's) + e (affine or None): the sum, and whether the branch-free generic addition cannot do
    it (an operand at infinity, or equal x: P = +-Q) -- the condition the device's `exc` must catch."""
    F = E.F
    if e is None:
        return acc, True
    if F.is_zero(acc[2]):
        return (e[0], e[1], F.one), True
    return E._jadd_affine(acc, e), F.mul(e[0], F.sqr(acc[2])) == acc[0]


def _jac_of(E, p):
    return (E.F.one, E.F.one, E.F.zero) if p is None else (p[0], p[1], E.F.one)


def ladder_uniform_model(E, p, k, top):
    """jac_ladder_uniform: [k] p for the leading one at bit `top`; (result, a special case occurred)."""
    acc, special = _jac_of(E, p), p is None
    for bit in range(top - 1, -1, -1):
        acc = E._jdbl(acc)
        if (k >> bit) & 1:
            acc, s = _walk_add(E, acc, p)
            special |= s
    return E._to_affine(acc), special


def sac_model(d):
    """sac_recode4 (the SAC_RECODE4 op pins the device's): signs s_i, bits u_j[i] (i < 64), the top bits and fix."""
    d0 = d[0] | 1
    s = [1 if (d0 >> (i + 1)) & 1 else -1 for i in range(64)]
    u, top = [], []
    for j in (1, 2, 3):
        k, uj = d[j], []
        for i in range(64):
            uj.append(k & 1)
            k = (k - s[i] * (k & 1)) >> 1
        u.append(uj)
        top.append(k)
    return s, u, top, d[0] % 2 == 0


def subset_table(E, pts, with_first):
    """with_first: entry m = B0 + sum_j bit_j(m) B_{j+1} (g2_sac_table); else entry m = sum_k bit_k(m) P_k (Straus)."""
    rest = pts[1:] if with_first else pts
    tbl = []
    for m in range(1 << len(rest)):
        e = pts[0] if with_first else None
        for j, b in enumerate(rest):
            if (m >> j) & 1:
                e = E.add(e, b)
        tbl.append(e)
    return tbl


def joint_mul4_model(bases, d):
    """g2_joint_mul4: (sum d_i B_i, special, fix)."""
    E = o.E2
    s, u, top, fix = sac_model(d)
    tbl = subset_table(E, bases, True)
    e = tbl[top[0] | top[1] << 1 | top[2] << 2]
    acc, special = _jac_of(E, e), e is None
    for i in range(63, -1, -1):
        acc = E._jdbl(acc)
        e = tbl[u[0][i] | u[1][i] << 1 | u[2][i] << 2]
        acc, sp = _walk_add(E, acc, e if s[i] > 0 else E.neg(e))
        special |= sp
    r = E._to_affine(acc)
    if fix:
        r = E.add(r, E.neg(bases[0]))
    return r, special, fix


def gls_digits(k):
    return [k // X ** j % X for j in range(3)] + [k // X ** 3]


def gls_bases(p):
    p1 = psi(p)
    p2 = psi(p1)
    return [p, o.E2.neg(p1), p2, o.E2.neg(psi(p2))]


def mul_gls_model(p, k):
    """g2_mul_gls: ([k] p, special).  An even k runs as r - k and the result is negated."""
    flip = k % 2 == 0
    r, special, fix = joint_mul4_model(gls_bases(p), gls_digits(R - k if flip else k))
    assert not fix
    return (o.E2.neg(r) if flip else r), special


def straus_model(E, pts, cs, nbits):
    """straus_chunk / straus_small: the joint ladder over the subset sums from the identity with a `started` flag."""
    tbl = subset_table(E, pts, False)
    acc, started, special = _jac_of(E, None), False, False
    for bit in range(nbits - 1, -1, -1):
        acc = E._jdbl(acc)
        m = sum(((c >> bit) & 1) << k for k, c in enumerate(cs))
        if m:
            if started:
                acc, sp = _walk_add(E, acc, tbl[m])
                special |= sp
            else:
                acc, started = _jac_of(E, tbl[m]), True
                special |= tbl[m] is None
    return E._to_affine(acc), special


def clear_cofactor_model(p, fix):
    """g2_clear_cofactor: its two (fix: three) uniform ladders; (result, special in any of them)."""
    E = o.E2
    xp, s1 = ladder_uniform_model(E, p, X, 63)
    t1 = E.neg(xp)
    t2 = psi(p)
    t3 = E.add(psi(psi(E.dbl(p))), E.neg(t2))
    xt, s2 = ladder_uniform_model(E, E.add(t1, t2), X, 63)
    t3 = E.add(E.add(E.add(t3, E.neg(xt)), E.neg(t1)), E.neg(p))
    if not fix:
        return t3, s1 or s2
    s = E.neg(psi(psi(psi(psi(E.add(t3, psi(t3)))))))
    r, s3 = ladder_uniform_model(E, s, COFACTOR_FIX_SHORT, 62)
    return r, s1 or s2 or s3


def combine_class(d):
    """tc_jobs.h combine_denominator_class."""
    return "one" if d == 1 else "pow2" if d & (d - 1) == 0 and d <= 1 << 16 else "generic"


def _path(case, fn):
    if not hasattr(case, "path"):
        case.path = fn(case)
    return case.path


def _of_path(make, path_of):
    """path -> a maker of random cases that the model puts on that path."""
    def of(path):
        def maker(rnd):
            for _ in range(200):
                c = make(rnd, path)
                if path_of(c) == path:
                    return c
            raise AssertionError("no random case of path %s" % path)
        return maker
    return of


def layout(op, path_of, make, paths):
    LAYOUTS[op] = (path_of, {p: _of_path(make, path_of)(p) for p in paths})


def _any_path(op):
    return lambda rnd: LAYOUTS[op][1][rnd.choice(list(LAYOUTS[op][1]))](rnd)


MUL_SCALARS = [0, 1, 2, 3, R - 1, R - 2] + [X ** j + e for j in (1, 2, 3) for e in (0, 1, -1)]
# the largest digits gls_decompose returns: d0 .. d2 = |x| - 1 below the largest d3, and r - 1 = (|x| - 1) (|x|^3 + |x|^2)
GLS_SCALARS = MUL_SCALARS + [((R - 1) // X ** 3 - 1) * X ** 3 + X ** 3 - 1, X ** 3 - 2, (X - 1) * X2, (X - 2) * X + 4, X2 * X2 % R]


# ---- jac_add_affine ---------------------------------------------------------------------------------------------------
def _add_affine_case(fld, rnd, p, q, tag, canon=False):
    w = fld.w
    return mcase(aff_slots(fld, rnd, p, canon) + aff_slots(fld, rnd, q, canon), aux=[int(p is None), int(q is None)],
                 tag=tag + (" canonical" if canon else ""), pts=(p, q))


def _add_affine_spec(op, fld):
    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            E, cases = fld.E, []
            for p in whole_curve_points(fld, rnd)[1:]:
                q = _pt(fld, rnd, rnd.random() < 0.5)
                for a, b, tag in [(None, q, "P=O"), (p, None, "Q=O"), (None, None, "P=Q=O"), (p, p, "P=Q"), (p, E.neg(p), "P=-Q"),
                                  (p, q, "generic"), (p, E.dbl(p), "Q=2P")]:
                    cases.append(_add_affine_case(fld, rnd, a, b, tag, canon=len(cases) % 2 == 0))
            return cases
        check_result(fld, case, out, flags, fld.E.add(*case.pts), "jac_add_affine")
    spec(op, lambda rnd: _add_affine_case(fld, rnd, _pt(fld, rnd, rnd.random() < 0.5), _pt(fld, rnd), "random", rnd.random() < 0.5),
         nflags=1)(fn)


_add_affine_spec("G1_ADD_AFFINE", G1F)
_add_affine_spec("G2_ADD_AFFINE", G2F)


# ---- jac_batch_to_common_z + affine_scale_z ------------------------------------------------------------------------------
def _common_z_case(fld, rnd, pts, extra, tag):
    w = fld.w
    nmax = 7 if w == 1 else 6
    slots, lams = [], []
    for p in pts:
        lam = fld.rand(rnd)
        lams.append(lam)
        slots += fld.jac(rnd, p, lam)
    slots += [encode(0)] * (3 * w * (nmax - len(pts)))
    slots += aff_slots(fld, rnd, extra, rnd.random() < 0.5)
    return mcase(slots, aux=[len(pts), int(extra is None)], tag=tag, pts=pts, lams=lams, extra=extra)


def _common_z_spec(op, fld):
    w = fld.w
    nmax = 7 if w == 1 else 6
    F = fld.F

    def rand_case(rnd):
        n = rnd.randint(1, nmax)
        return _common_z_case(fld, rnd, [_pt(fld, rnd) if rnd.random() < 0.85 else None for _ in range(n)], _pt(fld, rnd), "random n=%d" % n)

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            pool = whole_curve_points(fld, rnd)
            cases = []
            for n in range(1, nmax + 1):
                p = _pt(fld, rnd)
                cases.append(_common_z_case(fld, rnd, [rnd.choice(pool[1:]) for _ in range(n)], rnd.choice(pool[1:]), "n=%d finite" % n))
                cases.append(_common_z_case(fld, rnd, [None] * n, p, "n=%d all at infinity" % n))
                cases.append(_common_z_case(fld, rnd, [p] * n, None, "n=%d equal points, extra at infinity" % n))
                for hole in {0, n // 2, n - 1}:
                    pts = [rnd.choice(pool[1:]) for _ in range(n)]
                    pts[hole] = None
                    cases.append(_common_z_case(fld, rnd, pts, fld.E.neg(p), "n=%d infinity at %d" % (n, hole)))
            return cases
        n = len(case.pts)
        flags_agree(case, flags, 2)
        expect(flags[0] == inf_mask(case.pts), case, "common_z: infinity flags %x" % flags[0])
        expect(flags[1] == int(case.extra is None), case, "affine_scale_z: infinity flag")
        zc = fld.res(out, 2 * w * nmax)
        want_zc = F.one
        for p, lam in zip(case.pts, case.lams):
            if p is not None:
                want_zc = F.mul(want_zc, lam)
        expect(zc == want_zc, case, "common_z: zc is not the product of the finite points' Z")
        zi = F.inv(zc)
        zi2, zi3 = F.sqr(zi), F.mul(F.sqr(zi), zi)

        def back(s):
            return (F.mul(fld.res(out, s), zi2), F.mul(fld.res(out, s + w), zi3))
        for i, p in enumerate(case.pts):
            if p is not None:
                expect(back(2 * w * i) == p, case, "common_z: (x_%d, y_%d, zc) is not input %d" % (i, i, i))
                check_bounded(case, out, 2 * w * i, 2 * w, "common_z entry %d" % i)
        check_bounded(case, out, 2 * w * nmax, w, "common_z zc")
        s = 2 * w * nmax + w
        if case.extra is not None:
            expect(back(s) == case.extra, case, "affine_scale_z: not the same point at Z = zc")
            check_bounded(case, out, s, 2 * w, "affine_scale_z")
        for k, p in ((1, case.pts[n - 1]), (2, case.extra)):  # brought back to the original curve by jac_to_affine
            if p is not None:
                t = s + 2 * w * k
                expect((fld.res(out, t), fld.res(out, t + w)) == p, case, "common_z: jac_to_affine of (x, y, zc) %d" % k)
                check_bounded(case, out, t, 2 * w, "common_z to_affine", val_bound=1.25)
    spec(op, rand_case, nflags=2)(fn)


_common_z_spec("G1_COMMON_Z", G1F)
_common_z_spec("G2_COMMON_Z", G2F)


# ---- [|x|] P by jac_ladder_uniform ---------------------------------------------------------------------------------------
def _jac_case(fld, rnd, p, tag, words=(), aux=(), **kw):
    return mcase(fld.jac(rnd, p), words, aux, tag, p=p, **kw)


def _x_abs_spec(op, fld):
    def path_of(case):
        return _path(case, lambda c: "special" if ladder_uniform_model(fld.E, c.p, X, 63)[1] else "generic")

    def make(rnd, path):
        if path == "generic":
            return _jac_case(fld, rnd, _pt(fld, rnd, rnd.random() < 0.5), "random")
        p = rnd.choice([None] + small_points(fld)[:3] + small_points(fld)[5:])
        k = rnd.randrange(1, 1 << 20)
        return _jac_case(fld, rnd, fld.E.mul(p, k), "random small order")

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            return [_jac_case(fld, rnd, p, "point %d" % i) for i, p in enumerate(whole_curve_points(fld, rnd) * 2)]
        check_result(fld, case, out, flags, fld.E.mul(case.p, X), "mul_by_x_abs")
    layout(op, path_of, make, ("generic", "special"))
    spec(op, _any_path(op), nflags=1)(fn)


_x_abs_spec("G1_MUL_BY_X_ABS", G1F)
_x_abs_spec("G2_MUL_BY_X_ABS", G2F)


# ---- psi on Jacobian points, the GLS bases ---------------------------------------------------------------------------------
@spec("G2_PSI_JAC", lambda rnd: _jac_case(G2F, rnd, _pt(G2F, rnd, rnd.random() < 0.5), "random"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_jac_case(G2F, rnd, p, "point %d" % i) for i, p in enumerate(whole_curve_points(G2F, rnd))]
    check_result(G2F, case, out, flags, psi(case.p), "g2_psi(G2Jac)")


def _bases_case(rnd, p, tag, canon=False):
    return mcase(aff_slots(G2F, rnd, p, canon), aux=[int(p is None)], tag=tag, p=p)


@spec("G2_GLS_BASES", lambda rnd: _bases_case(rnd, _pt(G2F, rnd), "random", rnd.random() < 0.5), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_bases_case(rnd, p, "point %d" % i, i % 2 == 0) for i, p in enumerate(whole_curve_points(G2F, rnd) * 2)]
    flags_agree(case, flags, 1)
    expect(flags[0] == (15 if case.p is None else 0), case, "g2_gls_bases: infinity flags %x" % flags[0])
    if case.p is not None:
        for k, b in enumerate(gls_bases(case.p)):
            expect((G2F.res(out, 4 * k), G2F.res(out, 4 * k + 2)) == b, case, "g2_gls_bases: base %d" % k)
            check_bounded(case, out, 4 * k, 4, "g2_gls_bases %d" % k)


# ---- g2_sac_table, g2_joint_mul4 -------------------------------------------------------------------------------------------
def _base_sets(rnd):
    """Four independent bases, and the sets whose subset sums meet the special cases of the table builder."""
    E = o.E2
    b = [_pt(G2F, rnd) for _ in range(4)]
    c = curve_point(G2F, rnd)
    sets = [("independent", b), ("outside the subgroup", [c, b[1], curve_point(G2F, rnd), b[3]]),
            ("B1 = B0", [b[0], b[0], b[2], b[3]]), ("B1 = -B0", [b[0], E.neg(b[0]), b[2], b[3]]),
            ("B2 = -B1", [b[0], b[1], E.neg(b[1]), b[3]]), ("B3 = B2 = B1 = B0", [b[0]] * 4),
            ("B0 + B1 + B2 + B3 = O", [E.neg(E.add(E.add(b[1], b[2]), b[3])), b[1], b[2], b[3]]),
            ("B3 = -(B0 + B1)", [b[0], b[1], b[2], E.neg(E.add(b[0], b[1]))]), ("all at infinity", [None] * 4)]
    for j in range(4):
        sets.append(("B%d at infinity" % j, [None if i == j else b[i] for i in range(4)]))
    return sets


def _bases_slots(rnd, bases, canon):
    return sum((aff_slots(G2F, rnd, p, canon) for p in bases), [])


def _sac_table_case(rnd, bases, tag, canon=False):
    return mcase(_bases_slots(rnd, bases, canon), aux=[inf_mask(bases)], tag=tag, bases=bases)


@spec("G2_SAC_TABLE", lambda rnd: _sac_table_case(rnd, [_pt(G2F, rnd) for _ in range(4)], "random", rnd.random() < 0.5), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_sac_table_case(rnd, bs, tag, c) for tag, bs in _base_sets(rnd) for c in (False, True)]
    F = G2F.F
    want = subset_table(o.E2, case.bases, True)
    flags_agree(case, flags, 1)
    expect(flags[0] == inf_mask(want), case, "g2_sac_table: infinity flags %x, want %x" % (flags[0], inf_mask(want)))
    zi = F.inv(G2F.res(out, 32))
    zi2, zi3 = F.sqr(zi), F.mul(F.sqr(zi), zi)
    for m, e in enumerate(want):
        if e is not None:
            got = (F.mul(G2F.res(out, 4 * m), zi2), F.mul(G2F.res(out, 4 * m + 2), zi3))
            expect(got == e, case, "g2_sac_table: entry %d is not B0 + sum u_j B_j at Z = zc" % m)
            check_bounded(case, out, 4 * m, 4, "g2_sac_table entry %d" % m, val_bound=2.1)
    if want[7] is not None:
        expect((G2F.res(out, 34), G2F.res(out, 36)) == want[7], case, "g2_sac_table: jac_to_affine of entry 7")
        check_bounded(case, out, 34, 4, "g2_sac_table to_affine", val_bound=1.25)


def _joint_case(rnd, bases, d, tag, canon=False):
    return mcase(_bases_slots(rnd, bases, canon), u64_words(d), [inf_mask(bases)], "%s d=%s" % (tag, [hex(x) for x in d]), bases=bases, d=d)


def _joint_path(case):
    def model(c):
        _, special, fix = joint_mul4_model(c.bases, c.d)
        return "special" if special else "fix" if fix else "generic"
    return _path(case, model)


def _joint_make(rnd, path):
    b = [_pt(G2F, rnd) for _ in range(4)]
    d = [rnd.getrandbits(64) for _ in range(4)]
    if path == "generic":
        d[0] |= 1
    elif path == "fix":
        d[0] &= ~1
    else:
        kind = rnd.randrange(3)
        if kind == 0:
            b[1] = o.E2.neg(b[0]) if rnd.random() < 0.5 else b[0]
        elif kind == 1:
            b[rnd.randrange(4)] = None
        else:
            d = [rnd.randrange(4), 0, 0, 0]
    return _joint_case(rnd, b, d, "random")


JOINT_DIGITS = [[1, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 1, 1], [3, 0, 5, 0], [M64, M64, M64, M64], [M64 - 1, M64, 0, M64],
                [X - 1, X - 1, X - 1, X - 1], [X - 2, 0, X - 1, 1], [1 << 63, 1 << 63, 1, 0], [0, X - 1, 0, 0], [0, 0, 0, 1], [5, 0, 0, M64]]


@spec("G2_JOINT_MUL4", lambda rnd: _any_path("G2_JOINT_MUL4")(rnd), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        sets = _base_sets(rnd)
        cases = [_joint_case(rnd, sets[i % 2][1], d, sets[i % 2][0], i % 3 == 0) for i, d in enumerate(JOINT_DIGITS)]
        for i, (tag, bs) in enumerate(sets[2:]):
            d = [rnd.getrandbits(64) | 1 for _ in range(4)]
            cases.append(_joint_case(rnd, bs, d, tag, i % 2 == 0))
            cases.append(_joint_case(rnd, bs, [d[0] - 1, d[1], 0, d[3]], tag))
        return cases
    E = o.E2
    want = None
    for b, d in zip(case.bases, case.d):
        want = E.add(want, E.mul(b, d))
    check_result(G2F, case, out, flags, want, "g2_joint_mul4")


layout("G2_JOINT_MUL4", _joint_path, _joint_make, ("generic", "fix", "special"))


# ---- g2_mul_gls (affine and Jacobian; the second covers g2_gls_digits_mul) ---------------------------------------------------
def _scalar_point_case(fld, rnd, p, k, jac, tag, canon=False):
    slots = fld.jac(rnd, p) if jac else aff_slots(fld, rnd, p, canon)
    return mcase(slots, u32s(k), [int(p is None)], "%s k=%x" % (tag, k), p=p, k=k)


def _gls_path(case):
    return _path(case, lambda c: "special" if mul_gls_model(c.p, c.k)[1] else "generic")


def _mul_gls_spec(op, jac):
    def make(rnd, path):
        p, k = _pt(G2F, rnd), rnd.randrange(R)
        if path == "special":
            if rnd.random() < 0.6:
                p = None
            else:
                k = 0
        return _scalar_point_case(G2F, rnd, p, k, jac, "random", rnd.random() < 0.5)

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            p = _pt(G2F, rnd)
            cases = [_scalar_point_case(G2F, rnd, p if i % 3 else _pt(G2F, rnd), k, jac, "edge", i % 2 == 0) for i, k in enumerate(GLS_SCALARS)]
            cases += [_scalar_point_case(G2F, rnd, None, k, jac, "P = O") for k in (0, 1, 2, R - 1, rnd.randrange(R))]
            return cases
        check_result(G2F, case, out, flags, o.E2.mul(case.p, case.k), "g2_mul_gls")
    layout(op, _gls_path, make, ("generic", "special"))
    spec(op, lambda rnd: _any_path(op)(rnd), nflags=1)(fn)


_mul_gls_spec("G2_MUL_GLS", False)
_mul_gls_spec("G2_MUL_GLS_JAC", True)


# ---- g2_clear_cofactor -------------------------------------------------------------------------------------------------------
def _clear_case(rnd, p, fix, tag, canon=False):
    return mcase(aff_slots(G2F, rnd, p, canon), aux=[int(p is None), int(fix)], tag="%s fix=%d" % (tag, fix), p=p, fix=fix)


def _clear_path(case):
    return _path(case, lambda c: "special" if clear_cofactor_model(c.p, c.fix)[1] else "generic")


def _clear_make(rnd, path):
    if path == "generic":
        p = _pt(G2F, rnd, rnd.random() < 0.2)
    else:
        p = o.E2.mul(rnd.choice([None] + small_points(G2F)), rnd.randrange(1, 1 << 20))
    return _clear_case(rnd, p, rnd.random() < 0.5, "random", rnd.random() < 0.5)


@spec("G2_CLEAR_COFACTOR", lambda rnd: _any_path("G2_CLEAR_COFACTOR")(rnd), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_clear_case(rnd, p, fix, "point %d" % i, i % 2 == 0) for i, p in enumerate(whole_curve_points(G2F, rnd)) for fix in (1, 0)]
    want = cached("clear", (case.p, case.fix), lambda: o.E2.mul(case.p, H2 if case.fix else CLEAR_NOFIX))
    check_result(G2F, case, out, flags, want, "g2_clear_cofactor")


layout("G2_CLEAR_COFACTOR", _clear_path, _clear_make, ("generic", "special"))


# ---- g1_mul_glv: affine, Jacobian, arena (no per-wave decision: every addition of the ladder is the safe one) --------------------
def _mul_glv_spec(op, jac):
    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            p = _pt(G1F, rnd)
            ks = _g1_edges(rnd) + MUL_SCALARS
            cases = [_scalar_point_case(G1F, rnd, p if i % 3 else _pt(G1F, rnd), k, jac, "edge", i % 2 == 0) for i, k in enumerate(ks)]
            cases += [_scalar_point_case(G1F, rnd, None, k, jac, "P = O") for k in (0, 1, 2, R - 1, rnd.randrange(R))]
            return cases
        check_result(G1F, case, out, flags, o.E1.mul(case.p, case.k), "g1_mul_glv")
    spec(op, lambda rnd: _scalar_point_case(G1F, rnd, _pt(G1F, rnd), rnd.randrange(R), jac, "random", rnd.random() < 0.5), nflags=1)(fn)


_mul_glv_spec("G1_MUL_GLV", False)
_mul_glv_spec("G1_MUL_GLV_JAC", True)
_mul_glv_spec("G1_MUL_GLV_ARENA", False)


# ---- lincomb_chunk4 = straus_chunk<Fq, 4> ------------------------------------------------------------------------------------
def _point_sets(fld, rnd, n):
    """n points: independent, and the sets whose subset sums meet infinity or a doubling."""
    E = fld.E
    b = [_pt(fld, rnd) for _ in range(n)]
    sets = [("independent", b), ("P1 = P0", [b[0], b[0]] + b[2:]), ("P1 = -P0", [b[0], E.neg(b[0])] + b[2:]), ("all equal", [b[0]] * n),
            ("P0 at infinity", [None] + b[1:]), ("last at infinity", b[:-1] + [None]), ("all at infinity", [None] * n)]
    if n >= 3:
        sets.append(("P2 = -(P0 + P1)", b[:2] + [E.neg(E.add(b[0], b[1]))] + b[3:]))
    return sets


def _lincomb_case(rnd, pts, sc, tag, canon=False):
    ws = sum((u32s(s, NL) for s in sc), [])
    return mcase(sum((aff_slots(G1F, rnd, p, canon) for p in pts), []), ws, [inf_mask(pts)], tag, pts=pts, cs=sc)


def _lincomb_path(case):
    return _path(case, lambda c: "special" if straus_model(o.E1, c.pts, c.cs, 255)[1] else "generic")


def _lincomb_make(rnd, path):
    pts = [_pt(G1F, rnd) for _ in range(4)]
    sc = [rnd.randrange(R) for _ in range(4)]
    if path == "special":
        kind = rnd.randrange(3)
        if kind == 0:
            pts[1] = o.E1.neg(pts[0]) if rnd.random() < 0.5 else pts[0]
        elif kind == 1:
            pts[rnd.randrange(4)] = None
        else:
            sc[1] = sc[0]
            pts[1] = o.E1.neg(pts[0])
            sc[2] = sc[3] = 0
    return _lincomb_case(rnd, pts, sc, "random", rnd.random() < 0.5)


@spec("G1_LINCOMB_CHUNK4", lambda rnd: _any_path("G1_LINCOMB_CHUNK4")(rnd), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        sets = _point_sets(G1F, rnd, 4)
        scs = [[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [1, 1, 1, 1], [R - 1, R - 1, R - 1, R - 1], [R - 1, 1, R - 2, 2], [1 << 254, 0, 3, 0],
               [X2, X2 + 1, X, 1 << 128]]
        cases = [_lincomb_case(rnd, sets[0][1], sc, "scalars %d" % i, i % 2 == 0) for i, sc in enumerate(scs)]
        for i, (tag, pts) in enumerate(sets[1:]):
            sc = [rnd.randrange(R) for _ in range(4)]
            cases.append(_lincomb_case(rnd, pts, sc, tag, i % 2 == 0))
            cases.append(_lincomb_case(rnd, pts, [sc[0], sc[0], 0, 5], tag + ", equal scalars"))
        return cases
    want = None
    for p, s in zip(case.pts, case.cs):
        want = o.E1.add(want, o.E1.mul(p, s))
    check_result(G1F, case, out, flags, want, "lincomb_chunk4")


layout("G1_LINCOMB_CHUNK4", _lincomb_path, _lincomb_make, ("generic", "special"))


# ---- straus_small -----------------------------------------------------------------------------------------------------------
def _small_mul_case(fld, rnd, pts, cs, tag, canon=False):
    K = len(pts)
    w = fld.w
    slots = sum((aff_slots(fld, rnd, p, canon) for p in pts), []) + [encode(0)] * (2 * w * (4 - K))
    return mcase(slots, u64_words(cs), [K, inf_mask(pts)], "K=%d %s c=%s" % (K, tag, [hex(c) for c in cs]), pts=pts, cs=cs)


def _straus_small_spec(op, fld):
    E = fld.E

    def path_of(case):
        return _path(case, lambda c: "special" if straus_model(E, c.pts, c.cs, 64)[1] else "generic")

    def coeffs(rnd, K):
        # the shapes lagrange_small_coeffs hands on: a few bits to a few tens of bits, now and then one of 63 bits beside tiny ones
        kind = rnd.randrange(4)
        if kind == 0:
            return [rnd.getrandbits(rnd.choice([3, 9, 14])) for _ in range(K)]
        if kind == 1:
            return [rnd.getrandbits(63) | 1 << 62] + [rnd.getrandbits(4) for _ in range(K - 1)]
        if kind == 2:
            return [rnd.getrandbits(rnd.randint(1, 63)) for _ in range(K)]
        return [1 << rnd.randrange(20) for _ in range(K)]

    def make(rnd, path):
        K = rnd.choice([2, 3, 4])
        pts = [_pt(fld, rnd) for _ in range(K)]
        cs = coeffs(rnd, K)
        if path == "special":
            kind = rnd.randrange(3)
            if kind == 0:
                pts[1] = E.neg(pts[0]) if rnd.random() < 0.5 else pts[0]
                cs[0] |= 1
                cs[1] |= 3
            elif kind == 1:
                j = rnd.randrange(K)
                pts[j] = None
                cs[j] |= 1
            else:
                pts[1] = E.neg(pts[0])
                cs = [cs[0] | 1, cs[0] | 1] + [0] * (K - 2)
        return _small_mul_case(fld, rnd, pts, cs, "random", rnd.random() < 0.5)

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            cases = []
            for K in (2, 3, 4):
                sets = _point_sets(fld, rnd, K)
                big = (1 << 63) - 1
                css = [[0] * K, [1] + [0] * (K - 1), [0] * (K - 1) + [1], [1] * K, [big] * K, [big - 1] + [1] * (K - 1), [1 << 62] + [2] * (K - 1),
                       [3] * (K - 1) + [(1 << 62) + 1], [2, 1] + [0] * (K - 2)]
                cases += [_small_mul_case(fld, rnd, sets[0][1], cs, "coefficients %d" % i, i % 2 == 0) for i, cs in enumerate(css)]
                for i, (tag, pts) in enumerate(sets[1:]):
                    cases.append(_small_mul_case(fld, rnd, pts, coeffs(rnd, K), tag, i % 2 == 0))
                    cases.append(_small_mul_case(fld, rnd, pts, [7] * K, tag + ", equal coefficients"))
            return cases
        want = None
        for p, c in zip(case.pts, case.cs):
            want = E.add(want, E.mul(p, c))
        check_result(fld, case, out, flags, want, "straus_small")
    layout(op, path_of, make, ("generic", "special"))
    spec(op, lambda rnd: _any_path(op)(rnd), nflags=1)(fn)


_straus_small_spec("G1_STRAUS_SMALL", G1F)
_straus_small_spec("G1_STRAUS_SMALL_INLINE", G1F)
_straus_small_spec("G2_STRAUS_SMALL", G2F)


# ---- combine_divide, combine_divide_arena: [+-1 / D] Q --------------------------------------------------------------------------
DIVIDE_DS = [1] + [1 << a for a in range(1, 18)] + [3, 5, 6, 255, 65521, 3 << 15, (1 << 32) - 1, 1 << 32, (1 << 32) + 15, 3 ** 39,
                                                    (1 << 61) - 1, (1 << 62) - 1, (1 << 62) - 57, 1 << 61]


def _divide_case(fld, rnd, q, d, neg, tag=""):
    return _jac_case(fld, rnd, q, "%s D=%s%d" % (tag, "-" if neg else "", d), u32s(d, 2), [int(neg)], d=d, neg=neg)


def _divide_random_d(rnd, path):
    if path == "one":
        return 1
    if path == "pow2":
        return 1 << rnd.randint(1, 16)
    if path == "word":
        return rnd.randrange(2, 1 << 32)
    if path == "bit":
        return rnd.randrange(1 << 32, 1 << 62)
    while True:
        d = rnd.choice([rnd.randrange(2, 1 << 20), rnd.randrange(2, 1 << 62), 1 << rnd.randint(17, 61)])
        if combine_class(d) == "generic":
            return d


def _divide_spec(op, fld, paths):
    def path_of(case):
        def model(c):
            if fld.w == 1:  # (G1: g1_mul_glv has no branch-free pass; the per-wave decisions are D = 1 and fr_inverse_of_small's)
                return "one" if c.d == 1 else "word" if c.d < 1 << 32 else "bit"
            cls = combine_class(c.d)
            if cls == "pow2" and c.p is None:
                return "special"
            if cls == "generic" and mul_gls_model(c.p, pow(c.d, -1, R))[1]:
                return "special"
            return cls
        return _path(case, model)

    def make(rnd, path):
        if path == "special":
            return _divide_case(fld, rnd, None, _divide_random_d(rnd, rnd.choice(["pow2", "generic"])), rnd.random() < 0.5, "random Q = O")
        return _divide_case(fld, rnd, _pt(fld, rnd), _divide_random_d(rnd, path), rnd.random() < 0.5, "random")

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            q = _pt(fld, rnd)
            cases = [_divide_case(fld, rnd, q if i % 4 else _pt(fld, rnd), d, neg) for i, d in enumerate(DIVIDE_DS) for neg in (False, True)]
            cases += [_divide_case(fld, rnd, None, d, neg, "Q = O") for d in (1, 2, 1 << 16, 1 << 17, 3, (1 << 62) - 1) for neg in (False, True)]
            return cases
        k = pow(-case.d if case.neg else case.d, -1, R)
        check_result(fld, case, out, flags, fld.E.mul(case.p, k), "combine_divide")
    layout(op, path_of, make, paths)
    spec(op, lambda rnd: _any_path(op)(rnd), nflags=1)(fn)


_divide_spec("G1_COMBINE_DIVIDE", G1F, ("one", "word", "bit"))
_divide_spec("G1_COMBINE_DIVIDE_ARENA", G1F, ("one", "word", "bit"))
_divide_spec("G2_COMBINE_DIVIDE", G2F, ("one", "pow2", "generic", "special"))


# ---- g1_mul_u64 ---------------------------------------------------------------------------------------------------------------
@spec("G1_MUL_U64", lambda rnd: _jac_case(G1F, rnd, _pt(G1F, rnd), "random", u32s(rnd.getrandbits(rnd.choice([8, 33, 64])), 2)), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        xs = [0, 1, 2, 3, 1 << 63, M64, 1 << 32, (1 << 32) - 1, M64 - 1, (1 << 63) + 1]
        pts = whole_curve_points(G1F, rnd)
        cases = [_jac_case(G1F, rnd, pts[1 + i % 3], "edge x=%x" % x, u32s(x, 2)) for i, x in enumerate(xs)]
        cases += [_jac_case(G1F, rnd, p, "point %d x=%x" % (i, x), u32s(x, 2)) for i, p in enumerate(pts) for x in (3, M64, rnd.getrandbits(64))]
        return cases
    x = words_value(case.slots[3]) & M64
    check_result(G1F, case, out, flags, o.E1.mul(case.p, x), "g1_mul_u64")


# ---------------------------------------------------------------------------------------------------------------------
# the byte layer (ops 180 on): SHA3, ChaCha20, the samplers and the hash onto G2; the wire codecs and their wrappers
# ---------------------------------------------------------------------------------------------------------------------
ROW_BYTES = CONF_OUT * NL * 4  # 2240: a job's row as bytes
SLOT_BYTES = NL * 4
WRAP = 10 * SLOT_BYTES  # conformance.h kConfWrap: where the decode ops put their wrapper's bytes
MSG_B2, MSG_A4, MSG_B4 = 1120, 192, 1216  # conformance.h kConfMsgB2, kConfMsgA4, kConfMsgB4
SENT_ROW = bytes([SENTINEL & 0xff]) * ROW_BYTES
TABLES = {}  # op -> (edges, rnd) -> the whole table, for ops whose wave layout the generic hooks cannot express
BYTE_OPS_FROM = 180


def raw_bytes(parts):
    """Byte operands [(byte offset in the job's input row, bytes)] as raw little-endian words (beside raw_words)."""
    end = max([off + len(b) for off, b in parts] + [0])
    buf = bytearray(-(-end // 4) * 4)
    for off, b in parts:
        buf[off:off + len(b)] = b
    return raw_words([int.from_bytes(buf[k:k + 4], "little") for k in range(0, len(buf), 4)]) if buf else []


def bcase(parts, aux=(), tag="", **kw):
    c = Case(raw_bytes(parts), aux=aux, tag=tag)
    c.__dict__.update(kw)
    return c


def _sl(s, n=1):
    return (SLOT_BYTES * s, SLOT_BYTES * (s + n))


def check_row(case, out, want, regions, what):
    """want: [(byte offset, bytes)] the row must hold; outside `regions` (and the wanted bytes) every byte still holds
    the sentinel the row was filled with: the routine wrote exactly its documented length."""
    row = bytearray(out.tobytes())
    for off, b in want:
        got = bytes(row[off:off + len(b)])
        expect(got == bytes(b), case, "%s: bytes at %d: %s, want %s" % (what, off, got.hex(), bytes(b).hex()))
    for a, b in list(regions) + [(off, off + len(b)) for off, b in want]:
        row[a:b] = SENT_ROW[a:b]
    if bytes(row) != SENT_ROW:
        k = next(i for i in range(ROW_BYTES) if row[i] != SENT_ROW[i])
        expect(False, case, "%s: byte %d past the documented output was written (%02x)" % (what, k, row[k]))


def fixed_layout(op, uniform, mixed):
    """TABLES hook: one full wave per maker of `uniform` (every job of the wave from that maker), then the directed cases
    interleaved with cases of the `mixed` makers in turn, to three waves and a ragged tail at least."""
    def build(edges, rnd):
        wave = 64 // lanes(op)
        cases = []
        for make in uniform:
            cases += [make(rnd) for _ in range(wave)]
        pool = list(edges)
        n = max(len(cases) + 2 * len(pool), 3 * wave + 5)
        if n % wave == 0:
            n += 1
        k = 0
        while len(cases) < n:
            if pool and (len(cases) % 2 == 0 or len(cases) + len(pool) >= n):
                cases.append(pool.pop(0))
            else:
                cases.append(mixed[k % len(mixed)](rnd))
                k += 1
        return cases
    TABLES[op] = build


# ---- SHA3-256 ----------------------------------------------------------------------------------------------------------
SHA3_RATE = 136
SHA3_LENGTHS = [0, 1, 135, 136, 137, 271, 272, 273, 408, 2240]


def sha3_blocks(n):
    return n // SHA3_RATE + 1


def _sha_case(msg, call, tag):
    pad = bytes([0xa5]) * min(8, ROW_BYTES - len(msg))  # (bytes past the end that must not be read into the digest)
    return bcase([(0, bytes(msg) + pad)], [len(msg), call], "%s len=%d call=%d" % (tag, len(msg), call), msg=bytes(msg))


def _sha_rand(blocks):
    def make(rnd):
        n = rnd.randrange(SHA3_RATE * (blocks - 1), min(SHA3_RATE * blocks, ROW_BYTES + 1))
        return _sha_case(rnd.randbytes(n), rnd.randrange(2), "random")
    return make


@spec("SHA3_256", _sha_rand(1))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = [_sha_case(rnd.randbytes(n), call, "length") for n in SHA3_LENGTHS for call in (0, 1)]
        cases += [_sha_case(bytes([0xff]) * n, n % 2, "all ff") for n in (1, 135, 136, 137, 272, 2240)]
        cases += [_sha_case(rnd.randbytes(n - 1) + bytes([last]), (n + last) % 2, "last byte %02x" % last)
                  for n in (1, 135, 136, 137, 272) for last in (0x06, 0x80)]
        return cases
    d = hashlib.sha3_256(case.msg).digest()
    check_row(case, out, [(0, d)], [], "sha3_256")


fixed_layout("SHA3_256", [_sha_rand(1), _sha_rand(2)], [_sha_rand(b) for b in (1, 2, 3, 17)])


# ---- ChaCha20 word stream ------------------------------------------------------------------------------------------------
CHACHA_COUNTS = [0, 1, 15, 16, 17, 32, 33, 64]
CHACHA_ZERO_KEY_BLOCK = ("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
                         "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586")  # the published all-zero-key block


def chacha_words(key, ctr, n):
    ws = []
    for b in range(-(-n // 16)):
        ws += o.chacha20_block(key, (ctr + b) & M64)
    return ws[:n]


def _chacha_case(key, n, ctr, tag=""):
    use = ctr is not None
    ws = list(key) + [0] * (NL - 8) + u32s(ctr or 0, 2)
    return scase(ws, [n, int(use)], "%s n=%d ctr=%s" % (tag, n, ctr), key=list(key), n=n, ctr=ctr or 0)


def _rand_chacha(rnd):
    return _chacha_case([rnd.getrandbits(32) for _ in range(8)], rnd.randint(0, 64),
                        rnd.choice([None, 0, (1 << 32) - 1, rnd.getrandbits(64) >> rnd.choice([0, 31, 40])]), "random")


@spec("CHACHA_WORDS", _rand_chacha)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        key = [rnd.getrandbits(32) for _ in range(8)]
        cases = [_chacha_case(k, n, ctr, "edge") for n in CHACHA_COUNTS for ctr in (None, (1 << 32) - 1) for k in ([0] * 8, key)]
        return cases + [_chacha_case(key, 33, M64, "counter wraps"), _chacha_case(key, 17, 0, "explicit zero")]
    n, blocks = case.n, -(-case.n // 16)
    ws = chacha_words(case.key, case.ctr, n)
    ctr = (case.ctr + blocks) & M64
    tail = [n - 16 * (blocks - 1) if n else 16, ctr & 0xffffffff, ctr >> 32]
    check_row(case, out, [(0, b"".join(w.to_bytes(4, "little") for w in ws)),
                          (_sl(5)[0], b"".join(w.to_bytes(4, "little") for w in tail))], [], "chacha words")


# ---- fq_random ------------------------------------------------------------------------------------------------------------
def fq_seed(i):
    return o.sha3_256(b"conf-fq-%d" % i)


def fq_draws(seed, n=8):
    """[(value, stream words used so far, rejections of this draw)] of n successive o.fq_random draws."""
    rng = o.ChaChaRng(seed)
    res, used = [], 0
    for _ in range(n):
        v = o.fq_random(rng)
        res.append((v, rng.words_used, (rng.words_used - used) // 12 - 1))
        used = rng.words_used
    return res


def _fq_random_path(case):
    """The wave sees all eight draws of every lane (the op draws eight times whatever aux[0] says)."""
    m = max(r for _, _, r in cached("fqdraws", case.seed, lambda: fq_draws(case.seed)))
    return "none" if m == 0 else "one" if m == 1 else "many" if m >= 3 else "two"


def _fq_random_case(i, n, tag=""):
    seed = fq_seed(i)
    return scase(u32s(int.from_bytes(seed, "little")), [n], "%s seed %d n=%d" % (tag, i, n), seed=seed, n=n)


def _fq_random_of(path):
    def make(rnd):
        for _ in range(2000):
            c = _fq_random_case(rnd.randrange(1 << 16), 8, "random")
            if _fq_random_path(c) == path:
                return c
        raise AssertionError("no seed of path %s" % path)
    return make


@spec("FQ_RANDOM", _fq_random_of("none"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_fq_random_case(i, n, "edge") for i, n in enumerate([0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 8])]
    draws = cached("fqdraws", case.seed, lambda: fq_draws(case.seed))[:case.n]
    for k, (v, used, _) in enumerate(draws):
        l = out_limbs(out, k)
        check_carried(case, l, "fq_random")
        expect(residue(l) == v, case, "fq_random: draw %d" % k)
        expect(-P // 4 < value(l) < 5 * P // 4, case, "fq_random: value outside (-p/4, 5p/4)")
    check_row(case, out, [(_sl(8)[0], b"".join(u.to_bytes(4, "little") for _, u, _ in draws))], [_sl(0, case.n)], "fq_random")


fixed_layout("FQ_RANDOM", [_fq_random_of("none")], [_fq_random_of(p) for p in ("none", "one", "many")])


# ---- the candidates of G2::random ----------------------------------------------------------------------------------------
def hash_seed(i):
    return o.sha3_256(b"conf-hash-%d" % i)


def f2_is_square(a):
    """Euler's criterion on the norm."""
    n = (a[0] * a[0] + a[1] * a[1]) % P
    return n == 0 or pow(n, (P - 1) // 2, P) == 1


def g2_candidates(seed, upto):
    """The stream's candidates (x, greatest, x^3 + b a square) until `upto` of them were accepted."""
    rng = o.ChaChaRng(seed)
    cands, acc = [], 0
    while acc < upto:
        c0 = o.fq_random(rng)
        c1 = o.fq_random(rng)
        x = (c0, c1)
        g = rng.next_u32() % 2 != 0
        sq = f2_is_square(o.f2_add(o.f2_mul(o.f2_sqr(x), x), o._Fq2.b))
        cands.append((x, g, sq))
        acc += sq
    return cands


def seed_class(seed):
    """Which candidate of the stream (1, 2, ...) is the first accepted one."""
    return cached("class", seed, lambda: len(g2_candidates(seed, 1)))


def seed_classes():
    """class -> the indices i < 300 of that class, by the bounded search."""
    def search():
        found = {}
        for i in range(300):
            found.setdefault(seed_class(hash_seed(i)), []).append(i)
        return found
    return cached("classes", 0, search)


def g2_random_ref(seed, fix, nth=0):
    """G2::random of the seed's stream -- its (nth + 1)-th accepted candidate, cofactor cleared (fix = 0: by the multiple
    g2_clear_cofactor(fix = false) applies, the reference of G2_CLEAR_COFACTOR)."""
    def ref():
        x, g, _ = [c for c in g2_candidates(seed, nth + 1) if c[2]][nth]
        return o.E2.mul(o.g2_get_point_from_x(x, g), H2 if fix else CLEAR_NOFIX)
    return cached("g2random", (seed, int(bool(fix)), nth), ref)


def class_seed(rnd, k, pool=4):
    """A seed index of class k (one of the first `pool` found, so that the references are shared)."""
    return rnd.choice(seed_classes()[k][:pool])


def _seed_words(seed):
    return u32s(int.from_bytes(seed, "little"))


def _g2_random_case(i, fix, forced=0, tag=""):
    seed = hash_seed(i)
    return scase(_seed_words(seed), [int(fix), forced], "%s seed %d class %d fix=%d forced=%d" % (tag, i, seed_class(seed), fix, forced),
                 seed=seed, fix=int(fix), forced=forced)


@spec("G2_RANDOM_FROM_SEED", lambda rnd: _any_path("G2_RANDOM_FROM_SEED")(rnd), nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cls = seed_classes()
        assert all(cls.get(k) for k in range(1, 11)), sorted(cls)
        cases = [_g2_random_case(cls[k][0], fix, 0, "class") for k in range(1, 11) for fix in (1, 0)]
        # a second outer round (the host build forces it): the stream is re-read past the candidates already consumed
        cases += [_g2_random_case(cls[k][0], 1, 1, "second round") for k in (1, 2, 3, 4)]
        return cases
    flags_agree(case, flags, 2)
    expect(flags[1] in (0, case.forced), case, "forced rounds %d" % flags[1])
    check_result(G2F, case, out, flags, g2_random_ref(case.seed, case.fix, int(flags[1])), "g2_random_from_seed")
    check_row(case, out, [], [_sl(0, 10)], "g2_random_from_seed")


layout("G2_RANDOM_FROM_SEED", lambda c: str(seed_class(c.seed)),
       lambda rnd, path: _g2_random_case(class_seed(rnd, int(path), 6), rnd.randrange(2), 0, "random"), ("1", "2"))


def _g2_random_x2_case(ia, ib, fix, forced=0, tag=""):
    sa, sb = hash_seed(ia), hash_seed(ib)
    return scase(_seed_words(sa) + [0] * (NL - 8) + _seed_words(sb), [int(fix), forced],
                 "%s seeds %d, %d classes (%d, %d) fix=%d forced=%d" % (tag, ia, ib, seed_class(sa), seed_class(sb), fix, forced),
                 seeds=(sa, sb), fix=int(fix), forced=forced)


def _x2_of_classes(ka, kb, tag="random"):
    return lambda rnd: _g2_random_x2_case(class_seed(rnd, ka), class_seed(rnd, kb), rnd.randrange(2), 0, tag)


X2_PAIRS = [(1, 1), (1, 10), (10, 1), (2, 9)]


@spec("G2_RANDOM_FROM_SEED_X2", _x2_of_classes(1, 1), nflags=3)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cls = seed_classes()
        cases = [_g2_random_x2_case(cls[a][0], cls[b][-1], fix, 0, "pair") for a, b in X2_PAIRS for fix in (1, 0)]
        cases += [_g2_random_x2_case(cls[a][0], cls[b][0], 1, 1, "second round") for a, b in ((1, 2), (3, 1))]
        return cases
    flags_agree(case, flags, 3)
    expect(flags[2] in (0, case.forced), case, "forced rounds %d" % flags[2])
    for s, seed in enumerate(case.seeds):
        want = g2_random_ref(seed, case.fix, int(flags[2]))
        what = "g2_random_from_seed_x2 slot %d" % s
        expect(G2F.jac_to_aff(case, out, 6 * s) == want, case, what + ": wrong point")
        check_bounded(case, out, 6 * s, 6, what + " (Jacobian)")
        expect(flags[s] == 0, case, what + ": infinity flag")
        expect((f2_res(out, 12 + 4 * s), f2_res(out, 14 + 4 * s)) == want, case, what + ": wrong affine point")
        check_bounded(case, out, 12 + 4 * s, 4, what + " (affine)", val_bound=1.25)
    check_row(case, out, [], [_sl(0, 20)], "g2_random_from_seed_x2")


def _x2_table(edges, rnd):
    """Wave 0: every pair (1, 1) but one, whose slot B needs ten candidates; wave 1: the same with slot A; then the directed
    pairs interleaved with random pairs of the classes 1, 2, 3, 4, 9, 10."""
    wave = 32
    cases = []
    for at, (a, b) in ((13, (1, 10)), (6, (10, 1))):
        w = [_x2_of_classes(1, 1, "calm wave")(rnd) for _ in range(wave)]
        w[at] = _x2_of_classes(a, b, "the one slow slot")(rnd)
        cases += w
    pool = list(edges)
    mixed = (1, 2, 3, 4, 9, 10)
    n = max(len(cases) + 2 * len(pool), 3 * wave + 5)
    while len(cases) < n:
        if pool and (len(cases) % 2 == 0 or len(cases) + len(pool) >= n):
            cases.append(pool.pop(0))
        else:
            cases.append(_x2_of_classes(rnd.choice(mixed), rnd.choice(mixed))(rnd))
    return cases


TABLES["G2_RANDOM_FROM_SEED_X2"] = _x2_table


# ---- job_hash_g2, job_hash_g2_x2 ----------------------------------------------------------------------------------------------
def hash_msg(i):
    return b"conf-hash-%d" % i


LONG_MSGS = [bytes([65 + n % 7]) * n for n in (135, 136, 137, 192, 300)]


def _pad(msg):
    return bytes(msg) + bytes([0xa5]) * 4


def _hash_g2_case(msg, fix, tag=""):
    return bcase([(0, _pad(msg))], [len(msg), int(fix)], "%s len=%d fix=%d" % (tag, len(msg), fix), msg=bytes(msg), fix=int(fix))


def hash_g2_ref(msg, fix):
    return o.g2_uncompressed(g2_random_ref(o.sha3_256(msg), fix))


def _rand_hash_msg(rnd):
    return hash_msg(class_seed(rnd, rnd.choice([1, 1, 2, 3])))


@spec("HASH_G2", lambda rnd: _hash_g2_case(_rand_hash_msg(rnd), rnd.randrange(2), "random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cls = seed_classes()
        cases = [_hash_g2_case(hash_msg(cls[k][0]), 1, "class %d" % k) for k in range(1, 11)]
        cases += [_hash_g2_case(hash_msg(cls[k][0]), 0, "class %d" % k) for k in (1, 2, 10)]
        cases += [_hash_g2_case(m, i % 2, "long") for i, m in enumerate(LONG_MSGS)] + [_hash_g2_case(b"", 1, "empty")]
        return cases
    check_row(case, out, [(0, hash_g2_ref(case.msg, case.fix))], [], "job_hash_g2")


def _hash_g2_x2_case(ma, mb, fix, null_b, tag=""):
    return bcase([(0, _pad(ma)), (MSG_B2, _pad(mb))], [len(ma), len(mb), int(fix) | (int(null_b) << 1)],
                 "%s len=(%d, %d) fix=%d null_b=%d" % (tag, len(ma), len(mb), fix, null_b), msgs=(bytes(ma), bytes(mb)), fix=int(fix),
                 null_b=int(null_b))


@spec("HASH_G2_X2", lambda rnd: _hash_g2_x2_case(_rand_hash_msg(rnd), _rand_hash_msg(rnd), rnd.randrange(2), rnd.random() < 0.2, "random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cls = seed_classes()
        cases = [_hash_g2_x2_case(hash_msg(cls[a][0]), hash_msg(cls[b][-1]), fix, 0, "pair (%d, %d)" % (a, b))
                 for a, b in X2_PAIRS for fix in (1, 0)]
        cases += [_hash_g2_x2_case(hash_msg(cls[a][0]), hash_msg(cls[b][0]), 1, 1, "out_b null (%d, %d)" % (a, b)) for a, b in ((1, 10), (10, 1), (2, 2))]
        cases += [_hash_g2_x2_case(LONG_MSGS[i], LONG_MSGS[j], 1, 0, "long") for i, j in ((0, 1), (2, 0), (3, 4))]
        cases += [_hash_g2_x2_case(b"", LONG_MSGS[1], 1, 0, "empty beside two blocks")]
        return cases
    want = [(0, hash_g2_ref(case.msgs[0], case.fix))]
    if not case.null_b:
        want.append((192, hash_g2_ref(case.msgs[1], case.fix)))
    check_row(case, out, want, [], "job_hash_g2_x2")


# ---- hash_g1_g2, xor_with_hash -------------------------------------------------------------------------------------------------
IDENTITY = {(1, "unc"): o.g1_uncompressed(None), (1, "comp"): o.g1_compressed(None), (2, "unc"): o.g2_uncompressed(None),
            (2, "comp"): o.g2_compressed(None)}
SIZE = {(1, "unc"): 96, (1, "comp"): 48, (2, "unc"): 192, (2, "comp"): 96}


def byte_ref(g, form, b):
    """(verdict, point) of an encoding by the oracle: the checked decode of a compressed form; parse + on-curve (no
    subgroup test, EncodedPoint::into_affine_unchecked + is_on_curve) of an uncompressed one."""
    def ref():
        E = o.E1 if g == 1 else o.E2
        try:
            if form == "comp":
                return True, (o.g1_from_compressed if g == 1 else o.g2_from_compressed)(bytes(b))
            p = (o.g1_from_uncompressed if g == 1 else o.g2_from_uncompressed)(bytes(b), check=False)
            return (True, p) if p is None or E.on_curve(p) else (False, None)
        except o.DecodeError:
            return False, None
    return cached("byteref", (g, form, bytes(b)), ref)


def _g1_operands():
    """G1 operands of the hash jobs (uncompressed): (kind, bytes); two valid points, the identity, three that do not decode."""
    def make():
        rnd = random.Random("g1-operands")
        p, q = g1_point(rnd), g1_point(rnd, False)  # (the uncompressed decode has no subgroup test: q is accepted)
        off = bytearray(o.g1_uncompressed(p))
        off[95] ^= 1
        flag = bytearray(o.g1_uncompressed(p))
        flag[0] |= 0x80
        return [("valid", o.g1_uncompressed(p)), ("valid", o.g1_uncompressed(q)), ("identity", o.g1_uncompressed(None)),
                ("bad", bytes(off)), ("bad", bytes(flag)), ("bad", bytes([0xff]) * 96)]
    return cached("g1operands", 0, make)


def _g1_operand(rnd, kind):
    return rnd.choice([b for k, b in _g1_operands() if k == kind])


HASH_LENS = [0, 63, 64, 65, 200]
MSG_POOL = [bytes([33 + (7 * n + i) % 90 for i in range(n)]) for n in HASH_LENS + [1, 32, 136]]


def hash_g1_g2_ref(g1, msg, fix):
    """(status, 192 bytes) of job_hash_g1_g2."""
    ok, p = byte_ref(1, "unc", g1)
    if not ok:
        return 3, (IDENTITY[(2, "unc")] if fix else bytes([0xff]) * 192)
    m = o.sha3_256(msg) if len(msg) > 64 else bytes(msg)
    return 0, o.g2_uncompressed(g2_random_ref(o.sha3_256(m + o.g1_compressed(p)), fix))


def _hash_g1_g2_case(g1, msg, fix, tag=""):
    return bcase([(0, g1), (96, _pad(msg))], [len(msg), int(fix)], "%s len=%d fix=%d" % (tag, len(msg), fix), g1=bytes(g1), msg=bytes(msg),
                 fix=int(fix))


def _rand_hash_g1_g2(rnd):
    kind = rnd.choice(["valid", "valid", "valid", "identity", "bad"])
    return _hash_g1_g2_case(_g1_operand(rnd, kind), rnd.choice(MSG_POOL), rnd.randrange(2), "random " + kind)


@spec("HASH_G1_G2", _rand_hash_g1_g2, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        ops = _g1_operands()
        return [_hash_g1_g2_case(ops[i][1], MSG_POOL[j], fix, ops[i][0]) for i in (0, 2, 3) for j in range(len(HASH_LENS)) for fix in (1, 0)] + \
               [_hash_g1_g2_case(ops[i][1], MSG_POOL[1], fix, ops[i][0]) for i in (1, 4, 5) for fix in (1, 0)]
    flags_agree(case, flags, 1)
    st, want = hash_g1_g2_ref(case.g1, case.msg, case.fix)
    expect(flags[0] == st, case, "job_hash_g1_g2: status %d, want %d" % (flags[0], st))
    check_row(case, out, [(0, want)], [], "job_hash_g1_g2")


def _hash_g1_g2_x2_case(a, b, fix, null_b, tag=""):
    return bcase([(0, a[0]), (96, b[0]), (MSG_A4, _pad(a[1])), (MSG_B4, _pad(b[1]))], [len(a[1]), len(b[1]), int(fix) | (int(null_b) << 1)],
                 "%s len=(%d, %d) fix=%d null_b=%d" % (tag, len(a[1]), len(b[1]), fix, null_b), ops=((bytes(a[0]), bytes(a[1])), (bytes(b[0]), bytes(b[1]))),
                 fix=int(fix), null_b=int(null_b))


def _rand_hash_g1_g2_x2(rnd):
    def operand():
        return (_g1_operand(rnd, rnd.choice(["valid", "valid", "valid", "identity", "bad"])), rnd.choice(MSG_POOL))
    return _hash_g1_g2_x2_case(operand(), operand(), rnd.randrange(2), rnd.random() < 0.2, "random")


@spec("HASH_G1_G2_X2", _rand_hash_g1_g2_x2, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        ops = _g1_operands()
        v, idn, bad = ops[0][1], ops[2][1], ops[3][1]
        m = MSG_POOL
        cases = []
        for fix in (1, 0):
            cases += [_hash_g1_g2_x2_case((v, m[1]), (bad, m[2]), fix, 0, "valid, bad"), _hash_g1_g2_x2_case((bad, m[1]), (v, m[2]), fix, 0, "bad, valid"),
                      _hash_g1_g2_x2_case((bad, m[3]), (ops[5][1], m[0]), fix, 0, "bad, bad"), _hash_g1_g2_x2_case((idn, m[4]), (v, m[0]), fix, 0, "identity, valid"),
                      _hash_g1_g2_x2_case((v, m[1]), (v, m[3]), fix, 0, "63 beside 65"), _hash_g1_g2_x2_case((v, m[3]), (v, m[2]), fix, 0, "65 beside 64"),
                      _hash_g1_g2_x2_case((v, m[2]), (idn, m[4]), fix, 0, "64 beside 200"), _hash_g1_g2_x2_case((bad, m[2]), (v, m[1]), fix, 1, "bad A, out_b null"),
                      _hash_g1_g2_x2_case((v, m[4]), (bad, m[1]), fix, 1, "bad B, out_b null")]
        return cases
    flags_agree(case, flags, 2)
    want = []
    for s, (g1, msg) in enumerate(case.ops):
        st, enc = hash_g1_g2_ref(g1, msg, case.fix)
        expect(flags[s] == st, case, "job_hash_g1_g2_x2: status %d of slot %d, want %d" % (flags[s], s, st))
        if s == 0 or not case.null_b:
            want.append((192 * s, enc))
    check_row(case, out, want, [], "job_hash_g1_g2_x2")


XOR_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 1000]


def _xor_case(g1, data, tag=""):
    return bcase([(0, g1), (96, _pad(data))], [len(data)], "%s len=%d" % (tag, len(data)), g1=bytes(g1), data=bytes(data))


def _rand_xor(rnd):
    kind = rnd.choice(["valid", "valid", "valid", "identity", "bad"])
    return _xor_case(_g1_operand(rnd, kind), rnd.randbytes(rnd.choice([rnd.randrange(0, 70), rnd.randrange(0, 70), rnd.randrange(70, 300)])), "random " + kind)


@spec("XOR_WITH_HASH", _rand_xor, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        ops = _g1_operands()
        cases = [_xor_case(ops[i % 3][1], rnd.randbytes(n), ops[i % 3][0]) for i, n in enumerate(XOR_LENS)]
        cases += [_xor_case(b, rnd.randbytes(n), k) for (k, b), n in zip(ops[3:], (17, 1000, 0))]
        cases += [_xor_case(ops[0][1], bytes(33), "zero data"), _xor_case(ops[0][1], bytes([0xff]) * 64, "ff data")]
        return cases
    flags_agree(case, flags, 1)
    ok, p = byte_ref(1, "unc", case.g1)
    expect(flags[0] == (0 if ok else 3), case, "job_xor_with_hash: status %d" % flags[0])
    check_row(case, out, [(0, o.xor_with_hash(p, case.data))] if ok else [], [], "job_xor_with_hash")


# ---- field codecs -----------------------------------------------------------------------------------------------------------
BE_VALUES = [0, 1, P - 1, P, P + 1, (1 << 381) - 1]


def _be48(v, top=0):
    return (v | (top << 381)).to_bytes(48, "big")


def _check_from_be(case, out, s, raw, what):
    l = out_limbs(out, s)
    check_product(case, l, raw * (RM * RM % P), what)
    expect(residue(l) == raw, case, what + ": residue")


def _from_be48_case(v, top, mask, tag=""):
    return bcase([(0, _be48(v, top))], [int(mask)], "%s v=%x top=%d mask=%d" % (tag, v, top, mask), v=v, top=top, mask=int(mask))


@spec("FQ_FROM_BE48", lambda rnd: _from_be48_case(rnd.randrange(P), rnd.choice([0, 0, rnd.randrange(8)]), rnd.randrange(2), "random"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [_from_be48_case(v, top, mask, "edge") for v in BE_VALUES for top in range(8) for mask in (0, 1)]
    raw = case.v if case.mask else case.v | (case.top << 381)
    flags_agree(case, flags, 1)
    expect(flags[0] == int(raw < P), case, "fq_from_be48: verdict %d" % flags[0])
    if raw < P:
        _check_from_be(case, out, 0, raw, "fq_from_be48")
    check_row(case, out, [], [_sl(0)], "fq_from_be48")


def _lazy_fq(rnd, v):
    """A lazy in-contract representation, as FQ_TO_CANONICAL takes them."""
    return rnd.choice([lambda: encode(v), lambda: encode(v, rnd.randint(0, 13), PT_IV, rnd.choice(PUSHES)),
                       lambda: encode(v, rnd.randint(-299, 299), (-7.9, 7.9), rnd.choice(PUSHES))])()


@spec("FQ_TO_BE48", lambda rnd: Case([_lazy_fq(rnd, rnd.randrange(P))], tag="random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [Case([_lazy_fq(rnd, v)], tag="edge %x" % v) for v in (0, 1, P - 1, HALF, HALF + 1, (1 << 380), 255, 256 << 376) for _ in range(3)] + \
               [Case([encode_int(P)], tag="p"), Case([encode(0, -300, (-7.9, 7.9))], tag="-300 p")]
    check_row(case, out, [(0, residue(case.slots[0].limbs).to_bytes(48, "big"))], [], "fq_to_be48")


LEX_VALUES = [0, HALF, HALF + 1, P - 1, 1, HALF - 1]


@spec("FQ_LEX_LARGEST", lambda rnd: Case([_lazy_fq(rnd, rnd.randrange(P))], tag="random"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        return [Case([_lazy_fq(rnd, v)], tag="edge %x" % v) for v in LEX_VALUES for _ in range(3)] + [Case([encode_int(P)], tag="p")]
    flags_agree(case, flags, 1)
    v = residue(case.slots[0].limbs)
    expect(flags[0] == int(v > HALF), case, "fq_lex_largest(%x) = %d" % (v, flags[0]))
    check_row(case, out, [], [], "fq_lex_largest")


def _from_be96_case(c1, c0, top1, top0, mask, tag=""):
    return bcase([(0, _be48(c1, top1) + _be48(c0, top0))], [int(mask)], "%s c1=%x top %d c0=%x top %d mask=%d" % (tag, c1, top1, c0, top0, mask),
                 c=(c0, c1), tops=(top0, top1), mask=int(mask))


def _rand_from_be96(rnd):
    return _from_be96_case(rnd.randrange(P), rnd.randrange(P), rnd.choice([0, 0, rnd.randrange(8)]), rnd.choice([0, 0, 0, rnd.randrange(8)]), rnd.randrange(2),
                           "random")


@spec("FQ2_FROM_BE96", _rand_from_be96, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        good = rnd.randrange(P)
        cases = [_from_be96_case(v, good, top, 0, mask, "c1") for v in BE_VALUES for top in (0, 5) for mask in (0, 1)]
        cases += [_from_be96_case(good, v, 0, 0, mask, "c0") for v in BE_VALUES for mask in (0, 1)]
        cases += [_from_be96_case(good, 1, top1, top0, 1, "flag bits in c0") for top0 in (1, 2, 4, 7) for top1 in (0, 7)]
        cases += [_from_be96_case(P, P, 0, 0, 1, "both out of range"), _from_be96_case(P - 1, P - 1, 7, 0, 1, "both q - 1")]
        return cases
    (c0, c1), (top0, top1) = case.c, case.tops
    raw1 = c1 if case.mask else c1 | (top1 << 381)
    raw0 = c0 | (top0 << 381)  # (the mask applies to c1, the half that carries the flags, only)
    ok = raw0 < P and raw1 < P
    flags_agree(case, flags, 1)
    expect(flags[0] == int(ok), case, "fq2_from_be96: verdict %d" % flags[0])
    if ok:
        _check_from_be(case, out, 0, raw0, "fq2_from_be96 c0")
        _check_from_be(case, out, 1, raw1, "fq2_from_be96 c1")
    check_row(case, out, [], [_sl(0, 2)], "fq2_from_be96")


def _lazy_fq2(rnd, v):
    return [_lazy_fq(rnd, v[0]), _lazy_fq(rnd, v[1])]


@spec("FQ2_TO_BE96", lambda rnd: Case(_lazy_fq2(rnd, (rnd.randrange(P), rnd.randrange(P))), tag="random"))
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        vs = [(a, b) for a in (0, 1, P - 1, HALF + 1) for b in (0, 1, P - 1, 1 << 380)]
        return [Case(_lazy_fq2(rnd, v), tag="edge %x, %x" % v) for v in vs] + [Case([encode_int(P), encode(0, -300, (-7.9, 7.9))], tag="p, -300 p")]
    c0, c1 = f2_in(case, 0)
    check_row(case, out, [(0, c1.to_bytes(48, "big") + c0.to_bytes(48, "big"))], [], "fq2_to_be96")


@spec("FQ2_LEX_LARGEST", lambda rnd: Case(_lazy_fq2(rnd, (rnd.randrange(P), rnd.choice([0, rnd.randrange(P)]))), tag="random"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = [Case(_lazy_fq2(rnd, (v, 0)), tag="c1 = 0, c0 = %x" % v) for v in LEX_VALUES for _ in range(2)]
        cases += [Case([_lazy_fq(rnd, v), encode_int(P)], tag="c1 = p, c0 = %x" % v) for v in (HALF, HALF + 1)]
        cases += [Case(_lazy_fq2(rnd, (v, w)), tag="c1 = %x, c0 = %x" % (w, v)) for w in (HALF, HALF + 1, 1, P - 1) for v in (0, P - 1, HALF + 1)]
        return cases
    flags_agree(case, flags, 1)
    c0, c1 = f2_in(case, 0)
    expect(flags[0] == int(c1 > HALF if c1 else c0 > HALF), case, "fq2_lex_largest = %d" % flags[0])
    check_row(case, out, [], [], "fq2_lex_largest")


# ---- point encodings: one shared table of byte strings per group and form ------------------------------------------------------
KINDS = ("valid", "identity", "bad flags", "x out of range", "non-square", "outside subgroup")


def _enc_x(g, x, form, y=None):
    """The bytes of a finite point's coordinates, flags not yet set (compressed: x alone)."""
    fe = (lambda v: v.to_bytes(48, "big")) if g == 1 else (lambda v: v[1].to_bytes(48, "big") + v[0].to_bytes(48, "big"))
    return fe(x) + (fe(y) if form == "unc" else b"")


def _set_top(b, top):
    b = bytearray(b)
    b[0] = (b[0] & 0x1f) | (top << 5)
    return bytes(b)


def _or_byte(b, k, v):
    b = bytearray(b)
    b[k] |= v
    return bytes(b)


def _non_square_x(g, rnd):
    while True:
        x = rnd.randrange(P) if g == 1 else (rnd.randrange(P), rnd.randrange(P))
        if g == 1 and pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1:
            return x
        if g == 2 and not f2_is_square(o.f2_add(o.f2_mul(o.f2_sqr(x), x), o._Fq2.b)):
            return x


def byte_cases(g, form):
    """The shared table of encodings of group g in form "unc" / "comp": [(tag, kind, bytes)], kind one of KINDS or None.
    The expected verdict of each is byte_ref's, that is the oracle's."""
    def make():
        rnd = random.Random("byte-cases-%d-%s" % (g, form))
        fld, E = (G1F, o.E1) if g == 1 else (G2F, o.E2)
        F = fld.F
        n = SIZE[(g, form)]
        flag = 0x80 if form == "comp" else 0
        enc = (o.g1_uncompressed, o.g1_compressed, o.g2_uncompressed, o.g2_compressed)[2 * (g - 1) + (form == "comp")]
        p = _pt(fld, rnd)
        q = _pt(fld, rnd, False)
        valid, ident = enc(p), IDENTITY[(g, form)]
        cs = []
        for top in range(8):  # all eight values of the top three bits
            want_top = (valid[0] >> 5)
            cs.append(("top bits %d on a valid payload" % top, "valid" if top == want_top else "bad flags" if form == "unc" or not top & 4 else None,
                       _set_top(valid, top)))
            cs.append(("top bits %d on a zero payload" % top, "identity" if top == ident[0] >> 5 else None, _set_top(bytes(n), top)))
        strays = [(0, 0x01), (0, 0x10), (n - 1, 0x01), (n // 2 - 5, 0x40)]
        if g == 2:
            strays += [(50, 0x02), (95, 0x80)]  # the half of the first 96 bytes that the other lane of the pair owns
        if form == "unc":
            strays += [(n // 2 + 3, 0x04), (n // 2, 0x20)]  # the y half
        cs += [("identity with a stray bit %02x in byte %d" % (v, k), "bad flags" if k == 0 else None, _or_byte(ident, k, v)) for k, v in strays]
        if form == "comp":
            cs.append(("identity with the sort bit", "bad flags", _or_byte(ident, 0, 0x20)))
        y = p[1]
        for v in (P, P + 1, (1 << 381) - 1):  # x out of range (G2: c1 alone, c0 alone, both)
            xs = [("x", v)] if g == 1 else [("x.c1", (p[0][0], v)), ("x.c0", (v, p[0][1])), ("x.c0 and x.c1", (v, v))]
            cs += [("%s = %x" % (t, v), "x out of range", _or_byte(_enc_x(g, x, form, y), 0, flag)) for t, x in xs]
        if form == "unc":
            ys = [("y", y + P)] if g == 1 else [("y.c1", (y[0], y[1] + P)), ("y.c0", (y[0] + P, y[1]))]
            cs += [("%s + q" % t, None, _enc_x(g, p[0], form, yy)) for t, yy in ys if max(yy if g == 2 else [yy]) < 1 << 384]
            cs.append(("(x, -y)", "valid", enc(E.neg(p))))
            cs.append(("off the curve", None, _enc_x(g, p[0], form, F.add(y, F.one))))
            cs.append(("on the curve, outside the subgroup", "outside subgroup", enc(q)))
            if g == 1:
                cs.append(("x = 0: (0, 2)", None, enc((0, 2))))
            else:
                y0 = o.f2_sqrt(o._Fq2.b)
                cs.append(("x = 0", None, _enc_x(g, (0, 0), form, y0 if y0 is not None else (2, 0))))
            cs.append(("flag bits in y's top byte", None, _or_byte(valid, n // 2, 0x80)))
        else:
            cs.append(("non-square right-hand side", "non-square", _or_byte(_enc_x(g, _non_square_x(g, rnd), form), 0, 0x80)))
            cs.append(("non-square right-hand side, sort bit", "non-square", _or_byte(_enc_x(g, _non_square_x(g, rnd), form), 0, 0xa0)))
            cs.append(("outside the subgroup", "outside subgroup", enc(q)))
            cs.append(("the other sort bit", "valid", _or_byte(valid, 0, 0x20) if not valid[0] & 0x20 else _set_top(valid, 4)))
            cs.append(("x = 0", None, _or_byte(bytes(n), 0, 0x80)))
            cs.append(("x = 0, sort bit", None, _or_byte(bytes(n), 0, 0xa0)))
            if g == 1:
                cs.append(("x = 0 of (0, 2): outside G1", None, o.g1_compressed((0, 2))))
        for tag, kind, b in cs:
            assert len(b) == n, tag
            if kind in ("valid", "identity"):
                assert byte_ref(g, form, b)[0], tag
            elif kind is not None and not (kind == "outside subgroup" and form == "unc"):
                assert not byte_ref(g, form, b)[0], tag
        return cs
    return cached("bytecases", (g, form), make)


def _decode_spec(op, g, form):
    fld = G1F if g == 1 else G2F
    w = fld.w
    other = "comp" if form == "unc" else "unc"
    enc_other = (o.g1_uncompressed, o.g1_compressed, o.g2_uncompressed, o.g2_compressed)[2 * (g - 1) + (other == "comp")]
    enc_same = (o.g1_uncompressed, o.g1_compressed, o.g2_uncompressed, o.g2_compressed)[2 * (g - 1) + (form == "comp")]

    def rand_case(rnd):
        p = _pt(fld, rnd)
        b = enc_same(p if rnd.random() < 0.5 else fld.E.neg(p))
        return bcase([(0, b)], [], "random valid", b=b)

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            return [bcase([(0, b)], [], tag, b=b) for tag, _, b in byte_cases(g, form)]
        ok, p = byte_ref(g, form, case.b)
        what = op.lower()
        flags_agree(case, flags, 3)
        expect(flags[0] == int(ok), case, "%s: verdict %d, the oracle's %d" % (what, flags[0], ok))
        if ok:
            expect(flags[1] == int(p is None), case, "%s: infinity flag %d" % (what, flags[1]))
            if p is not None:
                expect((fld.res(out, 0), fld.res(out, w)) == p, case, what + ": wrong point")
                check_bounded(case, out, 0, 2 * w, what, limb=LIMB_MAX)
        expect(flags[2] == (0 if ok else 3), case, "%s wrapper: status %d" % (what, flags[2]))
        check_row(case, out, [(WRAP, enc_other(p) if ok else IDENTITY[(g, other)])], [_sl(0, 2 * w)], what + " wrapper")
    spec(op, rand_case, nflags=3)(fn)


_decode_spec("G1_DECODE_UNCOMPRESSED", 1, "unc")
_decode_spec("G1_DECODE_COMPRESSED", 1, "comp")
_decode_spec("G2_DECODE_UNCOMPRESSED", 2, "unc")
_decode_spec("G2_DECODE_COMPRESSED", 2, "comp")


def kind_encoding(kind, which=0):
    """An encoding of the shared compressed G2 table of that kind."""
    return [b for _, k, b in byte_cases(2, "comp") if k == kind][which]


def _decode_x2_case(a, b, null_b, tag=""):
    return bcase([(0, a), (96, b)], [int(null_b)], "%s null_b=%d" % (tag, null_b), encs=(bytes(a), bytes(b)), null_b=int(null_b))


def _rand_decode_x2(rnd):
    def one():
        p = g2_point(rnd)
        return o.g2_compressed(p if rnd.random() < 0.5 else o.E2.neg(p))
    return _decode_x2_case(one(), one(), rnd.random() < 0.15, "random valid")


@spec("G2_DECODE_COMPRESSED_X2", _rand_decode_x2, nflags=4)
def _(case=None, out=None, flags=None, rnd=None):
    if rnd is not None:
        cases = [_decode_x2_case(kind_encoding(ka), kind_encoding(kb, -1), 0, "%s, %s" % (ka, kb)) for ka in KINDS for kb in KINDS]
        cases += [_decode_x2_case(kind_encoding(ka), kind_encoding("valid"), 1, "%s, out_b null" % ka) for ka in KINDS]
        # the identity with a stray bit (either lane's half), in each slot beside a valid point
        tbl = [(tag, b) for tag, _, b in byte_cases(2, "comp") if tag.startswith("identity with")]
        cases += [_decode_x2_case(b, kind_encoding("valid"), 0, tag + " in slot A") if i % 2 else _decode_x2_case(kind_encoding("valid"), b, 0, tag + " in slot B")
                  for i, (tag, b) in enumerate(tbl)]
        return cases
    flags_agree(case, flags, 4)
    want = []
    for s, b in enumerate(case.encs):
        ok, p = byte_ref(2, "comp", b)
        what = "g2_decode_compressed_x2 slot %d" % s
        expect(flags[s] & 1 == int(ok), case, "%s: verdict %d, the oracle's %d" % (what, flags[s] & 1, ok))
        expect(flags[s] >> 1 == int(p is None), case, "%s: infinity flag (a failed decode leaves the identity)" % what)
        if p is not None:
            expect((f2_res(out, 4 * s), f2_res(out, 4 * s + 2)) == p, case, what + ": wrong point")
            check_bounded(case, out, 4 * s, 4, what, limb=LIMB_MAX)
        expect(flags[2 + s] == (0 if ok else 3), case, "%s wrapper: status %d" % (what, flags[2 + s]))
        if s == 0 or not case.null_b:
            want.append((WRAP + 192 * s, o.g2_uncompressed(p)))
    check_row(case, out, want, [_sl(0, 8)], "job_decompress_g2_x2")


def _encode_spec(op, g, form):
    fld = G1F if g == 1 else G2F
    enc = (o.g1_uncompressed, o.g1_compressed, o.g2_uncompressed, o.g2_compressed)[2 * (g - 1) + (form == "comp")]

    def make(rnd, p, tag, canon=False):
        return mcase(aff_slots(fld, rnd, p, canon), aux=[int(p is None)], tag=tag, p=p)

    def rand_case(rnd):
        return make(rnd, _pt(fld, rnd, rnd.random() < 0.8), "random", rnd.random() < 0.3)

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            F = fld.F
            pts = whole_curve_points(fld, rnd)
            pts += [fld.E.neg(p) for p in pts[1:4]]
            cases = [make(rnd, p, "point %d" % i, i % 2 == 0) for i, p in enumerate(pts)]
            # y at the turn of the lexicographic order (not curve points: the encoders do not look)
            ys = [HALF, HALF + 1, 0, P - 1] if g == 1 else [(0, HALF), (0, HALF + 1), (HALF, 0), (HALF + 1, 0), (P - 1, HALF), (0, 0), (5, HALF + 1)]
            x = pts[1][0]
            cases += [make(rnd, (x, y), "y = %s" % (y,), i % 2 == 0) for i, y in enumerate(ys)]
            cases += [make(rnd, (F.zero, pts[1][1]), "x = 0"), make(rnd, (fld.F.sub(F.zero, F.one), pts[1][1]), "x = q - 1")]
            return cases
        check_row(case, out, [(0, enc(case.p))], [], op.lower())
    spec(op, rand_case)(fn)


_encode_spec("G1_ENCODE_UNCOMPRESSED", 1, "unc")
_encode_spec("G1_ENCODE_COMPRESSED", 1, "comp")
_encode_spec("G2_ENCODE_UNCOMPRESSED", 2, "unc")
_encode_spec("G2_ENCODE_COMPRESSED", 2, "comp")


# ---------------------------------------------------------------------------------------------------------------------
# the wave-uniform forms of the G2 share combination: scalar ops 128 .. 130, point ops 172 .. 177, byte op 214
#
# The routines read K, the coefficients, D or (q, T, E) from the wave's first active lane (wave_uniform), so a table of
# these ops is a sequence of aligned blocks of 32 jobs that share that key (uniform_table), with a ragged last block: every
# prefix sizes() launches keeps each wave uniform, because lanes past the end copy the last job.  Inside a block the
# directed special lanes stand at lane-pair positions 0, 31 and in the middle (uniform_block), ordinary ones around them.
# ---------------------------------------------------------------------------------------------------------------------
def header_constant(header, name):
    """An integer constant of a product header, read from its text (`name = 123`)."""
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(r"\b%s = (\d+)" % name, f.read()).group(1))


QUOT_WIDTH = header_constant("tc_gls.h", "kQuotWidth")
WNAF_COLS = header_constant("tc_gls.h", "kWnafCols")
MACS = {n: header_constant("tc_jobs.h", n) for n in ("kMacsDbl", "kMacsAdd", "kMacsPsi2", "kMacsUniformFixed", "kMacsQuotientFixed")}
WAVE_JOBS = 32  # lane pairs per wave


def ten_signer_denominators(K):
    """The generic denominators of the K-subsets of ten signers."""
    ds = {small_coeffs_model(list(s))[2] for s in itertools.combinations(range(10), K)}
    return sorted(d for d in ds if combine_class(d) == "generic")


TEN_DS = sorted(set(ten_signer_denominators(2)) | set(ten_signer_denominators(3)) | set(ten_signer_denominators(4)))
DIVIDE_UNIFORM_DS = TEN_DS + [286, 5720, 65521, (1 << 13) + 1, (1 << 16) + 1, (1 << 20) + 7, (1 << 32) + 15, (1 << 61) - 1, (1 << 62) - 57]
QUOTIENT_DS = (list(range(8)) + TEN_DS + [286, 5720, 65521, (1 << 13) - 1, (1 << 13) + 1, (1 << 16) - 1, (1 << 16) + 1, (1 << 32) - 1,
                                          (1 << 32) + 15, 3 ** 39, (1 << 61) - 1, (1 << 62) - 57, (1 << 62) - 1, 1 << 62, (1 << 62) + 1,
                                          (1 << 63) + 1] + [1 << a for a in range(63)] + [X - 1, X, X + 1])


def wnaf_model(d, W):
    """tc_gls.h wnaf_recode<W>: the 65 digits."""
    k, dig = d, []
    for _ in range(WNAF_COLS):
        m = 0
        if k & 1:
            m = k & ((1 << W) - 1)
            if m > 1 << (W - 1):
                m -= 1 << W
            k -= m
        dig.append(m)
        k >>= 1
    return dig


def naf_model(c):
    """tc_gls.h naf_recode: (pos, neg) as 64-bit masks (a digit in column 64 is dropped, as the routine drops it)."""
    c3 = 3 * c
    return ((c3 & ~c) >> 1) & M64, ((c & ~c3) >> 1) & M64


def signed_naf(c):
    p, m = naf_model(abs(c))
    return (m, p) if c < 0 else (p, m)


def quotient_decompose_model(D):
    """tc_gls.h combine_quotient_decompose step by step: None where it refuses D, else (q, T, E, wide, negative) -- wide:
    some division went through the bit-by-bit 128-bit path of udiv_u128_u64; negative: the rounding met n < 0."""
    if D < 3 or D & (D - 1) == 0 or D >> 62:
        return None
    q, x0 = divmod(X, D)
    wide = (x0 * x0) >> 64 != 0
    x2 = x0 * x0 % D
    wide |= (x2 * x2) >> 64 != 0
    r1 = (x2 * x2 - x2 + 1) % D
    if math.gcd(r1, D) != 1:
        return None
    k = D - pow(r1, -1, D)
    dig = [k, 0, -k, 0, k + 1]
    c, cs, es, negative = 0, [], [], False
    for g in dig:
        v = c * x0 + g
        n = 2 * v + D
        negative |= n < 0
        wide |= (n if n >= 0 else -n + 2 * D - 1) >> 64 != 0
        e = n // (2 * D)
        cs.append(c)
        es.append(e)
        c = v - e * D
    if c:
        return None
    T = [cs[4 - j] for j in range(4)]
    E = [es[4 - j] for j in range(4)]
    E[2] += es[0]
    E[0] -= es[0]
    for j in (1, 3):
        T[j], E[j] = -T[j], -E[j]
    return q, T, E, wide, negative


def quotient_scalar(q, T, E):
    """sum_j (T_j q + E_j) (-|x|)^j mod r: what [q] T(psi) P + E(psi) P multiplies a point of G2 by."""
    return sum((T[j] * q + E[j]) * (-X) ** j for j in range(4)) % R


def divide_macs_model(D):
    """tc_jobs.h combine_divide_uniform_macs and combine_divide_quotient_macs from the digit counts: (uniform, quotient)."""
    top = nz = nz2 = 0
    for j, d in enumerate(gls_digits(pow(D, -1, R))):
        for col, m in enumerate(wnaf_model(d, 4)):
            if m:
                nz += 1
                nz2 += j >> 1
                top = max(top, col)
    uni = MACS["kMacsUniformFixed"] + top * MACS["kMacsDbl"] + (nz - 1) * MACS["kMacsAdd"] + nz2 * MACS["kMacsPsi2"]
    q, T, E = quotient_decompose_model(D)[:3]
    nt, ne = [signed_naf(t) for t in T], [signed_naf(e) for e in E]
    any_t, any_e = 0, 0
    for p, m in nt:
        any_t |= p | m
    for p, m in ne:
        any_e |= p | m
    top, nz, nz2 = (any_e.bit_length() - 1 if any_e else 0), 0, 0
    for col, m in enumerate(wnaf_model(q, QUOT_WIDTH)):
        if m:
            nz += 1
            top = max(top, col)
    for j in range(4):
        n = bin(nt[j][0] | nt[j][1]).count("1") + bin(ne[j][0] | ne[j][1]).count("1")
        nz += n
        nz2 += (j >> 1) * n
    top += any_t.bit_length() - 1 if any_t else 0
    quo = MACS["kMacsQuotientFixed"] + top * MACS["kMacsDbl"] + (nz - 2) * MACS["kMacsAdd"] + nz2 * MACS["kMacsPsi2"]
    return uni & 0xffffffff, quo & 0xffffffff


def takes_quotient_model(D):
    if quotient_decompose_model(D) is None:
        return False
    uni, quo = divide_macs_model(D)
    return quo < uni


def _signed(w, bits=32):
    return w - (1 << bits) if w >> (bits - 1) else w


# ---- the scalar block: the recodings, the decomposition, the choice of the form ------------------------------------------
def _u64_case(v, tag=""):
    return scase(u32s(v, 2), tag="%s %d" % (tag, v), v=v)


@spec("WNAF_RECODE", lambda rnd: _u64_case(rnd.getrandbits(rnd.choice([8, 31, 62, 63, 64])), "random"))
def _(case=None, out=None, flags=None, rnd=None):
    """sum dig[i] 2^i = d, every digit odd or zero and below 2^(W-1), nonzero digits at least W columns apart (W = 4 and
    kQuotWidth); naf_recode: pos - neg = c (mod 2^64, and exactly for c < 2^63), disjoint, no two adjacent digits."""
    if rnd is not None:
        vals = [0, 1, 1 << 63, M64, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, X, X >> 16] + [7 << k for k in range(62)]
        vals += [X // d for d in QUOTIENT_DS if d]
        return [_u64_case(v, "edge") for v in vals]
    v, ws = case.v, out_words(out)
    for W, off in ((4, 0), (QUOT_WIDTH, WNAF_COLS)):
        dig = [_signed(w) for w in ws[off:off + WNAF_COLS]]
        expect(sum(d << i for i, d in enumerate(dig)) == v, case, "wnaf_recode<%d>: the digits do not sum to d: %s" % (W, dig))
        expect(all(d == 0 or (d % 2 == 1 and abs(d) < 1 << (W - 1)) for d in dig), case, "wnaf_recode<%d>: digit out of range: %s" % (W, dig))
        nz = [i for i, d in enumerate(dig) if d]
        expect(all(b - a >= W for a, b in zip(nz, nz[1:])), case, "wnaf_recode<%d>: nonzero digits closer than W: %s" % (W, dig))
    pos, neg = out_u64(out, WNAF_COLS), out_u64(out, WNAF_COLS + 1)
    expect((pos - neg) % (1 << 64) == v and pos & neg == 0, case, "naf_recode: pos %x neg %x" % (pos, neg))
    if v < 1 << 63:
        expect(pos - neg == v and ((pos | neg) & ((pos | neg) >> 1)) == 0, case, "naf_recode: pos %x neg %x is no NAF of c" % (pos, neg))


def _rand_quotient_d(rnd):
    return rnd.getrandbits(rnd.choice([4, 8, 13, 16, 24, 33, 48, 62, 63]))


@spec("COMBINE_QUOTIENT_DECOMPOSE", lambda rnd: _u64_case(_rand_quotient_d(rnd), "random D"), nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    """The routine's stated promise: true exactly for 3 <= D < 2^62 that is no power of two, and then q = floor(|x| / D) >= 3,
    |T_j| <= D / 2, |E_j| <= D / 2 + 2 and D sum_j (T_j q + E_j) (-|x|)^j = 1 (mod r).  (D = |x| - 1, |x|, |x| + 1 would give
    q = 1, 1, 0: they lie above 2^62 and are refused, so the promise q >= 3 holds.)"""
    if rnd is not None:
        return [_u64_case(d, "D") for d in QUOTIENT_DS]
    D = case.v
    want = 3 <= D < 1 << 62 and D & (D - 1) != 0
    expect(flags[0] == int(want), case, "combine_quotient_decompose returned %d" % flags[0])
    if not want:
        return
    q = out_u64(out, 0)
    T = [_signed(out_u64(out, 1 + j), 64) for j in range(4)]
    E = [_signed(out_u64(out, 5 + j), 64) for j in range(4)]
    expect(q == X // D and q >= 3, case, "q = %d" % q)
    expect(all(2 * abs(t) <= D for t in T), case, "|T_j| > D / 2: %s" % T)
    expect(all(2 * abs(e) <= D + 4 for e in E), case, "|E_j| > D / 2 + 2: %s" % E)
    expect(D * quotient_scalar(q, T, E) % R == 1, case, "D sum (T_j q + E_j) (-|x|)^j != 1 (mod r): q %d T %s E %s" % (q, T, E))
    m = quotient_decompose_model(D)
    expect(m is not None and (q, T, E) == m[:3], case, "q %d T %s E %s, the model's %s" % (q, T, E, m))


@spec("COMBINE_DIVIDE_CHOICE", lambda rnd: _u64_case(_rand_quotient_d(rnd), "random D"), nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """The two cost predictions restated from the digit counts and the kMacs* constants of tc_jobs.h, and the verdict
    "quotient < uniform"; a D the decomposition refuses never takes the quotient form."""
    if rnd is not None:
        return [_u64_case(d, "D") for d in QUOTIENT_DS]
    D = case.v
    ok = quotient_decompose_model(D) is not None
    expect(flags[1] == int(ok), case, "the decomposition exists: %d" % flags[1])
    if not ok:
        expect(flags[0] == 0, case, "takes the quotient form without a decomposition")
        return
    uni, quo = divide_macs_model(D)
    expect((out_u64(out, 0), out_u64(out, 1)) == (uni, quo), case, "predictions %d %d, want %d %d" % (out_u64(out, 0), out_u64(out, 1), uni, quo))
    expect(flags[0] == int(quo < uni), case, "combine_divide_takes_quotient = %d at %d against %d" % (flags[0], quo, uni))


# ---- the ladder models: the wave-uniform ladders walked on the oracle's group law ----------------------------------------
def straus_uniform_model(E, pts, cs):
    """straus_small_uniform: (sum c_k P_k, special).  special: the first base taken is at infinity, or a later addition
    meets acc = O, e = O or acc = +-e -- what the routine's exc must report, no more and no less."""
    nafs = [naf_model(c) for c in cs]
    anyb = 0
    for p, m in nafs:
        anyb |= p | m
    acc, started, special = _jac_of(E, None), False, False
    for bit in range(anyb.bit_length() - 1, -1, -1):
        if started:
            acc = E._jdbl(acc)
        for k, (p, m) in enumerate(nafs):
            s = ((p >> bit) & 1) - ((m >> bit) & 1)
            if s:
                acc, started, special = _uniform_take(E, acc, started, special, pts[k] if s > 0 else E.neg(pts[k]))
    return E._to_affine(acc), special


def _uniform_take(E, acc, started, special, e):
    """One digit of a wave-uniform ladder: the first base starts the accumulator, later ones are generic additions."""
    if started:
        acc, sp = _walk_add(E, acc, e)
        return acc, True, special or sp
    return _jac_of(E, e), True, special or e is None


def psi_power(p, j):
    for _ in range(j):
        p = psi(p)
    return p


def wnaf_ladder_model(p, D):
    """combine_divide_uniform = g2_wnaf_table + g2_wnaf_ladder over the base-|x| digits of D^-1 mod r:
    (sum_j d_j (-psi)^j P, special).  On G2 the point is [1 / D] P; elsewhere (psi != [x]) it is the reference itself."""
    E = o.E2
    if p is None or E.dbl(p) is None:
        return None, True
    odd = [E.mul(p, 2 * m + 1) for m in range(4)]
    digs = [wnaf_model(d, 4) for d in gls_digits(pow(D, -1, R))]
    acc, started, special = _jac_of(E, None), False, False
    for col in range(WNAF_COLS - 1, -1, -1):
        if started:
            acc = E._jdbl(acc)
        for j in range(4):
            m = digs[j][col]
            if m:
                e = psi_power(odd[abs(m) >> 1], j)
                if (m < 0) != (j % 2 == 1):  # the bases are P, -psi(P), psi^2(P), -psi^3(P)
                    e = E.neg(e)
                acc, started, special = _uniform_take(E, acc, started, special, e)
    return E._to_affine(acc), special


def quotient_mul_model(p, q, T, Ec):
    """g2_quotient_mul: ([q] T(psi) P + E(psi) P, special) with T(psi) P = sum_j T_j psi^j(P)."""
    E = o.E2
    bases = [psi_power(p, j) for j in range(4)]

    def add_bases(acc, started, special, nafs, bit):
        for j, (pos, neg) in enumerate(nafs):
            s = ((pos >> bit) & 1) - ((neg >> bit) & 1)
            if s:
                acc, started, special = _uniform_take(E, acc, started, special, bases[j] if s > 0 else E.neg(bases[j]))
        return acc, started, special

    nt, ne = [signed_naf(t) for t in T], [signed_naf(e) for e in Ec]
    any_t = any_e = 0
    for pos, neg in nt:
        any_t |= pos | neg
    for pos, neg in ne:
        any_e |= pos | neg
    acc, started, special = _jac_of(E, None), False, False
    for bit in range(any_t.bit_length() - 1, -1, -1):
        if started:
            acc = E._jdbl(acc)
        acc, started, special = add_bases(acc, started, special, nt, bit)
    special |= not started
    p1 = E._to_affine(acc)
    tab = [p1, E.mul(p1, 3)]  # (kQuotWidth = 3: P1 and 3 P1)
    assert QUOT_WIDTH == 3
    special |= p1 is None or E.dbl(p1) is None or tab[1] is None
    dig = wnaf_model(q, QUOT_WIDTH)
    top = max([any_e.bit_length() - 1 if any_e else 0] + [col for col, m in enumerate(dig) if m])
    acc, started = _jac_of(E, None), False
    for col in range(top, -1, -1):
        if started:
            acc = E._jdbl(acc)
        m = dig[col]
        if m:
            e = tab[abs(m) >> 1]
            acc, started, special = _uniform_take(E, acc, started, special, e if m > 0 else E.neg(e))
        if col < 64:
            acc, started, special = add_bases(acc, started, special, ne, col)
    special |= not started
    return E._to_affine(acc), special


# ---- the wave layout of the uniform ops --------------------------------------------------------------------------------------
# where a block's directed cases stand, the special ones first (_special_first): both ends, then the middle; every third block
# keeps an ordinary job in the first lane, every third in the last one
SPECIAL_AT = ((0, 31, 13, 14, 7, 22, 1, 30, 16, 5, 26, 10), (31, 13, 14, 7, 22, 1, 30, 16, 5, 26, 10, 2), (0, 13, 14, 7, 22, 1, 30, 16, 5, 26, 10, 29))
UNIFORM = {}  # op -> (key of a case, special of a case or None): what test_wave_layout_of_uniform_ops reads
_POOL = {}


def g2_pool():
    """A handful of points of G2 that the uniform tables reuse (a reference costs a Python multiplication per distinct point)."""
    if "g2" not in _POOL:
        rnd = random.Random("uniform-pool")
        _POOL["g2"] = [g2_point(rnd) for _ in range(8)]
        _POOL["curve"] = [curve_point(G2F, rnd) for _ in range(2)]
    return _POOL["g2"]


def curve_pool():
    g2_pool()
    return _POOL["curve"]


def uniform_block(directed, ordinary, n=WAVE_JOBS, variant=0):
    """One block: makers of directed cases at SPECIAL_AT[variant % 3] (those that fit below n), ordinary(i) everywhere else."""
    assert len(directed) <= len(SPECIAL_AT[0])
    at = {p: make for p, make in zip(SPECIAL_AT[variant % 3], directed) if p < n}
    return [at[i]() if i in at else ordinary(i) for i in range(n)]


def uniform_table(op, blocks):
    key_of = UNIFORM[op][0]
    assert all(len(b) == WAVE_JOBS for b in blocks[:-1]) and 0 < len(blocks[-1]) < WAVE_JOBS
    assert all(len({key_of(c) for c in b}) == 1 for b in blocks), op
    return [c for b in blocks for c in b]


def whole_table(op):
    """A spec whose directed cases ARE the table (TABLES hook)."""
    TABLES[op] = lambda edges, rnd: edges


def _special_first(makers, special_of):
    """Directed makers ordered so that the special ones come first (positions 0 and 31)."""
    probe = [(m, special_of(m())) for m in makers]
    return [m for m, s in probe if s] + [m for m, s in probe if not s]


# ---- straus_small_uniform ------------------------------------------------------------------------------------------------------
def ten_signer_tuples(K):
    """(indices, c_abs, D) of the K-subsets of ten signers, the longest coefficients first: 9 bits for K = 4 (twelve subsets),
    7 bits for K = 3, 4 bits for K = 2."""
    out = [(list(s),) + tuple(small_coeffs_model(list(s))[i] for i in (0, 2)) for s in itertools.combinations(range(10), K)]
    return sorted(out, key=lambda t: -max(t[1]))


def _straus_uniform_ref(case):
    def ref():
        E = o.E2
        want = None
        for p, c in zip(case.pts, case.cs):
            want = E.add(want, E.mul(p, c))
        return want, straus_uniform_model(E, case.pts, case.cs)[1]
    return cached("straus-uniform", (tuple(case.cs), tuple(case.pts)), ref)


def related_point_sets(K, b):
    """Points that meet the exception in mid-ladder, not at the start: with c = (3, 1) the accumulator reaches 3 P0 (the NAF
    of 3 is 4 - 1) and then adds P1 = +-3 P0; with c = (2, 1) the doubling P1 = 2 P0 and the cancellation P1 = -2 P0 fire in
    the LAST column, with c = (4, 2) in the first column after the start."""
    E = o.E2
    p3, p2 = E.mul(b[0], 3), E.dbl(b[0])
    return [("P1 = 3 P0", [b[0], p3] + b[2:K]), ("P1 = -3 P0", [b[0], E.neg(p3)] + b[2:K]), ("P1 = 2 P0", [b[0], p2] + b[2:K]),
            ("P1 = -2 P0", [b[0], E.neg(p2)] + b[2:K])]


def _straus_uniform_keys(K):
    big = (1 << 63) - 1
    keys = [[3, 1] + [0] * (K - 2), [2, 1] + [0] * (K - 2), [4, 2] + [0] * (K - 2), [0] * K, [1] + [0] * (K - 1), [0] * (K - 1) + [1], [1] * K,
            [1 << 62] + [1, 2, 3][:K - 1], [big] * K]
    return keys + [c for _, c, _ in ten_signer_tuples(K)[:2]]


def _uniform_point_sets(rnd, K):
    pool = g2_pool()
    ordinary = [[pool[(3 * i + k) % len(pool)] for k in range(K)] for i in range(3)]
    return ordinary, _point_sets(G2F, rnd, K)[1:] + related_point_sets(K, ordinary[0])


@spec("G2_STRAUS_SMALL_UNIFORM", None, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """exc equals the model's `special` on every job -- a spurious flag is a failure: maybe_zero56 errs with probability
    2^-46 per addition --, and the point is sum c_k P_k wherever it is false (unspecified where it is true)."""
    if rnd is not None:
        blocks, specials = [], []
        for K in (2, 3, 4):
            ordinary, sets = _uniform_point_sets(rnd, K)
            for cs in _straus_uniform_keys(K):
                few = sets if max(cs) < 1 << 32 else sets[:2] + sets[-4:-2]  # (a long ladder: fewer distinct references)
                def mk(pts, tag, cs=cs):
                    return lambda: _small_mul_case(G2F, rnd, pts, cs, tag, rnd.random() < 0.3)
                directed = _special_first([mk(pts, tag) for tag, pts in few], lambda c: _straus_uniform_ref(c)[1])
                specials += [m for m in directed if K == 2 and cs == [1, 1] and _straus_uniform_ref(m())[1]]
                blocks.append(uniform_block(directed, lambda i, cs=cs: mk(ordinary[i % 3], "ordinary", cs)(), variant=len(blocks)))
        blocks.append([specials[i % len(specials)]() for i in range(WAVE_JOBS)])  # every job special
        pool = g2_pool()
        blocks.append(uniform_block([], lambda i: _small_mul_case(G2F, rnd, [pool[i % 3], pool[3 + i % 4]], [5, 9], "ordinary")))
        blocks.append(blocks[0][:7])
        return uniform_table("G2_STRAUS_SMALL_UNIFORM", blocks)
    want, special = _straus_uniform_ref(case)
    flags_agree(case, flags, 2)
    expect(flags[1] == int(special), case, "straus_small_uniform: exc = %d, the model's special = %d" % (flags[1], special))
    if not special:
        check_result(G2F, case, out, flags, want, "straus_small_uniform")


UNIFORM["G2_STRAUS_SMALL_UNIFORM"] = (lambda c: (len(c.cs), tuple(c.cs)), lambda c: _straus_uniform_ref(c)[1])
whole_table("G2_STRAUS_SMALL_UNIFORM")


# ---- g2_wnaf_table ---------------------------------------------------------------------------------------------------------------
def order_two_point(rnd):
    """(x, 0): of order two under the a = 0 group law, on the curve y^2 = x^3 - x^3 (the law never reads b)."""
    return ((rnd.randrange(1, P), rnd.randrange(P)), (0, 0))


def order_three_point(rnd):
    """(0, y): 2 P = (0, -y) = -P under the a = 0 group law, so 3 P = O, 5 P = -P and 7 P = P."""
    return ((0, 0), (rnd.randrange(1, P), rnd.randrange(P)))


def j0_curve_orders():
    """The orders of the six curves y^2 = x^3 + c over Fq2 (the sextic twists of one another), from the trace of E(Fq)."""
    t1 = 1 - X
    t2 = t1 * t1 - 2 * P
    f = math.isqrt((4 * P * P - t2 * t2) // 3)
    assert 3 * f * f == 4 * P * P - t2 * t2 and (P + 1 - t1) % R == 0
    return [P * P + 1 - t for t in (t2, -t2, (t2 + 3 * f) // 2, (t2 - 3 * f) // 2, (-t2 + 3 * f) // 2, (-t2 - 3 * f) // 2)]


def order_seven_point():
    """A point of order seven of the one curve y^2 = x^3 + c over Fq2 whose order 7 divides (none has a point of order five,
    so 5 P = O cannot be met by operands in Fq2; E' itself has none of order 3, 5 or 7).  7 P = O: entries 3 and 7."""
    if "seven" not in _POOL:
        E, F = o.E2, G2F.F
        rnd = random.Random("order-seven")
        assert H2 * R in j0_curve_orders() and not any(n % 5 == 0 for n in j0_curve_orders())
        n, = [n for n in j0_curve_orders() if n % 7 == 0]
        m = n
        while m % 7 == 0:
            m //= 7
        while "seven" not in _POOL:
            x, c = (rnd.randrange(P), rnd.randrange(P)), (rnd.randrange(P), rnd.randrange(P))
            y = o.f2_sqrt(F.add(F.mul(F.sqr(x), x), c))
            if y is None or E.mul((x, y), n) is not None:  # (not on a curve of that class)
                continue
            p7 = E.mul((x, y), m)
            while p7 is not None and E.mul(p7, 7) is not None:
                p7 = E.mul(p7, 7)
            if p7 is not None:
                _POOL["seven"] = p7
    return _POOL["seven"]


def _wnaf_table_special(p):
    return p is None or o.E2.dbl(p) is None


@spec("G2_WNAF_TABLE", None, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """Entry m < 4, taken back to the original curve as (x / zn^2, y / zn^3), is [2 m + 1] P, entry 4 + m is psi of entry m on
    the scaled curve, and every stored coordinate is inside the table-entry contract.  exc is raised by the table for the
    identity and for a point of order two (no table can be built); a point of small odd order only carries the infinity
    bit of its entry (3 P = O: entries 1 and 5; 7 P = O: entries 3 and 7) into the ladder, which raises exc when it meets
    that entry.  E'(Fq2) has no points of order 3, 5 or 7 (its cofactor is prime to 105), but the group law never reads b:
    the operand of order three is (0, y), a point of y^2 = x^3 + y^2, the one of order seven lies on the one sextic twist
    whose order 7 divides, and no curve y^2 = x^3 + c over Fq2 has a point of order five (order_seven_point)."""
    if rnd is not None:
        pool, small = g2_pool(), small_points(G2F)

        def mk(p, tag):
            return lambda: _jac_case(G2F, rnd, p, tag)
        special = [mk(None, "P = O"), mk(None, "P = O"), mk(order_two_point(rnd), "order two"), mk(order_two_point(rnd), "order two")]
        carried = [mk(order_three_point(rnd), "order three"), mk(order_seven_point(), "order seven"), mk(small[0], "order 13"), mk(small[1], "order 23"), mk(curve_pool()[0], "outside G2"),
                   mk(order_three_point(rnd), "order three")]
        blocks = [uniform_block(special + carried, lambda i: mk(pool[i % 4], "ordinary")()),
                  [special[i % 4]() for i in range(WAVE_JOBS)],
                  uniform_block([], lambda i: mk(pool[i % 8], "ordinary")()),
                  uniform_block(carried + special, lambda i: mk(pool[4 + i % 4], "ordinary")()),
                  uniform_block(special, lambda i: mk(pool[i % 4], "ordinary")(), variant=1),
                  uniform_block(special, lambda i: mk(pool[i % 4], "ordinary")(), variant=2),
                  uniform_block(special[:1], lambda i: mk(pool[i % 3], "ordinary")(), 9)]
        return uniform_table("G2_WNAF_TABLE", blocks)
    E, F = o.E2, G2F.F
    special = _wnaf_table_special(case.p)
    flags_agree(case, flags, 2)
    expect(flags[1] == int(special), case, "g2_wnaf_table: exc = %d, want %d" % (flags[1], special))
    if special:
        return
    want = cached("wnaf-table", case.p, lambda: [E.mul(case.p, 2 * m + 1) for m in range(4)])
    inf = sum((1 << m | 1 << (4 + m)) for m, e in enumerate(want) if e is None)
    expect(flags[0] == inf, case, "g2_wnaf_table: infinity bits %x, want %x" % (flags[0], inf))
    zi = (pow(residue(out[32]), -1, P), 0)
    zi2, zi3 = F.sqr(zi), F.mul(F.sqr(zi), zi)
    for m, e in enumerate(want):
        if e is None:
            continue
        raw = (G2F.res(out, 4 * m), G2F.res(out, 4 * m + 2))
        expect((F.mul(raw[0], zi2), F.mul(raw[1], zi3)) == e, case, "g2_wnaf_table: entry %d is not [%d] P at Z = zn" % (m, 2 * m + 1))
        expect((G2F.res(out, 16 + 4 * m), G2F.res(out, 18 + 4 * m)) == psi(raw), case, "g2_wnaf_table: entry %d is not psi of entry %d" % (4 + m, m))
        check_bounded(case, out, 4 * m, 4, "g2_wnaf_table entry %d" % m, val_bound=2.1)
        check_bounded(case, out, 16 + 4 * m, 4, "g2_wnaf_table entry %d" % (4 + m), val_bound=2.1)


UNIFORM["G2_WNAF_TABLE"] = (lambda c: None, lambda c: _wnaf_table_special(c.p))
whole_table("G2_WNAF_TABLE")


# ---- combine_divide_uniform, combine_divide_quotient: both forms of [1 / D] for every D -------------------------------------------
def _divide_uniform_ref(op, case):
    def ref():
        if op == "G2_COMBINE_DIVIDE_UNIFORM":
            res, special = wnaf_ladder_model(case.p, case.d)
        else:
            m = quotient_decompose_model(case.d)
            res, special = (None, True) if m is None else quotient_mul_model(case.p, m[0], m[1], m[2])
        if case.sub and not special:
            res = o.E2.mul(case.p, pow(case.d, -1, R))
        return res, special
    return cached(op, (case.d, case.p), ref)


def _divide_uniform_spec(op, extra_ds):
    def mk(rnd, p, d, tag, sub):
        return lambda: _jac_case(G2F, rnd, p, "%s D=%d" % (tag, d), u32s(d, 2), d=d, sub=sub)

    def fn(case=None, out=None, flags=None, rnd=None):
        if rnd is not None:
            pool, small, curve = g2_pool(), small_points(G2F), curve_pool()
            blocks = []
            for i, d in enumerate(DIVIDE_UNIFORM_DS + extra_ds):
                directed = [mk(rnd, None, d, "Q = O", True), mk(rnd, None, d, "Q = O", True), mk(rnd, small[i % len(small)], d, "small order", False),
                            mk(rnd, curve[i % 2], d, "outside G2", False)]
                directed = _special_first(directed, lambda c: _divide_uniform_ref(op, c)[1])
                ordinary = lambda k, d=d, i=i: mk(rnd, pool[(i + k % 3) % len(pool)], d, "ordinary", True)()
                blocks.append(uniform_block(directed, ordinary, variant=i))
                if i == 0:
                    blocks.append([mk(rnd, None, d, "Q = O", True)() for _ in range(WAVE_JOBS)])  # every job special
                    blocks.append(uniform_block([], ordinary))  # none
            blocks.append(blocks[3][:11])
            return uniform_table(op, blocks)
        want, special = _divide_uniform_ref(op, case)
        flags_agree(case, flags, 2)
        expect(flags[1] == int(special), case, "%s: exc = %d, the model's special = %d" % (op, flags[1], special))
        if not special:
            check_result(G2F, case, out, flags, want, op.lower())
    spec(op, None, nflags=2)(fn)
    UNIFORM[op] = (lambda c: c.d, lambda c: _divide_uniform_ref(op, c)[1])
    whole_table(op)


_divide_uniform_spec("G2_COMBINE_DIVIDE_UNIFORM", [])
_divide_uniform_spec("G2_COMBINE_DIVIDE_QUOTIENT", [1, 2, 4, 1 << 20])  # (refused by the decomposition: exc on every job)


# ---- g2_quotient_mul with q, T, E given freely -------------------------------------------------------------------------------------
def _quotient_keys():
    """What no D reaches: T = 0, E = 0, T a single +-1, E longer than q, q = 3 and 2^63 + 1, a digit of q in column 64 beside
    bits of E in column 63, negative T and E of 2^61 -- and a few real decompositions."""
    keys = [quotient_decompose_model(d)[:3] for d in (7, 3, 189, 65521)]
    q7, t7, e7 = keys[0]
    keys += [(q7, [0, 0, 0, 0], e7), (q7, t7, [0, 0, 0, 0])]
    keys += [(q7, [s if j == k else 0 for j in range(4)], [1, 0, -1, 2]) for k in range(4) for s in (1, -1)]
    keys += [(3, [1, 0, 0, 0], [(1 << 20) + 1, 0, -5, 0]), (3, t7, e7), ((1 << 63) + 1, [1, -1, 0, 2], [0, 3, 0, -1]),
             (M64, [1, 0, 0, 0], [(1 << 63) - 1, 0, -1, 0]), (X // 5, [-(1 << 61), 0, 1 << 61, 0], [1 << 61, -(1 << 61), 0, 0])]
    return [(q, tuple(T), tuple(E)) for q, T, E in keys]


def _quotient_mul_ref(case):
    def ref():
        q, T, E = case.key
        res, special = quotient_mul_model(case.p, q, T, E)
        if case.sub and not special:
            res = o.E2.mul(case.p, quotient_scalar(q, T, E))
        return res, special
    return cached("quotient-mul", (case.key, case.p), ref)


@spec("G2_QUOTIENT_MUL", None, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """[q] T(psi) P + E(psi) P by the model (on G2: the multiple by sum_j (T_j q + E_j) (-|x|)^j), exc = the model's special."""
    if rnd is not None:
        pool, small, curve = g2_pool(), small_points(G2F), curve_pool()

        def mk(p, key, tag, sub):
            q, T, E = key
            ws = u64_words([q] + [t % (1 << 64) for t in T] + [e % (1 << 64) for e in E])
            return lambda: _jac_case(G2F, rnd, p, "%s q=%x T=%s E=%s" % (tag, q, list(T), list(E)), ws, key=key, sub=sub)
        blocks = []
        for i, key in enumerate(_quotient_keys()):
            directed = [mk(None, key, "P = O", True), mk(None, key, "P = O", True), mk(small[i % len(small)], key, "small order", False),
                        mk(curve[i % 2], key, "outside G2", False)]
            blocks.append(uniform_block(_special_first(directed, lambda c: _quotient_mul_ref(c)[1]),
                                        lambda k, key=key, i=i: mk(pool[(i + k % 3) % len(pool)], key, "ordinary", True)(), variant=i))
            if i == 0:
                blocks.append(uniform_block([], lambda k: mk(pool[k % 3], key, "ordinary", True)()))
        blocks.append(blocks[0][:5])
        return uniform_table("G2_QUOTIENT_MUL", blocks)
    want, special = _quotient_mul_ref(case)
    flags_agree(case, flags, 2)
    expect(flags[1] == int(special), case, "g2_quotient_mul: exc = %d, the model's special = %d" % (flags[1], special))
    if not special:
        check_result(G2F, case, out, flags, want, "g2_quotient_mul")


UNIFORM["G2_QUOTIENT_MUL"] = (lambda c: c.key, lambda c: _quotient_mul_ref(c)[1])
whole_table("G2_QUOTIENT_MUL")


# ---- combine_uniform_wave: no flag -- the routine repairs its own exceptional lanes ------------------------------------------------
def uniform_wave_tuples():
    """Ten-signer index tuples of each class, with the real lagrange_small_coeffs outputs: D = 1, a power of two, a D that takes
    the quotient form -- and (0, 10, 100, 1000), D = 81 000 000, which keeps the 4-dimensional ladder."""
    out = []
    for K in (2, 3, 4):
        seen = set()
        for s in itertools.combinations(range(10), K):
            c, _, D = small_coeffs_model(list(s))
            cls = combine_class(D)
            if cls == "generic":
                cls = "quotient" if takes_quotient_model(D) else "ladder"
            if (cls, D > 20) not in seen and len([1 for k in seen if k[0] == cls]) < 2:
                seen.add((cls, D > 20))
                out.append((list(s), c, D, cls))
    c, _, D = small_coeffs_model([0, 10, 100, 1000])
    out.append(([0, 10, 100, 1000], c, D, "quotient" if takes_quotient_model(D) else "ladder"))
    return out


def _uniform_wave_case(rnd, pts, cs, d, neg, tag, sub=True):
    K = len(pts)
    slots = sum((aff_slots(G2F, rnd, p, rnd.random() < 0.3) for p in pts), []) + [encode(0)] * (4 * (4 - K))
    return mcase(slots, u64_words(list(cs) + [0] * (4 - K) + [d]), [K, inf_mask(pts), int(neg)],
                 "K=%d %s c=%s D=%s%d" % (K, tag, list(cs), "-" if neg else "", d), pts=pts, cs=list(cs), d=d, neg=neg, sub=sub)


def _uniform_divide_model(a, d):
    """The [1 / D] step of combine_uniform_wave for a generic D on ANY point: the fast form the prediction picks, and where
    that raises its flag the 4-dimensional GLS multiplication of combine_divide.  (fast result or fallback, fast special)"""
    if takes_quotient_model(d):
        q, T, Ec = quotient_decompose_model(d)[:3]
        res, special = quotient_mul_model(a, q, T, Ec)
    else:
        res, special = wnaf_ladder_model(a, d)
    return (mul_gls_model(a, pow(d, -1, R))[0] if special and a is not None else res), special


def _uniform_wave_ref(case):
    def ref():
        E = o.E2
        s = None
        for p, c in zip(case.pts, case.cs):
            s = E.add(s, E.mul(p, c))
        if case.sub:
            return E.mul(s, pow(-case.d if case.neg else case.d, -1, R))
        r = _uniform_divide_model(s, case.d)[0]
        return E.neg(r) if case.neg else r
    return cached("uniform-wave", (tuple(case.cs), case.d, case.neg, tuple(case.pts)), ref)


def _uniform_wave_special(case):
    """A lane that the fast forms cannot finish by themselves: the short ladder meets an exception, the sum is O, or the
    [1 / D] ladder meets an exception on a sum of small order."""
    E = o.E2
    s, special = straus_uniform_model(E, case.pts, case.cs)
    return special or s is None or (not case.sub and _uniform_divide_model(s, case.d)[1])


def small_order_sum_points(K, cs, d):
    """Multiples of ONE point of order 13 whose combination is not O: the only lanes of this op outside G2.  On G2 the [1 / D]
    ladders meet no exception except on a sum at infinity, where even an unrepaired result has Z = 0; a sum of small order
    makes them meet one with the accumulator anywhere, so these lanes are the ones that show whether the repair after the
    [1 / D] step took place.  Their reference is the model's: the form that ran, on the oracle's group law."""
    E = o.E2
    s = small_points(G2F)[0]
    for ms in itertools.product(range(1, 13), repeat=K):
        pts = [E.mul(s, m) for m in ms]
        a = None
        for p, c in zip(pts, cs):
            a = E.add(a, E.mul(p, c))
        if a is not None and _uniform_divide_model(a, d)[1]:
            return pts
    raise AssertionError("no small-order sum that meets an exception for D = %d" % d)


def zero_sum_points(pts, cs):
    """The last point replaced so that sum c_k P_k = O: the [1 / D] step then starts from the identity."""
    E = o.E2
    s = None
    for p, c in zip(pts[:-1], cs[:-1]):
        s = E.add(s, E.mul(p, c))
    return pts[:-1] + [E.mul(E.neg(s), pow(cs[-1], -1, R))]


@spec("G2_COMBINE_UNIFORM_WAVE", None, nflags=1)
def _(case=None, out=None, flags=None, rnd=None):
    """[+-1 / D] sum c_k P_k on EVERY lane: combine_uniform_wave recomputes the lanes whose fast form raised its flag (the select
    under wave_any), so no job may differ.  Operands are points of G2 and the identity only: the fast form and its fallback
    use different decompositions of D^-1 mod r (digits of psi against the quotient of |x|), equal on G2 but not outside it.
    The one exception is a lane per generic wave whose points are multiples of one point of order 13
    (small_order_sum_points): its reference is the model of the form that ran."""
    if rnd is not None:
        blocks = []
        for i, (ids, cs, d, cls) in enumerate(uniform_wave_tuples()):
            K = len(cs)
            ordinary, sets = _uniform_point_sets(rnd, K)
            sets = sets[:6] + [("sum = O", zero_sum_points(ordinary[1], cs)), ("sum = O", zero_sum_points(ordinary[2], cs))]
            for neg in (False, True):
                def mk(pts, tag, cs=cs, d=d, neg=neg, sub=True):
                    return lambda: _uniform_wave_case(rnd, pts, cs, d, neg, "%s %s" % (cls, tag), sub)
                half = sets[::2] if neg else sets[1::2]
                directed = [mk(pts, tag) for tag, pts in half]
                if cls in ("quotient", "ladder"):  # (the other classes have no fast [1 / D] form to repair)
                    directed.append(mk(small_order_sum_points(K, cs, d), "sum of order 13", sub=False))
                directed = _special_first(directed, _uniform_wave_special)
                blocks.append(uniform_block(directed, lambda k, mk=mk: mk(ordinary[k % 3], "ordinary")(), variant=len(blocks)))
                if i == 0 and not neg:
                    blocks.append([directed[k % 2]() for k in range(WAVE_JOBS)])  # every job exceptional
                    blocks.append(uniform_block([], lambda k, mk=mk: mk(ordinary[k % 3], "ordinary")()))
        blocks.append(blocks[-1][:13])
        return uniform_table("G2_COMBINE_UNIFORM_WAVE", blocks)
    check_result(G2F, case, out, flags, _uniform_wave_ref(case), "combine_uniform_wave")


UNIFORM["G2_COMBINE_UNIFORM_WAVE"] = (lambda c: (len(c.cs), tuple(c.cs), c.d, c.neg), _uniform_wave_special)
whole_table("G2_COMBINE_UNIFORM_WAVE")


# ---- job_combine_small_io<Fq2>: the job body of the grouped G2 combination, on bytes ------------------------------------------------
COMBINE_IDX_AT = 4 * 192  # conformance.h kConfIdx
COMBINE_LEFT = 0xee  # the status a job that left the fast path leaves untouched (conformance.h)


def _combine_case(ids, shares, wave, tag):
    parts = [(192 * k, s) for k, s in enumerate(shares)] + [(COMBINE_IDX_AT, b"".join(int(i).to_bytes(8, "little") for i in ids))]
    return bcase(parts, [len(ids)], "wave %s: %s %s" % (wave, tag, list(ids)), ids=list(ids), shares=[bytes(s) for s in shares], wave=wave, kind=tag)


def _combine_ref(case):
    """None: the fast path does not take the job (nothing is written); else (status, the 192 bytes): Oracle A's combination of
    the shares, or the identity under status 3 where a share does not decode."""
    def ref():
        if small_coeffs_model(case.ids) is None:
            return None
        pts = []
        for s in case.shares:
            ok, p = byte_ref(2, "unc", s)
            if not ok:
                return 3, IDENTITY[(2, "unc")]
            pts.append(p)
        return 0, o.g2_uncompressed(o.combine_signatures(len(pts) - 1, zip(case.ids, pts)))
    return cached("combine-small", (tuple(case.ids), tuple(case.shares)), ref)


def combine_leaves_early(case):
    """The job is gone before the uniformity ballot of its wave: not applicable, or a share that does not decode."""
    r = _combine_ref(case)
    return r is None or r[0] != 0


@spec("JOB_COMBINE_SMALL_G2", None, nflags=2)
def _(case=None, out=None, flags=None, rnd=None):
    """Oracle A's combination of the share bytes on every job the fast path takes; return value false and the sentinel row
    untouched where it does not.  The waves: (a) one tuple; (b) 32 different tuples (the mixed forms run); (c) one tuple
    except one lane; (d) one tuple with jobs that leave before the uniformity ballot -- an index of 65 535, an undecodable
    share, a duplicate index -- as job 0 (wave_uniform must read the first lane still there), as job 31 and as every other job;
    (e) one tuple with a share at infinity and two equal shares on some lanes."""
    if rnd is not None:
        pool = g2_pool()
        enc = [o.g2_uncompressed(p) for p in pool]
        bad = [b for _, _, b in byte_cases(2, "unc") if not byte_ref(2, "unc", b)[0]]
        tup = {4: [0, 1, 2, 7], 3: [0, 1, 7], 2: [0, 3]}

        def shares(K, i):
            return [enc[(3 * (i % 3) + k) % len(enc)] for k in range(K)]

        def ordinary(wave, K=4):
            return lambda i: _combine_case(tup[K], shares(K, i), wave, "ordinary")
        leavers = [lambda w, i: _combine_case([0, 1, 2, 65535], shares(4, i), w, "index 65535"),
                   lambda w, i: _combine_case(tup[4], shares(4, i)[:2] + [bad[i % 2]] + shares(4, i)[3:], w, "undecodable share"),
                   lambda w, i: _combine_case([0, 1, 2, 2], shares(4, i), w, "duplicate index")]
        blocks = [[ordinary("a%d" % K, K)(i) for i in range(WAVE_JOBS)] for K in (4, 3, 2)]
        pairs = list(itertools.combinations(range(10), 2))[:WAVE_JOBS]
        blocks.append([_combine_case(list(s), shares(2, 0), "b", "its own tuple") for s in pairs])
        blocks.append([_combine_case([0, 1, 2, 5], shares(4, i), "c", "the other tuple") if i == 17 else ordinary("c")(i) for i in range(WAVE_JOBS)])
        for k, leave in enumerate(leavers):
            blocks.append([leave("d first %d" % k, i) if i == 0 else ordinary("d first %d" % k)(i) for i in range(WAVE_JOBS)])
        blocks.append([leavers[i % 3]("d last", i) if i >= 30 else ordinary("d last")(i) for i in range(WAVE_JOBS)])
        blocks.append([leavers[(i // 2) % 3]("d every other", i) if i % 2 == 0 else ordinary("d every other")(i) for i in range(WAVE_JOBS)])
        ident = IDENTITY[(2, "unc")]

        def special(i):
            s = shares(4, i)
            if i in (0, 31, 13):
                return _combine_case(tup[4], [ident] + s[1:], "e", "share at infinity")
            if i in (1, 14, 30):
                return _combine_case(tup[4], [s[0], s[0]] + s[2:], "e", "two equal shares")
            return ordinary("e")(i)
        blocks.append([special(i) for i in range(WAVE_JOBS)])
        blocks.append([ordinary("tail")(i) for i in range(5)])
        assert all(len(b) == WAVE_JOBS for b in blocks[:-1])
        return [c for b in blocks for c in b]
    ref = _combine_ref(case)
    flags_agree(case, flags, 2)
    if ref is None:
        expect((flags[0], flags[1]) == (COMBINE_LEFT, 0), case, "left the fast path: status %d, returned %d" % (flags[0], flags[1]))
        check_row(case, out, [], [], "job_combine_small_io (not applicable)")
    else:
        expect((flags[0], flags[1]) == (ref[0], 1), case, "status %d, returned %d; want %d, 1" % (flags[0], flags[1], ref[0]))
        check_row(case, out, [(0, ref[1])], [], "job_combine_small_io")


whole_table("JOB_COMBINE_SMALL_G2")


# ---------------------------------------------------------------------------------------------------------------------
# tables and sizes
# ---------------------------------------------------------------------------------------------------------------------
def table(op, seed=1):
    """The op's case table: the directed edge cases interleaved with random ones (so that adversarial lanes share a wave
    with ordinary ones), padded with random cases to several workgroups and a ragged tail."""
    fn, rand_case, _ = SPECS[op]
    rnd = random.Random("%s-%d" % (op, seed))
    edges = fn(rnd=rnd)
    if op in TABLES:
        return TABLES[op](edges, rnd)
    if op in LAYOUTS:
        return _wave_layout(op, edges, rnd)
    wave = 64 // lanes(op)
    n = max(2 * len(edges), 3 * wave + 5)
    if n % wave == 0:
        n += 1
    cases = []
    e = list(edges)
    while len(cases) < n:
        if e and (len(cases) % 2 == 0 or len(cases) + len(e) >= n):
            cases.append(e.pop(0))
        else:
            cases.append(rand_case(rnd))
    return cases


def _wave_layout(op, edges, rnd):
    """The table of an op that decides once per wave (LAYOUTS): first, for every path, one full wave (64 // lanes(op)
    jobs) that all take it (its directed cases, then random ones of that path); then the other directed cases interleaved with random
    cases of every path in turn, so that the later waves mix the paths (lanes that return early next to lanes that
    finish), up to a ragged tail."""
    path_of, makers = LAYOUTS[op]
    wave = 64 // lanes(op)
    pool, cases = list(edges), []
    for p, make in makers.items():
        mine = [c for c in pool if path_of(c) == p][:wave]
        pool = [c for c in pool if not any(c is m for m in mine)]
        cases += mine + [make(rnd) for _ in range(wave - len(mine))]
    paths = list(makers)
    n = len(cases) + max(2 * len(pool), 2 * wave + 5)
    if n % wave == 0:
        n += 1
    k = 0
    while len(cases) < n:
        if pool and (len(cases) % 2 == 0 or len(cases) + len(pool) >= n):
            cases.append(pool.pop(0))
        else:
            cases.append(makers[paths[k % len(paths)]](rnd))
            k += 1
    return cases


def sizes(op, n):
    """Launch sizes: one job, a partial wave, exactly one wave, and the whole table (several workgroups, ragged tail)."""
    wave = 64 // lanes(op)
    return [1, wave // 2 + 3, wave, n]


def check(op, cases, out, flags, rows=None):
    fn, _, _ = SPECS[op]
    bad = []
    for j, c in enumerate(cases):
        try:
            fn(case=c, out=out[j], flags=flags[j], **({} if rows is None else {"rows": rows[j]}))
        except Fail as e:
            bad.append("job %d: %s" % (j, e))
    return bad


def _host_main(op):
    lib = ctypes.CDLL(build_host())
    cases = table(op)
    out, flags, rows = run_host(lib, op, cases)
    bad = check(op, cases, out, flags, rows)
    for b in bad[:20]:
        print(b)
    print("%s: %d cases, %d failed" % (op, len(cases), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "host":
        sys.exit(_host_main(sys.argv[2]))
    print(__doc__)
    sys.exit(2)
