"""Host-side mirror of the reference's `poly` module (src/poly.rs) for the DKG algebra: same type and
method names, group work on the MI355X behind the C ABI.

  Poly.commitment / BivarPoly.commitment   tc_g1_commitment_batch      (fixed-base G1, LDS window table)
  Commitment.evaluate                      tc_public_key_share_batch   (Horner in G1; src/poly.rs:497-508)
  BivarCommitment.row / evaluate           tc_bivar_commitment_row_batch (+ Horner in y)
  Poly.interpolate                         tc_fr_interpolate_batch
  Poly.evaluate_batch                      tc_fr_poly_evaluate_batch   (Horner in Fr, one lane per value)
  BivarPoly.row_batch                      tc_bivar_poly_row_batch
  BivarCommitment.verify_rows              tc_dkg_verify_rows_batch    (`row_poly.commitment() == bi_commit.row(m)`)
  Commitment.verify_values                 tc_dkg_verify_values_batch, or with a seed tc_dkg_verify_values_rlc_batch
                                           (`bi_commit.evaluate(m, s) == g1 * val`)
  Commitment.__add__ / Commitment.sum      tc_g1_sum_batch             (Commitment::add_assign, src/poly.rs:462-471)
  Poly.sum                                 tc_fr_sum_batch             (Poly::add_assign, src/poly.rs:68-80)
  BivarCommitment.row0_sum                 tc_bivar_commitment_row0_sum_batch (`sum_commit += bi_commit.row(0)`)
  dkg_generate                             tc_dkg_generate_batch       (the accepted parts -> commitment and share)
  Commitment.weighted_sum                  tc_g1_weighted_sum_batch    (`Poly * Fr` src/poly.rs:210-254 in the exponent, then :462-471)
  Poly.weighted_sum                        tc_fr_weighted_sum_batch    (`Poly * Fr`, then Poly::add_assign)
  dkg_reshare                              tc_dkg_reshare_batch        (old holders deal, the master key stays)

Secret polynomials (Poly, BivarPoly) are Fr coefficient lists.  Poly.evaluate, BivarPoly.row and add/mul keep their
host form (key generation outside the hot path in the reference; SecretKeySet does the same in api.py); the batch
methods above do the same arithmetic on the device, where every staged secret is wiped after the call.  Nothing here
imports the oracle; there is no CPU fallback for the group operations.
"""
import numpy as np

from .api import _R, _stack, _raise_status, _require_members, default_engine, Error


def into_fr(x):
    """IntoFr (src/into_fr.rs): integers map to Fr by value (negative i64 wrap), NOT plus one."""
    return int(x) % _R


def _fr_rows(vals):
    return _stack([into_fr(v).to_bytes(32, "little") for v in vals], 32)


def _mask_bytes(mask, n):
    if mask is None:
        return None
    mask = [1 if m else 0 for m in mask]
    if len(mask) != n:
        raise ValueError("one mask entry per term")
    return np.array(mask, dtype=np.uint8)


def coeff_pos(i, j):
    """coeff_pos (src/poly.rs:746-750)."""
    if j < i:
        i, j = j, i
    return i + j * (j + 1) // 2


class Commitment:
    """struct Commitment { coeff: Vec<G1> } (src/poly.rs:432-437): 96-byte uncompressed points."""

    def __init__(self, coeff, _trusted=False):
        self.coeff = [bytes(c) for c in coeff]
        if self.coeff and not _trusted:
            _require_members(None, False, _stack(self.coeff, 96))

    def __eq__(self, other):
        return isinstance(other, Commitment) and self._trimmed() == other._trimmed()

    def _trimmed(self):
        inf = bytes([0x40]) + bytes(95)
        c = list(self.coeff)
        while c and c[-1] == inf:
            c.pop()
        return c

    def degree(self):
        """Commitment::degree (src/poly.rs:492-494)."""
        return max(len(self.coeff) - 1, 0)

    def evaluate(self, i, engine=None):
        """Commitment::evaluate (src/poly.rs:497-508) at the u64 abscissa i (taken as given)."""
        return self.evaluate_batch([i], engine)[0]

    def evaluate_batch(self, xs, engine=None):
        """Commitment::evaluate for several abscissae.  `i: T: IntoFr` in the reference: any integer is taken by value
        modulo r (negative values wrap, src/into_fr.rs).  1 <= x < 2^64 runs the Horner kernel (tc_public_key_share_batch
        with idx = x - 1); x = 0 is coefficient 0; every other field element (x = 2^64 -- the share index 2^64 - 1 --
        and beyond) is the linear combination sum_k x^k commit[k] (tc_g1_lincomb_batch)."""
        e = engine or default_engine()
        if not self.coeff:
            return [bytes([0x40]) + bytes(95)] * len(xs)
        xs = [into_fr(x) for x in xs]
        out = [None] * len(xs)
        small = [k for k, x in enumerate(xs) if 1 <= x <= 2 ** 64 - 1]
        if small:
            res, st = e.public_key_shares(_stack(self.coeff, 96), np.array([xs[k] - 1 for k in small], dtype=np.uint64))
            for s in st:
                _raise_status(s)
            for k, r in zip(small, res):
                out[k] = bytes(r)
        wide = [k for k, x in enumerate(xs) if x > 2 ** 64 - 1]
        if wide:
            n = len(self.coeff)
            pts = np.ascontiguousarray(np.broadcast_to(_stack(self.coeff, 96)[None], (len(wide), n, 96)))
            sc = np.empty((len(wide), n, 32), dtype=np.uint8)
            for row, k in enumerate(wide):
                p = 1
                for d in range(n):
                    sc[row, d] = np.frombuffer(p.to_bytes(32, "little"), dtype=np.uint8)
                    p = p * xs[k] % _R
            res, st = e.lincomb_g1(sc, pts)
            for s in st:
                _raise_status(s)
            for k, r in zip(wide, res):
                out[k] = bytes(r)
        for k, x in enumerate(xs):
            if x == 0:
                out[k] = self.coeff[0]
        return out

    def __add__(self, other):
        """Commitment::add_assign (src/poly.rs:462-471)."""
        return Commitment.sum([self, other])

    @staticmethod
    def sum(commits, mask=None, engine=None):
        """Commitment::add_assign folded over `commits` on the device: shorter ones are padded with the identity, trailing
        identities are dropped like remove_zeros (src/poly.rs:466-470).  mask: one truthy / falsy entry per commitment (an
        excluded one is not even decoded), None = all."""
        e = engine or default_engine()
        commits = list(commits)
        width = max([len(c.coeff) for c in commits] + [0])
        if width == 0:
            return Commitment([], _trusted=True)
        inf = bytes([0x40]) + bytes(95)
        pts = np.stack([_stack(c.coeff + [inf] * (width - len(c.coeff)), 96) for c in commits])
        out, st = e.g1_sum(pts, _mask_bytes(mask, len(commits)))
        for s in st:
            _raise_status(s)
        return Commitment(Commitment([bytes(p) for p in out], _trusted=True)._trimmed(), _trusted=True)

    @staticmethod
    def weighted_sum(commits, weights, mask=None, engine=None):
        """sum_k weights[k] * commits[k] on the device (`Poly * Fr` src/poly.rs:210-254 in the exponent, folded by
        Commitment::add_assign :462-471).  weights: IntoFr values, public; mask as in Commitment.sum."""
        e = engine or default_engine()
        commits = list(commits)
        if len(weights) != len(commits):
            raise ValueError("one weight per commitment")
        width = max([len(c.coeff) for c in commits] + [0])
        if width == 0:
            return Commitment([], _trusted=True)
        inf = bytes([0x40]) + bytes(95)
        pts = np.stack([_stack(c.coeff + [inf] * (width - len(c.coeff)), 96) for c in commits])
        out, st = e.g1_weighted_sum(pts, _fr_rows(weights), _mask_bytes(mask, len(commits)))
        for s in st:
            _raise_status(s)
        return Commitment(Commitment([bytes(p) for p in out], _trusted=True)._trimmed(), _trusted=True)

    def verify_values(self, xs, vals, seed=None, engine=None):
        """`bi_commit.evaluate(m, s) == g1 * val` (src/poly.rs:846-848) with self = bi_commit.row(m): one bool per
        (u64 abscissa, value) pair.  With a 32-byte secret `seed` the values are checked by one random linear
        combination (tc_dkg_verify_values_rlc_batch) and value by value only when that fails: the same answers up to 2^-63."""
        return Commitment.verify_values_batch([self], [xs], [vals], seed, engine)[0]

    @staticmethod
    def verify_values_batch(commits, xs, vals, seed=None, engine=None):
        """verify_values for several row commitments of one degree, n values each, in one call"""
        e = engine or default_engine()
        if not commits:
            return []
        npts, n = len(commits[0].coeff), len(xs[0])
        if npts == 0 or any(len(c.coeff) != npts for c in commits):
            raise ValueError("all row commitments of one batch must hold the same, non-zero number of coefficients")
        if len(xs) != len(commits) or len(vals) != len(commits) or any(len(x) != n for x in xs) or any(len(v) != n for v in vals):
            raise ValueError("every commitment needs the same number of abscissae and values")
        if n == 0:
            return [[] for _ in commits]
        if any(not 0 <= int(x) < 2 ** 64 for row in xs for x in row):
            raise ValueError("values are addressed by u64 abscissae")
        rows = np.stack([_stack(c.coeff, 96) for c in commits])
        xa = np.array([[int(x) for x in row] for row in xs], dtype=np.uint64)
        va = np.stack([_fr_rows(row) for row in vals])
        ok = e.dkg_verify_values(rows, xa, va) if seed is None else e.dkg_verify_values_rlc(rows, xa, va, seed)[0]
        return [[bool(b) for b in row] for row in ok]


class Poly:
    """struct Poly { coeff: Vec<Fr> } (src/poly.rs:44-49)."""

    def __init__(self, coeff):
        self.coeff = [into_fr(c) for c in coeff]
        self._remove_zeros()

    def _remove_zeros(self):
        while self.coeff and self.coeff[-1] == 0:
            self.coeff.pop()

    def __eq__(self, other):
        return isinstance(other, Poly) and self.coeff == other.coeff

    def degree(self):
        return max(len(self.coeff) - 1, 0)

    def evaluate(self, i):
        """Poly::evaluate (src/poly.rs:358-369)."""
        x, res = into_fr(i), 0
        for c in reversed(self.coeff):
            res = (res * x + c) % _R
        return res

    @staticmethod
    def evaluate_batch(polys, xs, engine=None):
        """Poly::evaluate (src/poly.rs:358-369) for every polynomial at every abscissa (IntoFr values) on the device:
        a list of len(polys) lists of len(xs) integers"""
        e = engine or default_engine()
        if not polys or not xs:
            return [[] for _ in polys]
        n = max(len(p.coeff) for p in polys)
        coeff = np.zeros((len(polys), n, 32), dtype=np.uint8)
        for j, p in enumerate(polys):
            if p.coeff:
                coeff[j, :len(p.coeff)] = _fr_rows(p.coeff)
        out, st = e.fr_poly_evaluate(coeff, _fr_rows(xs))
        for s in st.reshape(-1):
            _raise_status(s)
        return [[int.from_bytes(bytes(out[j, m]), "little") for m in range(len(xs))] for j in range(len(polys))]

    def __add__(self, other):
        n = max(len(self.coeff), len(other.coeff))
        g = lambda p, k: p.coeff[k] if k < len(p.coeff) else 0
        return Poly([(g(self, k) + g(other, k)) % _R for k in range(n)])

    @staticmethod
    def sum(polys, mask=None, engine=None):
        """Poly::add_assign (src/poly.rs:68-80) folded over `polys` on the device (the staged coefficients are wiped there)."""
        e = engine or default_engine()
        polys = list(polys)
        width = max([len(p.coeff) for p in polys] + [0])
        if width == 0:
            return Poly([])
        vals = np.zeros((len(polys), width, 32), dtype=np.uint8)
        for k, p in enumerate(polys):
            if p.coeff:
                vals[k, :len(p.coeff)] = _fr_rows(p.coeff)
        out, st = e.fr_sum(vals, _mask_bytes(mask, len(polys)))
        for s in st:
            _raise_status(s)
        return Poly([int.from_bytes(bytes(c), "little") for c in out])

    @staticmethod
    def weighted_sum(polys, weights, mask=None, engine=None):
        """sum_k weights[k] * polys[k] on the device (`Poly * Fr` src/poly.rs:210-254, then Poly::add_assign :68-80); the staged
        coefficients are wiped there.  weights: IntoFr values, public."""
        e = engine or default_engine()
        polys = list(polys)
        if len(weights) != len(polys):
            raise ValueError("one weight per polynomial")
        width = max([len(p.coeff) for p in polys] + [0])
        if width == 0:
            return Poly([])
        vals = np.zeros((len(polys), width, 32), dtype=np.uint8)
        for k, p in enumerate(polys):
            if p.coeff:
                vals[k, :len(p.coeff)] = _fr_rows(p.coeff)
        out, st = e.fr_weighted_sum(vals, _fr_rows(weights), _mask_bytes(mask, len(polys)))
        for s in st:
            _raise_status(s)
        return Poly([int.from_bytes(bytes(c), "little") for c in out])

    def commitment(self, engine=None):
        """Poly::commitment (src/poly.rs:372-377)."""
        return Poly.commitment_batch([self], engine)[0]

    @staticmethod
    def commitment_batch(polys, engine=None):
        """every coefficient of every polynomial in ONE fixed-base launch"""
        e = engine or default_engine()
        flat = [c for p in polys for c in p.coeff]
        if not flat:
            return [Commitment([], _trusted=True) for _ in polys]
        out, st = e.g1_commitment(_fr_rows(flat))
        for s in st:
            _raise_status(s)
        res, pos = [], 0
        for p in polys:
            res.append(Commitment([bytes(out[pos + k]) for k in range(len(p.coeff))], _trusted=True))
            pos += len(p.coeff)
        return res

    @staticmethod
    def interpolate(samples, engine=None):
        """Poly::interpolate (src/poly.rs:341-350): samples = dict or sequence of (x, y) pairs, x and y IntoFr."""
        return Poly.interpolate_batch([samples], engine)[0]

    @staticmethod
    def interpolate_batch(jobs, engine=None):
        e = engine or default_engine()
        ordered = [sorted(j.items()) if isinstance(j, dict) else list(j) for j in jobs]
        n = len(ordered[0])
        if any(len(o) != n for o in ordered):
            raise ValueError("all jobs of one batch must hold the same number of samples")
        if n == 0:
            return [Poly([]) for _ in jobs]
        xs = np.stack([_fr_rows([x for x, _ in o]) for o in ordered])
        ys = np.stack([_fr_rows([y for _, y in o]) for o in ordered])
        out, st = e.fr_interpolate(xs, ys)
        for s in st:
            if int(s) == 2:
                raise ValueError("sample points must be distinct")   # the reference panics (src/poly.rs:404)
            _raise_status(s)
        return [Poly([int.from_bytes(bytes(out[j, k]), "little") for k in range(n)]) for j in range(len(jobs))]


class BivarPoly:
    """struct BivarPoly { degree, coeff: Vec<Fr> } (src/poly.rs:530-536): symmetric, coefficients in coeff_pos
    order."""

    def __init__(self, degree, coeff):
        self.degree_ = int(degree)
        self.coeff = [into_fr(c) for c in coeff]
        if len(self.coeff) != (self.degree_ + 1) * (self.degree_ + 2) // 2:
            raise ValueError("a symmetric polynomial of degree d has (d+1)(d+2)/2 coefficients")

    def degree(self):
        return self.degree_

    @staticmethod
    def random_with_constant(degree, secret, rng):
        """The dealer's side of a resharing: a random symmetric polynomial of `degree` with F(0, 0) = secret (BivarPoly::random,
        src/poly.rs:562-585, with coefficient (0, 0) replaced).  rng: anything with randrange, e.g. secrets.SystemRandom()."""
        n = (int(degree) + 1) * (int(degree) + 2) // 2
        return BivarPoly(degree, [into_fr(secret)] + [rng.randrange(_R) for _ in range(n - 1)])

    def _powers(self, x):
        out, p, x = [], 1, into_fr(x)
        for _ in range(self.degree_ + 1):
            out.append(p)
            p = p * x % _R
        return out

    def evaluate(self, x, y):
        """BivarPoly::evaluate (src/poly.rs:587-603)."""
        xp, yp = self._powers(x), self._powers(y)
        d = self.degree_
        return sum(self.coeff[coeff_pos(i, j)] * xp[i] * yp[j] for i in range(d + 1) for j in range(d + 1)) % _R

    def row(self, x):
        """BivarPoly::row (src/poly.rs:606-622)."""
        xp, d = self._powers(x), self.degree_
        return Poly([sum(self.coeff[coeff_pos(i, j)] * xp[j] for j in range(d + 1)) % _R for i in range(d + 1)])

    def row_batch(self, xs, engine=None):
        """BivarPoly::row (src/poly.rs:606-622) for several u64 abscissae on the device"""
        e = engine or default_engine()
        xs = [int(x) for x in xs]
        if any(x < 0 or x >= 2 ** 64 for x in xs):
            raise ValueError("rows are addressed by u64 abscissae")
        if not xs:
            return []
        out, st = e.bivar_poly_rows(_fr_rows(self.coeff), self.degree_, np.array(xs, dtype=np.uint64))
        for s in st.reshape(-1):
            _raise_status(s)
        return [Poly([int.from_bytes(bytes(out[m, i]), "little") for i in range(self.degree_ + 1)]) for m in range(len(xs))]

    def commitment(self, engine=None):
        """BivarPoly::commitment (src/poly.rs:625-632)."""
        e = engine or default_engine()
        out, st = e.g1_commitment(_fr_rows(self.coeff))
        for s in st:
            _raise_status(s)
        return BivarCommitment(self.degree_, [bytes(o) for o in out], _trusted=True)


class BivarCommitment:
    """struct BivarCommitment { degree, coeff: Vec<G1> } (src/poly.rs:664-670)."""

    def __init__(self, degree, coeff, _trusted=False):
        self.degree_ = int(degree)
        self.coeff = [bytes(c) for c in coeff]
        if len(self.coeff) != (self.degree_ + 1) * (self.degree_ + 2) // 2:
            raise ValueError("a symmetric commitment of degree d has (d+1)(d+2)/2 coefficients")
        if not _trusted:
            _require_members(None, False, _stack(self.coeff, 96))

    def __eq__(self, other):
        return isinstance(other, BivarCommitment) and (self.degree_, self.coeff) == (other.degree_, other.coeff)

    def degree(self):
        return self.degree_

    def row(self, x, engine=None):
        """BivarCommitment::row (src/poly.rs:713-727)."""
        return self.row_batch([x], engine)[0]

    def row_batch(self, xs, engine=None):
        e = engine or default_engine()
        xs = [int(x) for x in xs]
        if any(x < 0 or x >= 2 ** 64 for x in xs):
            raise ValueError("rows are addressed by u64 abscissae")
        out, st = e.bivar_commitment_rows(_stack(self.coeff, 96), self.degree_, np.array(xs, dtype=np.uint64))
        for s in st.reshape(-1):
            _raise_status(s)
        return [Commitment([bytes(out[m, i]) for i in range(self.degree_ + 1)], _trusted=True) for m in range(len(xs))]

    def evaluate(self, x, y, engine=None):
        """BivarCommitment::evaluate (src/poly.rs:694-710) = row(x).evaluate(y)."""
        return self.row(x, engine).evaluate(y, engine)

    @staticmethod
    def row0_sum(commits, mask=None, engine=None):
        """`sum_commit += bi_commit.row(0)` (src/poly.rs:895-898) over the included commitments of one degree: row(0)[i] is
        coefficient (i, 0), so this is a plain sum of points."""
        e = engine or default_engine()
        commits = list(commits)
        if not commits:
            return Commitment([], _trusted=True)
        d = commits[0].degree_
        if any(c.degree_ != d for c in commits):
            raise ValueError("all commitments of one batch must have the same degree")
        out, st = e.bivar_row0_sum(np.stack([_stack(c.coeff, 96) for c in commits]), d, _mask_bytes(mask, len(commits)))
        for s in st:
            _raise_status(s)
        return Commitment(Commitment([bytes(p) for p in out], _trusted=True)._trimmed(), _trusted=True)

    def verify_rows(self, xs, row_polys, engine=None):
        """`row_poly.commitment() == bi_commit.row(m)` (src/poly.rs:841-843) for several (m, row_poly) pairs under this
        commitment: (the row commitments, one bool per pair)"""
        return BivarCommitment.verify_rows_batch([self], xs, row_polys, engine)

    @staticmethod
    def verify_rows_batch(commits, xs, row_polys, engine=None):
        """the rows check for len(xs) parts: commits holds ONE commitment (shared by every part) or one per part"""
        e = engine or default_engine()
        xs = [int(x) for x in xs]
        if any(x < 0 or x >= 2 ** 64 for x in xs):
            raise ValueError("rows are addressed by u64 abscissae")
        if len(row_polys) != len(xs) or len(commits) not in (1, len(xs)):
            raise ValueError("one row polynomial per abscissa, and one commitment or one per abscissa")
        if not xs:
            return [], []
        d = commits[0].degree_
        if any(c.degree_ != d for c in commits):
            raise ValueError("all commitments of one batch must have the same degree")
        ok_len = [len(p.coeff) <= d + 1 for p in row_polys]            # a longer polynomial commits to something else
        rows = np.zeros((len(xs), d + 1, 32), dtype=np.uint8)
        for j, p in enumerate(row_polys):
            if p.coeff and ok_len[j]:
                rows[j, :len(p.coeff)] = _fr_rows(p.coeff)
        blob = _stack(commits[0].coeff, 96) if len(commits) == 1 else np.stack([_stack(c.coeff, 96) for c in commits])
        out, ok = e.dkg_verify_rows(blob, d, np.array(xs, dtype=np.uint64), rows)
        rc = [Commitment([bytes(out[j, i]) for i in range(d + 1)], _trusted=True) for j in range(len(xs))]
        return rc, [bool(ok[j]) and ok_len[j] for j in range(len(xs))]


def _stage_samples(samples, acc, P):
    """the (u64 abscissa, value) pairs a node received, one set per dealer, as the (P, n_v) / (P, n_v, 32) arrays of the
    finalisation entries; (None, None) for an observer"""
    if samples is None:
        return None, None
    if len(samples) != P:
        raise ValueError("one set of samples per dealer")
    taken = [acc is None or acc[p] for p in range(P)]
    ordered = [(sorted(s.items()) if isinstance(s, dict) else list(s)) if t else None for s, t in zip(samples, taken)]
    n_v = max([len(s) for s in ordered if s is not None] + [0])
    if any(s is not None and len(s) != n_v for s in ordered):
        raise ValueError("every accepted dealer needs the same number of samples")
    if any(not 0 <= int(x) < 2 ** 64 for s in ordered if s is not None for x, _ in s):
        raise ValueError("values are addressed by u64 abscissae")
    xs = np.zeros((P, n_v), dtype=np.uint64)
    vals = np.zeros((P, n_v, 32), dtype=np.uint8)
    for p, s in enumerate(ordered):
        if s is not None and n_v:
            xs[p] = [int(x) for x, _ in s]
            vals[p] = _fr_rows([y for _, y in s])
    return xs, vals


def dkg_generate(bi_commits, accepted, samples=None, engine=None):
    """The end of `distributed_key_generation` (src/poly.rs:870-876, 895-898) over the accepted parts: returns (the key set's
    Commitment, this node's secret key share or None).  bi_commits: one BivarCommitment per dealer; accepted: one truthy /
    falsy entry per dealer (None = all; a rejected dealer's commitment is never used); samples: per dealer the (u64 abscissa,
    value) pairs this node received from that dealer's row -- a dict or a sequence, the same number for every dealer (a rejected
    dealer's may be None) -- or None for an observer without a secret.  A failed accepted part raises."""
    e = engine or default_engine()
    bi_commits = list(bi_commits)
    P = len(bi_commits)
    if P == 0:
        return Commitment([], _trusted=True), (0 if samples is not None else None)
    d = bi_commits[0].degree_
    if any(c.degree_ != d for c in bi_commits):
        raise ValueError("all commitments of one batch must have the same degree")
    acc = _mask_bytes(accepted, P)
    xs, vals = _stage_samples(samples, acc, P)
    out, share, st = e.dkg_generate(np.stack([_stack(c.coeff, 96) for c in bi_commits]), d, acc, xs, vals)
    for s in st:
        if int(s) == 2:
            raise ValueError("sample points must be distinct")   # the reference panics (src/poly.rs:404)
        _raise_status(s)
    commit = Commitment(Commitment([bytes(p) for p in out], _trusted=True)._trimmed(), _trusted=True)
    return commit, (int.from_bytes(bytes(share), "little") if share is not None else None)


class ShareMismatch(Error):
    """a resharing dealer's constant term is not the public key share of the old node it claims to be (TC_JOB_SHARE_MISMATCH)"""


def dkg_reshare(old_commit, dealer_idx, bi_commits, accepted, samples=None, engine=None):
    """Hands the SAME master key to a new validator set (tc_dkg_reshare_batch): old node dealer_idx[p] dealt bi_commits[p], a
    symmetric polynomial of the new degree whose constant term is its share of old_commit's key.  The first
    old_commit.degree() + 1 accepted parts are combined with their Lagrange coefficients at zero.  accepted and samples as
    in dkg_generate.  Returns (the new key set's Commitment -- its coefficient 0 is old_commit's --, this node's new secret key
    share or None, used: one bool per dealer).  A failed accepted part raises, as in dkg_generate; a dealer whose constant
    term is not its public key share raises ShareMismatch, too few accepted parts NotEnoughShares."""
    e = engine or default_engine()
    bi_commits = list(bi_commits)
    P = len(bi_commits)
    if len(dealer_idx) != P:
        raise ValueError("one dealer index per part")
    if any(not 0 <= int(i) < 2 ** 64 for i in dealer_idx):
        raise ValueError("dealers are addressed by u64 indices")
    if not old_commit.coeff:
        raise ValueError("old_commit: the commitment of the key set being handed over")
    if P == 0:
        _raise_status(1)
    d = bi_commits[0].degree_
    if any(c.degree_ != d for c in bi_commits):
        raise ValueError("all commitments of one batch must have the same degree")
    acc = _mask_bytes(accepted, P)
    xs, vals = _stage_samples(samples, acc, P)
    out, share, used, st, status = e.dkg_reshare(_stack(old_commit.coeff, 96), np.array([int(i) for i in dealer_idx], dtype=np.uint64),
                                                 np.stack([_stack(c.coeff, 96) for c in bi_commits]), d, acc, xs, vals)
    for s in list(st) + [status[0]]:
        if int(s) == 4:
            raise ShareMismatch("a dealer's constant term is not its public key share")
        _raise_status(s)
    commit = Commitment(Commitment([bytes(p) for p in out], _trusted=True)._trimmed(), _trusted=True)
    return commit, (int.from_bytes(bytes(share), "little") if share is not None else None), [bool(u) for u in used]
