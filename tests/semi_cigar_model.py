"""Independent model of gasalx_semi_cigar_* (TEST INFRASTRUCTURE ONLY): SEMI_GLOBAL with HEAD =
TARGET and TAIL = TARGET, with the alignment itself.  There is no reference output for this call
(the reference's semi-global kernel has no traceback branch), so this module is the definition
restated: full matrices, the direction nibble of every cell, the walk, the CIGAR bytes.

Matrix.  Rows are query bases, columns target bases.  Boundaries as the semi-global kernels hold
them for HEAD = TARGET (semiglobal_kernel_template.h:87-99,123-128): H(-1, c) = 0 for every
column, c = -1 included, F(0, c) = H(-1, c) - (o + e); H(r, -1) = -(o + e*r) for r >= 1 and 0
for r = 0 (the reference's off-by-one: r + 1 bases for the price of r), E(r, 0) = H(r, -1) - OE.
N scores by the LOCAL rule (0, or -N_PENALTY).  Cells as the semi-global kernels compute them
(semiglobal_kernel_template.h:17-28): tmp = H(r-1, c-1) + s, H = max(tmp, F, E), then E(r, c+1) =
max(H - OE, E - e) and F(r+1, c) = max(H - OE, F - e): gaps open from H.  The GLOBAL kernel, on
whose cell the direction nibble was first defined (global.h:4-26), opens them from tmp; that is
another matrix as soon as an insertion run next to a deletion run beats the substitutions it
replaces (default scores: runs of seven), so the nibble's two "extended" bits are taken here
against H - OE.  tests/test_semi_cigar_model.py checks the scores and ends against
independent.semi on every batch.

Nibble: low2 = (H == tmp) ? (s < 0) : ((H == F) ? 3 : 2); bit 2 = E(r, c+1) extended (H - OE <=
E - e); bit 3 = F(r+1, c) extended.

Walk (get_tb.h:47-98 as a state machine), from the end cell (ql - 1, t_end) in H state:
  H state: low2 0 -> M, 1 -> X, both move diagonally; 2 -> D, move left, E state; 3 -> I, move up,
           F state.
  E state: the cell's bit 2 set -> D, move left; clear -> the run was opened from this cell's H:
           H state at the same cell, no op and no move (where the GLOBAL walk takes the diagonal
           as op 0, its rule G3, because GLOBAL's gaps open from the diagonal candidate).
  F state: the same with bit 3, I and up.
It stops when the query is exhausted; target bases left of that point are the free head.  When it
reaches column -1 first, the rows left are the left boundary's insertions.  t_start = the column
after the last move (the first target base consumed; t_end + 1 when none is), q_start = 0.

Bytes: count << 2 | op, runs of at most 63, written in walk order (so reversed), the boundary
insertions as bytes of their own after the walk's last run.

Rows are vectorised over pairs and columns.  E along a row is a running maximum: an H taken from E
never opens a better gap than extending that E (OE >= e), so E(r, c) = max over c' < c of
max(tmp, F)(r, c') - OE - e*(c - 1 - c'), with the left boundary as c' = -1.  The walk is a plain
loop per pair.
"""
from __future__ import annotations

import zlib

import numpy as np

import independent as I

NEG = -(1 << 40)
TARGET = 2
OPS = "MXDI"


class ModelBatch:
    """The six arrays of a GASAL2-layout batch (what independent.* and gasal_ffi.Batch take)."""

    def __init__(self, q_data, q_offsets, q_lens, t_data, t_offsets, t_lens):
        self.q_data, self.q_offsets, self.q_lens = q_data, q_offsets, q_lens
        self.t_data, self.t_offsets, self.t_lens = t_data, t_offsets, t_lens

    @property
    def n(self):
        return len(self.q_lens)

    @property
    def q_bytes(self):
        return len(self.q_data)

    @property
    def t_bytes(self):
        return len(self.t_data)

    def arrays(self):
        return (self.q_data, self.q_offsets, self.q_lens, self.t_data, self.t_offsets, self.t_lens)

    @staticmethod
    def _side(seqs):
        lens = np.array([len(s) for s in seqs], np.uint32)
        pads = (lens.astype(np.int64) + 7) // 8 * 8
        offs = np.concatenate([[0], np.cumsum(pads)[:-1]]).astype(np.uint32)
        data = np.full(max(int(pads.sum()), 8), 0x4E, np.uint8)
        for s, o in zip(seqs, offs):
            data[int(o):int(o) + len(s)] = np.frombuffer(bytes(s), np.uint8)
        return data, offs, lens

    @classmethod
    def from_pairs(cls, qs, ts):
        return cls(*cls._side(qs), *cls._side(ts))


def Hrow_left(n, r, o, e):
    """H(r, -1) as a column."""
    return np.full((n, 1), 0 if r == 0 else -(o + e * r), np.int64)


def semi_cigar(batch, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None):
    """score, q_end, t_end, q_start, t_start, n_ops (arrays), cigar (uint8, q_bytes, 0 where no op byte
    was written... bytes past the buffer dropped), text (forward CIGAR per pair), ops (bytes per pair)."""
    assert o >= 0 and e >= 0, "outside the scores the call supports"
    q, _ = I._codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, _ = I._codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    q = q.astype(np.int64); t = t.astype(np.int64)
    n, R = q.shape
    T = t.shape[1]
    nval, OE = n_code & 15, o + e
    ql, tl = batch.q_lens.astype(np.int64), batch.t_lens.astype(np.int64)
    cols = np.arange(T, dtype=np.int64)
    Hrow = np.zeros((n, T + 1), np.int64)             # H(r-1, c) at index c + 1; row -1: all 0
    F = np.full((n, T), -OE, np.int64)                # F(0, c) = H(-1, c) - OE
    nib = np.zeros((n, R, T), np.uint8)
    last = np.zeros((n, T), np.int64)                 # H of each pair's last query row
    for r in range(R):
        s = np.where(q[:, r:r + 1] == t, a, -b)
        s = np.where((q[:, r:r + 1] == nval) | (t == nval), -(npen or 0), s)
        tmp = Hrow[:, :T] + s
        # what opens a gap into column c + 1, less OE: H(r, c) unless it came from E; c' = -1 first
        src = np.concatenate([Hrow_left(n, r, o, e), np.maximum(tmp, F)], axis=1) - OE
        E = np.maximum.accumulate(src + e * np.arange(-1, T), axis=1)[:, :T] - e * (cols - 1)
        H = np.maximum(np.maximum(tmp, F), E)
        toe = H - OE
        low2 = np.where(H == tmp, (s < 0).astype(np.int64), np.where(H == F, 3, 2))
        nib[:, r, :] = low2 | np.where(toe <= E - e, 4, 0) | np.where(toe <= F - e, 8, 0)
        F = np.maximum(toe, F - e)
        Hrow = np.concatenate([Hrow_left(n, r, o, e), H], axis=1)
        last = np.where((ql - 1 == r)[:, None], H, last)
    inside = cols[None, :] < tl[:, None]
    masked = np.where(inside, last, NEG)
    score = masked.max(axis=1)
    t_end = masked.argmax(axis=1)                     # the first column holding the maximum
    out = {"score": score.astype(np.int32), "q_end": tl.astype(np.int32), "t_end": t_end.astype(np.int32),
           "q_start": np.zeros(n, np.int32), "t_start": np.zeros(n, np.int32), "n_ops": np.zeros(n, np.uint32),
           "cigar": np.zeros(batch.q_bytes, np.uint8), "text": [], "ops": []}
    for p in range(n):
        i, j, state, path = int(t_end[p]), int(ql[p]) - 1, "H", []
        while i >= 0 and j >= 0:
            cell = int(nib[p, j, i])
            if state == "H":
                op = cell & 3
                state = "E" if op == 2 else "F" if op == 3 else "H"
            elif cell & (4 if state == "E" else 8):
                op = 2 if state == "E" else 3
            else:
                state = "H"
                continue
            path.append(op)
            i -= op != 3
            j -= op != 2
        by = []
        k = 0
        while k < len(path):                          # runs of at most 63, in walk order
            m = k
            while m < len(path) and path[m] == path[k] and m - k < 63:
                m += 1
            by.append(path[k] | ((m - k) << 2))
            k = m
        rest = j + 1                                  # the left boundary's insertions
        path += [3] * rest
        while rest > 0:
            by.append(3 | (min(rest, 63) << 2))
            rest -= 63
        out["t_start"][p] = i + 1
        out["n_ops"][p] = len(by)
        off = int(batch.q_offsets[p])
        keep = by[:max(0, batch.q_bytes - off)]
        out["cigar"][off:off + len(keep)] = keep      # (a later pair's bytes overwrite a longer earlier run)
        out["ops"].append(bytes(by))
        fwd, text, k = path[::-1], [], 0
        while k < len(fwd):
            m = k
            while m < len(fwd) and fwd[m] == fwd[k]:
                m += 1
            text.append(f"{m - k}{OPS[fwd[k]]}")
            k = m
        out["text"].append("".join(text))
    return out


# ---------------------------------------------------------------------------------------------
# The batches both test files use, by name: builder() -> (ModelBatch, scores dict for semi_cigar).
# ---------------------------------------------------------------------------------------------
DEFAULT = dict(a=1, b=4, o=6, e=1)
SHAPE_QL = (1, 7, 8, 9, 63, 64, 65, 150, 152, 300)


def shape_tl(ql):
    return (ql, ql + 1, ql + 32, max(1, ql - 3))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n))


def _mutate(rng, read, subs, ins, dele):
    r = bytearray(read)
    for _ in range(subs):
        k = int(rng.integers(len(r)))
        r[k] = rng.choice([c for c in b"ACGT" if c != r[k]])
    if ins and len(r) > 2:
        k = int(rng.integers(1, len(r) - 1))
        r[k:k] = _dna(rng, 1)
    if dele and len(r) > 3:
        k = int(rng.integers(1, len(r) - 1))
        del r[k]
    return bytes(r)


def related_pairs(rng, n, ql, tl, unrelated_every=4):
    """Reads of exactly ql bases cut from windows of tl bases, with 0-3 substitutions, an insertion and
    a deletion at random places; every unrelated_every-th pair unrelated."""
    qs, ts = [], []
    for k in range(n):
        t = _dna(rng, tl)
        if unrelated_every and k % unrelated_every == unrelated_every - 1 or tl < 4 or ql < 4:
            qs.append(_dna(rng, ql)); ts.append(t)
            continue
        span = min(ql, tl)
        st = int(rng.integers(0, tl - span + 1))
        r = _mutate(rng, t[st:st + span], int(rng.integers(0, 4)), k % 2, k % 3 == 0)
        r = (r + _dna(rng, ql))[:ql]
        qs.append(r); ts.append(t)
    return qs, ts


def shape_batch(ql, tl, n=300):
    return ModelBatch.from_pairs(*related_pairs(_rng("shape", ql, tl), n, ql, tl))


def content_related():
    return ModelBatch.from_pairs(*related_pairs(_rng("related"), 300, 150, 182, 0))


def content_unrelated():
    rng = _rng("unrelated")
    return ModelBatch.from_pairs([_dna(rng, 150) for _ in range(300)], [_dna(rng, 182) for _ in range(300)])


def content_overhang():
    """Reads hanging over the window's left or right edge: leading or trailing insertions, ends at the
    first or last columns."""
    rng = _rng("overhang")
    qs, ts = [], []
    for k in range(300):
        t = _dna(rng, 182)
        h = int(rng.integers(1, 30))
        qs.append(_dna(rng, h) + t[:150 - h] if k % 2 else t[182 - (150 - h):] + _dna(rng, h))
        ts.append(t)
    return ModelBatch.from_pairs(qs, ts)


def content_repeats():
    rng = _rng("repeats")
    qs, ts = [], []
    for k in range(300):
        unit = [b"A", b"AC", b"T", b"GA", b"ACG"][k % 5]
        ql, tl = int(rng.integers(20, 150)), int(rng.integers(150, 183))
        qs.append((unit * 200)[:ql]); ts.append((unit * 200)[k % 3:][:tl])
    return ModelBatch.from_pairs(qs, ts)


def n_targets():
    """Targets holding N in pairs 64-127 and 200-209 only (whole packed blocks at G = 8 and part of one)."""
    qs, ts = related_pairs(_rng("ntargets"), 300, 150, 182)
    rng = _rng("ntargets", 2)
    for k in list(range(64, 128)) + list(range(200, 210)):
        t = bytearray(ts[k])
        for pos in rng.integers(0, len(t), 3):
            t[int(pos)] = ord("N")
        ts[k] = bytes(t)
    return ModelBatch.from_pairs(qs, ts)


def sorted_lengths():
    rng = _rng("sorted")
    qs, ts = [], []
    for k in range(4200):
        ql = int(rng.integers(40, 153))
        q, t = related_pairs(rng, 1, ql, ql + 32, 0)
        qs += q; ts += t
    return ModelBatch.from_pairs(qs, ts)


OVERFLOW = dict(a=20, b=3, o=1, e=1)
MATCH200 = dict(a=200, b=56, o=6, e=1)   # match + table offset past a byte: no packed kernel at any length
M200_QL = (1, 7, 8, 9)


def overflow_pairs():
    """Every query base matched with a one-base deletion between: about 2 * ql op bytes in pad8(ql)."""
    rng = _rng("overflow")
    qs, ts = [], []
    for k in range(40):
        q = _dna(rng, int(rng.integers(8, 17)))
        # a spacer that differs from both neighbours, so that the deletions are the best path
        t = b"".join(bytes([c]) + bytes([next(x for x in b"ACGT" if x != c and x != (q[m + 1] if m + 1 < len(q) else c))])
                     for m, c in enumerate(q))
        qs.append(q); ts.append(t)
    return ModelBatch.from_pairs(qs, ts)


def single_and_17():
    qs, ts = related_pairs(_rng("17"), 17, 150, 182, 0)
    return ModelBatch.from_pairs(qs[:1], ts[:1]), ModelBatch.from_pairs(qs, ts)


def ops_batch():
    return ModelBatch.from_pairs(*related_pairs(_rng("ops"), 300, 150, 182))


def ops_codes(n):
    return (np.arange(n) % 4).astype(np.uint8), ((np.arange(n) // 4) % 4).astype(np.uint8)


def named_batches():
    """name -> (builder, scores): every batch tests/test_gpu_semi_cigar.py runs."""
    reg = {}
    for ql in SHAPE_QL:
        for tl in shape_tl(ql):
            reg[f"shape_{ql}x{tl}"] = (lambda ql=ql, tl=tl: shape_batch(ql, tl), DEFAULT)
    reg["single"] = (lambda: single_and_17()[0], DEFAULT)
    reg["seventeen"] = (lambda: single_and_17()[1], DEFAULT)
    reg["related"] = (content_related, DEFAULT)
    reg["unrelated"] = (content_unrelated, DEFAULT)
    reg["overhang"] = (content_overhang, DEFAULT)
    reg["repeats"] = (content_repeats, DEFAULT)
    reg["n_targets"] = (n_targets, DEFAULT)
    # a score set the packed value window refuses; its int16 range admits the short shapes only
    for ql in M200_QL:
        for tl in shape_tl(ql):
            reg[f"m200_{ql}x{tl}"] = (lambda ql=ql, tl=tl: shape_batch(ql, tl), MATCH200)
    reg["sorted"] = (sorted_lengths, DEFAULT)
    reg["overflow"] = (overflow_pairs, OVERFLOW)
    reg["ops"] = (lambda: I.apply_ops(ops_batch(), *ops_codes(300)), DEFAULT)
    return reg


_cache = {}


def reference(name):
    """(batch, model result) of a named batch, computed once per process."""
    if name not in _cache:
        build, sc = named_batches()[name]
        b = build()
        _cache[name] = (b, semi_cigar(b, **sc))
    return _cache[name]
