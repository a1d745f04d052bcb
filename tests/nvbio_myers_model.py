"""Plain Python/numpy restatement of nvbio's banded Myers bit-vector edit distance, the function
behind EditDistanceAligner<TYPE, MyersTag<ALPHABET_SIZE>> under BatchedBandedAlignmentScore<BAND_LEN>:
banded_myers<BAND_LEN, C = 0, TYPE, ALPHABET_SIZE> (NvB/nvbio/alignment/myers/myers_banded_inl.h;
every rule below carries its line there) reporting into a BestSink (alignment/sink_inl.h).  Test
infrastructure only: the reference of tests/test_gpu_nvbio_myers.py, pinned by the hand-worked cases
of tests/test_nvbio_myers_model.py.  It reads the packed string sets the API takes
(gasal_ffi.PackedSet) and shares no code with the kernel or the oracle.

Two points the reference leaves open, settled as csrc/nvmyers.hpp settles them:
  - MyersBitVectors<5>'s constructor zeroes B[0..3] only (:160-164): B[4] starts at 0 here.
  - with text_len == pattern_len phase 2 starts at s = BAND_LEN (:272); at BAND_LEN 32 the report
    bits are HP >> 32 and HN >> 32, read as 0 (a shift by the register width, as the device code
    the reference compiles to gives)."""
import numpy as np

import gasal_ffi as G

INT32_MIN = -2 ** 31
NO_SINK = 0xFFFFFFFF
U32 = 0xFFFFFFFF


class BitVectors:
    """MyersBitVectors<ALPHABET_SIZE> (:42-194)."""

    def __init__(self, alphabet):
        assert alphabet in (2, 4, 5)
        self.alphabet = alphabet
        self.B = [0] * alphabet          # :52, :82, :121; <5> :163-164 zeroes B[0..3], B[4] = 0 here

    def load(self, c, v):
        if self.alphabet == 2:
            self.B[c & 1] |= v           # :88-90
        elif self.alphabet == 4:
            self.B[c & 3] |= v           # :127-131
        elif c <= 4:
            self.B[c] |= v               # :170-174: a symbol above 4 loads nothing

    def get(self, c):
        if self.alphabet == 2:
            return self.B[c & 1]         # :96-97
        if self.alphabet == 4:
            return self.B[c & 3]         # :137-140
        return self.B[c] if c <= 3 else self.B[4]   # :180-182: anything above 3 answers B[4]

    def shift(self):
        self.B = [b >> 1 for b in self.B]   # :62-67, :101-106, :144-149, :186-191


def column(eq, VP, VN):
    """The column both diagonal_column and horizontal_column run (:198-206, :215-221), in uint32:
    (D0, HP, HN, VP', VN')."""
    X = eq | VN
    D0 = ((((VP + (X & VP)) & U32) ^ VP) | X) & U32
    HN = VP & D0
    HP = (VN | (~(VP | D0) & U32)) & U32
    X = D0 >> 1
    VN = X & HP
    VP = (HN | (~(X | HP) & U32)) & U32
    return D0, HP, HN, VP, VN


def banded_myers(type_, alphabet, band, pattern, text):
    """(score, x, y) the BestSink holds after banded_myers<band, 0, type_, alphabet>(pattern, text,
    min_score = the sink's minimum, sink): INT32_MIN and the empty sink when nothing is reported."""
    assert type_ in (G.NV_GLOBAL, G.NV_SEMI_GLOBAL) and 2 <= band <= 32
    M, N = len(pattern), len(text)
    best, sink = INT32_MIN, (NO_SINK, NO_SINK)       # sink_inl.h:40

    def report(score, x, y):                          # sink_inl.h:59-68
        nonlocal best, sink
        if best <= score:
            best, sink = score, (x, y)

    if N < M:                                         # :245-246
        return best, sink[0], sink[1]
    B = BitVectors(alphabet)                          # :248
    VP, VN = U32, 0                                   # :250-251
    dist = 0                                          # :253, C = 0 (and :257-258 loads nothing)
    top = 1 << (band - 1)
    last = min((N - 1) & U32, M)                      # :261, uint32 arithmetic
    for i in range(last):                             # :262
        B.shift()                                     # :264
        B.load(int(pattern[i]), top)                  # :266
        D0, HP, HN, VP, VN = column(B.get(int(text[i])), VP, VN)
        dist -= 1 - ((D0 >> (band - 1)) & 1)          # :268, :208
    s = band - 1 + M - last                           # :272
    i = last
    while i < N and s >= 0:                           # :273
        B.shift()                                     # :275
        D0, HP, HN, VP, VN = column(B.get(int(text[i])), VP, VN)
        if s < 32:                                    # :223; s == 32: both bits read as 0 (module docstring)
            dist -= ((HP >> s) & 1) - ((HN >> s) & 1)   # :277
        if type_ == G.NV_SEMI_GLOBAL:                 # :280-281 (dist >= min_score always holds)
            report(dist, i + 1, M)
        s -= 1                                        # :283
        i += 1
    if type_ == G.NV_GLOBAL:                          # :285-286
        report(dist, N, M)
    return best, sink[0], sink[1]


def unpack(S, k=None):
    """Symbol codes of string k of a gasal_ffi.PackedSet (k None: the shared string), read as the
    API reads them: `bits` per symbol, from the top of each word when big_endian."""
    per = 32 // S.bits
    if S.offsets is None:
        a, b = 0, int(S.length)
    else:
        a, b = int(S.offsets[k]), int(S.offsets[k + 1])
    idx = np.arange(a, b, dtype=np.int64)
    pos = idx % per
    sh = (32 - S.bits * (pos + 1)) if S.big_endian else S.bits * pos
    w = np.asarray(S.words, np.uint32)[idx // per].astype(np.uint64)
    return ((w >> sh.astype(np.uint64)) & np.uint64((1 << S.bits) - 1)).astype(np.uint32)


def batch(type_, alphabet, band, P, T):
    """scores int32[n], sinks uint32[n, 2] of the packed sets P (patterns) and T (texts, per pair or shared)."""
    n = P.n
    shared = unpack(T) if T.offsets is None else None
    r = [banded_myers(type_, alphabet, band, unpack(P, k), shared if shared is not None else unpack(T, k))
         for k in range(n)]
    return (np.array([v[0] for v in r], np.int64).astype(np.int32),
            np.array([[v[1], v[2]] for v in r], np.uint32).reshape(-1, 2))
