"""A second witness for the banded BestSink: nvbio's banded score pass with its sink reports,
restated from the reference's own lines and not from oracle/nvbio_oracle.c.

  sw/sw_banded_inl.h:44-54      row zero, linear gaps: band[j] = GLOBAL ? j * deletion : 0
  sw/sw_banded_inl.h:365        a text shorter than its pattern returns before any report
  sw/sw_banded_inl.h:392-475    the rows; LOCAL clamps at 0 and reports every cell at
                                (i + j + 1, i + 1) (:416, :436-439, :465)
  sw/sw_banded_inl.h:453        the band's last text symbol reads 255 past the text's end
  sw/sw_banded_inl.h:494-510    GLOBAL reports band[B-1] at (M + B - 1, M); SEMI_GLOBAL band[0] at
                                (M, M), then band[j] at (M + j, M) while j < m,
                                m = min(M + B - 1, N) - (M - 1) in uint32
  ed/ed_banded_inl.h:63-78      ED is the SW pass under EditDistanceSWScheme: (0, -1, -1, -1)
  gotoh/gotoh_banded_inl.h:44-75, :463-618, :642-659   the same with affine gaps: F from the row
                                above, E carried along the row, the same reports
  sink_inl.h:59-68              BestSink::report keeps a score when best <= score: the last maximum

The loops over rows and band slots are the reference's; every step is taken for all pairs of a batch
at once (numpy arrays over the pairs), a pair standing still once its own rows are done.  A report
is made in the reference's order, so the first maximum (keep_first) can be had as well as the last:
the tests count the pairs where the two differ."""
import numpy as np

INT32_MIN = -2 ** 31
NO_SINK = 0xFFFFFFFF
ED, SW, GOTOH = 0, 1, 2
GLOBAL, LOCAL, SEMI_GLOBAL = 0, 1, 2


def unpack(S, k=0):
    """String k of a gasal_ffi.PackedSet (the one shared string when it has no offsets)."""
    per, mask = 32 // S.bits, (1 << S.bits) - 1
    lo, hi = (0, int(S.length)) if S.offsets is None else (int(S.offsets[k]), int(S.offsets[k + 1]))
    idx = np.arange(lo, hi, dtype=np.int64)
    pos = idx % per
    sh = (32 - S.bits * (pos + 1)) if S.big_endian else S.bits * pos
    return ((np.asarray(S.words, np.uint32)[idx // per].astype(np.int64) >> sh) & mask).astype(np.int64)


class _Sink:
    """BestSink over n pairs: report(h, x, y, who) offers score h at (x, y) to the pairs in `who`."""

    def __init__(self, n, keep_first):
        self.score = np.full(n, INT32_MIN, np.int64)
        self.x = np.full(n, NO_SINK, np.int64)
        self.y = np.full(n, NO_SINK, np.int64)
        self.keep_first = keep_first

    def report(self, h, x, y, who):
        take = who & ((self.score < h) if self.keep_first else (self.score <= h))
        self.score = np.where(take, h, self.score)
        self.x = np.where(take, x, self.x)
        self.y = np.where(take, y, self.y)


def best_sinks(al, band, patterns, texts, keep_first=False):
    """(scores int32[n], sinks uint32[n, 2]) of patterns[k] against texts[k] (lists of symbol arrays)."""
    n, B = len(patterns), band
    M = np.array([len(p) for p in patterns], np.int64)
    N = np.array([len(t) for t in texts], np.int64)
    rows = int(M.max(initial=0))
    pat = np.full((n, rows + 1), -1, np.int64)
    txt = np.full((n, int(N.max(initial=0)) + rows + B + 1), 255, np.int64)      # 255 past the text's end
    for k in range(n):
        pat[k, :M[k]] = patterns[k]
        txt[k, :N[k]] = texts[k]
    match, mismatch, go, ge, dele, ins = (al.match, al.mismatch, al.gap_open, al.gap_ext, al.deletion, al.insertion)
    if al.aligner == ED:
        match, mismatch, dele, ins = 0, -1, -1, -1
    gotoh, type_ = al.aligner == GOTOH, al.type
    run = N >= M                                                                  # the others return at once
    sink = _Sink(n, keep_first)
    col = lambda v: np.full(n, v, np.int64)
    if gotoh:
        infimum = -32768 - max(go, ge)
        H = [col(0)] + [col(go + (j - 1) * ge if type_ == GLOBAL else 0) for j in range(1, B)]
        F = [col(infimum) for _ in range(B)]
    else:
        H = [col(j * dele if type_ == GLOBAL else 0) for j in range(B)]
    for i in range(rows):
        live = run & (i < M)
        q = pat[:, i]
        Hn, Fn, E = [], [], None
        for j in range(B):
            diagonal = H[j] + np.where(txt[:, i + j] == q, match, mismatch)
            if gotoh:
                Fn.append(np.maximum(F[j + 1] + ge, H[j + 1] + go) if j < B - 1 else col(infimum))
                if j == 0:
                    hi = np.maximum(Fn[0], diagonal)
                elif j == B - 1:
                    hi = np.maximum(E, diagonal)
                else:
                    hi = np.maximum(np.maximum(Fn[j], E), diagonal)
            else:
                hi = diagonal
                if j < B - 1:
                    hi = np.maximum(hi, H[j + 1] + dele)                          # top
                if j > 0:
                    hi = np.maximum(hi, Hn[j - 1] + ins)                          # left: this row's cell
            if type_ == LOCAL:
                hi = np.maximum(hi, 0)
                sink.report(hi, i + j + 1, i + 1, live)
            Hn.append(hi)
            if gotoh:
                E = hi + go if j == 0 else np.maximum(hi + go, E + ge)
        H = [np.where(live, a, b) for a, b in zip(Hn, H)]
        if gotoh:
            F = [np.where(live, a, b) for a, b in zip(Fn, F)]
    if type_ == GLOBAL:
        sink.report(H[B - 1], M + B - 1, M, run)
    elif type_ == SEMI_GLOBAL:
        m = (np.minimum(M + B - 1, N) - (M - 1)) & 0xFFFFFFFF
        sink.report(H[0], M, M, run)
        for j in range(1, B):
            sink.report(H[j], M + j, M, run & (j < m))
    return sink.score.astype(np.int32), np.stack([sink.x, sink.y], axis=1).astype(np.uint32)


def batch(al, band, P, T, keep_first=False):
    """best_sinks over two gasal_ffi.PackedSets (T may be one shared text)."""
    shared = unpack(T) if T.offsets is None else None
    return best_sinks(al, band, [unpack(P, k) for k in range(P.n)],
                      [shared if shared is not None else unpack(T, k) for k in range(P.n)], keep_first)


def tie_pairs(seed, n=1500, max_m=200, symbols=4):
    """The inputs of the banded-sink tests: patterns of 0..max_m symbols against texts of m - 3 ..
    m + 40 (skipped pairs, clipped SEMI_GLOBAL ranges, LOCAL sinks past the text's end), related by
    a cut with substitutions.  Equal maxima are built in: every fourth pair is a run of a
    three-symbol unit against a longer run of the same unit (the same alignment one unit further
    along scores the same), every eighth pair has a pattern and a text without a common symbol (the
    best is 0 in every cell).  `symbols`: 4, or 5 to put N (4) into some patterns."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for k in range(n):
        m = int(rng.integers(0, max_m + 1)) if k % 16 else (k // 16) % 3          # empty and tiny patterns too
        tl = max(m + int(rng.integers(-3, 41)), 0)
        if k % 8 == 7:
            a, b = rng.permutation(4)[:2]
            p, t = np.full(m, a), np.full(tl, b)
        elif k % 4 == 1:
            unit = rng.permutation(4)[:3]
            reps = m // 3
            p, t = np.tile(unit, reps), np.tile(unit, reps + 3 + int(rng.integers(0, 4)))
        else:
            t = rng.integers(0, 4, tl)
            st = int(rng.integers(0, min(max(tl - m, 0), 12) + 1))
            p = np.concatenate([t[st:st + m], rng.integers(0, 4, max(m - len(t[st:st + m]), 0))])
            sub = rng.random(m) < 0.06
            p[sub] = rng.integers(0, symbols, int(sub.sum()))
        pats.append(np.asarray(p, np.uint32))
        texts.append(np.asarray(t, np.uint32))
    return pats, texts
