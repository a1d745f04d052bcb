"""The definition the quality-aware banded Gotoh kernels are tested against: nvbio's banded Gotoh
score pass and banded traceback under a scheme whose substitution score depends on the base quality
of the pattern symbol, restated in Python from the reference's own lines (no oracle code is used).

  nvBowtie/bowtie2/cuda/scoring.h:286-289   match(qq), mismatch(qq), substitution(r_i, q_j, r, q, qq) =
                                            r == q ? m_match(qq) : -m_mmp(qq)
  nvBowtie/bowtie2/cuda/scoring.h:97-101    QualCost: min + int(min(q, 40) / 40.0f * (max - min))
  nvBowtie/bowtie2/cuda/scoring.h:111-125   ConstantCost: the same value at every quality
  nvBowtie/bowtie2/cuda/scoring.h:68-80,
  nvBowtie/bowtie2/quality_coeffs.h:44-54   RoundedQualCost: phred_to_maq(q) = 0 / 10 / 20 / 30 by the
                                            steps q < 5, < 15, < 25
  nvBowtie/bowtie2/cuda/scoring_inl.h:117-118   the default m_mmp(2, 6): bowtie2's --mp 6,2
  gotoh/gotoh_banded_inl.h:431              a text shorter than its pattern returns before any report
  gotoh/gotoh_banded_inl.h:441-448          the first band of the text; G_o, G_e (the pattern gap scores) and
                                            the infimum
  gotoh/gotoh_banded_inl.h:44-75            row zero: H = 0, then GLOBAL G_o + (j - 1) G_e, else 0; F = infimum
  gotoh/gotoh_banded_inl.h:469-470          q = pattern[i], qq = quals[i]: one quality per row
  gotoh/gotoh_banded_inl.h:482-614          the row: F from the slot to the right in the row above, E carried
                                            along the row, S_ij = substitution(.., g, q, qq) in every cell
                                            (:492, :544, :591); LOCAL clamps at 0, reports every cell at
                                            (i + j + 1, i + 1) and flags a zero as SINK; the directions:
                                            top > left ? (top > diagonal ? INSERTION : SUBSTITUTION)
                                                       : (left > diagonal ? DELETION : SUBSTITUTION),
                                            fdir = ftop > htop, edir (of the next slot) = eleft > ediagonal
  gotoh/gotoh_banded_inl.h:580              the band's last text symbol reads 255 past the text's end
  gotoh/gotoh_banded_inl.h:639-656          GLOBAL reports band[B-1] at (M + B - 1, M); SEMI_GLOBAL band[0] at
                                            (M, M), then band[j] at (M + j, M) while j < m,
                                            m = min(M + B - 1, N) - (M - 1) in uint32
  gotoh/gotoh_banded_inl.h:323-339          a cell's flags: (LOCAL and score 0 ? SINK : hdir) | edir | fdir
  sink_inl.h:59-68                          BestSink keeps a score when best <= score: the last maximum
  banded_inl.h:352-427                      the traceback: score with checkpoints, then from the sink's
                                            window backwards recompute the flags and walk them; the source
                                            is where the walk ends
  gotoh/gotoh_banded_inl.h:908-961          the walk: entry = sink.x - sink.y, row = sink.y - 1; in H a SINK
                                            flag (LOCAL) ends it, DELETION enters E, INSERTION enters F, else
                                            one row up and push SUBSTITUTION; in E one entry left and push
                                            DELETION, leaving E when INSERTION_EXT is clear; in F one entry
                                            right, one row up and push INSERTION, leaving F when DELETION_EXT
                                            is clear; off the top the source is (entry, 0)

The checkpoints only bound the reference's storage (their int16 clamp is what the entry points'
range rule keeps every score away from), so one pass gives every cell's value and flags.  One pair
at a time, plain Python integers."""
import numpy as np

INT32_MIN = -2 ** 31
NO_SINK = 0xFFFFFFFF
GLOBAL, LOCAL, SEMI_GLOBAL = 0, 1, 2
SUBSTITUTION, INSERTION, DELETION, SINK = 0, 1, 2, 3
INSERTION_EXT, DELETION_EXT = 4, 8


# ---- the table builders (the host evaluates them, float arithmetic included) ----

def qual_cost(lo, hi, levels=256):
    """QualCost(min, max) at q = 0 .. levels - 1 (scoring.h:97-101): float32 as the reference."""
    f = np.float32
    return [int(lo) + int(f(f(min(q, 40)) / f(40.0)) * f(hi - lo)) for q in range(levels)]


def constant_cost(v, levels=256):
    return [int(v)] * levels


def rounded_qual_cost(levels=256):
    """RoundedQualCost (scoring.h:68-80) is phred_to_maq(q) whatever its two arguments
    (quality_coeffs.h:44-54): 0 below 5, 10 below 15, 20 below 25, else 30."""
    return [0 if q < 5 else 10 if q < 15 else 20 if q < 25 else 30 for q in range(levels)]


class Scheme:
    """match[l], mismatch[l] (signed scores), the number of levels, gap open and extension."""

    def __init__(self, match, mismatch, gap_open, gap_ext):
        assert len(match) == len(mismatch) and 1 <= len(match) <= 256
        self.match_t, self.mismatch_t = [int(v) for v in match], [int(v) for v in mismatch]
        self.levels, self.gap_open, self.gap_ext = len(match), int(gap_open), int(gap_ext)

    def level(self, qq):
        return min(int(qq), self.levels - 1)

    def substitution(self, r, q, qq):                      # scoring.h:289
        l = self.level(qq)
        return self.match_t[l] if r == q else self.mismatch_t[l]


def nvbowtie_default():
    """nvBowtie's defaults: match 0, mismatch -QualCost(2, 6), gaps -(5 + 3) and -3 (scoring.h:290-291)."""
    return Scheme(constant_cost(0), [-v for v in qual_cost(2, 6)], -8, -3)


def constant_scheme(match, mismatch, gap_open, gap_ext, levels=1):
    return Scheme(constant_cost(match, levels), constant_cost(mismatch, levels), gap_open, gap_ext)


# ---- one pair ----

def _pass(sc, type_, B, pattern, quals, text, want_flags):
    """The score pass: (score, sink x, sink y, flags[row][slot]) with BestSink's last maximum."""
    M, N = len(pattern), len(text)
    if N < M:
        return INT32_MIN, NO_SINK, NO_SINK, None
    G_o, G_e = sc.gap_open, sc.gap_ext
    infimum = -32768 - max(G_o, G_e)
    H = [0] + [(G_o + (j - 1) * G_e) if type_ == GLOBAL else 0 for j in range(1, B)]
    F = [infimum] * B
    best, bx, by = INT32_MIN, NO_SINK, NO_SINK
    flags = []
    txt = lambda x: int(text[x]) if x < N else 255
    for i in range(M):
        q, qq = int(pattern[i]), int(quals[i])
        row = []
        E, edir = None, SUBSTITUTION
        for j in range(B):
            last = j == B - 1
            if not last:
                ftop, htop = F[j + 1] + G_e, H[j + 1] + G_o
                F[j] = max(ftop, htop)
                fdir = DELETION_EXT if ftop > htop else SUBSTITUTION
            else:
                F[j] = infimum
                fdir = SUBSTITUTION
            diagonal = H[j] + sc.substitution(txt(i + j), q, qq)
            top, left = F[j], E
            if j == 0:
                hi = max(top, diagonal)
                hdir = INSERTION if top > diagonal else SUBSTITUTION
            elif last:
                hi = max(left, diagonal)
                hdir = DELETION if left > diagonal else SUBSTITUTION
            else:
                hi = max(top, left, diagonal)
                hdir = ((INSERTION if top > diagonal else SUBSTITUTION) if top > left
                        else (DELETION if left > diagonal else SUBSTITUTION))
            if type_ == LOCAL:
                hi = max(hi, 0)
                if hi == 0:
                    hdir = SINK
                if best <= hi:
                    best, bx, by = hi, i + j + 1, i + 1
            H[j] = hi
            row.append(hdir | (SUBSTITUTION if j == 0 else edir) | fdir)
            if j == 0:
                E, edir = hi + G_o, SUBSTITUTION
            else:
                eleft, ediagonal = E + G_e, hi + G_o
                edir = INSERTION_EXT if eleft > ediagonal else SUBSTITUTION
                E = max(ediagonal, eleft)
        if want_flags:
            flags.append(row)
    if type_ == GLOBAL:
        if best <= H[B - 1]:
            best, bx, by = H[B - 1], M + B - 1, M
    elif type_ == SEMI_GLOBAL:
        m = (min(M + B - 1, N) - (M - 1)) & 0xFFFFFFFF
        for j in range(B):
            if (j == 0 or j < m) and best <= H[j]:
                best, bx, by = H[j], M + j, M
    return best, bx, by, flags


def score_one(sc, type_, B, pattern, quals, text):
    s, x, y, _ = _pass(sc, type_, B, pattern, quals, text, False)
    return s, x, y


def traceback_one(sc, type_, B, pattern, quals, text):
    """(score, (source x, y), (sink x, y), ops in push order) of one pair."""
    best, bx, by, flags = _pass(sc, type_, B, pattern, quals, text, True)
    if bx == NO_SINK:
        return best, (NO_SINK, NO_SINK), (NO_SINK, NO_SINK), []
    entry, row, state, ops, found = bx - by, by - 1, 0, [], False
    while row >= 0:
        op = flags[row][entry]
        h_op = op & 3
        if type_ == LOCAL and state == 0 and h_op == SINK:
            found = True
            break
        if state == 1:                                     # E
            if not op & INSERTION_EXT:
                state = 0
            entry -= 1
            ops.append(DELETION)
        elif state == 2:                                   # F
            if not op & DELETION_EXT:
                state = 0
            entry += 1
            row -= 1
            ops.append(INSERTION)
        elif h_op == DELETION:
            state = 1
        elif h_op == INSERTION:
            state = 2
        else:
            row -= 1
            ops.append(SUBSTITUTION)
        assert 0 <= entry < B
    sy = row + 1 if found else 0
    return best, (entry + sy, sy), (bx, by), ops


# ---- batches: the same pass, every step taken for all pairs at once (numpy arrays over the pairs, a
#      pair standing still once its own rows are done), as nvbio_banded_sinks_model.py does; the walk
#      stays per pair.  test_nvbio_qual_model.py holds the two forms against each other. ----

def _pass_batch(sc, type_, B, patterns, quals, texts, want_flags):
    n = len(patterns)
    M = np.array([len(p) for p in patterns], np.int64)
    N = np.array([len(t) for t in texts], np.int64)
    rows = int(M.max(initial=0))
    pat = np.full((n, rows + 1), -1, np.int64)
    qq = np.zeros((n, rows + 1), np.int64)
    txt = np.full((n, int(N.max(initial=0)) + rows + B + 1), 255, np.int64)      # 255 past the text's end
    for k in range(n):
        pat[k, :M[k]] = patterns[k]
        qq[k, :M[k]] = quals[k]
        txt[k, :N[k]] = texts[k]
    match_t, mismatch_t = np.array(sc.match_t, np.int64), np.array(sc.mismatch_t, np.int64)
    G_o, G_e = sc.gap_open, sc.gap_ext
    infimum = -32768 - max(G_o, G_e)
    run = N >= M
    col = lambda v: np.full(n, v, np.int64)
    H = [col(0)] + [col(G_o + (j - 1) * G_e if type_ == GLOBAL else 0) for j in range(1, B)]
    F = [col(infimum) for _ in range(B)]
    best, bx, by = col(INT32_MIN), col(NO_SINK), col(NO_SINK)

    def report(h, x, y, who):
        nonlocal best, bx, by
        take = who & (best <= h)
        best, bx, by = np.where(take, h, best), np.where(take, x, bx), np.where(take, y, by)

    flags = np.zeros((rows, B, n), np.uint8) if want_flags else None
    for i in range(rows):
        live = run & (i < M)
        q = pat[:, i]
        level = np.minimum(qq[:, i], sc.levels - 1)
        s_eq, s_ne = match_t[level], mismatch_t[level]
        Hn, Fn, E, edir = [], [], None, col(SUBSTITUTION)
        for j in range(B):
            last = j == B - 1
            if not last:
                ftop, htop = F[j + 1] + G_e, H[j + 1] + G_o
                Fn.append(np.maximum(ftop, htop))
                fdir = np.where(ftop > htop, DELETION_EXT, SUBSTITUTION)
            else:
                Fn.append(col(infimum))
                fdir = col(SUBSTITUTION)
            diagonal = H[j] + np.where(txt[:, i + j] == q, s_eq, s_ne)
            top, left = Fn[j], E
            if j == 0:
                hi = np.maximum(top, diagonal)
                hdir = np.where(top > diagonal, INSERTION, SUBSTITUTION)
            elif last:
                hi = np.maximum(left, diagonal)
                hdir = np.where(left > diagonal, DELETION, SUBSTITUTION)
            else:
                hi = np.maximum(np.maximum(top, left), diagonal)
                hdir = np.where(top > left, np.where(top > diagonal, INSERTION, SUBSTITUTION),
                                np.where(left > diagonal, DELETION, SUBSTITUTION))
            if type_ == LOCAL:
                hi = np.maximum(hi, 0)
                hdir = np.where(hi == 0, SINK, hdir)
                report(hi, i + j + 1, i + 1, live)
            Hn.append(hi)
            if want_flags:
                flags[i, j] = hdir | (edir if j else SUBSTITUTION) | fdir
            if j == 0:
                E, edir = hi + G_o, col(SUBSTITUTION)
            else:
                eleft, ediagonal = E + G_e, hi + G_o
                edir = np.where(eleft > ediagonal, INSERTION_EXT, SUBSTITUTION)
                E = np.maximum(ediagonal, eleft)
        H = [np.where(live, a, b) for a, b in zip(Hn, H)]
        F = [np.where(live, a, b) for a, b in zip(Fn, F)]
    if type_ == GLOBAL:
        report(H[B - 1], M + B - 1, M, run)
    elif type_ == SEMI_GLOBAL:
        m = (np.minimum(M + B - 1, N) - (M - 1)) & 0xFFFFFFFF
        report(H[0], M, M, run)
        for j in range(1, B):
            report(H[j], M + j, M, run & (j < m))
    return best, bx, by, flags


def best_sinks(sc, type_, band, patterns, quals, texts):
    """(scores int32[n], sinks uint32[n, 2])"""
    best, bx, by, _ = _pass_batch(sc, type_, band, patterns, quals, texts, False)
    return best.astype(np.int32), np.stack([bx, by], axis=1).astype(np.uint32)


def _walk(type_, B, flags, k, bx, by):
    entry, row, state, ops, found = bx - by, by - 1, 0, [], False
    while row >= 0:
        op = int(flags[row, entry, k])
        h_op = op & 3
        if type_ == LOCAL and state == 0 and h_op == SINK:
            found = True
            break
        if state == 1:
            if not op & INSERTION_EXT:
                state = 0
            entry -= 1
            ops.append(DELETION)
        elif state == 2:
            if not op & DELETION_EXT:
                state = 0
            entry += 1
            row -= 1
            ops.append(INSERTION)
        elif h_op == DELETION:
            state = 1
        elif h_op == INSERTION:
            state = 2
        else:
            row -= 1
            ops.append(SUBSTITUTION)
        assert 0 <= entry < B
    sy = row + 1 if found else 0
    return (entry + sy, sy), ops


def traceback(sc, type_, band, patterns, quals, texts):
    """The dict oracle.nv_banded_traceback returns."""
    n = len(patterns)
    best, bx, by, flags = _pass_batch(sc, type_, band, patterns, quals, texts, True)
    source, ops = np.full((n, 2), NO_SINK, np.int64), []
    for k in range(n):
        if bx[k] == NO_SINK:
            ops.append(np.zeros(0, np.uint8))
            continue
        src, o = _walk(type_, band, flags, k, int(bx[k]), int(by[k]))
        source[k] = src
        ops.append(np.array(o, np.uint8))
    return dict(score=best.astype(np.int32), source=source.astype(np.uint32),
                sink=np.stack([bx, by], axis=1).astype(np.uint32), ops=ops)


def flat_quals(quals):
    """The byte array the entry points take: the pairs' qualities back to back (the pattern offsets)."""
    return np.ascontiguousarray(np.concatenate([np.asarray(q, np.uint8) for q in quals])
                                if quals else np.zeros(0, np.uint8), np.uint8)


def attach_quals(seed, pats):
    """Qualities for the test pairs: Phred-like bytes, mostly 2..41, a tenth spread over 0..255 (above
    40, the clamp of QualCost, and above levels - 1 of a short table), runs of equal bytes as
    sequencers give, and a low quality on most substituted-looking tails."""
    rng = np.random.default_rng(seed ^ 0x9A1)
    out = []
    for p in pats:
        m = len(p)
        q = rng.integers(2, 42, m)
        wide = rng.random(m) < 0.1
        q[wide] = rng.integers(0, 256, int(wide.sum()))
        if m > 8 and rng.random() < 0.5:
            a = int(rng.integers(0, m - 4))
            q[a:a + int(rng.integers(2, 9))] = int(rng.integers(0, 12))
        out.append(q.astype(np.uint8))
    return out
