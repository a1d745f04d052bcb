"""Plain-Python definition of nvbio's Smith-Waterman traceback, full-DP and banded, which the
edit-distance aligner traces back through as well (ed/ed_inl.h:347-365: EditDistanceSWScheme, match 0,
mismatch / deletion / insertion -1).  TEST INFRASTRUCTURE ONLY: the second reference of
nv_traceback_kernel<false, TYPE> and nv_banded_traceback_kernel<false, TYPE, BMAX, EX>
(csrc/nvtrace.hpp) beside oracle/nvbio_oracle.c.  Written from the reference lines below (paths under
NvB/nvbio/alignment), in another form than both: whole matrices of H and of directions first, with
the boundaries as row 0 / column 0 of the matrix; then BestSink's reports replayed in nvbio's order as
a step of its own; then the walk.  The band is indexed (pattern row, text column), not (row, entry).

Full DP (alignment_inl.h:365-465, PatternBlockingTag; rows i = text, columns j = pattern, one-based):
  H(0,0) = 0,  H(0,j) = LOCAL ? 0 : I*j (sw_inl.h:663-664, 712-713),  H(i,0) = GLOBAL ? G*i : 0 (:243-251)
  top = H(i-1,j) + G, left = H(i,j-1) + I, diagonal = H(i-1,j-1) + (t_i == p_j ? match : mismatch)
  H = max3, LOCAL: max(H, 0)                                                      (sw_inl.h:483-489)
  dir = top > left ? (top > diagonal ? DELETION : SUBSTITUTION)
                   : (left > diagonal ? INSERTION : SUBSTITUTION)                (sw_inl.h:497-499)
  LOCAL stores SINK where H == 0 (sw_inl.h:393-396)
  with G = scheme.deletion(), I = scheme.insertion() (sw_inl.h:637-638).
  BestSink (sink_inl.h:59-68) keeps the last maximum, best <= h, in report order: LOCAL every cell, per
  stripe of pattern columns, inside a stripe per text row, inside a row per column (sw_inl.h:509-526);
  SEMI_GLOBAL H(i, M) per text row (sw_inl.h:529-533, utils_inl.h:279-299); GLOBAL H(N, M)
  (sw_inl.h:754-755, utils_inl.h:273-285).  The stripes are sw_bandlen_selector<TYPE, 1, symbol>::BAND_LEN
  = 16 / DIM = 16 columns wide (sw_inl.h:1330-1334, taken at :1546 and :1595; ed_inl.h:95-290 take the
  same selector) -- the Gotoh selector is 8 (gotoh_inl.h:1492-1495), the SW one is not.
  The walk (sw_inl.h:1653-1709): from the sink while row > 0 and column >= 0; LOCAL stops on SINK; an op
  other than DELETION leaves the column, one other than INSERTION the row; the op is pushed.  Then the
  tails (alignment_inl.h:442-459): not LOCAL and row 0 reached -> INSERTIONs down to column 0; GLOBAL
  and column 0 reached -> DELETIONs down to row 0.  Source = where that ends.

Banded (banded_inl.h:352-427; rows i = pattern, zero-based cell (i, c) with 0 <= c - i < B; pairs whose
text is shorter than the pattern are skipped, sw_banded_inl.h:365-366):
  row -1 holds c = -1 .. B-2:  H(-1,c) = GLOBAL ? (c + 1) * G : 0               (sw_banded_inl.h:44-54)
  diagonal = H(i-1,c-1) + S;  top = H(i-1,c) + G where (i-1,c) is in the band (c - i < B - 1);
  left = H(i,c-1) + I where c > i; text symbols at c >= N read 255           (sw_banded_inl.h:406-474)
  dir = top > left ? (top > diagonal ? INSERTION : SUBSTITUTION)
                   : (left > diagonal ? DELETION : SUBSTITUTION), the two-way forms at the band's edges.
  So the banded file names the vertical move INSERTION and the horizontal one DELETION, as they are
  (rows = pattern), but keeps G on the vertical and I on the horizontal one: a pattern-only step costs
  scheme.deletion() here and scheme.insertion() in the full DP.  replay() prices steps that way.
  No SINK is ever stored (sw_banded_inl.h:268-279), so a LOCAL walk runs on through zero cells to row 0.
  Reports: LOCAL every cell, row by row, c ascending, at (c + 1, i + 1) (:416, :439, :465); GLOBAL
  H(M-1, M+B-2) at (M + B - 1, M) whatever the text length (:496-497); SEMI_GLOBAL H(M-1, M-1+j) for
  j = 0 and 0 < j < min(M + B - 1, N) - (M - 1) (:498-510).
  The walk (sw_banded_inl.h:740-798): entry = x - y, row = y - 1; DELETION: entry - 1; INSERTION:
  entry + 1, row - 1; SUBSTITUTION: row - 1; until row < 0; source = (entry, 0).  No tails: a GLOBAL
  source with x > 0 stands on row -1's x * G.

Empty strings, from the same lines:
  * Banded, empty pattern: the row loop does not run and row -1 is reported (:494-510): GLOBAL
    (B - 1) * G at (B - 1, 0), SEMI_GLOBAL 0 at (min(B - 1, N), 0), LOCAL nothing.  sink.y = 0 is a valid
    cell (banded_inl.h:389-392), no checkpoint holds it (:398, :413), so source = sink and no pushes.
  * Banded, empty text under a pattern: skipped.
  * Full DP, LOCAL or SEMI_GLOBAL, empty text: no row, so no report: BestSink stays INT32_MIN at
    (0xFFFFFFFF, 0xFFFFFFFF) and alignment_inl.h:408-411 returns that, no pushes.  LOCAL, empty
    pattern: the CHECK_M guard (sw_inl.h:514-518) reports nothing either.
  * Full DP, empty pattern, GLOBAL / SEMI_GLOBAL: the last stripe still runs its rows over the 16
    columns past M with a query cache that sw_inl.h:716-722 never filled, and select_dispatch
    (utils_inl.h:206-226) reports band[((M - 1) & 15) + 1] of it: the reference's answer is undefined.
  * Full DP, GLOBAL, empty text under a pattern: nvbio reports I * M at (0, M) (row 0 of the last stripe,
    sw_inl.h:712-713, :754-755), the walk does not start (row 0) and the first-row tail pushes M
    INSERTIONs (alignment_inl.h:444-451).  The front-end (kernels, oracle, every model here) reports
    nothing for every pair with an empty string instead -- its documented contract ("Pairs
    that report nothing"), which full() follows; reference_global_empty_text() gives nvbio's answer and
    test_nvbio_sw_traceback_model.py pins the difference.
"""
import numpy as np

import gasal_ffi as G

INT32_MIN = -2 ** 31
NO_CELL = 0xFFFFFFFF
SUB, INS, DEL, SNK = 0, 1, 2, 3
FULL_STRIPE = 16          # sw_bandlen_selector: 16 / DIM, DIM = 1
PAST_TEXT = 255           # sw_banded_inl.h:453
NOTHING = dict(score=INT32_MIN, source=(NO_CELL, NO_CELL), sink=(NO_CELL, NO_CELL), ops=[], ties=0)


def scores(al):
    """(match, mismatch, G = deletion, I = insertion) of a gasal_ffi.NvAligner, SW or ED."""
    if al.aligner == G.NV_ED:
        return 0, -1, -1, -1                                  # ed_utils.h:45-52
    assert al.aligner == G.NV_SW
    return al.match, al.mismatch, al.deletion, al.insertion


def _ints(s):
    return [int(v) for v in s]


def _best_sink(reports):
    """BestSink over (h, (x, y)) in the order given: the last maximum."""
    best, cell = INT32_MIN, (NO_CELL, NO_CELL)
    for h, xy in reports:
        if best <= h:
            best, cell = h, xy
    return best, cell


def _three(top, left, diag, vertical, horizontal):
    """The strict three-way choice; top / left may be None at a band edge."""
    if top is None:
        return horizontal if left > diag else SUB
    if left is None:
        return vertical if top > diag else SUB
    if top > left:
        return vertical if top > diag else SUB
    return horizontal if left > diag else SUB


def _tied(cands, h):
    return sum(1 for v in cands if v is not None and v == h) >= 2


# ---------------------------------------------------------------- full DP
def full_matrices(al, p, t):
    """H[i][j] for 0 <= i <= N (text), 0 <= j <= M (pattern), boundaries included; D[i][j] the stored
    direction and C[i][j] = (top, left, diagonal) of every real cell."""
    match, mismatch, g, ins = scores(al)
    local, glob = al.type == G.NV_LOCAL, al.type == G.NV_GLOBAL
    M, N = len(p), len(t)
    H = [[0] * (M + 1) for _ in range(N + 1)]
    D = [[None] * (M + 1) for _ in range(N + 1)]
    C = [[None] * (M + 1) for _ in range(N + 1)]
    for j in range(1, M + 1):
        H[0][j] = 0 if local else ins * j
    for i in range(1, N + 1):
        H[i][0] = g * i if glob else 0
    for i in range(1, N + 1):
        for j in range(1, M + 1):
            top, left = H[i - 1][j] + g, H[i][j - 1] + ins
            diag = H[i - 1][j - 1] + (match if t[i - 1] == p[j - 1] else mismatch)
            h = max(top, left, diag)
            if local:
                h = max(h, 0)
            H[i][j], C[i][j] = h, (top, left, diag)
            D[i][j] = SNK if local and h == 0 else _three(top, left, diag, DEL, INS)
    return H, D, C


def full_reports(type_, H, stripe=FULL_STRIPE):
    N, M = len(H) - 1, len(H[0]) - 1
    if type_ == G.NV_LOCAL:
        for c0 in range(0, M, stripe):
            for i in range(1, N + 1):
                for j in range(c0 + 1, min(c0 + stripe, M) + 1):
                    yield H[i][j], (i, j)
    elif type_ == G.NV_SEMI_GLOBAL:
        for i in range(1, N + 1):
            yield H[i][M], (i, M)
    else:
        yield H[N][M], (N, M)


def full_walk(type_, D, sink):
    """(ops, source, cells): the pushes, where the walk and the tails end, the cells whose direction was read."""
    ops, cells = [], []
    i, j = sink
    while i > 0 and j > 0:
        op = D[i][j]
        if type_ == G.NV_LOCAL and op == SNK:
            break
        cells.append((i, j))
        if op != DEL:
            j -= 1
        if op != INS:
            i -= 1
        ops.append(op)
    if type_ != G.NV_LOCAL and i == 0:
        ops += [INS] * j
        j = 0
    if type_ == G.NV_GLOBAL and j == 0:
        ops += [DEL] * i
        i = 0
    return ops, (i, j), cells


def full(al, p, t, stripe=FULL_STRIPE):
    """dict(score, sink, source, ops, ties) of one pair under the full-DP traceback."""
    p, t = _ints(p), _ints(t)
    if not p or not t:
        return dict(NOTHING)
    H, D, C = full_matrices(al, p, t)
    best, sink = _best_sink(full_reports(al.type, H, stripe))
    ops, source, cells = full_walk(al.type, D, sink)
    return dict(score=best, sink=sink, source=source, ops=ops,
                ties=sum(_tied(C[i][j], max(C[i][j])) for i, j in cells))


def reference_global_empty_text(al, m):
    """What nvbio's lines give for a GLOBAL pair of an m-symbol pattern and an empty text (the docstring):
    the front-end reports nothing there."""
    assert al.type == G.NV_GLOBAL and m > 0
    return dict(score=scores(al)[3] * m, sink=(0, m), source=(0, 0), ops=[INS] * m, ties=0)


# ---------------------------------------------------------------- banded
def banded_matrices(al, band, p, t):
    """H, D, C keyed by (i, c): pattern row i (row -1 the boundary), text column c, 0 <= c - i < band."""
    match, mismatch, g, ins = scores(al)
    local, glob = al.type == G.NV_LOCAL, al.type == G.NV_GLOBAL
    M, N = len(p), len(t)
    H, D, C = {}, {}, {}
    for c in range(-1, band - 1):
        H[(-1, c)] = (c + 1) * g if glob else 0
    for i in range(M):
        for c in range(i, i + band):
            sym = t[c] if c < N else PAST_TEXT
            diag = H[(i - 1, c - 1)] + (match if sym == p[i] else mismatch)
            top = H[(i - 1, c)] + g if c - i < band - 1 else None
            left = H[(i, c - 1)] + ins if c > i else None
            h = max(v for v in (top, left, diag) if v is not None)
            if local:
                h = max(h, 0)
            H[(i, c)], C[(i, c)] = h, (top, left, diag)
            D[(i, c)] = _three(top, left, diag, INS, DEL)
    return H, D, C


def banded_reports(type_, band, H, M, N):
    if type_ == G.NV_LOCAL:
        for i in range(M):
            for c in range(i, i + band):
                yield H[(i, c)], (c + 1, i + 1)
    elif type_ == G.NV_GLOBAL:
        yield H[(M - 1, M + band - 2)], (M + band - 1, M)
    else:
        m = min(M + band - 1, N) - (M - 1)
        for j in range(band):
            if j == 0 or j < m:
                yield H[(M - 1, M - 1 + j)], (M + j, M)


def banded_walk(D, sink):
    ops, cells = [], []
    i, c = sink[1] - 1, sink[0] - 1
    while i >= 0:
        op = D[(i, c)]                      # never SINK: the banded SW pass stores none
        cells.append((i, c))
        if op == DEL:
            c -= 1
        elif op == INS:
            i -= 1
        else:
            i -= 1; c -= 1
        ops.append(op)
    return ops, (c + 1, 0) if sink[1] else sink, cells


def banded(al, band, p, t):
    """dict(score, sink, source, ops, ties) of one pair under the banded traceback, band 2..32."""
    assert 2 <= band <= 32
    p, t = _ints(p), _ints(t)
    if len(t) < len(p):
        return dict(NOTHING)
    H, D, C = banded_matrices(al, band, p, t)
    best, sink = _best_sink(banded_reports(al.type, band, H, len(p), len(t)))
    if sink[0] == NO_CELL:
        return dict(NOTHING)
    ops, source, cells = banded_walk(D, sink)
    return dict(score=best, sink=sink, source=source, ops=ops,
                ties=sum(_tied(C[k], max(v for v in C[k] if v is not None)) for k in cells))


# ---------------------------------------------------------------- batches, comparison
_cache = {}


def _key(al):
    return (al.aligner, al.type) + scores(al)


def _pair(al, band, p, t):
    k = (_key(al), band, bytes(np.asarray(p, np.uint8)), bytes(np.asarray(t, np.uint8)))
    if k not in _cache:
        _cache[k] = full(al, p, t) if band is None else banded(al, band, p, t)
    return _cache[k]


def _batch(al, band, pats, texts):
    if len(texts) == 1 and len(pats) != 1:
        texts = list(texts) * len(pats)
    r = [_pair(al, band, p, t) for p, t in zip(pats, texts)]
    return dict(score=np.array([v["score"] for v in r], np.int32),
                source=np.array([v["source"] for v in r], np.uint32).reshape(-1, 2),
                sink=np.array([v["sink"] for v in r], np.uint32).reshape(-1, 2),
                ops=[np.array(v["ops"], np.uint8) for v in r],
                ties=np.array([v["ties"] for v in r], np.int64))


def full_batch(al, pats, texts):
    """The dict oracle.nv_traceback returns, and ties int64[n]; texts: one per pattern, or one shared."""
    return _batch(al, None, pats, texts)


def banded_batch(al, band, pats, texts):
    """The dict oracle.nv_banded_traceback returns, and ties."""
    return _batch(al, band, pats, texts)


def unpack(S, n=None):
    """The symbol lists of a gasal_ffi.PackedSet (n copies of a shared one)."""
    per, mask = 32 // S.bits, (1 << S.bits) - 1
    def sym(k):
        pos = k % per
        sh = 32 - S.bits * (pos + 1) if S.big_endian else S.bits * pos
        return (int(S.words[k // per]) >> sh) & mask
    if S.offsets is None:
        one = np.array([sym(k) for k in range(S.length)], np.uint32)
        return [one] * (n or 1)
    o = [int(v) for v in S.offsets]
    return [np.array([sym(k) for k in range(o[i], o[i + 1])], np.uint32) for i in range(len(o) - 1)]


def full_batch_packed(al, P, T):
    return full_batch(al, unpack(P), unpack(T, P.n))


def banded_batch_packed(al, band, P, T):
    return banded_batch(al, band, unpack(P), unpack(T, P.n))


def one(res, k):
    """Pair k of a batch result."""
    return dict(score=int(res["score"][k]), source=tuple(int(v) for v in res["source"][k]),
                sink=tuple(int(v) for v in res["sink"][k]), ops=[int(v) for v in res["ops"][k]])


def same(got, want, what=""):
    """Bit for bit: score, source, sink, the number of pushes and every push; the message names the first
    pair that differs and the first field and push it differs in."""
    n = len(want["score"])
    assert len(got["score"]) == n == len(got["ops"]), f"{what}: {len(got['score'])} pairs, not {n}"
    bad = []
    for k in range(n):
        g, w = one(got, k), one(want, k)
        for f in ("score", "sink", "source"):
            if g[f] != w[f]:
                bad.append((k, f"{f} {g[f]} != {w[f]}"))
                break
        else:
            if g["ops"] != w["ops"]:
                at = next((x for x in range(min(len(g["ops"]), len(w["ops"]))) if g["ops"][x] != w["ops"][x]),
                          min(len(g["ops"]), len(w["ops"])))
                bad.append((k, f"{len(g['ops'])} pushes against {len(w['ops'])}, first difference at push {at}: "
                               f"got {g['ops'][at:at + 6]} want {w['ops'][at:at + 6]}"))
    if bad:
        k, why = bad[0]
        raise AssertionError(f"{what}: {len(bad)}/{n} pairs differ, first #{k}: {why}; got {one(got, k)} want {one(want, k)}")


def replay(al, p, t, result, band=None):
    """Walks the pushes from the source to the sink over the two strings.  Returns the score they spell;
    for the banded form (score, every cell inside the band).  Asserts that they end on the sink.
    Steps are priced as the pass prices them (the docstring: the banded pass pays G for a pattern-only
    step); a banded GLOBAL source (x, 0) starts from row -1's x * G; the banded LOCAL walk runs through
    zero cells, so there the running score takes LOCAL's floor of 0 at every cell, as H does."""
    match, mismatch, g, ins = scores(al)
    p, t = _ints(p), _ints(t)
    x, y = (int(v) for v in result["source"])
    pat_only, text_only = (ins, g) if band is None else (g, ins)
    total = x * g if band is not None and al.type == G.NV_GLOBAL else 0
    floor = band is not None and al.type == G.NV_LOCAL
    inside = band is None or 0 <= x - y < band
    for op in reversed([int(v) for v in result["ops"]]):
        if op == SUB:
            sym = t[x] if x < len(t) else PAST_TEXT
            assert band is not None or x < len(t)
            total += match if sym == p[y] else mismatch
            x += 1; y += 1
        elif op == INS:
            total += pat_only
            y += 1
        else:
            assert op == DEL, op
            total += text_only
            x += 1
        if floor:
            total = max(total, 0)
        if band is not None:
            inside = inside and 1 <= y and 0 <= x - y < band
    assert (x, y) == tuple(int(v) for v in result["sink"]), ((x, y), result["sink"])
    return total if band is None else (total, inside)


def count_ties(al, p, t, band=None):
    """Cells on the walked path where a strict comparison decided: two of top, left and diagonal equal H."""
    return _pair(al, band, p, t)["ties"]


def tie_share(ties):
    return float((np.asarray(ties) > 0).mean())


# ---------------------------------------------------------------- schemes
TYPES = {"global": G.NV_GLOBAL, "local": G.NV_LOCAL, "semi": G.NV_SEMI_GLOBAL}
SCHEMES = {"sym": (2, -1, -1, -1), "asym": (2, -1, -2, -3), "asym2": (2, -3, -1, -4), "ed": None,
           "positive": (2, -3, 1, -1)}          # a gap that scores > 0 (deletion), LOCAL only
BANDS = (2, 3, 7, 8, 9, 15, 16, 17, 31, 32)


def aligner(scheme, type_):
    type_ = TYPES.get(type_, type_)
    s = SCHEMES[scheme]
    if s is None:
        return G.NvAligner(G.NV_ED, type_)
    return G.NvAligner(G.NV_SW, type_, match=s[0], mismatch=s[1], deletion=s[2], insertion=s[3])


# ---------------------------------------------------------------- input families, each a function of a seed
EDGE_LENS = (1, 7, 8, 9, 15, 16, 17, 24, 25)      # around the stripes of the full-DP pass
EDGE_TEXT_LENS = (1, 2, 8, 9, 31, 40)


def _u32(v):
    return np.asarray(list(v), np.uint32)


def _related(rng, m, n, top=4):
    """A pattern of m and a text of n symbols sharing a window, with a few substitutions and one gap."""
    t = rng.integers(0, top, n)
    p = rng.integers(0, top, m)
    w = min(m, n)
    sp, st = int(rng.integers(0, m - w + 1)), int(rng.integers(0, n - w + 1))
    p[sp:sp + w] = t[st:st + w]
    flip = rng.random(m) < 0.1
    p[flip] = rng.integers(0, top, int(flip.sum()))
    if w > 4 and rng.random() < 0.6:
        cut = int(rng.integers(sp + 1, sp + w - 1))
        p = np.concatenate([p[:cut], p[cut + 1:], rng.integers(0, top, 1)])
    return _u32(p), _u32(t)


def family_edges(seed):
    """54 pairs: every edge pattern length against every edge text length."""
    rng = np.random.default_rng(seed)
    pairs = [_related(rng, m, n) for m in EDGE_LENS for n in EDGE_TEXT_LENS]
    return [a for a, _ in pairs], [b for _, b in pairs]


def banded_edge_deltas(band):
    return (-1, 0, 1, band - 2, band - 1, band, band + 5)


def family_banded_edges(seed, band):
    """63 pairs: every edge pattern length with a text of M + d symbols, d around the band's width; the
    text holds the pattern at an offset inside the band where it is long enough.  d = -1 is skipped."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for m in EDGE_LENS:
        for d in banded_edge_deltas(band):
            n = max(m + d, 0)
            p = rng.integers(0, 4, m)
            t = rng.integers(0, 4, n)
            off = int(rng.integers(0, max(min(d, band - 1), 0) + 1))
            k = min(m, n - off)
            if k > 0:
                t[off:off + k] = p[:k]
                flip = rng.random(n) < 0.08
                t[flip] = rng.integers(0, 4, int(flip.sum()))
                if k > 5 and rng.random() < 0.5:          # drop one text symbol: a pattern-only step
                    cut = off + int(rng.integers(1, k - 1))
                    t = np.concatenate([t[:cut], t[cut + 1:], rng.integers(0, 4, 1)])
            pats.append(_u32(p)); texts.append(_u32(t))
    return pats, texts


def family_ties(seed, band=None):
    """Pairs whose walk crosses tied cells: homopolymers, period-2 and period-3 repeats, and a read against
    a window with one symbol inserted next to an equal one (the gap can sit on either side of the pair),
    patterns 4..40 (every length mod 4), texts no shorter than their pattern.  For the banded form the flanks stay inside the
    band, so that the read's diagonal and its one gap do."""
    rng = np.random.default_rng(seed)
    flank = 3 if band is None else min(3, band - 1)
    pats, texts = [], []
    for m in (4, 6, 7, 9, 14, 16, 17, 23, 31, 40):
        a, b, c = (int(v) for v in rng.choice(4, 3, replace=False))
        pats.append(_u32([a] * m)); texts.append(_u32([a] * (m + flank)))
        pats.append(_u32(([a, b] * m)[:m])); texts.append(_u32(([b, a] * (m + flank))[:m + flank]))
        pats.append(_u32(([a, b, c] * m)[:m])); texts.append(_u32(([a, b, c, c] * m)[:m + 2]))
        for _ in range(4):                               # a window of the read with a doubled symbol
            p = rng.integers(0, 4, m)
            at = int(rng.integers(0, m))
            t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, flank))), p[:at + 1], p[at:],
                                rng.integers(0, 4, int(rng.integers(0, flank)))])
            pats.append(_u32(p)); texts.append(_u32(t))
    return pats, texts


def family_symbols(seed, text_top=4):
    """N (code 4) in patterns; texts over 0 .. text_top - 1 (16 and 256: symbols >= 4 in 4-bit and 8-bit
    texts, where a text symbol 4 equals a pattern's N); an empty pattern, an empty text, both empty."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for m, n in ((5, 9), (8, 8), (9, 12), (16, 20), (17, 17), (25, 30), (12, 14), (3, 3)):
        p, t = _related(rng, m, n)
        p[int(rng.integers(0, m))] = 4
        if text_top > 4:
            hit = rng.random(len(t)) < 0.3
            t[hit] = rng.integers(4, text_top, int(hit.sum()))
            t[int(rng.integers(0, len(t)))] = 4
        pats.append(p); texts.append(t)
    for m, n in ((0, 6), (6, 0), (0, 0)):
        pats.append(_u32(rng.integers(0, 4, m))); texts.append(_u32(rng.integers(0, 4, n)))
    return pats, texts


def family_sink_ties(seed):
    """LOCAL maxima that tie across the two halves of a 16-column stripe: the pattern is u z v, the text
    v q u with |u| = |v| = k, so v scores its 2k (match 2) early in the text at column 2k + 1 > 8 and u the
    same late in the text at column k <= 8.  In report order (stripes of 16, then rows) u's cell is the
    last maximum; an order by stripes of 8 would keep v's.  k = 4 .. 7, and the same over two stripes
    (16 columns of filler first)."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for k in (4, 5, 6, 7):
        for lead in (0, 16):
            for _ in range(3):
                # u, z and the filler over {0, 1}, v and q over {2, 3}: u meets only the text's u, v only its v
                u, v = rng.integers(0, 2, k), rng.integers(2, 4, k)
                q = rng.integers(2, 4, int(rng.integers(1, 4)))
                pats.append(_u32(list(rng.integers(0, 2, lead)) + list(u) + [int(rng.integers(0, 2))] + list(v)))
                texts.append(_u32(list(v) + list(q) + list(u)))
    return pats, texts


FAMILY_SEEDS = {"edges": 0x51, "ties": 0x52, "symbols": 0x53, "banded_edges": 0x54, "sink_ties": 0x55}


def families(band=None):
    """name -> (pats, texts): the families of the full-DP tests, or of the banded tests at `band`."""
    out = {"ties": family_ties(FAMILY_SEEDS["ties"], band),
           "symbols": family_symbols(FAMILY_SEEDS["symbols"]),
           "symbols16": family_symbols(FAMILY_SEEDS["symbols"], 16),
           "symbols256": family_symbols(FAMILY_SEEDS["symbols"], 256)}
    if band is None:
        out["edges"] = family_edges(FAMILY_SEEDS["edges"])
        out["sink_ties"] = family_sink_ties(FAMILY_SEEDS["sink_ties"])
    else:
        out["edges"] = family_banded_edges(FAMILY_SEEDS["banded_edges"] + band, band)
    return out


def text_bits(name):
    """The narrowest text packing the GPU tests give a family."""
    return {"symbols16": 4, "symbols256": 8}.get(name, 2)


def block(n, band=None):
    """n pairs drawn round-robin from edges, ties and symbols: the batch-size cases (1, 63, 65, 257)."""
    f = families(band)
    pool = [(p, t) for name in ("ties", "edges", "symbols") for p, t in zip(*f[name])]
    return [pool[k % len(pool)][0] for k in range(n)], [pool[k % len(pool)][1] for k in range(n)]
