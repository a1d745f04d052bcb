"""Plain-Python model of nvbio's alignment_score(aligner, pattern, text, min_score, sink) with a
BestSink under a TextBlockingTag aligner: the reference of the sink tests (test_nvbio_sinks_ref.py
pins it to the C oracle's scores, test_gpu_nvbio_sinks.py compares the kernels with it).

It fills the whole H matrix of a pair from the recurrences the oracle's header cites
(NvB/nvbio/alignment: gotoh/gotoh_inl.h:985-1110 and :60-88, sw/sw_inl.h:895-970 and :60-80,
ed/ed_utils.h:45-52) and then replays the reports in nvbio's order, applying BestSink's
`best <= h` (sink_inl.h:59-68) literally:
  LOCAL        gotoh_inl.h:1075-1092 / sw_inl.h:949-966: per text stripe of BAND_LEN columns, per
               pattern row, the stripe's columns (those <= N), at (block + j, i + 1)
  SEMI_GLOBAL  gotoh_inl.h:1224-1229, :1403-1411 / sw_inl.h:1132-1137, :1192-1200: per stripe, the
               last row's columns (<= N), at (block + j, M)
  GLOBAL       gotoh_inl.h:1412-1420 / sw_inl.h:1201-1209: the column N, at (N, M)
BAND_LEN is the aligner's: 8 for Gotoh (gotoh_bandlen_selector, gotoh_inl.h:1492-1495: 8u / DIM,
DIM = 1), 16 for Smith-Waterman (sw_bandlen_selector, sw_inl.h:1330-1334: 16u / DIM; the score
dispatch instantiates it at sw_inl.h:1397) and for edit distance, which takes Smith-Waterman's
selector (ed_inl.h:95).
No order key and no arithmetic on positions: the walk is the definition.

The walk has two knobs that only the tests turn (rival()): another stripe width, and GASAL2's
`best < h` (the first maximum).  They answer "what would a wrong order have given", which is how
test_nvbio_sinks_ref.py checks that the inputs tell report orders apart.  pair() and batch()
always walk in nvbio's order."""
import functools
import re

import numpy as np

import gasal_ffi as G

INT32_MIN = -2 ** 31
NO_SINK = 0xFFFFFFFF
NEG = -(1 << 40)     # the infimum: never wins
ROW_MAJOR = 0        # rival(): one stripe over the whole text


def stripe(al):
    """Columns per text stripe of the TextBlockingTag scorer: the aligner's BAND_LEN (docstring)."""
    return 8 if al.aligner == G.NV_GOTOH else 16


def scheme(al):
    """(gotoh, match, mismatch, go, ge, deletion, insertion) of a gasal_ffi.NvAligner."""
    if al.aligner == G.NV_ED:
        return False, 0, -1, 0, 0, -1, -1
    return al.aligner == G.NV_GOTOH, al.match, al.mismatch, al.gap_open, al.gap_ext, al.deletion, al.insertion


def dp_matrix(al, p, t):
    """(top, H): top[c] = H(-1, c), the row above the pattern; H[i][c] for 0 <= i < M, 0 <= c < N."""
    gotoh, match, mismatch, go, ge, dele, ins = scheme(al)
    local, glob = al.type == G.NV_LOCAL, al.type == G.NV_GLOBAL
    M, N = len(p), len(t)
    if gotoh:
        top = [(go + ge * c) if glob else 0 for c in range(N)]
        left = [0 if local else go + ge * i for i in range(M)]
    else:
        top = [dele * (c + 1) if glob else 0 for c in range(N)]
        left = [0 if local else ins * (i + 1) for i in range(M)]
    H = []
    up, upF = top, [NEG] * N
    for i in range(M):
        row, rowF = [0] * N, [NEG] * N
        h_left = left[i]                       # H(i, c - 1)
        diag = left[i - 1] if i else 0         # H(i - 1, c - 1); H(-1, -1) = 0
        e = 0 if local else NEG                # E(i, -1) (Gotoh)
        pi = p[i]
        for c in range(N):
            s = match if pi == t[c] else mismatch
            if gotoh:
                f = max(upF[c] + ge, up[c] + go)
                e = max(e + ge, h_left + go)
                rowF[c] = f
                h = max(e, f, diag + s)
            else:
                h = max(up[c] + ins, h_left + dele, diag + s)
            if local:
                h = max(h, 0)
            diag = up[c]
            row[c] = h_left = h
        H.append(row)
        up, upF = row, rowF
    return top, H


def best_sink(type_, top, H, N, stripe, first=False):
    """BestSink after nvbio's reports in text stripes of `stripe` columns: (score, x, y, n_max)
    with n_max the number of reported cells that hold the score (more than one: the tie rule
    decided the sink).  first=True is not nvbio: it keeps the first maximum (`best < h`)."""
    M = len(H)
    best, sink = INT32_MIN, (NO_SINK, NO_SINK)
    reported = []

    def report(h, x, y):
        nonlocal best, sink
        reported.append(h)
        if best < h or (best == h and not first):
            best, sink = h, (x, y)

    last_row = H[M - 1] if M else top
    for block in range(0, N, stripe):
        cols = range(block, min(block + stripe, N))
        if type_ == G.NV_LOCAL:
            for i in range(M):
                for c in cols:
                    report(H[i][c], c + 1, i + 1)
        elif type_ == G.NV_SEMI_GLOBAL:
            for c in cols:
                report(last_row[c], c + 1, M)
        else:
            for c in cols:
                if c + 1 == N:
                    report(last_row[c], c + 1, M)
    return best, sink[0], sink[1], sum(1 for h in reported if h == best)


def _key(al):
    return (al.aligner, al.type, al.match, al.mismatch, al.gap_open, al.gap_ext, al.deletion, al.insertion)


_cache = {}      # (aligner, pattern, text, stripe, first) -> best_sink(): every input of the answer is in the key
_matrices = {}   # (aligner, pattern, text) -> dp_matrix(), read only


def _walk(al, p, t, width, first):
    k = (_key(al), bytes(np.asarray(p, np.uint8)), bytes(np.asarray(t, np.uint8)))
    if k + (width, first) not in _cache:
        if k not in _matrices:
            _matrices[k] = dp_matrix(al, [int(v) for v in p], [int(v) for v in t])
        top, H = _matrices[k]
        _cache[k + (width, first)] = best_sink(al.type, top, H, len(t), width or max(len(t), 1), first)
    return _cache[k + (width, first)]


def pair(al, p, t):
    """(score, x, y, n_max) of one pair; cached, so tests that share inputs share the reference."""
    return _walk(al, p, t, stripe(al), False)


def rival(al, p, t, stripe, first=False):
    """What another report order would have answered, for the tests of the inputs: stripes of
    `stripe` columns (ROW_MAJOR: one stripe), the first maximum when `first`."""
    return _walk(al, p, t, stripe, first)


def batch(al, pats, texts):
    """scores int32[n], sinks uint32[n, 2], n_max int64[n]; texts: one per pattern, or one shared."""
    if len(texts) == 1 and len(pats) != 1:
        texts = list(texts) * len(pats)
    r = [pair(al, p, t) for p, t in zip(pats, texts)]
    return (np.array([v[0] for v in r], np.int32), np.array([[v[1], v[2]] for v in r], np.uint32).reshape(-1, 2),
            np.array([v[3] for v in r], np.int64))


# ---- the inputs both test modules use ----
GOTOH = G.NvAligner(G.NV_GOTOH, 0, 2, -1, -2, -1)
SW = G.NvAligner(G.NV_SW, 0, 2, -3, 0, 0, -2, -3)
ED = G.NvAligner(G.NV_ED, 0)
BASES = {"gotoh": GOTOH, "sw": SW, "ed": ED}
TYPES = {"global": G.NV_GLOBAL, "local": G.NV_LOCAL, "semi": G.NV_SEMI_GLOBAL}
TEXT_LENS = (1, 7, 8, 9, 16, 17, 301)


def aligner(base, type_):
    b = BASES[base] if isinstance(base, str) else base
    return G.NvAligner(b.aligner, TYPES[type_] if isinstance(type_, str) else type_, b.match, b.mismatch, b.gap_open,
                       b.gap_ext, b.deletion, b.insertion)


def _u32(seq):
    return np.asarray(list(seq), np.uint32)


def tie_families(m, rng):
    """Pairs built to tie, for a pattern of m symbols (2-bit codes): a homopolymer pattern in a
    longer homopolymer text (the maximum on row M in every column >= M, over several stripes),
    period-2 repeats, and a pattern that occurs twice in the text, 8k and 8k + 3 apart."""
    out = []
    a, b = (int(v) for v in rng.choice(4, 2, replace=False))
    out.append((_u32([a] * m), _u32([a] * (m + 19))))
    out.append((_u32([a, b] * (m // 2) + [a] * (m % 2)), _u32(([a, b] * (m + 20))[:m + 37])))
    p = rng.integers(0, 4, m)
    c = 3 - int(p[-1])                                    # filler that does not extend the match
    for gap in (8 * (1 + m // 8) - m, 8 * (1 + m // 8) - m + 3):   # starts 8k and 8k + 3 apart
        out.append((_u32(p), _u32([c] * 2 + list(p) + [c] * gap + list(p) + [c] * 2)))
    return out


def edge_batch(pattern_lens, seed, text_lens=TEXT_LENS, ties=True):
    """Per-pair inputs: every pattern length against every text length, as a text-derived pattern
    (a few substitutions) and, when ties, the tie families."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for im, m in enumerate(pattern_lens):
        for it, n in enumerate(text_lens):
            a, b = (int(v) for v in rng.choice(4, 2, replace=False))
            if (im + it) % 3 == 1:       # homopolymers and period-2 repeats at every length: they tie
                pats.append(_u32([a] * m)); texts.append(_u32([a] * n))
                continue
            if (im + it) % 3 == 2:
                pats.append(_u32(([a, b] * m)[:m])); texts.append(_u32(([b, a] * n)[:n]))
                continue
            t = rng.integers(0, 4, n)
            if n > m:
                st = int(rng.integers(0, n - m + 1))
                p = t[st:st + m].copy()
                p[rng.random(m) < 0.05] = 0
            else:
                p = rng.integers(0, 4, m)
            pats.append(_u32(p)); texts.append(_u32(t))
        if ties:
            for p, t in tie_families(m, rng):
                pats.append(p); texts.append(t)
    return pats, texts


def shared_batch(pattern_lens, n_text, seed):
    """One shared text: a period-2 repeat, a homopolymer run and a random part, so that patterns
    cut from it (and homopolymer patterns) tie along the text."""
    rng = np.random.default_rng(seed)
    a, b = (int(v) for v in rng.choice(4, 2, replace=False))
    third = n_text // 3
    text = _u32([a, b] * (third // 2) + [a] * third + list(rng.integers(0, 4, n_text - third - 2 * (third // 2))))
    pats = []
    for m in pattern_lens:
        m = min(m, n_text)
        for st in (0, 1, third + 3, int(rng.integers(0, n_text - m + 1))):
            st = min(st, n_text - m)
            pats.append(text[st:st + m].copy())
        pats.append(_u32([a] * m))
        pats.append(_u32(rng.integers(0, 4, m)))
    return pats, [text]


@functools.lru_cache(maxsize=None)
def packed(kind, lens, seed, text_bits=2, text_big=False, n_text=0, text_lens=TEXT_LENS):
    """(pats, texts, P, T) of edge_batch / shared_batch, packed: patterns 4-bit big-endian (nvbio's
    reads), texts as asked."""
    if kind == "shared":
        pats, texts = shared_batch(lens, n_text, seed)
        T = G.PackedSet.pack(texts, bits=text_bits, big_endian=text_big, shared=True)
    else:
        pats, texts = edge_batch(lens, seed, text_lens)
        T = G.PackedSet.pack(texts, bits=text_bits, big_endian=text_big)
    return pats, texts, G.PackedSet.pack(pats, bits=4, big_endian=True), T


# ---- crossed ties: inputs whose sink depends on the report order ----
# The pattern is U + V (L symbols each, U over {0, 1}, V over {2, 3}); the text holds V ending at
# one-based column c1 and, further right, U ending at c2.  Every V symbol of the text lies left
# of every U symbol, so no alignment gains from both parts, and a part alone gives at most L
# matches: the maximum L * match is held by exactly the cells (c1, 2L) -- left and low -- and
# (c2, L) -- right and high.  Inside one stripe the lower row is reported later and (c1, 2L)
# wins; with a stripe boundary between the columns the later stripe and (c2, L) win.  So the
# winner changes with the stripe width exactly when a boundary of one width and not of the other
# lies between the two columns, and always with the first-or-last rule.
CROSS_WAYS = ("one 8-stripe", "two 8-stripes of one 16-stripe", "two 16-stripes of one 32-stripe", "two 32-stripes")
CROSS_TAILS = (0, 1, 9)      # text lengths c2, c2 + 1, c2 + 9: the last stripe partial and full
CROSS_MAX_TEXT = 64
CROSS_LEADS = (0, 3, 9, 12)  # filler columns before the nest of crossed_shared: shifts it across the stripes


def cross_way(a, b):
    """Which of CROSS_WAYS the zero-based columns a < b fall in."""
    return 0 if a // 8 == b // 8 else 1 if a // 16 == b // 16 else 2 if a // 32 == b // 32 else 3


def _maxima(al, p, t):
    _, H = dp_matrix(al, [int(v) for v in p], [int(v) for v in t])
    top = max(max(r) for r in H)
    return {(c + 1, i + 1) for i, r in enumerate(H) for c, h in enumerate(r) if h == top}


def crossed_pair(L, c1, c2, n, rng):
    """(pattern, text) with the LOCAL maxima at exactly (c1, 2L) and (c2, L) under both base
    schemes, for c1 >= L, c2 >= c1 + L, n >= c2.  The fillers never extend a copy: left of V the
    other symbol of V's alphabet than V[0], right of it the other symbol of U's than U[-1] (it
    differs from V[0], and the symbol before V from U[-1])."""
    assert L <= c1 and c1 + L <= c2 <= n
    for _ in range(64):
        U, V = [int(v) for v in rng.integers(0, 2, L)], [int(v) for v in 2 + rng.integers(0, 2, L)]
        fa, fb = 5 - V[0], 1 - U[-1]
        p, t = _u32(U + V), _u32([fa] * (c1 - L) + V + [fb] * (c2 - L - c1) + U + [fb] * (n - c2))
        if all(_maxima(aligner(b, "local"), p, t) == {(c1, 2 * L), (c2, L)} for b in ("sw", "gotoh")):
            return p, t
    raise AssertionError(("no crossed pair", L, c1, c2, n))


def crossed_ties(L, columns, rng):
    """Crossed pairs for every (c1, c2) of `columns` at the text lengths c2 + CROSS_TAILS."""
    out = [crossed_pair(L, c1, c2, c2 + tail, rng) for c1, c2 in columns for tail in CROSS_TAILS]
    return [p for p, _ in out], [t for _, t in out]


def crossed_columns(L, per_way, rng):
    """Up to per_way (c1, c2) per way of CROSS_WAYS that L allows (c2 - c1 >= L), texts within
    CROSS_MAX_TEXT; in one 8-stripe, at least three of four straddle a 4 boundary too."""
    cols = []
    for way in range(4):
        cand = [(a, b) for a in range(L - 1, CROSS_MAX_TEXT) for b in range(a + L, CROSS_MAX_TEXT - max(CROSS_TAILS))
                if cross_way(a, b) == way]
        if way == 0:
            split = [ab for ab in cand if ab[0] // 4 != ab[1] // 4]
            same = [ab for ab in cand if ab[0] // 4 == ab[1] // 4]
            pick = [split[i] for i in rng.choice(len(split), min(per_way - 1, len(split)), replace=False)] if split else []
            pick += [same[int(rng.integers(len(same)))]] if same else []
        else:
            pick = [cand[i] for i in rng.choice(len(cand), min(per_way, len(cand)), replace=False)] if cand else []
        cols += [(a + 1, b + 1) for a, b in pick]
    return cols


def twice_pair(L, lead, gap, tail, rng):
    """A text that holds the whole pattern U + V twice: the last row's maximum in two columns
    (SEMI_GLOBAL: first against last), and two LOCAL maxima on row 2L."""
    U, V = [int(v) for v in rng.integers(0, 2, L)], [int(v) for v in 2 + rng.integers(0, 2, L)]
    f = 1 - U[0]                                    # before a copy: does not continue V, does not start U
    return _u32(U + V), _u32([f] * lead + U + V + [f] * gap + U + V + [f] * tail)


def _alternate(base, pats, texts):
    """Neighbouring pairs with different winners: low (y = M), high, low, ... under the base's
    LOCAL order (edit distance: Smith-Waterman's, whose stripes it has); what is left over of the
    larger class goes last.  An odd batch: the last lane of the packed kernel holds one pair."""
    al = aligner("sw" if base == "ed" else base, "local")
    low = [k for k in range(len(pats)) if pair(al, pats[k], texts[k])[2] == len(pats[k])]
    high = [k for k in range(len(pats)) if k not in set(low)]
    order = [k for ab in zip(low, high) for k in ab] + low[len(high):] + high[len(low):]
    if len(order) % 2 == 0:
        order.append(order[1])
    return [pats[k] for k in order], [texts[k] for k in order]


@functools.lru_cache(maxsize=None)
def crossed_batch(base, Ls, seed=0xC7):
    """The crossed-tie batch of the sink tests, per-pair texts: for every L of Ls four column
    pairs per way of CROSS_WAYS at three text lengths, and four texts that hold the pattern
    twice; ordered by _alternate."""
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for L in Ls:
        p, t = crossed_ties(L, crossed_columns(L, 4, rng), rng)
        pats += p; texts += t
        for lead, gap, tail in ((0, 1, 0), (2, 3, 1), (1, 8, 9), (3, 0, 2)):
            p, t = twice_pair(L, lead, gap, tail, rng)
            pats.append(p); texts.append(t)
    return _alternate(base, pats, texts)


@functools.lru_cache(maxsize=None)
def crossed_shared(L, lead, seed=0xC8):
    """One shared text, V copies then U copies, nested: V_1 .. V_K U_K .. U_1 after `lead` filler
    columns (K = 3 words of L <= 4 symbols, else 2), and the patterns U_k + V_k cut from it.  Every
    V symbol lies left of every U symbol, as in crossed_pair, and the words are drawn until every
    pattern holds its maximum at the end of its own V and U and nowhere else under both base
    schemes: pattern k's columns are 2 (K - k) (L + 1) + L + 1 apart."""
    rng = np.random.default_rng(seed)
    K = 3 if L <= 4 else 2
    for _ in range(2000):
        words = [([int(v) for v in rng.integers(0, 2, L)], [int(v) for v in 2 + rng.integers(0, 2, L)]) for _ in range(K)]
        text, ends = [3] * lead, []
        for U, V in words:
            text += V + [5 - V[0]]
            ends.append([len(text) - 1])
        for k in reversed(range(K)):
            text += [1 - words[k][0][-1]] + words[k][0]
            ends[k].append(len(text))
        text += [1 - words[0][0][-1]] * 2
        pats = [_u32(U + V) for U, V in words]
        if all(_maxima(aligner(b, "local"), p, text) == {(e[0], 2 * L), (e[1], L)}
               for b in ("sw", "gotoh") for p, e in zip(pats, ends)):
            return pats, [_u32(text)]
    raise AssertionError(("no crossed shared text", L, lead))


def planned_rows(al, max_pattern, max_text, per_pair=True, text_bits=2):
    """R of the sink kernel planned for these bounds (rows per lane, from the plan's name)."""
    name = G.nv_describe_sinks_plan(al, max_pattern, max_text, per_pair_texts=per_pair, text_bits=text_bits)
    return int(re.search(r"_G\d+R(\d+)_sink$", name).group(1))


def crossed_lens(al, per_pair=True):
    """L of the crossed batches: 3, R and R + 1 of the shape planned for their own bounds (patterns
    of 2 (R + 1) rows), so that the tied rows L - 1 and 2L - 1 sit on one lane, on the last rows
    of two lanes, and on either side of a lane edge."""
    r = planned_rows(al, 1, CROSS_MAX_TEXT, per_pair)
    assert planned_rows(al, 2 * (r + 1), CROSS_MAX_TEXT, per_pair) == r
    return 3, r, r + 1
