"""Plain-Python model of nvbio's alignment_score(aligner, pattern, text, min_score, sink) with a
BestSink under a TextBlockingTag aligner: the reference of the sink tests (test_nvbio_sinks_ref.py
pins it to the C oracle's scores, test_gpu_nvbio_sinks.py compares the kernels with it).

It fills the whole H matrix of a pair from the recurrences the oracle's header cites
(NvB/nvbio/alignment: gotoh/gotoh_inl.h:985-1110 and :60-88, sw/sw_inl.h:895-970 and :60-80,
ed/ed_utils.h:45-52) and then replays the reports in nvbio's order, applying BestSink's
`best <= h` (sink_inl.h:59-68) literally:
  LOCAL        gotoh_inl.h:1075-1092 / sw_inl.h:949-966: per text stripe of 8 columns, per pattern
               row, the stripe's columns (those <= N), at (block + j, i + 1)
  SEMI_GLOBAL  gotoh_inl.h:1224-1229, :1403-1411 / sw_inl.h:1132-1137, :1192-1200: per stripe, the
               last row's columns (<= N), at (block + j, M)
  GLOBAL       gotoh_inl.h:1412-1420 / sw_inl.h:1201-1209: the column N, at (N, M)
No order key and no arithmetic on positions: the walk is the definition."""
import functools

import numpy as np

import gasal_ffi as G

INT32_MIN = -2 ** 31
NO_SINK = 0xFFFFFFFF
NEG = -(1 << 40)     # the infimum: never wins
STRIPE = 8


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


def best_sink(type_, top, H, N):
    """BestSink after nvbio's reports: (score, x, y, n_max) with n_max the number of reported
    cells that hold the score (more than one: the tie rule decided the sink)."""
    M = len(H)
    best, sink = INT32_MIN, (NO_SINK, NO_SINK)
    reported = []

    def report(h, x, y):
        nonlocal best, sink
        reported.append(h)
        if best <= h:
            best, sink = h, (x, y)

    last_row = H[M - 1] if M else top
    for block in range(0, N, STRIPE):
        cols = range(block, min(block + STRIPE, N))
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


_cache = {}


def pair(al, p, t):
    """(score, x, y, n_max) of one pair; cached, so tests that share inputs share the reference."""
    k = (_key(al), bytes(np.asarray(p, np.uint8)), bytes(np.asarray(t, np.uint8)))
    if k not in _cache:
        top, H = dp_matrix(al, [int(v) for v in p], [int(v) for v in t])
        _cache[k] = best_sink(al.type, top, H, len(t))
    return _cache[k]


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
