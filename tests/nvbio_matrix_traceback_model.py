"""Plain-Python definition of the matrix-scored Gotoh traceback (gasalx_nv_matrix_traceback_*): nvbio's
BatchedAlignmentTraceback over a GotohAligner whose scheme answers substitution(i, j, r, q, qq) from a
table (NvB/nvbio/alignment/gotoh/gotoh_inl.h:534): S(p, t) = mat[t + p * n] with t the text symbol and
p the pattern symbol, both read as n - 1 when they are >= n (nvbio_matrix_model's table and clamp).

It restates the PatternBlockingTag pass and the walk (gotoh_inl.h:462-593 and :1806-1872, the first
row / column of alignment_inl.h:442-459; csrc/nvtrace.hpp and oracle/nvbio_oracle.c
orc_nv_traceback_one for the Simple schemes).  Rows i = text, columns j = pattern:
  F(i,j) = max(F(i-1,j) + Ge, H(i-1,j) + Go)    DEL_EXT when the extension is strictly greater
  E(i,j) = max(E(i,j-1) + Ge, H(i,j-1) + Go)    INS_EXT when the extension is strictly greater
  H(i,j) = max3(E, F, H(i-1,j-1) + S)            LOCAL: max(H, 0)
  hdir   = F > E ? (F > diag ? DEL : SUB) : (E > diag ? INS : SUB);  LOCAL and H == 0: SINK
  H(-1,j) = LOCAL ? 0 : Go + Ge*j,  F(-1,j) = infimum,  H(-1,-1) = 0
  H(i,-1) = GLOBAL ? Go + Ge*i : 0,  E(i,-1) = LOCAL ? 0 : infimum,  infimum = -32768 - min(Go, Ge)
BestSink keeps the last maximum (best <= h) in report order: LOCAL every cell, stripes of 8 pattern
columns, inside a stripe the text rows, inside a row the columns; SEMI_GLOBAL H(i, M-1) per row;
GLOBAL the cell (N, M).  The walk goes from the sink through the H / E / F states, pushing
0 SUBSTITUTION, 1 INSERTION (a pattern symbol), 2 DELETION (a text symbol), and ends with the
first-row (INSERTIONs, not LOCAL) and first-column (DELETIONs, GLOBAL) tails.  A pair with an empty
string reports nothing: INT32_MIN, sources and sinks 0xFFFFFFFF, no pushes.

replay() walks the pushes back over the strings and returns the score of the alignment they spell,
a run of L equal gap ops costing Go + Ge * (L - 1).  That equals the DP score only for Ge >= Go: the
walk leaves the E (or F) state wherever the extension did not strictly beat a fresh opening and may
re-enter it at the next cell, so it can spell one run of L gaps whose DP cost was paid as two
openings; with Ge < Go that is the cheaper reading and the run-length cost overcharges, with
Ge >= Go merging runs never costs more and the optimum cannot cost less.  Every test uses Ge >= Go.
"""
import numpy as np

import gasal_ffi as G
import nvbio_matrix_model as M

INT32_MIN = -2 ** 31
NO_CELL = 0xFFFFFFFF
STRIPE = 8
SUB, INS, DEL, SNK, INS_EXT, DEL_EXT = 0, 1, 2, 3, 4, 8


def fill(al, mat, n, p, t):
    """(H, flags, best, (bx, by)): H[i][j] and flags[i][j] for text row i and pattern column j (both
    zero-based), the BestSink score and its one-based (x = text, y = pattern) cell."""
    local, glob, semi = al.type == G.NV_LOCAL, al.type == G.NV_GLOBAL, al.type == G.NV_SEMI_GLOBAL
    go, ge = al.gap_open, al.gap_ext
    inf = -32768 - min(go, ge)
    Mp, N = len(p), len(t)
    p = [min(int(v), n - 1) for v in p]
    t = [min(int(v), n - 1) for v in t]
    H = [[0] * Mp for _ in range(N)]
    flags = [[0] * Mp for _ in range(N)]
    # the column left of the stripe: H(i, c0 - 1), E(i, c0 - 1)
    leftH = [(go + ge * i) if glob else 0 for i in range(N)]
    leftE = [0 if local else inf for _ in range(N)]
    best, bx, by = INT32_MIN, NO_CELL, NO_CELL
    last_h = 0
    for c0 in range(0, Mp, STRIPE):
        cols = range(c0, min(c0 + STRIPE, Mp))
        upH = {j: (0 if local else go + ge * j) for j in cols}      # H(-1, j)
        upF = {j: inf for j in cols}
        corner = 0 if (local or c0 == 0) else go + ge * (c0 - 1)     # H(-1, c0 - 1)
        for i in range(N):
            diag, h_left, e = corner, leftH[i], leftE[i]
            corner = leftH[i]
            for j in cols:
                s = mat[t[i] + p[j] * n]
                ftop, htop = upF[j] + ge, upH[j] + go
                f = max(ftop, htop)
                eleft, hleft = e + ge, h_left + go
                e = max(eleft, hleft)
                d = diag + s
                h = max(e, f, d)
                if local:
                    h = max(h, 0)
                hdir = (DEL if f > d else SUB) if f > e else (INS if e > d else SUB)
                flags[i][j] = (SNK if local and h == 0 else hdir) | (INS_EXT if eleft > hleft else 0) | \
                              (DEL_EXT if ftop > htop else 0)
                diag = upH[j]
                upH[j], upF[j] = h, f
                H[i][j] = h_left = h
                if local and best <= h:
                    best, bx, by = h, i + 1, j + 1
                if j == Mp - 1:
                    last_h = h
            leftH[i], leftE[i] = h_left, e
            if semi and c0 + STRIPE >= Mp and best <= last_h:
                best, bx, by = last_h, i + 1, Mp
    if glob:
        best, bx, by = last_h, N, Mp
    return H, flags, best, (bx, by)


def walk(type_, flags, sink):
    """(ops, source, path): the pushes from `sink`, the source (x, y), and the (row, column, state)
    of every flag the walk read."""
    ops, path = [], []
    row, col, state = sink[0], sink[1] - 1, 0
    while row > 0 and col >= 0:
        op = flags[row - 1][col]
        h_op = op & 3
        if type_ == G.NV_LOCAL and state == 0 and h_op == SNK:
            break
        path.append((row - 1, col, state))
        if state == 1:
            if not op & INS_EXT:
                state = 0
            col -= 1; ops.append(INS)
        elif state == 2:
            if not op & DEL_EXT:
                state = 0
            row -= 1; ops.append(DEL)
        elif h_op == INS:
            state = 1
        elif h_op == DEL:
            state = 2
        else:
            col -= 1; row -= 1; ops.append(SUB)
    sx, sy = row, col + 1
    if type_ != G.NV_LOCAL and sx == 0:
        ops += [INS] * sy
        sy = 0
    if type_ == G.NV_GLOBAL and sy == 0:
        ops += [DEL] * sx
        sx = 0
    return ops, (sx, sy), path


def count_ties(al, mat, n, p, t, H, path):
    """Cells on the walked path where the strict comparisons decided: two of (E, F, diag + S) tie for H,
    or an extension ties its opening (E + Ge == H + Go to the left, F + Ge == H + Go above)."""
    go, ge = al.gap_open, al.gap_ext
    local, glob = al.type == G.NV_LOCAL, al.type == G.NV_GLOBAL
    inf = -32768 - min(go, ge)
    p = [min(int(v), n - 1) for v in p]
    t = [min(int(v), n - 1) for v in t]
    N, Mp = len(t), len(p)
    # E and F of every cell, recomputed row by row (not stripe by stripe: the values are the same)
    E = [[0] * Mp for _ in range(N)]
    F = [[0] * Mp for _ in range(N)]
    hcell = lambda i, j: (0 if (i < 0 and j < 0) else ((0 if local else go + ge * j) if i < 0 else
                                                      (((go + ge * i) if glob else 0) if j < 0 else H[i][j])))
    for i in range(N):
        for j in range(Mp):
            E[i][j] = max((E[i][j - 1] if j else (0 if local else inf)) + ge, hcell(i, j - 1) + go)
            F[i][j] = max((F[i - 1][j] if i else inf) + ge, hcell(i - 1, j) + go)
    ties = 0
    for i, j, state in path:
        e, f, d = E[i][j], F[i][j], hcell(i - 1, j - 1) + mat[t[i] + p[j] * n]
        if state == 0:
            h = max(e, f, d)
            ties += (e == h) + (f == h) + (d == h) >= 2
        elif state == 1:
            ties += (E[i][j - 1] if j else (0 if local else inf)) + ge == hcell(i, j - 1) + go
        else:
            ties += (F[i - 1][j] if i else inf) + ge == hcell(i - 1, j) + go
    return ties


_cache = {}


def pair(al, mat, n, p, t):
    """dict(score, source, sink, ops, ties) of one pair; cached on (type, gaps, table, strings)."""
    m = M.flat(mat, n)
    k = (al.type, al.gap_open, al.gap_ext, n, tuple(m), bytes(np.asarray(p, np.uint8)), bytes(np.asarray(t, np.uint8)))
    if k not in _cache:
        if len(p) == 0 or len(t) == 0:
            _cache[k] = dict(score=INT32_MIN, source=(NO_CELL, NO_CELL), sink=(NO_CELL, NO_CELL), ops=[], ties=0)
        else:
            H, flags, best, sink = fill(al, m, n, p, t)
            ops, source, path = walk(al.type, flags, sink)
            _cache[k] = dict(score=best, source=source, sink=sink, ops=ops,
                             ties=count_ties(al, m, n, p, t, H, path))
    return _cache[k]


def batch(al, mat, n, pats, texts):
    """The dict oracle.nv_traceback returns (score int32[k], source and sink uint32[k, 2], ops: a list of
    uint8 arrays), with ties int64[k]; texts: one per pattern, or one shared."""
    if len(texts) == 1 and len(pats) != 1:
        texts = list(texts) * len(pats)
    r = [pair(al, mat, n, p, t) for p, t in zip(pats, texts)]
    return dict(score=np.array([v["score"] for v in r], np.int32),
                source=np.array([v["source"] for v in r], np.uint32).reshape(-1, 2),
                sink=np.array([v["sink"] for v in r], np.uint32).reshape(-1, 2),
                ops=[np.array(v["ops"], np.uint8) for v in r],
                ties=np.array([v["ties"] for v in r], np.int64))


def replay(al, mat, n, p, t, result):
    """The score of the alignment `result` (dict(score, source, sink, ops) of one pair) spells over the
    strings, walking the pushes from the sink to the source; asserts that they consume exactly the
    pattern span source.y..sink.y and the text span source.x..sink.x."""
    m = M.flat(mat, n)
    go, ge = al.gap_open, al.gap_ext
    x, y = int(result["sink"][0]), int(result["sink"][1])
    total, prev = 0, SUB
    for op in (int(v) for v in result["ops"]):
        if op == SUB:
            x -= 1; y -= 1
            assert x >= 0 and y >= 0
            total += m[min(int(t[x]), n - 1) + min(int(p[y]), n - 1) * n]
        elif op == INS:
            y -= 1
            assert y >= 0
            total += ge if prev == INS else go
        else:
            assert op == DEL
            x -= 1
            assert x >= 0
            total += ge if prev == DEL else go
        prev = op
    assert (x, y) == (int(result["source"][0]), int(result["source"][1])), ((x, y), result["source"])
    return total


def one(res, k):
    """Pair k of a batch result as replay() takes it."""
    return dict(score=int(res["score"][k]), source=res["source"][k], sink=res["sink"][k], ops=res["ops"][k])


def same(got, want, what=""):
    """Bit for bit: score, source, sink, n_ops and every push."""
    n = len(want["score"])
    assert len(got["score"]) == n
    bad = [k for k in range(n)
           if got["score"][k] != want["score"][k] or not np.array_equal(got["source"][k], want["source"][k])
           or not np.array_equal(got["sink"][k], want["sink"][k]) or not np.array_equal(got["ops"][k], want["ops"][k])]
    if bad:
        k = bad[0]
        raise AssertionError(f"{what}: {len(bad)}/{n} differ, first #{k}: got {got['score'][k]} {got['source'][k]} "
                             f"{got['sink'][k]} {list(got['ops'][k])} want {want['score'][k]} {want['source'][k]} "
                             f"{want['sink'][k]} {list(want['ops'][k])}")


def tie_share(ties):
    """The share of pairs with a tied cell on their walked path."""
    return float((np.asarray(ties) > 0).mean())


def random_pairs(n_sym, lens, text_lens, seed, top=None):
    """Every pattern length against every text length: half the pairs a noisy copy of a text window (or
    a text a noisy copy of a pattern window), so that alignments are long and hold gaps."""
    rng = np.random.default_rng(seed)
    top = top or n_sym
    pats, texts = [], []
    for m in lens:
        for k in text_lens:
            t = rng.integers(0, top, k).astype(np.uint32)
            p = rng.integers(0, top, m).astype(np.uint32)
            if rng.random() < 0.7:
                w = min(m, k)
                sp, st = int(rng.integers(0, m - w + 1)), int(rng.integers(0, k - w + 1))
                p[sp:sp + w] = t[st:st + w]
                flip = rng.random(m) < 0.12
                p[flip] = rng.integers(0, top, int(flip.sum()))
                if w > 4 and rng.random() < 0.5:               # a gap: drop a few pattern symbols of the window
                    cut = int(rng.integers(sp + 1, sp + w - 1))
                    p = np.concatenate([p[:cut], p[cut + int(rng.integers(1, 3)):], rng.integers(0, top, 2)])[:m]
                    p = p.astype(np.uint32)
                    if len(p) < m:
                        p = np.concatenate([p, rng.integers(0, top, m - len(p)).astype(np.uint32)])
            pats.append(p); texts.append(t)
    return pats, texts


# the tie family of the GPU tests: entries -2..3 with Go = -3, Ge = -1 (few distinct values, cheap gaps)
TIE_GAPS = (-3, -1)


def tie_table(n, seed):
    """Random and asymmetric with few distinct values: E, F and the diagonal often tie under TIE_GAPS."""
    return M.random_table(n, seed, lo=-2, hi=3)


# ---- the input families of test_gpu_nvbio_matrix_traceback.py; test_nvbio_matrix_traceback_model.py
#      replays every pair of them on the CPU.  Each gives (aligner, table, n, pats, texts); Ge >= Go.
TYPES = {"global": G.NV_GLOBAL, "local": G.NV_LOCAL, "semi": G.NV_SEMI_GLOBAL}
EDGE_LENS = (1, 7, 8, 9, 16, 17, 63, 64, 65)       # the stripes of 8 pattern columns
EDGE_TEXT_LENS = (1, 8, 9, 33, 120)
# (n, pattern bits, pattern big-endian, text bits, text big-endian): test_gpu_nvbio_matrix.py's TABLES
PACKINGS = {"n24_8bit": (24, 8, False, 8, False), "n4_2bit_texts": (4, 4, True, 2, False),
            "n16_4bit": (16, 4, True, 4, True), "n32_8bit": (32, 8, False, 8, False)}


def family_edges(type_):
    """45 pairs: every stripe-edge pattern length against every text length, under the tie family."""
    pats, texts = random_pairs(24, EDGE_LENS, EDGE_TEXT_LENS, 0xA8)
    return M.gotoh(type_, *TIE_GAPS), tie_table(24, 0xA7), 24, pats, texts


def family_block(type_):
    """300 pairs: a full block of 256 threads and a part-filled one.  Long enough (patterns 24..65, texts
    24..90) that at least half of the pairs of every type walk through a tied cell
    (test_nvbio_matrix_traceback_model.py asserts the share)."""
    rng = np.random.default_rng(0xA9)
    lens, tlens = rng.integers(24, 66, 300), rng.integers(24, 91, 300)
    pats, texts = [], []
    for m, k in zip(lens, tlens):
        p, t = random_pairs(24, (int(m),), (int(k),), int(rng.integers(1 << 30)))
        pats += p; texts += t
    return M.gotoh(type_, *TIE_GAPS), tie_table(24, 0xA7), 24, pats, texts


def family_packing(type_, case):
    n = PACKINGS[case][0]
    pats, texts = random_pairs(n, (1, 9, 20, 33), (1, 8, 17, 60), 0xB0 + n)
    return M.gotoh(type_, -5, -3), M.random_table(n, 0xA5 + n), n, pats, texts


def family_positive(type_):
    """Entries 1..9; pattern lengths = 1..7 mod 8 (the last stripe has pad columns), mixed in one wave;
    GLOBAL and SEMI_GLOBAL take the first 16 pairs."""
    rng = np.random.default_rng(0xC1)
    mat = G.NvMatrix(rng.integers(1, 10, (24, 24)).astype(np.int8))
    lens = [8 * int(b) + int(r) for b, r in zip(rng.integers(0, 6, 45), rng.integers(1, 8, 45))]
    pats = [rng.integers(0, 24, m).astype(np.uint32) for m in lens]
    texts = [rng.integers(0, 24, int(k)).astype(np.uint32) for k in rng.integers(1, 101, 45)]
    k = 45 if TYPES.get(type_, type_) == G.NV_LOCAL else 16
    return M.gotoh(type_, -5, -3), mat, 24, pats[:k], texts[:k]


def family_clamp(type_):
    """n = 20 under strings that hold every byte value."""
    pats, texts = random_pairs(20, (1, 9, 20, 64), (1, 9, 17, 120), 0xD5, top=256)
    return M.gotoh(type_, -4, -2), M.random_table(20, 0xD4), 20, pats, texts


def family_chunks(type_):
    """61 pairs whose longest pattern and longest text lie in the last chunk of 7."""
    rng = np.random.default_rng(0xE7)
    pats = [rng.integers(0, 24, int(m)).astype(np.uint32) for m in rng.integers(1, 30, 61)]
    texts = [rng.integers(0, 24, int(k)).astype(np.uint32) for k in rng.integers(1, 50, 61)]
    pats[58] = rng.integers(0, 24, 37).astype(np.uint32)
    texts[59] = rng.integers(0, 24, 66).astype(np.uint32)
    pats[59] = texts[59][10:40].copy()
    return M.gotoh(type_, *TIE_GAPS), tie_table(24, 0xE8), 24, pats, texts


def family_device(type_):
    pats, texts = random_pairs(24, (1, 9, 20, 70), (8, 33, 90), 0xF5)
    return M.gotoh(type_, -5, -3), M.random_table(24, 0xF4), 24, pats, texts


def families():
    """name -> (aligner, table, n, pats, texts), every family above for every type it runs with."""
    out = {}
    for type_ in TYPES:
        for name, f in (("edges", family_edges), ("block", family_block), ("positive", family_positive),
                        ("clamp", family_clamp), ("chunks", family_chunks)):
            out[f"{name}-{type_}"] = f(type_)
        for case in PACKINGS:
            out[f"packing-{case}-{type_}"] = family_packing(type_, case)
    out["device-local"] = family_device("local")
    return out


# the strings of the comparison with the existing kernel (nvbio_sink_model.packed: 4-bit big-endian patterns,
# 2-bit texts, tie families included), under simple_table(4, match, mismatch) and nvbio_sink_model.GOTOH
SIMPLE_LENS = (1, 7, 8, 9, 17, 40)
SIMPLE_SEED = 0xE6
SIMPLE_SHARED_TEXT = 120
