"""Shared test helpers: fixture readers and random batch builders."""
from __future__ import annotations

import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def kat():
    with open(os.path.join(GOLDEN, "survey_kat.json")) as f:
        return json.load(f)


def read_fasta_pairs(limit=None):
    """The reference test_prog's 20K sample pairs (test_prog/{query,target}_batch.fasta.gz),
    read in lock step like test_prog.cpp:90-137; returns (queries, targets, q_mod, t_mod)."""
    starts = "></+"

    def records(path):
        out, mods, cur = [], [], None
        with gzip.open(path, "rt") as fh:
            for line in fh:
                line = line.rstrip("\n")
                if line and line[0] in starts:
                    if cur is not None:
                        out.append(cur)
                    mods.append(starts.index(line[0]))
                    cur = ""
                    if limit is not None and len(out) >= limit:
                        break
                elif cur is not None:
                    cur += line
        if cur is not None and (limit is None or len(out) < limit):
            out.append(cur)
        return out[:limit] if limit else out, mods[:limit] if limit else mods

    q, qm = records(os.path.join(GOLDEN, "query_batch.fasta.gz"))
    t, tm = records(os.path.join(GOLDEN, "target_batch.fasta.gz"))
    n = min(len(q), len(t))
    return q[:n], t[:n], qm[:n], tm[:n]


def read_pairhmm_dataset(path):
    """Synthetic PairHMM input (Non-CDP/PairHMM/Intra-task/Synthetic_data/dataset/*.txt),
    parsed as tile_1.cu:246-290: read len, read + base/ins/del/gcp quals, hap len, hap."""
    toks = open(path).read().split()
    pos = 0
    size = int(toks[pos]); pos += 1
    pairs = []
    for _ in range(size):
        rl = int(toks[pos]); pos += 1
        read = toks[pos]; pos += 1
        quals = []
        for _q in range(4):
            quals.append([int(x) for x in toks[pos:pos + rl]]); pos += rl
        hl = int(toks[pos]); pos += 1
        hap = toks[pos]; pos += 1
        pairs.append(dict(read=read, bq=quals[0], iq=quals[1], dq=quals[2], gcp=quals[3], hap=hap[:hl]))
    return pairs


BASES = np.frombuffer(b"ACGT", np.uint8)

# read lengths at the PairHMM lane-group boundaries (test_pairhmm_edge_lengths) and, per read
# length R, the haplotype lengths tried
HMM_READ_LENS = (1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256)


def hmm_hap_lens(R):
    return (1, 2, max(1, R - 1), R, R + 1, 500)


def hmm_insertion_bound(R, H):
    """True where no read of R rows can reach 1e-30 against a haplotype of H columns, whatever
    the qualities: at most H rows are match rows and each run of insertion rows opens once,
    after a match row, so at least R - 2H rows are insertion *extensions* at the model's
    constant 0.1; with c0 < 1.4e36 and fewer than R**(2H) paths the value stays below
    1.4e36 * R**(2H) * 0.1**(R-2H).  In the grid above: R >= 127 with H in (1, 2)."""
    return R - 2 * H >= 100


def hmm_args(pairs, params):
    """The ten pairhmm() arrays of a list of dict(read, hap, bq, iq, dq); params turns the
    three Phred arrays into (qm, delta, xiksi, alpha), e.g. oracle.pairhmm_params."""
    reads = b"".join(p["read"].encode() for p in pairs)
    haps = b"".join(p["hap"].encode() for p in pairs)
    rl = np.array([len(p["read"]) for p in pairs], np.uint32)
    hl = np.array([len(p["hap"]) for p in pairs], np.uint32)
    ro = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.uint32)
    ho = np.concatenate([[0], np.cumsum(hl)[:-1]]).astype(np.uint32)
    bq, iq, dq = (np.concatenate([p[k] for p in pairs]).astype(np.uint8) for k in ("bq", "iq", "dq"))
    qm, de, xi, al = params(bq, iq, dq)
    return (np.frombuffer(reads, np.uint8), ro, rl, qm, de, xi, al, np.frombuffer(haps, np.uint8), ho, hl)


def hmm_related_read(rng, hap, R, sub=0.02):
    """(hap * k)[:R] with about 2 % substitutions."""
    read = bytearray((hap * (R // len(hap) + 1))[:R].encode())
    for i in range(R):
        if rng.random() < sub:
            read[i] = b"ACGT"[int(rng.integers(0, 4))]
    return read.decode()


def hmm_related_grid(seed=0x64):
    """One related-read pair per (R, H) of the lane-boundary grid.  Insertion qualities stay
    at 10..25 so that a read one or two rows longer than the 64 insertion rows a short
    haplotype forces still ends above 1e-30 (each such row costs the constant 0.1)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for R in HMM_READ_LENS:
        for H in hmm_hap_lens(R):
            hap = random_seq(rng, H).decode()
            pairs.append(dict(read=hmm_related_read(rng, hap, R), hap=hap, bq=rng.integers(10, 41, R),
                              iq=rng.integers(10, 26, R), dq=rng.integers(10, 60, R)))
    return pairs


def hmm_unrelated(seed, read_lens, hap_lens=(64, 300)):
    """Random reads against random haplotypes with high base qualities: values far below 1."""
    rng = np.random.default_rng(seed)
    pairs = []
    for R in read_lens:
        for H in hap_lens:
            pairs.append(dict(read=random_seq(rng, R).decode(), hap=random_seq(rng, H).decode(),
                              bq=rng.integers(30, 60, R), iq=rng.integers(10, 60, R), dq=rng.integers(10, 60, R)))
    return pairs


def cigar_slots_kept(q_offsets, q_lens, n_ops):
    """a CIGAR longer than its pad8(ql)-byte slot runs into the slots after it.
    True for the pairs whose own CIGAR fits and whose slot no earlier pair overran."""
    off = np.asarray(q_offsets, np.int64)
    slot = (np.asarray(q_lens, np.int64) + 7) // 8 * 8
    ops = np.asarray(n_ops, np.int64)
    keep = np.ones(len(off), bool)
    reach = 0
    for k in np.argsort(off, kind="stable"):
        if off[k] < reach or ops[k] > slot[k]:
            keep[k] = False
        if ops[k] > slot[k]:
            reach = max(reach, off[k] + ops[k])
    return keep


def random_seq(rng, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, np.uint8)
    return bytes(a[rng.integers(0, len(a), n)])


def mutate(rng, s: bytes, sub=0.08, indel=0.02):
    out = bytearray()
    i = 0
    while i < len(s):
        u = rng.random()
        if u < indel / 2:
            out += random_seq(rng, int(rng.integers(1, 4)))
            out.append(s[i]); i += 1
        elif u < indel:
            i += int(rng.integers(1, 4))
        elif u < indel + sub:
            out += random_seq(rng, 1); i += 1
        else:
            out.append(s[i]); i += 1
    return bytes(out) if out else b"A"


def random_pairs(rng, n, qmin, qmax, tmin, tmax, related=0.7, alphabet=b"ACGT"):
    qs, ts = [], []
    for _ in range(n):
        ql = int(rng.integers(qmin, qmax + 1))
        q = random_seq(rng, ql, alphabet)
        if rng.random() < related:
            t = mutate(rng, q)
            tl = int(rng.integers(tmin, tmax + 1))
            t = (t + random_seq(rng, max(0, tl - len(t)), alphabet))[:tl]
        else:
            t = random_seq(rng, int(rng.integers(tmin, tmax + 1)), alphabet)
        qs.append(q); ts.append(t)
    return qs, ts


# ------------------------------------------------ reverse / complement ops ----
# query and target lengths of the edge batch: 1 to 5 words, odd and even word counts,
# len % 8 in {0, 1, 7}
OPS_EDGE_LENS = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33, 40)
# letters whose low nibble is a base's code (1, 3, 4, 7) without being A/C/G/T, with IUPAC
# letters of other codes beside them: the complement acts on nibbles, not on letters
OPS_ODD_ALPHABET = b"ACGTSWDQacgtswdqRYKM"
_NIB_COMP = {1: 4, 4: 1, 3: 7, 7: 3}
_BASE_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_BASE_COMP = bytes(_BASE_COMP[c] if c in b"ACGTacgt" else (c & 0xF0) | _NIB_COMP.get(c & 15, c & 15) for c in range(256))


def base_op(s: bytes, op: int) -> bytes:
    """Op code 0..3 on the bases alone (no slot, no pads): its own inverse."""
    if op & 1:
        s = s[::-1]
    if op & 2:
        s = s.translate(_BASE_COMP)
    return s


def _fit(rng, s, n, alphabet):
    return (s + random_seq(rng, max(0, n - len(s)), alphabet))[:n]


def ops_batch(kind, alphabet=b"ACGT", seed=0x0B5):
    """(queries, targets, q_ops, t_ops) for the reverse / complement tests.
    kind "edges": all 16 (q_op, t_op) combinations, 19 pairs each; per combination the first
      twelve pairs walk every query length of OPS_EDGE_LENS against a permutation of the
      target lengths, the rest draw both independently.
    kind "flagship": 300 pairs of 140..160 bases, ops uniform in 0..3.
    About half the pairs are related *after* their ops: the post-op query is drawn, mutated
    into the post-op target (10 % substitutions, a few indels), and the inverse op on the
    bases gives the inputs.  The slot reversal moves the pads to the front, so the kernels
    see these shifted by the pad count: still alignable, and far from the no-op answer."""
    rng = np.random.default_rng(seed + 977 * len(alphabet) + (0 if kind == "edges" else 1))
    L = OPS_EDGE_LENS
    shape = []
    if kind == "edges":
        for c in range(15, -1, -1):         # pair 0: ops (3, 3) on a one-word query at word 0
            for j in range(19):
                ql, tl = (L[j], L[(5 * j + c) % 12]) if j < 12 else (int(rng.choice(L)), int(rng.choice(L)))
                shape.append((c >> 2, c & 3, ql, tl))
    else:
        for _ in range(300):
            shape.append((int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(140, 161)),
                          int(rng.integers(140, 161))))
    qs, ts = [], []
    for k, (qo, to, ql, tl) in enumerate(shape):
        q = random_seq(rng, ql, alphabet)
        if k % 2 == 0:
            t = _fit(rng, mutate(rng, q, sub=0.10, indel=0.02), tl, alphabet)
        else:
            t = random_seq(rng, tl, alphabet)
        qs.append(base_op(q, qo)); ts.append(base_op(t, to))
    return qs, ts, np.array([s[0] for s in shape], np.uint8), np.array([s[1] for s in shape], np.uint8)


OPS_CASES = [("edges", b"ACGT"), ("edges", b"ACGTN"), ("edges", OPS_ODD_ALPHABET), ("flagship", b"ACGT"),
             ("flagship", b"ACGTN")]
OPS_SCORES = [(1, 4, 6, 1), (2, 3, 5, 2)]
_OPS_CASE = {}
_OPS_REF = {}


def ops_case(kind, alphabet):
    """One ops batch, built once per process: dict(qs, ts, b: the gasal_ffi.Batch, qo, to: the
    op arrays, ob: independent.apply_ops(b, qo, to), oq, ot: its sequences)."""
    import gasal_ffi as G
    import independent as I
    key = (kind, alphabet)
    if key not in _OPS_CASE:
        qs, ts, qo, to = ops_batch(kind, alphabet)
        b = G.Batch.from_pairs(qs, ts)
        ob = I.apply_ops(b, qo, to)
        oq, ot = I.op_sequences(ob)
        _OPS_CASE[key] = dict(qs=qs, ts=ts, b=b, qo=qo, to=to, ob=ob, oq=oq, ot=ot)
    return _OPS_CASE[key]


def ops_ref(kind, alphabet, name, fn):
    """fn(case) computed once per (batch, name) and shared by the tests that need it; the
    result is handed out as is and never written to."""
    key = (kind, alphabet, name)
    if key not in _OPS_REF:
        _OPS_REF[key] = fn(ops_case(kind, alphabet))
    return _OPS_REF[key]


def ops_dependence(case, sc=(1, 4, 6, 1)):
    """Per algorithm, the share of the pairs with a nonzero op whose independent answer on the
    op-transformed batch differs from the independent answer on the untouched batch (LOCAL and
    SEMI_GLOBAL: score and ends, GLOBAL: score).  A batch whose answers do not depend on its
    ops would pass with the ops ignored."""
    import independent as I
    b, ob = case["b"], case["ob"]
    has = (case["qo"] != 0) | (case["to"] != 0)
    out = {}
    for name, fn, fields in (("local", I.local, ("score", "q_end", "t_end")), ("global", I.global_, ("score",)),
                             ("semi", I.semi, ("score", "q_end", "t_end"))):
        r0 = fn(b, **dict(zip("aboe", sc)))
        r1 = fn(ob, **dict(zip("aboe", sc)))
        diff = np.zeros(b.n, bool)
        for f in fields:
            diff |= r0[f] != r1[f]
        out[name] = float(diff[has].mean())
    return out


# ------------------------------------------------------------------ KSW ----
def _unlike(rng, n, avoid):
    """n bases that never equal the base at the same position of `avoid` (cycled)."""
    out = bytearray()
    for k in range(n):
        c = avoid[k % len(avoid)] if avoid else 0
        out.append(random_seq(rng, 1, bytes(x for x in b"ACGT" if x != c))[0])
    return bytes(out)


def ksw_rule_batches(seed=0x155):
    """Constructed KSW batches, one per control-flow rule of ksw_kernel_template.h (rules K1-K3
    of tests/independent.py, the clip rule :188, seed 0, length 1).  name -> (queries, targets,
    seeds, scores).  Whether a rule fired is for the caller to assert, from independent.ksw's
    state=True counts."""
    rng = np.random.default_rng(seed)
    out = {}
    # K1 (:155): qlen a multiple of 8, a seed that dies after a few matching columns against an
    # unrelated tail, so rows are trimmed short of qlen.  The row's last cell is then an F
    # tail of the diagonal (diagonal - (o + e) - ...), which passes the clip rule only when
    # o + e < PEN_CLIP5: gap scores (2, 1), with (6, 1) pairs beside them
    qs, ts, sd = [], [], []
    for k in range(240):
        ql = 8 * int(rng.integers(1, 6))
        q = random_seq(rng, ql)
        p = int(rng.integers(1, 7))
        t = q[:p] + _unlike(rng, int(rng.integers(0, 12)), q[p:] + b"A")
        qs.append(q); ts.append(t); sd.append(int(rng.integers(1, 9)))
    out["line155"] = (qs, ts, sd, (1, 4, 2, 1))
    out["line155_oe7"] = (qs, ts, sd, (1, 4, 6, 1))
    # K2 (:159): a first target word of T against a query without T kills the seed inside the
    # word (m == 0 in row 1..3); the first-column value left in eh[0] revives the pair at row 8,
    # where the target goes on as the query itself and outgrows the seed
    qs, ts, sd = [], [], []
    for k in range(160):
        q = random_seq(rng, int(rng.integers(12, 41)), b"ACG")
        lead = 8 * int(rng.integers(1, 3))
        qs.append(q); ts.append(b"T" * lead + q[: int(rng.integers(1, len(q) + 1))]); sd.append(int(rng.integers(8, 22)))
    for k in range(40):                                       # and plain unrelated first words
        q = random_seq(rng, int(rng.integers(4, 30)))
        qs.append(q); ts.append(_unlike(rng, 8, q) + q); sd.append(int(rng.integers(0, 16)))
    out["tile_break"] = (qs, ts, sd, (1, 4, 6, 1))
    # K3 (:140): the main diagonal with two mismatches (-10) ties the diagonal four columns to
    # the right, entered through the first row's insertion of four (-(6 + 4)): q = XX + R[2:4] + R,
    # t = R with R of period 4; a query tail keeps the end of the query out of reach
    qs, ts, sd = [], [], []
    for k in range(120):
        unit = bytes(rng.permutation(np.frombuffer(b"ACGT", np.uint8)))
        R = unit * int(rng.integers(3, 8))
        xx = _unlike(rng, 2, unit)
        tail = bytes([b"ACGT"[(b"ACGT".index(unit[0]) + 1) % 4]]) * int(rng.integers(6, 14))
        qs.append(xx + unit[2:] + R + tail); ts.append(R); sd.append(int(rng.integers(11, 40)))
    out["tie"] = (qs, ts, sd, (1, 4, 6, 1))
    # the clip rule (:188): the best cell, then mismatches and matches down to the query's end:
    # max - gscore = 4 * x - y for x mismatches followed by y matches; 4, 5 and 6 among them
    qs, ts, sd = [], [], []
    for k in range(160):
        P = random_seq(rng, int(rng.integers(4, 24)))
        x, y = [(1, 0), (2, 3), (2, 2), (1, 0), (2, 3), (3, 7), (2, 4), (3, 6)][k % 8]
        mm = random_seq(rng, x)
        tailq = random_seq(rng, y)
        qs.append(P + mm + tailq); ts.append(P + _unlike(rng, x, mm) + tailq + random_seq(rng, int(rng.integers(0, 4))))
        sd.append(int(rng.integers(8, 30)))
    out["clip"] = (qs, ts, sd, (1, 4, 6, 1))
    # seed 0: every entry stays 0 (M = M ? M + s : 0), every word's first row ends its word
    qs, ts = random_pairs(rng, 80, 1, 40, 1, 40, related=1.0)
    out["seed0"] = (qs, ts, [0] * 80, (1, 4, 6, 1))
    # a single base on either side, on both, every seed around o + e
    qs, ts, sd = [], [], []
    for k in range(120):
        one = random_seq(rng, 1)
        other = random_seq(rng, int(rng.integers(1, 20)))
        if k % 3 == 0:
            other = one + other
        q, t = [(one, other), (other, one), (one, random_seq(rng, 1))][k % 3]
        qs.append(q); ts.append(t); sd.append(k % 20)
    out["length1"] = (qs, ts, sd, (1, 4, 6, 1))
    return out


def ksw_routing(qs, ts, seed, scores=(1, 4, 6, 1), env=None, npen=None):
    """Which KSW kernel form the dispatcher's documented rule (plan.cpp ksw16_ok, dispatch.hip
    run_ksw; ksw16.hpp header; gen_ksw_kernel) sends every pair of a batch to, from the inputs alone.
    Returns dict(taken: pairs ksw16 takes, level: the entry level 0/1/2 of the others' (and,
    for the taken ones, the level they would run), inst: the ksw16 instance 64 / 96 / 160 /
    0 = global entries / None = ksw16 off for the batch, tpb: threads per block of the LDS
    level 0, 0 = global entries, bound).  The tests assert on this so that a change of the
    rule fails them instead of moving them onto another kernel without notice."""
    env = env or {}
    a, b, o, e = scores
    ql = np.array([len(q) for q in qs], np.int64); tl = np.array([len(t) for t in ts], np.int64)
    seed = np.asarray(seed, np.int64)
    n = len(ql)
    step = max(a, -b, 0) if npen is None else max(a, -b, -npen, 0)
    bound = seed + step * np.minimum(ql, tl)
    if o < 0 or e < 0:
        bound = np.full(n, 1 << 62, np.int64)           # the negative-gap rule: int2 entries
    max_q = int(ql.max())
    k16 = env.get("GASALX_KSW16", "1") != "0" and o >= 0 and e >= 0 and o + e <= 0x300 and max_q <= 254
    ok = (bound <= 255) & (ql <= 254) & np.array([all(c in b"ACGT" for c in q) for q in qs])
    lane_ok = ok.copy()
    lane_ok[0:n - n % 2:2] &= ok[1:n:2]
    lane_ok[1:n:2] &= ok[0:n - n % 2:2]
    cols = (max_q + 3) & ~1
    inst = next((c for c in (64, 96, 160) if cols <= c), 0) if k16 else None
    lds_on = env.get("GASALX_KSW_LDS", "1" if n <= 4 * 1024 * 64 else "0") != "0"
    tpb = next((t for t in (256, 128, 64) if 2 * t * (max_q + 2) * 2 <= 160 * 1024), 0) if lds_on else 0
    return dict(taken=lane_ok & k16, level=np.where(bound <= 255, 0, np.where(bound <= 65535, 1, 2)),
                inst=inst, tpb=tpb, bound=bound, max_q=max_q)


def ksw_rule_fired(name, b, seed, r):
    """Whether the rule a constructed batch is named for decided at least one pair's answer,
    from the inputs and independent.ksw's own state (never from the oracle or the GPU)."""
    ql, tl = b.q_lens.astype(np.int64), b.t_lens.astype(np.int64)
    at_end = r["q_end"] == ql                           # the gscore branch was reported
    if name == "line155":
        # a row trimmed short of qlen took the gscore update and the answer is a gscore
        return int(((r["k1_rows"] > 0) & at_end & (ql % 8 == 0) & (r["score"] > 0)).sum())
    if name == "line155_oe7":
        return int(((r["k1_rows"] > 0) & (ql % 8 == 0)).sum())
    if name == "tile_break":
        # rows after the dead word were computed and carried the maximum past the seed
        return int(((r["k2_resumed"] > 0) & (r["score"] > seed) & (r["t_end"] > 8)).sum())
    if name == "tie":
        return int(((r["k3_ties"] > 0) & ~at_end).sum())
    if name == "clip":
        return min(int((r["margin"] == 5).sum()), int((r["margin"] == 4).sum()), int((r["margin"] == 6).sum()))
    if name == "seed0":
        return int(((seed == 0) & (r["score"] == 0) & (r["k2_resumed"] > 0)).sum())
    if name == "length1":
        return min(int((ql == 1).sum()), int((tl == 1).sum()), int(((ql == 1) & (tl == 1)).sum()))
    raise KeyError(name)
