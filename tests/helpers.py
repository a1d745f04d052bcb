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
