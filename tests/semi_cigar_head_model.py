"""Independent model of gasalx_semi_cigar_head_* (TEST INFRASTRUCTURE ONLY): SEMI_GLOBAL with TAIL =
TARGET and any HEAD, with the alignment itself.  No reference output exists (the reference's
semi-global kernel has no traceback branch); this module restates the definition.  It generalises
tests/semi_cigar_model.py (HEAD = TARGET), whose docstring holds the cell, the N rule, the nibble and
the state machine; what changes here is the boundary and how the walk ends.

Boundaries, as the semi-global kernels hold them (semiglobal_kernel_template.h:87-99,123-128;
independent.semi is the authority for score and ends):
  left, HEAD QUERY / BOTH   H(r, -1) = 0 and E(r, -1) = 0, so E(r, 0) = -e: a deletion out of the free
                            boundary costs e, not o + e
  left, HEAD NONE / TARGET  H(r, -1) = 0 for r = 0, -(o + e*r) otherwise; E(r, 0) = H(r, -1) - OE
  top, HEAD TARGET / BOTH   H(-1, c) = 0 as the diagonal and as the value above; F(0, c) = -OE
  top, HEAD NONE / QUERY    above (0, c): -(o + e*c) (Q3: -o at c = 0); diagonal into (0, c): 0 for c = 0,
                            -(o + e*c) otherwise; F(0, c) = the value above - OE

Walk: from (ql - 1, t_end) in H state with the state machine of semi_cigar_model, until the row j or
the column i goes below 0.
  j < 0, i >= 0   HEAD TARGET / BOTH: the target bases left are free, t_start = i + 1.  HEAD NONE /
                  QUERY: they are the top boundary's deletions, D bytes of their own after the walk's
                  last run (runs of at most 63), t_start = 0.
  i < 0, j >= 0   HEAD QUERY / BOTH: rows 0..j are free, q_start = j + 1.  HEAD NONE / TARGET: they are
                  the left boundary's insertions, I bytes of their own, q_start = 0.
  both < 0        no ops added.
  otherwise       q_start = 0; t_start = the first target base consumed (i + 1), t_end + 1 when none is.
"""
from __future__ import annotations

import re

import numpy as np

import independent as I
import semi_cigar_model as M

NONE, QUERY, TARGET, BOTH = 0, 1, 2, 3
HEADS = (NONE, QUERY, TARGET, BOTH)
HEAD_NAME = {NONE: "none", QUERY: "query", TARGET: "target", BOTH: "both"}


def semi_cigar_head(batch, head, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None):
    """The dict of semi_cigar_model.semi_cigar for any HEAD, q_start filled."""
    assert o >= 0 and e >= 0, "outside the scores the call supports"
    head_q, head_t = head in (QUERY, BOTH), head in (TARGET, BOTH)
    q, _ = I._codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, _ = I._codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    q = q.astype(np.int64); t = t.astype(np.int64)
    n, R = q.shape
    T = t.shape[1]
    nval, OE = n_code & 15, o + e
    ql, tl = batch.q_lens.astype(np.int64), batch.t_lens.astype(np.int64)
    cols = np.arange(T, dtype=np.int64)

    def left(r):                                      # H(r, -1) as a column
        return np.full((n, 1), 0 if (r == 0 or head_q) else -(o + e * r), np.int64)

    if head_t:
        diag0 = np.zeros((n, T), np.int64)            # the diagonal into (0, c)
        above = np.zeros((n, T), np.int64)            # the value above (0, c)
    else:
        diag0 = np.broadcast_to(np.where(cols == 0, 0, -(o + e * cols)), (n, T)).astype(np.int64)
        above = np.broadcast_to(-(o + e * cols), (n, T)).astype(np.int64)
    F = above - OE                                    # F(0, c)
    Hrow = None
    nib = np.zeros((n, R, T), np.uint8)
    last = np.zeros((n, T), np.int64)
    for r in range(R):
        s = np.where(q[:, r:r + 1] == t, a, -b)
        s = np.where((q[:, r:r + 1] == nval) | (t == nval), -(npen or 0), s)
        tmp = (diag0 if r == 0 else Hrow[:, :T]) + s
        # what opens or extends a gap into column c + 1, as E(r, c + 1) + e*c: max(tmp, F)(r, c) - OE; from
        # the left boundary (c' = -1) H(r, -1) - OE, or E(r, -1) - e = -e under the free query head
        first = np.full((n, 1), -e, np.int64) if head_q else left(r) - OE
        src = np.concatenate([first, np.maximum(tmp, F) - OE], axis=1)
        E = np.maximum.accumulate(src + e * np.arange(-1, T), axis=1)[:, :T] - e * (cols - 1)
        H = np.maximum(np.maximum(tmp, F), E)
        toe = H - OE
        low2 = np.where(H == tmp, (s < 0).astype(np.int64), np.where(H == F, 3, 2))
        nib[:, r, :] = low2 | np.where(toe <= E - e, 4, 0) | np.where(toe <= F - e, 8, 0)
        F = np.maximum(toe, F - e)
        Hrow = np.concatenate([left(r), H], axis=1)
        last = np.where((ql - 1 == r)[:, None], H, last)
    inside = cols[None, :] < tl[:, None]
    masked = np.where(inside, last, M.NEG)
    score = masked.max(axis=1)
    t_end = masked.argmax(axis=1)
    out = {"score": score.astype(np.int32), "q_end": tl.astype(np.int32), "t_end": t_end.astype(np.int32),
           "q_start": np.zeros(n, np.int32), "t_start": np.zeros(n, np.int32), "n_ops": np.zeros(n, np.uint32),
           "cigar": np.zeros(batch.q_bytes, np.uint8), "text": [], "ops": [], "bound": []}
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
        while k < len(path):
            m = k
            while m < len(path) and path[m] == path[k] and m - k < 63:
                m += 1
            by.append(path[k] | ((m - k) << 2))
            k = m
        q_start, t_start, bound = 0, i + 1, ""
        if j < 0 and i >= 0 and not head_t:           # the top boundary's deletions
            rest, t_start, bound = i + 1, 0, "D"
            path += [2] * rest
            while rest > 0:
                by.append(2 | (min(rest, 63) << 2))
                rest -= 63
        elif i < 0 and j >= 0 and head_q:             # the free query head
            q_start = j + 1
        elif i < 0 and j >= 0:                        # the left boundary's insertions
            rest, bound = j + 1, "I"
            path += [3] * rest
            while rest > 0:
                by.append(3 | (min(rest, 63) << 2))
                rest -= 63
        out["q_start"][p] = q_start
        out["t_start"][p] = t_start
        out["n_ops"][p] = len(by)
        out["bound"].append(bound)
        off = int(batch.q_offsets[p])
        keep = by[:max(0, batch.q_bytes - off)]
        out["cigar"][off:off + len(keep)] = keep
        out["ops"].append(bytes(by))
        fwd, text, k = path[::-1], [], 0
        while k < len(fwd):
            m = k
            while m < len(fwd) and fwd[m] == fwd[k]:
                m += 1
            text.append(f"{m - k}{M.OPS[fwd[k]]}")
            k = m
        out["text"].append("".join(text))
    return out


def rescore(q, t, text, head, q_start, t_start, a, b, o, e):
    """(query bases consumed, target bases consumed, score) of a forward CIGAR over q[q_start:] and
    t[t_start:], op by op.  M / X by the bases; a run of k D or I costs o + e*k, except the path's first
    run where it sits in a boundary, priced as the table of the module docstring has it:
      leading I run at t_start = 0, HEAD NONE / TARGET   the left boundary H(k - 1, -1): o + e*(k - 1), one
                                                         base nothing
      leading D run at q_start = 0, HEAD NONE / QUERY    the top boundary: before M / X the diagonal
                                                         -(o + e*k); before I the value above column
                                                         k - 1, -(o + e*(k - 1)) (Q3)
      leading D run at q_start > 0, HEAD QUERY / BOTH    out of the free query head: e*k
    (No pair of the test batches puts an N on a path; N cells score by the LOCAL rule.)"""
    head_q, head_t = head in (QUERY, BOTH), head in (TARGET, BOTH)
    runs = [(int(c), op) for c, op in re.findall(r"(\d+)([MXDI])", text)]
    qi, ti, score = q_start, t_start, 0
    for x, (k, op) in enumerate(runs):
        if op in "MX":
            for _ in range(k):
                score += a if q[qi] == t[ti] else -b
                qi += 1; ti += 1
        elif op == "D":
            if x == 0 and q_start > 0 and head_q:
                score -= e * k
            elif x == 0 and q_start == 0 and not head_t:
                score -= o + e * (k - 1 if x + 1 < len(runs) and runs[x + 1][1] == "I" else k)
            else:
                score -= o + e * k
            ti += k
        else:
            if x == 0 and t_start == 0 and not head_q:
                score -= 0 if k == 1 else o + e * (k - 1)
            else:
                score -= o + e * k
            qi += k
    return qi - q_start, ti - t_start, score


def content_overhang_q():
    """Reads whose first 1-30 bases are random and whose rest is the target's start: HEAD QUERY / BOTH
    leave the random prefix free (q_start > 0) wherever skipping it beats aligning it."""
    rng = M._rng("overhang_q")
    qs, ts = [], []
    for _ in range(300):
        t = M._dna(rng, 182)
        h = int(rng.integers(1, 31))
        qs.append(M._dna(rng, h) + t[:150 - h])
        ts.append(t)
    return M.ModelBatch.from_pairs(qs, ts)


def named_batches():
    """semi_cigar_model's batches and overhang_q."""
    reg = dict(M.named_batches())
    reg["overhang_q"] = (content_overhang_q, M.DEFAULT)
    return reg


_batches = {}
_cache = {}


def batch_of(name):
    if name not in _batches:
        _batches[name] = named_batches()[name][0]()
    return _batches[name]


def reference(name, head):
    """(batch, model result) of a named batch under a head, computed once per process."""
    if (name, head) not in _cache:
        b = batch_of(name)
        _cache[name, head] = (b, semi_cigar_head(b, head, **named_batches()[name][1]))
    return _cache[name, head]
