"""Second, independent CPU restatement of the GASAL2 score kernels, in numpy,
vectorised across pairs (TEST INFRASTRUCTURE ONLY).

Why a second one: the C oracle (oracle/gasal_oracle.c) and the engine's
thread-per-pair kernels (genomics-gpu_amd/csrc/generic.hpp) were written by the
same hand and follow each other closely, so a misreading shared by both would
pass every parity test between them.  This module is written directly from the
reference kernels' loop structure, in a different form (all pairs advance
together, one numpy op per cell position; state arrays indexed like the
reference's h/f/p/e/global registers), and is used to check the C oracle on
config 1 and on random batches (tests/test_independent.py).

Reference loop structure restated (paths under Non-CDP/GASAL2/src/kernels):
  for each 8-column target strip i:            (local_kernel_template.h:122, global.h:65,
      reset h/f/p for the strip                 semiglobal_kernel_template.h:110)
      for each query row ridx (padded):
          h[0], e = global[ridx]                (short2: int16 storage)
          for m = 1..8: CORE_*_COMPUTE          (local :19-30, global.h:4-12, semi :17-28)
          global[ridx] = (h[8], e)
Pad bases (N_CODE) are scored like the reference: LOCAL rule (N scores 0, or
-N_PENALTY) for local/semi-global, no N rule for global (gasal_kernels.h:39-56).

Beyond the score kernels this module also restates, each in a form of its own:
  banded()          gasal_banded_tiled_kernel (banded.h:10-139): local-type cells inside a
                    band of 8x8 tiles, H-based E/F (the "deprecated" core, Q4).
  local_start()     the WITH_START reverse pass (local_kernel_template.h:441-511), see below.
  pairhmm64()       the PairHMM forward model in float64, along anti-diagonals
                    (PairHMM/inter_task/Synthetic_data/tile_1/tile_1.cu:95-175).
  ksw()             gasal_ksw_kernel (ksw_kernel_template.h:47-199), see below.
  replay_cigar()    walks a forward CIGAR over the two sequences: consumed lengths, M/X
                    labels against the bases, the affine score of the path.
  global_textbook() plain affine global DP without any reference quirk, for rectangle checks.
  apply_ops()       the reverse / complement pre-op (pack_rc_seqs.h:56-212) in base space: a
                    slice reversal of the padded slot and a code table, no words; every function
                    above runs unchanged on the batch it returns.

What the WITH_START coordinates mean.  The reverse pass does not start at the
end cell (q_end, t_end).  It starts at the last base of the 8-base *word* that holds each
end: rend_reg = (q_end >> 3) + 1 words of query, gend_reg = (t_end >> 3) + 1 words of target
(:449-456), pad bases of a last word included.  It is a LOCAL alignment of the two reversed
word-aligned prefixes, in the forward kernel's own strip-major order, that stops at the first
cell where the running maximum reaches the forward score (:469,479,482).  So
  - q_start is a true query coordinate, t_start is gidx + (m-1) where the true column is
    gidx - (m-1) (Q8): true t_start = 2 * (8 * w + 7) - t_start with w = (t_start - 7) >> 3;
  - (q_start, true t_start) is the start of *an* alignment worth `score` that ends inside
    the end words, at or after the end cell; it need not be the alignment that ends at
    (q_end, t_end), whose start the LOCAL+TB walk reports.  q[q_start:q_end+1] against
    t[t_start:t_end+1] is therefore no rectangle of anything, even after undoing Q8;
  - a forward score of 0 runs no reverse cell and reports (0, 0).
The oracle and the HIP start pass (start.hpp) both read it this way; local_start() below
restates it by running local() on the reversed prefixes and mapping the end it finds back.

KSW (ksw(), ksw_kernel_template.h:47-199).  BWA's ksw_extend walks the
target row by row over one array eh[0..qlen] of (h, e) entries and trims the column range
[beg, end) after every row.  GASAL2 wrapped both loops in tiles of 8 packed bases, and three
of its control-flow rules follow from the tiling alone.  ksw() states them as closed forms:
  K1 `if (j == qlen)` (:155) tests the j that the tiled column loops (:113-152) left behind.
     There are regs = (qlen >> 3) + 1 query words (:56), so the last word starts at column
     L = (qlen >> 3) * 8, with L <= qlen <= L + 7.  `continue` (j < beg, :120) and `break`
     (j >= end, :122) leave only the inner loop: every word before the last one ends with
     j >= end or at its eighth base and the outer loop goes on.  In the last word j runs
     L, L+1, ..; beg <= end (the scans :178-183 keep it so), so every j < beg is also < end
     and the first j >= end breaks: j = max(L, end), which exists since end <= qlen <= L + 7.
     Hence j == qlen  <=>  end == qlen or L == qlen:
         reached_end = (end == qlen) | (qlen % 8 == 0)
     A query whose length is a multiple of 8 takes the gscore update in *every* row it
     computes, whatever end is, with h1 = H(i, end - 1), the last cell the row computed (or
     the row's first-column value when beg == end and no cell was computed).
  K2 `if (m == 0) break;` (:159) leaves the loop over the 8 bases of the current target word
     (:93), not the loop over the words (:89).  The rows left in that word are not computed;
     row 8 * (word + 1) starts again with beg, end and eh as the dead row left them: the
     trimming scans were skipped, eh[beg+1..end].h hold the dead row's H, eh[end] = (h1, 0)
     (:153-154 come before the break, and so does K1's update).  As state per pair:
         skipping |= (m == 0);   skipping = False where i % 8 == 0;   a row runs iff
         i < tlen and not skipping
     (`i >= tlen` (:98) is the same break, but every later word starts past tlen too.)
  K3 `mj = m > h ? mj : j` (:140): with m starting at 0 every cell with h >= m moves mj, so
     mj is the *last* column of [beg, end) that holds the row's maximum; max_j takes it
     only when m > max strictly (:161), so among rows the *first* one wins.
The trimming scans (:178-183) as a closed form: with Z = {j in [beg, end] : eh[j] != (0, 0)},
beg' = min(Z) and end' = min(max(Z) + 2, qlen); Z empty: beg' = end, end' = min(end + 1, qlen).
Entries right of end keep whatever an earlier row (or the first row, :78-81) left there and
are read again when end grows, so the whole eh array is kept.  Query pads are never read
(j < end <= qlen), target pad rows are skipped (:98), N scores by the LOCAL rule (Q6).
Cost: rows x columns numpy steps, so ksw() is meant for max(ql), max(tl) <= 256; longer
shapes (the LDS block sizes of the 8-bit level) are checked against the oracle only.
"""
from __future__ import annotations

import numpy as np

MINUS_INF = -32768


def _codes(data, offs, lens, n_code):
    """[n, pad8(max)] 4-bit codes; positions past a pair's padded length read N."""
    pad = (lens.astype(np.int64) + 7) // 8 * 8
    width = int(pad.max(initial=8))
    idx = offs.astype(np.int64)[:, None] + np.arange(width)[None, :]
    inside = np.arange(width)[None, :] < pad[:, None]
    src = np.where(inside, np.minimum(idx, len(data) - 1), 0)
    c = (data[src].astype(np.int32) & 15)
    return np.where(inside, c, n_code & 15), pad


OP_FORWARD, OP_REVERSE, OP_COMPLEMENT, OP_REVCOMP = 0, 1, 2, 3

# complement of a 4-bit code: A (1) <-> T (4), C (3) <-> G (7), every other code kept
_COMPLEMENT = np.arange(16, dtype=np.uint8)
_COMPLEMENT[[1, 4, 3, 7]] = [4, 1, 7, 3]


class OpBatch:
    """What apply_ops returns: the six arrays of a batch, the data being 4-bit codes."""

    def __init__(self, q_data, q_offsets, q_lens, t_data, t_offsets, t_lens):
        self.q_data, self.q_offsets, self.q_lens = q_data, q_offsets, q_lens
        self.t_data, self.t_offsets, self.t_lens = t_data, t_offsets, t_lens

    @property
    def n(self):
        return len(self.q_lens)

    @property
    def q_bytes(self):
        return len(self.q_data)

    @property
    def t_bytes(self):
        return len(self.t_data)


def apply_ops(batch, q_ops, t_ops, n_code=0x4E):
    """The batch as gasal_reversecomplement_kernel (pack_rc_seqs.h:56-212) leaves it, in base
    space: same offsets and lengths, every byte of a padded slot its 4-bit code (the pack
    kernel's `& 15`, :24-31; every reader of this module masks the same way).  Op bit 0
    reverses, bit 1 complements (:109,169); a pair whose two ops are both 0 is left alone (:62).

    Closed form for n_code > 15, derived from the reverse branch (:109-167) with R = the
    slot's words and S = ceil(R / 2) iterations (:72):
      - nbr_N counts the nibbles of the last word that equal N_CODE (:113-116).  A nibble is
        at most 15 and N_CODE is 0x4E, so the count is 0 and nbr_N << 2 is 0 (:121).
      - rpac_2 = (W[R-2-i] << 32) | (W[R-1-i] >> 0) (:136).  A 32-bit shift by 32 gives 0 on
        the device, so rpac_2 = W[R-1-i]: the word before the sequence, which a one-word
        sequence reads as W[-1], never reaches the result.
      - to_queue_1 = (rev(W[i]) << 0) | (W[R-1-i] & 0) = rev(W[i]) (:152), rev being the word's
        eight nibbles in opposite order (:144-148).  Stores :160-161 therefore exchange words i
        and R-1-i, each nibble-reversed.
      - to_queue_2 = (W[R-2-i] & 0xFFFFFFFF) | (rev(W[i]) >> 32) = W[R-2-i] as read before the
        stores (:153).  It is stored only for i < S-1 (:162), where R-2-i differs from both
        i and R-1-i (R-2-i == i needs i = R/2 - 1 = S-1): the third store writes back what
        it read.
      - odd R: the last iteration has i == R-1-i, both stores write rev of the word read
        before them: the middle word is reversed in place.
    Exchanging words i <-> R-1-i with each word's nibbles reversed is the reversal of the whole
    slot of pad8(len) nibbles, pads included: after a reverse the slot *begins* with its pads.
    The complement branch (:169-205) maps A_PAK <-> T_PAK and C_PAK <-> G_PAK (1 <-> 4, 3 <-> 7,
    :5-8,182-193) on every nibble of the slot's words and leaves any other code, the pad's
    0xE included, alone.  It runs after the reverse; a per-nibble map and a permutation of
    the nibbles commute, so the order does not show in the result.

    n_code <= 15 is out of scope (ValueError): that branch counts N nibbles anywhere in the
    last word, shifts by the count, and for a one-word sequence reads the neighbouring pair's
    word while another thread may be rewriting it.  The reference is never compiled that way.

    Written per slot as a slice reversal and a table lookup; a zero-length sequence has no
    slot and is left alone."""
    if n_code <= 15:
        raise ValueError("apply_ops: n_code <= 15 is out of scope (see the docstring)")
    q_ops = np.asarray(q_ops, np.uint8); t_ops = np.asarray(t_ops, np.uint8)
    touched = (q_ops != 0) | (t_ops != 0)                       # :62

    def side(data, offs, lens, ops):
        out = np.asarray(data, np.uint8) & 15
        for k in np.flatnonzero(touched & (ops != 0)):
            lo = int(offs[k]); hi = lo + (int(lens[k]) + 7) // 8 * 8
            slot = out[lo:hi].copy()
            if ops[k] & OP_REVERSE:
                slot = slot[::-1]
            if ops[k] & OP_COMPLEMENT:
                slot = _COMPLEMENT[slot]
            out[lo:hi] = slot
        return out

    arrays = (side(batch.q_data, batch.q_offsets, batch.q_lens, q_ops), batch.q_offsets, batch.q_lens,
              side(batch.t_data, batch.t_offsets, batch.t_lens, t_ops), batch.t_offsets, batch.t_lens)
    try:
        return type(batch)(*arrays)                 # a gasal_ffi.Batch stays one
    except TypeError:
        return OpBatch(*arrays)


def op_sequences(opb):
    """Every whole slot (pad8(len) codes) of an apply_ops batch, as bytes, for replay_batch in
    LOCAL mode.  After a reverse the slot begins with its pads and real bases sit past
    position len - 1; the LOCAL kernels sweep the whole padded slot, so an end (and a CIGAR)
    may lie there."""
    def side(data, offs, lens):
        return [bytes(data[int(o):int(o) + (int(n) + 7) // 8 * 8]) for o, n in zip(offs, lens)]
    return side(opb.q_data, opb.q_offsets, opb.q_lens), side(opb.t_data, opb.t_offsets, opb.t_lens)


def _sub(rb, gb, a, b, nval, npen, n_rule):
    s = np.where(rb == gb, a, -b)
    if n_rule or npen is not None:
        s = np.where((rb == nval) | (gb == nval), -(npen or 0) if npen is not None else 0, s)
    return s


def _i16(x):
    return x.astype(np.int16).astype(np.int32)


def local(batch, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None, second=False):
    """gasal_local_kernel<LOCAL, WITHOUT_START, B> (local_kernel_template.h:72-439)."""
    q, qpad = _codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, tpad = _codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    n, R = q.shape
    T = t.shape[1]
    nval, OE = n_code & 15, o + e
    gH = np.zeros((R + 1, n), np.int32)
    gE = np.zeros((R + 1, n), np.int32)
    maxHH = np.zeros(n, np.int32)
    maxY = np.zeros(n, np.int32)
    prev = np.zeros(n, np.int32)
    maxX = np.zeros(n, np.int32)
    m2 = np.zeros(n, np.int32); y2 = np.zeros(n, np.int32); prev2 = np.zeros(n, np.int32)
    x2 = np.zeros(n, np.int32)
    for i in range(T // 8):
        strip_ok = i * 8 < tpad
        h = np.zeros((9, n), np.int32); f = np.zeros((9, n), np.int32); p = np.zeros((9, n), np.int32)
        gb = t[:, i * 8:i * 8 + 8].T
        for r in range(R):
            ok = strip_ok & (r < qpad)
            h[0] = gH[r]; ee = gE[r].copy()
            rb = q[:, r]
            for m in range(1, 9):
                s = _sub(rb, gb[m - 1], a, b, nval, npen, True)
                tmp = p[m] + s
                H = np.maximum(np.maximum(np.maximum(tmp, f[m]), ee), 0)
                h[m] = H
                f[m] = np.maximum(tmp - OE, f[m] - e)
                ee = np.maximum(tmp - OE, ee - e)
                upd = ok & (maxHH < H)
                maxY = np.where(upd, i * 8 + m - 1, maxY)
                maxHH = np.where(upd, H, maxHH)
                if second:
                    ov = ok & (m2 < H) & (maxHH > H)
                    y2 = np.where(ov, i * 8 + m - 1, y2)
                    m2 = np.where(ov, H, m2)
                p[m] = h[m - 1]
            gH[r] = _i16(h[8]); gE[r] = _i16(ee)
            maxX = np.where(ok & (prev < maxHH), r, maxX)
            if second:
                x2 = np.where(ok & (prev2 < maxHH), r, x2)     # the reference compares maxHH here (:417)
                prev2 = np.where(ok, np.maximum(m2, prev2), prev2)
            prev = np.where(ok, np.maximum(maxHH, prev), prev)
    out = {"score": maxHH, "q_end": maxX, "t_end": maxY}
    if second:
        out.update(score2=m2, q_end2=x2, t_end2=y2)
    return out


def global_(batch, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None):
    """gasal_global_kernel (global.h:31-303): score = H(ql-1, tl-1)."""
    q, qpad = _codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, tpad = _codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    n, R = q.shape
    T = t.shape[1]
    nval, OE = n_code & 15, o + e
    ql, tl = batch.q_lens.astype(np.int64), batch.t_lens.astype(np.int64)
    rows = np.arange(R + 1)
    gH = _i16(np.broadcast_to(np.where(rows == 0, 0, -(o + e * rows))[:, None], (R + 1, n)))   # short2 init
    gE = np.full((R + 1, n), MINUS_INF, np.int32)
    score = np.zeros(n, np.int32)
    for i in range(T // 8):
        h = np.zeros((9, n), np.int32); p = np.zeros((9, n), np.int32)
        f = np.full((9, n), MINUS_INF, np.int32)
        for m in range(1, 9):
            c = i * 8 + m - 1
            p[m] = 0 if c == 0 else -(o + e * c)
        gb = t[:, i * 8:i * 8 + 8].T
        for r in range(R):
            h[0] = gH[r]; ee = gE[r].copy()
            rb = q[:, r]
            for m in range(1, 9):
                s = _sub(rb, gb[m - 1], a, b, nval, npen, False)
                tmp = p[m] + s
                h[m] = np.maximum(np.maximum(tmp, f[m]), ee)
                f[m] = np.maximum(tmp - OE, f[m] - e)
                ee = np.maximum(tmp - OE, ee - e)
                p[m] = h[m - 1]
            gH[r] = _i16(h[8]); gE[r] = _i16(ee)
            # global.h:98-103,299: H of row ql-1 at column tl-1 (the pair's last strip)
            hit = (r == ql - 1) & (i == (tl - 1) // 8)
            col = ((tl - 1) % 8 + 1).astype(np.int64)
            score = np.where(hit, h[col, np.arange(n)], score)
    return {"score": score}


def semi(batch, head=2, tail=2, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None):
    """gasal_semi_global_kernel<.., WITHOUT_START, FALSE, HEAD, TAIL>
    (semiglobal_kernel_template.h:40-225).  head/tail: 0 NONE 1 QUERY 2 TARGET 3 BOTH."""
    q, qpad = _codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, tpad = _codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    n, R = q.shape
    T = t.shape[1]
    nval, OE = n_code & 15, o + e
    ql, tl = batch.q_lens.astype(np.int64), batch.t_lens.astype(np.int64)
    head_q, head_t = head in (1, 3), head in (2, 3)
    tail_q, tail_t = tail in (1, 3), tail in (2, 3)
    rows = np.arange(R + 1)
    if head_q:
        gH = np.zeros((R + 1, n), np.int32); gE = np.zeros((R + 1, n), np.int32)
    else:
        gH = _i16(np.broadcast_to(np.where(rows == 0, 0, -(o + e * rows))[:, None], (R + 1, n)))   # short2 init
        gE = np.full((R + 1, n), MINUS_INF, np.int32)
    maxHH = np.full(n, MINUS_INF, np.int32)
    maxX = tl.astype(np.int32).copy()     # :63 (Q10)
    maxY = ql.astype(np.int32).copy()
    for i in range(T // 8):
        strip_ok = i * 8 < tpad
        h = np.zeros((9, n), np.int32); p = np.zeros((9, n), np.int32)
        f = np.full((9, n), MINUS_INF, np.int32)
        if not head_t:
            for m in range(1, 9):
                c = i * 8 + m - 1
                h[m] = -(o + e * c)                       # :123-128 (Q3)
                p[m] = 0 if c == 0 else -(o + e * c)
        gb = t[:, i * 8:i * 8 + 8].T
        for r in range(R):
            ok = strip_ok & (r < qpad)
            h[0] = gH[r]; ee = gE[r].copy()
            prev_d = h[0] - OE
            rb = q[:, r]
            for m in range(1, 9):
                s = _sub(rb, gb[m - 1], a, b, nval, npen, True)
                cur = h[m] - OE
                f[m] = np.maximum(cur, f[m] - e)
                cur = np.maximum(p[m] + s, f[m])
                ee = np.maximum(prev_d, ee - e)
                cur = np.maximum(cur, ee)
                h[m] = cur
                p[m] = prev_d + OE
                prev_d = cur - OE
            # a strip past the pair's own target leaves its row buffer alone (TAIL QUERY reads it)
            gH[r] = np.where(strip_ok, _i16(h[8]), gH[r]); gE[r] = np.where(strip_ok, _i16(ee), gE[r])
            if tail_t:
                last = ok & (r == ql - 1)
                for m in range(1, 9):
                    col = i * 8 + m - 1
                    upd = last & (h[m] > maxHH) & (col < tl)
                    maxY = np.where(upd, col, maxY)
                    maxHH = np.where(upd, h[m], maxHH)
    if tail_q:
        # :185-193: H at the last padded column (global[m].x), rows m < ql (Q11)
        for mrow in range(R):
            v = gH[mrow]
            upd = (v > maxHH) & (mrow < ql)
            maxX = np.where(upd, mrow, maxX)
            maxHH = np.where(upd, v, maxHH)
        maxY = np.where(maxX != tl, ql, maxY)
    return {"score": maxHH, "q_end": maxX, "t_end": maxY}


def banded(batch, k_band, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None):
    """gasal_banded_tiled_kernel (banded.h:10-139), launched with k_band >> 3 tiles
    (gasal_align.h:80).  local() with two differences: a strip i visits only the query tiles
    max(0, i - kother + 1) <= tile < min(kband + i, QR), kother = TR - (QR - kband) (:35,83-85),
    and E/F open from H, not from diag + s (:104-110, Q4).  The per-strip h/f/p registers and
    the row buffer are only written inside the band, so whatever they held before (zeros: a
    tile's band strips are consecutive) is what the next band cell reads, as in the reference."""
    q, qpad = _codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, tpad = _codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    n, R = q.shape
    T = t.shape[1]
    nval, OE = n_code & 15, o + e
    QR, TR = qpad // 8, tpad // 8
    kb = int(k_band) >> 3
    kother = TR - (QR - kb)
    gH = np.zeros((R, n), np.int32)
    gE = np.zeros((R, n), np.int32)
    maxHH = np.zeros(n, np.int32)
    maxY = np.zeros(n, np.int32)
    prev = np.zeros(n, np.int32)
    maxX = np.zeros(n, np.int32)
    for i in range(T // 8):
        first = np.maximum(0, i - kother + 1)
        last = np.minimum(kb + i, QR)
        h = np.zeros((9, n), np.int32); f = np.zeros((9, n), np.int32); p = np.zeros((9, n), np.int32)
        gb = t[:, i * 8:i * 8 + 8].T
        for r in range(R):
            ok = (i < TR) & (r // 8 >= first) & (r // 8 < last)
            if not ok.any():
                continue
            h0 = gH[r]; ee = gE[r].copy()
            rb = q[:, r]
            left = h0
            for m in range(1, 9):
                s = _sub(rb, gb[m - 1], a, b, nval, npen, True)
                fm = np.maximum(h[m] - OE, f[m] - e)
                ee = np.maximum(left - OE, ee - e)
                H = np.maximum(np.maximum(np.maximum(p[m] + s, fm), 0), ee)
                upd = ok & (maxHH < H)
                maxY = np.where(upd, i * 8 + m - 1, maxY)
                maxHH = np.where(upd, H, maxHH)
                p[m] = np.where(ok, left, p[m])
                f[m] = np.where(ok, fm, f[m])
                h[m] = np.where(ok, H, h[m])
                left = H
            gH[r] = np.where(ok, _i16(left), gH[r]); gE[r] = np.where(ok, _i16(ee), gE[r])
            maxX = np.where(ok & (prev < maxHH), r, maxX)
            prev = np.where(ok, np.maximum(maxHH, prev), prev)
    return {"score": maxHH, "q_end": maxX, "t_end": maxY}


def ksw(batch, seed, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None, state=False):
    """gasal_ksw_kernel<B> (ksw_kernel_template.h:47-199), rules K1-K3 of the module docstring.
    All pairs advance one target row together; eh is kept as H[j], E[j] vectors over the pairs,
    beg / end / skipping as arrays.  seed: the h0 of every pair (uint32; compared unsigned with
    o + e at :79).  state=True adds, per pair, how often each rule decided something:
      k1_rows    rows that took the gscore update with end < qlen (qlen % 8 == 0 only)
      k2_resumed rows with m == 0 that were followed by a computed row (of a later word)
      k3_ties    rows whose maximum set max_j while it stood in two or more columns
      margin     max - gscore at the end (the clip rule :188 compares it with PEN_CLIP5 = 5)"""
    q, _ = _codes(batch.q_data, batch.q_offsets, batch.q_lens, n_code)
    t, _ = _codes(batch.t_data, batch.t_offsets, batch.t_lens, n_code)
    ql, tl = batch.q_lens.astype(np.int64), batch.t_lens.astype(np.int64)
    n = len(ql)
    h0 = np.asarray(seed, np.uint32).astype(np.int64) if seed is not None else np.zeros(n, np.int64)
    nval, oe = n_code & 15, o + e
    Q = int(ql.max(initial=1))
    pn = np.arange(n)
    H = np.zeros((Q + 2, n), np.int64)
    E = np.zeros((Q + 2, n), np.int64)
    H[0] = h0                                                   # :78-81
    H[1] = np.where(h0 > (oe & 0xFFFFFFFF), h0 - oe, 0)
    going = np.ones(n, bool)
    for j in range(2, Q + 1):
        going &= (j <= ql) & (H[j - 1] > e)
        H[j] = np.where(going, H[j - 1] - e, 0)
    mx = h0.copy()
    mx_i = np.full(n, -1, np.int64); mx_j = mx_i.copy(); mx_ie = mx_i.copy(); gs = mx_i.copy()
    beg = np.zeros(n, np.int64); end = ql.copy()
    skipping = np.zeros(n, bool)
    k1 = np.zeros(n, np.int64); k2 = k1.copy(); k3 = k1.copy(); pending = np.zeros(n, bool)
    cols = np.arange(Q + 2)[:, None]
    for i in range(int(tl.max(initial=0))):
        if i % 8 == 0:
            skipping[:] = False                                 # K2
        act = (i < tl) & ~skipping
        if not act.any():
            continue
        k2 += pending & act
        pending &= ~act
        gb = t[:, i]
        h1 = np.where(beg == 0, np.maximum(h0 - (o + e * (i + 1)), 0), 0)      # :105-110
        f = np.zeros(n, np.int64); m = f.copy(); mj = np.full(n, -1, np.int64); cnt = f.copy()
        for j in range(int(beg[act].min()), int(end[act].max())):
            on = act & (beg <= j) & (j < end)
            M = H[j]
            M = np.where(M != 0, M + _sub(q[:, j], gb, a, b, nval, npen, True), 0)   # :136
            h = np.maximum(np.maximum(M, E[j]), f)
            H[j] = np.where(on, h1, H[j])                       # H(i, j-1) for the next row
            h1 = np.where(on, h, h1)
            cnt = np.where(on & (h > m), 1, cnt + (on & (h == m)))
            keep = m > h                                        # K3: >= moves mj
            mj = np.where(on & ~keep, j, mj)
            m = np.where(on & ~keep, h, m)
            open_ = np.maximum(M - oe, 0)
            E[j] = np.where(on, np.maximum(E[j] - e, open_), E[j])
            f = np.where(on, np.maximum(f - e, open_), f)
        a_idx = pn[act]
        H[end[act], a_idx] = h1[act]; E[end[act], a_idx] = 0    # :153-154
        reached = act & ((end == ql) | (ql % 8 == 0))           # K1
        k1 += reached & (end != ql)
        upd = reached & ~(gs > h1)
        mx_ie = np.where(upd, i, mx_ie)
        gs = np.where(upd, h1, gs)
        dead = act & (m == 0)
        skipping |= dead                                        # K2
        pending |= dead
        live = act & ~dead
        up = live & (m > mx)
        k3 += up & (cnt >= 2)
        mx_i = np.where(up, i, mx_i); mx_j = np.where(up, mj, mx_j); mx = np.where(up, m, mx)
        # :178-183: the first and last entry of [beg, end] other than (0, 0)
        nz = ((H != 0) | (E != 0)) & (cols >= beg) & (cols <= end)
        some = nz.any(axis=0)
        first = np.where(some, nz.argmax(axis=0), end)
        last = np.where(some, Q + 1 - nz[::-1].argmax(axis=0), end - 1)
        beg = np.where(live, first, beg)
        end = np.where(live, np.minimum(last + 2, ql), end)
    local_end = (gs <= 0) | (gs <= mx - 5)                      # :188, PEN_CLIP5
    out = {"score": np.where(local_end, mx, gs).astype(np.int32),
           "q_end": np.where(local_end, mx_j + 1, ql).astype(np.int32),
           "t_end": np.where(local_end, mx_i + 1, mx_ie + 1).astype(np.int32)}
    if state:
        out.update(k1_rows=k1, k2_resumed=k2, k3_ties=k3, margin=mx - gs)
    return out


class _Pairs:
    """The six arrays local() reads, for a batch built in this module."""

    def __init__(self, qs, ts, n_code):
        def side(seqs):
            lens = np.array([len(s) for s in seqs], np.uint32)
            pad = (lens.astype(np.int64) + 7) // 8 * 8
            offs = np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.uint32)
            data = np.full(max(int(pad.sum()), 8), n_code, np.uint8)
            for o, s in zip(offs, seqs):
                data[o:o + len(s)] = s
            return data, offs, lens
        self.q_data, self.q_offsets, self.q_lens = side(qs)
        self.t_data, self.t_offsets, self.t_lens = side(ts)


def start_true_t(t_start):
    """Undo Q8: the true target coordinate of a WITH_START t_start.  The reverse pass records
    gidx + (m-1) with gidx = 8*w + 7 where the cell it means is gidx - (m-1)
    (local_kernel_template.h:41,468,476)."""
    ts = np.asarray(t_start, np.int64)
    w = (ts - 7) >> 3
    return 2 * (8 * w + 7) - ts


def local_start(batch, a=1, b=4, o=6, e=1, n_code=0x4E, npen=None, fwd=None):
    """q_start / t_start of gasal_local_kernel<LOCAL, WITH_START> (local_kernel_template.h:441-511),
    see the module docstring.  Restated as: local() over the reversed word-aligned prefixes
    q[0 : 8*rend_reg], t[0 : 8*gend_reg] (pads of the end words included, :449-456,475,480);
    its first maximum in strip-major order is the cell at which the reference's running
    maximum reaches the forward score and every loop stops (:469,479,482); that cell (r', c')
    maps back to q_start = 8*rend_reg-1-r' (:477,502) and, with Q8,
    t_start = gidx + (m-1) = 8*(gend_reg - (c'>>3)) - 1 + (c'&7) (:468,476,41).
    A forward score of 0 enters no loop: (0, 0) (:459-462,469)."""
    if fwd is None:
        fwd = local(batch, a, b, o, e, n_code, npen)
    n = len(batch.q_lens)
    rq = (fwd["q_end"].astype(np.int64) >> 3) + 1
    rt = (fwd["t_end"].astype(np.int64) >> 3) + 1

    def rev(data, offs, words):
        return [np.asarray(data[int(o):int(o) + 8 * int(w)])[::-1] for o, w in zip(offs, words)]
    r = local(_Pairs(rev(batch.q_data, batch.q_offsets, rq), rev(batch.t_data, batch.t_offsets, rt), n_code),
              a, b, o, e, n_code, npen)
    assert np.array_equal(r["score"], fwd["score"]), "reversed prefixes must reach the forward score"
    rr, cc = r["q_end"].astype(np.int64), r["t_end"].astype(np.int64)
    qs = 8 * rq - 1 - rr
    ts = 8 * (rt - (cc >> 3)) - 1 + (cc & 7)
    zero = fwd["score"] == 0
    return {"q_start": np.where(zero, 0, qs).astype(np.int32), "t_start": np.where(zero, 0, ts).astype(np.int32)}


def pairhmm64(reads, read_off, read_len, qm, delta, xiksi, alpha, haps, hap_off, hap_len):
    """The PairHMM forward value of every pair in float64
    (PairHMM/inter_task/Synthetic_data/tile_1/tile_1.cu:95-175, constants :228-234).
    The fp32 parameter arrays and the reference's fp32 constants (c0 = 1.329228e+36f, 0.9f,
    0.1f) are widened as given, so only the arithmetic differs from an fp32 evaluation.
      D[-1][j] = c0/H, M[-1][j] = I[-1][j] = 0, column -1 is 0 (but D[-1][-1] = c0/H)
      prior(i,j) = 1 - qm_i if read_i == hap_j else qm_i / 3
      M[i][j] = prior(i,j) * (alpha_i*M[i-1][j-1] + 0.9*(I[i-1][j-1] + D[i-1][j-1]))
      I[i][j] = delta_i*M[i-1][j] + 0.1*I[i-1][j]
      D[i][j] = xi_i*M[i][j-1] + 0.1*D[i][j-1]
      result  = sum_j M[R-1][j] + I[R-1][j]
    Form: all pairs advance together one anti-diagonal d = i + j at a time; arrays are indexed
    by read row (slot 0 is row -1), the diagonals d-1 and d-2 are kept."""
    R = np.asarray(read_len, np.int64); H = np.asarray(hap_len, np.int64)
    ro = np.asarray(read_off, np.int64); ho = np.asarray(hap_off, np.int64)
    n = len(R)
    if n == 0:
        return np.zeros(0, np.float64)
    Rm = int(R.max())
    rows = np.arange(Rm)
    ridx = np.minimum(ro[:, None] + rows[None, :], len(reads) - 1)
    rd = np.asarray(reads, np.uint8)[ridx]
    w = lambda x: np.asarray(x, np.float32).astype(np.float64)[ridx]
    Qm, De, Xi, Al = w(qm), w(delta), w(xiksi), w(alpha)
    p_eq, p_ne = 1.0 - Qm, Qm / 3.0
    c0, c3, c4 = (float(np.float32(x)) for x in (1.329228e+36, 0.9, 0.1))
    haps = np.asarray(haps, np.uint8)
    row_ok = rows[None, :] < R[:, None]
    zero = np.zeros((n, Rm + 1))
    M1, I1, D1, M2, I2, D2 = (zero.copy() for _ in range(6))
    D1[:, 0] = D2[:, 0] = c0 / H                      # row -1, any column
    res = np.zeros(n)
    pn = np.arange(n)
    for d in range(int((R + H).max()) - 1):
        j = d - rows[None, :]
        ok = row_ok & (j >= 0) & (j < H[:, None])
        hb = haps[np.clip(ho[:, None] + j, 0, len(haps) - 1)]
        prior = np.where(hb == rd, p_eq, p_ne)
        M = np.where(ok, prior * (Al * M2[:, :-1] + c3 * (I2[:, :-1] + D2[:, :-1])), 0.0)
        I = np.where(ok, De * M1[:, :-1] + c4 * I1[:, :-1], 0.0)
        D = np.where(ok, Xi * M1[:, 1:] + c4 * D1[:, 1:], 0.0)
        jl = d - (R - 1)
        last = (jl >= 0) & (jl < H)
        res += np.where(last, M[pn, R - 1] + I[pn, R - 1], 0.0)
        M2, I2, D2 = M1, I1, D1
        M1 = np.concatenate([zero[:, :1], M], axis=1)
        I1 = np.concatenate([zero[:, :1], I], axis=1)
        D1 = np.concatenate([(c0 / H)[:, None], D], axis=1)
    return res


def _affine_rows(q, t, a, b, o, e, nval, npen, n_rule):
    """H of the textbook affine global DP, [len(q)+1, len(t)+1] with the boundary row/column."""
    q = np.asarray(q, np.int64) & 15; t = np.asarray(t, np.int64) & 15
    nq, nt = len(q), len(t)
    NEG = -(1 << 40)
    cols = np.arange(nt + 1, dtype=np.int64)
    H = np.empty((nq + 1, nt + 1), np.int64)
    H[0] = np.where(cols == 0, 0, -(o + e * cols))
    F = np.full(nt + 1, NEG, np.int64)
    for i in range(1, nq + 1):
        s = np.where(q[i - 1] == t, a, -b)
        if n_rule:
            s = np.where((q[i - 1] == nval) | (t == nval), -(npen or 0), s)
        F = np.maximum(H[i - 1] - (o + e), F - e)
        best = np.full(nt + 1, NEG, np.int64)
        best[0] = -(o + e * i)
        best[1:] = np.maximum(H[i - 1, :-1] + s, F[1:])
        # E[j] = max_{k<j} best[k] - o - e*(j-k): a gap never opens from an E-derived cell
        run = np.maximum.accumulate(best + e * cols)
        E = np.full(nt + 1, NEG, np.int64)
        E[1:] = run[:-1] - o - e * cols[1:]
        H[i] = np.maximum(best, E)
    return H


def global_textbook(q, t, scores=(1, 4, 6, 1), n_code=0x4E, npen=None, n_rule=False, full=False):
    """Plain affine global alignment score of byte sequences q and t (codes = byte & 15):
    H = max(diag + s, E, F), gaps of k cost o + e*k on every side, no reference quirk
    (no Q2 boundary, no Q4 shortcut, no int16 buffer).  n_rule: score N like the LOCAL
    kernels (0, or -npen).  full: return the whole H matrix with its boundary."""
    a, b, o, e = scores
    H = _affine_rows(np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8), a, b, o, e,
                     n_code & 15, npen, n_rule)
    return H if full else int(H[-1, -1])


LOCAL_MODE, GLOBAL_MODE = "local", "global"


def replay_cigar(q, t, cigar, scores=(1, 4, 6, 1), mode=LOCAL_MODE, n_code=0x4E, npen=None):
    """Walk the forward CIGAR text (gasal_ffi.decode_cigar) over byte sequences q and t.
    Returns (q_used, t_used, score, bad, n_pairs): the bases each side consumed, the affine
    score of the path (M/X by the bases' substitution score, a run of k I or D costs o + e*k),
    the first (op index, op, q position, t position) whose M/X label disagrees with the
    bases, or None, and the number of M/X base pairs that hold an N (LOCAL only, rule L1).
    M consumes both, X both, I the query, D the target (get_tb.h:107-108).

    LOCAL: q and t are the aligned slices q[q_start:q_end+1], t[t_start:t_end+1]; a base
    pair with an N scores 0 (-npen with N_PENALTY) and is labelled by that score's sign
    (gasal_kernels.h:39-51, local_kernel_template.h:49).
      L1 the LOCAL walk stops when its own running sum reaches `score`, and that sum counts
         every op-0 cell as +match (get_tb.h:100-103) although a pair with an N scored 0 in
         the forward pass.  A path through n such pairs therefore stops n*match early (the
         CIGAR is a suffix of the alignment: score here + n_pairs*match == `score`), or
         steps over `score` without ever equalling it and runs off the matrix (a start
         coordinate of -1).  Without N on the path the replayed score is `score` itself.

    GLOBAL: q and t are the whole sequences; no N rule (gasal_kernels.h:53-54).  Reference
    rules applied, each needed for the replay to close:
      G1 the walk starts at the pad cell (i, j) = (tl, ql), one past both ends (get_tb.h:21-23,
         Q9): the CIGAR ends with one M over the pad pair, which belongs to no base and is
         left out of the score; q_used / t_used count it (ql + 1, tl + 1).
      G2 a leading run of k I costs o + e*(k-1), and 0 for k = 1: the left boundary is
         H(r,-1) = -(o + e*r), H(0,-1) = 0 (global.h:57-60, Q2).
      G3 the last pair of an M run that is followed by an I or D run may hold unequal
         bases: in gap mode a cell whose extend bit is clear ends the gap through that
         cell's diagonal and is written as op 0 whatever the bases are (get_tb.h:74-82,
         Q19; the gap opened from diag + s, not from H, global.h:7-12, Q4).  It scores
         its real substitution value and is not a label disagreement."""
    import re
    a, b, o, e = scores
    nval = n_code & 15
    qc = np.frombuffer(bytes(q), np.uint8).astype(np.int64) & 15
    tc = np.frombuffer(bytes(t), np.uint8).astype(np.int64) & 15
    is_global = mode == GLOBAL_MODE
    if is_global:                                   # G1: the pad pair
        qc = np.append(qc, nval); tc = np.append(tc, nval)
    ops = [(int(k), op) for k, op in re.findall(r"(\d+)([MXDI])", cigar)]
    qi = ti = 0
    score = n_pairs = 0
    bad = None
    for u, (k, op) in enumerate(ops):
        if op in "MX":
            for x in range(k):
                if qi >= len(qc) or ti >= len(tc):
                    return qi + (k - x), ti + (k - x), score, bad or (u, op, qi, ti), n_pairs
                pad_pair = is_global and qi == len(qc) - 1 and ti == len(tc) - 1
                s = a if qc[qi] == tc[ti] else -b
                if not is_global and (qc[qi] == nval or tc[ti] == nval):
                    s = -npen if npen is not None else 0
                    n_pairs += 1
                elif is_global and npen is not None and (qc[qi] == nval or tc[ti] == nval):
                    s = -npen
                want = "M" if s >= 0 else "X"
                g3 = (is_global and op == "M" and x == k - 1 and u + 1 < len(ops) and ops[u + 1][1] in "ID")
                if op != want and not g3 and bad is None:
                    bad = (u, op, qi, ti)
                if not pad_pair:
                    score += s
                qi += 1; ti += 1
        else:
            cost = o + e * k
            if is_global and u == 0 and op == "I":                    # G2
                cost = o + e * (k - 1) if k > 1 else 0
            score -= cost
            if op == "I":
                qi += k
            else:
                ti += k
    if is_global and (not ops or ops[-1][1] != "M") and bad is None:   # G1: the pad pair is an M
        bad = (len(ops) - 1, ops[-1][1] if ops else "", qi, ti)
    return qi, ti, score, bad, n_pairs


def replay_batch(qs, ts, batch, res, scores, mode, decode, keep, rect=True):
    """replay_cigar over every kept pair of a WITH_TB result (res: score, cigar, n_ops and,
    LOCAL, the four coordinates; decode: gasal_ffi.decode_cigar).  Returns a dict of
    counts: checked, zero (LOCAL pairs of score 0: no alignment to replay), n_path (LOCAL
    pairs with an N pair on the path, rule L1), ran_off (of those, walks that left the
    matrix), stepped (of those, match > 1: not checked further), and `failures`, a list of (pair, what, detail).  Per pair it checks the
    consumed lengths, the labels, the replayed score and, LOCAL with rect, that
    global_textbook of the start-to-end rectangle equals `score`."""
    out = dict(checked=0, zero=0, n_path=0, ran_off=0, stepped=0, failures=[])
    fail = lambda k, what, d: out["failures"].append((int(k), what, d))
    a = scores[0]
    for k in np.flatnonzero(keep):
        cig = decode(res["cigar"], int(batch.q_offsets[k]), int(res["n_ops"][k]))
        sc = int(res["score"][k])
        if mode == GLOBAL_MODE:
            qu, tu, s, bad, _ = replay_cigar(qs[k], ts[k], cig, scores, mode)
            want = (len(qs[k]) + 1, len(ts[k]) + 1)
            npairs = 0
        else:
            if sc == 0:
                out["zero"] += 1
                continue
            q0, q1, t0, t1 = (int(res[f][k]) for f in ("q_start", "q_end", "t_start", "t_end"))
            if q0 < 0 or t0 < 0:                     # L1: the walk stepped over `score`
                out["n_path"] += 1; out["ran_off"] += 1
                if replay_cigar(qs[k][max(q0, 0):q1 + 1], ts[k][max(t0, 0):t1 + 1], cig, scores, mode)[4] == 0:
                    fail(k, "start", f"walk left the matrix without an N pair on the path: {cig}")
                continue
            q, t = qs[k][q0:q1 + 1], ts[k][t0:t1 + 1]
            qu, tu, s, bad, npairs = replay_cigar(q, t, cig, scores, mode)
            want = (len(q), len(t))
            out["n_path"] += npairs > 0
            if npairs and a != 1:                    # L1: the sum may have stepped over `score`
                out["stepped"] += 1                  # and met it again anywhere; nothing to hold
                continue
            s += npairs * a                          # L1
        out["checked"] += 1
        if (qu, tu) != want:
            fail(k, "lengths", f"consumed {(qu, tu)} of {want}: {cig}")
        if bad is not None:
            fail(k, "label", f"{bad}: {cig}")
        if s != sc:
            fail(k, "score", f"replayed {s}, reported {sc}: {cig}")
        if mode == LOCAL_MODE and rect and npairs == 0:
            g = global_textbook(q, t, scores, n_rule=True)
            if g != sc:
                fail(k, "rectangle", f"global alignment of the rectangle {g}, score {sc}")
    return out


def replay_global_slots(opb, res, scores, decode, keep):
    """replay_cigar over the GLOBAL + TB CIGARs of an apply_ops batch.  The score is H(ql-1, tl-1)
    over the first ql and tl codes of the slots, but the walk starts at the pad cell (tl, ql)
    (rule G1).  Without ops that cell holds two pads, which match, and the walk leaves it
    through its diagonal.  After a reverse the codes at positions ql and tl are real bases:
      - ql % 8 and tl % 8 both non-zero: (tl, ql) is a cell the sweep computed, with a
        direction of its own, possibly a gap that never passes through (ql-1, tl-1).  The
        CIGAR is then a global path over the sequences one code longer, and its score is that
        cell's H: global_() of the same slots with both lengths one larger (the padded slots
        are the same, so is the sweep).  Checked as such: replay_cigar over q[:ql+1], t[:tl+1]
        with a closing M for rule G1's unscored pair.  Where the CIGAR leaves the cell through
        its diagonal, the path without that pair must be worth the reported score.
      - otherwise the cell lies past the swept matrix, its direction word reads 0 and the
        walk writes M whatever the codes: replay_cigar's own G1.
    Returns dict(checked, through: pairs whose pad cell was left through its diagonal,
    failures)."""
    a, b, o, e = scores
    ql, tl = np.asarray(opb.q_lens, np.int64), np.asarray(opb.t_lens, np.int64)
    inner = (ql % 8 != 0) & (tl % 8 != 0)
    ext = OpBatch(opb.q_data, opb.q_offsets, (ql + inner).astype(np.uint32),
                  opb.t_data, opb.t_offsets, (tl + inner).astype(np.uint32))
    pad_h = global_(ext, a, b, o, e)["score"]
    out = dict(checked=0, through=0, failures=[])
    fail = lambda k, what, d: out["failures"].append((int(k), what, d))
    for k in np.flatnonzero(keep):
        cig = decode(res["cigar"], int(opb.q_offsets[k]), int(res["n_ops"][k]))
        sc = int(res["score"][k])
        x = int(inner[k])
        q = bytes(opb.q_data[int(opb.q_offsets[k]):int(opb.q_offsets[k]) + int(ql[k]) + x])
        t = bytes(opb.t_data[int(opb.t_offsets[k]):int(opb.t_offsets[k]) + int(tl[k]) + x])
        qu, tu, s, bad, _ = replay_cigar(q, t, cig + "1M" * x, scores, GLOBAL_MODE)
        out["checked"] += 1
        if (qu, tu) != (len(q) + 1, len(t) + 1):
            fail(k, "lengths", f"consumed {(qu, tu)} of {(len(q) + 1, len(t) + 1)}: {cig}")
        if bad is not None:
            fail(k, "label", f"{bad}: {cig}")
        if x:
            if s != int(pad_h[k]):
                fail(k, "pad cell", f"replayed {s}, H at the pad cell {int(pad_h[k])}: {cig}")
            if cig[-1] in "MX":
                out["through"] += 1
                s -= a if q[-1] & 15 == t[-1] & 15 else -b
            else:
                continue
        else:
            out["through"] += 1
        if s != sc:
            fail(k, "score", f"replayed {s}, reported {sc}: {cig}")
    return out
