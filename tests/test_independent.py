"""The C oracle against a second, independent numpy restatement of the reference
kernels (tests/independent.py) — CPU only.  Breaks the blind spot of the oracle and
the engine's thread-per-pair kernels sharing one reading of the reference: the two
restatements here differ in form (pair-vectorised numpy vs per-pair C).

Config 1 of BASELINE.json (1024 pairs, 64x64, seed 0x5EED0001, the repo's
host-side CPU verify scorer) runs here as the CPU plumbing case."""
import numpy as np
import pytest

import gasal_ffi as G
import helpers
import independent as I
import oracle as O


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


def _same(r, o, fields):
    for f in fields:
        bad = np.flatnonzero(r[f] != o[f])
        assert bad.size == 0, f"{f}: {bad.size} mismatches, first #{bad[0]}: numpy={r[f][bad[0]]} oracle={o[f][bad[0]]}"


def test_config1_cpu_plumbing():
    b = G.Batch.synth(1, 1024, 0x5EED0001)
    assert b.n == 1024 and set(b.q_lens) == {64} and set(b.t_lens) == {64}
    o = O.align(b, O.make_params(algo=O.LOCAL), n_threads=1)
    _same(I.local(b), o, ("score", "q_end", "t_end"))
    # related pairs (5% subs, 1% indels) align with high scores
    assert np.median(o["score"]) > 30


SCORES = [(1, 4, 6, 1), (2, 3, 5, 2), (3, 6, 0, 0)]


def _batch(seed, n=300, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    qs, ts = helpers.random_pairs(rng, n, 1, 70, 1, 90, alphabet=alphabet)
    return G.Batch.from_pairs(qs, ts)


@pytest.mark.parametrize("sc", SCORES)
@pytest.mark.parametrize("alphabet", [b"ACGT", b"ACGTN"])
def test_local_and_second_best(sc, alphabet):
    a, bb, o, e = sc
    b = _batch(11 + a, alphabet=alphabet)
    ref = O.align(b, O.make_params(algo=O.LOCAL, match=a, mismatch=bb, gap_open=o, gap_extend=e, second_best=1))
    _same(I.local(b, a, bb, o, e, second=True), ref, ("score", "q_end", "t_end", "score2", "q_end2", "t_end2"))


@pytest.mark.parametrize("sc", SCORES)
def test_global(sc):
    a, bb, o, e = sc
    b = _batch(21 + a, alphabet=b"ACGTN")
    ref = O.align(b, O.make_params(algo=O.GLOBAL, match=a, mismatch=bb, gap_open=o, gap_extend=e))
    _same(I.global_(b, a, bb, o, e), ref, ("score",))


def test_n_penalty():
    b = _batch(31, alphabet=b"ACGTN")
    for algo, fn, fields in ((O.LOCAL, I.local, ("score", "q_end", "t_end")), (O.GLOBAL, I.global_, ("score",))):
        ref = O.align(b, O.make_params(algo=algo, n_penalty=2))
        _same(fn(b, npen=2), ref, fields)


@pytest.mark.parametrize("head", [0, 1, 2, 3])
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_semiglobal(head, tail):
    b = _batch(41 + 4 * head + tail, n=200, alphabet=b"ACGTN")
    for a, bb, o, e in SCORES[:2]:
        ref = O.align(b, O.make_params(algo=O.SEMI_GLOBAL, head=head, tail=tail, match=a, mismatch=bb, gap_open=o,
                                       gap_extend=e))
        _same(I.semi(b, head, tail, a, bb, o, e), ref, ("score", "q_end", "t_end"))


def test_row_buffer_int16_wrap():
    # the inter-strip row buffer is short2; a long global alignment whose
    # left-boundary values fall below -32768 wraps there, in both restatements
    rng = np.random.default_rng(7)
    q = helpers.random_seq(rng, 40)
    t = helpers.random_seq(rng, 40)
    b = G.Batch.from_pairs([q], [t])
    ref = O.align(b, O.make_params(algo=O.GLOBAL, gap_open=2000, gap_extend=900))
    _same(I.global_(b, 1, 4, 2000, 900), ref, ("score",))


# ------------------------------------------------------------------ PairHMM ----
FLT_MIN = float(np.finfo(np.float32).tiny)


def test_pairhmm_oracle_against_float64():
    """The fp32 oracle against the float64 model on related reads over the lane-boundary
    grid.  Every cell whose haplotype is long enough for the read (helpers.hmm_insertion_bound)
    must stay >= 1e-30 in float64 and agree to 1e-5; the cells where the model itself forces
    the value below 1e-30 belong to the underflow class below."""
    pairs = helpers.hmm_related_grid()
    args = helpers.hmm_args(pairs, O.pairhmm_params)
    f = I.pairhmm64(*args)
    o = O.pairhmm(*args).astype(np.float64)
    forced = np.array([helpers.hmm_insertion_bound(len(p["read"]), len(p["hap"])) for p in pairs])
    assert forced.sum() == 10                      # R in 127, 128, 129, 255, 256 with H in 1, 2
    assert np.all(f[~forced] >= 1e-30), f[~forced].min()
    assert np.all(f[forced] < 1e-45) and np.all(o[forced] == 0.0)
    rel = np.abs(o[~forced] - f[~forced]) / f[~forced]
    print(f"pairhmm oracle vs float64: worst relative error {rel.max():.3g}, smallest value {f[~forced].min():.3g}")
    # measured: worst 3.2e-06 (R = 1, H = 500), smallest value 3.4e-28
    assert rel.max() <= 1e-5


def test_pairhmm_oracle_underflow_class():
    """What "the reference underflows" means: where the float64 value is below 1e-45 (under
    the smallest fp32 denormal) the fp32 oracle returns exactly 0, never NaN or inf."""
    pairs = helpers.hmm_unrelated(0xF10, (129, 256) * 6)
    args = helpers.hmm_args(pairs, O.pairhmm_params)
    f = I.pairhmm64(*args)
    o = O.pairhmm(*args)
    under = f < 1e-45
    assert under.sum() >= 12, (int(under.sum()), f)
    assert np.all(np.isfinite(o))
    assert np.all(o[under] == 0.0)


# -------------------------------------------------------------- CIGAR replay ----
TB_SCORES = [(1, 4, 6, 1), (2, 3, 5, 2)]
TB_ALPHABETS = [b"ACGT", b"ACGTACGTACGTN"]


def _tb_pairs(alphabet, seed=9):
    rng = np.random.default_rng(seed)
    qs, ts = helpers.random_pairs(rng, 400, 1, 80, 1, 90, alphabet=alphabet)
    return qs, ts, G.Batch.from_pairs(qs, ts)


def _replay(algo, mode, sc, alphabet, cap_zero=0.02):
    a, bb, o, e = sc
    qs, ts, b = _tb_pairs(alphabet)
    kw = dict(match=a, mismatch=bb, gap_open=o, gap_extend=e)
    r = O.align(b, O.make_params(algo=algo, start_pos=O.WITH_TB, **kw))
    keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, r["n_ops"])
    skipped = 1 - keep.mean()
    assert skipped <= 0.02, skipped                 # Q14
    st = I.replay_batch(qs, ts, b, r, sc, mode, G.decode_cigar, keep)
    print(f"{mode} {sc} {alphabet.decode()}: Q14 skipped {skipped:.3%}, score 0 {st['zero']}, "
          f"N on the path {st['n_path']} (ran off {st['ran_off']}, unchecked {st['stepped']}), checked {st['checked']}")
    assert not st["failures"], (len(st["failures"]), st["failures"][:3])
    assert st["zero"] <= cap_zero * b.n
    ref = (I.local if mode == I.LOCAL_MODE else I.global_)(b, a, bb, o, e)
    assert np.array_equal(r["score"], ref["score"])
    return st


@pytest.mark.parametrize("alphabet", TB_ALPHABETS)
@pytest.mark.parametrize("sc", TB_SCORES + [(1, 1, 0, 1)])
def test_local_tb_cigar_replay_and_rectangle(sc, alphabet):
    """Every oracle LOCAL+TB CIGAR replayed over the bases: consumed lengths equal the
    start-to-end rectangle, every M sits on a pair that scores >= 0 and every X on one that
    scores < 0, the replayed affine score equals `score`, `score` equals independent.local(),
    and the plain global alignment of the rectangle is worth `score` (the TB start is the
    start of the alignment that ends at the end cell).  Paths through an N pair follow
    rule L1 of replay_cigar and are not rectangles."""
    st = _replay(O.LOCAL, I.LOCAL_MODE, sc, alphabet)
    if alphabet == b"ACGT":
        assert st["n_path"] == 0 and st["checked"] + st["zero"] == 400
    # measured: Q14 skipped 0 everywhere, score 0: 0 pairs


@pytest.mark.parametrize("alphabet", TB_ALPHABETS)
@pytest.mark.parametrize("sc", TB_SCORES)
def test_global_tb_cigar_replay(sc, alphabet):
    """Every oracle GLOBAL+TB CIGAR replayed with the reference rules G1-G3 of replay_cigar:
    both sequences consumed (plus the pad pair), labels agree with the bases, the replayed
    score equals `score`, and `score` equals independent.global_().  G3 is what
    explains the M labels over unequal bases that G1 and G2 alone leave (about 1 % of pairs)."""
    _replay(O.GLOBAL, I.GLOBAL_MODE, sc, alphabet)
    # measured: Q14 skipped 0 of 400 on both score sets


def test_replay_cigar_rules_by_hand():
    # G2 / Q2: TTACGT against ACGT is 2I4M(+pad M) worth -3, not the textbook -4
    assert I.replay_cigar(b"TTACGT", b"ACGT", "2I5M", (1, 4, 6, 1), I.GLOBAL_MODE)[:4] == (7, 5, -3, None)
    assert I.global_textbook(b"TTACGT", b"ACGT") == -4
    # one leading I is free, one leading D is not
    assert I.replay_cigar(b"TACG", b"ACG", "1I4M", (1, 4, 6, 1), I.GLOBAL_MODE)[2] == 3
    assert I.replay_cigar(b"ACG", b"TACG", "1D4M", (1, 4, 6, 1), I.GLOBAL_MODE)[2] == -4
    # a wrong label is found, and swapping I and D breaks the consumed lengths
    assert I.replay_cigar(b"ACGT", b"ACCT", "5M", (1, 4, 6, 1), I.GLOBAL_MODE)[3] == (0, "M", 2, 2)
    assert I.replay_cigar(b"ACGT", b"ACCT", "2M1X2M", (1, 4, 6, 1), I.GLOBAL_MODE)[:4] == (5, 5, -1, None)
    assert I.replay_cigar(b"AACGT", b"ACGT", "1M1D4M", (1, 4, 6, 1), I.GLOBAL_MODE)[:2] != (6, 5)
    # G3 / Q19: the M before a gap may sit on unequal bases and scores as the mismatch it is
    assert I.replay_cigar(b"ACGTT", b"ACCAATT", "3M2D3M", (1, 4, 6, 1), I.GLOBAL_MODE)[2:4] == (2 - 4 - 8 + 2, None)
    # LOCAL: N pairs score 0 and are labelled M
    assert I.replay_cigar(b"ANG", b"ACG", "3M", (1, 4, 6, 1), I.LOCAL_MODE) == (3, 3, 2, None, 1)
    assert I.global_textbook(b"ACGT", b"AGT", (1, 4, 6, 1)) == 3 - 7


# -------------------------------------------------------------- WITH_START ----
@pytest.mark.parametrize("alphabet", TB_ALPHABETS)
@pytest.mark.parametrize("sc", TB_SCORES)
def test_local_with_start_restated(sc, alphabet):
    """WITH_START (module docstring of independent.py): the oracle's q_start and
    t_start equal independent.local_start() on every pair, and the coordinates mean what
    Q21 says: after undoing Q8 on t_start, some end cell inside the end words, at or after
    (q_end, t_end), closes a plain global alignment from the start that is worth `score`."""
    a, bb, o, e = sc
    qs, ts, b = _tb_pairs(alphabet, seed=5)
    kw = dict(match=a, mismatch=bb, gap_open=o, gap_extend=e)
    r = O.align(b, O.make_params(algo=O.LOCAL, start_pos=O.WITH_START, **kw))
    ref = I.local_start(b, a, bb, o, e)
    _same(ref, r, ("q_start", "t_start"))
    tt = I.start_true_t(r["t_start"])
    tb = O.align(b, O.make_params(algo=O.LOCAL, start_pos=O.WITH_TB, **kw))
    same = (r["q_start"] == tb["q_start"]) & (tt == tb["t_start"])
    print(f"WITH_START {sc} {alphabet.decode()}: decoded start equals the LOCAL+TB start on {same.mean():.1%}")
    for k in range(b.n):
        if r["score"][k] == 0:
            assert (r["q_start"][k], r["t_start"][k]) == (0, 0)
            continue
        q0, t0, q1, t1 = int(r["q_start"][k]), int(tt[k]), int(r["q_end"][k]), int(r["t_end"][k])
        assert 0 <= q0 <= (q1 | 7) and 0 <= t0 <= (t1 | 7), (k, q0, t0, q1, t1)
        # the end words, pads included (N scores 0 under the LOCAL rule)
        q = (qs[k] + b"N" * 8)[q0:(q1 | 7) + 1]
        t = (ts[k] + b"N" * 8)[t0:(t1 | 7) + 1]
        H = I.global_textbook(q, t, sc, n_rule=True, full=True)
        assert H.max() <= r["score"][k], (k, "an alignment from the start beats the local maximum")
        ends = H[max(q1 - q0, 0) + 1:, 1:]
        assert (ends == r["score"][k]).any(), (k, q0, t0, q1, t1, int(r["score"][k]))
    if alphabet == b"ACGT":
        assert same.mean() > 0.9                    # measured 95 %; with N (scores 0) under half


# ------------------------------------------------------------------ banded ----
@pytest.mark.parametrize("lens", [(1, 70, 1, 90), (120, 136, 120, 160)])
@pytest.mark.parametrize("k_band", [0, 1, 2, 4, 8, 400])
def test_banded(k_band, lens):
    rng = np.random.default_rng(3 + k_band)
    qs, ts = helpers.random_pairs(rng, 120, *lens, alphabet=b"ACGTN")
    b = G.Batch.from_pairs(qs, ts)
    for a, bb, o, e in SCORES[:2]:
        ref = O.align(b, O.make_params(algo=O.BANDED, k_band=k_band, match=a, mismatch=bb, gap_open=o, gap_extend=e))
        r = I.banded(b, k_band, a, bb, o, e)
        _same(r, ref, ("score", "q_end", "t_end"))
        if k_band == 400:
            # the whole matrix is inside the band; H-based and diag-based E/F (Q4) agree
            # while mismatch < open + 2*extend (an I next to a D never beats an X)
            _same(I.local(b, a, bb, o, e), ref, ("score", "q_end", "t_end"))


# --------------------------------------------------------------------- KSW ----
KSW_FIELDS = ("score", "q_end", "t_end")


def _ksw_both(qs, ts, seed, sc, npen=None):
    a, bb, o, e = sc
    b = G.Batch.from_pairs(qs, ts)
    seed = np.asarray(seed, np.uint32)
    kw = dict(match=a, mismatch=bb, gap_open=o, gap_extend=e)
    if npen is not None:
        kw["n_penalty"] = npen
    ref = O.align(b, O.make_params(algo=O.KSW, **kw), seed_scores=seed)
    r = I.ksw(b, seed, a, bb, o, e, npen=npen, state=True)
    _same(r, ref, KSW_FIELDS)
    return b, seed, r


@pytest.mark.parametrize("seeds", [(0, 5), (0, 60), (200, 300)])
@pytest.mark.parametrize("lens", [(1, 40), (100, 160)])
@pytest.mark.parametrize("alphabet", [b"ACGT", b"ACGTN"])
def test_ksw_random(alphabet, lens, seeds):
    """The oracle's k_ksw against independent.ksw() (rules K1-K3 as closed forms) on the
    shapes of test_gpu_parity.test_ksw_trimming, both score sets and an N penalty."""
    rng = np.random.default_rng(lens[0] * 7 + seeds[1] + len(alphabet))
    qs, ts = helpers.random_pairs(rng, 200, *lens, *lens, related=0.6, alphabet=alphabet)
    seed = rng.integers(*seeds, len(qs)).astype(np.uint32)
    for sc in SCORES[:2]:
        _ksw_both(qs, ts, seed, sc)
    if alphabet == b"ACGTN":
        _ksw_both(qs, ts, seed, SCORES[0], npen=2)


def test_ksw_every_length_residue():
    """Every query length 1..33 against every target length 1..33: all residues mod 8 on
    both axes (regs = (len >> 3) + 1 words, K1's extra word at the multiples of 8)."""
    rng = np.random.default_rng(0x3333)
    qs, ts = [], []
    for ql in range(1, 34):
        for tl in range(1, 34):
            q = helpers.random_seq(rng, ql)
            t = (helpers.mutate(rng, q) + helpers.random_seq(rng, tl))[:tl] if (ql + tl) % 3 else helpers.random_seq(rng, tl)
            qs.append(q); ts.append(t)
    seed = rng.integers(0, 30, len(qs)).astype(np.uint32)
    for sc in SCORES[:2] + [(1, 4, 2, 1)]:
        b, _, r = _ksw_both(qs, ts, seed, sc)
    assert set(b.q_lens) == set(range(1, 34)) and set(b.t_lens) == set(range(1, 34))


KSW_RULES = helpers.ksw_rule_batches()


@pytest.mark.parametrize("name", sorted(KSW_RULES))
def test_ksw_constructed_rules(name):
    qs, ts, sd, sc = KSW_RULES[name]
    b, seed, r = _ksw_both(qs, ts, sd, sc)
    fired = helpers.ksw_rule_fired(name, b, seed, r)
    print(f"{name}: rule decided {fired} of {b.n} pairs")
    assert fired >= 10, (name, fired)
    if name == "clip":
        # gscore == max - 5 reports the local end, max - 4 the end of the query (:188)
        assert np.all(r["q_end"][r["margin"] == 5] != b.q_lens[r["margin"] == 5])
        assert np.all(r["q_end"][(r["margin"] == 4) & (r["score"] > 4)] == b.q_lens[(r["margin"] == 4) & (r["score"] > 4)])
    if name == "seed0":
        assert not r["score"].any() and not r["q_end"].any() and not r["t_end"].any()


# --------------------------------------------------- reverse / complement ----
OPS_FIELDS = ("score", "q_end", "t_end")


def _nibbles(words):
    """Packed words as one code per base, first base in bits 31:28 (the pack kernel's order)."""
    return ((words[:, None] >> (28 - 4 * np.arange(8, dtype=np.uint32))[None, :]) & 15).astype(np.uint8).ravel()


@pytest.mark.parametrize("kind,alphabet", helpers.OPS_CASES)
def test_ops_slots_against_apply_ops(kind, alphabet):
    """orc_pack, then orc_revcomp_one pair by pair as orc_aln_batch calls it, against
    independent.apply_ops nibble for nibble.  The edge batch holds every op on sequences of one
    to five words; its pair 0 reverses a one-word query at word 0 (the read of the word before
    the sequence takes the base + idx < 0 guard), and later one-word pairs read a
    predecessor's last word whose nibbles are all non-zero."""
    import ctypes
    c = helpers.ops_case(kind, alphabet)
    b, qo, to = c["b"], c["qo"], c["to"]
    L = O.lib()
    L.orc_revcomp_one.restype = None
    for data, offs, lens, ops, other, want in ((b.q_data, b.q_offsets, b.q_lens, qo, to, c["ob"].q_data),
                                               (b.t_data, b.t_offsets, b.t_lens, to, qo, c["ob"].t_data)):
        w = np.zeros(len(data) // 8, np.uint32)
        L.orc_pack(O._ptr(data), ctypes.c_uint32(len(data)), O._ptr(w))
        plain = _nibbles(w)
        assert np.array_equal(plain, data & 15)
        for k in range(b.n):
            if ops[k] == 0 and other[k] == 0:
                continue
            L.orc_revcomp_one(O._ptr(w), ctypes.c_uint32(int(offs[k]) >> 3), ctypes.c_uint32(int(lens[k])),
                              ctypes.c_uint8(int(ops[k])), ctypes.c_int32(0x4E))
        got = _nibbles(w)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} nibbles differ, first at byte {bad[0]}: oracle {got[bad[0]]} apply_ops {want[bad[0]]}"
        moved = np.array([not np.array_equal(plain[int(o):int(o) + 8], want[int(o):int(o) + 8]) for o in offs])
        assert moved[ops != 0].mean() > 0.5
    if kind == "edges":
        words = (b.q_lens.astype(np.int64) + 7) // 8
        for op in (1, 2, 3):
            assert set(words[qo == op]) == {1, 2, 3, 4, 5}, op
            assert set(((b.t_lens.astype(np.int64) + 7) // 8)[to == op]) == {1, 2, 3, 4, 5}, op
        assert set(zip(qo.tolist(), to.tolist())) == {(x, y) for x in range(4) for y in range(4)}
        assert qo[0] & 1 and b.q_offsets[0] == 0 and words[0] == 1
        later = np.flatnonzero((qo & 1 == 1) & (words == 1) & (np.arange(b.n) > 0))
        assert later.size >= 3
        prev_last = np.array([b.q_data[int(b.q_offsets[k]) - 8:int(b.q_offsets[k])] for k in later])
        assert np.all(prev_last & 15 != 0)
        assert {int(x) % 8 for x in b.q_lens} == {0, 1, 7} and {int(x) % 8 for x in b.t_lens} == {0, 1, 7}
    else:
        assert b.n == 300 and b.q_lens.min() >= 140 and b.q_lens.max() <= 160
    if alphabet == helpers.OPS_ODD_ALPHABET:
        # bytes that are not A/C/G/T but carry a base's code: the complement must move them
        odd = np.isin(b.q_data, np.frombuffer(b"SWDQswdq", np.uint8))
        assert odd.sum() > 100 and np.all(np.isin(b.q_data[odd] & 15, [1, 3, 4, 7]))


def test_apply_ops_by_hand():
    # AACCC, reversed: the three pads move to the front (hand KAT 4); complement maps codes
    # 1 <-> 4 and 3 <-> 7 and leaves the pad's 0xE and any other code alone
    b = G.Batch.from_pairs([b"AACCC", b"ACGTNRYA"], [b"ACGTACGTA", b"T"])
    r = I.apply_ops(b, [1, 2], [3, 0])
    assert list(r.q_data[:8]) == [0xE, 0xE, 0xE, 3, 3, 3, 1, 1]
    assert list(r.q_data[8:16]) == [4, 7, 3, 1, 0xE, 2, 9, 4]
    assert list(r.t_data[:16]) == [0xE] * 7 + [4, 1, 3, 7, 4, 1, 3, 7, 4]
    assert list(r.t_data[16:24]) == [4] + [0xE] * 7
    # both ops 0: the pair is left alone whatever its neighbours do
    r = I.apply_ops(b, [0, 3], [0, 3])
    assert np.array_equal(r.q_data[:8], b.q_data[:8] & 15) and np.array_equal(r.t_data[:16], b.t_data[:16] & 15)
    with pytest.raises(ValueError):
        I.apply_ops(b, [1, 0], [0, 0], n_code=0xE)


@pytest.mark.parametrize("kind,alphabet", helpers.OPS_CASES)
def test_ops_batches_answers_depend_on_the_ops(kind, alphabet):
    """The condition on the inputs: among the pairs with a nonzero op at least half have an
    independent answer that differs from the same pair's answer without ops, for LOCAL,
    GLOBAL (score) and SEMI_GLOBAL.  On the reference alone: if a batch falls short, the
    batch changes (helpers.ops_batch), not the threshold."""
    dep = helpers.ops_dependence(helpers.ops_case(kind, alphabet))
    print(f"{kind} {alphabet.decode()}: answers that depend on the ops: {dep}")
    for name, share in dep.items():
        assert share >= 0.5, (name, share)


def _ops_oracle(c, **kw):
    return O.align(c["b"], O.make_params(**kw), q_ops=c["qo"], t_ops=c["to"])


@pytest.mark.parametrize("sc", helpers.OPS_SCORES)
@pytest.mark.parametrize("kind,alphabet", helpers.OPS_CASES)
def test_ops_oracle_local_global(kind, alphabet, sc):
    """O.align with ops against the independent functions on apply_ops(batch): LOCAL with and
    without second best, GLOBAL."""
    a, bb, o, e = sc
    c = helpers.ops_case(kind, alphabet)
    kw = dict(match=a, mismatch=bb, gap_open=o, gap_extend=e)
    ref = I.local(c["ob"], a, bb, o, e, second=True)
    _same(ref, _ops_oracle(c, algo=O.LOCAL, second_best=1, **kw), OPS_FIELDS + ("score2", "q_end2", "t_end2"))
    _same(ref, _ops_oracle(c, algo=O.LOCAL, **kw), OPS_FIELDS)
    _same(I.global_(c["ob"], a, bb, o, e), _ops_oracle(c, algo=O.GLOBAL, **kw), ("score",))


@pytest.mark.parametrize("head,tail", [(O.TARGET, O.TARGET), (O.NONE, O.TARGET), (O.QUERY, O.QUERY), (O.TARGET, O.BOTH),
                                       (O.BOTH, O.QUERY), (O.NONE, O.BOTH)])
@pytest.mark.parametrize("kind,alphabet", [helpers.OPS_CASES[1], helpers.OPS_CASES[2], helpers.OPS_CASES[3]])
def test_ops_oracle_semiglobal(kind, alphabet, head, tail):
    c = helpers.ops_case(kind, alphabet)
    for a, bb, o, e in helpers.OPS_SCORES:
        ref = _ops_oracle(c, algo=O.SEMI_GLOBAL, head=head, tail=tail, match=a, mismatch=bb, gap_open=o, gap_extend=e)
        _same(I.semi(c["ob"], head, tail, a, bb, o, e), ref, OPS_FIELDS)


@pytest.mark.parametrize("k_band", [4, 16])
@pytest.mark.parametrize("kind,alphabet", [helpers.OPS_CASES[1], helpers.OPS_CASES[3]])
def test_ops_oracle_banded(kind, alphabet, k_band):
    c = helpers.ops_case(kind, alphabet)
    for a, bb, o, e in helpers.OPS_SCORES:
        ref = _ops_oracle(c, algo=O.BANDED, k_band=k_band, match=a, mismatch=bb, gap_open=o, gap_extend=e)
        _same(I.banded(c["ob"], k_band, a, bb, o, e), ref, OPS_FIELDS)


def ops_seeds(n):
    return np.random.default_rng(0x5EED).integers(0, 41, n).astype(np.uint32)


@pytest.mark.parametrize("kind,alphabet", [helpers.OPS_CASES[1], helpers.OPS_CASES[3]])
def test_ops_oracle_ksw(kind, alphabet):
    c = helpers.ops_case(kind, alphabet)
    seed = ops_seeds(c["b"].n)
    for a, bb, o, e in helpers.OPS_SCORES:
        ref = O.align(c["b"], O.make_params(algo=O.KSW, match=a, mismatch=bb, gap_open=o, gap_extend=e),
                      q_ops=c["qo"], t_ops=c["to"], seed_scores=seed)
        _same(I.ksw(c["ob"], seed, a, bb, o, e), ref, OPS_FIELDS)


@pytest.mark.parametrize("sc", helpers.OPS_SCORES)
@pytest.mark.parametrize("kind,alphabet", helpers.OPS_CASES)
def test_ops_oracle_local_with_start(kind, alphabet, sc):
    """The WITH_START reverse pass over op-transformed slots: reversed loads of words that the
    op already reversed, with the moved pads inside the word-aligned prefixes."""
    a, bb, o, e = sc
    c = helpers.ops_case(kind, alphabet)
    r = _ops_oracle(c, algo=O.LOCAL, start_pos=O.WITH_START, match=a, mismatch=bb, gap_open=o, gap_extend=e)
    fwd = I.local(c["ob"], a, bb, o, e)
    _same(fwd, r, OPS_FIELDS)
    _same(I.local_start(c["ob"], a, bb, o, e, fwd=fwd), r, ("q_start", "t_start"))
