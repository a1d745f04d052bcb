"""The drop-in GASAL2 host API (genomics-gpu_amd/csrc/gasal_api.cpp) in the states a caller who
initialises its streams from estimates reaches: page chains that grow and are reused,
gasal_host_alns_resize in the middle of a fill, the three device growth paths of gasal_aln_async,
host and device blocks of different capacity (the four-copy upload and the per-field result
copies), two storages in different states, gasal_gpu_mem_free / gasal_gpu_mem_alloc and
gasal_host_batch_add / addbase / getlast.

Every scenario is one run of tools/gasal_api_states on a scenario file written here.  Its dump is
compared with two things.  The page chains, host_max_*, gpu_max_* and the values of
gasal_is_aln_async_done are compared with tests/gasal_page_chain_model.py (written from the
reference's host_batch.cpp and gasal_align.cu:70-145).  The result arrays are compared with the
oracle and with tests/independent.py on the same pairs in round order; the two references are
required to agree with each other before the client runs.

Streams are initialised with gasal_init_streams(16, 24, 4): first pages of 64 and 96 bytes.
SEMI_GLOBAL WITH_START has no function in independent.py: its score and ends are compared with
independent.semi, its starts with the oracle alone.
"""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import independent as I
import oracle as O
from gasal_page_chain_model import PageChain, grown, pad8

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIENT = os.path.join(ROOT, "tools", "gasal_api_states")
INIT = (16, 24, 4)
SCORES = (1, 4, 6, 1)

# The four-round schedule, as (query lengths, target lengths) per round; `|` in the comments marks
# a page end.  Slots are pad8(len).  Query pages 64 / 128 / 256, target pages 96 / 192 / 384.
SCHEDULE = [
    # 1: fits page 1, both sides exactly: 4 x 16 = 64, 4 x 24 = 96
    ([16, 9, 12, 16], [24, 17, 20, 24]),
    # 2: q 24 24 (16 left, 24 over) | 24 40 40 8 16 = 128 exactly | 32 40 40 32 16 16 40
    #    t 32 48 (16 left, 24 over) | 24 64 40 64 = 192 exactly   | 56 16 64 32 48 24 40 64
    ([20, 22, 18, 40, 33, 5, 12, 30, 40, 35, 25, 16, 9, 38], [30, 44, 24, 60, 37, 57, 50, 9, 58, 32, 41, 20, 40, 60]),
    # 3: small again: q 16 8 24 = 48, t 32 16 40 = 88
    ([13, 7, 24], [28, 16, 33]),
    # 4: q 16 40 (8 left, 24 over) | 24 32 40 16 (16 left, 40 over) | 40 8 40 24 32 40 16 8
    #    t 64 (32 left, 40 over)   | 40 56 64 (32 left, 48 over)    | 48 16 24 64 32 56 40 24 16 64 = 384 exactly
    ([16, 36, 21, 29, 40, 11, 37, 6, 34, 19, 27, 40, 15, 5], [60, 35, 52, 59, 45, 10, 23, 58, 30, 51, 38, 22, 13, 60]),
]
# The same with isPacked: a byte holds two bases, so a slot is pad8(pad8(len) / 2) bytes, while the
# batch bytes handed to gasal_aln_async count bases (twice the bytes filled) and must not exceed
# host_max_*: the rounds fill at most half of what the chain holds.
PACKED_SCHEDULE = [
    ([16, 9, 12, 16], [16, 9, 12, 16]),
    # q 24 24 (16 left) | 24 24 24 24 24 (8 left) | 16 8 8 8 8 8: 224 of 448
    # t 32 32 24 (8 left) | 32 x 6 = 192 exactly | 16 16 16 8: 336 of 672
    ([40, 35, 33, 40, 37, 34, 39, 20, 9, 16, 5, 12, 7], [60, 50, 40, 55, 49, 60, 52, 57, 53, 20, 30, 17, 9]),
    ([13, 7, 24], [28, 16, 33]),
    # q 24 24 8 (8 left) | 16 24 24 24 24 (16 left) | 24 8 8 8 8
    # t 32 32 16 (16 left) | 24 32 32 32 32 32 (8 left) | 16 24 8 8
    ([38, 33, 10, 30, 40, 36, 34, 35, 39, 8, 14, 6, 16], [58, 49, 25, 44, 60, 51, 56, 50, 59, 18, 35, 11, 16]),
]


# ------------------------------------------------------------------ inputs ----
class Round:
    """One fill + launch: the pairs, their ops and seeds, where the resize happens."""

    def __init__(self, st, qs, ts, qops=None, tops=None, seeds=None, resize_at=-1, new_n=0):
        self.st, self.qs, self.ts = st, qs, ts
        n = len(qs)
        self.qops = np.zeros(n, np.uint8) if qops is None else np.asarray(qops, np.uint8)
        self.tops = np.zeros(n, np.uint8) if tops is None else np.asarray(tops, np.uint8)
        self.seeds = np.zeros(n, np.uint32) if seeds is None else np.asarray(seeds, np.uint32)
        self.resize_at, self.new_n = resize_at, new_n

    @property
    def n(self):
        return len(self.qs)


def _pairs(rng, q_lens, t_lens, alphabet=b"ACGT"):
    """Related pairs of the given lengths: the target is a copy of the query with a few
    substitutions and at most one short indel, cut or extended with random bases to its length."""
    qs, ts = [], []
    for ql, tl in zip(q_lens, t_lens):
        q = helpers.random_seq(rng, ql, alphabet)
        t = helpers.mutate(rng, q, sub=0.06, indel=0.01)
        lead = helpers.random_seq(rng, int(rng.integers(0, max(1, tl - len(t)) + 1)) if tl > len(t) else 0, alphabet)
        t = (lead + t + helpers.random_seq(rng, tl, alphabet))[:tl]
        qs.append(q); ts.append(t)
    return qs, ts


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _schedule_rounds(tag, schedule=SCHEDULE, st=0, rc=False, ksw=False, alphabets=(b"ACGT", b"AC", b"ACGT", b"GT")):
    """The four rounds on one storage.  Round 2 is written in another alphabet than rounds 1 and 3,
    so that its bytes, were they uploaded from pages 2 and 3 in round 3, would change the scores."""
    rounds = []
    for k, (ql, tl) in enumerate(schedule):
        rng = _rng(tag, k)
        qs, ts = _pairs(rng, ql, tl, alphabets[k])
        n = len(qs)
        r = Round(st, qs, ts)
        if rc:
            r.qops = rng.permutation(np.arange(n) % 4).astype(np.uint8)     # all four ops present
            r.tops = rng.permutation(np.arange(n) % 4).astype(np.uint8)
        if ksw:
            r.seeds = np.where(np.arange(n) % 3 == 0, 0, rng.integers(1, 30, n)).astype(np.uint32)   # some 0
        if k == 1:
            r.resize_at, r.new_n = INIT[2], n       # BWA-GASAL2's way: at host_max_n_alns, mid-fill
        rounds.append(r)
    return rounds


def _pack_bytes(data):
    """4-bit packing of a padded batch, as tests/test_gpu_parity.py::test_packed_input does it."""
    data = np.ascontiguousarray(data, np.uint8)
    out = np.zeros(len(data) // 8, np.uint32)
    O.lib().orc_pack(O._ptr(data), ctypes.c_uint32(len(data)), O._ptr(out))
    return out.view(np.uint8).copy()


# --------------------------------------------------------------- the model ----
class StorageModel:
    def __init__(self):
        mq, mt, mn = INIT
        self.q, self.t = PageChain.for_streams(mq, mn), PageChain.for_streams(mt, mn)
        self.host_n = mn
        self.gpu = [self.q.total_bytes, self.t.total_bytes, mn]

    def state(self):
        return {"q": self.q.states(), "t": self.t.states(), "hostmax": (self.q.total_bytes, self.t.total_bytes, self.host_n)}


def _fills(r, packed):
    """The bytes handed to gasal_host_batch_fill per pair."""
    if not packed:
        return list(r.qs), list(r.ts)
    b = G.Batch.from_pairs(r.qs, r.ts)
    def side(data, offs, lens):
        pk = _pack_bytes(data)
        return [bytes(pk[int(o) // 2:int(o) // 2 + pad8(int(n)) // 2]) for o, n in zip(offs, lens)]
    return side(b.q_data, b.q_offsets, b.q_lens), side(b.t_data, b.t_offsets, b.t_lens)


def _expect(commands, n_storages, packed=False):
    """Walks the commands over the model.  Returns the expected dump events and, per round, the
    offsets the client wrote and the batch bytes it launched with."""
    sts = [StorageModel() for _ in range(n_storages)]
    mult = 2 if packed else 1
    events, layouts, last = [], [], {}
    for cmd in commands:
        if cmd[0] == "round":
            r = cmd[1]
            m = sts[r.st]
            qf, tf = _fills(r, packed)
            qi = ti = 0
            qo, to = [], []
            for j in range(r.n):
                if j == r.resize_at:
                    m.host_n = r.new_n
                assert j < m.host_n, "scenario fills past host_max_n_alns"
                qo.append(qi * mult); to.append(ti * mult)
                q2, t2 = m.q.fill(qi, qf[j]), m.t.fill(ti, tf[j])
                assert q2 > qi and t2 > ti, "scenario holds a sequence that the chain drops"
                qi, ti = q2, t2
            assert qi * mult <= m.q.total_bytes and ti * mult <= m.t.total_bytes and r.n <= m.host_n
            ev = dict(kind="round", st=r.st, n=r.n, pre=-2, filled=(qi, ti), **m.state())
            m.gpu = [grown(m.gpu[0], qi * mult), grown(m.gpu[1], ti * mult), grown(m.gpu[2], r.n)]
            ev["gpumax"] = tuple(m.gpu)
            events.append(ev)
            layouts.append(dict(q_offsets=np.array(qo, np.uint32), t_offsets=np.array(to, np.uint32), q_bytes=qi * mult,
                                t_bytes=ti * mult, q_image=m.q.image(), t_image=m.t.image(),
                                pages=(sum(p[1] > 0 for p in m.q.states()), sum(p[1] > 0 for p in m.t.states())),
                                state=m.state(), gpu=tuple(m.gpu)))
            last[r.st] = len(layouts) - 1
        elif cmd[0] == "collect":
            m = sts[cmd[1]]
            m.q.reset(); m.t.reset()
            events.append(dict(kind="collect", st=cmd[1], done=(0, 1), after=(-2, 1), round=last[cmd[1]], **m.state()))
        elif cmd[0] == "memcycle":
            _, st, qb, tb, na = cmd
            sts[st].gpu = [qb, tb, na]
            events.append(dict(kind="memcycle", st=st, gpumax=(qb, tb, na)))
    return events, layouts


# ------------------------------------------------------ running the client ----
def _scenario_text(kw, commands, n_storages, packed=False):
    p = dict(algo=G.LOCAL, start_pos=G.WITHOUT_START, second_best=0, head=G.TARGET, tail=G.TARGET, k_band=0, rc=0)
    p.update(kw)
    lines = [f"params {p['algo']} {p['start_pos']} {p['second_best']} {p['head']} {p['tail']} {p['k_band']} "
             f"{int(packed)} {p['rc']}",
             "scores %d %d %d %d" % SCORES, "init %d %d %d" % INIT, f"storages {n_storages}"]
    hx = lambda b: bytes(b).hex() if len(b) else "-"
    for cmd in commands:
        if cmd[0] == "round":
            r = cmd[1]
            qf, tf = _fills(r, packed)
            lines.append(f"round {r.st} {r.n} {r.resize_at} {r.new_n}")
            for j in range(r.n):
                lines.append(f"pair {hx(qf[j])} {hx(tf[j])} {len(r.qs[j])} {len(r.ts[j])} {r.qops[j]} {r.tops[j]} {r.seeds[j]}")
        elif cmd[0] in ("fill", "add"):
            lines.append(f"{cmd[0]} {cmd[1]} {cmd[2]} {cmd[3]} {hx(cmd[4])}")
        else:
            lines.append(" ".join(str(x) for x in cmd))
    return "\n".join(lines) + "\n"


def _run_client(tmp_path, text):
    """One subprocess with a time limit of its own; any exit(EXIT_FAILURE) of the library fails
    the test with the client's stderr."""
    assert os.path.exists(CLIENT), "tools/gasal_api_states not built (__graft_entry__.build())"
    scen, dump = tmp_path / "scenario.txt", tmp_path / "dump.txt"
    scen.write_text(text)
    r = subprocess.run([CLIENT, str(scen), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"gasal_api_states exited {r.returncode}:\n{r.stderr[-4000:]}"
    lines = dump.read_text().splitlines()
    assert lines and lines[-1] == "end", "dump is not complete"
    return lines[:-1]


def _parse(lines):
    events, cur, side = [], None, None
    ints = lambda ws: tuple(int(w) for w in ws)
    for ln in lines:
        w = ln.split()
        if w[0] == "round":
            cur = dict(kind="round", st=int(w[3]), n=int(w[5]), q=[], t=[]); events.append(cur)
        elif w[0] == "collect":
            cur = dict(kind="collect", st=int(w[2]), q=[], t=[], res={}, res2={}); events.append(cur)
        elif w[0] == "memcycle":
            cur = dict(kind="memcycle", st=int(w[2])); events.append(cur)
        elif w[0] == "pages":
            cur = dict(kind="pages", st=int(w[2]), q=[], t=[], bytes={"q": [], "t": []}, getlast=[]); events.append(cur)
        elif w[0] in ("fill", "add"):
            events.append(dict(kind=w[0], src=w[1], ret=int(w[3])))
        elif w[0] == "pre":
            cur["pre"] = int(w[1])
        elif w[0] == "resized":
            cur["resized"] = int(w[1])
        elif w[0] == "filled":
            cur["filled"] = ints(w[1:])
        elif w[0] == "chain":
            cur[w[1]] = []; cur["n_" + w[1]] = int(w[2])
        elif w[0] == "page":
            cur[w[1]].append(ints(w[2:6]))
            if len(w) > 6:
                cur["bytes"][w[1]].append(b"" if w[6] == "-" else bytes.fromhex(w[6]))
        elif w[0] in ("hostmax", "gpumax"):
            cur[w[0]] = ints(w[1:])
        elif w[0] in ("done", "after"):
            cur[w[0]] = (int(w[1]), int(w[3]))
        elif w[0] in ("res", "res2"):
            cur[w[0]][w[1]] = np.array(w[2:], np.int64).astype(np.int32)
        elif w[0] == "cigar":
            cur["cigar"] = np.frombuffer(b"" if w[1] == "-" else bytes.fromhex(w[1]), np.uint8)
        elif w[0] == "getlast":
            cur["getlast"].append(int(w[1]))
        else:
            raise AssertionError(f"unknown dump line: {ln[:80]}")
    return events


def _check_states(got, want):
    """Chain dumps, host_max_*, gpu_max_* and the gasal_is_aln_async_done values against the model."""
    assert [e["kind"] for e in got] == [e["kind"] for e in want]
    for k, (g, w) in enumerate(zip(got, want)):
        for f in ("st", "n", "pre", "filled", "q", "t", "hostmax", "gpumax", "done", "after"):
            if f in w:
                assert g.get(f) == w[f], f"event {k} ({w['kind']}, storage {w['st']}) {f}: client {g.get(f)}, model {w[f]}"


# ------------------------------------------------------------- references ----
def _references(kw, r, lay, packed=False):
    """(batch the results refer to, oracle results, fields that must match exactly).  The oracle
    and independent.py must agree first; raises AssertionError where they do not."""
    p = dict(algo=G.LOCAL, start_pos=G.WITHOUT_START, second_best=0, head=G.TARGET, tail=G.TARGET, k_band=0, rc=0)
    p.update(kw)
    algo, sp = p["algo"], p["start_pos"]
    b = G.Batch.from_pairs(r.qs, r.ts)
    if not packed:
        # the model's device image is the batch the references score, byte for byte
        assert lay["q_image"] == bytes(b.q_data[:lay["q_bytes"]]) and lay["q_bytes"] == b.q_bytes
        assert lay["t_image"] == bytes(b.t_data[:lay["t_bytes"]]) and lay["t_bytes"] == b.t_bytes
        assert np.array_equal(lay["q_offsets"], b.q_offsets) and np.array_equal(lay["t_offsets"], b.t_offsets)
    okw = dict(algo=algo, start_pos=sp, second_best=p["second_best"], head=p["head"], tail=p["tail"], k_band=p["k_band"],
               match=SCORES[0], mismatch=SCORES[1], gap_open=SCORES[2], gap_extend=SCORES[3])
    extra = {}
    if p["rc"]:
        extra.update(q_ops=r.qops, t_ops=r.tops)
    if algo == G.KSW:
        extra.update(seed_scores=r.seeds)
    o = O.align(b, O.make_params(**okw), **extra)
    if packed:
        # the oracle on the bytes the client uploads (offsets in bases) agrees with itself on the bases
        img = lambda im, nbytes: np.frombuffer(im + bytes(nbytes - len(im)), np.uint8).copy()
        bp = G.Batch(img(lay["q_image"], lay["q_bytes"]), lay["q_offsets"], b.q_lens,
                     img(lay["t_image"], lay["t_bytes"]), lay["t_offsets"], b.t_lens)
        op = O.align(bp, O.make_params(is_packed=1, **okw))
        for f in ("score", "q_end", "t_end"):
            assert np.array_equal(op[f], o[f]), f"oracle: packed and unpacked input differ in {f}"
    ib = I.apply_ops(b, r.qops, r.tops) if p["rc"] else b
    ends = ("score", "q_end", "t_end")
    if algo == G.LOCAL:
        ref = I.local(ib, *SCORES, second=bool(p["second_best"]))
        fields = ends + (("score2", "q_end2", "t_end2") if p["second_best"] else ())
        if sp in (G.WITH_START, G.WITH_TB) and not p["rc"]:
            if sp == G.WITH_START:
                ref.update(I.local_start(ib, *SCORES, fwd=ref))
                fields += ("q_start", "t_start")
    elif algo == G.GLOBAL:
        ref, fields = I.global_(ib, *SCORES), ("score",)
    elif algo == G.SEMI_GLOBAL:
        ref, fields = I.semi(ib, p["head"], p["tail"], *SCORES), ends
    elif algo == G.BANDED:
        ref, fields = I.banded(ib, p["k_band"], *SCORES), ends
    elif algo == G.KSW:
        ref, fields = I.ksw(ib, r.seeds, *SCORES), ends
    for f in fields:
        assert np.array_equal(ref[f], o[f]), f"the references disagree on {f}: independent {ref[f]}, oracle {o[f]}"
    # what the oracle alone decides: the starts it writes (SEMI_GLOBAL, LOCAL WITH_TB)
    fields = tuple(fields) + tuple(f for f in ("q_start", "t_start")
                                   if f not in fields and sp != G.WITHOUT_START and (o[f] != O.SENTINEL).all())
    keep = None
    if sp == G.WITH_TB:
        keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, o["n_ops"])
        # at most 10 % of a scenario's pairs may be left out (a condition on the inputs)
        assert 1 - keep.mean() <= 0.10, f"{(~keep).sum()} of {b.n} pairs have a CIGAR that overruns its slot"
        mode = I.GLOBAL_MODE if algo == G.GLOBAL else I.LOCAL_MODE
        st = I.replay_batch(r.qs, r.ts, b, o, SCORES, mode, G.decode_cigar, keep)
        assert not st["failures"], ("the oracle's CIGARs do not replay", st["failures"][:3])
    return b, o, fields, keep


_FIELD = {"score2": ("res2", "score"), "q_end2": ("res2", "q_end"), "t_end2": ("res2", "t_end")}


def _check_results(kw, ev, r, b, o, fields, keep):
    what = f"storage {r.st}, {r.n} pairs"
    for f in fields:
        blk, name = _FIELD.get(f, ("res", f))
        assert name in ev[blk], f"{what}: the client dumped no {blk} {name}"
        got = ev[blk][name]
        bad = np.flatnonzero(got != o[f])
        assert bad.size == 0, f"{what} {f}: {bad.size} differ, first #{bad[0]}: api={got[bad[0]]} references={o[f][bad[0]]}"
    if keep is not None:
        algo = kw["algo"]
        n_ops = ev["res"]["n_ops"]
        assert np.array_equal(n_ops[keep], o["n_ops"][keep].astype(np.int32)), f"{what}: n_cigar_ops"
        g = dict(score=ev["res"]["score"], cigar=ev["cigar"], n_ops=n_ops)
        for k in np.flatnonzero(keep):
            off, m = int(b.q_offsets[k]), int(n_ops[k])
            assert G.decode_cigar(ev["cigar"], off, m) == G.decode_cigar(o["cigar"], off, m), f"{what}: CIGAR of pair {k}"
        if algo != G.GLOBAL:
            g.update({f: ev["res"][f] for f in ("q_start", "q_end", "t_start", "t_end")})
        mode = I.GLOBAL_MODE if algo == G.GLOBAL else I.LOCAL_MODE
        st = I.replay_batch(r.qs, r.ts, b, g, SCORES, mode, G.decode_cigar, keep)
        assert not st["failures"], (what, st["failures"][:3])


def _run_scenario(tmp_path, kw, commands, n_storages=1, packed=False):
    O.build()
    want, layouts = _expect(commands, n_storages, packed)
    rounds = [c[1] for c in commands if c[0] == "round"]
    refs = [_references(kw, r, lay, packed) for r, lay in zip(rounds, layouts)]      # CPU side first
    got = _parse(_run_client(tmp_path, _scenario_text(kw, commands, n_storages, packed)))
    _check_states(got, want)
    for g, w in zip(got, want):
        if w["kind"] == "collect":
            k = w["round"]
            _check_results(kw, g, rounds[k], *refs[k])
    return got, want, layouts


def _single_storage(rounds):
    cmds = []
    for r in rounds:
        cmds += [("round", r), ("collect", r.st)]
    return cmds


def _assert_schedule_shape(layouts, packed=False):
    """The schedule takes the paths it is meant to: checked on the model, before anything runs."""
    l1, l2, l3, l4 = layouts
    assert l1["pages"] == (1, 1) and l3["pages"] == (1, 1)
    assert l2["pages"] == (3, 3) and l4["pages"] == (3, 3)
    q1, t1 = PageChain.for_streams(INIT[0], INIT[2]).total_bytes, PageChain.for_streams(INIT[1], INIT[2]).total_bytes
    assert (q1, t1) == (64, 96)
    assert all(g > c for g, c in zip(l2["gpu"], (q1, t1, INIT[2]))), "round 2 must grow all three device capacities"
    assert l3["gpu"] == l2["gpu"] == l4["gpu"]
    for side in ("q", "t"):
        assert len(l4["state"][side]) == 3, "round 4 reuses the chain: no page is added"
        off, ds, ps, locked = l4["state"][side][0]
        assert 0 < ds < ps and locked == 1, "round 4 leaves page 1 part-filled"
        assert [p[1] for p in l3["state"][side][1:]] == [0, 0], "round 3: pages 2 and 3 contribute nothing"
    if not packed:
        assert l1["state"]["q"][0][:3] == (0, 64, 64) and l1["state"]["t"][0][:3] == (0, 96, 96)    # exactly on the page end
        assert l2["state"]["q"][1][1:3] == (128, 128) and l2["state"]["t"][1][1:3] == (192, 192)
        assert l4["state"]["t"][2][1:3] == (384, 384)
    # host and device capacities differ from round 2 on: the four-copy upload and per-field result copies
    assert l2["state"]["hostmax"][2] != l2["gpu"][2]


# ---------------------------------------------------------------- scenarios ----
def test_client_built_and_linked():
    assert os.path.exists(CLIENT), "tools/gasal_api_states not built (__graft_entry__.build())"
    ldd = subprocess.run(["ldd", CLIENT], capture_output=True, text=True).stdout
    assert "libgasal.so" in ldd


def test_chain_growth_and_reuse(tmp_path):
    """LOCAL, WITHOUT_START, four rounds on one storage: page 1 only; resize + pages 2 and 3 on
    both sides + all three device growths in one call; small again (pages 2 and 3 hold round 2's
    bytes and must contribute nothing); large again through the existing chain."""
    cmds = _single_storage(_schedule_rounds("growth"))
    _assert_schedule_shape(_expect(cmds, 1)[1])
    got, want, _ = _run_scenario(tmp_path, dict(algo=G.LOCAL), cmds)
    assert [e["resized"] for e in got if "resized" in e] == [14]
    # gasal_is_aln_async_done: -2 idle, 0 at completion with both chains reset and is_free == 1, -2 again
    for e in got:
        if e["kind"] == "round":
            assert e["pre"] == -2
        else:
            assert e["done"] == (0, 1) and e["after"] == (-2, 1)
            assert all(p[0] == p[1] == p[3] == 0 for p in e["q"] + e["t"])


GROWN_CASES = [
    ("LOCAL start", dict(algo=G.LOCAL, start_pos=G.WITH_START)),
    ("LOCAL tb", dict(algo=G.LOCAL, start_pos=G.WITH_TB)),
    ("LOCAL second", dict(algo=G.LOCAL, second_best=1)),
    ("GLOBAL", dict(algo=G.GLOBAL)),
    ("GLOBAL tb", dict(algo=G.GLOBAL, start_pos=G.WITH_TB)),
    ("SEMI start QUERY BOTH", dict(algo=G.SEMI_GLOBAL, start_pos=G.WITH_START, head=G.QUERY, tail=G.BOTH)),
    ("BANDED 8", dict(algo=G.BANDED, k_band=8)),
    ("BANDED 24", dict(algo=G.BANDED, k_band=24)),
    ("KSW", dict(algo=G.KSW)),
    ("LOCAL rc", dict(algo=G.LOCAL, rc=1)),
]


@pytest.mark.parametrize("name,kw", GROWN_CASES, ids=[c[0] for c in GROWN_CASES])
def test_every_algorithm_through_the_grown_state(tmp_path, name, kw):
    """The four-round schedule for every algorithm and output form: each passes the resize, the
    chain growth, the device regrowth of its own buffers (second-best block, seed scores, ops,
    host CIGAR buffer) and the unequal-capacity copies."""
    cmds = _single_storage(_schedule_rounds(name, rc=bool(kw.get("rc")), ksw=kw["algo"] == G.KSW))
    _assert_schedule_shape(_expect(cmds, 1)[1])
    _run_scenario(tmp_path, kw, cmds)


def test_packed_input_through_the_grown_state(tmp_path):
    """LOCAL with isPacked: the packed and unpacked device buffers are one allocation, through growth."""
    O.build()
    cmds = _single_storage(_schedule_rounds("packed", schedule=PACKED_SCHEDULE))
    _assert_schedule_shape(_expect(cmds, 1, packed=True)[1], packed=True)
    _run_scenario(tmp_path, dict(algo=G.LOCAL), cmds, packed=True)


def test_growth_factor_edges(tmp_path):
    """gasal_align.cu:70-145: the smallest factor i >= 2 with cap * i >= need.  Six storages, one
    round each: query bytes 2 x 64 and 8 more, target bytes 2 x 96 and 8 more, n = 2 x 4 and 1 more
    (8 or 9 targets of at least 9 bases need 128 or 144 bytes: the target side doubles with n)."""
    cases = [
        ([32, 25, 30, 32], [24, 17, 20, 24], (128, 96, 4)),
        ([40, 25, 30, 32], [24, 17, 20, 24], (192, 96, 4)),
        ([16, 9, 12, 16], [48, 41, 45, 48], (64, 192, 4)),
        ([16, 9, 12, 16], [56, 41, 45, 48], (64, 288, 4)),
        ([8, 5, 6, 7, 8, 5, 6, 7], [16, 9, 12, 13, 16, 10, 11, 15], (64, 192, 8)),
        ([8, 5, 6, 7, 8, 5, 6, 7, 8], [16, 9, 12, 13, 16, 10, 11, 15, 14], (128, 192, 12)),
    ]
    cmds = []
    for st, (ql, tl, _) in enumerate(cases):
        qs, ts = _pairs(_rng("factor", st), ql, tl)
        n = len(qs)
        cmds.append(("round", Round(st, qs, ts, resize_at=INIT[2] if n > INIT[2] else -1, new_n=n)))
    cmds += [("collect", st) for st in range(len(cases))]
    got, _, layouts = _run_scenario(tmp_path, dict(algo=G.LOCAL), cmds, n_storages=len(cases))
    for st, (_, _, gpu) in enumerate(cases):
        assert layouts[st]["gpu"] == gpu                     # the closed form, by hand
        assert got[st]["gpumax"] == gpu


RESIZE_CASES = [
    ("LOCAL rc second", dict(algo=G.LOCAL, rc=1, second_best=1)),
    ("LOCAL rc", dict(algo=G.LOCAL, rc=1)),
    ("KSW", dict(algo=G.KSW)),
    ("KSW rc", dict(algo=G.KSW, rc=1)),
]


@pytest.mark.parametrize("name,kw", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resize_keeps_what_was_filled(tmp_path, name, kw):
    """gasal_host_alns_resize at host_max_n_alns, halfway through a round of 8: lens, offsets, ops
    (handed over with gasal_op_fill before the resize) and seed scores of the first 4 pairs must
    survive it; the ops and seeds of the last 4 are written after it."""
    rng = _rng("resize", name)
    qs, ts = _pairs(rng, [16, 9, 24, 13, 30, 8, 21, 17], [24, 17, 40, 20, 33, 12, 28, 19])
    n = len(qs)
    ops = lambda: rng.permutation(np.arange(n) % 4).astype(np.uint8) if kw.get("rc") else None
    seeds = np.array([7, 0, 19, 3, 0, 25, 11, 1], np.uint32) if kw["algo"] == G.KSW else None
    r = Round(0, qs, ts, qops=ops(), tops=ops(), seeds=seeds, resize_at=INIT[2], new_n=n)
    got, _, _ = _run_scenario(tmp_path, kw, [("round", r), ("collect", 0)])
    assert got[0]["resized"] == n and got[0]["hostmax"][2] == n


def test_two_storages_in_different_states(tmp_path):
    """Storage 0 grows in its first round, storage 1 stays at its initial size; both are in flight
    before either is collected, twice, collected in both orders."""
    big = _schedule_rounds("two", st=0)
    small = _schedule_rounds("two-b", st=1)
    cmds = [("round", big[1]), ("round", small[0]), ("collect", 0), ("collect", 1),
            ("round", big[2]), ("round", small[2]), ("collect", 1), ("collect", 0),
            ("round", small[0]), ("round", big[3]), ("collect", 0), ("collect", 1)]
    big[1].resize_at, big[1].new_n = INIT[2], big[1].n
    small[1].resize_at = -1
    got, want, layouts = _run_scenario(tmp_path, dict(algo=G.LOCAL), cmds, n_storages=2)
    g0 = [e["gpumax"] for e in got if e["kind"] == "round" and e["st"] == 0]
    g1 = [e["gpumax"] for e in got if e["kind"] == "round" and e["st"] == 1]
    assert g0 == [(448, 672, 16)] * 3 and g1 == [(64, 96, 4)] * 3
    h1 = [e["hostmax"] for e in got if e["st"] == 1 and "hostmax" in e]
    assert set(h1) == {(64, 96, 4)}


def test_gpu_mem_free_then_alloc(tmp_path):
    """gasal_gpu_mem_free then gasal_gpu_mem_alloc(128, 192, 8) on a fresh storage, then one LOCAL
    round: the device blocks now hold 8 entries per array, the host blocks 4."""
    r = _schedule_rounds("memcycle")[0]
    got, _, _ = _run_scenario(tmp_path, dict(algo=G.LOCAL), [("memcycle", 0, 128, 192, 8), ("round", r), ("collect", 0)])
    assert got[0]["gpumax"] == (128, 192, 8) and got[1]["gpumax"] == (128, 192, 8)


def test_host_batch_add_addbase_getlast(tmp_path):
    """gasal_host_batch_add / addbase across the first page's end, and gasal_host_batch_fill of a
    sequence that fits no page: chain, page bytes and returned indices equal the model (pinned
    reference behaviour: add() counts nothing in data_size; the oversized sequence is dropped)."""
    rng = _rng("add")
    model = {"q": PageChain.for_streams(INIT[0], INIT[2]), "t": PageChain.for_streams(INIT[1], INIT[2])}
    cmds, rets = [], []
    idx = 0
    for size in (10, 1, 20, 1, 25, 10, 1, 30):          # 98 bytes: crosses 64 and forces page 2
        data = helpers.random_seq(rng, size)
        cmds.append(("add", "q", 0, idx, data))
        idx = model["q"].add(idx, data)
        rets.append(idx)
    assert len(model["q"].pages) == 2 and model["q"].pages[1].offset < 64 < idx
    data = helpers.random_seq(rng, 7)                   # below page 2's offset: lands on page 1
    cmds.append(("add", "q", 0, 3, data)); rets.append(model["q"].add(3, data))
    tidx = 0
    for size in (40, 300, 50, 300):                     # 300 > 192: dropped; again: page 3 of 384 takes it
        data = helpers.random_seq(rng, size)
        cmds.append(("fill", "t", 0, tidx, data))
        tidx = model["t"].fill(tidx, data)
        rets.append(tidx)
    assert rets[-3] == rets[-4] and rets[-1] == rets[-2] + pad8(300)
    cmds.append(("pages", 0))
    got = _parse(_run_client(tmp_path, _scenario_text(dict(algo=G.LOCAL), cmds, 1)))
    assert [e["ret"] for e in got[:-1]] == rets
    pg = got[-1]
    for side in ("q", "t"):
        m = model[side]
        assert pg[side] == m.states(), f"{side} chain: client {pg[side]}, model {m.states()}"
        for k, page in enumerate(m.pages):
            w = np.frombuffer(bytes(page.written), np.uint8).astype(bool)
            have = np.frombuffer(pg["bytes"][side][k], np.uint8)
            assert len(have) == page.page_size
            assert np.array_equal(have[w], np.frombuffer(bytes(page.data), np.uint8)[w]), f"{side} page {k} bytes"
    assert pg["hostmax"] == (model["q"].total_bytes, model["t"].total_bytes, INIT[2])
    assert pg["getlast"] == [model["q"].getlast(), model["t"].getlast()]
    assert all(p[1] == 0 for p in pg["q"]), "add() must leave data_size alone"
