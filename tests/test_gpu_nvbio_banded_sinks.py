"""GPU parity of the banded scorer's BestSink positions (gasalx_nv_banded_score_sinks_*,
csrc/nvbanded_sink.hpp): score and sink bit-exact against the oracle's banded score pass
(O.nv_banded_traceback's score and sink, itself checked by a second restatement in
test_nvbio_banded_sinks_model.py), on inputs with tied maxima built in (R.tie_pairs)."""
import os
import subprocess

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_banded_sinks_model as R
import oracle as O
from test_nvbio_banded_sinks_model import ALIGNERS, BANDS, TYPES, _env, al_of, inputs

pytestmark = pytest.mark.gpu

GLOBAL, LOCAL, SEMI = G.NV_GLOBAL, G.NV_LOCAL, G.NV_SEMI_GLOBAL
EINVAL = -1


def _same(got, want, what):
    sc, sk = got
    bad = np.nonzero((sc != want["score"]) | (sk != want["sink"]).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size}/{len(sc)} differ, first #{bad[0]}: gpu {sc[bad[0]]} {sk[bad[0]]} "
                           f"oracle {want['score'][bad[0]]} {want['sink'][bad[0]]}")


@pytest.mark.parametrize("aname", list(ALIGNERS))
@pytest.mark.parametrize("tname", list(TYPES))
def test_every_instance(engine, aname, tname):
    # every BMAX instance at and inside its edges (8, 16, 32 take the exact-length instances), the
    # packed kernel by default and the int32 kernel through the switch
    d = inputs()
    al = al_of(ALIGNERS[aname], TYPES[tname])
    for band in BANDS:
        want = O.nv_banded_traceback(al, band, d["P"], d["T"])
        assert G.nv_describe_banded_sinks_plan(al, band, 200).startswith("nvbio_banded16_")
        _same(engine.nv_banded_score_sinks_host(al, band, d["P"], d["T"]), want, f"packed band {band}")
        try:
            _env("GASALX_NVB16", "0")
            assert G.nv_describe_banded_sinks_plan(al, band, 200).startswith("nvbio_banded_")
            _same(engine.nv_banded_score_sinks_host(al, band, d["P"], d["T"]), want, f"int32 band {band}")
        finally:
            _env("GASALX_NVB16", None)
        # the old call is untouched and gives the same scores
        assert np.array_equal(engine.nv_banded_score_host(al, band, d["P"], d["T"]), want["score"])


def _mixed(n, seed):
    """n pairs whose lane partners differ in length, every seventh pattern past 1,000 symbols."""
    pats, texts = R.tie_pairs(seed, n=n, max_m=150, symbols=5)
    rng = np.random.default_rng(seed + 1)
    for k in range(0, n, 7):
        m = 1001 + int(rng.integers(0, 60))
        texts[k] = rng.integers(0, 4, m + int(rng.integers(0, 20))).astype(np.uint32)
        pats[k] = texts[k][:m].copy()
        pats[k][rng.random(m) < 0.05] = 4
    return pats, texts


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_packed_equals_int32(engine, n):
    # an odd count leaves the last lane's high half empty; the halves of a lane run to different rows
    pats, texts = _mixed(n, 0x16 + n)
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)
    max_p = max(len(p) for p in pats)
    for aname in ("gotoh", "ed"):
        for type_ in (GLOBAL, LOCAL, SEMI):
            al = al_of(ALIGNERS[aname], type_)
            want = O.nv_banded_traceback(al, 15, P, T)
            assert G.nv_describe_banded_sinks_plan(al, 15, max_p) == \
                f"nvbio_banded16_{aname}_{('global', 'local', 'semi')[type_]}_b16_sink"
            packed = engine.nv_banded_score_sinks_host(al, 15, P, T)
            try:
                _env("GASALX_NVB16", "0")
                int32 = engine.nv_banded_score_sinks_host(al, 15, P, T)
            finally:
                _env("GASALX_NVB16", None)
            _same(packed, want, f"packed {aname} {type_}")
            _same(int32, want, f"int32 {aname} {type_}")


@pytest.mark.parametrize("bits,big", [(2, True), (2, False), (4, True), (4, False), (8, True), (8, False)])
def test_text_encodings(engine, bits, big):
    pats, texts = R.tie_pairs(0x7E + bits + big, n=300, max_m=90)
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, bits, big)
    for type_ in (GLOBAL, LOCAL, SEMI):
        al = al_of(ALIGNERS["gotoh"], type_)
        _same(engine.nv_banded_score_sinks_host(al, 17, P, T), O.nv_banded_traceback(al, 17, P, T), f"type {type_}")


@pytest.mark.parametrize("bits", [2, 8])
def test_shared_text(engine, bits):
    # one text for every pattern (offsets NULL); the longest pattern is longer than the text
    rng = np.random.default_rng(0x5A)
    text = np.tile(rng.permutation(4)[:3], 30).astype(np.uint32)
    pats = [text[st:st + m].copy() for m in (0, 1, 30, 60, 88, 89, 90) for st in (0, 1)] + [np.tile(text, 2)[:91]]
    P = G.PackedSet.pack(pats, 4, True)
    T = G.PackedSet.pack([text], bits, False, shared=True)
    for type_ in (GLOBAL, LOCAL, SEMI):
        for aname in ("gotoh", "sw"):
            al = al_of(ALIGNERS[aname], type_)
            want = O.nv_banded_traceback(al, 9, P, T)
            _same(engine.nv_banded_score_sinks_host(al, 9, P, T), want, f"{aname} {type_}")
            assert want["score"][-1] == R.INT32_MIN


def test_output_combinations(engine):
    d = inputs()
    al = al_of(ALIGNERS["sw"], LOCAL)
    sc, sk = engine.nv_banded_score_sinks_host(al, 16, d["P"], d["T"])
    only_sc, no_sk = engine.nv_banded_score_sinks_host(al, 16, d["P"], d["T"], sinks=False)
    no_sc, only_sk = engine.nv_banded_score_sinks_host(al, 16, d["P"], d["T"], scores=False)
    assert no_sk is None and no_sc is None
    assert np.array_equal(only_sc, sc) and np.array_equal(only_sk, sk)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): null argument"):
        engine.nv_banded_score_sinks_host(al, 16, d["P"], d["T"], scores=False, sinks=False)
    for band in (1, 33):
        with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): band length must be 2\.\.32"):
            engine.nv_banded_score_sinks_host(al, band, d["P"], d["T"])


def _device_sets(P, T):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
    keep = [dev(P.words), dev(P.offsets), dev(T.words), dev(T.offsets)]
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    return keep, mk(P, keep[0], keep[1]), mk(T, keep[2], keep[3])


@pytest.mark.parametrize("max_pattern_len", [0, 256])
def test_device_entry_point_on_a_stream(engine, max_pattern_len):
    # the bound read back (0) or given as an upper bound; each output alone leaves the other untouched
    import torch
    d = inputs()
    P, T, n = d["P"], d["T"], d["P"].n
    al = al_of(ALIGNERS["gotoh"], LOCAL)
    want = O.nv_banded_traceback(al, 31, P, T)
    keep, pat, txt = _device_sets(P, T)
    stream = torch.cuda.Stream()
    fresh = lambda m: torch.full((m,), -77, dtype=torch.int32, device="cuda:0")
    for want_sc, want_sk in ((True, True), (True, False), (False, True)):
        dsc, dsk = fresh(n), fresh(2 * n)
        torch.cuda.synchronize()
        engine.nv_banded_score_sinks_device_ptrs(al, 31, n, pat, txt, dsc.data_ptr() if want_sc else 0,
                                                 dsk.data_ptr() if want_sk else 0, max_pattern_len=max_pattern_len,
                                                 stream=stream.cuda_stream)
        stream.synchronize()
        sc, sk = dsc.cpu().numpy(), dsk.cpu().numpy().view(np.uint32).reshape(n, 2)
        assert np.array_equal(sc, want["score"]) if want_sc else (sc == -77).all()
        assert np.array_equal(sk, want["sink"]) if want_sk else (dsk.cpu().numpy() == -77).all()
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): null argument"):
        engine.nv_banded_score_sinks_device_ptrs(al, 31, n, pat, txt, 0, 0)


def test_client_tool_agrees_with_the_banded_traceback():
    # tools/nvbio_banded_sinks_test (client of include/nvbio_batched.h alone): nvBowtie's scorer call with
    # sinks against BatchedBandedAlignmentTraceback on the same pairs; exits non-zero on any difference
    prog = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "nvbio_banded_sinks_test")
    r = subprocess.run([prog, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2000 pairs" in r.stdout and " 0 differ" in r.stdout and len(r.stdout.splitlines()) == 1
