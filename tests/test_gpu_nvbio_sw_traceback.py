"""The Smith-Waterman / edit-distance half of the nvbio traceback kernels, nv_traceback_kernel<false, TYPE>
and nv_banded_traceback_kernel<false, TYPE, BMAX, EX> (csrc/nvtrace.hpp), against the plain-Python
definition written from the reference lines (tests/nvbio_sw_traceback_model.py) -- directly, not through
oracle/nvbio_oracle.c.  test_nvbio_sw_traceback_model.py holds what these comparisons rest on: the tie
families tie, the sink-tie family sees the LOCAL report order, the pushes cover every residue mod 4.
The plain banded traceback has no plan-describe call, so the exact 7 / 15 / 31 instances are covered by
running those bands, not by name."""
import numpy as np
import pytest

import gasal_ffi as G
import nvbio_qual_model as Q
import nvbio_sw_traceback_model as S
from test_gpu_nvbio import BUDGET, DEV_BAND, _device_traceback

pytestmark = pytest.mark.gpu

TYPES = list(S.TYPES)
SCHEMES = ["sym", "asym", "ed"]


def _texts(name, texts, shared=False):
    """Texts 2-bit little-endian where the symbols fit, else the family's own width; and 8-bit."""
    out = []
    for bits in sorted({S.text_bits(name), 8}):
        out.append(G.PackedSet.pack([max(texts, key=len)] if shared else texts, bits=bits, big_endian=False, shared=shared))
    return out


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("type_", TYPES)
def test_full_families(engine, type_, scheme):
    al = S.aligner(scheme, type_)
    for name, (pats, texts) in S.families().items():
        P = G.PackedSet.pack(pats, bits=4, big_endian=True)
        want = S.full_batch(al, pats, texts)
        for T in _texts(name, texts):
            S.same(engine.nv_traceback_host(al, P, T), want, f"{name} {scheme} {type_} texts {T.bits}-bit")
        want = S.full_batch(al, pats, [max(texts, key=len)])
        for T in _texts(name, texts, shared=True):
            S.same(engine.nv_traceback_host(al, P, T), want, f"{name} {scheme} {type_} shared {T.bits}-bit")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_full_batch_sizes(engine, n):
    # the flags lie [row][stripe][pair]: a partial wave and a partial block
    pats, texts = S.block(n)
    P, T = G.PackedSet.pack(pats, bits=4, big_endian=True), G.PackedSet.pack(texts, bits=2, big_endian=False)
    for scheme in SCHEMES + ["asym2", "positive"]:
        for type_ in (["local"] if scheme == "positive" else TYPES):
            al = S.aligner(scheme, type_)
            want = S.full_batch(al, pats, texts)
            if n == 257 and not (scheme == "ed" and type_ == "local"):
                assert {len(o) % 4 for o in want["ops"]} == {0, 1, 2, 3}     # bytes to the boundary, then words
            S.same(engine.nv_traceback_host(al, P, T), want, f"{n} pairs {scheme} {type_}")


@pytest.mark.parametrize("band", S.BANDS)
@pytest.mark.parametrize("type_", TYPES)
def test_banded_families(engine, type_, band):
    # 2..8, 9..16, 17..32: the three register classes; 7 / 15 / 31 the exact instances; every residue of the
    # four-cells-per-word flag layout
    for scheme in SCHEMES:
        al = S.aligner(scheme, type_)
        for name, (pats, texts) in S.families(band).items():
            P = G.PackedSet.pack(pats, bits=4, big_endian=True)
            want = S.banded_batch(al, band, pats, texts)
            for T in _texts(name, texts):
                S.same(engine.nv_banded_traceback_host(al, band, P, T), want, f"{name} {scheme} {type_} band {band} {T.bits}-bit")
            if name == "ties":
                want = S.banded_batch(al, band, pats, [max(texts, key=len)])
                for T in _texts(name, texts, shared=True):
                    S.same(engine.nv_banded_traceback_host(al, band, P, T), want, f"{name} {scheme} {type_} band {band} shared")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_banded_batch_sizes(engine, n):
    for band in (3, 15, 32):
        pats, texts = S.block(n, band)
        P, T = G.PackedSet.pack(pats, bits=4, big_endian=True), G.PackedSet.pack(texts, bits=2, big_endian=False)
        for scheme in ("asym2", "ed", "positive"):
            for type_ in (["local"] if scheme == "positive" else TYPES):
                al = S.aligner(scheme, type_)
                want = S.banded_batch(al, band, pats, texts)
                if n == 257:
                    assert {len(o) % 4 for o in want["ops"]} == {0, 1, 2, 3}
                S.same(engine.nv_banded_traceback_host(al, band, P, T), want, f"{n} pairs band {band} {scheme} {type_}")


def _ties23(band=None):
    pats, texts = S.families(band)["ties"]
    return pats[7:30], texts[7:30]


@pytest.mark.parametrize("kind", ["full", "banded"])
def test_chunked(engine, monkeypatch, kind):
    # chunks of 5 pairs over 23 pairs of the tie family
    band = None if kind == "full" else 15
    pats, texts = _ties23(band)
    assert len(pats) == 23
    P, T = G.PackedSet.pack(pats, bits=4, big_endian=True), G.PackedSet.pack(texts, bits=2, big_endian=False)
    max_p, max_t = max(len(p) for p in pats), max(len(t) for t in texts)
    per = G.nv_traceback_workspace(max_p, max_t, 1) if kind == "full" else G.nv_banded_traceback_workspace(max_p, band, 1)
    for scheme in ("sym", "ed"):
        for type_ in TYPES:
            al = S.aligner(scheme, type_)
            monkeypatch.setenv(BUDGET, str(5 * per))
            if kind == "full":
                got, want = engine.nv_traceback_host(al, P, T), S.full_batch(al, pats, texts)
            else:
                got, want = engine.nv_banded_traceback_host(al, band, P, T), S.banded_batch(al, band, pats, texts)
            monkeypatch.delenv(BUDGET)
            S.same(got, want, f"{kind} chunks of 5 {scheme} {type_}")


@pytest.mark.parametrize("kind", ["full", "banded"])
def test_device_entry(engine, kind):
    # the smallest ops_stride the entry point takes (M + N; 2 M + band), and one more: odd, no multiple of 4
    band = None if kind == "full" else DEV_BAND
    pats, texts = _ties23(band)
    P, T = G.PackedSet.pack(pats, bits=4, big_endian=True), G.PackedSet.pack(texts, bits=2, big_endian=False)
    max_p, max_t = max(len(p) for p in pats), max(len(t) for t in texts)
    need = max_p + max_t if kind == "full" else 2 * max_p + band
    strides = [need, need + 1 if need % 2 == 0 else need + 2]
    assert any(s % 4 for s in strides)
    for stride in strides:
        for scheme, type_ in (("asym", "local"), ("ed", "global"), ("sym", "semi")):
            al = S.aligner(scheme, type_)
            got = _device_traceback(engine, kind, al, P, T, stride, max_p, max_t)
            want = S.full_batch(al, pats, texts) if kind == "full" else S.banded_batch(al, band, pats, texts)
            S.same(got, want, f"{kind} device stride {stride} {scheme} {type_}")


@pytest.mark.parametrize("band", [7, 16, 31])
def test_plain_gotoh_banded_against_the_qual_model(engine, band):
    # nv_banded_traceback_kernel<true, ...> against nvbio_qual_model.traceback under a constant scheme
    pats, texts = S.families(band)["ties"]
    P, T = G.PackedSet.pack(pats, bits=4, big_endian=True), G.PackedSet.pack(texts, bits=2, big_endian=False)
    sc = Q.constant_scheme(2, -1, -2, -1)
    quals = [np.zeros(len(p), np.uint8) for p in pats]
    for type_ in TYPES:
        al = G.NvAligner(G.NV_GOTOH, S.TYPES[type_], 2, -1, -2, -1)
        want = Q.traceback(sc, S.TYPES[type_], band, [list(map(int, p)) for p in pats], quals, [list(map(int, t)) for t in texts])
        S.same(engine.nv_banded_traceback_host(al, band, P, T), want, f"gotoh {type_} band {band}")


@pytest.mark.parametrize("kind", ["full", "banded"])
def test_replay_of_the_gpu_output(engine, kind):
    band = None if kind == "full" else 9
    pats, texts = S.families(band)["edges"]
    P, T = G.PackedSet.pack(pats, bits=4, big_endian=True), G.PackedSet.pack(texts, bits=2, big_endian=False)
    for scheme in ("asym", "ed"):
        for type_ in TYPES:
            al = S.aligner(scheme, type_)
            g = engine.nv_traceback_host(al, P, T) if kind == "full" else engine.nv_banded_traceback_host(al, band, P, T)
            ran = 0
            for k in range(len(pats)):
                r = S.one(g, k)
                if r["sink"][0] == S.NO_CELL:
                    continue
                ran += 1
                want = r["score"] if kind == "full" else (r["score"], True)
                assert S.replay(al, pats[k], texts[k], r, band) == want, (kind, scheme, type_, k)
            assert ran >= len(pats) // 2
