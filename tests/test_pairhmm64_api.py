"""The float64 PairHMM and log10 entry points at the C-ABI boundary (no GPU), and forward64,
the reference the GPU tests of test_gpu_pairhmm64.py use where tests/independent.py's
pairhmm64 (fixed initial constant 2^120) underflows: a plain row-by-row float64 evaluation
with the initial constant as an argument, pinned here to pairhmm64."""
import ctypes
import os
import re

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import independent as I
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = (
    "gasalx_pairhmm64_device", "gasalx_pairhmm64_host", "gasalx_pairhmm64_quals_device",
    "gasalx_pairhmm64_quals_host", "gasalx_pairhmm_log10_device", "gasalx_pairhmm_log10_host",
    "gasalx_pairhmm_quals_log10_device", "gasalx_pairhmm_quals_log10_host",
)


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


def forward64(pair, c0):
    """The PairHMM forward value of one pair, dict(read, hap, bq, iq, dq), in float64 from the
    initial constant c0: the recurrence and boundary of independent.pairhmm64's docstring, one
    read row at a time (index k of a row is column k - 1).  The fp32 parameters
    (oracle.pairhmm_params) and the constants 0.9f / 0.1f are widened as given."""
    bq, iq, dq = (np.asarray(pair[k]).astype(np.uint8) for k in ("bq", "iq", "dq"))
    qm, de, xi, al = (np.asarray(a, np.float32).astype(np.float64) for a in O.pairhmm_params(bq, iq, dq))
    read = np.frombuffer(pair["read"].encode(), np.uint8)
    hap = np.frombuffer(pair["hap"].encode(), np.uint8)
    R, H = len(read), len(hap)
    c3, c4 = float(np.float32(0.9)), float(np.float32(0.1))
    Mp, Ip, Dp = np.zeros(H + 1), np.zeros(H + 1), np.full(H + 1, c0 / H)      # row -1
    for i in range(R):
        prior = np.where(hap == read[i], 1.0 - qm[i], qm[i] / 3.0)
        M, Iv = np.zeros(H + 1), np.zeros(H + 1)
        M[1:] = prior * (al[i] * Mp[:-1] + c3 * (Ip[:-1] + Dp[:-1]))
        Iv[1:] = de[i] * Mp[1:] + c4 * Ip[1:]
        xm = (xi[i] * M).tolist()
        D = [0.0] * (H + 1)
        d = 0.0
        for k in range(1, H + 1):
            d = xm[k - 1] + c4 * d
            D[k] = d
        Mp, Ip, Dp = M, Iv, np.array(D)
    return float((Mp[1:] + Ip[1:]).sum())


def test_names_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "gasalx.h")).read()
    declared = set(re.findall(r"^\s*int\s*(gasalx_\w+)\s*\(", src, re.M))
    lib = G.lib()
    for name in NAMES:
        assert name in declared, name
        assert name in G.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.gasalx_abi_version() == 1


def test_null_engine_is_einval():
    lib = G.lib()
    hb, qb = G.CHmmBatch(), G.CHmmQualBatch()
    out = np.zeros(4, np.float64)
    used = np.zeros(4, np.uint8)
    cnt = ctypes.c_uint32(7)
    o, u = ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(used.ctypes.data)
    EINVAL = -1          # GASALX_EINVAL
    f0 = ctypes.c_float(0.0)
    assert lib.gasalx_pairhmm64_device(None, ctypes.byref(hb), o, None) == EINVAL
    assert lib.gasalx_pairhmm64_host(None, ctypes.byref(hb), o) == EINVAL
    assert lib.gasalx_pairhmm64_quals_device(None, ctypes.byref(qb), o, None) == EINVAL
    assert lib.gasalx_pairhmm64_quals_host(None, ctypes.byref(qb), o) == EINVAL
    assert lib.gasalx_pairhmm_log10_device(None, ctypes.byref(hb), f0, o, u, None) == EINVAL
    assert lib.gasalx_pairhmm_log10_host(None, ctypes.byref(hb), f0, o, u, ctypes.byref(cnt)) == EINVAL
    assert lib.gasalx_pairhmm_quals_log10_device(None, ctypes.byref(qb), f0, o, u, None) == EINVAL
    assert lib.gasalx_pairhmm_quals_log10_host(None, ctypes.byref(qb), f0, o, u, ctypes.byref(cnt)) == EINVAL
    assert not out.any() and not used.any()


def test_engine_methods_present():
    for name in ("pairhmm64_host", "pairhmm64_quals_host", "pairhmm_log10_host", "pairhmm_quals_log10_host"):
        assert callable(getattr(G.Engine, name)), name


def test_forward64_matches_pairhmm64():
    """forward64 from 2^1020, scaled by 2^-900 (exact: every value is >= 2e-220), is pairhmm64."""
    pairs = helpers.hmm_related_grid() + helpers.hmm_unrelated(0xF10, (129, 256) * 6)
    f = I.pairhmm64(*helpers.hmm_args(pairs, O.pairhmm_params))
    assert f.min() >= 2e-220
    g = np.array([forward64(p, 2.0 ** 1020) for p in pairs]) * 2.0 ** -900
    np.testing.assert_allclose(g, f, rtol=1e-12, atol=0)
