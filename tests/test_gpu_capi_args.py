"""The flat C API's argument checks (capi.cpp), called through ctypes on a real engine: which
return code and which gasalx_last_error() text each bad call gives, the order of the checks, the
calls that return early for an empty batch without touching their outputs, and the device forms
that read the lengths or offsets back when the caller passes zero maxima (bit-equal to the same
call with the true maxima).  The table's calls launch nothing."""
import ctypes as C

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import oracle as O

pytestmark = pytest.mark.gpu

OK, EINVAL, ERANGE, EUNSUPPORTED = 0, -1, -2, -5
NULLARG = "null argument"
BAND = "band length must be 2..32"
ENG = object()                       # stands for the engine's handle in a case's arguments
u32, u64, f32 = C.c_uint32, C.c_uint64, C.c_float
SENT = 0x5A

# host arrays the calls point at; OUT must come back as it is
SEQ = np.full(8, G.N_CODE, np.uint8)
Z32 = np.zeros(8, np.uint32)
LEN4 = np.full(2, 4, np.uint32)
F32 = np.zeros(8, np.float32)
OUT = np.full(256, SENT, np.uint8)
_keep = []


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def ref(s):
    return C.byref(s)


def offsets(*o):
    a = np.array(o, np.uint32)
    _keep.append(a)
    return ptr(a)


def params(**kw):
    return G.make_params(**kw)


def set_field(s, name, value):
    setattr(s, name, value)
    return s


def batch(n=0):
    return G.CBatch(ptr(SEQ), ptr(Z32), ptr(LEN4), ptr(SEQ), ptr(Z32), ptr(LEN4), 8, 8, n, None, None, None, 0, 0)


def results():
    return G.CResults(*([ptr(OUT)] * 10))


def hmm(n=0):
    return G.CHmmBatch(ptr(SEQ), ptr(Z32), ptr(LEN4), ptr(F32), ptr(F32), ptr(F32), ptr(F32), ptr(SEQ), ptr(Z32),
                       ptr(LEN4), 4, 4, n, 0, 0)


def hmmq(n=1):
    return G.CHmmQualBatch(ptr(SEQ), ptr(Z32), ptr(LEN4), ptr(SEQ), ptr(SEQ), ptr(SEQ), ptr(SEQ), ptr(Z32), ptr(LEN4),
                           4, 4, n, 0, 0)


def strings(off=None, bits=4, big=1):
    return G.CNvStrings(ptr(Z32), off if off is not None else offsets(0, 4), 0, bits, big)


def aligner(kind=G.NV_GOTOH, mag=2, type_=G.NV_GLOBAL):
    """an aligner whose largest |score| is mag"""
    return G.CNvAligner(kind, type_, mag, -1, -2, -1, -1, -1)


def matrix(n=4, entry=-1):
    """an n x n substitution table whose largest |entry| is |entry|"""
    a = np.full(n * n, entry, np.int8)
    _keep.append(a)
    return G.CNvMatrix(ptr(a), n)


def shared_text(length, bits=2):
    """one shared text: no offsets, its length in the struct"""
    return G.CNvStrings(ptr(Z32), None, length, bits, 0)


BATCH_ARRAYS = ("q_batch", "t_batch", "q_offsets", "t_offsets", "q_lens", "t_lens")
QUAL_ARRAYS = ("reads", "read_offsets", "read_lens", "base_quals", "ins_quals", "del_quals", "haps", "hap_offsets",
               "hap_lens")
STRING_ARRAYS = ((0, "words"), (0, "offsets"), (1, "words"))        # (pattern / text, field) the host forms need
o = ptr(OUT)


NV_SCORE = ("score", "score_sinks", "matrix_score", "banded_score", "banded_score_sinks", "banded_myers")
NV_TRACEBACK = ("traceback", "matrix_traceback", "banded_traceback")
NV_DEVICE = tuple(f"gasalx_nv_{f}_device" for f in NV_SCORE + NV_TRACEBACK)
NV_HOST = tuple(f"gasalx_nv_{f}_host" for f in NV_SCORE + NV_TRACEBACK)
NV_FIRST = ("score", "banded_score", "traceback", "banded_traceback")   # the pairs with loops of their own below


def nv_args(name, n=0, band=16, al=None, pat=None, txt=None, stride=64, mat=None, myers=(G.NV_SEMI_GLOBAL, 4),
            max_p=0, max_t=0):
    """the argument list of an nvbio entry point, and the positions of its pattern and text sets;
    myers: the Myers forms' (type, alphabet), which stand where the others have their aligner;
    max_p, max_t: the device forms' bounds"""
    device = name.endswith("device")
    family = name[len("gasalx_nv_"):].rsplit("_", 1)[0]
    pat, txt = ref(pat or strings()), ref(txt or strings(bits=2, big=0))
    b = (u32(band),) if "banded" in name else ()
    if family == "banded_myers":
        head = (ENG, C.c_int32(myers[0]), u32(myers[1])) + b + (u32(n),)
    else:
        head = (ENG, ref(al or aligner())) + ((ref(mat or matrix()),) if "matrix" in name else ()) + b + (u32(n),)
    at = len(head)
    sets = (pat, txt) if device else (pat, u64(1), txt, u64(1))
    at_txt = at + (1 if device else 2)
    maxima = ((u32(max_p),) if "banded" in name else (u32(max_p), u32(max_t))) if device else ()
    if "traceback" in name:
        tail = maxima + (o, o, o, o, u32(stride), o)
    elif family == "banded_score":
        tail = (o,) + maxima                                         # scores
    elif family == "score":
        tail = (o, None) + maxima                                    # scores, scores16
    else:
        tail = (o, o) + maxima                                       # scores, sinks
    args = head + sets + tail + ((None,) if device else ())
    return args, at, at_txt


def nv_structs(name, at, at_txt):
    """the positions of an nvbio entry point's engine, aligner (the Myers forms have none), matrix and
    string sets"""
    return [0] + ([] if "myers" in name else [1]) + ([2] if "matrix" in name else []) + [at, at_txt]


def nv_string_fields(name, args, at, at_txt):
    """one case per array of the two string sets that a host form needs"""
    c = []
    for which, field in STRING_ARRAYS:
        make = strings if which == 0 else (lambda: strings(bits=2, big=0))
        c += null_field(name, args, (at, at_txt)[which], make, (field,), tag=("patterns.", "texts.")[which])
    return c


def null_at(name, args, positions, msg=NULLARG):
    """one case per position: that argument NULL"""
    return [(f"{name}-arg{i}", name, args[:i] + (None,) + args[i + 1:], EINVAL, msg) for i in positions]


def null_field(name, args, i, make, fields, msg=NULLARG, tag=""):
    """one case per field: argument i a struct with that array NULL"""
    return [(f"{name}-{tag}{f}", name, args[:i] + (ref(set_field(make(), f, None)),) + args[i + 1:], EINVAL, msg)
            for f in fields]


def _null_cases():
    c = []
    P, buf = params(), C.create_string_buffer(128)
    # align
    dev = (ENG, ref(P), ref(batch()), ref(results()), None)
    c += null_at("gasalx_align_device", dev, (0, 1, 2, 3))
    c += null_at("gasalx_align_host", dev[:4], (0, 1, 2, 3))
    c += null_field("gasalx_align_host", dev[:4], 2, batch, BATCH_ARRAYS, "missing batch array")
    for field, value in (("algo", 7), ("algo", -1), ("start_pos", 3), ("head", 4), ("tail", 4)):
        bad = ref(set_field(params(), field, value))
        tag = f"{field}{value}"
        c.append((f"align_host-{tag}", "gasalx_align_host", (ENG, bad) + dev[2:4], EINVAL, NULLARG))
        c.append((f"align_device-{tag}", "gasalx_align_device", (ENG, bad) + dev[2:], EINVAL, NULLARG))
        c.append((f"describe_plan-{tag}", "gasalx_describe_plan", (bad, u32(100), u32(100), buf, u32(128)), EINVAL,
                  None))
    plan = (ref(P), u32(100), u32(100), buf, u32(128))
    c += null_at("gasalx_describe_plan", plan, (0, 3), None)
    c.append(("describe_plan-len0", "gasalx_describe_plan", plan[:4] + (u32(0),), EINVAL, None))
    # PairHMM, parameter form
    for name in ("gasalx_pairhmm_device", "gasalx_pairhmm64_device"):
        c += null_at(name, (ENG, ref(hmm()), o, None), (0, 1, 2))
    for name in ("gasalx_pairhmm_host", "gasalx_pairhmm64_host"):
        c += null_at(name, (ENG, ref(hmm()), o), (0, 1, 2))
    cnt = u32(7)
    c += null_at("gasalx_pairhmm_log10_device", (ENG, ref(hmm()), f32(0), o, o, None), (0, 1, 3))
    c += null_at("gasalx_pairhmm_log10_host", (ENG, ref(hmm()), f32(0), o, o, ref(cnt)), (0, 1, 3))
    # PairHMM, quality form: every array hmm_qual_batch_ok asks for
    for name, args, at in (
            ("gasalx_pairhmm_quals_device", (ENG, ref(hmmq()), o, None), (0, 1, 2)),
            ("gasalx_pairhmm_quals_host", (ENG, ref(hmmq()), o), (0, 1, 2)),
            ("gasalx_pairhmm64_quals_device", (ENG, ref(hmmq()), o, None), (0, 1, 2)),
            ("gasalx_pairhmm64_quals_host", (ENG, ref(hmmq()), o), (0, 1, 2)),
            ("gasalx_pairhmm_quals_log10_device", (ENG, ref(hmmq()), f32(0), o, o, None), (0, 1, 3)),
            ("gasalx_pairhmm_quals_log10_host", (ENG, ref(hmmq()), f32(0), o, o, ref(cnt)), (0, 1, 3))):
        c += null_at(name, args, at)
        c += null_field(name, args, 1, hmmq, QUAL_ARRAYS)
    # nvbio front-end
    for name in ("gasalx_nv_score_device", "gasalx_nv_banded_score_device", "gasalx_nv_traceback_device",
                 "gasalx_nv_banded_traceback_device"):
        args, at, at_txt = nv_args(name)
        c += null_at(name, args, (0, 1, at, at_txt))
    for name in ("gasalx_nv_score_host", "gasalx_nv_banded_score_host", "gasalx_nv_traceback_host",
                 "gasalx_nv_banded_traceback_host"):
        args, at, at_txt = nv_args(name)
        outs = [i for i, a in enumerate(args) if a is o]
        if name == "gasalx_nv_score_host":
            outs = []                                                # scores, scores16: one of them is enough
            c.append((f"{name}-both-scores", name, args[:-2] + (None, None), EINVAL, NULLARG))
        c += null_at(name, args, [0, 1, at, at_txt] + outs)
        for which, field in STRING_ARRAYS:
            make = strings if which == 0 else (lambda: strings(bits=2, big=0))
            c += null_field(name, args, (at, at_txt)[which], make, (field,), tag=("patterns.", "texts.")[which])
    # the pairs the two loops above leave out: sinks, matrix, banded sinks, Myers, matrix traceback
    for name in NV_DEVICE:
        if name[len("gasalx_nv_"):-len("_device")] in NV_FIRST:
            continue
        args, at, at_txt = nv_args(name)
        c += null_at(name, args, nv_structs(name, at, at_txt))
        if name == "gasalx_nv_matrix_traceback_device":              # the one device form that checks as a host form
            c += null_at(name, args, [i for i, a in enumerate(args) if a is o])
            c += nv_string_fields(name, args, at, at_txt)
    for name in NV_HOST:
        if name[len("gasalx_nv_"):-len("_host")] in NV_FIRST:
            continue
        args, at, at_txt = nv_args(name)
        outs = [i for i, a in enumerate(args) if a is o]
        if "traceback" not in name:                                   # scores, sinks: one of them is enough
            c.append((f"{name}-both-outputs", name, args[:-2] + (None, None), EINVAL, NULLARG))
            outs = []
        c += null_at(name, args, nv_structs(name, at, at_txt) + outs)
        c += nv_string_fields(name, args, at, at_txt)
    # A NULL table: the traceback forms' own checks refuse it; the score forms leave it to the launcher,
    # which an empty host batch never reaches.
    for name in ("gasalx_nv_matrix_score_device", "gasalx_nv_matrix_score_host", "gasalx_nv_matrix_traceback_device",
                 "gasalx_nv_matrix_traceback_host"):
        args = nv_args(name, mat=set_field(matrix(), "scores", None))[0]
        quiet = name == "gasalx_nv_matrix_score_host"
        c.append((f"{name}-matrix.scores", name, args, OK if quiet else EINVAL, None if quiet else NULLARG))
    # the five describe functions: NULL aligner (where there is one) and buffer, no room, one good call,
    # the inputs the three that can refuse do refuse, and the null test before them
    nvp = (ref(aligner()), u32(10), u32(10), C.c_int(0), u32(2), buf, u32(128))
    c += null_at("gasalx_nv_describe_plan", nvp, (0, 5))
    c.append(("nv_describe_plan-len0", "gasalx_nv_describe_plan", nvp[:6] + (u32(0),), EINVAL, NULLARG))
    al, sw = ref(aligner()), ref(aligner(G.NV_SW))
    msize, bits, alphabet = "matrix size must be 2..32", "symbol bits must be 2, 4 or 8", "alphabet size must be 2, 4 or 5"
    for short, good, nulls, bad in (
            ("sinks_plan", nvp, (0, 5), ()),
            ("matrix_plan", (al, u32(4), u32(10), u32(10), C.c_int(1), C.c_int(0), buf, u32(128)), (0, 6),
             (("n33", (al, u32(33)), EINVAL, msize), ("n1", (al, u32(1)), EINVAL, msize),
              ("type3", (ref(aligner(type_=3)),), EINVAL, "bad aligner"),
              ("sw", (sw,), EUNSUPPORTED, "only the Gotoh aligner takes a substitution matrix"))),
            ("banded_sinks_plan", (al, u32(16), u32(10), u32(2), buf, u32(128)), (0, 4),
             (("band33", (al, u32(33)), EINVAL, BAND), ("band1", (al, u32(1)), EINVAL, BAND),
              ("bits3", (al, u32(16), u32(10), u32(3)), EINVAL, bits))),
            ("myers_plan", (C.c_int32(G.NV_SEMI_GLOBAL), u32(4), u32(16), buf, u32(128)), (3,),
             (("type3", (C.c_int32(3),), EINVAL, "bad aligner"),
              ("band33", (C.c_int32(G.NV_GLOBAL), u32(4), u32(33)), EINVAL, BAND),
              ("alphabet3", (C.c_int32(G.NV_GLOBAL), u32(3)), EINVAL, alphabet),
              ("local", (C.c_int32(G.NV_LOCAL),), EUNSUPPORTED, "banded Myers has no LOCAL form")))):
        name = "gasalx_nv_describe_" + short
        c += null_at(name, good, nulls)
        c.append((f"nv_describe_{short}-len0", name, good[:-1] + (u32(0),), EINVAL, NULLARG))
        c.append((f"nv_describe_{short}-ok", name, good, OK, None))
        for tag, lead, rc, msg in bad:
            c.append((f"nv_describe_{short}-{tag}", name, lead + good[len(lead):], rc, msg))
            c.append((f"nv_describe_{short}-{tag}-len0", name, lead + good[len(lead):-1] + (u32(0),), EINVAL, NULLARG))
    c.append(("nv_describe_plan-ok", "gasalx_nv_describe_plan", nvp, OK, None))
    # the rest
    h, t = u64(0), u64(0)
    c += null_at("gasalx_packed_pairs", (ENG, ref(h), ref(t)), (0, 1, 2), "gasalx_packed_pairs: NULL argument")
    c.append(("host_alloc-out", "gasalx_host_alloc", (u64(16), None), EINVAL, "gasalx_host_alloc: null output"))
    c.append(("engine_create-out", "gasalx_engine_create", (C.c_int(0), None), EINVAL, None))
    c.append(("device_count-out", "gasalx_device_count", (None,), EINVAL, None))
    c.append(("engine_destroy-null", "gasalx_engine_destroy", (None,), OK, None))
    c += null_at("gasalx_pairhmm_params", (ptr(SEQ), ptr(SEQ), ptr(SEQ), u32(1), ptr(F32), ptr(F32), ptr(F32), ptr(F32)),
                 (0, 1, 2, 4, 5, 6, 7), None)
    return c


def _range_cases():
    """the traceback forms' checks, host forms with one pair described by its offsets alone: the
    checks run before anything is staged"""
    c = []

    def tb(tag, al, p, t, stride, rc, msg):
        args, _, _ = nv_args("gasalx_nv_traceback_host", n=1, al=al, pat=strings(offsets(0, p)),
                             txt=strings(offsets(0, t), bits=2, big=0), stride=stride)
        c.append((f"traceback-{tag}", "gasalx_nv_traceback_host", args, rc, msg))

    def btb(tag, al, band, p, stride, rc, msg, n=1):
        args, _, _ = nv_args("gasalx_nv_banded_traceback_host", n=n, band=band, al=al, pat=strings(offsets(0, p)),
                             txt=strings(offsets(0, p + band), bits=2, big=0), stride=stride)
        c.append((f"banded_traceback-{tag}", "gasalx_nv_banded_traceback_host", args, rc, msg))

    ed = aligner(G.NV_ED)
    # (max_p + max_t + 2) * |score|: 256 * 128 = 32768 is refused, 217 * 151 = 32767 passes on to the stride check
    tb("int16-above", aligner(mag=128), 127, 127, 254, ERANGE, "int16 columns")
    tb("int16-exact", aligner(mag=151), 100, 115, 214, EINVAL, "ops_stride < max pattern")
    tb("stride-short", aligner(), 100, 100, 199, EINVAL, "ops_stride < max pattern")
    # the stride check comes before the cell limit: 4096 x 4096 is within it, 4097 x 4097 is not
    tb("cells", ed, 4097, 4097, 8194, ERANGE, "16 M cells")
    tb("cells-4096-stride", ed, 4096, 4096, 8191, EINVAL, "ops_stride < max pattern")
    # (max_p + band + 3) * |score|: 1723 * 19 = 32737 is refused, 1023 * 32 = 32736 passes on to the stride check
    btb("int16-above", aligner(mag=19), 16, 1704, 2 * 1704 + 16, ERANGE, "int16 checkpoints")
    btb("int16-exact", aligner(mag=32), 16, 1004, 2 * 1004 + 15, EINVAL, "ops_stride < 2 x max pattern")
    btb("stride-short", aligner(), 16, 10, 2 * 10 + 15, EINVAL, "ops_stride < 2 x max pattern")
    # a bad band is refused even for an empty batch, by both banded host forms
    for band in (1, 33):
        for n in (0, 1):
            btb(f"band{band}-n{n}", aligner(), band, 10, 64, EINVAL, BAND, n=n)
            args, _, _ = nv_args("gasalx_nv_banded_score_host", n=n, band=band, pat=strings(offsets(0, 10)),
                                 txt=strings(offsets(0, 20), bits=2, big=0))
            c.append((f"banded_score-band{band}-n{n}", "gasalx_nv_banded_score_host", args, EINVAL, BAND))

    # the matrix traceback: gasalx_nv_traceback_host's rows, the table's largest |entry| (an int8) standing
    # for match and mismatch: 256 * 128 = 32768 is refused, 1057 * 31 = 32767 passes on to the stride check
    def mtb(tag, entry, p, t, stride, rc, msg):
        args, _, _ = nv_args("gasalx_nv_matrix_traceback_host", n=1, mat=matrix(entry=entry),
                             pat=strings(offsets(0, p)), txt=strings(offsets(0, t), bits=2, big=0), stride=stride)
        c.append((f"matrix_traceback-{tag}", "gasalx_nv_matrix_traceback_host", args, rc, msg))

    assert (127 + 127 + 2) * 128 == 32768 and (500 + 555 + 2) * 31 == 32767
    mtb("int16-above", -128, 127, 127, 254, ERANGE, "int16 columns")
    mtb("int16-exact", -31, 500, 555, 1054, EINVAL, "ops_stride < max pattern")
    mtb("stride-short", -1, 100, 100, 199, EINVAL, "ops_stride < max pattern")
    mtb("cells", -1, 4097, 4097, 8194, ERANGE, "16 M cells")
    mtb("cells-4096-stride", -1, 4096, 4096, 8191, EINVAL, "ops_stride < max pattern")
    return c


def _order_cases():
    """which checks come before the early return for an empty batch, entry point by entry point"""
    c = []
    pat10, txt20 = (lambda: strings(offsets(0, 10))), (lambda: strings(offsets(0, 20), bits=2, big=0))
    # both banded score host forms: the band (gasalx_nv_banded_score_host has its rows in _range_cases)
    name = "gasalx_nv_banded_score_sinks_host"
    for band in (1, 33):
        for n in (0, 1):
            args = nv_args(name, n=n, band=band, pat=pat10(), txt=txt20())[0]
            c.append((f"banded_score_sinks-band{band}-n{n}", name, args, EINVAL, BAND))
    # the Myers host form: nv_myers_plan_name's codes and texts
    name = "gasalx_nv_banded_myers_host"
    for tag, myers, band, rc, msg in (("type3", (3, 4), 16, EINVAL, "bad aligner"),
                                      ("band1", (G.NV_GLOBAL, 4), 1, EINVAL, BAND),
                                      ("band33", (G.NV_GLOBAL, 4), 33, EINVAL, BAND),
                                      ("alphabet3", (G.NV_GLOBAL, 3), 16, EINVAL, "alphabet size must be 2, 4 or 5"),
                                      ("local", (G.NV_LOCAL, 4), 16, EUNSUPPORTED, "banded Myers has no LOCAL form")):
        for n in (0, 1):
            args = nv_args(name, n=n, band=band, myers=myers, pat=pat10(), txt=txt20())[0]
            c.append((f"banded_myers-{tag}-n{n}", name, args, rc, msg))
    # the banded traceback host form: nv_btb_checks with a longest pattern of 0
    name = "gasalx_nv_banded_traceback_host"
    assert (0 + 16 + 3) * 1724 > 32736 >= (0 + 16 + 3) * 1722
    c.append(("banded_traceback-n0-int16", name, nv_args(name, al=aligner(mag=1724))[0], ERANGE, "int16 checkpoints"))
    c.append(("banded_traceback-n0-int16-below", name, nv_args(name, al=aligner(mag=1722))[0], OK, None))
    c.append(("banded_traceback-n0-stride", name, nv_args(name, stride=15)[0], EINVAL, "ops_stride < 2 x max pattern"))
    c.append(("banded_traceback-n0-stride-exact", name, nv_args(name, stride=16)[0], OK, None))
    # both matrix traceback forms: nv_mtb_checks (aligner, table size, table, symbol bits) in that order,
    # after the null test
    for name in ("gasalx_nv_matrix_traceback_host", "gasalx_nv_matrix_traceback_device"):
        short = name[len("gasalx_nv_"):]
        for tag, kw, rc, msg in (
                ("type3", lambda: dict(al=aligner(type_=3)), EINVAL, "bad aligner"),
                ("sw", lambda: dict(al=aligner(G.NV_SW)), EUNSUPPORTED, "only the Gotoh aligner takes a substitution matrix"),
                ("n1", lambda: dict(mat=matrix(1)), EINVAL, "matrix size must be 2..32"),
                ("n33", lambda: dict(mat=matrix(33)), EINVAL, "matrix size must be 2..32"),
                ("bits3", lambda: dict(pat=strings(bits=3)), EINVAL, "symbol bits must be 2, 4 or 8"),
                ("sw-n33", lambda: dict(al=aligner(G.NV_SW), mat=matrix(33)), EUNSUPPORTED, "only the Gotoh aligner"),
                ("n33-bits3", lambda: dict(mat=matrix(33), pat=strings(bits=3)), EINVAL, "matrix size must be 2..32")):
            for n in (0, 1):
                c.append((f"{short}-{tag}-n{n}", name, nv_args(name, n=n, **kw())[0], rc, msg))
        args = nv_args(name, al=aligner(G.NV_SW))[0]
        last = max(i for i, a in enumerate(args) if a is o)
        c.append((f"{short}-sw-null-output", name, args[:last] + (None,) + args[last + 1:], EINVAL, NULLARG))
    # The score device forms have no early return of their own.  The launcher's comes first in the two
    # full-DP score forms and after its checks in the others, which refuse an empty batch with a bad
    # band, alphabet or table size.
    for tag, name, kw, msg in (("band33", "gasalx_nv_banded_score_device", dict(band=33), BAND),
                               ("band33", "gasalx_nv_banded_score_sinks_device", dict(band=33), BAND),
                               ("band33", "gasalx_nv_banded_myers_device", dict(band=33), BAND),
                               ("alphabet3", "gasalx_nv_banded_myers_device", dict(myers=(G.NV_GLOBAL, 3)),
                                "alphabet size must be 2, 4 or 5"),
                               ("n33", "gasalx_nv_matrix_score_device", dict(mat=matrix(33)), "matrix size must be 2..32")):
        c.append((f"{name}-n0-{tag}", name, nv_args(name, **kw)[0], EINVAL, msg))
    for name in ("gasalx_nv_score_device", "gasalx_nv_score_sinks_device"):
        c.append((f"{name}-n0-type3", name, nv_args(name, al=aligner(type_=3))[0], OK, None))
    # Patterns without offsets and no bound: both banded score device forms skip the read-back, and the
    # launcher refuses the set.  (The banded traceback form has no such guard; no row calls it that way.)
    for name in ("gasalx_nv_banded_score_device", "gasalx_nv_banded_score_sinks_device"):
        args = nv_args(name, n=1, pat=set_field(strings(), "offsets", None))[0]
        c.append((f"{name}-no-offsets", name, args, EINVAL, NULLARG))
    # One shared text: the full-DP traceback device forms take its length, not the caller's max_t.
    # 100 + 100 + 2 at |score| 163 leaves the int16 range; with the caller's 5 it would not, and the
    # call would be refused for its stride instead.
    assert (100 + 100 + 2) * 163 > 32767 >= (100 + 5 + 2) * 163
    for name in ("gasalx_nv_traceback_device", "gasalx_nv_matrix_traceback_device"):
        gap = G.CNvAligner(G.NV_GOTOH, G.NV_GLOBAL, 1, -1, -163, -1, -1, -1)
        args = nv_args(name, n=1, al=gap, txt=shared_text(100), max_p=100, max_t=5, stride=104)[0]
        c.append((f"{name}-shared-text-length", name, args, ERANGE, "int16 columns"))
    return c


def _empty_cases():
    """n = 0: the forms that return OK before they look further"""
    c = []
    for name in ("gasalx_pairhmm_quals_host", "gasalx_pairhmm64_quals_host"):
        c.append((f"{name}-n0", name, (ENG, ref(hmmq(0)), o), OK, None))
    c.append(("gasalx_pairhmm64_host-n0", "gasalx_pairhmm64_host", (ENG, ref(hmm(0)), o), OK, None))
    c.append(("log10_device-n0", "gasalx_pairhmm_log10_device", (ENG, ref(hmm(0)), f32(0), o, o, None), OK, None))
    c.append(("quals_log10_device-n0", "gasalx_pairhmm_quals_log10_device", (ENG, ref(hmmq(0)), f32(0), o, o, None),
              OK, None))
    for name in ("gasalx_nv_score_host", "gasalx_nv_banded_score_host", "gasalx_nv_traceback_device",
                 "gasalx_nv_traceback_host", "gasalx_nv_banded_traceback_device", "gasalx_nv_banded_traceback_host"):
        c.append((f"{name}-n0", name, nv_args(name)[0], OK, None))
    # The device forms do not check their output pointers, they hand them to the kernels: a NULL one
    # is no argument error, so the NULL-in-turn table leaves them out.  The two traceback device forms
    # return for an empty batch before they look at them:
    for name in ("gasalx_nv_traceback_device", "gasalx_nv_banded_traceback_device"):
        args = tuple(None if a is o else a for a in nv_args(name)[0])
        c.append((f"{name}-n0-null-outputs", name, args, OK, None))
    # every other nv entry point returns OK for an empty batch as well
    done = {case[1] for case in c}
    for name in NV_DEVICE + NV_HOST:
        if name not in done:
            c.append((f"{name}-n0", name, nv_args(name)[0], OK, None))
    # the score device forms: NULL outputs reach the launcher, which returns for an empty batch
    for name in NV_DEVICE[:len(NV_SCORE)]:
        args = tuple(None if a is o else a for a in nv_args(name)[0])
        c.append((f"{name}-n0-null-outputs", name, args, OK, None))
    # two outputs of which one is enough: either alone
    for name in NV_HOST[:len(NV_SCORE)]:
        if name != "gasalx_nv_banded_score_host":
            args = nv_args(name)[0]
            c.append((f"{name}-n0-first-output-only", name, args[:-1] + (None,), OK, None))
            c.append((f"{name}-n0-second-output-only", name, args[:-2] + (None, o), OK, None))
    return c


CASES = _null_cases() + _range_cases() + _order_cases() + _empty_cases()


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


def call(engine, name, args):
    lib = G.lib()
    lib.gasalx_host_alloc(u64(0), None)          # a known message first: an earlier case's text cannot pass for this one's
    rc = getattr(lib, name)(*[engine._h if a is ENG else a for a in args])
    return rc, lib.gasalx_last_error().decode()


def test_case_ids_unique():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) and len(ids) > 200


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_check(engine, case):
    _, name, args, want, msg = case
    rc, text = call(engine, name, args)
    assert rc == want, (name, rc, text)
    if msg is not None:
        assert msg in text, (name, text)
    assert (OUT == SENT).all(), f"{name} wrote to an output"


@pytest.mark.parametrize("name,make", [("gasalx_pairhmm_log10_host", hmm), ("gasalx_pairhmm_quals_log10_host", hmmq)])
def test_log10_host_clears_count_first(engine, name, make):
    cnt = u32(7)
    rc, text = call(engine, name, (ENG, ref(make(0)), f32(0), o, o, ref(cnt)))
    assert rc == OK and cnt.value == 0, (rc, text)
    assert (OUT == SENT).all()


def test_traceback_at_the_int16_bound(engine):
    """100 x 100 with |score| 162: 202 * 162 <= 32767 < 202 * 163; the call passes the check and runs"""
    assert 202 * 162 <= 32767 < 202 * 163
    rng = np.random.default_rng(0xA162)
    p = rng.integers(0, 4, 100)
    t = p.copy()
    t[rng.random(100) < 0.1] = rng.integers(0, 4)
    P = G.PackedSet.pack([p])
    T = G.PackedSet.pack([t], bits=2, big_endian=False)
    al = G.NvAligner(G.NV_GOTOH, G.NV_GLOBAL, 162, -1, -2, -1)
    g, ref_ = engine.nv_traceback_host(al, P, T), O.nv_traceback(al, P, T)
    assert np.array_equal(g["score"], ref_["score"])
    assert np.array_equal(g["source"], ref_["source"]) and np.array_equal(g["sink"], ref_["sink"])
    assert np.array_equal(g["ops"][0], ref_["ops"][0])
    with pytest.raises(RuntimeError, match="int16 columns"):
        engine.nv_traceback_host(G.NvAligner(G.NV_GOTOH, G.NV_GLOBAL, 163, -1, -2, -1), P, T)


# ---- zero maxima: the device forms read the lengths (or offsets) back ----
# 33 pairs, lengths 1 to 40.  gasalx_nv_traceback_device and gasalx_nv_banded_traceback_device have
# their case in test_gpu_nvbio.py::test_traceback_device_entry[full-readback] / [banded-readback].
N = 33


def _lens(rng):
    a = rng.integers(1, 41, N)
    a[0], a[1] = 1, 40
    return a


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to("cuda:0")


def test_align_device_reads_lengths_back(engine):
    import torch
    rng = np.random.default_rng(0xA11)
    b = G.Batch.from_pairs([helpers.random_seq(rng, int(k)) for k in _lens(rng)],
                           [helpers.random_seq(rng, int(k)) for k in _lens(rng)])
    d = {k: _dev(getattr(b, a)) for k, a in (("q_batch", "q_data"), ("t_batch", "t_data"), ("q_offsets", "q_offsets"),
                                             ("t_offsets", "t_offsets"), ("q_lens", "q_lens"), ("t_lens", "t_lens"))}
    got = []
    for mq, mt in ((0, 0), (int(b.q_lens.max()), int(b.t_lens.max()))):
        outs = {f: torch.full((N,), -77, dtype=torch.int32, device="cuda:0") for f in ("aln_score", "q_end", "t_end")}
        torch.cuda.synchronize()
        engine.align_device_ptrs(params(algo=G.LOCAL), {k: v.data_ptr() for k, v in {**d, **outs}.items()}, b.q_bytes,
                                 b.t_bytes, N, mq, mt)
        torch.cuda.synchronize()
        got.append(np.stack([outs[f].cpu().numpy() for f in outs]))
    assert (got[1][0] > 0).any() and np.array_equal(got[0], got[1])


HMM_DEVICE = [("gasalx_pairhmm_device", False, np.float32, False), ("gasalx_pairhmm_quals_device", True, np.float32, False),
              ("gasalx_pairhmm64_device", False, np.float64, False),
              ("gasalx_pairhmm64_quals_device", True, np.float64, False),
              ("gasalx_pairhmm_log10_device", False, np.float64, True),
              ("gasalx_pairhmm_quals_log10_device", True, np.float64, True)]


@pytest.mark.parametrize("name,quals,dtype,log10", HMM_DEVICE, ids=[h[0] for h in HMM_DEVICE])
def test_pairhmm_device_reads_lengths_back(engine, name, quals, dtype, log10):
    import torch
    rng = np.random.default_rng(0xA12)
    pairs = []
    for R, H in zip(_lens(rng), _lens(rng)):
        hap = helpers.random_seq(rng, int(H)).decode()
        pairs.append(dict(read=helpers.hmm_related_read(rng, hap, int(R)), hap=hap, bq=rng.integers(10, 41, R),
                          iq=rng.integers(10, 26, R), dq=rng.integers(10, 60, R)))
    reads, ro, rl, qm, de, xi, al, haps, ho, hl = helpers.hmm_args(pairs, O.pairhmm_params)
    if quals:
        h = G.HmmData.from_pairs(pairs)
        t = [_dev(a) for a in (h.reads, h.read_offsets, h.read_lens, h.base_quals, h.ins_quals, h.del_quals, h.haps,
                               h.hap_offsets, h.hap_lens)]
        make = lambda mr, mh: G.CHmmQualBatch(*[x.data_ptr() for x in t], len(h.reads), len(h.haps), N, mr, mh)
    else:
        t = [_dev(a) for a in (reads, ro, rl, qm, de, xi, al, haps, ho, hl)]
        make = lambda mr, mh: G.CHmmBatch(*[x.data_ptr() for x in t], len(reads), len(haps), N, mr, mh)
    got = []
    for mr, mh in ((0, 0), (int(rl.max()), int(hl.max()))):
        out = torch.full((N,), -1.0, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda:0")
        used = torch.full((N,), 9, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        b = make(mr, mh)
        args = (ENG, ref(b)) + ((f32(0), C.c_void_p(out.data_ptr()), C.c_void_p(used.data_ptr())) if log10 else
                                (C.c_void_p(out.data_ptr()),)) + (None,)
        rc, text = call(engine, name, args)
        assert rc == OK, text
        torch.cuda.synchronize()
        got.append((out.cpu().numpy(), used.cpu().numpy()))
    assert (got[1][0] != -1.0).all()
    assert np.array_equal(got[0][0].view(np.uint8), got[1][0].view(np.uint8)) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("banded", [False, True], ids=["nv_score_device", "nv_banded_score_device"])
def test_nv_score_device_reads_offsets_back(engine, banded):
    import torch
    rng = np.random.default_rng(0xA13)
    pl = _lens(rng)
    P = G.PackedSet.pack([rng.integers(0, 4, int(k)) for k in pl])
    tl = pl + 15 if banded else _lens(rng)
    T = G.PackedSet.pack([rng.integers(0, 4, int(k)) for k in tl], bits=2, big_endian=False)
    al = G.NvAligner(G.NV_GOTOH, G.NV_SEMI_GLOBAL if banded else G.NV_LOCAL, 2, -1, -2, -1)
    keep = [_dev(P.words), _dev(P.offsets), _dev(T.words), _dev(T.offsets)]
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    pat, txt = mk(P, keep[0], keep[1]), mk(T, keep[2], keep[3])
    got = []
    for mp, mt in ((0, 0), (int(pl.max()), int(tl.max()))):
        sc = torch.full((N,), -77, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        if banded:
            engine.nv_banded_score_device_ptrs(al, 16, N, pat, txt, sc.data_ptr(), max_pattern_len=mp)
        else:
            engine.nv_score_device_ptrs(al, N, pat, txt, sc.data_ptr(), max_pattern_len=mp, max_text_len=mt)
        torch.cuda.synchronize()
        got.append(sc.cpu().numpy())
    assert (got[1] != -77).all() and np.array_equal(got[0], got[1])
