// capi.cpp — extern "C" flat API (include/gasalx.h) over the engine.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "engine.hpp"
#include "gasalx.h"

// One stage of the host-staged pipeline (gasalx_align_host on large batches):
// its own stream, workspace and device copies of one chunk of pairs.
enum SlotBuf { S_Q, S_T, S_META, S_CIG, S_COUNT };
struct HostSlot {
    hipStream_t st = nullptr;
    gx::Workspace ws;
    gx::DevBuf buf[S_COUNT];
    std::vector<uint8_t> hmeta;   // host image of the chunk's per-pair region (S_META)
    void release() {
        ws.release_all();
        for (gx::DevBuf &b : buf) b.release();
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
    }
};

// The engine's device buffers outside its workspaces, by role.  A buffer exists in this list and
// nowhere else: gasalx_engine::release() walks the array.  No buffer serves two roles: the ones
// marked "device forms" are still in use on the caller's stream after the call has returned, so a
// host form's staging must never land in them.
enum Buf {
    // gasalx_align_host, single shot: the batch, then the ten result fields in gasalx_results order
    B_Q, B_T, B_QO, B_TO, B_QL, B_TL, B_QOP, B_TOP, B_SEED, B_OUT, B_OUT_LAST = B_OUT + 9,
    // PairHMM host forms: the batch in either input form, the slot order, the results
    B_READS, B_RO, B_RL, B_QM, B_DE, B_XI, B_AL, B_HAPS, B_HO, B_HL, B_BQ, B_IQ, B_DQ, B_PERM,
    B_RES, B_RES64, B_USED,
    // PairHMM, device forms too: the ph2pr table, the log10 calls' fp32 results and their rescue
    // list (its count in the first of four words, then one word per pair)
    B_PH2PR, B_HM_R32, B_HM_LIST,
    // nvbio host forms: the two string sets, the outputs
    B_NV_PW, B_NV_PO, B_NV_TW, B_NV_TO, B_NV_S, B_NV_S16, B_NV_SRC, B_NV_SNK, B_NV_OPS, B_NV_NOPS,
    // nvbio traceback, device forms too: flags of every cell, one DP row per pair
    B_NV_DIR, B_NV_ROW,
    // nvbio quality host forms: one quality byte per pattern symbol
    B_NV_Q,
    B_COUNT
};

struct gasalx_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    gx::Workspace ws;
    HostSlot slot[2];
    gx::DevBuf buf[B_COUNT];
    void release() {
        ws.release_all();
        for (HostSlot &s : slot) s.release();
        for (gx::DevBuf &b : buf) b.release();
    }
};

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e__ = (x);                                                        \
        if (e__ != hipSuccess) {                                                     \
            gx::set_error(std::string(#x) + ": " + hipGetErrorString(e__));          \
            return e__ == hipErrorOutOfMemory ? GASALX_ENOMEM : GASALX_EDEVICE;      \
        }                                                                            \
    } while (0)

hipStream_t gx::engine_stream(gasalx_engine *e) { return e->stream; }

namespace {

// Every engine call starts here, after its own argument checks: the engine's device becomes
// current, and the call runs on the caller's stream or, without one (every host form), the engine's.
int enter(gasalx_engine *eng, void *stream, hipStream_t *st) {
    CK(hipSetDevice(eng->device));
    *st = stream ? (hipStream_t)stream : eng->stream;
    return GASALX_OK;
}

// Every host form ends here: rc is what its launches returned, back the results to copy out.
// A host form synchronises on an error too: its staging buffers are reused by the next call, which
// must not overwrite what this call's queued copies and kernels still read.  The device forms
// return an error as it is: the caller owns the stream and decides when to wait for it.
struct Back { void *host; const void *dev; size_t bytes; };
int host_finish(hipStream_t st, int rc, std::initializer_list<Back> back) {
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    for (const Back &b : back)
        if (b.host) CK(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    return GASALX_OK;
}

uint32_t host_max(const uint32_t *a, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) m = std::max(m, a[i]);
    return m;
}

// max over i of off[i+1] - off[i]
uint32_t max_span(const uint32_t *off, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) m = std::max(m, off[i + 1] - off[i]);
    return m;
}

// The maxima of a device batch's two length arrays where the caller left one of them zero: both
// read back (synchronises `st`).
int device_max_lens(const uint32_t *dq, const uint32_t *dt, uint32_t n, hipStream_t st, uint32_t *mq, uint32_t *mt) {
    if ((*mq && *mt) || !n) return GASALX_OK;
    std::vector<uint32_t> hq(n), ht(n);
    CK(hipMemcpyAsync(hq.data(), dq, n * 4ull, hipMemcpyDeviceToHost, st));
    CK(hipMemcpyAsync(ht.data(), dt, n * 4ull, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    *mq = host_max(hq.data(), n);
    *mt = host_max(ht.data(), n);
    return GASALX_OK;
}

// The same for device string sets: the offsets read back (synchronises `st`) where *max_p is zero
// or, with txt (per-pair texts that have a bound to give), *max_t is.
int device_max_spans(const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, uint32_t n, hipStream_t st,
                     uint32_t *max_p, uint32_t *max_t) {
    const bool texts = txt && txt->offsets;
    if (!n || (*max_p && !(texts && !*max_t))) return GASALX_OK;
    std::vector<uint32_t> po(n + 1), to(texts ? n + 1 : 0);
    CK(hipMemcpyAsync(po.data(), pat->offsets, (n + 1) * 4ull, hipMemcpyDeviceToHost, st));
    if (texts) CK(hipMemcpyAsync(to.data(), txt->offsets, (n + 1) * 4ull, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    if (!*max_p) *max_p = max_span(po.data(), n);
    if (texts && !*max_t) *max_t = max_span(to.data(), n);
    return GASALX_OK;
}

template <class T>
int stage_in(gx::DevBuf &d, const T *h, size_t count, hipStream_t st, T **dptr) {
    *dptr = nullptr;
    if (!h) return GASALX_OK;
    CK(d.reserve(count * sizeof(T) + 16));
    CK(hipMemcpyAsync(d.p, h, count * sizeof(T), hipMemcpyHostToDevice, st));
    *dptr = d.as<T>();
    return GASALX_OK;
}

// Stages the arrays of a host batch into the engine's buffers: in(buffer, field, count) replaces
// the host pointer in `field` by its device copy (NULL stays NULL).  After a failure the remaining
// calls do nothing and rc holds the code.
struct Stager {
    gasalx_engine *eng;
    hipStream_t st;
    int rc = GASALX_OK;
    template <class T>
    void operator()(Buf b, const T *&field, size_t count) {
        T *d = nullptr;
        if (!rc) rc = stage_in(eng->buf[b], field, count, st, &d);
        field = d;
    }
};

// The three input forms, staged: db (dp, dt) = the device image of the host batch.
// PairHMM parameter form; max_read_len / max_hap_len filled in.
int hmm_stage_host(gasalx_engine *eng, const gasalx_hmm_batch *hb, hipStream_t st, gasalx_hmm_batch &db) {
    const uint32_t n = hb->n_pairs;
    db = *hb;
    Stager in{eng, st};
    in(B_READS, db.reads, hb->read_bytes);
    in(B_RO, db.read_offsets, n);
    in(B_RL, db.read_lens, n);
    in(B_QM, db.qm, hb->read_bytes);
    in(B_DE, db.delta, hb->read_bytes);
    in(B_XI, db.xiksi, hb->read_bytes);
    in(B_AL, db.alpha, hb->read_bytes);
    in(B_HAPS, db.haps, hb->hap_bytes);
    in(B_HO, db.hap_offsets, n);
    in(B_HL, db.hap_lens, n);
    if (in.rc) return in.rc;
    db.max_read_len = hb->max_read_len ? hb->max_read_len : host_max(hb->read_lens, n);
    db.max_hap_len = hb->max_hap_len ? hb->max_hap_len : host_max(hb->hap_lens, n);
    return GASALX_OK;
}

// PairHMM quality form; the maxima stay the caller's.
int hmm_stage_quals(gasalx_engine *eng, const gasalx_hmm_qual_batch *hb, hipStream_t st, gasalx_hmm_qual_batch &db) {
    const uint32_t n = hb->n_pairs;
    db = *hb;
    Stager in{eng, st};
    in(B_READS, db.reads, hb->read_bytes);
    in(B_BQ, db.base_quals, hb->read_bytes);
    in(B_IQ, db.ins_quals, hb->read_bytes);
    in(B_DQ, db.del_quals, hb->read_bytes);
    in(B_RO, db.read_offsets, n);
    in(B_RL, db.read_lens, n);
    in(B_HAPS, db.haps, hb->hap_bytes);
    in(B_HO, db.hap_offsets, n);
    in(B_HL, db.hap_lens, n);
    return in.rc;
}

// nvbio string pair: patterns and texts (one shared text has no offsets) as a host form takes them,
// and their device image with the longest pattern and text (a shared text's length).
struct NvHostIn { uint32_t n; const gasalx_nv_strings *pat; uint64_t pat_words; const gasalx_nv_strings *txt; uint64_t txt_words; };
struct NvStaged { gasalx_nv_strings pat, txt; uint32_t max_p, max_t; };
void nv_host_spans(const NvHostIn &h, NvStaged &s) {
    s.max_p = max_span(h.pat->offsets, h.n);
    s.max_t = h.txt->offsets ? max_span(h.txt->offsets, h.n) : h.txt->length;
}
int nv_stage_strings(gasalx_engine *eng, const NvHostIn &h, hipStream_t st, NvStaged &s) {
    s.pat = *h.pat;
    s.txt = *h.txt;
    Stager in{eng, st};
    in(B_NV_PW, s.pat.words, h.pat_words);
    in(B_NV_PO, s.pat.offsets, (size_t)h.n + 1);
    in(B_NV_TW, s.txt.words, h.txt_words);
    in(B_NV_TO, s.txt.offsets, (size_t)h.n + 1);
    return in.rc;
}

// the quality bytes of a host batch (one per pattern symbol, offsets[n] of them) as a device array;
// the tables stay the caller's host arrays
int nv_stage_quals(gasalx_engine *eng, const NvHostIn &h, const gasalx_nv_quals *q, hipStream_t st, gasalx_nv_quals &dq) {
    dq = *q;
    const size_t bytes = h.pat->offsets[h.n];
    if (!bytes) {   // a batch of empty patterns: a pointer the kernels never read through
        CK(eng->buf[B_NV_Q].reserve(16));
        dq.quals = eng->buf[B_NV_Q].as<uint8_t>();
        return GASALX_OK;
    }
    Stager in{eng, st};
    in(B_NV_Q, dq.quals, bytes);
    return in.rc;
}

bool valid_params(const gasalx_params *p) {
    if (!p) return false;
    if (p->algo < 0 || p->algo > 6) return false;
    if (p->start_pos < 0 || p->start_pos > 2) return false;
    if (p->head < 0 || p->head > 3 || p->tail < 0 || p->tail > 3) return false;
    return true;
}

// gasalx_results as a table: field f is the struct's f-th pointer.  Every field holds one 4-byte
// entry per pair but cigar, whose q_bytes bytes sit at the pairs' query offsets.  The single-shot
// path stages field f in buffer B_OUT + f; a pipelined chunk lays the per-pair fields out as
// columns in this order.  The fields' types differ (int32_t *, uint8_t *, uint32_t *), so one array
// of member pointers cannot name them all; the pointers are read and written as bytes instead
// (memcpy, so no object is accessed through another pointer type), and the copies move bytes.
constexpr int kFields = 10, kCigar = 8, kNops = 9;
static_assert(sizeof(gasalx_results) == kFields * sizeof(void *) && offsetof(gasalx_results, cigar) == kCigar * sizeof(void *) &&
                  offsetof(gasalx_results, n_cigar_ops) == kNops * sizeof(void *) && B_OUT_LAST - B_OUT + 1 == kFields,
              "gasalx_results: ten pointers");
void *get_field(const gasalx_results &r, int f) {
    void *p;
    std::memcpy(&p, reinterpret_cast<const char *>(&r) + f * sizeof(void *), sizeof(p));
    return p;
}
void set_field(gasalx_results &r, int f, void *p) {
    std::memcpy(reinterpret_cast<char *>(&r) + f * sizeof(void *), &p, sizeof(p));
}
size_t field_bytes(int f, uint32_t n, uint32_t q_bytes) { return f == kCigar ? q_bytes : (size_t)n * 4; }

// Sequences laid out back to back from offset 0 (what gasal_host_batch_fill
// produces): chunks of pairs then own contiguous byte ranges.
bool contiguous(const uint32_t *off, const uint32_t *len, uint32_t n, uint32_t bytes) {
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (off[i] != at) return false;
        at += gx::pad8(len[i]);
    }
    return at == bytes;
}

// Large host batches: chunks of pairs alternate between two streams, so the
// H2D copy of chunk k+1 overlaps the kernels of chunk k (the copies run at
// PCIe speed from pageable memory on this platform, tools/h2d_probe.cpp).
// Per chunk: two sequence copies plus ONE copy of everything per-pair
// (rebased offsets, lengths, ops, seeds, the caller's output contents) and
// ONE copy back of the per-pair outputs.  mq, mt: the batch's maximum lengths.
int align_host_pipelined(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *hb,
                         const gasalx_results *ho, uint32_t chunk, bool tb, uint32_t mq, uint32_t mt) {
    const uint32_t n = hb->n_alns;
    // the caller's per-pair result fields, one column each: all but cigar (the slot's own buffer,
    // copied on its own), n_cigar_ops only with traceback
    uint8_t *hcol[kFields];
    for (int f = 0; f < kFields; f++)
        hcol[f] = (f == kCigar || (f == kNops && !tb)) ? nullptr : static_cast<uint8_t *>(get_field(*ho, f));
    // outputs every kernel of the algorithm writes (generic.hpp, wavefront*.hpp):
    // the score for all aligning algos, the ends for all but GLOBAL
    const bool ends = params->algo == 2 || params->algo == 3 || params->algo == 5 || params->algo == 6;
    const bool aligns = ends || params->algo == 1;   // UNKNOWN / MICROLOCAL launch nothing
    const bool written[kFields] = {aligns, ends, ends};
    for (HostSlot &s : eng->slot) {
        if (!s.st) CK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
        s.ws.device = eng->device;
    }
    // per-pair region of a chunk of m pairs: 4-byte columns, 16-byte aligned
    auto col = [](uint32_t m) { return ((size_t)m * 4 + 15) & ~(size_t)15; };
    auto bcol = [](uint32_t m) { return ((size_t)m + 15) & ~(size_t)15; };
    struct Pending { uint32_t i0, i1; uint64_t qlo, qhi; size_t out_at, out_len; bool live; } pend[2] = {};
    auto drain = [&](int k) -> int {   // the slot's previous chunk: results back to the caller
        Pending &pp = pend[k];
        if (!pp.live) return GASALX_OK;
        HostSlot &s = eng->slot[k];
        const uint32_t m = pp.i1 - pp.i0;
        if (pp.out_len)
            CK(hipMemcpyAsync(s.hmeta.data() + pp.out_at, s.buf[S_META].as<uint8_t>() + pp.out_at, pp.out_len,
                              hipMemcpyDeviceToHost, s.st));
        if (tb && ho->cigar)
            CK(hipMemcpyAsync(ho->cigar + pp.qlo, s.buf[S_CIG].p, pp.qhi - pp.qlo, hipMemcpyDeviceToHost, s.st));
        CK(hipStreamSynchronize(s.st));
        size_t at = pp.out_at;
        for (int f = 0; f < kFields; f++)
            if (hcol[f]) { std::memcpy(hcol[f] + pp.i0 * 4ull, s.hmeta.data() + at, m * 4ull); at += col(m); }
        pp.live = false;
        return GASALX_OK;
    };
    int rc = GASALX_OK, k = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += chunk, k ^= 1) {
        const uint32_t i1 = std::min(n, i0 + chunk), m = i1 - i0;
        HostSlot &s = eng->slot[k];
        if ((rc = drain(k))) return rc;
        const uint64_t qlo = hb->q_offsets[i0], qhi = (uint64_t)hb->q_offsets[i1 - 1] + gx::pad8(hb->q_lens[i1 - 1]);
        const uint64_t tlo = hb->t_offsets[i0], thi = (uint64_t)hb->t_offsets[i1 - 1] + gx::pad8(hb->t_lens[i1 - 1]);
        // host image of the per-pair region
        size_t at = 0;
        const size_t a_qo = at; at += col(m);
        const size_t a_to = at; at += col(m);
        const size_t a_ql = at; at += col(m);
        const size_t a_tl = at; at += col(m);
        const size_t a_qop = at; if (hb->q_ops) at += bcol(m);
        const size_t a_top = at; if (hb->t_ops) at += bcol(m);
        const size_t a_seed = at; if (hb->seed_scores) at += col(m);
        const size_t out_at = at;
        size_t a_out[kFields];
        for (int f = 0; f < kFields; f++) { a_out[f] = at; if (hcol[f]) at += col(m); }
        const size_t total = at;
        s.hmeta.resize(total);
        uint8_t *h = s.hmeta.data();
        uint32_t *qo = reinterpret_cast<uint32_t *>(h + a_qo), *to = reinterpret_cast<uint32_t *>(h + a_to);
        for (uint32_t i = 0; i < m; i++) {
            qo[i] = hb->q_offsets[i0 + i] - (uint32_t)qlo;
            to[i] = hb->t_offsets[i0 + i] - (uint32_t)tlo;
        }
        std::memcpy(h + a_ql, hb->q_lens + i0, m * 4ull);
        std::memcpy(h + a_tl, hb->t_lens + i0, m * 4ull);
        if (hb->q_ops) std::memcpy(h + a_qop, hb->q_ops + i0, m);
        if (hb->t_ops) std::memcpy(h + a_top, hb->t_ops + i0, m);
        if (hb->seed_scores) std::memcpy(h + a_seed, hb->seed_scores + i0, m * 4ull);
        // the caller's contents, so fields the reference does not write come back
        // unchanged; fields every kernel of this algo writes need no copy in
        for (int f = 0; f < kFields; f++)
            if (hcol[f] && !written[f]) std::memcpy(h + a_out[f], hcol[f] + i0 * 4ull, m * 4ull);
        CK(s.buf[S_META].reserve(total + 16));
        uint8_t *dm = s.buf[S_META].as<uint8_t>();
        uint8_t *p8;
        // isPacked (score-only): the caller's pages hold 4-bit words, half the bytes of the
        // unpacked units that offsets and q_bytes count (pack_rc_seqs.h:24-31); only those move
        const uint64_t pk = params->is_packed ? 2 : 1;
        if ((rc = stage_in(s.buf[S_Q], hb->q_batch + qlo / pk, (qhi - qlo) / pk, s.st, &p8))) return rc;
        gasalx_batch db = *hb;
        db.q_batch = p8;
        if ((rc = stage_in(s.buf[S_T], hb->t_batch + tlo / pk, (thi - tlo) / pk, s.st, &p8))) return rc;
        db.t_batch = p8;
        CK(hipMemcpyAsync(dm, h, total, hipMemcpyHostToDevice, s.st));
        db.q_offsets = reinterpret_cast<uint32_t *>(dm + a_qo);
        db.t_offsets = reinterpret_cast<uint32_t *>(dm + a_to);
        db.q_lens = reinterpret_cast<uint32_t *>(dm + a_ql);
        db.t_lens = reinterpret_cast<uint32_t *>(dm + a_tl);
        db.q_ops = hb->q_ops ? dm + a_qop : nullptr;
        db.t_ops = hb->t_ops ? dm + a_top : nullptr;
        db.seed_scores = hb->seed_scores ? reinterpret_cast<uint32_t *>(dm + a_seed) : nullptr;
        db.q_bytes = (uint32_t)(qhi - qlo);
        db.t_bytes = (uint32_t)(thi - tlo);
        db.n_alns = m;
        db.max_q_len = mq;
        db.max_t_len = mt;
        gasalx_results dout;
        for (int f = 0; f < kFields; f++) set_field(dout, f, hcol[f] ? dm + a_out[f] : nullptr);
        if (tb && ho->cigar) {
            CK(s.buf[S_CIG].reserve(qhi - qlo + 16));
            dout.cigar = s.buf[S_CIG].as<uint8_t>();
        }
        gx::BatchShape shape;
        shape.max_q = mq;
        shape.max_t = mt;
        shape.sort = gx::uneven_lengths(*params, hb->q_lens + i0, hb->t_lens + i0, m);
        shape.one_t8 = gx::one_pad8(hb->t_lens + i0, m, shape.max_t);
        shape.tb_split = false;   // the two slots' streams already overlap one chunk's walk with the next DP
        if ((rc = gx::align_device(s.ws, *params, db, dout, s.st, shape))) {
            for (HostSlot &x : eng->slot) (void)hipStreamSynchronize(x.st);
            return rc;
        }
        pend[k] = {i0, i1, qlo, qhi, out_at, total - out_at, true};
    }
    for (int j = 0; j < 2; j++) {
        k ^= 1;
        if ((rc = drain(k))) return rc;
    }
    return GASALX_OK;
}

// gasalx_semi_cigar_* and gasalx_semi_cigar_head_* (heads: any HEAD, its own message prefix): the argument
// checks, one text each, in this order.  b / out NULL (the describe
// call): the checks on the parameters only.
bool ranges_overlap(const void *a, uint64_t an, const void *b, uint64_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}
int semi_cigar_checks(const gasalx_params *p, const gasalx_batch *b, const gasalx_results *out, bool heads) {
    const std::string call = heads ? "semi_cigar_head: " : "semi_cigar: ";
    static const char *const src[] = {"NONE", "QUERY", "TARGET", "BOTH"};
    if (p->algo != 2) { gx::set_error(call + "algo must be SEMI_GLOBAL"); return GASALX_EINVAL; }
    if (p->second_best) { gx::set_error(call + "second_best is not supported"); return GASALX_EUNSUPPORTED; }
    if ((!heads && p->head != 2) || p->tail != 2) {
        gx::set_error(call + "HEAD=" + src[p->head] + " TAIL=" + src[p->tail] + " is not supported (" +
                      (heads ? "TAIL=TARGET only)" : "HEAD=TARGET TAIL=TARGET only)"));
        return GASALX_EUNSUPPORTED;
    }
    if (!b || !out) return GASALX_OK;
    if (!out->aln_score || !out->cigar || !out->n_cigar_ops) {
        gx::set_error(call + "aln_score, cigar and n_cigar_ops outputs are required");
        return GASALX_EINVAL;
    }
    if (out->aln_score2 || out->q_end2 || out->t_end2) {
        gx::set_error(call + "the second-best outputs must be NULL");
        return GASALX_EINVAL;
    }
    if (b->q_batch && ranges_overlap(out->cigar, b->q_bytes, b->q_batch, b->q_bytes)) {
        gx::set_error(call + "cigar overlaps q_batch (it must be a buffer of its own)");
        return GASALX_EINVAL;
    }
    return GASALX_OK;
}

// ph2pr[q] = powf(10, -q/10) on the host, as the reference builds it (tile_1.cu:216-220)
void ph2pr_table(float *t) {
    for (int i = 0; i < 128; i++) t[i] = powf(10.f, -((float)i) / 10.f);
}

// The engine's device copy of the table (uploaded once, synchronously).
int ph2pr_device(gasalx_engine *eng, const float **out) {
    gx::DevBuf &tab = eng->buf[B_PH2PR];
    if (!tab.p) {
        float t[128];
        ph2pr_table(t);
        CK(tab.reserve(sizeof(t)));
        CK(hipMemcpy(tab.p, t, sizeof(t), hipMemcpyHostToDevice));
    }
    *out = tab.as<float>();
    return GASALX_OK;
}

bool hmm_qual_batch_ok(const gasalx_hmm_qual_batch *b) {
    return b && (b->n_pairs == 0 || (b->reads && b->read_offsets && b->read_lens && b->base_quals && b->ins_quals &&
                                     b->del_quals && b->haps && b->hap_offsets && b->hap_lens));
}

// The fp32 pass of a host batch in parameter form: staged (db = the device image), results in
// B_RES.  Like quals_host_fp32 it synchronises the stream only when its launch fails; after a good
// launch the caller queues what follows (the copy back, the rescue pass) and waits once.
int hmm_host_fp32(gasalx_engine *eng, const gasalx_hmm_batch *hb, hipStream_t st, gasalx_hmm_batch &db) {
    int rc = hmm_stage_host(eng, hb, st, db);
    if (rc) return rc;
    CK(eng->buf[B_RES].reserve((size_t)hb->n_pairs * 4 + 16));
    rc = gx::pairhmm_device(eng->ws, db, eng->buf[B_RES].as<float>(), st, db.max_read_len, db.max_hap_len);
    if (rc) (void)hipStreamSynchronize(st);   // on error only: the caller's host_finish is the one wait of a good call
    return rc;
}

// The fp32 pass of a host batch in quality form: pairs staged into the engine's device buffers
// (db = the device image, max lengths filled in), run sorted by (read length, haplotype length)
// in classes of reads that share a lane-group size, results in B_RES by pair index.
// perm: the slot order, the caller's so that it outlives its copy (until the stream is synchronised).
int quals_host_fp32(gasalx_engine *eng, const gasalx_hmm_qual_batch *hb, hipStream_t st, gasalx_hmm_qual_batch &db,
                    const float **tab_out, std::vector<uint32_t> &perm) {
    const uint32_t n = hb->n_pairs;
    // slots in (read length, haplotype length) order (tile_1.cu:180-195 operator<, :325)
    perm.resize(n);
    for (uint32_t i = 0; i < n; i++) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
        const uint32_t rx = hb->read_lens[x], ry = hb->read_lens[y];
        return rx != ry ? rx < ry : hb->hap_lens[x] < hb->hap_lens[y];
    });
    // classes: runs of slots whose reads need the same lane-group size
    std::vector<gx::HmmClass> classes;
    uint32_t mr = 0, mh = 0;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t r = hb->read_lens[perm[s]], h = hb->hap_lens[perm[s]];
        const int g = gx::pairhmm_group(r);
        if (classes.empty() || gx::pairhmm_group(classes.back().max_r) != g) classes.push_back({s, s, 0, 0});
        gx::HmmClass &c = classes.back();
        c.slot1 = s + 1;
        c.max_r = std::max(c.max_r, r);
        c.max_h = std::max(c.max_h, h);
        mr = std::max(mr, r);
        mh = std::max(mh, h);
    }
    int rc = hmm_stage_quals(eng, hb, st, db);
    if (rc) return rc;
    db.max_read_len = mr;
    db.max_hap_len = mh;
    uint32_t *dperm;
    if ((rc = stage_in(eng->buf[B_PERM], perm.data(), n, st, &dperm))) return rc;
    CK(eng->buf[B_RES].reserve((size_t)n * 4 + 16));
    if ((rc = ph2pr_device(eng, tab_out))) return rc;
    rc = gx::pairhmm_quals_device(eng->ws, db, eng->buf[B_RES].as<float>(), st, *tab_out, dperm, classes.data(),
                                  (int)classes.size(), 0, 0);
    if (rc) (void)hipStreamSynchronize(st);   // on error only, as hmm_host_fp32
    return rc;
}

// ---- PairHMM in float64 and the log10 entry points (pairhmm64.hip) ----
// The rescue pass after an fp32 pass whose results are at r32 (device): scratch from the engine.
int log10_rescue(gasalx_engine *eng, const gx::Hmm64Src &src, uint32_t n, const float *r32, float min_accepted,
                 double *out, uint8_t *used, hipStream_t st, uint32_t mr, uint32_t mh) {
    CK(eng->buf[B_HM_LIST].reserve(((size_t)n + 4) * 4));
    uint32_t *count = eng->buf[B_HM_LIST].as<uint32_t>();
    return gx::pairhmm_log10_device(src, n, r32, min_accepted, out, used, count, count + 4, st, mr, mh);
}

// Host forms: device outputs in B_RES64 / B_USED, copied back with the count.
int log10_host_finish(gasalx_engine *eng, const gx::Hmm64Src &src, uint32_t n, float min_accepted, double *hlog,
                      uint8_t *hused, uint32_t *n_rescued, hipStream_t st, uint32_t mr, uint32_t mh) {
    gx::DevBuf &res = eng->buf[B_RES64], &used = eng->buf[B_USED];
    CK(res.reserve((size_t)n * 8 + 16));
    CK(used.reserve((size_t)n + 16));
    int rc = log10_rescue(eng, src, n, eng->buf[B_RES].as<float>(), min_accepted, res.as<double>(),
                          hused ? used.as<uint8_t>() : nullptr, st, mr, mh);
    uint32_t cnt = 0;
    rc = host_finish(st, rc, {{hlog, res.p, (size_t)n * 8}, {hused, used.p, n}, {&cnt, eng->buf[B_HM_LIST].p, 4}});
    if (!rc && n_rescued) *n_rescued = cnt;
    return rc;
}

// The float64 forward values of a staged host batch (src points at its device image), copied out.
int hmm64_host_run(gasalx_engine *eng, const gx::Hmm64Src &src, uint32_t n, double *hres, hipStream_t st, uint32_t mr,
                   uint32_t mh) {
    gx::DevBuf &res = eng->buf[B_RES64];
    CK(res.reserve((size_t)n * 8 + 16));
    const int rc = gx::pairhmm64_device(src, n, res.as<double>(), st, mr, mh);
    return host_finish(st, rc, {{hres, res.p, (size_t)n * 8}});
}

// nvbio BatchedAlignmentTraceback (nvtrace.hpp).  nvbio keeps its DP columns and checkpoints in
// int16 (alignment/utils.h:49-64): the scores of every cell must stay within them.
int64_t nv_score_mag(const gasalx_nv_aligner *al) {
    if (al->aligner == GASALX_NV_ED) return 1;   // ED: EditDistanceSWScheme's 0 / -1 (ed_utils.h:45-52)
    return std::max<int64_t>({std::abs((int64_t)al->match), std::abs((int64_t)al->mismatch),
                              std::abs((int64_t)al->gap_open), std::abs((int64_t)al->gap_ext),
                              std::abs((int64_t)al->deletion), std::abs((int64_t)al->insertion), 1});
}

// nvbio traceback workspace per call (the engine's: flags of every cell, one DP row per pair) and
// the chunk budget the device entry points split a batch by
constexpr uint64_t kNvTbBudget = 4ull << 30;
// GASALX_NV_TB_BUDGET (bytes) replaces it for tests that force several chunks; read on every
// call, and unset, empty, zero or unparsable leave the 4 GiB
uint64_t nv_tb_budget() {
    const char *e = std::getenv("GASALX_NV_TB_BUDGET");
    if (!e || !*e) return kNvTbBudget;
    for (const char *c = e; *c; c++)
        if (*c < '0' || *c > '9') return kNvTbBudget;
    errno = 0;
    const unsigned long long v = std::strtoull(e, nullptr, 10);
    return (errno || !v) ? kNvTbBudget : (uint64_t)v;
}
// pairs per chunk of a batch of n whose workspace takes `per` bytes per pair
uint64_t nv_tb_chunk(uint32_t n, uint64_t per) {
    return std::max<uint64_t>(1, std::min<uint64_t>(n, nv_tb_budget() / std::max<uint64_t>(per, 1)));
}

int nv_tb_checks(const gasalx_nv_aligner *al, uint32_t max_p, uint32_t max_t, uint32_t ops_stride) {
    const int64_t mag = nv_score_mag(al);
    if (((int64_t)max_p + max_t + 2) * mag > 32767) {
        gx::set_error("traceback: scores would leave nvbio's int16 columns (lengths x |score|)");
        return GASALX_ERANGE;
    }
    if (ops_stride < max_p + max_t) { gx::set_error("traceback: ops_stride < max pattern + max text length"); return GASALX_EINVAL; }
    if ((uint64_t)max_p * max_t > (1ull << 24)) { gx::set_error("traceback: pattern x text above 16 M cells"); return GASALX_ERANGE; }
    return GASALX_OK;
}

// nvbio BatchedBandedAlignmentTraceback<band> (nvtrace.hpp).  nvbio's checkpoints are int16
// pairs clamped at -32736 (gotoh_banded_inl.h:234-239): every score must stay above it.
int nv_btb_checks(const gasalx_nv_aligner *al, uint32_t band, uint32_t max_p, uint32_t ops_stride) {
    if (band < 2 || band > 32) { gx::set_error("band length must be 2..32"); return GASALX_EINVAL; }
    if (((int64_t)max_p + band + 3) * nv_score_mag(al) > 32736) {
        gx::set_error("banded traceback: scores would leave nvbio's int16 checkpoints (lengths x |score|)");
        return GASALX_ERANGE;
    }
    if ((uint64_t)ops_stride < 2ull * max_p + band) {
        gx::set_error("banded traceback: ops_stride < 2 x max pattern length + band");
        return GASALX_EINVAL;
    }
    return GASALX_OK;
}

// The outputs of a traceback call, device or host.
struct NvTbOut {
    int32_t *scores;
    uint32_t *sources, *sinks;
    uint8_t *ops;
    uint32_t ops_stride;
    uint32_t *n_ops;
};

// A traceback batch in chunks of `chunk` pairs over the engine's workspace (band 0: the full DP;
// mat: its substitution-matrix form, NULL otherwise; q: the banded form under a quality scheme, NULL
// otherwise): the chunk from pair s on works on offsets + s, scores + s, sources + 2s, sinks + 2s,
// ops + s * ops_stride and n_ops + s (the quality bytes follow the offsets' own values).
int nv_tb_chunks(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                 const gasalx_nv_quals *q, uint32_t band, uint32_t n,
                 const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, uint32_t max_p, uint32_t max_t,
                 const NvTbOut &o, uint32_t chunk, hipStream_t st) {
    gx::DevBuf &dir = eng->buf[B_NV_DIR];
    for (uint32_t s = 0; s < n; s += chunk) {
        const uint32_t m = std::min(chunk, n - s);
        gasalx_nv_strings p = *pat, t = *txt;
        p.offsets = pat->offsets + s;
        if (txt->offsets) t.offsets = txt->offsets + s;
        int32_t *scores = o.scores + s;
        uint32_t *sources = o.sources + 2ull * s, *sinks = o.sinks + 2ull * s, *n_ops = o.n_ops + s;
        uint8_t *ops = o.ops + (size_t)s * o.ops_stride;
        const int rc = q    ? gx::nv_banded_qual_traceback_device(*al, q, band, m, p, t, max_p, dir.as<uint32_t>(), scores,
                                                                  sources, sinks, ops, o.ops_stride, n_ops, st)
                     : band ? gx::nv_banded_traceback_device(*al, band, m, p, t, max_p, dir.as<uint32_t>(), scores, sources,
                                                             sinks, ops, o.ops_stride, n_ops, st)
                     : mat  ? gx::nv_matrix_traceback_device(*al, *mat, m, p, t, max_p, max_t, dir.as<uint8_t>(),
                                                             eng->buf[B_NV_ROW].as<int32_t>(), scores, sources, sinks,
                                                             ops, o.ops_stride, n_ops, st)
                            : gx::nv_traceback_device(*al, m, p, t, max_p, max_t, dir.as<uint8_t>(),
                                                      eng->buf[B_NV_ROW].as<int32_t>(), scores, sources, sinks, ops,
                                                      o.ops_stride, n_ops, st);
        if (rc) return rc;
    }
    return GASALX_OK;
}

// ---- The gasalx_nv_* entry points: each family's call sequence, written once.  An entry point keeps
//      its own argument test, its pre-checks in their order, and the one gx:: call that is its own; a
//      new score pair is an output list and a callable, not a copy of its neighbour. ----

int nv_null() { gx::set_error("null argument"); return GASALX_EINVAL; }

// What every host form (and gasalx_nv_matrix_traceback_device) needs of its two string sets, and
// the traceback host forms of their outputs.
bool nv_sets_ok(const gasalx_nv_strings *pat, const gasalx_nv_strings *txt) {
    return pat && txt && pat->words && pat->offsets && txt->words;
}
bool nv_tb_out_ok(const NvTbOut &o) { return o.scores && o.sources && o.sinks && o.ops && o.n_ops; }

// A device form's start: enter, then the bounds the caller left zero read back from the offsets.
enum NvBounds {
    NV_BOTH,              // the longest pattern and, for per-pair texts, the longest text
    NV_BOTH_SHARED,       // the same, and one shared text's length replaces the caller's max_t (traceback)
    NV_PATTERN,           // the longest pattern alone (banded traceback)
    NV_PATTERN_IF_OFFSETS // the same, unless the pattern set has no offsets to read (the banded scorers)
};
int nv_device_enter(gasalx_engine *eng, void *stream, NvBounds which, uint32_t n, const gasalx_nv_strings *pat,
                    const gasalx_nv_strings *txt, uint32_t *max_p, uint32_t *max_t, hipStream_t *st) {
    int rc = enter(eng, stream, st);
    if (rc) return rc;
    const bool both = which == NV_BOTH || which == NV_BOTH_SHARED;
    if (which != NV_PATTERN_IF_OFFSETS || pat->offsets)
        if ((rc = device_max_spans(pat, both ? txt : nullptr, n, *st, max_p, both ? max_t : nullptr))) return rc;
    if (which == NV_BOTH_SHARED && !txt->offsets) *max_t = txt->length;
    return GASALX_OK;
}

// The score host forms: the sets staged, the wanted outputs reserved, launch(staged sets and bounds,
// the outputs' device pointers in `out`'s order (NULL where the caller's is), stream), the results back.
// An output: the caller's array (NULL: not wanted), the engine buffer that stages it, bytes per pair.
struct NvOut { void *host; Buf buf; size_t per_pair; };
template <class Launch>
int nv_score_host_run(gasalx_engine *eng, const NvHostIn &h, const NvOut (&out)[2], Launch launch) {
    if (h.n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    NvStaged s;
    nv_host_spans(h, s);
    if ((rc = nv_stage_strings(eng, h, st, s))) return rc;
    void *d[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++)
        if (out[k].host) {
            CK(eng->buf[out[k].buf].reserve(h.n * out[k].per_pair));
            d[k] = eng->buf[out[k].buf].p;
        }
    rc = launch(s, d, st);
    return host_finish(st, rc, {{out[0].host, d[0], h.n * out[0].per_pair}, {out[1].host, d[1], h.n * out[1].per_pair}});
}

// Bytes per pair of the traceback workspace: the full DP's flags of every cell and its one DP row,
// the banded form's flags (gasalx_nv_*traceback_workspace and the device forms' reserves).
uint64_t nv_tb_dir_bytes(uint32_t max_p, uint32_t max_t) { return (uint64_t)((max_p + 7) / 8) * 8 * max_t; }
uint64_t nv_tb_row_bytes(uint32_t max_t) { return (uint64_t)max_t * 8; }
uint64_t nv_btb_dir_bytes(uint32_t max_p, uint32_t band) { return (uint64_t)max_p * ((band + 3) / 4) * 4; }

// The full-DP traceback device forms (mat: the substitution-matrix form, NULL otherwise) after their
// argument tests; `ranged` is the aligner nv_tb_checks takes.
int nv_tb_device_run(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                     const gasalx_nv_aligner *ranged, uint32_t n, const gasalx_nv_strings *pat,
                     const gasalx_nv_strings *txt, uint32_t max_p, uint32_t max_t, const NvTbOut &o, void *stream) {
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = nv_device_enter(eng, stream, NV_BOTH_SHARED, n, pat, txt, &max_p, &max_t, &st);
    if (rc) return rc;
    if ((rc = nv_tb_checks(ranged, max_p, max_t, o.ops_stride))) return rc;
    // the batch runs in chunks whose workspace (flags of every cell + one row per pair) stays
    // within nv_tb_budget() (1 M 150 x 182 pairs would otherwise take 28 GB of HBM)
    const uint32_t chunk = (uint32_t)nv_tb_chunk(n, gasalx_nv_traceback_workspace(max_p, max_t, 1));
    CK(eng->buf[B_NV_DIR].reserve((size_t)nv_tb_dir_bytes(max_p, max_t) * chunk + 64));
    CK(eng->buf[B_NV_ROW].reserve((size_t)nv_tb_row_bytes(max_t) * chunk + 64));
    return nv_tb_chunks(eng, al, mat, nullptr, 0, n, pat, txt, max_p, max_t, o, chunk, st);
}

// The traceback host forms after their argument tests (band 0: the full DP, refused by nv_tb_checks
// over `ranged` before anything is staged; mat: its substitution-matrix form, NULL otherwise; the
// banded form has made its checks): the sets staged, the five device outputs reserved, the device
// form run on them, the results copied to the caller's arrays `h`.  q: the banded form under a
// quality scheme (NULL otherwise), its quality bytes staged beside the sets.
int nv_tb_host_run(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat, uint32_t band,
                   const gasalx_nv_aligner *ranged, const NvHostIn &in, const NvTbOut &h,
                   const gasalx_nv_quals *q = nullptr) {
    const uint32_t n = in.n;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    NvStaged d;
    nv_host_spans(in, d);
    if (!band && (rc = nv_tb_checks(ranged, d.max_p, d.max_t, h.ops_stride))) return rc;
    if ((rc = nv_stage_strings(eng, in, st, d))) return rc;
    gasalx_nv_quals dq = {};
    if (q && (rc = nv_stage_quals(eng, in, q, st, dq))) return rc;
    gx::DevBuf &s = eng->buf[B_NV_S], &src = eng->buf[B_NV_SRC], &snk = eng->buf[B_NV_SNK], &ops = eng->buf[B_NV_OPS],
               &nops = eng->buf[B_NV_NOPS];
    CK(s.reserve((size_t)n * 4));
    CK(src.reserve((size_t)n * 8));
    CK(snk.reserve((size_t)n * 8));
    CK(ops.reserve((size_t)n * h.ops_stride + 64));
    CK(nops.reserve((size_t)n * 4));
    rc = q    ? gasalx_nv_banded_qual_traceback_device(eng, al, &dq, band, n, &d.pat, &d.txt, d.max_p, s.as<int32_t>(),
                                                       src.as<uint32_t>(), snk.as<uint32_t>(), ops.as<uint8_t>(),
                                                       h.ops_stride, nops.as<uint32_t>(), st)
       : band ? gasalx_nv_banded_traceback_device(eng, al, band, n, &d.pat, &d.txt, d.max_p, s.as<int32_t>(),
                                                  src.as<uint32_t>(), snk.as<uint32_t>(), ops.as<uint8_t>(), h.ops_stride,
                                                  nops.as<uint32_t>(), st)
         : mat ? gasalx_nv_matrix_traceback_device(eng, al, mat, n, &d.pat, &d.txt, d.max_p, d.max_t, s.as<int32_t>(),
                                                   src.as<uint32_t>(), snk.as<uint32_t>(), ops.as<uint8_t>(), h.ops_stride,
                                                   nops.as<uint32_t>(), st)
               : gasalx_nv_traceback_device(eng, al, n, &d.pat, &d.txt, d.max_p, d.max_t, s.as<int32_t>(),
                                            src.as<uint32_t>(), snk.as<uint32_t>(), ops.as<uint8_t>(), h.ops_stride,
                                            nops.as<uint32_t>(), st);
    return host_finish(st, rc, {{h.scores, s.p, (size_t)n * 4}, {h.sources, src.p, (size_t)n * 8},
                                {h.sinks, snk.p, (size_t)n * 8}, {h.ops, ops.p, (size_t)n * h.ops_stride},
                                {h.n_ops, nops.p, (size_t)n * 4}});
}

// The matrix traceback forms' checks after the null arguments: the aligner and the table's size, the
// table and the symbol bits (before anything is read back or staged); `ranged` is then the aligner
// nv_tb_checks takes, the largest |entry| standing for match and mismatch (the aligner's own match,
// mismatch, deletion and insertion are never read)
int nv_mtb_checks(const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat, const gasalx_nv_strings *pat,
                  const gasalx_nv_strings *txt, gasalx_nv_aligner *ranged) {
    int32_t mag = 0;
    if (int rc = gx::nv_matrix_traceback_check(*al, *mat, *pat, *txt, &mag)) return rc;
    *ranged = {al->aligner, al->type, mag, mag, al->gap_open, al->gap_ext, 0, 0};
    return GASALX_OK;
}

// The quality forms' checks after the null arguments, in gasalx.h's order (before anything is read
// back or staged); `ranged` is then the aligner nv_btb_checks takes, the largest |entry| standing
// for match and mismatch
int nv_qual_checks(const gasalx_nv_aligner *al, const gasalx_nv_quals *q, uint32_t band, const gasalx_nv_strings *pat,
                   const gasalx_nv_strings *txt, gasalx_nv_aligner *ranged) {
    int32_t mag = 0;
    if (int rc = gx::nv_banded_qual_check(*al, q, true, band, *pat, *txt, &mag)) return rc;
    if (ranged) *ranged = {al->aligner, al->type, mag, mag, al->gap_open, al->gap_ext, 0, 0};
    return GASALX_OK;
}

// The describe functions: name(s) puts the plan's name into s or returns the code that refuses it.
template <class Name>
int nv_describe(bool args_ok, char *buf, uint32_t buf_len, Name name) {
    if (!args_ok || !buf || buf_len == 0) return nv_null();
    std::string s;
    if (int rc = name(s)) return rc;
    std::snprintf(buf, buf_len, "%s", s.c_str());
    return GASALX_OK;
}

}  // namespace

extern "C" {

int gasalx_abi_version(void) { return GASALX_ABI_VERSION; }
const char *gasalx_last_error(void) { return gx::last_error(); }

int gasalx_device_count(int *count) {
    if (!count) return GASALX_EINVAL;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; gx::set_error(hipGetErrorString(e)); return GASALX_EDEVICE; }
    *count = c;
    return GASALX_OK;
}

int gasalx_engine_create(int device, gasalx_engine **out) {
    if (!out) return GASALX_EINVAL;
    *out = nullptr;
    CK(hipSetDevice(device));
    gasalx_engine *e = new (std::nothrow) gasalx_engine();
    if (!e) return GASALX_ENOMEM;
    e->device = device;
    e->ws.device = device;
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { delete e; gx::set_error(hipGetErrorString(he)); return GASALX_EDEVICE; }
    *out = e;
    return GASALX_OK;
}

int gasalx_engine_destroy(gasalx_engine *eng) {
    if (!eng) return GASALX_OK;
    (void)hipSetDevice(eng->device);
    if (eng->stream) { (void)hipStreamSynchronize(eng->stream); (void)hipStreamDestroy(eng->stream); }
    eng->release();
    delete eng;
    return GASALX_OK;
}

int gasalx_describe_plan(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len, char *buf,
                         uint32_t buf_len) {
    if (!valid_params(params) || !buf || buf_len == 0) return GASALX_EINVAL;
    gx::BatchShape s;
    s.max_q = max_q_len; s.max_t = max_t_len;
    gx::Plan pl = gx::make_plan(*params, s, false);
    std::snprintf(buf, buf_len, "%s", pl.name.c_str());
    return GASALX_OK;
}

int gasalx_align_device(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *b,
                        const gasalx_results *out, void *stream) {
    if (!eng || !valid_params(params) || !b || !out) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    gx::BatchShape shape;
    shape.max_q = b->max_q_len;
    shape.max_t = b->max_t_len;
    if ((rc = device_max_lens(b->q_lens, b->t_lens, b->n_alns, st, &shape.max_q, &shape.max_t))) return rc;
    return gx::align_device(eng->ws, *params, *b, *out, st, shape);
}

int gasalx_align_host(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *hb,
                      const gasalx_results *ho) {
    if (!eng || !valid_params(params) || !hb || !ho) { gx::set_error("null argument"); return GASALX_EINVAL; }
    if (!hb->q_batch || !hb->t_batch || !hb->q_offsets || !hb->t_offsets || !hb->q_lens || !hb->t_lens) {
        gx::set_error("missing batch array");
        return GASALX_EINVAL;
    }
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    const uint32_t n = hb->n_alns;
    const bool tb = params->start_pos == 2;
    const uint32_t mq = hb->max_q_len ? hb->max_q_len : host_max(hb->q_lens, n);
    const uint32_t mt = hb->max_t_len ? hb->max_t_len : host_max(hb->t_lens, n);
    // large batches in the standard layout go through the two-stream pipeline
    // TB: the traceback walk is latency-bound per chunk whatever its size, so chunks
    // of ~5.5 G padded cells, 2 to 8 of them (1 M x 150 bp: 4, 34.0 ms pageable against
    // 50.5 with 2; 100 K x 300 bp: 2); score-only: 8
    uint32_t n_chunks = 8;
    if (tb) n_chunks = (uint32_t)std::min(8.0, std::max(2.0, std::round((double)n * mq * mt / 5.5e9)));
    const uint32_t chunk = std::max<uint32_t>(16384, (uint32_t)(((uint64_t)n + n_chunks - 1) / n_chunks));
    if (n >= 2 * chunk && !(params->is_packed && tb) && contiguous(hb->q_offsets, hb->q_lens, n, hb->q_bytes) &&
        contiguous(hb->t_offsets, hb->t_lens, n, hb->t_bytes))
        return align_host_pipelined(eng, params, hb, ho, chunk, tb, mq, mt);
    gasalx_batch db = *hb;
    // isPacked without traceback: only the packed half of the pages moves (with traceback the
    // device CIGAR buffer starts as the whole query batch, gasal_align.cu:281)
    const uint32_t pk = params->is_packed && !tb ? 2 : 1;
    Stager in{eng, st};
    in(B_Q, db.q_batch, hb->q_bytes / pk);
    in(B_T, db.t_batch, hb->t_bytes / pk);
    in(B_QO, db.q_offsets, n);
    in(B_TO, db.t_offsets, n);
    in(B_QL, db.q_lens, n);
    in(B_TL, db.t_lens, n);
    in(B_QOP, db.q_ops, n);
    in(B_TOP, db.t_ops, n);
    in(B_SEED, db.seed_scores, n);
    db.max_q_len = mq;
    db.max_t_len = mt;
    // outputs: staged in with the caller's contents so fields the reference
    // would not write come back unchanged
    gasalx_results dout;
    for (int f = 0; f < kFields; f++) {
        const uint8_t *p = static_cast<const uint8_t *>(get_field(*ho, f));
        in(Buf(B_OUT + f), p, field_bytes(f, n, hb->q_bytes));
        set_field(dout, f, const_cast<uint8_t *>(p));
    }
    if (in.rc) return in.rc;
    gx::BatchShape shape;
    shape.max_q = mq;
    shape.max_t = mt;
    shape.sort = gx::uneven_lengths(*params, hb->q_lens, hb->t_lens, n);
    shape.one_t8 = gx::one_pad8(hb->t_lens, n, shape.max_t);
    if ((rc = gx::align_device(eng->ws, *params, db, dout, st, shape))) return host_finish(st, rc, {});
    for (int f = 0; f < kFields; f++)
        if (void *h = get_field(*ho, f))
            CK(hipMemcpyAsync(h, get_field(dout, f), field_bytes(f, n, hb->q_bytes), hipMemcpyDeviceToHost, st));
    return host_finish(st, GASALX_OK, {});
}

// the three semi-CIGAR calls, HEAD = TARGET (gasalx_semi_cigar_*) or any HEAD (gasalx_semi_cigar_head_*)
static int semi_cigar_describe(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len, char *buf,
                               uint32_t buf_len, bool heads) {
    if (!valid_params(params) || !buf || buf_len == 0) { gx::set_error("null argument"); return GASALX_EINVAL; }
    buf[0] = 0;
    int rc = semi_cigar_checks(params, nullptr, nullptr, heads);
    if (rc) return rc;
    gx::BatchShape s;
    s.max_q = max_q_len; s.max_t = max_t_len;
    std::string why;
    const gx::Plan pl = gx::make_semi_cigar_plan(*params, s, false, &rc, &why, heads);
    if (rc) gx::set_error(why);
    std::snprintf(buf, buf_len, "%s", pl.name.c_str());
    return rc;
}

static int semi_cigar_dev(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *b,
                          const gasalx_results *out, void *stream, bool heads) {
    if (!eng || !valid_params(params) || !b || !out) { gx::set_error("null argument"); return GASALX_EINVAL; }
    int rc = semi_cigar_checks(params, b, out, heads);
    if (rc) return rc;
    hipStream_t st;
    if ((rc = enter(eng, stream, &st))) return rc;
    gx::BatchShape shape;
    shape.max_q = b->max_q_len;
    shape.max_t = b->max_t_len;
    if ((rc = device_max_lens(b->q_lens, b->t_lens, b->n_alns, st, &shape.max_q, &shape.max_t))) return rc;
    return gx::semi_cigar_device(eng->ws, *params, *b, *out, st, shape, false, heads);
}

static int semi_cigar_hst(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *hb,
                         const gasalx_results *ho, bool heads) {
    if (!eng || !valid_params(params) || !hb || !ho) { gx::set_error("null argument"); return GASALX_EINVAL; }
    int rc = semi_cigar_checks(params, hb, ho, heads);
    if (rc) return rc;
    if (!hb->q_batch || !hb->t_batch || !hb->q_offsets || !hb->t_offsets || !hb->q_lens || !hb->t_lens) {
        gx::set_error("missing batch array");
        return GASALX_EINVAL;
    }
    hipStream_t st;
    if ((rc = enter(eng, nullptr, &st))) return rc;
    const uint32_t n = hb->n_alns;
    gasalx_batch db = *hb;
    const uint32_t pk = params->is_packed ? 2 : 1;   // packed input: half the bytes the offsets count
    Stager in{eng, st};
    in(B_Q, db.q_batch, hb->q_bytes / pk);
    in(B_T, db.t_batch, hb->t_bytes / pk);
    in(B_QO, db.q_offsets, n);
    in(B_TO, db.t_offsets, n);
    in(B_QL, db.q_lens, n);
    in(B_TL, db.t_lens, n);
    in(B_QOP, db.q_ops, n);
    in(B_TOP, db.t_ops, n);
    if (in.rc) return in.rc;
    db.max_q_len = hb->max_q_len ? hb->max_q_len : host_max(hb->q_lens, n);
    db.max_t_len = hb->max_t_len ? hb->max_t_len : host_max(hb->t_lens, n);
    // the outputs the caller asked for, each in its own device buffer; the CIGAR buffer starts as
    // zeros, so the bytes the walk does not write come back the same on every call
    gasalx_results dout = {};
    for (int f : {0, 1, 2, 3, 4, kCigar, kNops}) {
        if (!get_field(*ho, f)) continue;
        gx::DevBuf &d = eng->buf[B_OUT + f];
        CK(d.reserve(field_bytes(f, n, hb->q_bytes) + 16));
        set_field(dout, f, d.p);
    }
    CK(hipMemsetAsync(dout.cigar, 0, hb->q_bytes, st));
    gx::BatchShape shape;
    shape.max_q = db.max_q_len;
    shape.max_t = db.max_t_len;
    shape.sort = gx::uneven_lengths(*params, hb->q_lens, hb->t_lens, n);   // the score launch: by query length
    gasalx_params by_target = *params;
    by_target.algo = 1;                                                    // the flags launch: by target length
    const bool sort_t = gx::uneven_lengths(by_target, hb->q_lens, hb->t_lens, n);
    rc = gx::semi_cigar_device(eng->ws, *params, db, dout, st, shape, sort_t, heads);
    return host_finish(st, rc, {{ho->aln_score, dout.aln_score, (size_t)n * 4}, {ho->q_end, dout.q_end, (size_t)n * 4},
                                {ho->t_end, dout.t_end, (size_t)n * 4}, {ho->q_start, dout.q_start, (size_t)n * 4},
                                {ho->t_start, dout.t_start, (size_t)n * 4}, {ho->cigar, dout.cigar, hb->q_bytes},
                                {ho->n_cigar_ops, dout.n_cigar_ops, (size_t)n * 4}});
}

int gasalx_describe_semi_cigar_plan(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len, char *buf,
                                    uint32_t buf_len) {
    return semi_cigar_describe(params, max_q_len, max_t_len, buf, buf_len, false);
}
int gasalx_semi_cigar_device(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *b,
                             const gasalx_results *out, void *stream) {
    return semi_cigar_dev(eng, params, b, out, stream, false);
}
int gasalx_semi_cigar_host(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *hb,
                           const gasalx_results *ho) {
    return semi_cigar_hst(eng, params, hb, ho, false);
}
int gasalx_describe_semi_cigar_head_plan(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len, char *buf,
                                         uint32_t buf_len) {
    return semi_cigar_describe(params, max_q_len, max_t_len, buf, buf_len, true);
}
int gasalx_semi_cigar_head_device(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *b,
                                  const gasalx_results *out, void *stream) {
    return semi_cigar_dev(eng, params, b, out, stream, true);
}
int gasalx_semi_cigar_head_host(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *hb,
                                const gasalx_results *ho) {
    return semi_cigar_hst(eng, params, hb, ho, true);
}

int gasalx_pairhmm_device(gasalx_engine *eng, const gasalx_hmm_batch *b, float *res, void *stream) {
    if (!eng || !b || !res) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    uint32_t mr = b->max_read_len, mh = b->max_hap_len;
    if ((rc = device_max_lens(b->read_lens, b->hap_lens, b->n_pairs, st, &mr, &mh))) return rc;
    return gx::pairhmm_device(eng->ws, *b, res, st, mr, mh);
}

int gasalx_pairhmm_host(gasalx_engine *eng, const gasalx_hmm_batch *hb, float *hres) {
    if (!eng || !hb || !hres) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    gasalx_hmm_batch db;
    if ((rc = hmm_host_fp32(eng, hb, st, db))) return rc;
    return host_finish(st, GASALX_OK, {{hres, eng->buf[B_RES].p, (size_t)hb->n_pairs * 4}});
}

int gasalx_pairhmm_quals_device(gasalx_engine *eng, const gasalx_hmm_qual_batch *b, float *res, void *stream) {
    if (!eng || !hmm_qual_batch_ok(b) || !res) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    uint32_t mr = b->max_read_len, mh = b->max_hap_len;
    if ((rc = device_max_lens(b->read_lens, b->hap_lens, b->n_pairs, st, &mr, &mh))) return rc;
    const float *tab;
    if ((rc = ph2pr_device(eng, &tab))) return rc;
    return gx::pairhmm_quals_device(eng->ws, *b, res, st, tab, nullptr, nullptr, 0, mr, mh);
}

int gasalx_pairhmm_quals_host(gasalx_engine *eng, const gasalx_hmm_qual_batch *hb, float *hres) {
    if (!eng || !hmm_qual_batch_ok(hb) || !hres) { gx::set_error("null argument"); return GASALX_EINVAL; }
    const uint32_t n = hb->n_pairs;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    gasalx_hmm_qual_batch db;
    const float *tab;
    std::vector<uint32_t> perm;
    if ((rc = quals_host_fp32(eng, hb, st, db, &tab, perm))) return rc;
    return host_finish(st, GASALX_OK, {{hres, eng->buf[B_RES].p, (size_t)n * 4}});
}

int gasalx_pairhmm64_device(gasalx_engine *eng, const gasalx_hmm_batch *b, double *res, void *stream) {
    if (!eng || !b || !res) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    uint32_t mr = b->max_read_len, mh = b->max_hap_len;
    if ((rc = device_max_lens(b->read_lens, b->hap_lens, b->n_pairs, st, &mr, &mh))) return rc;
    return gx::pairhmm64_device(gx::Hmm64Src{b, nullptr, nullptr}, b->n_pairs, res, st, mr, mh);
}

int gasalx_pairhmm64_host(gasalx_engine *eng, const gasalx_hmm_batch *hb, double *hres) {
    if (!eng || !hb || !hres) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    const uint32_t n = hb->n_pairs;
    if (n == 0) return GASALX_OK;
    gasalx_hmm_batch db;
    if ((rc = hmm_stage_host(eng, hb, st, db))) return rc;
    return hmm64_host_run(eng, gx::Hmm64Src{&db, nullptr, nullptr}, n, hres, st, db.max_read_len, db.max_hap_len);
}

int gasalx_pairhmm64_quals_device(gasalx_engine *eng, const gasalx_hmm_qual_batch *b, double *res, void *stream) {
    if (!eng || !hmm_qual_batch_ok(b) || !res) { gx::set_error("null argument"); return GASALX_EINVAL; }
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    uint32_t mr = b->max_read_len, mh = b->max_hap_len;
    if ((rc = device_max_lens(b->read_lens, b->hap_lens, b->n_pairs, st, &mr, &mh))) return rc;
    const float *tab;
    if ((rc = ph2pr_device(eng, &tab))) return rc;
    return gx::pairhmm64_device(gx::Hmm64Src{nullptr, b, tab}, b->n_pairs, res, st, mr, mh);
}

int gasalx_pairhmm64_quals_host(gasalx_engine *eng, const gasalx_hmm_qual_batch *hb, double *hres) {
    if (!eng || !hmm_qual_batch_ok(hb) || !hres) { gx::set_error("null argument"); return GASALX_EINVAL; }
    const uint32_t n = hb->n_pairs;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    gasalx_hmm_qual_batch db;
    if ((rc = hmm_stage_quals(eng, hb, st, db))) return rc;
    const float *tab;
    if ((rc = ph2pr_device(eng, &tab))) return rc;
    // one launch sized by the longest read, as the parameter form's
    return hmm64_host_run(eng, gx::Hmm64Src{nullptr, &db, tab}, n, hres, st, host_max(hb->read_lens, n),
                          host_max(hb->hap_lens, n));
}

int gasalx_pairhmm_log10_device(gasalx_engine *eng, const gasalx_hmm_batch *b, float min_accepted, double *dlog,
                                uint8_t *dused, void *stream) {
    if (!eng || !b || !dlog) { gx::set_error("null argument"); return GASALX_EINVAL; }
    const uint32_t n = b->n_pairs;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    uint32_t mr = b->max_read_len, mh = b->max_hap_len;
    if ((rc = device_max_lens(b->read_lens, b->hap_lens, n, st, &mr, &mh))) return rc;
    gx::DevBuf &r32 = eng->buf[B_HM_R32];
    CK(r32.reserve((size_t)n * 4 + 16));
    if ((rc = gx::pairhmm_device(eng->ws, *b, r32.as<float>(), st, mr, mh))) return rc;
    return log10_rescue(eng, gx::Hmm64Src{b, nullptr, nullptr}, n, r32.as<float>(), min_accepted, dlog, dused, st, mr, mh);
}

int gasalx_pairhmm_log10_host(gasalx_engine *eng, const gasalx_hmm_batch *hb, float min_accepted, double *hlog,
                              uint8_t *hused, uint32_t *n_rescued) {
    if (!eng || !hb || !hlog) { gx::set_error("null argument"); return GASALX_EINVAL; }
    if (n_rescued) *n_rescued = 0;
    const uint32_t n = hb->n_pairs;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    gasalx_hmm_batch db;
    if ((rc = hmm_host_fp32(eng, hb, st, db))) return rc;
    return log10_host_finish(eng, gx::Hmm64Src{&db, nullptr, nullptr}, n, min_accepted, hlog, hused, n_rescued, st,
                             db.max_read_len, db.max_hap_len);
}

int gasalx_pairhmm_quals_log10_device(gasalx_engine *eng, const gasalx_hmm_qual_batch *b, float min_accepted,
                                      double *dlog, uint8_t *dused, void *stream) {
    if (!eng || !hmm_qual_batch_ok(b) || !dlog) { gx::set_error("null argument"); return GASALX_EINVAL; }
    const uint32_t n = b->n_pairs;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, stream, &st);
    if (rc) return rc;
    uint32_t mr = b->max_read_len, mh = b->max_hap_len;
    if ((rc = device_max_lens(b->read_lens, b->hap_lens, n, st, &mr, &mh))) return rc;
    const float *tab;
    if ((rc = ph2pr_device(eng, &tab))) return rc;
    gx::DevBuf &r32 = eng->buf[B_HM_R32];
    CK(r32.reserve((size_t)n * 4 + 16));
    if ((rc = gx::pairhmm_quals_device(eng->ws, *b, r32.as<float>(), st, tab, nullptr, nullptr, 0, mr, mh))) return rc;
    return log10_rescue(eng, gx::Hmm64Src{nullptr, b, tab}, n, r32.as<float>(), min_accepted, dlog, dused, st, mr, mh);
}

int gasalx_pairhmm_quals_log10_host(gasalx_engine *eng, const gasalx_hmm_qual_batch *hb, float min_accepted,
                                    double *hlog, uint8_t *hused, uint32_t *n_rescued) {
    if (!eng || !hmm_qual_batch_ok(hb) || !hlog) { gx::set_error("null argument"); return GASALX_EINVAL; }
    if (n_rescued) *n_rescued = 0;
    const uint32_t n = hb->n_pairs;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = enter(eng, nullptr, &st);
    if (rc) return rc;
    gasalx_hmm_qual_batch db;
    const float *tab;
    std::vector<uint32_t> perm;
    if ((rc = quals_host_fp32(eng, hb, st, db, &tab, perm))) return rc;
    // the rescue pass: one launch over the list, sized by the batch's longest read
    return log10_host_finish(eng, gx::Hmm64Src{nullptr, &db, tab}, n, min_accepted, hlog, hused, n_rescued, st,
                             db.max_read_len, db.max_hap_len);
}

int gasalx_nv_score_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *pat,
                           const gasalx_nv_strings *txt, int32_t *scores, int16_t *scores16, uint32_t max_p,
                           uint32_t max_t, void *stream) {
    if (!eng || !al || !pat || !txt) return nv_null();
    hipStream_t st;
    if (int rc = nv_device_enter(eng, stream, NV_BOTH, n, pat, txt, &max_p, &max_t, &st)) return rc;
    return gx::nv_score_device(*al, n, *pat, *txt, scores, scores16, max_p, max_t, st);
}

int gasalx_nv_describe_plan(const gasalx_nv_aligner *al, uint32_t max_p, uint32_t max_t, int per_pair,
                            uint32_t text_bits, char *buf, uint32_t buf_len) {
    return nv_describe(al, buf, buf_len, [&](std::string &s) {
        s = gx::nv_plan_name(*al, max_p, max_t, per_pair != 0, text_bits);
        return GASALX_OK;
    });
}

int gasalx_nv_score_host(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *pat,
                         uint64_t pat_words, const gasalx_nv_strings *txt, uint64_t txt_words, int32_t *scores,
                         int16_t *scores16) {
    if (!eng || !al || !nv_sets_ok(pat, txt) || (!scores && !scores16)) return nv_null();
    return nv_score_host_run(eng, {n, pat, pat_words, txt, txt_words}, {{scores, B_NV_S, 4}, {scores16, B_NV_S16, 2}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 return gx::nv_score_device(*al, n, s.pat, s.txt, (int32_t *)d[0], (int16_t *)d[1],
                                                            s.max_p, s.max_t, st);
                             });
}

int gasalx_nv_score_sinks_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n,
                                 const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, int32_t *scores,
                                 uint32_t *sinks, uint32_t max_p, uint32_t max_t, void *stream) {
    if (!eng || !al || !pat || !txt) return nv_null();
    hipStream_t st;
    if (int rc = nv_device_enter(eng, stream, NV_BOTH, n, pat, txt, &max_p, &max_t, &st)) return rc;
    return gx::nv_score_sinks_device(*al, n, *pat, *txt, scores, sinks, max_p, max_t, st);
}

int gasalx_nv_describe_sinks_plan(const gasalx_nv_aligner *al, uint32_t max_p, uint32_t max_t, int per_pair,
                                  uint32_t text_bits, char *buf, uint32_t buf_len) {
    return nv_describe(al, buf, buf_len, [&](std::string &s) {
        s = gx::nv_sinks_plan_name(*al, max_p, max_t, per_pair != 0, text_bits);
        return GASALX_OK;
    });
}

int gasalx_nv_score_sinks_host(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n,
                               const gasalx_nv_strings *pat, uint64_t pat_words, const gasalx_nv_strings *txt,
                               uint64_t txt_words, int32_t *scores, uint32_t *sinks) {
    if (!eng || !al || !nv_sets_ok(pat, txt) || (!scores && !sinks)) return nv_null();
    return nv_score_host_run(eng, {n, pat, pat_words, txt, txt_words}, {{scores, B_NV_S, 4}, {sinks, B_NV_SNK, 8}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 return gx::nv_score_sinks_device(*al, n, s.pat, s.txt, (int32_t *)d[0], (uint32_t *)d[1],
                                                                  s.max_p, s.max_t, st);
                             });
}

int gasalx_nv_matrix_score_device(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                                  uint32_t n, const gasalx_nv_strings *pat, const gasalx_nv_strings *txt,
                                  int32_t *scores, uint32_t *sinks, uint32_t max_p, uint32_t max_t, void *stream) {
    if (!eng || !al || !mat || !pat || !txt) return nv_null();
    hipStream_t st;
    if (int rc = nv_device_enter(eng, stream, NV_BOTH, n, pat, txt, &max_p, &max_t, &st)) return rc;
    return gx::nv_matrix_score_device(*al, *mat, n, *pat, *txt, scores, sinks, max_p, max_t, st);
}

int gasalx_nv_describe_matrix_plan(const gasalx_nv_aligner *al, uint32_t matrix_n, uint32_t max_p, uint32_t max_t,
                                   int per_pair, int want_sinks, char *buf, uint32_t buf_len) {
    return nv_describe(al, buf, buf_len, [&](std::string &s) {
        return gx::nv_matrix_plan_name(*al, matrix_n, max_p, max_t, per_pair != 0, want_sinks != 0, s);
    });
}

int gasalx_nv_matrix_score_host(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                                uint32_t n, const gasalx_nv_strings *pat, uint64_t pat_words,
                                const gasalx_nv_strings *txt, uint64_t txt_words, int32_t *scores, uint32_t *sinks) {
    if (!eng || !al || !mat || !nv_sets_ok(pat, txt) || (!scores && !sinks)) return nv_null();
    return nv_score_host_run(eng, {n, pat, pat_words, txt, txt_words}, {{scores, B_NV_S, 4}, {sinks, B_NV_SNK, 8}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 return gx::nv_matrix_score_device(*al, *mat, n, s.pat, s.txt, (int32_t *)d[0],
                                                                   (uint32_t *)d[1], s.max_p, s.max_t, st);
                             });
}

int gasalx_nv_banded_score_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t band, uint32_t n,
                                  const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, int32_t *scores,
                                  uint32_t max_p, void *stream) {
    if (!eng || !al || !pat || !txt) return nv_null();
    hipStream_t st;
    if (int rc = nv_device_enter(eng, stream, NV_PATTERN_IF_OFFSETS, n, pat, txt, &max_p, nullptr, &st)) return rc;
    return gx::nv_banded_score_device(*al, band, n, *pat, *txt, scores, st, max_p);
}

int gasalx_nv_banded_score_host(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t band, uint32_t n,
                                const gasalx_nv_strings *pat, uint64_t pat_words, const gasalx_nv_strings *txt,
                                uint64_t txt_words, int32_t *scores) {
    if (!eng || !al || !nv_sets_ok(pat, txt) || !scores) return nv_null();
    if (band < 2 || band > 32) { gx::set_error("band length must be 2..32"); return GASALX_EINVAL; }
    return nv_score_host_run(eng, {n, pat, pat_words, txt, txt_words}, {{scores, B_NV_S, 4}, {nullptr, B_NV_SNK, 0}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 return gx::nv_banded_score_device(*al, band, n, s.pat, s.txt, (int32_t *)d[0], st, s.max_p);
                             });
}

int gasalx_nv_banded_score_sinks_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t band, uint32_t n,
                                        const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, int32_t *scores,
                                        uint32_t *sinks, uint32_t max_p, void *stream) {
    if (!eng || !al || !pat || !txt) return nv_null();
    hipStream_t st;
    if (int rc = nv_device_enter(eng, stream, NV_PATTERN_IF_OFFSETS, n, pat, txt, &max_p, nullptr, &st)) return rc;
    return gx::nv_banded_score_sinks_device(*al, band, n, *pat, *txt, scores, sinks, st, max_p);
}

int gasalx_nv_describe_banded_sinks_plan(const gasalx_nv_aligner *al, uint32_t band, uint32_t max_p,
                                         uint32_t text_bits, char *buf, uint32_t buf_len) {
    return nv_describe(al, buf, buf_len, [&](std::string &s) {
        return gx::nv_banded_sinks_plan_name(*al, band, max_p, text_bits, s);
    });
}

int gasalx_nv_banded_score_sinks_host(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t band, uint32_t n,
                                      const gasalx_nv_strings *pat, uint64_t pat_words, const gasalx_nv_strings *txt,
                                      uint64_t txt_words, int32_t *scores, uint32_t *sinks) {
    if (!eng || !al || !nv_sets_ok(pat, txt) || (!scores && !sinks)) return nv_null();
    if (band < 2 || band > 32) { gx::set_error("band length must be 2..32"); return GASALX_EINVAL; }
    return nv_score_host_run(eng, {n, pat, pat_words, txt, txt_words}, {{scores, B_NV_S, 4}, {sinks, B_NV_SNK, 8}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 return gx::nv_banded_score_sinks_device(*al, band, n, s.pat, s.txt, (int32_t *)d[0],
                                                                         (uint32_t *)d[1], st, s.max_p);
                             });
}

int gasalx_nv_banded_myers_device(gasalx_engine *eng, int32_t type, uint32_t alphabet, uint32_t band, uint32_t n,
                                  const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, int32_t *scores,
                                  uint32_t *sinks, uint32_t max_p, void *stream) {
    (void)max_p;   // the kernel has no value window to size: the bound is not needed, nothing is read back
    if (!eng || !pat || !txt) return nv_null();
    hipStream_t st;
    if (int rc = enter(eng, stream, &st)) return rc;
    return gx::nv_banded_myers_device(type, alphabet, band, n, *pat, *txt, scores, sinks, st);
}

int gasalx_nv_describe_myers_plan(int32_t type, uint32_t alphabet, uint32_t band, char *buf, uint32_t buf_len) {
    return nv_describe(true, buf, buf_len, [&](std::string &s) { return gx::nv_myers_plan_name(type, alphabet, band, s); });
}

int gasalx_nv_banded_myers_host(gasalx_engine *eng, int32_t type, uint32_t alphabet, uint32_t band, uint32_t n,
                                const gasalx_nv_strings *pat, uint64_t pat_words, const gasalx_nv_strings *txt,
                                uint64_t txt_words, int32_t *scores, uint32_t *sinks) {
    if (!eng || !nv_sets_ok(pat, txt) || (!scores && !sinks)) return nv_null();
    // refused before anything is staged, with the device path's own codes and texts
    std::string name;
    if (int rc = gx::nv_myers_plan_name(type, alphabet, band, name)) return rc;
    return nv_score_host_run(eng, {n, pat, pat_words, txt, txt_words}, {{scores, B_NV_S, 4}, {sinks, B_NV_SNK, 8}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 return gx::nv_banded_myers_device(type, alphabet, band, n, s.pat, s.txt, (int32_t *)d[0],
                                                                   (uint32_t *)d[1], st);
                             });
}

uint64_t gasalx_nv_traceback_workspace(uint32_t max_p, uint32_t max_t, uint32_t n) {
    const uint64_t per = nv_tb_dir_bytes(max_p, max_t) + nv_tb_row_bytes(max_t);
    return per * nv_tb_chunk(n, per) + 128;
}
uint64_t gasalx_nv_banded_traceback_workspace(uint32_t max_p, uint32_t band, uint32_t n) {
    const uint64_t per = nv_btb_dir_bytes(max_p, band);
    return per * nv_tb_chunk(n, per) + 64;
}

int gasalx_nv_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n,
                               const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, uint32_t max_p,
                               uint32_t max_t, int32_t *scores, uint32_t *sources, uint32_t *sinks, uint8_t *ops,
                               uint32_t ops_stride, uint32_t *n_ops, void *stream) {
    if (!eng || !al || !pat || !txt) return nv_null();
    return nv_tb_device_run(eng, al, nullptr, al, n, pat, txt, max_p, max_t, {scores, sources, sinks, ops, ops_stride, n_ops},
                            stream);
}

int gasalx_nv_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *pat,
                             uint64_t pat_words, const gasalx_nv_strings *txt, uint64_t txt_words, int32_t *scores,
                             uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops) {
    const NvTbOut out = {scores, sources, sinks, ops, ops_stride, n_ops};
    if (!eng || !al || !nv_sets_ok(pat, txt) || !nv_tb_out_ok(out)) return nv_null();
    return nv_tb_host_run(eng, al, nullptr, 0, al, {n, pat, pat_words, txt, txt_words}, out);
}

int gasalx_nv_matrix_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                                      uint32_t n, const gasalx_nv_strings *pat, const gasalx_nv_strings *txt,
                                      uint32_t max_p, uint32_t max_t, int32_t *scores, uint32_t *sources,
                                      uint32_t *sinks, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops,
                                      void *stream) {
    const NvTbOut out = {scores, sources, sinks, ops, ops_stride, n_ops};
    if (!eng || !al || !mat || !nv_sets_ok(pat, txt) || !nv_tb_out_ok(out)) return nv_null();
    gasalx_nv_aligner ranged;
    if (int rc = nv_mtb_checks(al, mat, pat, txt, &ranged)) return rc;
    return nv_tb_device_run(eng, al, mat, &ranged, n, pat, txt, max_p, max_t, out, stream);
}

int gasalx_nv_matrix_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                                    uint32_t n, const gasalx_nv_strings *pat, uint64_t pat_words,
                                    const gasalx_nv_strings *txt, uint64_t txt_words, int32_t *scores,
                                    uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                                    uint32_t *n_ops) {
    const NvTbOut out = {scores, sources, sinks, ops, ops_stride, n_ops};
    if (!eng || !al || !mat || !nv_sets_ok(pat, txt) || !nv_tb_out_ok(out)) return nv_null();
    gasalx_nv_aligner ranged;
    if (int rc = nv_mtb_checks(al, mat, pat, txt, &ranged)) return rc;
    return nv_tb_host_run(eng, al, mat, 0, &ranged, {n, pat, pat_words, txt, txt_words}, out);
}

int gasalx_nv_banded_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t band, uint32_t n,
                                      const gasalx_nv_strings *pat, const gasalx_nv_strings *txt, uint32_t max_p,
                                      int32_t *scores, uint32_t *sources, uint32_t *sinks, uint8_t *ops,
                                      uint32_t ops_stride, uint32_t *n_ops, void *stream) {
    if (!eng || !al || !pat || !txt) return nv_null();
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = nv_device_enter(eng, stream, NV_PATTERN, n, pat, txt, &max_p, nullptr, &st);
    if (rc) return rc;
    if ((rc = nv_btb_checks(al, band, max_p, ops_stride))) return rc;
    const uint32_t chunk = (uint32_t)nv_tb_chunk(n, gasalx_nv_banded_traceback_workspace(max_p, band, 1));
    CK(eng->buf[B_NV_DIR].reserve((size_t)nv_btb_dir_bytes(max_p, band) * chunk + 64));
    return nv_tb_chunks(eng, al, nullptr, nullptr, band, n, pat, txt, max_p, 0, {scores, sources, sinks, ops, ops_stride, n_ops}, chunk, st);
}

int gasalx_nv_banded_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t band, uint32_t n,
                                    const gasalx_nv_strings *pat, uint64_t pat_words, const gasalx_nv_strings *txt,
                                    uint64_t txt_words, int32_t *scores, uint32_t *sources, uint32_t *sinks,
                                    uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops) {
    const NvTbOut out = {scores, sources, sinks, ops, ops_stride, n_ops};
    if (!eng || !al || !nv_sets_ok(pat, txt) || !nv_tb_out_ok(out)) return nv_null();
    if (int rc = nv_btb_checks(al, band, max_span(pat->offsets, n), ops_stride)) return rc;
    return nv_tb_host_run(eng, al, nullptr, band, nullptr, {n, pat, pat_words, txt, txt_words}, out);
}

int gasalx_nv_banded_qual_score_device(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_quals *q,
                                       uint32_t band, uint32_t n, const gasalx_nv_strings *pat,
                                       const gasalx_nv_strings *txt, int32_t *scores, uint32_t *sinks, uint32_t max_p,
                                       void *stream) {
    if (!eng || !al || !q || !pat || !txt) return nv_null();
    if (int rc = nv_qual_checks(al, q, band, pat, txt, nullptr)) return rc;
    hipStream_t st;
    if (int rc = nv_device_enter(eng, stream, NV_PATTERN_IF_OFFSETS, n, pat, txt, &max_p, nullptr, &st)) return rc;
    return gx::nv_banded_qual_score_device(*al, q, band, n, *pat, *txt, scores, sinks, st, max_p);
}

int gasalx_nv_describe_banded_qual_plan(const gasalx_nv_aligner *al, const gasalx_nv_quals *q, uint32_t band,
                                        uint32_t max_p, uint32_t text_bits, int want_traceback, char *buf,
                                        uint32_t buf_len) {
    return nv_describe(al && q, buf, buf_len, [&](std::string &s) {
        return gx::nv_banded_qual_plan_name(*al, q, band, max_p, text_bits, want_traceback != 0, s);
    });
}

int gasalx_nv_banded_qual_score_host(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_quals *q,
                                     uint32_t band, uint32_t n, const gasalx_nv_strings *pat, uint64_t pat_words,
                                     const gasalx_nv_strings *txt, uint64_t txt_words, int32_t *scores,
                                     uint32_t *sinks) {
    if (!eng || !al || !q || !nv_sets_ok(pat, txt) || (!scores && !sinks)) return nv_null();
    if (int rc = nv_qual_checks(al, q, band, pat, txt, nullptr)) return rc;
    const NvHostIn in = {n, pat, pat_words, txt, txt_words};
    return nv_score_host_run(eng, in, {{scores, B_NV_S, 4}, {sinks, B_NV_SNK, 8}},
                             [&](const NvStaged &s, void *const *d, hipStream_t st) {
                                 gasalx_nv_quals dq;
                                 if (int rc = nv_stage_quals(eng, in, q, st, dq)) return rc;
                                 return gx::nv_banded_qual_score_device(*al, &dq, band, n, s.pat, s.txt, (int32_t *)d[0],
                                                                        (uint32_t *)d[1], st, s.max_p);
                             });
}

int gasalx_nv_banded_qual_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_quals *q,
                                           uint32_t band, uint32_t n, const gasalx_nv_strings *pat,
                                           const gasalx_nv_strings *txt, uint32_t max_p, int32_t *scores,
                                           uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                                           uint32_t *n_ops, void *stream) {
    if (!eng || !al || !q || !pat || !txt) return nv_null();
    gasalx_nv_aligner ranged;
    if (int rc = nv_qual_checks(al, q, band, pat, txt, &ranged)) return rc;
    if (n == 0) return GASALX_OK;
    hipStream_t st;
    int rc = nv_device_enter(eng, stream, NV_PATTERN, n, pat, txt, &max_p, nullptr, &st);
    if (rc) return rc;
    if ((rc = nv_btb_checks(&ranged, band, max_p, ops_stride))) return rc;
    const uint32_t chunk = (uint32_t)nv_tb_chunk(n, gasalx_nv_banded_traceback_workspace(max_p, band, 1));
    CK(eng->buf[B_NV_DIR].reserve((size_t)nv_btb_dir_bytes(max_p, band) * chunk + 64));
    return nv_tb_chunks(eng, al, nullptr, q, band, n, pat, txt, max_p, 0, {scores, sources, sinks, ops, ops_stride, n_ops},
                        chunk, st);
}

int gasalx_nv_banded_qual_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_quals *q,
                                         uint32_t band, uint32_t n, const gasalx_nv_strings *pat, uint64_t pat_words,
                                         const gasalx_nv_strings *txt, uint64_t txt_words, int32_t *scores,
                                         uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                                         uint32_t *n_ops) {
    const NvTbOut out = {scores, sources, sinks, ops, ops_stride, n_ops};
    if (!eng || !al || !q || !nv_sets_ok(pat, txt) || !nv_tb_out_ok(out)) return nv_null();
    gasalx_nv_aligner ranged;
    if (int rc = nv_qual_checks(al, q, band, pat, txt, &ranged)) return rc;
    if (int rc = nv_btb_checks(&ranged, band, max_span(pat->offsets, n), ops_stride)) return rc;
    return nv_tb_host_run(eng, al, nullptr, band, nullptr, {n, pat, pat_words, txt, txt_words}, out, q);
}

int gasalx_pairhmm_params(const uint8_t *bq, const uint8_t *iq, const uint8_t *dq, uint32_t n, float *qm,
                          float *delta, float *xiksi, float *alpha) {
    if (n && (!bq || !iq || !dq || !qm || !delta || !xiksi || !alpha)) return GASALX_EINVAL;
    float ph2pr[128];
    ph2pr_table(ph2pr);
    for (uint32_t k = 0; k < n; k++) {                                         // :415-419
        qm[k] = ph2pr[bq[k] & 127];
        delta[k] = ph2pr[iq[k] & 127];
        xiksi[k] = ph2pr[dq[k] & 127];
        alpha[k] = 1.0f - ph2pr[((int)(iq[k] & 127) + (int)(dq[k] & 127)) & 127];
    }
    return GASALX_OK;
}

int gasalx_host_alloc(uint64_t bytes, void **out) {
    if (!out) { gx::set_error("gasalx_host_alloc: null output"); return GASALX_EINVAL; }
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        *out = nullptr;
        gx::set_error(std::string("hipHostMalloc: ") + hipGetErrorString(e));
        return GASALX_ENOMEM;
    }
    return GASALX_OK;
}

int gasalx_host_free(void *p) {
    if (!p) return GASALX_OK;
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) { gx::set_error(std::string("hipHostFree: ") + hipGetErrorString(e)); return GASALX_EDEVICE; }
    return GASALX_OK;
}

// Diagnostics (gasalx.h): the last packed launch's "aligned here" flags of each workspace.
int gasalx_packed_pairs(gasalx_engine *e, uint64_t *handled, uint64_t *total) {
    if (!e || !handled || !total) { gx::set_error("gasalx_packed_pairs: NULL argument"); return GASALX_EINVAL; }
    *handled = *total = 0;
    CK(hipSetDevice(e->device));
    auto one = [&](gx::Workspace &ws, hipStream_t st) -> int {
        if (st) CK(hipStreamSynchronize(st));
        if (!ws.pk_flags || !ws.misc.p) return GASALX_OK;
        std::vector<uint8_t> f(ws.pk_flags);
        CK(hipMemcpy(f.data(), ws.misc.p, f.size(), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < ws.pk_flags; i++) {
            // (a mixed-shape launch: the blocks from pk_b1 on cover pk_ppb2 pairs from pk_p1 on)
            const bool t2 = ws.pk_p1 != 0xFFFFFFFFu && i >= ws.pk_b1;
            const uint64_t lo = t2 ? (uint64_t)ws.pk_p1 + (uint64_t)(i - ws.pk_b1) * ws.pk_ppb2 : (uint64_t)i * ws.pk_ppb;
            const uint64_t hi = std::min<uint64_t>(lo + (t2 ? ws.pk_ppb2 : ws.pk_ppb), ws.pk_pairs);
            if (hi > lo && f[i]) *handled += hi - lo;
        }
        *total += ws.pk_pairs;
        ws.pk_flags = 0;   // read once: the next call counts only launches after this one
        return GASALX_OK;
    };
    int rc;
    if ((rc = one(e->ws, e->stream))) return rc;
    for (HostSlot &s : e->slot)
        if ((rc = one(s.ws, s.st))) return rc;
    return GASALX_OK;
}

}  // extern "C"
