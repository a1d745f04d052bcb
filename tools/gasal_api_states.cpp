// gasal_api_states.cpp — scenario client of the drop-in C++ API (include/gasal_header.h, -lgasal).
//
// It takes the host state machine of the API through the states that a caller who initialises
// its streams from estimates reaches (BWA-GASAL2's way): page chains that grow and are reused,
// gasal_host_alns_resize in the middle of a fill, the device growth paths of gasal_aln_async,
// several storages in different states, gasal_gpu_mem_free / gasal_gpu_mem_alloc, and
// gasal_host_batch_add / addbase / getlast.  It decides nothing itself: a scenario file says what
// to do, a dump file records what the library did, and tests/test_gpu_gasal_api_states.py
// compares the dump with the page-chain model and with the two alignment references.
//
//   gasal_api_states scenario.txt dump.txt
//
// Scenario file, one command per line (numbers decimal, bytes as hex, "-" = no bytes):
//   params ALGO START_POS SECOND HEAD TAIL K_BAND IS_PACKED IS_RC       (first four lines, in
//   scores MATCH MISMATCH GAP_OPEN GAP_EXTEND                            this order)
//   init MAX_QUERY_LEN MAX_TARGET_LEN MAX_N_ALNS
//   storages N
//   round ST N RESIZE_AT NEW_N     then N lines  pair QHEX THEX QLEN TLEN QOP TOP SEED
//       fills storage ST and launches it.  RESIZE_AT = k >= 0: pairs 0..k-1 are filled and their
//       ops handed over with gasal_op_fill, then gasal_host_alns_resize(ST, NEW_N) is called and
//       the fill goes on (ops of the later pairs are written to host_*_op directly, so that the
//       first k are the ones the resize carried over).  QHEX / THEX are the bytes given to
//       gasal_host_batch_fill; offsets and the batch bytes are the fill index, times 2 with
//       IS_PACKED (offsets count bases, a packed byte holds two).
//   collect ST                     waits for ST (bounded), dumps the protocol values and results
//   memcycle ST QBYTES TBYTES N    gasal_gpu_mem_free then gasal_gpu_mem_alloc on ST
//   fill SRC ST IDX HEX            gasal_host_batch_fill alone, dumps the returned index
//   add SRC ST IDX HEX             gasal_host_batch_add (one byte: gasal_host_batch_addbase)
//   pages ST                       dumps both chains of ST with the bytes of every page
// The dump format is described where it is written (dump_*).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gasal_header.h"

namespace {

constexpr double WAIT_SECONDS = 60.0;   // a batch of some dozens of pairs takes milliseconds

[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "gasal_api_states: %s\n", msg.c_str());
    exit(2);
}

std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    if (s.size() % 2) die("odd hex string");
    auto nib = [](char c) -> int {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        die("bad hex digit");
    };
    for (size_t i = 0; i < s.size(); i += 2) out.push_back((uint8_t)(nib(s[i]) << 4 | nib(s[i + 1])));
    return out;
}

void hex(FILE *f, const uint8_t *p, size_t n) {
    if (n == 0) fputc('-', f);
    for (size_t i = 0; i < n; ++i) fprintf(f, "%02x", p[i]);
}

data_source src_of(const std::string &s) {
    if (s == "q") return QUERY;
    if (s == "t") return TARGET;
    die("source must be q or t");
}

// chain SRC NPAGES, then per page: page SRC OFFSET DATA_SIZE PAGE_SIZE IS_LOCKED [HEX of the page]
void dump_chain(FILE *f, const char *name, const host_batch_t *head, bool bytes) {
    int pages = 0;
    for (const host_batch_t *p = head; p; p = p->next) ++pages;
    fprintf(f, "chain %s %d\n", name, pages);
    for (const host_batch_t *p = head; p; p = p->next) {
        fprintf(f, "page %s %u %u %u %d", name, p->offset, p->data_size, p->page_size, p->is_locked);
        if (bytes) { fputc(' ', f); hex(f, p->data, p->page_size); }
        fputc('\n', f);
    }
}

void dump_state(FILE *f, const gasal_gpu_storage_t *st, bool bytes = false) {
    dump_chain(f, "q", st->extensible_host_unpacked_query_batch, bytes);
    dump_chain(f, "t", st->extensible_host_unpacked_target_batch, bytes);
    fprintf(f, "hostmax %u %u %u\n", st->host_max_query_batch_bytes, st->host_max_target_batch_bytes,
            st->host_max_n_alns);
}

void dump_array(FILE *f, const char *name, const int32_t *a, uint32_t n) {
    if (!a) return;
    fprintf(f, "%s", name);
    for (uint32_t i = 0; i < n; ++i) fprintf(f, " %d", a[i]);
    fputc('\n', f);
}

// every non-NULL result array: res FIELD v0 v1 .., res2 FIELD .. for the second-best block
void dump_results(FILE *f, const gasal_gpu_storage_t *st, uint32_t n, uint32_t qbytes, const Parameters &P) {
    const gasal_res_t *r = st->host_res;
    dump_array(f, "res score", r->aln_score, n);
    dump_array(f, "res q_end", r->query_batch_end, n);
    dump_array(f, "res t_end", r->target_batch_end, n);
    dump_array(f, "res q_start", r->query_batch_start, n);
    dump_array(f, "res t_start", r->target_batch_start, n);
    if (const gasal_res_t *r2 = st->host_res_second) {
        dump_array(f, "res2 score", r2->aln_score, n);
        dump_array(f, "res2 q_end", r2->query_batch_end, n);
        dump_array(f, "res2 t_end", r2->target_batch_end, n);
        dump_array(f, "res2 q_start", r2->query_batch_start, n);
        dump_array(f, "res2 t_start", r2->target_batch_start, n);
    }
    if (P.start_pos == WITH_TB) {
        dump_array(f, "res n_ops", (const int32_t *)r->n_cigar_ops, n);
        fprintf(f, "cigar ");
        hex(f, r->cigar, qbytes);
        fputc('\n', f);
    }
}

struct Flight { uint32_t n = 0, qbytes = 0; bool busy = false; };

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) die("usage: gasal_api_states scenario.txt dump.txt");
    std::ifstream in(argv[1]);
    if (!in) die("cannot read the scenario file");
    FILE *out = fopen(argv[2], "w");
    if (!out) die("cannot write the dump file");

    Parameters *args = new Parameters(0, nullptr);
    gasal_gpu_storage_v vec;
    vec.n = 0; vec.a = nullptr;
    std::vector<Flight> flight;
    int max_q = 0, max_t = 0, max_n = 0, round_no = 0;
    bool ready = false;

    auto storage = [&](int s) -> gasal_gpu_storage_t * {
        if (!ready || s < 0 || s >= vec.n) die("storage index out of range, or used before `storages`");
        return &vec.a[s];
    };

    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        std::string cmd;
        ls >> cmd;
        if (cmd == "params") {
            int algo, sp, second, head, tail, kb, packed, rc;
            if (!(ls >> algo >> sp >> second >> head >> tail >> kb >> packed >> rc)) die("bad params line");
            args->algo = (algo_type)algo; args->start_pos = (comp_start)sp; args->secondBest = second ? TRUE : FALSE;
            args->semiglobal_skipping_head = (data_source)head; args->semiglobal_skipping_tail = (data_source)tail;
            args->k_band = kb; args->isPacked = packed != 0; args->isReverseComplement = rc != 0;
        } else if (cmd == "scores") {
            if (!(ls >> args->sa >> args->sb >> args->gapo >> args->gape)) die("bad scores line");
            gasal_subst_scores sc;
            sc.match = args->sa; sc.mismatch = args->sb; sc.gap_open = args->gapo; sc.gap_extend = args->gape;
            gasal_copy_subst_scores(&sc);
        } else if (cmd == "init") {
            if (!(ls >> max_q >> max_t >> max_n)) die("bad init line");
        } else if (cmd == "storages") {
            int n = 0;
            if (!(ls >> n) || n < 1 || n > 8 || max_n <= 0) die("bad storages line");
            vec = gasal_init_gpu_storage_v(n);
            gasal_init_streams(&vec, max_q, max_t, max_n, args);
            flight.assign(n, Flight());
            ready = true;
        } else if (cmd == "round") {
            int s, n, resize_at, new_n;
            if (!(ls >> s >> n >> resize_at >> new_n) || n < 1) die("bad round line");
            gasal_gpu_storage_t *st = storage(s);
            if (flight[s].busy) die("round on a storage that is in flight");
            const uint32_t mult = args->isPacked ? 2 : 1;
            fprintf(out, "round %d st %d n %d\n", round_no++, s, n);
            fprintf(out, "pre %d\n", gasal_is_aln_async_done(st));
            std::vector<uint8_t> qops(n), tops(n);
            uint32_t qidx = 0, tidx = 0;
            const bool resizes = resize_at >= 0;
            for (int j = 0; j < n; ++j) {
                std::string pl, word, qh, th;
                uint32_t ql, tl, qop, top, seed;
                if (!std::getline(in, pl)) die("round: pair lines missing");
                std::istringstream ps(pl);
                if (!(ps >> word >> qh >> th >> ql >> tl >> qop >> top >> seed) || word != "pair") die("bad pair line");
                if (j == resize_at) {
                    gasal_op_fill(st, qops.data(), j, QUERY);
                    gasal_op_fill(st, tops.data(), j, TARGET);
                    gasal_host_alns_resize(st, new_n, args);
                    fprintf(out, "resized %u\n", st->host_max_n_alns);
                }
                if ((uint32_t)j >= st->host_max_n_alns) die("round: more pairs than host_max_n_alns and no resize");
                const std::vector<uint8_t> q = unhex(qh), t = unhex(th);
                st->host_query_batch_offsets[j] = qidx * mult;
                st->host_target_batch_offsets[j] = tidx * mult;
                st->host_query_batch_lens[j] = ql;
                st->host_target_batch_lens[j] = tl;
                qidx = gasal_host_batch_fill(st, qidx, (const char *)q.data(), (uint32_t)q.size(), QUERY);
                tidx = gasal_host_batch_fill(st, tidx, (const char *)t.data(), (uint32_t)t.size(), TARGET);
                qops[j] = (uint8_t)qop; tops[j] = (uint8_t)top;
                if (resizes && j >= resize_at) { st->host_query_op[j] = qops[j]; st->host_target_op[j] = tops[j]; }
                if (args->algo == KSW) st->host_seed_scores[j] = seed;
            }
            if (!resizes) {
                gasal_op_fill(st, qops.data(), n, QUERY);
                gasal_op_fill(st, tops.data(), n, TARGET);
            }
            fprintf(out, "filled %u %u\n", qidx, tidx);
            dump_state(out, st);
            st->current_n_alns = n;
            gasal_aln_async(st, qidx * mult, tidx * mult, n, args);
            st->current_n_alns = 0;
            fprintf(out, "gpumax %u %u %u\n", st->gpu_max_query_batch_bytes, st->gpu_max_target_batch_bytes,
                    st->gpu_max_n_alns);
            flight[s].n = n; flight[s].qbytes = qidx * mult; flight[s].busy = true;
        } else if (cmd == "collect") {
            int s;
            if (!(ls >> s)) die("bad collect line");
            gasal_gpu_storage_t *st = storage(s);
            if (!flight[s].busy) die("collect on an idle storage");
            const auto t0 = std::chrono::steady_clock::now();
            int v;
            while ((v = gasal_is_aln_async_done(st)) == -1)
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > WAIT_SECONDS) {
                    fprintf(stderr, "gasal_api_states: storage %d not done after %.0f s\n", s, WAIT_SECONDS);
                    fclose(out);
                    return 3;
                }
            fprintf(out, "collect st %d\n", s);
            fprintf(out, "done %d is_free %d\n", v, st->is_free);
            dump_state(out, st);
            fprintf(out, "after %d is_free %d\n", gasal_is_aln_async_done(st), st->is_free);
            dump_results(out, st, flight[s].n, flight[s].qbytes, *args);
            flight[s].busy = false;
        } else if (cmd == "memcycle") {
            int s, qb, tb, na;
            if (!(ls >> s >> qb >> tb >> na)) die("bad memcycle line");
            gasal_gpu_storage_t *st = storage(s);
            if (flight[s].busy) die("memcycle on a storage that is in flight");
            gasal_gpu_mem_free(st, args);
            gasal_gpu_mem_alloc(st, qb, tb, na, args);
            fprintf(out, "memcycle st %d\ngpumax %u %u %u\n", s, st->gpu_max_query_batch_bytes,
                    st->gpu_max_target_batch_bytes, st->gpu_max_n_alns);
        } else if (cmd == "fill" || cmd == "add") {
            std::string src, h;
            int s;
            uint32_t idx;
            if (!(ls >> src >> s >> idx >> h)) die("bad fill/add line");
            gasal_gpu_storage_t *st = storage(s);
            const std::vector<uint8_t> b = unhex(h);
            uint32_t r;
            if (cmd == "fill") r = gasal_host_batch_fill(st, idx, (const char *)b.data(), (uint32_t)b.size(), src_of(src));
            else if (b.size() == 1) r = gasal_host_batch_addbase(st, idx, (char)b[0], src_of(src));
            else r = gasal_host_batch_add(st, idx, (const char *)b.data(), (uint32_t)b.size(), src_of(src));
            fprintf(out, "%s %s ret %u\n", cmd.c_str(), src.c_str(), r);
        } else if (cmd == "pages") {
            int s;
            if (!(ls >> s)) die("bad pages line");
            gasal_gpu_storage_t *st = storage(s);
            fprintf(out, "pages st %d\n", s);
            dump_state(out, st, true);
            // the page gasal_host_batch_getlast returns, as its index in the chain
            for (host_batch_t *head : {st->extensible_host_unpacked_query_batch, st->extensible_host_unpacked_target_batch}) {
                const host_batch_t *last = gasal_host_batch_getlast(head);
                int k = 0, at = -1;
                for (const host_batch_t *p = head; p; p = p->next, ++k)
                    if (p == last) at = k;
                fprintf(out, "getlast %d\n", at);
            }
        } else {
            die("unknown command: " + cmd);
        }
    }
    for (size_t s = 0; s < flight.size(); ++s)
        if (flight[s].busy) die("scenario ends with a storage in flight");
    if (ready) {
        gasal_destroy_streams(&vec, args);
        gasal_destroy_gpu_storage_v(&vec);
    }
    fprintf(out, "end\n");
    fclose(out);
    delete args;
    return 0;
}
