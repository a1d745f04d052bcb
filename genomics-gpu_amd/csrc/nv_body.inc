// nv_body.inc — the body of nv_kernel (nvbio.hpp) and of its sink-tracking form (nvbio_sink.hpp),
// included into both kernels: the including scope defines the template parameters, A (the
// arguments), SINK (constexpr bool) and sinks (uint32_t *, 2 per pair, or NULL).
// SINK (nvbio_sink.hpp): also track where the BestSink score was reached and
// write it to sinks[2 * pair ..]; pad rows and columns are then always masked (a pad cell may
// tie with a real one), whatever MASK says.
    extern __shared__ __attribute__((aligned(16))) uint16_t nvlds[];
    constexpr int P = 64 / G;
    constexpr bool GOTOH = ALN == NV_GOTOH;
    constexpr uint32_t SB = GOTOH ? 3 : 4;        // SINK: log2 of the report stripe (nvbio_sink.hpp)
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lg = lane & (G - 1), slot = lane / G;
    const uint32_t pair = (blockIdx.x * 4 + wave) * P + slot;
    const bool valid = pair < A.n;
    const bool shared_text = A.toff == nullptr;
    uint32_t M = 0, N = 0, po = 0, to = 0;
    if (valid) {
        po = A.poff[pair]; M = A.poff[pair + 1] - po;
        if (shared_text) N = A.tlen0;
        else { to = A.toff[pair]; N = A.toff[pair + 1] - to; }
    }
    const uint32_t stride = A.lds_stride;
    // ---- text codes in LDS (one copy per block when shared) ----
    uint16_t *mine;
    if (shared_text) {
        for (uint32_t i = threadIdx.x; i < stride; i += blockDim.x)
            nvlds[i] = i < A.tlen0 ? (uint16_t)nv_symbol(A.tw, A.tbits, A.tbig, i) : (uint16_t)0xFFFF;
        mine = nvlds;
    } else {
        uint16_t *wl = nvlds + (size_t)wave * P * stride;
        for (uint32_t ps = 0; ps < (uint32_t)P; ps++) {   // uniform trip counts: shuffles see all lanes
            const uint32_t pN = __shfl(N, ps * G), pto = __shfl(to, ps * G);
            for (uint32_t i = lane; i < stride; i += 64)
                wl[ps * stride + i] = i < pN ? (uint16_t)nv_symbol(A.tw, A.tbits, A.tbig, pto + i) : (uint16_t)0xFFFF;
        }
        mine = wl + slot * stride;
    }
    __syncthreads();

    // ---- the lane's pattern rows ----
    const uint32_t r0 = lg * R;
    const uint32_t nrow = M > r0 ? min(M - r0, (uint32_t)R) : 0u;   // SINK: real rows of this lane
    uint32_t pc[R];
    int32_t Hk[R], Ek[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t r = r0 + k;
        pc[k] = (valid && r < M) ? nv_symbol(A.pw, A.pbits, A.pbig, po + r) : 0xFFFEu;
        if (GOTOH) {
            Hk[k] = TYPE == NV_LOCAL ? 0 : A.go + A.ge * (int32_t)r;
            Ek[k] = TYPE == NV_LOCAL ? 0 : kNvInf;
        } else {
            Hk[k] = TYPE == NV_LOCAL ? 0 : A.ins * (int32_t)(r + 1);
            Ek[k] = 0;
        }
    }
    uint32_t nmax = N;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor(nmax, m));
    const uint32_t nsteps = nmax + G - 1;
    const uint32_t last_lane = M ? (M - 1) / R : 0, last_k = M ? (M - 1) - last_lane * R : 0;
    int32_t best = INT32_MIN;                     // BestSink() (sink_inl.h:38-40)
    uint32_t bcol = 0xFFFFFFFFu;                  // SINK, SEMI_GLOBAL: zero-based column of `best`
    long long bc = -1;                            // SINK, LOCAL: H << 32 | key; H >= 0, so -1 is "no cell"
    // from the lane above: H(r0-1, c), F(r0-1, c), H(r0-1, c-1).  rH starts as the left
    // boundary H(r0-1, -1): lane 1 takes it as its diagonal at column 0 (lane 0 never
    // runs a column -1 step to hand it down)
    const int32_t rb = (int32_t)r0 - 1;
    int32_t rH = (TYPE == NV_LOCAL || lg == 0) ? 0 : (GOTOH ? A.go + A.ge * rb : A.ins * (rb + 1));
    int32_t rF = kNvInf, pH = 0;
    for (uint32_t s = 0; s < nsteps; ++s) {
        const int32_t c = (int32_t)s - (int32_t)lg;
        int32_t Hup, Fup, Hdg;
        if (lg == 0) {
            if (TYPE == NV_GLOBAL) {
                Hup = GOTOH ? A.go + A.ge * c : A.del * (c + 1);
                Hdg = GOTOH ? (c >= 1 ? A.go + A.ge * (c - 1) : 0) : A.del * c;
            } else { Hup = 0; Hdg = 0; }
            Fup = kNvInf;
        } else { Hup = rH; Fup = rF; Hdg = pH; }
        if (c >= 0 && (uint32_t)c < stride) {
            const uint32_t tc = mine[c];
            const bool cin = (uint32_t)c < N;
            // SINK: report-order key of (r0, c); row r0 + k adds k << SB
            const uint32_t kb = ((((uint32_t)c >> SB) * M + r0) << SB) | ((uint32_t)c & ((1u << SB) - 1u));
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int32_t S = (pc[k] == tc) ? A.match : A.mismatch;
                int32_t H;
                if (GOTOH) {
                    const int32_t F = max(Fup + A.ge, Hup + A.go);
                    const int32_t E = max(Ek[k] + A.ge, Hk[k] + A.go);
                    H = max(max(E, F), Hdg + S);
                    Ek[k] = E;
                    Fup = F;
                } else {
                    H = max(max(Hup + A.ins, Hk[k] + A.del), Hdg + S);
                }
                if (TYPE == NV_LOCAL) {
                    H = max(H, 0);
                    if constexpr (SINK) {
                        const long long cand = ((long long)H << 32) | (long long)(kb + ((uint32_t)k << SB));
                        bc = (cin && (uint32_t)k < nrow && cand > bc) ? cand : bc;
                    } else if (MASK) best = (cin && r0 + k < M) ? max(best, H) : best;
                    else best = max(best, H);
                }
                Hdg = Hk[k];
                Hk[k] = H;
                Hup = H;
            }
            if (TYPE != NV_LOCAL && lg == last_lane && cin) {
                int32_t h = 0;
#pragma unroll
                for (int k = 0; k < R; ++k) h = (k == (int)last_k) ? Hk[k] : h;
                if (TYPE == NV_SEMI && SINK) {
                    if (h >= best) { best = h; bcol = (uint32_t)c; }   // columns come in order: the last maximum
                } else if (TYPE == NV_SEMI) best = max(best, h);
                else if ((uint32_t)c == N - 1) best = h;
            }
        }
        // hand the bottom row down: H(r0+R-1, c) once active; before that Hk[R-1] still
        // holds the row's left boundary H(r0+R-1, -1), the diagonal the lane below needs
        // at its column 0
        pH = rH;
        rH = nv_shr(Hk[R - 1]);
        rF = nv_shr(Fup);
    }
    // LOCAL: the pair's best over its lanes
    if (TYPE == NV_LOCAL && SINK) {   // the greatest (H, key)
#pragma unroll
        for (int m = 1; m < G; m <<= 1) {
            const long long o = __shfl_xor(bc, m);
            bc = o > bc ? o : bc;
        }
    } else if (TYPE == NV_LOCAL) {
#pragma unroll
        for (int m = 1; m < G; m <<= 1) best = max(best, __shfl_xor(best, m));
    }
    const bool writer = TYPE == NV_LOCAL ? lg == 0 : lg == last_lane;
    if (valid && writer) {
        int32_t v = best;
        uint32_t x = N, y = M;                    // SINK: the cell, one-based; GLOBAL: (N, M)
        if constexpr (SINK) {
            if (TYPE == NV_SEMI) x = bcol + 1;
            if (TYPE == NV_LOCAL && bc >= 0) {
                v = (int32_t)(bc >> 32);
                const uint32_t key = (uint32_t)bc, q = key >> SB, sb = q / M;   // bc >= 0: a real row, M >= 1
                x = (sb << SB) + (key & ((1u << SB) - 1u)) + 1;
                y = q - sb * M + 1;
            }
        }
        if (M == 0) {   // no pattern rows: only the band initialisation reaches the sink
            v = TYPE == NV_SEMI ? (N ? 0 : INT32_MIN)
              : TYPE == NV_GLOBAL ? (N ? (GOTOH ? A.go + A.ge * (int32_t)(N - 1) : A.del * (int32_t)N) : INT32_MIN)
                                  : INT32_MIN;
        } else if (N == 0) v = INT32_MIN;
        if (A.score) A.score[pair] = v;
        if (A.score16) A.score16[pair] = (int16_t)v;   // sw-benchmark's int16 score vector
        if constexpr (SINK) {
            if (M == 0) x = N;                    // the band initialisation, reported at y = 0
            if (N == 0 || (TYPE == NV_LOCAL && M == 0)) x = y = 0xFFFFFFFFu;   // no cell was reported
            if (sinks) { sinks[2 * (size_t)pair] = x; sinks[2 * (size_t)pair + 1] = y; }
        }
    }
