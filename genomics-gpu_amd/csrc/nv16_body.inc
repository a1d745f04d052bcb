// nv16_body.inc — the body of nv16_sink_kernel (nvbio_sink.hpp): nv16_kernel's (nvbio16.hpp) with
// the BestSink position tracked per half.  It is a copy, not shared text: with the tracking
// compiled out, the shared form gave 27 of the 108 score-only nv16_kernel instances other code
// than before, and those instances must keep theirs.  A change to nv16_kernel's recurrences or
// boundaries is made here too.  The including scope defines the template parameters, A (the
// arguments), SINK (constexpr bool, true) and sinks (uint32_t *, 2 per pair, or NULL).
// Both halves of a lane sit on the same row and column, so one report-order key serves both:
// key(i, c) = (c >> SB) << (SB + 10) | i << SB | (c & (2^SB - 1)), SB = 3 for Gotoh and 4 for SW and ED
// (the report stripe, nvbio_sink.hpp; rows < 1024: 10 bits; no pattern length in it).  LOCAL
// keeps H << 32 | key per half in place of the packed running maximum; SEMI_GLOBAL a column per
// half on the lane that owns the half's last row.
    extern __shared__ __attribute__((aligned(16))) uint32_t nvt[];
    constexpr int P = 64 / G;
    constexpr bool GOTOH = ALN == NV_GOTOH;
    constexpr bool FR = GOTOH && TYPE != NV_LOCAL;   // the drift frame (header)
    constexpr uint32_t SB = GOTOH ? 3 : 4;           // SINK: log2 of the report stripe
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lg = lane & (G - 1), grp = lane / G;
    const uint32_t pa = 2 * ((blockIdx.x * 4 + wave) * P + grp), pb = pa + 1;
    const bool va = pa < A.n, vb = pb < A.n;
    uint32_t Ma = 0, Mb = 0, poa = 0, pob = 0;
    if (va) { poa = A.poff[pa]; Ma = A.poff[pa + 1] - poa; }
    if (vb) { pob = A.poff[pb]; Mb = A.poff[pb + 1] - pob; }
    // ---- the text(s) as per-column tables (pads: all mismatch) ----
    const uint32_t dm = (uint32_t)(A.match - A.mismatch);
    const uint32_t cols = A.lds_cols;
    uint32_t Na = A.tlen0, Nb = A.tlen0, toa = 0, tob = 0;
    const uint32_t *Ta = nvt, *Tb = nvt;
    if (SHARED) {
        for (uint32_t c = threadIdx.x; c < cols; c += blockDim.x)
            nvt[c] = c < Na ? dm << (8 * nv_symbol(A.tw, 2, A.tbig, c)) : 0u;
    } else {
        // one slot per pair of the wave: slot 2*grp + half
        Na = Nb = 0;
        if (va) { toa = A.toff[pa]; Na = A.toff[pa + 1] - toa; }
        if (vb) { tob = A.toff[pb]; Nb = A.toff[pb + 1] - tob; }
        uint32_t *wl = nvt + (size_t)wave * 2 * P * cols;
        for (uint32_t ps = 0; ps < 2u * P; ++ps) {   // uniform trip counts: shuffles see all lanes
            const uint32_t src = (ps >> 1) * G;
            const uint32_t pN = __shfl((ps & 1) ? Nb : Na, src), pto = __shfl((ps & 1) ? tob : toa, src);
            for (uint32_t c = lane; c < cols; c += 64)
                wl[ps * cols + c] = c < pN ? dm << (8 * nv_symbol(A.tw, 2, A.tbig, pto + c)) : 0u;
        }
        Ta = wl + 2 * grp * cols;
        Tb = Ta + cols;
    }
    __syncthreads();
    const uint32_t N = max(Na, Nb);

    const int32_t B = (int32_t)A.base;
    const uint32_t BB = A.base * 0x10001u, NEG = 0x04000400u;
    const uint32_t FLOOR = TYPE == NV_LOCAL ? BB : NEG;
    const uint32_t MIS = (uint32_t)A.mismatch * 0x10001u;
    const uint32_t GO = (uint32_t)(-A.go) * 0x10001u, GE = (uint32_t)(-A.ge) * 0x10001u;   // gaps <= 0
    const uint32_t DEL = (uint32_t)(-A.del) * 0x10001u, INS = (uint32_t)(-A.ins) * 0x10001u;
    auto pk = [&](int32_t v) { return (uint32_t)(v + B) * 0x10001u; };
    // ---- the lane's pattern rows ----
    // BOT (one shared text, SEMI_GLOBAL): rows bottom-aligned per half, so both pairs'
    // last row M-1 is row R-1 of lane G-1 and the sink is one maximum per step.  The
    // rows above row 0 are virtual: they score every column with the constant byte
    // |mismatch| (v_perm's second source, selector 4), so tmp = Hdg and, from the free
    // top boundary H = 0 (F = -inf), each passes H = 0 down unchanged (E and F stay
    // below it: gap scores <= 0) — row 0 sees exactly nvbio's boundary.
    constexpr bool BOT = SHARED && TYPE == NV_SEMI;
    const uint32_t VCONST = (uint32_t)(-A.mismatch);
    const int32_t ra0 = (int32_t)(lg * R) - (BOT ? (int32_t)(G * R - Ma) : 0);
    const int32_t rb0 = (int32_t)(lg * R) - (BOT ? (int32_t)(G * R - Mb) : 0);
    const uint32_t last_a = Ma ? Ma - 1 : 0xFFFFFFFFu, last_b = Mb ? Mb - 1 : 0xFFFFFFFFu;
    uint32_t sel[R], Hk[R], Ek[R], msk[R];
    bool has_last = false;
    auto left = [&](int32_t r) {   // H(r, -1); virtual rows: 0
        if (TYPE == NV_LOCAL || r < 0) return 0;
        return GOTOH ? A.go + A.ge * r : A.ins * (r + 1);
    };
    auto pk2 = [&](int32_t a, int32_t b) { return (uint32_t)(a + B) | ((uint32_t)(b + B) << 16); };
    const int32_t g = -A.ge, dl = A.go - A.ge;           // FR: drift per anti-diagonal, H^ offset
    // FR: H^ of H value h at (r, c)
    auto fr = [&](int32_t h, int32_t r, int32_t c) { return h + g * (r + c) + dl; };
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int32_t ra = ra0 + k, rb = rb0 + k;
        const uint32_t ca = (va && ra >= 0 && ra < (int32_t)Ma) ? nv_symbol(A.pw, A.pbits, A.pbig, poa + ra) : 4u;
        const uint32_t cb = (vb && rb >= 0 && rb < (int32_t)Mb) ? nv_symbol(A.pw, A.pbits, A.pbig, pob + rb) : 4u;
        // SHARED: both halves read the one table (v_perm(VCONST, T, .)); otherwise the
        // high half's bytes come from the second source, selectors 4..7
        const uint32_t sa = ra < 0 ? 4u : (ca < 4 ? ca : 0x0Cu);
        const uint32_t sb = rb < 0 ? 4u : (cb < 4 ? cb + (SHARED ? 0u : 4u) : 0x0Cu);
        sel[k] = sa | 0x0C00u | (sb << 16) | 0x0C000000u;
        Hk[k] = FR ? pk2(fr(left(ra), ra, -1), fr(left(rb), rb, -1)) : pk2(left(ra), left(rb));
        Ek[k] = GOTOH ? (TYPE == NV_LOCAL ? BB : NEG) : 0u;
        msk[k] = ((uint32_t)ra == last_a ? 0x0000FFFFu : 0u) | ((uint32_t)rb == last_b ? 0xFFFF0000u : 0u);
        has_last |= msk[k] != 0u;
    }
    uint32_t nmax = N;
    if (!SHARED) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor(nmax, m));
    }
    const uint32_t nsteps = nmax + G - 1;
    // per-half column limits of the sinks (SEMI: c < N of the half; GLOBAL: c == N - 1)
    const uint32_t lastc_a = Na - 1, lastc_b = Nb - 1;
    uint32_t best = TYPE == NV_LOCAL ? BB : NEG;   // stored; NEG = no cell seen (BestSink, sink_inl.h:38-40)
    // SINK.  LOCAL: stored H << 32 | key of either half (-1: no cell; rows are top-aligned here, so
    // the lane's real rows are the first nra / nrb); SEMI_GLOBAL: zero-based column of either best
    long long bca = -1, bcb = -1;
    uint32_t cola = 0xFFFFFFFFu, colb = 0xFFFFFFFFu;
    const uint32_t nra = Ma > lg * R ? min(Ma - lg * R, (uint32_t)R) : 0u;
    const uint32_t nrb = Mb > lg * R ? min(Mb - lg * R, (uint32_t)R) : 0u;
    // from the lane above: H(r0-1, c), F(r0-1, c), H(r0-1, c-1); rH starts as the
    // left boundary H(r0-1, -1), lane 1's diagonal at column 0 (nvbio.hpp)
    uint32_t rH = lg == 0 ? BB
                : FR ? pk2(fr(left(ra0 - 1), ra0 - 1, -1), fr(left(rb0 - 1), rb0 - 1, -1))
                     : pk2(left(ra0 - 1), left(rb0 - 1));
    const uint32_t MISF = (uint32_t)(A.mismatch + g - A.go) * 0x10001u, DL = (uint32_t)dl * 0x10001u;
    uint32_t rF = NEG, pH = BB;
    for (uint32_t s = 0; s < nsteps; ++s) {
        const int32_t c = (int32_t)s - (int32_t)lg;
        uint32_t Hup, Fup, Hdg;
        if (lg == 0) {
            if (FR) {   // H of the row above the lane's first (-1; BOT: virtual rows per half), in the frame
                const int32_t hu = TYPE == NV_GLOBAL ? A.go + A.ge * c : 0;
                const int32_t hd = TYPE == NV_GLOBAL && c >= 1 ? A.go + A.ge * (c - 1) : 0;
                Hup = pk2(fr(hu, ra0 - 1, c), fr(hu, rb0 - 1, c));
                Hdg = pk2(fr(hd, ra0 - 1, c - 1), fr(hd, rb0 - 1, c - 1));
            } else if (TYPE == NV_GLOBAL) {
                Hup = pk(GOTOH ? A.go + A.ge * c : A.del * (c + 1));
                Hdg = pk(GOTOH ? (c >= 1 ? A.go + A.ge * (c - 1) : 0) : A.del * c);
            } else { Hup = BB; Hdg = BB; }
            Fup = NEG;
        } else { Hup = rH; Fup = rF; Hdg = pH; }
        if (c >= 0 && (uint32_t)c < N) {
            const uint32_t T = Ta[c], T1 = SHARED ? VCONST : Tb[c];
            uint32_t lbest = best;
            const bool cina = SHARED || (uint32_t)c < Na, cinb = SHARED || (uint32_t)c < Nb;
            const uint32_t kb = (((uint32_t)c >> SB) << (SB + 10)) | ((lg * R) << SB) | ((uint32_t)c & ((1u << SB) - 1u));
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const uint32_t v = __builtin_amdgcn_perm(T1, T, sel[k]);
                const uint32_t tmp = Hdg + v + MIS;
                uint32_t H;
                if (FR) {
                    const uint32_t tmp2 = Hdg + v + MISF;
                    const uint32_t F = pk_max_u16(Fup, Hup);
                    const uint32_t E = pk_max_u16(Ek[k], Hk[k]);
                    H = pk_max3(E, F, tmp2) + DL;
                    Ek[k] = E;
                    Fup = F;
                } else if (GOTOH) {
                    const uint32_t F = pk_max3(Fup - GE, Hup - GO, FLOOR);
                    const uint32_t E = pk_max3(Ek[k] - GE, Hk[k] - GO, FLOOR);
                    H = pk_max3(E, F, tmp);
                    Ek[k] = E;
                    Fup = F;
                } else {
                    H = pk_max3(Hup - INS, Hk[k] - DEL, tmp);
                    if (TYPE == NV_LOCAL) H = pk_max3(H, BB, BB);
                }
                if (TYPE == NV_LOCAL && SINK) {
                    const uint32_t key = kb + ((uint32_t)k << SB);
                    const long long ca = ((long long)(H & 0xFFFFu) << 32) | (long long)key;
                    const long long cb = ((long long)(H >> 16) << 32) | (long long)key;
                    bca = (cina && (uint32_t)k < nra && ca > bca) ? ca : bca;
                    bcb = (cinb && (uint32_t)k < nrb && cb > bcb) ? cb : bcb;
                } else if (TYPE == NV_LOCAL) {   // two rows per maximum3: Hup is still row k - 1's H here
                    if (k & 1) lbest = pk_max3(lbest, H, Hup);
                    else if (k == R - 1) lbest = pk_max3(lbest, H, H);
                }
                Hdg = Hk[k];
                Hk[k] = H;
                Hup = H;
            }
            if (TYPE == NV_LOCAL) best = lbest;
            if (BOT) {
                // FR: the row's columns in one frame, + g*(N-1-c) (c < N here)
                const uint32_t kof = FR ? (uint32_t)(g * (int32_t)(N - 1 - (uint32_t)c)) * 0x10001u : 0u;
                if (lg == G - 1) {
                    const uint32_t hv = Hk[R - 1] + kof;
                    if constexpr (SINK) {   // columns come in order: >= keeps the last maximum
                        if ((hv & 0xFFFFu) >= (best & 0xFFFFu)) cola = (uint32_t)c;
                        if ((hv >> 16) >= (best >> 16)) colb = (uint32_t)c;
                    }
                    best = pk_max3(best, hv, best);
                }
            } else if (TYPE != NV_LOCAL && has_last) {
                uint32_t h = 0, hm = 0;
#pragma unroll
                for (int k = 0; k < R; ++k) { h |= Hk[k] & msk[k]; hm |= msk[k]; }
                if (TYPE == NV_SEMI) {   // a half without its last row here, or past its text: +0
                    if (!SHARED) hm &= ((uint32_t)c < Na ? 0x0000FFFFu : 0u) | ((uint32_t)c < Nb ? 0xFFFF0000u : 0u);
                    // FR: + g*(N-1-c) per half, masked first so that no add carries across
                    const uint32_t off = FR ? (((uint32_t)(g * (int32_t)(Na - 1 - (uint32_t)c)) & 0xFFFFu) |
                                               ((uint32_t)(g * (int32_t)(Nb - 1 - (uint32_t)c)) << 16)) & hm
                                            : 0u;
                    h = (h & hm) + off;
                    if constexpr (SINK) {   // a half masked out is 0, below every stored value
                        if ((h & 0xFFFFu) >= (best & 0xFFFFu)) cola = (uint32_t)c;
                        if ((h >> 16) >= (best >> 16)) colb = (uint32_t)c;
                    }
                    best = pk_max3(best, h, best);
                } else if (SHARED) {
                    if ((uint32_t)c == N - 1) best = h;
                } else {
                    if ((uint32_t)c == lastc_a) best = (best & 0xFFFF0000u) | (h & 0x0000FFFFu);
                    if ((uint32_t)c == lastc_b) best = (best & 0x0000FFFFu) | (h & 0xFFFF0000u);
                }
            }
        }
        pH = rH;
        rH = nv16_dpp(Hk[R - 1]);
        rF = nv16_dpp(Fup);
    }
    // LOCAL: the pair's best over its lanes
    if (TYPE == NV_LOCAL && SINK) {   // the greatest (H, key) of either half
#pragma unroll
        for (int m = 1; m < G; m <<= 1) {
            const long long oa = __shfl_xor(bca, m), ob = __shfl_xor(bcb, m);
            bca = oa > bca ? oa : bca;
            bcb = ob > bcb ? ob : bcb;
        }
    } else if (TYPE == NV_LOCAL) {
#pragma unroll
        for (int m = 1; m < G; m <<= 1) best = pk_max3(best, (uint32_t)__shfl_xor((int)best, m), best);
    }
    auto out = [&](bool valid, uint32_t pair, uint32_t M, uint32_t N, uint32_t half, bool writer) {
        if (!valid || !writer) return;
        int32_t v = (int32_t)((best >> (16 * half)) & 0xFFFFu) - B;
        uint32_t x = N, y = M;                    // SINK: the cell, one-based; GLOBAL: (N, M)
        if constexpr (SINK) {
            if (TYPE == NV_SEMI) x = (half ? colb : cola) + 1;
            const long long bc = half ? bcb : bca;
            if (TYPE == NV_LOCAL && bc >= 0) {
                v = (int32_t)(bc >> 32) - B;
                const uint32_t key = (uint32_t)bc;
                x = ((key >> (SB + 10)) << SB) + (key & ((1u << SB) - 1u)) + 1;
                y = ((key >> SB) & 1023u) + 1;
            }
        }
        if (FR) v -= dl + g * (int32_t)(M + N - 2);   // the frame at (M-1, N-1); SEMI keys: + g*(N-1-c)
        if (M == 0) {
            v = TYPE == NV_SEMI ? (N ? 0 : INT32_MIN)
              : TYPE == NV_GLOBAL ? (N ? (GOTOH ? A.go + A.ge * (int32_t)(N - 1) : A.del * (int32_t)N) : INT32_MIN)
                                  : INT32_MIN;
        } else if (N == 0) v = INT32_MIN;
        if (A.score) A.score[pair] = v;
        if (A.score16) A.score16[pair] = (int16_t)v;
        if constexpr (SINK) {
            if (M == 0) x = N;                    // the band initialisation, reported at y = 0
            if (N == 0 || (TYPE == NV_LOCAL && M == 0)) x = y = 0xFFFFFFFFu;   // no cell was reported
            if (sinks) { sinks[2 * (size_t)pair] = x; sinks[2 * (size_t)pair + 1] = y; }
        }
    };
    const bool wa = TYPE == NV_LOCAL ? lg == 0 : BOT ? lg == G - 1 : (Ma ? (Ma - 1) / R == lg : lg == 0);
    const bool wb = TYPE == NV_LOCAL ? lg == 0 : BOT ? lg == G - 1 : (Mb ? (Mb - 1) / R == lg : lg == 0);
    out(va, pa, Ma, Na, 0, wa);
    out(vb, pb, Mb, Nb, 1, wb);
