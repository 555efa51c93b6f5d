// wsmc_ssm_body.h — the step body of the fused scalar-SSM kernels: one statement over a thread's
// particles (ss_statement) and the Resample on the block's log-weights (ss_resample), with the
// block's LDS state they work on. Included by csrc/wsmc_ssm.hip (k_ssm_segment: one filter, one
// workgroup) and csrc/wsmc_ssm_batch.hip (k_ssm_batch_segment: B filters, one workgroup each);
// both kernels run the same arithmetic on the same layout, so a filter of a batch gives the bits
// of the single run. Everything sits in an anonymous namespace: each file compiles its own copy.
//
// The including file defines WSMC_TABLES_LDS for its device pass before wsmc_internal.h.
#ifndef WSMC_SSM_BODY_H
#define WSMC_SSM_BODY_H

#include "wsmc_internal.h"

#include <algorithm>
#include <cstddef>

namespace wsmc {

namespace {

constexpr int kSsMaxThreads = 1024;
constexpr int kSsWaves = kSsMaxThreads / 64;
constexpr int kSsScratch = 2 * kSsWaves * 4 + 8;   // u64 words: two reduction halves, the broadcast

__device__ inline uint64_t ss_shfl_xor(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t ss_shfl_up(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

__host__ __device__ inline size_t ss_n8(int n) { return ((size_t)n + 1) & ~(size_t)1; }   // doubles, 16-B multiples
__host__ __device__ inline size_t ss_n4(int n) { return ((size_t)n + 3) & ~(size_t)3; }

// the block's state in LDS and the kernel's uniform values
struct SsState {
    double* cb;          // [(S + 1) * stride] the column buffers
    double* lw;          // [n] log-weights
    int32_t* anc;        // [n] the last resampling step's ancestors
    uint64_t* red;       // [kSsScratch]
    int stride;          // doubles between two column buffers
    int S, off;          // column k is buffer (k + off) mod (S + 1); the spare is (S + off) mod (S + 1)
    int N, i0, i1;       // this thread's particles [i0, i1)
    int lane, wave, nw;
};
__device__ inline int ss_buf(const SsState& L, int col) {
    const int b = col + L.off;
    return b > L.S ? b - (L.S + 1) : b;
}

// the step's data row, in registers (loaded a step ahead). The table is written before the run's
// first launch and by nothing while a kernel runs, so it is read as constant memory: uniform
// addresses, scalar loads
typedef const double __attribute__((address_space(4))) * SsConstPtr;
struct SsData {
    double d0, d1, d2, d3;   // named, not an array: nothing is indexed at run time
};
static_assert(WSMC_SSM_MAX_DATA == 4, "SsData holds WSMC_SSM_MAX_DATA values");
// (values, not lvalues, are selected: a conditional over the members themselves selects an address
// and would put the row in memory)
__device__ inline double ss_data(const SsData d, int j) { return j == 0 ? +d.d0 : j == 1 ? +d.d1 : j == 2 ? +d.d2 : +d.d3; }
// row t of the table (dd columns; the others stay 0)
__device__ inline SsData ss_row(SsConstPtr data, int dd, int t) {
    SsData r = {0.0, 0.0, 0.0, 0.0};
    const SsConstPtr p = data + (size_t)t * dd;
    if (dd > 0) r.d0 = p[0];
    if (dd > 1) r.d1 = p[1];
    if (dd > 2) r.d2 = p[2];
    if (dd > 3) r.d3 = p[3];
    return r;
}

// a program's stack (WSMC_XSTACK_MAX values) as a shift register: the top and the seven below it
// in named registers, a push or a pop moving them by one, so nothing is indexed at run time
// (an indexed array of this size leaves the registers at this kernel's register budget)
struct SsStack {
    double top, s1, s2, s3, s4, s5, s6, s7;
    __device__ inline void push(double v) {
        s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = top;
        top = v;
    }
    __device__ inline double pop() {
        const double v = top;
        top = s1; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
        return v;
    }
};
static_assert(WSMC_XSTACK_MAX == 8, "SsStack holds WSMC_XSTACK_MAX values");

// an operand resolved once per statement on the scalar side: the data reference folded into the
// constant, the columns to offsets of their buffers; the value is wsmc_operand_eval's
struct SsOp {
    double c0, k0, k1;
    int o0, o1;          // offset of the column's buffer in cb, -1: no column
};
__device__ inline SsOp ss_resolve(const wsmc_operand& o, const SsState& L, const SsData& d) {
    SsOp r;
    r.c0 = o.c0;
    if (o.col[0] == WSMC_OPERAND_DATA) r.c0 = ss_data(d, o.comp[0]);
    if (o.col[1] == WSMC_OPERAND_DATA) r.c0 = ss_data(d, o.comp[1]);
    r.k0 = o.coef[0];
    r.k1 = o.coef[1];
    r.o0 = o.col[0] >= 0 ? ss_buf(L, o.col[0]) * L.stride : -1;
    r.o1 = o.col[1] >= 0 ? ss_buf(L, o.col[1]) * L.stride : -1;
    return r;
}
__device__ inline double ss_eval(const SsOp& r, const double* cb, int i) {
    double v = r.c0;
    if (r.o0 >= 0) v = v + r.k0 * cb[r.o0 + i];
    if (r.o1 >= 0) v = v + r.k1 * cb[r.o1 + i];
    return v;
}
// the statement's dist (Src: SsmStmt), or an importance Sample's target (SsmTarget), with its two
// parameters evaluated for one particle
template <class Src>
__device__ inline void ss_dist(wsmc_dist* d, const Src& st, double m, double s) {
    d->family = st.family;
    d->mean_fn = WSMC_MEAN_AFFINE;
    d->dim = 1;
    d->reserved = 0;
    d->mu[0].c0 = m;
    d->mu[0].col[0] = d->mu[0].col[1] = -1;
    d->scale.c0 = s;
    d->scale.col[0] = d->scale.col[1] = -1;
    d->param[0] = st.param[0];
    d->param[1] = st.param[1];
}

// one statement over this thread's particles. op: the statement's op counter (a SAMPLE's draws).
// GUIDED (the guided kernels alone): the spec may hold an importance SAMPLE, whose target is tg,
// and a WEIGHT, which is OBSERVE's arithmetic
template <unsigned FEAT, bool GUIDED = false>
__device__ inline void ss_statement(const SsmStmt& st, const SsmIns* ins, SsState& L, const SsData& dv, uint64_t seed,
                                    uint64_t op, const SsmTarget* tg = nullptr) {
    double* cb = L.cb;
    const int kind = st.kind;
    if constexpr (GUIDED) {
        if (kind == WSMC_SSM_SAMPLE_IMPORTANCE) {   // k_sample_importance, a particle at a time
            const SsOp pm = ss_resolve(st.mu, L, dv), ps = ss_resolve(st.scale, L, dv);
            const SsOp tm = ss_resolve(tg->mu, L, dv), ts = ss_resolve(tg->scale, L, dv);
            double* out = cb + ss_buf(L, st.col) * L.stride;
            for (int i = L.i0; i < L.i1; ++i) {
                wsmc_dist d;
                ss_dist(&d, st, ss_eval(pm, cb, i), ss_eval(ps, cb, i));
                double x[4];
                wsmc_dist_sample_mf(&d, x, seed, op, (uint64_t)i, nullptr, L.N, i, nullptr, FEAT);
                out[i] = x[0];
                // both dists' operands again: one that reads the output column sees the new value
                wsmc_dist t;
                ss_dist(&t, *tg, ss_eval(tm, cb, i), ss_eval(ts, cb, i));
                const double lt = wsmc_dist_logpdf_mf(&t, x, nullptr, L.N, i, nullptr, nullptr, FEAT);
                ss_dist(&d, st, ss_eval(pm, cb, i), ss_eval(ps, cb, i));
                const double lp = wsmc_dist_logpdf_mf(&d, x, nullptr, L.N, i, nullptr, nullptr, FEAT);
                L.lw[i] = L.lw[i] + (lt - lp);
            }
            return;
        }
    }
    if (kind == WSMC_SSM_SAMPLE) {
        const SsOp mu = ss_resolve(st.mu, L, dv), sc = ss_resolve(st.scale, L, dv);
        double* out = cb + ss_buf(L, st.col) * L.stride;
        for (int i = L.i0; i < L.i1; ++i) {
            wsmc_dist d;
            ss_dist(&d, st, ss_eval(mu, cb, i), ss_eval(sc, cb, i));
            double x[4];
            wsmc_dist_sample_mf(&d, x, seed, op, (uint64_t)i, nullptr, L.N, i, nullptr, FEAT);
            out[i] = x[0];
        }
    } else if (kind == WSMC_SSM_ASSIGN) {
        const SsOp e = ss_resolve(st.value, L, dv);
        double* out = cb + ss_buf(L, st.col) * L.stride;
        for (int i = L.i0; i < L.i1; ++i) out[i] = ss_eval(e, cb, i);
    } else if (kind == WSMC_SSM_ASSIGN_EXPR) {
        double* out = cb + ss_buf(L, st.col) * L.stride;
        const int p0 = st.prog, p1 = st.prog + st.prog_len;
        for (int i = L.i0; i < L.i1; ++i) {
            SsStack k = {};
            for (int pc = p0; pc < p1; ++pc) {
                const SsmIns& I = ins[pc];
                const int xo = I.op;
                if (xo == WSMC_X_CONST) {
                    k.push(I.c);
                } else if (xo == WSMC_X_COL) {
                    const int c = I.col;
                    k.push(c < 0 ? ss_data(dv, -1 - c) : cb[ss_buf(L, c) * L.stride + i]);
                } else if (xo == WSMC_X_IFELSE) {
                    const double f = k.pop(), t = k.pop();
                    k.top = k.top != 0.0 ? t : f;
                } else if (xo < WSMC_X_ADD) {
                    k.top = wsmc_xop1(xo, k.top, I.c);
                } else {
                    const double b = k.pop();
                    k.top = wsmc_xop2(xo, k.top, b);
                }
            }
            out[i] = k.top;
        }
    } else {   // OBSERVE (a guided kernel: or WEIGHT)
        const SsOp mu = ss_resolve(st.mu, L, dv), sc = ss_resolve(st.scale, L, dv), xv = ss_resolve(st.value, L, dv);
        wsmc_logmemo lm = {0, 0.0, 0.0, 0};   // the thread's particles often share one scale value
        for (int i = L.i0; i < L.i1; ++i) {
            wsmc_dist d;
            ss_dist(&d, st, ss_eval(mu, cb, i), ss_eval(sc, cb, i));
            double x[4];
            x[0] = ss_eval(xv, cb, i);
            L.lw[i] = L.lw[i] + wsmc_dist_logpdf_mf(&d, x, nullptr, L.N, i, nullptr, &lm, FEAT);
        }
    }
}

// what a Resample that ran leaves for the block
struct SsDecision {
    double ess;
    double logev;        // a traced run: wsmc_log_evidence of the weights the Resample met
    int resampled;
};

// Resample on the block's log-weights (wsmc_lgssm.hip's, its arithmetic unchanged): the ESS and
// the strict decision; a resampling step gathers every column and resets the weights to the
// log-mean. Every thread calls it (it holds barriers). op: the Resample's op counter. TR: a traced
// run, whose first wave also finishes the evidence from the sums it holds. COND (the conditional
// kernels alone): the ancestors are N independent draws with slot N - 1 forced to N - 1
// (wsmc_ssm_run_conditional), `scheme` is not read.
template <bool TR, bool COND = false>
__device__ inline SsDecision ss_resample(SsState& L, int K, double ess_min, int scheme, uint64_t seed, uint64_t op) {
    const int N = L.N, i0 = L.i0, i1 = L.i1, lane = L.lane, wave = L.wave, nw = L.nw;
    uint64_t* red0 = L.red;
    uint64_t* red1 = L.red + kSsWaves * 4;
    uint64_t* bc = L.red + 2 * kSsWaves * 4;   // wave 0's results: ESS bits, decision, sum q, log-mean bits
    uint64_t* cdf = reinterpret_cast<uint64_t*>(L.cb + ss_buf(L, L.S) * L.stride);   // the spare buffer

    uint64_t menc = WSMC_ORD_NEG_INF;
    for (int i = i0; i < i1; ++i) {
        const uint64_t e = wsmc_ord_enc(L.lw[i]);
        menc = e > menc ? e : menc;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = ss_shfl_xor(menc, m);
        menc = o > menc ? o : menc;
    }
    if (lane == 0) red0[wave] = menc;
    __syncthreads();
    for (int w = 0; w < nw; ++w) menc = red0[w] > menc ? red0[w] : menc;
    const double M = wsmc_ord_dec(menc);   // NaN if any NaN (the canonical NaN is the largest code)
    const double R = wsmc_qref(M);

    // the exact sums: q and q2 in u64; wf, wf2 < 2^42 each, N < 2^13: u64 too
    uint64_t sQ = 0, sQ2 = 0, sWf = 0, sWf2 = 0;
    for (int i = i0; i < i1; ++i) {
        const wsmc_qparts p = wsmc_qparts_of(L.lw[i], R, K);
        cdf[i] = p.q;
        sQ += p.q; sQ2 += p.q2; sWf += p.wf; sWf2 += p.wf2;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        sQ += ss_shfl_xor(sQ, m);
        sQ2 += ss_shfl_xor(sQ2, m);
        sWf += ss_shfl_xor(sWf, m);
        sWf2 += ss_shfl_xor(sWf2, m);
    }
    if (lane == 0) {
        red1[wave * 4 + 0] = sQ; red1[wave * 4 + 1] = sQ2; red1[wave * 4 + 2] = sWf; red1[wave * 4 + 3] = sWf2;
    }
    __syncthreads();
    // the decision, once for the block: the ESS on the first wave while the last one takes the
    // log-mean a resampling step resets to
    if (wave == 0 || wave == nw - 1) {
        wsmc_shard_stats st;
        st.M = M; st.Q = 0; st.Q2 = 0; st.Wf = 0; st.Wf2 = 0; st.n = (uint64_t)N;
        for (int w = 0; w < nw; ++w) {
            st.Q += red1[w * 4 + 0]; st.Q2 += red1[w * 4 + 1];
            st.Wf += red1[w * 4 + 2]; st.Wf2 += red1[w * 4 + 3];
        }
        if (wave == 0) {
            const double ess = wsmc_global_ess(&st, 1);
            const bool go = ess < ess_min && st.Q > 0;   // strict; all -inf weights (Q = 0, ESS NaN) never resample
            if (lane == 0) {
                bc[0] = wsmc_d2bits(ess);
                bc[1] = go ? 1u : 0u;
                bc[2] = st.Q;
            }
            if (TR) {
                const double le = wsmc_global_log_evidence(&st, 1);
                if (lane == 0) bc[4] = wsmc_d2bits(le);
            }
        }
        if (wave == nw - 1 && st.Q > 0) {   // (one wave: it does both in turn)
            const double mean = wsmc_shard_mean(&st);
            if (lane == 0) bc[3] = wsmc_d2bits(mean);
        }
    }
    __syncthreads();
    SsDecision dec;
    dec.ess = wsmc_bits2d(bc[0]);
    dec.logev = TR ? wsmc_bits2d(bc[4]) : 0.0;
    dec.resampled = bc[1] != 0 ? 1 : 0;
    if (!dec.resampled) return dec;   // uniform over the block
    const uint64_t Q = bc[2];
    const double mean = wsmc_bits2d(bc[3]);

    // inclusive scan of q (in place): thread-local, then across the wave, then across waves
    uint64_t run = 0;
    for (int i = i0; i < i1; ++i) { run += cdf[i]; cdf[i] = run; }
    uint64_t incl = run;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = ss_shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) red0[wave] = incl;   // (red0's readers passed the barriers above)
    __syncthreads();
    uint64_t excl = incl - run;
    for (int w = 0; w < wave; ++w) excl += red0[w];
    if constexpr (COND) {
        // the full C_i in place of the thread-local sums; then slot j is wsmc_sample_particles(N,
        // replace)'s draw j: the smallest m with C_m > its target (C_{N-1} = Q is above every target)
        for (int i = i0; i < i1; ++i) cdf[i] += excl;
        __syncthreads();
        for (int i = i0; i < i1; ++i) {
            int lo = N - 1;
            if (i < N - 1) {
                const uint64_t x = wsmc_multi_target(wsmc_multi_word(seed, op, (uint64_t)i), Q);
                lo = 0;
                for (int hi = N - 1; lo < hi;) {
                    const int mid = (lo + hi) >> 1;
                    if (cdf[mid] > x) hi = mid; else lo = mid + 1;
                }
            }
            L.anc[i] = lo;
        }
        // the weight reset and column 0's gather into the spare, which holds the CDF: behind the
        // last search of any thread
        __syncthreads();
        const double* src = L.cb + ss_buf(L, 0) * L.stride;
        double* dst = reinterpret_cast<double*>(cdf);
        for (int i = i0; i < i1; ++i) {
            dst[i] = src[L.anc[i]];
            L.lw[i] = mean;
        }
    } else {
        // rank of each particle's CDF end: its slots are [rank(C_{m-1}), rank(C_m)); the rank goes
        // into the low word of the particle's own CDF entry (no other thread reads that entry)
        const double ratio = wsmc_u64_to_d((uint64_t)N) / wsmc_u64_to_d(Q);
        for (int i = i0; i < i1; ++i) {
            const uint64_t C = cdf[i] + excl;
            const uint64_t rk = wsmc_rank_r(C, Q, (uint64_t)N, ratio, scheme, seed, op, 0);
            reinterpret_cast<int32_t*>(cdf + i)[0] = (int32_t)rk;
            L.anc[i] = 0;
        }
        __syncthreads();
        // marks: particle m writes m at its first slot (the slot ranges partition [0, N))
        for (int i = i0; i < i1; ++i) {
            const int lo = i ? reinterpret_cast<const int32_t*>(cdf + (i - 1))[0] : 0;
            const int hi = reinterpret_cast<const int32_t*>(cdf + i)[0];
            if (lo < hi && lo < N) L.anc[lo] = i;
        }
        __syncthreads();
        // inclusive max-scan of the marks: the ancestors
        int rmax = 0;
        for (int i = i0; i < i1; ++i) { const int v = L.anc[i]; rmax = v > rmax ? v : rmax; }
        int imax = rmax;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(imax, d, 64);
            if (lane >= d) imax = o > imax ? o : imax;
        }
        if (lane == 63) red1[wave] = (uint64_t)(uint32_t)imax;   // (red1's readers: two barriers back)
        int before = __shfl_up(imax, 1, 64);
        if (lane == 0) before = 0;
        __syncthreads();
        for (int w = 0; w < wave; ++w) {
            const int o = (int)(uint32_t)red1[w];
            before = o > before ? o : before;
        }
        // the ancestors, the weight reset and column 0's gather into the spare (the ranks in it were
        // last read before the marks' barrier), each new particle written by its owner
        {
            const double* src = L.cb + ss_buf(L, 0) * L.stride;
            double* dst = reinterpret_cast<double*>(cdf);
            for (int i = i0; i < i1; ++i) {
                const int v = L.anc[i];
                before = v > before ? v : before;
                L.anc[i] = before;
                dst[i] = src[before];
                L.lw[i] = mean;
            }
        }
    }
    // column k > 0 into the buffer column k - 1 has just left: a barrier first, other threads
    // were still reading it
    for (int k = 1; k < L.S; ++k) {
        __syncthreads();
        const double* src = L.cb + ss_buf(L, k) * L.stride;
        double* dst = L.cb + ss_buf(L, k - 1) * L.stride;
        for (int i = i0; i < i1; ++i) dst[i] = src[L.anc[i]];
    }
    // every column one buffer down; column S - 1's old buffer is the spare, next written as a
    // CDF behind the next Resample's first barrier
    L.off = L.off == 0 ? L.S : L.off - 1;
    return dec;
}

// ---- the traced run's row (wsmc_ssm_run_traced): wsmc_weighted_moments of the columns -----------
// The sums are the canonical ones (oracle/wsmc_oracle.c canon_block, csrc/wsmc_kernels.hip
// k_moments / k_moments_final): tiles of 2048 items, canonical thread th of 256 adding items
// base + j * 256 + th, j = 0..7, from 0.0 (0.0 past N); an xor butterfly 1, 2, .., 32 over each 64
// lanes; (w0 + w1) + (w2 + w3); the tile partials through the same block shape. A thread here
// owns consecutive particles and the block has 64..1024 threads, so the unit of work is a
// canonical wave (64 lanes x 8 strided items, 4 to a tile) of one of the values, dealt over the
// block's waves.
constexpr int kSsCanonWaves = 4 * ((kLgCap + 2047) / 2048);   // 12: three tiles at the largest cap
constexpr int kSsTrVals = 1 + WSMC_SSM_MAX_COLS;              // pass 1: e and e z_k
static_assert(kSsCanonWaves * (kSsTrVals + WSMC_SSM_MAX_COLS) <= 2 * kSsWaves * 4,
              "both passes' wave totals fit the reduction scratch");

// a thread's canonical items of canonical wave cw: its tile's base + (cw & 3) * 64 + lane + j * 256
__device__ inline int ss_canon_item(int cw, int lane, int j) { return (cw >> 2) * 2048 + j * 256 + (cw & 3) * 64 + lane; }
__device__ inline double ss_canon_wave(double v) {
    for (int m = 1; m < 64; m <<= 1) v = v + wsmc_bits2d(ss_shfl_xor(wsmc_d2bits(v), m));
    return v;
}
// the total from the canonical waves' totals wv[cw * stride]: each tile's (w0 + w1) + (w2 + w3),
// then the combine block, whose thread th starts from 0.0 and adds partial th. With at most three
// partials its butterfly leaves (a0 + a1) + (a2 + a3) in lane 0 after the offsets 1 and 2; the
// other four offsets and the three idle waves add the zeros they hold
__device__ inline double ss_canon_total(const double* wv, int stride, int ntiles) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    a0 = a0 + ((wv[0] + wv[stride]) + (wv[2 * stride] + wv[3 * stride]));
    if (ntiles > 1) a1 = a1 + ((wv[4 * stride] + wv[5 * stride]) + (wv[6 * stride] + wv[7 * stride]));
    if (ntiles > 2) a2 = a2 + ((wv[8 * stride] + wv[9 * stride]) + (wv[10 * stride] + wv[11 * stride]));
    double r = (a0 + a1) + (a2 + 0.0);
    for (int m = 4; m < 64; m <<= 1) r = r + 0.0;
    return (r + 0.0) + (0.0 + 0.0);
}

// Row t of the moments, at the trace point (before the Resample that follows the step's last
// OBSERVE): mean[k] and var[k] as wsmc_weighted_moments gives them for expression k = column k
// alone (z = 0.0 + 1.0 * x) under exp_norm of the weights. Every thread calls it (it holds
// barriers); thread 0 stores. mean / var: the row's [S] values in global memory, null: not wanted.
__device__ inline void ss_trace_row(SsState& L, double* mean_out, double* var_out) {
    const int N = L.N, S = L.S, lane = L.lane, wave = L.wave, nw = L.nw;
    double* ebuf = L.cb + ss_buf(L, S) * L.stride;   // the spare buffer: free until ss_resample's first barrier
    double* wv1 = reinterpret_cast<double*>(L.red);  // the scratch is idle before the Resample
    double* wv2 = wv1 + kSsCanonWaves * kSsTrVals;
    const int ntiles = (N + 2047) / 2048, ncw = 4 * ntiles;

    // the block max, ss_resample's
    uint64_t menc = WSMC_ORD_NEG_INF;
    for (int i = L.i0; i < L.i1; ++i) {
        const uint64_t e = wsmc_ord_enc(L.lw[i]);
        menc = e > menc ? e : menc;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = ss_shfl_xor(menc, m);
        menc = o > menc ? o : menc;
    }
    if (lane == 0) L.red[wave] = menc;
    __syncthreads();   // (also: the last Resample's gathers out of the spare's buffer are through)
    for (int w = 0; w < nw; ++w) menc = L.red[w] > menc ? L.red[w] : menc;
    const double M = wsmc_ord_dec(menc);   // NaN if any NaN
    for (int i = L.i0; i < L.i1; ++i) ebuf[i] = wsmc_exp(L.lw[i] - M);
    __syncthreads();

    // pass 1: S0 = sum e and the sums of e z_k. A unit of work is one canonical wave of one value
    // (k = -1: e itself), the units dealt over the block's waves
    for (int u = wave; u < (1 + S) * ncw; u += nw) {
        const int k = u / ncw - 1, cw = u - (k + 1) * ncw;
        const double* x = L.cb + ss_buf(L, k < 0 ? 0 : k) * L.stride;
        double s = 0.0;
        for (int j = 0; j < 8; ++j) {
            const int i = ss_canon_item(cw, lane, j);
            double v = 0.0;
            if (i < N) v = k < 0 ? ebuf[i] : ebuf[i] * (0.0 + 1.0 * x[i]);
            s = s + v;
        }
        s = ss_canon_wave(s);
        if (lane == 0) wv1[cw * kSsTrVals + 1 + k] = s;
    }
    __syncthreads();
    // S0 and the means from the waves' totals, where they are used: thread 0 (the row's means) and
    // the waves that have a unit of pass 2
    const bool mine = var_out && wave < S * ncw;
    double S0 = 0.0;
    if (mine || (wave == 0 && lane == 0)) S0 = ss_canon_total(wv1, kSsTrVals, ntiles);
    if (mean_out && wave == 0 && lane == 0)
        for (int k = 0; k < S; ++k) mean_out[k] = ss_canon_total(wv1 + 1 + k, kSsTrVals, ntiles) / S0;

    // pass 2 (a trace with the variances): the sums of (e (z_k - mean_k)) (z_k - mean_k), the same
    // units; a wave takes the mean of its unit's column from the waves' totals again
    if (mine)
        for (int u = wave; u < S * ncw; u += nw) {
            const int k = u / ncw, cw = u - k * ncw;
            const double* x = L.cb + ss_buf(L, k) * L.stride;
            const double m = ss_canon_total(wv1 + 1 + k, kSsTrVals, ntiles) / S0;
            double s = 0.0;
            for (int j = 0; j < 8; ++j) {
                const int i = ss_canon_item(cw, lane, j);
                double v = 0.0;
                if (i < N) {
                    const double z = 0.0 + 1.0 * x[i];
                    v = (ebuf[i] * (z - m)) * (z - m);
                }
                s = s + v;
            }
            s = ss_canon_wave(s);
            if (lane == 0) wv2[cw * WSMC_SSM_MAX_COLS + k] = s;
        }
    // with or without pass 2: every read of pass 1's totals (words 0..59 of the scratch) is through
    // before ss_resample, which the other waves enter next, writes its block max into words 0..15.
    // Thread 0 then reads pass 2's words 60..107 only, which ss_resample writes behind its first
    // barrier
    __syncthreads();
    if (var_out && wave == 0 && lane == 0)
        for (int k = 0; k < S; ++k) var_out[k] = ss_canon_total(wv2 + k, WSMC_SSM_MAX_COLS, ntiles) / S0;
}

// ---- a smoothed run's recording (wsmc_ssm_run_smoothed; the recording units alone call these) ----
// The trace point's columns to row t of the history, every thread its own particles: plain stores,
// nothing waits on them. hist: the row's [S][N] doubles in global memory
__device__ inline void ss_record_cols(const SsState& L, double* hist) {
    for (int k = 0; k < L.S; ++k) {
        const double* src = L.cb + ss_buf(L, k) * L.stride;
        double* dst = hist + (size_t)k * L.N;
        for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
    }
}
// (wsmc_ssm_run_backward's recording units) the trace point's log-weights to row t of their log,
// beside the columns: lwlog: the row's [N] doubles in global memory
__device__ inline void ss_record_lw(const SsState& L, double* lwlog) {
    for (int i = L.i0; i < L.i1; ++i) lwlog[i] = L.lw[i];
}
// After a Resample that ran: its ancestors (each written by its particle's owner in ss_resample)
// to the slot's [N] row of the log, and the slot's flag
__device__ inline void ss_record_anc(const SsState& L, int32_t* slot, int32_t* ran) {
    for (int i = L.i0; i < L.i1; ++i) slot[i] = L.anc[i];
    if (L.lane == 0 && L.wave == 0) *ran = 1;
}

// The instantiations by feature set (k_sample<...>'s): a spec without the log-Gamma families
// never carries wsmc_lgamma and the rejection samplers, one without the extended scalar
// families not their code either. Each variant has its own launch bound; all three fit the 128
// VGPRs of a 1024-thread workgroup without a spill (DESIGN.md §4 has the listing).
constexpr unsigned kSsFeatExt = WSMC_FEAT_EXT, kSsFeatGam = WSMC_FEAT_EXT | WSMC_FEAT_GAM;
constexpr int kSsGamThreads = 1024;
// the guided kernels' (an importance Sample holds a sampler and two log-densities at once): their
// log-Gamma variant does not fit 128 VGPRs without a spill, so it runs at most 512 threads, with
// more particles a thread at the sizes past 1024 (the caps are LDS's and do not move)
constexpr int kSsGuidedGamThreads = 512;

// ---- host side: what the launch wrappers of both files share (no kernel calls these) ----
// a segment's arguments within the kernels' limits, for the fields SsmArgs and SsmBatchArgs share
template <class Args>
inline bool ss_segment_ok(const Args& a, unsigned feat, int threads, bool guided = false) {
    const int tmax = (feat & WSMC_FEAT_GAM) ? (guided ? kSsGuidedGamThreads : kSsGamThreads) : kSsMaxThreads;
    return !(a.S < 1 || a.S > WSMC_SSM_MAX_COLS || a.N < 1 || a.N > ssm_cap(a.S) || threads < 64 || threads > tmax ||
        (threads & 63) || (int64_t)a.P * threads < a.N || a.nsteps < 0 || a.t0 < 0 || a.data_dim < 0 ||
        a.data_dim > WSMC_SSM_MAX_DATA || a.n_init < 0 || a.n_init > WSMC_SSM_MAX_INIT || a.n_step < 1 ||
        a.n_step > WSMC_SSM_MAX_STMTS) &&
           ssm_lds_bytes(a.N, a.S) + 4096 <= 160 * 1024;   // with the static tables: the workgroup's LDS
}
// past 64 KiB a kernel must ask for its dynamic LDS (per device: set at each launch, and before an
// occupancy query, which refuses what the kernel has not asked for)
template <class Kernel>
inline hipError_t ss_ask_lds(Kernel k, size_t lds) {
    if (lds <= 65536 - 4096) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

}  // namespace wsmc

#endif  // WSMC_SSM_BODY_H
