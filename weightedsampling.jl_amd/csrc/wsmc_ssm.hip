// wsmc_ssm.hip — the fused run of a scalar state-space model the caller specifies (wsmc_ssm_run):
// csrc/wsmc_lgssm.hip's persistent workgroup with the step body read from a description instead
// of hard-coded. One workgroup runs the steps of a segment in a loop on the device,
// the S state columns and the log-weights in LDS for the whole segment.
//
// The statements (SsmArgs: init, step, the programs' instructions) are read in place through the
// kernarg segment pointer: every lane runs the same statement, so the loads are scalar and the
// branches uniform. Per particle a statement calls the functions the statement kernels call
// (include/wsmc_terms.h): wsmc_dist_sample_mf / wsmc_dist_logpdf_mf on a dist whose two operands
// have been evaluated to constants by wsmc_operand_eval's arithmetic (a constant operand
// evaluates to its c0, so the dist sees the same parameter bits), wsmc_xop1 / wsmc_xop2 for a
// program. The draws are keyed by (seed, op, particle) as the statement path's.
//
// The Resample is wsmc_lgssm.hip's, restated: the block max, the exact integer sums, the decision
// by one wave, the scan, ranks, marks and max-scan. The gather moves one column at a time into
// the spare buffer (S + 1 buffers for S columns): column k sits in buffer (k + off) mod (S + 1),
// and a resampling step lowers `off` by one, so no pointer is ever indexed at run time.
//
// Layout: thread t owns the P = ceil(N / threads) consecutive particles from t * P; a statement
// reads and writes its own particles only, so statements need no barrier between them. The only
// synchronisation is __syncthreads; no workgroup waits on another.
#ifdef __HIP_DEVICE_COMPILE__
#define WSMC_TABLES_LDS   // include/wsmc_math.h: the device pass reads LDS copies of the tables
#endif
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
// the statement's dist with its two parameters evaluated for one particle
__device__ inline void ss_dist(wsmc_dist* d, const SsmStmt& st, double m, double s) {
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

// one statement over this thread's particles. op: the statement's op counter (a SAMPLE's draws)
template <unsigned FEAT>
__device__ inline void ss_statement(const SsmStmt& st, const SsmIns* ins, SsState& L, const SsData& dv, uint64_t seed,
                                    uint64_t op) {
    double* cb = L.cb;
    const int kind = st.kind;
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
    } else {   // OBSERVE
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
    int resampled;
};

// Resample on the block's log-weights (wsmc_lgssm.hip's, its arithmetic unchanged): the ESS and
// the strict decision; a resampling step gathers every column and resets the weights to the
// log-mean. Every thread calls it (it holds barriers). op: the Resample's op counter.
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
        }
        if (wave == nw - 1 && st.Q > 0) {   // (one wave: it does both in turn)
            const double mean = wsmc_shard_mean(&st);
            if (lane == 0) bc[3] = wsmc_d2bits(mean);
        }
    }
    __syncthreads();
    SsDecision dec;
    dec.ess = wsmc_bits2d(bc[0]);
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

}  // namespace

// the kernel's dynamic LDS for n particles in S columns (beside the 4 KiB of static log / exp tables)
size_t ssm_lds_bytes(int n, int S) {
    return ((size_t)S + 2) * ss_n8(n) * sizeof(double) + ss_n4(n) * sizeof(int32_t) + kSsScratch * sizeof(uint64_t);
}

template <unsigned FEAT, int THREADS>
__global__ __launch_bounds__(THREADS) void k_ssm_segment(SsmArgs) {
    const SsmArgs& a = *(const SsmArgs*)(const char*)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) char ss_smem[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int N = a.N, P = a.P, S = a.S;
    SsState L;
    L.stride = (int)ss_n8(N);
    L.cb = reinterpret_cast<double*>(ss_smem);
    L.lw = L.cb + (size_t)(S + 1) * L.stride;
    L.anc = reinterpret_cast<int32_t*>(L.lw + L.stride);
    L.red = reinterpret_cast<uint64_t*>(L.anc + ss_n4(N));
    L.S = S;
    L.off = 0;
    L.N = N;
    L.i0 = tid * P < N ? tid * P : N;
    L.i1 = L.i0 + P < N ? L.i0 + P : N;
    L.lane = tid & 63;
    L.wave = tid >> 6;
    L.nw = (nthr + 63) >> 6;

#ifdef WSMC_TABLES_LDS
    wsmc_tables_to_lds();   // before any log / exp (every thread: it ends in a barrier)
#endif
    for (int i = L.i0; i < L.i1; ++i) L.lw[i] = a.w[i];
    for (int k = 0; k < S; ++k) {
        const double* src = k == 0 ? a.x[0] : k == 1 ? a.x[1] : k == 2 ? a.x[2] : a.x[3];
        double* dst = L.cb + (size_t)k * L.stride;
        for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
    }

    const int K = wsmc_qbits((uint64_t)N);
    const int dd = a.data_dim;
    const SsConstPtr data = (SsConstPtr)a.data;
    long long nres = 0;
    int last_dec = 0, ran = 0;
    double last_ess = 0.0;
    SsData dv = {0.0, 0.0, 0.0, 0.0};

    SsData dnext = dv;
    if (a.nsteps > 0) dnext = ss_row(data, dd, a.t0);

    // s = -1: `init` (the run's first segment; it reads no data, and the weights are unchanged on
    // entry), then the segment's steps: one statement loop, so the body is in the code once
    static_assert(offsetof(SsmArgs, step) == offsetof(SsmArgs, init) + WSMC_SSM_MAX_INIT * sizeof(SsmStmt),
                  "step follows init: one statement array");
    for (int s = a.first ? -1 : 0; s < a.nsteps; ++s) {
        const int t = a.t0 + s;
        const bool init = s < 0;
        const SsmStmt* list = a.init + (init ? 0 : WSMC_SSM_MAX_INIT);
        const int nst = init ? a.n_init : a.n_step;
        uint64_t op = init ? a.op_base : a.op_base + (uint64_t)a.init_ops + (uint64_t)a.step_ops * (uint64_t)t;
        if (!init) {
            dv = dnext;
            if (s + 1 < a.nsteps) dnext = ss_row(data, dd, t + 1);   // in flight during this step
        }
        for (int q = 0; q < nst; ++q) {
            const SsmStmt& st = list[q];
            ss_statement<FEAT>(st, a.ins, L, dv, a.seed, op);
            if (st.kind == WSMC_SSM_SAMPLE) {
                op += 2;   // the draws, then a Resample that does not run (the weights have not changed)
            } else if (st.kind == WSMC_SSM_OBSERVE) {
                const SsDecision d = ss_resample(L, K, a.ess_min, a.scheme, a.seed, op);
                op += 1;
                nres += d.resampled;
                last_dec = d.resampled;
                last_ess = d.ess;
                ran = 1;
                if (!init && q == a.last_obs && a.ess_trace && tid == 0) a.ess_trace[t] = d.ess;
            }
        }
    }

    for (int k = 0; k < S; ++k) {
        double* dst = k == 0 ? a.x[0] : k == 1 ? a.x[1] : k == 2 ? a.x[2] : a.x[3];
        const double* src = L.cb + (size_t)ss_buf(L, k) * L.stride;
        for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
    }
    for (int i = L.i0; i < L.i1; ++i) a.w[i] = L.lw[i];
    if (nres > 0)
        for (int i = L.i0; i < L.i1; ++i) a.anc[i] = L.anc[i];
    if (tid == 0 && ran) {
        a.rec->nres += nres;
        a.rec->last_dec = last_dec;
        a.rec->last_ess = last_ess;
    }
}

// The instantiations by feature set (k_sample<...>'s): a spec without the log-Gamma families
// never carries wsmc_lgamma and the rejection samplers, one without the extended scalar
// families not their code either. Each variant has its own launch bound; all three fit the 128
// VGPRs of a 1024-thread workgroup without a spill (DESIGN.md §4 has the listing).
constexpr unsigned kSsFeatExt = WSMC_FEAT_EXT, kSsFeatGam = WSMC_FEAT_EXT | WSMC_FEAT_GAM;
constexpr int kSsGamThreads = 1024;

int ssm_threads(unsigned feat, int n) {
    const int cap = (feat & WSMC_FEAT_GAM) ? kSsGamThreads : kSsMaxThreads;
    // two particles a thread where the workgroup allows (wsmc_lgssm1d_run's measured choice)
    return std::max(64, std::min(cap, ((n + 127) / 128) * 64));
}

template <unsigned FEAT, int THREADS>
static hipError_t ssm_launch(hipStream_t s, const SsmArgs& a, int threads, size_t lds) {
    if (lds > 65536 - 4096) {   // past 64 KiB a kernel must ask for its dynamic LDS (per device: set at each launch)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ssm_segment<FEAT, THREADS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_ssm_segment<FEAT, THREADS>), dim3(1), dim3(threads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_ssm_segment(hipStream_t s, const SsmArgs& a, unsigned feat, int threads) {
    const int tmax = (feat & WSMC_FEAT_GAM) ? kSsGamThreads : kSsMaxThreads;
    if (a.S < 1 || a.S > WSMC_SSM_MAX_COLS || a.N < 1 || a.N > ssm_cap(a.S) || threads < 64 || threads > tmax ||
        (threads & 63) || (int64_t)a.P * threads < a.N || a.nsteps < 0 || a.t0 < 0 || a.data_dim < 0 ||
        a.data_dim > WSMC_SSM_MAX_DATA || a.n_init < 0 || a.n_init > WSMC_SSM_MAX_INIT || a.n_step < 1 ||
        a.n_step > WSMC_SSM_MAX_STMTS)
        return hipErrorInvalidValue;
    const size_t lds = ssm_lds_bytes(a.N, a.S);
    if (lds + 4096 > 160 * 1024) return hipErrorInvalidValue;   // with the static tables: the workgroup's LDS
    if (feat & WSMC_FEAT_GAM) return ssm_launch<kSsFeatGam, kSsGamThreads>(s, a, threads, lds);
    if (feat & WSMC_FEAT_EXT) return ssm_launch<kSsFeatExt, kSsMaxThreads>(s, a, threads, lds);
    return ssm_launch<0u, kSsMaxThreads>(s, a, threads, lds);
}

}  // namespace wsmc
