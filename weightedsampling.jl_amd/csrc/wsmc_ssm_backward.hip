// wsmc_ssm_backward.hip — forward filtering, backward simulation over the record of a scalar-SSM
// run (wsmc_ssm_backward, wsmc_ssm_run_backward).
//
// k_ssm_backward: one workgroup a (filter, trajectory), t looped on the device from T - 1 down to 0.
// At t < T - 1 every thread takes its particles' columns and log-weight of trace point t straight
// from the record in device memory and runs step t + 1's statements on them in registers, with the
// successor's row z (the record's row t + 1 at the index drawn last, a uniform address) in place
// of the draws: the included terms add to the log-weight in statement order, ((lw + term_1) +
// term_2) ..., the only order-sensitive arithmetic here. The operand, program and dist evaluation
// is the fused kernel's (csrc/wsmc_ssm_body.h, include/wsmc_terms.h), so a term has the bits
// wsmc_weight gives it. Then wsmc_sample_particles(1, replace)'s draw: the block max over
// wsmc_ord_enc, the integer weights against wsmc_qref of it, their block sum and exclusive scan,
// and the one thread whose range holds wsmc_multi_target(wsmc_multi_word(seed, t M + m, 0), Q)
// walks its particles to the first index whose running sum exceeds it. The reductions are integer,
// so any order gives the same bits. A NaN maximum or Q == 0 (exp_norm of the weights is NaN) sets
// the call's flag, which the host turns into WSMC_ESTATE, and ends the workgroup.
//
// k_ssm_backward_rows: one workgroup a (filter, step) gathers row t of the record through idx into
// LDS in the fused kernel's layout with N := M and zero log-weights, stores it (the paths) and
// calls ss_trace_row on it: the canonical sums of wsmc_weighted_moments on M particles with fresh
// weights. csrc/wsmc_ssm_smooth.hip's k_ssm_smooth_rows, with another source of the indices.
#ifdef __HIP_DEVICE_COMPILE__
#define WSMC_TABLES_LDS   // include/wsmc_math.h: the device pass reads LDS copies of the tables
#endif
#include "wsmc_ssm_body.h"

#include <cstdint>

namespace wsmc {

namespace {

constexpr int kBwThreads = 1024;
constexpr int kBwScratch = 2 * kSsWaves + 2;   // u64 words: the waves' maxima, their sums, the winner

typedef const SsmBwFilter __attribute__((address_space(4))) * BwFilterPtr;

// one particle's columns in registers (named, not an array: nothing is indexed at run time)
struct BwEnv {
    double e0, e1, e2, e3;
};
static_assert(WSMC_SSM_MAX_COLS == 4, "BwEnv holds WSMC_SSM_MAX_COLS values");
__device__ inline double bw_get(const BwEnv& e, int c) { return c == 0 ? +e.e0 : c == 1 ? +e.e1 : c == 2 ? +e.e2 : +e.e3; }
__device__ inline void bw_set(BwEnv& e, int c, double v) {
    e.e0 = c == 0 ? v : e.e0;
    e.e1 = c == 1 ? v : e.e1;
    e.e2 = c == 2 ? v : e.e2;
    e.e3 = c == 3 ? v : e.e3;
}
// columns 0 .. S-1 of a record row at index i (the others stay 0)
__device__ inline BwEnv bw_load(const double* row, int S, int N, int i) {
    BwEnv e = {0.0, 0.0, 0.0, 0.0};
    e.e0 = row[i];
    if (S > 1) e.e1 = row[(size_t)N + i];
    if (S > 2) e.e2 = row[(size_t)2 * N + i];
    if (S > 3) e.e3 = row[(size_t)3 * N + i];
    return e;
}
// wsmc_operand_eval's arithmetic (ss_resolve and ss_eval in one): the data slot folded into the constant
__device__ inline double bw_operand(const wsmc_operand& o, const BwEnv& e, const SsData& d) {
    double v = o.c0;
    if (o.col[0] == WSMC_OPERAND_DATA) v = ss_data(d, o.comp[0]);
    if (o.col[1] == WSMC_OPERAND_DATA) v = ss_data(d, o.comp[1]);
    if (o.col[0] >= 0) v = v + o.coef[0] * bw_get(e, o.col[0]);
    if (o.col[1] >= 0) v = v + o.coef[1] * bw_get(e, o.col[1]);
    return v;
}
// an ASSIGN_EXPR's program (ss_statement's loop, the columns from registers)
__device__ inline double bw_program(const SsmIns* ins, int p0, int p1, const BwEnv& e, const SsData& dv) {
    SsStack k = {};
    for (int pc = p0; pc < p1; ++pc) {
        const SsmIns& I = ins[pc];
        const int xo = I.op;
        if (xo == WSMC_X_CONST) {
            k.push(I.c);
        } else if (xo == WSMC_X_COL) {
            const int c = I.col;
            k.push(c < 0 ? ss_data(dv, -1 - c) : bw_get(e, c));
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
    return k.top;
}

struct SsmBwRowsArgs {
    const double* hist;   // [B][T][S][N]
    const int32_t* idx;   // [B][T][M]
    double* paths;        // [B][T][S][M] or null
    double* mean;         // [B][T][S] or null
    double* var;          // [B][T][S] or null
    int32_t N, M, S, P;   // P: trajectories per thread
};

}  // namespace

template <unsigned FEAT>
__global__ __launch_bounds__(kBwThreads) void k_ssm_backward(SsmBwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char bw_smem[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = (nthr + 63) >> 6;
    const int N = a.N, P = a.P, S = a.S, T = a.T, M = a.M, nst = a.n_step, dd = a.data_dim;
    const size_t b = blockIdx.x / (unsigned)M;
    const int m = (int)(blockIdx.x - b * (unsigned)M);
    double* lwb = reinterpret_cast<double*>(bw_smem);               // [N] the step's log-weights
    uint64_t* red0 = reinterpret_cast<uint64_t*>(lwb + ss_n8(N));   // [kSsWaves] the waves' maxima
    uint64_t* red1 = red0 + kSsWaves;                               // [kSsWaves] the waves' sums
    uint64_t* bc = red1 + kSsWaves;                                 // the index drawn
    if (tid == 0) bc[0] = 0;   // (read behind three barriers)
#ifdef WSMC_TABLES_LDS
    wsmc_tables_to_lds();   // before any log / exp (every thread: it ends in a barrier)
#endif
    // the filter's step: written before the launch and by nothing while the kernel runs; a uniform
    // address, so the loads are scalar (as the batch kernel reads its SsmBatchFilter)
    const SsmBwFilter& F = *(const SsmBwFilter*)(BwFilterPtr)(a.filt + b);
    const SsConstPtr data = (SsConstPtr)F.data;
    const uint64_t seed = F.seed;
    const double* hist = a.hist + b * (size_t)T * S * N;
    const double* lwlog = a.lwlog + b * (size_t)T * N;
    int32_t* idx = a.idx + b * (size_t)T * M;
    const int i0 = tid * P < N ? tid * P : N;
    const int i1 = i0 + P < N ? i0 + P : N;
    const int K = wsmc_qbits((uint64_t)N);
    int sel = 0;

    for (int t = T - 1; t >= 0; --t) {
        const double* row = hist + (size_t)t * S * N;
        const double* lwr = lwlog + (size_t)t * N;
        if (t == T - 1) {
            for (int i = i0; i < i1; ++i) lwb[i] = lwr[i];
        } else {
            const BwEnv z = bw_load(hist + (size_t)(t + 1) * S * N, S, N, sel);   // the successor's row
            const SsData dv = ss_row(data, dd, t + 1);
            wsmc_logmemo lm = {0, 0.0, 0.0, 0};   // the particles often share one scale value
            for (int i = i0; i < i1; ++i) {
                BwEnv e = bw_load(row, S, N, i);
                double lw = lwr[i];
                for (int q = 0; q < nst; ++q) {
                    const SsmStmt& st = F.step[q];
                    const int kind = st.kind;
                    const bool inc = F.included[q] != 0;
                    if (kind == WSMC_SSM_SAMPLE) {   // weight(dist, const z[col]) if included, then assign(col, const z[col])
                        const double zc = bw_get(z, st.col);
                        if (inc) {
                            wsmc_dist d;
                            ss_dist(&d, st, bw_operand(st.mu, e, dv), bw_operand(st.scale, e, dv));
                            double x[4];
                            x[0] = zc;
                            lw = lw + wsmc_dist_logpdf_mf(&d, x, nullptr, N, i, nullptr, &lm, FEAT);
                        }
                        bw_set(e, st.col, zc);
                    } else if (kind == WSMC_SSM_SAMPLE_IMPORTANCE) {   // assign(col, const z[col]), then weight(target, col) if included
                        bw_set(e, st.col, bw_get(z, st.col));
                        if (inc) {
                            const SsmTarget& tg = F.targ[q];
                            wsmc_dist d;
                            ss_dist(&d, tg, bw_operand(tg.mu, e, dv), bw_operand(tg.scale, e, dv));
                            double x[4];
                            x[0] = 0.0 + 1.0 * bw_get(e, st.col);   // the operand that names the column
                            lw = lw + wsmc_dist_logpdf_mf(&d, x, nullptr, N, i, nullptr, &lm, FEAT);
                        }
                    } else if (kind == WSMC_SSM_ASSIGN) {
                        bw_set(e, st.col, bw_operand(st.value, e, dv));
                    } else if (kind == WSMC_SSM_ASSIGN_EXPR) {
                        bw_set(e, st.col, bw_program(F.ins, st.prog, st.prog + st.prog_len, e, dv));
                    } else if (inc) {   // OBSERVE, WEIGHT: weight(dist, value)
                        wsmc_dist d;
                        ss_dist(&d, st, bw_operand(st.mu, e, dv), bw_operand(st.scale, e, dv));
                        double x[4];
                        x[0] = bw_operand(st.value, e, dv);
                        lw = lw + wsmc_dist_logpdf_mf(&d, x, nullptr, N, i, nullptr, &lm, FEAT);
                    }
                }
                lwb[i] = lw;
            }
        }
        // the draw: wsmc_sample_particles(1, replace) at op counter t M + m. The block max
        // (ss_resample's); a thread reads back its own entries of lwb only
        uint64_t menc = WSMC_ORD_NEG_INF;
        for (int i = i0; i < i1; ++i) {
            const uint64_t en = wsmc_ord_enc(lwb[i]);
            menc = en > menc ? en : menc;
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const uint64_t o = ss_shfl_xor(menc, s);
            menc = o > menc ? o : menc;
        }
        if (lane == 0) red0[wave] = menc;
        __syncthreads();
        for (int w = 0; w < nw; ++w) menc = red0[w] > menc ? red0[w] : menc;
        const double R = wsmc_qref(wsmc_ord_dec(menc));   // NaN if any NaN (the canonical NaN is the largest code)
        // the integer weights' sum and exclusive scan: thread-local, across the wave, across waves
        uint64_t run = 0;
        for (int i = i0; i < i1; ++i) run += wsmc_qweight(lwb[i], R, K);
        uint64_t incl = run;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = ss_shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) red1[wave] = incl;
        __syncthreads();
        uint64_t excl = incl - run, Q = 0;
        for (int w = 0; w < nw; ++w) {
            if (w < wave) excl += red1[w];
            Q += red1[w];
        }
        if (Q == 0) {   // uniform over the block: exp_norm of these weights is NaN
            if (tid == 0) *a.flag = 1;
            return;
        }
        const uint64_t x = wsmc_multi_target(wsmc_multi_word(seed, (uint64_t)t * (uint64_t)M + (uint64_t)m, 0), Q);
        if (run > 0 && excl <= x && x - excl < run) {   // the one thread whose range holds the target
            uint64_t C = excl;
            int win = i1 - 1;
            for (int i = i0; i < i1; ++i) {
                C += wsmc_qweight(lwb[i], R, K);
                if (C > x) {
                    win = i;
                    break;
                }
            }
            bc[0] = (uint64_t)(uint32_t)win;
            idx[(size_t)t * M + m] = win;
        }
        __syncthreads();
        sel = (int)(uint32_t)bc[0];
        // (the next step writes red0 behind this barrier, red1 behind its first, bc behind its second)
    }
}

__global__ __launch_bounds__(kSsMaxThreads) void k_ssm_backward_rows(SsmBwRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char br_smem[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int N = a.N, M = a.M, P = a.P, S = a.S;
    const size_t bt = blockIdx.x;   // row (b, t)
    SsState L;
    L.stride = (int)ss_n8(M);
    L.cb = reinterpret_cast<double*>(br_smem);
    L.lw = L.cb + (size_t)(S + 1) * L.stride;
    L.anc = nullptr;   // (no Resample here)
    L.red = reinterpret_cast<uint64_t*>(L.lw + L.stride);
    L.S = S;
    L.off = 0;
    L.N = M;
    L.i0 = tid * P < M ? tid * P : M;
    L.i1 = L.i0 + P < M ? L.i0 + P : M;
    L.lane = tid & 63;
    L.wave = tid >> 6;
    L.nw = (nthr + 63) >> 6;
#ifdef WSMC_TABLES_LDS
    wsmc_tables_to_lds();   // before any exp (every thread: it ends in a barrier)
#endif
    const int32_t* idx = a.idx + bt * (size_t)M;
    const double* hist = a.hist + bt * (size_t)S * N;
    for (int i = L.i0; i < L.i1; ++i) L.lw[i] = 0.0;   // fresh (equal) weights
    for (int k = 0; k < S; ++k) {
        const double* src = hist + (size_t)k * N;
        double* dst = L.cb + (size_t)k * L.stride;
        for (int i = L.i0; i < L.i1; ++i) {
            int j = idx[i];
            j = j < 0 ? 0 : j >= N ? N - 1 : j;   // (a pass that ended early leaves rows it never drew)
            dst[i] = src[j];
        }
    }
    if (a.paths)
        for (int k = 0; k < S; ++k) {
            double* dst = a.paths + (bt * S + (size_t)k) * M;
            const double* src = L.cb + (size_t)k * L.stride;
            for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
        }
    if (a.mean || a.var) ss_trace_row(L, a.mean ? a.mean + bt * S : nullptr, a.var ? a.var + bt * S : nullptr);
}

int ssm_backward_threads(int n) { return std::max(64, std::min(kBwThreads, ((n + 63) / 64) * 64)); }

hipError_t launch_ssm_backward(hipStream_t s, const SsmBwArgs& a, unsigned feat, int threads) {
    if (!a.hist || !a.lwlog || !a.idx || !a.flag || !a.filt || a.N < 1 || a.N > kLgCap || a.S < 1 || a.S > WSMC_SSM_MAX_COLS ||
        a.T < 1 || a.M < 1 || a.B < 1 || (int64_t)a.B * a.M > INT32_MAX || threads < 64 || threads > kBwThreads || (threads & 63) ||
        a.P < 1 || (int64_t)a.P * threads < a.N || a.n_step < 1 || a.n_step > WSMC_SSM_MAX_STMTS || a.data_dim < 0 ||
        a.data_dim > WSMC_SSM_MAX_DATA)
        return hipErrorInvalidValue;
    const size_t lds = ss_n8(a.N) * sizeof(double) + kBwScratch * sizeof(uint64_t);   // at most 41 KiB: within the default
    const dim3 grid((unsigned)((int64_t)a.B * a.M)), block((unsigned)threads);
    if (feat & WSMC_FEAT_GAM)
        hipLaunchKernelGGL(k_ssm_backward<kSsFeatGam>, grid, block, lds, s, a);
    else if (feat & WSMC_FEAT_EXT)
        hipLaunchKernelGGL(k_ssm_backward<kSsFeatExt>, grid, block, lds, s, a);
    else
        hipLaunchKernelGGL(k_ssm_backward<0u>, grid, block, lds, s, a);
    return hipGetLastError();
}

hipError_t launch_ssm_backward_rows(hipStream_t s, const double* hist, const int32_t* idx, double* paths, double* mean,
                                    double* var, int N, int M, int S, int T, int B) {
    if (!hist || !idx || S < 1 || S > WSMC_SSM_MAX_COLS || N < 1 || N > kLgCap || M < 1 || M > ssm_cap(S) || T < 1 || B < 1 ||
        (int64_t)B * T > INT32_MAX)
        return hipErrorInvalidValue;
    if (!paths && !mean && !var) return hipSuccess;
    const int threads = std::max(64, std::min(kSsMaxThreads, ((M + 127) / 128) * 64));
    // the fused kernel's layout without the ancestors: S + 1 column buffers, the log-weights, the scratch
    const size_t lds = ((size_t)S + 2) * ss_n8(M) * sizeof(double) + kSsScratch * sizeof(uint64_t);
    if (lds + 4096 > 160 * 1024) return hipErrorInvalidValue;
    if (const hipError_t e = ss_ask_lds(k_ssm_backward_rows, lds); e != hipSuccess) return e;
    SsmBwRowsArgs a;
    a.hist = hist;
    a.idx = idx;
    a.paths = paths;
    a.mean = mean;
    a.var = var;
    a.N = N;
    a.M = M;
    a.S = S;
    a.P = (M + threads - 1) / threads;
    hipLaunchKernelGGL(k_ssm_backward_rows, dim3((unsigned)((int64_t)B * T)), dim3(threads), lds, s, a);
    return hipGetLastError();
}

}  // namespace wsmc
