// wsmc_ssm_batch.hip — B independent fused runs of a specified scalar SSM in one launch
// (wsmc_ssm_run_batch): block b of a dim3(B) grid is csrc/wsmc_ssm.hip's persistent workgroup for
// filter b, with the same step body (csrc/wsmc_ssm_body.h), the same LDS layout and the same
// thread-to-particle map, so filter b's bits are those of wsmc_ssm_run on a fresh context.
//
// What differs per filter is read per block: its image of the compact statements (the numbers
// differ, the shape does not), its seed and its data table, from filt[blockIdx.x] through a
// constant-address-space pointer. The images are written before the first launch and by nothing
// while a kernel runs; the address is block-uniform, so the loads are scalar and the branches
// uniform, as with the single run's kernel arguments. What is one for the batch (sizes, the
// segment, the scheme, the threshold) rides in the kernel arguments.
//
// No block waits on another: a grid larger than the device holds simply queues. The state between
// segments is in the call's device buffers, [B] rows of what the single run keeps in its context.
// The run's last segment leaves the record of the final weights (the max and the exact integer
// sums the Resample takes), from which the host finishes the evidence.
#ifdef __HIP_DEVICE_COMPILE__
#define WSMC_TABLES_LDS   // include/wsmc_math.h: the device pass reads LDS copies of the tables
#endif
#include "wsmc_ssm_body.h"

namespace wsmc {

// compiled twice, as csrc/wsmc_ssm.hip is: as it stands for the untraced instantiations, through
// csrc/wsmc_ssm_batch_traced.hip (WSMC_SSM_TRACED) for the traced ones
// and through csrc/wsmc_ssm_batch_smooth.hip (WSMC_SSM_SMOOTH) for the recording ones of a smoothed
// batch: a kernel of another name with arguments of its own, as in csrc/wsmc_ssm.hip
// and through csrc/wsmc_ssm_batch_guided.hip (WSMC_SSM_GUIDED) and
// csrc/wsmc_ssm_batch_guided_smooth.hip (both macros) for the kernels of a guided spec's batch, as
// in csrc/wsmc_ssm.hip
// and through csrc/wsmc_ssm_batch_backward_rec.hip (WSMC_SSM_BWREC) and
// csrc/wsmc_ssm_batch_guided_backward_rec.hip (with WSMC_SSM_GUIDED) for a batch that ends in backward
// simulation: the trace point's columns and log-weights logged, no ancestors, as in csrc/wsmc_ssm.hip
// and through csrc/wsmc_ssm_batch_conditional.hip (WSMC_SSM_COND over WSMC_SSM_BWREC) for a conditional
// batch (wsmc_ssm_run_conditional): the backward-recording kernel with the reference trajectory pinned
// into particle N - 1 after every SAMPLE of `step` and ss_resample's conditional branch. Kernels of
// other names once more
#if defined(WSMC_SSM_COND) && (!defined(WSMC_SSM_BWREC) || defined(WSMC_SSM_GUIDED) || defined(WSMC_SSM_SMOOTH))
#error "WSMC_SSM_COND goes with WSMC_SSM_BWREC alone"
#endif
#if defined(WSMC_SSM_GUIDED)
constexpr bool kSsbTraced = true, kSsbGuided = true;
#if defined(WSMC_SSM_BWREC)
#define WSMC_SSB_OCCUPANCY ssb_occupancy_guided_bwrec
#define WSMC_SSB_VARIANTS ssb_launch_guided_bwrec
#define WSMC_SSB_KERNEL k_ssm_batch_guided_segment_bwrec
typedef SsmBatchGuidedBwArgs SsbKernArgs;
#elif defined(WSMC_SSM_SMOOTH)
#define WSMC_SSB_OCCUPANCY ssb_occupancy_guided_rec
#define WSMC_SSB_VARIANTS ssb_launch_guided_rec
#define WSMC_SSB_KERNEL k_ssm_batch_guided_segment_rec
typedef SsmBatchGuidedArgs SsbKernArgs;
#else
#define WSMC_SSB_OCCUPANCY ssb_occupancy_guided
#define WSMC_SSB_VARIANTS ssb_launch_guided
#define WSMC_SSB_KERNEL k_ssm_batch_guided_segment
typedef SsmBatchGuidedArgs SsbKernArgs;
#endif
namespace {
constexpr int kSsbVariantGamThreads = kSsGuidedGamThreads;
typedef const SsmTarget __attribute__((address_space(4))) * SsTargetPtr;
}
#elif defined(WSMC_SSM_COND)
constexpr bool kSsbTraced = true;
#define WSMC_SSB_OCCUPANCY ssb_occupancy_cond
#define WSMC_SSB_VARIANTS ssb_launch_cond
#define WSMC_SSB_KERNEL k_ssm_batch_segment_cond
typedef SsmBatchCondArgs SsbKernArgs;
#elif defined(WSMC_SSM_BWREC)
constexpr bool kSsbTraced = true;
#define WSMC_SSB_OCCUPANCY ssb_occupancy_bwrec
#define WSMC_SSB_VARIANTS ssb_launch_bwrec
#define WSMC_SSB_KERNEL k_ssm_batch_segment_bwrec
typedef SsmBatchBwRecArgs SsbKernArgs;
#elif defined(WSMC_SSM_SMOOTH)
constexpr bool kSsbTraced = true;
#define WSMC_SSB_OCCUPANCY ssb_occupancy_rec
#define WSMC_SSB_VARIANTS ssb_launch_rec
#define WSMC_SSB_KERNEL k_ssm_batch_segment_rec
typedef SsmBatchRecArgs SsbKernArgs;
#elif defined(WSMC_SSM_TRACED)
constexpr bool kSsbTraced = true;
#define WSMC_SSB_OCCUPANCY ssb_occupancy_traced
#define WSMC_SSB_VARIANTS ssb_launch_traced
#define WSMC_SSB_KERNEL k_ssm_batch_segment
typedef SsmBatchArgs SsbKernArgs;
#else
constexpr bool kSsbTraced = false;
#define WSMC_SSB_OCCUPANCY ssb_occupancy_untraced
#define WSMC_SSB_VARIANTS ssb_launch_untraced
#define WSMC_SSB_KERNEL k_ssm_batch_segment
typedef SsmBatchArgs SsbKernArgs;
#endif

namespace {
typedef const SsmBatchFilter __attribute__((address_space(4))) * SsFilterPtr;
#ifndef WSMC_SSM_GUIDED
constexpr bool kSsbGuided = false;
constexpr int kSsbVariantGamThreads = kSsGamThreads;
#endif
#ifdef WSMC_SSM_COND
constexpr bool kSsbCond = true;
#else
constexpr bool kSsbCond = false;
#endif
}

// TR: the traced batch (wsmc_ssm_run_batch_traced), k_ssm_segment's flag
template <unsigned FEAT, int THREADS, bool TR>
#if defined(WSMC_SSM_GUIDED) && defined(WSMC_SSM_BWREC)
__global__ __launch_bounds__(THREADS) void WSMC_SSB_KERNEL(const SsmBatchGuidedBwArgs ga) {
    const SsmBatchBwRecArgs& ka = ga.ra;
    const SsmBatchArgs& a = ka.a;
#elif defined(WSMC_SSM_GUIDED)
__global__ __launch_bounds__(THREADS) void WSMC_SSB_KERNEL(const SsmBatchGuidedArgs ga) {
    const SsmBatchRecArgs& ka = ga.ra;
    const SsmBatchArgs& a = ka.a;
#elif defined(WSMC_SSM_COND)
__global__ __launch_bounds__(THREADS) void WSMC_SSB_KERNEL(const SsmBatchCondArgs ca) {
    const SsmBatchBwRecArgs& ka = ca.ra;
    const SsmBatchArgs& a = ka.a;
#elif defined(WSMC_SSM_BWREC)
__global__ __launch_bounds__(THREADS) void WSMC_SSB_KERNEL(const SsmBatchBwRecArgs ka) {
    const SsmBatchArgs& a = ka.a;
#elif defined(WSMC_SSM_SMOOTH)
__global__ __launch_bounds__(THREADS) void WSMC_SSB_KERNEL(const SsmBatchRecArgs ka) {
    const SsmBatchArgs& a = ka.a;
#else
__global__ __launch_bounds__(THREADS) void WSMC_SSB_KERNEL(const SsmBatchArgs a) {
#endif
    extern __shared__ __attribute__((aligned(16))) char ssb_smem[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const size_t b = blockIdx.x;
#ifdef WSMC_SSM_SMOOTH
    // filter b's rows of the history and of the log
    double* hist = ka.r.hist + b * (size_t)ka.r.T * (size_t)a.S * (size_t)a.N;
    int32_t* alog = ka.r.alog + b * (size_t)ka.r.T * (size_t)ka.r.n_slots * (size_t)a.N;
    int32_t* ranf = ka.r.ran + b * (size_t)ka.r.T * (size_t)ka.r.n_slots;
#endif
#ifdef WSMC_SSM_BWREC
    // filter b's rows of the record
    double* hist = ka.r.hist + b * (size_t)ka.r.T * (size_t)a.S * (size_t)a.N;
    double* lwlog = ka.r.lwlog + b * (size_t)ka.r.T * (size_t)a.N;
#endif
#ifdef WSMC_SSM_GUIDED
    // filter b's targets (block-uniform: scalar loads, as its statements' below)
    const SsmTarget* const tgs = (const SsmTarget*)((SsTargetPtr)ga.targ + b * (size_t)kSsmTargets);
#endif
    const SsmBatchFilter& f = *(const SsmBatchFilter*)((SsFilterPtr)a.filt + b);
    const int N = a.N, P = a.P, S = a.S;
    SsState L;
    L.stride = (int)ss_n8(N);
    L.cb = reinterpret_cast<double*>(ssb_smem);
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

    double* gw = a.w + b * (size_t)N;
    double* gx = a.x + b * (size_t)S * (size_t)N;
    int32_t* ganc = a.anc + b * (size_t)N;
    SsmBatchRec* rec = a.rec + b;

#ifdef WSMC_TABLES_LDS
    wsmc_tables_to_lds();   // before any log / exp (every thread: it ends in a barrier)
#endif
    for (int i = L.i0; i < L.i1; ++i) L.lw[i] = gw[i];
    for (int k = 0; k < S; ++k) {
        const double* src = gx + (size_t)k * N;
        double* dst = L.cb + (size_t)k * L.stride;
        for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
    }

    const int K = wsmc_qbits((uint64_t)N);
    const int dd = a.data_dim;
    const SsConstPtr data = (SsConstPtr)f.data;
    const uint64_t seed = f.seed;
    long long nres = 0;
    int last_dec = 0, ran = 0;
    double last_ess = 0.0;
    SsData dv = {0.0, 0.0, 0.0, 0.0};

    SsData dnext = dv;
    if (a.nsteps > 0) dnext = ss_row(data, dd, a.t0);
#ifdef WSMC_SSM_COND
    // filter b's reference trajectory [T][S], read as the data table is: the step's row a step ahead
    static_assert(WSMC_SSM_MAX_COLS <= WSMC_SSM_MAX_DATA, "SsData holds a row of the reference");
    const SsConstPtr ref = (SsConstPtr)ca.ref + b * (size_t)a.T * (size_t)S;
    SsData rv = dv, rnext = dv;
    if (a.nsteps > 0) rnext = ss_row(ref, S, a.t0);
#endif

    // k_ssm_segment's loop: s = -1 is `init` (a fresh context: the op counter starts at 0)
    static_assert(offsetof(SsmBatchFilter, step) == offsetof(SsmBatchFilter, init) + WSMC_SSM_MAX_INIT * sizeof(SsmStmt),
                  "step follows init: one statement array");
    for (int s = a.first ? -1 : 0; s < a.nsteps; ++s) {
        const int t = a.t0 + s;
        const bool init = s < 0;
        const SsmStmt* list = f.init + (init ? 0 : WSMC_SSM_MAX_INIT);
        const int nst = init ? a.n_init : a.n_step;
        uint64_t op = init ? 0 : (uint64_t)a.init_ops + (uint64_t)a.step_ops * (uint64_t)t;
        if (!init) {
            dv = dnext;
            if (s + 1 < a.nsteps) dnext = ss_row(data, dd, t + 1);   // in flight during this step
#ifdef WSMC_SSM_COND
            rv = rnext;
            if (s + 1 < a.nsteps) rnext = ss_row(ref, S, t + 1);
#endif
        }
#ifdef WSMC_SSM_SMOOTH
        int slot = t * ka.r.n_slots;   // the log's slot of the step's next Resample that can run
#endif
        for (int q = 0; q < nst; ++q) {
            const SsmStmt& st = list[q];
#ifdef WSMC_SSM_GUIDED
            ss_statement<FEAT, true>(st, f.ins, L, dv, seed, op, tgs + (init ? q : WSMC_SSM_MAX_INIT + q));
#else
            ss_statement<FEAT>(st, f.ins, L, dv, seed, op);
#endif
            if (st.kind == WSMC_SSM_SAMPLE) {
#ifdef WSMC_SSM_COND
                // the pin: the owner of particle N - 1 overwrites the draw it has just stored
                if (!init && L.i0 < N && L.i1 == N) L.cb[(size_t)ss_buf(L, st.col) * L.stride + (N - 1)] = ss_data(rv, st.col);
#endif
                op += 2;   // the draws, then a Resample that does not run (the weights have not changed)
            } else if (st.kind == WSMC_SSM_OBSERVE ||
                       (kSsbGuided && (st.kind == WSMC_SSM_WEIGHT || st.kind == WSMC_SSM_SAMPLE_IMPORTANCE))) {
                if (kSsbGuided && st.kind == WSMC_SSM_SAMPLE_IMPORTANCE) op += 1;   // its draws took `op`; its Resample can run
                const bool row = TR && !init && q == a.last_obs;
                const size_t r = b * (size_t)a.T + (size_t)t;
#if defined(WSMC_SSM_SMOOTH) || defined(WSMC_SSM_BWREC)
                if (row) ss_record_cols(L, hist + (size_t)t * S * N);
#endif
#ifdef WSMC_SSM_BWREC
                if (row) ss_record_lw(L, lwlog + (size_t)t * N);
#endif
                if (row && (a.tr_mean || a.tr_var))
                    ss_trace_row(L, a.tr_mean ? a.tr_mean + r * S : nullptr, a.tr_var ? a.tr_var + r * S : nullptr);
                const SsDecision d = ss_resample<TR, kSsbCond>(L, K, a.ess_min, a.scheme, seed, op);
#ifdef WSMC_SSM_SMOOTH
                if (!init) {
                    if (d.resampled) ss_record_anc(L, alog + (size_t)slot * N, ranf + slot);
                    slot += 1;
                }
#endif
                if (row && a.tr_logev && tid == 0) a.tr_logev[r] = d.logev;
                op += 1;
                nres += d.resampled;
                last_dec = d.resampled;
                last_ess = d.ess;
                ran = 1;
                if (!init && q == a.last_obs && a.ess_trace && tid == 0) a.ess_trace[b * (size_t)a.T + t] = d.ess;
            }
        }
    }

    for (int k = 0; k < S; ++k) {
        double* dst = gx + (size_t)k * N;
        const double* src = L.cb + (size_t)ss_buf(L, k) * L.stride;
        for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
    }
    for (int i = L.i0; i < L.i1; ++i) gw[i] = L.lw[i];
    if (nres > 0)
        for (int i = L.i0; i < L.i1; ++i) ganc[i] = L.anc[i];
    if (tid == 0 && ran) {
        rec->nres += nres;
        rec->last_dec = last_dec;
        rec->last_ess = last_ess;
    }

    // the run's end: the record of the final weights, ss_resample's max and sums (exact integers:
    // any order of summation gives the same record), for wsmc_global_log_evidence on the host
    if (a.last) {
        uint64_t* red0 = L.red;
        uint64_t* red1 = L.red + kSsWaves * 4;
        __syncthreads();   // the last Resample's readers of the scratch are through
        uint64_t menc = WSMC_ORD_NEG_INF;
        for (int i = L.i0; i < L.i1; ++i) {
            const uint64_t e = wsmc_ord_enc(L.lw[i]);
            menc = e > menc ? e : menc;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t o = ss_shfl_xor(menc, m);
            menc = o > menc ? o : menc;
        }
        if (L.lane == 0) red0[L.wave] = menc;
        __syncthreads();
        for (int w = 0; w < L.nw; ++w) menc = red0[w] > menc ? red0[w] : menc;
        const double M = wsmc_ord_dec(menc);
        const double R = wsmc_qref(M);
        uint64_t sQ = 0, sQ2 = 0, sWf = 0, sWf2 = 0;
        for (int i = L.i0; i < L.i1; ++i) {
            const wsmc_qparts p = wsmc_qparts_of(L.lw[i], R, K);
            sQ += p.q; sQ2 += p.q2; sWf += p.wf; sWf2 += p.wf2;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            sQ += ss_shfl_xor(sQ, m);
            sQ2 += ss_shfl_xor(sQ2, m);
            sWf += ss_shfl_xor(sWf, m);
            sWf2 += ss_shfl_xor(sWf2, m);
        }
        if (L.lane == 0) {
            red1[L.wave * 4 + 0] = sQ; red1[L.wave * 4 + 1] = sQ2; red1[L.wave * 4 + 2] = sWf; red1[L.wave * 4 + 3] = sWf2;
        }
        __syncthreads();
        if (tid == 0) {
            uint64_t Q = 0, Q2 = 0, Wf = 0, Wf2 = 0;
            for (int w = 0; w < L.nw; ++w) {
                Q += red1[w * 4 + 0]; Q2 += red1[w * 4 + 1];
                Wf += red1[w * 4 + 2]; Wf2 += red1[w * 4 + 3];
            }
            rec->M = M;
            rec->Q = Q; rec->Q2 = Q2; rec->Wf = Wf; rec->Wf2 = Wf2;
        }
    }
}

namespace {

template <unsigned FEAT, int THREADS>
hipError_t ssb_occupancy(int threads, size_t lds, int* per_cu) {
    const void* k = reinterpret_cast<const void*>(WSMC_SSB_KERNEL<FEAT, THREADS, kSsbTraced>);
    if (const hipError_t e = ss_ask_lds(k, lds); e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, k, threads, lds);
}

template <unsigned FEAT, int THREADS>
hipError_t ssb_launch(hipStream_t s, const SsbKernArgs& a, int threads, size_t lds, int B) {
    if (const hipError_t e = ss_ask_lds(WSMC_SSB_KERNEL<FEAT, THREADS, kSsbTraced>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((WSMC_SSB_KERNEL<FEAT, THREADS, kSsbTraced>), dim3((unsigned)B), dim3(threads), lds, s, a);
    return hipGetLastError();
}

}  // namespace

// this unit's three feature variants
hipError_t WSMC_SSB_OCCUPANCY(unsigned feat, int threads, size_t lds, int* per_cu) {
    if (feat & WSMC_FEAT_GAM) return ssb_occupancy<kSsFeatGam, kSsbVariantGamThreads>(threads, lds, per_cu);
    if (feat & WSMC_FEAT_EXT) return ssb_occupancy<kSsFeatExt, kSsMaxThreads>(threads, lds, per_cu);
    return ssb_occupancy<0u, kSsMaxThreads>(threads, lds, per_cu);
}
hipError_t WSMC_SSB_VARIANTS(hipStream_t s, const SsbKernArgs& a, unsigned feat, int threads, size_t lds, int B) {
    if (feat & WSMC_FEAT_GAM) return ssb_launch<kSsFeatGam, kSsbVariantGamThreads>(s, a, threads, lds, B);
    if (feat & WSMC_FEAT_EXT) return ssb_launch<kSsFeatExt, kSsMaxThreads>(s, a, threads, lds, B);
    return ssb_launch<0u, kSsMaxThreads>(s, a, threads, lds, B);
}

#if !defined(WSMC_SSM_TRACED) && !defined(WSMC_SSM_SMOOTH) && !defined(WSMC_SSM_GUIDED) && !defined(WSMC_SSM_BWREC)
hipError_t ssb_occupancy_cond(unsigned feat, int threads, size_t lds, int* per_cu);           // csrc/wsmc_ssm_batch_conditional.hip
hipError_t ssb_launch_cond(hipStream_t s, const SsmBatchCondArgs& a, unsigned feat, int threads, size_t lds, int B);
hipError_t ssb_occupancy_bwrec(unsigned feat, int threads, size_t lds, int* per_cu);          // csrc/wsmc_ssm_batch_backward_rec.hip
hipError_t ssb_launch_bwrec(hipStream_t s, const SsmBatchBwRecArgs& a, unsigned feat, int threads, size_t lds, int B);
hipError_t ssb_occupancy_guided_bwrec(unsigned feat, int threads, size_t lds, int* per_cu);   // csrc/wsmc_ssm_batch_guided_backward_rec.hip
hipError_t ssb_launch_guided_bwrec(hipStream_t s, const SsmBatchGuidedBwArgs& a, unsigned feat, int threads, size_t lds, int B);
hipError_t ssb_occupancy_guided(unsigned feat, int threads, size_t lds, int* per_cu);       // csrc/wsmc_ssm_batch_guided.hip
hipError_t ssb_launch_guided(hipStream_t s, const SsmBatchGuidedArgs& a, unsigned feat, int threads, size_t lds, int B);
hipError_t ssb_occupancy_guided_rec(unsigned feat, int threads, size_t lds, int* per_cu);   // csrc/wsmc_ssm_batch_guided_smooth.hip
hipError_t ssb_launch_guided_rec(hipStream_t s, const SsmBatchGuidedArgs& a, unsigned feat, int threads, size_t lds, int B);
hipError_t ssb_occupancy_traced(unsigned feat, int threads, size_t lds, int* per_cu);   // csrc/wsmc_ssm_batch_traced.hip
hipError_t ssb_launch_traced(hipStream_t s, const SsmBatchArgs& a, unsigned feat, int threads, size_t lds, int B);
hipError_t ssb_occupancy_rec(unsigned feat, int threads, size_t lds, int* per_cu);      // csrc/wsmc_ssm_batch_smooth.hip
hipError_t ssb_launch_rec(hipStream_t s, const SsmBatchRecArgs& a, unsigned feat, int threads, size_t lds, int B);

hipError_t ssm_batch_occupancy(int device, unsigned feat, int variant, int threads, size_t lds, int* per_cu, int* cus) {
    const hipError_t e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    if (variant == 7) return ssb_occupancy_cond(feat, threads, lds, per_cu);
    if (variant == 6) return ssb_occupancy_guided_bwrec(feat, threads, lds, per_cu);
    if (variant == 5) return ssb_occupancy_bwrec(feat, threads, lds, per_cu);
    if (variant == 4) return ssb_occupancy_guided_rec(feat, threads, lds, per_cu);
    if (variant == 3) return ssb_occupancy_guided(feat, threads, lds, per_cu);
    if (variant == 2) return ssb_occupancy_rec(feat, threads, lds, per_cu);
    return variant ? ssb_occupancy_traced(feat, threads, lds, per_cu) : ssb_occupancy_untraced(feat, threads, lds, per_cu);
}

static bool ssb_segment_ok(const SsmBatchArgs& a, unsigned feat, int threads, bool guided = false) {
    return ss_segment_ok(a, feat, threads, guided) && a.B >= 1 && a.t0 + a.nsteps <= a.T && a.x && a.w && a.anc && a.rec && a.filt;
}

hipError_t launch_ssm_batch_segment(hipStream_t s, const SsmBatchArgs& a, unsigned feat, int threads) {
    if (!ssb_segment_ok(a, feat, threads)) return hipErrorInvalidValue;
    const size_t lds = ssm_lds_bytes(a.N, a.S);
    if (a.tr_mean || a.tr_var || a.tr_logev) return ssb_launch_traced(s, a, feat, threads, lds, a.B);
    return ssb_launch_untraced(s, a, feat, threads, lds, a.B);
}

hipError_t launch_ssm_batch_segment_rec(hipStream_t s, const SsmBatchRecArgs& a, unsigned feat, int threads) {
    if (!ssb_segment_ok(a.a, feat, threads) || !a.r.hist || !a.r.alog || !a.r.ran || a.r.n_slots < 1 || a.r.T != a.a.T)
        return hipErrorInvalidValue;
    return ssb_launch_rec(s, a, feat, threads, ssm_lds_bytes(a.a.N, a.a.S), a.a.B);
}

hipError_t launch_ssm_batch_guided_segment(hipStream_t s, const SsmBatchGuidedArgs& a, unsigned feat, int threads, bool rec) {
    const SsmBatchArgs& ba = a.ra.a;
    const SsmRec& r = a.ra.r;
    if (!ssb_segment_ok(ba, feat, threads, true) || !a.targ) return hipErrorInvalidValue;
    if (rec && (!r.hist || !r.alog || !r.ran || r.n_slots < 1 || r.trace_slot < 0 || r.trace_slot >= r.n_slots || r.T != ba.T))
        return hipErrorInvalidValue;
    const size_t lds = ssm_lds_bytes(ba.N, ba.S);
    return rec ? ssb_launch_guided_rec(s, a, feat, threads, lds, ba.B) : ssb_launch_guided(s, a, feat, threads, lds, ba.B);
}

hipError_t launch_ssm_batch_segment_bwrec(hipStream_t s, const SsmBatchBwRecArgs& a, unsigned feat, int threads) {
    if (!ssb_segment_ok(a.a, feat, threads) || !a.r.hist || !a.r.lwlog || a.r.T != a.a.T) return hipErrorInvalidValue;
    return ssb_launch_bwrec(s, a, feat, threads, ssm_lds_bytes(a.a.N, a.a.S), a.a.B);
}

hipError_t launch_ssm_batch_guided_segment_bwrec(hipStream_t s, const SsmBatchGuidedBwArgs& a, unsigned feat, int threads) {
    const SsmBatchArgs& ba = a.ra.a;
    if (!ssb_segment_ok(ba, feat, threads, true) || !a.targ || !a.ra.r.hist || !a.ra.r.lwlog || a.ra.r.T != ba.T) return hipErrorInvalidValue;
    return ssb_launch_guided_bwrec(s, a, feat, threads, ssm_lds_bytes(ba.N, ba.S), ba.B);
}

hipError_t launch_ssm_batch_segment_cond(hipStream_t s, const SsmBatchCondArgs& a, unsigned feat, int threads) {
    const SsmBatchArgs& ba = a.ra.a;
    if (!ssb_segment_ok(ba, feat, threads) || !a.ref || !a.ra.r.hist || !a.ra.r.lwlog || a.ra.r.T != ba.T) return hipErrorInvalidValue;
    return ssb_launch_cond(s, a, feat, threads, ssm_lds_bytes(ba.N, ba.S), ba.B);
}
#endif

}  // namespace wsmc
