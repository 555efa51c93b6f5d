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
#include "wsmc_ssm_body.h"   // the step body (ss_statement, ss_resample), shared with wsmc_ssm_batch.hip

namespace wsmc {

// This file is compiled twice: as it stands for the untraced instantiations, and through
// csrc/wsmc_ssm_traced.hip, which defines WSMC_SSM_TRACED, for the traced ones. A translation
// unit of their own keeps the untraced kernels what the compiler made of them before there was a
// trace: with six kernels in one unit instead of three the inliner's choices change and the
// log-Gamma variant goes from 116 VGPRs to 128 and spills.
// A third time through csrc/wsmc_ssm_smooth.hip (WSMC_SSM_SMOOTH) for the recording ones of a
// smoothed run: traced instantiations that also log the trace point's columns and each Resample's
// ancestors (SsmRec). They are a kernel of another name with arguments of their own, so the other
// two units' kernels are, to the instruction, what they were before there was a log.
// A fourth and a fifth time through csrc/wsmc_ssm_guided.hip (WSMC_SSM_GUIDED) and
// csrc/wsmc_ssm_guided_smooth.hip (both macros) for the kernels of a guided spec, one with an
// importance SAMPLE or a WEIGHT: traced-capable instantiations (null trace pointers serve an
// untraced call) whose statement body also holds k_sample_importance's arithmetic, and their
// recording twins. Kernels of other names again, so a spec without the new kinds launches what it
// always has.
// A sixth and a seventh time through csrc/wsmc_ssm_backward_rec.hip (WSMC_SSM_BWREC) and
// csrc/wsmc_ssm_guided_backward_rec.hip (with WSMC_SSM_GUIDED) for a run that ends in backward
// simulation (wsmc_ssm_run_backward): traced instantiations that log the trace point's columns and
// log-weights (SsmBwRec) and no ancestors. Kernels of other names once more.
#if defined(WSMC_SSM_GUIDED)
constexpr bool kSsTraced = true, kSsGuided = true;
#if defined(WSMC_SSM_BWREC)
#define WSMC_SSM_VARIANTS ssm_launch_guided_bwrec
#define WSMC_SSM_KERNEL k_ssm_guided_segment_bwrec
typedef SsmGuidedBwArgs SsKernArgs;
#elif defined(WSMC_SSM_SMOOTH)
#define WSMC_SSM_VARIANTS ssm_launch_guided_rec
#define WSMC_SSM_KERNEL k_ssm_guided_segment_rec
typedef SsmGuidedArgs SsKernArgs;
#else
#define WSMC_SSM_VARIANTS ssm_launch_guided
#define WSMC_SSM_KERNEL k_ssm_guided_segment
typedef SsmGuidedArgs SsKernArgs;
#endif
namespace {
constexpr int kSsVariantGamThreads = kSsGuidedGamThreads;
typedef const SsmTarget __attribute__((address_space(4))) * SsTargetPtr;
}
#elif defined(WSMC_SSM_BWREC)
constexpr bool kSsTraced = true;
#define WSMC_SSM_VARIANTS ssm_launch_bwrec
#define WSMC_SSM_KERNEL k_ssm_segment_bwrec
typedef SsmBwRecArgs SsKernArgs;
#elif defined(WSMC_SSM_SMOOTH)
constexpr bool kSsTraced = true;
#define WSMC_SSM_VARIANTS ssm_launch_rec
#define WSMC_SSM_KERNEL k_ssm_segment_rec
typedef SsmRecArgs SsKernArgs;
#elif defined(WSMC_SSM_TRACED)
constexpr bool kSsTraced = true;
#define WSMC_SSM_VARIANTS ssm_launch_traced
#define WSMC_SSM_KERNEL k_ssm_segment
typedef SsmArgs SsKernArgs;
#else
constexpr bool kSsTraced = false;
#define WSMC_SSM_VARIANTS ssm_launch_untraced
#define WSMC_SSM_KERNEL k_ssm_segment
typedef SsmArgs SsKernArgs;

// the kernel's dynamic LDS for n particles in S columns (beside the 4 KiB of static log / exp tables)
size_t ssm_lds_bytes(int n, int S) {
    return ((size_t)S + 2) * ss_n8(n) * sizeof(double) + ss_n4(n) * sizeof(int32_t) + kSsScratch * sizeof(uint64_t);
}
#endif

#ifndef WSMC_SSM_GUIDED
namespace {
constexpr bool kSsGuided = false;
constexpr int kSsVariantGamThreads = kSsGamThreads;
}
#endif

// TR: the traced run (wsmc_ssm_run_traced), which also leaves row t of the moments and the evidence
// at the ESS trace's point
template <unsigned FEAT, int THREADS, bool TR>
__global__ __launch_bounds__(THREADS) void WSMC_SSM_KERNEL(SsKernArgs) {
    const SsmArgs& a = *(const SsmArgs*)(const char*)__builtin_amdgcn_kernarg_segment_ptr();
#ifdef WSMC_SSM_SMOOTH
    static_assert(offsetof(SsmRecArgs, a) == 0, "the run's arguments come first");
    const SsmRec& rc = *(const SsmRec*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SsmRecArgs, r));
#endif
#ifdef WSMC_SSM_BWREC
    static_assert(offsetof(SsmBwRecArgs, a) == 0, "the run's arguments come first");
    const SsmBwRec& rc = *(const SsmBwRec*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SsmBwRecArgs, r));
#endif
#ifdef WSMC_SSM_GUIDED
    static_assert(offsetof(SsKernArgs, ra) == 0, "the run's arguments come first");
    // the targets: written before the run's first launch and by nothing while a kernel runs; a
    // uniform address, so the loads are scalar (as the batch kernel reads its SsmBatchFilter)
    const SsmTarget* const tgs = (const SsmTarget*)(SsTargetPtr)(
        *(const SsmTarget* const*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SsKernArgs, targ)));
#endif
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
#ifdef WSMC_SSM_SMOOTH
        int slot = t * rc.n_slots;   // the log's slot of the step's next Resample that can run
#endif
        for (int q = 0; q < nst; ++q) {
            const SsmStmt& st = list[q];
#ifdef WSMC_SSM_GUIDED
            ss_statement<FEAT, true>(st, a.ins, L, dv, a.seed, op, tgs + (init ? q : WSMC_SSM_MAX_INIT + q));
#else
            ss_statement<FEAT>(st, a.ins, L, dv, a.seed, op);
#endif
            if (st.kind == WSMC_SSM_SAMPLE) {
                op += 2;   // the draws, then a Resample that does not run (the weights have not changed)
            } else if (st.kind == WSMC_SSM_OBSERVE ||
                       (kSsGuided && (st.kind == WSMC_SSM_WEIGHT || st.kind == WSMC_SSM_SAMPLE_IMPORTANCE))) {
                if (kSsGuided && st.kind == WSMC_SSM_SAMPLE_IMPORTANCE) op += 1;   // its draws took `op`; its Resample can run
                const bool row = TR && !init && q == a.last_obs;
#if defined(WSMC_SSM_SMOOTH) || defined(WSMC_SSM_BWREC)
                if (row) ss_record_cols(L, rc.hist + (size_t)t * S * N);
#endif
#ifdef WSMC_SSM_BWREC
                if (row) ss_record_lw(L, rc.lwlog + (size_t)t * N);
#endif
                if (row && (a.tr_mean || a.tr_var))
                    ss_trace_row(L, a.tr_mean ? a.tr_mean + (size_t)t * S : nullptr, a.tr_var ? a.tr_var + (size_t)t * S : nullptr);
                const SsDecision d = ss_resample<TR>(L, K, a.ess_min, a.scheme, a.seed, op);
#ifdef WSMC_SSM_SMOOTH
                if (!init) {
                    if (d.resampled) ss_record_anc(L, rc.alog + (size_t)slot * N, rc.ran + slot);
                    slot += 1;
                }
#endif
                if (row && a.tr_logev && tid == 0) a.tr_logev[t] = d.logev;
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

template <unsigned FEAT, int THREADS>
static hipError_t ssm_launch(hipStream_t s, const SsKernArgs& a, int threads, size_t lds) {
    if (const hipError_t e = ss_ask_lds(WSMC_SSM_KERNEL<FEAT, THREADS, kSsTraced>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((WSMC_SSM_KERNEL<FEAT, THREADS, kSsTraced>), dim3(1), dim3(threads), lds, s, a);
    return hipGetLastError();
}
// this unit's three feature variants (launch_ssm_segment has checked the arguments)
hipError_t WSMC_SSM_VARIANTS(hipStream_t s, const SsKernArgs& a, unsigned feat, int threads, size_t lds) {
    if (feat & WSMC_FEAT_GAM) return ssm_launch<kSsFeatGam, kSsVariantGamThreads>(s, a, threads, lds);
    if (feat & WSMC_FEAT_EXT) return ssm_launch<kSsFeatExt, kSsMaxThreads>(s, a, threads, lds);
    return ssm_launch<0u, kSsMaxThreads>(s, a, threads, lds);
}

#if !defined(WSMC_SSM_TRACED) && !defined(WSMC_SSM_SMOOTH) && !defined(WSMC_SSM_GUIDED) && !defined(WSMC_SSM_BWREC)
int ssm_threads(unsigned feat, int n) {
    const int cap = (feat & WSMC_FEAT_GAM) ? kSsGamThreads : kSsMaxThreads;
    // two particles a thread where the workgroup allows (wsmc_lgssm1d_run's measured choice)
    return std::max(64, std::min(cap, ((n + 127) / 128) * 64));
}
int ssm_guided_threads(unsigned feat, int n) {
    const int cap = (feat & WSMC_FEAT_GAM) ? kSsGuidedGamThreads : kSsMaxThreads;
    return std::max(64, std::min(cap, ((n + 127) / 128) * 64));
}

hipError_t ssm_launch_traced(hipStream_t s, const SsmArgs& a, unsigned feat, int threads, size_t lds);   // csrc/wsmc_ssm_traced.hip

hipError_t ssm_launch_rec(hipStream_t s, const SsmRecArgs& a, unsigned feat, int threads, size_t lds);   // csrc/wsmc_ssm_smooth.hip

hipError_t launch_ssm_segment(hipStream_t s, const SsmArgs& a, unsigned feat, int threads) {
    if (!ss_segment_ok(a, feat, threads)) return hipErrorInvalidValue;
    const size_t lds = ssm_lds_bytes(a.N, a.S);
    if (a.tr_mean || a.tr_var || a.tr_logev) return ssm_launch_traced(s, a, feat, threads, lds);
    return ssm_launch_untraced(s, a, feat, threads, lds);
}

hipError_t launch_ssm_segment_rec(hipStream_t s, const SsmRecArgs& a, unsigned feat, int threads) {
    if (!ss_segment_ok(a.a, feat, threads) || !a.r.hist || !a.r.alog || !a.r.ran || a.r.n_slots < 1 ||
        a.a.t0 + a.a.nsteps > a.r.T)
        return hipErrorInvalidValue;
    return ssm_launch_rec(s, a, feat, threads, ssm_lds_bytes(a.a.N, a.a.S));
}

hipError_t ssm_launch_guided(hipStream_t s, const SsmGuidedArgs& a, unsigned feat, int threads, size_t lds);       // csrc/wsmc_ssm_guided.hip
hipError_t ssm_launch_guided_rec(hipStream_t s, const SsmGuidedArgs& a, unsigned feat, int threads, size_t lds);   // csrc/wsmc_ssm_guided_smooth.hip

hipError_t launch_ssm_guided_segment(hipStream_t s, const SsmGuidedArgs& a, unsigned feat, int threads, bool rec) {
    const SsmArgs& ra = a.ra.a;
    const SsmRec& r = a.ra.r;
    if (!ss_segment_ok(ra, feat, threads, true) || !a.targ) return hipErrorInvalidValue;
    if (rec && (!r.hist || !r.alog || !r.ran || r.n_slots < 1 || r.trace_slot < 0 || r.trace_slot >= r.n_slots ||
                ra.t0 + ra.nsteps > r.T))
        return hipErrorInvalidValue;
    const size_t lds = ssm_lds_bytes(ra.N, ra.S);
    return rec ? ssm_launch_guided_rec(s, a, feat, threads, lds) : ssm_launch_guided(s, a, feat, threads, lds);
}

hipError_t ssm_launch_bwrec(hipStream_t s, const SsmBwRecArgs& a, unsigned feat, int threads, size_t lds);             // csrc/wsmc_ssm_backward_rec.hip
hipError_t ssm_launch_guided_bwrec(hipStream_t s, const SsmGuidedBwArgs& a, unsigned feat, int threads, size_t lds);   // csrc/wsmc_ssm_guided_backward_rec.hip

hipError_t launch_ssm_segment_bwrec(hipStream_t s, const SsmBwRecArgs& a, unsigned feat, int threads) {
    if (!ss_segment_ok(a.a, feat, threads) || !a.r.hist || !a.r.lwlog || a.a.t0 + a.a.nsteps > a.r.T) return hipErrorInvalidValue;
    return ssm_launch_bwrec(s, a, feat, threads, ssm_lds_bytes(a.a.N, a.a.S));
}

hipError_t launch_ssm_guided_segment_bwrec(hipStream_t s, const SsmGuidedBwArgs& a, unsigned feat, int threads) {
    const SsmArgs& ra = a.ra.a;
    if (!ss_segment_ok(ra, feat, threads, true) || !a.targ || !a.ra.r.hist || !a.ra.r.lwlog || ra.t0 + ra.nsteps > a.ra.r.T)
        return hipErrorInvalidValue;
    return ssm_launch_guided_bwrec(s, a, feat, threads, ssm_lds_bytes(ra.N, ra.S));
}
#endif

}  // namespace wsmc
