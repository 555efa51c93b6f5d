// wsmc_ssm_smooth.hip — a smoothed scalar-SSM run (wsmc_ssm_run_smoothed, wsmc_ssm_run_batch_smoothed;
// DESIGN.md §4): the recording instantiations of the fused kernel, k_ssm_segment_rec<.., true> in
// three feature variants from csrc/wsmc_ssm.hip's source, and the two kernels that turn what they
// logged into trajectories and smoothed moments after the run's last segment.
//
// The log (SsmRec): row t of `hist` holds the S columns at trace point t; slot (t, j) of `alog`
// holds the ancestors of step t's j-th Resample that can run (after an OBSERVE, a WEIGHT or an
// importance SAMPLE) where `ran` says it ran. The final particle i sits at index i; going back, a
// Resample that ran sends index idx to anc[idx]. Trace point t lies before the Resample of slot
// (t, trace_slot), the step's last OBSERVE's, and after those of slots (t, 0 .. trace_slot - 1) and
// of step t - 1; in a spec without WEIGHT and importance SAMPLE trace_slot is the step's last slot.
//
// Phase 1 (k_ssm_traceback) is sequential in t: one workgroup a filter walks the slots from the
// last to the first. The dependent chain idx -> anc[idx] would run at memory latency if it read the
// log in place, so the workgroup stages a chunk of rows in LDS (independent, coalesced loads, all in
// flight at once) and every thread walks its particles through the chunk at LDS latency. idx_t is
// written over slot (t, trace_slot), whose row has been staged by then.
// Phase 2 (k_ssm_smooth_rows) is parallel: one workgroup a (filter, step) gathers row t of the
// history through idx_t into LDS in the fused kernel's layout, writes it back in place (the
// paths) and calls ss_trace_row on it with the final log-weights: the canonical sums of
// wsmc_weighted_moments.
#define WSMC_SSM_SMOOTH 1
#include "wsmc_ssm.hip"

#include <cstdint>

namespace wsmc {

namespace {

constexpr int kTbThreads = 1024;
constexpr int kTbLdsWords = 15 * 1024;   // 60 KiB of int32: the particles' indices, the staged rows, their flags
constexpr int kTbMaxRows = 64;

// the rows a chunk stages for n particles (at least one: 2 n + 64 words fit at the largest cap)
__host__ __device__ inline int tb_rows(int n) {
    const int r = (kTbLdsWords - (int)ss_n4(n) - kTbMaxRows) / n;
    return r < 1 ? 1 : r > kTbMaxRows ? kTbMaxRows : r;
}

}  // namespace

__global__ __launch_bounds__(kTbThreads) void k_ssm_traceback(SsmRec r, int N) {
    extern __shared__ __attribute__((aligned(16))) int32_t tb_smem[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const size_t b = blockIdx.x;
    const int n_slots = r.n_slots, trace_slot = r.trace_slot, M = r.T * n_slots, R = tb_rows(N);
    int32_t* alog = r.alog + b * (size_t)M * (size_t)N;
    const int32_t* ran = r.ran + b * (size_t)M;
    int32_t* cur = tb_smem;                      // [N] where each final particle's ancestor sits
    int32_t* flag = tb_smem + ss_n4(N);          // [R] the chunk's flags
    int32_t* rows = flag + kTbMaxRows;           // [R][N] the chunk's rows (those that ran)
    for (int i = tid; i < N; i += nthr) cur[i] = i;
    for (int hi = M; hi > 0; hi -= R) {
        const int lo = hi > R ? hi - R : 0, cnt = hi - lo;
        // the chunk's flags first (one load each, side by side), so that no row's loads wait for a
        // flag's: a row that did not run holds nothing and is not read
        if (tid < cnt) flag[tid] = ran[lo + tid];
        __syncthreads();
        for (int q = 0; q < cnt; ++q)
            if (flag[q]) {
                const int32_t* src = alog + (size_t)(lo + q) * N;
                for (int i = tid; i < N; i += nthr) rows[q * N + i] = src[i];
            }
        __syncthreads();
        for (int i = tid; i < N; i += nthr) {
            int idx = cur[i];
            for (int q = cnt - 1; q >= 0; --q) {
                if (flag[q]) idx = rows[q * N + idx];
                const int slot = lo + q;
                if (slot % n_slots == trace_slot) alog[(size_t)slot * N + i] = idx;   // idx_t
            }
            cur[i] = idx;
        }
        __syncthreads();   // the chunk is read before the next one is staged over it
    }
}

struct SsmRowsArgs {
    SsmRec r;
    const double* w;      // [B][N] the final log-weights
    double* mean;         // [B][T][S] or null
    double* var;          // [B][T][S] or null
    int32_t N, P, S, paths;
};

__global__ __launch_bounds__(kSsMaxThreads) void k_ssm_smooth_rows(SsmRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sr_smem[];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int N = a.N, P = a.P, S = a.S;
    const size_t bt = blockIdx.x, b = bt / (size_t)a.r.T;   // row (b, t) of the batch
    SsState L;
    L.stride = (int)ss_n8(N);
    L.cb = reinterpret_cast<double*>(sr_smem);
    L.lw = L.cb + (size_t)(S + 1) * L.stride;
    L.anc = nullptr;   // (no Resample here)
    L.red = reinterpret_cast<uint64_t*>(L.lw + L.stride);
    L.S = S;
    L.off = 0;
    L.N = N;
    L.i0 = tid * P < N ? tid * P : N;
    L.i1 = L.i0 + P < N ? L.i0 + P : N;
    L.lane = tid & 63;
    L.wave = tid >> 6;
    L.nw = (nthr + 63) >> 6;
#ifdef WSMC_TABLES_LDS
    wsmc_tables_to_lds();   // before any exp (every thread: it ends in a barrier)
#endif
    const int32_t* idx = a.r.alog + (bt * a.r.n_slots + (size_t)a.r.trace_slot) * N;
    double* hist = a.r.hist + bt * (size_t)S * N;
    const double* w = a.w + b * (size_t)N;
    for (int i = L.i0; i < L.i1; ++i) L.lw[i] = w[i];
    for (int k = 0; k < S; ++k) {
        const double* src = hist + (size_t)k * N;
        double* dst = L.cb + (size_t)k * L.stride;
        for (int i = L.i0; i < L.i1; ++i) dst[i] = src[idx[i]];
    }
    if (a.paths) {
        __syncthreads();   // every read of the row is through before it is written in place
        for (int k = 0; k < S; ++k) {
            double* dst = hist + (size_t)k * N;
            const double* src = L.cb + (size_t)k * L.stride;
            for (int i = L.i0; i < L.i1; ++i) dst[i] = src[i];
        }
    }
    if (a.mean || a.var) ss_trace_row(L, a.mean ? a.mean + bt * S : nullptr, a.var ? a.var + bt * S : nullptr);
}

hipError_t launch_ssm_traceback(hipStream_t s, const SsmRec& r, int N, int B) {
    if (!r.alog || !r.ran || r.n_slots < 1 || r.trace_slot < 0 || r.trace_slot >= r.n_slots || r.T < 1 || N < 1 || N > kLgCap || B < 1) return hipErrorInvalidValue;
    const size_t lds = (ss_n4(N) + kTbMaxRows + (size_t)tb_rows(N) * N) * sizeof(int32_t);
    if (lds > 65536) return hipErrorInvalidValue;
    const int threads = std::max(64, std::min(kTbThreads, ((N + 63) / 64) * 64));
    hipLaunchKernelGGL(k_ssm_traceback, dim3((unsigned)B), dim3(threads), lds, s, r, N);
    return hipGetLastError();
}

hipError_t launch_ssm_smooth_rows(hipStream_t s, const SsmRec& r, const double* w, double* mean, double* var, bool paths,
                                  int N, int S, int B, int threads) {
    if (!r.hist || !r.alog || r.n_slots < 1 || r.trace_slot < 0 || r.trace_slot >= r.n_slots || r.T < 1 || !w || S < 1 || S > WSMC_SSM_MAX_COLS || N < 1 || N > ssm_cap(S) ||
        B < 1 || (int64_t)B * r.T > INT32_MAX || threads < 64 || threads > kSsMaxThreads || (threads & 63))
        return hipErrorInvalidValue;
    // the fused kernel's layout without the ancestors: S + 1 column buffers, the log-weights, the scratch
    const size_t lds = ((size_t)S + 2) * ss_n8(N) * sizeof(double) + kSsScratch * sizeof(uint64_t);
    if (lds + 4096 > 160 * 1024) return hipErrorInvalidValue;
    if (const hipError_t e = ss_ask_lds(k_ssm_smooth_rows, lds); e != hipSuccess) return e;
    SsmRowsArgs a;
    a.r = r;
    a.w = w;
    a.mean = mean;
    a.var = var;
    a.N = N;
    a.P = (N + threads - 1) / threads;
    a.S = S;
    a.paths = paths ? 1 : 0;
    hipLaunchKernelGGL(k_ssm_smooth_rows, dim3((unsigned)((int64_t)B * r.T)), dim3(threads), lds, s, a);
    return hipGetLastError();
}

}  // namespace wsmc
