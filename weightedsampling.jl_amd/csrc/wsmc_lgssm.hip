// wsmc_lgssm.hip — the fused 1D linear-Gaussian SSM run for small populations (wsmc_lgssm1d_run):
// one persistent workgroup runs the steps of a segment in a loop on the device, the particles and
// their log-weights in LDS for the whole segment.
//
//   x ~ Normal(0, x0_std); for y in data: x ~ Normal(a*x, q); y => Normal(x, r); end
//   (benchmarks/ssm/WeightedSampling/lgssm1d.jl:18-24, + the auto-inserted Resamples)
//
// Every per-particle value is the statement path's: the same draws keyed by (seed, op, index),
// the same Normal log-density sequence, the integer weights against ceil(max), the exact sums,
// wsmc_global_ess / wsmc_shard_mean, and ancestors from wsmc_rank of each particle's CDF interval
// (the smallest m with C_m > x_n, as the oracle's merge). Integer sums are order-free, so the
// workgroup's reduction shape shows nowhere.
//
// Layout: thread t owns the P = ceil(N / threads) consecutive particles from t * P. The only
// synchronisation is __syncthreads; no workgroup waits on another. One workgroup is one CU: the
// step's time is the CU's instruction issue, so what is uniform over the block (the ESS, the
// decision, the log-mean) is computed by one wave and passed through LDS, and the log / exp
// tables are LDS copies (no global load inside a step but the next observation's, issued a step
// ahead).
#ifdef __HIP_DEVICE_COMPILE__
#define WSMC_TABLES_LDS   // include/wsmc_math.h: the device pass reads LDS copies of the tables
#endif
#include "wsmc_internal.h"

namespace wsmc {

namespace {

constexpr int kLgWaves = kLgThreads / 64;
constexpr int kLgScratch = 2 * kLgWaves * 4 + 8;   // u64 words: two reduction halves, the broadcast

__device__ inline uint64_t lg_shfl_xor(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t lg_shfl_up(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

// the dynamic LDS of one workgroup, carved for n particles (every offset a multiple of 16 B)
struct LgLds {
    double* xa;          // [n] the particles
    double* xb;          // [n] the CDF of q (u64) during a Resample, then the gathered particles
    double* lw;          // [n] log-weights
    int32_t* anc;        // [n] the last resampling step's ancestors
    uint64_t* red;       // [kLgScratch] reduction / scan scratch (two alternating halves), the broadcast
};
__device__ inline LgLds lg_carve(char* base, int n) {
    const size_t n8 = ((size_t)n + 1) & ~(size_t)1;   // doubles, 16-B multiples
    const size_t n4 = ((size_t)n + 3) & ~(size_t)3;
    LgLds l;
    l.xa = reinterpret_cast<double*>(base);
    l.xb = l.xa + n8;
    l.lw = l.xb + n8;
    l.anc = reinterpret_cast<int32_t*>(l.lw + n8);
    l.red = reinterpret_cast<uint64_t*>(l.anc + n4);
    return l;
}

}  // namespace

// the kernel's dynamic LDS for n particles (beside the 4 KiB of static log / exp tables)
size_t lgssm_lds_bytes(int n) {
    const size_t n8 = ((size_t)n + 1) & ~(size_t)1;
    const size_t n4 = ((size_t)n + 3) & ~(size_t)3;
    return 3 * n8 * sizeof(double) + n4 * sizeof(int32_t) + kLgScratch * sizeof(uint64_t);
}

__global__ __launch_bounds__(kLgThreads) void k_lgssm_segment(const LgArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lg_smem[];
    const LgLds L = lg_carve(lg_smem, a.N);
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = (nthr + 63) >> 6;
    const int N = a.N, P = a.P;
    const int i0 = tid * P < N ? tid * P : N, i1 = i0 + P < N ? i0 + P : N;   // this thread's particles
    double* x = L.xa;
    double* xo = L.xb;
    uint64_t* red0 = L.red;
    uint64_t* red1 = L.red + kLgWaves * 4;
    uint64_t* bc = L.red + 2 * kLgWaves * 4;   // wave 0's results: ESS bits, decision, sum q, log-mean bits

#ifdef WSMC_TABLES_LDS
    wsmc_tables_to_lds();   // before any log / exp (every thread: it ends in a barrier)
#endif
    for (int i = i0; i < i1; ++i) L.lw[i] = a.w[i];
    if (a.first) {   // x ~ Normal(0, x0_std): op_base (its Resample, a no-op, takes op_base + 1)
        for (int i = i0; i < i1; ++i) {
            double z0, z1;
            wsmc_normal_pair(wsmc_rng_block(a.seed, a.op_base, (uint64_t)i, 0), &z0, &z1);
            const double mu = 0.0;
            x[i] = mu + a.x0_std * z0;
        }
    } else {
        for (int i = i0; i < i1; ++i) x[i] = a.x[i];
    }

    const int K = wsmc_qbits((uint64_t)N);
    long long nres = 0;
    int last_dec = 0;
    double last_ess = 0.0;
    double y_next = a.nsteps > 0 ? a.data[a.t0] : 0.0;

    for (int s = 0; s < a.nsteps; ++s) {
        const int t = a.t0 + s;
        const uint64_t op = a.op_base + 2 + 3 * (uint64_t)t;   // Sample op; op + 1 a no-op Resample; op + 2 the Resample
        const double y = y_next;
        if (s + 1 < a.nsteps) y_next = a.data[t + 1];   // in flight during this step
        // x ~ Normal(a x, q); y => Normal(x, r); the block max of the log-weights
        uint64_t menc = WSMC_ORD_NEG_INF;
        for (int i = i0; i < i1; ++i) {
            double z0, z1;
            wsmc_normal_pair(wsmc_rng_block(a.seed, op, (uint64_t)i, 0), &z0, &z1);
            double mu = 0.0;
            mu = mu + a.a * x[i];
            const double xn = mu + a.q * z0;
            x[i] = xn;
            double mo = 0.0;
            mo = mo + 1.0 * xn;
            const double lw = L.lw[i] + wsmc_normal_lh((y - mo) * a.rh, a.c);
            L.lw[i] = lw;
            const uint64_t e = wsmc_ord_enc(lw);
            menc = e > menc ? e : menc;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t o = lg_shfl_xor(menc, m);
            menc = o > menc ? o : menc;
        }
        if (lane == 0) red0[wave] = menc;
        __syncthreads();
        for (int w = 0; w < nw; ++w) menc = red0[w] > menc ? red0[w] : menc;
        const double M = wsmc_ord_dec(menc);   // NaN if any NaN (the canonical NaN is the largest code)
        const double R = wsmc_qref(M);

        // the exact sums: q and q2 in u64; wf, wf2 < 2^42 each, N < 2^13: u64 too
        uint64_t sQ = 0, sQ2 = 0, sWf = 0, sWf2 = 0;
        uint64_t* cdf = reinterpret_cast<uint64_t*>(xo);
        for (int i = i0; i < i1; ++i) {
            const wsmc_qparts p = wsmc_qparts_of(L.lw[i], R, K);
            cdf[i] = p.q;
            sQ += p.q; sQ2 += p.q2; sWf += p.wf; sWf2 += p.wf2;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            sQ += lg_shfl_xor(sQ, m);
            sQ2 += lg_shfl_xor(sQ2, m);
            sWf += lg_shfl_xor(sWf, m);
            sWf2 += lg_shfl_xor(sWf2, m);
        }
        if (lane == 0) {
            red1[wave * 4 + 0] = sQ; red1[wave * 4 + 1] = sQ2; red1[wave * 4 + 2] = sWf; red1[wave * 4 + 3] = sWf2;
        }
        __syncthreads();
        // the decision, once for the block: the ESS on the first wave while the last one takes
        // the log-mean a resampling step resets to (two serial chains side by side; the other
        // waves wait at the barrier)
        if (wave == 0 || wave == nw - 1) {
            wsmc_shard_stats st;
            st.M = M; st.Q = 0; st.Q2 = 0; st.Wf = 0; st.Wf2 = 0; st.n = (uint64_t)N;
            for (int w = 0; w < nw; ++w) {
                st.Q += red1[w * 4 + 0]; st.Q2 += red1[w * 4 + 1];
                st.Wf += red1[w * 4 + 2]; st.Wf2 += red1[w * 4 + 3];
            }
            if (wave == 0) {
                const double ess = wsmc_global_ess(&st, 1);
                const bool go = ess < a.ess_min && st.Q > 0;   // strict; all -inf weights (Q = 0, ESS NaN) never resample
                if (lane == 0) {
                    bc[0] = wsmc_d2bits(ess);
                    bc[1] = go ? 1u : 0u;
                    bc[2] = st.Q;
                    if (a.ess_trace) a.ess_trace[t] = ess;
                }
            }
            if (wave == nw - 1 && st.Q > 0) {   // (one wave: it does both in turn)
                const double mean = wsmc_shard_mean(&st);
                if (lane == 0) bc[3] = wsmc_d2bits(mean);
            }
        }
        __syncthreads();
        last_ess = wsmc_bits2d(bc[0]);
        const bool rs = bc[1] != 0;
        last_dec = rs ? 1 : 0;
        if (!rs) continue;   // uniform over the block
        nres += 1;
        const uint64_t Q = bc[2];
        const double mean = wsmc_bits2d(bc[3]);

        // inclusive scan of q (in place): thread-local, then across the wave, then across waves
        uint64_t run = 0;
        for (int i = i0; i < i1; ++i) { run += cdf[i]; cdf[i] = run; }
        uint64_t incl = run;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = lg_shfl_up(incl, d);
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
            const uint64_t rk = wsmc_rank_r(C, Q, (uint64_t)N, ratio, a.scheme, a.seed, op + 2, 0);
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
        if (lane == 63) red1[wave] = (uint64_t)(uint32_t)imax;   // (red1's readers: wave 0, two barriers back)
        int before = __shfl_up(imax, 1, 64);
        if (lane == 0) before = 0;
        __syncthreads();
        for (int w = 0; w < wave; ++w) {
            const int o = (int)(uint32_t)red1[w];
            before = o > before ? o : before;
        }
        // ... and in the same pass the gather through LDS (the ranks in the CDF buffer were last
        // read before the marks' barrier: the buffer takes the new particles, each written by its
        // owner) and the weight reset. The old buffer is next written as the next step's CDF,
        // behind that step's first barrier.
        double* xn = reinterpret_cast<double*>(cdf);
        for (int i = i0; i < i1; ++i) {
            const int v = L.anc[i];
            before = v > before ? v : before;
            L.anc[i] = before;
            xn[i] = x[before];
            L.lw[i] = mean;
        }
        xo = x;
        x = xn;
    }

    for (int i = i0; i < i1; ++i) {
        a.x[i] = x[i];
        a.w[i] = L.lw[i];
    }
    if (nres > 0)
        for (int i = i0; i < i1; ++i) a.anc[i] = L.anc[i];
    if (tid == 0 && a.nsteps > 0) {
        a.rec->nres += nres;
        a.rec->last_dec = last_dec;
        a.rec->last_ess = last_ess;
    }
}

hipError_t launch_lgssm_segment(hipStream_t s, const LgArgs& a, int threads) {
    if (a.N < 1 || a.N > kLgCap || threads < 64 || threads > kLgThreads || (threads & 63) ||
        (int64_t)a.P * threads < a.N || a.nsteps < 0 || a.t0 < 0)
        return hipErrorInvalidValue;
    const size_t lds = lgssm_lds_bytes(a.N);
    if (lds > 65536 - 4096) {   // past 64 KiB a kernel must ask for its dynamic LDS (per device: set at each launch)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lgssm_segment),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lgssm_lds_bytes(kLgCap));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_lgssm_segment, dim3(1), dim3(threads), lds, s, a);
    return hipGetLastError();
}

}  // namespace wsmc
