/*
 * wsmc.h — C ABI of the MI355X-native SMC inner loop for WeightedSampling.jl.
 *
 * This library replaces the per-particle hot path that sits behind the reference's
 * store / state / operator interface. Each entry point names the reference interface it
 * stands in for (paths relative to the reference repository root):
 *
 *   store      AbstractParticleStore            src/stores.jl:1-35, ColumnStore :70-128
 *   state      SMCState weights / flags         src/types.jl:48-65
 *   operators  apply!(Assign|Sample|Observe|Weight|Resample|Move, state)
 *                                               src/transformers.jl:28, 172, 228, 283, 474, 588
 *   numerics   exp_norm / ess_perc / logsumexp / stratified_resample / icdf
 *                                               src/resampling.jl:13-77
 *   proposals  RW / autoRW                      src/move_kernels.jl:189-253
 *   kernels    default_kernels Normal / MvNormal / Uniform, the example HalfNormal
 *                                               src/default_kernels.jl:83-102,
 *                                               examples/damped_oscillator.jl:24-28
 *   score fold score_logpdf! / score!          src/types.jl:198-206, src/transformers.jl:193-302
 *
 * Conventions
 *   - All functions return WSMC_OK (0) or a nonzero wsmc_status; wsmc_last_error()
 *     returns a thread-local message for the last failure.
 *   - A context owns every device buffer of one particle shard on one GPU. Host pointers
 *     are borrowed for the duration of a call. Downloads synchronise; everything else is
 *     enqueued on the context's stream.
 *   - Columns are particle-major SoA f64: a column of dimension d is d contiguous arrays
 *     of N doubles (component-major), so component k of particle i is data[k*N + i].
 *   - Particle, slot and column indices are 0-based (the reference is 1-based).
 *   - One context per host thread (the reference is single-threaded, src/types.jl:24-26).
 *   - No host pointers to device memory escape except through wsmc_col_device_ptr.
 */
#ifndef WSMC_H
#define WSMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    WSMC_OK = 0,
    WSMC_EARG = 1,     /* invalid argument (reference: ArgumentError, src/move_kernels.jl:26) */
    WSMC_EHIP = 2,     /* HIP runtime failure */
    WSMC_ENOTPD = 3,   /* proposal covariance not positive definite (reference: PosDefException) */
    WSMC_ERCCL = 4,    /* RCCL failure */
    WSMC_ESTATE = 5,   /* operation invalid in the current state */
    WSMC_ENOMEM = 6
} wsmc_status;

typedef struct wsmc_ctx wsmc_ctx;

/* ---- argument forms -------------------------------------------------------
 * The reference passes opaque Julia closures (argfn). The device path accepts the
 * argument shapes @model's `vectorize` produces for the supported kernels: constants
 * (Ref), columns, and affine combinations of up to two column components.
 *   value(i) = c0 + coef[0]*col[0][comp[0]][i] + coef[1]*col[1][comp[1]][i]
 * Unused slots have col = -1.                                                  */
typedef struct {
    double  c0;
    int32_t col[2];
    int32_t comp[2];
    double  coef[2];
} wsmc_operand;

typedef enum {
    WSMC_FAM_NORMAL = 0,        /* Normal(mu, sigma), sigma a std               */
    WSMC_FAM_HALFNORMAL = 1,    /* Truncated(Normal(0, sigma), 0, Inf)          */
    WSMC_FAM_UNIFORM = 2,       /* Uniform(a, b) = param[0], param[1]           */
    WSMC_FAM_MVNORMAL_ISO = 3,  /* MvNormal(mu, var*I), dim <= 4                */
    WSMC_FAM_MVNORMAL = 4,      /* MvNormal(mu, Sigma), constant covariance Sigma, dim <= 3:
                                   build it with wsmc_dist_mvnormal_cov (the factor is
                                   packed into the dist, see wsmc_terms.h)       */
    /* scalar families of src/default_kernels.jl:83-102 with closed-form draws (one uniform
       word pair each) and Distributions.jl's logpdf formulas; location mu[0], scale `scale`: */
    WSMC_FAM_BERNOULLI = 5,     /* Bernoulli(p = mu[0]): x in {0.0, 1.0}            */
    WSMC_FAM_BERNOULLI_LOGIT = 6, /* BernoulliLogit(logitp = mu[0])                   */
    WSMC_FAM_EXPONENTIAL = 7,   /* Exponential(theta = scale), theta the mean       */
    WSMC_FAM_LOGNORMAL = 8,     /* LogNormal(mu, sigma)                             */
    WSMC_FAM_LAPLACE = 9,       /* Laplace(mu, theta)                               */
    WSMC_FAM_CAUCHY = 10,       /* Cauchy(mu, sigma)                                */
    WSMC_FAM_LOGISTIC = 11,     /* Logistic(mu, theta)                              */
    WSMC_FAM_GUMBEL = 12,       /* Gumbel(mu, theta)                                */
    WSMC_FAM_RAYLEIGH = 13,     /* Rayleigh(sigma = scale)                          */
    WSMC_FAM_GEOMETRIC = 14,    /* Geometric(p = mu[0]): failures before the first success */
    /* 15 is reserved: it stays an unknown family (WSMC_EARG). */
    /* the families of src/default_kernels.jl:83-102 built on log Gamma (wsmc_lgamma) and
       bounded rejection samplers (wsmc_terms.h); first parameter mu[0], second `scale`: */
    WSMC_FAM_GAMMA = 16,        /* Gamma(alpha = mu[0], theta = scale), theta a scale        */
    WSMC_FAM_INVERSEGAMMA = 17, /* InverseGamma(alpha = mu[0], theta = scale), theta a scale */
    WSMC_FAM_CHISQ = 18,        /* Chisq(nu = mu[0])                                        */
    WSMC_FAM_BETA = 19,         /* Beta(alpha = mu[0], beta = scale)                        */
    WSMC_FAM_TDIST = 20,        /* TDist(nu = mu[0])                                        */
    WSMC_FAM_POISSON = 21,      /* Poisson(lambda = mu[0])                                  */
    WSMC_FAM_BINOMIAL = 22,     /* Binomial(n = mu[0], p = scale)                           */
    WSMC_FAM_NEGBINOMIAL = 23   /* NegativeBinomial(r = mu[0] > 0 real, p = scale): failures
                                   before the r-th success                                  */
} wsmc_family;

typedef enum {
    WSMC_MEAN_AFFINE = 0,       /* mean component k = mu[k]                      */
    WSMC_MEAN_OSCILLATOR = 1    /* mean = mu[0]*exp(-mu[2]*t)*cos(mu[1]*t+mu[3]), t = param[0]
                                   (examples/damped_oscillator.jl:11)            */
} wsmc_mean_fn;

typedef struct {
    int32_t family;
    int32_t mean_fn;
    int32_t dim;                /* 1 for scalar families */
    int32_t reserved;
    wsmc_operand mu[4];
    wsmc_operand scale;         /* sigma (NORMAL, HALFNORMAL) or variance (MVNORMAL_ISO) */
    double param[2];
} wsmc_dist;

/* MvNormal(mu, Sigma) with a constant covariance Sigma (src/default_kernels.jl:93; the
 * reference builds Distributions' MvNormal, whose PDMat factors Sigma once). On entry d->dim
 * (1..3) and d->mu[0..dim-1] are set; Sigma is dim x dim row-major. Sets family
 * WSMC_FAM_MVNORMAL and packs the Cholesky factor and log det Sigma into d. Host only (no
 * device call). WSMC_EARG: bad dim or Sigma not exactly symmetric (LinearAlgebra.cholesky's
 * ishermitian check); WSMC_ENOTPD: Sigma not positive definite (PosDefException). */
int wsmc_dist_mvnormal_cov(wsmc_dist* d, const double* cov);

typedef enum { WSMC_TERM_SAMPLE = 0, WSMC_TERM_OBSERVE = 1, WSMC_TERM_WEIGHT = 2 } wsmc_term_kind;

/* One entry of the score tape: the statement's log-density contribution as
 * score!(Sample|Observe|Weight) recomputes it (src/transformers.jl:193-199, 243-249, 297-302). */
typedef struct {
    wsmc_dist    dist;
    wsmc_operand x[4];          /* the scored value (Sample: the drawn column) */
    int32_t      kind;
    int32_t      depth;         /* execution depth of the statement (src/types.jl:162-177) */
} wsmc_term;

typedef enum {
    WSMC_RESAMPLE_STRATIFIED = 0,   /* the reference's stratified_resample (src/resampling.jl:35-43) */
    WSMC_RESAMPLE_SYSTEMATIC = 1,   /* one uniform for all strata (north-star addition) */
    WSMC_RESAMPLE_MULTINOMIAL = 2   /* independent draws (north-star addition) */
} wsmc_scheme;
typedef enum { WSMC_PROPOSAL_RW = 0, WSMC_PROPOSAL_AUTORW = 1 } wsmc_proposal;

typedef struct {
    int32_t resampled;          /* SMCState.resampled */
    int32_t weights_changed;    /* SMCState.weights_changed */
    int32_t depth;              /* SMCState.depth */
    int32_t n_terms;            /* score tape length */
    double  last_ess_perc;      /* last ESS/N computed by a Resample */
    uint64_t op_counter;        /* stochastic-statement counter (RNG stream position) */
    int64_t n_resamples;
} wsmc_state;

/* ---- context --------------------------------------------------------------- */
const char* wsmc_last_error(void);
int wsmc_version(int32_t* major, int32_t* minor);
int wsmc_device_count(int32_t* n);
/* SMCState(n_particles; rng) — src/types.jl:62-78. The seed keys the Philox streams. */
int wsmc_create(wsmc_ctx** out, int64_t n_particles, int32_t device, uint64_t seed);
int wsmc_destroy(wsmc_ctx* ctx);
/* SMCState over n_gpus devices in ONE handle ("multi-GPU inside one
 * context"): the population [0, n_particles) is split into n_gpus contiguous shards (ragged),
 * shard g on devices[g] (NULL: device g). transport WSMC_TRANSPORT_RCCL: one communicator per
 * device from ncclCommInitAll (distinct devices); WSMC_TRANSPORT_HOST: records exchanged in
 * host memory between the shards' threads (several shards may share a device). Every other
 * entry point accepts the handle: a call runs on every shard concurrently (one host thread per
 * shard, so each shard's collectives meet the others', as one process per GPU would) and host
 * buffers of n_particles are split / joined by shard. Island sharding by default
 * (wsmc_comm_set_shard_mode applies to every shard). Per-shard-only calls
 * (wsmc_col_device_ptr, wsmc_store_resample, wsmc_debug_kernel_bench) need n_gpus = 1. */
typedef enum { WSMC_TRANSPORT_RCCL = 0, WSMC_TRANSPORT_HOST = 1 } wsmc_transport;
int wsmc_create_multi(wsmc_ctx** out, int64_t n_particles, int32_t n_gpus, const int32_t* devices,
                      uint64_t seed, int32_t transport);
int wsmc_sync(wsmc_ctx* ctx);
int wsmc_nparticles(wsmc_ctx* ctx, int64_t* n);
int wsmc_get_state(wsmc_ctx* ctx, wsmc_state* out);
/* Test hooks used by the reference's own tests (test/move_test.jl:36-37 set state.depth). */
int wsmc_set_depth(wsmc_ctx* ctx, int32_t depth);
int wsmc_set_op_counter(wsmc_ctx* ctx, uint64_t op);

/* ---- multi-GPU shard (one process per GPU) ----------------------------------
 * A context may own the shard [global_offset, global_offset + N) of a global
 * population of global_n particles; RNG streams are keyed by the global index.
 * RCCL is initialised from a unique id distributed by the caller (rank 0 creates it). */
int wsmc_comm_unique_id(uint8_t out_id[128]);
int wsmc_comm_init(wsmc_ctx* ctx, const uint8_t id[128], int32_t world, int32_t rank,
                   int64_t global_offset, int64_t global_n);
/* The same sharding with a host-side exchange instead of RCCL: `exchange` receives this
 * shard's record (`words` u64) and must return every rank's record in rank order in `all`
 * (world * words), returning 0 on success. For hosts that carry their own transport (an
 * MPI binding, a test harness putting several shards on one device); the device path is
 * otherwise identical. */
typedef int (*wsmc_exchange_fn)(void* user, const uint64_t* mine, int32_t words, uint64_t* all);
int wsmc_comm_init_host(wsmc_ctx* ctx, wsmc_exchange_fn exchange, void* user, int32_t world, int32_t rank,
                        int64_t global_offset, int64_t global_n);
/* How a sharded Resample draws:
 *  WSMC_SHARD_ISLAND (default): one record all-gather per step; each shard resamples
 *    within itself and resets to its own log-mean (evidence-preserving). Not the
 *    single-GPU ancestors.
 *  WSMC_SHARD_EXACT: the reference's stratified/systematic Resample over the whole
 *    population — identical bits to one context holding every particle (ancestors as
 *    global indices, columns, weights, evidence): the global max is exchanged first,
 *    the records are summed as integers, each shard fills its contiguous window of
 *    global slots and the particles move to their owners (grouped send/recv).
 * Exact mode covers the statement operators and wsmc_ssm2d_run (history traced back
 * across ranks); multinomial draws on exact shards return WSMC_EARG. */
typedef enum { WSMC_SHARD_ISLAND = 0, WSMC_SHARD_EXACT = 1 } wsmc_shard_mode;
int wsmc_comm_set_shard_mode(wsmc_ctx* ctx, int32_t mode);
/* A watchdog on every wait for the context's stream (each shard's, on a multi-device handle)
 * while it holds an RCCL communicator: a wait longer than `seconds` (a collective whose peer
 * never arrives) aborts the communicator (ncclCommAbort) and the call returns WSMC_ERCCL, so a
 * lost rank ends the job instead of hanging the node. 0 (the default) waits without bound. */
int wsmc_comm_set_timeout(wsmc_ctx* ctx, double seconds);
/* What a context (or a multi-device handle) is sharded over, as the communicator itself
 * reports it — for a benchmark line that must say how many devices it measured (no reference
 * counterpart: the reference is single-threaded, /root/reference/TODO.md:28).
 *   shards      shards in this handle (1 for a plain context, G for wsmc_create_multi)
 *   world/rank  the sharding (world 1: unsharded)
 *   rccl_ranks  ncclCommCount of the (first) shard's communicator, 0 when it has none
 *   transport   WSMC_TRANSPORT_RCCL, WSMC_TRANSPORT_HOST, or -1 (unsharded)
 *   shard_mode  WSMC_SHARD_ISLAND / WSMC_SHARD_EXACT
 *   devices[g], shard_n[g]  HIP device and particle count of shard g < min(shards, 8) */
typedef struct {
    int32_t shards, world, rank, rccl_ranks, transport, shard_mode;
    int32_t devices[8];
    int64_t shard_n[8];
} wsmc_comm_info_t;
int wsmc_comm_info(wsmc_ctx* ctx, wsmc_comm_info_t* out);

/* ---- store: AbstractParticleStore (src/stores.jl:1-35) ----------------------- */
/* broadcast_setcol! column creation (src/stores.jl:85-96); existing name => same id */
int wsmc_col_create(wsmc_ctx* ctx, const char* name, int32_t dim, int32_t* col_id);
/* hascol / lookup; *col_id = -1 when absent */
int wsmc_col_find(wsmc_ctx* ctx, const char* name, int32_t* col_id);
/* colnames (insertion order) */
int wsmc_col_count(wsmc_ctx* ctx, int32_t* n);
int wsmc_col_info(wsmc_ctx* ctx, int32_t col_id, char* name_buf, int32_t buf_len, int32_t* dim);
/* getcol (host copy, synchronising) */
int wsmc_col_download(wsmc_ctx* ctx, int32_t col_id, double* host);
/* broadcast_setcol!(store, name, identity, (v,)) with a host vector */
int wsmc_col_upload(wsmc_ctx* ctx, int32_t col_id, const double* host);
/* device pointer of the live buffer (valid until the next resample/gather) */
int wsmc_col_device_ptr(wsmc_ctx* ctx, int32_t col_id, double** dptr);
/* resample!(store, indices) with caller-supplied 0-based indices (src/stores.jl:105-128) */
int wsmc_store_resample(wsmc_ctx* ctx, const int32_t* host_indices);
/* Lazy genealogy of the store (the default; ColumnStore.resample! gathers every column at
 * every resample, src/stores.jl:105-128, which is O(T^2 N) over a run that keeps a history
 * column per step). A Resample logs its int32 ancestors and gathers only the columns an
 * operator touched since the previous Resample; the others are brought up to date, all in
 * one trace over the log, when a later operator or getcol reads one. Values are bit-identical
 * to the eager gathers (a gather is a copy). lazy = 0 restores the eager gathers (after
 * bringing every column up to date); exact shards are always eager.
 * wsmc_store_info: log entries held and columns currently behind the log. */
int wsmc_store_set_lazy(wsmc_ctx* ctx, int32_t lazy);
/* bring every column up to date now (one trace over the log; what a DataFrame(state) export
 * or a run's end needs), without a host copy */
int wsmc_store_materialize(wsmc_ctx* ctx);
int wsmc_store_info(wsmc_ctx* ctx, int64_t* log_entries, int32_t* stale_columns);

/* ---- weights: SMCState.weights (src/types.jl:48-60) ------------------------- */
int wsmc_weights_upload(wsmc_ctx* ctx, const double* host);
int wsmc_weights_download(wsmc_ctx* ctx, double* host);
/* logsumexp(weights) - log(N)  (src/utils.jl:21) */
int wsmc_log_evidence(wsmc_ctx* ctx, double* out);

/* ---- analysis reductions (src/utils.jl), no N-sized download -------------------------
 * Weighted moments under w = exp_norm(weights) of up to 4 expressions (operand form):
 * mean[k] = sum w_i v_k(i) / sum w_i           expectation / @E (src/utils.jl:11, 23-58)
 * cov[a*d+b] = sum w_i (v_a - mean_a)(v_b - mean_b) / sum w_i
 *                                             describe's std(..., corrected=false) (:233-240)
 * in the canonical reduction order of the autoRW moments; cov may be NULL. */
int wsmc_weighted_moments(wsmc_ctx* ctx, const wsmc_operand* exprs, int32_t d, double* mean, double* cov);
/* unweighted minimum / maximum of a column component (describe, src/utils.jl:238-239) */
int wsmc_col_minmax(wsmc_ctx* ctx, int32_t col_id, int32_t comp, double* min_out, double* max_out);
/* ess_perc(exp_norm(weights)) (src/resampling.jl:51-54) without resampling or any state change */
int wsmc_ess(wsmc_ctx* ctx, double* ess_perc);
/* describe()'s weighted median (StatsBase.quantile(v, Weights(w), 0.5)) and 8-bin sparkline
 * histogram levels (1..8, src/utils.jl:134-141) of one column component, on the integer
 * weights (include/wsmc_math.h). On shards both are population-wide: the median takes the
 * union of every rank's (value, q) pairs, the sparkline sums integer bins taken at the
 * population's max log-weight — the bits of one context holding every particle. */
int wsmc_weighted_median(wsmc_ctx* ctx, int32_t col_id, int32_t comp, double* out);
int wsmc_histogram(wsmc_ctx* ctx, int32_t col_id, int32_t comp, int32_t levels[8]);
/* sample(state, n; replace) (src/utils.jl:92-118): n particle indices (0-based) drawn by
 * the normalised weights — with replacement independent draws in draw order, without
 * replacement the n largest Efraimidis–Spirakis keys (include/wsmc_math.h wsmc_es_key).
 * Consumes one op counter (the reference draws from the global RNG). WSMC_EARG for n <= 0
 * or (!replace && n > N), as the reference's ArgumentError. On shards the indices are
 * global and the draws are the single-context draws (each target located by the rank whose
 * CDF range holds it; without replacement the union of the ranks' top-n keys). */
int wsmc_sample_particles(wsmc_ctx* ctx, int64_t n, int32_t replace, int64_t* idx_out);
/* rows idx[0..n) of a column, [dim][n] (getcol(store, c)[indices], src/utils.jl:117) */
int wsmc_col_gather_rows(wsmc_ctx* ctx, int32_t col_id, const int64_t* idx, int64_t n, double* out);

/* ---- operators (apply!) ------------------------------------------------------ */
/* Assign: out[k] .= expr[k] for k < dim(out)            src/transformers.jl:28-32 */
int wsmc_assign(wsmc_ctx* ctx, int32_t out_col, const wsmc_operand* expr);
/* Assign of a general expression: out[k] .= f_k(columns...) for k < dim(out).
 * The reference's `vectorize` (src/rewrites.jl:146-219) turns the right-hand side into one
 * fused broadcast over the columns: calls f.(args...), `cond ? a : b` as ifelse.(...),
 * `a || b` / `a && b` as .| / .&, `x[j]` component reads. The device form is one postfix
 * program per output component, the components' programs back to back in `prog`, len[k]
 * instructions for component k (k < dim(out)); at most WSMC_XPROG_MAX instructions in all and
 * WSMC_XSTACK_MAX values on the stack. Binary operators pop b (the top) then a and push
 * f(a, b); each component's program must leave exactly one value. The arithmetic is
 * wsmc_xop1 / wsmc_xop2 (include/wsmc_terms.h). Columns read one lazy Resample behind are
 * read through its ancestors (as wsmc_assign). WSMC_EARG: a malformed program, an unknown
 * column or component. Domain errors Julia throws (sqrt / log of a negative, a negative
 * base to a fractional power) give NaN. */
typedef enum {
    WSMC_X_CONST = 0,   /* push c                                                         */
    WSMC_X_COL = 1,     /* push column col, component comp                                */
    WSMC_X_NEG = 2, WSMC_X_ABS = 3, WSMC_X_SQRT = 4, WSMC_X_EXP = 5, WSMC_X_LOG = 6,
    WSMC_X_LOG1P = 7, WSMC_X_SIN = 8, WSMC_X_COS = 9,
    WSMC_X_POWI = 10,   /* a^n, n = c (an integer, |n| < 2^62): Base.literal_pow for
                           n in -2..3, else Base's compensated power by squaring       */
    WSMC_X_NOT = 11,    /* !a: 1 if a == 0 else 0                                        */
    WSMC_X_ADD = 16, WSMC_X_SUB = 17, WSMC_X_MUL = 18, WSMC_X_DIV = 19,
    WSMC_X_MIN = 20, WSMC_X_MAX = 21,   /* Base.min / max (NaN-propagating, -0.0 < 0.0)   */
    WSMC_X_POW = 22,    /* a^b: integer b as POWI, else exp(b * log(a))                   */
    WSMC_X_LT = 23, WSMC_X_LE = 24, WSMC_X_GT = 25, WSMC_X_GE = 26, WSMC_X_EQ = 27,
    WSMC_X_NE = 28,     /* comparisons: 1.0 / 0.0                                         */
    WSMC_X_AND = 29, WSMC_X_OR = 30,    /* (a != 0) & (b != 0), (a != 0) | (b != 0)       */
    WSMC_X_IFELSE = 31  /* pops f, t, cond: cond != 0 ? t : f (both evaluated)            */
} wsmc_xop;
typedef struct {
    int32_t op;         /* wsmc_xop */
    int32_t col;        /* WSMC_X_COL: the column */
    int32_t comp;       /* WSMC_X_COL: its component */
    int32_t reserved;
    double  c;          /* WSMC_X_CONST: the value; WSMC_X_POWI: the exponent */
} wsmc_xinst;
#define WSMC_XPROG_MAX 96
#define WSMC_XSTACK_MAX 8
int wsmc_assign_expr(wsmc_ctx* ctx, int32_t out_col, const wsmc_xinst* prog, const int32_t* len);
/* Sample: out ~ dist (weighter === nothing)            src/transformers.jl:172-182 */
int wsmc_sample(wsmc_ctx* ctx, int32_t out_col, const wsmc_dist* dist);
/* Sample with importance_kernel(proposal, target)      src/default_kernels.jl:69-73 */
int wsmc_sample_importance(wsmc_ctx* ctx, int32_t out_col, const wsmc_dist* proposal,
                           const wsmc_dist* target);
/* Observe: weights .+= logpdf(dist, x)                  src/transformers.jl:228-235 */
int wsmc_observe(wsmc_ctx* ctx, const wsmc_dist* dist, const wsmc_operand* x);
/* Weight (_ ~ f(args)): weights .+= logpdf(dist, x)     src/transformers.jl:283-289 */
int wsmc_weight(wsmc_ctx* ctx, const wsmc_dist* dist, const wsmc_operand* x);
/* Resample (gated on weights_changed, strict ESS test, log-mean reset)
 *                                                       src/transformers.jl:474-498
 *   resampled_out / ess_perc_out both NULL: asynchronous — the decision stays on the device
 *   (gated gather and weight reset, no host wait) and is folded into wsmc_get_state's
 *   resampled / n_resamples / last_ess_perc at the next read (exact shards always wait). */
int wsmc_resample(wsmc_ctx* ctx, double ess_perc_min, int32_t scheme,
                  int32_t* resampled_out, double* ess_perc_out);
/* Move with RW / autoRW (src/transformers.jl:588-623, src/move_kernels.jl:189-253).
 *   targets: d <= 4 scalar columns; lo/hi: per-target bounds (NULL = unbounded);
 *   step: RW step size (std) or autoRW min_step; target_depth: state.depth at the move
 *   (pass -1 to use the context's current depth); diversity: NaN = ungated.
 *   *accepted_out (may be NULL) receives the number of accepted proposals. With
 *   accepted_out NULL the Move is asynchronous (no host wait, as the reference's Move
 *   returns nothing): a not-positive-definite autoRW covariance leaves the Move's targets
 *   untouched and is reported as WSMC_ENOTPD by the next synchronizing call (wsmc_sync,
 *   get_state, a download, a waited Resample or Move). Operators enqueued in between have
 *   run (later asynchronous Moves skip on the same flag): nothing is rolled back, the state
 *   is the one those statements produce with the failed Moves left out, where the reference
 *   would have thrown at the failing Move. Callers that need the reference's stop-at-the-
 *   failure behaviour pass accepted_out.                                                  */
int wsmc_move(wsmc_ctx* ctx, int32_t proposal, const int32_t* targets, int32_t d, double step,
              const double* lo, const double* hi, int32_t target_depth, double diversity,
              int64_t* accepted_out);
/* Move.apply! inside `if resampled ... end` (the Cond of src/rewrites.jl:360-368;
 * examples/linear_regression.jl:23-24, examples/damped_oscillator.jl:38-41) with the condition
 * decided on the device: the Move runs only if the last Resample resampled, and the host never
 * reads the flag (an asynchronous Resample followed by gated Moves keeps the whole step on the
 * stream). Asynchronous like wsmc_move with accepted_out NULL. A gated Move consumes its two
 * op counters whether or not it runs, so its streams do not depend on the decision. With a
 * diversity gate or on shards the decision is read on the host first.                       */
int wsmc_move_gated(wsmc_ctx* ctx, int32_t proposal, const int32_t* targets, int32_t d, double step,
                    const double* lo, const double* hi, int32_t target_depth, double diversity);
/* One Move of a block (wsmc_move_block): wsmc_move's arguments without the diversity gate. */
typedef struct {
    int32_t proposal;        /* WSMC_PROPOSAL_RW / WSMC_PROPOSAL_AUTORW */
    int32_t d;               /* 1..4 targets */
    int32_t targets[4];
    int32_t bounded;         /* 0: lo / hi ignored (wsmc_move's NULL lo and hi) */
    int32_t target_depth;    /* < 0: the current depth */
    double step;             /* RW step / autoRW min_step */
    double lo[4], hi[4];
} wsmc_move_spec;
/* A statement block of consecutive Moves — `α << autoRW(); β << autoRW()` in the body of
 * `if resampled ... end` (examples/linear_regression.jl:23-24) or a sweep of
 * examples/damped_oscillator.jl:38-41 without its diversity gate: exactly n wsmc_move calls
 * in order (gated != 0: n wsmc_move_gated calls), the same results bit for bit, op counters
 * taken two per Move in order. Autorw Moves on disjoint targets (4 at most in all) with one
 * target depth run as one moments pass, one combine and one Move kernel; anything else runs
 * the Moves one by one. accepted_out: n counts (synchronizing, the ENOTPD check of the first
 * failing Move as wsmc_move's) or NULL (asynchronous).                                     */
int wsmc_move_block(wsmc_ctx* ctx, int32_t n, const wsmc_move_spec* specs, int32_t gated, int64_t* accepted_out);
/* score_logpdf!(scores, state, targets, target_depth) (src/types.jl:198-206) -> host */
int wsmc_score(wsmc_ctx* ctx, int32_t target_depth, double* host_scores);
/* marginal_diversity(store, targets)  (src/transformers.jl:560-565) */
int wsmc_marginal_diversity(wsmc_ctx* ctx, const int32_t* targets, int32_t d, double* out);
/* the last resample's ancestors (0-based; debug/parity; synchronising); a multi-device
 * handle returns population indices (island shards resample within their own range) */
int wsmc_last_ancestors(wsmc_ctx* ctx, int32_t* host);

/* ---- fused runners (whole model loops; one HIP graph per run) ------------------
 * 2D SSM bootstrap filter (examples/2D_ssm.jl:7-17) on a fresh context:
 *   x{1} .= x0; v .= v0; for t: x{t+1} .= x{t} + v; dv ~ MvNormal(0, q_var I);
 *   v .= v + dv; o_t => MvNormal(x{t+1}, r_var I)   (+ the auto-inserted Resamples)
 * Columns created: x_1 .. x_{T+1} (dim 2, when keep_history), x (dim 2, otherwise), v, dv.
 * Produces the same columns, weights and RNG stream positions as issuing the same
 * statements one by one through the operators above.
 * The fused kernels write these columns and no other. A context that holds any other column (an
 * earlier, longer run's x_{T+2} .., the other store mode's, the caller's own) gets the same
 * statements issued one by one through the operators above instead, whose Resamples gather
 * every column of the store (wsmc_debug_ssm2d_routes counts the two routes).             */
int wsmc_ssm2d_run(wsmc_ctx* ctx, const double* obs /* T x 2, row-major */, int32_t T,
                   const double* x0, const double* v0, double q_var, double r_var,
                   double ess_perc_min, int32_t scheme, int32_t keep_history,
                   double* log_evidence_out);
/* benchmarks/ssm/WeightedSampling/lgssm1d.jl:18-24 as one call:
 *   x ~ Normal(0, x0_std); for y in data: x ~ Normal(a*x, q); y => Normal(x, r); end
 * (+ the auto-inserted Resample after every ~ / =>). Produces the same column `x`, weights,
 * ancestors, state fields, score tape and RNG stream positions as issuing those statements one
 * by one (models.lgssm1d_statements). Synchronous: on return the run is complete and folded in.
 * One unsharded context of at most wsmc_debug_lgssm's cap particles, holding no column but a
 * dim-1 `x`, with a stratified or systematic scheme runs on one persistent workgroup (the
 * population in LDS, the steps looped on the device, a launch per segment of steps); everything
 * else issues the statements themselves inside the library.
 * ess_trace_out (may be NULL): T doubles, the ESS% each step's post-Observe Resample computed
 * (what a waited wsmc_resample returns in ess_perc_out; NaN kept).
 * WSMC_EARG: null data, T < 1, q <= 0, r <= 0, x0_std <= 0, an unknown scheme. */
int wsmc_lgssm1d_run(wsmc_ctx* ctx, const double* data, int32_t T, double a, double q, double r,
                     double x0_std, double ess_perc_min, int32_t scheme,
                     double* log_evidence_out, double* ess_trace_out);
/* segment_steps > 0 sets the steps per launch, 0 restores the default, < 0 leaves it; stats_out[6]
 * (may be NULL) = the largest N the persistent kernel takes, runs it took, runs that went through
 * the statement route, segments launched (cumulative per context), then the last run's host
 * bookkeeping time (tape and state, done while the device runs) and whole-call time, microseconds. */
int wsmc_debug_lgssm(wsmc_ctx* ctx, int32_t segment_steps, int64_t* stats_out);
/* ---- a scalar state-space model the caller specifies, as one call ----------------------
 * The step body wsmc_lgssm1d_run hard-codes, described instead: up to WSMC_SSM_MAX_COLS scalar
 * (dim-1) state columns, an `init` list run once at the start of the call and a `step` list run
 * for t = 0 .. T-1. Operands, dists and programs inside a spec name the spec's columns by their
 * local index 0 .. n_cols-1; the run creates the columns that are missing (in order) and maps
 * the indices to column ids.
 *   SAMPLE       col ~ dist                      (wsmc_sample)
 *   ASSIGN       col .= value                    (wsmc_assign)
 *   ASSIGN_EXPR  col .= prog[0 .. prog_len)      (wsmc_assign_expr: one postfix program of at
 *                                                 most WSMC_SSM_XPROG_MAX instructions)
 *   OBSERVE      value => dist                   (wsmc_observe)
 *   SAMPLE_IMPORTANCE  col ~ importance_kernel(dist, target)   (wsmc_sample_importance: `dist` is
 *                                                 the proposal; the weights gain
 *                                                 logpdf(target, x) - logpdf(dist, x), both dists'
 *                                                 operands read after x is stored, so one that
 *                                                 names `col` sees the new value)
 *   WEIGHT       _ ~ dist, scored at value       (wsmc_weight; OBSERVE's fields)
 * A Resample(ess_perc_min, scheme) follows every SAMPLE, OBSERVE, SAMPLE_IMPORTANCE and WEIGHT
 * (what @model inserts); it takes its op counter whether or not it runs, and runs only if the
 * weights changed. The trace point of a traced or smoothed run stays the step's last OBSERVE.
 * dists: dim 1, WSMC_MEAN_AFFINE, family NORMAL, HALFNORMAL, UNIFORM, 5 .. 14 or 16 .. 23.
 * Data: the call takes a row-major T x data_dim table (data_dim <= WSMC_SSM_MAX_DATA). In an
 * operand of `step` at most one slot k may have col[k] == WSMC_OPERAND_DATA with comp[k] = j <
 * data_dim: the operand's value at step t is that of the same operand with slot k removed and
 * c0 = data[t][j] (it must have c0 == 0 and coef[k] == 1, so the fold is exact: the constant
 * operand the statements get). In a program WSMC_X_COL with col == WSMC_OPERAND_DATA pushes
 * data[t][comp]. `init` reads no data; `step` holds at least one OBSERVE. */
#define WSMC_SSM_MAX_COLS 4
#define WSMC_SSM_MAX_INIT 4
#define WSMC_SSM_MAX_STMTS 8
#define WSMC_SSM_MAX_DATA 4
#define WSMC_SSM_XPROG_MAX 32
#define WSMC_SSM_NAME_MAX 32
#define WSMC_OPERAND_DATA (-2)
typedef enum {
    WSMC_SSM_SAMPLE = 0, WSMC_SSM_ASSIGN = 1, WSMC_SSM_ASSIGN_EXPR = 2, WSMC_SSM_OBSERVE = 3,
    WSMC_SSM_SAMPLE_IMPORTANCE = 4, WSMC_SSM_WEIGHT = 5
} wsmc_ssm_kind;
typedef struct {
    int32_t kind;               /* wsmc_ssm_kind */
    int32_t col;                /* SAMPLE, ASSIGN, ASSIGN_EXPR: the output column (local index) */
    int32_t prog_len;           /* ASSIGN_EXPR: instructions of prog */
    int32_t reserved;
    wsmc_dist dist;             /* SAMPLE, OBSERVE, WEIGHT; SAMPLE_IMPORTANCE: the proposal */
    wsmc_operand value;         /* ASSIGN: the right-hand side; OBSERVE, WEIGHT: the scored value */
    wsmc_xinst prog[WSMC_SSM_XPROG_MAX];
    wsmc_dist target;           /* SAMPLE_IMPORTANCE: the target (last, so every other offset holds) */
} wsmc_ssm_stmt;
typedef struct {
    int32_t n_cols;             /* 1 .. WSMC_SSM_MAX_COLS */
    int32_t data_dim;           /* 0 .. WSMC_SSM_MAX_DATA columns of the data table */
    int32_t n_init;             /* 0 .. WSMC_SSM_MAX_INIT */
    int32_t n_step;             /* 1 .. WSMC_SSM_MAX_STMTS */
    char col_names[WSMC_SSM_MAX_COLS][WSMC_SSM_NAME_MAX];   /* NUL-terminated, distinct */
    wsmc_ssm_stmt init[WSMC_SSM_MAX_INIT];
    wsmc_ssm_stmt step[WSMC_SSM_MAX_STMTS];
} wsmc_ssm_spec;
/* The rules above, on the host alone (no device call, no context): WSMC_OK, or WSMC_EARG with
 * the reason in wsmc_last_error(). */
int wsmc_ssm_spec_check(const wsmc_ssm_spec* spec);
/* sizeof(wsmc_ssm_stmt) and sizeof(wsmc_ssm_spec) as the library was built (layout checks) */
int wsmc_ssm_spec_sizeof(int64_t* stmt_bytes, int64_t* spec_bytes);
/* Runs the spec: on return the columns, weights, ancestors, every wsmc_state field, the score
 * tape, the evidence and the RNG stream positions are, bit for bit, those of issuing the spec's
 * statements (and their Resamples) one by one through the operators above, with the step's data
 * folded into constants. Synchronous: on return the run is complete and folded in.
 * One unsharded context that holds no column but the spec's (dim 1), with at most
 * wsmc_debug_ssm's cap particles for the spec's column count, weights_changed clear, a
 * stratified or systematic scheme and at most WSMC_XPROG_MAX program instructions in the whole
 * spec runs on one persistent workgroup (the columns in LDS, the steps looped on the device, a
 * launch per segment of steps); everything else issues the statements themselves inside the
 * library, which is also the definition of the results.
 * data: T x spec->data_dim, row-major (may be NULL when data_dim == 0).
 * ess_trace_out (may be NULL): T doubles, the ESS% computed by the Resample that follows each
 * step's last OBSERVE (NaN kept).
 * WSMC_EARG: a spec wsmc_ssm_spec_check refuses, T < 1, null data, an unknown scheme, a spec
 * column that exists with another dimension. */
int wsmc_ssm_run(wsmc_ctx* ctx, const wsmc_ssm_spec* spec, const double* data, int32_t T,
                 double ess_perc_min, int32_t scheme, double* log_evidence_out, double* ess_trace_out);
/* segment_steps > 0 sets the steps per launch, 0 restores the default, < 0 leaves it; stats_out[9]
 * (may be NULL) = the largest N the persistent kernel takes with 1, 2, 3, 4 columns, the runs it
 * took, the runs that went through the statement route, the segments launched (cumulative per
 * context), then the last run's host bookkeeping time (tape and state, done while the device
 * runs) and whole-call time, microseconds. */
int wsmc_debug_ssm(wsmc_ctx* ctx, int32_t segment_steps, int64_t* stats_out);
/* ---- many independent filters in one call ------------------------------------------------
 * The results of a batch: caller-owned host buffers, each may be NULL (not wanted). */
typedef struct {
    double*  log_evidence;      /* [B] */
    double*  ess_trace;         /* [B][T] the ESS% after each step's last OBSERVE (NaN kept) */
    double*  cols;              /* [B][n_cols][n] the final columns, in the spec's order */
    double*  log_weights;       /* [B][n] */
    int32_t* last_ancestors;    /* [B][n] row b: the last resampling step's ancestors if n_resamples[b] > 0,
                                   else zeros (wsmc_last_ancestors of a fresh context) */
    int64_t* n_resamples;       /* [B] */
    int32_t* last_resampled;    /* [B] the last Resample's decision */
} wsmc_ssm_batch_out;
/* B independent runs of wsmc_ssm_run in one call, one persistent workgroup per run, B workgroups
 * a launch. Filter b is, bit for bit, what wsmc_ssm_run(spec b, table b, T, ess_perc_min, scheme)
 * gives on a fresh wsmc_create(n, seeds[b]) context: final columns, log-weights, last ancestors,
 * log evidence, per-step ESS trace, number of resamples, the last decision.
 * specs: n_specs = 1 (one spec for every filter) or B; data: n_tables = 1 or B row-major tables of
 * T x data_dim, back to back (may be NULL when data_dim == 0). With n_specs == B the specs must be
 * of one shape (wsmc_ssm_spec_same_shape): only their numbers may differ.
 * ctx gives the device and the stream; its particles, columns, weights, tape, counters and RNG
 * position are neither read nor written, so the call may stand between any two statements of a
 * program on ctx. Synchronous: on return every filter is complete.
 * The call has the persistent route only. WSMC_EARG, with the reason in wsmc_last_error(): n above
 * the cap for the spec's column count (wsmc_debug_ssm), multinomial or unknown resampling, more than
 * WSMC_XPROG_MAX program instructions in the spec, a sharded or multi-device ctx, B < 1, T < 1,
 * n < 1, n_specs or n_tables not 1 or B, null specs / seeds / out, null data with data_dim > 0,
 * a spec wsmc_ssm_spec_check refuses ("spec b: ..."), specs of different shape. */
int wsmc_ssm_run_batch(wsmc_ctx* ctx, const wsmc_ssm_spec* specs, int32_t n_specs,
                       const double* data, int32_t n_tables, int32_t T, int32_t n, int32_t B,
                       const uint64_t* seeds, double ess_perc_min, int32_t scheme,
                       wsmc_ssm_batch_out* out);
/* Host only: WSMC_OK when a and b differ in their numbers alone (an operand's c0 / coef, a dist's
 * param, the value of a WSMC_X_CONST instruction); WSMC_EARG with the first differing field in
 * wsmc_last_error() when a count, a column name, a kind, a column, a family, a data reference or
 * an instruction's opcode (or a WSMC_X_POWI exponent) differs. */
int wsmc_ssm_spec_same_shape(const wsmc_ssm_spec* a, const wsmc_ssm_spec* b);
/* sizeof(wsmc_ssm_batch_out) as the library was built (layout check) */
int wsmc_ssm_batch_out_sizeof(int64_t* bytes);
/* segment_steps > 0 sets the steps per launch of wsmc_ssm_run_batch on this context, 0 restores the
 * default (wsmc_ssm_run's, divided by the rounds of resident workgroups B takes), < 0 leaves it;
 * stats_out[4] (may be NULL) = the last batch's resident workgroups per CU, the device's CU count,
 * the segments it launched and its whole-call time in microseconds. */
int wsmc_debug_ssm_batch(wsmc_ctx* ctx, int32_t segment_steps, int64_t* stats_out);
/* ---- the per-step filtering trace of the two runs above ------------------------------------
 * Trace point t (t = 0 .. T-1) is the ESS trace's: after step t's last OBSERVE, before the
 * Resample that follows it. Row t is what the operators return there when the statements are
 * issued one by one: mean[t][k] and var[t][k] are mean[k] and cov[k * d + k] of
 * wsmc_weighted_moments with d = n_cols and expression k = column k alone (c0 = 0, coef = 1), so
 * E[x_t | y_1:t] and the uncorrected variance under exp_norm of the weights; log_evidence[t] is
 * wsmc_log_evidence (cumulative: its first difference is log p(y_t | y_1:t-1)); ess[t] is the
 * ESS trace. Bit for bit, NaN kept. A function of the state is traced by making it a column.
 * Caller-owned host buffers, each may be NULL (not wanted). */
typedef struct {
    double* ess;                /* [T]          (batch: [B][T])         */
    double* mean;               /* [T][n_cols]  (batch: [B][T][n_cols]), the spec's column order */
    double* var;                /* [T][n_cols]  (batch: [B][T][n_cols]) */
    double* log_evidence;       /* [T]          (batch: [B][T])         */
} wsmc_ssm_trace;
/* sizeof(wsmc_ssm_trace) as the library was built (layout check) */
int wsmc_ssm_trace_sizeof(int64_t* bytes);
/* wsmc_ssm_run with the trace. Everything else the run leaves (columns, weights, ancestors, state
 * fields, tape, evidence, RNG positions, wsmc_debug_ssm's routes) is bit for bit the untraced
 * run's, and neither the route nor the particle caps depend on the trace. On the persistent
 * route the workgroup takes the moments from LDS in the canonical order of summation; on the
 * statement route the library calls wsmc_weighted_moments and wsmc_log_evidence at the trace
 * point, where the Resample waits as it does for the ESS trace. trace NULL, or every member NULL:
 * wsmc_ssm_run without an ESS trace. */
int wsmc_ssm_run_traced(wsmc_ctx* ctx, const wsmc_ssm_spec* spec, const double* data, int32_t T,
                        double ess_perc_min, int32_t scheme, double* log_evidence_out,
                        const wsmc_ssm_trace* trace);
/* wsmc_ssm_run_batch with the trace of every filter (row b of each array is filter b's, what
 * wsmc_ssm_run_traced gives on a fresh wsmc_create(n, seeds[b]) context); the same refusals. The
 * ESS trace goes to out->ess_trace and trace->ess, whichever is set. The trace is part of the
 * call's device allocation: 8 B T (2 n_cols + 2) bytes when all four are asked for. */
int wsmc_ssm_run_batch_traced(wsmc_ctx* ctx, const wsmc_ssm_spec* specs, int32_t n_specs,
                              const double* data, int32_t n_tables, int32_t T, int32_t n, int32_t B,
                              const uint64_t* seeds, double ess_perc_min, int32_t scheme,
                              wsmc_ssm_batch_out* out, const wsmc_ssm_trace* trace);
/* ---- sampled trajectories and smoothed moments from the two runs above -----------------------
 * The genealogy of the final particles, traced back through every resampling step of the run:
 * paths[t][k][i] is column k at trace point t (the filtering trace's: after step t's last OBSERVE,
 * before the Resample that follows it) of final particle i's ancestor; mean[t][k] and var[t][k]
 * are wsmc_weighted_moments of row t (d = n_cols, expression k = paths[t][k] alone) under the
 * final weights, so E[x_t | y_1:T] and the uncorrected variance of the genealogy's estimate. Bit
 * for bit what the statements issued one by one give when every column is copied at each trace
 * point into a column of its own, which the Resamples that follow gather like any other. A row
 * of paths picked by exp_norm of the final weights is a draw from the smoothing distribution.
 * Caller-owned host buffers, each may be NULL (not wanted). */
typedef struct {
    double* paths;              /* [T][n_cols][n]   (batch: [B][T][n_cols][n]) */
    double* mean;               /* [T][n_cols]      (batch: [B][T][n_cols])    */
    double* var;                /* [T][n_cols]      (batch: [B][T][n_cols])    */
} wsmc_ssm_smooth;
/* sizeof(wsmc_ssm_smooth) as the library was built (layout check) */
int wsmc_ssm_smooth_sizeof(int64_t* bytes);
/* wsmc_ssm_run_traced with the smoothed output. The persistent workgroup stores its columns at
 * every trace point and its ancestors after every Resample that ran to device memory; after the
 * last step one kernel follows every final particle's ancestors back through the log and a second
 * gathers the rows and takes their moments: O(T n) work, no host round trip per step. Everything
 * else the run leaves (columns, weights, ancestors, state fields, tape, evidence, RNG positions,
 * wsmc_debug_ssm's routes, the filtering trace if asked) is bit for bit wsmc_ssm_run_traced's, and
 * the particle caps are the same (the history is not in LDS).
 * The call has the persistent route only (the store could not drop the T n_cols columns the
 * statements would leave): WSMC_EARG, with the reason in wsmc_last_error() and the context as it
 * was, for n above the cap of the column count, a column that is not the spec's, multinomial
 * resampling, a sharded or multi-device handle, weights_changed set, more than WSMC_XPROG_MAX
 * program instructions. smooth NULL, or every member NULL: wsmc_ssm_run_traced.
 * The call allocates, for its duration, 8 T n n_cols bytes for the history, 4 T n n_obs for the
 * ancestor log (n_obs: the OBSERVEs, WEIGHTs and importance SAMPLEs of a step: the Resamples
 * that can run) and 16 T n_cols + 4 T n_obs for the rows and the
 * log's flags; WSMC_ENOMEM (the context as it was) when the device refuses them. */
int wsmc_ssm_run_smoothed(wsmc_ctx* ctx, const wsmc_ssm_spec* spec, const double* data, int32_t T,
                          double ess_perc_min, int32_t scheme, double* log_evidence_out,
                          const wsmc_ssm_trace* trace, const wsmc_ssm_smooth* smooth);
/* wsmc_ssm_run_batch_traced with the smoothed output of every filter (row b of each array is what
 * wsmc_ssm_run_smoothed gives on a fresh wsmc_create(n, seeds[b]) context); the same refusals as
 * wsmc_ssm_run_batch. The bytes above, per filter, are part of the call's device allocation;
 * WSMC_ENOMEM when the device refuses it. smooth NULL, or every member NULL:
 * wsmc_ssm_run_batch_traced. */
int wsmc_ssm_run_batch_smoothed(wsmc_ctx* ctx, const wsmc_ssm_spec* specs, int32_t n_specs,
                                const double* data, int32_t n_tables, int32_t T, int32_t n, int32_t B,
                                const uint64_t* seeds, double ess_perc_min, int32_t scheme,
                                wsmc_ssm_batch_out* out, const wsmc_ssm_trace* trace,
                                const wsmc_ssm_smooth* smooth);
/* stats_out[4] = the last smoothed run or batch on ctx: device time (HIP events on the stream) of its
 * segments, of the trace-back (phase 1) and of the rows kernel (phase 2), microseconds, and the
 * bytes the call allocated for the log and the rows. */
int wsmc_debug_ssm_smooth(wsmc_ctx* ctx, int64_t* stats_out);
/* ---- backward simulation: trajectories that do not collapse ------------------------------------
 * The genealogy above degenerates once T exceeds about n steps: every final particle then shares
 * one ancestor. Forward filtering, backward simulation keeps the filter's particles and weights at
 * every trace point (the record) and draws each of M trajectories backwards: at t = T-1 by the
 * last weights (src/utils.jl's `sample`, wsmc_sample_particles with replace), at t < T-1 with
 * particle i reweighted by the density of going from i to the successor already drawn, the
 * `logpdf` fields of src/default_kernels.jl's kernels.
 *
 * Which terms enter, and which specs are eligible (host only, no context). Walk `step` once with
 * every column tainted (it holds the previous trace point's value); z is the successor's row:
 *   SAMPLE col ~ dist        logpdf(dist, z[col]) is included iff an operand of dist reads a
 *                            tainted column (operands are read before the store, so its own column
 *                            counts as old); then col is untainted and holds z[col]
 *   SAMPLE_IMPORTANCE        col takes z[col] and is untainted; logpdf(target, z[col]) is included
 *                            iff an operand of target then reads a tainted column; the proposal is
 *                            not part of the model and never enters
 *   ASSIGN / ASSIGN_EXPR     col is tainted iff the right-hand side reads a tainted column; it
 *                            takes the computed value, never z[col]
 *   OBSERVE / WEIGHT         its logpdf is included iff its dist or value reads a tainted column
 * included[q] is set to 1 for an included statement q of `step`, else 0. WSMC_EARG, with the
 * reason in wsmc_last_error(): a spec wsmc_ssm_spec_check refuses; (a) the step's last statement is
 * not its last OBSERVE, the trace point; (b) a column written by a SAMPLE of either kind is
 * written by another statement of the step; (c) a state column, one that a statement of the step
 * reads before the step overwrites it, is tainted at the end of the step: a static parameter, a lag
 * carried by assignment, any deterministic carry-over (the transition is a Dirac and backward
 * simulation is not defined).
 * Caveat: an auxiliary column assigned from the old state (x / 2 + ... of the previous x, a copy
 * of it) holds in row t+1 of a drawn trajectory the filter particle's own value: f of that
 * particle's genealogical parent, not f of the drawn x_t. */
int wsmc_ssm_spec_backward(const wsmc_ssm_spec* spec, int32_t included[WSMC_SSM_MAX_STMTS]);
/* The results of a backward pass: caller-owned host buffers, each may be NULL (not wanted).
 * idx[t][m] is the filter particle trajectory m passes through at trace point t; paths[t][k][m] =
 * particles[t][k][idx[t][m]]; mean[t][k] and var[t][k] are wsmc_weighted_moments of row t of paths
 * (d = n_cols, expression k = paths[t][k] alone) on M particles with fresh (equal) weights. */
typedef struct {
    int32_t* idx;               /* [T][M]          */
    double*  paths;             /* [T][n_cols][M]  */
    double*  mean;              /* [T][n_cols]     */
    double*  var;               /* [T][n_cols]     */
    double*  particles;         /* [T][n_cols][n]  the record (wsmc_ssm_run_backward) */
    double*  log_weights;       /* [T][n]          */
} wsmc_ssm_backward_out;
/* sizeof(wsmc_ssm_backward_out) as the library was built (layout check) */
int wsmc_ssm_backward_out_sizeof(int64_t* bytes);
/* The backward pass over a record the caller supplies: particles [T][n_cols][n] and log_weights
 * [T][n] at the trace points of a run of `spec` over `data` (T x data_dim). Bit for bit what these
 * operators give, for trajectory m = 0 .. M-1 and t = T-1 down to 0 on a scratch context of n
 * particles and seed `seed`: wsmc_weights_upload(log_weights[t]); for t < T-1 wsmc_col_upload of
 * particles[t] and step t+1's statements in order, data row t+1 folded in, z = particles[t+1][.]
 * [idx[t+1][m]]: a SAMPLE as wsmc_weight(dist, const z[col]) if included, then wsmc_assign(col,
 * const z[col]); an importance SAMPLE as wsmc_assign(col, const z[col]), then wsmc_weight(target,
 * col) if included; an assignment as it is; an OBSERVE or WEIGHT as wsmc_weight(dist, value) if
 * included; no Resample; then wsmc_set_op_counter(t M + m) and wsmc_sample_particles(1, replace):
 * idx[t][m]. So the weights sum as ((lw + term_1) + term_2) ... in statement order and the draw is
 * wsmc_multi_target(wsmc_multi_word(seed, t M + m, 0), Q) on the integer weights, the first index
 * whose running sum exceeds it. One workgroup a trajectory, t looped on the device.
 * ctx gives the device and the stream only (as in wsmc_ssm_run_batch): nothing of it is read or
 * written. n <= 5120 (the record is not held in LDS, so the cap does not depend on n_cols);
 * 1 <= M <= wsmc_debug_ssm's cap for n_cols columns. out->particles and out->log_weights are not
 * written. WSMC_EARG: a spec wsmc_ssm_spec_backward refuses, n or M out of range, T < 1, null
 * record, out or data (with data_dim > 0), more than WSMC_XPROG_MAX program instructions, a
 * sharded or multi-device ctx. WSMC_ESTATE, the outputs unspecified: wsmc_sample_particles would
 * return it for some (t, m) (exp_norm of the weights is NaN). WSMC_ENOMEM: the device refuses the
 * record and the outputs. */
int wsmc_ssm_backward(wsmc_ctx* ctx, const wsmc_ssm_spec* spec, const double* data, int32_t T,
                      const double* particles, const double* log_weights, int32_t n, int32_t M,
                      uint64_t seed, const wsmc_ssm_backward_out* out);
/* wsmc_ssm_run_traced on the persistent route with the record logged to device memory (every
 * column and the log-weights at each trace point), and wsmc_ssm_backward's pass over it behind the
 * last segment on the stream, no host round trip in between. out->particles and out->log_weights
 * return the record if asked for. Everything the run leaves on ctx (columns, weights, ancestors,
 * state fields, tape, evidence, RNG positions, the filtering trace if asked) is bit for bit
 * wsmc_ssm_run_traced's; the backward pass draws from `seed`, not from the context's stream.
 * The call has the persistent route only: wsmc_ssm_run_smoothed's refusals and
 * wsmc_ssm_spec_backward's, M < 1 or above the cap, null out: WSMC_EARG with the context as it
 * was. WSMC_ENOMEM, the context as it was, when the device refuses the 8 T n (n_cols + 1) bytes of
 * the record plus the outputs. WSMC_ESTATE as above: the run itself is then complete. The genealogy
 * pass of wsmc_ssm_run_smoothed rewrites its history in place, so there is no `smooth` argument: a
 * caller who wants both makes two calls. */
int wsmc_ssm_run_backward(wsmc_ctx* ctx, const wsmc_ssm_spec* spec, const double* data, int32_t T,
                          double ess_perc_min, int32_t scheme, double* log_evidence_out,
                          const wsmc_ssm_trace* trace, int32_t M, uint64_t seed,
                          const wsmc_ssm_backward_out* out);
/* wsmc_ssm_run_batch_traced with wsmc_ssm_run_backward's pass for every filter: filter b is, bit for
 * bit, what wsmc_ssm_run_backward gives on a fresh wsmc_create(n, seeds[b]) context with
 * bw_seeds[b]. Every array of bw_out is [B]-leading (idx [B][T][M], paths [B][T][n_cols][M], mean and
 * var [B][T][n_cols], particles [B][T][n_cols][n], log_weights [B][T][n]). wsmc_ssm_run_batch's
 * refusals, wsmc_ssm_spec_backward's for every spec ("spec b: ..."), M < 1 or above the cap, null
 * bw_seeds or bw_out: WSMC_EARG. The record and the outputs of all B filters are part of the call's
 * device allocation: WSMC_ENOMEM when the device refuses it. WSMC_ESTATE, the backward outputs
 * unspecified, when a draw of any filter fails; the filters themselves are then complete. */
int wsmc_ssm_run_batch_backward(wsmc_ctx* ctx, const wsmc_ssm_spec* specs, int32_t n_specs,
                                const double* data, int32_t n_tables, int32_t T, int32_t n, int32_t B,
                                const uint64_t* seeds, double ess_perc_min, int32_t scheme,
                                wsmc_ssm_batch_out* out, const wsmc_ssm_trace* trace, int32_t M,
                                const uint64_t* bw_seeds, const wsmc_ssm_backward_out* bw_out);
/* stats_out[5] = the last backward pass on ctx: device time (HIP events on the stream) of the
 * run's segments (0 for wsmc_ssm_backward), of the backward kernel and of the rows and moments
 * kernel, microseconds, and the bytes the call allocated for the record and the outputs; then the
 * segments launched on the backward-recording kernels, cumulative per context (no other entry
 * point launches them). */
int wsmc_debug_ssm_backward(wsmc_ctx* ctx, int64_t* stats_out);
/* ---- conditional SMC: a filter run conditionally on a trajectory (particle Gibbs) ----------------
 * A conditional run of `spec` over `data` with a reference trajectory ref[T][n_cols] is the
 * unconditional run with two changes; particle n-1 is the reference particle.
 *   Pin. In `step`, never in `init`, right after a SAMPLE col ~ dist of step t has stored its
 *   draws, row n-1 of col becomes ref[t][col] (wsmc_sample, then wsmc_col_download, the last entry
 *   set, wsmc_col_upload). Every other particle keeps its draw; assignments recompute their columns
 *   for row n-1 from the pinned values; entries of ref for columns no SAMPLE of the step writes are
 *   ignored. `init` is not pinned (the record has no row for it): the run is conditional SMC for
 *   the model with `init` integrated out.
 *   Conditional Resample. The decision, the ESS, the evidence and the reset of the weights to the
 *   log-mean are the ordinary Resample's. When it runs, the ancestors are n independent draws with
 *   slot n-1 forced: idx[j] is wsmc_sample_particles(n, replace)'s draw j on the weights the
 *   Resample met, keyed by the op counter r the Resample takes (the first index whose running sum
 *   of the wsmc_qweight integers exceeds wsmc_multi_target(wsmc_multi_word(seed, r, j), Q)), then
 *   idx[n-1] = n-1. In operators: read the op counter r, the weights and every column; wsmc_resample
 *   (stratified); if it ran (wsmc_get_state's n_resamples grew: a Resample that meets unchanged
 *   weights, as after a SAMPLE, does nothing), wsmc_weights_upload of the saved weights to a scratch context of the
 *   same n and seed, wsmc_set_op_counter(r) and wsmc_sample_particles(n, 1) there, the last index
 *   forced, wsmc_col_upload(k, saved[k][idx]) for every column. Forcing a slot is exact for
 *   independent draws only, so there is no scheme argument.
 * Which columns are pinned, and which specs are eligible (host only, no context): pinned[k] is set
 * to 1 for a column a SAMPLE of `step` writes, else 0. WSMC_EARG, with the reason in
 * wsmc_last_error(): a spec wsmc_ssm_spec_check refuses; one that holds an importance SAMPLE or a
 * WEIGHT (pinning an importance Sample needs its weight term at the pinned value); an `init` that
 * holds anything but SAMPLE and assignments; a spec wsmc_ssm_spec_backward refuses (every state
 * column is then redrawn each step, so the pinned rows determine the reference particle). */
int wsmc_ssm_spec_conditional(const wsmc_ssm_spec* spec, int32_t pinned[WSMC_SSM_MAX_COLS]);
/* B conditional runs in one call, one persistent workgroup each: filter b is, bit for bit, the
 * definition above on a fresh wsmc_create(n, seeds[b]) context with reference[b] ([B][T][n_cols],
 * the spec's column order), and out, trace and the record are what wsmc_ssm_run_batch_backward
 * gives for it (out->last_ancestors: idx of the last Resample that ran). The record is always
 * logged. With M >= 1 filter b's backward pass is wsmc_ssm_backward's over its record with
 * bw_seeds[b]: a conditional sweep followed by one backward trajectory is the particle Gibbs
 * kernel with backward sampling, which leaves p(x_0:T-1 | y) invariant. M = 0 runs no backward
 * kernel: bw_seeds may be NULL, and bw_out may be NULL or ask for particles / log_weights alone.
 * ctx gives the device and the stream only (as in wsmc_ssm_run_batch). WSMC_EARG:
 * wsmc_ssm_run_batch_backward's refusals, wsmc_ssm_spec_conditional's for every spec ("spec b:
 * ..."), a null reference, M < 0. WSMC_ENOMEM and WSMC_ESTATE as there. */
int wsmc_ssm_run_conditional(wsmc_ctx* ctx, const wsmc_ssm_spec* specs, int32_t n_specs,
                             const double* data, int32_t n_tables, int32_t T, int32_t n, int32_t B,
                             const uint64_t* seeds, double ess_perc_min, const double* reference,
                             wsmc_ssm_batch_out* out, const wsmc_ssm_trace* trace, int32_t M,
                             const uint64_t* bw_seeds, const wsmc_ssm_backward_out* bw_out);
/* stats_out[5] = the last conditional batch on ctx: device time (HIP events on the stream) of its
 * segments, of the backward kernel and of the rows and moments kernel, microseconds, and the bytes
 * the call allocated for the record, the references and the outputs; then the segments launched on
 * the conditional kernels, cumulative per context (no other entry point launches them). */
int wsmc_debug_ssm_conditional(wsmc_ctx* ctx, int64_t* stats_out);
/* per-kernel timing of the last fused run (HIP events on the ctx stream), ms */
typedef struct {
    double total_ms;            /* whole run, first kernel to last                       */
    double propagate_ms;        /* sum over steps of the propagate/observe kernel         */
    double reduce_ms;           /* sum over steps of the weight-statistics kernel         */
    double resample_ms;         /* sum over steps of the scan/ancestor kernel             */
    double finalize_ms;         /* trace-back + final gather                              */
    int32_t steps;
    int32_t n_resamples;
} wsmc_run_timing;
int wsmc_run_set_timing(wsmc_ctx* ctx, int32_t enabled);
int wsmc_run_get_timing(wsmc_ctx* ctx, wsmc_run_timing* out);

/* ---- diagnostics ---------------------------------------------------------------
 * Average time (us) of `iters` back-to-back launches of one resample kernel on the
 * context's current weights: kernel 0 = weight statistics, 1 = reduce, 2 = ancestor scan;
 * mode 0 = production variant, > 0 = ablations (see csrc/wsmc_kernels.hip).        */
int wsmc_debug_kernel_bench(wsmc_ctx* ctx, int32_t kernel, int32_t mode, int32_t iters, double* avg_us);
/* Test hook: shard `shard` of the handle (0 for a single context) fails its nth next shard
 * record exchange (a Resample's or an evidence query's) with WSMC_EHIP before exchanging.
 * On a multi-device handle the other shards then leave their exchange with WSMC_ERCCL
 * instead of waiting for it; shards that left in different states mark the handle failed
 * (every later call returns WSMC_ESTATE). nth = 0 disarms. nth >= 1000: the failure is a
 * WSMC_EARG at exchange nth - 1000 (an argument error one shard meets alone past an exchange:
 * it requests the abort at once rather than waiting for peers that meet the same error). */
int wsmc_debug_inject_failure(wsmc_ctx* ctx, int32_t shard, int32_t nth);
/* Exact-sharded fused run: the fixed neighbour block (slots per step) and
 * trace window (ids per level) sizes — > 0 sets, 0 restores the defaults, < 0 leaves as is —
 * and, in stats_out[6] (may be NULL), the last run's largest block needed, its largest
 * lineage excursion, the runs re-done on the eager path after a block overflow, the block
 * size, the runs whose history was traced across ranks after a window overflow, and 1 when
 * later runs ship no trace windows (lineages wander past half a shard). */
int wsmc_debug_exact(wsmc_ctx* ctx, int64_t cap, int64_t ctr, int64_t* stats_out);
/* Statement batches compiled for their shape at run time (hiprtc; csrc/wsmc_jit.hip):
 * stats_out[5] = signatures compiled, signatures that failed to compile (their batches run on
 * the interpreter kernel), batches launched on compiled kernels, batches run on the
 * interpreter, total compile time (us) — process-wide. */
int wsmc_debug_jit_stats(int64_t* stats_out);
/* Compile representative batch signatures (the 2D SSM step, with and without the Resample
 * statistics, and four log-Gamma batches with column parameters: NegativeBinomial and Binomial each
 * drawn and scored, six Samples a batch, the other families) for gfx950 without a device:
 * WSMC_OK, or WSMC_EHIP with hiprtc's log in wsmc_last_error(). */
int wsmc_debug_jit_selfcheck(void);
/* The Move acceptance screen (csrc/wsmc_kernels.hip move_accept) on the current device: for each
 * u[i], out[2i] = the single-precision estimate of log u and out[2i+1] = the restated double log,
 * so a test can check the screen's band bound. Host buffers of n and 2n doubles. */
int wsmc_debug_log_screen(const double* u, int64_t n, double* out);
/* Move blocks compiled for their shape at run time (hiprtc; csrc/wsmc_mv_body.h): stats_out[5]
 * = signatures compiled, signatures that failed to compile, blocks launched on compiled kernels,
 * blocks run on the interpreter kernels, total compile time (us) — process-wide. */
int wsmc_debug_mv_jit_stats(int64_t* stats_out);
/* Compile a representative Move block (C3's shape) for gfx950 without a device: WSMC_OK, or
 * WSMC_EHIP with hiprtc's log in wsmc_last_error(). */
int wsmc_debug_mv_jit_selfcheck(void);
/* The fused 2D-SSM run's Resample statistics, cumulative over the context's
 * runs: stats_out[0] = the steps whose propagate guessed the reference point wrong (one GPU: found
 * by the fill; sharded: recomputed in place, k_rs_qfix), stats_out[1] = where the statistics are
 * taken (0 = their own kernel, 1 = the propagate with q stored, 2 = the propagate, the fill
 * recomputing q), stats_out[2] = the runs re-done on the exact path after a miss (one GPU),
 * stats_out[3] = the generic Resamples whose statistics the statement batch took (round 6; its
 * misses, recomputed by k_rs_qfix, count in stats_out[0]). stats_out holds 4 values. */
int wsmc_debug_run_stats(wsmc_ctx* ctx, int64_t* stats_out);
/* The fused 2D-SSM run's weight rows, counted on the device by the
 * propagate launches themselves and cumulative over the context's runs (a sharded handle reports
 * its first shard): stats_out[0] = the launches with the Resample statistics (steps 2..T of a
 * stratified or systematic run) that stored their weight row, stats_out[1] = those that recomputed
 * the previous step's row instead of loading it, stats_out[2] = those launches in all,
 * stats_out[3] = the launches without the statistics (step 1, the multinomial scheme, an exact
 * replay), which always store. A one-GPU run in statistics mode 1 stores the row of step t >= 2
 * only when step t - 1 did not resample or t is the last step; every other layout stores every
 * row. stats_out holds 4 values. */
int wsmc_debug_weight_stores(wsmc_ctx* ctx, int64_t* stats_out);
/* wsmc_ssm2d_run's calls by route, cumulative (a sharded handle reports its first shard):
 * stats_out[0] = the fused runs, stats_out[1] = the runs issued as statements because the context
 * held a column that is not the run's. stats_out holds 2 values. */
int wsmc_debug_ssm2d_routes(wsmc_ctx* ctx, int64_t* stats_out);

#ifdef __cplusplus
}
#endif
#endif /* WSMC_H */
