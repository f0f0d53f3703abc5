/*
 * deftri.h — C-ABI of the MI355X-native deformable-triangulation LM solver.
 *
 * This is the drop-in boundary for the hot path of
 * luicalrob/Triangulation-in-Deformable-Scenes: the g2o Levenberg–Marquardt
 * solve inside `arapOptimization` (Modules/Optimization/g2oBundleAdjustment.cc:608-1008
 * at the surveyed revision; the LM call is `optimizer.optimize(nOptIterations)`
 * at g2oBundleAdjustment.cc:962), and the BlockSolver_6_3 Schur LM of its BA entry
 * points (:38-444).  The reference's C++ entry points (Modules/Optimization/g2oBundleAdjustment.h:36-75)
 * are mirrored by deftri/optimization.py and deftri/ba.py; the adapter a C++ maintainer would put
 * behind those signatures is shown in INTEGRATION.md.  Both sit on this plain C interface.
 *
 * Conventions
 *  - every function returns int: 0 = OK, < 0 = error (see DEFTRI_E_*); the message
 *    of the last error on a context is available from deftri_last_error().
 *  - host arrays are owned by the caller and only read (or written, for outputs)
 *    during the call; device buffers are owned by the context.
 *  - one context per host thread; contexts are independent.
 *  - no C++ exceptions cross this boundary.
 *
 * Problem layout ("graph descriptor"): the flattened g2o graph that
 * arapOptimization builds (g2oBundleAdjustment.cc:640-953) — see DESIGN.md §2.
 *   vertices : points (3 dof, VertexSBAPointXYZ, g2oTypes.h:39-56),
 *              per KF-pair one SE3 T_g (g2o::VertexSE3Expmap, 6 dof, T <- exp(d)*T)
 *              and per KF-pair two depth scales (VertexDepthScale, g2oTypes.h:78-94)
 *   edges    : reprojection  EdgeSE3ProjectXYZPerKeyFrameOnlyPoints (g2oTypes.h:267-298),
 *              depth         EdgeDepthCorrection (g2oTypes.h:390-421),
 *              ARAP          EdgeARAP (g2oTypes.h:300-349).
 */
#ifndef DEFTRI_H
#define DEFTRI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEFTRI_ABI_VERSION 8

/* error codes */
#define DEFTRI_OK             0
#define DEFTRI_E_ARG         -1   /* invalid argument / inconsistent descriptor */
#define DEFTRI_E_HIP         -2   /* HIP runtime error (allocation, launch) */
#define DEFTRI_E_NOPROBLEM   -3   /* solve/download before upload */
#define DEFTRI_E_NUMERIC     -4   /* non-finite state */
#define DEFTRI_E_NODEVICE    -5   /* no usable gfx950 device */
#define DEFTRI_E_GRAPH       -6   /* graph construction failed (e.g. < 3 mesh points) */
#define DEFTRI_E_SEARCH      -7   /* the weight search ended on a failure code (nlopt::opt::optimize
                                     throws there, g2oBundleAdjustment.cc:515): the round is not run */
#define DEFTRI_E_INTERNAL    -8   /* an invariant of the library's own did not hold (the projection matchers'
                                     claim rounds did not settle in n + 1) */

/* solver status written into deftri_report.status (g2o SparseOptimizer::optimize semantics) */
#define DEFTRI_STATUS_OK         0  /* ran all requested iterations */
#define DEFTRI_STATUS_TERMINATE  1  /* g2o "Terminate": 10 failed trials, rho == 0 or lambda not finite */

typedef struct deftri_ctx deftri_ctx;

/* Flattened non-rigid BA / ARAP problem (all indices are 0-based). */
typedef struct deftri_problem_desc {
    int32_t n_points;   /* P   point vertices, 3 dof each                                  */
    int32_t n_pairs;    /* Q   KF pairs: one SE3 T_g vertex each                            */
    int32_t n_scales;   /* S   depth-scale vertices (reference: 2 per pair)                 */
    int32_t n_cams;     /* C   fixed camera poses / calibrations used by the edges          */
    int32_t n_rep;      /* R   reprojection edges                                           */
    int32_t n_depth;    /* D   depth edges                                                  */
    int32_t n_arap;     /* E   ARAP edges (directed, as the reference inserts them)         */
    int32_t n_rot;      /* rows of the per-mesh-vertex rotation table R_i                   */

    /* initial state */
    const double *points;     /* [P*3]  VertexSBAPointXYZ estimates                         */
    const double *tg;         /* [Q*7]  SE3Quat per pair: qx qy qz qw tx ty tz              */
    const double *scales;     /* [S]    VertexDepthScale estimates                           */

    /* cameras (fixed): Kannala–Brandt8 params and pose T_cw (g2o::SE3Quat of the KF pose)   */
    const float  *cam_kb8;    /* [C*8]  fx fy cx cy k0 k1 k2 k3 (KannalaBrandt8.cc:22-29)   */
    const double *cam_pose;   /* [C*7]  qx qy qz qw tx ty tz                                */

    /* reprojection edges: e = obs - KB8(T_cw * p), info = invSigma2(octave)*repW * I2,
       Huber(delta) — g2oBundleAdjustment.cc:765-812                                          */
    const int32_t *rep_point; /* [R] */
    const int32_t *rep_cam;   /* [R] */
    const double  *rep_obs;   /* [R*2] */
    const double  *rep_info;  /* [R]  scalar multiple of I2 */
    double huber_delta;       /* robust kernel delta (reference: (float)sqrt(100.991)); <= 0 disables */

    /* depth edges: e = (d/s - (T_cw p)_z)^2 (x500 if s <= 0), info = 1/sigma^2
       — g2oTypes.h:403-417, g2oBundleAdjustment.cc:816-856                                   */
    const int32_t *dep_point; /* [D] */
    const int32_t *dep_scale; /* [D] */
    const int32_t *dep_cam;   /* [D] */
    const double  *dep_meas;  /* [D] */
    const double  *dep_info;  /* [D] */

    /* ARAP edges (g2oTypes.h:311-342): vertices (p1_i, p2_i, p1_j, p2_j, T_g[pair]),
       R_i = rot[arap_rot[2e]], R_j = rot[arap_rot[2e+1]], w_ij = arap_w[e],
       area = pair_area[pair], info = pair_info[pair] (= arapW * T^2, :946)                 */
    const int32_t *arap_pts;  /* [E*4] */
    const int32_t *arap_pair; /* [E]   */
    const int32_t *arap_rot;  /* [E*2] */
    const double  *arap_w;    /* [E]   */
    const double  *rot;       /* [n_rot*9] row-major 3x3 */
    const double  *pair_area; /* [Q] */
    const double  *pair_info; /* [Q] */

    /* optional: 2-D ordering coordinates per point (the mesh plane).  NULL = use points x,y.
       Only affects the fill-reducing ordering of the sparse LDL^T, never the result's meaning. */
    const double *order_xy;   /* [P*2] or NULL */
} deftri_problem_desc;

typedef struct deftri_lm_params {
    int32_t n_iterations;   /* g2o optimize(n) */
    int32_t max_trials;     /* g2o _maxTrialsAfterFailure (default 10) */
    double  tau;            /* lambda init = tau * max diag(H) (default 1e-5) */
    double  user_lambda;    /* > 0: use as initial lambda (g2o _userLambdaInit) */
    int32_t analytic_jacobians; /* 1 = analytic ARAP/depth Jacobians (GPU default); 0 = g2o numeric central differences (delta 1e-9) */
    int32_t verbose;
} deftri_lm_params;

#define DEFTRI_MAX_REPORT_ITERS 1024

typedef struct deftri_report {
    int32_t status;                  /* DEFTRI_STATUS_* */
    int32_t iterations;              /* completed optimize() iterations */
    int32_t trials_total;            /* LM trials (accepted + rejected) */
    int32_t trials_rejected;
    double  chi2_initial;            /* activeRobustChi2 before the first iteration */
    double  chi2_final;
    double  lambda_final;
    double  chi2_iter[DEFTRI_MAX_REPORT_ITERS];   /* accepted chi2 after each iteration */
    int32_t trials_iter[DEFTRI_MAX_REPORT_ITERS]; /* trials used by each iteration */
    /* timing (ms, device-timed with HIP events) */
    double  ms_total;
    double  ms_linearize;            /* residuals + Jacobians + H/b assembly */
    double  ms_factor;               /* multifrontal LDL^T numeric factorization */
    double  ms_solve;                /* forward/backward substitution */
    double  ms_update;               /* oplus + chi2 re-evaluation; the three are -1 (not measured) for
                                        sequential trials unless DEFTRI_TRIAL_EVENTS=1 and on the iterative
                                        plan (per-trial events cost ~6 us of stream time each) */
    /* sizes of the sparse factorization */
    int64_t n_unknowns;
    int64_t nnz_factor;              /* entries of L (incl. dense fronts' boundary rows) */
    double  factor_flops;            /* per factorization */
    int32_t n_fronts;
    int32_t n_levels;
    /* speculative lambda lanes: trials_executed >= trials_total counts the lane trials run,
       including those past the accepted one (their results are discarded) */
    int32_t lanes;
    int32_t trials_executed;
    /* point-sharded solves (deftri_dist_*): this rank, the rank count, the factorization flops of
       all ranks (factor_flops and nnz_factor above are this rank's fronts) */
    int32_t rank;
    int32_t nranks;
    double  factor_flops_total;
    /* uploads on this context that found the same structure (index arrays and counts) as the
       analysed plan and only copied the values (no ordering / symbolic analysis / plan upload) */
    int64_t plan_reuses;
    /* PCG steps (deftri_set_linear_solver): trials solved by PCG, their CG iterations, trials that
       fell back to the factorization, and the device time of the PCG solves (ms, host-timed around
       the solve's final synchronization) */
    int32_t pcg_trials;
    int32_t pcg_fallbacks;           /* multifrontal plan: trials solved by the LDL^T instead; iterative
                                        plan: trials whose PCG failed (rejected, as a failed g2o solve) */
    int64_t pcg_iterations;
    double  ms_pcg;
    /* round 3 */
    int32_t pcg_given_up;            /* multifrontal plan: 1 when two consecutive fallbacks sent the rest of
                                        the call's trials straight to the LDL^T */
    int32_t plan;                    /* DEFTRI_PLAN_MULTIFRONTAL / DEFTRI_PLAN_ITERATIVE */
    /* round 4 (ABI 6) */
    int32_t pcg_continuations;       /* iterative plan: trials whose PCG outran the CG iterations queued
                                        before the evaluation (the last converged count + a margin):
                                        evaluated, restored, continued in chunks of 4 */
} deftri_report;

/* ---- context ---------------------------------------------------------------------- */
/* device >= 0: HIP device ordinal.  device < 0: host-only context (graph construction and
   symbolic analysis only; every device entry point then returns DEFTRI_E_NODEVICE). */
int deftri_ctx_create(int32_t device, deftri_ctx **out);
int deftri_ctx_destroy(deftri_ctx *ctx);
const char *deftri_last_error(const deftri_ctx *ctx);
int deftri_abi_version(void);

/* ---- flat-graph API ---------------------------------------------------------------- */
/* Validate, order (nested dissection), analyse (multifrontal symbolic) and copy to HBM.  A problem
   with the same structure (counts and index arrays) as the one uploaded before keeps the plan and
   the device buffers: only the values are copied (deftri_report.plan_reuses counts these). */
int deftri_problem_upload(deftri_ctx *ctx, const deftri_problem_desc *desc);
/* Run g2o-semantics Levenberg–Marquardt on the device. */
int deftri_solve_lm(deftri_ctx *ctx, const deftri_lm_params *params, deftri_report *report);
/* Speculative lambda lanes (0 = default: env DEFTRI_LM_LANES, else 2 below 3e10 flops per
   factorization (latency-bound) and 1 above; 1 = strictly sequential
   trials; at most 8).  g2o's trials within an iteration use a lambda sequence fixed in advance
   (reject: lambda *= ni, ni *= 2), so up to `lanes` consecutive trials are factored and solved in
   one batched pass (the lane is the second grid dimension of every factor/solve launch), each in
   its own arena and scratch state, and the accept/reject decisions are replayed in trial order:
   results are bit-identical to lanes = 1.  Fewer lanes are used when their buffers would not fit
   in half of the free device memory.  Pays off when the factorization is latency-bound (1k-30k
   correspondences: 11-24% per iteration); at C2 a 3-lane round costs 2.1 trials. */
int deftri_set_lm_lanes(deftri_ctx *ctx, int32_t lanes);
/* Jacobians used by deftri_arap_optimization: 0 (default) g2o's numeric central differences
   (delta 1e-9) for the ARAP and depth edges, as the reference (EdgeARAP has no linearizeOplus,
   g2oTypes.h:341; its analytic one is commented out, g2oTypes.cc:308-331); 1 the closed-form
   Jacobians (an opt-in speed-up, not the reference's arithmetic). */
int deftri_set_jacobian_mode(deftri_ctx *ctx, int32_t analytic);
/* Arithmetic of the factorization's trailing (Schur-complement) updates: 0 (default) fp64
   v_mfma_f64_16x16x4, the reference's precision (SimplicialLDLT in double); 1 fp32 products on
   v_mfma_f32_16x16x4 (operands rounded to fp32, fp32 accumulation per update launch, the result
   subtracted from the fp64 front), the panel factorizations, TRSM and substitution staying fp64.
   For the fp32-vs-fp64 sweep of BASELINE config C5 (tests/test_precision_sweep.py);
   not the reference's arithmetic. */
int deftri_set_factor_precision(deftri_ctx *ctx, int32_t fp32_updates);
/* Linear solver of the LM step (H + lambda I) dx = b inside deftri_solve_lm /
   deftri_arap_optimization (the reference: g2o BlockSolver + LinearSolverEigen, an exact sparse
   LDL^T).  DEFTRI_SOLVER_PCG (default): conjugate gradients preconditioned by the vertex blocks of
   H + lambda I (6x6 T_g, 1x1 scale, 3x3 point), stopped when the CG recurrence's residual r_k
   (not a recomputed b - A dx) satisfies ||r_k|| <= tol ||b|| (tol <= 0: 1e-12); the true residual
   differs from r_k by rounding drift, which tests/test_full_size_props.py measures through
   deftri_eval_hessian_product (< 1e-11 relative at C2).  What a solve that misses its budget or
   breaks down does depends on the plan: the multifrontal plan hands it to its LDL^T (max_iterations
   <= 0: a budget of about one factorization's cost, from the plan's sizes: ~70 at 100k
   correspondences, ~25 for a few hundred points); the iterative plan has no factorization, and the
   trial counts as a failed linear solve — g2o's rejected trial (lambda *= ni) — with a budget of
   1000 iterations when max_iterations <= 0 (DEFTRI_PLAN_ITERATIVE below).  Point-sharded contexts
   take PCG steps on the iterative plan by default and LDL^T steps on the sharded multifrontal plan
   with DEFTRI_SOLVER_DIRECT.  DEFTRI_SOLVER_DIRECT: the multifrontal LDL^T for every trial. */
#define DEFTRI_SOLVER_DIRECT 0
#define DEFTRI_SOLVER_PCG    1
int deftri_set_linear_solver(deftri_ctx *ctx, int32_t solver, double tol, int32_t max_iterations);
/* The last PCG step of this context (solve_lm trial or eval_damped_solve): CG iterations and
   whether it converged (0: the LDL^T solved that step). */
int deftri_last_step_info(const deftri_ctx *ctx, int32_t *pcg_iterations, int32_t *pcg_converged);

/* ---- plan kind (round 3) ---------------------------------------------------------------------
   DEFTRI_PLAN_MULTIFRONTAL: nested dissection + multifrontal LDL^T analysis at upload; PCG steps use
   the sliced matrix-free product where it fits (one KF pair) with the LDL^T as fallback.
   DEFTRI_PLAN_ITERATIVE: the point-sharded matrix-free PCG plan (csrc/spcg.h) — no factorization:
   rows = points grouped by mesh vertex in Morton order, dealt to the ranks in contiguous
   work-balanced ranges; per CG iteration an edge-parallel pass s_e = W_e J_e p over the rank's local
   ARAP edges and a row-parallel gather q_v = sum J_{e,v}^T s_e (+ the folded reprojection / depth
   blocks); sharded: one halo exchange of the boundary rows' (z, p) and ONE all-reduce per CG
   iteration (Chronopoulos-Gear single-reduction CG: r.z, r.r, z.Az and the global-vertex partials
   of A z travel together; plan_info.cg_collectives = 1).  A step whose PCG does not converge within
   the budget (deftri_set_linear_solver max_iterations; <= 0: 1000) counts as a failed linear solve
   (g2o: the trial is rejected; no LDL^T stands behind it).  One rank from 50,000 unknowns: two
   launches per CG iteration (the merged chain), whose alpha is handed from phase 2's workgroup 0 to
   the others through a published value and a flag; this relies on the dispatcher starting a
   launch's workgroups in index order (workgroup 0 resident while the others poll), which HIP does not
   promise: the poll is bounded, and a timeout fails the call with DEFTRI_E_HIP (never a rejected
   trial) and switches the context to a separate alpha launch for later calls.  Any keyframe count (all-pairs graphs, BASELINE C3-C5).
   DEFTRI_PLAN_AUTO (default): ITERATIVE when the step solver is DEFTRI_SOLVER_PCG at upload and the
   context is point-sharded (nranks > 1) or the problem has >= 50,000 unknowns (measured faster from
   C2 up); MULTIFRONTAL otherwise.  Applies to the next deftri_problem_upload.  A
   context on the iterative plan that is asked for what only the factorization has (LDL^T steps or
   solves after deftri_set_linear_solver(DIRECT)) analyses and uploads the multifrontal plan at that
   point, continuing from its current state; deftri_eval_hessian_product stays on the iterative plan
   (its own matrix-free product, H never assembled). */
#define DEFTRI_PLAN_AUTO          0
#define DEFTRI_PLAN_MULTIFRONTAL  1
#define DEFTRI_PLAN_ITERATIVE     2
int deftri_set_plan(deftri_ctx *ctx, int32_t plan);
/* Storage of the ARAP Jacobians the iterative plan's product reads: 0 (default) fp64, 1 fp32 (the
   C5 precision sweep: the product then applies the fp32-rounded J; b, the preconditioner, the
   vectors and every reduction stay fp64).  Applies to the next deftri_problem_upload. */
int deftri_set_jacobian_storage(deftri_ctx *ctx, int32_t fp32);
typedef struct deftri_plan_info {
    int32_t plan;              /* DEFTRI_PLAN_MULTIFRONTAL / DEFTRI_PLAN_ITERATIVE of the uploaded problem */
    int32_t rank, nranks;
    int32_t own_rows;          /* iterative: point rows this rank owns */
    int64_t halo_rows;         /* iterative: rows received from other ranks per exchange */
    int64_t local_arap_edges;  /* iterative: ARAP edges this rank evaluates (owned + halo-only) */
    int64_t n_unknowns;
    int32_t phase1_blocks, row_blocks;
    double  product_bytes;     /* algorithmic bytes of one matrix-free product on this rank */
    int32_t jacobian_fp32;
    int32_t cg_launches;       /* iterative: kernel launches per CG iteration (one rank from 50,000
                                  unknowns: 2, the merged chain — phase 1 forms p.Ap, phase 2 the
                                  update; one rank below that: 3, the dots and the heavy-vertex finish
                                  in last workgroups; sharded: 3, the single-reduction chain —
                                  phase 1 and phase 2 form w = A z, k_sp_update_sd the update) */
    int32_t cg_collectives;    /* iterative: all-reduces per CG iteration (one rank 0; sharded 1, plus
                                  one grouped halo send / receive) */
    int32_t sharded;           /* iterative: the sharded control flow (nranks > 1, or one rank with an
                                  RCCL communicator: deftri_dist_init_rccl(ctx, 1, 0, id)) */
    double  survey_bytes;      /* SURVEY.md §8(d)'s B_pcg of this rank's share: 176 E + 48 R + 40 D + 156 P
                                  (owned ARAP edges, own rows' reprojection / depth edges, own rows) */
    int32_t tiles;             /* iterative: the fused product's tiles (every ARAP edge read once per CG
                                  iteration) — one rank (one keyframe pair since round 5, several since
                                  round 6) or a sharded one-pair plan; 0: the two-phase product */
    int32_t halo_overlap;      /* iterative, sharded (round 5): 1 when the boundary rows' exchange runs
                                  on its own stream beside the interior edges' product */
} deftri_plan_info;
int deftri_get_plan_info(const deftri_ctx *ctx, deftri_plan_info *info);
/* TEST ONLY (no GPU): host emulation of one product q = (H + lambda I) p with the iterative plan's
   decomposition on this rank (deftri_dist_set_transport: rank / nranks and the callback): the rank
   reads only its own rows of p, receives its halo rows through the callback's send / receive in the
   device exchange's global order, all-reduces the global vertices' partials of its owned edges
   (sum), and sums its rows' incidences.  H = sum_e J_e^T W_e J_e over the edges of `desc` with the
   caller's per-edge Jacobians (jarap [E*18] as g2o orders an ARAP edge's vertices, jrep [R*6] 2x3,
   jdep [D*4] point + scale) and scalar weights.  p, q [n], vertex order [T_g][scales][points]; q
   receives this rank's point rows and the global vertices, zeros elsewhere.  stats (may be NULL):
   own rows, halo rows, local ARAP edges, owned ARAP edges. */
int deftri_debug_sp_product(deftri_ctx *ctx, const deftri_problem_desc *desc, const double *jarap, const double *warap,
                            const double *jrep, const double *wrep, const double *jdep, const double *wdep,
                            double lambda, const double *p, double *q, int64_t n, int64_t *stats);
/* ---- simulated observations (upstream producer, host) --------------------------------------
   SLAM::setCameraPoses + getSimulatedDepthMeasurements + createKeyPoints (Modules/System/SLAM.cc:
   223-338): T1w = (I, c1), T2w = (lookAt(c2, moved[0]), c2) as Sophus SE3f (pose = the fp32 unit
   quaternion qx qy qz qw + t); depth_k = z_c * depth_scale_k + N(0, depth_error_mm / 1000) and
   keypoints = KB8 project + N(0, rep_error) rounded to `decimals`, from libstdc++'s
   std::default_random_engine + std::normal_distribution<float> (one fresh engine per function, as
   the reference).  orig / moved [n*3], uv [n*2], depth [n]. */
int deftri_sim_two_view(int32_t n, const float *orig, const float *moved, const float c1[3], const float c2[3],
                        const float kb8_1[8], const float kb8_2[8], float rep_error, int32_t decimals,
                        float depth_error_mm, float depth_scale_1, float depth_scale_2, float *uv1, float *uv2,
                        float *depth1, float *depth2, float pose1[7], float pose2[7]);
/* n draws of one fresh std::default_random_engine + std::normal_distribution<float>(mean, stddev). */
int deftri_sim_normal_stream(int64_t n, float mean, float stddev, float *out);

/* ---- point-sharded ARAP solve (multi-GPU) -------------------------------------------------
   One context per GPU, rank `rank` of `nranks`; every rank uploads the same full problem.  The
   nested-dissection tree is split by rank ranges (a rank owns one subtree, the leading ranks of
   each range also the separator fronts above it); each rank linearizes the edges whose
   first-eliminated vertex it owns, assembles and factors its fronts, and per LM trial sends one
   packed contribution block (lower triangle) up to the owner of its top front's parent, one
   forward-update vector up and receives the boundary solution back; chi2, dx.(lambda dx + b) and
   the zero-pivot flags are all-reduced (sum), the lambda init takes the max of the all-reduced
   diagonal.  Every rank then holds the solution of its own vertices and of its top front's
   boundary vertices (deftri_dist_vertex_owner tells which rank is authoritative for each vertex).
   Transport: RCCL (ncclCommInitRank from a deftri_rccl_unique_id shared by the caller; send/recv
   and all-reduce on the solver stream, over xGMI) or a caller callback through host memory (tests:
   gloo).  Set before deftri_problem_upload / deftri_problem_analyse (it discards the uploaded
   problem); nranks == 1 restores the single-GPU plan.  Diagnostics entry points other than
   deftri_eval_chi2 refuse a sharded context.
   Callback: op 0 all-reduce sum / 1 all-reduce max of n doubles in place (peer = -1), 2 send n
   doubles to `peer`, 3 receive n doubles from `peer`; returns 0 on success.  Every rank makes the
   calls in the same global order. */
typedef int (*deftri_xfer_fn)(void *user, int32_t op, int32_t peer, double *buf, int64_t n);
int deftri_dist_init_rccl(deftri_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t id[128]);
int deftri_dist_set_transport(deftri_ctx *ctx, int32_t nranks, int32_t rank, deftri_xfer_fn fn, void *user);
/* Elimination order of the analysed plan: order[k] = vertex [T_g per pair][scales][points]
   eliminated k-th (nv entries). */
int deftri_plan_vertex_order(const deftri_ctx *ctx, int64_t *order, int64_t nv);
/* Owning rank of every vertex [T_g per pair][scales][points] of the analysed problem (nv entries). */
int deftri_dist_vertex_owner(const deftri_ctx *ctx, int32_t *owner, int64_t nv);
/* 0/1 per edge of the analysed problem: edges this rank linearizes (any output may be NULL). */
int deftri_dist_owned_edges(const deftri_ctx *ctx, uint8_t *rep, uint8_t *dep, uint8_t *arap);
/* TEST ONLY: host emulation of this rank's damped solve (H_q + lambda on its diagonal) x = b_q, with
   H_q, b_q this rank's partial system (row-major n x n, the sum over ranks is H, b), exchanging
   through the callback transport; x receives the solution of the rank's own and boundary dofs. */
int deftri_debug_plan_solve_dist(deftri_ctx *ctx, const double *Hq, double lambda, const double *bq, double *x,
                                 int64_t n);

/* Copy the current state back: points [P*3], scales [S], tg [Q*7] (any may be NULL). */
int deftri_download(deftri_ctx *ctx, double *points, double *scales, double *tg);
/* Reset the device state to the uploaded initial values (no re-analysis). */
int deftri_reset_state(deftri_ctx *ctx);

/* ---- diagnostics (parity tests) ----------------------------------------------------- */
/* activeRobustChi2 at the current device state. */
int deftri_eval_chi2(deftri_ctx *ctx, double *chi2);
/* Linearize at the current state and return b (gradient side, g2o sign: b = -J^T W e)
   in the vertex order [T_g(6) per pair][scales][points(3)], and the diagonal of H. */
int deftri_eval_gradient(deftri_ctx *ctx, double *b, double *hdiag, int64_t n);
/* y = H x for the current linearization (same vertex order).  On the iterative plan: the CG
   chain's own matrix-free product kernels (H is never assembled; analytic-Jacobian linearization,
   as deftri_eval_damped_solve), so a solve's true residual ||b - (H + lambda I) x|| can be measured
   at any size; on the multifrontal plan: the assembled blocks. */
int deftri_eval_hessian_product(deftri_ctx *ctx, const double *x, double *y, int64_t n);
/* Solve (H + lambda I) x = rhs (analytic-Jacobian linearization at the current state) with the
   configured step solver (deftri_set_linear_solver: PCG with LDL^T fallback, or the LDL^T). */
int deftri_eval_damped_solve(deftri_ctx *ctx, double lambda, const double *rhs, double *x, int64_t n);
/* Number of unknowns of the uploaded problem. */
int64_t deftri_num_unknowns(const deftri_ctx *ctx);

/* Validate + analyse (ordering, multifrontal plan) without touching a device. */
int deftri_problem_analyse(deftri_ctx *ctx, const deftri_problem_desc *desc);
/* Plan statistics of the analysed problem: n_unknowns, nnz_factor, factor_flops, n_fronts,
   n_levels (other report fields zero). */
int deftri_plan_stats(const deftri_ctx *ctx, deftri_report *report);
/* TEST ONLY: execute the analysed multifrontal plan with host loops on a dense, row-major
   n x n H (vertex order as above) to check the symbolic analysis without a GPU.  Not used by
   any solve path. */
int deftri_debug_plan_solve(deftri_ctx *ctx, const double *H, double lambda, const double *rhs,
                            double *x, int64_t n);
/* Per-kernel device timing of one LM trial (linearize + assemble + setLambda + LDL^T + solve),
   each launch bracketed by HIP events on the solver's stream.  flops are algorithmic counts
   for the dense factor kernels (0 where not defined). */
typedef struct deftri_kernel_stat {
    char    name[32];
    int64_t launches;
    double  ms;          /* summed device time */
    double  flops;       /* algorithmic flops of all launches */
    double  bytes;       /* algorithmic HBM bytes of all launches (0 where not defined) */
} deftri_kernel_stat;
int deftri_profile_trial(deftri_ctx *ctx, double lambda, deftri_kernel_stat *stats,
                         int32_t max_stats, int32_t *n_stats);

/* sizeof() of the ABI structs for binding checks: 0 deftri_problem_desc, 1 deftri_lm_params,
   2 deftri_report, 3 deftri_keyframe, 4 deftri_map, 5 deftri_ba_desc, 6 deftri_pixels_error,
   7 deftri_plan_info, 8 deftri_deformation_params, 9 deftri_deformation_report,
   10 deftri_deformation_eval, 11 deftri_depth_image, 12 deftri_real_abs_errors,
   14 deftri_feature_grid, 15 deftri_fast_params, 16 deftri_fast_report, 17 deftri_orb_params,
   18 deftri_orb_report, 20 deftri_projection_report, 22 deftri_essential_report,
   23 deftri_triangulation_match_report, 24 deftri_delaunay_report, 25 deftri_arap_deform_params,
   26 deftri_arap_deform_report (13, 19 and 21 are unassigned and answer -1, like every other
   index). */
int64_t deftri_sizeof(int32_t which);

/* ---- map-level API (Modules/Optimization/g2oBundleAdjustment.h:56-60) ---------------- */
/* A keyframe as the solver reads/writes it (Modules/Map/KeyFrame.h): slots i = 0..n_slots-1
   hold an optional MapPoint (point_id < 0 = null), its keypoint, octave and simulated depth. */
typedef struct deftri_keyframe {
    int64_t id;                 /* KeyFrame id */
    double  pose[7];            /* T_cw as qx qy qz qw tx ty tz (from Sophus::SE3f) */
    float   kb8[8];             /* calibration */
    int32_t n_scales;           /* octave table size */
    const float *inv_sigma2;    /* [n_scales] Frame::vInvSigma2_ (Frame.cc:61-75) */
    double  depth_scale;        /* estimatedDepthScale_ (in/out) */
    int32_t n_slots;
    int64_t *point_id;          /* [n_slots] MapPoint id, < 0 = null slot                  */
    float   *point_pos;         /* [n_slots*3] MapPoint world position (in/out, fp32 as the reference) */
    const int32_t *obs_index;   /* [n_slots] Map::isMapPointInKeyFrame(point, kf) (< 0 = none) */
    const float *kp_uv;         /* [n_obs*2] keypoints by observation index */
    const int32_t *kp_octave;   /* [n_obs] */
    const float *depth;         /* [n_obs] simulated depth per observation index (KeyFrame.cc:123-125);
                                   unused, and may be NULL, for a keyframe with a depth image on the
                                   context (deftri_set_depth_images) */
    int32_t n_obs;
} deftri_keyframe;

/* One entry of Map::mGTransformation_ (Modules/Map/Map.cc:323-343): the transformation stored for
   the ordered KeyFrame-id pair (kf1, kf2).  insertGlobalKeyFramesTransformation stores T for
   (kf1, kf2) and T.inverse() (Sophus, fp32) for (kf2, kf1): pass both entries. */
typedef struct deftri_global_entry {
    int64_t kf1, kf2;
    double  t[7];                 /* qx qy qz qw tx ty tz */
} deftri_global_entry;

typedef struct deftri_map {
    int32_t n_keyframes;
    deftri_keyframe *keyframes;   /* in the reference's unordered_map iteration order */
    double global_t[7];           /* out: the optimized T_g, stored by the reference as (0, 1) (:1007).
                                     in (legacy, only when n_global == 0): T for the first pair */
    int32_t n_global;             /* in: entries of the map's global-transformation table */
    const deftri_global_entry *globals;   /* every pair (kf1, kf2) of the graph starts from
                                     getGlobalKeyFramesTransformation(kf1.id, kf2.id) (:664): the
                                     entry for that ordered id pair, identity when absent */
} deftri_map;

/* arapOptimization(Map*, rep, global, arap, alpha, beta, depthError, nIt, optimizationUpdate)
   (g2oBundleAdjustment.cc:608).  Builds the graph on the host (Delaunay mesh, cotangent
   weights, per-vertex R_i, reference indexing), solves on the device, writes back
   positions (fp32), depth scales and the global transformation.  optimization_update may be
   NULL; when given it receives sum ||p_old - p_new|| (:974-990). */
int deftri_arap_optimization(deftri_ctx *ctx, deftri_map *map, double rep_weight,
                             double global_weight, double arap_weight, double alpha,
                             double beta, float depth_error, int32_t n_iterations,
                             double *optimization_update, deftri_report *report);

/* PixelsError (Modules/Utils/CommonTypes.h:23-30). */
typedef struct deftri_pixels_error {
    double avgc1, avgc2, avg;      /* mean |obs - proj| per camera (last pair), their average */
    double desvc1, desvc2, desv;   /* RMS |obs - proj| per camera (last pair), their average */
} deftri_pixels_error;

/* calculatePixelsStandDev(Map, PixelsError&) (Modules/Utils/Geometry.cc:370-498) on the device:
   for every keyframe pair (k1, k2 > k1 in map order; camera 1 = k2, camera 2 = k1) and every slot
   whose MapPoints both exist and are observed, the fp32 homogeneous projection error; per pair the
   reference's formulas (nMatches and the mean accumulators carry across pairs, the squared sums
   do not; the values of the last pair are returned).  Reads the map's fp32 positions. */
int deftri_pixels_stand_dev(deftri_ctx *ctx, const deftri_map *map, deftri_pixels_error *out);

/* ---- map-error measurements (Modules/Utils/Measurements.cc) --------------------------------- */
/* measureSimAbsoluteMapErrors (:8-98): MapPoints 2j and 2j+1 (by id) against original[j] / moved[j]
   for j < (#MapPoints)/2; the figures the reference prints / writes to Experiment.txt, in mm. */
typedef struct deftri_abs_errors {
    double average_movement;        /* mean |original - moved| */
    double average_error_original;  /* mean |p_2j - original| */
    double average_error_moved;     /* mean |p_2j+1 - moved| */
    double average_error;           /* (sum of both) / #MapPoints ("Av. error") */
    double rmse;                    /* sqrt(sum of squared errors / #MapPoints) ("RMSE") */
    int64_t point_count;            /* #MapPoints */
} deftri_abs_errors;
int deftri_measure_sim_absolute_map_errors(int32_t device, const deftri_map *map, int32_t n_points,
                                           const float *original, const float *moved, deftri_abs_errors *out);
/* measureRelativeMapErrors (:350-518), per keyframe pair in the map's order: the values after that
   pair (the accumulators carry over pairs, as in the reference).  Depth uses the per-index simulated
   measurement (the reference's depth-image lookup throws in the simulation). */
typedef struct deftri_rel_errors {
    int64_t kf1, kf2;               /* KeyFrame ids (k2->first, k1->first) */
    int32_t reported;               /* validPairs > 1: the reference prints / writes the pair */
    double rel_error;               /* sum ||(pi2 - pj2) - (pi1 - pj1)||^2 / mesh area ("Rel. error") */
    double depth_error;             /* sum (d - z s)^2 ("depthError") */
    double global_t_error;          /* sum ||(R pi2 - t - pi1) + (R pj2 - t - pj1)||^2 / area */
    double area;                    /* the pair's mesh surface area */
    int64_t valid_pairs, n_matches;
} deftri_rel_errors;
int deftri_measure_relative_map_errors(int32_t device, const deftri_map *map, deftri_rel_errors *out,
                                       int32_t max_pairs, int32_t *n_pairs);

/* ---- real-image input: keyframe depth images ------------------------------------------------
   With real keyframes the reference takes every depth measurement from the keyframe's depth image:
   KeyFrame::getDepthMeasure(x, y, scaled) (KeyFrame.cc:181-202) = the bilinear Interpolate
   (Geometry.cc:607-620, fp32) of the CV_32F image, (double)interp / 100, and — for scaled == 0; the
   reference's flag name reads backwards, KeyFrame.cc:196-201 — times imageDepthScale_.
   arapOptimization's depth edges (g2oBundleAdjustment.cc:816,846) and measureRelativeMapErrors
   (Measurements.cc:439-440) call it with scaled = false, measureRealAbsoluteMapErrors (:179-180)
   with the default true.
   deftri_set_depth_images copies the images to memory owned by the context (device memory on a
   device context), where they stay until the next call replaces the set (n = 0 clears it).  From then
   on every graph build on the context (deftri_arap_build_graph, deftri_arap_optimization, every
   clone and round of deftri_deformation_optimization) reads the depth measurement of a keyframe
   that has an image from the image at the observation's keypoint; such a keyframe's `depth` may be
   NULL.  Keyframes without an image use depth[] as before (mixed maps are legal).  The depths of a
   keyframe are sampled once per (image set, keyframe, keypoints) and cached on the context.
   Status per pixel: 0 ok; 1 x >= cols or y >= rows (the reference throws std::out_of_range); 2 the
   reference would read outside the buffer (a negative or non-finite coordinate, or one of the four
   linear indices r*cols+c, +1, (r+1)*cols+c, +1 at or beyond rows*cols, e.g. y in the last row).
   The reference's row-major spill into the next row at x in [cols-1, cols) of a row that is not the
   last is defined memory and is reproduced.  A pixel with a non-zero status is never loaded and its
   depth is NaN; a graph build or measurement fails with DEFTRI_E_ARG only when an observation it
   uses has a non-zero status (the message names the keyframe id, the observation index and the
   pixel), leaving the map unchanged. */
typedef struct deftri_depth_image {
    int64_t kf_id;             /* KeyFrame id */
    int32_t rows, cols;        /* CV_32F, row-major, continuous */
    const float *pixels;       /* [rows*cols], host, read during the call only */
    double image_depth_scale;  /* KeyFrame::imageDepthScale_ */
    float ph[4];               /* KeyFrame::phcalibration_: fx fy cx cy (PinHole.h:42) */
} deftri_depth_image;
int deftri_set_depth_images(deftri_ctx *ctx, int32_t n, const deftri_depth_image *images);
/* getDepthMeasure(uv[2k], uv[2k+1], scaled) of keyframe kf_id's image for n pixels: depth [n] and
   status [n] (either may be NULL).  On a device context the device samples (k_depth_sample); a
   host-only context runs the same function on the host. */
int deftri_depth_measure(deftri_ctx *ctx, int64_t kf_id, int32_t n, const float *uv, int32_t scaled,
                         double *depth, uint8_t *status);
/* Images copied by deftri_set_depth_images and keyframe samplings (cache misses) over the context's
   life; both stay 0 on a context that never received an image. */
int deftri_depth_image_stats(const deftri_ctx *ctx, int64_t *uploads, int64_t *samplings);

/* measureRealAbsoluteMapErrors (Measurements.cc:101-348) with the context's depth images: per pair
   (camera 1 = k2) and matched slot, both keypoints unprojected with keyframe 1's pinhole calibration,
   scaled by each keyframe's own getDepthMeasure(x, y) and taken to the world by T.inverse().matrix();
   a second pass per pair divides by the running scales.  n_points, scale1 and scale2 carry across
   the pairs as in the reference (scale = scale / n_points after each pair's first pass).  Figures
   in mm; the per-slot terms are summed in fp64 in a fixed order and the totals cast to float before
   the reference's float divisions.  Every keyframe needs an image; kf2.n_slots <
   kf1.n_slots or an observation index out of range is DEFTRI_E_ARG (the reference indexes
   unchecked). */
typedef struct deftri_real_abs_errors {
    double average_movement;           /* "Av. movement" (:335) */
    double average_error;              /* "Av. error" */
    double rmse;                       /* "RMSE" */
    double average_up_to_scale_error;  /* "Av. up-to-scale error in 3D" */
    int64_t point_count;               /* Map::getMapPoints().size() */
    int64_t n_points;                  /* matched slots over all pairs (testing) */
    double scale1, scale2;             /* the float accumulators after the last pair (testing) */
} deftri_real_abs_errors;
int deftri_measure_real_absolute_map_errors(deftri_ctx *ctx, const deftri_map *map, deftri_real_abs_errors *out);
/* deftri_measure_relative_map_errors with the depth measurements of keyframes that have an image
   taken from the context's images (getDepthMeasure(u, v, false)), on the context's device.  As the
   reference (Measurements.cc:432,440), the pixel looked up in keyframe 2's image is keyframe 1's
   keypoint idx2; idx2 >= kf1.n_obs is DEFTRI_E_ARG. */
int deftri_measure_relative_map_errors_images(deftri_ctx *ctx, const deftri_map *map, deftri_rel_errors *out,
                                              int32_t max_pairs, int32_t *n_pairs);


/* Mapping::triangulateSimulatedMapPoints (Modules/Mapping/Mapping.cc:280-349) for Triangulation.method
   "NRSLAM", seed.location "FarPoints" (Simulation.yaml): per correspondence i, KB8 unproject of
   uv1[i] / uv2[i] (KannalaBrandt8.cc:51-83), triangulateNRSLAM (Geometry.cc:103-153) and
   isValidParallax (Mapping.cc:351-366: both depths >= 0, cos parallax <= min_cos).  Poses are
   T_cw as 3x4 fp32 row-major [R | t] (Sophus::SE3f::matrix3x4()).  Outputs: world points for KF 1
   and KF 2 [n*3] and valid[n] (the reference's `continue` skips invalid ones). */
int deftri_triangulate_nrslam(deftri_ctx *ctx, int32_t n, const float *uv1, const float *uv2,
                              const float *kb8_1, const float *kb8_2, const float *T1w, const float *T2w,
                              float min_cos, float *x3d_1, float *x3d_2, uint8_t *valid);

/* ---- every seed the reference defines (useTriangulationMethod, Geometry.cc:216-230) -----------
   Triangulation.method and Triangulation.seed.location as enums.  The reference's `if` chains map the
   strings: a method other than "Classic", "ORBSLAM", "DepthMeasurement" is NRSLAM; a location other
   than "TwoPoints" / "FarPoints" is the in-rays seed (each point on its own ray).
     NRSLAM  triangulateNRSLAM (:103-153): TwoPoints, FarPoints, in-rays.
     CLASSIC triangulateClassic (:62-101): TwoPoints, in-rays; FarPoints falls into its else (in-rays).
             n = svd.matrixV().col(1) of A = M^T (I - t t^T) is computed in closed form: v0 from the 2x2
             A A^T, n = t x v0 (an fp32 SVD does not resolve col(1)).
     DEPTH   triangulateDepth (:189-214) is defined only inside reconstructPoints, where the unit rays
             go straight in.  In the simulated entry its inputs are CameraModel::unproject(x, d), which
             returns an unset vector (CameraModel.h:128-135, unprojectWithZ commented out):
             deftri_triangulate returns DEFTRI_E_ARG.
     ORBSLAM triangulateORBSLAM (:155-186) never writes x3D_1 / x3D_2 and the callers read unset
             memory: DEFTRI_E_ARG in both entries. */
#define DEFTRI_TRI_CLASSIC 0
#define DEFTRI_TRI_NRSLAM  1
#define DEFTRI_TRI_ORBSLAM 2
#define DEFTRI_TRI_DEPTH   3
#define DEFTRI_LOC_INRAYS    0   /* any string other than the two below */
#define DEFTRI_LOC_TWOPOINTS 1
#define DEFTRI_LOC_FARPOINTS 2

/* deftri_triangulate_nrslam for any defined (method, location): the same unprojection, isValidParallax
   test, conventions and outputs; deftri_triangulate_nrslam is its (NRSLAM, FARPOINTS). */
int deftri_triangulate(deftri_ctx *ctx, int32_t n, int32_t method, int32_t location, const float *uv1,
                       const float *uv2, const float *kb8_1, const float *kb8_2, const float *T1w,
                       const float *T2w, float min_cos, float *x3d_1, float *x3d_2, uint8_t *valid);

/* MonocularMapInitializer::reconstructPoints (MonocularMapInitializer.cc:281-395) for n matched pixel
   pairs (uv2 already gathered through vMatches_), the poses given.  Per correspondence: both world
   points, cos_parallax (:324-326) and a status, the reference's tests in order, first failure wins:
     0 kept;  1 a point not finite or isZero() (every |coefficient| <= 1e-5, :315);
     2 z_1 < 0 or z_1 > depth_limit (:329);  3 checks and squared reprojection error in view 1 > 5.991
     (:339);  4 the depth test in view 2 (:346);  5 the reprojection test in view 2 (:355).
   The report restates :370-394 on the host: n_triangulated = 2 * kept, parallax_deg = the degrees of
   the min(50, kept - 1)-th smallest kept cosine, accepted = that cosine in [0, 1] and n_triangulated >=
   25 and parallax_deg > min_parallax (the reference passes Triangulation.minCos here, Mapping.cc:60).
   Nothing kept, or the cosine outside [0, 1] (the reference returns before setting it): parallax_deg 0,
   accepted 0.  n == 0 returns 0 with a zeroed report. */
typedef struct deftri_reconstruct_params {
    int32_t method, location;   /* DEFTRI_TRI_*, DEFTRI_LOC_* */
    int32_t checks;             /* Triangulation.checks == "true" */
    float depth_limit;          /* Triangulation.depthLimit */
    float min_parallax;
} deftri_reconstruct_params;
typedef struct deftri_reconstruct_report {
    int64_t n_triangulated, n_nonfinite, n_depth1, n_err1, n_depth2, n_err2;
    float parallax_deg;
    int32_t accepted;
} deftri_reconstruct_report;
int deftri_reconstruct_points(deftri_ctx *ctx, int32_t n, const float *uv1, const float *uv2,
                              const float *kb8_1, const float *kb8_2, const float *T1w, const float *T2w,
                              const deftri_reconstruct_params *params, float *x3d_1, float *x3d_2,
                              uint8_t *status, float *cos_parallax, deftri_reconstruct_report *report);

/* The initial estimatedDepthScale_ of two real keyframes (Mapping.cc:183-254) for the n correspondences
   reconstructPoints kept, from the context's depth images of kf_id_1 / kf_id_2.  keep[i] = 0 where
   getDepthMeasure(x, y) <= 0 in either image or a pixel is outside (0.1, 1500) in x or y (the
   reference's literals, :194-200); such a pair gets no MapPoints.  A kept pair whose parallax angle in
   DEGREES exceeds min_cos — the reference compares degrees with Triangulation.minCos (:220), reproduced
   as it stands — adds getDepthMeasure(x, y, false) / z_c to its keyframe's fp64 sum; scale = sum /
   n_points.  The sums are reduced per workgroup on the device and added in workgroup order on the
   host (no atomics: the same bits every run).  n_points == 0 leaves both scales NaN, the reference's
   0 / 0.  A pixel whose sampler status is not 0 fails the call with DEFTRI_E_ARG (the message names the
   keyframe id and the pixel) and leaves every output untouched. */
int deftri_init_depth_scales(deftri_ctx *ctx, int64_t kf_id_1, int64_t kf_id_2, int32_t n, const float *uv1,
                             const float *uv2, const float *x3d_1, const float *x3d_2, const float *kb8_1,
                             const float *kb8_2, const float *T1w, const float *T2w, float min_cos,
                             uint8_t *keep, double *scale_1, double *scale_2, int64_t *n_points);

/* ---- from keypoints to correspondences: the two steps in front of reconstructPoints ----------- */
/* The feature grid of a Frame (Frame.cc:213-250).  Without Camera.k1 the bounds are 0, 0, Camera.cols,
   Camera.rows (:222-227).  scale_factor: FeatureExtractor.fScaleFactor, n_scales: .nScales
   (vScaleFactor_[0] = 1, [i] = [i-1] * fScaleFactor in float, :65-70). */
typedef struct deftri_feature_grid {   /* Frame.cc:213-250 */
    int32_t cols, rows;                /* FeatureGrid.nGridCols / nGridRows */
    float min_col, min_row, max_col, max_row;
    int32_t n_scales; float scale_factor;
} deftri_feature_grid;

/* searchForInitializaion(refFrame, currFrame, th, windowSizeFactor, vMatches)
   (Modules/Matching/DescriptorMatching.cc:39-99).  Frame 1 is the reference frame, frame 2 the current
   one: uv [n*2] keypoints, octave [n], desc [n*32] the 256-bit descriptors.  matches[i] = the current
   keypoint matched to reference keypoint i, or -1; best_dist / second_dist (each may be NULL) the two
   smallest Hamming distances among the candidates of i, 255 where there is none (the reference's start
   values; also for a reference keypoint of octave > 0, which is not searched); *n_matches the
   reference's return value.  Restated as it stands:
     - only reference keypoints of octave <= 0 are searched (:56); radius = windowSizeFactor * 1 *
       getScaleFactor(octave); candidates are getFeaturesInArea(x, y, radius, octave - 1, octave + 1)
       (Frame.cc:288-323): the cell range from four posInGrid calls that fall back to 0 / size - 1 when
       they fail, then octave in range and |dx| < radius && |dy| < radius, strict, in float;
     - posInGrid (Frame.cc:277-286) rounds (half away from zero) to a cell index and a current keypoint is
       in the grid only if its own posInGrid succeeds (:204-210): one in the last half cell on the right
       or at the bottom (x >= 1428.75 on 1440 columns and 64 cells) is in no cell, never a candidate;
     - best and second start at 255, so a distance of 255 or 256 never becomes the best; accepted when
       bestDist <= th && (float)bestDist < float(secondBestDist) * 0.9 — a tie for best rejects;
     - nothing makes the matches one-to-one.
   The result does not depend on the order the candidates are visited in; the device (cell lists as a
   CSR, one 64-lane wave per reference keypoint) equals the sequential host loop exactly.  A host-only
   context runs that loop.  n1 == 0 or n2 == 0 returns 0 with every entry -1 and *n_matches 0.
   DEFTRI_E_ARG with a message: cols or rows <= 0 (or more than 2^24 cells), max <= min, n_scales < 1, an
   octave outside [0, n_scales) (the reference would index vScaleFactor_ out of range), a null required
   pointer. */
int deftri_match_for_initialization(deftri_ctx *ctx, const deftri_feature_grid *grid,
        int32_t n1, const float *uv1, const int32_t *octave1, const uint8_t *desc1,   /* n1 x 32 */
        int32_t n2, const float *uv2, const int32_t *octave2, const uint8_t *desc2,
        int32_t th, float window_size_factor,
        int32_t *matches /* n1, -1 = none */, int32_t *best_dist, int32_t *second_dist /* may be NULL */,
        int32_t *n_matches);

/* The vTriangulated mask MonocularMapInitializer::initialize builds with Triangulation.checks
   (MonocularMapInitializer.cc:93-104) for n matched pixel pairs.  findEssentialWithRANSAC (:119-178)
   builds the same E = [t]x R of T12 = T1w * T2w^-1 (computeEssentialMatrixFromPose, Geometry.cc:239-256)
   in each of its 16 iterations (computeE is commented out), so its result is one
   computeScoreAndInliers (:206-223): per match, in float, r = unproject(uv).normalized() of both views,
   r1_hat = (E r1).normalized(), err = |float(pi/2) - acos(r1_hat . r2.normalized())|, inlier = err <
   epipolar_th (Epipolar.th).  *score = the inliers; a score of 0 leaves vBestInliers empty in the
   reference: nothing is triangulated.  err may be NULL.  T1w, T2w: row-major 3x4.  n < 8 returns
   DEFTRI_E_ARG: cv::kmeans refuses fewer samples than its 8 clusters and the reference throws.  A
   host-only context runs the sequential loop of the same functions. */
int deftri_epipolar_inliers(deftri_ctx *ctx, int32_t n, const float *uv1, const float *uv2,
        const float *kb8_1, const float *kb8_2, const float *T1w, const float *T2w,
        float epipolar_th, uint8_t *inlier, float *err /* may be NULL */, int32_t *score);

/* ---- the second pose from the matches alone: E by RANSAC, then the cameras --------------------- */
typedef struct deftri_essential_report {
    int32_t n_matches, n_hypotheses;
    int32_t n_degenerate;                /* hypotheses flagged degenerate (below) */
    int32_t best;                        /* the hypothesis kept, -1 when every score is 0 */
    int32_t best_score;                  /* nInliers (:175) */
    int32_t round_trips;                 /* blocking device-to-host copies: 1 (0 on a host-only context) */
    double ms_rays, ms_models, ms_score; /* the stages: device events around the kernels (k_best counts as score),
                                            the host clock on a host-only context */
    double ms_total;                     /* host clock over the call */
} deftri_essential_report;

/* findEssentialWithRANSAC (MonocularMapInitializer.cc:119-178) with the model the reference left commented
   out (:158): per hypothesis computeE (:180-203) of its 8 matches, computeScoreAndInliers (:206-223)
   against all n matches, and the first E of the highest score (:167-171).  uv1 / uv2 [2 * n] the matched
   pixel pairs; samples int32 [n_hyp * 8] the eight match indices of each hypothesis in the order the
   reference's loop would draw them.  The draws are an input: the reference takes them from cv::kmeans
   under OpenCV's RNG and random_shuffle under srand(10) (:125-155), neither of which is restated.
   Outputs: E_best [9] row-major, inlier [n], and (each may be NULL) err [n], scores [n_hyp], E_all
   [n_hyp * 9], degenerate [n_hyp], report.
     - Rays: unproject(uv).normalized() in float (:79-80), once per match.
     - Model: A (8 x 9) with row i = [r1_i * r2_i.x, r1_i * r2_i.y, r1_i * r2_i.z]; e = the right singular
       vector of its smallest singular value as a row-major 3 x 3; Ef = U diag(1, 1, 0) V^T of e; E = -Ef.
       Instead of the two JacobiSVDs: the null vector of A by elimination with complete pivoting (rank 8
       leaves an exact one-dimensional null space) and Ef = e (v1 v1^T / s1 + v2 v2^T / s2) from the two
       largest eigenpairs (s_i^2, v_i) of e^T e, all in fp64 from the float rays without contraction; E is
       rounded to float at the end (the reference's is a Matrix3f).
     - Sign: an SVD leaves the null vector's sign open.  Here its component of largest magnitude is
       positive (the lowest index on ties), then E = -Ef.  The score does not depend on it.
     - A hypothesis is degenerate when its sample repeats an index, a sampled ray is not finite, a pivot of
       the elimination is exactly zero, the second singular value of e is exactly zero, or E is not finite.
       It is flagged, its E_all row is zero, it scores 0 and is never the best.
     - Score: per match |float(pi/2) - acos((E r1).normalized() . r2.normalized())| < epipolar_th, the
       arithmetic of deftri_epipolar_inliers.
     - Best: replaced on score > bestScore from 0, so the lowest index among the highest scores.  When
       every score is 0: report.best = -1, E_best is zero, every inlier is 0 (the reference's empty
       vBestInliers) and err is NaN.  Otherwise inlier and err are those of E_best.
   The device scores every hypothesis against every match at once (integer counts: the result does not
   depend on the order) with one upload and one download; a host-only context runs the same functions as
   sequential loops.  The model arithmetic is the same on both, the rays differ where the two libm's sinf /
   cosf do.  DEFTRI_E_ARG with a message: n < 8 (as deftri_epipolar_inliers), n_hyp < 1, a sample index
   outside [0, n), a null required pointer. */
int deftri_find_essential_ransac(deftri_ctx *ctx, int32_t n, const float *uv1, const float *uv2,
        const float *kb8_1, const float *kb8_2, int32_t n_hyp, const int32_t *samples, float epipolar_th,
        float *E_best /* [9] */, uint8_t *inlier /* [n] */,
        float *err, int32_t *scores, float *E_all, uint8_t *degenerate /* may be NULL */,
        deftri_essential_report *report /* may be NULL */);

/* reconstructCameras (MonocularMapInitializer.cc:246-262) over decomposeE (:264-279) for the matches with
   use[i] != 0 (use [n] may be NULL: all of them), their rays built as reconstructEnvironment does
   (:228-237).  The reference unprojects both views with its single calibration_; a caller who wants
   exactly that passes the same kb8 twice.  E [9] row-major; T2w [12] the row-major 3 x 4 (Rgood, t); *away
   the vote.
     - R1 = U W^T V^T and R2 = U W V^T of E's SVD, each negated when its determinant is negative; Rgood = R2
       if trace(R2) > trace(R1), else R1.  As a set {R1, R2} does not depend on the freedom in U and V.
     - t = U.col(2).normalized(), whose sign the SVD leaves open; the vote depends on it ((R r1 - r2) . (r2 -
       t) is not odd in t).  Here: the unit left null vector of E with its component of largest magnitude
       positive (the lowest index on ties).
     - away = sum over the matches of sign((Rgood r1 - r2) . (r2 - t)), in float per match, an integer sum;
       t is negated when away is negative (signbit, :259).
   The decomposition runs on the host in fp64 from the float E (the two largest eigenpairs of E^T E, u_i =
   E v_i / s_i, u3 = u1 x u2) and is rounded to float; the vote is a kernel on a device context, the
   sequential loop on a host-only one.  DEFTRI_E_ARG with a message: n < 0, a null required pointer, an E
   with fewer than two non-zero singular values or a non-finite entry.  n == 0 returns (Rgood, +t) and
   away 0. */
int deftri_reconstruct_cameras(deftri_ctx *ctx, int32_t n, const float *uv1, const float *uv2,
        const float *kb8_1, const float *kb8_2, const uint8_t *use /* may be NULL */, const float *E,
        float *T2w /* [12] */, int32_t *away);

/* TEST ONLY: the cell lists of n keypoints as deftri_match_for_initialization builds them for the current
   frame (the device's CSR on a device context, Frame::distributeFeatures' grid on a host-only one):
   cell_start [cols*rows + 1], the keys of cell (col, row) at cell_keys[cell_start[col*rows + row] ..
   cell_start[col*rows + row + 1]); cell_keys [n], of which the first cell_start[cols*rows] are written.
   The order inside a cell is not defined on the device. */
int deftri_debug_feature_grid_cells(deftri_ctx *ctx, const deftri_feature_grid *grid, int32_t n, const float *uv,
        int32_t *cell_start, int32_t *cell_keys);

/* ---- the frame the matchers read: undistorted keys, grid bounds and cell lists ------------------- */
/* cv::undistortPoints(src, dst, K, dist, R = empty, P = K) with its default termination (5 iterations,
   count only), as Frame::undistortKeys calls it (Frame.cc:252-275), for n points: uv_in / uv_out [2 * n]
   pixels, calib [4] = fx, fy, cx, cy (calibration_->getParameter(0..3)), dist [n_dist] = k1, k2, p1, p2
   [, k3] (Camera.k1, k2, p1, p2, k3; n_dist 4 or 5, k3 = 0 with 4).  OpenCV's function is restated from
   its definition and has not been run against an OpenCV build.  Per point, in double from the floats,
   one rounding per operation (no contraction), on host and device:
       ifx = 1.0 / fx;  ify = 1.0 / fy;  x0 = (u - cx) * ifx;  y0 = (v - cy) * ify;  x = x0;  y = y0
       5 times:  r2 = x*x + y*y;  icdist = 1.0 / (1 + ((k3*r2 + k2)*r2 + k1)*r2)
                 if icdist < 0:  x = x0; y = y0; stop
                 dX = 2*p1*x*y + p2*(r2 + 2*x*x);  dY = p1*(r2 + 2*y*y) + 2*p2*x*y
                 x = (x0 - dX) * icdist;  y = (y0 - dY) * icdist
       out = (float(x*fx + cx), float(y*fy + cy))
   Kept as it stands: 5 iterations whether or not they have converged; double inside, float out; ifx a
   reciprocal that is multiplied by; a negative icdist gives the point up and returns the round trip of
   its distorted position, float(x0*fx + cx), which need not be u; all-zero coefficients still run the
   path; a NaN propagates.  The rational (k4..k6), thin-prism and tilt terms are absent: the reference
   never passes more than 5 coefficients.  The device runs one thread per point with one upload and one
   blocking download; a host-only context runs the sequential loop; the two are equal bit for bit.  n == 0
   writes nothing.  uv_in == uv_out is allowed (the reference calls it in place).
   DEFTRI_E_ARG with a message: a null required pointer, n < 0, n_dist not 4 or 5, fx or fy zero or not
   finite (the reference would divide by it). */
int deftri_undistort_points(deftri_ctx *ctx, int32_t n, const float *uv_in, const float *calib /* [4] */,
        const float *dist, int32_t n_dist, float *uv_out);

/* Frame::computeImageBoundaries (Frame.cc:221-250): bounds [4] = minCol_, minRow_, maxCol_, maxRow_.
   n_dist == 0 (no Camera.k1): 0, 0, cols, rows, and calib / dist may be NULL.  Otherwise the corners
   (0, 0), (cols, 0), (0, rows), (cols, rows) as float go through deftri_undistort_points' function to o0..o3
   and min_col = min(o0.x, o2.x), min_row = min(o0.y, o1.y), max_col = max(o1.x, o3.x), max_row = max(o2.y,
   o3.y).  Four points: computed on the host on every context.  DEFTRI_E_ARG with a message: a null
   required pointer, n_dist not 0, 4 or 5, fx or fy zero or not finite while n_dist > 0, max <= min after
   undistortion (also a bound that is not a number). */
int deftri_image_bounds(deftri_ctx *ctx, int32_t cols, int32_t rows, const float *calib, const float *dist,
        int32_t n_dist, float *bounds /* [4] */);

/* What Frame's constructor and Frame::distributeFeatures (Frame.cc:46-50, :188-211) make of the n keypoint
   slots FAST::extract filled, in one call:
     1. *grid: the bounds of deftri_image_bounds for (cols, rows) = (Camera.cols, Camera.rows) with grid_cols,
        grid_rows (FeatureGrid.nGridCols / nGridRows), n_scales and scale_factor as given: what every
        matcher takes; the two inverse cell sizes follow from it in float as initializeGrid computes them;
     2. uv [2 * n]: Frame::undistortKeys of uv_dis [2 * n] (deftri_undistort_points), or a copy of it when
        n_dist == 0.  Every slot is undistorted, also the zeros behind the extracted keypoints of a frame
        with nFeatures slots, as the reference's loop over all of vKeysDis_ does.  uv == uv_dis is allowed;
     3. grid_[col][row] as a CSR: cell_start [grid_cols * grid_rows + 1], cell (col, row) holding the
        keypoint indices cell_items[cell_start[col * grid_rows + row] .. cell_start[col * grid_rows + row + 1])
        in keypoint order, as push_back leaves them; cell_items [n], -1 behind the last list; in_grid [n]
        (may be NULL) 1 where the slot's own posInGrid is true.  A slot is stored only there: the rounding
        and the last-half-cell behaviour are those of deftri_match_for_initialization, and an undistorted
        position that rounds to column or row -1, or is NaN, is in no cell.
   The device undistorts a slot, finds its cell and counts the cell in one launch, then builds the lists
   with the kernels the matchers build theirs with and puts each list into keypoint order; the keys do
   not travel to the host in between; one upload and one blocking download.  A host-only context runs the
   sequential loops; every output is equal bit for bit.  n == 0 writes *grid and a cell_start of zeros.
   DEFTRI_E_ARG with a message, every output untouched: a null required pointer, n < 0, n_dist not 0, 4
   or 5, fx or fy zero or not finite while n_dist > 0, grid_cols or grid_rows <= 0 or more than 2^24 cells,
   max <= min after undistortion, n_scales < 1. */
int deftri_distribute_features(deftri_ctx *ctx, int32_t grid_cols, int32_t grid_rows, int32_t n_scales,
        float scale_factor, int32_t cols, int32_t rows, const float *calib, const float *dist, int32_t n_dist,
        int32_t n, const float *uv_dis, float *uv /* out */, deftri_feature_grid *grid /* out */,
        int32_t *cell_start /* out, grid_cols * grid_rows + 1 */, int32_t *cell_items /* out, n */,
        uint8_t *in_grid /* out, n, may be NULL */);

/* ---- map points into a frame by projection: what poseOnlyOptimization's frame is filled by -------- */
typedef struct deftri_projection_report {
    int32_t n_points;                    /* points (searchWithProjection) or reference slots (guidedMatching) */
    int32_t n_matches;                   /* the reference's return value: status 0 */
    int32_t n_view_cos, n_inv_dist;      /* its vCos and invDist counters: status 1 and 2 */
    int32_t n_no_candidates;             /* status 3 */
    int32_t n_rejected;                  /* status 4 */
    int32_t n_undefined;                 /* status 5 */
    int32_t rounds;                      /* claim-resolution rounds on the device (1 on a host-only context) */
    int32_t round_trips;                 /* blocking device-to-host copies: one flag per round, then the results (0 on a host-only context) */
    int32_t reserved;
    double ms_setup;                     /* host clock: checks, allocation, uploads and the grid and point kernels enqueued */
    double ms_rounds;                    /* host clock over the rounds, each with its flag read (the whole loop on a host-only context) */
    double ms_total;                     /* host clock over the call */
} deftri_projection_report;

/* searchWithProjection(currFrame, th, vMapPoints) (Modules/Matching/DescriptorMatching.cc:164-253).  The
   frame: its feature grid, Tcw (row-major 3x4), kb8, n2 keypoints uv2 [2 * n2], octave2 [n2], desc2 [32 * n2]
   and slot_point [n2], in and out: -1 a free slot, anything else a slot occupied before the call (-2 by
   convention), which keeps its value; on return a slot claimed by this call holds the index of its map
   point.  The n map points: pos [3 * n], normal [3 * n], min_dist / max_dist [n] (the scale-invariance
   distances), desc [32 * n], as deftri_map_point_descriptors gives them.  Per point: match [n] the slot or -1,
   status [n], and (each may be NULL) uv [2 * n] the projection, view_cos [n], predicted_octave [n] (-1 where
   status is 1 or 2), best / second [n] (255 where nothing was compared).  report may be NULL.
   Status: 0 matched, 1 viewCos < 0.5, 2 outside [min_dist, max_dist], 3 no candidate in the window,
   4 candidates but no accepted best, 5 undefined in the reference (below): not searched, claims nothing.
   Restated as it stands, in float, one rounding per operation:
     - rayWorld = X - Tcw^-1.translation(); viewCos = rayWorld.normalized() . normal (Eigen's normalized()
       returns the vector itself when its squared norm is not positive); viewCos < 0.5: status 1 (:180);
     - dist = |rayWorld|; dist < min || dist > max: status 2 (:190);
     - predictedOctave = (int)ceil(log(max / dist) / log(getScaleFactor(1))), the float overloads of log and
       ceil, clamped to [0, nScales] (:197-200): the upper end is nScales, not nScales - 1, and at nScales the
       reference reads vScaleFactor_[nScales], past its end: status 5 (a NaN ratio, which has no int value,
       too).  A non-finite projection is status 5 as well: posInGrid converts it to int;
     - uv = project(Tcw X), with no depth test (:203-204); radius = getScaleFactor(predictedOctave) * (viewCos
       > 0.998 ? 2.5 : 4.0), the comparison and the product in double (:206-210);
     - candidates = getFeaturesInArea(uv, radius, predictedOctave - 1, predictedOctave + 1) with the rounding
       and last-half-cell behaviour of deftri_match_for_initialization; none: status 3 (:220), decided
       before the slots are looked at;
     - a candidate whose slot is occupied is skipped entirely: neither best nor second (:230-232);
     - best and second start at 255; accepted iff best <= th && (float)best < float(second) * 0.9 (a tie for
       best rejects); then slot_point[bestIdx] = i (:246-249), else status 4.
   uv and view_cos are written for every point, also where the reference never computes them.
   The skip makes point i depend on the claims of every accepted point before it.  The device resolves
   that in rounds and equals the sequential loop for every input: claim[j] is the lowest index of a point
   that claimed keypoint j in the previous round (-1 occupied before the call, INT_MAX free); in a round
   every point (one wave each) computes its result over the candidates with claim[j] >= its own index;
   accepted points enter the next round's table by atomicMin; the rounds end when no point's accepted
   keypoint changed.  After round r points 0 .. r - 1 hold their sequential results and keep them (point k
   skips j exactly when some claimant below k exists, and the claimants below k are final), so the fixed
   point is unique, is the loop's result, and is reached in at most n rounds plus the one that sees no
   change; a round's result does not depend on the order the candidates are visited in (an accepted best
   is strictly below the second).  More than n + 1 rounds: DEFTRI_E_INTERNAL.  One 4-byte flag is read
   back per round.  A host-only context runs the reference's loop.  The two context kinds use different
   libm (atan2f, sinf, cosf, logf), so uv differs by ulps and a decision can differ where an input sits within
   those ulps of a threshold.
   DEFTRI_E_ARG with a message: n_scales < 2 (getScaleFactor(1)), an octave of a keypoint outside [0,
   n_scales), the grid errors of deftri_match_for_initialization, a null required pointer.  n == 0 or
   n2 == 0 writes nothing beyond the report. */
int deftri_search_with_projection(deftri_ctx *ctx, const deftri_feature_grid *grid, const float *Tcw, const float *kb8,
        int32_t n2, const float *uv2, const int32_t *octave2, const uint8_t *desc2, int32_t *slot_point /* [n2] in/out */,
        int32_t n, const float *pos, const float *normal, const float *min_dist, const float *max_dist,
        const uint8_t *desc /* n x 32 */, int32_t th,
        int32_t *match /* [n] */, uint8_t *status /* [n] */,
        float *uv, float *view_cos, int32_t *predicted_octave, int32_t *best, int32_t *second /* may be NULL */,
        deftri_projection_report *report /* may be NULL */);

/* guidedMatching(refFrame, currFrame, th, vMatches, windowSizeFactor) (DescriptorMatching.cc:101-162).  The
   current frame as above, but every slot starts free (clearMapPoints, :102): slot_point [n2] is output
   only and holds the REFERENCE SLOT whose map point now sits in the slot, or -1.  The reference frame: n1
   slots with has_point [n1] (0: the slot holds no map point and is passed over, :112), and for the slots
   that hold one pos [3 * n1] the map point's world position, octave1 [n1] the reference keypoint's octave,
   desc [32 * n1] the map point's own descriptor.  The points are taken in slot order.  Per slot: matches
   [n1] the current slot or -1 (-1 for a slot without a map point), status [n1] as above with 6 = no map
   point in the slot, and (each may be NULL) uv, best, second.  There is no view-cosine, distance or
   octave-prediction step: the octave is octave1[i], radius = float(15 * windowSizeFactor) *
   getScaleFactor(octave) — windowSizeFactor is an int, so the product is an integer — and the levels are
   octave +- 1.  The skip rule, the acceptance, the claim and its resolution on the device are those of
   deftri_search_with_projection; the kernel is the same.  DEFTRI_E_ARG as there (n_scales < 1 instead of
   2), and for window_size_factor outside [0, 2^20].  n1 == 0 or n2 == 0 writes nothing beyond the report. */
int deftri_guided_matching(deftri_ctx *ctx, const deftri_feature_grid *grid, const float *Tcw, const float *kb8,
        int32_t n2, const float *uv2, const int32_t *octave2, const uint8_t *desc2, int32_t *slot_point /* [n2] out */,
        int32_t n1, const uint8_t *has_point, const float *pos, const int32_t *octave1, const uint8_t *desc /* n1 x 32 */,
        int32_t th, int32_t window_size_factor,
        int32_t *matches /* [n1] */, uint8_t *status /* [n1] */, float *uv, int32_t *best, int32_t *second /* may be NULL */,
        deftri_projection_report *report /* may be NULL */);

/* Map::updateOrientationAndDescriptor (Modules/Map/Map.cc:270-321) for n map points: pos [3 * n]; their
   observations as a CSR, obs_start [n + 1] into obs_kf / obs_slot (keyframe index, keypoint slot).  The
   reference visits mMapPointObs_[mp], an unordered_map, in libstdc++'s iteration order: this entry takes
   the observations in the order it is given, and the caller provides that order (deftri_keyframe_order of
   the keyframe ids in insertion order gives it).  The n_kf keyframes: kf_Tcw [12 * n_kf] row-major 3x4,
   their slots concatenated, kf_slot_start [n_kf + 1] into kf_desc [32 * slots] and kf_octave [slots];
   n_scales and scale_factor give vScaleFactor_ as in deftri_feature_grid.  Per point: normal [3 * n],
   max_dist / min_dist [n], desc [32 * n], ref_obs [n] the ordinal of the chosen observation, status [n].
   Restated as it stands, in float:
     - normal = sum over the observations, in order, of (X - Tcw^-1.translation()).normalized(), divided by
       the count and normalized (:286-293);
     - all pairwise Hamming distances; per observation the element nth_element puts at nObs / 2: the
       (nObs / 2)-th smallest counting from 0, the self-distance 0 included (:299-303);
     - the first observation whose median is strictly below the running best wins; the running best starts
       at 255.0f, so medians of 255 or 256 leave obsIdx = 0 (:296-307);
     - dist = |X - centre of the chosen keyframe|; maxDist = dist * getScaleFactor(refOctave), minDist =
       maxDist / getScaleFactor(nScales - 1) (:311-315);
     - KEPT QUIRK: refOctave is read from keypoint obsIdx of the chosen keyframe (:312), obsIdx being the
       observation's ordinal, not its slot.
   status 0 written; 1 no observation (the reference indexes an empty vector): the point's outputs are
   not written, ref_obs -1.  An ordinal beyond the chosen keyframe's slots is DEFTRI_E_ARG (the outputs are
   then undefined), as are an observation that names no keyframe or slot, an octave outside [0, n_scales),
   n_scales < 1, and a null required pointer.  On the device one wave per map point: the lanes stride over
   the observation pairs, and the median comes from counting (a 257-bin histogram per observation), not
   sorting.  desc, ref_obs and status equal a host-only context's; normal and the distances are the same
   float expressions.  n == 0 writes nothing. */
int deftri_map_point_descriptors(deftri_ctx *ctx, int32_t n, const float *pos, const int32_t *obs_start,
        const int32_t *obs_kf, const int32_t *obs_slot,
        int32_t n_kf, const float *kf_Tcw, const int32_t *kf_slot_start, const uint8_t *kf_desc, const int32_t *kf_octave,
        int32_t n_scales, float scale_factor,
        float *normal, float *max_dist, float *min_dist, uint8_t *desc, int32_t *ref_obs, uint8_t *status);

/* ---- growing the map past two keyframes: searchForTriangulation and fuse ------------------------- */
typedef struct deftri_triangulation_match_report {
    int32_t n1, n2;
    int32_t n_matches;                   /* the reference's return value: rows of status 0 */
    int32_t n_occupied;                  /* status 1 */
    int32_t n_unmatched;                 /* status 2 */
    int32_t n_stolen;                    /* status 3 */
    int32_t n_flag_skipped;              /* status 4 */
    int32_t flag_row;                    /* the row accepted at distance exactly 2 that set vbMatched2[2]; -1: none */
    int64_t n_listed;                    /* pairs in the device's candidate lists (0 on a host-only context) */
    int32_t round_trips;                 /* blocking device-to-host copies: 1, or 2 when the lists outgrew the first buffer (0 on a host-only context) */
    int32_t reserved;
    double ms_device;                    /* host clock: checks, uploads, kernels and the download */
    double ms_loop;                      /* host clock over the sequential loop (the whole search on a host-only context) */
    double ms_total;                     /* host clock over the call */
} deftri_triangulation_match_report;

/* searchForTriangulation(kf1, kf2, th, fEpipolarTh, E, vMatches) (Modules/Matching/DescriptorMatching.cc:255-328).
   Keyframe 1: n1 keypoints uv1 [2 * n1], desc1 [32 * n1], has_point1 [n1] (non-zero: the slot already holds a
   map point); keyframe 2 likewise.  One kb8: the reference unprojects both frames with kf1's calibration
   (:267).  E [9] row-major.  Outputs: matches [n1] the keypoint of keyframe 2 or -1; best_dist [n1] (may be
   NULL) the distance a row was accepted at, 255 where it never was; status [n1]; *n_matches; report (may be
   NULL).  Status: 0 matched, 1 slot occupied, not searched, 2 no eligible candidate below th, 3 matched, then
   un-matched by a later row that took its keypoint (best_dist keeps the distance), 4 passed over by the flag
   quirk.  Restated as it stands:
     - rows in order; row i is searched only if has_point1[i] == 0 (:277);
     - ray1 = (E * unproject(uv1_i)).normalized(), the unprojected ray not normalized first (:282);
     - bestDist starts at 255; candidates j in order; skipped if has_point2[j] != 0 (:288), if dist > 50 or
       dist > bestDist (:293), or if vMatchedDistance[j] <= dist (:296); only then ray2 =
       unproject(uv2_j).normalized() and the epipolar test, and only a pass sets bestDist = dist, bestIdx = j;
     - the test: float err = fabs(M_PI/2 - acos(ray2.dot(ray1))) < fEpipolarTh.  The dot product is a float
       and acos its float overload (the file is `using namespace std`); M_PI/2 is a double, so the difference
       and fabs are double, rounded to float when stored in err; the comparison is float.  This is not
       computeScoreAndInliers' float(pi/2) - acos(.) in float (deftri_epipolar_inliers).  normalized() is
       Eigen's (a vector whose squared norm is not positive is returned as it is); a NaN compares false, so a
       non-finite ray fails every test;
     - bestDist moves only on a pass, so a row's result does not depend on the order of j: it is the minimum
       dist over the j that pass every test, the LARGEST such j among equals (an equal distance replaces);
     - accepted iff bestDist < th, strictly (:310).  Then vMatchedDistance[bestIdx] = bestDist, and a row
       that held bestIdx before loses it (matches -1, *n_matches one less): the steal, always by a strictly
       smaller distance.  A robbed row does not search again;
     - SIZES: the reference sizes vMatchedDistance and vnMatches21 by n1 and indexes them by j.  Here they
       have n2 elements: identical for n2 <= n1, and a definition where the reference writes past its vectors;
     - KEPT QUIRK (flag_quirk != 0): vbMatched2 is read as vbMatched2[2] for every j and written as
       vbMatched2[bestDist] = true, so the whole vector is one boolean: some earlier row was accepted at
       distance exactly 2.  From then on every j is passed over and no row matches: status 4; the report
       names the row that set it.  (For n2 <= 2 the reference reads past the vector; here the boolean stands
       for it.)  flag_quirk == 0 ignores the vector; vMatchedDistance already makes the result one-to-one.
   On a device context: a ray kernel (one thread per keypoint of either frame); a candidate kernel, one wave
   per searched row, that lists the pairs with a free slot, dist <= min(50, th - 1) and a passed epipolar test
   (a pair with dist >= th can only raise a bestDist that is not accepted) compacted per row in ascending j,
   sized by a count pass and a scan; one download; then the loop above over the lists, whose remaining tests
   are dist > bestDist and vMatchedDistance.  The first fill pass has room for 64 n1 + 4096 pairs; only a
   call with more takes a second fill pass into a buffer of the exact size and a second download
   (round_trips 2).  The result equals a host-only context's loop over all pairs for every input, except
   where err sits within the two libm's ulps (sinf, cosf, acosf) of epipolar_th.
   DEFTRI_E_ARG with a message: th > 255 (a row without candidate would pass bestDist < th and the reference
   uses an uninitialised bestIdx), n1 < 0 or n2 < 0, a null required pointer.  n1 == 0 or n2 == 0 returns 0
   with every match -1. */
int deftri_search_for_triangulation(deftri_ctx *ctx, int32_t n1, const float *uv1, const uint8_t *desc1,
        const uint8_t *has_point1, int32_t n2, const float *uv2, const uint8_t *desc2, const uint8_t *has_point2,
        const float *kb8, const float *E /* [9] */, int32_t th, float epipolar_th, int32_t flag_quirk,
        int32_t *matches /* [n1] */, int32_t *best_dist /* [n1], may be NULL */, uint8_t *status /* [n1] */,
        int32_t *n_matches, deftri_triangulation_match_report *report /* may be NULL */);

/* The search of fuse(pKF, th, vMapPoints, pMap) (DescriptorMatching.cc:330-428) for n map points against the
   keyframe, given as the frame of deftri_guided_matching (grid, Tcw, kb8, uv2, octave2, desc2).  Inside fuse
   the search for point i does not depend on earlier iterations — no candidate is skipped because its slot is
   taken — only the map edits are sequential, and those stay with the caller.  Per point: consider [n] (0: the
   point is passed over, status 6), pos [3 * n], octave [n] (the reference reads pKF->getKeyPoint(i).octave,
   the list index used as a keypoint index, :366: the caller passes what it wants read), desc [32 * n].
   Outputs: match [n] the accepted keypoint or -1, status [n], and (each may be NULL) uv [2 * n], best, second
   [n], report with rounds = 1.
     - uv = project(Tcw X), no depth test (:362-363); a non-finite projection is status 5;
     - radius = (float)(2.5 * (double)getScaleFactor(octave)) (:369), levels octave +- 1;
     - getFeaturesInArea with the rounding and last-half-cell behaviour of deftri_match_for_initialization;
       no candidate: status 3 (:375);
     - best and second start at 255; accepted iff best <= th && (float)best < float(second) * 0.9, else
       status 4 (a best of 255 or more leaves bestIdx unset, :400, and is rejected by the same test).
   The kernel is deftri_search_with_projection's with every slot free, run once; one blocking copy.  An
   octave outside [0, n_scales) on a considered point or on a keypoint is DEFTRI_E_ARG, as are the grid
   errors and a null required pointer.  n == 0 or n2 == 0 writes nothing beyond the report. */
int deftri_fuse_search(deftri_ctx *ctx, const deftri_feature_grid *grid, const float *Tcw, const float *kb8,
        int32_t n2, const float *uv2, const int32_t *octave2, const uint8_t *desc2,
        int32_t n, const uint8_t *consider, const float *pos, const int32_t *octave, const uint8_t *desc /* n x 32 */,
        int32_t th, int32_t *match /* [n] */, uint8_t *status /* [n] */, float *uv, int32_t *best,
        int32_t *second /* may be NULL */, deftri_projection_report *report /* may be NULL */);

/* ---- from an image to keypoints: FAST::extract (Modules/Features/FAST.cc:81-118, FAST.h:52-97) --- */
#define DEFTRI_FAST_MAX_LEVELS 16
typedef struct deftri_fast_params {
    int32_t n_scales; float scale_factor;   /* FeatureExtractor.nScales / .fScaleFactor */
    int32_t n_max_features;                 /* nMaxFeatures_: the reference passes 2 * nFeatures (Mapping.cc:46) */
    int32_t th_fast, min_th_fast;           /* 10 and 4 there */
    int32_t max_keys;                       /* the capacity of the caller's vKeys: nFeatures (Frame.cc:36) */
} deftri_fast_params;

typedef struct deftri_fast_report {
    int32_t n_levels, n_keys;
    int32_t level_cols[DEFTRI_FAST_MAX_LEVELS], level_rows[DEFTRI_FAST_MAX_LEVELS];
    int32_t features_per_level[DEFTRI_FAST_MAX_LEVELS];   /* vFeaturesPerLevel_ */
    int32_t n_candidates[DEFTRI_FAST_MAX_LEVELS];         /* vToDistributeKeys */
    int32_t n_octree[DEFTRI_FAST_MAX_LEVELS];             /* distributeOctTree's result */
    int32_t n_after_mask[DEFTRI_FAST_MAX_LEVELS];         /* ... of which outside the dilated mask */
    int32_t n_fallback_cells[DEFTRI_FAST_MAX_LEVELS];     /* cells redone at min_th_fast */
    int32_t n_empty_cells[DEFTRI_FAST_MAX_LEVELS];        /* ... of which still empty */
    int32_t n_truncated[DEFTRI_FAST_MAX_LEVELS];          /* unmasked keypoints past max_keys */
    int32_t round_trips;                 /* blocking device-to-host copies of the call (0 on a host-only context) */
    int32_t reserved;
    double ms_resize, ms_cells;          /* device: the kernels' time between events (the resize with its uploads) */
    double ms_octree, ms_keypoints;      /* host clock: the octree; the mask reads, orientation and assembly */
    double ms_total;                     /* host clock over the call */
} deftri_fast_report;

/* FAST::extract of an 8-bit single-channel image [rows x cols, row stride in bytes], restated as it
   stands.  border_mask: FeatureExtractor.imageBoderMask decoded by the caller (uint8, the image's size),
   or NULL for the reference's empty imread.  Outputs, each of capacity max_keys, in the reference's
   order (level by level, inside a level distributeOctTree's list after the mask filter): uv [2 * n]
   = pt * vScaleFactor_[octave], octave, angle (degrees), response, size = int(31 * vScaleFactor_[level]);
   *n_keys the number written.  report may be NULL.
     1. Scale tables and vFeaturesPerLevel_ (FAST.h:54-78) in float; cvRound rounds half to even.
     2. Pyramid (FAST.cc:120-139): level 0 is the image, level l = cv::resize(level l - 1,
        Size(cvRound(cols * inv[l]), cvRound(rows * inv[l])), INTER_LINEAR); the 19-pixel reflected border
        is never read by extract and is not built.  The resize is OpenCV's 8-bit fixed-point bilinear:
        scale = src / dst in double; per destination index d, f = float((d + 0.5) * scale - 0.5),
        s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0, both taps on that
        pixel; weights (cvRound((1 - f) * 2048), cvRound(f * 2048)); h = S[s] * a0 + S[s + 1] * a1 in int;
        dst = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.  A level that halves the one
        above it exactly on both axes takes OpenCV's area path instead: DEFTRI_E_ARG.
     3. Cells (:141-203): borders 16 and size - 16, W = 30, nCols, nRows, wCell, hCell, the + 6 overlap,
        the two `continue` tests and the clamps as written.  cv::FAST(cell, th, true) is FAST-9/16 on the
        cell alone with the cell's own 3-pixel margin excluded: with s the maximum over the 16 arcs of 9
        contiguous ring pixels of the arc's minimum of p_i - c, and the same of c - p_i, the pixel is a
        corner at t iff s > t, its response is s - 1, and it is kept iff that is strictly greater than
        the responses of its 8 neighbours (0 for one that is no corner at t or lies in the margin);
        row-major.  A cell with nothing at th_fast is redone whole at min_th_fast (:189-193).  Suppression
        and fallback are per cell: this is not one FAST over the image.
     4. distributeOctTree (:243-434) and DivideNode (:24-79), sequential, on the host for both context
        kinds: nIni = round(width / height), the integer truncations of the node corners, push_front,
        the two termination tests, the first maximum response per node.  The reference sorts
        pair<int, ExtractorNode*> and so breaks equal sizes by address; here the most recently created
        node goes first (what increasing allocation addresses would give) — a choice.
     5. Mask (:223-234, :470-528): base = image > 240, OR border_mask; level i's mask is its dilation
        by side x side, side = ceil(2^(i+1) * float(2.5 / 1.5)) * 2 + 5, read at (cvRound(y), cvRound(x))
        in level coordinates on the full-resolution mask (kept).  A keypoint is dropped iff a base-mask
        pixel lies in its window clipped to the image; an integral image of the base mask answers that.
     6. IC_Angle (:443-467) with umax_ (FAST.h:82-96): integer moments over the radius-15 patch, then
        cv::fastAtan2(float(m_01), float(m_10)): c = min / (max + float(DBL_EPSILON)), the odd polynomial
        with 57.283627, -18.667446, 8.9140005, -2.5397246, then 90 - a, 180 - a, 360 - a; float, one
        rounding per operation on host and device.
     7. Assembly (:98-117): pt *= vScaleFactor_[octave], levels in order, stop at max_keys.
   OpenCV's parts of 2, 3 and 6 are restated from their definitions and have not been run against an
   OpenCV build.  A device context equals a host-only one bit for bit.  DEFTRI_E_ARG with a message: a
   null required pointer, a level below 62 pixels a side (the reference divides by nCols = 0), stride <
   cols, n_scales outside [1, 16], scale_factor <= 1, thresholds outside 1 <= min_th_fast <= th_fast <=
   255, max_keys < 0, n_max_features < 0, a border mask of another size (cv::bitwise_or throws), a level
   whose round(width / height) is 0 (the reference divides by it).  max_keys == 0 returns no keypoints
   (the outputs may then be NULL). */
int deftri_fast_extract(deftri_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t stride,
        const uint8_t *border_mask /* may be NULL */, int32_t mask_rows, int32_t mask_cols, int32_t mask_stride,
        const deftri_fast_params *params,
        float *uv, int32_t *octave, float *angle, float *response, float *size, int32_t *n_keys,
        deftri_fast_report *report /* may be NULL */);

/* TEST ONLY: one pyramid level's pixels as deftri_fast_extract builds them, packed: out [at most rows *
   cols], *out_rows x *out_cols written. */
int deftri_debug_fast_pyramid(deftri_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t stride,
        const deftri_fast_params *params, int32_t level, uint8_t *out, int32_t *out_rows, int32_t *out_cols);
/* TEST ONLY: one level's candidates in front of distributeOctTree (vToDistributeKeys, :197-199), in the
   reference's order: xy [2 * max_cand] relative to the 16-pixel border, response [max_cand]; *n the
   number found, of which the first min(*n, max_cand) are written. */
int deftri_debug_fast_candidates(deftri_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t stride,
        const deftri_fast_params *params, int32_t level, int32_t max_cand, int32_t *xy, float *response, int32_t *n);
/* TEST ONLY: level `level`'s dilated mask (0 .. 15: only the side depends on it) read at n positions
   xy (x, y) inside the image, by the method deftri_fast_extract uses: hit [n], 1 = masked. */
int deftri_debug_fast_mask(deftri_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t stride,
        const uint8_t *border_mask /* may be NULL */, int32_t mask_rows, int32_t mask_cols, int32_t mask_stride,
        int32_t level, int32_t n, const int32_t *xy, uint8_t *hit);

/* ---- from keypoints to descriptors: ORB::describe (Modules/Features/ORB.cc:20-90, ORB.h:34-68) ---- */
typedef struct deftri_orb_params {
    int32_t n_scales; float scale_factor;   /* FeatureExtractor.nScales / .fScaleFactor */
} deftri_orb_params;

typedef struct deftri_orb_report {
    int32_t n_levels, n_keys;
    int32_t level_cols[DEFTRI_FAST_MAX_LEVELS], level_rows[DEFTRI_FAST_MAX_LEVELS];   /* without the border */
    int32_t n_outside;                   /* keypoints with status 1 */
    int32_t round_trips;                 /* blocking device-to-host copies of the call (0 on a host-only context) */
    double ms_pyramid, ms_describe;      /* device: the kernels' time between events (host clock on a host-only context) */
    double ms_total;                     /* host clock over the call */
} deftri_orb_report;

/* The sampling pattern of ORB::describe: 512 points as xy [1024] = x0 y0 x1 y1 ..., in the order of the
   reference's bit_pattern_31_ (ORB.h:70-328), which this library does not carry: the caller passes its own
   copy.  Comparison c of the descriptor reads points 2c and 2c + 1.  Kept on the context as int8 pairs
   and uploaded to its device once; a later call replaces it.  DEFTRI_E_ARG with a message: a null
   pointer, a coordinate outside [-15, 15] (the 31-pixel patch). */
int deftri_orb_set_pattern(deftri_ctx *ctx, const int32_t *xy /* [1024]: x0 y0 x1 y1 ... */);

/* ORB::describe of n keypoints (uv [2 * n] in full-resolution pixels, octave [n], angle [n] in degrees, as
   deftri_fast_extract returns them) on an 8-bit single-channel image [rows x cols, row stride in bytes],
   restated as it stands: desc [n * 32], status [n] (0 described; 1 the reference would read memory it
   does not own, the descriptor is zero).  report may be NULL.
     1. Scale tables (ORB.h:39-49) in float: vScaleFactor_[0] = 1, [i] = [i - 1] * scale_factor, inv[i] =
        1.0f / vScaleFactor_[i].  cvRound rounds half to even.
     2. Pyramid (ORB.cc:32-52), which is not deftri_fast_extract's: per level l the interior has the size
        (cvRound((float)cols * inv[l]), cvRound((float)rows * inv[l])), from the original image at every
        level.  Level 0's interior is the image; level l's is cv::resize(level l - 1's interior, INTER_LINEAR)
        of the BLURRED level l - 1 (the blur is in place, so it cascades), by the 8-bit fixed-point bilinear
        of deftri_fast_extract 2. (a level that halves the one above it exactly on both axes: DEFTRI_E_ARG).
        The 19-pixel border (EDGE_THRESHOLD) on all sides is BORDER_REFLECT_101 of that unblurred interior
        (-k -> k, n - 1 + k -> n - 1 - k).  Then GaussianBlur(interior, interior, Size(7, 7), 2, 2,
        BORDER_REFLECT_101) in place on the interior only: it reads up to 3 pixels of the border just
        written, so it equals a reflect-101 blur of the unblurred interior, and the border keeps the
        unblurred reflections, which descriptor samples that fall there read (kept).
     3. The blur this call takes in OpenCV: the source is a sub-matrix and the border type is not
        isolated, so the bit-exact 8-bit Gaussian is not taken and the call goes to the generic separable
        filter with getGaussianKernel(7, 2, CV_32F) = exp(-x^2 / 8), x = -3 .. 3, normalized in double and
        stored as float; for 8-bit data and a symmetric smoothing kernel both 1-D kernels become int by
        cvRound(k * 256) = 18 34 49 55 49 34 18 (sum 257); the row pass is an int32 sum of 7 products, the
        column pass an int32 sum of 7 products of row results, then (s + 32768) >> 16 saturated to [0, 255].
     4. Per keypoint (ORB.cc:24-29, 54-66): x = uv.x * inv[octave], y = uv.y * inv[octave] in float, the centre
        (cvRound(y), cvRound(x)) in level pixels; angle_r = angle * (float)(CV_PI / 180.f); a = (float)
        cos((double)angle_r), b = (float)sin((double)angle_r), by the host's libm for both context kinds
        (whether the reference's unqualified cos(float) is cosf or cos depends on its headers: the double
        form is a choice).  Pattern point (px, py) is read at row offset cvRound(px * b + py * a) and column
        offset cvRound(px * a - py * b), in float, one rounding per operation, no contraction.
     5. Bits (:66-87): byte i bit j = sample(16 i + 2 j) < sample(16 i + 2 j + 1).
     6. status 1: any of the 512 sample positions outside [-19, cols_l + 19) x [-19, rows_l + 19) of the
        keypoint's level, decided on the rounded float values before the conversion to int (a non-finite
        coordinate or angle lands here).
   OpenCV's parts of 2 and 3 are restated from their definitions and have not been run against an OpenCV
   build.  A device context equals a host-only one bit for bit; it makes one upload (image, keypoints and
   resize tables in one copy) and one blocking download (descriptors and status).  DEFTRI_E_ARG with a
   message: a null required pointer, stride < cols, n_scales outside [1, 16], scale_factor <= 1, an octave
   outside [0, n_scales), a level with a side below 20 (reflect-101 by 19 needs it), no pattern set, n < 0.
   n == 0 writes nothing (the arrays may then be NULL). */
int deftri_orb_describe(deftri_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t stride,
        const deftri_orb_params *params, int32_t n, const float *uv, const int32_t *octave, const float *angle,
        uint8_t *desc /* [n * 32] */, uint8_t *status /* [n] */, deftri_orb_report *report /* may be NULL */);

/* TEST ONLY: one level of deftri_orb_describe's pyramid WITH its 19-pixel border, packed: out [(level rows
   + 38) * (level cols + 38)] (at most (rows + 38) * (cols + 38)); *out_rows x *out_cols are the bordered
   sizes.  Needs no pattern. */
int deftri_debug_orb_pyramid(deftri_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t stride,
        const deftri_orb_params *params, int32_t level, uint8_t *out, int32_t *out_rows, int32_t *out_cols);
/* TEST ONLY: the integer 1-D kernel of 3., as the library computes it from that definition: k [7]. */
int deftri_debug_orb_blur_kernel(int32_t *k);

/* Build the flattened graph only (no solve): the arrays are owned by the context and stay
   valid until the next call on it.  Used by the parity tests to compare indexing. */
/* MapPoint id of every point vertex of the last graph deftri_arap_build_graph built (n = its
   n_points): the write-back key of :974-990. */
int deftri_arap_graph_point_ids(const deftri_ctx *ctx, int64_t *ids, int64_t n);
/* Graph builds of this context so far answered by the memo (the same map: NLopt's clones) and by
   the structure memo (deformationOptimization's next round: positions, depth scales and T_g moved,
   every pair's Delaunay triangulation still valid — the values refreshed in place, the descriptor
   equal bit for bit to a full build's), and the host time of the last build in ms. */
int deftri_graph_stats(const deftri_ctx *ctx, int64_t *memo_hits, int64_t *struct_hits, double *ms_last);
/* Full graph builds' keyframe meshes that were repaired from the previous build's triangulation of
   the same vertices (Lawson flips with exact predicates, then the same strict uniqueness check as the
   structure memo — so the mesh equals a new Delaunay triangulation triangle for triangle) instead of
   triangulated anew, and the flips they took, over this context's life. */
int deftri_graph_repairs(const deftri_ctx *ctx, int64_t *meshes, int64_t *flips);

/* ---- the Delaunay mesh on the device: one star per wave (delaunay_dev.hip) -------------- */
typedef struct deftri_delaunay_report {
    int32_t n_tris;                      /* triangles written to tris */
    int32_t hull_size;                   /* convex-hull vertices */
    int32_t skipped;                     /* duplicate points the triangulation left out (a fallback's) */
    int32_t path;                        /* 0 the host sweep (delaunay.cpp), 1 stars on the host, 2 stars on the device */
    int32_t host_stars;                  /* stars the device marked (an uncertain predicate, more than 64
                                            triangles) and the host rebuilt with exact predicates; n on path 1 */
    int32_t fallback;                    /* why the host sweep ran: 0 it did not, 1 a tie (a zero predicate), 2 a
                                            duplicate point, 3 more than max(64, n / 64) marked stars, 4 n < 3 */
    int32_t max_degree;                  /* the largest star (neighbours of one point); 0 after a fallback */
    int32_t round_trips;                 /* blocking device synchronisations of the call (1 on the device path) */
    double ms_grid, ms_stars, ms_host, ms_total;   /* device grid and star kernels (events), host resolution, the call */
} deftri_delaunay_report;                /* deftri_sizeof(24) */

/* The Delaunay triangulation of n points xy [2 * n] (x, y interleaved, double): tris [3 * n_tris], counter-
   clockwise, each triangle starting at its smallest vertex, sorted by (first, second, third) — the order and
   the triangles of the library's host sweep (delaunay2d), triangle for triangle, on every input.  Every point
   builds its own star from a uniform grid of about n cells: the nearest neighbour first, then the next
   neighbour counter-clockwise by the in-circle order, until the sweep closes or meets the hull; a point emits
   the triangles in which it is the smallest vertex.  On a device context one wave builds a star with the
   floating-point filters of the host's predicates; a star with a predicate inside its filter bound, or more than
   64 neighbours, is marked and rebuilt on the host with the exact predicates.  A host-only context builds every
   star with the exact predicates in a sequential loop.  A tie (a predicate that is exactly zero: cocircular or
   collinear points), a duplicate point, more than max(64, n / 64) marked stars or n < 3 run the host sweep
   instead, whose result (skipped included) is then returned; report->fallback says why.
   tris_cap: the triangles tris has room for; 2 * n is always enough.  One upload and one blocking download.
   DEFTRI_E_ARG with a message, outputs untouched: a null pointer, n < 0, a coordinate that is not finite,
   tris_cap below the number of triangles (the message names it).  DEFTRI_E_GRAPH: all points on a line (n >= 3);
   *report is written (fallback), tris is not.  n < 3 returns 0 with n_tris 0 and fallback 4. */
int deftri_delaunay2d(deftri_ctx *ctx, int32_t n, const double *xy, int32_t tris_cap, int32_t *tris /* out */,
        deftri_delaunay_report *report /* out */);
/* Who triangulates a keyframe's positions in deftri_arap_build_graph / _optimization when neither the graph
   memo nor the structure memo supplies the mesh: 0 (default) the host sweep, 1 deftri_delaunay2d's path on this
   context (the same triangles, so the same graph bit for bit).  deftri_graph_stats / _repairs keep their meaning. */
int deftri_set_mesh_builder(deftri_ctx *ctx, int32_t mode);

/* ---- as-rigid-as-possible mesh deformation (arap_deform.hip) ------------------------------
   Open3D's TriangleMesh::DeformAsRigidAsPossible restated (the local/global iteration of Sorkine and Alexa;
   not run against Open3D): the constraints C[cid[k]] = cpos[k] for k < min(n_cid, n_cpos) (a repeated id keeps
   its last position); edge weights w_ij the mean over the edge's opposite vertices of a.b / |a x b|, clamped at
   0; p = v, then max_iter times, always: the local step R_i = V diag(1, 1, det(V U^T)) U^T of S_i = sum_j w_ij
   (v_i - v_j)(p_i - p_j)^T = U S V^T (Smoothed, from the second iteration on: S = 2 S + (4 alpha area / nb_i)
   (sum_j R_old_j)^T), the global step L p = b with unit rows for the constrained vertices and b_i = sum_j
   (w_ij / 2)(R_i + R_j)(v_i - v_j), and the energy E = sum_i sum_j w_ij |(p_i - p_j) - R_i (v_i - v_j)|^2
   (Smoothed: + alpha area sum_i sum_j |R_i - R_j|_F^2), returned per iteration.
   The global step eliminates the constrained rows and solves the symmetric positive definite rest by a
   diagonally preconditioned CG over the three coordinate columns at once, from the previous iterate; a column
   stops when r.r <= cg_tol^2 b.b, tested before the first iteration too.  A device context keeps every array on
   the device for the whole call (one upload, one download; the host reads only the convergence flags); a
   host-only context runs the same arithmetic in plain loops.  Every sum over vertices is taken in a fixed
   order, so two calls with equal arguments give equal bits. */
typedef struct deftri_arap_deform_params {   /* deftri_sizeof(25) */
    int32_t max_iter;            /* Open3D default 50; the reference passes 500 */
    int32_t energy;              /* 0 Spokes, 1 Smoothed */
    double  smoothed_alpha;      /* 0.01 */
    double  cg_tol;              /* relative residual per column; <= 0 means 1e-12 */
    int32_t cg_max_iterations;   /* per global step; <= 0 means 10 n + 100 */
    int32_t reserved;
} deftri_arap_deform_params;

typedef struct deftri_arap_deform_report {   /* deftri_sizeof(26) */
    int32_t iterations, n_constraints, n_free, zero_weight_edges;
    int32_t cg_max_in_step, cg_unconverged_steps, on_device, reserved;
    int64_t cg_iterations;                   /* summed over steps and columns */
    double  energy_first, energy_last, area;
    double  ms_total, ms_local, ms_global;
} deftri_arap_deform_report;

/* DEFTRI_E_ARG: n < 3, a triangle or constraint index out of range, no effective constraint, max_iter < 0, an
   energy other than 0 or 1, a null required pointer.  DEFTRI_E_GRAPH (before any solve): a connected component
   of the positive-weight edges holds no constrained vertex (a vertex whose weights sum to 0 is such a
   component) — Open3D's factorization fails there, and CG would return an arbitrary translation of it.
   DEFTRI_E_NUMERIC: a non-finite iterate, det R <= 0, a global step that did not reach cg_tol within
   cg_max_iterations (counted in cg_unconverged_steps; *rep is filled up to that step).  On every error out and
   energies are untouched.  prm NULL: the defaults (50, Spokes, 0.01). */
int deftri_arap_deform(deftri_ctx *ctx, int32_t n, const double *vertices /*[3n]*/,
                       int32_t n_tris, const int32_t *tris /*[3 n_tris]*/,
                       int32_t n_cid, const int32_t *cid, int32_t n_cpos, const double *cpos /*[3 n_cpos]*/,
                       const deftri_arap_deform_params *prm,
                       double *out /*[3n]*/, double *energies /*[max_iter] or NULL*/,
                       deftri_arap_deform_report *rep);

/* arapOpen3DOptimization(Map*) (g2oBundleAdjustment.cc:1010-1104): per keyframe pair in the order of
   deftri_arap_optimization (keyframe 1 the later one), the Delaunay mesh of keyframe 1's positions (the mesh
   builder switch applies), createVectorMap and its inverse, then deftri_arap_deform with the reference's
   arguments — ten constraint ids 0, every position of keyframe 2 as constraint positions, 500 iterations,
   Spokes — and the reference's write-back: for every slot index below keyframe 1's slot count that the
   inverse map holds as a position index (the slot/compaction quirk, kept), keyframe 1's MapPoint of that slot
   takes float(mesh vertex) and then keyframe 2's takes float(deformed vertex); a MapPoint is one object, so
   each write reaches every slot with its id.  Pairs run in sequence on the updated positions.  DEFTRI_E_ARG: a
   found slot that is empty or past the end in either keyframe (the reference dereferences it).  The map is
   written only when every pair succeeded.  rep (may be NULL): the last pair's report. */
int deftri_arap_open3d_optimization(deftri_ctx *ctx, deftri_map *map, deftri_arap_deform_report *rep);
/* Who builds the iterative plan at the next deftri_problem_upload (and in the uploads inside
   deftri_arap_optimization / deftri_deformation_optimization): 0 (default) the host passes of
   csrc/spcg_plan.cpp; 1 the device stages of csrc/plan_dev.hip where they apply, the host passes elsewhere.
   The device stages apply on a device context of one rank to a problem of one keyframe pair, at most two depth
   scales and at least one ARAP edge whose upload asks for the tile layout (from 50,000 unknowns); with
   deftri_set_multi_pair_builder(1) to several pairs as well.  The plan is equal array for array.  DEFTRI_E_ARG: a mode other than 0 or 1.  A HIP error inside the builder fails the
   upload with DEFTRI_E_HIP. */
int deftri_set_plan_builder(deftri_ctx *ctx, int32_t mode);
/* Who cuts the one-pair tile layout (build_tiles, csrc/spcg_tile.cpp) wherever plan builder 1's device stages
   apply: 0 (default) the host; 1 the device stages of csrc/plan_dev.hip (groups and edges by group, the partition,
   entries and slots, cross slots), which also keep the groups and the tile-entry edge order on the device between
   the plan builder's stages.  The plan is equal array for array.  A graph build_tiles refuses (a keyframe-copy
   group of more than 2 rows, an edge whose copies lie in two groups or inside one group, a vertex with more than
   64 ARAP edges) is handed to the host's build_tiles after the device's rows, as with mode 0.  With plan
   builder 0, on a host-only context or where the plan builder does not apply it has no effect.  DEFTRI_E_ARG: a
   mode other than 0 or 1.  deftri_debug_plan_digest with mode 1 honours this setting. */
int deftri_set_tile_builder(deftri_ctx *ctx, int32_t mode);
/* Who builds the plan's phase-1 blocks and phase-2 wave layout (stages 7 and 8b of csrc/spcg_plan.cpp: dperm, blk,
   hv_blk, hv_blk_off; rowmap, woff, wsplit, pmap, pidx) wherever plan builder 1 and tile builder 1 both ran — the
   device built the tile layout, not refused: 0 (default) the host; 1 the device stages of csrc/plan_dev.hip.  In an
   upload the two slot arrays pmap and pidx then stay on the device and reach the solver by a device-to-device
   copy (with DEFTRI_PLAN_DIGEST=1 they are downloaded for the digest).  The plan is equal array for array.  The
   host builds stage 8b when 64 x its slot steps does not fit an int.  Anywhere else — plan or tile builder 0, a
   host-only context, a refused tile layout, a sharded context — it has no effect.  On more than one pair it acts
   only under deftri_set_multi_pair_builder(1), and then on stage 8b alone, whatever the tile builder says.
   DEFTRI_E_ARG: a mode other than 0 or 1.  A HIP error inside the builder fails the upload with DEFTRI_E_HIP.
   deftri_debug_plan_digest with mode 1 honours this setting; every array then comes back to the host. */
int deftri_set_layout_builder(deftri_ctx *ctx, int32_t mode);
/* Whether plan builder 1's device stages also take a problem of several keyframe pairs: 0 (default) no — such a
   plan is the host's, and deftri_plan_build_info says "not applicable"; 1 yes.  It applies where all of these
   hold: plan builder 1 and this switch at 1; a device context of one rank; more than one pair, at least one ARAP
   edge and fewer than 2^29, fewer than 2^21 cameras; an upload (or deftri_debug_plan_digest with tile = 1) that
   asks for the tile layout.  The device then builds the groups, their Morton order and the keyframe-major rows of
   a multi-pair tile plan — the points by (camera of the point's reprojection edges, curve key of the point's own
   position in that camera's box, point id), or the group order where a point's reprojection edges name two
   cameras — and, after build_tiles_multi, the rotation numbering, the reprojection / depth edges by row and the
   incidences (stages 0x3f).  build_tiles_multi (csrc/spcg_tile.cpp) stays on the host whatever
   deftri_set_tile_builder says (bits 6-9 come only with deftri_set_multi_tile_builder(1)); where it refuses the
   graph the host goes on from the device's rows (stages 0x7).  With deftri_set_layout_builder(1) stage 8b (rowmap, woff, wsplit, pmap, pidx) runs
   on the device too and an upload keeps pmap and pidx there (stages 0x183f: bits 11 and 12); stage 7 (dperm, blk,
   hv_blk, hv_blk_off) is the host's for several pairs, so bit 10 stays clear.  A row with more than 256
   incidences reaches the builder's bound: the whole plan is then the host's (reason 2).  The plan is equal array
   for array.  Anywhere else — one pair, where the other switches decide as before; a sharded or host-only
   context; plan builder 0; no tile request — it has no effect.  DEFTRI_E_ARG: a mode other than 0 or 1.  A HIP
   error inside the builder fails the upload with DEFTRI_E_HIP.  deftri_debug_plan_digest and
   deftri_debug_plan_layout_stats with mode 1 honour this setting. */
int deftri_set_multi_pair_builder(deftri_ctx *ctx, int32_t mode);
/* Who cuts the tile layout of several keyframe pairs (build_tiles_multi, csrc/spcg_tile.cpp) wherever
   deftri_set_multi_pair_builder(1)'s device stages apply: 0 (default) the host; 1 the device stages of
   csrc/plan_dev.hip — the (pair, group) units in each pair's own Morton order and the edges by unit (stages bit 6),
   the partition per pair (bit 7), entries, slots, own rows and shares (bit 8), cross slots (bit 9) — which also keep
   the groups and the tile-entry edge order on the device between the plan builder's stages: stages 0x3ff, 0x1bff with
   layout builder 1 (stage 7 stays the host's, bit 10 clear).  The plan is equal array for array.  A graph
   build_tiles_multi refuses (not two depth scales per pair, an edge inside one group, an edge's copies in two
   groups, a unit whose rows differ between its edges, a vertex with more than 64 ARAP edges in a pair, a depth edge
   outside its pair's mesh, a row in no pair's mesh) is handed to the host's build_tiles_multi after the device's
   rows, as with mode 0 (stages 0x7); so is one whose (pair, group) table has 2^28 entries or more, which the host
   then accepts (stages 0x3f).  A unit with more than 256 in-edges, or a row in more than 256 pairs, reaches the
   builder's bound (reason 2).  It is a switch of its own: deftri_set_tile_builder acts on one pair only.  Anywhere
   else — one pair, plan or multi-pair builder 0, a sharded or host-only context, no tile request — it has no effect.
   DEFTRI_E_ARG: a mode other than 0 or 1.  A HIP error inside the builder fails the upload with DEFTRI_E_HIP.
   deftri_debug_plan_digest, deftri_debug_plan_tile_digest and deftri_debug_plan_layout_stats with mode 1 honour this
   setting. */
int deftri_set_multi_tile_builder(deftri_ctx *ctx, int32_t mode);
/* What the last iterative plan build of this context did: builder_used 0 / 1; stages = bit mask of
   the stages that ran on the device (bit 0 groups, 1 Morton order, 2 rows, 3 rotation numbering,
   4 rep/depth by row, 5 incidences; with deftri_set_tile_builder(1) also 6 groups and edges by group,
   7 partition, 8 entries and slots, 9 cross slots: 0x3ff for a full device build; bits 0-2 alone: the tile
   layout was refused after them and the build went on on the host; with deftri_set_layout_builder(1) also
   10 phase-1 blocks, 11 row sort and wave cut, 12 slot fill, set only when those stages ran: 0x1fff for a full
   device build with all three switches; several pairs with deftri_set_multi_pair_builder(1): 0x3f built on the
   device, 0x183f with layout builder 1 — bits 6-10 stay with the host there — and 0x7 where build_tiles_multi
   refused; with deftri_set_multi_tile_builder(1) also bits 6 units and edges by unit, 7 partition, 8 entries, slots,
   own rows and shares, 9 cross slots: 0x3ff, 0x1bff with layout builder 1, bit 10 staying clear); reason = why builder_used is 0 although mode is 1 (0 none, 1 not applicable, 2 a bounded loop reached
   its bound); ms = wall time of the build.  All zero before the first build. */
int deftri_plan_build_info(const deftri_ctx *ctx, int32_t *builder_used, int32_t *stages,
                           int32_t *reason, double *ms);
/* Who runs the passes of a full ARAP graph build (deftri_arap_build_graph, deftri_arap_optimization; the branch
   taken when neither the graph memo nor the structure memo answers): 0 (default) the host; 1 the device stages of
   csrc/graph_build_dev.hip — the CSR adjacency, the vector map, the cot weights and rotations, the slot scan, the
   point numbering and the edges; the triangulation (deftri_set_mesh_builder) and the area sum stay where they
   are.  The graph is the host's, array for array.  It applies on a device context to a map with at least one
   pair whose MapPoint ids take the direct id table, whose meshes skip no point and whose counts fit an int32;
   anywhere else, and on a host-only context, the host build runs.  DEFTRI_E_ARG: a mode other than 0 or 1.  A
   HIP error inside the builder fails the call with DEFTRI_E_HIP. */
int deftri_set_graph_builder(deftri_ctx *ctx, int32_t mode);
/* What the last full graph build of this context did (a memo hit leaves it as it is): builder_used 0 / 1; stages =
   bit mask of the stages that ran on the device (bit 0 CSR adjacency, 1 vector map, 2 geometry, 3 slot scan,
   4 point numbering, 5 edges: 0x3f for a device build); reason = why builder_used is 0 although mode is 1 (0 none,
   1 not applicable, 2 an input error, which the host build reports, 3 a mesh the device stages hand back: an edge
   with more than two opposite corners, a row above the sort's bound); ms = wall time of the build.  All zero
   before the first full build. */
int deftri_graph_build_info(const deftri_ctx *ctx, int32_t *builder_used, int32_t *stages,
                            int32_t *reason, double *ms);
/* TEST: build the plan of `desc` as an upload of this context would, with builder `mode` and with
   the tile layout requested (tile = 1) or not, allocate no solver, and return one FNV-1a digest
   per plan array in the order of the DEFTRI_PLAN_DIGEST block of build_sp_plan (32: row_of_point,
   point_of_row, rank_row_begin, arap_ids, rep_ids, dep_ids, rot_ids, arap_rot_local, blk, hv_blk, hv_blk_off,
   dperm, inc_off, inc, rep_off, dep_off, rowmap, woff, wsplit, pmap, pidx, tile_tab, tile_m0, tile_m1,
   tile_chunk, tile_rs, tile_halo, tile_xoff, tile_xdst, send_rows, recv_rows, the scalars), then the combined
   digest that block prints.  *n receives the count (33); cap too small: DEFTRI_E_ARG.  Works on a host-only
   context (mode 1 is then not applicable).  deftri_plan_build_info afterwards describes this build. */
int deftri_debug_plan_digest(deftri_ctx *ctx, const deftri_problem_desc *desc, int32_t mode,
                             int32_t tile, uint64_t *digests, int32_t cap, int32_t *n);
/* TEST ONLY: build the plan exactly as deftri_debug_plan_digest does (the context's switches honoured) and return
   FNV-1a digests of what only a tile plan of several pairs holds and the 33 above leave out: tile_trow, tile_tdst,
   tile_poff, tile_nshare, the scalars {ntile, tile_entries, tile_cross, tile_segmax, tile_lds, tile_halo_rows,
   tile_planes, tile_multi} as int64, then their combination.  *n receives the count (6); cap too small:
   DEFTRI_E_ARG.  For a one-pair plan the four arrays are empty.  Works on a host-only context. */
int deftri_debug_plan_tile_digest(deftri_ctx *ctx, const deftri_problem_desc *desc, int32_t mode,
                                  int32_t tile, uint64_t *digests, int32_t cap, int32_t *n);
/* TEST ONLY: build the plan exactly as deftri_debug_plan_digest does and write 8 figures of its phase-1 blocks and
   wave layout, computed on the host from the finished plan: waves; waves with wsplit 1; waves whose 64-row
   look-ahead covers rows of two sort windows; waves with zero steps; the slot steps (woff's last entry); phase-1
   blocks; depth blocks among them; the largest hv_blk run.  cap < 8: DEFTRI_E_ARG.  Works on a host-only context. */
int deftri_debug_plan_layout_stats(deftri_ctx *ctx, const deftri_problem_desc *desc, int32_t mode, int32_t tile,
                                   int64_t *out, int32_t cap);
/* TEST ONLY: 1 when tris [3 * n_tris] is THE Delaunay triangulation of xy (delaunay_still_valid, the structure
   memo's exact certificate), else 0. */
int deftri_debug_delaunay_still_valid(int32_t n, const double *xy, int32_t n_tris, const int32_t *tris);
/* TEST ONLY: the host sweep itself (delaunay2d): returns n_tris, or DEFTRI_E_GRAPH for collinear input /
   n < 3, or DEFTRI_E_ARG when tris_cap is too small. */
int deftri_debug_delaunay_sweep(int32_t n, const double *xy, int32_t tris_cap, int32_t *tris, int32_t *hull_size,
        int32_t *skipped);
/* Keyframe pairs of the graphs this context builds (deftri_arap_build_graph / _optimization): 0
   (default) every pair (a, b > a) in map order, as the reference's loop (g2oBundleAdjustment.cc:
   640-645); w > 0 only pairs with b - a <= w (a sliding window: the documented deviation used for
   BASELINE C5's 20 keyframes, 19 consecutive pairs at w = 1). */
int deftri_set_pair_window(deftri_ctx *ctx, int32_t window);
int deftri_arap_build_graph(deftri_ctx *ctx, const deftri_map *map, double rep_weight,
                            double arap_weight, float depth_error,
                            const deftri_problem_desc **desc_out);

/* ---- deformationOptimization (g2oBundleAdjustment.cc:446-606), round 5 --------------------
   The outer loop in native code: rounds i = 1 .. n_optimizations while the last round's update
   sum ||p_old - p_new|| >= 1e-4 n_map_points (:482).  A round of selection 0 ("g2oArap") is one
   arapOptimization with the current weights; selection 1 ("twoOptimizations" + weightsSelection
   "nlopt", the Simulation.yaml default) first runs NLopt's LN_NELDERMEAD over (rep, global, arap)
   within [lb, ub] (xtol_rel, xtol_abs, maxeval; :486-530) — NLopt 2.x's nldrmd.c with its default
   initial step, elimdim and relstop restated (deftri/nlopt_nm.py is the same algorithm) — whose
   every evaluation is outerObjective (nloptOptimization.cc:4-37): arapOptimization on a clone of
   a clone of the map as the round started (:499, nloptOptimization.cc:13; Map::clone, Map.cc:30-58:
   here a copy of the positions and depth scales, the rest shared read-only — with the reference's
   two observable properties: the clone's global table is EMPTY, Map::clone does not copy
   mGTransformation_, so its pairs start T_g at the identity; and the clone iterates its keyframes
   in the order deftri_keyframe_order gives), then calculatePixelsStandDev
   on the device, f = log(desvc1)^2 + log(desvc2)^2; then arapOptimization on the map itself with
   the optimum, whose weights the next round starts from.  A search that ends on a failure code
   (nldrmd's degenerate initial simplex) returns DEFTRI_E_SEARCH before that round's
   arapOptimization (the reference's nlopt::opt::optimize throws there); weightsSelection "eigen"
   is selection 0: the reference's Eigen::LevenbergMarquardt::minimize returns
   ImproperInputParameters before evaluating anything (its functor declares 2 values for 3 inputs,
   m < n, EigenOptimization.h:31, g2oBundleAdjustment.cc:532-550) and the round runs
   arapOptimization with the unchanged weights.  The map's positions and depth scales are
   written back in place after every round and global_t holds the last T_g; the global table the
   next round reads is updated as Map::insertGlobalKeyFramesTransformation(0, 1, T) does
   (Map.cc:323-330: T and its fp32 inverse).  The Eigen-LM weight search (weightsSelection
   "eigen", EigenOptimization.h) is not built (its functor reads 3 of 2 declared inputs). */
typedef struct deftri_deformation_params {
    int32_t selection;            /* 0 g2oArap (fixed weights), 1 twoOptimizations + nlopt */
    double  rep, global, arap;    /* Optimization.* weights: the search's start */
    double  alpha, beta;          /* stored on the ARAP edges, unused by their error (as the reference) */
    float   depth_error;          /* sigma_d (m) */
    int32_t n_iterations;         /* LM iterations per arapOptimization (Optimization.numberOfIterations) */
    int32_t n_optimizations;      /* outer rounds at most (Optimization.numberOfOptimizations) */
    double  lb[3], ub[3];         /* nlopt bounds of (rep, global, arap) */
    double  xtol_rel, xtol_abs;   /* nlopt.relTolerance / absTolerance */
    int32_t maxeval;              /* nlopt.numberOfIterations */
    int32_t n_map_points;         /* |MapPoints| of the map (the stop test's scale) */
} deftri_deformation_params;
typedef struct deftri_deformation_eval {
    int32_t round, eval;          /* 1-based round, 1-based evaluation inside the round's search */
    double  x[3], f;              /* the weights evaluated and outerObjective's value */
} deftri_deformation_eval;
typedef struct deftri_deformation_report {
    int32_t rounds;               /* outer rounds run */
    int32_t arap_calls;           /* arapOptimization calls (evaluations + one per round) */
    double  weights[3];           /* the last round's weights */
    double  minf;                 /* the last search's best objective */
    int32_t nlopt_result;         /* the last search's result code (1 success, 4 xtol, 5 maxeval, -1 failure) */
    double  update;               /* the last round's update */
    double  seconds;              /* wall time of the call */
    deftri_deformation_eval *evals;   /* caller's buffer (may be NULL): every evaluation, in order */
    int32_t max_evals, n_evals;   /* its capacity; evaluations recorded (all, up to the capacity) */
    double  round_update[64];     /* per round (first 64): its update, */
    double  round_weights[64][3]; /* its weights */
} deftri_deformation_report;
int deftri_deformation_optimization(deftri_ctx *ctx, deftri_map *map, const deftri_deformation_params *params,
                                    deftri_deformation_report *report);
/* Map::insertGlobalKeyFramesTransformation(0, 1, T) of the map-level call's T_g (global_t):
   the (kf1, kf2) entry and its fp32 inverse for (kf2, kf1), each as the g2o::SE3Quat the next
   arapOptimization reads back (getGlobalKeyFramesTransformation, :664) — Sophus SE3f from the
   estimate cast to float (quaternion normalized in float), the inverse as the conjugate rotation and
   -(R^T t) by Eigen's quaternion-vector product, in float.  The one implementation the native outer
   loop and the host mirror's Map model both use.  No context, no GPU. */
int deftri_global_insert(const double t7[7], double fwd7[7], double inv7[7]);
/* The KeyFrame iteration order of Map::mKeyFrames_ (std::unordered_map<ID, KeyFrame_>, Map.h:185),
   which every reference loop over keyframes follows (:640-645, Geometry.cc:387): `insert_ids` in the
   order Map::insertKeyFrame was called; `clones` applications of Map::clone (Map.cc:30-58, which
   re-inserts the keyframes in the source's iteration order) after that.  Evaluated with the same
   standard-library container (libstdc++), not restated.  out[n]: ids in iteration order.  No GPU. */
int deftri_keyframe_order(const int64_t *insert_ids, int32_t n, int32_t clones, int64_t *out);
/* TEST ONLY (no GPU): the restated NLopt LN_NELDERMEAD on a caller objective f(x, n, user) over n <= 8
   dimensions — the search deftri_deformation_optimization runs.  x: in the start, out the best;
   *result the NLopt result code (1 success, 4 xtol reached, 5 maxeval reached, -1 failure), *minf,
   *nevals.  Returns 0, or DEFTRI_E_ARG (bad arguments, x0 outside the bounds). */
typedef double (*deftri_objective_fn)(const double *x, int32_t n, void *user);
int deftri_debug_nelder_mead(deftri_objective_fn f, void *user, int32_t n, double *x, const double *lb,
                             const double *ub, double xtol_rel, double xtol_abs, int32_t maxeval, double *minf,
                             int32_t *nevals, int32_t *result);

/* ==== bundle adjustment ============================================
 * The BlockSolver_6_3 Schur LM of the reference's BA entry points:
 *   bundleAdjustment(Map*)             g2oBundleAdjustment.cc:38-138   (optimize(20), KF 0 fixed)
 *   localBundleAdjustment(Map*, ID)    g2oBundleAdjustment.cc:245-444  (optimize(5), outlier
 *                                      levels, robust kernels off, optimize(10))
 *   poseOnlyOptimization(Frame&)       g2oBundleAdjustment.cc:140-243  (4 rounds x optimize(10))
 * Vertices: poses g2o::VertexSE3Expmap (6 dof, T <- exp(d) * T), points VertexSBAPointXYZ
 * (3 dof, marginalized).  Edges: EdgeSE3ProjectXYZ (g2oTypes.h:150-189, linearizeOplus
 * g2oTypes.cc:121-142) with info = invSigma2(octave) * I2 and optional Huber; with every point
 * fixed the edges are EdgeSE3ProjectXYZOnlyPose (g2oTypes.h:191-229, g2oTypes.cc:173-189).
 * On the device: per-edge residual/Jacobian, per-point 3x3 blocks, per-pose 6x6 blocks, the
 * Schur complement S = Hpp - sum_l Hpl Hll^-1 Hlp (dense, 6 x free poses), a dense LDL^T of S,
 * point back-substitution.  Points may be sharded over ranks (one rank per GPU): each rank
 * uploads every pose but only its points and their edges; the pose blocks and S are summed
 * across ranks (RCCL all-reduce, or a caller-provided all-reduce) once per LM trial. */
typedef struct deftri_ba_ctx deftri_ba_ctx;

typedef struct deftri_ba_desc {
    int32_t n_poses;             /* K  VertexSE3Expmap                                      */
    int32_t n_points;            /* P  VertexSBAPointXYZ (marginalized)                      */
    int32_t n_edges;             /* E  EdgeSE3ProjectXYZ                                     */
    int32_t reserved;
    const double  *poses;        /* [K*7] T_cw: qx qy qz qw tx ty tz                         */
    const uint8_t *pose_fixed;   /* [K] 1 = setFixed(true); NULL = none                      */
    const float   *pose_kb8;     /* [K*8] KannalaBrandt8 fx fy cx cy k0..k3 of each pose's KF */
    const double  *points;       /* [P*3] world positions                                   */
    const uint8_t *point_fixed;  /* [P] 1 = constant (poseOnly's Xworld); NULL = none        */
    const int32_t *edge_point;   /* [E] */
    const int32_t *edge_pose;    /* [E] */
    const double  *edge_obs;     /* [E*2] keypoint (u, v)                                   */
    const double  *edge_info;    /* [E]   information = edge_info * I2                      */
    const uint8_t *edge_level;   /* [E] g2o edge level; NULL = all 0                        */
    const uint8_t *edge_robust;  /* [E] 1 = RobustKernelHuber(huber_delta); NULL = all 1     */
    double huber_delta;          /* reference: (float)sqrt(5.99)                            */
} deftri_ba_desc;

/* Caller-supplied all-reduce over ranks (tests, non-RCCL transports): n doubles in HOST memory,
   reduced in place; op 0 = sum, 1 = max.  The library stages the device buffer through host
   memory around the call (the RCCL path reduces device-resident buffers directly).  Returns 0
   on success. */
typedef int (*deftri_allreduce_fn)(void *user, double *host_buf, int64_t n, int32_t op);

int deftri_ba_create(int32_t device, deftri_ba_ctx **out);
int deftri_ba_destroy(deftri_ba_ctx *ctx);
const char *deftri_ba_last_error(const deftri_ba_ctx *ctx);
/* Copy the graph to HBM (edges are kept in point order internally; per-edge in/out arrays of
   this API always use the caller's edge order). */
int deftri_ba_upload(deftri_ba_ctx *ctx, const deftri_ba_desc *desc);
/* vertex->setEstimate(): replace poses [K*7] and/or points [P*3] (NULL = unchanged). */
int deftri_ba_set_state(deftri_ba_ctx *ctx, const double *poses, const double *points);
/* e->setLevel() / e->setRobustKernel(0 or Huber) for every edge (NULL = unchanged). */
int deftri_ba_set_edge_flags(deftri_ba_ctx *ctx, const uint8_t *level, const uint8_t *robust);
/* optimizer.initializeOptimization(level); optimizer.optimize(params->n_iterations).  Active
   edges = level `level` with a non-fixed vertex; active vertices = those with an active edge. */
int deftri_ba_solve_lm(deftri_ba_ctx *ctx, const deftri_lm_params *params, int32_t level,
                       deftri_report *report);
/* e->computeError() on every edge (active or not) whose mask entry is non-zero (caller edge
   order; NULL = every edge). */
int deftri_ba_compute_errors(deftri_ba_ctx *ctx, const uint8_t *mask);
/* Per edge (caller order): e->chi2() of the cached error (no robust kernel) and
   e->isDepthPositive() at the current state.  Either output may be NULL. */
int deftri_ba_edge_chi2(deftri_ba_ctx *ctx, double *chi2, uint8_t *depth_positive);
/* Current estimates: poses [K*7], points [P*3] (either may be NULL). */
int deftri_ba_download(deftri_ba_ctx *ctx, double *poses, double *points);
/* Diagnostics (parity tests): initializeOptimization(level), linearize at the current state and
   form the damped Schur system at `lambda`.  Outputs (any may be NULL): chi2 (activeRobustChi2,
   summed over ranks), S [ns*ns] (row-major, full) and rhs [ns] of the reduced pose system, dx
   [6K + 3P] (poses in pose order, 0 for fixed/inactive; then points), b [6K + 3P] (g2o sign).
   *ns receives 6 x (number of free active poses). */
int deftri_ba_eval_system(deftri_ba_ctx *ctx, int32_t level, double lambda, double *chi2, double *S,
                          double *rhs, double *dx, double *b, int32_t *ns);
/* Point-sharded multi-GPU: this context is rank `rank` of `nranks`.  Either RCCL (the
   production path: ncclCommInitRank over xGMI, all-reduce on the solver stream; the 128-byte id
   comes from deftri_rccl_unique_id on rank 0, shared by the caller) or a caller-supplied
   all-reduce (tests: e.g. gloo through host memory).  nranks == 1 with a NULL id / fn clears the
   setting (an RCCL communicator of one rank is kept when an id is given). */
int deftri_rccl_unique_id(uint8_t id[128]);
int deftri_ba_dist_init_rccl(deftri_ba_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t id[128]);
int deftri_ba_dist_set_allreduce(deftri_ba_ctx *ctx, int32_t nranks, int32_t rank, deftri_allreduce_fn fn,
                                 void *user);
/* Per-kernel device timing of one LM trial of the BA path (HIP events on the solver stream). */
int deftri_ba_profile_trial(deftri_ba_ctx *ctx, double lambda, deftri_kernel_stat *stats, int32_t max_stats,
                            int32_t *n_stats);

#ifdef __cplusplus
}
#endif
#endif /* DEFTRI_H */
