/*
 * admm_tomo.h -- C-ABI of the MI355X-native decentralized-ADMM tomography hot path.
 *
 * The reference (prsinha1/Distributed-Inverse-Problem-Admm) is pure Python and
 * has no FFI.  Its hot-path boundary is two duck-typed Python functions:
 *
 *   build_node_problem(Ai, bi, rho, neighbor_terms, N, lam_tv, Qij_terms)
 *       -> /root/reference/block_5_node_problem.py:6-32
 *   decentralized_admm(A_dense_list, sinograms, G, Wi_list, Qij_diag_fn, N, ...)
 *       -> /root/reference/block_6_admm_loop_ver2.py:15-326
 *          (kwarg surface also of block_6_admm_loop.py:72-84)
 *
 * plus the operator they consume, the ODL ray transform materialised as a dense
 * matrix (block_2_load_odl_data.py:16-96), used only through `A @ x`,
 * `A.T @ r` and column norms (block_6_admm_loop_ver2.py:145,193;
 * block_3_graph_and_precisions.py:20-23).  The Python drop-ins in
 * distributed-inverse-problem-admm_amd/ call the entry points below through
 * ctypes.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers owned by the caller (PyTorch
 *     tensors).  The context owns only geometry tables and scratch.
 *   - Image layout: node-major, C-order pixels, x[v*N*N + i*N + j] <-> pixel
 *     (x_i, y_j) of ODL's uniform_discr([-1,-1],[1,1],[N,N]) (axis 0 = x).
 *   - Sinogram layout: node-major, angle-major: b[v*A*D + t*D + k]
 *     (block_6_admm_loop_ver2.py:46 flattens the (angles, det) sinogram in C order).
 *   - "sample" arrays (images given to the projector, sinograms) have the
 *     context dtype (ADMM_DTYPE_F32 or ADMM_DTYPE_F64); solver state
 *     (x, d, e, y, z, q, A^T b, sum q) is always float64.
 *   - Every call is stream-ordered and asynchronous on `stream` (a hipStream_t;
 *     NULL = default stream); nothing synchronises the host except
 *     admm_ctx_create / admm_ctx_destroy / admm_batch_bind.
 *   - Return 0 on success; a negative code on failure, with a message
 *     available from admm_last_error() (thread-local).
 *   - One context per device, used from one host thread.
 */
#ifndef ADMM_TOMO_H
#define ADMM_TOMO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADMM_ABI_VERSION 9

#define ADMM_OK 0
#define ADMM_E_INVALID (-1)
#define ADMM_E_HIP (-2)
#define ADMM_E_STATE (-3)

#define ADMM_DTYPE_F32 0
#define ADMM_DTYPE_F64 1

#define ADMM_TV_ISO 0
#define ADMM_TV_ANISO 1

/* edge fusion (admm_batch.fusion) */
#define ADMM_FUSE_MIDPOINT 0 /* z = (a_i + a_j)/2   (block_6_admm_loop_ver2.py:220-223, as run) */
#define ADMM_FUSE_WEIGHTED 1 /* z = (W_i a_i + W_j a_j)/(W_i + W_j)  (commented at _ver2:221-222;
                                ADMM_Algo.pdf eq.(2)); keeps both endpoint duals */

/* admm_batch.flags: x_ext's local rows are written only by admm_node_update (the caller
 * never changes x between updates), so an update may start from the previous update's
 * diagnostics instead of projecting x again. */
#define ADMM_BATCH_KEEP_X 1

/* per-node statistics written by admm_node_update (float64) */
#define ADMM_NODE_STAT_MSE_SINO 0 /* ||A x - b||^2           (block_6_admm_loop_ver2.py:190-194);
                                   * with ray weights: sum_r omega_r (A x - b)_r^2 */
#define ADMM_NODE_STAT_G2 1       /* ||g||^2 stationarity    (block_6_admm_loop_ver2.py:145-149) */
#define ADMM_NODE_STAT_TV 2       /* TV(x)                   (block_4_tv_helpers.py:5-14) */
#define ADMM_NODE_STAT_QUAD 3     /* sum_j rho/2 ||x-v_ij||^2_Q (block_5_node_problem.py:26-29); a batch
                                   * bound with a bound-constraint slot per node (admm_bound_project)
                                   * counts that incidence's term too: it is part of the subproblem */
#define ADMM_NODE_STAT_IMG 4      /* ||x - phantom||^2       (block_6_admm_loop_ver2.py:199-204) */
#define ADMM_NODE_STAT_SBRES2 5   /* ||A^T(Ax-b) + rho(D x - c) + mu K^T e||^2: stationarity of eq.(1)
                                     with the split-Bregman dual p = mu e / lam (ABI 3) */
#define ADMM_NODE_STATS 6

/* per-edge statistics written by admm_consensus (float64) */
#define ADMM_EDGE_STAT_RA2 0 /* ||x_a - z||^2 */
#define ADMM_EDGE_STAT_RB2 1 /* ||x_b - z||^2 */
#define ADMM_EDGE_STAT_DZ2 2 /* ||z_new - z_old||^2 */
#define ADMM_EDGE_STATS 3

/* Parallel-beam geometry of one graph node.  Replaces the ODL construction of
 * block_2_load_odl_data.py:16-65: space [-1,1]^2 (N x N), angles
 * uniform_partition(angle_min, angle_max, n_angles) midpoints, detector
 * uniform_partition(det_min, det_max, n_det) midpoints.  All nodes share it. */
typedef struct admm_geom {
    int32_t N;
    int32_t n_angles;
    int32_t n_det;
    int32_t reserved;
    double angle_min, angle_max;
    double det_min, det_max;
} admm_geom;

typedef struct admm_ctx admm_ctx;

/* The batch of graph nodes this device updates, their incident edges and the
 * solver parameters.  All pointers are device pointers. */
typedef struct admm_batch {
    int32_t V;        /* local graph nodes (rows 0..V-1 of x_ext) */
    int32_t n_xext;   /* rows of x_ext: local nodes + halo (neighbour) nodes */
    int32_t n_edges;  /* edge slots stored on this device */
    int32_t tv_iters; /* split-Bregman rounds per x-update (T_tv) */
    int32_t cg_iters; /* CG steps per round (K_cg) */
    int32_t tv_kind;  /* ADMM_TV_ISO / ADMM_TV_ANISO */
    double rho, lam, mu;

    double* x_ext;        /* [n_xext][n]  node images; rows < V updated in place   */
    double* d;            /* [V][2][n]    split variable d ~ Kx (warm state)        */
    double* e;            /* [V][2][n]    Bregman variable (warm state)             */
    const double* atb;    /* [V][n]       A^T b                                     */
    const double* dsum;   /* [V][n]       D_i = sum_j q_ij (setup data: also packed into the
                           * CG operator's sample layout at admm_batch_bind -- rebind
                           * after changing it)                                     */
    const void* b;        /* [V][m]       sinograms (context dtype)                 */
    const double* phantom;/* [n] or NULL  for ||x - phantom||^2                     */

    double* y;            /* [E][n] dual of the lower-numbered endpoint (y_ij,min)  */
    double* z;            /* [E][n] consensus z_ij; NULL (ABI 7, midpoint fusion): derived
                           * from x_prev below instead of stored                       */
    const double* q;      /* [Qslots][n] precision vectors                         */
    const int32_t* edge_a;    /* [E] x_ext row of the lower endpoint               */
    const int32_t* edge_b;    /* [E] x_ext row of the higher endpoint              */
    const int32_t* inc_off;   /* [V+1] CSR over local nodes of incident edge-ends  */
    const int32_t* inc_edge;  /* [nnz] edge slot                                   */
    const int32_t* inc_qslot; /* [nnz] q slot of q_ij seen from this node           */
    const int32_t* inc_sign;  /* [nnz] +1 if this node is the lower endpoint, else -1 */

    double* node_stats;   /* [V][ADMM_NODE_STATS] */
    double* edge_stats;   /* [E][ADMM_EDGE_STATS] */

    /* ABI 2: edge fusion.  MIDPOINT keeps the single-y form (y_ij,max = -y);
     * WEIGHTED needs y_b and w (both NULL for MIDPOINT). */
    int32_t fusion;       /* ADMM_FUSE_* */
    int32_t flags;        /* ADMM_BATCH_* (0 in ABI-2 callers that predate it: was reserved) */
    double* y_b;          /* [E][n] dual of the higher-numbered endpoint (y_ij,max)   */
    const double* w;      /* [n_xext][n] W of the node in each x_ext row (W_i, make_precisions) */

    /* ABI 7: derived consensus (midpoint fusion, z == NULL).  z_ij is never stored: by the
     * single-y invariant it is the midpoint of the two endpoint images of the last consensus
     * (block_6_admm_loop_ver2.py:210-223 with y_ij,i + y_ij,j = 0), so the library keeps
     * those images instead -- one row per x_ext row, not one per edge -- and forms
     * z_ij = (x_prev[a] + x_prev[b]) / 2 wherever z is read (neighbour gather, diagnostics,
     * the dual residual); admm_consensus sets x_prev = x_ext after its edge updates.
     * Zero-filled by the caller before the first iteration (z = 0, block_6_..._ver2.py:42). */
    double* x_prev;       /* [n_xext][n] or NULL (stored z)                            */
} admm_batch;

int admm_abi_version(void);
const char* admm_last_error(void);

/* Context: geometry tables + scratch.  dtype = ADMM_DTYPE_*.  max_images bounds
 * the batch size of the operator entry points below. */
int admm_ctx_create(admm_ctx** out, const admm_geom* geom, int dtype, int max_images, int device);
/* ABI 4: a context for an operator given as an explicit matrix instead of a geometry:
 * the reference's A_dense_list entries (block_2_load_odl_data.py:68-96 `_to_dense_matrix`,
 * loaded back at block_7_main.py:16-22 / block_3_graph_and_precisions.py:283-287).
 * HOST arrays: A (m x N*N, rows = sinogram entries in the layout above, columns = C-order
 * pixels) as CSR -- indptr[m + 1] (int64), indices[nnz] (int32), values[nnz] (float64,
 * rounded to the context dtype).  The library keeps A and A^T as device CSR; every entry
 * point below (operator, batch, consensus) works unchanged, with the projector replaced
 * by CSR products.  nnz < 2^31. */
int admm_ctx_create_matrix(admm_ctx** out, int N, int m, long long nnz, const long long* indptr,
                           const int* indices, const double* values, int dtype, int max_images, int device);
int admm_ctx_destroy(admm_ctx* ctx);

/* --- operator entry points (replace ODL RayTransform / dense A) ---------- */

/* sino[v] = A img[v] for v < nimg.  Replaces `Ai @ x`
 * (block_5_node_problem.py:21, block_6_admm_loop_ver2.py:193). */
int admm_project_fwd(admm_ctx* ctx, const void* img, void* sino, int nimg, void* stream);
/* img[v] = A^T sino[v].  Replaces `Ai.T @ r` (block_6_admm_loop_ver2.py:145). */
int admm_project_adj(admm_ctx* ctx, const void* sino, void* img, int nimg, void* stream);
/* W[p] = max(sum_r A[r,p]^2, 1e-12) (float64).  Replaces make_precisions'
 * column sums (block_3_graph_and_precisions.py:20-23, block_1_env_and_imports.py:16-18). */
int admm_column_norms_sq(admm_ctx* ctx, double* W, void* stream);
/* W[p] = max(sum_r w_r A[r,p]^2, 1e-12) (float64) for per-ray weights w: [m] in the context dtype
 * (the precisions of a weighted data term); all-ones w gives admm_column_norms_sq bitwise.  Setup
 * only.  Explicit-matrix contexts: ADMM_E_INVALID.  Additive: ADMM_ABI_VERSION stays 9. */
int admm_column_norms_sq_weighted(admm_ctx* ctx, const void* w, double* W, void* stream);
/* (gx, gy) = K x, forward differences (block_4_tv_helpers.py:17-23), float64. */
int admm_tv_grad(admm_ctx* ctx, const double* x, double* gx, double* gy, int nimg, void* stream);
/* out = K^T (px, py), exact adjoint of admm_tv_grad (block_4_tv_helpers.py:25-35). */
int admm_tv_div(admm_ctx* ctx, const double* px, const double* py, double* out, int nimg,
                void* stream);

/* --- node batch (replaces the node loop + CVXPY/SCS solve and the edge updates) --- */

/* Bind a batch (pointers are captured; the contents may change between calls).
 * Allocates scratch and records the update sequence as a hipGraph.  Synchronous. */
int admm_batch_bind(admm_ctx* ctx, const admm_batch* batch);
/* A^T b for the bound batch (setup; writes batch->atb, which is then const).  With ray weights
 * set (admm_batch_set_ray_weights): A^T (omega b), the product rounded once in the context dtype. */
int admm_batch_atb(admm_ctx* ctx, double* atb_out, void* stream);
/* Per-ray weights of the bound batch: every node then solves eq.(1) with the data term
 * 1/2 sum_r omega_r (A x - b)_r^2 (weighted least squares; omega = 0 masks a ray).  w: [V][m] in the
 * context dtype, finite and >= 0 (the caller's promise), copied into the library's own buffer, packed
 * in the layout of the sinogram scratch; NULL clears the weights.  The weight is applied where the
 * forward projection is written (A x -> omega A x, A x - b -> omega (A x - b): no extra launch), so the
 * back projectors form A^T Omega A; call admm_batch_atb afterwards for A^T Omega b.  Re-records the
 * batch's sequences; synchronous like admm_batch_bind, which drops the weights (set them again after
 * every bind).  ADMM_NODE_STAT_MSE_SINO becomes sum_r omega_r (A x - b)_r^2; admm_time_forward /
 * admm_time_back time the weighted launches.  All-ones weights give bitwise the unweighted results.
 * Explicit-matrix contexts: ADMM_E_INVALID (scale the rows of A and b by sqrt(omega) there).
 * Additive: ADMM_ABI_VERSION stays 9. */
int admm_batch_set_ray_weights(admm_ctx* ctx, const void* w, void* stream);
/* New values for the weights of a bound batch that already has some (ADMM_E_STATE otherwise;
 * explicit-matrix contexts: ADMM_E_INVALID): w ([V][m], context dtype, not NULL) is packed into the
 * library's own buffer by the set call's launch, on `stream`, and the kept A^T s is dropped.  Nothing
 * else: no synchronisation and no re-recording -- the recorded sequences hold the weighted launches and
 * read that buffer by a pointer that does not move while the batch stays bound.  Follow it with
 * admm_batch_atb.  The next admm_node_update is bitwise that of a batch given the same weights by
 * admm_batch_set_ray_weights.  Additive: ADMM_ABI_VERSION stays 9. */
int admm_batch_update_ray_weights(admm_ctx* ctx, const void* w, void* stream);
/* For a batch bound with ADMM_BATCH_KEEP_X whose kept A^T s admm_batch_update_ray_weights has just dropped
 * (ADMM_E_STATE otherwise): the kept A^T s formed again under the new weights, from the samples of the
 * last update's x that the library still holds, by that update's own epilogue launches on `stream` -- the
 * forward projection with the weighted residual and the back projection -- without touching node_stats.
 * The next admm_node_update then starts from the kept A^T s as it does in a run whose weights never
 * change, instead of projecting x again; if the new weights equal the old ones bit for bit, so does the
 * kept A^T s and with it that update.  No synchronisation, nothing re-recorded.  Additive:
 * ADMM_ABI_VERSION stays 9. */
int admm_batch_refresh_kept(admm_ctx* ctx, void* stream);
/* One x-update of every bound node: neighbour gather v_ij = z_ij - y_ij,i
 * (y_ij,i = y for the lower endpoint, -y or y_b for the higher one),
 * fixed-count split-Bregman/CG solve of eq.(1), diagnostics into node_stats.
 * Replaces block_6_admm_loop_ver2.py:81-197 (build_node_problem + SCS + g check). */
int admm_node_update(admm_ctx* ctx, void* stream);
/* admm_node_update with `tv_iters` split-Bregman rounds instead of the bound count
 * (warm-started from the current x, d, e: k calls of r rounds continue one solve of
 * k*r rounds up to rounding).  The chunked solves of block_6_admm_loop.py:14-69
 * (_scs_solve_in_chunks) use it between snapshots.  ABI 3. */
int admm_node_update_rounds(admm_ctx* ctx, int tv_iters, void* stream);
/* Edge updates z = (a_i + a_j)/2 (or the W-weighted mean, ADMM_FUSE_WEIGHTED),
 * y += x - z at both ends, and the residual partial sums
 * into edge_stats.  Replaces block_6_admm_loop_ver2.py:210-253.  Every edge
 * slot of the batch is processed; x_ext halo rows must be current. */
int admm_consensus(admm_ctx* ctx, void* stream);
/* Average duration (ms) of a launch of the forward projector's tap kernel (k_fwdg,
 * which makes every sample tap; its segment partial sums are not combined) on the
 * bound batch, timed with HIP events on `stream`.
 * in_solve = 0: `reps` back-to-back launches on the batch's current x (the image
 *   rows stay in L2 from one launch to the next).
 * in_solve = 1 (ABI 5): one x-update of the bound batch is enqueued directly (the
 *   launch sequence its graph replays) with events around each CG step's forward
 *   tap launch -- right after the CG / TV update that wrote p and p^T, as in every
 *   solve; the batch's state advances by that x-update.  `reps` is ignored.
 * Measurement helper for bench.py; synchronises. */
int admm_time_forward(admm_ctx* ctx, int reps, int in_solve, void* stream, double* ms_out);
/* ABI 6: the grouped forward projector's plan `plan` (0: 64-ray chunks, 1: chunks aligned
 * per (row segment, angle) at the detector centre, 2: chunks aligned per (row segment,
 * chunk); 3-5: plans 0-2 with each block's rays clipped to those crossing its row segment
 * inside the image) for this context's geometry: angle groups, blocks per node chunk, touched row
 * pixels staged per node chunk (the host planner's model), and active = 1 if it is the plan
 * the bound batch (or, before a bind, the context) uses.  groups = 0: no such plan.
 * No device work.  (Tests and tuning; the plans give bitwise-identical projections.) */
int admm_fwd_plan_info(admm_ctx* ctx, int plan, int* groups, int* blocks, double* staged, int* active);
/* ABI 8: how the bound batch projects: vb = node-interleave width of its sample buffers;
 * mirror = 1 if the projectors run in mirror mode (angles (t + 1/2) pi / a over [0, pi), a even,
 * symmetric detector: angle a-1-t projects I as angle t projects flipud(I), so each batch
 * projects virtual images -- its nodes at (i, j) and at (N-1-i, j) -- over the first a/2 angles,
 * full-width sample vectors even for narrow batches; admm_fwd_plan_info then reports the half
 * geometry's plans).  No device work. */
int admm_batch_info(admm_ctx* ctx, int* vb, int* mirror);
/* ABI 9: admm_consensus for the edge slots [e0, e1) only (stored z, midpoint fusion), whose
 * endpoints must all lie in x_ext rows [0, rows) -- the caller's promise; only those rows are
 * read.  With the rank-internal edges (both endpoints local, rows < V) first in slot order
 * (admm_hip/plan.py), a rank runs them while the halo exchange is still writing rows >= V, then
 * the rest: the same per-edge arithmetic and statistics as one admm_consensus, bitwise.
 * Replaces block_6_admm_loop_ver2.py:210-253 for those edges.  Enqueued directly (no graph). */
int admm_consensus_range(admm_ctx* ctx, int e0, int e1, int rows, void* stream);
/* ABI 9: average duration (ms) of the bound batch's back projector launch inside the CG solve
 * (the adjoint `Ai.T @ r` of block_6_admm_loop_ver2.py:145 fused with the CG operator
 * H p = A^T A p + rho D p + mu K^T K p and its dot products): one x-update is enqueued directly
 * with HIP events around each CG step's back projection (right after its forward combine, as in
 * every solve); the batch's state advances by that x-update.  Measurement helper for bench.py's
 * roofline of the dominant kernel; synchronises. */
int admm_time_back(admm_ctx* ctx, void* stream, double* ms_out);

/* --- per-pixel edge masks for masked precisions (setup) --- */

#define ADMM_MASK_KNN 0   /* top-k per node, symmetrised, + max spanning tree if disconnected */
#define ADMM_MASK_MST 1   /* maximum spanning tree of the complete graph at the pixel        */
#define ADMM_MASK_CHAIN 2 /* random permutation chain (orders from admm_chain_orders)         */
#define ADMM_Q_ARITHMETIC 0 /* q_ij = max((W_i + W_j)/2, 1e-12)        (block_3:33-39) */
#define ADMM_Q_HARMONIC 1   /* q_ij = max(W_i W_j / (W_i + W_j), 1e-12) (block_3:26-32) */
#define ADMM_MASK_MAX_NODES 64

/* keep[(i*V + j)*n + p] = 1 if edge (i, j) is active at pixel p, for all ordered pairs
 * (symmetric, zero diagonal).  Replaces _build_all_pixel_masks and its per-pixel helpers
 * (block_3_graph_and_precisions.py:62-187: _pixel_mask_knn_then_connect :62-110,
 * _pixel_mask_mst :113-131, _pixel_mask_chain :134-151).  W: [V][n] float64 device
 * (make_precisions' W_i), orders: [n][V] int32 device (ADMM_MASK_CHAIN only, else NULL),
 * keep: [V][V][n] uint8 device.  2 <= V <= ADMM_MASK_MAX_NODES.  kNN ties (equal q) go to
 * the higher node index; the reference's tie order is numpy argpartition's (unspecified).
 * Asynchronous on `stream` (current device). */
int admm_pixel_masks(const double* W, int V, int64_t n, int strategy, int k, int q_mode,
                     const int32_t* orders, uint8_t* keep, void* stream);
/* Host: the node orders of `_pixel_mask_chain` (block_3:134-151) for n pixels --
 * numpy Generator(PCG64).permutation(V) called n times in pixel order, replayed from
 * the bit generator state {state, inc} (pcg[0..3] = state_hi, state_lo, inc_hi, inc_lo;
 * has_uint32 / uinteger as numpy reports them).  orders: [n][V] int32 host memory.
 * pcg_out (may be NULL) receives the state afterwards (same layout + has_uint32, uinteger). */
int admm_chain_orders(const uint64_t pcg[4], int has_uint32, uint32_t uinteger, int V, int64_t n,
                      int32_t* orders, uint64_t pcg_out[6]);

/* --- filtered back projection: the ramp filter (setup) --- */

#define ADMM_FBP_RAMLAK 0      /* h[0] = 1/(4 tau^2), h[k] = -1/(pi^2 k^2 tau^2) for odd k, else 0 */
#define ADMM_FBP_SHEPP_LOGAN 1 /* h[k] = -2/(pi^2 tau^2 (4 k^2 - 1))                               */
#define ADMM_FBP_HANN 2        /* h[k] = rl[k]/2 + (rl[k-1] + rl[k+1])/4, rl the Ram-Lak taps      */

/* out[v][t][j] = scale * det_spacing * sum_k sino[v][t][k] * h[j-k],  v < nimg, t < n_angles, j,k < n_det.
 * dtype = ADMM_DTYPE_* of sino and out (device pointers, sinogram layout of this header); out != sino.
 * The filter step of the "optional FBP reconstruction" the reference's legacy loader reserves a key
 * for and leaves empty (block_2_test.py:11,77: agg_fbp_recon = None); the back projection is
 * admm_project_adj, with scale = dtheta * det_spacing / h^2 turning A^T into the back projection
 * integral (admm_hip/fbp.py).  tau = det_spacing; sums in float64 (explicit fma, ascending k), rounded
 * once to dtype, so a row's result does not depend on nimg or on its place in the batch.  Context-free
 * like admm_pixel_masks; 1 <= n_det <= 4096, nimg * n_angles * n_det < 2^31.  Asynchronous on `stream`
 * (current device).  Added without an ABI bump: ADMM_ABI_VERSION stays 9 -- the change is additive
 * (one new function, no struct or existing signature changes). */
int admm_fbp_filter(const void* sino, void* out, int dtype, int n_angles, int n_det, int nimg,
                    double det_spacing, double scale, int filter, void* stream);

/* --- image quality of the reconstructions: squared error and SSIM sums --- */

/* out[v][0] = sum_p (img_v[p] - ref[p])^2 over the pixels with mask[p] != 0 (mask NULL: all N * N) and
 * out[v][1] = the sum of the SSIM map of (img_v, ref) over the valid window centres 5 <= i, j <= N - 6
 * under the same mask, for v < nimg; img_v = img + v * img_stride (doubles, img_stride >= N * N), ref one
 * [N * N] image, mask [N * N] uint8 or NULL, out [nimg][2]: float64 device pointers, C-order pixels.
 * The squared error is what the reference's evaluation helper scores strategies by
 * (test_final_integration.py:41-50: psnr = 20 log10(data_range) - 10 log10(mean((x_hat - x_true)^2)) with
 * data_range = x_true.max() - x_true.min(), then the mean over nodes); the caller divides by its pixel
 * counts (admm_hip/metrics.py).  SSIM as Wang et al. 2004: 11 x 11 Gaussian window, sigma = 1.5,
 * normalised to sum 1; moments mx, my, E[x^2], E[y^2], E[xy], population (co)variances E[.] - mu mu,
 * S = (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx^2 + sy^2 + c2)), c1 = (0.01 L)^2,
 * c2 = (0.03 L)^2 for data range L; no boundary extension.  All arithmetic float64 with explicit fma; no
 * atomics: per-tile partial sums in fixed slots of `work`, then one fixed-order sum per image, so an
 * image's two outputs depend neither on nimg, nor on its place in the batch, nor on img_stride.
 * Masked-out pixels and centres contribute exactly 0 whatever they hold.  `work`: caller-owned scratch of
 * admm_image_metrics_work doubles; nothing is allocated.  Context-free like admm_fbp_filter;
 * 11 <= N <= 4096, 1 <= nimg <= 65535, c1, c2 > 0.  Asynchronous on `stream` (current device).
 * Additive: ADMM_ABI_VERSION stays 9. */
int admm_image_metrics(const double* img, long long img_stride, const double* ref, const uint8_t* mask,
                       int N, int nimg, double c1, double c2, double* work, double* out, void* stream);
/* *n_doubles = the doubles of `work` admm_image_metrics needs for this N and nimg.  No device work. */
int admm_image_metrics_work(int N, int nimg, long long* n_doubles);

/* --- bound constraints lo <= x <= hi on the images --- */

/* The projection step of the splitting x_i = w_i, w_i in [lo, hi], with the scaled dual f_i.  For
 * image v < nimg and pixel p < n, with x_v = x + v * x_stride, w_v = w + v * wf_stride, f_v = f + v *
 * wf_stride (doubles; both strides >= n):
 *   l = lo_map ? max(lo, lo_map[p]) : lo,   h = hi_map ? min(hi, hi_map[p]) : hi
 *   t = x_v[p] + f_v[p],   w' = t < l ? l : (t > h ? h : t),   f' = t - w'
 *   out[v] = { sum_p (x - w')^2,  sum_p (w' - w_old)^2,  sum_p (x - P(x))^2 },  P(x) the same clip of x
 * w_v and f_v are updated in place; out is [nimg][3].  Comparisons, not fmin / fmax: t = -0 with l = 0
 * stays -0, a tie returns the bound's own bits, and lo = -inf / hi = +inf switch a side off (then w' = t
 * and f' = +0 exactly).  lo_map / hi_map: one [n] map each shared by every image, or NULL; lo <= hi and
 * neither NaN (the maps are the caller's to check: admm_hip/bounds.py does).  The x-update reads w as
 * one more stored z row and f as its y row (incidence sign +1), so the constraint costs the hot kernels
 * one incidence per node and this call per iteration; with the slot bound, ADMM_NODE_STAT_QUAD includes
 * its term rho/2 ||x - (w - f)||^2_{q_c}.  Layout of k_consensus<false>: 1024 pixels per block, grid
 * ceil(n / 1024) x nimg, 8-byte accesses (rows of an odd n need no alignment), 40 B per pixel-image.
 * No atomics: per-block partial sums in fixed slots of `work` (admm_bound_project_work doubles,
 * caller-owned), then one fixed-order sum per image, so an image's w, f and three sums depend neither
 * on nimg, nor on its place in the batch, nor on a stride.  All device pointers float64; nothing is
 * allocated; context-free like admm_image_metrics; 1 <= nimg <= 65535.  Asynchronous on `stream`
 * (current device).  Additive: ADMM_ABI_VERSION stays 9. */
int admm_bound_project(const double* x, long long x_stride, double* w, double* f, long long wf_stride,
                       const double* lo_map, const double* hi_map, double lo, double hi, long long n,
                       int nimg, double* work, double* out, void* stream);
/* *n_doubles = the doubles of `work` admm_bound_project needs for this n and nimg.  No device work. */
int admm_bound_project_work(long long n, int nimg, long long* n_doubles);

/* --- over-relaxation of the edge and constraint updates --- */

/* The stored-z edge update of admm_consensus with x_i replaced by xh_i = alpha x_i + (1 - alpha) z_old
 * in the z- and y-updates (Eckstein-Bertsekas over-relaxation), for the edge slots [e0, e1).  Per pixel
 * of slot e with x_a = x_ext[edge_a[e]], x_b = x_ext[edge_b[e]] and om = 1 - alpha (formed once on the
 * host), every line one IEEE float64 operation:
 *   hz = om * z,   xha = alpha * x_a + hz,   xhb = alpha * x_b + hz
 *   y_b == w == NULL (midpoint):  aa = xha + y,  ab = xhb - y,    z' = (aa + ab) * 0.5
 *   y_b, w set (weighted):        aa = xha + y,  ab = xhb + y_b,  z' = (W_a aa + W_b ab) / (W_a + W_b),
 *                                 y_b' = (y_b + xhb) - z'          (W_r = w[r], one row per x_ext row)
 *   y' = (y + xha) - z'
 *   edge_stats[e] = { sum (x_a - z')^2, sum (x_b - z')^2, sum (z' - z)^2 }     (the true x_a, x_b)
 * y, z (and y_b) rows e0 .. e1 - 1 are updated in place and edge_stats rows e0 .. e1 - 1 written; nothing
 * else is.  x_ext is [n_rows][n]; an edge with an endpoint row outside [0, n_rows) is left unchanged and
 * its statistics are NaN.  Layout of k_consensus<false>: 1024 pixels per block, one edge per blockIdx.y,
 * 8-byte accesses, 48 B per pixel-edge.  No atomics: per-(edge, block) partial sums in fixed slots of
 * `work` (admm_consensus_relaxed_work doubles for at least e1 edges, caller-owned), then one fixed-order
 * sum per edge, so an edge's results depend neither on [e0, e1) nor on its neighbours.  0 < alpha < 2,
 * finite (alpha = 1: the unrelaxed update).  Context-free, allocates nothing, asynchronous on `stream`
 * (current device).  Additive: ADMM_ABI_VERSION stays 9. */
int admm_consensus_relaxed(const double* x_ext, long long n, int n_rows, double* y, double* y_b, double* z,
                           const double* w, const int32_t* edge_a, const int32_t* edge_b, int e0, int e1,
                           double alpha, double* work, double* edge_stats, void* stream);
/* *n_doubles = the doubles of `work` admm_consensus_relaxed needs for n pixels and n_edges edge slots
 * (e1 <= n_edges).  No device work. */
int admm_consensus_relaxed_work(long long n, int n_edges, long long* n_doubles);
/* admm_bound_project around the relaxed image: t = (alpha * x + om * w) + f, then w', f' and the three
 * sums as there (the sums with the true x).  `work`: admm_bound_project_work doubles. */
int admm_bound_project_relaxed(const double* x, long long x_stride, double* w, double* f, long long wf_stride,
                               const double* lo_map, const double* hi_map, double lo, double hi, long long n,
                               int nimg, double alpha, double* work, double* out, void* stream);

/* --- unreliable links: the gated edge update --- */

/* The stored-z edge update of the slots [e0, e1) with one gate per slot: up[e] != 0 (slot e is up) or
 * up[e] == 0 (down); `up` is a device array of at least e1 bytes, indexed by the absolute slot.
 *   up:    exactly the update of admm_consensus (alpha == 1.0) or of admm_consensus_relaxed (any other
 *          alpha), operation for operation, either fusion (y_b, w both null or both set, as there);
 *   down:  y, z (and y_b) rows of the slot are not written; edge_stats[e] = { sum (x_a - z)^2,
 *          sum (x_b - z)^2, +0.0 } with the z the slot holds.
 * edge_stats rows e0 .. e1 - 1 are written; nothing else outside the up slots' y, z (y_b) rows is.  An edge
 * with an endpoint row outside [0, n_rows) is left unchanged and its statistics are NaN, up or down.
 * Layout of admm_consensus_relaxed: 1024 pixels per block, one edge per blockIdx.y, 8-byte accesses, 48 B
 * per pixel of an up edge and 24 B of a down edge; no atomics: per-(edge, block) partial sums in fixed
 * slots of `work` (admm_consensus_gated_work doubles for at least e1 edges, caller-owned), then one
 * fixed-order sum per edge.  0 < alpha < 2, finite.  Context-free, allocates nothing, asynchronous on
 * `stream` (current device).  Additive: ADMM_ABI_VERSION stays 9. */
int admm_consensus_gated(const double* x_ext, long long n, int n_rows, double* y, double* y_b, double* z,
                         const double* w, const int32_t* edge_a, const int32_t* edge_b, int e0, int e1,
                         double alpha, const uint8_t* up, double* work, double* edge_stats, void* stream);
/* *n_doubles = the doubles of `work` admm_consensus_gated needs for n pixels and n_edges edge slots
 * (e1 <= n_edges).  No device work. */
int admm_consensus_gated_work(long long n, int n_edges, long long* n_doubles);

/* --- residual-balancing rho and the scale-free stop test --- */

/* rho of the bound batch <- rho, finite and > 0 (ADMM_E_INVALID otherwise; ADMM_E_STATE without a bound
 * batch; both before any device work).  Does what admm_batch_bind does with rho and nothing else: rho D is
 * packed again as interleaved samples by the bind's own launch, the kept A^T s of an ADMM_BATCH_KEEP_X
 * batch is dropped (the next update projects x once more) and the batch's sequences are recorded again.
 * The per-ray weights, the forward plan and all scratch stay.  After it the next admm_node_update is
 * bitwise the update of a freshly bound batch with this rho holding the same x_ext, d, e, y, z.  The
 * scaled duals y (and y_b) stand for rho y: rescaling them by rho_old / rho_new is the caller's
 * (admm_hip/solver.py NodeBatch.set_rho).  Synchronous like admm_batch_bind.  Additive:
 * ADMM_ABI_VERSION stays 9. */
int admm_batch_set_rho(admm_ctx* ctx, double rho, void* stream);
/* The three norms of Boyd et al.'s (3.12) stop thresholds in node-centric form.  For image v < nimg
 * (x_v = x + v * x_stride doubles, x_stride >= n) and pixel p < n, over the incidences
 * q = inc_off[v] .. inc_off[v + 1] - 1 in ascending order, every line one IEEE float64 operation:
 *   e = inc_edge[q],   yv = inc_sign[q] > 0 ? y[e][p] : (y_b ? y_b[e][p] : -y[e][p])
 *   s += yv,   zz += z[e][p] * z[e][p]                                   (both from +0)
 *   out[v] = { X2 = sum_p x_v[p]^2,  Z2 = sum_p zz,  U2 = sum_p s * s }
 * so that for the stacked constraint "x_i - z_e = 0 at both ends of every edge" ||Ax||^2 = sum_i ninc_i
 * X2_i, ||Bz||^2 = sum_i Z2_i and ||A^T u||^2 = sum_i U2_i (u the scaled dual; ninc_i = node i's
 * incidences).  y, z (and y_b, or NULL: midpoint fusion) are [n_edges][n]; inc_off has nimg + 1 entries;
 * a bound constraint's slot is one more incidence (z row w, y row f, sign +1).  Nothing but `work` and
 * out ([nimg][3]) is written.  The index arrays are device memory: an incidence whose slot lies outside
 * [0, n_edges) is not dereferenced and that image's three sums are NaN.  inc_edge, inc_sign, y, z may be
 * NULL only when n_edges == 0.  Layout of admm_bound_project: 1024 pixels per block, grid ceil(n / 1024)
 * x nimg, 8-byte accesses, 8 (1 + 2 deg) B read per pixel-image.  No atomics: per-block partial sums in
 * fixed slots of `work` (admm_node_norms_work doubles, caller-owned), then one fixed-order sum per image,
 * so an image's sums depend neither on nimg, nor on its place in the batch, nor on x_stride.
 * Context-free, allocates nothing, 1 <= nimg <= 65535, asynchronous on `stream` (current device).
 * Additive: ADMM_ABI_VERSION stays 9. */
int admm_node_norms(const double* x, long long x_stride, const double* y, const double* y_b, const double* z,
                    long long n, int nimg, const int32_t* inc_off, const int32_t* inc_edge,
                    const int32_t* inc_sign, int n_edges, double* work, double* out, void* stream);
/* *n_doubles = the doubles of `work` admm_node_norms needs for this n and nimg.  No device work. */
int admm_node_norms_work(long long n, int nimg, long long* n_doubles);

/* --- the network-fused image and the consensus error --- */

/* The fused image xbar = (sum_i w_i x_i) / (sum_i w_i) per pixel over ALL v_total graph nodes (w = 1: the
 * plain mean) is built from sums over nodes that live in different batches, streams and ranks.  They are
 * fixed-point sums: exact, hence the same bits in any order and grouping.  fixed_sum(t) of terms t_i[p]
 * over all v_total nodes and p < n, every line one IEEE float64 operation:
 *   B = max_{i,p} |t_i[p]|                   (a NaN or +-inf term: B = +inf, and every output is NaN)
 *   B == 0: s = 0;  else B = m 2^e with 0.5 <= m < 1 (frexp), L = bit_length(v_total - 1), s = 61 - e - L
 *   q_i[p] = llrint(ldexp(t_i[p], s))        (|q| <= 2^(61 - L): v_total of them fit int64)
 *   S[p]   = sum_i q_i[p]                    (int64: exact, associative)
 *   fixed_sum[p] = ldexp((double)S[p], -s)   (the conversion rounds to nearest even)
 * and   Nn = fixed_sum(w x),  Dn = fixed_sum(w) (v_total for w = 1),  xbar = Nn / Dn,
 *       spread = sqrt(fixed_sum(w ((x - xbar) (x - xbar))) / Dn),  dev2_i = sum_p (x_i[p] - xbar[p])^2.
 * Resolution: all pixels share the grid 2^-s, so a sum is within v_total 2^-s <= 2 v_total^2 B 2^-61 of the
 * exact sum of its terms: relative to the largest term of the whole network, not to the pixel (one wild
 * pixel coarsens every pixel's grid; with B within a few powers of two of the typical values the grid is
 * finer than double).
 * Across batches B chains through admm_fuse_absmax and S through admm_fuse_accumulate; across ranks B is a
 * MAX all-reduce of one double and S an int64 SUM all-reduce of n values.  `mode` selects the terms:
 * 0: w x,  1: w,  2: w ((x - m) (x - m)) with m [n]; w == NULL is w = 1 (x * 1 = x, so the same bits); x may
 * be NULL in mode 1.  Image v is x + v * x_stride (x_stride >= n), its weights w + v * w_stride.  Layout of
 * admm_bound_project: 256 threads, 1024 pixels per block, 8-byte accesses; no atomics.  All entry points:
 * context-free, allocate nothing, 1 <= nimg <= 65535, 1 <= v_total <= 2^30, arguments checked before any
 * HIP call (ADMM_E_INVALID), asynchronous on `stream` (current device).  Additive: ADMM_ABI_VERSION stays 9. */

/* out[0] <- max(out[0], max_{v < nimg, p < n} |t_v[p]|), a term that is not finite counting as +inf (and a
 * NaN already in out[0] becoming +inf): start from out[0] = 0 and call once per batch.  Grid ceil(n / 1024) x
 * nimg, each block's maximum to its slot of `work` (admm_fuse_absmax_work doubles), then one block folds
 * the slots into out[0].  Reads 8 B (16 B with w) per pixel-image. */
int admm_fuse_absmax(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                     long long n, int nimg, int mode, double* work, double* out, void* stream);
/* *n_doubles = the doubles of `work` admm_fuse_absmax needs for this n and nimg.  No device work. */
int admm_fuse_absmax_work(long long n, int nimg, long long* n_doubles);
/* acc[p] += sum_{v < nimg} q_v[p] with s derived on the device from bmax[0] = the B of ALL v_total nodes (a
 * device pointer: the host never reads B) -- start from acc = 0 and call once per batch, in any order.  One
 * thread per pixel loops over the images, four images' loads in flight together.  bmax[0] not finite: acc is
 * left alone (admm_fuse_finish writes NaN).  A term larger than bmax[0] is the caller's error.  nimg <=
 * v_total.  Reads 8 B (16 B with w) per pixel-image, 8 B read and written per pixel. */
int admm_fuse_accumulate(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                         long long n, int nimg, int mode, const double* bmax, int v_total, int64_t* acc,
                         void* stream);
/* out[p] = fixed_sum_num[p] / fixed_sum_den[p] (root != 0: its sqrt, the spread) from the accumulators and
 * the B they were formed with; acc_den == bmax_den == NULL: the denominator is (double)v_total (w = 1).  If
 * a B is not finite every out[p] is NaN. */
int admm_fuse_finish(const int64_t* acc_num, const double* bmax_num, const int64_t* acc_den, const double* bmax_den,
                     int v_total, long long n, int root, double* out, void* stream);
/* out[v] = sum_p (x_v[p] - mean[p])^2 for v < nimg: per-block sums in fixed slots of `work`
 * (admm_fuse_deviation_work doubles), then one fixed-order sum per image, as admm_node_norms does -- an
 * image's sum depends neither on nimg, nor on its place in the batch, nor on x_stride.  Nothing but `work`
 * and out is written. */
int admm_fuse_deviation(const double* x, long long x_stride, const double* mean, long long n, int nimg, double* work,
                        double* out, void* stream);
/* *n_doubles = the doubles of `work` admm_fuse_deviation needs for this n and nimg.  No device work. */
int admm_fuse_deviation_work(long long n, int nimg, long long* n_doubles);

/* --- the Huber data term by reweighted rays --- */

/* Context-free.  ax, b, w (or NULL: w = 1) and w_out are [nimg][m], contiguous, of the sample type T =
 * dtype (ADMM_DTYPE_*); w_out is distinct from the inputs; out is [nimg][2] float64.  Per ray, every
 * line one IEEE operation:
 *
 *   r = ax - b (T);  a = |(double)r|;  h64 = a <= delta ? 1.0 : delta / a;  h = (T)h64
 *   w_out = w ? w * h (T) : h
 *   psi = a <= delta ? 0.5 * (a * a) : delta * a - hd,   hd = 0.5 * (delta * delta) formed on the host
 *   out[v][0] = sum_r (double)w psi,   out[v][1] = the number of rays with w != 0 and a > delta
 *
 * the Huber weights of the residual and the weighted Huber value of image v.  A ray with w == 0 is masked:
 * w_out = 0, its term is +0 whatever ax and b hold, and it is not counted.  delta > 0, not NaN; +inf is
 * allowed: every h = 1 and w_out is w (or 1) bitwise.  A NaN residual propagates.  The sums are per-block
 * partials in fixed slots of `work` (admm_huber_weights_work doubles, caller-owned), then one fixed-order
 * sum per image, as admm_node_norms does: an image's results depend neither on nimg nor on its place in
 * the batch.  No atomics.  Allocates nothing; arguments are checked before any HIP call (ADMM_E_INVALID);
 * asynchronous on `stream` (current device).  Reads 2 (3 with w) and writes 1 sample per ray.
 * Additive: ADMM_ABI_VERSION stays 9. */
int admm_huber_weights(const void* ax, const void* b, const void* w, void* w_out, int dtype, long long m, int nimg,
                       double delta, double* work, double* out, void* stream);
/* *n_doubles = the doubles of `work` admm_huber_weights needs for this m and nimg.  No device work. */
int admm_huber_weights_work(long long m, int nimg, long long* n_doubles);
/* admm_huber_weights with the threshold of image v read from device memory: delta_v = delta[v * delta_stride]
 * (float64; delta_stride >= 1 doubles, 3 reads admm_ray_quantile's out in place) and hd = 0.5 * (delta_v *
 * delta_v) formed on the device -- the same single IEEE operations, one kernel text -- so with delta[v] == d
 * for every v, w_out and out are bitwise those of admm_huber_weights(..., d, ...).  The host never reads
 * delta, so a NaN or non-positive delta[v] cannot be reported: it is the caller's precondition
 * (admm_ray_quantile never writes one).  `work` as admm_huber_weights_work says. */
int admm_huber_weights_dev(const void* ax, const void* b, const void* w, void* w_out, int dtype, long long m,
                           int nimg, const double* delta, long long delta_stride, double* work, double* out,
                           void* stream);

/* --- the self-scaling Huber threshold: an exact quantile of |ax - b| --- */

/* Context-free.  ax, b, w (or NULL) are [nimg][m], contiguous, of the sample type T = dtype; out is
 * [nimg][3] float64.  Per image v:
 *
 *   r   = ax - b (T);  a = |r| (T);  a ray with w != NULL and w == 0 is masked and takes no part, whatever
 *         ax and b hold (NaN included)
 *   cnt = the number of unmasked rays
 *   the keys ordered as np.sort(np.abs(r)) orders them: -0 counts as +0, +inf after every finite value,
 *         NaN after +inf
 *   k   = (long long)floor(q * (double)(cnt - 1))      one multiply, then the floor; q in [0, 1]
 *   a_k = the k-th smallest key, counted from 0        (one ray's value: never interpolated, never a sum)
 *   t   = c * (double)a_k                              one multiply
 *   delta_v = +inf if cnt == 0 or t is not a finite number > 0, else t >= floor ? t : floor
 *   out[v] = { delta_v, (double)a_k (0 when cnt == 0), (double)cnt }
 *
 * q = 0.5 is the lower median, 0 the minimum, 1 the maximum; c > 0 (1.4826 * scale for a Gaussian scale
 * estimate), floor >= 0 (+inf allowed: every delta_v = +inf), neither NaN.  A zero estimate (more than half
 * the rays with exactly zero residual) says nothing about the noise: the fallback is least squares
 * (+inf), never a zero threshold.  delta_v is never NaN and never <= 0.  An a_k that is NaN is written as
 * the quiet NaN of float64.
 *
 * One block of 1024 threads per image: a most-significant-first radix select on the bit pattern of |r|
 * (non-negative IEEE values order as unsigned integers), 11 + 10 + 10 bits for float32, 11 + 11 + 11 + 10 +
 * 10 + 10 for float64, each pass counting into an LDS histogram with integer atomics -- exact in any order,
 * so an image's three outputs depend on its rays alone: not on nimg, its place in the batch, or the
 * stream.  No floating-point atomic, no sum of samples.  m in [1, 2^32 - 1], nimg in [1, 65535].  `work`
 * is not used (admm_ray_quantile_work reports 0 bytes; NULL is accepted).  Allocates nothing; arguments are
 * checked before any HIP call (ADMM_E_INVALID); asynchronous on `stream`.  Reads 2 (3 with w) samples per
 * ray and pass.  Additive: ADMM_ABI_VERSION stays 9. */
int admm_ray_quantile(const void* ax, const void* b, const void* w, int dtype, long long m, int nimg, double q,
                      double c, double floor, void* work, double* out, void* stream);
/* *n_bytes = the bytes of `work` admm_ray_quantile needs for this m and nimg (0).  No device work. */
int admm_ray_quantile_work(long long m, int nimg, long long* n_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ADMM_TOMO_H */
