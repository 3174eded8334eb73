/*
 * ccmpc.h -- C ABI of libccmpc.so, the MI355X (gfx950) implementation of CC-MPC's
 * Monte-Carlo prediction + MVOE chance-constraint path (planner v8ideal).
 *
 * The reference is pure Python (HyeontaeSung/CC-MPC, snapshot 2025-10-31).  Each entry point
 * below replaces one stage of its hot path; the reference function it replaces is cited as
 * file:line, relative to /root/reference/collect/in_simulation/midlevel/ unless stated.
 * The host-side mirror of the reference interface (cc-mpc_amd/ccmpc) binds these with ctypes;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer unless its comment says "host".
 *  - All buffers are caller-allocated; no entry point allocates, frees or synchronises, so every
 *    call can be captured into a hipGraph.  Work is enqueued on `stream` (a hipStream_t; NULL =
 *    the null stream).  Calls are reentrant per stream.
 *  - Return value: CCMPC_OK (0) or a negative CCMPC_ERR_* code for bad arguments / launch
 *    failures (ccmpc_last_error() gives the message, per host thread).  Numerical failures of a
 *    single record (singular covariance, no real tangent, ...) do not fail the call; they are
 *    reported in that record's `status` field with a CCMPC_REC_* code, mirroring where the
 *    reference raises.
 *
 * Particle store ("plane-major SoA")
 *  - positions[(2*t + c) * ld + i], c = 0 for x, 1 for y: plane 2t+c holds coordinate c at step
 *    t of every particle.  Consecutive particles are consecutive in memory, so one wavefront
 *    reads 64 particles of one plane as a single coalesced burst.
 *  - A *cell* is one (obstacle vehicle, latent mode) pair; it owns particles
 *    [cell_off[c], cell_off[c] + cell_cnt[c]) in every plane.  cell_off must be a multiple of 4
 *    and ld a multiple of 4 (16-byte aligned 4-particle vectors).
 *  - dtype CCMPC_F64: world-frame float64 (what predict_ideal writes, v8ideal/__init__.py:2667).
 *    dtype CCMPC_F32: float32 relative to a per-cell origin (what Trajectron++ writes before
 *    `+ minpos`, v8ideal/__init__.py:486); every reduction promotes to float64 first.
 */
#ifndef CCMPC_H
#define CCMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ccmpc_stream_t; /* hipStream_t */

#define CCMPC_ABI_VERSION 2

/* call status */
#define CCMPC_OK 0
#define CCMPC_ERR_ARG -1
#define CCMPC_ERR_LAUNCH -2
#define CCMPC_ERR_WORKSPACE -3
#define CCMPC_ERR_UNSUPPORTED -4

/* per-record status (0 = ok) */
#define CCMPC_REC_SINGULAR -10   /* inv(cov_tau) or solve(Sigma1, Sigma2) singular (LinAlgError) */
#define CCMPC_REC_NO_TANGENT -11 /* n^T Sigma n <= 0: choose_closest_tangent returns None tuple */
#define CCMPC_REC_NONFINITE -12  /* slope m or a moment is inf/nan (ref_y == mean_y, N_k < 2) */
#define CCMPC_REC_NOT_PD -13     /* conditional covariance not PD (np.linalg.cholesky raises) */
#define CCMPC_REC_NOT_PSD -14    /* sqrtm of an indefinite covariance would be complex */

/* particle dtypes */
#define CCMPC_F64 0
#define CCMPC_F32 1

/* One Minkowski/MVOE half-space (one (cell, t, tau) pair), 128 bytes.
 * Constraint on the ego position x_t:  side=+1:  n . x_t >= d ;  side=-1:  n . x_t <= d
 * (v8ideal/__init__.py:926-939).  The reference's (A, b) = (-n, -d) or (n, d). */
typedef struct ccmpc_halfspace {
  double n0, n1;          /* normal [-m, 1]                                            */
  double d;               /* offset of the chosen slope-m tangent                      */
  double q00, q01, q11;   /* Q  = MVOE(cov_infer*chi_r, cov_mu*chi_p)   (:915)           */
  double r00, r01, r11;   /* QR = MVOE(Q, R^2 I)                        (:917-918)       */
  double beta1, beta2;    /* fixed-point solutions of the two MVOE calls               */
  double lower_bound;     /* compute_lower_bound(cov_infer, cov_mu, cov_t, eps) (:942)   */
  double mean0, mean1;    /* ellipsoid centre = particle mean at step t (:896)         */
  int32_t which;          /* 0: the "+" tangent, 1: the "-" tangent                    */
  int32_t side;           /* +1 (>=) or -1 (<=)                                        */
  int32_t status;         /* CCMPC_REC_* or 0                                          */
  int32_t t_tau;          /* (t << 16) | tau                                           */
} ccmpc_halfspace;

/* One GMM-affine half-space (one (cell, t)), 128 bytes (v8ideal/__init__.py:1476-1515).
 * side=+1:  n . x_t >= rhs = d + margin ;  side=-1:  n . x_t <= rhs = d - margin
 * (plus the caller's S_big_repeated[0, t] term, which is a QP variable, not data). */
typedef struct ccmpc_affine_rec {
  double n0, n1, d;
  double margin;          /* Gamma * || sqrtm(cov) [m, -1]^T ||_2                       */
  double rhs;
  double mean0, mean1;
  double c00, c01, c11;   /* particle covariance at step t (ddof = 1)                  */
  double s00, s01, s11;   /* sqrtm(cov)                                                */
  double m;               /* slope -(ref_x - mean_x) / (ref_y - mean_y)                 */
  int32_t which, side, status, t;
} ccmpc_affine_rec;

/* The fields of a record the QP reads, 32 bytes: what the multi-GPU exchange moves instead of
 * the 128-byte record (the one collective is a record all-gather; no reference
 * counterpart -- the reference solves one scene per process).  rhs = the halfspace record's d
 * or the affine record's rhs; t_tau = the source record's last field. */
typedef struct ccmpc_gather_rec {
  double n0, n1, rhs;
  int16_t side, status;
  int32_t t_tau;
} ccmpc_gather_rec;

/* Pack n_rec records of kind CCMPC_REC_KIND_HALFSPACE / _AFFINE into ccmpc_gather_rec
 * (device pointers; one launch, 128 B read + 32 B written per record). */
int ccmpc_compact_records(const void *rec, int rec_kind, int64_t n_rec, ccmpc_gather_rec *out,
                          ccmpc_stream_t stream);

int ccmpc_abi_version(void);
const char *ccmpc_last_error(void);
const char *ccmpc_status_string(int status);

/* Stream-ordered copy of `bytes` between host (pinned) and device buffers, direction inferred
 * from the pointers (hipMemcpyDefault).  Graph plumbing with no reference counterpart: a
 * captured planning step (ccmpc/step.py) carries its packed input upload and output download
 * as graph nodes, so one replay is the whole step. */
int ccmpc_copy_async(void *dst, const void *src, size_t bytes, ccmpc_stream_t stream);
/* The same copy as a device kernel reading / writing the pinned host buffer directly (a graph
 * kernel node rather than a memcpy node); bytes and both pointers 16-byte aligned. */
int ccmpc_copy_kernel_async(void *dst, const void *src, size_t bytes, ccmpc_stream_t stream);

/* Stream-ordered signal: *host_word (pinned) = *value (device), visible to the host only after
 * every write this stream made before it (a system-scope release).  A captured step's host side
 * polls the word rather than synchronising the stream. */
int ccmpc_signal_host(int64_t *host_word, const int64_t *value, ccmpc_stream_t stream);
/* ccmpc_copy_kernel_async (device -> pinned host) and ccmpc_signal_host in one single-workgroup
 * launch: *host_word = *value becomes visible only after the copied bytes. */
int ccmpc_copy_signal_async(void *dst, const void *src, size_t bytes, int64_t *host_word,
                            const int64_t *value, ccmpc_stream_t stream);

/* Graph capture of a planning step (ccmpc/step.py): begin / end a relaxed-mode capture on
 * `stream` (the library calls and event record / wait pairs issued in between become the
 * graph; end instantiates it into *out_exec), replay it on a stream, release it.  The graph
 * holds the buffer addresses it was captured with: keep them alive while it exists, and let
 * its last replay finish before destroying it or them. */
int ccmpc_graph_capture_begin(ccmpc_stream_t stream);
int ccmpc_graph_capture_end(ccmpc_stream_t stream, void **out_exec);
int ccmpc_graph_launch(void *exec, ccmpc_stream_t stream);
int ccmpc_graph_destroy(void *exec);

/* ---------------------------------------------------------------------------------------
 * Moment (Gram) reduction.  Replaces every np.mean / np.cov over particle clouds on the path:
 *   v8ideal/__init__.py:864-875 (t=0 stats), :896 + makeconstraint.py:41-70 predict_moments
 *   (each (t,tau) np.cov is a 4x4 block of out_cov), :1485-1493 (affine), :2584-2606
 *   save_moments (mean_p0p1[t] = out_mean[t], cov_p0p1[t] = diagonal 2x2 block,
 *   cross_cov[t][tau] = block (t, tau)).
 * out_mean[c][t][2] (origin added back for F32), out_cov[c][2T][2T] (ddof = 1, symmetric).
 * n_particles_bound >= sum(cell_cnt) sizes the grid, so counts may be produced on the device.
 * T <= 40.  ONE kernel launch: per-chunk partial Gram sums are combined in-launch through a
 * fixed fan-in-16 tree of arrival counters (the last arriver of each group combines it), so
 * the result is deterministic and uses no float atomics.
 *
 * Workspace contract (every *_workspace_bytes-sized workspace): its first
 * round_up(workspace_bytes / 8, 256) bytes hold the tree's arrival counters (one per 128-byte
 * line), the rest the partial-Gram slabs.  Zero-fill a fresh workspace ONCE (hipMemset after allocating); every
 * call leaves the counters zero again.  One workspace may serve calls of ANY shape (moments,
 * cycles, ideal rollouts, any T / cell count) as long as every call passes the same
 * workspace_bytes (the whole buffer) and that is >= the call's *_workspace_bytes: the counter
 * region depends on workspace_bytes only, so no call's slabs overwrite another call's
 * counters.  Do not share one workspace between concurrent streams.
 * ------------------------------------------------------------------------------------- */
size_t ccmpc_moments_workspace_bytes(int64_t T, int64_t n_cells, int64_t n_particles_bound);
int ccmpc_moments(const void *positions, int dtype, int64_t ld, int64_t T,
                  const double *origin /* [n_cells][2] for F32, NULL for F64 */,
                  const int64_t *cell_off, const int64_t *cell_cnt, int64_t n_cells,
                  int64_t n_particles_bound, void *workspace, size_t workspace_bytes,
                  double *out_mean, double *out_cov, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Minkowski / MVOE half-space assembly for every (cell, t, tau < t), from ccmpc_moments output.
 * Replaces v8ideal/__init__.py:893-947 with makeconstraint.py predict_moments (:41-70),
 * compute_mvoe (:7-38, called twice), choose_closest_tangent (:176-207) and
 * compute_lower_bound (:282-303).
 *  ref_traj[r][t][2]   reference trajectory r (host load_refT, :2768-2787), cell c uses
 *                      r = cell_ref[c] (NULL -> 0)
 *  cell_risk[c][3]     {chi_r = chi2.ppf(1-eps_ijt, 2), chi_p = chi2.ppf(0.9999, 2),
 *                       gamma = norm.ppf(1-eps_ijt)}, eps_ijt = eps_ura[ov,k]/ph (:910-913)
 *  R                   3.4 (:795); tol 1e-8, maxiter 1000 (makeconstraint.py:7)
 *  out_rec[c][T(T-1)/2] in the reference's append order: pair p = t(t-1)/2 + tau
 *  out_prob_lower[c][T] min over tau of the lower bound, 1.0 at t = 0 (:898, :943)
 * ------------------------------------------------------------------------------------- */
int ccmpc_minkowski(const double *mean, const double *cov, int64_t T, int64_t n_cells,
                    const double *ref_traj, const int32_t *cell_ref, const double *cell_risk,
                    double R, double tol, int32_t maxiter, ccmpc_halfspace *out_rec,
                    double *out_prob_lower, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * One-launch Minkowski constraint-generation cycle: ccmpc_moments + ccmpc_minkowski fused.
 * The last-arriving workgroup of each cell finalises its moments and immediately assembles the
 * cell's T(T-1)/2 half-spaces, so one planning step's obstacle constraints cost one kernel
 * (v8ideal/__init__.py:881-947 and the save_moments statistics :2575-2606).
 * Same arguments and outputs as the two calls it replaces; same workspace contract.
 * ------------------------------------------------------------------------------------- */
int ccmpc_minkowski_cycle(const void *positions, int dtype, int64_t ld, int64_t T,
                          const double *origin, const int64_t *cell_off, const int64_t *cell_cnt,
                          int64_t n_cells, int64_t n_particles_bound, void *workspace,
                          size_t workspace_bytes, const double *ref_traj, const int32_t *cell_ref,
                          const double *cell_risk, double R, double tol, int32_t maxiter,
                          double *out_mean, double *out_cov, ccmpc_halfspace *out_rec,
                          double *out_prob_lower, ccmpc_stream_t stream);

/* The same call with its arguments in one struct, filled once by a caller that launches the
 * same cycle every step (the argument marshalling of a 22-argument foreign call is microseconds
 * of host time in front of every launch from an interpreter).  ccmpc_cycle_args_size() =
 * sizeof(ccmpc_cycle_args), for a binding to check its layout.
 *
 * slot_cap (the last field) is 0 for a packed store.  Above 0 the store is slotted: every
 * cell_off[c] == c * slot_cap, slot_cap is a multiple of the launch's item chunk (256 particles at
 * T <= 8) and at least every cell_cnt[c], and ld >= n_cells * slot_cap.  Short horizons (T <= 8)
 * below the balanced-mode bound then run one workgroup per (cell, chunk of the slot) whose first
 * particle loads do not wait for the cell tables.  The workspace holds one slab per such item:
 * size it with ccmpc_moments_workspace_bytes(T, n_cells, max(n_particles_bound, n_cells *
 * slot_cap)).  A slot_cap that is no multiple of the chunk or does not fit ld is CCMPC_ERR_ARG and
 * launches nothing.  Every other launch ignores the field and reads the tables. */
typedef struct ccmpc_cycle_args {
  const void *positions;
  int32_t dtype, maxiter;
  int64_t ld, T;
  const double *origin;
  const int64_t *cell_off, *cell_cnt;
  int64_t n_cells, n_particles_bound;
  void *workspace;
  size_t workspace_bytes;
  const double *ref_traj;
  const int32_t *cell_ref;
  const double *cell_risk;
  double R, tol;
  double *out_mean, *out_cov;
  ccmpc_halfspace *out_rec;
  double *out_prob_lower;
  ccmpc_stream_t stream;
  int64_t slot_cap;
} ccmpc_cycle_args;
int ccmpc_minkowski_cycle_args(const ccmpc_cycle_args *args);
size_t ccmpc_cycle_args_size(void);

/* ---------------------------------------------------------------------------------------
 * GMM-affine half-spaces for every (cell, t).  Replaces v8ideal/__init__.py:1470-1515.
 *  cell_gamma[c] = norm.ppf(1 - eps_ura[ov,k]/ph) (:1481-1482); out_rec[c][T].
 * ------------------------------------------------------------------------------------- */
int ccmpc_affine(const double *mean, const double *cov, int64_t T, int64_t n_cells,
                 const double *ref_traj, const int32_t *cell_ref, const double *cell_gamma,
                 double R, ccmpc_affine_rec *out_rec, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * GMM-affine half-spaces with the recursive-feasibility covariance scale, for every (cell, t):
 * compute_obstacle_constraints_GMM_affine_scale_ideal (v8ideal/__init__.py:2320-2425), and with
 * scaled = 0 its unscaled twin compute_obstacle_constraints_GMM_affine_robust (:1541-1878).
 *  scale(t) = max(1, max_{tau<t} compute_scale(predict_moments(t, tau), Gamma, chi_p))
 *             (makeconstraint.py:259-280) if scaled, else 1; cov = scale C_tt
 *  cell_risk[c][3]     as ccmpc_minkowski_cycle (chi_p = chi2.ppf(0.9999, 2), Gamma = norm.ppf(1 - eps))
 *  tangent_in[c][T]    slope m per (cell, t); NULL -> m from ref_traj (the T == ph case)
 *  const_idx_in[c][T]  with tangent_in: CCMPC_TANGENT_CHOOSE (-2) = the reference's None (closest
 *                      tangent to ref), or -1 / 0 / 1 = the index it passes (Python indexing; -1 is
 *                      the last candidate and is also what the record reports in `which`)
 * Constraint: n.x >= rhs (side +1) or <= rhs (side -1), rhs = d +/- Gamma sqrt(|cov|_F) |[m, -1]|.
 * Record fields: c00/c01/c11 = the unscaled cov (what the generator saves), s00 = scale,
 * s01 = sqrt(|cov|_F) of the scaled cov, s11 = 0.
 * ------------------------------------------------------------------------------------- */
#define CCMPC_TANGENT_CHOOSE -2
int ccmpc_affine_scale(const double *mean, const double *cov, int64_t T, int64_t n_cells,
                       const double *ref_traj, const int32_t *cell_ref, const double *cell_risk,
                       double R, int32_t scaled, const double *tangent_in,
                       const int32_t *const_idx_in, ccmpc_affine_rec *out_rec,
                       ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * predict_ideal: affine conditional-Gaussian forward rollout (v8ideal/__init__.py:2620-2711)
 * from the PREVIOUS planning step's moments, which stay device-resident (no pickle round trip).
 *  prev_mean[s][T_src][2], prev_cov[s][2T_src][2T_src]  -- ccmpc_moments output of that step
 *  src_cell[c]         the reference's data_idx fallback, resolved by the host (:2650-2656)
 *  x0[c][2]            the shared initial draw (:2662-2665); NULL -> x0 = mean_0 + chol(cov_0) z,
 *                      z = Philox pair (0, 0, rng_cell[c], STREAM_IDEAL_X0)
 *  Z[c][t][2][n]       step noise (:2699-2700); NULL -> Philox pair (i, t, rng_cell[c], STREAM_IDEAL_Z)
 *  rng_cell[c]         RNG stream id per cell (NULL -> c), so results are identical however the
 *                      cells are sharded over GPUs
 *  out positions: cell c occupies [c*S, c*S + n_samples) of every plane, S = n_samples rounded
 *  up to a multiple of 4 (so the output is a valid ccmpc_moments store), dtype F64, slot t holds
 *  x_{t+1} (the reference's slot quirk).  T <= T_src - 1, ld >= n_cells * S.
 *  out_status[c]: 0 or CCMPC_REC_SINGULAR / CCMPC_REC_NOT_PD.
 *
 *  A failed cell (out_status[c] != 0; the reference raises LinAlgError for the frame, and the
 *  host is expected to raise on the status) still has defined outputs, the same bits on every
 *  run whatever ran on the device before:
 *   - step t fails where det(Sigma_t) is 0 or not finite (SINGULAR; a NaN source covariance,
 *     as the moments of a one-particle cell are, ends here) or Sigma_{t+1} - A_t C^T has no
 *     Cholesky factor (NOT_PD); the status is the smallest code over the steps and the draw.
 *   - slots before the first failed step hold the values a good cell would; from the first
 *     failed step on every position, and with it every mean and covariance entry that touches
 *     such a step, is NaN.  A failed x0 draw (x0 == NULL, cov_0 not PD) makes every slot NaN.
 *   - in ccmpc_ideal_minkowski_cycle[_ex] every half-space record of the cell has a non-zero
 *     status: its own code where it has one, the cell's code otherwise.
 *  The other cells of the launch are not affected.
 * ------------------------------------------------------------------------------------- */
int ccmpc_ideal_rollout(const double *prev_mean, const double *prev_cov, int64_t T_src,
                        const int32_t *src_cell, int64_t n_cells, int64_t T, int64_t n_samples,
                        const double *x0, const double *Z, uint64_t seed,
                        const int32_t *rng_cell, double *out_positions, int64_t ld,
                        int32_t *out_status, ccmpc_stream_t stream);

/* Same rollout fused with the moment reduction: particles are generated in registers and
 * reduced without ever being written to HBM (the reference's only consumer of the 1e6-row
 * ideal trajectories is np.cov, :886-907 and :2586-2606).  Noise from Philox only.  Same
 * workspace contract as ccmpc_moments.  out_mean / out_cov as ccmpc_moments for T steps. */
size_t ccmpc_ideal_moments_workspace_bytes(int64_t T, int64_t n_cells, int64_t n_samples);
int ccmpc_ideal_moments(const double *prev_mean, const double *prev_cov, int64_t T_src,
                        const int32_t *src_cell, int64_t n_cells, int64_t T, int64_t n_samples,
                        const double *x0, uint64_t seed, const int32_t *rng_cell,
                        void *workspace, size_t workspace_bytes, double *out_mean,
                        double *out_cov, int32_t *out_status, ccmpc_stream_t stream);

/* The shrinking-horizon step (T < ph) in one launch: ideal rollout -> moments -> half-spaces
 * (v8ideal/__init__.py:824-825 + :881-947).  Arguments as ccmpc_ideal_moments plus the
 * ccmpc_minkowski ones. */
int ccmpc_ideal_minkowski_cycle(const double *prev_mean, const double *prev_cov, int64_t T_src,
                                const int32_t *src_cell, int64_t n_cells, int64_t T,
                                int64_t n_samples, const double *x0, uint64_t seed,
                                const int32_t *rng_cell, void *workspace, size_t workspace_bytes,
                                const double *ref_traj, const int32_t *cell_ref,
                                const double *cell_risk, double R, double tol, int32_t maxiter,
                                double *out_mean, double *out_cov, int32_t *out_status,
                                ccmpc_halfspace *out_rec, double *out_prob_lower,
                                ccmpc_stream_t stream);

/* As ccmpc_ideal_minkowski_cycle; seed_dev (nullable) points at the Philox seed in device
 * memory and overrides `seed`, so a captured graph draws a fresh rollout per replay (the
 * planning-step graphs of ccmpc/step.py write it with the step's packed inputs). */
int ccmpc_ideal_minkowski_cycle_ex(const double *prev_mean, const double *prev_cov,
                                   int64_t T_src, const int32_t *src_cell, int64_t n_cells,
                                   int64_t T, int64_t n_samples, const double *x0, uint64_t seed,
                                   const uint64_t *seed_dev, const int32_t *rng_cell,
                                   void *workspace, size_t workspace_bytes,
                                   const double *ref_traj, const int32_t *cell_ref,
                                   const double *cell_risk, double R, double tol, int32_t maxiter,
                                   double *out_mean, double *out_cov, int32_t *out_status,
                                   ccmpc_halfspace *out_rec, double *out_prob_lower,
                                   ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * GMM-latent particle sampler (Trajectron++ predict tail behind prediction.py:81-86):
 * z ~ Categorical(p(z|x)) by inverse CDF, per step a = mu + L eps (GMM2D.rsample, one
 * component, L = [[s0, 0], [s1 rho, s1 sqrt(1 - rho^2)]]), Unicycle integration (exact at
 * constant turn rate and acceleration; straight when |dphi| <= 1e-2), float32 as torch runs it.
 *  init_state[o][4]   x, y, heading, speed (scene-relative)
 *  latent_cdf[o][L]   cumulative p(z|x) (host), L <= 64
 *  gmm[o][L][T][5]    mu_dphi, mu_a, log sigma_dphi, log sigma_a, rho   (float32)
 *  out_z[o][N]        latent id per particle (the reference's argmax z, prediction.py:103)
 *  out_pos            F32 store in SAMPLE order: OV o occupies [o*S, o*S + N), S = round_up(N, 4)
 * Noise: z uses Philox (i, 0, g, STREAM_SAMPLER_Z), eps uses (i, t, g, STREAM_SAMPLER_EPS) with
 * g = ov_base + o the GLOBAL OV id, so a scene's draws do not depend on how scenes are sharded
 * over ranks or batched into calls.
 * PARITY UNPINNED upstream (absent submodule): checked against the repo's own restatement.
 * This is the synthetic mode (Philox z and eps, per-latent parameters); the upstream-shaped
 * boundary is ccmpc_sample_unicycle_ex below, of which this is the (PER_LATENT, NULL, NULL) case.
 * ------------------------------------------------------------------------------------- */
int ccmpc_sample_unicycle(const double *init_state, const double *latent_cdf, int64_t n_latent,
                          const float *gmm, int64_t n_ov, int64_t N, int64_t T, double dt,
                          uint64_t seed, int64_t ov_base, int32_t *out_z, float *out_pos,
                          int64_t ld, ccmpc_stream_t stream);

/* The sampler at the boundary Trajectron++ actually emits (prediction.py:81-86): torch draws
 * z (latent.sample_p, one-hot -> argmax as :103 does) and the decoder's noise eps (randn inside
 * GMM2D.rsample), and p_y_xz's GRU decoder is autoregressive, so every sample carries its OWN
 * GMM parameters per step.  Replaces the action draw + Unicycle.integrate_samples tail of
 * p_y_xz (:85) and the argmax of :103.
 *  gmm_layout CCMPC_GMM_PER_LATENT:   gmm[o][L][T][5] selected by z (as ccmpc_sample_unicycle)
 *             CCMPC_GMM_PER_PARTICLE: gmm[o][T][5][N] (particle-minor; needs z_in)
 *  z_in[o][N]       injected latent ids in [0, n_latent) (ids outside are clamped for memory
 *                   safety; the Python mirror rejects them), or NULL: Philox inverse CDF of
 *                   latent_cdf (which may be NULL when z_in is given)
 *  eps_in[o][T][2][N] injected standard-normal noise (float32), or NULL: Philox
 *  seed_dev         device copy of the Philox seed (read at launch, so a captured graph draws
 *                   fresh particles per replay), or NULL: `seed`
 * Per-step action a = mu + L eps with L = [[s0, 0], [s1 rho, s1 sqrt(clamp(1 - rho^2, 1e-5,
 * 1))]] (GMM2D's clamp), the L eps row summed before mu is added.  out_z / out_pos as above.
 * PARITY UNPINNED upstream (Trajectron++ absent): checked against the repo's restatement. */
#define CCMPC_GMM_PER_LATENT 0
#define CCMPC_GMM_PER_PARTICLE 1
int ccmpc_sample_unicycle_ex(const double *init_state, const double *latent_cdf, int64_t n_latent,
                             const float *gmm, int32_t gmm_layout, const int32_t *z_in,
                             const float *eps_in, int64_t n_ov, int64_t N, int64_t T, double dt,
                             uint64_t seed, const uint64_t *seed_dev, int64_t ov_base,
                             int32_t *out_z, float *out_pos, int64_t ld, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Particle bucketing by latent mode: make_ovehicles (v8ideal/__init__.py:469-505) +
 * OVehicle.from_trajectron (ovehicle.py:24-117) on the sampler's sample-order store.
 *  keep_map[o][L]   kept-mode index of each latent value, -1 if p(z|x) <= filter (host decides;
 *                   latent_probs are host data); n_kept[o] >= 1 (the reference cannot regroup
 *                   into zero modes); cell_base[o] = first global cell of OV o
 *  minpos[o][2]     scene origin added in float64 to the float32 predictions (:486)
 *  region[o]        first slot of OV o's region in pos_out (4-aligned; each region needs
 *                   N + 4 * n_kept[o] slots)
 *  out: pos_out     F32 store (origin = minpos), cells in (ov, kept mode) order, each cell's
 *                   particles in the reference's order (native mode in sample order, then the
 *                   regrouped rare modes in ascending latent order, each in sample order)
 *       cell_off/cell_cnt [n_cells], cell_pmf = N_k / N, init_center [n_cells][2] (world)
 * Rare particles go to the kept mode whose centre (mean final position) is nearest, first
 * index on ties (scipy.spatial.distance_matrix + np.argmin).  Deterministic.
 * Workspace: ccmpc_bucket_workspace_bytes; its head holds the per-OV and per-chunk (16 blocks
 * of 256 particles) arrival counters, so zero-fill it once (every call leaves them zero).
 * Three launches.
 * ------------------------------------------------------------------------------------- */
size_t ccmpc_bucket_workspace_bytes(int64_t n_ov, int64_t N, int64_t n_latent, int64_t max_k);
int ccmpc_bucket(const int32_t *z, const float *pos_in, int64_t ld_in, int64_t T, int64_t n_ov,
                 int64_t N, int64_t n_latent, const int32_t *keep_map, const int32_t *n_kept,
                 const int32_t *cell_base, int64_t max_k, const double *minpos,
                 const int64_t *region, void *workspace, size_t workspace_bytes, float *pos_out,
                 int64_t ld_out, int64_t *cell_off, int64_t *cell_cnt, double *cell_pmf,
                 double *init_center, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The reference's own prediction boundary into ccmpc_bucket's input.  Replaces the per-OV
 * `predictions[idx]` / `z[idx]` reads of make_ovehicles (v8ideal/__init__.py:469-490) on the
 * 5-tuple generate_vehicle_latents returns (prediction.py:93-105):
 *  pred[row][N][T][2]  float32, scene-relative (numpy's swapaxes(predictions, 0, 1) layout)
 *  z[row][N]           latent ids, int64 (z_bytes = 8: np.argmax's dtype) or int32 (4).
 *                      make_ovehicles indexes a list of n_latent entries by them (:488-491):
 *                      an id in [-n_latent, 0) wraps as a Python index; any other id outside
 *                      [0, n_latent) is where the reference raises IndexError -- it is counted
 *                      into z_bad[o] (and clamped, for memory safety, so the output is then
 *                      not the reference's: the caller must refuse it)
 *  rows[n_ov]          device int32: the node row of OV o (make_ovehicles skips the ego's
 *                      node); NULL = rows 0 .. n_ov-1
 *  out: pos_out        F32 sample-order store, OV o at o * ov_stride (ov_stride >= N, 4-aligned
 *                      for ccmpc_bucket): pos_out[(2t + c) * ld_out + o * ov_stride + i]
 *       z_out[n_ov][N] int32, as ccmpc_bucket reads it
 *       z_bad[n_ov]    device int32, optional (NULL): invalid ids of OV o ADDED (the caller
 *                      zero-fills it first)
 * One launch; traffic 2 x 8 T B per particle.  The step graph uses the one-pass placement
 * ccmpc_bucket_predictions below instead (no sample-order store).
 * ------------------------------------------------------------------------------------- */
int ccmpc_load_predictions(const float *pred, const void *z, int z_bytes, const int32_t *rows,
                           int64_t n_ov, int64_t N, int64_t T, int64_t n_latent, float *pos_out,
                           int64_t ld_out, int64_t ov_stride, int32_t *z_out, int32_t *z_bad,
                           ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Sampler + bucketing as one placement pass, for clouds of N <= 262144 particles per OV: the
 * same draws as ccmpc_sample_unicycle_ex (same Philox streams, same float32 arithmetic)
 * bucketed as ccmpc_bucket buckets them -- every cell holds the same particles in the same
 * order and the same init_center / pmf bits.  Replaces prediction.py:81-86 +
 * v8ideal/__init__.py:469-505 + ovehicle.py:24-117.  Launches: latent ids + counts, then the
 * sampler writing each native particle straight into its cell (rare ones into a rare list),
 * then the rare particles' placement -- one launch up to N = 8192, keys then copy above it.
 * Differences from ccmpc_bucket's output: only where the cells start.  Cell k of OV o starts at
 *   region[o] + sum_{j<k} round4(n_j + R_o)   (n_j = mode j's own particles, R_o = rare ones)
 * so region[o] needs n_kept[o] * (N + 4) free slots of pos_out.  out_z (optional, may be NULL)
 * gets the sample-order latent ids.  N > 262144: the sampler + ccmpc_bucket.
 * Workspace: ccmpc_sample_bucket_workspace_bytes (0 = shape not supported), 256-byte aligned;
 * no initialisation needed (the first launch writes everything the second reads).
 * ------------------------------------------------------------------------------------- */
size_t ccmpc_sample_bucket_workspace_bytes(int64_t n_ov, int64_t N, int64_t T, int64_t max_k);
int ccmpc_sample_bucket(const double *init_state, const double *latent_cdf, int64_t n_latent,
                        const float *gmm, int32_t gmm_layout, const int32_t *z_in,
                        const float *eps_in, int64_t n_ov, int64_t N, int64_t T, double dt,
                        uint64_t seed, const uint64_t *seed_dev, int64_t ov_base,
                        const int32_t *keep_map, const int32_t *n_kept, const int32_t *cell_base,
                        int64_t max_k, const double *minpos, const int64_t *region,
                        void *workspace, size_t workspace_bytes, int32_t *out_z, float *pos_out,
                        int64_t ld_out, int64_t *cell_off, int64_t *cell_cnt, double *cell_pmf,
                        double *init_center, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * make_ovehicles (v8ideal/__init__.py:469-505, ovehicle.py:24-117) on the reference's own
 * predictor output in ONE placement pass: ccmpc_sample_bucket's launches with the predictor's
 * coordinates in place of the sampler (no sample-order store, no re-read + scatter of every
 * particle).  Inputs as ccmpc_load_predictions (pred[row][N][T][2] float32 scene-relative,
 * z[row][N] int64 / int32, rows[n_ov] or NULL); bucketing arguments and outputs as
 * ccmpc_sample_bucket (its workspace size: ccmpc_sample_bucket_workspace_bytes(n_ov, N, T,
 * max_k)); cells bit-identical to ccmpc_load_predictions + ccmpc_bucket.
 *  z_bad[n_ov]  device int32, optional: the number of OV o's ids make_ovehicles' list index
 *               would refuse (outside [-n_latent, n_latent); [-n_latent, 0) wraps) -- WRITTEN
 *               (no zero-fill needed).  Non-zero: the reference raises IndexError there, and
 *               the output is not the reference's (those ids were clamped).
 * ------------------------------------------------------------------------------------- */
int ccmpc_bucket_predictions(const float *pred, const void *z, int z_bytes, const int32_t *rows,
                             int64_t n_ov, int64_t N, int64_t T, int64_t n_latent,
                             const int32_t *keep_map, const int32_t *n_kept,
                             const int32_t *cell_base, int64_t max_k, const double *minpos,
                             const int64_t *region, void *workspace, size_t workspace_bytes,
                             float *pos_out, int64_t ld_out, int64_t *cell_off, int64_t *cell_cnt,
                             double *cell_pmf, double *init_center, int32_t *z_bad,
                             ccmpc_stream_t stream);
/* The same with the predictor's tensors named at RUN time: ptrs (device memory, e.g. a field of
 * a captured graph's input pack) holds the addresses {pred, z} of that launch's tensors, so a
 * graph captured once reads each frame's predictor output in place (no device-to-device copy
 * into buffers of its own).  The tensors must stay alive until the launch's outputs are read. */
int ccmpc_bucket_predictions_indirect(const uint64_t *ptrs, int z_bytes, const int32_t *rows,
                                      int64_t n_ov, int64_t N, int64_t T, int64_t n_latent,
                                      const int32_t *keep_map, const int32_t *n_kept,
                                      const int32_t *cell_base, int64_t max_k,
                                      const double *minpos, const int64_t *region,
                                      void *workspace, size_t workspace_bytes, float *pos_out,
                                      int64_t ld_out, int64_t *cell_off, int64_t *cell_cnt,
                                      double *cell_pmf, double *init_center, int32_t *z_bad,
                                      ccmpc_stream_t stream);

/* The three placement calls above with the caller's input pack copied in the same first launch
 * (the planning-step graph's packed H2D copy): equal to
 *   ccmpc_copy_kernel_async(pack_dev, pack_host, pack_bytes, stream)
 * followed by the unpacked call, whose pointer arguments may point into pack_dev.  The latent-id
 * pass reads its own inputs (latent CDF, keep map, seed, z or the predictor's addresses) from the
 * pinned host side while the copy runs, so the copy's kernel boundary leaves the step.
 * pack_host: pinned host memory (device-accessible by its host address); pack_bytes % 16 == 0,
 * both pointers 16-byte aligned. */
int ccmpc_sample_bucket_packed(void *pack_dev, const void *pack_host, size_t pack_bytes,
                               const double *init_state, const double *latent_cdf,
                               int64_t n_latent, const float *gmm, int32_t gmm_layout,
                               const int32_t *z_in, const float *eps_in, int64_t n_ov, int64_t N,
                               int64_t T, double dt, uint64_t seed, const uint64_t *seed_dev,
                               int64_t ov_base, const int32_t *keep_map, const int32_t *n_kept,
                               const int32_t *cell_base, int64_t max_k, const double *minpos,
                               const int64_t *region, void *workspace, size_t workspace_bytes,
                               int32_t *out_z, float *pos_out, int64_t ld_out, int64_t *cell_off,
                               int64_t *cell_cnt, double *cell_pmf, double *init_center,
                               ccmpc_stream_t stream);
int ccmpc_bucket_predictions_packed(void *pack_dev, const void *pack_host, size_t pack_bytes,
                                    const float *pred, const void *z, int z_bytes,
                                    const int32_t *rows, int64_t n_ov, int64_t N, int64_t T,
                                    int64_t n_latent, const int32_t *keep_map,
                                    const int32_t *n_kept, const int32_t *cell_base,
                                    int64_t max_k, const double *minpos, const int64_t *region,
                                    void *workspace, size_t workspace_bytes, float *pos_out,
                                    int64_t ld_out, int64_t *cell_off, int64_t *cell_cnt,
                                    double *cell_pmf, double *init_center, int32_t *z_bad,
                                    ccmpc_stream_t stream);
int ccmpc_bucket_predictions_indirect_packed(void *pack_dev, const void *pack_host,
                                             size_t pack_bytes, const uint64_t *ptrs,
                                             int z_bytes, const int32_t *rows, int64_t n_ov,
                                             int64_t N, int64_t T, int64_t n_latent,
                                             const int32_t *keep_map, const int32_t *n_kept,
                                             const int32_t *cell_base, int64_t max_k,
                                             const double *minpos, const int64_t *region,
                                             void *workspace, size_t workspace_bytes,
                                             float *pos_out, int64_t ld_out, int64_t *cell_off,
                                             int64_t *cell_cnt, double *cell_pmf,
                                             double *init_center, int32_t *z_bad,
                                             ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Headings, bounding-box vertices and L4 outer approximation for every (cell, t).
 * Replaces ovehicle.py:72-76 (yaws = atan2 of step deltas, step 0 from past[-1]),
 * v8ideal/__init__.py:627-640 (vertices_of_bboxes, restated from midlevel/util.py:104-124),
 * :694-736 -> midlevel/util.py:171-200 (A = [I; -I] R(mean yaw), b = max_{particles, corners} A v)
 * and the t = 0 yaw statistics of :872, :875.
 *  past_last[c][2]   world-frame past[-1] of the cell's OV;  bbox[c][2] = {lon, lat}
 *  out_A[c][T][4][2], out_b[c][T][4], out_yaw_mean[c][T], out_yaw0_var[c] (ddof = 1)
 *  out_yaw (nullable)       pred_yaws in store layout [T][ld]
 *  out_vertices (nullable)  corners in store layout [T][8][ld], plane 8t + 2 corner + xy
 * ------------------------------------------------------------------------------------- */
int ccmpc_l4(const void *positions, int dtype, int64_t ld, int64_t T, const double *origin,
             const int64_t *cell_off, const int64_t *cell_cnt, int64_t n_cells,
             const double *past_last, const double *bbox, double *out_A, double *out_b,
             double *out_yaw_mean, double *out_yaw0_var, double *out_yaw, double *out_vertices,
             ccmpc_stream_t stream);

/* The same outputs with every (cell, t) split over ~n_particles_bound / (n_cells 1024) workgroups
 * in two launches (pass 1: headings and their sums; pass 2: corners and maxima; each
 * (cell, t)'s last arriving workgroup combines the chunks, sums in chunk order, so the result is
 * deterministic).  One workgroup per (cell, t) is issue-bound on its f64 atan2 / division work
 * for large clouds; this form spreads it over the chip.  Workspace: ccmpc_l4_workspace_bytes,
 * 256-byte aligned, its head (arrival counters) zero-filled once; every call leaves it zero. */
size_t ccmpc_l4_workspace_bytes(int64_t T, int64_t n_cells, int64_t n_particles_bound);
int ccmpc_l4_split(const void *positions, int dtype, int64_t ld, int64_t T, const double *origin,
                   const int64_t *cell_off, const int64_t *cell_cnt, int64_t n_cells,
                   int64_t n_particles_bound, const double *past_last, const double *bbox,
                   void *workspace, size_t workspace_bytes, double *out_A, double *out_b,
                   double *out_yaw_mean, double *out_yaw0_var, double *out_yaw,
                   double *out_vertices, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The caller of the path: the planning step's quadratic program,
 * batched over scenes.  Replaces the cvxpy + CPLEX problem of do_highlevel_control
 * (v8ideal/__init__.py:2850-2930, :2999-3012, :3040-3110) with the road-boundary MILP off (the reference
 * default, :217), so the problem is a convex QP in the controls u (2T values):
 *   state      x = Gamma_f (u - u_bar) + x_bar + Gamma_p u_prev            (:2877-2891)
 *   bounds     [min_a, -max_delta] <= (u[2t], u[2t+1]) <= [max_a, max_delta]  (:2874-2878)
 *              0 <= v_t <= max_v                                           (:610-626)
 *   obstacles  every record with status 0:  n . x_t >= d (side +1) or <= d (side -1)
 *              (Minkowski :926-939; affine: rhs, :1503-1515 with S_big = 0)
 *   objective  w_final |X_{T-1} - goal|^2 + sum_t w_ref |X_t - ref_t|^2
 *              + sum_t U_t^T R1 U_t + sum_{t>=1} dU_t^T R2 dU_t                (:2478-2507)
 * U = cp.reshape(u, (T, 2)) in the objective uses cvxpy's default column-major order
 * (U_t = (u[t], u[T+t]), CCMPC_U_ORDER_F) in the reference, while the bounds and Gamma's columns
 * interleave (accel, steer) per step; CCMPC_U_ORDER_C pairs the objective the same way.
 * Solved by a primal-dual interior point method (Mehrotra predictor-corrector), one workgroup
 * per scene, the whole iteration in LDS, then polished: the equality-constrained QP on the
 * IPM's active set, kept only when it is a verified KKT point (T <= 32; beyond, the IPM's
 * answer at tol).
 * ------------------------------------------------------------------------------------- */
#define CCMPC_U_ORDER_F 0
#define CCMPC_U_ORDER_C 1
#define CCMPC_REC_KIND_HALFSPACE 0 /* ccmpc_halfspace records [cells][T(T-1)/2] */
#define CCMPC_REC_KIND_AFFINE 1    /* ccmpc_affine_rec records [cells][T] */
/* the same records packed as ccmpc_gather_rec (ccmpc_compact_records): what the multi-GPU
 * record exchange moves, and what the QP can read in place after it */
#define CCMPC_REC_KIND_HALFSPACE_COMPACT 2
#define CCMPC_REC_KIND_AFFINE_COMPACT 3

/* QP status per scene */
#define CCMPC_QP_OK 0
#define CCMPC_QP_MAXITER 1      /* no verified solution within max_iter: infeasible (the
                                   reference returns InSimulationException, :3099-3110)   */
#define CCMPC_QP_NUMERIC 2      /* the objective's Hessian is not positive definite       */
#define CCMPC_QP_SKIPPED_ROWS 4 /* flag: records with status != 0 were left out */

/* QP method (environment CCMPC_QP_METHOD = "gi" / "ipm", read per ccmpc_mpc_qp call):
 * the Goldfarb-Idnani dual active-set method for n = 2T <= 16 (one wave per scene), the
 * Mehrotra interior point + active-set polish otherwise (and where the active-set solve
 * exceeds its step budget).  Both return the problem's unique minimiser (strictly convex). */
#define CCMPC_QP_METHOD_IPM 0
#define CCMPC_QP_METHOD_GI 1

typedef struct ccmpc_mpc_params {
  double w_final, w_ref;                     /* objective weights (:93-102)          */
  double w_accel, w_joint, w_turning;        /* R1                                   */
  double w_ch_accel, w_ch_joint, w_ch_turning; /* R2                                 */
  double min_a, max_a, max_delta, max_v;     /* control / speed limits (:88-109)     */
} ccmpc_mpc_params;

/* LTV model of the ego vehicle about u_init = 0, the only linearisation input the planner
 * uses (make_local_params, v8ideal/__init__.py:537-557 -> dynamics/bicycle_v2.py
 * VehicleModel.get_optimization_ltv :261-308).  Per scene:
 *  x_init[s][4] = [x, y, psi, v];  out_xbar[s][4T] = X_bar[1:];  out_gamma[s][4T][2T]. */
int ccmpc_mpc_ltv(const double *x_init, int64_t n_scenes, int64_t T, double Ts, double l_r,
                  double L, double *out_xbar, double *out_gamma, ccmpc_stream_t stream);

/* Workspace for scenes holding at most max_cells_per_scene cells of records. */
size_t ccmpc_mpc_qp_workspace_bytes(int64_t n_scenes, int64_t T, int64_t max_cells_per_scene,
                                    int rec_kind);

/* One QP per scene s, horizon T <= T_full, T_prev = T_full - T steps already executed:
 *  gamma[s][4 T_full][2 T_full], xbar[s][4 T_full]  (the full-horizon model of the first step)
 *  ubar[s][2 T_full] or NULL (= 0, u_init = 0);  u_prev[s][2 T_prev] or NULL when T_prev = 0
 *  goal[s][2];  ref[s][n_ref][2] (step t uses ref[min(t, n_ref - 1)], :2492-2501)
 *  rec: records of every scene's cells, scene s owning cells [scene_cell[s], scene_cell[s+1]),
 *       128-byte records (rec_kind CCMPC_REC_KIND_HALFSPACE / _AFFINE) or their 32-byte
 *       ccmpc_gather_rec packing (_HALFSPACE_COMPACT / _AFFINE_COMPACT): the same solve
 *  params: HOST pointer.
 *  out_u[s][2T] (the cvxpy variable u), out_x[s][T][4], out_cost[s], out_status[s],
 *  out_iter[s] (IPM iterations). */
int ccmpc_mpc_qp(int64_t n_scenes, int64_t T, int64_t T_full, const double *gamma,
                 const double *xbar, const double *ubar, const double *u_prev,
                 const double *goal, const double *ref, int64_t n_ref, const void *rec,
                 int rec_kind, const int64_t *scene_cell, int64_t max_cells_per_scene,
                 const ccmpc_mpc_params *params, int u_order, int32_t max_iter, double tol,
                 void *workspace, size_t workspace_bytes, double *out_u, double *out_x,
                 double *out_cost, int32_t *out_status, int32_t *out_iter,
                 ccmpc_stream_t stream);

/* ccmpc_mpc_qp with the LTV rebuild fused in (the planning frame at Tsh == ph: one launch
 * instead of ccmpc_mpc_ltv then ccmpc_mpc_qp).  Each scene's model about u = 0 is computed from
 * ltv->x_init[s][4] with ccmpc_mpc_ltv's arithmetic (the same bits), written to gamma / xbar
 * (OUTPUTS here, [s][4 T_full][2 T_full] and [s][4 T_full]: later frames pass them to
 * ccmpc_mpc_qp) and used by the solve without reading them back. */
typedef struct ccmpc_qp_ltv {
  const double *x_init; /* device, [n_scenes][4] */
  double Ts, l_r, L;
} ccmpc_qp_ltv;
int ccmpc_mpc_qp_ltv(const ccmpc_qp_ltv *ltv, int64_t n_scenes, int64_t T, int64_t T_full,
                     double *gamma, double *xbar, const double *u_prev, const double *goal,
                     const double *ref, int64_t n_ref, const void *rec, int rec_kind,
                     const int64_t *scene_cell, int64_t max_cells_per_scene,
                     const ccmpc_mpc_params *params, int u_order, int32_t max_iter, double tol,
                     void *workspace, size_t workspace_bytes, double *out_u, double *out_x,
                     double *out_cost, int32_t *out_status, int32_t *out_iter,
                     ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Monte-Carlo audit of a plan and of constraint records on the particles they were built from.
 * No reference counterpart (as ccmpc_compact_records): the reference computes an analytic
 * lower bound per record and never counts particles; this call gives the empirical number to
 * set beside it.  One streaming pass over planes 0 .. 2T-1 of the store (T may be smaller than
 * the horizon the store holds), the bytes ccmpc_moments reads, reduced to integers per cell.
 * World position of particle i of cell c at step t: the stored pair (F64), or
 * (double)rel + origin[c] per coordinate (F32; origin NULL = 0).
 *
 * Plan half (plan != NULL):
 *  plan[r][T][2]    ego positions (the first two columns of ccmpc_mpc_qp's out_x), float64
 *  cell_plan[c]     the plan row cell c is audited against (NULL -> row 0), as cell_ref
 *  In float64, in this order: dx = px - plan_x, dy = py - plan_y, d2 = dx*dx + dy*dy;
 *  a particle is hit at step t iff d2 < R*R (strict).
 *  out_hit[c][T]      particles of cell c hit at step t
 *  out_hit_any[c]     particles hit at any t < T (the event the per-mode risk budget bounds)
 *  out_min_d2[c][T]   the smallest d2, +inf for an empty cell
 *
 * Record half (rec != NULL): rec[c][P] of rec_kind CCMPC_REC_KIND_HALFSPACE / _AFFINE or their
 * _COMPACT packing, P = T(T-1)/2 (half-space kinds) or T (affine kinds).  Of a record only
 * n0, n1, rhs (the half-space record's d, the affine record's rhs, as ccmpc_compact_records),
 * side, status and its step t (t_tau >> 16 for the half-space kinds, else t / t_tau) are read.
 * A record protects a particle when the ego may stand anywhere on the record's feasible side
 * and still be at least R away: with s = n0*px + n1*py and v = side * (rhs - s),
 *   protected iff v >= 0 && v*v >= (R*R) * (n0*n0 + n1*n1)     (no square root)
 *  out_rec_open[c][P] particles of the cell the record does not protect at its step; -1 for a
 *                     record with status != 0 or t outside [0, T): such a record indexes no
 *                     plane and protects nothing
 *  out_open[c][T]     particles protected by no status-0 record of (c, t); the whole cell
 *                     where (c, t) has none (t = 0 of the half-space kinds)
 * If the plan satisfies every status-0 record of (c, t), every hit particle is open there:
 * out_hit[c][t] <= out_open[c][t].
 *
 * plan == NULL skips the three plan outputs, rec == NULL the two record outputs (those
 * pointers may then be NULL); both NULL is CCMPC_ERR_ARG, as are T outside [1, 40], R not
 * finite or <= 0, an unknown rec_kind, ld not a multiple of 4 and a missing output of an
 * enabled half.  cell_off entries must be multiples of 4, as for ccmpc_moments.
 * n_particles_bound >= sum(cell_cnt) sizes the grid; counts and offsets are read on the device.
 * Outputs need no initialisation: the call is two launches (initial values, then the pass),
 * no workspace.  Counts are integer atomics and min_d2 an unsigned integer minimum on the bit
 * pattern of the non-negative double, so the result does not depend on execution order.
 * ------------------------------------------------------------------------------------- */
int ccmpc_risk_audit(const void *positions, int dtype, int64_t ld, int64_t T,
                     const double *origin, const int64_t *cell_off, const int64_t *cell_cnt,
                     int64_t n_cells, int64_t n_particles_bound, const double *plan,
                     const int32_t *cell_plan, const void *rec, int rec_kind, double R,
                     int64_t *out_hit, int64_t *out_hit_any, double *out_min_d2,
                     int64_t *out_rec_open, int64_t *out_open, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The same audit on the samples of the ideal rollout, which are never materialised: the
 * shrinking-horizon frames (T < ph) build their constraints from ccmpc_ideal_minkowski_cycle's
 * rollout, which exists only in registers, so there is no store for ccmpc_risk_audit to read.
 *
 * The contract: the outputs equal those of ccmpc_ideal_rollout (Z = NULL, the same prev_mean,
 * prev_cov, T_src, src_cell, T, n_samples, x0, seed and rng_cell) followed by ccmpc_risk_audit
 * on that store with cell_cnt[c] = n_samples for every cell and the same plan, cell_plan, rec,
 * rec_kind and R.  Consequences:
 *  - every count is equal count for count and out_min_d2 is equal bit for bit: the samples are
 *    regenerated in registers by the rollout's own arithmetic (a sample is a pure function of
 *    (seed, rng_cell[c], i, t) and the source moments) and tested by the audit's own;
 *  - out_status[c] (nullable) is the rollout's status, and a failed cell obeys the same
 *    sentence: its slots are NaN from the first failed step on, and a NaN position is hit by
 *    nothing (it does not enter out_min_d2 either) and protected by nothing (it is open for
 *    every record of that step);
 *  - sharding invariance: the cells of one call give the same outputs as the same cells in
 *    several calls with the matching rng_cell (and src_cell, x0, cell_plan, rec) slices.
 * Rollout arguments as ccmpc_ideal_minkowski_cycle_ex: noise from Philox only, x0 and seed_dev
 * nullable (seed_dev, device memory, overrides seed, so a captured graph audits a fresh seed
 * per replay), rng_cell NULL = stream c.  Audit arguments and outputs as ccmpc_risk_audit with
 * N = n_samples for every cell.
 *
 * CCMPC_ERR_ARG, all checked before any device call: T_src outside [2, 40], T outside
 * [1, T_src - 1], n_cells outside [0, 65536), n_samples outside [1, 2^32), R not finite or
 * <= 0, an unknown rec_kind when rec != NULL, plan and rec both NULL, a missing output of an
 * enabled half.  n_cells == 0 returns CCMPC_OK.  The call is two launches (initial values,
 * then the pass) with no workspace; it never synchronises and never reads device memory on
 * the host, so it can be captured, and outputs need no initialisation.  Counts are integer
 * atomics and out_min_d2 an unsigned integer minimum on the bit pattern of the non-negative
 * double: no output bit depends on execution order.
 * ------------------------------------------------------------------------------------- */
int ccmpc_ideal_risk_audit(const double *prev_mean, const double *prev_cov, int64_t T_src,
                           const int32_t *src_cell, int64_t n_cells, int64_t T,
                           int64_t n_samples, const double *x0, uint64_t seed,
                           const uint64_t *seed_dev, const int32_t *rng_cell,
                           const double *plan, const int32_t *cell_plan, const void *rec,
                           int rec_kind, double R, int64_t *out_hit, int64_t *out_hit_any,
                           double *out_min_d2, int64_t *out_rec_open, int64_t *out_open,
                           int32_t *out_status, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Monte-Carlo calibration of half-space offsets to a risk budget: which offset would leave at
 * most cell_allow[c] particles of the cell open?  The companion of ccmpc_risk_audit (no
 * reference counterpart): an exact batched selection, one order statistic per record, on the
 * planes the audit streams.  Store arguments (positions .. n_particles_bound), rec / rec_kind,
 * R and the fields read of a record (n0, n1, rhs, side, status, its step t) are the audit's,
 * with the same F32 rule (double)rel + origin[c]; P = T(T-1)/2 (half-space kinds) or T.
 *  cell_allow[c]   device int64, NULL = all zeros: the number m of particles of cell c a
 *                  record may leave open (e.g. floor(eps_ura / ph * N_c))
 *
 * All arithmetic is float64, in the stated order, with no contraction.  A record is calibrated
 * when status == 0, 0 <= t < T, and n0 and n1 are finite and not both non-finite.  For a
 * calibrated record of cell c take N = cell_cnt[c] and m = cell_allow[c]; a negative m is an
 * argument error, detected on the device and reported per record as SKIPPED (the call never
 * reads device memory on the host).
 *  Projection of particle i: s_i = n0*px + n1*py (the audit's s, from the world position at
 *  step t), w_i = side*s_i + 0.0 (the + 0.0 makes -0 a +0, so bit order equals value order).
 *  out_q[c][P]      when m < N: the (m+1)-th largest w_i, i.e. the element at index N-1-m of the
 *                   ascending sort.  Its bits are exact: each w_i is two products and one sum,
 *                   no evaluation order can change it.
 *  out_rhs[c][P]    side*u*, where u* is the smallest double u for which the audit's own
 *                   predicate protects a particle with s = side*q under rhs = side*u:
 *                     v = side*(rhs - s);  v >= 0 && v*v >= (R*R)*(n0*n0 + n1*n1)
 *                   The predicate is monotone in u, so u* is unique and the output is
 *                   bit-comparable (+inf where no double satisfies it).
 *  out_status[c][P] int32: 0 calibrated;
 *                   CCMPC_CAL_VACUOUS: m >= N, empty cells included -- nothing needs
 *                   protecting: out_q = -inf, out_rhs = the record's own rhs, copied;
 *                   CCMPC_CAL_SKIPPED: the record is not calibrated: out_q = NaN, out_rhs =
 *                   the record's own rhs.
 * Consequences: feed the record back to ccmpc_risk_audit with rhs replaced by out_rhs.  Every
 * particle with w_i <= q is then protected, so its rec_open is at most #{i : w_i > q} <= m --
 * exactly that number unless some w_i > q lies within the rounding of u* - q.  With u* moved
 * one ulp towards the particles, rec_open is >= #{w_i >= q} > m.
 * Positions are assumed finite; non-finite projections give unspecified values but no
 * out-of-range access.
 *
 * CCMPC_ERR_ARG: T outside [1, 40], R not finite or <= 0, an unknown rec_kind, ld not a
 * multiple of 4, a NULL output (none is needed where P == 0: T = 1 of the half-space kinds,
 * where the call writes nothing), a workspace smaller than
 * ccmpc_risk_quantile_workspace_bytes(T, rec_kind, n_cells) (which returns 0 for arguments the
 * call rejects) or not 16-byte aligned, n_particles_bound >= 2^32 (counts are 32-bit).
 * The call is capturable: it never synchronises, never reads device memory on the host, and
 * needs neither an initialised workspace nor initialised outputs (its first launch writes the
 * initial values).  The launch sequence is fixed by (T, rec_kind, n_cells, n_particles_bound):
 * the first launch, then 8 x (a counting pass over the store, a narrowing launch); a radix
 * select on the order-preserving 64-bit key of w, 8 bits per pass.  Integer atomics only: no
 * output bit depends on execution order.  Do not share one workspace between concurrent
 * streams.
 * ------------------------------------------------------------------------------------- */
#define CCMPC_CAL_VACUOUS 1
#define CCMPC_CAL_SKIPPED 2
size_t ccmpc_risk_quantile_workspace_bytes(int64_t T, int rec_kind, int64_t n_cells);
int ccmpc_risk_quantile(const void *positions, int dtype, int64_t ld, int64_t T,
                        const double *origin, const int64_t *cell_off, const int64_t *cell_cnt,
                        int64_t n_cells, int64_t n_particles_bound, const void *rec,
                        int rec_kind, double R, const int64_t *cell_allow, void *workspace,
                        size_t workspace_bytes, double *out_q, double *out_rhs,
                        int32_t *out_status, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The same calibration on the samples of the ideal rollout, which are never materialised: the
 * counterpart of ccmpc_ideal_risk_audit for the question "which offset would meet the budget on
 * the samples this shrinking-horizon frame's records were built from?".
 *
 * The contract: out_q, out_rhs and out_status equal, bit for bit, those of ccmpc_ideal_rollout
 * (Z = NULL, the same prev_mean, prev_cov, T_src, src_cell, T, n_samples, x0, seed and rng_cell)
 * followed by ccmpc_risk_quantile on that store with cell_cnt[c] = n_samples for every cell and
 * the same rec, rec_kind, R and cell_allow.  The rollout would cost 16 T n_samples bytes per
 * cell; this call regenerates every sample in registers in each counting pass (a sample is a
 * pure function of (seed, rng_cell[c], i, t) and the source moments) and needs only the
 * workspace of ccmpc_ideal_risk_quantile_workspace_bytes(T, rec_kind, n_cells), which returns 0
 * for arguments the call rejects.
 * Rollout arguments as ccmpc_ideal_risk_audit: seed_dev (device memory, nullable) overrides
 * seed, rng_cell NULL = stream c, x0 nullable.  Record arguments and cell_allow as
 * ccmpc_risk_quantile: the same fields read, the same definition of a calibrated record, the
 * same w, q and u*; N = n_samples for every cell, so m >= n_samples gives CCMPC_CAL_VACUOUS and
 * a negative cell_allow[c], found on the device, CCMPC_CAL_SKIPPED.
 *
 * Failed cells, which the store call leaves unspecified ("positions are assumed finite"), are
 * defined here.  Let f(c) be the first step whose samples are NaN: 0 if the initial draw fails,
 * else the smallest t for which the step's conditional cannot be built (the codes of
 * out_cell_status), else T.  A record of cell c with step t >= f(c) is CCMPC_CAL_SKIPPED
 * (out_q = NaN, out_rhs = the record's own rhs); records with t < f(c) are calibrated and the
 * sentence above holds for them: their samples are finite and are the rollout's bits.
 *  out_cell_status[c]  int32, nullable: the rollout's status.
 * Sharding invariance as ccmpc_ideal_risk_audit: the cells of one call give the same outputs as
 * the same cells in several calls with the matching rng_cell, src_cell, x0, rec and cell_allow
 * slices.
 *
 * CCMPC_ERR_ARG, all checked before any device call: T_src outside [2, 40], T outside
 * [1, T_src - 1], n_cells outside [0, 65536), n_samples outside [1, 2^32), R not finite or
 * <= 0, an unknown rec_kind, rec NULL, a NULL out_q, out_rhs or out_status where P > 0, a
 * workspace that is too small or not 16-byte aligned.  n_cells == 0 returns CCMPC_OK, as does
 * P == 0 (T = 1 of the half-space kinds), which writes at most out_cell_status.
 * The call is capturable: it never synchronises, never reads device memory on the host, and
 * needs neither an initialised workspace nor initialised outputs.  The launch sequence is fixed
 * by (T, rec_kind, n_cells, n_samples): the first launch, then 8 x (a counting pass that
 * generates the samples, a narrowing launch).  A record whose selected bin holds few enough
 * samples has them hand their whole keys over in the next pass and is resolved from that list
 * (the rank-th largest, ties included: a function of the multiset only); passes in which no
 * record of a workgroup is live generate nothing.  Integer atomics only: no output bit depends
 * on execution order.  Do not share one workspace between concurrent streams.
 * ------------------------------------------------------------------------------------- */
size_t ccmpc_ideal_risk_quantile_workspace_bytes(int64_t T, int rec_kind, int64_t n_cells);
int ccmpc_ideal_risk_quantile(const double *prev_mean, const double *prev_cov, int64_t T_src,
                              const int32_t *src_cell, int64_t n_cells, int64_t T,
                              int64_t n_samples, const double *x0, uint64_t seed,
                              const uint64_t *seed_dev, const int32_t *rng_cell,
                              const void *rec, int rec_kind, double R,
                              const int64_t *cell_allow, void *workspace, size_t workspace_bytes,
                              double *out_q, double *out_rhs, int32_t *out_status,
                              int32_t *out_cell_status, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Box-face chance constraints (the "TCST" family): the second-order-cone row data of
 * compute_obstacle_constraints_GMM (v8ideal/__init__.py:966-1094, "nominal"),
 * compute_robust_constraints_GMM (:1096-1229, "robust") and
 * compute_obstacle_constraints_GMM_approx (:1231-1376, nominal rows with ref_traj given), for
 * every (cell, t) in one call.  Replaces the per-(cell, t) loop that stacks the four 3 x N face
 * coefficient arrays (:1058-1061), takes np.mean / np.cov of each and sqrtm (nominal, approx)
 * or sqrt(|C|_F) (robust) of the covariance.
 *
 * Per particle at step t: (x, y) its world position, (c, s) the unit vector of its step delta
 * (ovehicle.py:72-76: p_t - p_{t-1}, step 0 from past_last; formed exactly as ccmpc_l4 forms
 * it, a zero step giving c = 1, s = 0), lon = extent[0], lat = extent[1]:
 *   a1 = (-c,  s,   c x - s y + lat/2)      a3 = ( c, -s,  -c x + s y + lat/2)
 *   a2 = (-s, -c,   s x + c y + lon/2)      a4 = ( s,  c,  -s x - c y + lon/2)
 * Face f (0..3 for a1..a4) of (cell, t):  mean_f . xi + Gamma |root_f xi|_2 + 0.5 car_r <= ...
 * with xi = (X, Y, 1), mean_f = the particle mean of a_f, C_f its covariance (ddof = 1),
 * root_f = sqrtm(C_f) (CCMPC_FACE_NOMINAL) or sqrt(|C_f|_F) I (CCMPC_FACE_ROBUST), Gamma =
 * cell_gamma[c].  Faces 2 and 3 are the mirror images of 0 and 1 (a3 = -a1 + (0, 0, lat)), so
 * they share C and root with them; only two moment sets are reduced from the particles.
 * The sums run over coefficients shifted by the cell's first particle (its position and its
 * coefficient vector), in float64, chunk partials added in chunk order: bit-reproducible.
 *
 * One record per (cell, t, face), 128 bytes. */
typedef struct ccmpc_face_rec {
  double mean[3];         /* np.mean(a_f, axis=1)                       (:1067-1070)           */
  double root[6];         /* r00 r01 r02 r11 r12 r22 of the symmetric root_f (:1072-1075);
                             robust: s = sqrt(|C_f|_F) on the diagonal, 0 elsewhere (:1205-1208) */
  double C[6];            /* c00 c01 c02 c11 c12 c22 of np.cov(a_f)                             */
  int32_t status;         /* 0, CCMPC_REC_NONFINITE (fewer than 2 particles, or a non-finite
                             moment) or CCMPC_REC_NOT_PSD (an eigenvalue below -64 eps lambda_max;
                             nominal only).  A failed record's numeric fields are all NaN.      */
  uint32_t t_face_chosen; /* (t << 16) | (face << 8) | chosen; chosen = 1 for the face with the
                             smallest left-hand side at xi_ref = (ref_traj[r][t], 1), first index
                             on equality (val.index(min(val)), :1352), 0 for the other three, and
                             CCMPC_FACE_NO_CHOICE where ref_traj is NULL or a face of (c, t) failed */
} ccmpc_face_rec;
#define CCMPC_FACE_NOMINAL 0
#define CCMPC_FACE_ROBUST 1
#define CCMPC_FACE_NO_CHOICE 255u
/*  past_last[c][2]   world-frame past[-1] of the cell's OV, as ccmpc_l4
 *  extent            device, {lon, lat}: the reference hard-codes truck_d = (3.7, 1.79) (:976-977)
 *  cell_gamma[c]     norm.ppf(1 - eps_ura[ov, k] / Tpred) (:1064-1065, :1196-1197, :1330-1331)
 *  ref_traj[r][T][2] nullable; cell c uses row cell_ref[c] (NULL -> 0) (approx, :1343-1352)
 *  car_r             CAR_R = 4.47213 (:978); the rows add 0.5 car_r
 *  out_rec[c][T][4]  written in full by every call: the caller initialises nothing
 * Workspace: ccmpc_face_workspace_bytes (0 for T > 40 or bad arguments), 256-byte aligned, NOT
 * initialised by the caller and holding no counters: two launches, no atomics (the first writes
 * one partial per (cell, t, chunk of 2048 particles), the second, one wave per
 * (cell, t), adds them in chunk order, undoes the shift, and takes the principal root by a
 * cyclic Jacobi eigen-decomposition of 8 sweeps).  The call overwrites the head of its workspace:
 * do not hand it one whose arrival counters another call needs zero (the workspace contract of
 * ccmpc_moments).  cell_off / ld multiples of 4, as ccmpc_moments;
 * n_particles_bound >= sum(cell_cnt) sizes the grid. */
size_t ccmpc_face_workspace_bytes(int64_t T, int64_t n_cells, int64_t n_particles_bound);
int ccmpc_face_constraints(const void *positions, int dtype, int64_t ld, int64_t T,
                           const double *origin, const int64_t *cell_off, const int64_t *cell_cnt,
                           int64_t n_cells, int64_t n_particles_bound, const double *past_last,
                           const double *extent, const double *cell_gamma, const double *ref_traj,
                           const int32_t *cell_ref, int kind, double car_r, void *workspace,
                           size_t workspace_bytes, ccmpc_face_rec *out_rec, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Monte-Carlo audit of the box-face rows on the particles they were built from: of the
 * particles of (cell, t), how many violate face f's inequality at a plan?  The companion of
 * ccmpc_risk_audit for the cone rows (no reference counterpart): the analytic row bounds that
 * fraction by eps_ura / Tpred under a Gaussian assumption, this call counts it.  One streaming
 * pass over planes 0 .. 2T-1 of the store (T may be smaller than the horizon the store holds).
 *
 * Store arguments (positions .. n_particles_bound), past_last and extent = {lon, lat} are those
 * of ccmpc_face_constraints, with the same F32 rule (double)rel + origin[c].
 *  plan[r][T][ld_plan]  ego positions: x, y = the first two of each step's ld_plan doubles
 *                       (ld_plan = 4 reads ccmpc_mpc_qp's out_x in place, as ccmpc_face_cuts;
 *                       ld_plan >= 2)
 *  cell_plan[c]         the plan row cell c is audited against (NULL -> row 0)
 *  face_sel[c][T]       nullable.  0..3: that face is the row of (c, t); any other value: (c, t)
 *                       has no row (the cells of ungated OVs, -1 in the planner)
 *
 * Per particle of cell c at step t, in float64, with no contraction, products before sums:
 *   (x, y)  its world position;  (c, s) the unit vector of its step delta exactly as
 *           ccmpc_face_constraints forms it (step 0 from past_last, a zero step gives c = 1,
 *           s = 0)
 *   ex = X - x,  ey = Y - y                     (X, Y) = plan[cell_plan[c]][t]
 *   p  = c*ex - s*ey,   q = s*ex + c*ey
 *   hlat = 0.5*lat + 0.5*car_r,   hlon = 0.5*lon + 0.5*car_r
 *   v0 = hlat - p,  v1 = hlon - q,  v2 = hlat + p,  v3 = hlon + q
 * In exact arithmetic v_f = a_f . (X, Y, 1) + 0.5 car_r with a1..a4 of ccmpc_face_constraints;
 * the relative form avoids the cancellation of the ~200 m terms.  Face f's inequality holds for
 * the particle iff v_f <= 0; the particle is open under face f iff v_f > 0 (strict).
 *
 * Outputs, all written in full by every call (the caller initialises nothing):
 *  out_face_open[c][T][4]  particles of the cell with v_f > 0
 *  out_in_box[c][T]        particles with all four v_f > 0: the ego point lies inside that
 *                          particle's inflated box, so no choice of face protects it
 *  out_in_box_any[c]       particles in the box at any t < T
 *  out_sel_open[c][T]      out_face_open at the selected face; -1 where (c, t) has no row
 *  out_sel_open_any[c]     particles open under the selected row at any step that has one: the
 *                          event the per-mode budget eps_ura bounds, which the rows split by
 *                          / Tpred; 0 if no step has a row
 *  out_worst[c][T][4]      the largest v_f over the cell's particles, -inf for an empty cell:
 *                          the shift that would make row f hold for every particle; <= 0 iff the
 *                          row holds for all of them
 * face_sel == NULL skips the two sel outputs (their pointers may then be NULL); out_worst may be
 * NULL and is then skipped; the other three outputs are required.
 *
 * CCMPC_ERR_ARG, all checked on the host before any launch: T outside [1, 40], ld not a positive
 * multiple of 4, ld_plan < 2, car_r not finite, n_cells < 0, a NULL positions, cell_off,
 * cell_cnt, past_last, extent, plan or required output, a non-NULL face_sel with a NULL sel
 * output.  cell_off entries must be multiples of 4, as for ccmpc_moments;
 * n_particles_bound >= sum(cell_cnt) sizes the grid; counts and offsets are read on the device.
 * Two launches (initial values, then the pass), no workspace, no host synchronisation: the call
 * is capturable.  Counts are integer atomics.  out_worst is an unsigned 64-bit atomic maximum on
 * the order-preserving key of the double (ccmpc_risk_quantile's key), applied to the double's
 * own bits: a signed integer maximum for a sign-clear pattern, an unsigned integer minimum for a
 * sign-set one, each of which raises the stored pattern's key to the larger of the two.  No
 * output bit depends on execution order.  Positions are assumed finite; non-finite ones give
 * unspecified values but no out-of-range access.
 * ------------------------------------------------------------------------------------- */
int ccmpc_face_audit(const void *positions, int dtype, int64_t ld, int64_t T,
                     const double *origin, const int64_t *cell_off, const int64_t *cell_cnt,
                     int64_t n_cells, int64_t n_particles_bound, const double *past_last,
                     const double *extent, double car_r, const double *plan, int64_t ld_plan,
                     const int32_t *cell_plan, const int32_t *face_sel,
                     int64_t *out_face_open, int64_t *out_in_box, int64_t *out_in_box_any,
                     int64_t *out_sel_open, int64_t *out_sel_open_any, double *out_worst,
                     ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Outer-approximation (Kelley) cuts of the box-face cone rows: what turns ccmpc_face_rec rows
 * into records ccmpc_mpc_qp reads.  The reference hands the rows to cvxpy / CPLEX as
 * second-order cones (v8ideal/__init__.py:1353-1363); with one face fixed per (cell, t) -- the
 * approx generator's choice, or the caller's -- each row is convex in the ego position of step t,
 *   g(x_t) = mean . xi + Gamma |root xi|_2 + 0.5 car_r <= 0,   xi = (X_t, Y_t, 1),
 * and the plan follows from the strictly convex planning QP over linearisations of g: cut every
 * row at the current plan, solve the QP over all cuts so far, repeat until max g <= tol_g.  The
 * cuts are an outer approximation, so a QP that is infeasible in some round certifies that the
 * cone programme is infeasible.  One call = one round's cuts for every scene, one launch.
 *
 *  rec[cells][T][4]   ccmpc_face_constraints' records;  scene s owns cells
 *                     [scene_cell[s], scene_cell[s+1])  (device, as ccmpc_mpc_qp)
 *  face_sel[cells][T] 0..3: that face; -1: no row for (cell, t) (an OV outside the junction
 *                     gate); NULL: the face whose record has chosen == 1
 *  cell_gamma[cells]  Gamma, as ccmpc_face_constraints;  car_r likewise
 *  plan[s][T][ld_plan] the point to linearise at: x, y = the first two of each step's ld_plan
 *                     doubles (ld_plan = 4 reads ccmpc_mpc_qp's out_x in place; ld_plan >= 2)
 *
 * A selected record with status != 0, a face_sel outside [-1, 3], and (face_sel == NULL) a
 * (cell, t) whose records carry CCMPC_FACE_NO_CHOICE or no chosen face make the scene's state
 * CCMPC_SOCP_BAD_ROW: no cuts are written for it, in this or any later round.
 *
 * Arithmetic of a row at p = (x, y) = plan[s][t], float64, no contraction, in this order
 * (products before sums, sums left to right; root = r00 r01 r02 r11 r12 r22):
 *   w0 = r00 x + r01 y + r02,  w1 = r01 x + r11 y + r12,  w2 = r02 x + r12 y + r22
 *   nw = sqrt(w0 w0 + w1 w1 + w2 w2)
 *   g  = m0 x + m1 y + m2 + Gamma nw + 0.5 car_r
 *   v0 = r00 w0 + r01 w1 + r02 w2,  v1 = r01 w0 + r11 w1 + r12 w2
 *   a  = (m0 + Gamma v0 / nw, m1 + Gamma v1 / nw), or (m0, m1) where nw == 0 (a valid subgradient)
 *   b  = a0 x + a1 y - g
 * The cut a . x_t <= b is stored as n = a, rhs = b, side = -1, status = 0, t_tau = t.  It
 * supports g at p (a . p - b = g(p)) and lies below it everywhere (a . q - b <= g(q)).
 *
 * Pool: scene s owns pool cells [pool_cell[s], pool_cell[s+1]), which must number
 * (max_rounds + 1) x the scene's cells: region r = cells [r cells_s, (r + 1) cells_s) of T
 * records, record t of a cell belonging to step t.  The call with `round` = r writes region r in
 * full -- a cut or an empty record (status CCMPC_CUT_EMPTY, n = rhs = 0) per (cell, t) -- and the
 * call with round == 0 also empties every later region: the caller initialises nothing.
 * ccmpc_mpc_qp reads the pool in place with rec_kind CCMPC_REC_KIND_AFFINE_COMPACT, scene_cell =
 * pool_cell and max_cells_per_scene = (max_rounds + 1) x the largest scene; it skips the empty
 * records (and raises CCMPC_QP_SKIPPED_ROWS, which means nothing here).  A scene whose pool
 * range has another size gets CCMPC_SOCP_BAD_LAYOUT and its pool is not touched.
 *
 * Outputs, all written by every call (no initial values needed):
 *  out_g[cells][T]  g of the selected row; -inf where face_sel is -1, NaN for a bad row
 *  out_viol[s]      the largest g of the scene's selected rows, -inf if it has none, NaN if a
 *                   row is bad or some g is NaN
 *  out_state[s]     sticky: read back by the calls with round > 0.
 *                   CCMPC_SOCP_CUT      cuts were written (always in round 0, which judges the
 *                                       linearisation point, not a plan of the programme);
 *                   CCMPC_SOCP_OK       round > 0 and out_viol[s] <= tol_g: this call and every
 *                                       later one write only empty records for the scene, so its
 *                                       QP stays the same problem and returns the same bits;
 *                   CCMPC_SOCP_BAD_ROW, CCMPC_SOCP_BAD_LAYOUT as above.
 * only_violated != 0: rounds >= 1 write a cut only for rows with g > 0 (the others cannot
 * be active at the next plan's neighbourhood; fewer QP rows, possibly more rounds).
 *
 * One workgroup of one wave per scene, the maximum reduced in the wave (exact, so no order can
 * change it), no atomics, no workspace, no host synchronisation: capturable.
 * CCMPC_ERR_ARG: T outside [1, 40], tol_g or car_r not finite, max_rounds < 0 or >= 2^15, round
 * outside [0, max_rounds], ld_plan < 2, n_scenes outside [0, 2^31), a NULL pointer other than
 * face_sel, pool not 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
#define CCMPC_SOCP_OK 0
#define CCMPC_SOCP_CUT 1
#define CCMPC_SOCP_BAD_ROW 2
#define CCMPC_SOCP_BAD_LAYOUT 3
#define CCMPC_CUT_EMPTY 1 /* ccmpc_gather_rec.status of a pool record that holds no cut */
int ccmpc_face_cuts(const ccmpc_face_rec *rec, int64_t T, int64_t n_scenes,
                    const int64_t *scene_cell, const int32_t *face_sel, const double *cell_gamma,
                    double car_r, const double *plan, int64_t ld_plan, int32_t round,
                    int32_t max_rounds, double tol_g, int32_t only_violated,
                    ccmpc_gather_rec *pool, const int64_t *pool_cell, double *out_g,
                    double *out_viol, int32_t *out_state, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Monte-Carlo calibration of the box-face rows to a risk budget: by how far does face f's row
 * of (cell, t) miss, or clear, a budget of cell_allow[c] open particles at a plan -- and which
 * half-space would meet it?  The companion of ccmpc_face_audit (which counts) as
 * ccmpc_risk_quantile is of ccmpc_risk_audit; no reference counterpart.  An exact order
 * statistic of ccmpc_face_audit's face values on the particle store.
 *
 * Store arguments (positions .. n_particles_bound), past_last, extent, car_r, plan, ld_plan and
 * cell_plan are exactly those of ccmpc_face_audit, with the same F32 rule.
 *  cell_allow[c]   device int64, NULL = all zeros: the number m of particles of cell c a row
 *                  may leave open (as ccmpc_risk_quantile)
 *  margin          >= 0 and finite: subtracted from every cut's rhs (below)
 *
 * The values v_f, f = 0..3, of every particle of (cell, t) are ccmpc_face_audit's, word for
 * word: ex, ey, p, q, hlat, hlon, v0..v3 in float64 with no contraction, products before sums,
 * the heading as ccmpc_face_constraints forms it.  Both calls evaluate one shared inline
 * function, so they form the same bits.  N = cell_cnt[c], m = cell_allow[c].
 *
 * Outputs, all written in full by every call (neither they nor the workspace need initial
 * values):
 *  out_q[c][T][4]     double.  m < N: the (m+1)-th largest v_f + 0.0 over the cell's particles
 *                     at step t, i.e. index N-1-m of the ascending sort by the order-preserving
 *                     key (the + 0.0 makes -0 a +0, so bit order equals value order).  It is the
 *                     distance in metres along face f's normal by which the row misses (> 0) or
 *                     clears (<= 0) the budget at this plan: #{v_f > q} <= m by construction, so
 *                     out_face_open[c][t][f] <= m  <=>  q <= 0.  With m = 0 it is out_worst.
 *  out_arg[c][T][4]   int64: the index within the cell of the particle that attains q; among
 *                     particles whose value has q's bits, the lowest index.  -1 where nothing is
 *                     selected.
 *  out_cut[c][T][4]   ccmpc_gather_rec: the half-space n . x <= rhs on which that particle's own
 *                     face inequality v_f(x) <= 0 holds, shifted to the budget.  n is the gradient
 *                     of v_f in (X, Y): (-c, s), (-s, -c), (c, -s), (s, c) for f = 0..3, (c, s)
 *                     the arg particle's heading (the same bits the selection used).  With
 *                     P = (X, Y) the plan point of (c, t), in this order:
 *                       rhs = ((n0*X + n1*Y) - q) - margin
 *                     so n . P - rhs = q + margin up to rounding.  side = -1, t_tau = t, status
 *                     0, as ccmpc_face_cuts writes its cuts.  The record is empty (status
 *                     CCMPC_CUT_EMPTY, n = rhs = 0) where q + margin <= 0 (the row already meets
 *                     the budget) or nothing is selected; ccmpc_mpc_qp skips empty records.
 *                     Where all particles of the cell share a heading, v_f is one affine
 *                     function of the plan point shifted per particle, q is affine in the plan
 *                     and the cut is exact; with differing headings {x : q(x) <= 0} is not convex
 *                     in general and the cut is the selected particle's constraint only.
 *  out_status[c][T]   int32.  0: a value was selected.  CCMPC_CAL_VACUOUS: m >= N, empty cells
 *                     included: q = -inf, arg = -1, empty cuts.  CCMPC_CAL_SKIPPED: m < 0,
 *                     detected on the device: q = NaN, arg = -1, empty cuts.
 *
 * Workspace: ccmpc_face_quantile_workspace_bytes(T, n_cells) bytes (0 for arguments the call
 * rejects), 16-byte aligned: 1048 bytes per (cell, t, face), never a function of the particle
 * count.  Do not share one workspace between concurrent streams.
 * Launches, fixed by (T, n_cells, n_particles_bound): the initial values; 8 x (a counting pass
 * over the store, a narrowing launch) -- ccmpc_risk_quantile's radix select on the 64-bit key, 8
 * bits per pass, on ccmpc_face_audit's streaming geometry, in chunks of 8 steps x 4 faces; one
 * more pass that finds the lowest index holding q's bits; the cuts.  Every pass forms the
 * headings again.  Integer atomics only (32-bit adds and minima): no output bit depends on
 * execution order.  No host synchronisation, no host read of device memory: capturable.
 *
 * CCMPC_ERR_ARG, all checked on the host before any launch: those of ccmpc_face_audit (T outside
 * [1, 40], ld not a positive multiple of 4, ld_plan < 2, car_r not finite, n_cells < 0, a NULL
 * positions, cell_off, cell_cnt, past_last, extent, plan or output), margin negative or not
 * finite, a workspace that is too small, NULL (n_cells > 0) or not 16-byte aligned,
 * n_particles_bound >= 2^32 (counts and indices are 32-bit).  Positions are assumed finite;
 * non-finite ones give unspecified values but no out-of-range access.
 * ------------------------------------------------------------------------------------- */
size_t ccmpc_face_quantile_workspace_bytes(int64_t T, int64_t n_cells);
int ccmpc_face_quantile(const void *positions, int dtype, int64_t ld, int64_t T,
                        const double *origin, const int64_t *cell_off, const int64_t *cell_cnt,
                        int64_t n_cells, int64_t n_particles_bound, const double *past_last,
                        const double *extent, double car_r, const double *plan, int64_t ld_plan,
                        const int32_t *cell_plan, const int64_t *cell_allow, double margin,
                        void *workspace, size_t workspace_bytes, double *out_q, int64_t *out_arg,
                        ccmpc_gather_rec *out_cut, int32_t *out_status, ccmpc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * TEST ONLY (not a reference interface): the half-space tail's device functions -- the ones
 * ccmpc_minkowski_cycle / ccmpc_minkowski / ccmpc_affine_scale run per record -- on n batched
 * inputs, so the reference's component golden vectors reach the device arithmetic.  Device
 * pointers, float64, row-major 2x2 matrices (a, b, c, d):
 *  MVOE     in[n][8]  = S1, S2                 out[n][6]  = beta, Q, ok (1/0)
 *           (compute_mvoe, makeconstraint.py:7-38; tol / maxiter as the cycle's)
 *  TANGENT  in[n][10] = mu[2], Sigma, c, m, a[2]  out[n][5] = n[2], d, which, status (0 or
 *           CCMPC_REC_NO_TANGENT)  (choose_closest_tangent, makeconstraint.py:134-207)
 *  BOUND    in[n][14] = cov_infer, cov_mu, cov_t, Gamma, chi_p   out[n][2] = lower bound,
 *           scale  (compute_lower_bound / compute_scale, makeconstraint.py:259-303)
 *  PAIR     in[n][18] = 4x4 cov of (x_tau, y_tau, x_t, y_t), Gamma, chi_p
 *           out[n][14] = cov_infer, cov_mu, cov_t, lower bound, scale
 *           (predict_moments, makeconstraint.py:41-70, then BOUND)
 *  PRIM     in[n][2]  = a, b      out[n][4] = rcp_nr(b), div_nr(a, b), sqrt_gs(b), and one
 *           update of the MVOE fixed point from beta = a with s = b, p2 = 1
 *           (the hand-made reciprocal / division / square root of the MVOE chain)
 *  CHAIN    in[n][8]  = S1, S2    out[n][5] = s = tr(S1^-1 S2), p2 = 2 det(S1^-1 S2), beta,
 *           ok (1/0), beta before the last update
 *           (compute_mvoe's set-up and fixed point before Q is formed; no NaN selects)
 * ------------------------------------------------------------------------------------- */
#define CCMPC_SELFTEST_MVOE 0
#define CCMPC_SELFTEST_TANGENT 1
#define CCMPC_SELFTEST_BOUND 2
#define CCMPC_SELFTEST_PAIR 3
#define CCMPC_SELFTEST_PRIM 4
#define CCMPC_SELFTEST_CHAIN 5
int ccmpc_selftest(int kind, int64_t n, const double *in, double *out, double tol,
                   int32_t maxiter, ccmpc_stream_t stream);

/* Test aid: fill every CU's LDS with `value` (tests/test_gpu_lds_poison.py runs the kernels
 * after NaN and after zero fills and requires the same bits: no kernel reads LDS it did not
 * write). */
int ccmpc_poison_lds(double value, ccmpc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CCMPC_H */
