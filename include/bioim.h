/*
 * bioim.h — C-ABI of the MI355X-native vectorized env step (libbioim.so).
 *
 * This is the drop-in boundary for the reference's physics facade
 * `OsimModel` (bioimitation/imitation_envs/utils/opensim_wrapper.py:6-338)
 * plus the per-step env arithmetic layered on it by the task envs
 * (muscle_walking_imitation_env2D.py:115-403, torque_walking_imitation_env2D.py:117-366)
 * and by `OsimEnv.step/reset` (opensim_environment.py:86-113).  One handle
 * owns N independent environment instances of one registered env ID on one
 * GPU; every call advances/reads all of them (a batched `env.step`).
 *
 * Each entry point cites the reference interface it replaces:
 *
 *   bioim_create   <- OsimEnv.__init__ -> OsimModel.__init__ (opensim_wrapper.py:7-90),
 *                     per instance, N times
 *   bioim_reset    <- Env.reset (muscle_walking_imitation_env2D.py:133-156) =
 *                     OsimModel.reset/set_time/set_coordinates/set_velocities
 *                     (opensim_wrapper.py:293-332) + get_observation
 *   bioim_step     <- Env.step (muscle_walking_imitation_env2D.py:115-131) ->
 *                     OsimEnv.step (opensim_environment.py:100-113) =
 *                     actuate (opensim_wrapper.py:92-107) + integrate (:299-301)
 *                     + get_state_dict/get_reward/is_done
 *   bioim_get_state/bioim_set_state <- (no reference equivalent; the env
 *                     state is not checkpointable upstream) parity re-sync,
 *                     checkpoint/resume
 *   bioim_destroy  <- garbage collection of the OsimModel instances
 *
 * Conventions
 *   - Real-valued buffers are float (precision 32) or double (precision 64),
 *     fixed at create time.  All buffers passed to reset/step are DEVICE
 *     pointers on the handle's device; the caller owns them.
 *   - obs is [N][obs_dim] row-major, reward [N], done [N] (uint8 0/1),
 *     info [N][info_dim] (the reference's info['all_rewards']).
 *   - Calls are asynchronous on the handle's HIP stream (bioim_stream /
 *     bioim_set_stream); bioim_sync waits.  Not re-entrant per handle.
 *   - Every entry returns 0 on success, < 0 on error; bioim_last_error()
 *     returns the thread-local message.  A missing GPU or a pack whose
 *     topology has no compiled kernel is an error (there is no CPU fallback).
 *
 * Flat per-env state (bioim_get_state/set_state, doubles), matching the
 * oracle's layout: the field order is given at bioim_state_dim below.
 */
#ifndef BIOIM_H
#define BIOIM_H

#include <stddef.h>
#include <stdint.h>

#include "bioim_modelpack.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bioim_handle bioim_handle_t;

enum {
    BIOIM_OK = 0,
    BIOIM_E_ARG = -1,
    BIOIM_E_DEVICE = -2,
    BIOIM_E_PACK = -3,
    BIOIM_E_NOKERNEL = -4,
    BIOIM_E_LAUNCH = -5,
};

/* Create N env instances of the pack's env ID on `device`; precision 32|64.
 * `seed` drives reset indices drawn on the device (randint(0, reset_hi)). */
int bioim_create(const bioim_modelpack_t *pack, int n_envs, int device, int precision, uint64_t seed,
                 bioim_handle_t **out);
int bioim_destroy(bioim_handle_t *h);

/* Reset `n` envs.  env_ids: device int32[n] (NULL = all envs, n ignored).
 * ref_index: device int32[n] reference-row indices (NULL = draw
 * randint(0, reset_hi) per env from the handle's counter-based RNG).
 * obs (may be NULL): device [N][obs_dim] — rows of the reset envs are written. */
int bioim_reset(bioim_handle_t *h, const int32_t *env_ids, const int32_t *ref_index, int n, void *obs);

/* One env step for all N envs.  actions: device [N][nact].  Outputs may be
 * NULL except done.  With auto-reset on, envs that finish are reset in the
 * same launch and their obs row is the post-reset observation. */
int bioim_step(bioim_handle_t *h, const void *actions, void *obs, void *reward, uint8_t *done, void *info);
int bioim_set_auto_reset(bioim_handle_t *h, int on);
/* In-kernel auto-resets (default step kernels: no push table, semi-implicit
 * or RK-Merson, no force report / state storage) read the reset state
 * and observation of the drawn reference row from a per-handle table (torque
 * models: with M^-1 at the row, for the held torques' share of q'')
 * instead of running the reset realize with fiber equilibrium in the step
 * launch (that realize made every launch wait for its slowest wave).  The
 * table is built once, on the first such step, by that same reset realize
 * (one scratch env per reference row); that step blocks while it is built
 * (milliseconds).  on = 1 (default) uses it, 0 runs the
 * realize in the launch as before, with the same results bit for bit (both
 * start the fiber-velocity roots cold; the row also carries the reset
 * realize's cache for the next step's first substep).  Replaces nothing in the
 * reference (OsimModel.reset + equilibrateMuscles per reset,
 * opensim_wrapper.py:293-297). */
int bioim_set_reset_table(bioim_handle_t *h, int on);
/* rows of the handle's built reset table (0: none built yet or none wanted) */
int bioim_reset_table_rows(const bioim_handle_t *h);
/* Row strides (in elements) of the actions / obs / info buffers this handle
 * reads and writes (default nact, obs_dim, info_dim).  Larger strides let
 * handles of different env IDs share padded buffers. */
int bioim_set_io_strides(bioim_handle_t *h, int act_stride, int obs_stride, int info_stride);
/* One env step of a mixed batch (BASELINE config C5): handle i
 * owns rows [sum(n_<i), sum(n_<=i)) of the padded buffers (all handles on one
 * device, same precision and strides; auto-reset per handle).  Segment 0 runs
 * on hs[0]'s stream, the others concurrently on private per-handle streams
 * forked from and joined back into it (events), so the call is ordered on
 * hs[0]'s stream like bioim_step.  Two segments whose topologies form a fused
 * pair (the spatial prosthetic and full muscle models, config C5) and that
 * run the default step (no push table, semi-implicit) go in ONE launch of a
 * fused two-topology kernel on hs[0]'s stream instead (bioim_set_group_fusion).  Later calls on a member handle's own
 * stream must be ordered after hs[0]'s stream (share one stream, as
 * VectorEnv does).  Replaces nothing in the reference
 * (one OsimModel per Ray worker); the batch is the RLlib VectorEnv over
 * heterogeneous sub-envs. */
int bioim_step_group(bioim_handle_t **hs, int nh, const void *actions, void *obs, void *reward, uint8_t *done,
                     void *info);
/* Process-wide switch of the fused two-topology launch in bioim_step_group
 * (default on; off: one concurrent launch per segment).  Results are the
 * same bit for bit either way. */
int bioim_set_group_fusion(int on);
/* 1 if the last bioim_step_group call with h as its first handle ran as ONE
 * fused two-topology launch, 0 if it ran one launch per segment (or no group
 * step yet); -1 for a null handle.  Lets callers and tests see that the
 * fused kernel really ran (it falls back to per-segment launches for fp32,
 * a push table, RK-Merson or a pair without a fused kernel). */
int bioim_group_fused(const bioim_handle_t *h);
/* apply_perturbations (muscle_walking_imitation_env2D.py:83-100 and the same
 * block in every task env): a PrescribedForce on the torso whose ground-frame
 * x force is a PiecewiseConstantFunction of simulation time.  Here: a
 * zero-order-hold table per env — force y[e][k] on [x[k], x[k+1]) (y[e][0]
 * before x[0]) along ground x, applied at the origin of OpenSim body
 * `os_body` (ModelPack osbody index) at every substep and realize.  x: host
 * double[npts], strictly increasing, shared by all envs; y: host double
 * [N][npts].  npts = 0 removes the force.  Synchronous (copies to device). */
int bioim_set_perturbation(bioim_handle_t *h, int os_body, int npts, const double *x, const double *y);
/* Per-env external body forces (OpenSim's PrescribedForce / ExternalForce;
 * no counterpart in the reference envs beyond the torso push above): up to
 * BIOIM_MAX_EXT force slots per handle.  Slot j acts on OpenSim body
 * os_body[j] (ModelPack osbody index) and takes its point of application in
 * that body's frame (BIOIM_EXT_POINT_BODY: the point moves with the body and
 * is evaluated at every dynamics call) or in the ground frame
 * (BIOIM_EXT_POINT_GROUND: fixed in space); both are the same for all envs.
 * wrench: the caller's device buffer [N][k][9] in the handle's precision,
 * per env and slot (fx fy fz, px py pz, tx ty tz) — ExternalForce's column
 * order: force in ground, point, torque in ground.  The buffer is read, never
 * written, by every later step, reset, OsimModel call and every step of a
 * rollout, once per env at the start of the launch; within a step the values
 * are held over all substeps and the realize.  The caller writes new values
 * between steps on the handle's stream, like actions.  The wrench is an input,
 * not state: bioim_copy_state_rows / bioim_load_state / bioim_clone_envs do
 * not carry it, an auto-reset leaves it, and it is not sanitized (a
 * non-finite entry makes that env's state non-finite and the step's finite
 * check sets its done flag; other envs are untouched).  Two slots on one body
 * add in slot order.  While forces are set the step runs kernels of its own
 * (semi-implicit integrator, in-launch auto-reset, no realize cache), a
 * rollout runs as one launch per step and a group step as one launch per
 * segment.  k = 0 removes the forces (the arrays are ignored).
 * Errors (BIOIM_E_ARG), checked in this order before anything else happens:
 * null handle; k outside [0, BIOIM_MAX_EXT]; a null array with k > 0; a body
 * outside [0, nosbody); a frame that is neither constant; a perturbation
 * table set (bioim_set_perturbation: a push is one slot here); RK-Merson or
 * an RK budget set.  With forces set, bioim_set_perturbation (npts > 0),
 * bioim_set_integrator (kind 1) and bioim_set_rk_budget (attempts > 0) are
 * refused the same way.  No device allocation, no synchronization. */
#define BIOIM_MAX_EXT 8
enum { BIOIM_EXT_POINT_BODY = 0, BIOIM_EXT_POINT_GROUND = 1 };
int bioim_set_external_forces(bioim_handle_t *h, int k, const int32_t *os_body /* host [k] */,
                              const int32_t *point_frame /* host [k] */, const void *wrench /* device [N][k][9] */);
/* Inverse-dynamics primitives of the reference's InverseDynamics helper
 * (bioimitation/imitation_envs/inverse_dynamics/inverse_dynamics.cpp:45-205;
 * Boost.Python, built against OpenSim) on the handle's model, batched over n
 * states: muscles disabled, actuator controls 0, the model's gravity,
 * Hunt-Crossley contact and coordinate limit forces.  q, u, v, out: device
 * [n][ndof] in the handle's precision, dof order (locked coordinates are not
 * dofs).  `u` is read by CORIOLIS/RESIDUAL/TOTAL, `v` by MULT_M/MULT_MINV/
 * RESIDUAL.  Conventions (inverse_dynamics.cpp comments): M q'' + c = g + tau;
 * RESIDUAL = M v + c - f_applied (calculateResidualForces, :63-94); TOTAL =
 * c - f_applied, i.e. M q'' + f = tau (calculateTotalForces, :96-125);
 * GRAVITY = g (:127-141); CORIOLIS = c (:143-158); MULT_M = M v (:160-175);
 * MULT_MINV = M^-1 v (:177-192).  Asynchronous on the handle's stream. */
enum {
    BIOIM_ID_GRAVITY = 0,
    BIOIM_ID_CORIOLIS = 1,
    BIOIM_ID_MULT_M = 2,
    BIOIM_ID_MULT_MINV = 3,
    BIOIM_ID_RESIDUAL = 4,
    BIOIM_ID_TOTAL = 5,
};
int bioim_id_eval(bioim_handle_t *h, int op, int n, const void *q, const void *u, const void *v, void *out);
/* Muscle analysis (OpenSim's MuscleAnalysis next to InverseDynamics) on the
 * handle's model, batched over n arbitrary states — not the handle's envs:
 * the env state and the realize cache are neither read nor written.  All
 * pointers are device pointers in the handle's precision, dof order as for
 * bioim_id_eval; any output may be NULL.
 *   length [n][nmuscle]        musculotendon path length L;
 *   speed  [n][nmuscle]        dL/dt = sum_d dL/dq_d u_d (u NULL: u = 0);
 *   dldq   [n][nmuscle][ndof]  dL/dq over every dof: exact zeros outside the
 *     muscle's span and on the floating-base dofs (their sum over a path is
 *     zero).  OpenSim's moment arm is -dL/dq;
 *   fiber  [n][nmuscle][BIOIM_MUSCLE_FIBER_DIM]  fiber length, fiber velocity
 *     (m/s), tendon force, fiber force, active fiber force: the values the
 *     step's muscle evaluation forms at (act, lce, L), the excitation taken
 *     equal to act and the fiber-velocity solve started cold.  lce NULL: each
 *     fiber length is first set to its static equilibrium at (act, L)
 *     (equilibrateMuscles); a given lce is clamped at the muscle's minimum
 *     fiber length as in the step;
 *   tau    [n][ndof]           the muscles' generalized force,
 *     tau_d = -sum_m dL_m/dq_d Ft_m.
 * fiber and tau need act ([n][nmuscle]).  BIOIM_E_ARG, before any device
 * call, for: a null handle, n < 0, null q with n > 0, every output NULL, fiber
 * or tau without act, a model without muscles.  n == 0 returns BIOIM_OK
 * without a launch.  Asynchronous on the handle's stream; synchronizes
 * nothing.  No reference counterpart (the reference reaches these values one
 * OpenSim state at a time, through OsimModel). */
#define BIOIM_MUSCLE_FIBER_DIM 5
int bioim_muscle_eval(bioim_handle_t *h, int n, const void *q, const void *u, const void *act, const void *lce,
                      void *length, void *speed, void *dldq, void *fiber, void *tau);
/* Static optimization (OpenSim's StaticOptimization, the step that joins
 * InverseDynamics and MuscleAnalysis) on the handle's model, batched over n
 * arbitrary states — not the handle's envs: the env state and the realize
 * cache are neither read nor written.  Per state: the activations a that
 * produce the target generalized force tau (normally bioim_id_eval's
 * BIOIM_ID_RESIDUAL at (q, u, q'')) at least effort,
 *     minimize sum_m a_m^2 + sum_d lam_d (tau_d - (B a + c)_d)^2
 *     subject to lo <= a_m <= hi,
 * with OpenSim's assumptions (use_muscle_physiology, rigid tendons), which
 * make the muscle force linear in the activation.  With L, dL/dt, dL/dq as
 * bioim_muscle_eval's length, speed, dldq, per muscle
 *     w = l_opt sin(alpha_opt),  l_t = max(L - l_ts, 0),
 *     l_m = max(sqrt(l_t^2 + w^2), l_min),  cos = sqrt(l_m^2 - w^2) / l_m,
 *     Fa = F0 fal(l_m / l_opt) fv(dL/dt cos / (l_opt v_max)) cos   (the active
 *          capacity: the force at a = 1),
 *     Fp = F0 fpe(l_m / l_opt) cos                               (the passive force),
 * both cut at 0 from below (a muscle without capacity has B = 0 exactly and
 * stays at lo), and dL/dq taken as the exact 0 it is on a dof that moves
 * every point of the path (a rigid motion of the path; a moving point's own
 * coordinate excepted), so a muscle without a moment arm stays at lo too,
 * the curves the step's own; B[d][m] = -dL_m/dq_d Fa_m, and c_d = -sum_m
 * dL_m/dq_d Fp_m when `passive` is nonzero, else 0 (OpenSim's balance carries
 * the active force only).  The exponent is 2 only.  The residual tau - B a - c
 * is OpenSim's reserve actuators: a reserve of optimal torque w_d is
 * lam_d = 1 / w_d^2; lam_d = 0 leaves row d out.  Rows no muscle spans (the
 * floating base) do not influence a.  H = I + B^T lam B >= I: the minimizer
 * is unique.
 *   q, u, tau  [n][ndof]   device, dof order as for bioim_id_eval (u NULL: 0);
 *   row_weight [ndof]      device, lam_d >= 0 (the caller's contract); NULL: all 1;
 *   act        [n][nmuscle]     the activations (required);
 *   tau_muscle [n][ndof]        B a + c;
 *   residual   [n][ndof]        tau - tau_muscle, on every dof;
 *   capacity   [n][nmuscle][2]  Fa, Fp;
 *   status     [n] int32        the solver's passes (>= 0), -1: the iteration
 *     cap was hit, -2: a factorization failed (a pivot <= 0, which H >= I
 *     excludes, or a NaN that came in); act then holds the last feasible
 *     iterate, not the minimizer.
 * Outputs other than act may be NULL.  The solve is exact and finite: a
 * primal active-set (BVLS) iteration from a = lo with a Cholesky
 * factorization per pass, ties to the lowest muscle index; no stop tolerance
 * (cond(H) reaches 3e5 at unit reserves).  The cap is 8 nmuscle passes (112 /
 * 176 / 152 for 14 / 22 / 19 muscles); the most observed is 21 / 29 / 18 (over
 * 4096 / 4096 / 64 states at unit reserves).  A state's result does not depend on n or on the other
 * states, and a repeated call repeats it bit for bit.
 * fp64 handles only: the normal equations behind H leave single precision
 * no digits at cond(H) ~ 1e5-1e6.  BIOIM_E_ARG, before any device call and in
 * this order, for: a null handle, n < 0, null q with n > 0, null tau, null
 * act, bounds that are not finite with lo < hi, a model without muscles, an
 * fp32 handle.  n == 0 returns BIOIM_OK without a launch.  Asynchronous on
 * the handle's stream; synchronizes nothing.  No reference counterpart (the
 * reference ships StaticOptimization results, not the solver). */
int bioim_static_opt(bioim_handle_t *h, int n, const void *q, const void *u, const void *tau,
                     const void *row_weight /* device [ndof], NULL = all 1 */, double lo, double hi, int passive,
                     void *act /* [n][nmuscle], required */, void *residual /* [n][ndof] */,
                     void *tau_muscle /* [n][ndof] */, void *capacity /* [n][nmuscle][2]: Fa, Fp */,
                     int32_t *status /* [n]: iterations used, or -1 cap hit, -2 factorization failed */);
/* Computed muscle control (OpenSim's CMC, the step after StaticOptimization)
 * on the handle's model, batched over n arbitrary states — not the handle's
 * envs: the env state and the realize cache are neither read nor written.
 * Per state and window [t, t + T]: the excitations e whose muscles, run
 * through the step's own activation and contraction dynamics (compliant
 * tendons, the fiber-length state, first-order activation), deliver at t + T
 * the tendon forces that produce the target generalized force tau (normally
 * bioim_id_eval's BIOIM_ID_RESIDUAL at the wanted q'').  fp64 handles only.
 * Inputs, device pointers, dof order as for bioim_id_eval:
 *   q, u       [n][ndof]     the state at the window's start t;
 *   act, lce   [n][nmuscle]  the muscle states at t;
 *   q1         [n][ndof]     the coordinates at t + T; NULL: q + T u (product,
 *                            then sum, two roundings: the same bits as the
 *                            caller's own q + T u passed as q1);
 *   tau        [n][ndof]     the generalized force the muscles are to deliver;
 *   row_weight [ndof]        lam_d >= 0 as in bioim_static_opt (lam_d = 1 /
 *                            reserve^2, 0 leaves row d out); NULL: all 1;
 *   T                        the window length, > 0;
 *   nsub                     predictor substeps, >= 1 (the step's own count is
 *                            20 at T = 0.01; the predictor with 5 differs from
 *                            it by up to 0.28 F0);
 *   emin, emax               per muscle the bracket is [max(emin, amin_m),
 *                            min(emax, 1)]; a bracket these leave empty
 *                            collapses onto its lower end;
 *   ftol                     root-solve force tolerance in units of F0;
 *   max_iter                 cap on predictor evaluations per root solve, >= 1.
 * Four phases per state.
 *   1. Paths.  L0 is the path length at q; L1 and dL/dq are taken at q1, the
 *      structural zeros of dL/dq exact as in bioim_static_opt.  Inside the
 *      window the path length is L(s) = L0 + (s / T)(L1 - L0).
 *   2. Predictor P_m(e).  From (act_m, lce_m), nsub times the step's muscle
 *      substep at h = T / nsub with constant excitation e: substep k = 0 ..
 *      nsub - 1 evaluates the muscle at path length L0 + (k / nsub)(L1 - L0)
 *      with a cold fiber-velocity start, then a += h da/dt and, unless the
 *      fiber is clamped, lce += h vce / (1 - h dvce/dlce) cut at l_min (the
 *      semi-implicit update of the step).  P_m(e) is the tendon force of one
 *      more evaluation at the end state and L1.  The force range is P_m at the
 *      two bracket ends; each end keeps its own force, and Fmin_m / Fmax_m are
 *      the smaller / the larger of the two.
 *   3. Force allocation over x_m = F_m / F0_m (OpenSim's CMC target, the sum
 *      of squared muscle stresses):
 *          minimize sum_m x_m^2 + sum_d lam_d (tau_d - sum_m (-dL_m/dq_d) F0_m x_m)^2
 *          subject to Fmin_m / F0_m <= x_m <= Fmax_m / F0_m.
 *      No passive term: F is the whole tendon force.  A muscle with Fmax <=
 *      Fmin stays bound at Fmin and is never offered to the solver.  The solve
 *      is bioim_static_opt's active-set iteration (one piece of code: the same
 *      passes, ties, cap of 8 nmuscle and status codes), started at the lower
 *      bounds.  F*_m is Fmin_m (Fmax_m) itself where x_m ends on its lower
 *      (upper) bound, else x_m F0_m.
 *   4. Root solve per muscle.  F* on a bound: that bound's bracket end (for an
 *      empty range the lower end), zero evaluations, root_status 0.  Otherwise
 *      Illinois regula falsi on g(e) = P_m(e) - F*_m:
 *        a. a, b = the lower, upper bracket end, ga, gb = their forces of
 *           phase 2 minus F* (opposite signs: F* lies strictly between), no
 *           side retained;
 *        b. with max_iter evaluations done: return the evaluated iterate with
 *           the smallest |g| (the earliest of equals), root_status -1;
 *        c. c = b - gb (b - a) / (gb - ga), replaced by (a + b) / 2 unless a < c
 *           < b; gc = P_m(c) - F*, one evaluation;
 *        d. |gc| <= ftol F0_m: return c, root_status = the evaluations used;
 *        e. gc and gb of one sign (both < 0 or neither): b, gb = c, gc, and if
 *           b's side was also the one replaced last, ga = ga / 2; otherwise a,
 *           ga = c, gc, and if a's side was also the one replaced last, gb =
 *           gb / 2; back to b.
 * Outputs (excitation required, the others may be NULL):
 *   excitation  [n][nmuscle]     the returned excitation e*;
 *   force       [n][nmuscle]     the allocated force F*;
 *   force_range [n][nmuscle][2]  P_m at the lower and at the upper bracket
 *                                end, in that order (phase 3's bounds are
 *                                their min and max);
 *   predicted   [n][nmuscle]     P_m(e*);
 *   state_end   [n][nmuscle][2]  the predicted activation and fiber length at
 *                                t + T under e* (bioim_muscle_eval at q1 with
 *                                them returns predicted as its tendon force);
 *   tau_muscle  [n][ndof]        sum_m (-dL_m/dq_d) F0_m x_m;
 *   residual    [n][ndof]        tau - tau_muscle, on every dof;
 *   status      [n] int32        phase 3: the solver's passes (>= 0), -1: its
 *                                cap was hit, -2: a factorization failed or a
 *                                NaN came in;
 *   root_status [n][nmuscle] int32  phase 4: evaluations used; 0 for a muscle
 *                                on a bound or with an empty range; -1: the cap.
 * Every loop is bounded: nsub + 1 muscle evaluations per predictor, 2 +
 * max_iter predictors per muscle, 8 nmuscle solver passes, and the
 * fiber-velocity iteration's own cap.  A state's result does not depend on n
 * or on the other states, and a repeated call repeats it bit for bit.
 * Out of scope: residual actuators on the pelvis (bioim_set_external_forces
 * is the place to apply them), inverting the envs' action smoothing, the
 * torque models, fp32 (the allocation has bioim_static_opt's conditioning)
 * and RRA.  BIOIM_E_ARG, before any device call and in this order, for: a
 * null handle, n < 0, with n > 0 a null q, u, act, lce, tau or excitation (in
 * that order), T, ftol, emin or emax not finite or T <= 0 or emin >= emax,
 * nsub < 1 or max_iter < 1, a model without muscles, an fp32 handle.  n == 0
 * returns BIOIM_OK without a launch.  Asynchronous on the handle's stream;
 * synchronizes nothing.  No reference counterpart (the reference drives its
 * muscles from a policy; it ships no controller). */
int bioim_cmc(bioim_handle_t *h, int n, const void *q, const void *u, const void *act, const void *lce,
              const void *q1 /* [n][ndof], NULL = q + T u */, const void *tau,
              const void *row_weight /* device [ndof], NULL = all 1 */, double T, int nsub, double emin, double emax,
              double ftol, int max_iter, void *excitation /* [n][nmuscle], required */, void *force /* [n][nmuscle] */,
              void *force_range /* [n][nmuscle][2] */, void *predicted /* [n][nmuscle] */,
              void *state_end /* [n][nmuscle][2]: activation, fiber length */, void *tau_muscle /* [n][ndof] */,
              void *residual /* [n][ndof] */, int32_t *status /* [n] */, int32_t *root_status /* [n][nmuscle] */);
/* Marker inverse kinematics (OpenSim's InverseKinematicsTool, the first link
 * of the chain IK -> InverseDynamics -> StaticOptimization) on the handle's
 * model, batched over n frames — not the handle's envs: the env state and the
 * realize cache are neither read nor written.  Per frame f, over the handle's
 * dofs (locked coordinates are not dofs and keep their pack values, as in
 * bioim_id_eval), it minimizes OpenSim's IK objective (IKMarkerTasks plus
 * optional IKCoordinateTasks)
 *     sum_i w_i |x_i(q) - x_exp[f][i]|^2 + sum_d c_d (q_d - q_target[f][d])^2,
 * x_i(q) = o_b + R_b loc_i: marker i on its composite body b.
 *   nm                     markers, 1 .. BIOIM_IK_MAX_MARKERS;
 *   marker_body [nm] int32 composite-body index (a value outside the model is
 *                          the caller's contract; the Python layer checks it);
 *   marker_loc  [nm][3]    location in the composite body's frame;
 *   weight      [nm]       w_i >= 0 (0 leaves the marker out); these three
 *                          tables are shared by all frames of the call;
 *   x_exp  [n][nm][3]      measured positions, ground frame, metres; a marker
 *                          with a NaN component in a frame is left out of that
 *                          frame (a gap in a .trc file; OpenSim skips it too);
 *   q0     [n][ndof]       the start (required), dof order as for bioim_id_eval;
 *   coord_weight [ndof], q_target [n][ndof]   c_d >= 0 and the coordinate
 *                          tasks' values: both or neither (NULL: no tasks);
 *   tol                    stop once an accepted step has max_d |dq_d| <= tol;
 *   max_iter               >= 0; 0 evaluates only: the forward marker
 *                          kinematics (markers, err, jacobian) at q0.
 * Outputs (q required, the others may be NULL), all at the returned q:
 *   q        [n][ndof];
 *   markers  [n][nm][3]        the model's marker positions;
 *   err      [n][2]            sqrt(sum w_i |r_i|^2 / sum w_i) and max |r_i|
 *                              over the markers used (finite x_exp, w_i > 0):
 *                              the weighted marker RMS and the largest marker
 *                              distance, the figures of OpenSim's IK log; 0, 0
 *                              when no marker is used;
 *   jacobian [n][nm][3][ndof]  dx_i/dq_d (the station Jacobian), from the
 *                              dofs' ground-frame Plucker columns: Omega_d x
 *                              x_i + V_d; exact zeros where dof d is not on
 *                              marker i's root chain;
 *   status   [n] int32         >= 0: the iterations used; -1: max_iter was hit,
 *                              q holds the last accepted iterate; -2: a pivot
 *                              <= 0 or a NaN that came in (q0, a target), q
 *                              holds the last accepted iterate (q0 if none).
 *                              A frame with no marker used and no coordinate
 *                              task has A = 0: it returns -2 and q = q0.
 * The algorithm is fixed: damped Gauss-Newton on the normal equations
 * A = J^T W J + C, g = J^T W r + C (q - q_target), f the objective.
 *   1. mu = 1e-3 max_d A_dd at q0.
 *   2. Every iteration solves (A + mu I) dq = -g by Cholesky (a pivot <= 0 ends
 *      the frame with -2) and evaluates f at q + dq.
 *   3. The step is accepted if f_new <= f (1 + 64 eps) or max |dq| <= tol.  An
 *      accepted step with max |dq| <= tol returns; otherwise A and g are
 *      re-formed at the new q and mu <- mu / 4.
 *   4. A step that is not accepted leaves q, A and g, sets mu <- 8 mu and
 *      solves again.
 * Every solve counts as an iteration; before each, max_iter solves already
 * done end the frame with -1.  (The "or small step" clause ends a frame at
 * the rounding floor of f, where a decrease test alone rejects forever.)
 * A frame's result does not depend on n or on the other frames, and a
 * repeated call repeats it bit for bit.  BIOIM_IK_MAX_MARKERS is 64: the
 * kernel keeps no per-marker storage (each lane sums its markers in
 * registers), so the bound is not an LDS limit of any topology.
 * Out of scope: coordinate range clamping (neither IK model the reference
 * ships has a clamped coordinate; a solution may leave a coordinate's range).
 * fp64 handles only: the iteration converges linearly on a trial with a
 * large residual, and a step-size stop at 1e-9 rad has no meaning in single
 * precision.  BIOIM_E_ARG, before any device call and in this order, for: a
 * null handle, n < 0, nm < 1 or nm > BIOIM_IK_MAX_MARKERS, a null marker
 * table (marker_body, marker_loc, weight) with n > 0, null x_exp with n > 0,
 * null q0 with n > 0, null q with n > 0, exactly one of coord_weight /
 * q_target, tol not finite or < 0, max_iter < 0, an fp32 handle.  n == 0
 * returns BIOIM_OK without a launch.  Asynchronous on the handle's stream;
 * synchronizes nothing.  No reference counterpart (the reference ships IK
 * results, not the solver). */
#define BIOIM_IK_MAX_MARKERS 64
int bioim_ik_solve(bioim_handle_t *h, int n, int nm, const int32_t *marker_body /* [nm] */,
                   const void *marker_loc /* [nm][3] */, const void *weight /* [nm] */,
                   const void *x_exp /* [n][nm][3] */, const void *q0 /* [n][ndof], required */,
                   const void *coord_weight /* [ndof] or NULL */, const void *q_target /* [n][ndof] or NULL */,
                   double tol, int max_iter, void *q /* [n][ndof], required */, void *markers /* [n][nm][3] */,
                   void *err /* [n][2] */, void *jacobian /* [n][nm][3][ndof] */,
                   int32_t *status /* [n]: iterations used, or -1 cap hit, -2 factorization failed / NaN */);
/* Joint reaction analysis (OpenSim's JointReaction, the fifth link of the
 * chain after IK, InverseDynamics, MuscleAnalysis and StaticOptimization) on
 * the handle's model, batched over n arbitrary states — not the handle's
 * envs: the env state and the realize cache are neither read nor written.
 * Per state, the resultant force and moment each composite body's inboard
 * joint carries.  All pointers are device pointers in the handle's precision,
 * dof order as for bioim_id_eval.  The arithmetic is fp64 on either handle: an
 * fp32 handle keeps an fp64 image of the model for this call and converts at
 * its loads and stores (a foot's contact force turns the 1e-7 m of an fp32
 * kinematic chain into 0.1 N), so its results are the fp64 ones of its
 * fp32 inputs, rounded.  That image is built and uploaded on an fp32 handle's
 * first call, which blocks for the copy; no later call does.
 *
 * All definitions are per state, in the ground frame.  The sums run over
 * composite bodies k (the pack's cbody, 5 or 7 per model).
 * The wrench that body k's own balance leaves for its joints is
 *     W_k = I_k a_k + v_k x* I_k v_k - (gravity on k)
 *           - (Hunt-Crossley contact on k, if flag CONTACT)
 *           - ext_k - (muscle point forces on k)
 * Here a_k = AL_k + sum over the dofs d on k's root path of S_d q''_d.  AL
 * holds the velocity-product accelerations the prologue already publishes,
 * and S_d are the ground-frame Plucker columns.
 * Reaction.  F_b = sum over k in subtree(b) of W_k is the wrench the parent
 * (ground for the root) exerts on body b through b's inboard joint.  Its
 * moment is taken about c_b = o_b - R_b R_mb^T p_mb, the origin of the
 * joint's child-side frame M, which is o_b in every shipped pack.
 * Muscle point forces.  For muscle m with tendon force Ft_m, take every
 * active path point j with exactly muscle_path's activity rule:
 *   - conditional points are out of range when q < lo || q > hi;
 *   - moving points sit at their function values.
 * The force on point j's body at P_j is Ft_m (e_{j->j+1} - e_{j-1->j}), where
 * e is the unit segment directions and the end points have one term each.
 * This is -Ft g in muscle_path's notation.
 * A moving point's own-coordinate term (g . dP/dq, muscle_path's gd) is a
 * mobility force, not a body force.  It is not part of F.
 * Coordinate limit forces, coordinate actuators and reserves are mobility
 * forces too.  They never enter this kernel.  They appear in tau_joint as
 * what the coordinate itself must carry.
 * Generalized force.  tau_joint_d = S_d . F_{cb(d)}, taken with Omega_d on
 * the moment and V_d on the force, both about the same point.
 *
 *   q, u, qdd [n][ndof]          u, qdd NULL: zeros;
 *   ft   [n][nmuscle]            tendon forces (bioim_muscle_eval's fiber
 *                                column 2, or the REALIZE report's); NULL: no
 *                                muscle forces, bit for bit as all zeros;
 *   ext  [n][ncbody][6]          fx fy fz mx my mz applied to each body, ground
 *                                frame, moment about the ground origin;
 *   flags                        BIOIM_JR_CONTACT adds the model's Hunt-Crossley
 *                                contact at (q, u) (the explicit force,
 *                                bioim_id_eval's);
 *   frame                        rotates `reaction` only: CHILD is body b's
 *                                composite frame, PARENT the parent's composite
 *                                frame (ground for the root).
 * Outputs (any may be NULL, not all):
 *   reaction      [n][ncbody][6]  fx fy fz mx my mz of F_b about c_b;
 *   point         [n][ncbody][3]  c_b in the ground frame;
 *   tau_joint     [n][ndof];
 *   muscle_wrench [n][ncbody][6]  the muscles' net wrench on body k alone (not
 *                                the subtree), ground frame, about the ground
 *                                origin; zeros on a model without muscles.
 * Planar models keep all six components: their hips sit off the plane, so mx,
 * my (and a lateral force, where one acts) are loads the joints carry.
 * Joints inside a composite body (welded or locked ones) have no row.
 * A state's result does not depend on n or on the other states, and a
 * repeated call repeats it bit for bit (the muscle forces are summed per body
 * in a fixed order).  BIOIM_E_ARG, before any device call and in this order,
 * for: a null handle, n < 0, null q with n > 0, ft on a model without
 * muscles, unknown flag bits, frame outside 0..2, every output NULL.  n == 0
 * returns BIOIM_OK without a launch.  Asynchronous on the handle's stream;
 * synchronizes nothing.  No reference counterpart (the reference ships
 * JointReaction results of its OpenSim runs, not the analysis). */
enum { BIOIM_JR_GROUND = 0, BIOIM_JR_CHILD = 1, BIOIM_JR_PARENT = 2 };   /* frame the outputs are expressed in */
#define BIOIM_JR_CONTACT 1                                               /* flags: add the model's contact at (q, u) */
int bioim_joint_reaction(bioim_handle_t *h, int n, const void *q, const void *u /* NULL: 0 */,
        const void *qdd /* NULL: 0 */, const void *ft /* [n][nmuscle] tendon forces, NULL: none */,
        const void *ext /* [n][ncbody][6] fx fy fz mx my mz on each body, ground frame, moment about the ground origin; NULL: none */,
        int flags, int frame,
        void *reaction /* [n][ncbody][6]: fx fy fz mx my mz of F_b about c_b */,
        void *point /* [n][ncbody][3]: c_b in the ground frame */,
        void *tau_joint /* [n][ndof] */,
        void *muscle_wrench /* [n][ncbody][6]: the muscles' net wrench on body k alone (not the subtree), ground frame, about the ground origin */);
/* Induced accelerations (OpenSim's InducedAccelerations analysis) at n
 * arbitrary states, not the handle's envs: the env state and the realize cache
 * are neither read nor written.  Per state: how much of each coordinate's
 * acceleration, of the mass centre's acceleration and of each foot's ground
 * reaction is due to gravity, to the velocity terms, and to each single force.
 * fp64 handles only: every column goes through M^-1, and POINT mode through a
 * Schur complement J M^-1 J^T on a floating base, whose conditioning leaves an
 * fp32 result no digits worth reporting.  All pointers are device pointers
 * (doubles unless noted), dof order as for bioim_id_eval.
 *
 * Contributors.  NC = 6 + ncforce + nmuscle columns, in this fixed order, each
 * with its generalized force Q_c:
 *   0            gravity     g(q) (BIOIM_ID_GRAVITY);
 *   1            velocity    -c(q, u) (BIOIM_ID_CORIOLIS, negated);
 *   2 ..         one per Hunt-Crossley force f (the feet): J^T of the force's
 *                explicit sphere forces at (q, u), which is what bioim_id_eval
 *                applies.  In POINT mode it is exactly 0 for a constrained foot;
 *   then         limits      the coordinate limit forces;
 *   then         actuators   tau_act [n][ndof], given by the caller (coordinate
 *                actuators, PD torques, reserves).  NULL: zeros;
 *   then         external    projection of ext [n][ncbody][6], with
 *                bioim_joint_reaction's convention (fx fy fz mx my mz, ground
 *                frame, moment about the ground origin).  NULL: zeros;
 *   then         one per muscle m: -Ft_m dL_m/dq, the full generalized force
 *                including a moving point's own-coordinate term.  The muscle
 *                columns sum to bioim_muscle_eval's tau.  ft [n][nmuscle] NULL:
 *                zeros, bit for bit;
 *   last         total       the sum of all Q_c.
 * Modes (kind).
 *   BIOIM_IA_FORCE = 0: contact is the applied Hunt-Crossley force.
 *     A_c = M^-1 Q_c.  The total column is then the model's forward-dynamics
 *     acceleration.
 *   BIOIM_IA_POINT = 1: OpenSim's way.  Each foot in contact is held by a point
 *     constraint, and each contributor's share of the ground reaction is solved
 *     for:
 *         M A_c - sum_f J_f^T lambda_{c,f} = Q_c,
 *         J_f A_c + [c is velocity or total] beta_f = 0  for every constrained f.
 *     J_f is the station Jacobian (Omega_d x P_f + V_d) of the body-fixed point
 *     coincident with P_f.  The body is the composite body that carries force
 *     f's spheres.  beta_f is that point's acceleration along q(t) = q + u t,
 *     that is, at q'' = 0.  Rows per constrained foot: 3 on spatial topologies,
 *     2 (x, y) on planar ones.  The planar z row is identically zero, and the
 *     planar reaction z is exactly 0.  The total column here is the
 *     constrained model's acceleration, not forward dynamics.
 * Which feet are constrained, and where.  The caller gives both
 * cactive [n][ncforce] (uint8) and cpoint [n][ncforce][3] (ground frame), or
 * neither.  With neither, the model decides: foot f is constrained when the
 * summed normal force of its active spheres exceeds force_threshold (finite,
 * >= 0), and P_f is then sum_s fn_s P_s / sum_s fn_s over that foot's active
 * spheres, with the contact point P_s and normal force fn_s of the model's
 * Hunt-Crossley contact.  cactive and cpoint are ignored in FORCE mode.
 * Outputs (any may be NULL, not all):
 *   accel       [n][NC][ndof]        A_c;
 *   com_accel   [n][NC][3]           J_com A_c, plus d^2/dt^2 com(q + u t) on
 *                                    the velocity and total columns;
 *   reaction    [n][NC][ncforce][3]  lambda_{c,f}.  Zeros in FORCE mode and for
 *                                    unconstrained feet;
 *   cpoint_out  [n][ncforce][3], cactive_out [n][ncforce] (uint8): what was
 *                                    used (zeros for a foot not constrained);
 *   status      [n] int32            0 ok; -2 for a pivot <= 0 or a NaN that
 *                                    came in (from M or from the Schur
 *                                    complement S = J M^-1 J^T, or through u,
 *                                    ft, tau_act, ext).  The outputs are then
 *                                    zeros.
 * u NULL: zeros.  A state's result does not depend on n or on the other
 * states, and a repeated call repeats it bit for bit (every sum has a fixed
 * order).  BIOIM_E_ARG, before any device call and in this order, for: a null
 * handle, n < 0, null q with n > 0, ft on a model without muscles, kind
 * outside 0..1, exactly one of cactive / cpoint, force_threshold not finite or
 * < 0, every output NULL, an fp32 handle.  n == 0 returns BIOIM_OK without a
 * launch.  Asynchronous on the handle's stream; synchronizes nothing.  No
 * reference counterpart (the reference ships no induced-acceleration
 * analysis). */
enum { BIOIM_IA_FORCE = 0, BIOIM_IA_POINT = 1 };   /* kind */
int bioim_induced_accel(bioim_handle_t *h, int n, const void *q, const void *u /* NULL: 0 */,
        const void *ft /* [n][nmuscle] tendon forces, NULL: none */,
        const void *tau_act /* [n][ndof], NULL: none */,
        const void *ext /* [n][ncbody][6] fx fy fz mx my mz on each body, ground frame, moment about the ground origin; NULL: none */,
        int kind, const uint8_t *cactive /* [n][ncforce] */, const void *cpoint /* [n][ncforce][3], ground frame */,
        double force_threshold,
        void *accel /* [n][NC][ndof] */, void *com_accel /* [n][NC][3] */, void *reaction /* [n][NC][ncforce][3] */,
        void *cpoint_out /* [n][ncforce][3] */, uint8_t *cactive_out /* [n][ncforce] */, int32_t *status /* [n] */);
/* Body kinematics (OpenSim's BodyKinematics and PointKinematics analyses, the
 * kinematics-analysis stage between IK and MuscleAnalysis) at n arbitrary
 * states, not the handle's envs: the env state and the realize cache are
 * neither read nor written.  Both precisions, every topology (no muscle is
 * involved).  q, u, qdd [n][ndof] are device pointers in the handle's
 * precision, dof order as for bioim_id_eval; u, qdd NULL: zeros, bit for bit.
 * A body's spatial acceleration is a_k = AL_k + sum over the dofs d on k's
 * root path of S_d q''_d (bioim_joint_reaction's definition).
 *
 * Points.  npt points, 0 .. BIOIM_BK_MAX_POINTS, shared by all states:
 *   pt_body  [npt] int32   HOST array: OpenSim body index (the pack's osbody
 *                          order), -1 = ground;
 *   pt_local [npt][3]      HOST array of doubles (either precision): the
 *                          point in that OpenSim body's frame.
 * Both are read and checked before the call returns and travel to the kernel
 * inside its argument list, so the caller may reuse them at once and a bad
 * body index is refused before any launch.  BIOIM_BK_MAX_POINTS is 64: with the
 * OpenSim bodies' mass centres the tables take 2.2 KiB of the 4 KiB a kernel's
 * arguments may have; the kernel itself keeps no per-point storage.
 *
 * Outputs (device pointers in the handle's precision; any may be NULL, not
 * all).  Bodies in the pack's OpenSim-body order; [3][3] rows are position,
 * velocity, acceleration (x y z each), in the ground frame:
 *   origin   [n][nosbody][3][3]  each OpenSim body frame's origin;
 *   com      [n][nosbody][3][3]  each OpenSim body's own mass centre
 *                                (osbody.com; what BodyKinematics reports);
 *   orient   [n][nosbody][3][3]  body-fixed XYZ angles of R = Rx Ry Rz, angular
 *                                velocity, angular acceleration;
 *   rot      [n][nosbody][9]     R (body -> ground), row-major;
 *   system   [n][3][3]           the whole-body mass centre;
 *   momentum [n][2][3]           linear momentum sum m_k v_k, and angular
 *                                momentum about the whole-body mass centre,
 *                                sum R_k I_k R_k^T w_k + m_k (c_k - C) x (v_k - V);
 *   energy   [n][2]              kinetic energy sum (m_k v_k^2 + w_k . I_k w_k)/2
 *                                and gravitational potential energy -m g . C;
 *   point    [n][npt][3][3]      each listed point; a ground point is fixed
 *                                (its position is pt_local, the rest zeros).
 * The sums run over the composite bodies k in index order (c_k, v_k their mass
 * centres, m the sum of their masses).
 * flags: BIOIM_BK_LOCAL is OpenSim's express_results_in_body_local_frame: the
 * linear velocity and acceleration in origin and com and the angular velocity
 * and acceleration in orient are expressed in the OpenSim body's own frame;
 * positions, angles and every other output stay in the ground frame.
 * No status output: a NaN in q, u or qdd simply comes out.  A state's result
 * does not depend on n or on the other states, and a repeated call repeats it
 * bit for bit; origins, mass centres and points go through one piece of code,
 * so a point at a body's origin (or at osbody.com) equals that body's origin
 * (com) row bit for bit.  BIOIM_E_ARG, before any device call and in this
 * order, for: a null handle, n < 0, npt < 0 or npt > BIOIM_BK_MAX_POINTS, a
 * null point table with npt > 0, a body index outside [-1, nosbody), unknown
 * flag bits, null q with n > 0, every output NULL.  n == 0 returns BIOIM_OK
 * without a launch.  Asynchronous on the handle's stream; synchronizes
 * nothing. */
#define BIOIM_BK_MAX_POINTS 64
#define BIOIM_BK_LOCAL 1   /* flags: velocities and accelerations in the body's own frame */
int bioim_body_kin(bioim_handle_t *h, int n, const void *q, const void *u /* NULL: 0 */, const void *qdd /* NULL: 0 */,
        int npt, const int32_t *pt_body /* host [npt]: OpenSim body index, -1 = ground */,
        const void *pt_local /* host double [npt][3], in that body's frame */, int flags /* BIOIM_BK_LOCAL */,
        void *origin /* [n][nosbody][3][3] */, void *com /* [n][nosbody][3][3] */, void *orient /* [n][nosbody][3][3] */,
        void *rot /* [n][nosbody][9] */, void *system /* [n][3][3] */, void *momentum /* [n][2][3] */,
        void *energy /* [n][2] */, void *point /* [n][npt][3][3] */);
/* OsimModel calls on single envs (the reference's physics facade,
 * opensim_wrapper.py:92-332), for callers that drive the model directly
 * (tests/example_position_control.py:203-223; the env methods
 * get_state_dict / get_limit_forces / calc_cost_of_transport).  For the n
 * listed envs (env_ids: device int32[n]):
 *   controls (device [n][nact], may be NULL): OsimModel.actuate first —
 *     NaN -> 0, clip to [min_control, max_control], held from then on;
 *   op BIOIM_OSIM_REALIZE: nothing else (the calc_* realizations);
 *   op BIOIM_OSIM_EQUILIBRATE: reset_manager (:287-291) — a new integrator
 *     and equilibrateMuscles: each muscle's static fiber equilibrium at the
 *     held activation; the caller writes time / coordinates / speeds with
 *     bioim_set_state first (set_time :303-307, set_coordinates :309-319,
 *     set_velocities :321-332, reset :293-297);
 *   op BIOIM_OSIM_INTEGRATE: integrate (:299-301) — istep += 1, then the
 *     handle's integrator to step_size * istep with the held controls;
 * then the state is realized: obs (device [N][obs_stride], may be NULL)
 * gets the env's observation row, report (device [N][bioim_osim_report_dim],
 * may be NULL) the realized quantities (rows indexed by env):
 *   [time, istep, q[nc], u[nc], qdd[nc] (CoordinateSet order),
 *    per OpenSim body: origin pos[3], vel[3], acc[3], body-fixed XYZ angles[3],
 *      angular vel[3], angular acc[3] (ground frame); then the system COM
 *      pos[3], vel[3], acc[3],
 *    per muscle: activation, fiber_length, fiber_velocity, fiber_force,
 *      active_fiber_force, excitation, tendon_force,
 *    per actuator: actuation,
 *    per Hunt-Crossley force: force[3], moment about the ground origin[3] on the feet,
 *    per CoordinateLimitForce: its generalized force,
 *    calc_cost_of_transport() (0 for torque models)].
 * Env-level state (action deque, last action, old pelvis x, done) is left
 * alone.  A REALIZE, with or without controls, reads the state and leaves
 * the next bioim_step's results bit for bit what they are without it (the
 * realize cache stays valid); EQUILIBRATE and INTEGRATE move the state and
 * mark the handle's realize-cache rows stale.
 * Refused while envs are suspended mid-step (bioim_set_rk_budget).
 * Asynchronous on the handle's stream. */
enum {
    BIOIM_OSIM_REALIZE = 0,
    BIOIM_OSIM_EQUILIBRATE = 1,
    BIOIM_OSIM_INTEGRATE = 2,
};
int bioim_osim_report_dim(const bioim_handle_t *h);
int bioim_osim(bioim_handle_t *h, int op, const int32_t *env_ids, int n, const void *controls, void *obs, void *report);
/* The REALIZE report of the n listed envs (env_ids: device int32[n], distinct,
 * in [0, N): the caller's contract) into report (device
 * [N][bioim_osim_report_dim], rows indexed by env), as bioim_osim with op
 * BIOIM_OSIM_REALIZE, no controls and no obs: the state is read, the next
 * bioim_step's results stay bit for bit what they are without the call.
 * Unlike bioim_osim it does not read the suspended-step flags back first, so
 * it is asynchronous on the handle's stream and synchronizes nothing: the
 * form for a per-step reward or constraint (VectorEnv.joint_reaction).  In
 * exchange it is refused on a handle that was ever given an RK budget
 * (bioim_set_rk_budget with attempts > 0), the only handles whose envs can be
 * suspended mid-step; those use bioim_osim.  BIOIM_E_ARG, before any device
 * call and in this order, for: a null handle, n < 0, null env_ids with n > 0,
 * a null report, a handle that has had an RK budget.  n == 0 returns BIOIM_OK
 * without a launch. */
int bioim_realize_report(bioim_handle_t *h, const int32_t *env_ids, int n, void *report);
/* Global index of this handle's env 0 (multi-GPU sharding): device-drawn
 * reset indices depend on the global env index, so a sharded run is
 * bit-identical to an unsharded one. */
int bioim_set_env_offset(bioim_handle_t *h, int offset);

/* Host-side state transfer (synchronous).
 *
 * The flat state row, state_dim doubles per env, holds these fields in this
 * order (the oracle's layout):
 *
 *   field     values          meaning
 *   t         1               time
 *   istep     1               step index (an int32 in the record)
 *   has_last  1               a last action exists (int32)
 *   old_px    1               pelvis x at the last step
 *   done      1               (int32)
 *   q         ndof            coordinates
 *   u         ndof            speeds
 *   act       nmuscle         activations
 *   lce       nmuscle         fiber lengths
 *   hist      horizon * nact  action history, index hh * nact + a
 *   last      nact            last action
 *   hrk       1               RK-Merson step size carried to the next step
 *   ctl       nact            held actuator controls (the PrescribedController's
 *                             Constant functions, set by each step's actuate
 *                             and kept through resets)
 *
 * state_dim = 5 + 2 ndof + 2 nmuscle + horizon nact + nact + 1 + nact.
 * Values are stored in the handle's precision, t and hrk always as doubles;
 * bioim_set_state / bioim_load_state truncate the int32 fields. */
int bioim_state_dim(const bioim_handle_t *h);
int bioim_get_state(bioim_handle_t *h, double *host_state /* [N][state_dim] */);
int bioim_set_state(bioim_handle_t *h, const double *host_state);
/* The same rows as bioim_get_state, written as doubles into a device buffer
 * [N][state_dim] on the handle's stream, without synchronizing (the
 * single-env recorder copies them with the step's outputs in one transfer).
 * Rows of envs suspended mid-step by the RK budget are not at a step
 * boundary (bioim_get_state refuses them; this call does not check).  No
 * reference counterpart. */
int bioim_copy_state(bioim_handle_t *h, void *device_out);
/* Indexed state save / restore and env cloning on the device.  All three
 * are asynchronous on the handle's stream and synchronize nothing; every
 * pointer is a device pointer on the handle's device.  Argument errors (a
 * null handle, a null buffer or id list, n <= 0 or n > N with an id list)
 * return BIOIM_E_ARG with a message before any device call.  An id outside
 * [0, N) is skipped by the kernels, never used.  No reference counterpart
 * (the reference state is not checkpointable, and one OsimModel is one env).
 *
 * bioim_copy_state_rows: bioim_copy_state for the n listed envs — row i of
 * device_out [n][state_dim] (doubles) is the flat state row of env
 * env_ids[i]; ids may repeat.  env_ids NULL = all envs in order (n ignored).
 * Like bioim_copy_state it does not check for envs suspended mid-step. */
int bioim_copy_state_rows(bioim_handle_t *h, const int32_t *env_ids, int n, void *device_out);
/* bioim_load_state: bioim_set_state for the n listed envs from device rows
 * [n][state_dim] (doubles, bioim_get_state's layout) — row i goes to env
 * env_ids[i] (distinct ids; NULL = all envs in order, n ignored), with
 * bioim_set_state's conversions (values to the handle's precision; istep,
 * has_last and done truncated to int32).  The listed envs are put at a step
 * boundary (a suspended RK step is dropped) and their realize-cache rows are
 * marked stale; their fiber-velocity warm starts and counters stay, as with
 * bioim_set_state.  Every other env is left exactly as it is, its realize
 * cache included (bioim_set_state clears every env's). */
int bioim_load_state(bioim_handle_t *h, const int32_t *env_ids, int n, const void *device_rows);
/* bioim_clone_envs: for each of the n pairs, env dst_ids[i] becomes a copy
 * of env src_ids[i] that continues bit for bit like it under the same
 * actions.  The whole per-env record is copied, not only the flat row:
 * q, u, activations, fiber lengths, the action history, last action, old
 * pelvis x, time, step index, has_last, done, the RK step size, the
 * suspended-step record (pending flag, integration time, step size, attempt
 * count, held controls, smoothed actions), the fiber-velocity warm starts
 * and the realize-cache row with its valid flag.  A clone of an env that is
 * suspended mid-step by the RK budget is suspended as well and resumes
 * identically.  Not copied: the env's reset counter and RK counters (its
 * shares of bioim_reset_count / bioim_eval_count / bioim_finished_count,
 * which a clone therefore leaves unchanged) and its row of the push table
 * (bioim_set_perturbation).  Device-drawn reset rows are a function of the
 * seed, the global env index and the env's reset counter, so after its next
 * reset without a ref_index (an auto-reset included) a clone draws its own
 * row, not the one its source draws: the two part ways there.  The same src
 * may appear many times; dst ids must be distinct and none of them may also
 * be a src (the caller's contract: a violation races on that env's record,
 * it does not leave the state buffer).  One launch. */
int bioim_clone_envs(bioim_handle_t *h, const int32_t *src_ids, const int32_t *dst_ids, int n);
/* bioim_rollout: `steps` consecutive env steps from an action sequence, for
 * shooting planners, population branching (after bioim_clone_envs) and action
 * repeat.  Every pointer is a device pointer on the handle's device, in the
 * handle's precision and I/O strides:
 *   actions: step k reads [N][act_stride] at actions + k * action_step_stride
 *     elements; a stride of 0 repeats the same actions every step (frame skip);
 *   reward_seq [steps][N] (may be NULL); done_seq [steps][N] (required);
 *   obs_seq (may be NULL) [steps][N][obs_stride];
 *   obs_last (may be NULL) [N][obs_stride]: the last step's rows only;
 *   info_seq (may be NULL) [steps][N][info_stride].
 * State and every output are bit for bit those of `steps` bioim_step calls on
 * the same slices: in-kernel auto-resets (reset-table rows, device-drawn
 * rows, reset counters), the realize cache, the active mask (a masked-out
 * env's rows are left as they are) and final_obs, which keeps the last
 * step's values.  The reset table is built before the launch, as on
 * bioim_step's first step.  Asynchronous on the handle's stream; apart from
 * that one-time table build (and the first stop_at_done call's allocation of
 * its mask) nothing is synchronized on the default path.
 * stop_at_done (auto-reset off only): an env whose step k returned done is
 * not stepped again in this call — its state stays the one right after that
 * step, its later rows are reward 0, done 1, info 0 and its terminal
 * observation again (obs_last holds the terminal one).  The caller's active
 * mask is read, never written: the call keeps its own mask per handle.
 * Paths: with the default step configuration (semi-implicit, no push table,
 * no force report, no state storage) the whole call is ONE launch of the
 * rollout kernel, which runs the step kernel's code in a loop (step k+1 of
 * an env reads only what its own workgroup stored in step k), and
 * bioim_rollout_fused returns 1.  With a push table, unbudgeted RK-Merson, a
 * force report or state storage the same call enqueues `steps` launches of
 * the step kernels from C (results identical, bioim_rollout_fused returns 0;
 * an RK handle's check for suspended envs waits for its stream).
 * Refused with BIOIM_E_ARG and a message before any device call: a null
 * handle, null actions or done_seq, steps <= 0, a negative stride, a budgeted
 * RK handle (rk_budget > 0: a suspended step has no per-step rows) or one
 * with suspended envs, stop_at_done with auto-reset on.  The buffers' sizes
 * are the caller's contract (VectorEnv.rollout checks them).  No reference
 * counterpart (one OsimModel steps one env from Python). */
int bioim_rollout(bioim_handle_t *h, const void *actions, int steps, int64_t action_step_stride,
                  void *obs_seq, void *obs_last, void *reward_seq, uint8_t *done_seq, void *info_seq,
                  int stop_at_done);
/* 1 if the last bioim_rollout on h ran as one launch of the rollout kernel, 0
 * if it looped over the step kernels (or none ran yet); -1 for a null handle. */
int bioim_rollout_fused(const bioim_handle_t *h);
/* bioim_rollout_group: `steps` consecutive env steps of a mixed batch from an
 * action sequence — bioim_rollout for the handles of bioim_step_group.  The
 * buffers are that call's padded full-batch ones (all handles on one device,
 * same precision and I/O strides): handle i owns rows [sum(n_<i), sum(n_<=i))
 * of every step's slice, N is the sum of the handles' env counts:
 *   actions: step k reads [N][act_stride] at actions + k * action_step_stride
 *     elements; a stride of 0 repeats the same actions every step;
 *   reward_seq [steps][N] (may be NULL); done_seq [steps][N] (required);
 *   obs_seq (may be NULL) [steps][N][obs_stride];
 *   obs_last (may be NULL) [N][obs_stride]: the last step's rows only;
 *   info_seq (may be NULL) [steps][N][info_stride].
 * State and every output are bit for bit those of `steps` bioim_step_group
 * calls on the same slices: in-kernel auto-resets (reset-table rows, reset
 * counters), the realize cache, each handle's active mask and final_obs.
 * Columns past a handle's own row widths are not written.
 * stop_at_done (auto-reset off in every handle) works as in bioim_rollout,
 * per env; each handle's caller mask is read, never written (the call keeps
 * its own mask per handle).
 * Asynchronous on hs[0]'s stream; only the one-time reset-table builds and
 * the first stop_at_done call's allocation of a handle's mask synchronize
 * (an RK handle's check for suspended envs waits for its stream).
 * Paths: where bioim_step_group would fuse (nh == 2, group fusion on, fp64,
 * a fused topology pair, no push table, semi-implicit) and neither handle
 * has a force report or state storage, the whole call is ONE launch of the
 * two-topology rollout kernel (the workgroups of one segment first, then the
 * other's; the per-step pitch of the sequence buffers is N rows), and
 * bioim_rollout_group_fused returns 1.  Every other case loops from C over
 * what bioim_step_group enqueues per step — the fused step launch where
 * eligible, else one launch per segment, forked and joined — followed, with
 * stop_at_done, by the per-segment freeze launches on hs[0]'s stream; results
 * identical, bioim_rollout_group_fused returns 0.  bioim_group_fused's answer
 * is left as it was.  nh == 1 behaves as bioim_rollout.
 * Refused with BIOIM_E_ARG and a message starting "bioim_rollout_group:"
 * before any device call: null hs, nh <= 0 or a null handle in the list, null
 * actions or done_seq, steps <= 0, a negative stride, handles differing in
 * device, precision or I/O strides, any budgeted RK handle (rk_budget > 0) or
 * one with suspended envs, stop_at_done with auto-reset on in any handle.
 * The buffers' sizes are the caller's contract (MixedVectorEnv.rollout checks
 * them).  No reference counterpart (one OsimModel steps one env from Python;
 * the mixed batch is this project's). */
int bioim_rollout_group(bioim_handle_t **hs, int nh, const void *actions, int steps, int64_t action_step_stride,
                        void *obs_seq, void *obs_last, void *reward_seq, uint8_t *done_seq, void *info_seq,
                        int stop_at_done);
/* 1 if the last bioim_rollout_group with h as its first handle ran as one
 * launch of the two-topology rollout kernel (nh == 1: of the rollout kernel),
 * 0 if it looped over the step kernels (or none ran yet); -1 for a null
 * handle. */
int bioim_rollout_group_fused(const bioim_handle_t *h);

/* Integrator of the physics between env steps.  kind 0: the fixed
 * semi-implicit substeps (the pack's nsub; default).  kind 1: the reference's
 * integrator, an adaptive Kutta-Merson 4(5) at `accuracy` (OpenSim's
 * Manager, opensim_wrapper.py:287-301, accuracy 1e-3 from
 * muscle_walking_imitation_env2D.py:42), restated in
 * oracle/bioim_oracle.c integrate_rk_merson.  Replaces the integrator
 * choice inside OsimModel.reset_manager. */
int bioim_set_integrator(bioim_handle_t *h, int kind, double accuracy);
/* Budgeted steps for the adaptive integrator (kind 1).  attempts > 0: each
 * bioim_step gives every env at most `attempts` Kutta-Merson step attempts
 * (5 dynamics evaluations each);
 * an env whose env step is not finished by then is suspended at its last
 * accepted integration point and resumed by the next bioim_step (its action
 * row is ignored until it finishes).  ready_out (device [n], may be NULL)
 * receives 1 for the envs whose step finished in this launch — only their
 * obs / reward / done / info rows are written (done is 0 for the others).
 * A resumed step continues bit for bit as if it had never been suspended
 * (state, step size, attempt count and the fiber-velocity warm starts are
 * saved), so the trajectories equal the unbudgeted run's; what changes is
 * that one stiff env no longer holds the whole launch.  The consumer pattern
 * is RLlib's BaseEnv.poll() / send_actions(): new actions only for ready
 * envs.  attempts = 0 restores one-step-per-launch.  No reference
 * counterpart (OpenSim steps one env at a time). */
int bioim_set_rk_budget(bioim_handle_t *h, int attempts, uint8_t *ready_out);
/* Dynamics evaluations the adaptive integrator (kind 1) has spent so far,
 * summed over the handle's envs (5 per Kutta-Merson attempt, 1 per realize
 * after a step or reset).  Synchronizes the handle's streams.
 * 0 for handles that never ran the adaptive integrator.  No reference
 * counterpart (bench.py's evaluations per env step). */
int bioim_eval_count(bioim_handle_t *h, uint64_t *total);
/* Env steps the adaptive integrator (kind 1) has finished so far, summed
 * over the handle's envs: the count of bioim_step rows whose ready flag was
 * 1 (bioim_set_rk_budget).  Synchronizes the handle's streams.  No reference
 * counterpart (bench.py counts the reference-integrator rate with it instead
 * of reading ready[] after every launch). */
int bioim_finished_count(bioim_handle_t *h, uint64_t *total);
/* Sets every env's two RK counters (the evaluations and the finished steps
 * that bioim_eval_count / bioim_finished_count sum) to the given values,
 * e.g. to restart the counting of a measurement window or to carry counts
 * across a handle re-creation.  Each counter is 32 bits per env and wraps on
 * its own (no carry into the other).  Synchronizes the handle's streams.  No
 * reference counterpart. */
int bioim_set_rk_counters(bioim_handle_t *h, uint32_t evals, uint32_t finished);
/* envs suspended mid-step (synchronizes the handle's stream) */
int bioim_pending_count(bioim_handle_t *h);
/* Optional per-env step mask (device [n], NULL = every env steps): an env
 * with 0 is left untouched by bioim_step (state, outputs, ready flag) unless
 * it is finishing a suspended RK step.  Lets an asynchronous consumer step
 * only the envs it sent actions to (RLlib BaseEnv.send_actions). */
int bioim_set_active_mask(bioim_handle_t *h, const uint8_t *active);
/* Optional terminal-observation output: when set (a device buffer with the
 * handle's obs row stride), every step also writes each env's observation
 * as computed by that step *before* an in-kernel auto-reset replaces it, so
 * a done env's terminal observation survives (gym's final_observation;
 * bootstrapping in the reference's jaxrl SAC loop,
 * tests/sample_baselines_training.py:69-91).  NULL disables it. */
int bioim_set_final_obs(bioim_handle_t *h, void *final_obs);
/* Optional per-force-element report (the reference's ForceReporter analysis,
 * opensim_wrapper.py:10-15, printed by save_simulation :334-338): when set,
 * every realize writes per env a row of bioim_force_report_dim() values:
 * [actuation of each muscle (tendon force, N) or coordinate actuator
 * (control x optimal force)] [per Hunt-Crossley force: force (3) and moment
 * about the ground origin (3) on the feet] [per CoordinateLimitForce: its
 * generalized force] [per contact sphere, pack order: its force (3) on its
 * OpenSim body and the moment (3) about that body's origin, in ground — the
 * HuntCrossleyForce record's foot-side entries sum these per body].  NULL
 * disables it. */
int bioim_force_report_dim(const bioim_handle_t *h);
/* Optional state storage of the adaptive integrator (kind 1): OpenSim's
 * Manager stores the state at every accepted integration step, which
 * save_simulation prints (opensim_wrapper.py:334-337).  When set, each env
 * step (bioim_step, or bioim_osim INTEGRATE) writes per env one row per
 * accepted Kutta-Merson step: rows [n][capacity][1 + 2 ndof + 2 nmuscle] =
 * (time, q, u in dof order, activation, fiber length); count[n] receives the
 * number of accepted steps of the env's last env step (rows beyond capacity
 * are counted, not stored; a budgeted step's count spans its launches).
 * Device buffers owned by the caller; rows = NULL disables it. */
int bioim_set_state_storage(bioim_handle_t *h, void *rows, int capacity, int32_t *count);
int bioim_set_force_report(bioim_handle_t *h, void *force_out);
/* Sum over the handle's envs of their reset counters (explicit resets and
 * in-kernel auto-resets); synchronizes the handle's streams.  Lets a caller
 * count terminations over a stretch of steps without touching the step
 * launches (bench.py's done rate).  No reference counterpart. */
int bioim_reset_count(bioim_handle_t *h, uint64_t *total);
/* out[0..7] = n_envs, obs_dim, nact, info_dim, precision, lanes_per_env, nsub, state_dim */
int bioim_query(const bioim_handle_t *h, int32_t *out);
/* out[0..4] = lanes per env, threads per workgroup, envs per workgroup,
 * LDS bytes per workgroup (model image + env regions), workgroups per step */
int bioim_query_launch(const bioim_handle_t *h, int32_t *out);
void *bioim_stream(bioim_handle_t *h);
int bioim_set_stream(bioim_handle_t *h, void *hip_stream);
int bioim_sync(bioim_handle_t *h);
const char *bioim_last_error(void);
/* sizeof(bioim_modelpack_t) as compiled into the library (layout check). */
uint64_t bioim_modelpack_size(void);
/* Build id: sha256 (16 hex digits) over the kernel sources and hipcc flags the
 * library was compiled from (bioimitation/_buildinfo.py); the Python host
 * refuses a library whose id differs from its source tree's.  No reference
 * counterpart (build hygiene). */
const char *bioim_build_id(void);

/* ---- debug / tests ---- */
/* One whole plane of the per-env record, by the name of its DState member
 * (q, u, act, lce, hist, last, old_px, t, istep, has_last, done, resets, hrk,
 * pend, rkt, rkh, rka, ctl, cur, vnw, rkev, cache, cache_ok), copied
 * device -> host, or host -> device when `write` is not 0.  Synchronizes both
 * of the handle's streams first.  The plane is raw device memory:
 * [count][N] with the env index fastest (the cache: [N][cache_dim] rows), in
 * the handle's precision for the real-valued planes (t, hrk, rkt, rkh are
 * doubles; the flags and counters int32; rkev uint64).  `bytes` must be the
 * plane's exact size; an unknown name, a null handle or buffer or another
 * size returns BIOIM_E_ARG before any device call.  For tests of what the
 * flat state row does not show (the realize cache and its flags, the warm
 * starts, a suspended RK step, the counters); a write is taken as is, so a
 * caller can leave an env's record inconsistent on purpose.  No reference
 * counterpart. */
int bioim_debug_plane(bioim_handle_t *h, const char *name, void *host, size_t bytes, int write);

#ifdef __cplusplus
}
#endif
#endif /* BIOIM_H */
