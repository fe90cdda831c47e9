// bioim_config.h — the compile-time switches of libbioim.so that have a
// default, and the macros every layer uses.  Each `#ifndef BIOIM_X` below is a
// default that a -DBIOIM_X=... on the compile line overrides
// (tools/build_variants.py, tools/ab_flags.sh); the shipped objects are built
// with none set.  Not here, because they select text where they stand:
// BIOIM_ID_NO_WAVES_ATTR (id_kernel's attributes), BIOIM_BUILD_ID (the build
// stamps it, beside bioim_build_id()), and the unit selectors BIOIM_TOPO_ONLY /
// BIOIM_ABI_ONLY / BIOIM_FUSED_ONLY (bioim_step.hip); and with what they size:
// BIOIM_LDS_PAD (bioim_device.h), BIOIM_G_SPATIAL_MUSCLE (topologies.h).
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "bioim.h"

#define DEV __device__ __forceinline__
#define BIOIM_EPB 16 /* envs per workgroup (BIOIM_EPB * G threads) share one LDS model image */
/* env flags baked into a kernel (topologies.h FLAGS); RAW_ACTION, TARGET_OBS, GRF_OBS are run-time */
#define BIOIM_STRUCT_FLAGS (BIOIM_ENV_MUSCLE | BIOIM_ENV_HAS_TZ | BIOIM_ENV_REWARD_FEET | BIOIM_ENV_DONE_CROSS | BIOIM_ENV_PD)

#ifndef BIOIM_CHECK
#define BIOIM_CHECK 0
#endif
/* BIOIM_CHECK=1 (a diagnostic build, never shipped): every global load and
 * store of the env kernel goes through a bounds check that prints the source
 * line, the index, the bound, the workgroup and the thread, then traps — the
 * stale-lane class of DESIGN.md 5.5 then ends as a named trap instead of an
 * anonymous illegal-address fault.  With BIOIM_CHECK=0 the accessors expand to
 * plain subscripts (the shipped kernels are unchanged).  The accessors pass
 * __FILE__ with __LINE__: they are used from several files, and __FILE__
 * inside bioim_chk would always name this header. */
DEV size_t bioim_chk(size_t i, size_t n, const char *file, int line) {
    if (i >= n) {
        printf("BIOIM_CHECK %s:%d index %llu outside [0, %llu) workgroup %u thread %u\n", file, line,
               (unsigned long long)i, (unsigned long long)n, blockIdx.x, threadIdx.x);
        __builtin_trap();
    }
    return i;
}
#if BIOIM_CHECK
#define GAT(p, i, n) ((p)[bioim_chk((size_t)(i), (size_t)(n), __FILE__, __LINE__)])
#define GIDX(i, n) bioim_chk((size_t)(i), (size_t)(n), __FILE__, __LINE__)
#else
#define GAT(p, i, n) ((p)[i])
#define GIDX(i, n) (i)
#endif

#ifndef BIOIM_ENV_MOD
#define BIOIM_ENV_MOD -1
#endif
#ifndef BIOIM_BF3
#define BIOIM_BF3 122
#endif
#ifndef BIOIM_BF_SPATIAL
#define BIOIM_BF_SPATIAL 0
#endif
/* BIOIM_BF3_RK=1 (shipped): the BIOIM_BF3 pieces in the spatial RK-Merson
 * kernels too — no scratch, hazard gate clean, same-box Running3D RK launch
 * 0.7826 -> 0.7452 ms, LockedKnee3D 0.7289 -> 0.6989 ms (profiles/r04/r04g/ab_rk.log) */
#ifndef BIOIM_BF3_RK
#define BIOIM_BF3_RK 1
#endif
/* fiber-velocity warm start (round-5 experiments): BIOIM_FV_HERMITE = cubic
 * Hermite u(v) start from the table slopes instead of linear interpolation;
 * BIOIM_FV_PRED = linear extrapolation of the previous two substeps' roots
 * in the semi-implicit substep loop */
#ifndef BIOIM_FV_HERMITE
#define BIOIM_FV_HERMITE 0
#endif
#ifndef BIOIM_FV_PRED
#define BIOIM_FV_PRED 0
#endif
/* the substep's fiber-length update through fast_rcp instead of the IEEE
 * division (round-5 experiment, off: the oracle divides, and after 6 steps
 * the realize report drifted to 1.4e-9 of it, past the 1e-9 report test,
 * profiles/r05/r05p/gpu_tests.log) */
#ifndef BIOIM_SUBSTEP_RCP
#define BIOIM_SUBSTEP_RCP 0
#endif
/* BIOIM_SGB: sched_group_barrier pipelines in the muscle eval (round-5
 * experiment, off; same box C3 +1.3 % / +1.8 %: profiles/r05/r05o) */
#ifndef BIOIM_SGB
#define BIOIM_SGB 0
#endif
/* solve_fv: a lane whose root lies past the curve's end leaves the Newton
 * loop after one step (0: it iterates to the segment end as before) */
#ifndef BIOIM_FV_PAST_END
#define BIOIM_FV_PAST_END 1
#endif
#ifndef BIOIM_FV_PE_PLANAR
#define BIOIM_FV_PE_PLANAR 0
#endif
/* the reset table (LaunchArgs::reset_tab) in the planar RK-Merson step
 * kernels too, and (round 6) in the spatial ones: they fit it at 486-512
 * registers with no scratch; same-box reference-integrator legs C4 +3.9 %,
 * LockedKnee3D +4.4 %, Palsy3D +5.6 % (profiles/r06/r06e/ab_rk.txt) */
#ifndef BIOIM_RESET_TAB_RK_SPATIAL
#define BIOIM_RESET_TAB_RK_SPATIAL 1
#endif
#ifndef BIOIM_RESET_TAB_RK
#define BIOIM_RESET_TAB_RK 1
#endif

/* BIOIM_EXACT_RCP=1: a diagnostic build (never shipped) whose reciprocals
 * and inverse square roots (bioim_math.h) are IEEE divisions and square
 * roots, the oracle's operations — to attribute the GPU's operation-level
 * distance from the oracle */
#ifndef BIOIM_EXACT_RCP
#define BIOIM_EXACT_RCP 0
#endif

/* The realize cache (DState::cache): a step's realize runs at
 * the state the next step's first substep starts from, and a muscle model's
 * forces there do not depend on the excitations the policy sends next (they
 * enter only the activation rate).  So the realize also forms the implicit
 * system of that substep (h = the next step's substep length: M + h C + h^2 K
 * and its right-hand side, CJ / LIM at that h) and the muscles' fiber-velocity
 * roots, and stores them per env; the next launch's first substep loads them
 * and goes straight to the solve instead of a whole dynamics call.  Torque
 * models: the actuator torques are the controls, so their cached right-hand
 * side stops short of them and the cached substep adds this step's. */
#ifndef BIOIM_REALIZE_CACHE
#define BIOIM_REALIZE_CACHE 1
#endif
#ifndef BIOIM_REALIZE_CACHE_SPATIAL
#define BIOIM_REALIZE_CACHE_SPATIAL 1
#endif
#ifndef BIOIM_REALIZE_CACHE_TORQUE
#define BIOIM_REALIZE_CACHE_TORQUE 1
#endif
/* the spatial kernels load the cache row at the substep (0) or at kernel
 * start like the planar ones (1) */
#ifndef BIOIM_CACHE_PREFETCH_SPATIAL
#define BIOIM_CACHE_PREFETCH_SPATIAL 0
#endif

/* BIOIM_FRONTEND (the step kernels' dynamics calls; the analysis kernels
 * reach these helpers through state_kinematics with FE = 0, the forms below
 * without it): waits and duplicate LDS traffic taken out of the kinematics
 * front end, every arithmetic operation and its order kept.  One bit per item:
 *   1 (FE_COLS)    kin_local sums a body's joint columns per local dof in
 *                  registers (0 + its axes' contributions, in axis order) and
 *                  stores each dof's words to SL once: no read-modify-write of
 *                  SL at a run-time dof index, no per-call zeroing of SL, and
 *                  an axis without a dof contributes to nothing (no sink row)
 *   2 (FE_KINDS)   planar kin_local: the linear / constant axis forms are
 *                  computed from unconditional loads and selected (as the
 *                  spline arm), no EXEC-masked arm per kind
 *   4 (FE_INERTIA) kin_chain hands its frame to body_inertia in registers, in
 *                  the same body-lane block: no reload of KB / AL, and the
 *                  columns run with the subtree sums' reads (one sync fewer)
 *   8 (FE_LEVEL0)  the chain's first level composes with the ground frame
 *                  (R = I, o = (-x0, 0, 0), no motion) by copy and offset
 * One byte per kernel family (TailSwitch): bits 0-7 the planar topologies'
 * kernels, 8-15 the spatial ones', 16-23 the fused two-topology kernels.
 * Shipped (same-box A/B): all four in the planar kernels.  None in
 * the spatial ones: FE_LEVEL0 changes result bits there (the fused kernels and
 * the parent build no longer agree with them bit for bit), FE_INERTIA alone
 * puts one spatial RK kernel on scratch, and FE_COLS | FE_INERTIA gained less
 * than the builds' round spread on Running3D.  None in the fused kernels, which
 * measured no faster with any of them. */
#ifndef BIOIM_FRONTEND
#define BIOIM_FRONTEND 0x00000F
#endif
constexpr int FE_COLS = 1, FE_KINDS = 2, FE_INERTIA = 4, FE_LEVEL0 = 8;

/* BIOIM_LANEIDX (the step kernels' dynamics calls; the analysis kernels and
 * state_kinematics call the helpers without a record, the forms below without
 * it): the small integers a lane reads from the model image in every call —
 * body slots, gather lists, path point numbers, which depend on the lane
 * alone — are read once per launch into a packed per-lane record (LaneIdx,
 * bioim_kinematics.h) that stays in registers; a call unpacks them with a
 * bit-field extract instead of a dependent LDS round trip.  Only loads and
 * integer arithmetic go; every floating-point operation and its order stay.
 * One bit per consumer:
 *   1 (LI_COLS)   kin_column's parent-frame offset, phase 3's body (WB, IC)
 *   2 (LI_TAU)    the dof lane's TAU gather list (phase 3 and the cached first
 *                 substep), its limit mask, the limit lane's coordinate
 *   4 (LI_PATH)   muscle_path: the muscle's point offset and count, its span,
 *                 each point slot's frame, and the conditional / moving slots'
 *                 flags, coordinate and function slots
 * One byte per kernel family, as BIOIM_FRONTEND.  Shipped (same-box A/B,
 * DESIGN.md 9): all three in the planar kernels; the spatial and the fused byte
 * are 0 (not measured there), the RK kernels take none (TailSwitch), and
 * those kernels are unchanged.  Two more bits were measured and taken out:
 * the muscle curves' base offsets (slower) and the function slots' numbers
 * (inside the spread). */
#ifndef BIOIM_LANEIDX
#define BIOIM_LANEIDX 0x000007
#endif
constexpr int LI_COLS = 1, LI_TAU = 2, LI_PATH = 4;

/* BIOIM_GROUND_ONCE (the step kernels): the ground slot's constants — the KB
 * rotation, its zero origin / velocity words and the zero AL row, which no
 * other code writes — go to LDS once per launch (kin_ground_const) and a call
 * writes only kb[9] = -x0.  The identity LOC slot lies in the union region:
 * where the call's force slots (TAU, CJ) end below it (ground_loc_free), only
 * the report's staging (OBS, REP) writes over it, and it is written once per
 * launch too and again before a realize that follows a report (the reset
 * realize); elsewhere (the spatial muscle topologies) it stays with the call.
 * Bits (TailSwitch): 1 the planar topologies' kernels, 2 the spatial ones',
 * 4 the fused two-topology kernels (env_kernel2, rollout_kernel2), which
 * measured no faster with it (C5 0.4687 -> 0.4708 ms same box) and keep the
 * per-call writes. */
#ifndef BIOIM_GROUND_ONCE
#define BIOIM_GROUND_ONCE 3
#endif

/* the reference integrator's attempt cap per env step (rk_update) */
#define BIOIM_RK_MAX_ATTEMPTS 4096
