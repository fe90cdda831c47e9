// bioim_layout.h — where things live: the muscle-to-lane-slot map, the per-env
// LDS region (Lay), the realize-cache row (CacheLay), the report slots and the
// observation offsets.
#pragma once

#include <hip/hip_runtime.h>

#include "bioim_config.h"
#include "bioim_device.h"
#include "bioim_math.h"
#include "topologies.h"

/* muscle of lane slot s (slot = lane + j * G): when the muscles take two
 * passes over the lanes, the second, partly idle pass holds the cheapest
 * paths (T::mperm, tools/build_packs.py); a bijection of [0, NM), the
 * identity elsewhere, so slot-range checks stay valid */
template <class T> DEV int mslot(int s) {
    int r = s;
    if constexpr (T::NM > T::G) {
        sfor<0, T::NM>([&](auto iI) {
            constexpr int i = decltype(iI)::value;
            r = s == i ? T::mperm[i] : r;
        });
    }
    return r;
}

/* ---------------------------------------------------------- LDS layout
 * Per workgroup: the shared model image (SModel, bioim_device.h), then one
 * region per env.  Phase 1 (lane-parallel kinematics) publishes frames,
 * Plucker columns, per-body inertias and Newton-Euler wrenches; the force
 * phases read them and publish per-lane slots that are reduced in a fixed
 * order (bitwise deterministic).  The union region U is reused by phase 1
 * (joint-local data), phases 2-3 (force slots) and the observation staging. */
template <class T, typename Real> struct Lay {
    static constexpr int NB = T::NB, ND = T::ND > 0 ? T::ND : 1, NC = T::NC, NP = ND * (ND + 1) / 2;
    static constexpr int NMS = T::NM > T::NA ? T::NM : T::NA;
    static constexpr int MPL = (NMS + T::G - 1) / T::G;      /* muscles (actions) per lane            */
    static constexpr int NS = T::NS > 0 ? T::NS : 1, NL = T::NL > 0 ? T::NL : 1;
    static constexpr int CJN = 10;               /* per sphere: P3, F3 (implicit), C4 (xx xz yy zz)  */
    static constexpr int NTR = (T::TX >= 0) + (T::TY >= 0) + (T::TZ >= 0);
    /* largest observation of the topology (target obs and GRF on) */
    static constexpr int OBSMAX = 1 + (NC - NTR) + 2 * NC + 2 * (NC - 1) + 3 * (T::NOBP + T::NOBV) + 3 * T::NM +
                                  6 * T::NF;
    static constexpr int KB = 0;                 /* [NB+1][18]: R9 o3 w3 vO3 (slot NB: ground)      */
    static constexpr int AL = KB + 18 * (NB + 1); /* [NB+1][6]: alpha3, aO3 (velocity-product accels) */
    static constexpr int S = AL + 6 * (NB + 1);  /* [ND][6]: Plucker columns (Omega, V at origin)   */
    static constexpr int QF = S + 6 * ND;        /* [NC] coordinate values                          */
    static constexpr int UF = QF + NC;           /* [NC] coordinate speeds                          */
    static constexpr int IC = UF + NC;           /* [NB][10]: m, h3, J6; then in place: subtree sums */
    static constexpr int WB = IC + 10 * NB;      /* [NB][6]: n3, f3; then in place: subtree sums     */
    static constexpr int MP = WB + 6 * NB;       /* [NP] packed lower M (+implicit)                 */
    static constexpr int RHS = MP + NP;          /* [ND]                                            */
    static constexpr int CW = RHS + ND;          /* [NS][8]: F3, Mo3, active                        */
    static constexpr int LIM = CW + 8 * NS;      /* [NL][4]: f, diag add, tau add                   */
    static constexpr int NSLOT = TopoInfo<T>::nslot();
    static constexpr int MF = LIM + 4 * NL;      /* [NSLOT][3]: function slots f, f', f''           */
    static constexpr int U = ((MF + 3 * (NSLOT > 0 ? NSLOT : 1) + 1) / 2) * 2;
    static constexpr int LOC = U;                /* phase 1: [NB+1][24] joint-local data (NB: identity) */
    static constexpr int SL = LOC + 24 * (NB + 1); /* phase 1: [ND][6] joint-local Plucker columns, + sink row */
    /* phases 2-3: [MPL * G][MAXSPAN] per muscle slot, -F_t dL/dq over its
     * span (actuator slot: its torque), then one zero slot (TZ) */
    static constexpr int TZ = MPL * T::G * T::MAXSPAN;
    static constexpr int TAUN = TZ + 1;
    static constexpr int TAU = U;
    static constexpr int CJ = TAU + TAUN;        /* phases 2-3: [NS][CJN] contact slots             */
    static constexpr int OBS = U;                /* report: observation staging                     */
    static constexpr int REP = OBS + OBSMAX;     /* report: [NOS+1][6] body pos/vel (NOS: COM)      */
    static constexpr int U1 = 24 * (NB + 1) + 6 * (ND + 1), U2 = TAUN + NS * CJN;
    static constexpr int U3 = OBSMAX + 6 * (T::NOS + 1);
    static constexpr int USZ = U1 > U2 ? (U1 > U3 ? U1 : U3) : (U2 > U3 ? U2 : U3);
    static constexpr int SIZE0 = ((U + USZ + 1) / 2) * 2;
    /* per-env stride residue mod 32 doubles (BIOIM_ENV_MOD >= 0, planar
     * topologies; the spatial ones have no LDS to spare): it sets which banks
     * the other env of a 32-lane group hits (ds_read_b64: 2 x 32 lanes;
     * ds_read_b128: 16-lane groups mixing both envs) */
    static constexpr int SIZE = (BIOIM_ENV_MOD >= 0 && T::PLANAR) ? SIZE0 + ((BIOIM_ENV_MOD - SIZE0 % 32) + 32) % 32 : SIZE0;
};

template <class T> struct CacheLay {
    /* torque models: the cached right-hand side leaves out the actuator
     * torques (the controls), which the cached substep adds */
    static constexpr bool ON = BIOIM_REALIZE_CACHE &&
                               (T::NM > 0 ? (T::PLANAR || BIOIM_REALIZE_CACHE_SPATIAL) : BIOIM_REALIZE_CACHE_TORQUE);
    /* planar kernels load the row at kernel start, ahead of the action
     * pre-processing; the spatial ones (no register headroom) at the substep */
    static constexpr bool PREFETCH = T::PLANAR || BIOIM_CACHE_PREFETCH_SPATIAL;
    static constexpr int ND = T::ND > 0 ? T::ND : 1, NP = ND * (ND + 1) / 2;
    static constexpr int SYS = NP + ND;          /* [NP] packed lower M(h), [ND] rhs(h): LDS MP..RHS order */
    static constexpr int MUS = SYS;              /* [NM][3] fiber-velocity root, dv/dl, clamped (0 / 1) */
    static constexpr int H = MUS + 3 * T::NM;    /* the h the system was formed at */
    static constexpr int DIM = ON ? H + 1 : 0;
    static constexpr int PF = (SYS + T::G - 1) / T::G;   /* system values per lane */
};

/* apply_perturbations kernels only: per env 5 doubles after all env regions
 * (call time base, substep length, cursor segment [lo, hi), its force) */
constexpr int PERT_SLOT = 5;

/* external-force kernels only (bioim_set_external_forces): per env the
 * caller's BIOIM_MAX_EXT rows of 9 values (force, point, torque), staged once
 * per launch after all env regions.  LDS: the slots fit beside the image and
 * the env regions; where they do not (the 7-body spatial muscle topology in
 * fp64 has 832 bytes to spare, the slots take 9216) the body lanes read the
 * caller's rows at each dynamics call instead. */
constexpr int EXT_ROW = 9;
template <class T, typename Real> struct ExtLay {
    static constexpr int SLOT = BIOIM_MAX_EXT * EXT_ROW;   /* reals per env */
    static constexpr size_t BYTES = (size_t)BIOIM_EPB * SLOT * sizeof(Real);
    static constexpr bool LDS = smodel_bytes<T, Real>() + (size_t)BIOIM_EPB * Lay<T, Real>::SIZE * sizeof(Real) + BYTES <= 163840;
};

/* REP slot of an OpenSim body index (-1 = COM) */
template <class T> DEV constexpr int rep_slot(int ob) { return ob >= 0 ? ob : T::NOS; }

/* observation offsets (get_state_dict order, muscle_walking_imitation_env2D.py:158-225) */
template <class T> struct ObsLayout {
    static constexpr int NTR = (T::TX >= 0) + (T::TY >= 0) + (T::TZ >= 0);
    static constexpr int NQ = T::NC - NTR;
    static constexpr int QPOS = 1, QVEL = QPOS + NQ, QACC = QVEL + T::NC, TGT = QACC + T::NC;
    static constexpr int body(bool tgt) { return TGT + (tgt ? 2 * (T::NC - 1) : 0); }
};
