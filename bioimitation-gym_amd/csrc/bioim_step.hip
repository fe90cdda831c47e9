// bioim_step.hip — MI355X (gfx950) batched env step for bioimitation-gym.
//
// One launch advances N environments by one env step (0.01 s): action
// pre-processing, nsub semi-implicit substeps of the musculoskeletal
// forward dynamics, the realize at the end state, and the observation,
// reward and termination of the reference's task envs.
//
// Work decomposition (CDNA4, wave64): an environment is a
// group of G = 16 lanes for every topology, 4 envs per wave, 16 envs per
// 256-thread workgroup, one wave per SIMD.
//   - lanes take roles per phase: composite body (joint kinematics, frame
//     composition, inertias, subtree sums), dof (lane d owns coordinate d's
//     value and speed in registers, M entries, rhs), muscle (path geometry,
//     moment arms over its span, Millard damped equilibrium; lane l also
//     takes muscle l + 16 where a topology has more than 16), contact sphere,
//     limit force, report slot;
//   - lanes of one env exchange data through its per-env LDS region (frames,
//     Plücker columns, packed M, torque slots) with wave-scope fences: the env
//     never leaves its wave; group sums are xor-butterflies (bitwise identical
//     totals on every lane);
//   - the tree-sparse LTL solve runs redundantly on every lane in registers;
//   - the lane-indexed model image (muscles, path points, joints, splines,
//     spheres) is staged into LDS once per workgroup; uniform constants and
//     the reference-motion tables are scalar loads.
// Per-env state is SoA in HBM (env index fastest).  Reference semantics: see
// oracle/bioim_oracle.c, which this kernel must match (tests/test_gpu_*.py).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <memory>
#include <vector>

#include "bioim.h"
#include "bioim_device.h"
#include "topologies.h"

// The lowest layers, lowest first (DESIGN.md 5.6 has the map); each header
// includes what it uses.
#include "bioim_config.h"
#include "bioim_math.h"
#include "bioim_diag.h"
#include "bioim_layout.h"
#include "bioim_curves.h"
#include "bioim_kinematics.h"

/* ---------------------------------------------------- contact + limits */

/* Hunt-Crossley sphere s (this lane) vs the ground plane.  Publishes the
 * sphere's wrench about the (shifted) ground origin (CW) and, for the
 * generalized force / implicit matrix, the contact point P, the force F
 * (normal component at the implicitly advanced position) and the 3x3
 * implicit damping/stiffness block C (h > 0) into CJ.  Phase 3 forms the
 * contact-point Jacobian J_d = S_d.ang x P + S_d.lin from the Plucker
 * columns it already holds: M_lk += J_l.C J_k, rhs_d += S_d.(P x F, F). */
/* One sphere's Hunt-Crossley contact (lane = sphere s): the force and its
 * moment about the ground origin (CW slot: F3, Mo3, active), and for the
 * implicit step the contact point, the force with the -h Kn v_y term and
 * the 3x3 damping/stiffness block (CJ slot).  Branch-free (selects only), so
 * the muscle lanes can evaluate it inside the muscle block where the
 * scheduler interleaves it with the curve evaluations' dependency chains
 * (contact_store writes it); an inactive sphere's CJ values are unused. */
template <typename Real> struct ContactOut {
    Real cw[7], cj[10];
};
template <bool BFK, class T, typename Real>
DEV void contact_compute(const SModel<T, Real> &SM, const Real *lds, int s, Real h, ContactOut<Real> &o) {
    using LY = Lay<T, Real>;
    using PL = Planar<T>;
    const int cb = SM.sph_cb[s], fo = SM.sph_force[s];
    const Real *kbp = lds + LY::KB + 18 * cb;
    Real kb[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) kb[i] = kbp[i];
    PL::frame(kb);
    Real Cn[3];
    mv3m<PL::ZR, 0>(kb, SM.sph_loc[s], Cn);
#pragma unroll
    for (int i = 0; i < 3; ++i) Cn[i] += kb[9 + i];
    const Real rad = SM.sph_r[s];
    const Real depth = rad - Cn[1];
    const bool pen = depth > 0;
    const Real P[3] = {Cn[0], Cn[1] - (rad - Real(0.5) * depth), Cn[2]};
    Real t[3], vs[3];
    cross3m<PL::ZW, 0>(kb + 12, P, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) vs[i] = kb[15 + i] + t[i];
    PL::lin(vs);
    const Real vn = -vs[1];
    const Real kk = SM.cf_kk[fo], cc = SM.cf_c[fo];
    const Real dps = pen ? depth : Real(1), zero = 0;
    const Real rkd = rad * kk * dps;
    /* ?: arms are plain locals: an expression arm makes clang emit a branch */
    constexpr bool BF = BFK;
    Real fH;
    if constexpr (BF) {
        const Real fHp = Real(4.0 / 3.0) * kk * dps * (rkd * fast_rsqrt(rkd));
        fH = pen ? fHp : zero;
    } else {
        fH = pen ? Real(4.0 / 3.0) * kk * dps * (rkd * fast_rsqrt(rkd)) : Real(0);
    }
    const Real fn = fH * (Real(1) + Real(1.5) * cc * vn);
    const bool active = pen && fn > 0;
    const Real vt0 = -vs[0], vt2 = -vs[2];
    const Real vs2 = vt0 * vt0 + vt2 * vt2;
    Real ivs;
    if constexpr (BF) {
        const Real rvs = fast_rsqrt(vs2);
        ivs = vs2 > 0 ? rvs : zero;
    } else {
        ivs = vs2 > 0 ? fast_rsqrt(vs2) : Real(0);
    }
    const Real vslip = vs2 * ivs;
    const Real vtr = SM.cf_vt[fo], ms = SM.cf_ms[fo], md = SM.cf_md[fo], mv = SM.cf_mv[fo];
    const Real ivtr = fast_rcp(vtr);
    const Real r_ = vslip * ivtr, den = Real(1) + r_ * r_;
    const Real iden = fast_rcp(den);
    const Real ff = fn * (fmin(r_, Real(1)) * (md + Real(2) * (ms - md) * iden) + mv * vslip);
    const bool slip = vslip != 0;
    Real F[3];
    if constexpr (BF) {
        const Real fx = ff * vt0 * ivs, fz = ff * vt2 * ivs;
        F[0] = slip ? fx : zero; F[1] = fn; F[2] = slip ? fz : zero;
    } else {
        F[0] = slip ? ff * vt0 * ivs : Real(0); F[1] = fn; F[2] = slip ? ff * vt2 * ivs : Real(0);
    }
    Real mo[3];
    cross3(P, F, mo);
#pragma unroll
    for (int i = 0; i < 3; ++i) { o.cw[i] = active ? F[i] : Real(0); o.cw[3 + i] = active ? mo[i] : Real(0); }
    o.cw[6] = active ? Real(1) : Real(0);
    const Real kn = Real(1.5) * fH * fast_rcp(dps) * (Real(1) + Real(1.5) * cc * vn);
    /* implicit extra force -h*Kn*v_y (Hertz force at the advanced position) */
#pragma unroll
    for (int i = 0; i < 3; ++i) o.cj[i] = P[i];
    o.cj[3] = F[0];
    o.cj[4] = F[1] - (h > 0 ? h * kn * vs[1] : Real(0));
    o.cj[5] = F[2];
    const Real base = (md + Real(2) * (ms - md) * iden);
    const bool low = r_ < 1;
    Real g_s = low ? base * ivtr + mv : base * ivs + mv;
    Real gp = low ? base * ivtr - Real(4) * (ms - md) * r_ * r_ * (iden * iden * ivtr) + mv
                  : -Real(4) * (ms - md) * r_ * (iden * iden * ivtr) + mv;
    gp = gp < 0 ? Real(0) : gp;
    const Real tx = vslip > 0 ? vt0 * ivs : Real(0), tz = vslip > 0 ? vt2 * ivs : Real(0);
    const Real ctt = h * fn * g_s, cq = h * fn * (gp - g_s);
    const bool imp = h > 0;
    o.cj[6] = imp ? ctt + cq * tx * tx : Real(0);
    o.cj[7] = imp ? cq * tx * tz : Real(0);
    o.cj[8] = imp ? h * Real(1.5) * cc * fH + h * h * kn : Real(0);
    o.cj[9] = imp ? ctt + cq * tz * tz : Real(0);
}
template <class T, typename Real> DEV void contact_store(Real *lds, int s, const ContactOut<Real> &o) {
    using LY = Lay<T, Real>;
    Real *cw = lds + LY::CW + 8 * s, *cj = lds + LY::CJ + LY::CJN * s;
#pragma unroll
    for (int i = 0; i < 7; ++i) cw[i] = o.cw[i];
#pragma unroll
    for (int i = 0; i < 10; ++i) cj[i] = o.cj[i];
}
template <bool BFK, class T, typename Real>
DEV void contact_lane(const SModel<T, Real> &SM, Real *lds, int s, Real h) {
    ContactOut<Real> o;
    contact_compute<BFK, T, Real>(SM, lds, s, h, o);
    contact_store<T, Real>(lds, s, o);
}

/* contact-point Jacobian column of a dof: S.ang x P + S.lin */
template <typename Real> DEV void contact_jac(const Real *Sd, const Real *P, Real *j) {
    cross3(Sd, P, j);
#pragma unroll
    for (int i = 0; i < 3; ++i) j[i] += Sd[3 + i];
}

/* ------------------------------------------------------------ muscles */
template <typename Real> struct MState {
    Real act, lce, vN, vce, Ft, Ff, Fa, dadt, dvdl;
    bool clamped;
};

/* activation rate du/dt = (u - a) / tau, tau = tau_act (0.5 + 1.5 a) or
 * tau_deact / (0.5 + 1.5 a), a the clamped activation (muscle_eval; the
 * cached first substep of CACHE kernels) */
template <bool BF, typename Real> DEV Real act_rate(const SMuscle<Real> &mu, Real a, Real excitation) {
    if constexpr (BF) {
        const Real amin = mu.amin, one = 1;
        Real u = excitation < amin ? amin : (excitation > one ? one : excitation);
        const Real ab = Real(0.5) + Real(1.5) * a;
        const Real da_act = (u - a) * fast_rcp(mu.tau_act * ab), da_deact = (u - a) * ab * fast_rcp(mu.tau_deact);
        return u > a ? da_act : da_deact;
    } else {
        Real u = excitation < mu.amin ? mu.amin : (excitation > Real(1) ? Real(1) : excitation);
        const Real ab = Real(0.5) + Real(1.5) * a;
        return u > a ? (u - a) * fast_rcp(mu.tau_act * ab) : (u - a) * ab * fast_rcp(mu.tau_deact);
    }
}

template <bool BFK, bool BFC, class T, typename Real>
DEV void muscle_eval(const SModel<T, Real> &SM, const SMuscle<Real> &mu, Real a_state, Real l_state, Real excitation,
                     Real L, Real v_warm, MState<Real> &s) {
    STAMP_DECL
    const DCurve<Real> &Cfal = SM.curve[mu.cv[0]], &Cfv = SM.curve[mu.cv[1]], &Cfpe = SM.curve[mu.cv[2]],
                       &Cfse = SM.curve[mu.cv[3]];
    /* ?: arms are plain locals throughout (see below) */
    constexpr bool BF = BFK;
    const Real amin = mu.amin, lmin = mu.lmin, one = 1, zero = 0;
    Real a, lce;
    if constexpr (BF) {
        a = a_state < amin ? amin : (a_state > one ? one : a_state);
        lce = l_state < lmin ? lmin : l_state;
    } else {
        a = a_state < mu.amin ? mu.amin : (a_state > Real(1) ? Real(1) : a_state);
        lce = l_state < mu.lmin ? mu.lmin : l_state;
    }
    Real w = mu.width;
    const Real sq2 = lce * lce - w * w;
    const Real isq = fast_rsqrt(sq2), sq = sq2 * isq;
    const Real icos = lce * isq;          /* 1 / cos(pennation) */
    Real lt = L - sq;
    Real fse, dfse, fal, dfal, fpe, dfpe;
    /* BFC: the three curve chains and the fiber-velocity start and
     * extrapolation in one basic block (every semi-implicit kernel; in the
     * spatial ones only these, the other branch-free forms would spill) */
    curve_eval<BFC>(Cfse, lt * mu.inv_lts, fse, dfse);
    curve_eval<BFC>(Cfal, lce * mu.inv_lopt, fal, dfal);
    curve_eval<BFC>(Cfpe, lce * mu.inv_lopt, fpe, dfpe);
#if BIOIM_SGB == 1
    /* round-5 scheduling experiment: a pipeline that issues
     * the curves' LDS reads in groups ahead of VALU work of this block */
#pragma unroll
    for (int gI = 0; gI < 6; ++gI) {
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);   /* DS reads */
        __builtin_amdgcn_sched_group_barrier(0x2, 12, 0);    /* VALU */
    }
#elif BIOIM_SGB == 2
#pragma unroll
    for (int gI = 0; gI < 24; ++gI) {
        __builtin_amdgcn_sched_group_barrier(0x2, 3, 0);     /* VALU */
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   /* DS read */
    }
#endif
    Real rhs = fse * icos - fpe;
    STAMP(16);
    Real vN, fvv, dfv;
    solve_fv<BFC, !T::PLANAR || BIOIM_FV_PE_PLANAR>(Cfv, a * fal, mu.beta, rhs, v_warm, vN, fvv, dfv);
    STAMP(17);
    Real dGdv = a * fal * dfv + mu.beta;
    /* selects over plain locals (a load in a ?: arm or an if body becomes a
     * branch that splits the muscle eval's basic block) */
    bool clamped;
    if constexpr (BF) {
        const Real fv_at0 = Cfv.y_at0;
        clamped = ((l_state <= lmin) & (vN <= 0)) | (l_state < lmin);
        vN = clamped ? zero : vN;
        fvv = clamped ? fv_at0 : fvv;
    } else {
        clamped = (l_state <= mu.lmin && vN <= 0) || l_state < mu.lmin;
        if (clamped) {
            vN = 0;
            fvv = Cfv.y_at0;
        }
    }
    s.act = a;
    s.lce = lce;
    s.vN = vN;
    s.vce = vN * mu.lv;
    s.Ft = mu.fiso * fse;
    s.Fa = mu.fiso * a * fal * fvv;
    s.Ff = mu.fiso * (a * fal * fvv + fpe + mu.beta * vN);
    s.clamped = clamped;
    Real dGdl = (a * dfal * fvv + dfpe) * mu.inv_lopt + dfse * mu.inv_lts * (icos * icos) + fse * w * w * (isq * isq * isq);
    if constexpr (BF) {
        const Real dvdl = -(dGdl * fast_rcp(dGdv)) * mu.lv;
        s.dvdl = clamped ? zero : dvdl;
    } else {
        s.dvdl = clamped ? Real(0) : -(dGdl * fast_rcp(dGdv)) * mu.lv;
    }
    s.dadt = act_rate<BF>(mu, a, excitation);
    STAMP(18);
}

/* static fiber equilibrium at reset (zero fiber velocity) */
template <bool BFK, class T, typename Real>
DEV Real muscle_equilibrium(const SModel<T, Real> &SM, const SMuscle<Real> &mu, Real a_state, Real L) {
    const DCurve<Real> &Cfal = SM.curve[mu.cv[0]], &Cfpe = SM.curve[mu.cv[2]], &Cfse = SM.curve[mu.cv[3]];
    Real a = a_state < mu.amin ? mu.amin : (a_state > Real(1) ? Real(1) : a_state);
    Real w = mu.width, lo = mu.lmin;
    Real hi = sqrt((L - mu.lts) * (L - mu.lts) + w * w);
    if (!(L - mu.lts > sqrt(lo * lo - w * w))) return lo;
    {   /* the fiber out-pulls the tendon even at its minimum length: no root */
        Real sq = sqrt(lo * lo - w * w), fal, dfal, fpe, dfpe, fse, dfse;
        curve_eval<BFK>(Cfal, lo * mu.inv_lopt, fal, dfal);
        curve_eval<BFK>(Cfpe, lo * mu.inv_lopt, fpe, dfpe);
        curve_eval<BFK>(Cfse, (L - sq) * mu.inv_lts, fse, dfse);
        if ((a * fal + fpe) * (sq / lo) - fse >= 0) return lo;
    }
    Real l = sqrt((L - Real(1.01) * mu.lts) * (L - Real(1.01) * mu.lts) + w * w), dprev = 1;
    if (!(l > lo && l < hi)) l = Real(0.5) * (lo + hi);
    for (int it = 0; it < 4 * Eps<Real>::it_max; ++it) {
        Real sq = sqrt(l * l - w * w), cphi = sq / l;
        Real fal, dfal, fpe, dfpe, fse, dfse;
        curve_eval<BFK>(Cfal, l * mu.inv_lopt, fal, dfal);
        curve_eval<BFK>(Cfpe, l * mu.inv_lopt, fpe, dfpe);
        curve_eval<BFK>(Cfse, (L - sq) * mu.inv_lts, fse, dfse);
        Real H = (a * fal + fpe) * cphi - fse;
        Real dH = (a * dfal + dfpe) * mu.inv_lopt * cphi + (a * fal + fpe) * (w * w) / (l * l * sq) + dfse * mu.inv_lts / cphi;
        if (H > 0) hi = l; else lo = l;
        Real ln = l - H / dH;
        const bool newton = ln >= lo && ln <= hi;
        if (!newton) ln = Real(0.5) * (lo + hi);
        /* the residual stop as a zero step (the l_tol exit below), not an
         * exit of its own: the spatial RK kernels have no register to spare */
        ln = fabs(H) < Eps<Real>::h_stop ? l : ln;
        Real dl = fabs(ln - l);
        l = ln;
        if (dl <= Eps<Real>::l_tol || (it >= 1 && dl <= Real(1e3) * Eps<Real>::l_tol && dl >= Real(0.5) * dprev)) break;
        /* a Newton step of at most l_stop leaves an error ~ |H''/2H'| l_stop^2,
         * far below l_tol (as u_stop for the fiber velocity) */
        if (newton && dl <= Eps<Real>::l_stop) break;
        dprev = dl;
    }
    return l;
}

/* path length and dL/dq of one muscle.  Frames from LDS, Plucker columns
 * from registers (loaded once per dynamics call).  Fixed trip count over
 * the topology's maximum point count; only the point indices that can be
 * conditional / moving (compile-time masks) carry that code. */
/* Path length L and the moment arms dL/dq over the muscle's span (dLs[k]
 * for dof mu.span[k], k < mu.nspan): per active point the
 * change of the unit direction g acts at the point, dL/dq_d += S_d . (P x g, g)
 * for the dofs moving the point, plus g . dP/dq for a moving point's own
 * coordinate.  The floating-base dofs are skipped: their sum over a path is
 * zero (sum g = 0, sum P x g = 0).  The span's Plucker columns are read from
 * LDS once per muscle into registers. */
template <bool BFK, class T, typename Real, int LI = 0>
DEV void muscle_path(const SModel<T, Real> &SM, const SMuscle<Real> &mu, const Real *lds, Real &L,
                     Real (&dLs)[T::MAXSPAN], const LaneIdx<T, Real> *I = nullptr, int jm = 0) {
    using LY = Lay<T, Real>;
    using PL = Planar<T>;
    constexpr unsigned ZR = PL::ZR, ZW = PL::ZW, ZV = PL::ZV;
    constexpr int NSP = T::MAXSPAN;
    constexpr bool BF = BFK;
    const Real *ldsq = lds + LY::QF;
    L = 0;
    int sd[NSP];
    Real Ss[NSP][6];
#pragma unroll
    for (int k = 0; k < NSP; ++k) {
        dLs[k] = 0;
        /* planar: ?: over plain locals only (an arm with a load becomes a
         * branch); the spatial kernels keep the branches (fewer live values
         * in their two muscle passes) */
        int dk;
        if constexpr ((LI & LI_PATH) != 0) {   /* the span's dof from the record (0 past nspan) */
            const uint32_t w = I->path[jm];
            const int spk = (int)li_bits(w, 16 + 4 * k, 4), none = -1;
            const bool ink = k < (int)li_bits(w, 12, 4);
            sd[k] = ink ? spk : none;
            dk = spk;
        } else if constexpr (BF) {
            const int spk = mu.span[k], none = -1, zero = 0;
            const bool ink = k < mu.nspan;
            sd[k] = ink ? spk : none;
            dk = ink ? spk : zero;
        } else {
            sd[k] = k < mu.nspan ? mu.span[k] : -1;
            dk = k < mu.nspan ? mu.span[k] : 0;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) Ss[k][i] = lds[LY::S + 6 * dk + i];
        PL::col(Ss[k]);
    }
    Real Pp[3] = {0, 0, 0}, ep[3] = {0, 0, 0}, dPp[3] = {0, 0, 0};
    uint32_t maskp = 0;
    int mdofp = -1;
    bool have = false;
    auto flush = [&](const Real *g) {
        Real mo[3];
        cross3(Pp, g, mo);
        const Real gd = dot3(g, dPp);
#pragma unroll
        for (int k = 0; k < NSP; ++k) {
            const int d = sd[k];
            const Real on = d >= 0 && ((maskp >> d) & 1u) ? Real(1) : Real(0);
            const Real sm = dot3m<ZW, 0>(Ss[k], mo);
            const Real sg = dot3m<ZV, 0>(Ss[k] + 3, g);
            dLs[k] += on * (sm + sg) + (mdofp == d && d >= 0 ? gd : Real(0));
        }
    };
    /* the muscle's point count and first point (LI_PATH: from the record) */
    auto path_npt = [&]() -> int {
        if constexpr ((LI & LI_PATH) != 0) return (int)li_bits(I->path[jm], 8, 4);
        else return mu.npt;
    };
    auto path_off = [&]() -> int {
        if constexpr ((LI & LI_PATH) != 0) return (int)li_bits(I->path[jm], 0, 8);
        else return mu.pt_off;
    };
    const int npt = path_npt();
    /* point slot j's kind test and the function slot of its axis a, -1: the
     * point's own location (LI_PATH: from the record) */
    auto pt_is = [&](auto kI, const DPathPt<Real> &pt, int j) -> bool {
        constexpr int kind = decltype(kI)::value;
        if constexpr ((LI & LI_PATH) != 0) return ((I->pt[jm][j] >> (kind == BIOIM_PT_COND ? 0 : 6)) & 1u) != 0;
        else return pt.type == kind;
    };
    auto pt_mf = [&](const DPathPt<Real> &pt, int j, int a) -> int {
        if constexpr ((LI & LI_PATH) != 0) {
            const uint32_t fw = li_bits(I->pt[jm][j], 8 + 6 * a, 6);
            return (fw & 32u) ? -1 : (int)fw;
        } else {
            return pt.mf[a];
        }
    };
    constexpr int MP = T::MAXPT > 0 ? T::MAXPT : 1;
    /* every slot's body and activity first (branch-free, slot 0 for slots
     * past the count), so a point's frame loads wait on one LDS round trip
     * inside its branch, not two */
    int cbj[MP];
    bool onj[MP];
    sfor<0, MP>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const DPathPt<Real> &pt = SM.pt[path_off() + (j < npt ? j : 0)];
        if constexpr ((LI & LI_PATH) != 0) cbj[j] = (int)li_bits(I->frame[jm], 4 * j, 4);
        else cbj[j] = pt.cbody;
        onj[j] = j < npt;
        if constexpr (((T::PT_COND >> j) & 1u) != 0) {
            const bool cnd = pt_is(std::integral_constant<int, BIOIM_PT_COND>{}, pt, j);
            if constexpr ((LI & LI_PATH) != 0) {   /* the coordinate from the record (0: not conditional) */
                const Real qc = ldsq[li_bits(I->pt[jm][j], 1, 5)], plo = pt.lo, phi = pt.hi;
                onj[j] = onj[j] & !(cnd & ((qc < plo) | (qc > phi)));
            } else if constexpr (BF) {
                const int ccd = pt.cond_coord, zero = 0;
                const Real qc = ldsq[cnd ? ccd : zero], plo = pt.lo, phi = pt.hi;
                onj[j] = onj[j] & !(cnd & ((qc < plo) | (qc > phi)));   /* no short-circuit branches */
            } else {
                const Real qc = ldsq[cnd ? pt.cond_coord : 0];
                onj[j] = onj[j] && !(cnd && (qc < pt.lo || qc > pt.hi));
            }
        }
    });
    sfor<0, MP>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        {
            const DPathPt<Real> &pt = SM.pt[path_off() + j];
            if (onj[j]) {
                Real loc[3] = {pt.loc[0], pt.loc[1], pt.loc[2]}, dloc[3] = {0, 0, 0};
                if constexpr (((T::PT_MOVING >> j) & 1u) != 0) {
                    if (pt_is(std::integral_constant<int, BIOIM_PT_MOVING>{}, pt, j)) {
                        Real ll[3], dl[3] = {0, 0, 0};
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const int f = pt_mf(pt, j, a);
                            if constexpr (BF) {
                                const Real l0 = pt.loc[a], fv = lds[LY::MF + 3 * (f < 0 ? 0 : f)],
                                           fd = lds[LY::MF + 3 * (f < 0 ? 0 : f) + 1], zero = 0;
                                ll[a] = f < 0 ? l0 : fv;
                                dl[a] = f < 0 ? zero : fd;
                            } else {
                                ll[a] = f < 0 ? pt.loc[a] : lds[LY::MF + 3 * (f < 0 ? 0 : f)];
                                dl[a] = f < 0 ? Real(0) : lds[LY::MF + 3 * (f < 0 ? 0 : f) + 1];
                            }
                        }
                        mv3(pt.R, ll, loc);
#pragma unroll
                        for (int i = 0; i < 3; ++i) loc[i] += pt.p[i];
                        mv3(pt.R, dl, dloc);
                    }
                }
                const Real *kbp = lds + LY::KB + 18 * cbj[j];
                Real Rb[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) Rb[i] = kbp[i];
                PL::rot(Rb);
                Real P[3], dP[3];
                mv3m<ZR, 0>(Rb, loc, P);
#pragma unroll
                for (int i = 0; i < 3; ++i) P[i] += Rb[9 + i];
                mv3m<ZR, 0>(Rb, dloc, dP);
                Real e[3] = {0, 0, 0};
                if (have) {
                    Real sgm[3] = {P[0] - Pp[0], P[1] - Pp[1], P[2] - Pp[2]};
                    const Real l2 = dot3(sgm, sgm);
                    const Real inv = fast_rsqrt(l2), len = l2 * inv;
                    L += len;
#pragma unroll
                    for (int a = 0; a < 3; ++a) e[a] = sgm[a] * inv;
                    Real g[3] = {ep[0] - e[0], ep[1] - e[1], ep[2] - e[2]};
                    flush(g);
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) { ep[a] = e[a]; Pp[a] = P[a]; dPp[a] = dP[a]; }
                maskp = pt.dofmask;
                mdofp = pt.mdof;
                have = true;
            }
        }
    });
    if (have) flush(ep);
}

/* ------------------------------------------------------------ dynamics */
template <class T, typename Real> struct Dyn {
    static constexpr int MPL = Lay<T, Real>::MPL;
    Real qdd;        /* this lane's dof (lane < ND): generalized acceleration / substep increment */
    MState<Real> ms[MPL]; /* this lane's muscles m = lane + j*G */
    Real act[MPL], lce[MPL]; /* their state used (after a reset equilibrium) */
    Real x0;         /* floating origin used for the published frames */
    bool ok;
};

/* apply_perturbations table (see LaunchArgs) as seen by one env */
template <typename Real> struct PertArgs {
    const double *x;
    const Real *y;   /* [n][N] */
    int n, ob, env, N;
};

/* bioim_set_external_forces as the EXT kernels take it (a launch argument of
 * its own, so LaunchArgs and with it every other kernel stay as they are):
 * rows — the caller's [N][k][9]; inside env_block, one env's k rows (its
 * staged LDS slot, or its rows of the caller's buffer where ExtLay::LDS is
 * false).  body: slot j's OpenSim body in bits [8j, 8j + 8); ground: bit j set
 * for a ground-frame point.  Wave-uniform, read with shifts (no indexed
 * argument array). */
template <typename Real> struct ExtArgs {
    const Real *rows;
    int k;
    uint32_t ground;
    uint64_t body;
};

/* The env's external wrenches on composite body `lane` (its own lane, after
 * body_inertia stored WB): per slot of an OpenSim body of this composite body,
 * in slot order, the force, its moment about the kernel's frame origin (the
 * floating origin x0 on the ground x axis) and the torque, subtracted from
 * the body's Newton-Euler wrench like the push.  A body-frame point goes
 * through the OpenSim body's frame in the composite body (os_p, os_R), a
 * ground-frame point is shifted by x0. */
template <class T, typename Real>
DEV void ext_apply(const DModel<Real> &M, const SModel<T, Real> &SM, const ExtArgs<Real> &X, Real *lds, int lane, Real x0) {
    using LY = Lay<T, Real>;
    const Real *kb = lds + LY::KB + 18 * lane;
    Real *wb = lds + LY::WB + 6 * lane;
#pragma unroll 1
    for (int j = 0; j < X.k; ++j) {
        const int ob = (int)((X.body >> (8 * j)) & 0xFFu);
        if (lane != SM.os_cb[ob]) continue;
        const Real *row = X.rows + EXT_ROW * j;
        const Real f[3] = {row[0], row[1], row[2]}, pt[3] = {row[3], row[4], row[5]};
        Real r[3], m[3];
        if ((X.ground >> j) & 1u) {
            r[0] = pt[0] - x0; r[1] = pt[1]; r[2] = pt[2];
        } else {
            Real pl[3], pc[3];
            mv3(M.os_R[ob], pt, pl);
#pragma unroll
            for (int i = 0; i < 3; ++i) pc[i] = SM.os_p[ob][i] + pl[i];
            mv3(kb, pc, r);
#pragma unroll
            for (int i = 0; i < 3; ++i) r[i] += kb[9 + i];
        }
        cross3(r, f, m);
#pragma unroll
        for (int i = 0; i < 3; ++i) { wb[i] -= m[i] + row[6 + i]; wb[3 + i] -= f[i]; }
    }
}

/* Force of the env's zero-order-hold table at the call time t0 + k*dt (the
 * slot's base and step, written by lane 0 before the call); the segment
 * cursor [lo, hi) and its value live in the slot, so a binary search over
 * the table runs only when the time leaves the segment. */
template <typename Real>
DEV Real pert_force(const PertArgs<Real> &P, double *sl, int k) {
    const double tc = sl[0] + (double)k * sl[1];
    if (!(tc >= sl[2] && tc < sl[3])) {
        int lo = -1, hi = P.n;               /* x[lo] <= tc < x[hi] */
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (P.x[mid] <= tc) lo = mid; else hi = mid;
        }
        sl[2] = lo >= 0 ? P.x[lo] : -INFINITY;
        sl[3] = hi < P.n ? P.x[hi] : INFINITY;
        sl[4] = (double)GAT(P.y, (size_t)(lo >= 0 ? lo : 0) * P.N + P.env, (size_t)P.n * P.N);
    }
    return (Real)sl[4];
}

/* Forward dynamics at (q, u, this lane's muscle states) with held controls.
 * Lane d < ND owns dof d (qd, ud in, D.qdd out); lane's j-th muscle is
 * m = lane + j*G.  h > 0: increment of the linearly-implicit substep;
 * h == 0: the true accelerations (realize).  Leaves coordinates, frames,
 * contact wrenches, limit forces and q'' (RHS slots) published in LDS.
 * CACHE kernels (CacheLay): CI.make — a realize also forms the implicit
 * system at h = CI.hc and stores it with the fiber-velocity roots into the
 * env's cache row (CI.row()); CI.use — a first substep takes its system and
 * roots from the cache (CI.sys / CI.mus loaded at kernel start in the
 * planar kernels, the row itself in the spatial ones) and only solves: the
 * state is the one the last realize ran at. */
template <class T, typename Real> struct CacheIO {
    static constexpr int PF = CacheLay<T>::PF > 0 ? CacheLay<T>::PF : 1;
    static constexpr int PFA = CacheLay<T>::PREFETCH ? PF : 1, MPA = CacheLay<T>::PREFETCH ? Lay<T, Real>::MPL : 1;
    bool use = false, make = false;
    Real hc = 0;
    /* this env's row, formed at each use from the uniform base and an opaque
     * copy of the env index: a row address kept live through the kernel was
     * split by the register allocator into lane-divergent AGPR copies in the
     * fused C5 kernel (tools/hazard_gate.py) */
    Real *base = nullptr;
    int env = 0, N = 0;
    DEV Real *row() const {
        int e = env;
        asm volatile("" : "+v"(e));
        return base + GIDX((size_t)e * CacheLay<T>::DIM, (size_t)N * CacheLay<T>::DIM);
    }
    Real sys[PFA];     /* PREFETCH: the row's system values k = lane + i G */
    Real mus[MPA][3];  /* PREFETCH: this lane's muscles' root, dv/dl, clamp flag */
};

/* Which device functions take their branch-free forms (selects over plain
 * locals, blended extrapolations, one basic block per muscle eval) in topology
 * T's kernels.  IMP: a semi-implicit kernel; the analysis kernels take the
 * semi-implicit step's switches (the default).
 * BFK: all of them in the planar kernels, except the torque-model RK ones: an
 * RK build of these forms put a lane-divergent copy of a live-in-all-lanes
 * address into an AGPR in the Torque2D RK kernel and faulted;
 * that kernel keeps the GPU-verified code (round 4: the same forms there again
 * give 4 flagged copies in tools/hazard_gate.py), and the gate checks the others.
 * BF3: per piece in the spatial semi-implicit kernels (BIOIM_BF3 bits:
 * 1 function slots, 2 muscle paths, 4 contact, 8 limits, 16 fiber equilibrium,
 * 32 phase-3 rows, 64 implicit terms without a branch on h, 128 muscle eval) */
template <class T, bool IMP = true> struct BfSwitch {
    static constexpr bool BFK = (T::PLANAR || BIOIM_BF_SPATIAL) && (IMP || T::NM > 0);
    static constexpr bool BF3 = !T::PLANAR && (IMP || BIOIM_BF3_RK);
    static constexpr bool FN = BFK || (BF3 && (BIOIM_BF3 & 1)), PATH = BFK || (BF3 && (BIOIM_BF3 & 2));
    static constexpr bool CON = BFK || (BF3 && (BIOIM_BF3 & 4)), LIM = BFK || (BF3 && (BIOIM_BF3 & 8));
    static constexpr bool EQ = BFK || (BF3 && (BIOIM_BF3 & 16)), ROW = BFK || (BF3 && (BIOIM_BF3 & 32));
    static constexpr bool ME = BFK || (BF3 && (BIOIM_BF3 & 128));
};

/* The step-tail switch of one kernel family (BIOIM_GROUND_ONCE's bits) */
template <class T, bool FUSED = false, bool RK = false> struct TailSwitch {
    static constexpr int BIT = FUSED ? 4 : (T::PLANAR ? 1 : 2);
    static constexpr bool GROUND = (BIOIM_GROUND_ONCE & BIT) != 0;
    /* the family's BIOIM_FRONTEND byte (FE_* bits) */
    static constexpr int FE = (BIOIM_FRONTEND >> (FUSED ? 16 : (T::PLANAR ? 0 : 8))) & 0xFF;
    /* the family's BIOIM_LANEIDX byte (LI_* bits); none in the RK kernels:
     * LI_TAU put two flagged copies (tools/hazard_gate.py) into the Torque2D
     * push + RK kernel, the one DESIGN.md 5.5 is about, so the reference
     * integrator's kernels keep the parent's code */
    static constexpr int LI = RK ? 0 : (BIOIM_LANEIDX >> (FUSED ? 16 : (T::PLANAR ? 0 : 8))) & 0xFF;
};
template <class T, typename Real, bool PERT, bool BF_ROWS, bool IMP, bool CACHE = false, class TS = TailSwitch<T>, bool EXT = false>
DEV void dynamics(const DModel<Real> &M, const SModel<T, Real> &SM, Real qd, Real ud,
                  const Real (&act)[Lay<T, Real>::MPL], const Real (&lce)[Lay<T, Real>::MPL],
                  const Real (&control)[Lay<T, Real>::MPL], int lane, Real *lds, Real h, bool equilibrate,
                  const PertArgs<Real> &P, double *pslot, int pk, Dyn<T, Real> &D, const CacheIO<T, Real> &CI,
                  const LaneIdx<T, Real> &LXL, const ExtArgs<Real> &X = ExtArgs<Real>{}) {
    using LY = Lay<T, Real>;
    constexpr int ND = LY::ND, NP = LY::NP, NB = T::NB, G = T::G, MPL = LY::MPL;
    constexpr int LI = TS::LI;   /* the family's BIOIM_LANEIDX byte: LX's fields in use */
    const LaneIdx<T, Real> LX = LI != 0 ? LXL.template call_copy<LI>() : LXL;
    static_assert(!CACHE || (CacheLay<T>::ON && IMP && !PERT && !EXT), "the realize cache: the default (semi-implicit, no push, no external forces) step kernels");
    static_assert(NB < G && ND <= G, "lane NB writes the ground slot; one lane per dof");
    /* the semi-implicit planar kernels: the implicit contact / limit terms
     * without a branch on h (the spatial kernels keep it: register budget) */
    constexpr bool IMP_BF = IMP && (T::PLANAR || BIOIM_BF_SPATIAL || ((BIOIM_BF3 & 64) && !PERT));
    using SW = BfSwitch<T, IMP>;
    /* the muscle eval's curves and fiber-velocity solve in one block, in
     * every kernel (spatial too: no scratch; same-box 3D -1.6 %,
     * profiles/r03/r03k, r03l) */
    constexpr bool BFC = true;
    /* LX's fields instead of the model image's tables (constant conditions:
     * with a bit off the expression is the table read alone) */
    constexpr bool LCOLS = (LI & LI_COLS) != 0, LTAU = (LI & LI_TAU) != 0;
    STAMP_DECL
    if (CACHE && CI.use) {
        /* the first substep of a launch from the last realize's cache: the
         * implicit system at this h into MP..RHS, the muscles' roots, and the
         * activation rates at this step's excitations */
        using CL = CacheLay<T>;
        Real *const crow = CL::PREFETCH ? nullptr : CI.row();
#pragma unroll
        for (int i = 0; i < CacheIO<T, Real>::PF; ++i)
            if (lane + i * G < CL::SYS) {
                if constexpr (CL::PREFETCH) lds[LY::MP + lane + i * G] = CI.sys[i];
                else lds[LY::MP + lane + i * G] = GAT(crow, lane + i * G, CL::DIM);
            }
        if constexpr (T::NM > 0) {
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
                if (m < T::NM) {
                    const SMuscle<Real> &mu = SM.mus[m];
                    const Real amin = mu.amin, one = 1, a_state = act[j];
                    const Real a = a_state < amin ? amin : (a_state > one ? one : a_state);
                    MState<Real> &s = D.ms[j];
                    Real cv[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if constexpr (CL::PREFETCH) cv[c] = CI.mus[j][c];
                        else cv[c] = GAT(crow, CL::MUS + 3 * m + c, CL::DIM);
                    }
                    s.vN = cv[0];
                    s.vce = s.vN * mu.lv;
                    s.dvdl = cv[1];
                    s.clamped = cv[2] != Real(0);
                    s.dadt = act_rate<SW::ME>(mu, a, control[j]);
                }
            }
        } else {
            /* this step's actuator torques (as phase 2 stores them), added
             * to the cached right-hand side in phase 3's order */
            if (lane == 0) lds[LY::TAU + LY::TZ] = Real(0);
            sfor<0, MPL>([&](auto jI) {
                constexpr int j = decltype(jI)::value;
                const int m = mslot<T>(lane + j * G);
                if (m < T::NA) lds[LY::TAU + (lane + j * G) * T::MAXSPAN] = control[j] * SM.ca_opt[m];
            });
            wave_sync();
            if (lane < ND) {
                Real r = lds[LY::RHS + lane];
#pragma unroll
                for (int i = 0; i < T::MAXARM; ++i) r += lds[LY::TAU + (LTAU ? LX.tau_src(i) : SM.tau_src[lane][i])];
                lds[LY::RHS + lane] = r;
            }
        }
        wave_sync();
    } else {
    constexpr int FE = TS::FE;
    publish_coords<T, Real>(M, SM, lds, lane, qd, ud);
    if constexpr (!(FE & FE_COLS)) {   /* FE_COLS: kin_local stores every dof's SL row whole */
        if (lane < ND) {
#pragma unroll
            for (int i = 0; i < 6; ++i) lds[LY::SL + 6 * lane + i] = 0;
        }
    }
    wave_sync();
    Real x0 = 0;
    if constexpr (T::TX >= 0) {
        if constexpr (T::coord_dof[T::TX] >= 0) x0 = M.float_origin ? lds[LY::QF + T::TX] : Real(0);
    }
    D.x0 = x0;

    /* ---- phase 0b: function slots, one lane each — the moving path points'
     * location functions (read by every muscle that has the point) and the
     * joints' spline axes (read by their body's lane) */
    fn_slots<SW::FN, T, Real>(SM, lds, lane);
    STAMP(15);

    /* ---- phase 1: lane-parallel kinematics */
    if (lane < NB) kin_local<T, Real, FE>(SM, lds, lane);
    if (lane == NB) kin_ground<T, Real, TS::GROUND>(lds, x0);
    wave_sync();
    STAMP(0);
    /* apply_perturbations: ground-frame force (fx, 0, 0) at the origin of
     * OpenSim body P.ob (the torso), muscle_walking_imitation_env2D.py:83-100
     * (the body's own lane: it reads back the frame and wrench it stored) */
    auto push = [&]() {
        if (PERT && lane == SM.os_cb[P.ob]) {
            const Real fpx = pert_force<Real>(P, pslot, pk);
            const Real *kb = lds + LY::KB + 18 * lane;
            Real p[3];
            mv3(kb, SM.os_p[P.ob], p);
            Real *wb = lds + LY::WB + 6 * lane;
            wb[1] -= (p[2] + kb[11]) * fpx;
            wb[2] += (p[1] + kb[10]) * fpx;
            wb[3] -= fpx;
        }
        /* bioim_set_external_forces: the env's held wrenches, same place */
        if constexpr (EXT) ext_apply<T, Real>(M, SM, X, lds, lane, x0);
    };
    if constexpr ((FE & FE_INERTIA) != 0) {
        /* the body lane goes from its chain to its inertia and wrench with the
         * frame in registers; the columns (which read the parents' frames)
         * then run with the subtree sums' reads below, after one sync */
        if (lane < NB) {
            Frame<Real> F;
            kin_chain<T, Real, FE>(SM, lds, lane, x0, F);
            body_inertia<T, Real, true>(SM, M, lds, lane, &F);
            push();
        }
        wave_sync();
        STAMP(1);
        if (lane < ND) kin_column<T, Real, LI>(SM, lds, lane, &LX);
    } else {
        if (lane < NB) {
            Frame<Real> F;
            kin_chain<T, Real, FE>(SM, lds, lane, x0, F);
        }
        wave_sync();
        STAMP(1);
        if (lane < ND) kin_column<T, Real, LI>(SM, lds, lane, &LX);
        if (lane < NB) {
            body_inertia<T, Real>(SM, M, lds, lane);
            push();
        }
        wave_sync();
    }
    STAMP(2);

    /* ---- phase 2: lane-parallel force elements */
    {   /* subtree sums of inertia and wrench, in place (all reads, then all
         * writes).  Planar models: only the components phase 3 reads against
         * planar columns (m, h_x, h_y, J_zz; n_z, f_x, f_y) */
        constexpr unsigned ICU = T::PLANAR ? 0x47u : 0x3FFu, WBU = T::PLANAR ? 0x1Cu : 0x3Fu;
        Real ic[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, wb[6] = {0, 0, 0, 0, 0, 0};
        if (lane < NB) {
            /* planar: every body's record is read and weighted by 0 / 1 (lane
             * an ancestor of d, or d): one basic block, the loads batch */
            sfor<0, NB>([&](auto dI) {
                constexpr int d = decltype(dI)::value;
                const bool mine = (T::anc[d] >> lane) & 1u;
                if (T::PLANAR || mine) {
                    const Real on = !T::PLANAR || mine ? Real(1) : Real(0);
#pragma unroll
                    for (int i = 0; i < 10; ++i)
                        if ((ICU >> i) & 1u) ic[i] = fma(on, lds[LY::IC + 10 * d + i], ic[i]);
#pragma unroll
                    for (int i = 0; i < 6; ++i)
                        if ((WBU >> i) & 1u) wb[i] = fma(on, lds[LY::WB + 6 * d + i], wb[i]);
                }
            });
        }
        wave_sync();
        if (lane < NB) {
#pragma unroll
            for (int i = 0; i < 10; ++i)
                if ((ICU >> i) & 1u) lds[LY::IC + 10 * lane + i] = ic[i];
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if ((WBU >> i) & 1u) lds[LY::WB + 6 * lane + i] = wb[i];
        }
    }
    STAMP(3);
    /* the implicit terms' h: a CACHE realize forms them at the next step's
     * substep length (its explicit q'' below does not use them) */
    const Real hi = (CACHE && CI.make) ? CI.hc : h;
    /* contacts computed by the first muscle pass when every sphere lane
     * holds a muscle there */
    constexpr bool MUSCLE_CONTACT = T::NM >= T::NS && T::NS > 0;
    ContactOut<Real> CO;
    if constexpr (T::NM > 0) {
        /* this lane's muscles' -F_t dL/dq over their spans, stored per muscle
         * slot and span entry (plain stores); the dof lanes gather them in
         * phase 3 through SM.tau_src.  (An LDS read-modify-write of per-lane
         * torque slots at the span's runtime dof indices, combined with the
         * early deque store, produced wrong fp32 3D results on the GPU —
         * DESIGN.md 5.1.) */
        if (lane == 0) lds[LY::TAU + LY::TZ] = Real(0);
        sfor<0, MPL>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            const int m = mslot<T>(lane + j * G);
            if (m < T::NM) {
                const SMuscle<Real> &mu = SM.mus[m];
                Real L, dLs[T::MAXSPAN];
                muscle_path<SW::PATH, T, Real, LI>(SM, mu, lds, L, dLs, &LX, j);
                STAMP(4);
                Real a_ = act[j], l_ = lce[j];
                if (equilibrate) /* equilibrateMuscles: static fiber equilibrium at the held activation
                                  * (a reset has set the default activation) */
                    l_ = muscle_equilibrium<SW::EQ, T, Real>(SM, mu, a_, L);
                D.act[j] = a_;
                D.lce[j] = l_;
                /* the sphere contacts ride in the first muscle pass (every
                 * sphere lane holds a muscle): same block as the curve
                 * evaluations, so their chains interleave */
                if constexpr (j == 0 && MUSCLE_CONTACT) contact_compute<SW::CON, T, Real>(SM, lds, lane < T::NS ? lane : 0, hi, CO);
                muscle_eval<SW::ME, BFC, T, Real>(SM, mu, a_, l_, control[j], L, D.ms[j].vN, D.ms[j]);
                const Real nFt = -D.ms[j].Ft;
                Real *ts = lds + LY::TAU + (lane + j * G) * T::MAXSPAN;
#pragma unroll
                for (int k = 0; k < T::MAXSPAN; ++k) ts[k] = nFt * dLs[k];
            }
        });
    } else {
        /* coordinate actuators: one torque per slot, gathered the same way */
        if (lane == 0) lds[LY::TAU + LY::TZ] = Real(0);
        sfor<0, MPL>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            const int m = mslot<T>(lane + j * G);
            if (m < T::NA) lds[LY::TAU + (lane + j * G) * T::MAXSPAN] = control[j] * SM.ca_opt[m];
        });
    }
    STAMP(5);
    if constexpr (MUSCLE_CONTACT) {
        if (lane < T::NS) contact_store<T, Real>(lds, lane, CO);
    } else {
        if (lane < T::NS) contact_lane<SW::CON, T, Real>(SM, lds, lane, hi);
    }
    STAMP(6);
    if (lane < T::NL) {
        int cc = LTAU ? LX.lim_coord() : SM.lim_coord[lane];
        Real qv = lds[LY::QF + cc], qd = lds[LY::UF + cc];
        Real qup = SM.lim_qup[lane], qlo = SM.lim_qlow[lane], tr = SM.lim_trans[lane], itr = SM.lim_itrans[lane];
        Real up = smooth_step<SW::LIM>(Real(0), Real(1), qup, qup + tr, itr, qv);
        Real lo = smooth_step<SW::LIM>(Real(1), Real(0), qlo - tr, qlo, itr, qv);
        Real f = -SM.lim_kup[lane] * up * (qv - qup) + SM.lim_klow[lane] * lo * (qlo - qv) - SM.lim_damp[lane] * (up + lo) * qd;
        Real diag = 0, tadd = f;
        if (IMP_BF || (!IMP_BF && hi > 0)) {   /* IMP_BF: no branch on h (at h = 0 this gives diag = 0, tadd = f) */
            Real dup = smooth_step_d<SW::LIM>(Real(0), Real(1), qup, qup + tr, itr, qv);
            Real dlo = smooth_step_d<SW::LIM>(Real(1), Real(0), qlo - tr, qlo, itr, qv);
            Real kq = SM.lim_kup[lane] * (up + dup * (qv - qup)) + SM.lim_klow[lane] * (lo - dlo * (qlo - qv));
            Real cq = SM.lim_damp[lane] * (up + lo);
            diag = hi * cq + hi * hi * kq;
            tadd = f - hi * kq * qd;
        }
        Real *lm = lds + LY::LIM + 4 * lane;
        lm[0] = f; lm[1] = diag; lm[2] = tadd;
    }
    wave_sync();
    STAMP(7);

    /* ---- phase 3 (lane = dof k): right-hand side and row k of the packed
     * lower M, fixed-order sums.
     * rhs_k = -S_k.WB + muscle/actuator torques + contact J_k(s).F_s + limits.
     * Row k holds the entries (k, l) for the dofs l on k's root path (l = k
     * included; the others are structural zeros, never read by ltl_solve):
     * M_kl = S_l . I^c S_k, the composite inertia of k's body times k's
     * column (CRBA).  The implicit contact block of an entry is
     * J_l(s)^T C_s J_k(s) over the spheres s below k; with
     * J_l(s)^T w = S_l . (P_s x w, w) it folds into the same vector:
     * G_k = I^c S_k + sum_s (P_s x w_s, w_s), w_s = C_s J_k(s), and
     * M_kl = S_l . G_k (every l on k's path moves the spheres k moves).  All
     * inputs (S, IC, CJ, LIM) were published before the last sync, so the
     * row needs no exchange between lanes. */
    const bool implicit = hi > 0;
    using PL = Planar<T>;
    constexpr unsigned ZW = PL::ZW, ZV = PL::ZV;
    /* EX: the explicit system of a CACHE realize (h = 0: the contact force
     * without its implicit correction — the CW slot — the limit forces, no
     * implicit blocks), after its implicit one went to the cache; otherwise
     * the system at hi */
    auto phase3 = [&](auto EXc) {
    constexpr bool EX = decltype(EXc)::value;
    if (lane < ND) {
        Real Sd[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) Sd[i] = lds[LY::S + 6 * lane + i];
        PL::col(Sd);
        const Real *wb = lds + LY::WB + 6 * (LCOLS ? LX.body() : SM.dof_cb[lane]);
        Real r = -(dot3m<ZW, 0>(Sd, wb) + dot3m<ZV, 0>(Sd + 3, wb + 3));
        /* torque models with the realize cache: the actuator torques last
         * (the cache keeps the sum before them) */
        constexpr bool TAU_LAST = CACHE && T::NM == 0;
        if constexpr (!TAU_LAST) {
#pragma unroll
            for (int i = 0; i < T::MAXARM; ++i) r += lds[LY::TAU + (LTAU ? LX.tau_src(i) : SM.tau_src[lane][i])];
        }
        Real Gk[6];
        {
            const Real *ic = lds + LY::IC + 10 * (LCOLS ? LX.body() : SM.dof_cb[lane]);
            Real t[3];
            symvm<ZW>(ic + 4, Sd, Gk);
            cross3m<0, ZV>(ic + 1, Sd + 3, t);
#pragma unroll
            for (int i = 0; i < 3; ++i) Gk[i] += t[i];
            cross3m<ZW, 0>(Sd, ic + 1, t);
#pragma unroll
            for (int i = 0; i < 3; ++i) Gk[3 + i] = ic[0] * Sd[3 + i] + t[i];
        }
        sfor<0, T::NS>([&](auto sI) {
            constexpr int sp = decltype(sI)::value;
            constexpr unsigned msk = T::dofmask[T::sphere_cb[sp]];
            const Real *cj = lds + LY::CJ + LY::CJN * sp, *C = cj + 6;
            /* the force: CW (= F where the sphere is active, 0 elsewhere, so
             * on * F alike) for the explicit system */
            const Real *Fs = EX ? lds + LY::CW + 8 * sp : cj + 3;
            Real jd[3];
            cross3m<ZW, 0>(Sd, cj, jd);
#pragma unroll
            for (int i = 0; i < 3; ++i) jd[i] += Sd[3 + i];
            PL::lin(jd);
            /* weighted by on = 0 / 1 (every CJ value is finite: contact_compute
             * is branch-free): a select made the compiler load cj under a
             * branch, two basic blocks per sphere */
            const bool onb = lds[LY::CW + 8 * sp + 6] > 0 && ((msk >> lane) & 1u);
            const Real on = onb ? Real(1) : Real(0);
            if constexpr (SW::ROW) r = fma(on, dot3m<ZV, 0>(jd, Fs), r);
            else r += onb ? dot3m<ZV, 0>(jd, Fs) : Real(0);
            /* IMP (the semi-implicit kernels): no branch on h — a realize
             * call (h = 0) has C = 0 (contact_compute), adding zeros */
            if (!EX && (IMP_BF || (!IMP_BF && implicit))) {
                Real w[3] = {(ZV & 4u) ? C[0] * jd[0] : C[0] * jd[0] + C[1] * jd[2], C[2] * jd[1],
                             C[1] * jd[0] + C[3] * jd[2]};
                Real pw[3];
                cross3(cj, w, pw);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if constexpr (SW::ROW) {
                        Gk[i] = fma(on, pw[i], Gk[i]);
                        Gk[3 + i] = fma(on, w[i], Gk[3 + i]);
                    } else {
                        Gk[i] += onb ? pw[i] : Real(0);
                        Gk[3 + i] += onb ? w[i] : Real(0);
                    }
                }
            }
        });
        Real dg = 0;
#pragma unroll
        for (int li = 0; li < T::NL; ++li) {   /* selects: no per-limit branch */
            const bool mine = LTAU ? LX.lim_mine(li) : SM.lim_dof[li] == lane;
            r += mine ? lds[LY::LIM + 4 * li + (EX ? 0 : 2)] : Real(0);
            if constexpr (!EX) dg += mine ? lds[LY::LIM + 4 * li + 1] : Real(0);
        }
        if constexpr (TAU_LAST) {
            Real rt = r;
#pragma unroll
            for (int i = 0; i < T::MAXARM; ++i) rt += lds[LY::TAU + (LTAU ? LX.tau_src(i) : SM.tau_src[lane][i])];
            lds[LY::RHS + lane] = (!EX && CI.make) ? r : rt;   /* the cache's rhs: without the controls */
        } else {
            lds[LY::RHS + lane] = r;
        }
        /* Row k's entries (k, l), l <= k.  BF_ROWS: branch-free, every l is
         * computed and stored in row k's own slots (those off k's root path
         * are structural zeros ltl_solve never reads); columns l > k (not in
         * row k) go to slot (k, 0) first, descending l, so the true (k, 0) —
         * dof 0 is every dof's ancestor — is written last.  Same-box 2D
         * 0.329 -> 0.316 ms, 3D 0.581 -> 0.561 (profiles/r03/ab_rows.txt).
         * Otherwise only k's path entries, each under its own branch. */
        static_assert(DofTree<T>::root_common(), "row stores park columns l > k in slot (k, 0)");
        Real *row = lds + LY::MP + (lane * (lane + 1)) / 2;
        unsigned path = 0;   /* dofs on k's root path, k included (compile-time per dof, selected by lane) */
        if constexpr (!BF_ROWS) {
            sfor<0, ND>([&](auto kI) {
                constexpr int k = decltype(kI)::value;
                constexpr unsigned pm = DofTree<T>::path_mask(k);
                path = lane == k ? pm : path;
            });
        }
        sfor<0, ND>([&](auto lI) {
            constexpr int l = ND - 1 - decltype(lI)::value;
            auto entry = [&]() {
                Real Sl[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) Sl[i] = lds[LY::S + 6 * l + i];
                PL::col(Sl);
                Real v = dot3m<ZW, 0>(Sl, Gk) + dot3m<ZV, 0>(Sl + 3, Gk + 3);
                return EX ? v : v + (implicit && l == lane ? dg : Real(0));
            };
            if constexpr (BF_ROWS) row[l <= lane ? l : 0] = entry();
            else if ((path >> l) & 1u) row[l] = entry();
        });
    }
    };
    phase3(std::integral_constant<bool, false>{});
    wave_sync();
    if constexpr (CACHE) {
        if (CI.make) {
            /* the implicit system at hi for the next launch's first substep, then
             * this realize's explicit one over it */
            using CL = CacheLay<T>;
            Real *const crow = CI.row();
            for (int k = lane; k < CL::SYS; k += G) GAT(crow, k, CL::DIM) = lds[LY::MP + k];
            if (lane == 0) GAT(crow, CL::H, CL::DIM) = hi;
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
                if (m < T::NM) {
                    GAT(crow, CL::MUS + 3 * m, CL::DIM) = D.ms[j].vN;
                    GAT(crow, CL::MUS + 3 * m + 1, CL::DIM) = D.ms[j].dvdl;
                    GAT(crow, CL::MUS + 3 * m + 2, CL::DIM) = D.ms[j].clamped ? Real(1) : Real(0);
                }
            }
            wave_sync();
            phase3(std::integral_constant<bool, true>{});
            wave_sync();
        }
    }
    }   /* phases 0-3 (not a cached first substep) */
    STAMP(8);

    /* ---- phase 4: tree-sparse LTL solve (ltl_solve), redundant in every
     * lane's registers (the shortest dependency chain for these 9x9 / 14x14
     * systems; a lane-distributed dense factorization with one LDS round trip
     * per column measured 7 % slower per step); lane d keeps q''_d and
     * publishes it for the report */
    Real A[NP], xs[ND];
#pragma unroll
    for (int e = 0; e < NP; ++e) A[e] = lds[LY::MP + e];
#pragma unroll
    for (int d = 0; d < ND; ++d) xs[d] = lds[LY::RHS + d];
    D.ok = ltl_solve<T, ND, Real>(A, xs);
    Real x = 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) x = lane == d ? xs[d] : x;
    D.qdd = x;
    wave_sync();
    if (lane < ND) lds[LY::RHS + lane] = x;   /* q'' of every dof for the report */
    wave_sync();
    STAMP(9);
}

/* Lane-parallel report (lane = OpenSim body b < NOS; lane NOS = system
 * COM): origin position and velocity in absolute ground coordinates, from
 * the published frames, into REP[b] */
template <class T, typename Real>
DEV void report_points(const SModel<T, Real> &SM, Real *lds, int lane, Real x0) {
    using LY = Lay<T, Real>;
    static_assert(T::NOS < T::G, "one lane per reported body plus one for the COM");
    Real pos[3], vel[3], t[3];
    if (lane < T::NOS) {
        const Real *kb = lds + LY::KB + 18 * SM.os_cb[lane];
        mv3(kb, SM.os_p[lane], pos);
#pragma unroll
        for (int i = 0; i < 3; ++i) pos[i] += kb[9 + i];
        cross3(kb + 12, pos, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) vel[i] = kb[15 + i] + t[i];
    } else {
        Real mt = 0, cs[3] = {0, 0, 0}, vs[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < T::NB; ++c) {
            const Real *kb = lds + LY::KB + 18 * c;
            Real cG[3], vc[3];
            mv3(kb, SM.body[c].com, cG);
#pragma unroll
            for (int i = 0; i < 3; ++i) cG[i] += kb[9 + i];
            cross3(kb + 12, cG, t);
#pragma unroll
            for (int i = 0; i < 3; ++i) vc[i] = kb[15 + i] + t[i];
            Real m = SM.body[c].mass;
#pragma unroll
            for (int i = 0; i < 3; ++i) { cs[i] += m * cG[i]; vs[i] += m * vc[i]; }
            mt += m;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { pos[i] = cs[i] / mt; vel[i] = vs[i] / mt; }
    }
    pos[0] += x0;
    Real *r = lds + LY::REP + 6 * (lane < T::NOS ? lane : T::NOS);
#pragma unroll
    for (int i = 0; i < 3; ++i) { r[i] = pos[i]; r[3 + i] = vel[i]; }
}

DEV int clamp_row(int r, int nrows) { return r < 0 ? 0 : (r >= nrows ? nrows - 1 : r); }

/* counter-based RNG (splitmix64) for device-drawn reset indices */
DEV uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
DEV int draw_index(uint64_t seed, int env, int count, int hi) {
    uint64_t r = splitmix64(seed ^ splitmix64(((uint64_t)env << 32) | (uint32_t)count));
    return (int)(r % (uint64_t)(hi + 1));
}

/* ------------------------------------------- the analysis kernels' frame
 * id / ma / so / ik / jr / ia_kernel share one launch shape and prologue:
 * one state per T::G lanes, EPB states per workgroup (BIOIM_EPB; ia_kernel:
 * IaLay::EPB), the SModel image staged into LDS in front of the states' Lay
 * regions, then the env kernel's kinematics at the state's (q, u).  A
 * kernel's arguments are the handle's model (ModelArgs) and the call's own
 * list, a struct templated on its pointee type that follows the kernel: P =
 * void is what the bioim_* entry point fills, P = Real (jr_kernel: IO) what
 * the kernel takes (analysis_launch converts). */
template <class T, typename Real> struct ModelArgs {
    const DModel<Real> *Mg;
    const SModel<T, Real> *Sg;
};

/* the model image into LDS by all EPB * G threads (before any lane exits), a barrier, the image */
template <int EPB, class T, typename Real>
DEV const SModel<T, Real> &stage_model(const SModel<T, Real> *Sg, unsigned char *smem_raw) {
    const uint4 *src = reinterpret_cast<const uint4 *>(Sg);
    uint4 *dst = reinterpret_cast<uint4 *>(smem_raw);
    for (int i = threadIdx.x; i < (int)(smodel_bytes<T, Real>() / 16); i += EPB * T::G) dst[i] = src[i];
    __syncthreads();
    return *reinterpret_cast<const SModel<T, Real> *>(smem_raw);
}

/* dof lane: row idx of an optional [n][ND] input (IO: the caller's type), 0 where it is not given */
template <typename Real, int ND, typename IO> DEV Real opt_row(const IO *p, int idx, int lane, int n) {
    return p ? Real(GAT(p, (size_t)idx * ND + lane, (size_t)n * ND)) : Real(0);
}

/* The step's kinematics at (qd, ud) of the dof lanes, publish_coords through
 * kin_column: frames (KB) and columns (S) are in LDS after the caller's next
 * wave_sync (none here: id / jr / ia go on to body_inertia first).  FN: the
 * fn_slots switch.  Returns x0, the shift of the ground origin. */
template <bool FN, class T, typename Real>
DEV Real state_kinematics(const DModel<Real> &M, const SModel<T, Real> &SM, Real *lds, int lane, Real qd, Real ud) {
    using LY = Lay<T, Real>;
    constexpr int ND = LY::ND, NB = T::NB;
    publish_coords<T, Real>(M, SM, lds, lane, qd, ud);
    if (lane < ND) {
#pragma unroll
        for (int i = 0; i < 6; ++i) lds[LY::SL + 6 * lane + i] = 0;
    }
    wave_sync();
    Real x0 = 0;
    if constexpr (T::TX >= 0) {
        if constexpr (T::coord_dof[T::TX] >= 0) x0 = M.float_origin ? lds[LY::QF + T::TX] : Real(0);
    }
    fn_slots<FN, T, Real>(SM, lds, lane);
    if (lane < NB) kin_local<T, Real>(SM, lds, lane);
    if (lane == NB) kin_ground<T, Real>(lds, x0);
    wave_sync();
    if (lane < NB) kin_chain<T, Real>(SM, lds, lane, x0);
    wave_sync();
    if (lane < ND) kin_column<T, Real>(SM, lds, lane);
    return x0;
}

/* body lane, after body_inertia: the body's gravity wrench (moment about the
 * shifted origin, force) taken back out of WB, which then holds the velocity
 * terms only; KEEP: the wrench itself goes to wg[6] (else wg is not read).
 * The stores to wg stay between the updates of WB: with all of WB updated
 * first the compiler forwards body_inertia's values into the sums and fuses
 * them differently, which moved ia_kernel's results by some ulp */
template <bool KEEP, class T, typename Real>
DEV void gravity_wrench_out(const DModel<Real> &M, const SModel<T, Real> &SM, Real *lds, int lane, Real *wg) {
    using LY = Lay<T, Real>;
    const Real *kb = lds + LY::KB + 18 * lane;
    Real cG[3], mg[3], t[3];
    mv3(kb, SM.body[lane].com, cG);
#pragma unroll
    for (int i = 0; i < 3; ++i) { cG[i] += kb[9 + i]; mg[i] = SM.body[lane].mass * M.gravity[i]; }
    cross3(cG, mg, t);
    Real *wb = lds + LY::WB + 6 * lane;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        wb[i] += t[i]; wb[3 + i] += mg[i];
        if constexpr (KEEP) { wg[i] = t[i]; wg[3 + i] = mg[i]; }
    }
}

/* ------------------------------------------------- inverse dynamics
 * Batched primitives of the reference's Boost.Python InverseDynamics helper
 * (bioimitation/imitation_envs/inverse_dynamics/inverse_dynamics.cpp:45-205),
 * muscles disabled (:47-52), no controller (actuator controls 0).  One
 * state per G lanes, the env kernel's LDS image and kinematics:
 *   GRAVITY   g(q)            M q'' + c = g + tau           (:127-141)
 *   CORIOLIS  c(q, u)                                       (:143-158)
 *   MULT_M    M(q) v                                        (:160-175)
 *   MULT_MINV M(q)^-1 v                                     (:177-192)
 *   RESIDUAL  M v + c - f_applied(q, u), v = q''            (:63-94)
 *   TOTAL     c - f_applied(q, u)  (M q'' + f = tau)        (:96-125)
 * f_applied = gravity + Hunt-Crossley contact + coordinate limit forces
 * (generalized).  Vectors are [n][ndof] in dof order. */
template <typename P> struct IdFields {   /* bioim_inverse_dynamics */
    int n, op;
    const P *q, *u, *v;
    P *out;
};

template <class T, typename Real>
#ifndef BIOIM_ID_NO_WAVES_ATTR
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void id_kernel(ModelArgs<T, Real> md, IdFields<Real> a) {
#else   /* the compiler-crash reproducer (profiles/r03/regalloc_crash/): without the occupancy attribute */
__global__ __launch_bounds__(BIOIM_EPB * T::G) void id_kernel(ModelArgs<T, Real> md, IdFields<Real> a) {
#endif
    using LY = Lay<T, Real>;
    constexpr int G = T::G, ND = LY::ND, NB = T::NB, NP = LY::NP, EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    const int op = a.op;
    const bool use_u = op == BIOIM_ID_CORIOLIS || op == BIOIM_ID_RESIDUAL || op == BIOIM_ID_TOTAL;
    const bool applied = op == BIOIM_ID_RESIDUAL || op == BIOIM_ID_TOTAL;
    const bool need_m = op == BIOIM_ID_MULT_M || op == BIOIM_ID_MULT_MINV || op == BIOIM_ID_RESIDUAL;
    Real qd = 0, ud = 0, vd = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = use_u ? GAT(a.u, (size_t)idx * ND + lane, (size_t)a.n * ND) : Real(0);
        vd = (need_m || op == BIOIM_ID_MULT_MINV) ? GAT(a.v, (size_t)idx * ND + lane, (size_t)a.n * ND) : Real(0);
    }
    state_kinematics<false, T, Real>(M, SM, lds, lane, qd, ud);
    if (lane < NB) {
        body_inertia<T, Real>(SM, M, lds, lane);
        if (op == BIOIM_ID_CORIOLIS) gravity_wrench_out<false, T, Real>(M, SM, lds, lane, nullptr);   /* velocity terms only */
    }
    wave_sync();
    {   /* subtree sums of inertia and wrench (all reads, then all writes) */
        Real ic[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, wb[6] = {0, 0, 0, 0, 0, 0};
        if (lane < NB) {
            sfor<0, NB>([&](auto dI) {
                constexpr int d = decltype(dI)::value;
                if ((T::anc[d] >> lane) & 1u) {
#pragma unroll
                    for (int i = 0; i < 10; ++i) ic[i] += lds[LY::IC + 10 * d + i];
#pragma unroll
                    for (int i = 0; i < 6; ++i) wb[i] += lds[LY::WB + 6 * d + i];
                }
            });
        }
        wave_sync();
        if (lane < NB) {
#pragma unroll
            for (int i = 0; i < 10; ++i) lds[LY::IC + 10 * lane + i] = ic[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) lds[LY::WB + 6 * lane + i] = wb[i];
        }
    }
    if (applied) {
        if (lane < T::NS) contact_lane<false, T, Real>(SM, lds, lane, Real(0));
        if (lane < T::NL) {
            const int cc = SM.lim_coord[lane];
            const Real qv = lds[LY::QF + cc], qdv = lds[LY::UF + cc];
            const Real qup = SM.lim_qup[lane], qlo = SM.lim_qlow[lane], tr = SM.lim_trans[lane];
            const Real itr = SM.lim_itrans[lane];
            const Real up = smooth_step<false>(Real(0), Real(1), qup, qup + tr, itr, qv);
            const Real lo = smooth_step<false>(Real(1), Real(0), qlo - tr, qlo, itr, qv);
            lds[LY::LIM + 4 * lane] = -SM.lim_kup[lane] * up * (qv - qup) + SM.lim_klow[lane] * lo * (qlo - qv) -
                                      SM.lim_damp[lane] * (up + lo) * qdv;
        }
    }
    wave_sync();
    if (need_m && lane < ND) {
        /* row k = lane of the packed lower M, every entry (the structural
         * zeros too: the products below read whole rows): M_kl = S_l . I^c S_k
         * for l on k's root path (as phase 3 of dynamics, without the
         * implicit terms) */
        const Real *Sd = lds + LY::S + 6 * lane, *ic = lds + LY::IC + 10 * SM.dof_cb[lane];
        Real Gk[6], t[3];
        symv(ic + 4, Sd, Gk);
        cross3(ic + 1, Sd + 3, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) Gk[i] += t[i];
        cross3(Sd, ic + 1, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) Gk[3 + i] = ic[0] * Sd[3 + i] + t[i];
        unsigned path = 0;
        sfor<0, ND>([&](auto kI) {
            constexpr int k = decltype(kI)::value;
            constexpr unsigned pm = DofTree<T>::path_mask(k);
            path = lane == k ? pm : path;
        });
        Real *row = lds + LY::MP + (lane * (lane + 1)) / 2;
        sfor<0, ND>([&](auto lI) {
            constexpr int l = decltype(lI)::value;
            if (l <= lane) {
                const Real *Sl = lds + LY::S + 6 * l;
                row[l] = ((path >> l) & 1u) ? dot3(Sl, Gk) + dot3(Sl + 3, Gk + 3) : Real(0);
            }
        });
    }
    if (lane < ND) lds[LY::RHS + lane] = vd;
    wave_sync();
    Real r = 0;
    if (op == BIOIM_ID_MULT_MINV) {
        Real A[NP], xs[ND];
#pragma unroll
        for (int e = 0; e < NP; ++e) A[e] = lds[LY::MP + e];
#pragma unroll
        for (int d = 0; d < ND; ++d) xs[d] = lds[LY::RHS + d];
        ltl_solve<T, ND, Real>(A, xs);
#pragma unroll
        for (int d = 0; d < ND; ++d) r = lane == d ? xs[d] : r;
    } else if (lane < ND) {
        const Real *Sd = lds + LY::S + 6 * lane, *wb = lds + LY::WB + 6 * SM.dof_cb[lane];
        const Real bias = dot3(Sd, wb) + dot3(Sd + 3, wb + 3);   /* c - g (gravity removed for CORIOLIS) */
        Real fa = 0;
        if (applied) {
            sfor<0, T::NS>([&](auto sI) {
                constexpr int sp = decltype(sI)::value;
                constexpr unsigned msk = T::dofmask[T::sphere_cb[sp]];
                const Real *cj = lds + LY::CJ + LY::CJN * sp;
                Real jd[3];
                contact_jac(Sd, cj, jd);
                const Real term = dot3(jd, cj + 3);
                fa += (lds[LY::CW + 8 * sp + 6] > 0 && ((msk >> lane) & 1u)) ? term : Real(0);
            });
#pragma unroll
            for (int li = 0; li < T::NL; ++li)
                if (SM.lim_dof[li] == lane) fa += lds[LY::LIM + 4 * li];
        }
        Real mv = 0;
        if (need_m) {
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                const int hi = lane > k ? lane : k, lo = lane > k ? k : lane;
                mv += lds[LY::MP + hi * (hi + 1) / 2 + lo] * lds[LY::RHS + k];
            }
        }
        if (op == BIOIM_ID_GRAVITY) r = -bias;
        else if (op == BIOIM_ID_CORIOLIS) r = bias;
        else if (op == BIOIM_ID_MULT_M) r = mv;
        else if (op == BIOIM_ID_RESIDUAL) r = mv + bias - fa;
        else r = bias - fa;
    }
    if (lane < ND) GAT(a.out, (size_t)idx * ND + lane, (size_t)a.n * ND) = r;
}

/* -------------------------------------------------------- muscle analysis
 * bioim_muscle_eval (include/bioim.h): the muscles' geometry, fiber state
 * and generalized force at n arbitrary states.  One state per G lanes, the
 * env kernel's LDS image and kinematics (as id_kernel, without the inertia
 * half); then lane l takes the muscles of slots l, l + G, ... (mslot, the
 * step's own assignment) and runs the step's device functions on them, with
 * the step's branch-free switches: muscle_path, then muscle_equilibrium where
 * no fiber length is given, then muscle_eval at excitation = activation and a
 * cold fiber-velocity start.  -F_t dL/dq goes to the step's TAU slots and the
 * dof lanes gather it through SM.tau_src in the step's order.  Nothing of the
 * env state is read or written.  Any output may be null. */
template <typename P> struct MaFields {   /* bioim_muscle_eval */
    int n;
    const P *q, *u, *act, *lce;
    P *length, *speed, *dldq, *fiber, *tau;
};

template <class T, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void ma_kernel(ModelArgs<T, Real> md, MaFields<Real> a) {
    using LY = Lay<T, Real>;
    using SW = BfSwitch<T>;   /* the step's switches (dynamics(), semi-implicit kernels) */
    constexpr int G = T::G, ND = LY::ND, NM = T::NM, MPL = LY::MPL, NSP = T::MAXSPAN, EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    static_assert(NM > 0, "muscle topologies only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    Real qd = 0, ud = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = opt_row<Real, ND>(a.u, idx, lane, a.n);
    }
    state_kinematics<SW::FN, T, Real>(M, SM, lds, lane, qd, ud);
    wave_sync();   /* the columns are out, and the joint-local region (LOC / SL) the TAU slots share is free */
    const bool fib = a.act != nullptr;
    if (lane == 0) lds[LY::TAU + LY::TZ] = Real(0);
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int m = mslot<T>(lane + j * G);
        if (m < NM) {
            const SMuscle<Real> &mu = SM.mus[m];
            const size_t row = (size_t)idx * NM + m, rows = (size_t)a.n * NM;
            Real L, dLs[NSP];
            muscle_path<SW::PATH, T, Real>(SM, mu, lds, L, dLs);
            if (a.length) GAT(a.length, row, rows) = L;
            if (a.speed) {
                Real s = 0;
#pragma unroll
                for (int k = 0; k < NSP; ++k) {
                    const int dk = k < mu.nspan ? mu.span[k] : 0;
                    const Real uk = lds[LY::UF + SM.dof_coord[dk]];
                    s += k < mu.nspan ? dLs[k] * uk : Real(0);
                }
                GAT(a.speed, row, rows) = s;
            }
            if (a.dldq) {
                /* the whole row: the span's entries, exact zeros elsewhere */
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    Real v = 0;
#pragma unroll
                    for (int k = 0; k < NSP; ++k) v = (k < mu.nspan && mu.span[k] == d) ? dLs[k] : v;
                    GAT(a.dldq, row * ND + d, rows * ND) = v;
                }
            }
            if (fib) {
                const Real a_ = GAT(a.act, row, rows);
                Real l_;
                if (a.lce) l_ = GAT(a.lce, row, rows);
                else l_ = muscle_equilibrium<SW::EQ, T, Real>(SM, mu, a_, L);
                MState<Real> ms;
                muscle_eval<SW::ME, true, T, Real>(SM, mu, a_, l_, a_, L, Real(0), ms);
                if (a.fiber) {
                    Real *f = a.fiber + GIDX(row * BIOIM_MUSCLE_FIBER_DIM, rows * BIOIM_MUSCLE_FIBER_DIM);
                    f[0] = ms.lce; f[1] = ms.vce; f[2] = ms.Ft; f[3] = ms.Ff; f[4] = ms.Fa;
                }
                const Real nFt = -ms.Ft;
                Real *ts = lds + LY::TAU + (lane + j * G) * NSP;
#pragma unroll
                for (int k = 0; k < NSP; ++k) ts[k] = nFt * dLs[k];
            }
        }
    });
    wave_sync();
    if (fib && a.tau && lane < ND) {
        Real r = 0;
#pragma unroll
        for (int i = 0; i < T::MAXARM; ++i) r += lds[LY::TAU + SM.tau_src[lane][i]];
        GAT(a.tau, (size_t)idx * ND + lane, (size_t)a.n * ND) = r;
    }
}

/* ----------------------------------------------------- static optimization
 * bioim_static_opt (include/bioim.h): per state the muscle activations that
 * produce a target generalized force at least effort,
 *     min sum_m a_m^2 + sum_d lam_d (tau_d - (B a + c)_d)^2,  lo <= a_m <= hi,
 * B[d][m] = -dL_m/dq_d Fa_m, c_d = -sum_m dL_m/dq_d Fp_m (0: passive off), Fa /
 * Fp the rigid-tendon capacities of muscle_rigid_capacity.  fp64 only.
 *
 * ma_kernel's launch shape and prologue (one state per G lanes, the model
 * image in LDS, kinematics without inertias or contact).  The QP's variable s
 * is the muscle of lane slot s (mslot: a bijection of [0, NM)), so lane l owns
 * the variables l, l + G.  The muscle rounds leave per slot the B entries over
 * the muscle's span (the step's TAU slots, gathered per dof through
 * SM.tau_src) and, behind them, the passive entries -dL/dq Fp.  After them the
 * frames and columns are dead and [0, Lay::U) of the state's LDS region takes
 * the solver's data (SoLay).
 *
 * Solver: a primal active set (BVLS).  All variables start at lo.  Per pass
 * the dof lanes form the residual rho = tau - c - B a in dof space and the
 * muscle lanes the negative gradient w = B^T lam rho - a from it (the
 * normal-equations right-hand side g - H a loses cond(H) ~ 1e5 digits of a
 * large tau; this form loses them of the small residual only).  A pass in
 * CHECK mode frees the bound variable whose w points furthest inward (ties:
 * the lowest muscle index; w must exceed 16 ulp of the sums that form it, rho's
 * cancellation included), or ends: the KKT conditions hold.  Every pass not
 * ended then solves H_FF dz = w_F over the free set by a Cholesky
 * factorization of H with the bound rows and columns replaced by the
 * identity (fixed size NM, no index sets), the right-hand side carried as row
 * NM of the packed matrix; a full step that stays inside the box is taken
 * and the pass after it checks again, otherwise the step stops at the first
 * bound met (ties: the lowest muscle index), that variable is bound, and the
 * next pass solves again.  A variable freed by rounding noise (its step leads
 * straight back out) is bound again and kept out of the choice until a full
 * step succeeds.  Each pass costs one factorization; the count of them is
 * the state's status.  SoLay::CAP passes end the loop with status -1, a
 * pivot <= 0 (or NaN) with -2.
 *
 * The 4 states of a wave need different pass counts: every lane loops under
 * its own state's done flag (uniform over the state's G lanes) and the wave
 * leaves when all are done; only wave_sync orders the LDS traffic, and no
 * workgroup barrier follows the idx >= n exit.  No atomics, no read-modify-
 * write at run-time indices shared between lanes, sums in a fixed order: a
 * state's result does not depend on n or its neighbours.  Matrices, sets and
 * flags live in LDS; the per-lane arrays have compile-time indices only.
 * The iteration itself is box_qp_solve, with a lower and an upper bound per
 * variable in LDS (SoLay::LO / HI), shared with cmc_kernel; this kernel writes
 * its two scalars there. */

template <typename P> struct SoFields {   /* bioim_static_opt (fp64 only) */
    int n, passive;
    const P *q, *u, *tau, *row_weight;
    double lo, hi;
    P *act, *residual, *tau_muscle, *capacity;
    int32_t *status;
};

/* the solver's map of [0, Lay::U) (reals), and the slot arrays behind it */
template <class T, typename Real> struct SoLay {
    using LY = Lay<T, Real>;
    static constexpr int NM = T::NM > 0 ? T::NM : 1, ND = LY::ND, NSP = T::MAXSPAN;
    static constexpr int NH = NM * (NM + 1) / 2;
    static constexpr int H = 0;                /* [NH] packed lower H = I + B^T lam B                    */
    static constexpr int A = H + NH;           /* [NH + NM] the masked copy, then its factor; row NM: rhs */
    static constexpr int DSP = A;              /* assembly only: [NM][NSP] dof of each B entry (-1: none) */
    static constexpr int D = A + NH + NM;      /* [NM] reciprocal pivots                                  */
    static constexpr int X = D + NM;           /* [NM] the activations                                    */
    static constexpr int Z = X + NM;           /* [NM] the step dz                                        */
    static constexpr int F = Z + NM;           /* [NM] -1 at lo, +1 at hi, 0 free                         */
    static constexpr int RHO = F + NM;         /* [ND] lam_d rho_d                                        */
    static constexpr int RER = RHO + ND;       /* [ND] lam_d (|tau_d - c_d| + sum |B a|): rho's rounding scale */
    static constexpr int END = RER + ND;
    static constexpr int BS = LY::TAU;         /* [MPL G][NSP] + zero slot: B entries by lane slot        */
    static constexpr int CS = BS + LY::TAUN;   /* the same for -dL/dq Fp                                  */
    static constexpr int LO = CS;              /* the solve: [NM] lower bounds by slot (the passive entries */
    static constexpr int HI = LO + NM;         /* are summed by then), [NM] upper bounds                  */
    static constexpr int CAP = 8 * NM;         /* passes; the most observed: 21 (NM = 14), 29 (NM = 22), 18 (NM = 19) */
    static_assert(END <= LY::U, "the solver's data must fit below the union region");
    static_assert(NM * NSP <= NH + NM, "the dof table must fit in the work matrix");
    static_assert(CS + LY::TAUN <= LY::SIZE0, "two slot arrays must fit in the union region");
    static_assert(2 * NM <= LY::TAUN, "the bounds must fit in the second slot array");
};

/* Rigid-tendon capacity of one muscle at path length L and lengthening speed
 * Ld (OpenSim's StaticOptimization assumptions): Fa the active fiber force
 * along the tendon at activation 1, Fp the passive one.
 *   w = l_opt sin(alpha_opt), l_t = max(L - l_ts, 0),
 *   l_m = max(sqrt(l_t^2 + w^2), l_min), cos = sqrt(l_m^2 - w^2) / l_m,
 *   Fa = F0 fal(l_m / l_opt) fv(Ld cos / (l_opt v_max)) cos,
 *   Fp = F0 fpe(l_m / l_opt) cos,  both cut at 0 from below */
template <class T, typename Real>
DEV void muscle_rigid_capacity(const SModel<T, Real> &SM, const SMuscle<Real> &mu, Real L, Real Ld, Real &Fa, Real &Fp) {
    const DCurve<Real> &Cfal = SM.curve[mu.cv[0]], &Cfv = SM.curve[mu.cv[1]], &Cfpe = SM.curve[mu.cv[2]];
    const Real w = mu.width, lmin = mu.lmin, zero = 0;
    Real lt = L - mu.lts;
    lt = lt > zero ? lt : zero;
    Real lm = sqrt(lt * lt + w * w);
    lm = lm > lmin ? lm : lmin;
    const Real cosa = sqrt(lm * lm - w * w) / lm;
    Real fal, fv, fpe, d;
    curve_eval<true>(Cfal, lm / mu.lopt, fal, d);
    curve_eval<true>(Cfv, Ld * cosa / mu.lv, fv, d);
    curve_eval<true>(Cfpe, lm / mu.lopt, fpe, d);
    Fa = mu.fiso * fal * fv * cosa;
    Fp = mu.fiso * fpe * cosa;
    /* a curve whose minimum is exactly 0 (the palsy model's fal) comes out of
     * the power-basis Horner form as -1e-32 at its first node; a capacity is
     * not negative, and a muscle without one must have B = 0 exactly */
    const Real zero_f = 0;
    Fa = Fa > zero_f ? Fa : zero_f;
    Fp = Fp > zero_f ? Fp : zero_f;
}

/* The box QP's solve (the comment above: passes, ties, caps, status codes),
 * shared by so_kernel and cmc_kernel:
 *     min sum_s x_s^2 + sum_d lam_d (tc_d - (B x)_d)^2,  LO_s <= x_s <= HI_s.
 * On entry the state's LDS region holds the B entries by lane slot (SoLay::BS,
 * with its zero slot) and every lane has written the bounds of its own slots
 * to SoLay::LO / HI, in the second slot array (so_kernel: its two scalars,
 * broadcast, once the passive entries there are summed); mi[j] is the
 * slot's muscle (NM: none), lam and tc the dof lane's row weight and target.
 * A variable whose range is empty (HI <= LO) stays bound at LO and is never
 * offered to the iteration.  On return xv[j] (and SoLay::X by slot) hold the
 * solution; the value is the state's status.  Every lane of the state calls
 * it; [0, Lay::U) must be dead (it becomes the solver's, SoLay). */
template <class T, typename Real>
DEV int box_qp_solve(const SModel<T, Real> &SM, Real *lds, int lane, const int (&mi)[Lay<T, Real>::MPL], Real lam,
                     Real tc, Real (&xv)[Lay<T, Real>::MPL]) {
    using LY = Lay<T, Real>;
    using SL = SoLay<T, Real>;
    constexpr int G = T::G, ND = LY::ND, NM = T::NM, MPL = LY::MPL, NSP = T::MAXSPAN, NH = SL::NH;
    /* muscle lanes: the slot's bounds; the variables start at lo; the dof table
     * of the B entries; own entries and dofs to registers */
    Real lo[MPL], hi[MPL], fl[MPL], bown[MPL][NSP];
    int down[MPL][NSP];
    bool blk[MPL], fixed[MPL];
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int s = lane + j * G;
        lo[j] = s < NM ? lds[SL::LO + s] : Real(0);
        hi[j] = s < NM ? lds[SL::HI + s] : Real(0);
        fixed[j] = !(hi[j] > lo[j]);   /* an empty range: bound at lo for good */
        xv[j] = lo[j]; fl[j] = Real(-1); blk[j] = false;
        const SMuscle<Real> &mu = SM.mus[mi[j] < NM ? mi[j] : 0];
#pragma unroll
        for (int k = 0; k < NSP; ++k) {
            const bool in = mi[j] < NM && k < mu.nspan;
            down[j][k] = in ? mu.span[k] : -1;
            bown[j][k] = lds[SL::BS + s * NSP + k];
            if (s < NM) lds[SL::DSP + s * NSP + k] = Real(down[j][k]);
        }
        if (s < NM) { lds[SL::X + s] = lo[j]; lds[SL::F + s] = Real(-1); }
    });
    if (lane < ND) lds[SL::RHO + lane] = lam;   /* lam_d, for the assembly (RHO is rewritten per pass) */
    wave_sync();
    /* H: row s (uniform), the lane's columns t <= s */
    for (int s = 0; s < NM; ++s) {
        Real ws[NSP], dsr[NSP];
#pragma unroll
        for (int k = 0; k < NSP; ++k) {
            dsr[k] = lds[SL::DSP + s * NSP + k];
            const int dk = dsr[k] >= Real(0) ? (int)dsr[k] : 0;
            ws[k] = lds[SL::RHO + dk] * lds[SL::BS + s * NSP + k];   /* lam_d B_ds (0 for an unused entry) */
        }
        sfor<0, MPL>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            const int t = lane + j * G;
            if (t <= s) {
                Real acc = t == s ? Real(1) : Real(0);
#pragma unroll
                for (int k = 0; k < NSP; ++k)
#pragma unroll
                    for (int kk = 0; kk < NSP; ++kk)
                        acc += (dsr[k] == Real(down[j][kk]) && down[j][kk] >= 0) ? ws[k] * bown[j][kk] : Real(0);
                lds[SL::H + s * (s + 1) / 2 + t] = acc;
            }
        });
    }
    wave_sync();   /* the dof table is dead: its place is the work matrix */
    const Real tiny = Real(16) * Real(2.220446049250313e-16);   /* 16 ulp of the sums that form w */
    int status = 0, it = 0, mode = 0, tnew = -1;
    bool done = false;
    while (!done) {
        /* rho and its rounding scale (dof lanes), then w (muscle lanes) */
        if (lane < ND) {
            Real sum = 0, asum = 0;
#pragma unroll
            for (int i = 0; i < T::MAXARM; ++i) {
                const int src = SM.tau_src[lane][i];
                const int sx = src / NSP < NM ? src / NSP : NM - 1;
                const Real term = lds[SL::BS + src] * lds[SL::X + sx];   /* the zero slot: B = 0 */
                sum += term; asum += fabs(term);
            }
            lds[SL::RHO + lane] = lam * (tc - sum);
            lds[SL::RER + lane] = lam * (fabs(tc) + asum);
        }
        wave_sync();
        Real wv[MPL], wtol[MPL];
        sfor<0, MPL>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            Real w = 0, e = 0;
#pragma unroll
            for (int k = 0; k < NSP; ++k) {
                const int dk = down[j][k] >= 0 ? down[j][k] : 0;
                w += bown[j][k] * lds[SL::RHO + dk];
                e += fabs(bown[j][k]) * lds[SL::RER + dk];
            }
            wv[j] = w - xv[j];
            wtol[j] = tiny * (e + fabs(xv[j]));
        });
        if (mode == 0) {
            /* CHECK: free the bound variable whose w points furthest inward */
            Real best = 0;
            Real sc[MPL];
            int bad = 0;
            sfor<0, MPL>([&](auto jI) {
                constexpr int j = decltype(jI)::value;
                bad |= (mi[j] < NM && !(wv[j] == wv[j])) ? 1 : 0;   /* a NaN came in */
                Real v = fl[j] < Real(0) ? wv[j] : (fl[j] > Real(0) ? -wv[j] : Real(0));
                v = (mi[j] < NM && !blk[j] && !fixed[j] && v > wtol[j]) ? v : Real(0);
                sc[j] = v;
                best = v > best ? v : best;
            });
            best = group_max<G>(best);
            if (group_min<G>(-bad) < 0) {
                done = true;
                status = -2;
            } else if (!(best > Real(0))) {
                done = true;
                status = it;
            } else {
                int cand = NM;
                sfor<0, MPL>([&](auto jI) {
                    constexpr int j = decltype(jI)::value;
                    cand = (sc[j] == best && mi[j] < cand) ? mi[j] : cand;
                });
                const int t = group_min<G>(cand);
                sfor<0, MPL>([&](auto jI) {
                    constexpr int j = decltype(jI)::value;
                    if (mi[j] == t) { fl[j] = Real(0); lds[SL::F + lane + j * G] = Real(0); }
                });
                tnew = t;
                mode = 1;
            }
        }
        if (!done && ++it > SL::CAP) {
            done = true;
            status = -1;
        }
        if (!done) {
            wave_sync();
            /* the masked matrix (bound rows and columns: identity) and, as row NM, the right-hand side */
            for (int i = 0; i < NM; ++i) {
                const bool fi = lds[SL::F + i] == Real(0);
                sfor<0, MPL>([&](auto jI) {
                    constexpr int j = decltype(jI)::value;
                    const int t = lane + j * G;
                    if (t <= i) {
                        const int e = i * (i + 1) / 2 + t;
                        const Real hv = lds[SL::H + e];
                        lds[SL::A + e] = (fi && fl[j] == Real(0)) ? hv : (t == i ? Real(1) : Real(0));
                    }
                });
            }
            sfor<0, MPL>([&](auto jI) {
                constexpr int j = decltype(jI)::value;
                const int t = lane + j * G;
                if (t < NM) lds[SL::A + NH + t] = fl[j] == Real(0) ? wv[j] : Real(0);
            });
            wave_sync();
            /* Cholesky, right-looking; row NM comes out as L^-1 rhs */
            bool ok = true;
            for (int k = 0; k < NM && ok; ++k) {
                const Real piv = lds[SL::A + k * (k + 1) / 2 + k];
                ok = piv > Real(0);
                if (ok) {
                    const Real rp = Real(1) / sqrt(piv);
                    for (int i = k + 1 + lane; i <= NM; i += G) lds[SL::A + i * (i + 1) / 2 + k] *= rp;
                    if (lane == 0) lds[SL::D + k] = rp;
                    wave_sync();
                    for (int i = k + 1 + lane; i <= NM; i += G) {
                        Real *ri = lds + SL::A + i * (i + 1) / 2;
                        const Real lik = ri[k];
                        const int je = i < NM ? i : NM - 1;
                        for (int jc = k + 1; jc <= je; ++jc) ri[jc] -= lik * lds[SL::A + jc * (jc + 1) / 2 + k];
                    }
                    wave_sync();
                }
            }
            if (!ok) {
                done = true;
                status = -2;
            } else {
                /* L^T dz = y, last row first */
                for (int k = NM - 1; k >= 0; --k) {
                    const Real zk = lds[SL::A + NH + k] * lds[SL::D + k];
                    const Real *rk = lds + SL::A + k * (k + 1) / 2;
                    for (int i = lane; i < k; i += G) lds[SL::A + NH + i] -= rk[i] * zk;
                    if (lane == 0) lds[SL::Z + k] = zk;
                    wave_sync();
                }
                /* the step: whole if it stays in the box, else to the first bound met */
                Real zv[MPL], al[MPL], bd[MPL];
                Real amin = Real(2);
                sfor<0, MPL>([&](auto jI) {
                    constexpr int j = decltype(jI)::value;
                    const int t = lane + j * G;
                    const bool fr = t < NM && fl[j] == Real(0);
                    zv[j] = fr ? xv[j] + lds[SL::Z + (t < NM ? t : 0)] : xv[j];
                    const bool under = fr && zv[j] < lo[j], over = fr && zv[j] > hi[j];
                    bd[j] = under ? lo[j] : hi[j];
                    const Real den = zv[j] - xv[j];
                    Real av = (under || over) ? (bd[j] - xv[j]) / den : Real(2);
                    av = av < Real(0) ? Real(0) : av;     /* an under / over step has den != 0; rounding only */
                    al[j] = (under || over) ? (av < Real(1) ? av : Real(1)) : Real(2);
                    amin = al[j] < amin ? al[j] : amin;
                });
                amin = group_min<G>(amin);
                if (amin > Real(1)) {   /* inside the box: take it, check again */
                    sfor<0, MPL>([&](auto jI) {
                        constexpr int j = decltype(jI)::value;
                        xv[j] = zv[j];
                        blk[j] = false;
                    });
                    mode = 0;
                } else {
                    int cand = NM;
                    sfor<0, MPL>([&](auto jI) {
                        constexpr int j = decltype(jI)::value;
                        cand = (al[j] == amin && mi[j] < cand) ? mi[j] : cand;
                    });
                    const int jm = group_min<G>(cand);
                    const bool back = jm == tnew && amin == Real(0);   /* freed by rounding noise */
                    sfor<0, MPL>([&](auto jI) {
                        constexpr int j = decltype(jI)::value;
                        const int t = lane + j * G;
                        if (t < NM && fl[j] == Real(0)) xv[j] = xv[j] + amin * (zv[j] - xv[j]);
                        if (mi[j] == jm) {
                            xv[j] = bd[j];
                            fl[j] = bd[j] == lo[j] ? Real(-1) : Real(1);
                            blk[j] = back;
                            lds[SL::F + t] = fl[j];
                        }
                        /* a free variable the partial step leaves outside by rounding stays inside */
                        xv[j] = xv[j] < lo[j] ? lo[j] : (xv[j] > hi[j] ? hi[j] : xv[j]);
                    });
                    if (back) mode = 0;
                }
                tnew = -1;
                sfor<0, MPL>([&](auto jI) {
                    constexpr int j = decltype(jI)::value;
                    const int t = lane + j * G;
                    if (t < NM) lds[SL::X + t] = xv[j];
                });
            }
        }
        wave_sync();
    }
    return status;
}

template <class T, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void so_kernel(ModelArgs<T, Real> md, SoFields<Real> a) {
    using LY = Lay<T, Real>;
    using SL = SoLay<T, Real>;
    using SW = BfSwitch<T>;
    constexpr int G = T::G, ND = LY::ND, NM = T::NM, MPL = LY::MPL, NSP = T::MAXSPAN, EPB = BIOIM_EPB;
    constexpr int NH = SL::NH;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    static_assert(NM > 0, "muscle topologies only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    Real qd = 0, ud = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = opt_row<Real, ND>(a.u, idx, lane, a.n);
    }
    state_kinematics<SW::FN, T, Real>(M, SM, lds, lane, qd, ud);
    wave_sync();   /* the columns are out, and the joint-local region (LOC / SL) the slot arrays share is free */
    const bool passive = a.passive != 0;
    const Real lo = a.lo, hi = a.hi;
    if (lane == 0) {
        lds[SL::BS + LY::TZ] = Real(0);
        lds[SL::CS + LY::TZ] = Real(0);
    }
    /* muscle rounds: capacity, then the B (and passive) entries of the slot */
    int mi[MPL];     /* the slot's muscle (NM: none) */
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int s = lane + j * G;
        const int m = mslot<T>(s);
        mi[j] = m < NM ? m : NM;
        Real *bs = lds + SL::BS + s * NSP, *cs = lds + SL::CS + s * NSP;
        if (m < NM) {
            const SMuscle<Real> &mu = SM.mus[m];
            Real L, dLs[NSP];
            muscle_path<SW::PATH, T, Real>(SM, mu, lds, L, dLs);
            /* a dof that moves every point of the path moves it rigidly: dL/dq is
             * exactly 0 there (the sum over the path vanishes, as on the floating
             * base, which the span leaves out for that reason), unless a moving
             * point's own coordinate is that dof.  muscle_path's sum leaves
             * rounding noise (1e-15), which Fa ~ 1e4 N and a joint residual ~ 1e3
             * N m turn into activations of 1e-8 for a muscle without any moment
             * arm: such span entries are set to the 0 they stand for */
            unsigned common = ~0u, mov = 0u;
#pragma unroll
            for (int p = 0; p < T::MAXPT; ++p) {
                const DPathPt<Real> &pt = SM.pt[mu.pt_off + (p < mu.npt ? p : 0)];
                common &= pt.dofmask;
                mov |= (p < mu.npt && pt.mdof >= 0) ? 1u << pt.mdof : 0u;
            }
            const unsigned rigid = common & ~mov;
            Real Ld = 0;
#pragma unroll
            for (int k = 0; k < NSP; ++k) {
                const int dk = k < mu.nspan ? mu.span[k] : 0;
                dLs[k] = ((rigid >> dk) & 1u) ? Real(0) : dLs[k];
                const Real uk = lds[LY::UF + SM.dof_coord[dk]];
                Ld += k < mu.nspan ? dLs[k] * uk : Real(0);
            }
            Real Fa, Fp;
            muscle_rigid_capacity<T, Real>(SM, mu, L, Ld, Fa, Fp);
            if (a.capacity) {
                const size_t row = (size_t)idx * NM + m, rows = (size_t)a.n * NM;
                Real *cp = a.capacity + GIDX(row * 2, rows * 2);
                cp[0] = Fa; cp[1] = Fp;
            }
#pragma unroll
            for (int k = 0; k < NSP; ++k) {
                const bool in = k < mu.nspan;
                bs[k] = in ? -dLs[k] * Fa : Real(0);
                cs[k] = (in && passive) ? -dLs[k] * Fp : Real(0);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NSP; ++k) { bs[k] = Real(0); cs[k] = Real(0); }
        }
    });
    wave_sync();   /* frames, columns, coordinates are dead: [0, U) is the solver's */
    /* dof lanes: row weight, target minus passive force */
    Real lam = 0, tq = 0, cq = 0, tc = 0;
    if (lane < ND) {
        lam = a.row_weight ? a.row_weight[lane] : Real(1);
        tq = GAT(a.tau, (size_t)idx * ND + lane, (size_t)a.n * ND);
#pragma unroll
        for (int i = 0; i < T::MAXARM; ++i) cq += lds[SL::CS + SM.tau_src[lane][i]];
        tc = tq - cq;
    }
    wave_sync();   /* the passive entries are summed: their place takes the bounds */
    /* the bounds of the lane's own slots, then the solve */
    Real xv[MPL];
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int s = lane + j * G;
        if (s < NM) { lds[SL::LO + s] = lo; lds[SL::HI + s] = hi; }
    });
    const int status = box_qp_solve<T, Real>(SM, lds, lane, mi, lam, tc, xv);
    /* outputs: act by muscle; tau_muscle = B a + c, residual = tau - tau_muscle by dof */
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        if (mi[j] < NM) GAT(a.act, (size_t)idx * NM + mi[j], (size_t)a.n * NM) = xv[j];
    });
    if (lane == 0 && a.status) a.status[idx] = status;
    if (lane < ND && (a.residual || a.tau_muscle)) {
        Real sum = 0;
#pragma unroll
        for (int i = 0; i < T::MAXARM; ++i) {
            const int src = SM.tau_src[lane][i];
            const int sx = src / NSP < NM ? src / NSP : NM - 1;
            sum += lds[SL::BS + src] * lds[SL::X + sx];
        }
        const Real tm = sum + cq;
        if (a.tau_muscle) GAT(a.tau_muscle, (size_t)idx * ND + lane, (size_t)a.n * ND) = tm;
        if (a.residual) GAT(a.residual, (size_t)idx * ND + lane, (size_t)a.n * ND) = tq - tm;
    }
}

/* ------------------------------------------------- computed muscle control
 * bioim_cmc (include/bioim.h): per state the excitations whose muscles, run
 * through the step's own activation and contraction dynamics over a window T,
 * deliver at its end the forces that produce a target generalized force.
 * fp64 only.
 *
 * so_kernel's launch shape and prologue, the kinematics run twice: at q for
 * the path lengths L0, then (after a wave_sync: every lane has read the first
 * frames) at q1 for L1 and dL/dq, with so_kernel's structural zeros.  Lane l
 * owns the muscles of slots l, l + G through all four phases.
 *   2. cmc_predict at the two ends of the slot's excitation bracket: registers
 *      only (the muscle substep reads the model image, nothing of the state's
 *      LDS region), so the lanes of a wave need no order among them.
 *   3. B = -dL/dq F0 by slot in the step's TAU slots (SoLay::BS), the force
 *      range over F0 as the slot's bounds (SoLay::LO / HI), box_qp_solve.
 *   4. Illinois on P(e) - F* per slot, each lane under its own count, at most
 *      max_iter evaluations; no LDS traffic, no barrier inside.
 * LDS: Lay's state region as so_kernel uses it (SoLay below Lay::U, the slot
 * array at Lay::TAU, the bounds in the second slot array, which has no passive
 * entries to hold here); nothing is added.  Loops: nsub + 1 muscle evaluations
 * per predictor, 2 + max_iter predictors per slot, SoLay::CAP passes, and
 * solve_fv's own cap inside muscle_eval.  No atomics, fixed summation order: a
 * state's result does not depend on n or its neighbours. */
template <typename P> struct CmcFields {   /* bioim_cmc (fp64 only) */
    int n, nsub, max_iter;
    const P *q, *u, *act, *lce, *q1, *tau, *row_weight;
    double window, emin, emax, ftol;
    P *excitation, *force, *force_range, *predicted, *state_end, *tau_muscle, *residual;
    int32_t *status, *root_status;
};

/* a b + c in two roundings whatever the contraction mode: q + T u must equal
 * the caller's own product and sum bit for bit */
template <typename Real> DEV Real mul_then_add(Real a, Real b, Real c) {
    Real p = a * b;
    asm volatile("" : "+v"(p));
    return p + c;
}

/* The predictor P_m(e): from (a0, l0) nsub muscle substeps of length h at
 * constant excitation e, substep k at path length L0 + (k / nsub)(L1 - L0) with
 * a cold fiber-velocity start, the updates those of the step (a += h da/dt;
 * unless clamped l += h vce / (1 - h dvce/dl), cut at l_min); then one more
 * evaluation at the end state and L1, whose tendon force is the value.  aE, lE:
 * the end state. */
template <class T, typename Real>
DEV Real cmc_predict(const SModel<T, Real> &SM, const SMuscle<Real> &mu, Real a0, Real l0, Real L0, Real L1, Real e,
                     Real h, int nsub, Real &aE, Real &lE) {
    using SW = BfSwitch<T>;
    Real av = a0, lv = l0, Ft = 0;
    const Real dL = L1 - L0, rn = Real(nsub);
#pragma nounroll
    for (int k = 0; k <= nsub; ++k) {
        const Real L = k < nsub ? L0 + (Real(k) / rn) * dL : L1;
        MState<Real> ms;
        muscle_eval<SW::ME, true, T, Real>(SM, mu, av, lv, e, L, Real(0), ms);
        Ft = ms.Ft;
        if (k < nsub) {
            av += h * ms.dadt;
            if (!ms.clamped) {
#if BIOIM_SUBSTEP_RCP
                const Real ln = lv + h * ms.vce * fast_rcp(Real(1) - h * ms.dvdl);
#else
                const Real ln = lv + h * ms.vce / (Real(1) - h * ms.dvdl);
#endif
                lv = ln < mu.lmin ? mu.lmin : ln;
            }
        }
    }
    aE = av;
    lE = lv;
    return Ft;
}

template <class T, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void cmc_kernel(ModelArgs<T, Real> md, CmcFields<Real> a) {
    using LY = Lay<T, Real>;
    using SL = SoLay<T, Real>;
    using SW = BfSwitch<T>;
    constexpr int G = T::G, ND = LY::ND, NM = T::NM, MPL = LY::MPL, NSP = T::MAXSPAN, EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    static_assert(NM > 0, "muscle topologies only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    const size_t rows = (size_t)a.n * NM;
    Real qd = 0, ud = 0, q1d = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = GAT(a.u, (size_t)idx * ND + lane, (size_t)a.n * ND);
        q1d = a.q1 ? GAT(a.q1, (size_t)idx * ND + lane, (size_t)a.n * ND) : mul_then_add<Real>(a.window, ud, qd);
    }
    /* phase 1: L0 at q, then L1 and dL/dq at q1 */
    state_kinematics<SW::FN, T, Real>(M, SM, lds, lane, qd, ud);
    wave_sync();
    int mi[MPL];     /* the slot's muscle (NM: none) */
    Real L0[MPL], L1[MPL];
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int m = mslot<T>(lane + j * G);
        mi[j] = m < NM ? m : NM;
        L0[j] = 0;
        if (m < NM) {
            Real dLs[NSP];
            muscle_path<SW::PATH, T, Real>(SM, SM.mus[m], lds, L0[j], dLs);
        }
    });
    wave_sync();   /* every lane has read the frames at q */
    state_kinematics<SW::FN, T, Real>(M, SM, lds, lane, q1d, ud);
    wave_sync();   /* the columns are out, and the joint-local region (LOC / SL) the slot array shares is free */
    if (lane == 0) lds[SL::BS + LY::TZ] = Real(0);
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int s = lane + j * G;
        Real *bs = lds + SL::BS + s * NSP;
        L1[j] = 0;
        if (mi[j] < NM) {
            const SMuscle<Real> &mu = SM.mus[mi[j]];
            Real dLs[NSP];
            muscle_path<SW::PATH, T, Real>(SM, mu, lds, L1[j], dLs);
            /* so_kernel's structural zeros: a dof that moves every point of the path */
            unsigned common = ~0u, mov = 0u;
#pragma unroll
            for (int p = 0; p < T::MAXPT; ++p) {
                const DPathPt<Real> &pt = SM.pt[mu.pt_off + (p < mu.npt ? p : 0)];
                common &= pt.dofmask;
                mov |= (p < mu.npt && pt.mdof >= 0) ? 1u << pt.mdof : 0u;
            }
            const unsigned rigid = common & ~mov;
#pragma unroll
            for (int k = 0; k < NSP; ++k) {
                const int dk = k < mu.nspan ? mu.span[k] : 0;
                const Real dl = ((rigid >> dk) & 1u) ? Real(0) : dLs[k];
                bs[k] = k < mu.nspan ? -dl * mu.fiso : Real(0);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NSP; ++k) bs[k] = Real(0);
        }
    });
    wave_sync();   /* frames, columns, coordinates are dead: [0, U) is the solver's */
    /* phase 2: the predictor at the two ends of the slot's bracket */
    const Real h = a.window / Real(a.nsub);
    Real a0[MPL], l0[MPL], eE[MPL][2], fE[MPL][2], aE[MPL][2], lE[MPL][2];
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int s = lane + j * G;
        a0[j] = 0; l0[j] = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) { eE[j][e] = 0; fE[j][e] = 0; aE[j][e] = 0; lE[j][e] = 0; }
        if (mi[j] < NM) {
            const SMuscle<Real> &mu = SM.mus[mi[j]];
            const size_t row = (size_t)idx * NM + mi[j];
            a0[j] = GAT(a.act, row, rows);
            l0[j] = GAT(a.lce, row, rows);
            const Real one = 1;
            const Real el = a.emin > mu.amin ? Real(a.emin) : mu.amin;
            Real eh = a.emax < one ? Real(a.emax) : one;
            eh = eh < el ? el : eh;   /* an empty bracket collapses onto its lower end */
            eE[j][0] = el; eE[j][1] = eh;
#pragma nounroll
            for (int e = 0; e < 2; ++e) {
                Real ae, le;
                const Real f = cmc_predict<T, Real>(SM, mu, a0[j], l0[j], L0[j], L1[j], e ? eh : el, h, a.nsub, ae, le);
                if (e) { fE[j][1] = f; aE[j][1] = ae; lE[j][1] = le; }
                else { fE[j][0] = f; aE[j][0] = ae; lE[j][0] = le; }
            }
            if (a.force_range) {
                Real *fr = a.force_range + GIDX(row * 2, rows * 2);
                fr[0] = fE[j][0]; fr[1] = fE[j][1];
            }
            const bool up = fE[j][0] <= fE[j][1];
            lds[SL::LO + s] = (up ? fE[j][0] : fE[j][1]) / mu.fiso;
            lds[SL::HI + s] = (up ? fE[j][1] : fE[j][0]) / mu.fiso;
        }
    });
    /* phase 3: the allocation over x = F / F0 */
    Real lam = 0, tq = 0;
    if (lane < ND) {
        lam = a.row_weight ? a.row_weight[lane] : Real(1);
        tq = GAT(a.tau, (size_t)idx * ND + lane, (size_t)a.n * ND);
    }
    Real xv[MPL];
    const int status = box_qp_solve<T, Real>(SM, lds, lane, mi, lam, tq, xv);
    if (lane == 0 && a.status) a.status[idx] = status;
    /* phase 4: the excitation of each slot's force */
    sfor<0, MPL>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const int s = lane + j * G;
        if (mi[j] < NM) {
            const SMuscle<Real> &mu = SM.mus[mi[j]];
            const size_t row = (size_t)idx * NM + mi[j];
            const Real xl = lds[SL::LO + s], xh = lds[SL::HI + s];
            const bool up = fE[j][0] <= fE[j][1];
            const bool atlo = !(xv[j] > xl), athi = !atlo && !(xv[j] < xh);
            /* at a bound (an empty range included): that end of the bracket, its force and its end state */
            const bool hiend = atlo ? !up : up;
            Real be = hiend ? eE[j][1] : eE[j][0], bf = hiend ? fE[j][1] : fE[j][0];
            Real ba = hiend ? aE[j][1] : aE[j][0], bl = hiend ? lE[j][1] : lE[j][0];
            Real Fs = bf;
            int rs = 0;
            if (!atlo && !athi) {
                Fs = xv[j] * mu.fiso;
                const Real tolF = a.ftol * mu.fiso;
                Real ea = eE[j][0], eb = eE[j][1], ga = fE[j][0] - Fs, gb = fE[j][1] - Fs, bg = 0;
                int ev = 0, side = 0;
                rs = -1;
                while (ev < a.max_iter) {
                    Real ec = eb - gb * (eb - ea) / (gb - ga);
                    ec = (ec > ea && ec < eb) ? ec : Real(0.5) * (ea + eb);
                    Real ae, le;
                    const Real fc = cmc_predict<T, Real>(SM, mu, a0[j], l0[j], L0[j], L1[j], ec, h, a.nsub, ae, le);
                    const Real gc = fc - Fs, ag = fabs(gc);
                    ++ev;
                    if (ev == 1 || ag < bg) { be = ec; bf = fc; ba = ae; bl = le; bg = ag; }
                    if (ag <= tolF) { rs = ev; break; }
                    if ((gc < Real(0)) == (gb < Real(0))) {
                        eb = ec; gb = gc;
                        ga = side == 1 ? Real(0.5) * ga : ga;
                        side = 1;
                    } else {
                        ea = ec; ga = gc;
                        gb = side == -1 ? Real(0.5) * gb : gb;
                        side = -1;
                    }
                }
            }
            GAT(a.excitation, row, rows) = be;
            if (a.force) GAT(a.force, row, rows) = Fs;
            if (a.predicted) GAT(a.predicted, row, rows) = bf;
            if (a.state_end) {
                Real *se = a.state_end + GIDX(row * 2, rows * 2);
                se[0] = ba; se[1] = bl;
            }
            if (a.root_status) a.root_status[GIDX(row, rows)] = rs;
        }
    });
    /* tau_muscle = B x, residual = tau - tau_muscle by dof */
    if (lane < ND && (a.residual || a.tau_muscle)) {
        Real sum = 0;
#pragma unroll
        for (int i = 0; i < T::MAXARM; ++i) {
            const int src = SM.tau_src[lane][i];
            const int sx = src / NSP < NM ? src / NSP : NM - 1;
            sum += lds[SL::BS + src] * lds[SL::X + sx];
        }
        if (a.tau_muscle) GAT(a.tau_muscle, (size_t)idx * ND + lane, (size_t)a.n * ND) = sum;
        if (a.residual) GAT(a.residual, (size_t)idx * ND + lane, (size_t)a.n * ND) = tq - sum;
    }
}

/* ------------------------------------------------------ inverse kinematics
 * bioim_ik_solve (include/bioim.h): per frame the coordinates that bring the
 * model's markers closest to the measured ones,
 *     min sum_i w_i |x_i(q) - xe_i|^2 + sum_d c_d (q_d - qt_d)^2,
 * x_i = o_b + R_b loc_i on the marker's composite body.  fp64 only.
 *
 * ma_kernel's launch shape (one frame per G lanes, the model image in LDS).
 * One loop body serves every evaluation: the kinematics prologue at a trial q
 * (frames KB and ground-frame Plucker columns S), then the marker pass: lane
 * l takes the markers l, l + G, ... (tables and measurements from global
 * memory), forms x_i, the residual r_i and the rows J_id = Omega_d x x_i + V_d
 * (exact 0 where dof d is not on the body's root chain, SM.dofmask) and adds
 * w_i J_id . J_ie, w_i J_id . r_i and w_i |r_i|^2 to its own partial sums in
 * registers; a fixed xor butterfly over the G lanes then leaves the entries
 * of the packed lower A = J^T W J + C, of g = J^T W r + C (q - qt) and f in
 * every lane, so no nm x ndof Jacobian and no per-marker array is stored (nm
 * is bounded by BIOIM_IK_MAX_MARKERS only).  The sums of all entries at once
 * do not fit the registers of the 14-dof models: the rows of A are taken in
 * IkLay::NBLK blocks, one marker pass each.  With float_origin the frames sit
 * in a ground frame shifted by x0 = pelvis_tx, which moves with every trial
 * q: the measured point is shifted with it, and the columns are the
 * world-frame derivatives at the shifted point.
 *
 * Solver (the rule of include/bioim.h): damped Gauss-Newton.  mu starts at
 * 1e-3 max diag A.  Each iteration solves (A + mu I) dq = -g by so_kernel's
 * Cholesky factorization in LDS (g as row ND), evaluates at q + dq, and
 * accepts if f_new <= f (1 + 64 eps) or max |dq| <= tol: then either returns
 * (max |dq| <= tol) or takes the A and g of the new point and mu / 4; a
 * rejected step keeps A and g and retries with 8 mu.  A and g of the last
 * accepted point live in the frame's MP / RHS slots (the dynamics' system
 * matrix and right-hand side, which the kinematics prologue never writes);
 * the union region behind Lay::U is overwritten by every prologue and holds
 * only the factorization's work area (IkLay), between one evaluation and the
 * next prologue; q, f, mu, the step and the iteration count stay in
 * registers.  When the solve ends, one more prologue and marker pass at the
 * returned q writes the outputs.
 *
 * The 4 frames of a wave need different iteration counts: every lane loops
 * under its own frame's state (uniform over the frame's G lanes); only
 * wave_sync orders the LDS traffic, and no workgroup barrier follows the
 * idx >= n exit.  No atomics, sums in a fixed order: a frame's result does
 * not depend on n or its neighbours. */
template <typename P> struct IkFields {   /* bioim_ik_solve (fp64 only) */
    int n, nm, max_iter;
    const int32_t *marker_body;
    const P *marker_loc, *weight, *x_exp, *q0, *coord_weight, *q_target;
    double tol;
    P *q, *markers, *err, *jacobian;
    int32_t *status;
};

/* the blocks of rows of A the marker passes take one at a time (the partial
 * sums of all NP + ND entries at once do not fit the registers of the 14-dof
 * models), and the solver's map of the union region: free from the last
 * kin_column to the next prologue, which is when the factorization runs */
template <class T, typename Real> struct IkLay {
    using LY = Lay<T, Real>;
    static constexpr int ND = LY::ND, NP = LY::NP;
    static constexpr int row0(int c) {
        return c <= 0 ? 0 : (c == 1 ? ND / 2 : (c == 2 ? (ND * 7 + 5) / 10 : (c == 3 ? (ND * 13 + 7) / 15 : ND)));
    }
    static constexpr int NBLK = 4;
    static constexpr int W = LY::U;            /* [NP + ND] A + mu I, then its factor; row ND: g, then L^-1 g */
    static constexpr int D = W + NP + ND;      /* [ND] reciprocal pivots */
    static constexpr int Z = D + ND;           /* [ND] z = -dq           */
    static constexpr int END = Z + ND;
    static_assert(row0(1) > 0 && row0(1) <= row0(2) && row0(2) <= row0(3) && row0(3) <= ND, "row blocks in order");
    static_assert(END <= LY::SIZE0, "the solver's data must fit in the union region");
};

template <class T, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void ik_kernel(ModelArgs<T, Real> md, IkFields<Real> a) {
    using LY = Lay<T, Real>;
    using PL = Planar<T>;
    using IK = IkLay<T, Real>;
    constexpr int G = T::G, ND = LY::ND, NP = LY::NP, EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    static_assert(LY::RHS == LY::MP + NP, "g is row ND of the packed matrix");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    const int nm = a.nm, max_iter = a.max_iter;
    const Real tol = a.tol;
    const size_t rows = (size_t)a.n * nm;
    /* dof lanes: the accepted iterate, the trial point, the coordinate task */
    Real qa = 0, qt = 0, cw = 0, qg = 0;
    if (lane < ND) {
        qa = GAT(a.q0, (size_t)idx * ND + lane, (size_t)a.n * ND);
        if (a.coord_weight) {
            cw = a.coord_weight[lane];
            qg = GAT(a.q_target, (size_t)idx * ND + lane, (size_t)a.n * ND);
        }
    }
    qt = qa;
    Real f = 0, mu = 0, step = 0;
    int it = 0, status = 0;
    bool first = true, fin = max_iter == 0;
    /* marker i at the frames in LDS: its point x (shifted ground frame), the
     * residual r and weight ww (0, 0: left out), the dofs on its root chain */
    auto marker_eval = [&](int i, Real x0, Real (&x)[3], Real (&r)[3], Real &ww, unsigned &dm) {
        const int b = a.marker_body[i];
        const Real w = a.weight[i];
        Real loc[3], xe[3], K[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            loc[k] = a.marker_loc[3 * i + k];
            xe[k] = GAT(a.x_exp, ((size_t)idx * nm + i) * 3 + k, rows * 3);
        }
        const Real *kb = lds + LY::KB + 18 * b;
#pragma unroll
        for (int k = 0; k < 12; ++k) K[k] = kb[k];
        PL::rot(K);
        mv3(K, loc, x);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] += K[9 + k];
        /* a gap in the measurement (NaN) or no weight: the marker is left out */
        const bool used = xe[0] == xe[0] && xe[1] == xe[1] && xe[2] == xe[2] && w > Real(0);
        ww = used ? w : Real(0);
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = used ? x[k] - xe[k] + (k == 0 ? x0 : Real(0)) : Real(0);
        dm = SM.dofmask[b];
    };
    /* row d of the marker's Jacobian from dof d's column */
    auto jac_row = [&](auto dI, const Real (&x)[3], unsigned dm, Real (&Jd)[3]) {
        constexpr int d = decltype(dI)::value;
        Real sc[6], t[3];
        /* spatial models: an opaque offset, so the columns are read again per
         * marker instead of hoisted out of the marker loop into 6 ND registers
         * (the 14-dof kernels otherwise spill) */
        int so = LY::S + 6 * d;
        if constexpr (!T::PLANAR) asm volatile("" : "+v"(so));
#pragma unroll
        for (int k = 0; k < 6; ++k) sc[k] = lds[so + k];
        PL::col(sc);
        cross3(sc, x, t);
        const bool on = (dm >> d) & 1u;
#pragma unroll
        for (int k = 0; k < 3; ++k) Jd[k] = on ? t[k] + sc[3 + k] : Real(0);
    };
    while (true) {
        /* the kinematics prologue at the trial point */
        const Real x0 = state_kinematics<BfSwitch<T>::FN, T, Real>(M, SM, lds, lane, qt, Real(0));
        wave_sync();   /* frames and columns are out; the union region (LOC / SL) is free until the next prologue */
        if (fin) {
            /* the outputs at the returned q */
            Real fm = 0, sw = 0, dmax = 0;
            for (int i = lane; i < nm; i += G) {
                Real x[3], r[3], ww;
                unsigned dm;
                marker_eval(i, x0, x, r, ww, dm);
                const Real rr = dot3(r, r);
                fm += ww * rr;
                sw += ww;
                dmax = rr > dmax ? rr : dmax;
                if (a.markers) {
                    Real *mo = a.markers + GIDX(((size_t)idx * nm + i) * 3, rows * 3);
                    mo[0] = x[0] + x0; mo[1] = x[1]; mo[2] = x[2];
                }
                if (a.jacobian) {
                    Real *jo = a.jacobian + GIDX(((size_t)idx * nm + i) * 3 * ND, rows * 3 * ND);
                    sfor<0, ND>([&](auto dI) {
                        constexpr int d = decltype(dI)::value;
                        Real Jd[3];
                        jac_row(dI, x, dm, Jd);
                        jo[d] = Jd[0]; jo[ND + d] = Jd[1]; jo[2 * ND + d] = Jd[2];
                    });
                }
            }
            fm = group_sum<G>(fm);
            sw = group_sum<G>(sw);
            dmax = group_max<G>(dmax);
            if (a.err && lane == 0) {
                Real *eo = a.err + GIDX((size_t)idx * 2, (size_t)a.n * 2);
                eo[0] = sw > Real(0) ? sqrt(fm / sw) : Real(0);
                eo[1] = sqrt(dmax);
            }
            break;
        }
        /* the marker passes, one per block of rows of A (IkLay::row0): the
         * lane's partial sums of the block's entries and of its g entries, the
         * butterfly, then the entries to MP / RHS.  The first block also sums f
         * and decides on the step, so a rejected step stops after it and leaves
         * A and g of the accepted point where they are */
        const Real dqt = qt - qg;
        bool accept = false, conv = false;
        sfor<0, IK::NBLK>([&](auto cI) {
            constexpr int c = decltype(cI)::value;
            constexpr int r0 = IK::row0(c), r1 = IK::row0(c + 1);
            constexpr int e0 = r0 * (r0 + 1) / 2, NE = r1 * (r1 + 1) / 2 - e0, NR = r1 - r0;
            if (c > 0 && !(accept && !conv)) return;
            Real acc[NE + NR];
            sfor<0, NE + NR>([&](auto kI) { acc[decltype(kI)::value] = 0; });
            Real fm = 0;
            for (int i = lane; i < nm; i += G) {
                Real x[3], r[3], ww, J[r1][3];
                unsigned dm;
                marker_eval(i, x0, x, r, ww, dm);
                if constexpr (c == 0) fm += ww * dot3(r, r);
                sfor<0, r1>([&](auto dI) { jac_row(dI, x, dm, J[decltype(dI)::value]); });
                sfor<r0, r1>([&](auto dI) {
                    constexpr int d = decltype(dI)::value;
                    const Real wj[3] = {ww * J[d][0], ww * J[d][1], ww * J[d][2]};
                    sfor<0, d + 1>([&](auto eI) {
                        constexpr int e = decltype(eI)::value;
                        acc[d * (d + 1) / 2 + e - e0] += dot3(wj, J[e]);
                    });
                    acc[NE + d - r0] += dot3(wj, r);
                });
            }
            /* the coordinate tasks (dof lane d: its own diagonal entry) */
            sfor<r0, r1>([&](auto dI) {
                constexpr int d = decltype(dI)::value;
                acc[d * (d + 1) / 2 + d - e0] += lane == d ? cw : Real(0);
                acc[NE + d - r0] += lane == d ? cw * dqt : Real(0);
            });
            sfor<0, NE + NR>([&](auto kI) {
                constexpr int k = decltype(kI)::value;
                acc[k] = group_sum<G>(acc[k]);
                if constexpr (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);   /* a few butterflies in flight, not all */
            });
            if constexpr (c == 0) {
                const Real fn = group_sum<G>(fm) + group_sum<G>(cw * dqt * dqt);
                if (first) {
                    accept = true;
                    if (!(fn == fn)) {   /* a NaN that came in */
                        status = -2;
                        fin = true;
                    }
                } else {
                    conv = step <= tol;
                    accept = fn <= f * (Real(1) + Real(64) * Real(2.220446049250313e-16)) || conv;
                }
                if (accept) {
                    qa = qt;
                    f = fn;
                    if (conv) {
                        status = it;
                        fin = true;
                    } else if (!first) {
                        mu *= Real(0.25);
                    }
                } else {
                    mu *= Real(8);
                }
            }
            if (accept && !conv) {
                sfor<0, NE>([&](auto kI) {
                    constexpr int k = decltype(kI)::value;
                    if (lane == k % G) lds[LY::MP + e0 + k] = acc[k];
                });
                sfor<0, NR>([&](auto kI) {
                    constexpr int k = decltype(kI)::value;
                    if (lane == (NE + k) % G) lds[LY::RHS + r0 + k] = acc[NE + k];
                });
            }
        });
        wave_sync();
        if (first) {
            const Real dg = lane < ND ? lds[LY::MP + lane * (lane + 1) / 2 + lane] : Real(0);
            mu = Real(1e-3) * group_max<G>(dg);
            first = false;
        }
        if (!fin) {
            if (it >= max_iter) {
                status = -1;
                fin = true;
            } else {
                ++it;
                /* (A + mu I) dq = -g: the work copy (lane i: row i; row ND is g), then
                 * so_kernel's right-looking Cholesky on the frame's lanes; row ND
                 * comes out as L^-1 g */
                if (lane <= ND) {
                    const int o = lane * (lane + 1) / 2;
                    for (int j = 0; j <= (lane < ND ? lane : ND - 1); ++j)
                        lds[IK::W + o + j] = lds[LY::MP + o + j] + ((j == lane) ? mu : Real(0));
                }
                wave_sync();
                bool ok = true;
                for (int k = 0; k < ND && ok; ++k) {
                    const Real piv = lds[IK::W + k * (k + 1) / 2 + k];
                    ok = piv > Real(0);
                    if (ok) {
                        const Real rp = Real(1) / sqrt(piv);
                        for (int i = k + 1 + lane; i <= ND; i += G) lds[IK::W + i * (i + 1) / 2 + k] *= rp;
                        if (lane == 0) lds[IK::D + k] = rp;
                        wave_sync();
                        for (int i = k + 1 + lane; i <= ND; i += G) {
                            Real *ri = lds + IK::W + i * (i + 1) / 2;
                            const Real lik = ri[k];
                            const int je = i < ND ? i : ND - 1;
                            for (int jc = k + 1; jc <= je; ++jc) ri[jc] -= lik * lds[IK::W + jc * (jc + 1) / 2 + k];
                        }
                        wave_sync();
                    }
                }
                Real dqd = 0;
                if (ok) {
                    /* L^T z = y, last row first; dq = -z */
                    for (int k = ND - 1; k >= 0; --k) {
                        const Real zk = lds[IK::W + NP + k] * lds[IK::D + k];
                        const Real *rk = lds + IK::W + k * (k + 1) / 2;
                        for (int i = lane; i < k; i += G) lds[IK::W + NP + i] -= rk[i] * zk;
                        if (lane == 0) lds[IK::Z + k] = zk;
                        wave_sync();
                    }
                    dqd = lane < ND ? -lds[IK::Z + lane] : Real(0);
                }
                const bool bad = group_max<G>((dqd == dqd) ? Real(0) : Real(1)) > Real(0);
                if (!ok || bad) {   /* a pivot <= 0, or a NaN that came in */
                    status = -2;
                    fin = true;
                } else {
                    step = group_max<G>(fabs(dqd));
                    qt = qa + dqd;
                }
            }
        }
        if (fin) qt = qa;
        wave_sync();
    }
    if (lane < ND) GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND) = qa;
    if (lane == 0 && a.status) a.status[idx] = status;
}

/* --------------------------------------------------------- joint reaction
 * bioim_joint_reaction (include/bioim.h): per state the wrench every
 * composite body's inboard joint carries.  ma_kernel's launch shape (one
 * state per G lanes, the model image in LDS) and id_kernel's prologue up to
 * body_inertia, which leaves the un-summed spatial inertias I_k (IC) and the
 * velocity-product + gravity wrenches (WB) about the shifted origin.  Then
 *   body lane k:   W_k = I_k (sum_{d on k's root path} S_d q''_d) + WB_k
 *                        - contact (CW of k's spheres) - ext_k - muscles_k,
 *   muscle lanes:  muscle_point_wrench sums each muscle's point forces per
 *                  body in registers; the per-body sums over the lanes are the
 *                  fixed butterfly of group_sum (6 NB sums), so every lane
 *                  holds every body's muscle wrench and lane k picks its own
 *                  (moments about o_k until then, shifted once),
 *   body lane b:   F_b = sum_{k in subtree(b)} W_k (T::anc, fixed order),
 *   outputs:       moment shifted to c_b, rotated into the requested frame;
 *                  tau_joint_d = S_d . F_cb(d).
 * Nothing is masked by Planar<T>: a planar model's out-of-plane components are
 * loads its joints carry.  The q'' are staged in the RHS slots (no mass matrix
 * is formed here); W_k and then F_b go to body k's own WB slot.  Every sum has
 * a fixed order, so a state's result depends on nothing else.
 * IO is the type of the caller's arrays (the handle's precision).  The model
 * image and all arithmetic are fp64 on either handle: the Hunt-Crossley force
 * turns 1e-7 m of a sphere's height into 0.1 N, and an fp32 kinematic chain
 * places the sphere no better than that, ten times what rounding the inputs
 * to fp32 costs.  An fp32 handle therefore gets a second, fp64 model image
 * on its first call (jr_fp64_model) and converts only at the kernel's loads
 * and stores. */
template <typename P> struct JrFields {   /* bioim_joint_reaction */
    int n, flags, frame;
    const P *q, *u, *qdd, *ft, *ext;
    P *reaction, *point, *tau_joint, *muscle_wrench;
};

/* The point forces of one muscle at tendon force Ft, summed per composite
 * body: wr[b] += ((P - o_b) x f, f) for every active path point on body b —
 * the moment about the body's own origin (lever arms of a segment's length,
 * not of the model's distance from the ground origin, which costs fp32 two
 * digits in sums that cancel); the caller shifts each body's sum once.
 * f = Ft (e_next - e_prev) = -Ft g in muscle_path's notation.  muscle_path's point loop and activity rule
 * (conditional points out of range are skipped, moving points sit at their
 * function values), without the moment arms; a moving point's g . dP/dq is a
 * mobility force and is not formed.  The body index is matched by selects, so
 * wr stays in registers. */
template <bool BFK, class T, typename Real>
DEV void muscle_point_wrench(const SModel<T, Real> &SM, const SMuscle<Real> &mu, const Real *lds, Real Ft,
                             Real (&wr)[T::NB][6]) {
    using LY = Lay<T, Real>;
    constexpr bool BF = BFK;
    const Real *ldsq = lds + LY::QF;
    Real Pp[3] = {0, 0, 0}, rp[3] = {0, 0, 0}, ep[3] = {0, 0, 0};
    int cbp = -1;
    bool have = false;
    auto flush = [&](const Real *g) {
        Real f[3] = {-Ft * g[0], -Ft * g[1], -Ft * g[2]}, mo[3];
        cross3(rp, f, mo);
        sfor<0, T::NB>([&](auto bI) {
            constexpr int b = decltype(bI)::value;
            const bool on = cbp == b;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                wr[b][i] += on ? mo[i] : Real(0);
                wr[b][3 + i] += on ? f[i] : Real(0);
            }
        });
    };
    const int npt = mu.npt;
    constexpr int MP = T::MAXPT > 0 ? T::MAXPT : 1;
    int cbj[MP];
    bool onj[MP];
    sfor<0, MP>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const DPathPt<Real> &pt = SM.pt[mu.pt_off + (j < npt ? j : 0)];
        cbj[j] = pt.cbody;
        onj[j] = j < npt;
        if constexpr (((T::PT_COND >> j) & 1u) != 0) {
            const bool cnd = pt.type == BIOIM_PT_COND;
            if constexpr (BF) {
                const int ccd = pt.cond_coord, zero = 0;
                const Real qc = ldsq[cnd ? ccd : zero], plo = pt.lo, phi = pt.hi;
                onj[j] = onj[j] & !(cnd & ((qc < plo) | (qc > phi)));
            } else {
                const Real qc = ldsq[cnd ? pt.cond_coord : 0];
                onj[j] = onj[j] && !(cnd && (qc < pt.lo || qc > pt.hi));
            }
        }
    });
    sfor<0, MP>([&](auto jI) {
        constexpr int j = decltype(jI)::value;
        const DPathPt<Real> &pt = SM.pt[mu.pt_off + (j < npt ? j : 0)];
        if (onj[j]) {
            Real loc[3] = {pt.loc[0], pt.loc[1], pt.loc[2]};
            if constexpr (((T::PT_MOVING >> j) & 1u) != 0) {
                if (pt.type == BIOIM_PT_MOVING) {
                    Real ll[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const int f = pt.mf[a];
                        ll[a] = f < 0 ? pt.loc[a] : lds[LY::MF + 3 * (f < 0 ? 0 : f)];
                    }
                    mv3(pt.R, ll, loc);
#pragma unroll
                    for (int i = 0; i < 3; ++i) loc[i] += pt.p[i];
                }
            }
            const Real *kbp = lds + LY::KB + 18 * cbj[j];
            Real Rb[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) Rb[i] = kbp[i];
            Real P[3], r[3];
            mv3(Rb, loc, r);
#pragma unroll
            for (int i = 0; i < 3; ++i) P[i] = r[i] + Rb[9 + i];
            Real e[3] = {0, 0, 0};
            if (have) {
                Real sgm[3] = {P[0] - Pp[0], P[1] - Pp[1], P[2] - Pp[2]};
                const Real l2 = dot3(sgm, sgm);
                const Real inv = fast_rsqrt(l2);
#pragma unroll
                for (int a = 0; a < 3; ++a) e[a] = sgm[a] * inv;
                Real g[3] = {ep[0] - e[0], ep[1] - e[1], ep[2] - e[2]};
                flush(g);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) { ep[a] = e[a]; Pp[a] = P[a]; rp[a] = r[a]; }
            cbp = cbj[j];
            have = true;
        }
    });
    if (have) flush(ep);
}

template <class T, typename IO>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void jr_kernel(ModelArgs<T, double> md, JrFields<IO> a) {
    using Real = double;
    using LY = Lay<T, Real>;
    constexpr int G = T::G, ND = LY::ND, NB = T::NB, NM = T::NM, EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    const bool contact = (a.flags & BIOIM_JR_CONTACT) != 0;
    Real qd = 0, ud = 0, ad = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = opt_row<Real, ND>(a.u, idx, lane, a.n);
        ad = opt_row<Real, ND>(a.qdd, idx, lane, a.n);
    }
    const Real x0 = state_kinematics<false, T, Real>(M, SM, lds, lane, qd, ud);
    if (lane < NB) body_inertia<T, Real>(SM, M, lds, lane);
    if (lane < ND) lds[LY::RHS + lane] = ad;
    wave_sync();   /* columns, inertias and wrenches are out; the joint-local region the CJ slots share is free */
    if (contact && lane < T::NS) contact_lane<false, T, Real>(SM, lds, lane, Real(0));
    /* the muscles' wrench on every body, in every lane (moment3, force3 about the shifted origin) */
    Real mw[NB][6];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 6; ++i) mw[b][i] = 0;
    if constexpr (NM > 0) {
        sfor<0, (NM + G - 1) / G>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            const int m = mslot<T>(lane + j * G);
            if (m < NM) {
                const Real Ft = a.ft ? GAT(a.ft, (size_t)idx * NM + m, (size_t)a.n * NM) : Real(0);
                muscle_point_wrench<false, T, Real>(SM, SM.mus[m], lds, Ft, mw);
            }
        });
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 6; ++i) mw[b][i] = group_sum<G>(mw[b][i]);
    }
    wave_sync();
    Real mk[6] = {0, 0, 0, 0, 0, 0}, W[6] = {0, 0, 0, 0, 0, 0};
    if (lane < NB) {
        sfor<0, NB>([&](auto bI) {
            constexpr int b = decltype(bI)::value;
#pragma unroll
            for (int i = 0; i < 6; ++i) mk[i] = lane == b ? mw[b][i] : mk[i];
        });
        {   /* from the body's own origin to the (shifted) ground origin */
            Real ts[3];
            cross3(lds + LY::KB + 18 * lane + 9, mk + 3, ts);
#pragma unroll
            for (int i = 0; i < 3; ++i) mk[i] += ts[i];
        }
        /* spatial acceleration of the q'' on k's root path, then I_k a (the I S form of id_kernel) */
        const unsigned dm = SM.dofmask[lane];
        Real acc[6] = {0, 0, 0, 0, 0, 0}, t[3];
        sfor<0, ND>([&](auto dI) {
            constexpr int d = decltype(dI)::value;
            const Real ddq = ((dm >> d) & 1u) ? lds[LY::RHS + d] : Real(0);
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[i] += lds[LY::S + 6 * d + i] * ddq;
        });
        const Real *ic = lds + LY::IC + 10 * lane, *wb = lds + LY::WB + 6 * lane;
        symv(ic + 4, acc, W);
        cross3(ic + 1, acc + 3, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) W[i] += t[i];
        cross3(acc, ic + 1, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) W[3 + i] = ic[0] * acc[3 + i] + t[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) W[i] += wb[i];
        if (contact) {
            sfor<0, T::NS>([&](auto sI) {
                constexpr int sp = decltype(sI)::value;
                const bool on = SM.sph_cb[sp] == lane;
                const Real *cw = lds + LY::CW + 8 * sp;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    W[i] -= on ? cw[3 + i] : Real(0);
                    W[3 + i] -= on ? cw[i] : Real(0);
                }
            });
        }
        {   /* ext: fx fy fz mx my mz about the true ground origin, which sits at (-x0, 0, 0) here */
            Real e[6] = {0, 0, 0, 0, 0, 0};
            if (a.ext) {
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    e[i] = GAT(a.ext, ((size_t)idx * NB + lane) * 6 + i, (size_t)a.n * NB * 6);
            }
            W[0] -= e[3];
            W[1] -= e[4] + x0 * e[2];
            W[2] -= e[5] - x0 * e[1];
#pragma unroll
            for (int i = 0; i < 3; ++i) W[3 + i] -= e[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) W[i] -= mk[i];
    }
    wave_sync();
    if (lane < NB) {
#pragma unroll
        for (int i = 0; i < 6; ++i) lds[LY::WB + 6 * lane + i] = W[i];
    }
    wave_sync();
    Real F[6] = {0, 0, 0, 0, 0, 0};
    if (lane < NB) {
        sfor<0, NB>([&](auto dI) {
            constexpr int d = decltype(dI)::value;
            if ((T::anc[d] >> lane) & 1u) {
#pragma unroll
                for (int i = 0; i < 6; ++i) F[i] += lds[LY::WB + 6 * d + i];
            }
        });
    }
    wave_sync();
    if (lane < NB) {
#pragma unroll
        for (int i = 0; i < 6; ++i) lds[LY::WB + 6 * lane + i] = F[i];
    }
    wave_sync();
    if (lane < NB) {
        const SBody<Real> &b = SM.body[lane];
        const Real *kb = lds + LY::KB + 18 * lane;
        /* c_b = o_b - R_b R_mb^T p_mb: the origin of the joint's child-side frame */
        Real pm[3], c[3], t[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) pm[i] = b.R_mb[i] * b.p_mb[0] + b.R_mb[3 + i] * b.p_mb[1] + b.R_mb[6 + i] * b.p_mb[2];
        mv3(kb, pm, c);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = kb[9 + i] - c[i];
        const size_t row = (size_t)idx * NB + lane, rows = (size_t)a.n * NB;
        if (a.point) {
            GAT(a.point, row * 3, rows * 3) = IO(c[0] + x0);
            GAT(a.point, row * 3 + 1, rows * 3) = IO(c[1]);
            GAT(a.point, row * 3 + 2, rows * 3) = IO(c[2]);
        }
        if (a.reaction) {
            Real f[3] = {F[3], F[4], F[5]}, mo[3];
            cross3(c, f, t);
#pragma unroll
            for (int i = 0; i < 3; ++i) mo[i] = F[i] - t[i];
            if (a.frame != BIOIM_JR_GROUND) {   /* ground -> frame: R^T */
                const Real *Rf = lds + LY::KB + 18 * (a.frame == BIOIM_JR_CHILD ? lane : b.pslot);
                Real fo[3], mq[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    fo[i] = Rf[i] * f[0] + Rf[3 + i] * f[1] + Rf[6 + i] * f[2];
                    mq[i] = Rf[i] * mo[0] + Rf[3 + i] * mo[1] + Rf[6 + i] * mo[2];
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) { f[i] = fo[i]; mo[i] = mq[i]; }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                GAT(a.reaction, row * 6 + i, rows * 6) = IO(f[i]);
                GAT(a.reaction, row * 6 + 3 + i, rows * 6) = IO(mo[i]);
            }
        }
        if (a.muscle_wrench) {   /* about the true ground origin: M + (x0, 0, 0) x f */
            GAT(a.muscle_wrench, row * 6, rows * 6) = IO(mk[3]);
            GAT(a.muscle_wrench, row * 6 + 1, rows * 6) = IO(mk[4]);
            GAT(a.muscle_wrench, row * 6 + 2, rows * 6) = IO(mk[5]);
            GAT(a.muscle_wrench, row * 6 + 3, rows * 6) = IO(mk[0]);
            GAT(a.muscle_wrench, row * 6 + 4, rows * 6) = IO(mk[1] - x0 * mk[5]);
            GAT(a.muscle_wrench, row * 6 + 5, rows * 6) = IO(mk[2] + x0 * mk[4]);
        }
    }
    if (a.tau_joint && lane < ND) {
        const Real *Sd = lds + LY::S + 6 * lane, *Fb = lds + LY::WB + 6 * SM.dof_cb[lane];
        GAT(a.tau_joint, (size_t)idx * ND + lane, (size_t)a.n * ND) = IO(dot3(Sd, Fb) + dot3(Sd + 3, Fb + 3));
    }
}

/* ---------------------------------------------------- induced accelerations
 * bioim_induced_accel (include/bioim.h): per state the share of every
 * coordinate's acceleration, of the mass centre's acceleration and of every
 * foot's ground reaction that is due to gravity, to the velocity terms, to each
 * contact force, the limit forces, the caller's actuator and external forces,
 * and to each single muscle: one column per contributor, the last their total.
 * fp64 only (M^-1 and a Schur complement on a floating base).
 *
 * The other analysis kernels' shape: one state per G lanes, the model image in
 * LDS, then the env regions of Lay (unchanged), then this kernel's private
 * tail (IaLay), one per state.  The tail does not fit beside 16 env regions on
 * the spatial muscle topologies, so IaLay::EPB states share a workgroup: 16
 * where that fits into 160 KiB, 8 elsewhere.
 *   1. id_kernel's prologue through body_inertia; body lanes split the
 *      gravity wrench off WB (WG) and stage ext (XW, moved to the shifted
 *      origin, jr_kernel's form); subtree sums of IC, WB, WG, XW, and the mass
 *      centre's velocity-product acceleration sum_b m_b ac_b (lane NB);
 *      contact_lane at h = 0, the limit lanes, the packed M.
 *   2. POINT: foot lane f decides (cactive / cpoint, or sum fn_s > threshold
 *      and P_f = sum fn_s P_s / sum fn_s over its active spheres, sphere order).
 *   3. Dof lane d writes entry d of the gravity, velocity, contact, limit,
 *      actuator and external columns and of the J rows; muscle lanes run
 *      muscle_path by mslot and write their own column -Ft dL/dq; foot lanes
 *      form beta_f.  Then the total column (fixed order).
 *   4. M = L L^T in place in LDS (so_kernel's right-looking form on the lanes);
 *      lane l substitutes the columns l, l + G, ... (the J^T columns too: Y),
 *      reading L by broadcast.
 *   5. POINT: S = J Y (+ identity on the rows of feet not held), its Cholesky
 *      on lane 0, then per column lambda = -S^-1 (J A + beta), A += Y lambda.
 *   6. com_accel per column from J_com (subtree mass and first moment times
 *      the Plucker columns), then the stores; accel is one contiguous copy.
 * A pivot <= 0 or a NaN (M, S, or the total column) gives status -2 and zero
 * outputs.  No atomics, no shared slot written at a run-time index (a lane
 * writes only columns it owns), every sum in a fixed order. */
template <typename P> struct IaFields {   /* bioim_induced_accel (fp64 only) */
    int n, kind;
    double thr;
    const P *q, *u, *ft, *tau_act, *ext, *cpoint;
    const uint8_t *cactive;
    P *accel, *com_accel, *reaction, *cpoint_out;
    uint8_t *cactive_out;
    int32_t *status;
};

template <class T, typename Real> struct IaLay {
    using LY = Lay<T, Real>;
    static constexpr int ND = LY::ND, NB = T::NB, NF = T::NF, NM = T::NM;
    static constexpr int NCOL = 6 + NF + NM;         /* contributors (include/bioim.h order)          */
    static constexpr int NR = T::PLANAR ? 2 : 3;     /* constraint rows per foot                      */
    static constexpr int NJ = NF * NR, NX = NCOL + NJ;
    static constexpr int COL = 0;                    /* [NX][ND]: Q_c then A_c; rows NCOL..: J^T then Y */
    static constexpr int D = COL + NX * ND;          /* [ND] reciprocal pivots of M                   */
    static constexpr int JR = D + ND;                /* [NJ][ND] J rows                               */
    static constexpr int SS = JR + NJ * ND;          /* [NJ][NJ] S, then its factor (lower)           */
    static constexpr int SD = SS + NJ * NJ;          /* [NJ] reciprocal pivots of S                   */
    static constexpr int BETA = SD + NJ;             /* [NJ]                                          */
    static constexpr int WG = BETA + NJ;             /* [NB][6] gravity wrenches; in place: subtree sums */
    static constexpr int XW = WG + 6 * NB;           /* [NB][6] ext wrenches; in place: subtree sums  */
    static constexpr int JC = XW + 6 * NB;           /* [3][ND] mass-centre Jacobian                  */
    static constexpr int CB = JC + 3 * ND;           /* [3] sum m_b ac_b, [1] total mass              */
    static constexpr int PF = CB + 4;                /* [NF][4]: P_f (shifted origin), held (0 / 1)   */
    static constexpr int FLAG = PF + 4 * NF;         /* [1] S factored (0 / 1)                        */
    static constexpr int SIZE = ((FLAG + 1 + 1) / 2) * 2;
    static constexpr size_t bytes(int epb) {
        return smodel_bytes<T, Real>() + (size_t)epb * (LY::SIZE + SIZE) * sizeof(Real);
    }
    static constexpr int EPB = bytes(BIOIM_EPB) <= 163840 ? BIOIM_EPB : BIOIM_EPB / 2;
    static constexpr size_t lds_bytes = bytes(EPB);
    static_assert(lds_bytes <= 163840, "LDS image + env regions + induced-acceleration tails exceed 160 KiB");
    /* the composite body that carries force f's spheres */
    static constexpr int foot_cb(int f) {
        for (int s = 0; s < T::NS; ++s)
            if (T::sphere_force[s] == f) return T::sphere_cb[s];
        return 0;
    }
    static constexpr bool one_body_per_force() {
        for (int s = 0; s < T::NS; ++s)
            if (T::sphere_cb[s] != foot_cb(T::sphere_force[s])) return false;
        return true;
    }
    static_assert(one_body_per_force(), "a contact force's spheres sit on one composite body");
};

template <class T, typename Real>
__global__ __launch_bounds__((IaLay<T, Real>::EPB * T::G)) __attribute__((amdgpu_waves_per_eu(1, 1))) void ia_kernel(ModelArgs<T, Real> md, IaFields<Real> a) {
    using LY = Lay<T, Real>;
    using IA = IaLay<T, Real>;
    using PL = Planar<T>;
    using SW = BfSwitch<T>;
    constexpr int G = T::G, ND = LY::ND, NB = T::NB, NM = T::NM, NF = T::NF, EPB = IA::EPB;
    constexpr int NCOL = IA::NCOL, NR = IA::NR, NJ = IA::NJ;
    constexpr int C_CON = 2, C_LIM = 2 + NF, C_ACT = 3 + NF, C_EXT = 4 + NF, C_MUS = 5 + NF, C_TOT = NCOL - 1;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    static_assert(NB < G && NF <= G && NJ <= G, "body, foot and constraint-row lanes");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    Real *tl = reinterpret_cast<Real *>(smem_raw + SMB) + EPB * LY::SIZE + slot * IA::SIZE;
    const bool point = a.kind == BIOIM_IA_POINT;
    Real qd = 0, ud = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = opt_row<Real, ND>(a.u, idx, lane, a.n);
    }
    const Real x0 = state_kinematics<(NM > 0 ? SW::FN : false), T, Real>(M, SM, lds, lane, qd, ud);
    if (lane < NB) {
        body_inertia<T, Real>(SM, M, lds, lane);
        /* the gravity wrench out of WB into WG; ext about the shifted origin into XW */
        gravity_wrench_out<true, T, Real>(M, SM, lds, lane, tl + IA::WG + 6 * lane);
        Real *xw = tl + IA::XW + 6 * lane;
        Real e[6] = {0, 0, 0, 0, 0, 0};
        if (a.ext) {
#pragma unroll
            for (int i = 0; i < 6; ++i) e[i] = GAT(a.ext, ((size_t)idx * NB + lane) * 6 + i, (size_t)a.n * NB * 6);
        }
        xw[0] = e[3];
        xw[1] = e[4] + x0 * e[2];
        xw[2] = e[5] - x0 * e[1];
#pragma unroll
        for (int i = 0; i < 3; ++i) xw[3 + i] = e[i];
    }
    wave_sync();
    {   /* subtree sums (all reads, then all writes); lane NB: sum_b m_b ac_b and the total mass */
        Real ic[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, wb[6] = {0, 0, 0, 0, 0, 0}, wg[6] = {0, 0, 0, 0, 0, 0};
        Real xw[6] = {0, 0, 0, 0, 0, 0}, cb[4] = {0, 0, 0, 0};
        if (lane < NB) {
            sfor<0, NB>([&](auto dI) {
                constexpr int d = decltype(dI)::value;
                if ((T::anc[d] >> lane) & 1u) {
#pragma unroll
                    for (int i = 0; i < 10; ++i) ic[i] += lds[LY::IC + 10 * d + i];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        wb[i] += lds[LY::WB + 6 * d + i];
                        wg[i] += tl[IA::WG + 6 * d + i];
                        xw[i] += tl[IA::XW + 6 * d + i];
                    }
                }
            });
        } else if (lane == NB) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
#pragma unroll
                for (int i = 0; i < 3; ++i) cb[i] += lds[LY::WB + 6 * b + 3 + i];
                cb[3] += lds[LY::IC + 10 * b];
            }
        }
        wave_sync();
        if (lane < NB) {
#pragma unroll
            for (int i = 0; i < 10; ++i) lds[LY::IC + 10 * lane + i] = ic[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                lds[LY::WB + 6 * lane + i] = wb[i];
                tl[IA::WG + 6 * lane + i] = wg[i];
                tl[IA::XW + 6 * lane + i] = xw[i];
            }
        } else if (lane == NB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) tl[IA::CB + i] = cb[i];
        }
    }
    if (lane < T::NS) contact_lane<false, T, Real>(SM, lds, lane, Real(0));
    if (lane < T::NL) {
        const int cc = SM.lim_coord[lane];
        const Real qv = lds[LY::QF + cc], qdv = lds[LY::UF + cc];
        const Real qup = SM.lim_qup[lane], qlo = SM.lim_qlow[lane], tr = SM.lim_trans[lane];
        const Real itr = SM.lim_itrans[lane];
        const Real up = smooth_step<false>(Real(0), Real(1), qup, qup + tr, itr, qv);
        const Real lo = smooth_step<false>(Real(1), Real(0), qlo - tr, qlo, itr, qv);
        lds[LY::LIM + 4 * lane] = -SM.lim_kup[lane] * up * (qv - qup) + SM.lim_klow[lane] * lo * (qlo - qv) -
                                  SM.lim_damp[lane] * (up + lo) * qdv;
    }
    wave_sync();
    if (lane < ND) {   /* row lane of the packed lower M (id_kernel's form) */
        const Real *Sd = lds + LY::S + 6 * lane, *ic = lds + LY::IC + 10 * SM.dof_cb[lane];
        Real Gk[6], t[3];
        symv(ic + 4, Sd, Gk);
        cross3(ic + 1, Sd + 3, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) Gk[i] += t[i];
        cross3(Sd, ic + 1, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) Gk[3 + i] = ic[0] * Sd[3 + i] + t[i];
        unsigned path = 0;
        sfor<0, ND>([&](auto kI) {
            constexpr int k = decltype(kI)::value;
            constexpr unsigned pm = DofTree<T>::path_mask(k);
            path = lane == k ? pm : path;
        });
        Real *row = lds + LY::MP + (lane * (lane + 1)) / 2;
        sfor<0, ND>([&](auto lI) {
            constexpr int l = decltype(lI)::value;
            if (l <= lane) {
                const Real *Sl = lds + LY::S + 6 * l;
                row[l] = ((path >> l) & 1u) ? dot3(Sl, Gk) + dot3(Sl + 3, Gk + 3) : Real(0);
            }
        });
        /* mass-centre Jacobian column: (Omega_d x h + m V_d) / m_total over the subtree dof d moves */
        Real jc[3];
        cross3(Sd, ic + 1, jc);
        const Real im = Real(1) / tl[IA::CB + 3];
#pragma unroll
        for (int i = 0; i < 3; ++i) tl[IA::JC + i * ND + lane] = (jc[i] + ic[0] * Sd[3 + i]) * im;
    }
    if (lane < NF) {   /* which feet are held, and where */
        Real fs = 0, Ps[3] = {0, 0, 0};
        sfor<0, T::NS>([&](auto sI) {
            constexpr int sp = decltype(sI)::value;
            const bool on = T::sphere_force[sp] == lane && lds[LY::CW + 8 * sp + 6] > 0;
            const Real fnv = lds[LY::CW + 8 * sp + 1];
            const Real fn = on ? fnv : Real(0);
            fs += fn;
#pragma unroll
            for (int i = 0; i < 3; ++i) Ps[i] += fn * lds[LY::CJ + LY::CJN * sp + i];
        });
        bool held = false;
        Real Pf[3] = {0, 0, 0};
        if (point) {
            if (a.cactive) {
                held = GAT(a.cactive, (size_t)idx * NF + lane, (size_t)a.n * NF) != 0;
#pragma unroll
                for (int i = 0; i < 3; ++i) Pf[i] = GAT(a.cpoint, ((size_t)idx * NF + lane) * 3 + i, (size_t)a.n * NF * 3);
                Pf[0] -= x0;
            } else {
                held = fs > a.thr;
                const Real inv = Real(1) / (held ? fs : Real(1));
#pragma unroll
                for (int i = 0; i < 3; ++i) Pf[i] = Ps[i] * inv;
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) tl[IA::PF + 4 * lane + i] = held ? Pf[i] : Real(0);
        tl[IA::PF + 4 * lane + 3] = held ? Real(1) : Real(0);
    }
    wave_sync();   /* M, J_com, the feet; CW / CJ / LIM are out */
    if (lane < ND) {
        const Real *Sd = lds + LY::S + 6 * lane;
        const int cb = SM.dof_cb[lane];
        const Real *wb = lds + LY::WB + 6 * cb, *wg = tl + IA::WG + 6 * cb, *xw = tl + IA::XW + 6 * cb;
        Real *col = tl + IA::COL + lane;
        col[0] = dot3(Sd, wg) + dot3(Sd + 3, wg + 3);
        col[ND] = -(dot3(Sd, wb) + dot3(Sd + 3, wb + 3));
        Real fc[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) fc[f] = 0;
        sfor<0, T::NS>([&](auto sI) {
            constexpr int sp = decltype(sI)::value;
            constexpr unsigned msk = T::dofmask[T::sphere_cb[sp]];
            const Real *cj = lds + LY::CJ + LY::CJN * sp;
            Real jd[3];
            contact_jac(Sd, cj, jd);
            const Real term = dot3(jd, cj + 3);
            fc[T::sphere_force[sp]] += (lds[LY::CW + 8 * sp + 6] > 0 && ((msk >> lane) & 1u)) ? term : Real(0);
        });
        sfor<0, NF>([&](auto fI) {
            constexpr int f = decltype(fI)::value;
            constexpr unsigned msk = T::dofmask[IA::foot_cb(f)];
            const bool held = tl[IA::PF + 4 * f + 3] > 0;
            col[(C_CON + f) * ND] = held ? Real(0) : fc[f];
            /* J_f: (Omega_d x P_f + V_d) over the dofs that move the foot */
            Real sc[6], jd[3];
#pragma unroll
            for (int i = 0; i < 6; ++i) sc[i] = Sd[i];
            PL::col(sc);
            contact_jac(sc, tl + IA::PF + 4 * f, jd);
            const bool on = held && ((msk >> lane) & 1u);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const Real v = on ? jd[r] : Real(0);
                tl[IA::JR + (f * NR + r) * ND + lane] = v;
                col[(NCOL + f * NR + r) * ND] = v;
            }
        });
        Real lim = 0;
#pragma unroll
        for (int li = 0; li < T::NL; ++li)
            if (SM.lim_dof[li] == lane) lim += lds[LY::LIM + 4 * li];
        col[C_LIM * ND] = lim;
        col[C_ACT * ND] = opt_row<Real, ND>(a.tau_act, idx, lane, a.n);
        col[C_EXT * ND] = dot3(Sd, xw) + dot3(Sd + 3, xw + 3);
    }
    if (lane < NF) {
        /* beta_f: the acceleration of the body-fixed point at P_f along q + u t,
         * aO + alpha x P + w x (vO + w x P) of the foot's body */
        int fb = 0;
        sfor<0, NF>([&](auto fI) {
            constexpr int f = decltype(fI)::value;
            fb = lane == f ? IA::foot_cb(f) : fb;
        });
        Real K[18], A[6], P[3], t[3], v[3], t2[3];
#pragma unroll
        for (int i = 0; i < 18; ++i) K[i] = lds[LY::KB + 18 * fb + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i] = lds[LY::AL + 6 * fb + i];
        PL::frame(K); PL::acc(A);
#pragma unroll
        for (int i = 0; i < 3; ++i) P[i] = tl[IA::PF + 4 * lane + i];
        const bool held = tl[IA::PF + 4 * lane + 3] > 0;
        cross3(K + 12, P, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = K[15 + i] + t[i];
        cross3(A, P, t);
        cross3(K + 12, v, t2);
#pragma unroll
        for (int r = 0; r < NR; ++r) tl[IA::BETA + lane * NR + r] = held ? A[3 + r] + t[r] + t2[r] : Real(0);
    }
    if constexpr (NM > 0) {
        constexpr int NSP = T::MAXSPAN;
        sfor<0, (NM + G - 1) / G>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            const int m = mslot<T>(lane + j * G);
            if (m < NM) {
                const SMuscle<Real> &mu = SM.mus[m];
                Real L, dLs[NSP];
                muscle_path<SW::PATH, T, Real>(SM, mu, lds, L, dLs);
                const Real nFt = a.ft ? -GAT(a.ft, (size_t)idx * NM + m, (size_t)a.n * NM) : Real(0);
                Real *col = tl + IA::COL + (C_MUS + m) * ND;   /* this lane's own column */
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    Real v = 0;
#pragma unroll
                    for (int k = 0; k < NSP; ++k) v = (k < mu.nspan && mu.span[k] == d) ? nFt * dLs[k] : v;
                    col[d] = v;
                }
            }
        });
    }
    wave_sync();
    if (lane < ND) {
        Real s = 0;
#pragma unroll
        for (int c = 0; c < C_TOT; ++c) s += tl[IA::COL + c * ND + lane];
        tl[IA::COL + C_TOT * ND + lane] = s;
    }
    wave_sync();
    /* M = L L^T in place (strict lower part scaled, reciprocal pivots in D).
     * From here on `ok` differs between the states of one wave (it is uniform
     * over a state's G lanes), so the syncs inside its regions are the
     * lane-divergent form */
    bool ok = true;
    for (int k = 0; k < ND && ok; ++k) {
        const Real piv = lds[LY::MP + k * (k + 1) / 2 + k];
        ok = piv > Real(0);
        if (ok) {
            const Real rp = Real(1) / sqrt(piv);
            for (int i = k + 1 + lane; i < ND; i += G) lds[LY::MP + i * (i + 1) / 2 + k] *= rp;
            if (lane == 0) tl[IA::D + k] = rp;
            wave_sync_lanes();
            for (int i = k + 1 + lane; i < ND; i += G) {
                Real *ri = lds + LY::MP + i * (i + 1) / 2;
                const Real lik = ri[k];
                for (int jc = k + 1; jc <= i; ++jc) ri[jc] -= lik * lds[LY::MP + jc * (jc + 1) / 2 + k];
            }
            wave_sync_lanes();
        }
    }
    const int nx = point ? IA::NX : NCOL;
    if (ok) {
        /* lane l: columns l, l + G, ...: L y = b, then L^T x = y, in place */
        for (int c = lane; c < nx; c += G) {
            Real *x = tl + IA::COL + c * ND;
            for (int k = 0; k < ND; ++k) {
                const Real *rk = lds + LY::MP + k * (k + 1) / 2;
                Real s = x[k];
                for (int j = 0; j < k; ++j) s -= rk[j] * x[j];
                x[k] = s * tl[IA::D + k];
            }
            for (int k = ND - 1; k >= 0; --k) {
                Real s = x[k];
                for (int i = k + 1; i < ND; ++i) s -= lds[LY::MP + i * (i + 1) / 2 + k] * x[i];
                x[k] = s * tl[IA::D + k];
            }
        }
    }
    wave_sync();
    if (ok) {   /* a NaN that came in (u, ft, tau_act, ext) shows in the total column */
        const Real tv = lane < ND ? tl[IA::COL + C_TOT * ND + lane] : Real(0);
        ok = !(group_max<G>((tv == tv) ? Real(0) : Real(1)) > Real(0));
    }
    if (ok && point) {
        if (lane < NJ) {   /* row lane of S = J Y; a foot not held keeps the identity */
            const bool held = tl[IA::PF + 4 * (lane / NR) + 3] > 0;
            for (int i = 0; i < NJ; ++i) {
                Real s = (i == lane && !held) ? Real(1) : Real(0);
                for (int d = 0; d < ND; ++d) s += tl[IA::JR + lane * ND + d] * tl[IA::COL + (NCOL + i) * ND + d];
                tl[IA::SS + lane * NJ + i] = s;
            }
        }
        wave_sync_lanes();
        if (lane == 0) {   /* NJ <= 6: the lower triangle, in place */
            bool oks = true;
            for (int k = 0; k < NJ; ++k) {
                Real s = tl[IA::SS + k * NJ + k];
                for (int j = 0; j < k; ++j) s -= tl[IA::SS + k * NJ + j] * tl[IA::SS + k * NJ + j];
                oks = oks && s > Real(0);
                const Real rp = Real(1) / sqrt(s > Real(0) ? s : Real(1));
                tl[IA::SD + k] = rp;
                for (int i = k + 1; i < NJ; ++i) {
                    Real v = tl[IA::SS + i * NJ + k];
                    for (int j = 0; j < k; ++j) v -= tl[IA::SS + i * NJ + j] * tl[IA::SS + k * NJ + j];
                    tl[IA::SS + i * NJ + k] = v * rp;
                }
            }
            tl[IA::FLAG] = oks ? Real(1) : Real(0);
        }
        wave_sync_lanes();
        ok = tl[IA::FLAG] > Real(0);
    }
    const size_t crow = (size_t)idx * NCOL, crows = (size_t)a.n * NCOL;
    if (ok) {
        for (int c = lane; c < NCOL; c += G) {
            Real *x = tl + IA::COL + c * ND;
            const bool vel = c == 1 || c == C_TOT;
            Real lam[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) lam[j] = 0;
            if (point) {
                /* lambda = -S^-1 (J A + beta), A += Y lambda */
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    Real s = vel ? tl[IA::BETA + j] : Real(0);
                    for (int d = 0; d < ND; ++d) s += tl[IA::JR + j * ND + d] * x[d];
                    lam[j] = -s;
                }
#pragma unroll
                for (int k = 0; k < NJ; ++k) {
#pragma unroll
                    for (int j = 0; j < k; ++j) lam[k] -= tl[IA::SS + k * NJ + j] * lam[j];
                    lam[k] *= tl[IA::SD + k];
                }
#pragma unroll
                for (int k = NJ - 1; k >= 0; --k) {
#pragma unroll
                    for (int i = k + 1; i < NJ; ++i) lam[k] -= tl[IA::SS + i * NJ + k] * lam[i];
                    lam[k] *= tl[IA::SD + k];
                }
                for (int d = 0; d < ND; ++d) {
                    Real s = x[d];
#pragma unroll
                    for (int j = 0; j < NJ; ++j) s += tl[IA::COL + (NCOL + j) * ND + d] * lam[j];
                    x[d] = s;
                }
            }
            if (a.reaction) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        GAT(a.reaction, ((crow + c) * NF + f) * 3 + r, crows * NF * 3) = r < NR ? lam[f * NR + (r < NR ? r : 0)] : Real(0);
            }
            if (a.com_accel) {
                const Real im = Real(1) / tl[IA::CB + 3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    Real s = vel ? tl[IA::CB + i] * im : Real(0);
                    for (int d = 0; d < ND; ++d) s += tl[IA::JC + i * ND + d] * x[d];
                    GAT(a.com_accel, (crow + c) * 3 + i, crows * 3) = s;
                }
            }
        }
    }
    wave_sync();
    if (a.accel) {
        for (int e = lane; e < NCOL * ND; e += G)
            GAT(a.accel, crow * ND + e, crows * ND) = ok ? tl[IA::COL + e] : Real(0);
    }
    if (!ok) {
        if (a.reaction)
            for (int e = lane; e < NCOL * NF * 3; e += G) GAT(a.reaction, crow * NF * 3 + e, crows * NF * 3) = Real(0);
        if (a.com_accel)
            for (int e = lane; e < NCOL * 3; e += G) GAT(a.com_accel, crow * 3 + e, crows * 3) = Real(0);
    }
    if (lane < NF) {
        const bool held = ok && tl[IA::PF + 4 * lane + 3] > 0;
        if (a.cactive_out) GAT(a.cactive_out, (size_t)idx * NF + lane, (size_t)a.n * NF) = held ? 1 : 0;
        if (a.cpoint_out) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                GAT(a.cpoint_out, ((size_t)idx * NF + lane) * 3 + i, (size_t)a.n * NF * 3) =
                    held ? tl[IA::PF + 4 * lane + i] + (i == 0 ? x0 : Real(0)) : Real(0);
        }
    }
    if (lane == 0 && a.status) a.status[idx] = ok ? 0 : -2;
}

/* ---------------------------------------------------------------- kernel
 * Launch arguments of one env segment (one handle).  mode 0: env step
 * (optionally with in-kernel auto-reset); mode 1: reset the listed envs.
 * I/O rows are strided so several segments (a mixed-topology group) can
 * share padded [N_total][stride] buffers. */
template <class T, typename Real> struct LaunchArgs {
    const DModel<Real> *Mg;
    const SModel<T, Real> *Sg;
    DState<Real> st;
    int N, mode, n_list, auto_reset, env_offset, blocks;
    int act_stride, obs_stride, info_stride;
    const Real *actions;
    Real *obs, *reward, *info;
    Real *final_obs;   /* optional: the step's observation before any auto-reset (row stride obs_stride) */
    Real *force_out;   /* optional: per-force-element values of the realized state, row stride force_dim */
    int force_dim;
    /* optional (RK kernels): the Manager's state storage — a row (t, q, u,
     * activation, fiber length) per accepted integration step of the env step,
     * [N][traj_cap][traj_dim]; traj_n[N] counts them (past traj_cap: counted, not stored) */
    Real *traj;
    int32_t *traj_n;
    int traj_cap, traj_dim;
    uint8_t *done_out;
    const int32_t *env_ids, *ref_index;
    uint64_t seed;
    /* apply_perturbations: zero-order-hold force table x[pert_n] (shared),
     * y[pert_n][N]; force on OpenSim body pert_ob; pert_n == 0: off */
    const double *pert_x;
    const Real *pert_y;
    int pert_n, pert_ob;
    double rk_acc;     /* RK-Merson accuracy (RK kernels) */
    int rk_budget;     /* RK kernels: attempts per env per launch (0: finish every step) */
    uint8_t *ready_out; /* optional [N]: 1 where the env finished its step in this launch */
    const uint8_t *active; /* optional [N] (steps): 0 = no new action, the env is left untouched
                              unless it is finishing a suspended RK step */
    /* mode 2 (OsimModel calls, REP kernels only; bioim_osim): op BIOIM_OSIM_*,
     * optional controls [n_list][nact] actuated first, report rows [N][osim_dim] */
    int osim_op, osim_dim;
    const Real *controls_in;
    Real *osim_out;
    /* optional (default step kernels of muscle models, no push, no force
     * report): the reset table — per reference row r its equilibrium fiber
     * lengths [nmuscle] and reset observation [obs_dim] (row stride
     * reset_tab_dim), computed once per handle by the reset realize itself
     * (build_reset_table); an in-kernel auto-reset reads row r instead of
     * running that realize again */
    const Real *reset_tab;
    int reset_tab_dim;
};

/* Reference integrator (RK kernels): OpenSim's Manager integrates with an
 * adaptive Kutta-Merson 4(5) at accuracy 1e-3 (opensim_wrapper.py:287-301).
 * Stage form, error norm, step control and the attempt cap follow
 * oracle/bioim_oracle.c integrate_rk_merson exactly; per state value the lane
 * keeps y0, K, E (three registers) besides the value itself. */
template <typename Real> DEV void rk_update(int s, Real h, Real f, Real &y, Real &y0, Real &K, Real &E, Real &err) {
    switch (s) {
    case 0: y0 = y; K = f; E = Real(2) * f; y = y0 + h / Real(3) * f; break;
    case 1: y = y0 + h / Real(6) * (K + f); break;
    case 2: E -= Real(9) * f; y = y0 + h / Real(8) * (K + Real(3) * f); break;
    case 3: {
        const Real B = (K + E) / Real(3);
        E += Real(8) * f;
        y = y0 + Real(0.5) * h * (B + Real(4) * f);
        K += Real(4) * f;
        break;
    }
    default: {
        E -= f;
        y = y0 + h / Real(6) * (K + f);
        const Real w = fabs(y0) > Real(1) ? fabs(y0) : Real(1);
        const Real ei = fabs(h / Real(30) * E) / w;
        if (!(ei <= err)) err = ei;
    }
    }
}

/* one muscle's term of calc_cost_of_transport (muscle_walking_imitation_env2D.py:360-403,
 * Umberger-style heat and work rates): mass * (activation + maintenance heat)
 * + shortening + work, from the excitation ex and the realized fiber state */
template <typename Real> DEV Real muscle_cot(const SMuscle<Real> &mu, const MState<Real> &ms, Real ex) {
    Real l = mu.slow, aa = ms.act, hp = Real(0.5 * 3.14159265358979323846);
    Real se, ce, sa, ca;
    sincos_rt(hp * ex, se, ce);
    sincos_rt(hp * aa, sa, ca);
    Real fa = Real(40) * l * se + Real(133) * (Real(1) - l) * (Real(1) - ce);
    Real fm = Real(74) * l * sa + Real(111) * (Real(1) - l) * (Real(1) - ca);
    Real ln = ms.lce * mu.inv_lopt, vv = ms.vce;
    Real g = 0;
    if (ln < Real(0.5)) g = Real(0.5);
    else if (ln < Real(1)) g = ln;
    else if (ln < Real(1.5)) g = Real(-2) * ln + Real(3);
    Real es = fmax(Real(0), Real(0.25) * ms.Ff * -vv);
    Real ew = fmax(Real(0), ms.Fa * -vv);
    return mu.mass * fa + mu.mass * g * fm + es + ew;
}

/* OpenSim's body-fixed XYZ angles of R = Rx(a) Ry(b) Rz(c)
 * (Rotation::convertRotationToBodyFixedXYZ, opensim_wrapper.py:164-167) */
template <typename Real> DEV void body_fixed_xyz(const Real *R, Real *ang) {
    ang[0] = atan2(-R[5], R[8]);
    ang[1] = atan2(R[2], sqrt(R[0] * R[0] + R[1] * R[1]));
    ang[2] = atan2(-R[1], R[0]);
}

/* The realized state as the OsimModel calc_* calls read it (REP kernels,
 * bioim_osim; layout in include/bioim.h, BIOIM_OSIM_REPORT): time, istep;
 * q, u, q'' (CoordinateSet order); per OpenSim body origin position,
 * velocity, acceleration, body-fixed XYZ angles, angular velocity and
 * acceleration (calc_body_kinematics, :137-190), then the system COM
 * position, velocity, acceleration; per muscle activation, fiber length,
 * fiber velocity, fiber force, active fiber force, excitation, tendon force
 * (calc_muscles_info :238-259 and calc_cost_of_transport's getters); the
 * actuation of each actuator; per Hunt-Crossley force the wrench on the feet
 * about the ground origin (calc_forces_info :192-236); the limit forces;
 * calc_cost_of_transport().  Reads the frames, accelerations, columns, q''
 * and force slots the realize left in LDS; lane-parallel. */
template <class T, typename Real>
DEV void osim_report(const DModel<Real> &M, const SModel<T, Real> &SM, const Real *lds, int lane, const Dyn<T, Real> &D,
                     const Real (&control)[Lay<T, Real>::MPL], double t, int istep, Real *out) {
    using LY = Lay<T, Real>;
    constexpr int G = T::G, NC = T::NC, ND = LY::ND, NOS = T::NOS, NM = T::NM, NA = T::NA, MPL = LY::MPL;
    constexpr int CPL = (NC + G - 1) / G;
    constexpr int OB = 2 + 3 * NC, OCOM = OB + 18 * NOS, OMU = OCOM + 9, OACT = OMU + 7 * NM, OCF = OACT + NA;
    constexpr int OLIM = OCF + 6 * T::NF, OCOT = OLIM + T::NL;
    const Real x0 = D.x0;
    if (lane == 0) { out[0] = Real(t); out[1] = Real(istep); }
    /* the muscle rows first: their fiber states then die before the body
     * terms below are live (3D REP kernels: fewer values spilled) */
    Real cot = 0;
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        const int m = mslot<T>(lane + j * G);
        if constexpr (NM > 0) {
            if (m < NM) {
                const MState<Real> &ms = D.ms[j];
                Real *o = out + OMU + 7 * m;
                o[0] = ms.act; o[1] = ms.lce; o[2] = ms.vce; o[3] = ms.Ff; o[4] = ms.Fa; o[5] = control[j]; o[6] = ms.Ft;
                cot += muscle_cot<Real>(SM.mus[m], ms, control[j]);
            }
        }
        if (m < NA) {
            if constexpr (NM > 0) out[OACT + m] = D.ms[j].Ft;
            else out[OACT + m] = control[j] * SM.ca_opt[m];
        }
    }
    cot = group_sum<G>(cot);
    if (lane == 0) out[OCOT] = NM > 0 ? cot + Real(1.51) * M.total_mass : Real(0);
    /* loops over bodies, spheres and coordinates run rolled (unroll 1): the
     * report is off the stepping path, and unrolled it held every body's terms
     * live at the kernel's peak register pressure — 0.6-2.9 KB/lane of scratch
     * in the REP kernels (profiles/r03/resources.txt).  (Round 4's first cut
     * kept the prosthetic model's loops unrolled: rolled, its non-RK REP
     * kernels then got two lane-divergent AGPR copies of the env offset that
     * tools/hazard_gate.py flags; with the compile-time mode of the REP
     * kernels (env_block) the rolled form is clean there too.) */
    constexpr int UC = 1, UB = 1, US = 1;
#pragma unroll UC
    for (int jc = 0; jc < CPL; ++jc) {
        const int c = lane + jc * G;
        if (c < NC) {
            const int dc = SM.coord_dof[c];
            out[2 + c] = lds[LY::QF + c];
            out[2 + NC + c] = lds[LY::UF + c];
            out[2 + 2 * NC + c] = dc >= 0 ? lds[LY::RHS + dc] : Real(0);
        }
    }
    /* spatial acceleration of composite body cb (at the shifted ground
     * origin): the velocity-product part plus its root path's columns x q'' */
    auto body_acc = [&](int cb, Real *al, Real *aO) {
        const Real *ab = lds + LY::AL + 6 * cb;
        const uint32_t dm = SM.dofmask[cb];
#pragma unroll
        for (int i = 0; i < 3; ++i) { al[i] = ab[i]; aO[i] = ab[3 + i]; }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const Real qdd = ((dm >> d) & 1u) ? lds[LY::RHS + d] : Real(0);
            const Real *S = lds + LY::S + 6 * d;
#pragma unroll
            for (int i = 0; i < 3; ++i) { al[i] += S[i] * qdd; aO[i] += S[3 + i] * qdd; }
        }
    };
    if (lane < NOS) {
        /* each term stored as soon as it is computed (fewer values live at once) */
        const int cb = SM.os_cb[lane];
        const Real *kb = lds + LY::KB + 18 * cb;
        Real *o = out + OB + 18 * lane;
        {
            Real Rb[9], ang[3];
            mm3(kb, M.os_R[lane], Rb);
            body_fixed_xyz(Rb, ang);
#pragma unroll
            for (int i = 0; i < 3; ++i) { o[9 + i] = ang[i]; o[12 + i] = kb[12 + i]; }
        }
        Real P[3], v[3], tt[3], al[3], aO[3];
        mv3(kb, SM.os_p[lane], P);
#pragma unroll
        for (int i = 0; i < 3; ++i) P[i] += kb[9 + i];
        cross3(kb + 12, P, tt);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v[i] = kb[15 + i] + tt[i];
            o[i] = P[i] + (i == 0 ? x0 : Real(0)); o[3 + i] = v[i];
        }
        body_acc(cb, al, aO);
        Real t2[3];
        cross3(al, P, tt);
        cross3(kb + 12, v, t2);
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[6 + i] = aO[i] + tt[i] + t2[i]; o[15 + i] = al[i]; }
    } else if (lane == NOS) {
        Real mt = 0, cs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, as[3] = {0, 0, 0};
#pragma unroll UB
        for (int c = 0; c < T::NB; ++c) {
            const Real *kb = lds + LY::KB + 18 * c;
            Real cG[3], vc[3], ac[3], tt[3], t2[3], al[3], aO[3];
            mv3(kb, SM.body[c].com, cG);
#pragma unroll
            for (int i = 0; i < 3; ++i) cG[i] += kb[9 + i];
            cross3(kb + 12, cG, tt);
#pragma unroll
            for (int i = 0; i < 3; ++i) vc[i] = kb[15 + i] + tt[i];
            body_acc(c, al, aO);
            cross3(al, cG, tt);
            cross3(kb + 12, vc, t2);
#pragma unroll
            for (int i = 0; i < 3; ++i) ac[i] = aO[i] + tt[i] + t2[i];
            const Real m = SM.body[c].mass;
#pragma unroll
            for (int i = 0; i < 3; ++i) { cs[i] += m * cG[i]; vs[i] += m * vc[i]; as[i] += m * ac[i]; }
            mt += m;
        }
        Real *o = out + OCOM;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o[i] = cs[i] / mt + (i == 0 ? x0 : Real(0)); o[3 + i] = vs[i] / mt; o[6 + i] = as[i] / mt;
        }
    }
    if (lane < T::NF) {
        Real F[3] = {0, 0, 0}, Mo[3] = {0, 0, 0};
#pragma unroll US
        for (int s2 = 0; s2 < T::NS; ++s2) {
            const Real *cw = lds + LY::CW + 8 * s2;
            const bool mine = SM.sph_force[s2] == lane;
#pragma unroll
            for (int i = 0; i < 3; ++i) { F[i] += mine ? cw[i] : Real(0); Mo[i] += mine ? cw[3 + i] : Real(0); }
        }
        Mo[1] += -x0 * F[2];
        Mo[2] += x0 * F[1];
#pragma unroll
        for (int i = 0; i < 3; ++i) { out[OCF + 6 * lane + i] = F[i]; out[OCF + 6 * lane + 3 + i] = Mo[i]; }
    }
    if (lane < T::NL) out[OLIM + lane] = lds[LY::LIM + 4 * lane];
}

/* ---------------------------------------------------------- body kinematics
 * bioim_body_kin (include/bioim.h): OpenSim's BodyKinematics and
 * PointKinematics at n arbitrary (q, u, q'') rows, plus the whole-body mass
 * centre, momentum and energy.  ma_kernel's launch shape and prologue (one
 * state per G lanes, the model image in LDS, the step's kinematics).  Then:
 *   1. body lane c: the full spatial acceleration, AL_c + sum over the dofs d
 *      on c's root path of S_d q''_d (osim_report's body_acc), in place in AL;
 *   2. the stations — every OpenSim body's origin, every OpenSim body's own
 *      mass centre, the caller's points — are one list that the lanes walk in
 *      strides of G through one piece of code (bk_station), so a point at a
 *      body's origin or mass centre is that row bit for bit;
 *   3. the lanes walk the OpenSim bodies again for the angles and R;
 *   4. body lane c leaves its mass centre's p, v, a, its kinetic energy and
 *      I_c w_c in the (otherwise unused) IC / WB slots, and lane 0 sums them
 *      over c = 0 .. NB-1, so a state's sums do not depend on its neighbours.
 * The point table and the OpenSim bodies' mass centres are part of the
 * argument list itself (the entry point checks and copies them): the lanes
 * read them from the kernel-argument segment.  No atomics, nothing of the env
 * state is read or written, no workgroup barrier after the exit. */
template <typename P> struct BkFields {   /* bioim_body_kin */
    int n, npt, flags, pad;
    const P *q, *u, *qdd;
    P *origin, *com, *orient, *rot, *system, *momentum, *energy, *point;
    double os_com[BIOIM_MAX_OSBODY][3];             /* each OpenSim body's mass centre, in its own frame */
    double pt_local[BIOIM_BK_MAX_POINTS][3];
    int8_t pt_body[BIOIM_BK_MAX_POINTS];            /* OpenSim body index, -1: ground */
};

/* A station `loc` of the OpenSim body placed at (osR, osp) in its composite
 * body: position (from the shifted ground origin), velocity and acceleration
 * in ground.  kb: the composite body's frame (R9 o3 w3 vO3); ab: its spatial
 * acceleration (alpha3, aO3), the q'' terms included. */
template <typename Real>
DEV void bk_station(const Real *kb, const Real *ab, const Real *osR, const Real *osp, const Real *loc, Real *P, Real *v,
                    Real *acc) {
    Real lc[3], t[3], t2[3];
    mv3(osR, loc, lc);
#pragma unroll
    for (int i = 0; i < 3; ++i) lc[i] += osp[i];
    mv3(kb, lc, P);
#pragma unroll
    for (int i = 0; i < 3; ++i) P[i] += kb[9 + i];
    cross3(kb + 12, P, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = kb[15 + i] + t[i];
    cross3(ab, P, t);
    cross3(kb + 12, v, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] = ab[3 + i] + t[i] + t2[i];
}

/* o = R^T v */
template <typename Real> DEV void bk_tmv3(const Real *R, const Real *v, Real *o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2];
}

template <class T, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void bk_kernel(ModelArgs<T, Real> md, BkFields<Real> a) {
    using LY = Lay<T, Real>;
    constexpr int G = T::G, ND = LY::ND, NB = T::NB, NOS = T::NOS, EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SModel<T, Real> &SM = stage_model<EPB, T, Real>(md.Sg, smem_raw);
    const DModel<Real> &M = *md.Mg;
    const int lane = threadIdx.x % G, slot = threadIdx.x / G;
    const int idx = blockIdx.x * EPB + slot;
    if (idx >= a.n) return;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    const bool local = (a.flags & BIOIM_BK_LOCAL) != 0;
    Real qd = 0, ud = 0, ad = 0;
    if (lane < ND) {
        qd = GAT(a.q, (size_t)idx * ND + lane, (size_t)a.n * ND);
        ud = opt_row<Real, ND>(a.u, idx, lane, a.n);
        ad = opt_row<Real, ND>(a.qdd, idx, lane, a.n);
    }
    const Real x0 = state_kinematics<BfSwitch<T>::FN, T, Real>(M, SM, lds, lane, qd, ud);
    if (lane < ND) lds[LY::RHS + lane] = ad;
    wave_sync();   /* frames, velocity-product accelerations, columns and q'' are out */
    if (lane < NB) {
        Real *ab = lds + LY::AL + 6 * lane;
        const uint32_t dm = SM.dofmask[lane];
        Real sa[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) sa[i] = ab[i];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const Real qdd = ((dm >> d) & 1u) ? lds[LY::RHS + d] : Real(0);
            const Real *S = lds + LY::S + 6 * d;
#pragma unroll
            for (int i = 0; i < 6; ++i) sa[i] += S[i] * qdd;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) ab[i] = sa[i];   /* its own slot only: no other lane reads it before the sync */
    }
    wave_sync();
    /* the stations: [0, NOS) body origins, [NOS, 2 NOS) the bodies' own mass centres, then the points */
    const int nst = 2 * NOS + a.npt;
    for (int s = lane; s < nst; s += G) {
        const int kind = s < NOS ? 0 : (s < 2 * NOS ? 1 : 2);
        const int k = s - kind * NOS;
        Real *out = kind == 0 ? a.origin : (kind == 1 ? a.com : a.point);
        if (!out) continue;
        const int b = kind == 2 ? (int)a.pt_body[k] : k;
        Real loc[3], P[3], v[3], acc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            loc[i] = kind == 0 ? Real(0) : (kind == 1 ? Real(a.os_com[k][i]) : Real(a.pt_local[k][i]));
        if (b < 0) {   /* a ground point is fixed */
#pragma unroll
            for (int i = 0; i < 3; ++i) { P[i] = loc[i]; v[i] = 0; acc[i] = 0; }
        } else {
            const int cb = SM.os_cb[b];
            const Real *kb = lds + LY::KB + 18 * cb;
            bk_station(kb, lds + LY::AL + 6 * cb, M.os_R[b], SM.os_p[b], loc, P, v, acc);
            P[0] += x0;
            if (local && kind != 2) {   /* ground -> the OpenSim body's frame: (R_cb R_os)^T */
                Real t[3];
                bk_tmv3(kb, v, t); bk_tmv3(M.os_R[b], t, v);
                bk_tmv3(kb, acc, t); bk_tmv3(M.os_R[b], t, acc);
            }
        }
        const size_t cnt = kind == 2 ? (size_t)a.npt : (size_t)NOS;
        const size_t row = ((size_t)idx * cnt + k) * 9, rows = (size_t)a.n * cnt * 9;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            GAT(out, row + i, rows) = P[i]; GAT(out, row + 3 + i, rows) = v[i]; GAT(out, row + 6 + i, rows) = acc[i];
        }
    }
    if (a.orient || a.rot) {
        for (int b = lane; b < NOS; b += G) {
            const int cb = SM.os_cb[b];
            const Real *kb = lds + LY::KB + 18 * cb, *ab = lds + LY::AL + 6 * cb;
            Real Rb[9], ang[3], w[3], al[3];
            mm3(kb, M.os_R[b], Rb);
            body_fixed_xyz(Rb, ang);
            if (local) { bk_tmv3(Rb, kb + 12, w); bk_tmv3(Rb, ab, al); }
            else {
#pragma unroll
                for (int i = 0; i < 3; ++i) { w[i] = kb[12 + i]; al[i] = ab[i]; }
            }
            const size_t r9 = ((size_t)idx * NOS + b) * 9, rows = (size_t)a.n * NOS * 9;
            if (a.orient) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    GAT(a.orient, r9 + i, rows) = ang[i]; GAT(a.orient, r9 + 3 + i, rows) = w[i];
                    GAT(a.orient, r9 + 6 + i, rows) = al[i];
                }
            }
            if (a.rot) {
#pragma unroll
                for (int i = 0; i < 9; ++i) GAT(a.rot, r9 + i, rows) = Rb[i];
            }
        }
    }
    if (a.system || a.momentum || a.energy) {
        if (lane < NB) {   /* IC_c: mass centre p3 v3 a3, kinetic energy; WB_c: I_c w_c in ground */
            const SBody<Real> &bd = SM.body[lane];
            const Real *kb = lds + LY::KB + 18 * lane;
            const Real zero[3] = {0, 0, 0}, eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            Real cG[3], vc[3], ac[3], wl[3], Il[3], Iw[3];
            bk_station(kb, lds + LY::AL + 6 * lane, eye, bd.com, zero, cG, vc, ac);
            bk_tmv3(kb, kb + 12, wl);
            Il[0] = bd.inertia[0] * wl[0] + bd.inertia[3] * wl[1] + bd.inertia[4] * wl[2];
            Il[1] = bd.inertia[3] * wl[0] + bd.inertia[1] * wl[1] + bd.inertia[5] * wl[2];
            Il[2] = bd.inertia[4] * wl[0] + bd.inertia[5] * wl[1] + bd.inertia[2] * wl[2];
            mv3(kb, Il, Iw);
            Real *ic = lds + LY::IC + 10 * lane, *wb = lds + LY::WB + 6 * lane;
#pragma unroll
            for (int i = 0; i < 3; ++i) { ic[i] = cG[i]; ic[3 + i] = vc[i]; ic[6 + i] = ac[i]; wb[i] = Iw[i]; }
            ic[9] = Real(0.5) * (bd.mass * dot3(vc, vc) + dot3(wl, Il));
        }
        wave_sync();
        if (lane == 0) {
            Real mt = 0, ke = 0, cs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, as[3] = {0, 0, 0}, hs[3] = {0, 0, 0};
#pragma unroll 1
            for (int c = 0; c < NB; ++c) {
                const Real *ic = lds + LY::IC + 10 * c;
                const Real m = SM.body[c].mass;
#pragma unroll
                for (int i = 0; i < 3; ++i) { cs[i] += m * ic[i]; vs[i] += m * ic[3 + i]; as[i] += m * ic[6 + i]; }
                mt += m;
                ke += ic[9];
            }
            Real C0[3], V0[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { C0[i] = cs[i] / mt; V0[i] = vs[i] / mt; }
#pragma unroll 1
            for (int c = 0; c < NB; ++c) {   /* angular momentum about the whole-body mass centre */
                const Real *ic = lds + LY::IC + 10 * c, *wb = lds + LY::WB + 6 * c;
                const Real m = SM.body[c].mass;
                Real r[3], dv[3], t[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) { r[i] = ic[i] - C0[i]; dv[i] = ic[3 + i] - V0[i]; }
                cross3(r, dv, t);
#pragma unroll
                for (int i = 0; i < 3; ++i) hs[i] += wb[i] + m * t[i];
            }
            C0[0] += x0;
            if (a.system) {
                const size_t r9 = (size_t)idx * 9, rows = (size_t)a.n * 9;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    GAT(a.system, r9 + i, rows) = C0[i]; GAT(a.system, r9 + 3 + i, rows) = V0[i];
                    GAT(a.system, r9 + 6 + i, rows) = as[i] / mt;
                }
            }
            if (a.momentum) {
                const size_t r6 = (size_t)idx * 6, rows = (size_t)a.n * 6;
#pragma unroll
                for (int i = 0; i < 3; ++i) { GAT(a.momentum, r6 + i, rows) = vs[i]; GAT(a.momentum, r6 + 3 + i, rows) = hs[i]; }
            }
            if (a.energy) {
                GAT(a.energy, (size_t)idx * 2, (size_t)a.n * 2) = ke;
                GAT(a.energy, (size_t)idx * 2 + 1, (size_t)a.n * 2) = -mt * dot3(M.gravity, C0);
            }
        }
    }
}

/* One 256-thread workgroup = 256/G envs of segment `a`, block `blk`.
 * RK: the reference integrator (adaptive Kutta-Merson) instead of the
 * fixed semi-implicit substeps. */
template <class T, typename Real, bool PERT, bool RK, bool REP, bool FUSED = false, bool EXT = false>
DEV void env_block(const LaunchArgs<T, Real> &a, int blk, const ExtArgs<Real> &xa = ExtArgs<Real>{}) {
    static_assert(!EXT || (!PERT && !RK && !FUSED), "external forces: the semi-implicit step and report kernels only");
    using LY = Lay<T, Real>;
    using TS = TailSwitch<T, FUSED, RK>;
    constexpr int G = T::G, ND = LY::ND, NA = T::NA, NM = T::NM;
    constexpr int EPB = BIOIM_EPB;
    constexpr size_t SMB = smodel_bytes<T, Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const DModel<Real> *__restrict__ Mg = a.Mg;
    const DState<Real> &st = a.st;
    /* mode 2 (OsimModel calls) exists in the REP kernels only, and they run
     * nothing else (launch_impl): a compile-time mode there, so the step's
     * reward / termination / auto-reset tail and the RK carry past the report
     * are dead code in them instead of live registers */
    const int N = a.N, mode = REP ? 2 : a.mode;
    const bool osim = REP;
    const Real *__restrict__ actions = a.actions;
    Real *__restrict__ obs = a.obs;
#ifdef BIOIM_STAMPS
    const unsigned long long k_t0 = __builtin_amdgcn_s_memtime();
#endif
    /* stage the shared model image (one copy per workgroup) */
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.Sg);
        uint4 *dst = reinterpret_cast<uint4 *>(smem_raw);
        for (int i = threadIdx.x; i < (int)(SMB / 16); i += BIOIM_EPB * G) dst[i] = src[i];
    }
    __syncthreads();
#ifdef BIOIM_STAMPS
    const unsigned long long k_t1 = __builtin_amdgcn_s_memtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) { g_stamps[11] += k_t1 - k_t0; g_stamps[26] = 1 + TS::FE; }   /* 26: the kernel's front-end bits + 1 (tools/stamps.py names slots 1-2 by FE_INERTIA) */
#endif
    const SModel<T, Real> &SM = *reinterpret_cast<const SModel<T, Real> *>(smem_raw);
    const DModel<Real> &M = *Mg;
    const int lane = threadIdx.x % G;
    const int slot = threadIdx.x / G;
    int gidx = blk * EPB + slot;
    Real *lds = reinterpret_cast<Real *>(smem_raw + SMB) + slot * LY::SIZE;
    int env;
    if (mode == 1 || osim) {
        if (gidx >= a.n_list) return;
        env = a.env_ids ? GAT(a.env_ids, gidx, a.n_list) : gidx;
        if (env < 0 || env >= N) return;
    } else {
        if (gidx >= N) return;
        env = gidx;
        if (a.active && !GAT(a.active, env, N) && !(RK && GAT(st.pend, env, (size_t)N) != 0)) return;
    }
    const int H = M.horizon;
    /* the ground slot's constants, once per launch (kin_ground); the first
     * call's own syncs come before their first read */
    if constexpr (TS::GROUND) {
        if (lane == T::NB) {
            kin_ground_const<T, Real>(lds);
            if constexpr (ground_loc_free<T, Real>()) kin_ground_loc<T, Real>(lds);
        }
    }
    /* the lane's index record (BIOIM_LANEIDX), once per launch: it depends on
     * the lane and the staged image alone */
    LaneIdx<T, Real> LX{};
    lane_index<TS::LI, T, Real>(SM, lane, LX);
    constexpr int MPL = LY::MPL;                  /* muscles / actions per lane: m = lane + j*G */
    constexpr int CPL = (T::NC + G - 1) / G;      /* coordinates per lane (report)              */
    Dyn<T, Real> D;
#pragma unroll
    for (int j = 0; j < MPL; ++j) D.ms[j].vN = 0;
#if BIOIM_FV_PRED
    Real vprev[MPL];
#pragma unroll
    for (int j = 0; j < MPL; ++j) vprev[j] = 0;
#endif
    /* lane d < ND owns dof d (coordinate value qd, speed ud) */
    Real qd = 0, ud = 0;
    if (lane < ND) { qd = GAT(st.q, (size_t)lane * N + env, (size_t)ND * N); ud = GAT(st.u, (size_t)lane * N + env, (size_t)ND * N); }
    double t = GAT(st.t, env, (size_t)N);
    /* has_last, resets, old_px and last[] change only in a step (mode 0) or a
     * reset (mode 1): the REP kernels neither load nor store them, instead of
     * carrying them through the kernel unchanged */
    int istep = GAT(st.istep, env, (size_t)N), has_last = REP ? 0 : GAT(st.has_last, env, (size_t)N),
        resets = REP ? 0 : GAT(st.resets, env, (size_t)N);
    Real old_px = REP ? Real(0) : GAT(st.old_px, env, (size_t)N);
    Real act[MPL], lce[MPL], control[MPL], curr[MPL], last[MPL], hist[MPL][BIOIM_MAX_HORIZON];
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        const int m = mslot<T>(lane + j * G);
        act[j] = 0; lce[j] = 0; control[j] = 0; curr[j] = 0; last[j] = 0;
        if (NM > 0 && m < NM) { act[j] = GAT(st.act, (size_t)m * N + env, (size_t)(NM > 0 ? NM : 1) * N); lce[j] = GAT(st.lce, (size_t)m * N + env, (size_t)(NM > 0 ? NM : 1) * N); }
#pragma unroll
        for (int hh = 0; hh < BIOIM_MAX_HORIZON; ++hh) hist[j][hh] = 0;
        if (m < NA) {
            if (!REP) last[j] = GAT(st.last, (size_t)m * N + env, (size_t)NA * N);
#pragma unroll
            for (int hh = 0; hh < BIOIM_MAX_HORIZON; ++hh)
                hist[j][hh] = hh < H ? GAT(st.hist, ((size_t)hh * NA + m) * N + env, (size_t)BIOIM_MAX_HORIZON * NA * N) : Real(0);
            /* held controls (OsimModel calls act on the last actuate) */
            if (osim) control[j] = GAT(st.ctl, (size_t)m * N + env, (size_t)NA * N);
        }
    }
    /* the realize cache (CacheLay): a step's first substep takes its system
     * from the last launch's realize when that row is valid for this state
     * and was formed at this step's substep length (checked below); loaded
     * here, ahead of the action pre-processing */
    constexpr bool CACHE = CacheLay<T>::ON && !PERT && !RK && !REP && !EXT;
    CacheIO<T, Real> CI;
    bool cache_valid = false;
    Real cache_h = 0;
    if constexpr (CACHE) {
        using CL = CacheLay<T>;
        CI.base = st.cache; CI.env = env; CI.N = N;
        Real *const crow = st.cache + GIDX((size_t)env * CL::DIM, (size_t)N * CL::DIM);
        cache_valid = mode == 0 && GAT(st.cache_ok, env, (size_t)N) != 0;
        cache_h = GAT(crow, CL::H, CL::DIM);
        if constexpr (CL::PREFETCH) {
#pragma unroll
            for (int i = 0; i < CacheIO<T, Real>::PF; ++i)
                CI.sys[i] = lane + i * G < CL::SYS ? GAT(crow, lane + i * G, CL::DIM) : Real(0);
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
#pragma unroll
                for (int c = 0; c < 3; ++c) CI.mus[j][c] = m < NM ? GAT(crow, CL::MUS + 3 * m + c, CL::DIM) : Real(0);
            }
        }
    }
    int done = 0;
    Real rew = 0, inf[5] = {0, 0, 0, 0, 0};
    bool do_reset = (mode == 1);
    /* budgeted RK: a suspended step resumes (its action row is ignored) */
    const bool budget = RK && !REP && a.rk_budget > 0;   /* make_args: 0 unless mode 0 */
    const bool resume = RK && mode == 0 && GAT(st.pend, env, (size_t)N) != 0;
    bool suspend = false;
    /* RK: dynamics evaluations spent in this launch (the budget is 5 per
     * attempt) and so far (bioim_eval_count).  (Reusing a rejected attempt's
     * first stage for its retry — same start point — saves about a fifth of
     * the rejected attempts' evaluations but measured slower at 4096 envs:
     * the stores of k1 cost every attempt, and the saving rarely removes a
     * launch from a step; profiles/r03/ab_dropped/ab_rk_k1_reuse.txt) */
    int launch_evals = 0;
    /* state-storage rows of this env step so far (a resumed step continues its count) */
    int traj_k = (RK && a.traj && mode == 0 && GAT(st.pend, env, (size_t)N) != 0) ? GAT(a.traj_n, env, N) : 0;
    int reset_row = 0;
    if (mode == 1) reset_row = a.ref_index ? GAT(a.ref_index, gidx, a.n_list) : draw_index(a.seed, a.env_offset + env, resets, M.reset_hi);

    int remaining = 0;
    Real dt = 0;
    /* RK kernels: current step [rk_t, rk_t + rk_h], stage, attempts, next step size */
    double rk_t = 0, rk_tf = 0, rk_h = 0, rk_hnext = RK ? GAT(st.hrk, env, (size_t)N) : 0.0;
    int rk_stage = 0, rk_attempts = 0;
    bool rk_last = false, rk_fail = false;
    Real y0q = 0, y0u = 0, Kq = 0, Ku = 0, Eq = 0, Eu = 0, rk_err = 0;
    Real y0a[MPL], y0l[MPL], Ka[MPL], Kl[MPL], Ea[MPL], El[MPL];
#pragma unroll
    for (int j = 0; j < MPL; ++j) { y0a[j] = y0l[j] = Ka[j] = Kl[j] = Ea[j] = El[j] = 0; }
    const PertArgs<Real> PA{a.pert_x, a.pert_y, a.pert_n, a.pert_ob, env, N};
    double *pslot = reinterpret_cast<double *>(smem_raw + SMB + sizeof(Real) * EPB * LY::SIZE) + PERT_SLOT * slot;
    if (PERT && lane == 0) { pslot[0] = t; pslot[1] = 0; pslot[2] = 0; pslot[3] = -1; pslot[4] = 0; }
    /* bioim_set_external_forces: this env's rows, read once per launch into
     * its slot after the env regions (ExtLay; the env's own lanes write and
     * read it, and the first dynamics call syncs before the body lanes do);
     * held over every substep, the realize and an auto-reset's realize */
    ExtArgs<Real> XE = xa;
    if constexpr (EXT) {
        const int nx = xa.k * EXT_ROW;
        const Real *xrow = xa.rows + GIDX((size_t)env * nx, (size_t)N * nx);
        if constexpr (ExtLay<T, Real>::LDS) {
            Real *xs = reinterpret_cast<Real *>(smem_raw + SMB + sizeof(Real) * EPB * LY::SIZE) + ExtLay<T, Real>::SLOT * slot;
            for (int i = lane; i < nx; i += G) xs[i] = GAT(xrow, i, nx);
            XE.rows = xs;
        } else {
            XE.rows = xrow;
        }
    }
    /* OsimModel.integrate (opensim_wrapper.py:299-301): istep += 1, then
     * integrate to the absolute time step_size * istep with the held controls */
    auto begin_integrate = [&]() {
        istep += 1;
        double tf = M.step_size * (double)istep;
        double hstep = tf - t;
        if (hstep > 0) {
            if constexpr (RK) {
                rk_t = t; rk_tf = tf;
                rk_h = rk_hnext > 0 ? rk_hnext : 1e-4;
                remaining = 1;      /* integrating until rk_t reaches rk_tf */
            } else {
                dt = Real(hstep / (double)M.nsub);
                remaining = M.nsub;
                /* substep k starts at t + k * hstep / nsub (the oracle's substep times) */
                if (PERT && lane == 0) { pslot[0] = t; pslot[1] = hstep / (double)M.nsub; }
            }
        }
        t = tf;
    };
    bool eq_only = false;   /* mode 2 EQUILIBRATE: fiber equilibrium at the held state */
    if (osim) {
        if (a.controls_in) {
            /* OsimModel.actuate (opensim_wrapper.py:92-107): NaN -> 0, clip */
            Real raw[MPL];
            bool nan_here = false;
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
                raw[j] = m < NA ? GAT(a.controls_in, (size_t)gidx * NA + m, (size_t)a.n_list * NA) : Real(0);
                nan_here = nan_here || (m < NA && isnan(raw[j]));
            }
            const bool anynan = group_any<G>(nan_here);
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G), ms = m < NA ? m : 0;
                const Real lo = NM > 0 ? Real(0) : SM.ca_min[ms];
                const Real hi = NM > 0 ? Real(1) : SM.ca_max[ms];
                const Real v = anynan ? Real(0) : raw[j];
                control[j] = m < NA ? (v < lo ? lo : (v > hi ? hi : v)) : Real(0);
                if (m < NA) GAT(st.ctl, (size_t)m * N + env, (size_t)NA * N) = control[j];
            }
        }
        if (a.osim_op == BIOIM_OSIM_INTEGRATE) begin_integrate();
        if (a.osim_op == BIOIM_OSIM_EQUILIBRATE) {
            eq_only = true;
            rk_hnext = 0;   /* reset_manager: a new Manager / integrator (opensim_wrapper.py:287-291) */
        }
    } else if (resume) {
        /* the state is at the accepted RK point rk_t of the step ending at t.
         * The loads index with an opaque copy of env made inside this
         * lane-divergent branch: with env itself, the allocator split the
         * kernel-long env offsets here and copied them into AGPRs for the
         * resuming lanes only, which the state write-back then used as store
         * addresses in every lane (the r03i fault) */
        int er = env;
        asm volatile("" : "+v"(er));
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            const int m = mslot<T>(lane + j * G);
            if (m < NA) { control[j] = GAT(st.ctl, (size_t)m * N + er, (size_t)NA * N); curr[j] = GAT(st.cur, (size_t)m * N + er, (size_t)NA * N); }
            if (NM > 0 && m < NM) D.ms[j].vN = GAT(st.vnw, (size_t)m * N + er, (size_t)(NM > 0 ? NM : 1) * N);
        }
        rk_t = GAT(st.rkt, er, (size_t)N); rk_tf = t; rk_h = GAT(st.rkh, er, (size_t)N); rk_attempts = GAT(st.rka, er, (size_t)N);
        remaining = 1;
    } else if (mode == 0) {
        /* ---- action pre-processing (Env.step) */
        Real raw[MPL];
        bool nan_here = false;
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            const int m = mslot<T>(lane + j * G);
            raw[j] = m < NA ? GAT(actions, (size_t)env * a.act_stride + m, (size_t)N * a.act_stride) : Real(0);
            nan_here = nan_here || (m < NA && isnan(raw[j]));
        }
        const bool anynan = group_any<G>(nan_here);
        Real av[MPL];
#pragma unroll
        for (int j = 0; j < MPL; ++j) av[j] = anynan ? Real(0) : raw[j];
        if constexpr ((T::FLAGS & BIOIM_ENV_PD) != 0) {
            /* PD law on the state at the start of the step (torque_walking_imitation_env2D.py:125-139) */
            publish_coords<T, Real>(M, SM, lds, lane, qd, ud);
            wave_sync();
            if (!anynan) {
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const int m = mslot<T>(lane + j * G);
                    Real xq = 0, xu = 0;
                    sfor<0, NA>([&](auto iI) {
                        constexpr int i = decltype(iI)::value;
                        if (m == i) { xq = lds[LY::QF + T::pd_coord[i]]; xu = lds[LY::UF + T::pd_vcoord[i]]; }
                    });
                    if (m < NA) av[j] = SM.kp[m] * (raw[j] - xq) - SM.kv[m] * xu;
                }
            }
        }
        bool pnan_here = false;
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            const int m = mslot<T>(lane + j * G);
            if (!has_last) {
                last[j] = av[j];
#pragma unroll
                for (int hh = 0; hh < BIOIM_MAX_HORIZON; ++hh) hist[j][hh] = av[j];
            }
            /* fixed-trip loops keep the history in registers */
#pragma unroll
            for (int hh = 0; hh + 1 < BIOIM_MAX_HORIZON; ++hh)
                if (hh + 1 < H) hist[j][hh] = hist[j][hh + 1];
#pragma unroll
            for (int hh = 0; hh < BIOIM_MAX_HORIZON; ++hh)
                if (hh == H - 1) hist[j][hh] = av[j];
            Real sm = 0;
#pragma unroll
            for (int hh = 0; hh < BIOIM_MAX_HORIZON; ++hh)
                if (hh < H) sm += hist[j][hh];
            curr[j] = sm / Real(H);
            /* the deque is final here: store it now instead of holding it in
             * registers through the substep loop (34 AGPRs in 3D fp64) */
            if (m < NA) {
#pragma unroll
                for (int hh = 0; hh < BIOIM_MAX_HORIZON; ++hh)
                    if (hh < H) GAT(st.hist, ((size_t)hh * NA + m) * N + env, (size_t)BIOIM_MAX_HORIZON * NA * N) = hist[j][hh];
            }
            const Real phys = (M.env_flags & BIOIM_ENV_RAW_ACTION) ? av[j] : curr[j];
            pnan_here = pnan_here || (m < NA && isnan(phys));
            control[j] = phys;
        }
        has_last = 1;
        const bool pnan = group_any<G>(pnan_here);
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            const int m = mslot<T>(lane + j * G), ms = m < NA ? m : 0;
            const Real lo = NM > 0 ? Real(0) : SM.ca_min[ms];
            const Real hi = NM > 0 ? Real(1) : SM.ca_max[ms];
            const Real v = pnan ? Real(0) : control[j];
            control[j] = m < NA ? (v < lo ? lo : (v > hi ? hi : v)) : Real(0);
            /* the held controls (PrescribedController's Constants): kept through
             * resets, read by resets and OsimModel calls; stored now, so they
             * are not held in registers past the last dynamics call */
            if (m < NA) GAT(st.ctl, (size_t)m * N + env, (size_t)NA * N) = control[j];
        }
        /* ---- integrate to step_size * istep */
        begin_integrate();
    }

    /* One dynamics call site (inlined once): the substeps, then the realize
     * at the end state; a reset (mode 1, or auto-reset after done) loads the
     * reference row and folds the muscle fiber equilibrium into its realize. */
    bool pending_reset = (mode == 1), reported_reset = false;
#ifdef BIOIM_STAMPS
    /* the prologue, kernel start to loop entry with its loads landed (the
     * staging, slot 11, is part of it) */
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0070);
    const unsigned long long k_t2 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (blockIdx.x == 0 && threadIdx.x == 0) g_stamps[22] += k_t2 - k_t0;
    __builtin_amdgcn_sched_barrier(0);
#endif
    for (;;) {
        if constexpr (RK) {
            if (remaining > 0 && rk_stage == 0) {   /* start an RK step, or stop */
                const int cost = 5;
                if (!(rk_tf - rk_t > 1e-14 * (1.0 + fabs(rk_tf)))) remaining = 0;
                else if (budget && launch_evals + cost > 5 * a.rk_budget) { suspend = true; break; }
                else if (++rk_attempts > BIOIM_RK_MAX_ATTEMPTS) { rk_fail = true; remaining = 0; }
                else {
                    launch_evals += cost;
                    rk_last = false;
                    if (rk_h >= rk_tf - rk_t) { rk_h = rk_tf - rk_t; rk_last = true; }
                    rk_err = 0;
                }
            }
        }
        const bool sub = remaining > 0;
        const bool eq = !sub && (pending_reset || eq_only);
        if (!sub && pending_reset) {
                        int r = clamp_row(reset_row, M.nrows);
            if (lane < ND) {
                const int c = SM.dof_coord[lane];
                qd = M.ref_q[r][c];
                ud = M.ref_u[r][c];
            }
            t = M.ref_time[r];
            istep = M.ref_istep[r];
            has_last = 0;
            rk_hnext = 0;   /* reset_manager: a new integrator (opensim_wrapper.py:287-291) */
            /* initializeState: the default activation.  The held controls stay:
             * the PrescribedController's Constant functions keep the last
             * actuate() through OsimModel.reset (opensim_wrapper.py:92-107,
             * :293-297), so a reset realizes with them — reloaded from HBM
             * (stored when the step computed them) rather than kept in
             * registers through the report (+40 VGPRs in 3D fp64) */
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
                control[j] = m < NA ? GAT(st.ctl, (size_t)m * N + env, (size_t)NA * N) : Real(0);
                if constexpr (NM > 0)
                    if (m < NM) act[j] = SM.mus[m].default_act;
                /* CACHE: the reset realize's fiber-velocity roots start cold,
                 * as the reset table's do (build_reset_table), so the cache row
                 * it leaves is the table's bit for bit */
                if constexpr (CACHE) D.ms[j].vN = 0;
            }
            resets += 1;
            /* an auto-reset's realize follows a report, whose staging (OBS,
             * REP) lies over the identity LOC slot: written again (the
             * report's last LDS reads are behind its closing sync) */
            if constexpr (TS::GROUND && ground_loc_free<T, Real>())
                if (lane == T::NB) kin_ground_loc<T, Real>(lds);
        }
        if constexpr (CACHE) {
            /* the first substep from the cache; a realize (step or reset) forms
             * the cache at the next step's substep length (begin_integrate's
             * arithmetic for istep + 1) */
            CI.use = cache_valid && sub && remaining == M.nsub && cache_h == dt;
            cache_valid = false;
            CI.make = !sub;
            if (!sub) {
                const double tf = M.step_size * (double)(istep + 1);
                const double hstep = tf - t;
                CI.hc = Real(hstep / (double)M.nsub);
            }
        }
        {
            /* opaque per-iteration model pointer: keeps the compiler from
             * hoisting hundreds of loop-invariant constants into registers
             * (they are re-read from the scalar cache instead of spilled) */
            typedef const __attribute__((address_space(4))) DModel<Real> CModel;
            CModel *Mi = (CModel *)Mg;
            asm volatile("" : "+s"(Mi));
            /* realize / reset realize: the call time is t itself */
            if (PERT && !sub && lane == 0) { pslot[0] = t; pslot[1] = 0; }
            if (RK && PERT && sub && lane == 0) {
                const double cs = rk_stage == 0 ? 0.0 : rk_stage <= 2 ? 1.0 / 3.0 : rk_stage == 3 ? 0.5 : 1.0;
                pslot[0] = rk_t + cs * rk_h; pslot[1] = 0;
            }
#if BIOIM_FV_PRED
            if constexpr (!RK && NM > 0) {
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const Real vc = D.ms[j].vN;
                    D.ms[j].vN = vc + (vc - vprev[j]);
                    vprev[j] = vc;
                }
            }
#endif
            /* RK: explicit accelerations (h = 0, the implicit terms compile away) */
            /* branch-free phase-3 row stores, except in the spatial RK kernels
             * (they would take those kernels past the 512-register budget) */
            dynamics<T, Real, PERT, !RK || T::PLANAR, !RK, CACHE, TS, EXT>(*(const DModel<Real> *)Mi, SM, qd, ud, act, lce, control, lane, lds,
                                    RK ? Real(0) : (sub ? dt : Real(0)), eq && NM > 0, PA, pslot,
                                    RK ? 0 : M.nsub - remaining, D, CI, LX, XE);
        }
        if (RK && sub) {
            const Real h = Real(rk_h);
            if (lane < ND) {
                const Real fq = ud, fu = D.qdd;
                rk_update<Real>(rk_stage, h, fq, qd, y0q, Kq, Eq, rk_err);
                rk_update<Real>(rk_stage, h, fu, ud, y0u, Ku, Eu, rk_err);
            }
            if constexpr (NM > 0) {
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const int m = mslot<T>(lane + j * G);
                    if (m < NM) {
                        const Real fl = D.ms[j].clamped ? Real(0) : D.ms[j].vce;
                        rk_update<Real>(rk_stage, h, D.ms[j].dadt, act[j], y0a[j], Ka[j], Ea[j], rk_err);
                        rk_update<Real>(rk_stage, h, fl, lce[j], y0l[j], Kl[j], El[j], rk_err);
                    }
                }
            }
            if (rk_stage < 4) {
                ++rk_stage;
                continue;
            }
            rk_stage = 0;
            Real e = isnan(rk_err) ? Real(INFINITY) : rk_err;
            e = group_max<G>(e);
            const double err = (double)e;
            double fac = err > 0 ? 0.9 * sqrt(sqrt(a.rk_acc / err)) : 5.0;
            if (!(fac == fac)) fac = 0.1;
            fac = fac < 0.1 ? 0.1 : (fac > 5.0 ? 5.0 : fac);
            if (err <= a.rk_acc) {
                if constexpr (NM > 0) {
#pragma unroll
                    for (int j = 0; j < MPL; ++j) {
                        const int m = mslot<T>(lane + j * G);
                        if (m < NM && lce[j] < SM.mus[m].lmin) lce[j] = SM.mus[m].lmin;
                    }
                }
                rk_t = rk_last ? rk_tf : rk_t + rk_h;
                if (!rk_last) rk_hnext = rk_h * fac;
                if (a.traj) {   /* the Manager stores every accepted step (opensim_wrapper.py:336) */
                    if (traj_k < a.traj_cap) {
                        Real *row = a.traj + GIDX(((size_t)env * a.traj_cap + traj_k), (size_t)N * a.traj_cap) * a.traj_dim;
                        if (lane == 0) GAT(row, 0, a.traj_dim) = Real(rk_t);
                        if (lane < ND) { GAT(row, 1 + lane, a.traj_dim) = qd; GAT(row, 1 + ND + lane, a.traj_dim) = ud; }
                        if constexpr (NM > 0) {
#pragma unroll
                            for (int j = 0; j < MPL; ++j) {
                                const int m = mslot<T>(lane + j * G);
                                if (m < NM) { GAT(row, 1 + 2 * ND + m, a.traj_dim) = act[j]; GAT(row, 1 + 2 * ND + NM + m, a.traj_dim) = lce[j]; }
                            }
                        }
                    }
                    ++traj_k;
                }
            } else {
                qd = y0q; ud = y0u;
#pragma unroll
                for (int j = 0; j < MPL; ++j) { act[j] = y0a[j]; lce[j] = y0l[j]; }
            }
            rk_h *= fac;
            continue;
        }
        if (!RK && sub) {
#ifdef BIOIM_STAMPS
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long su_t0 = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_sched_barrier(0);
#endif
            if (lane < ND) { ud += dt * D.qdd; qd += dt * ud; }
            if constexpr (NM > 0) {
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const int m = mslot<T>(lane + j * G);
                    if (m < NM) {
                        act[j] += dt * D.ms[j].dadt;
                        if (!D.ms[j].clamped) {
#if BIOIM_SUBSTEP_RCP
                            /* a refined hardware reciprocal (fast_rcp) instead of the IEEE
                             * division: the divisor 1 - dt dv/dl is a well-scaled positive
                             * quantity; once per muscle and substep */
                            Real ln = lce[j] + dt * D.ms[j].vce * fast_rcp(Real(1) - dt * D.ms[j].dvdl);
#else
                            Real ln = lce[j] + dt * D.ms[j].vce / (Real(1) - dt * D.ms[j].dvdl);
#endif
                            lce[j] = ln < SM.mus[m].lmin ? SM.mus[m].lmin : ln;
                        }
                    }
                }
            }
#ifdef BIOIM_STAMPS
            {   /* the substep update of the first env of workgroup 0: its results pinned, then the clock */
                asm volatile("" : "+v"(qd), "+v"(ud));
#pragma unroll
                for (int j = 0; j < MPL; ++j) asm volatile("" : "+v"(act[j]), "+v"(lce[j]));
                __builtin_amdgcn_sched_barrier(0);
                const unsigned long long su_t1 = __builtin_amdgcn_s_memtime();
                __builtin_amdgcn_s_waitcnt(0xC07F);
                if (blockIdx.x == 0 && threadIdx.x == 0) g_stamps[24] += su_t1 - su_t0;
                __builtin_amdgcn_sched_barrier(0);
            }
#endif
            --remaining;
            continue;
        }
        if (eq) {
            if constexpr (NM > 0) {
#pragma unroll
                for (int j = 0; j < MPL; ++j)
                    if (lane + j * G < NM) { act[j] = D.act[j]; lce[j] = D.lce[j]; }
            }
            reported_reset = pending_reset;
            pending_reset = false;
            eq_only = false;
        }
                /* ---- realized state: observation (lane-parallel; get_state_dict,
         * muscle_walking_imitation_env2D.py:158-225).  The realize call left
         * the coordinates (QF/UF), frames (KB), contact wrenches (CW) and limit
         * forces (LIM) in LDS; report points first. */
#ifdef BIOIM_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long rp_t0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
#endif
        using OL = ObsLayout<T>;
        const Real x0 = D.x0;
        Real *ob = lds + LY::OBS;
        const bool tgt = (M.env_flags & BIOIM_ENV_TARGET_OBS) != 0, grf = (M.env_flags & BIOIM_ENV_GRF_OBS) != 0;
        if (lane <= T::NOS) report_points<T, Real>(SM, lds, lane, x0);
        wave_sync();
        const Real px = lds[LY::QF + T::TX], py = lds[LY::QF + T::TY];
        Real pz = 0;
        if constexpr (T::TZ >= 0) pz = lds[LY::QF + T::TZ];
        if (lane == 0) {
            double ph = (double)istep / (double)M.cycle;
            ob[0] = Real(ph - floor(ph));
        }
        const int obody = OL::body(tgt);
#pragma unroll
        for (int jc = 0; jc < CPL; ++jc) {
            const int c = lane + jc * G;
            if (c < T::NC) {
                const bool trans = c == T::TX || c == T::TY || c == T::TZ;
                const int qi = c - (T::TX >= 0 && T::TX < c) - (T::TY >= 0 && T::TY < c) - (T::TZ >= 0 && T::TZ < c);
                if (!trans) ob[OL::QPOS + qi] = lds[LY::QF + c];
                ob[OL::QVEL + c] = lds[LY::UF + c];
                const int dc = SM.coord_dof[c];
                ob[OL::QACC + c] = dc >= 0 ? lds[LY::RHS + dc] : Real(0);
                if (tgt && c != T::TX) {
                    const int r1 = clamp_row(istep + 1, M.nrows), ti = c - (T::TX >= 0 && T::TX < c);
                    ob[OL::TGT + ti] = M.ref_q[r1][c];
                    ob[OL::TGT + (T::NC - 1) + ti] = M.ref_u[r1][c];
                }
            }
        }
        if (lane < T::NOBP) {
            const Real *rp = lds + LY::REP + 6 * SM.obs_slot[lane];
            ob[obody + 3 * lane] = rp[0] - px; ob[obody + 3 * lane + 1] = rp[1] - py; ob[obody + 3 * lane + 2] = rp[2] - pz;
        }
        if (lane < T::NOBV) {
            const Real *rp = lds + LY::REP + 6 * SM.obs_slot[T::NOBP + lane];
#pragma unroll
            for (int i = 0; i < 3; ++i) ob[obody + 3 * T::NOBP + 3 * lane + i] = rp[3 + i];
        }
        const int omus = obody + 3 * T::NOBP + 3 * T::NOBV;
        if constexpr (NM > 0) {
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
                if (m < NM) {
                    ob[omus + 3 * m] = D.ms[j].act;
                    ob[omus + 3 * m + 1] = D.ms[j].lce;
                    ob[omus + 3 * m + 2] = D.ms[j].vce;
                }
            }
        }
        if (grf && lane < T::NF) {
            Real F[3] = {0, 0, 0}, Mo[3] = {0, 0, 0};
#pragma unroll
            for (int s2 = 0; s2 < T::NS; ++s2) {
                const Real *cw = lds + LY::CW + 8 * s2;
                const bool mine = SM.sph_force[s2] == lane;
#pragma unroll
                for (int i = 0; i < 3; ++i) { F[i] += mine ? cw[i] : Real(0); Mo[i] += mine ? cw[3 + i] : Real(0); }
            }
            /* moments about the absolute ground origin: (x0,0,0) x F */
            Mo[1] += -x0 * F[2];
            Mo[2] += x0 * F[1];
            const int og = omus + 3 * NM + 6 * lane;
#pragma unroll
            for (int i = 0; i < 3; ++i) { ob[og + i] = F[i] / M.weight; ob[og + 3 + i] = Mo[i] / M.moment; }
        }
        if (a.force_out) {
            /* ForceReporter values (opensim_wrapper.py:10-15): actuation of each
             * muscle (tendon force) or coordinate actuator, the wrench on the feet
             * of each contact force about the ground origin, each limit force */
            Real *fo = a.force_out + GIDX((size_t)env, (size_t)N) * a.force_dim;
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const int m = mslot<T>(lane + j * G);
                if (m < NA) {
                    if constexpr (NM > 0) GAT(fo, m, a.force_dim) = D.ms[j].Ft;
                    else GAT(fo, m, a.force_dim) = control[j] * SM.ca_opt[m];
                }
            }
            if (lane < T::NF) {
                Real F[3] = {0, 0, 0}, Mo[3] = {0, 0, 0};
#pragma unroll
                for (int s2 = 0; s2 < T::NS; ++s2) {
                    const Real *cw = lds + LY::CW + 8 * s2;
                    const bool mine = SM.sph_force[s2] == lane;
#pragma unroll
                    for (int i = 0; i < 3; ++i) { F[i] += mine ? cw[i] : Real(0); Mo[i] += mine ? cw[3 + i] : Real(0); }
                }
                Mo[1] += -x0 * F[2];
                Mo[2] += x0 * F[1];
#pragma unroll
                for (int i = 0; i < 3; ++i) { GAT(fo, NA + 6 * lane + i, a.force_dim) = F[i]; GAT(fo, NA + 6 * lane + 3 + i, a.force_dim) = Mo[i]; }
            }
            if (lane < T::NL) GAT(fo, NA + 6 * T::NF + lane, a.force_dim) = lds[LY::LIM + 4 * lane];
            /* the contact record's foot-side entries: per sphere its force on
             * its OpenSim body and the moment about that body's origin (the
             * HuntCrossleyForce record sums these per body, in ground) */
            if (lane < T::NS) {
                const Real *cw = lds + LY::CW + 8 * lane;
                const Real *rp = lds + LY::REP + 6 * SM.sph_ob[lane];   /* body origin, absolute x */
                const Real O[3] = {rp[0] - x0, rp[1], rp[2]}, F[3] = {cw[0], cw[1], cw[2]};
                Real oxf[3];
                cross3(O, F, oxf);
                Real *fs = fo + NA + 6 * T::NF + T::NL + 6 * lane;
#pragma unroll
                for (int i = 0; i < 3; ++i) { fs[i] = F[i]; fs[3 + i] = cw[3 + i] - oxf[i]; }
            }
        }
        if constexpr (REP) {
            /* the observation rows first, so the report runs with ob's
             * addresses dead (the spatial push + RK report kernel is at 512) */
            wave_sync();
            if (obs)
                for (int k = lane; k < M.obs_dim; k += G) GAT(obs, (size_t)env * a.obs_stride + k, (size_t)N * a.obs_stride) = ob[k];
            wave_sync();
            if (a.osim_out)
                osim_report<T, Real>(M, SM, lds, lane, D, control, t, istep, a.osim_out + GIDX((size_t)env, (size_t)N) * a.osim_dim);
            break;
        }
        wave_sync();
        if (obs)
            for (int k = lane; k < M.obs_dim; k += G) GAT(obs, (size_t)env * a.obs_stride + k, (size_t)N * a.obs_stride) = ob[k];
        if (a.final_obs && !reported_reset)
            for (int k = lane; k < M.obs_dim; k += G) GAT(a.final_obs, (size_t)env * a.obs_stride + k, (size_t)N * a.obs_stride) = ob[k];
        wave_sync();
        if (reported_reset || osim) break;

#ifdef BIOIM_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long rp_t1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
#endif
        /* ---- reward (get_reward) and termination (is_done); group sums are
         * xor butterflies, so every lane holds bitwise-identical totals */
        {
            const int r = clamp_row(istep, M.nrows);
            Real e2 = 0;
#pragma unroll
            for (int jc = 0; jc < CPL; ++jc) {
                const int c = lane + jc * G;
                if (c < T::NC) {
                    Real e = lds[LY::QF + c] - M.ref_q[r][c];
                    e2 += e * e;
                }
            }
            const Real qerr = group_sum<G>(e2) / Real(T::NC);
            Real eb = 0;
            if (lane < BIOIM_NREFBODY) {
                const Real *rp = lds + LY::REP + 6 * SM.rw_slot[lane];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    Real e = rp[i] - M.ref_x[r][lane][i];
                    eb += e * e;
                }
                eb /= Real(3);
            }
            /* rw bodies: 0 COM, 1/2 femur r/l, 3/4 tibia, 5/6 talus, 7/8 calcn */
            const bool odd = (lane & 1) != 0 && lane < BIOIM_NREFBODY, even = (lane & 1) == 0 && lane > 0 && lane < BIOIM_NREFBODY;
            const Real err_com = group_sum<G>(lane == 0 ? eb : Real(0));
            const Real err_r = group_sum<G>(odd ? eb : Real(0));
            const Real err_l = group_sum<G>(even ? eb : Real(0));
            Real position_r = exp(Real(-30) * qerr);
            Real com_r = exp(Real(-20) * err_com);
            Real foot_r = Real(0.5) * exp(Real(-20) * err_r);
            Real foot_l = Real(0.5) * exp(Real(-20) * err_l);
            Real pelvis_x = px;
            Real da2 = 0;
#pragma unroll
            for (int j = 0; j < MPL; ++j) {
                const Real da = lane + j * G < NA ? curr[j] - last[j] : Real(0);
                da2 += da * da;
            }
            Real action_r = exp(-M.action_r_scale * sqrt(group_sum<G>(da2)));
            Real effort, a_error = 0;
            if constexpr (NM > 0) {
                Real an = 0, cot = 0;
#pragma unroll
                for (int j = 0; j < MPL; ++j) {
                    const int m = mslot<T>(lane + j * G);
                    if (m < NM) {
                        an += D.ms[j].act * D.ms[j].act;
                        cot += muscle_cot<Real>(SM.mus[m], D.ms[j], control[j]);
                    }
                }
                a_error = exp(Real(-2) * sqrt(group_sum<G>(an)));
                cot = group_sum<G>(cot) + Real(1.51) * M.total_mass;
                effort = cot / (Real(20) * Real(NM * NM));
            } else {
                Real cn = 0;
#pragma unroll
                for (int j = 0; j < MPL; ++j) cn += lane + j * G < NA ? curr[j] * curr[j] : Real(0);
                effort = sqrt(group_sum<G>(cn)) / (M.max_actuation * Real(NA * NA));
            }
            Real effort_r = exp(-effort / fmax(pelvis_x - old_px + Real(1), Real(1)));
            Real imit = position_r * com_r;
            if constexpr ((T::FLAGS & BIOIM_ENV_REWARD_FEET) != 0) imit *= (foot_l + foot_r);
            rew = (Real(0.5) + M.w_imitate) * imit + M.w_effort * effort_r + M.w_action * action_r;
            inf[0] = position_r; inf[1] = com_r; inf[2] = foot_l; inf[3] = foot_r; inf[4] = a_error;
#pragma unroll
            for (int j = 0; j < MPL; ++j) last[j] = curr[j];
            old_px = pelvis_x;
            /* is_done (muscle_walking_imitation_env2D.py:237-265) */
            const Real torso_y = lds[LY::REP + 6 * T::TORSO + 1];
            Real lmax = 0, amax = 0;
#pragma unroll
            for (int li = 0; li < T::NL; ++li) lmax = fmax(lmax, fabs(lds[LY::LIM + 4 * li]));
            amax = group_max<G>(lane < ND ? fabs(D.qdd) : Real(0));
            int d_ = 0;
            if (torso_y < M.torso_y_min) d_ = 1;
            else if (lmax > M.limit_force_max) d_ = 1;
            else if (amax > M.acc_max) d_ = 1;
            else if (istep >= M.n_episode) d_ = 1;
            else if constexpr ((T::FLAGS & BIOIM_ENV_DONE_CROSS) != 0) {
                if (lds[LY::REP + 6 * T::CALCN_R + 2] - lds[LY::REP + 6 * T::CALCN_L + 2] < 0) d_ = 1;
            }
            if (group_any<G>(lane < ND && (!isfinite(qd) || !isfinite(ud)))) d_ = 1;
            if (!D.ok || rk_fail) d_ = 1;
            done = d_;
        }
        if (lane == 0) {
            if (a.reward) GAT(a.reward, env, N) = rew;
            GAT(a.done_out, env, N) = (uint8_t)done;
        }
        if (a.info && lane < M.info_dim) {
            Real iv = inf[0];
#pragma unroll
            for (int i = 1; i < 5; ++i) iv = lane == i ? inf[i] : iv;
            GAT(a.info, (size_t)env * a.info_stride + lane, (size_t)N * a.info_stride) = iv;
        }
        wave_sync();
#ifdef BIOIM_STAMPS
        {   /* the report of the first env of workgroup 0: observation part, reward + done part, reports */
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long rp_t2 = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_waitcnt(0xC07F);
            if (blockIdx.x == 0 && threadIdx.x == 0) { g_stamps[19] += rp_t1 - rp_t0; g_stamps[20] += rp_t2 - rp_t1; g_stamps[21] += 1; }
            __builtin_amdgcn_sched_barrier(0);
        }
#endif
        if (done && a.auto_reset) {
            pending_reset = true;
            do_reset = true;
            reset_row = draw_index(a.seed, a.env_offset + env, resets, M.reset_hi);
            if constexpr ((!RK || (BIOIM_RESET_TAB_RK && (T::PLANAR || BIOIM_RESET_TAB_RK_SPATIAL))) && !PERT && !REP && !EXT) {
                /* the reset table (LaunchArgs::reset_tab): the state the reset
                 * realize would leave (reference row, default activation,
                 * equilibrium fiber lengths) and its observation, without a
                 * dynamics call and fiber equilibrium in this wave — they made
                 * the launch wait for its slowest wave.  Torque
                 * models: the observation's q'' holds the held torques, so the
                 * row carries M^-1 too and q''_d = q''_d(0) + (M^-1 tau)_d */
                if (a.reset_tab) {
                    const int r = clamp_row(reset_row, M.nrows);
                    const Real *tr = a.reset_tab + (size_t)r * a.reset_tab_dim;
                    if (lane < ND) {
                        const int c = SM.dof_coord[lane];
                        qd = M.ref_q[r][c];
                        ud = M.ref_u[r][c];
                    }
                    t = M.ref_time[r];
                    istep = M.ref_istep[r];
                    has_last = 0;
                    rk_hnext = 0;   /* reset_manager: a new integrator (opensim_wrapper.py:287-291) */
                    resets += 1;
                    if constexpr (RK) launch_evals -= 1;   /* no reset realize ran: not an evaluation */
                    if constexpr (NM > 0) {
#pragma unroll
                        for (int j = 0; j < MPL; ++j) {
                            const int m = mslot<T>(lane + j * G);
                            if (m < NM) { act[j] = SM.mus[m].default_act; lce[j] = tr[m]; }
                        }
                        if (obs)
                            for (int k = lane; k < M.obs_dim; k += G)
                                GAT(obs, (size_t)env * a.obs_stride + k, (size_t)N * a.obs_stride) = tr[NM + k];
                        if constexpr (CACHE) {   /* the row's realize cache (after its observation) */
                            using CL = CacheLay<T>;
                            const Real *tc = tr + NM + M.obs_dim;
                            Real *const crow = CI.row();
                            for (int k = lane; k < CL::DIM; k += G) GAT(crow, k, CL::DIM) = tc[k];
                        }
                    } else {
                        /* the held torques per dof, gathered as in the dynamics
                         * call (TAU slots, SM.tau_src), then q'' per dof lane */
                        constexpr int NI = ND * ND;
                        if (lane == 0) lds[LY::TAU + LY::TZ] = Real(0);
#pragma unroll
                        for (int j = 0; j < MPL; ++j) {
                            const int m = mslot<T>(lane + j * G);
                            if (m < NA) lds[LY::TAU + (lane + j * G) * T::MAXSPAN] = control[j] * SM.ca_opt[m];
                        }
                        wave_sync();
                        if (lane < ND) {
                            Real tau = 0;
#pragma unroll
                            for (int i = 0; i < T::MAXARM; ++i) tau += lds[LY::TAU + SM.tau_src[lane][i]];
                            lds[LY::RHS + lane] = tau;
                        }
                        wave_sync();
                        Real *ob = lds + LY::OBS;
                        for (int k = lane; k < M.obs_dim; k += G) ob[k] = tr[NI + k];
                        wave_sync();
                        if (lane < ND) {
                            using OL = ObsLayout<T>;
                            const int c = SM.dof_coord[lane];
                            Real x = ob[OL::QACC + c];
#pragma unroll
                            for (int k = 0; k < ND; ++k) x = fma(tr[lane * ND + k], lds[LY::RHS + k], x);
                            ob[OL::QACC + c] = x;
                        }
                        wave_sync();
                        if (obs)
                            for (int k = lane; k < M.obs_dim; k += G)
                                GAT(obs, (size_t)env * a.obs_stride + k, (size_t)N * a.obs_stride) = ob[k];
                        if constexpr (CACHE) {   /* the row's realize cache (after its observation) */
                            using CL = CacheLay<T>;
                            const Real *tc = tr + NI + M.obs_dim;
                            Real *const crow = CI.row();
                            for (int k = lane; k < CL::DIM; k += G) GAT(crow, k, CL::DIM) = tc[k];
                        }
                    }
                    break;
                }
            }
            continue;
        }
        break;
    }

#ifdef BIOIM_STAMPS
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long k_t3 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    /* slot 10: staging barrier to loop exit (as before); slot 25: the loop alone */
    if (blockIdx.x == 0 && threadIdx.x == 0) { g_stamps[10] += k_t3 - k_t1; g_stamps[25] += k_t3 - k_t2; }
    __builtin_amdgcn_sched_barrier(0);
#endif
    /* ---- store state */
        if (lane == 0) {
        GAT(st.t, env, (size_t)N) = t;
        GAT(st.istep, env, (size_t)N) = istep;
        if (!REP) {
            GAT(st.has_last, env, (size_t)N) = has_last;
            GAT(st.old_px, env, (size_t)N) = old_px;
            GAT(st.done, env, (size_t)N) = (mode == 0 && !do_reset && !suspend) ? done : 0;
            GAT(st.resets, env, (size_t)N) = resets;
        }
        if (RK || mode == 1 || (osim && a.osim_op == BIOIM_OSIM_EQUILIBRATE)) GAT(st.hrk, env, (size_t)N) = rk_hnext;
        /* the realize cache: every step or reset of a CACHE kernel ends with a
         * realize (or a reset-table row) that formed this env's row.  The other
         * kernels of such a topology (push, RK, OsimModel calls) change the
         * state without it: the host clears the flags before launching them
         * (launch_impl; a store here cost the spatial push + RK kernel its
         * last registers) */
        if constexpr (CACHE) GAT(st.cache_ok, env, (size_t)N) = 1;
        if constexpr (RK) {
            GAT(st.pend, env, (size_t)N) = suspend ? 1 : 0;
            /* evaluations (low 32 bits): the attempts', plus one realize per
             * finished step and per reset that ran one (a reset-table reset
             * took one back, see above); finished steps (high 32 bits).  Two
             * independent wrapping halves: no carry from one into the other */
            const uint64_t ev0 = GAT(st.rkev, env, (size_t)N);
            const uint32_t ev_lo = (uint32_t)ev0 + (uint32_t)(launch_evals + (suspend ? 0 : 1) + (do_reset && mode == 0 ? 1 : 0));
            const uint32_t ev_hi = (uint32_t)(ev0 >> 32) + (uint32_t)(mode == 0 && !suspend);
            GAT(st.rkev, env, (size_t)N) = ((uint64_t)ev_hi << 32) | ev_lo;
            if (a.traj && (mode == 0 || (osim && a.osim_op == BIOIM_OSIM_INTEGRATE))) GAT(a.traj_n, env, N) = traj_k;
            if (suspend) {
                GAT(st.rkt, env, (size_t)N) = rk_t; GAT(st.rkh, env, (size_t)N) = rk_h; GAT(st.rka, env, (size_t)N) = rk_attempts;
                GAT(a.done_out, env, N) = 0;
            }
            if (mode == 0 && a.ready_out) GAT(a.ready_out, env, N) = suspend ? 0 : 1;
        }
    }
    if (RK && suspend) {
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            const int m = mslot<T>(lane + j * G);
            if (m < NA) GAT(st.cur, (size_t)m * N + env, (size_t)NA * N) = curr[j];
            if (NM > 0 && m < NM) GAT(st.vnw, (size_t)m * N + env, (size_t)(NM > 0 ? NM : 1) * N) = D.ms[j].vN;
        }
    }
    if (lane < ND) {
        GAT(st.q, (size_t)lane * N + env, (size_t)ND * N) = qd;
        GAT(st.u, (size_t)lane * N + env, (size_t)ND * N) = ud;
    }
#pragma unroll
    for (int j = 0; j < MPL; ++j) {
        const int m = mslot<T>(lane + j * G);
        if (NM > 0 && m < NM) { GAT(st.act, (size_t)m * N + env, (size_t)(NM > 0 ? NM : 1) * N) = act[j]; GAT(st.lce, (size_t)m * N + env, (size_t)(NM > 0 ? NM : 1) * N) = lce[j]; }
        if (!REP && m < NA) GAT(st.last, (size_t)m * N + env, (size_t)NA * N) = last[j];
    }
#ifdef BIOIM_STAMPS
    /* the epilogue: loop exit to the state write-back issued */
    __builtin_amdgcn_sched_barrier(0);
    if (blockIdx.x == 0 && threadIdx.x == 0) g_stamps[23] += __builtin_amdgcn_s_memtime() - k_t3;
#endif
}

/* REP: the OsimModel-call kernels (mode 2, bioim_osim): the same code plus
 * the full realize report; separate instantiations, so the step kernels are
 * untouched by it */
template <class T, typename Real, bool PERT, bool RK, bool REP = false>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void env_kernel(LaunchArgs<T, Real> a) {
#ifdef BIOIM_WAVETIME
    const unsigned long long w0 = __builtin_amdgcn_s_memtime();
    if (diag_tid() < BIOIM_WAVETIME_N * 4) { g_fvit[diag_tid()] = 0; g_fvmax[diag_tid()] = 0; g_fvbis[diag_tid()] = 0; }
#endif
    env_block<T, Real, PERT, RK, REP>(a, blockIdx.x);
#ifdef BIOIM_WAVETIME
    const unsigned w = blockIdx.x * (BIOIM_EPB * T::G / 64) + threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0 && w < BIOIM_WAVETIME_N) g_wavetime[w] = __builtin_amdgcn_s_memtime() - w0;
#endif
}

/* EXT: the external-force kernels (bioim_set_external_forces) — the
 * semi-implicit step (modes 0 and 1) and its REP variant with the env's held
 * wrenches added in the dynamics call; separate instantiations under a name
 * of their own, so every other kernel is untouched by them */
template <class T, typename Real, bool REP>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void env_kernel_ext(LaunchArgs<T, Real> a, ExtArgs<Real> x) {
    env_block<T, Real, false, false, REP, false, true>(a, blockIdx.x, x);
}


/* Fused two-topology step (a mixed batch, config C5, in ONE launch):
 * workgroups [0, a0.blocks) step segment 0 with topology T0, the rest segment
 * 1 with T1.  Both segments are the default step kernels' code (no push
 * table, semi-implicit); the two bodies sit in one kernel, so its registers
 * are the larger of the two (the 3D pair: 462, no scratch, hazard gate clean).
 * Instantiated for the pairs in BIOIM_FUSED_PAIRS, in the library's fused
 * unit (-DBIOIM_FUSED_ONLY). */
template <class T0, class T1, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T0::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void env_kernel2(
    LaunchArgs<T0, Real> a0, LaunchArgs<T1, Real> a1) {
    static_assert(T0::G == T1::G, "a fused launch needs one workgroup shape");
    if ((int)blockIdx.x < a0.blocks) env_block<T0, Real, false, false, false, true>(a0, blockIdx.x);
    else env_block<T1, Real, false, false, false, true>(a1, blockIdx.x - a0.blocks);
}

/* Fused multi-step rollout (bioim_rollout): `steps` consecutive env steps of
 * the default step kernel's code in ONE launch.  Envs never talk to each
 * other and a lane group loads its env's record, advances it and stores it
 * back, so step k+1 of an env needs only what its own workgroup wrote in step
 * k: no grid-wide synchronisation.  a0 holds step 0's arguments; step k runs
 * env_block on a copy with the I/O pointers at that step's slices. */
template <typename Real> struct RolloutSeq {
    int steps, stop_at_done;
    int64_t act_step;      /* elements between two steps' action blocks (0: the same actions every step) */
    Real *obs_seq;         /* optional [steps][N][obs_stride] */
    Real *obs_last;        /* optional [N][obs_stride]: the last step's rows */
    Real *reward_seq;      /* optional [steps][N] */
    uint8_t *done_seq;     /* [steps][N] */
    Real *info_seq;        /* optional [steps][N][info_stride] */
    uint8_t *live;         /* stop_at_done: per-handle scratch mask [N], this launch's active mask */
    const uint8_t *active; /* the caller's active mask (bioim_set_active_mask) or null */
};

/* step k's view of the launch arguments */
template <class T, typename Real>
DEV LaunchArgs<T, Real> rollout_step_args(const LaunchArgs<T, Real> &a0, const RolloutSeq<Real> &r, int k) {
    LaunchArgs<T, Real> a = a0;
    const size_t N = (size_t)a0.N;
    a.actions = a0.actions + (size_t)k * (size_t)r.act_step;
    /* without a sequence buffer the observation goes to obs_last: from the
     * last step only, or from every step when envs can freeze at their
     * terminal one (stop_at_done) */
    a.obs = r.obs_seq ? r.obs_seq + (size_t)k * N * a0.obs_stride
                      : (k == r.steps - 1 || r.stop_at_done ? r.obs_last : nullptr);
    a.reward = r.reward_seq ? r.reward_seq + (size_t)k * N : nullptr;
    a.done_out = r.done_seq + (size_t)k * N;
    a.info = r.info_seq ? r.info_seq + (size_t)k * N * a0.info_stride : nullptr;
    if (r.stop_at_done) a.active = r.live;
    return a;
}

/* This thread's lane in its env's group and the env, for the rollout loop's
 * bookkeeping — not from threadIdx: that register would be live across the
 * step code, where the register allocator may park a value in an AGPR under
 * the narrowed EXEC that follows env_block's early returns, with the lanes
 * that returned left out (the hazard of DESIGN.md 5.5; a frozen env's lanes
 * are such lanes, and they store rows afterwards).  The wave's index in the
 * workgroup is a scalar, which EXEC does not touch; the lane's index in the
 * wave is counted anew where it is needed, in full EXEC. */
DEV int rollout_wave() { return __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6; }   /* at kernel entry: every lane active */
template <class T> DEV void rollout_thread(int wave, int &lane, int &env) {
    static_assert(BIOIM_EPB * T::G % 64 == 0, "whole waves");
    /* (as volatile asm: the mbcnt builtins are pure, so the compiler counts
     * once at kernel entry and carries the result through the step code) */
    int in_wave;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(in_wave));
    const int tid = wave * 64 + in_wave;
    lane = tid % T::G;
    env = blockIdx.x * BIOIM_EPB + tid / T::G;
}

template <class T, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_kernel(
    LaunchArgs<T, Real> a0, RolloutSeq<Real> r) {
    constexpr int G = T::G;
    static_assert(G <= 64, "an env's lane group lies in one wave (the mask below is read, then cleared, in program order)");
    /* stop_at_done: this launch's mask starts as the caller's (or all ones);
     * an env the caller masked out is never touched, a live one leaves the
     * mask after its first done */
    const int wave = rollout_wave();
    if (r.stop_at_done) {
        int lane, env;
        rollout_thread<T>(wave, lane, env);
        if (env < a0.N && lane == 0) r.live[env] = !r.active || r.active[env] != 0 ? 1 : 0;
    }
    /* The loop over the steps is written with a second, never-taken entry
     * (steps > 0 is bioim_rollout's contract), so that the optimizer does not
     * see a natural loop: as one it moved the step code's thread-only values
     * (a hundred lane-derived indices, masks and LDS offsets, which env_block
     * forms from threadIdx) in front of the loop and kept them in registers
     * across the whole step body, and the fp64 spatial muscle kernels spilled
     * to scratch.  Values it could still move that way are made opaque below. */
    int k = 0, blk = blockIdx.x;
    LaunchArgs<T, Real> a = a0;
    if (r.steps <= 0) goto meet;
step:
    {
        a = rollout_step_args<T, Real>(a0, r, k);
        /* each step's block index, env count, model and plane pointers are
         * opaque to the compiler: otherwise it forms the step's
         * loop-invariant address parts (a 64-bit pair per state plane and
         * lane: plane + index * N) and model constants once, ahead of the
         * steps, and keeps them in registers across the whole step body */
        blk = blockIdx.x;
        asm volatile("" : "+s"(blk));
        asm volatile("" : "+s"(a.N));
        asm volatile("" : "+s"(a.Mg));
        asm volatile("" : "+s"(a.Sg));
        asm volatile("" : "+s"(a.act_stride), "+s"(a.obs_stride), "+s"(a.info_stride));
        asm volatile("" : "+s"(a.st.q), "+s"(a.st.u), "+s"(a.st.act), "+s"(a.st.lce), "+s"(a.st.hist), "+s"(a.st.last));
        asm volatile("" : "+s"(a.st.vnw), "+s"(a.st.cache), "+s"(a.st.cache_ok));
        /* every thread makes every call: env_block holds a workgroup barrier
         * (before it reads the mask) and returns early only after it */
        env_block<T, Real, false, false, false>(a, blk);
    }
meet:
    {
        /* step k+1 reads what step k stored through global memory (state
         * planes, realize-cache row, cache_ok, the mask): release the stores,
         * meet, acquire — at workgroup scope, the env's lanes share one CU */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (r.stop_at_done) {
            int lane, env;
            rollout_thread<T>(wave, lane, env);
            if (env < a0.N && (!r.active || r.active[env] != 0)) {
                if (r.live[env]) {   /* stepped just now */
                    if (a.done_out[env] && lane == 0) r.live[env] = 0;
                } else {
                    /* a frozen env's later rows: reward 0, done 1, info 0, and
                     * its terminal observation again */
                    if (lane == 0) {
                        if (a.reward) a.reward[env] = Real(0);
                        a.done_out[env] = 1;
                    }
                    if (a.info && lane < a0.Mg->info_dim) a.info[(size_t)env * a0.info_stride + lane] = Real(0);
                    if (r.obs_seq) {
                        Real *row = a.obs + (size_t)env * a0.obs_stride;
                        const Real *prev = row - (size_t)a0.N * a0.obs_stride;
                        for (int j = lane; j < a0.Mg->obs_dim; j += G) row[j] = prev[j];
                    }
                }
            }
        }
        if (++k < r.steps) goto step;
    }
    /* with a sequence buffer the last rows also go to obs_last (envs the step
     * left untouched keep theirs, as with bioim_step); the rows were stored
     * before the loop's last barrier */
    if (r.obs_seq && r.obs_last) {
        int lane, env;
        rollout_thread<T>(wave, lane, env);
        if (env < a0.N && (!a0.active || a0.active[env] != 0)) {
            const Real *last = r.obs_seq + ((size_t)(r.steps - 1) * a0.N + env) * a0.obs_stride;
            Real *row = r.obs_last + (size_t)env * a0.obs_stride;
            for (int j = lane; j < a0.Mg->obs_dim; j += G) row[j] = last[j];
        }
    }
}

/* Fused multi-step rollout of a two-segment mixed batch (bioim_rollout_group):
 * rollout_kernel crossed with env_kernel2.  Workgroups [0, a0.blocks) run
 * segment 0's rollout loop with topology T0, the rest segment 1's with T1, on
 * the block index counted from the segment's first workgroup.  Each segment's
 * base pointers (a0 / a1 and r0 / r1) are already offset by its first row of
 * the padded full-batch buffers, so env indices stay segment-local; only the
 * per-step pitch of the sequence buffers is the whole batch's: `rows` rows,
 * not the segment's a.N.  The loop is rollout_kernel's, with every register
 * measure it takes; it is a separate body, so that kernel's
 * code stays as it is.  Every thread of a workgroup takes the same branch:
 * the barriers stay uniform. */
template <class T, typename Real>
DEV LaunchArgs<T, Real> rollout2_step_args(const LaunchArgs<T, Real> &a0, const RolloutSeq<Real> &r, int k, size_t rows) {
    LaunchArgs<T, Real> a = a0;
    a.actions = a0.actions + (size_t)k * (size_t)r.act_step;
    a.obs = r.obs_seq ? r.obs_seq + (size_t)k * rows * a0.obs_stride
                      : (k == r.steps - 1 || r.stop_at_done ? r.obs_last : nullptr);
    a.reward = r.reward_seq ? r.reward_seq + (size_t)k * rows : nullptr;
    a.done_out = r.done_seq + (size_t)k * rows;
    a.info = r.info_seq ? r.info_seq + (size_t)k * rows * a0.info_stride : nullptr;
    if (r.stop_at_done) a.active = r.live;
    return a;
}

/* rollout_thread with the segment's first workgroup `blk0` (a scalar) taken
 * off the block index */
template <class T> DEV void rollout2_thread(int wave, int blk0, int &lane, int &env) {
    static_assert(BIOIM_EPB * T::G % 64 == 0, "whole waves");
    int in_wave;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(in_wave));
    const int tid = wave * 64 + in_wave;
    lane = tid % T::G;
    env = ((int)blockIdx.x - blk0) * BIOIM_EPB + tid / T::G;
}

template <class T, typename Real>
DEV void rollout2_segment(const LaunchArgs<T, Real> &a0, const RolloutSeq<Real> &r, const int wave, const int blk0,
                          const int rows_total) {
    constexpr int G = T::G;
    static_assert(G <= 64, "an env's lane group lies in one wave (the mask below is read, then cleared, in program order)");
    const size_t rows = (size_t)rows_total;
    if (r.stop_at_done) {
        int lane, env;
        rollout2_thread<T>(wave, blk0, lane, env);
        if (env < a0.N && lane == 0) r.live[env] = !r.active || r.active[env] != 0 ? 1 : 0;
    }
    /* the never-taken second loop entry and the opaque scalar operands of
     * rollout_kernel, for the reasons given there */
    int k = 0, blk = (int)blockIdx.x - blk0;
    LaunchArgs<T, Real> a = a0;
    if (r.steps <= 0) goto meet;
step:
    {
        a = rollout2_step_args<T, Real>(a0, r, k, rows);
        blk = (int)blockIdx.x - blk0;
        asm volatile("" : "+s"(blk));
        asm volatile("" : "+s"(a.N));
        asm volatile("" : "+s"(a.Mg));
        asm volatile("" : "+s"(a.Sg));
        asm volatile("" : "+s"(a.act_stride), "+s"(a.obs_stride), "+s"(a.info_stride));
        asm volatile("" : "+s"(a.st.q), "+s"(a.st.u), "+s"(a.st.act), "+s"(a.st.lce), "+s"(a.st.hist), "+s"(a.st.last));
        asm volatile("" : "+s"(a.st.vnw), "+s"(a.st.cache), "+s"(a.st.cache_ok));
        env_block<T, Real, false, false, false, true>(a, blk);
    }
meet:
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (r.stop_at_done) {
            int lane, env;
            rollout2_thread<T>(wave, blk0, lane, env);
            if (env < a0.N && (!r.active || r.active[env] != 0)) {
                if (r.live[env]) {   /* stepped just now */
                    if (a.done_out[env] && lane == 0) r.live[env] = 0;
                } else {
                    if (lane == 0) {
                        if (a.reward) a.reward[env] = Real(0);
                        a.done_out[env] = 1;
                    }
                    if (a.info && lane < a0.Mg->info_dim) a.info[(size_t)env * a0.info_stride + lane] = Real(0);
                    if (r.obs_seq) {
                        /* the previous step's row: one whole batch of rows back */
                        Real *row = a.obs + (size_t)env * a0.obs_stride;
                        const Real *prev = row - rows * a0.obs_stride;
                        for (int j = lane; j < a0.Mg->obs_dim; j += G) row[j] = prev[j];
                    }
                }
            }
        }
        if (++k < r.steps) goto step;
    }
    if (r.obs_seq && r.obs_last) {
        int lane, env;
        rollout2_thread<T>(wave, blk0, lane, env);
        if (env < a0.N && (!a0.active || a0.active[env] != 0)) {
            const Real *last = r.obs_seq + ((size_t)(r.steps - 1) * rows + env) * a0.obs_stride;
            Real *row = r.obs_last + (size_t)env * a0.obs_stride;
            for (int j = lane; j < a0.Mg->obs_dim; j += G) row[j] = last[j];
        }
    }
}

template <class T0, class T1, typename Real>
__global__ __launch_bounds__(BIOIM_EPB * T0::G) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_kernel2(
    LaunchArgs<T0, Real> a0, RolloutSeq<Real> r0, LaunchArgs<T1, Real> a1, RolloutSeq<Real> r1, int rows_total) {
    static_assert(T0::G == T1::G, "a fused launch needs one workgroup shape");
    const int wave = rollout_wave();
    if ((int)blockIdx.x < a0.blocks) rollout2_segment<T0, Real>(a0, r0, wave, 0, rows_total);
    else rollout2_segment<T1, Real>(a1, r1, wave, a0.blocks, rows_total);
}

#define BIOIM_FUSED_PAIRS(X)                                                         \
    X(Topo_MuscleLockedKneeImitation3D_v0, Topo_MuscleWalkingImitation3D_v0)          \
    X(Topo_MuscleWalkingImitation3D_v0, Topo_MuscleLockedKneeImitation3D_v0)

/* The pairs rollout_kernel2 is instantiated for.  A group of BIOIM_FUSED_PAIRS
 * in the other order runs the same instantiation with the two argument sets
 * swapped (which segment takes the low block indices changes no result): the
 * <LockedKnee3D, Walking3D> instantiation did not clear the hazard gate
 * (DESIGN.md 5.13). */
#define BIOIM_ROLLOUT_PAIRS(X)                                                       \
    X(Topo_MuscleWalkingImitation3D_v0, Topo_MuscleLockedKneeImitation3D_v0)

/* =================================================================== host
 * Build modes (the library links 8 objects compiled in parallel):
 *   BIOIM_TOPO_ONLY=k  the kernels and host launchers of topology k only
 *                      (bioim_pick_k);
 *   BIOIM_ABI_ONLY     the C-ABI, no kernels;
 *   BIOIM_FUSED_ONLY   the fused two-topology kernels (BIOIM_FUSED_PAIRS) and their launcher;
 *   neither            everything in one translation unit (diagnostic builds). */
#if defined(BIOIM_TOPO_ONLY) + defined(BIOIM_ABI_ONLY) + defined(BIOIM_FUSED_ONLY) > 1
#error "BIOIM_TOPO_ONLY, BIOIM_ABI_ONLY and BIOIM_FUSED_ONLY are exclusive"
#endif
extern thread_local std::string g_err;   /* bioim_last_error(); defined with the C-ABI */

namespace {

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(x)                                                                       \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) return fail(BIOIM_E_DEVICE, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

double host_bez5(const double *p, double u) {
    double v = 1.0 - u;
    return p[0] * v * v * v * v * v + 5 * p[1] * u * v * v * v * v + 10 * p[2] * u * u * v * v * v +
           10 * p[3] * u * u * u * v * v + 5 * p[4] * u * u * u * u * v + p[5] * u * u * u * u * u;
}

double host_dbez5(const double *p, double u) {
    double v = 1.0 - u;
    return 5 * ((p[1] - p[0]) * v * v * v * v + 4 * (p[2] - p[1]) * u * v * v * v +
                6 * (p[3] - p[2]) * u * u * v * v + 4 * (p[4] - p[3]) * u * u * u * v + (p[5] - p[4]) * u * u * u * u);
}

/* exact inverse of the monotone quintic x(u) by bisection (host, table build) */
double host_invert(const double *px, double x) {
    double lo = 0.0, hi = 1.0;
    for (int it = 0; it < 200; ++it) {
        double m = 0.5 * (lo + hi);
        if (host_bez5(px, m) > x) hi = m; else lo = m;
    }
    return 0.5 * (lo + hi);
}

/* y(x) of a pack curve, to machine precision (the device's curve_eval
 * semantics: linear extrapolation outside [x0, x1]) */
double host_curve_y(const bioim_curve_t &s, double x) {
    if (x < s.x0) return s.y0 + s.dydx0 * (x - s.x0);
    if (x > s.x1) return s.y1 + s.dydx1 * (x - s.x1);
    int k = 0;
    while (k < s.nseg - 1 && x > s.x[k][5]) ++k;
    return host_bez5(s.y[k], host_invert(s.x[k], x));
}

/* Bernstein control points of a quintic -> power-basis coefficients:
 * c_j = C(5, j) sum_{k <= j} C(j, k) (-1)^(j-k) p_k */
void bernstein_to_power(const double *p, double *c) {
    static const double B5[6] = {1, 5, 10, 10, 5, 1};
    for (int j = 0; j < 6; ++j) {
        double s = 0, bjk = 1;   /* C(j, k) */
        for (int k = 0; k <= j; ++k) {
            s += bjk * (((j - k) & 1) ? -p[k] : p[k]);
            bjk = bjk * (j - k) / (k + 1);
        }
        c[j] = B5[j] * s;
    }
}

template <typename Real> void convert_curve(const bioim_curve_t &s, DCurve<Real> &d) {
    for (int i = 0; i < BIOIM_MAX_CURVESEG; ++i) {
        double cx[6], cy[6];
        bernstein_to_power(s.x[i], cx);
        bernstein_to_power(s.y[i], cy);
        for (int j = 0; j < 6; ++j) { d.cx[i][j] = (Real)cx[j]; d.cy[i][j] = (Real)cy[j]; }
        d.xa[i] = i < s.nseg ? (Real)s.x[i][0] : (Real)INFINITY; d.xb[i] = (Real)s.x[i][5];
        d.ya[i] = i < s.nseg ? (Real)s.y[i][0] : Real(0); d.yb[i] = (Real)s.y[i][5];
        d.xsep[i] = i < s.nseg - 1 ? (Real)s.x[i][5] : (Real)INFINITY;
    }
    for (int k = 0; k < BIOIM_MAX_CURVESEG; ++k) {
        if (k >= s.nseg) {
            d.inv_h[k] = 0;
            for (int i = 0; i <= BIOIM_UTAB; ++i) d.ut[k][i] = d.mt[k][i] = 0;
            continue;
        }
        double a = s.x[k][0], b = s.x[k][5];
        d.inv_h[k] = (Real)(BIOIM_UTAB / (b - a));
        for (int i = 0; i <= BIOIM_UTAB; ++i) {
            double u = host_invert(s.x[k], a + (b - a) * i / BIOIM_UTAB);
            d.ut[k][i] = (float)u;
            /* du/dt = (dx/dt) / (dx/du), dx/dt = (b - a) / BIOIM_UTAB */
            d.mt[k][i] = (float)((b - a) / BIOIM_UTAB / host_dbez5(s.x[k], u));
        }
    }
    d.x0 = (Real)s.x0; d.y0 = (Real)s.y0; d.dydx0 = (Real)s.dydx0;
    d.x1 = (Real)s.x1; d.y1 = (Real)s.y1; d.dydx1 = (Real)s.dydx1;
    d.y_at0 = s.nseg > 0 ? (Real)host_curve_y(s, 0.0) : Real(0);
    d.nseg = s.nseg;
}

template <typename Real> void convert_model(const bioim_modelpack_t &p, DModel<Real> &m) {
    memset(&m, 0, sizeof(m));
    for (int c = 0; c < p.ncbody; ++c) {
        for (int i = 0; i < 3; ++i) m.com[c][i] = (Real)p.cbody[c].com[i];
        m.mass[c] = (Real)p.cbody[c].mass;
    }
    for (int c = 0; c < p.ncoord; ++c) { m.coord_default[c] = (Real)p.coord[c].default_value; m.coord_dof[c] = p.coord[c].dof; }
    for (int b = 0; b < p.nosbody; ++b) {
        for (int i = 0; i < 9; ++i) m.os_R[b][i] = (Real)p.osbody[b].R[i];
        for (int i = 0; i < 3; ++i) m.os_p[b][i] = (Real)p.osbody[b].p[i];
    }
    m.w_imitate = (Real)p.w_imitate; m.w_effort = (Real)p.w_effort; m.w_action = (Real)p.w_action;
    m.action_r_scale = (Real)p.action_r_scale; m.max_actuation = (Real)p.max_actuation;
    m.total_mass = (Real)p.total_mass;
    double wgt = fabs(p.total_mass * p.gravity[1]);
    m.weight = (Real)wgt;
    m.moment = (Real)(wgt * p.height);
    m.torso_y_min = (Real)p.torso_y_min; m.limit_force_max = (Real)p.limit_force_max; m.acc_max = (Real)p.acc_max;
    for (int i = 0; i < 3; ++i) m.gravity[i] = (Real)p.gravity[i];
    m.float_origin = 1;
    m.horizon = p.horizon; m.cycle = p.cycle; m.n_episode = p.n_episode; m.reset_hi = p.reset_hi;
    m.nsub = p.nsub; m.nrows = p.nrows; m.obs_dim = p.obs_dim; m.info_dim = p.info_dim; m.env_flags = p.env_flags;
    m.step_size = p.step_size;
    for (int r = 0; r < p.nrows; ++r) {
        m.ref_time[r] = p.ref_time[r];
        m.ref_istep[r] = p.ref_istep[r];
        for (int c = 0; c < p.ncoord; ++c) { m.ref_q[r][c] = (Real)p.ref_q[r][c]; m.ref_u[r][c] = (Real)p.ref_u[r][c]; }
        for (int b = 0; b < BIOIM_NREFBODY; ++b)
            for (int i = 0; i < 3; ++i) m.ref_x[r][b][i] = (Real)p.ref_x[r][b][i];
    }
}

/* distinct muscle curves in first-appearance order over (fal, fv, fpe, fse)
 * of each muscle (tools/build_packs.py: unique_curves) */
static std::vector<const bioim_curve_t *> unique_curves(const bioim_modelpack_t &p, std::vector<int> *index) {
    std::vector<const bioim_curve_t *> u;
    for (int i = 0; i < p.nmuscle; ++i) {
        const bioim_curve_t *cs[4] = {&p.muscle[i].fal, &p.muscle[i].fv, &p.muscle[i].fpe, &p.muscle[i].fse};
        for (const bioim_curve_t *c : cs) {
            int k = 0;
            while (k < (int)u.size() && memcmp(u[k], c, sizeof(bioim_curve_t)) != 0) ++k;
            if (k == (int)u.size()) u.push_back(c);
            if (index) index->push_back(k);
        }
    }
    return u;
}

/* the LDS model image of a pack (layout: bioim_device.h, SModel) */
template <class T, typename Real> void build_smodel(const bioim_modelpack_t &p, SModel<T, Real> &m) {
    memset(&m, 0, sizeof(m));
    std::vector<int> cidx;
    std::vector<const bioim_curve_t *> cu = unique_curves(p, &cidx);
    for (size_t k = 0; k < cu.size(); ++k) convert_curve(*cu[k], m.curve[k]);
    for (int i = 0; i < p.nmuscle; ++i) {
        const bioim_muscle_t &s = p.muscle[i];
        SMuscle<Real> &d = m.mus[i];
        d.fiso = (Real)s.fiso; d.lopt = (Real)s.lopt; d.inv_lopt = (Real)(1.0 / s.lopt);
        d.lts = (Real)s.lts; d.inv_lts = (Real)(1.0 / s.lts); d.lv = (Real)(s.lopt * s.vmax);
        d.tau_act = (Real)s.tau_act; d.tau_deact = (Real)s.tau_deact; d.amin = (Real)s.amin; d.beta = (Real)s.damping;
        d.width = (Real)s.width; d.lmin = (Real)s.lmin; d.slow = (Real)s.slow_twitch; d.mass = (Real)s.mass;
        d.default_act = (Real)s.default_act; d.pt_off = s.pt_off; d.npt = s.npt;
        for (int k = 0; k < 4; ++k) d.cv[k] = cidx[4 * i + k];
        uint32_t root = ~0u, u = 0;
        for (int c = 0; c < T::NB; ++c) root &= T::dofmask[c];
        for (int j = 0; j < s.npt; ++j) u |= T::dofmask[p.pathpt[s.pt_off + j].cbody];
        u &= ~root;
        d.nspan = 0;
        for (int dd = 0; dd < T::ND; ++dd)
            if ((u >> dd) & 1u) d.span[d.nspan++] = dd;
        for (int k = d.nspan; k < BIOIM_MAX_SPAN; ++k) d.span[k] = d.nspan ? d.span[0] : 0;
    }
    {   /* muscle torque gather lists (Lay::TZ: the zero slot) */
        using LY = Lay<T, Real>;
        static_assert(LY::TZ < 256, "TAU slot indices are bytes");
        for (int d = 0; d < SDim<T>::NDD; ++d)
            for (int i = 0; i < T::MAXARM; ++i) m.tau_src[d][i] = (uint8_t)LY::TZ;
        int cnt[SDim<T>::NDD] = {};
        auto add = [&](int d, int slot) {
            if (d >= 0 && d < T::ND && cnt[d] < T::MAXARM) m.tau_src[d][cnt[d]++] = (uint8_t)slot;
        };
        for (int sl = 0; sl < LY::MPL * T::G; ++sl) {
            const int mi = (T::NM > T::G && sl < T::NM) ? T::mperm[sl] : sl;
            if constexpr (T::NM > 0) {
                if (mi < p.nmuscle)
                    for (int k = 0; k < m.mus[mi].nspan; ++k) add(m.mus[mi].span[k], sl * T::MAXSPAN + k);
            } else {
                if (mi < T::NA) add(T::act_dof[mi], sl * T::MAXSPAN);
            }
        }
    }
    std::vector<uint32_t> dofmask(T::NB, 0);
    for (int c = 0; c < T::NB; ++c) dofmask[c] = T::dofmask[c];
    int nmf = 0;
    for (int j = 0; j < p.npathpt; ++j) {
        const bioim_pathpt_t &s = p.pathpt[j];
        DPathPt<Real> &d = m.pt[j];
        d.type = s.type; d.cbody = s.cbody; d.cond_coord = s.cond_coord;
        d.mcoord = -1; d.mdof = -1;
        for (int a = 0; a < 3; ++a) {
            d.mf[a] = -1;
            if (s.type == BIOIM_PT_MOVING && s.fn[a] >= 0) {
                d.mcoord = p.fn[s.fn[a]].coord;
                d.mdof = d.mcoord >= 0 ? p.coord[d.mcoord].dof : -1;
                if (nmf < T::NMF) {
                    m.mf_fn[nmf] = s.fn[a];
                    m.mf_coord[nmf] = p.fn[s.fn[a]].coord;
                    d.mf[a] = nmf;
                }
                ++nmf;
            }
        }
        d.dofmask = dofmask[s.cbody];
        for (int i = 0; i < 3; ++i) { d.loc[i] = (Real)s.loc[i]; d.p[i] = (Real)s.p[i]; }
        for (int i = 0; i < 9; ++i) d.R[i] = (Real)s.R[i];
        d.lo = (Real)s.range_lo; d.hi = (Real)s.range_hi;
    }
    int jslot = T::NMF;   /* joint spline slots follow the moving-point ones */
    for (int c = 0; c < p.ncbody; ++c) {
        const bioim_cbody_t &b = p.cbody[c];
        SBody<Real> &d = m.body[c];
        for (int a = 0; a < 6; ++a) {
            const int fi = p.cbody[c].fn[a];
            if (fi >= 0 && p.fn[fi].type == BIOIM_FN_SPLINE && jslot < TopoInfo<T>::nslot()) {
                m.mf_fn[jslot] = fi;   /* slot TopoInfo<T>::jslot(c, a) */
                m.mf_coord[jslot] = p.fn[fi].coord;
                ++jslot;
            }
        }
        for (int i = 0; i < 9; ++i) { d.R_pf[i] = (Real)b.R_pf[i]; d.R_mb[i] = (Real)b.R_mb[i]; }
        for (int i = 0; i < 3; ++i) { d.p_pf[i] = (Real)b.p_pf[i]; d.p_mb[i] = (Real)b.p_mb[i]; d.com[i] = (Real)b.com[i]; }
        for (int a = 0; a < 6; ++a) {
            for (int i = 0; i < 3; ++i) d.axis[a][i] = (Real)b.axis[a][i];
            d.fa[a] = b.fn[a] >= 0 ? (Real)p.fn[b.fn[a]].a : Real(0);
            d.fb[a] = b.fn[a] >= 0 ? (Real)p.fn[b.fn[a]].b : Real(0);
        }
        d.mass = (Real)b.mass;
        for (int i = 0; i < 6; ++i) d.inertia[i] = (Real)b.inertia[i];
        d.pslot = b.parent >= 0 ? b.parent : T::NB;
        d.pad = 0;
        constexpr int DEP = TopoInfo<T>::depth();
        int path[DEP], n = 0;
        for (int q = c; q >= 0 && n < DEP; q = p.cbody[q].parent) path[n++] = q;
        for (int l = 0; l < DEP; ++l) m.chain[c][l] = l < DEP - n ? T::NB : path[DEP - 1 - l];
    }
    for (int f = 0; f < p.nfn; ++f) {
        m.fn[f].type = p.fn[f].type; m.fn[f].coord = p.fn[f].coord; m.fn[f].off = p.fn[f].knot_off;
        m.fn[f].n = p.fn[f].nknots; m.fn[f].a = (Real)p.fn[f].a; m.fn[f].b = (Real)p.fn[f].b;
    }
    for (int k = 0; k < p.nknots; ++k) {
        m.kx[k] = (Real)p.knot_x[k]; m.ky[k] = (Real)p.knot_y[k]; m.kb[k] = (Real)p.knot_b[k];
        m.kc[k] = (Real)p.knot_c[k]; m.kd[k] = (Real)p.knot_d[k];
    }
    for (int s = 0; s < p.nsphere; ++s) {
        for (int i = 0; i < 3; ++i) m.sph_loc[s][i] = (Real)p.sphere[s].loc[i];
        m.sph_r[s] = (Real)p.sphere[s].radius;
        m.sph_cb[s] = p.sphere[s].cbody; m.sph_force[s] = p.sphere[s].force; m.sph_ob[s] = p.sphere[s].obody;
    }
    for (int f = 0; f < p.ncforce; ++f) {
        const bioim_cforce_t &c = p.cforce[f];
        m.cf_kk[f] = (Real)(0.5 * pow(c.stiffness, 2.0 / 3.0));
        m.cf_c[f] = (Real)c.dissipation; m.cf_ms[f] = (Real)c.static_friction; m.cf_md[f] = (Real)c.dynamic_friction;
        m.cf_mv[f] = (Real)c.viscous_friction; m.cf_vt[f] = (Real)c.transition_velocity;
    }
    for (int l = 0; l < p.nlimit; ++l) {
        const bioim_limit_t &s = p.limit[l];
        m.lim_qup[l] = (Real)s.qup; m.lim_qlow[l] = (Real)s.qlow; m.lim_kup[l] = (Real)s.kup;
        m.lim_klow[l] = (Real)s.klow; m.lim_damp[l] = (Real)s.damping; m.lim_trans[l] = (Real)s.trans;
        m.lim_itrans[l] = (Real)(1.0 / s.trans);
        m.lim_coord[l] = s.coord; m.lim_dof[l] = s.dof;
    }
    for (int a = 0; a < p.ncoordact; ++a) {
        m.ca_opt[a] = (Real)p.coordact[a].optimal_force;
        m.ca_min[a] = (Real)p.coordact[a].min_control;
        m.ca_max[a] = (Real)p.coordact[a].max_control;
        m.act_dof[a] = p.coordact[a].dof;
    }
    for (int a = 0; a < p.nact && a < SDim<T>::NAD; ++a) { m.kp[a] = (Real)p.kp[a]; m.kv[a] = (Real)p.kv[a]; }
    for (int c = 0; c < p.ncoord; ++c) m.coord_dof[c] = p.coord[c].dof;
    for (int c = 0; c < p.ncoord; ++c)
        if (p.coord[c].dof >= 0) { m.dof_cb[p.coord[c].dof] = p.coord[c].cbody; m.dof_coord[p.coord[c].dof] = c; }
    for (int c = 0; c < T::NB; ++c) m.dofmask[c] = T::dofmask[c];
    for (int b = 0; b < T::NOBP; ++b) m.obs_slot[b] = T::obs_bpos[b] >= 0 ? T::obs_bpos[b] : T::NOS;
    for (int b = 0; b < T::NOBV; ++b) m.obs_slot[T::NOBP + b] = T::obs_bvel[b] >= 0 ? T::obs_bvel[b] : T::NOS;
    for (int b = 0; b < BIOIM_NREFBODY; ++b) m.rw_slot[b] = T::rw_body[b] >= 0 ? T::rw_body[b] : T::NOS;
    for (int b = 0; b < T::NOS; ++b) {
        m.os_cb[b] = p.osbody[b].cbody;
        for (int i = 0; i < 3; ++i) m.os_p[b][i] = (Real)p.osbody[b].p[i];
    }
}

/* structural match of a pack against a compiled topology */
/* the pack keeps every motion in the x-y plane (tools/build_packs.py:
 * is_planar; the PLANAR kernels carry planar frames' zeros as constants) */
static bool pack_is_planar(const bioim_modelpack_t &p) {
    auto zrot = [](const double *R) { return R[2] == 0 && R[5] == 0 && R[6] == 0 && R[7] == 0 && R[8] == 1; };
    for (int c = 0; c < p.ncbody; ++c) {
        const bioim_cbody_t &b = p.cbody[c];
        if (!zrot(b.R_pf) || !zrot(b.R_mb)) return false;
        for (int a = 0; a < 6; ++a) {
            const int fi = b.fn[a];
            if (fi < 0) continue;
            if (a < 3 && !(b.axis[a][0] == 0 && b.axis[a][1] == 0)) return false;
            if (a >= 3 && p.fn[fi].type != BIOIM_FN_CONST && b.axis[a][2] != 0) return false;
        }
    }
    return p.gravity[2] == 0;
}

template <class T> bool topology_matches(const bioim_modelpack_t &p) {
    if (T::PLANAR && !pack_is_planar(p)) return false;
    if (p.ncbody != T::NB || p.ndof != T::ND || p.ncoord != T::NC || p.nmuscle != T::NM || p.nact != T::NA ||
        p.nsphere != T::NS || p.ncforce != T::NF || p.nlimit != T::NL || p.nosbody != T::NOS ||
        p.n_obs_bpos != T::NOBP || p.n_obs_bvel != T::NOBV)
        return false;
    if (p.coord_tx != T::TX || p.coord_ty != T::TY || p.coord_tz != T::TZ) return false;
    for (int s = 0; s < p.nsphere; ++s)   /* the report slot a sphere's foot-side record reads */
        if (p.sphere[s].obody < 0 || p.sphere[s].obody >= p.nosbody || T::os_cb[p.sphere[s].obody] != p.sphere[s].cbody)
            return false;
    if (p.npathpt != T::NPT || p.nfn != T::NFN || p.nknots != T::NKNOT) return false;
    {   /* moving-point function slots and muscle spans fit the compiled sizes */
        int nmf = 0;
        for (int j = 0; j < p.npathpt; ++j)
            for (int a = 0; a < 3; ++a) nmf += (p.pathpt[j].type == BIOIM_PT_MOVING && p.pathpt[j].fn[a] >= 0) ? 1 : 0;
        if (nmf != T::NMF) return false;
        uint32_t root = ~0u;
        for (int c = 0; c < T::NB; ++c) root &= T::dofmask[c];
        int arms[32] = {};
        for (int i = 0; i < p.nmuscle; ++i) {
            uint32_t u = 0;
            for (int j = 0; j < p.muscle[i].npt; ++j) u |= T::dofmask[p.pathpt[p.muscle[i].pt_off + j].cbody];
            if (__builtin_popcount(u & ~root) > T::MAXSPAN || T::MAXSPAN > BIOIM_MAX_SPAN) return false;
            for (int d = 0; d < T::ND; ++d) arms[d] += ((u & ~root) >> d) & 1u;
        }
        for (int d = 0; d < T::ND; ++d)
            if (arms[d] > T::MAXARM) return false;
    }
    for (int f = 0; f < p.nfn; ++f)
        if (p.fn[f].nknots > T::NKMAX) return false;
    if ((int)unique_curves(p, nullptr).size() != T::NCURVE) return false;
    if (p.nmuscle == 0 && p.nact > SDim<T>::NAD) return false;
    if (p.torso_body != T::TORSO || p.calcn_r_body != T::CALCN_R || p.calcn_l_body != T::CALCN_L) return false;
    if ((p.env_flags & BIOIM_STRUCT_FLAGS) != T::FLAGS) return false;
    for (int c = 0; c < T::NB; ++c) {
        if (p.cbody[c].parent != T::parent[c]) return false;
        uint32_t m = 1u << c;
        for (int q = p.cbody[c].parent; q >= 0; q = p.cbody[q].parent) m |= 1u << q;
        if (m != T::anc[c]) return false;
        for (int a = 0; a < 6; ++a) {
            int fi = p.cbody[c].fn[a];
            int kind = fi < 0 ? -1 : p.fn[fi].type, cc = fi < 0 ? -1 : p.fn[fi].coord;
            if (kind != T::axis_kind[c * 6 + a] || cc != T::axis_coord[c * 6 + a]) return false;
        }
    }
    for (int c = 0; c < T::NC; ++c)
        if (p.coord[c].dof != T::coord_dof[c]) return false;
    for (int c = 0; c < T::NC; ++c) {
        int d = p.coord[c].dof;
        if (d >= 0 && (p.coord[c].cbody != T::dof_cb[d] || T::dof_coord[d] != c)) return false;
    }
    for (int s = 0; s < T::NS; ++s)
        if (p.sphere[s].cbody != T::sphere_cb[s] || p.sphere[s].force != T::sphere_force[s]) return false;
    for (int b = 0; b < T::NOS; ++b)
        if (p.osbody[b].cbody != T::os_cb[b]) return false;
    for (int l = 0; l < T::NL; ++l)
        if (p.limit[l].dof != T::limit_dof[l] || p.limit[l].coord != T::limit_coord[l]) return false;
    if (p.nmuscle == 0) {
        int arms[32] = {};
        for (int a = 0; a < T::NA; ++a) {
            if (p.coordact[a].dof != T::act_dof[a] || p.pd_coord[a] != T::pd_coord[a] || p.pd_vcoord[a] != T::pd_vcoord[a])
                return false;
            if (T::act_dof[a] >= 0 && ++arms[T::act_dof[a]] > T::MAXARM) return false;
        }
    }
    for (int b = 0; b < T::NOBP; ++b)
        if (p.obs_bpos[b] != T::obs_bpos[b]) return false;
    for (int b = 0; b < T::NOBV; ++b)
        if (p.obs_bvel[b] != T::obs_bvel[b]) return false;
    for (int b = 0; b < BIOIM_NREFBODY; ++b)
        if (p.rw_body[b] != T::rw_body[b]) return false;
    return true;
}

}  // namespace

struct OsimCall {   /* mode 2 launch arguments (bioim_osim) */
    int op;
    const void *controls;
    void *report;
};

struct RolloutCall {   /* bioim_rollout's arguments (untyped), for Ops::rollout */
    const void *actions;
    int steps;
    int64_t act_step;
    void *obs_seq, *obs_last, *reward_seq;
    uint8_t *done_seq;
    void *info_seq;
    int stop_at_done;
};

struct Ops {
    const char *topo;   /* the topology struct's name (fused-pair lookup) */
    int lanes;
    size_t lds_bytes;   /* per workgroup: model image + BIOIM_EPB env regions */
    int cache_dim;      /* reals per env of the realize cache (CacheLay<T>::DIM; 0: none) */
    int (*upload)(bioim_handle_t *);
    void (*launch)(bioim_handle_t *, int mode, const void *actions, void *obs, void *reward, uint8_t *done, void *info,
                   const int32_t *env_ids, const int32_t *ref_index, int n_list, const OsimCall *oc);
    /* the analysis launchers take the entry point's arguments as the kernel's own list with void pointees */
    void (*id_launch)(bioim_handle_t *, const IdFields<void> &);
    /* bioim_muscle_eval's launcher; null for a torque topology (no muscles, no kernel) */
    void (*ma_launch)(bioim_handle_t *, const MaFields<void> &);
    /* bioim_static_opt's launcher; null for a torque topology and for an fp32 handle (fp64 kernels only) */
    void (*so_launch)(bioim_handle_t *, const SoFields<void> &);
    /* bioim_cmc's launcher; null as so_launch is */
    void (*cmc_launch)(bioim_handle_t *, const CmcFields<void> &);
    /* bioim_ik_solve's launcher (every topology); null for an fp32 handle (fp64 kernels only) */
    void (*ik_launch)(bioim_handle_t *, const IkFields<void> &);
    /* bioim_joint_reaction's launcher (every topology, both precisions); < 0: the fp64 image's upload failed */
    int (*jr_launch)(bioim_handle_t *, const JrFields<void> &);
    /* bioim_induced_accel's launcher (every topology); null for an fp32 handle (fp64 kernels only) */
    void (*ia_launch)(bioim_handle_t *, const IaFields<void> &);
    /* bioim_body_kin's launcher (every topology, both precisions) */
    void (*bk_launch)(bioim_handle_t *, const BkFields<void> &);
    /* the fused rollout kernel's launcher; null where that instantiation is
     * left out (bioim_rollout then loops over `launch`) */
    void (*rollout)(bioim_handle_t *, const RolloutCall &);
};

struct bioim_handle {
    int n, device, precision, ndof, nmuscle, nact, horizon, obs_dim, info_dim, nsub, auto_reset, env_offset;
    int act_stride, obs_stride, info_stride; /* I/O row strides (default nact, obs_dim, info_dim) */
    uint64_t seed;
    hipStream_t stream;
    bool own_stream;
    hipStream_t side;     /* private stream: this handle's segment of a concurrent group step */
    hipEvent_t ev_fork, ev_join;
    void *model;        /* DModel<Real> on device */
    void *smodel;       /* SModel<T, Real> on device (staged into LDS per workgroup) */
    void *jr_model, *jr_smodel;   /* fp32 handles: the fp64 DModel / SModel of jr_kernel (null on fp64 handles) */
    void *state_buf;    /* one allocation for every SoA array */
    size_t state_bytes;
    void *dstate;       /* DState<Real> (host copy of pointers) */
    void *pert_x, *pert_y; /* apply_perturbations table: double [pert_n], Real [pert_n][n] */
    int pert_n, pert_ob;
    /* bioim_set_external_forces: the caller's device rows [n][ext_k][9], slot
     * j's OpenSim body in bits [8j, 8j + 8) of ext_body, bit j of ext_ground
     * set for a ground-frame point; ext_k == 0: off */
    const void *ext_wrench;
    int ext_k;
    uint32_t ext_ground;
    uint64_t ext_body;
    void *final_obs;    /* caller's device buffer [n][obs_stride] or null (bioim_set_final_obs) */
    void *force_out;    /* caller's device buffer [n][force_dim] or null (bioim_set_force_report) */
    void *traj;         /* caller's device buffers (bioim_set_state_storage) or null */
    int32_t *traj_n;
    int traj_cap;
    int rk;             /* integrator: 0 semi-implicit substeps (pack nsub), 1 RK-Merson (bioim_set_integrator) */
    double rk_acc;
    int rk_budget;      /* RK attempts per env per launch, 0: unbudgeted (bioim_set_rk_budget) */
    int rk_budgeted;    /* a budget was set at some time: only then can an env be suspended mid-step */
    uint8_t *ready_out; /* caller's device buffer [n] or null */
    const uint8_t *active; /* caller's device buffer [n] or null (bioim_set_active_mask) */
    int last_group_fused; /* the last bioim_step_group with this handle first ran one fused launch */
    void *reset_tab;      /* Real [pack.nrows][reset_table_dim] or null (build_reset_table) */
    int planar;           /* the pack's topology is planar (pack_is_planar) */
    int reset_tab_on;     /* bioim_set_reset_table (default 1) */
    int cache_live;       /* a default step kernel ran since the realize-cache flags were last cleared */
    uint8_t *rollout_live; /* bioim_rollout stop_at_done: scratch mask [n], allocated on first use */
    int last_rollout_fused; /* the last bioim_rollout ran as one launch of the rollout kernel */
    int last_rollout_group_fused; /* the last bioim_rollout_group with this handle first ran as one launch */
    Ops ops;
    bioim_modelpack_t pack;
};

/* the launches that read the reset table: steps of a muscle model with the
 * default kernels (no push table, semi-implicit) and no force report or
 * state storage (their rows come from the reset realize itself) */
static inline bool reset_table_wanted(const bioim_handle_t *h) {
    return h->reset_tab_on && h->auto_reset && h->pert_n == 0 && h->ext_k == 0 && (!h->rk || (BIOIM_RESET_TAB_RK && (h->planar || BIOIM_RESET_TAB_RK_SPATIAL))) &&
           !h->force_out && !h->traj;
}
static inline bool reset_table_eligible(const bioim_handle_t *h) { return h->reset_tab && reset_table_wanted(h); }
/* reals per env of the realize cache (CacheLay) */
static inline int cache_dim(const bioim_handle_t *h) { return h->ops.cache_dim; }
/* reals per table row: muscle models [nmuscle fiber lengths][obs]; torque
 * models [ndof x ndof M^-1, row-major][obs at zero held torques]; then the
 * reset realize's cache row (CacheLay; torque models: without the controls) */
static inline int reset_table_dim(const bioim_handle_t *h) {
    return (h->nmuscle > 0 ? h->nmuscle : h->ndof * h->ndof) + h->obs_dim + cache_dim(h);
}

namespace {

template <class T, typename Real, bool PERT = false> constexpr size_t lds_bytes() {
    return smodel_bytes<T, Real>() + (size_t)BIOIM_EPB * Lay<T, Real>::SIZE * sizeof(Real) +
           (PERT ? (size_t)BIOIM_EPB * PERT_SLOT * sizeof(double) : 0);
}

/* the EXT kernels: the env regions, then the staged rows where they fit (ExtLay) */
template <class T, typename Real> constexpr size_t lds_bytes_ext() {
    return lds_bytes<T, Real, false>() + (ExtLay<T, Real>::LDS ? ExtLay<T, Real>::BYTES : 0);
}

/* bioim_osim_report_dim (include/bioim.h layout) */
int osim_report_dim(const bioim_modelpack_t &p) {
    return 2 + 3 * p.ncoord + 18 * p.nosbody + 9 + 7 * p.nmuscle + p.nact + 6 * p.ncforce + p.nlimit + 1;
}

template <class T, typename Real>
LaunchArgs<T, Real> make_args(bioim_handle_t *h, int mode, const void *actions, void *obs, void *reward, uint8_t *done,
                              void *info, const int32_t *env_ids, const int32_t *ref_index, int n_list,
                              const OsimCall *oc) {
    constexpr int EPB = BIOIM_EPB;
    LaunchArgs<T, Real> a;
    const int count = mode != 0 ? n_list : h->n;
    a.Mg = reinterpret_cast<const DModel<Real> *>(h->model);
    a.Sg = reinterpret_cast<const SModel<T, Real> *>(h->smodel);
    a.st = *reinterpret_cast<DState<Real> *>(h->dstate);
    a.N = h->n; a.mode = mode; a.n_list = n_list; a.auto_reset = h->auto_reset; a.env_offset = h->env_offset;
    a.blocks = (count + EPB - 1) / EPB;
    a.act_stride = h->act_stride; a.obs_stride = h->obs_stride; a.info_stride = h->info_stride;
    a.actions = reinterpret_cast<const Real *>(actions);
    a.obs = reinterpret_cast<Real *>(obs);
    a.final_obs = mode == 0 ? reinterpret_cast<Real *>(h->final_obs) : nullptr;
    a.force_out = reinterpret_cast<Real *>(h->force_out);
    a.force_dim = h->nact + 6 * h->pack.ncforce + h->pack.nlimit + 6 * h->pack.nsphere;   /* bioim_force_report_dim */
    const bool integrates = mode == 0 || (oc && oc->op == BIOIM_OSIM_INTEGRATE);
    a.traj = integrates ? reinterpret_cast<Real *>(h->traj) : nullptr;
    a.traj_n = h->traj_n;
    a.traj_cap = h->traj_cap;
    a.traj_dim = 1 + 2 * h->ndof + 2 * h->nmuscle;
    a.reward = reinterpret_cast<Real *>(reward);
    a.info = reinterpret_cast<Real *>(info);
    a.done_out = done;
    a.env_ids = env_ids; a.ref_index = ref_index;
    a.seed = h->seed;
    a.pert_x = reinterpret_cast<const double *>(h->pert_x);
    a.pert_y = reinterpret_cast<const Real *>(h->pert_y);
    a.pert_n = h->pert_n; a.pert_ob = h->pert_ob;
    a.rk_acc = h->rk_acc;
    a.rk_budget = h->rk && mode == 0 ? h->rk_budget : 0;   /* an OsimModel integrate finishes its step */
    a.ready_out = mode == 0 ? h->ready_out : nullptr;
    a.active = mode == 0 ? h->active : nullptr;
    a.osim_op = oc ? oc->op : 0;
    a.osim_dim = osim_report_dim(h->pack);
    a.controls_in = oc ? reinterpret_cast<const Real *>(oc->controls) : nullptr;
    a.osim_out = oc ? reinterpret_cast<Real *>(oc->report) : nullptr;
    a.reset_tab = mode == 0 && reset_table_eligible(h) ? reinterpret_cast<const Real *>(h->reset_tab) : nullptr;
    a.reset_tab_dim = reset_table_dim(h);
    return a;
}

template <class T, typename Real>
void launch_impl(bioim_handle_t *h, int mode, const void *actions, void *obs, void *reward, uint8_t *done, void *info,
                 const int32_t *env_ids, const int32_t *ref_index, int n_list, const OsimCall *oc) {
    LaunchArgs<T, Real> a = make_args<T, Real>(h, mode, actions, obs, reward, done, info, env_ids, ref_index, n_list, oc);
    if (a.blocks <= 0) return;
    /* the perturbation kernels are separate instantiations, so the default
     * kernels' code is untouched by the (rarely used) push */
    constexpr size_t lds0 = lds_bytes<T, Real, false>(), lds1 = lds_bytes<T, Real, true>();
    const dim3 g(a.blocks), b(BIOIM_EPB * T::G);
    /* the realize cache (CacheLay): only the default step kernels form and
     * read it; before any other kernel changes the state, every env's row is
     * marked stale (once per switch: cache_live says a default launch may
     * have set flags since).  An OsimModel realize reads the state and moves
     * none of it (the REP kernels store q/u/act/lce/t/istep back as loaded;
     * with controls it writes ctl, which the stored system excludes and the
     * next step's actuate replaces): the rows stay valid across it, so a
     * read-only query leaves the next step's bits alone */
    const bool default_kernel = mode != 2 && a.pert_n == 0 && !h->rk && h->ext_k == 0;
    const bool reads_only = mode == 2 && oc && oc->op == BIOIM_OSIM_REALIZE;
    if constexpr (CacheLay<T>::ON) {
        if (!default_kernel && !reads_only && h->cache_live) {
            hipMemsetAsync(a.st.cache_ok, 0, sizeof(int32_t) * (size_t)h->n, h->stream);
            h->cache_live = 0;
        }
        if (default_kernel) h->cache_live = 1;
    }
    if (h->ext_k > 0) {   /* external forces (no push table, semi-implicit: bioim_set_external_forces) */
        ExtArgs<Real> x;
        x.rows = reinterpret_cast<const Real *>(h->ext_wrench);
        x.k = h->ext_k; x.ground = h->ext_ground; x.body = h->ext_body;
        constexpr size_t ldsx = lds_bytes_ext<T, Real>();
        if (mode == 2) hipLaunchKernelGGL((env_kernel_ext<T, Real, true>), g, b, ldsx, h->stream, a, x);
        else hipLaunchKernelGGL((env_kernel_ext<T, Real, false>), g, b, ldsx, h->stream, a, x);
        return;
    }
    if (mode == 2) {   /* OsimModel calls: the REP kernels */
        if (a.pert_n > 0 && h->rk) hipLaunchKernelGGL((env_kernel<T, Real, true, true, true>), g, b, lds1, h->stream, a);
        else if (a.pert_n > 0) hipLaunchKernelGGL((env_kernel<T, Real, true, false, true>), g, b, lds1, h->stream, a);
        else if (h->rk) hipLaunchKernelGGL((env_kernel<T, Real, false, true, true>), g, b, lds0, h->stream, a);
        else hipLaunchKernelGGL((env_kernel<T, Real, false, false, true>), g, b, lds0, h->stream, a);
        return;
    }
    if (a.pert_n > 0 && h->rk) hipLaunchKernelGGL((env_kernel<T, Real, true, true>), g, b, lds1, h->stream, a);
    else if (a.pert_n > 0) hipLaunchKernelGGL((env_kernel<T, Real, true, false>), g, b, lds1, h->stream, a);
    else if (h->rk) hipLaunchKernelGGL((env_kernel<T, Real, false, true>), g, b, lds0, h->stream, a);
    else hipLaunchKernelGGL((env_kernel<T, Real, false, false>), g, b, lds0, h->stream, a);
}

/* one launch of env_kernel2 for the segments h0 (rows [0, n0)) and h1 (the
 * rows after them) of a group step; on h0's stream */
template <class T0, class T1, typename Real>
int fused_launch_impl(bioim_handle_t *h0, bioim_handle_t *h1, const void *actions, void *obs, void *reward,
                      uint8_t *done, void *info) {
    constexpr size_t R = sizeof(Real);
    const size_t n0 = (size_t)h0->n;
    LaunchArgs<T0, Real> a0 = make_args<T0, Real>(h0, 0, actions, obs, reward, done, info, nullptr, nullptr, 0, nullptr);
    LaunchArgs<T1, Real> a1 = make_args<T1, Real>(
        h1, 0, (const char *)actions + n0 * h1->act_stride * R, obs ? (char *)obs + n0 * h1->obs_stride * R : nullptr,
        reward ? (char *)reward + n0 * R : nullptr, done + n0, info ? (char *)info + n0 * h1->info_stride * R : nullptr,
        nullptr, nullptr, 0, nullptr);
    constexpr size_t l0 = lds_bytes<T0, Real, false>(), l1 = lds_bytes<T1, Real, false>();
    constexpr size_t lds = l0 > l1 ? l0 : l1;
    static_assert(lds <= 163840, "LDS image + env regions exceed 160 KiB");
    /* the dynamic-LDS attribute is per device: set it once on each (the
     * per-topology kernels set theirs at handle creation, upload_smodel) */
    static bool attr[64] = {};
    const int dev = h0->device;
    if (dev < 0 || dev >= 64 || !attr[dev]) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&env_kernel2<T0, T1, Real>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (dev >= 0 && dev < 64) attr[dev] = true;
    }
    if (a0.blocks + a1.blocks <= 0) return 0;
    h0->cache_live = 1; h1->cache_live = 1;   /* default step kernels: they form the realize cache */
    hipLaunchKernelGGL((env_kernel2<T0, T1, Real>), dim3(a0.blocks + a1.blocks), dim3(BIOIM_EPB * T0::G), lds,
                       h0->stream, a0, a1);
    return 0;
}

/* one launch of rollout_kernel: the default step configuration only
 * (bioim_rollout checks it), on the handle's stream */
template <class T, typename Real>
void rollout_launch_impl(bioim_handle_t *h, const RolloutCall &c) {
    LaunchArgs<T, Real> a = make_args<T, Real>(h, 0, c.actions, nullptr, nullptr, c.done_seq, nullptr, nullptr, nullptr, 0, nullptr);
    if (a.blocks <= 0) return;
    RolloutSeq<Real> r;
    r.steps = c.steps; r.stop_at_done = c.stop_at_done; r.act_step = c.act_step;
    r.obs_seq = reinterpret_cast<Real *>(c.obs_seq); r.obs_last = reinterpret_cast<Real *>(c.obs_last);
    r.reward_seq = reinterpret_cast<Real *>(c.reward_seq); r.done_seq = c.done_seq;
    r.info_seq = reinterpret_cast<Real *>(c.info_seq);
    r.live = h->rollout_live; r.active = h->active;
    if constexpr (CacheLay<T>::ON) h->cache_live = 1;   /* default step code: it forms the realize cache */
    constexpr size_t lds = lds_bytes<T, Real, false>();
    hipLaunchKernelGGL((rollout_kernel<T, Real>), dim3(a.blocks), dim3(BIOIM_EPB * T::G), lds, h->stream, a, r);
}

/* one segment's arguments of a rollout_kernel2 launch: handle h owns the rows
 * from `off` on of the padded full-batch buffers of c */
template <class T, typename Real>
void rollout2_segment_args(bioim_handle_t *h, const RolloutCall &c, size_t off, LaunchArgs<T, Real> &a, RolloutSeq<Real> &r) {
    const Real *actions = reinterpret_cast<const Real *>(c.actions) + off * h->act_stride;
    Real *obs_seq = reinterpret_cast<Real *>(c.obs_seq), *obs_last = reinterpret_cast<Real *>(c.obs_last);
    Real *reward_seq = reinterpret_cast<Real *>(c.reward_seq), *info_seq = reinterpret_cast<Real *>(c.info_seq);
    a = make_args<T, Real>(h, 0, actions, nullptr, nullptr, c.done_seq + off, nullptr, nullptr, nullptr, 0, nullptr);
    r.steps = c.steps; r.stop_at_done = c.stop_at_done; r.act_step = c.act_step;
    r.obs_seq = obs_seq ? obs_seq + off * h->obs_stride : nullptr;
    r.obs_last = obs_last ? obs_last + off * h->obs_stride : nullptr;
    r.reward_seq = reward_seq ? reward_seq + off : nullptr;
    r.done_seq = c.done_seq + off;
    r.info_seq = info_seq ? info_seq + off * h->info_stride : nullptr;
    r.live = h->rollout_live; r.active = h->active;
}

/* one launch of rollout_kernel2 for a two-segment group rollout: h0 (topology
 * T0, rows from off0 on) takes the low block indices, h1 (T1, rows from off1
 * on) the rest; `rows` is the whole batch's row count, the sequence buffers'
 * per-step pitch; on `stream` (the group's first handle's) */
template <class T0, class T1, typename Real>
int rollout2_launch_impl(bioim_handle_t *h0, size_t off0, bioim_handle_t *h1, size_t off1, const RolloutCall &c, int rows,
                         hipStream_t stream) {
    LaunchArgs<T0, Real> a0;
    LaunchArgs<T1, Real> a1;
    RolloutSeq<Real> r0, r1;
    rollout2_segment_args<T0, Real>(h0, c, off0, a0, r0);
    rollout2_segment_args<T1, Real>(h1, c, off1, a1, r1);
    constexpr size_t l0 = lds_bytes<T0, Real, false>(), l1 = lds_bytes<T1, Real, false>();
    constexpr size_t lds = l0 > l1 ? l0 : l1;
    static_assert(lds <= 163840, "LDS image + env regions exceed 160 KiB");
    static bool attr[64] = {};   /* the dynamic-LDS attribute is per device */
    const int dev = h0->device;
    if (dev < 0 || dev >= 64 || !attr[dev]) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rollout_kernel2<T0, T1, Real>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (dev >= 0 && dev < 64) attr[dev] = true;
    }
    if (a0.blocks + a1.blocks <= 0) return 0;
    h0->cache_live = 1; h1->cache_live = 1;   /* default step code: it forms the realize cache */
    hipLaunchKernelGGL((rollout_kernel2<T0, T1, Real>), dim3(a0.blocks + a1.blocks), dim3(BIOIM_EPB * T0::G), lds, stream,
                       a0, r0, a1, r1, rows);
    return 0;
}

/* an entry point's argument list F<void> as the kernel's F<P>: the same struct but for its pointee type */
template <typename P, template <typename> class F> F<P> typed(const F<void> &c) {
    static_assert(sizeof(F<P>) == sizeof(F<void>) && alignof(F<P>) == alignof(F<void>) &&
                  std::is_standard_layout<F<P>>::value && std::is_trivially_copyable<F<P>>::value,
                  "the argument list must differ in its pointee type only");
    F<P> a;
    memcpy(&a, &c, sizeof a);
    return a;
}

/* Every analysis launch: n states, one per T::G lanes, EPB to a workgroup,
 * `lds` bytes (the model image and EPB state regions) on the handle's stream;
 * model / smodel: the DModel<Real> / SModel<T, Real> images on the device. */
template <int EPB, class T, typename Real, typename P, template <typename> class F>
void analysis_launch(bioim_handle_t *h, void (*kernel)(ModelArgs<T, Real>, F<P>), const F<void> &c, size_t lds,
                     const void *model, const void *smodel) {
    const ModelArgs<T, Real> md{static_cast<const DModel<Real> *>(model), static_cast<const SModel<T, Real> *>(smodel)};
    hipLaunchKernelGGL(kernel, dim3((c.n + EPB - 1) / EPB), dim3(EPB * T::G), lds, h->stream, md, typed<P>(c));
}

template <class T, typename Real> void id_launch_impl(bioim_handle_t *h, const IdFields<void> &c) {
    analysis_launch<BIOIM_EPB>(h, &id_kernel<T, Real>, c, lds_bytes<T, Real, false>(), h->model, h->smodel);
}

template <class T, typename Real> void ma_launch_impl(bioim_handle_t *h, const MaFields<void> &c) {
    analysis_launch<BIOIM_EPB>(h, &ma_kernel<T, Real>, c, lds_bytes<T, Real, false>(), h->model, h->smodel);
}

template <class T> void so_launch_impl(bioim_handle_t *h, const SoFields<void> &c) {
    analysis_launch<BIOIM_EPB>(h, &so_kernel<T, double>, c, lds_bytes<T, double, false>(), h->model, h->smodel);
}

template <class T> void cmc_launch_impl(bioim_handle_t *h, const CmcFields<void> &c) {
    analysis_launch<BIOIM_EPB>(h, &cmc_kernel<T, double>, c, lds_bytes<T, double, false>(), h->model, h->smodel);
}

template <class T> void ik_launch_impl(bioim_handle_t *h, const IkFields<void> &c) {
    analysis_launch<BIOIM_EPB>(h, &ik_kernel<T, double>, c, lds_bytes<T, double, false>(), h->model, h->smodel);
}

/* its own LDS size (IaLay: the env regions plus the private tails) and states per workgroup */
template <class T> void ia_launch_impl(bioim_handle_t *h, const IaFields<void> &c) {
    using IA = IaLay<T, double>;
    analysis_launch<IA::EPB>(h, &ia_kernel<T, double>, c, IA::lds_bytes, h->model, h->smodel);
}

template <class T, typename Real> void bk_launch_impl(bioim_handle_t *h, const BkFields<void> &c) {
    analysis_launch<BIOIM_EPB>(h, &bk_kernel<T, Real>, c, lds_bytes<T, Real, false>(), h->model, h->smodel);
}

/* fp32 handles: the fp64 DModel / SModel of jr_kernel, built from the pack
 * and uploaded on the handle's first bioim_joint_reaction (that call blocks
 * for the two copies; handles that never ask for joint reactions carry
 * nothing); freed with the handle */
template <class T> int jr_fp64_model(bioim_handle_t *h) {
    if (h->jr_smodel) return 0;
    constexpr size_t B = smodel_bytes<T, double>();
    std::vector<unsigned char> img(B, 0);
    build_smodel<T, double>(h->pack, *reinterpret_cast<SModel<T, double> *>(img.data()));
    std::unique_ptr<DModel<double>> hm(new DModel<double>());
    convert_model<double>(h->pack, *hm);
    if (!h->jr_model) HIPCHK(hipMalloc(&h->jr_model, sizeof(DModel<double>)));
    HIPCHK(hipMemcpy(h->jr_model, hm.get(), sizeof(DModel<double>), hipMemcpyHostToDevice));
    void *sm = nullptr;
    HIPCHK(hipMalloc(&sm, B));
    if (hipMemcpy(sm, img.data(), B, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(sm);
        return fail(BIOIM_E_DEVICE, "bioim_joint_reaction: uploading the fp64 model image failed");
    }
    h->jr_smodel = sm;
    return 0;
}

/* IO: the handle's precision (the caller's arrays); the kernel is fp64 either
 * way, on the handle's own image (fp64 handle) or on its fp64 copy (fp32) */
template <class T, typename IO> int jr_launch_impl(bioim_handle_t *h, const JrFields<void> &c) {
    constexpr bool own = std::is_same<IO, double>::value;
    if constexpr (!own) {
        if (const int rc = jr_fp64_model<T>(h)) return rc;
    }
    analysis_launch<BIOIM_EPB>(h, &jr_kernel<T, IO>, c, lds_bytes<T, double, false>(), own ? h->model : h->jr_model,
                               own ? h->smodel : h->jr_smodel);
    return 0;
}

/* the dynamic LDS kernel K (in parentheses) may ask for, above the 64 KiB default; a failure names the kernel */
#define ALLOW_LDS(K, BYTES) \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES)))

template <class T, typename Real> int upload_smodel(bioim_handle_t *h) {
    static_assert(lds_bytes<T, Real, true>() <= 163840, "LDS image + env regions exceed 160 KiB");
    ALLOW_LDS((env_kernel<T, Real, false, false>), (lds_bytes<T, Real, false>()));
    ALLOW_LDS((env_kernel<T, Real, true, false>), (lds_bytes<T, Real, true>()));
    ALLOW_LDS((env_kernel<T, Real, false, true>), (lds_bytes<T, Real, false>()));
    ALLOW_LDS((env_kernel<T, Real, true, true>), (lds_bytes<T, Real, true>()));
    ALLOW_LDS((env_kernel<T, Real, false, false, true>), (lds_bytes<T, Real, false>()));
    ALLOW_LDS((env_kernel<T, Real, true, false, true>), (lds_bytes<T, Real, true>()));
    ALLOW_LDS((env_kernel<T, Real, false, true, true>), (lds_bytes<T, Real, false>()));
    ALLOW_LDS((env_kernel<T, Real, true, true, true>), (lds_bytes<T, Real, true>()));
    static_assert(lds_bytes_ext<T, Real>() <= 163840, "LDS image + env regions + external-force slots exceed 160 KiB");
    ALLOW_LDS((env_kernel_ext<T, Real, false>), (lds_bytes_ext<T, Real>()));
    ALLOW_LDS((env_kernel_ext<T, Real, true>), (lds_bytes_ext<T, Real>()));
    ALLOW_LDS((id_kernel<T, Real>), (lds_bytes<T, Real, false>()));
    ALLOW_LDS((rollout_kernel<T, Real>), (lds_bytes<T, Real, false>()));
    if constexpr (T::NM > 0) ALLOW_LDS((ma_kernel<T, Real>), (lds_bytes<T, Real, false>()));
    if constexpr (T::NM > 0 && std::is_same<Real, double>::value) ALLOW_LDS((so_kernel<T, double>), (lds_bytes<T, double, false>()));
    if constexpr (T::NM > 0 && std::is_same<Real, double>::value) ALLOW_LDS((cmc_kernel<T, double>), (lds_bytes<T, double, false>()));
    if constexpr (std::is_same<Real, double>::value) ALLOW_LDS((ik_kernel<T, double>), (lds_bytes<T, double, false>()));
    ALLOW_LDS((jr_kernel<T, Real>), (lds_bytes<T, double, false>()));
    if constexpr (std::is_same<Real, double>::value) ALLOW_LDS((ia_kernel<T, double>), (IaLay<T, double>::lds_bytes));
    ALLOW_LDS((bk_kernel<T, Real>), (lds_bytes<T, Real, false>()));
    constexpr size_t B = smodel_bytes<T, Real>();
    std::vector<unsigned char> img(B, 0);
    build_smodel<T, Real>(h->pack, *reinterpret_cast<SModel<T, Real> *>(img.data()));
    HIPCHK(hipMalloc(&h->smodel, B));
    HIPCHK(hipMemcpyAsync(h->smodel, img.data(), B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

template <class T> bool pick(const bioim_modelpack_t &p, int precision, Ops &ops, const char *name) {
    if (!topology_matches<T>(p)) return false;
    if (p.obs_dim > Lay<T, double>::OBSMAX) return false;
    ops.topo = name;
    ops.lanes = T::G;
    ops.cache_dim = CacheLay<T>::DIM;
    ops.ma_launch = nullptr;
    ops.so_launch = nullptr;
    ops.cmc_launch = nullptr;
    ops.ik_launch = precision == 64 ? &ik_launch_impl<T> : nullptr;
    ops.ia_launch = precision == 64 ? &ia_launch_impl<T> : nullptr;
    if (precision == 64) ops.jr_launch = &jr_launch_impl<T, double>;
    else ops.jr_launch = &jr_launch_impl<T, float>;
    if (precision == 64) ops.bk_launch = &bk_launch_impl<T, double>;
    else ops.bk_launch = &bk_launch_impl<T, float>;
    if constexpr (T::NM > 0) {
        if (precision == 64) ops.ma_launch = &ma_launch_impl<T, double>;
        else ops.ma_launch = &ma_launch_impl<T, float>;
        if (precision == 64) ops.so_launch = &so_launch_impl<T>;
        if (precision == 64) ops.cmc_launch = &cmc_launch_impl<T>;
    }
    if (precision == 64) {
        ops.launch = &launch_impl<T, double>;
        ops.id_launch = &id_launch_impl<T, double>;
        ops.upload = &upload_smodel<T, double>;
        ops.rollout = &rollout_launch_impl<T, double>;
        ops.lds_bytes = lds_bytes<T, double>();
    } else {
        ops.launch = &launch_impl<T, float>;
        ops.id_launch = &id_launch_impl<T, float>;
        ops.upload = &upload_smodel<T, float>;
        ops.rollout = &rollout_launch_impl<T, float>;
        ops.lds_bytes = lds_bytes<T, float>();
    }
    return true;
}

}  // namespace

/* topology k's kernel table (one object per topology, or all in this TU) */
#define BIOIM_PICK_DECL(S, NAME) bool bioim_pick_##S(const bioim_modelpack_t &p, int precision, Ops &ops);
BIOIM_FOR_EACH_TOPOLOGY(BIOIM_PICK_DECL)
#undef BIOIM_PICK_DECL
/* the fused two-topology launches (the fused unit, or all in this TU):
 * 1 if (h0, h1) is a pair of BIOIM_FUSED_PAIRS and was launched, 0 if not */
int bioim_fused_launch(bioim_handle_t *h0, bioim_handle_t *h1, const void *actions, void *obs, void *reward,
                       uint8_t *done, void *info);
#if defined(BIOIM_FUSED_ONLY) || (!defined(BIOIM_TOPO_ONLY) && !defined(BIOIM_ABI_ONLY))
int bioim_fused_launch(bioim_handle_t *h0, bioim_handle_t *h1, const void *actions, void *obs, void *reward,
                       uint8_t *done, void *info) {
    /* fp64 only: the fp32 fused kernel of the 3D pair spills 68 B/lane; fp32
     * batches keep the concurrent per-segment launches */
    if (h0->precision != 64) return 0;
#define BIOIM_TRY_PAIR(S0, S1)                                                                      \
    if (!strcmp(h0->ops.topo, #S0) && !strcmp(h1->ops.topo, #S1)) {                                  \
        const int rc = fused_launch_impl<S0, S1, double>(h0, h1, actions, obs, reward, done, info);  \
        return rc ? rc : 1;                                                                          \
    }
    BIOIM_FUSED_PAIRS(BIOIM_TRY_PAIR)
#undef BIOIM_TRY_PAIR
    return 0;
}
#endif
/* the fused two-segment rollout (the fused unit, or all in this TU): h0 owns
 * rows [0, n0) of c's padded full-batch buffers, h1 the rows after them.
 * 1 if the pair has a rollout_kernel2 instantiation (BIOIM_ROLLOUT_PAIRS, in
 * either order) and was launched on h0's stream, 0 if not */
int bioim_rollout2_launch(bioim_handle_t *h0, bioim_handle_t *h1, const RolloutCall &c);
#if defined(BIOIM_FUSED_ONLY) || (!defined(BIOIM_TOPO_ONLY) && !defined(BIOIM_ABI_ONLY))
int bioim_rollout2_launch(bioim_handle_t *h0, bioim_handle_t *h1, const RolloutCall &c) {
    if (h0->precision != 64) return 0;   /* as bioim_fused_launch */
    const size_t n0 = (size_t)h0->n;
    const int rows = h0->n + h1->n;
#define BIOIM_TRY_PAIR(S0, S1)                                                                                  \
    if (!strcmp(h0->ops.topo, #S0) && !strcmp(h1->ops.topo, #S1)) {                                              \
        const int rc = rollout2_launch_impl<S0, S1, double>(h0, 0, h1, n0, c, rows, h0->stream);                 \
        return rc ? rc : 1;                                                                                      \
    }                                                                                                            \
    if (!strcmp(h0->ops.topo, #S1) && !strcmp(h1->ops.topo, #S0)) {   /* the argument sets swapped */            \
        const int rc = rollout2_launch_impl<S0, S1, double>(h1, n0, h0, 0, c, rows, h0->stream);                 \
        return rc ? rc : 1;                                                                                      \
    }
    BIOIM_ROLLOUT_PAIRS(BIOIM_TRY_PAIR)
#undef BIOIM_TRY_PAIR
    return 0;
}
#endif
#if !defined(BIOIM_ABI_ONLY) && !defined(BIOIM_FUSED_ONLY)
#define BIOIM_PICK_DEF(S, NAME)                                                      \
    bool bioim_pick_##S(const bioim_modelpack_t &p, int precision, Ops &ops) { return pick<S>(p, precision, ops, #S); }
#ifdef BIOIM_TOPO_ONLY
#define BIOIM_PICK_ONE(S, NAME) BIOIM_PICK_DEF(S, NAME)
BIOIM_TOPOLOGY_AT(BIOIM_TOPO_ONLY, BIOIM_PICK_ONE)
#undef BIOIM_PICK_ONE
#else
BIOIM_FOR_EACH_TOPOLOGY(BIOIM_PICK_DEF)
#endif
#undef BIOIM_PICK_DEF
#endif

#if !defined(BIOIM_TOPO_ONLY) && !defined(BIOIM_FUSED_ONLY)
thread_local std::string g_err;

/* The per-env record: every plane of DState, described once.  The allocation
 * (alloc_state) lays the planes out in this order and sets the DState
 * pointers from it; the clone launch and the single-plane copies (plane_io)
 * walk it too, so a plane added to the state has one place to be listed. */
enum PlaneElem { PE_REAL, PE_F64, PE_I32, PE_U64 };
enum PlaneCount { PC_ONE, PC_NDOF, PC_NM1, PC_HIST, PC_NACT, PC_NA1, PC_CACHE };   /* elements per env */
enum PlaneLayout { PL_SOA, PL_ROWS };   /* [count][N], env fastest | [N][count], row-major per env */
struct StatePlane {
    const char *name;
    size_t member;   /* offset of the plane's pointer in DState (the same for both precisions) */
    PlaneElem elem;
    PlaneCount count;
    PlaneLayout layout;
    bool cloned;
};
#define BIOIM_PLANE(m, elem, count, layout, cloned) {#m, __builtin_offsetof(DState<double>, m), elem, count, layout, cloned}
static constexpr StatePlane g_state_planes[] = {
    BIOIM_PLANE(q, PE_REAL, PC_NDOF, PL_SOA, true),
    BIOIM_PLANE(u, PE_REAL, PC_NDOF, PL_SOA, true),
    BIOIM_PLANE(act, PE_REAL, PC_NM1, PL_SOA, true),
    BIOIM_PLANE(lce, PE_REAL, PC_NM1, PL_SOA, true),
    BIOIM_PLANE(hist, PE_REAL, PC_HIST, PL_SOA, true),
    BIOIM_PLANE(last, PE_REAL, PC_NACT, PL_SOA, true),
    BIOIM_PLANE(old_px, PE_REAL, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(t, PE_F64, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(istep, PE_I32, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(has_last, PE_I32, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(done, PE_I32, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(resets, PE_I32, PC_ONE, PL_SOA, false),   /* the env's share of bioim_reset_count */
    BIOIM_PLANE(hrk, PE_F64, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(pend, PE_I32, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(rkt, PE_F64, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(rkh, PE_F64, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(rka, PE_I32, PC_ONE, PL_SOA, true),
    BIOIM_PLANE(ctl, PE_REAL, PC_NA1, PL_SOA, true),
    BIOIM_PLANE(cur, PE_REAL, PC_NA1, PL_SOA, true),
    BIOIM_PLANE(vnw, PE_REAL, PC_NM1, PL_SOA, true),
    BIOIM_PLANE(rkev, PE_U64, PC_ONE, PL_SOA, false),     /* its share of bioim_eval_count / bioim_finished_count */
    BIOIM_PLANE(cache, PE_REAL, PC_CACHE, PL_ROWS, true),
    BIOIM_PLANE(cache_ok, PE_I32, PC_ONE, PL_SOA, true),
};
#undef BIOIM_PLANE
constexpr int BIOIM_NPLANES = (int)(sizeof(g_state_planes) / sizeof(g_state_planes[0]));
constexpr bool planes_cover_dstate() {   /* every pointer of DState is listed exactly once */
    for (size_t k = 0; k < (size_t)BIOIM_NPLANES; ++k) {
        int hits = 0;
        for (const StatePlane &p : g_state_planes) hits += p.member == k * sizeof(void *) ? 1 : 0;
        if (hits != 1) return false;
    }
    return true;
}
static_assert(sizeof(DState<double>) == BIOIM_NPLANES * sizeof(void *) && sizeof(DState<float>) == sizeof(DState<double>) &&
                  planes_cover_dstate(),
              "g_state_planes must list every plane of DState");

static const StatePlane *find_plane(const char *name) {
    for (const StatePlane &p : g_state_planes)
        if (strcmp(p.name, name) == 0) return &p;
    return nullptr;
}
static size_t plane_count(const bioim_handle_t *h, PlaneCount c) {
    switch (c) {
    case PC_NDOF: return (size_t)h->ndof;
    case PC_NM1: return h->nmuscle ? (size_t)h->nmuscle : 1;
    case PC_HIST: return (size_t)BIOIM_MAX_HORIZON * h->nact;
    case PC_NACT: return (size_t)h->nact;
    case PC_NA1: return h->nact ? (size_t)h->nact : 1;
    case PC_CACHE: return (size_t)cache_dim(h);
    default: return 1;
    }
}
static size_t plane_elem_bytes(const bioim_handle_t *h, PlaneElem e) {
    return e == PE_I32 ? 4 : e == PE_REAL ? (h->precision == 64 ? 8 : 4) : 8;
}
static size_t plane_bytes(const bioim_handle_t *h, const StatePlane &p) {
    return plane_elem_bytes(h, p.elem) * plane_count(h, p.count) * (size_t)h->n;
}
static char *&plane_base(const bioim_handle_t *h, const StatePlane &p) {
    return *reinterpret_cast<char **>(reinterpret_cast<char *>(h->dstate) + p.member);
}

/* one allocation for the whole record: the planes in table order, each
 * rounded up to 256 bytes, zeroed; then the device model images */
template <typename Real> static int alloc_state(bioim_handle_t *h) {
    auto span = [h](const StatePlane &p) { return (plane_bytes(h, p) + 255) & ~(size_t)255; };
    for (const StatePlane &p : g_state_planes) h->state_bytes += span(p);
    HIPCHK(hipMalloc(&h->state_buf, h->state_bytes));
    HIPCHK(hipMemsetAsync(h->state_buf, 0, h->state_bytes, h->stream));
    h->dstate = new DState<Real>();
    char *at = (char *)h->state_buf;
    for (const StatePlane &p : g_state_planes) {
        plane_base(h, p) = at;
        at += span(p);
    }
    DModel<Real> *hm = new DModel<Real>();
    convert_model<Real>(h->pack, *hm);
    HIPCHK(hipMalloc(&h->model, sizeof(DModel<Real>)));
    HIPCHK(hipMemcpyAsync(h->model, hm, sizeof(DModel<Real>), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    delete hm;
    return h->ops.upload(h);
}

/* The flat state row (bioim_get_state's layout, documented in include/bioim.h
 * at bioim_state_dim): the fields in order, each the first `count` rows of
 * its plane.  This table is the only place the order is written: the row's
 * length, row_offset and the gather / load kernel all walk it. */
enum RowCount { RC_ONE, RC_NDOF, RC_NM, RC_HIST, RC_NACT };   /* values per env; RC_NM: nmuscle, not its plane's padded count */
struct RowField {
    const char *plane;
    RowCount count;
};
static const RowField g_state_row[] = {
    {"t", RC_ONE},   {"istep", RC_ONE}, {"has_last", RC_ONE}, {"old_px", RC_ONE}, {"done", RC_ONE},
    {"q", RC_NDOF},  {"u", RC_NDOF},    {"act", RC_NM},       {"lce", RC_NM},
    {"hist", RC_HIST},   /* [horizon][nact] = hh * nact + a, of the plane's BIOIM_MAX_HORIZON * nact rows */
    {"last", RC_NACT},   {"hrk", RC_ONE},   {"ctl", RC_NACT},
};
constexpr int BIOIM_NROWFIELDS = (int)(sizeof(g_state_row) / sizeof(g_state_row[0]));

static int row_count(const bioim_handle_t *h, RowCount c) {
    switch (c) {
    case RC_NDOF: return h->ndof;
    case RC_NM: return h->nmuscle;
    case RC_HIST: return h->horizon * h->nact;
    case RC_NACT: return h->nact;
    default: return 1;
    }
}
/* where `field` starts in the row; null: past the last field, the row's length */
static int row_offset(const bioim_handle_t *h, const char *field) {
    int k = 0;
    for (const RowField &f : g_state_row) {
        if (field && strcmp(f.plane, field) == 0) break;
        k += row_count(h, f.count);
    }
    return k;
}

/* the row table as the kernel takes it, by value */
struct RowTable {
    void *base[BIOIM_NROWFIELDS];
    int32_t end[BIOIM_NROWFIELDS];    /* running sum of the counts: field f holds the row's values [end[f - 1], end[f]) */
    int32_t elem[BIOIM_NROWFIELDS];   /* PlaneElem */
    int32_t *pend, *cache_ok;         /* what a load clears */
};
static RowTable row_table(const bioim_handle_t *h) {
    RowTable tb{};
    int k = 0;
    for (int f = 0; f < BIOIM_NROWFIELDS; ++f) {
        const StatePlane &p = *find_plane(g_state_row[f].plane);
        tb.base[f] = plane_base(h, p);
        tb.end[f] = k += row_count(h, g_state_row[f].count);
        tb.elem[f] = p.elem;
    }
    tb.pend = reinterpret_cast<int32_t *>(plane_base(h, *find_plane("pend")));
    tb.cache_ok = reinterpret_cast<int32_t *>(plane_base(h, *find_plane("cache_ok")));
    return tb;
}

/* one whole plane of the record, by name, copied to the host or from it;
 * synchronizes both of the handle's streams.  `bytes` must be the plane's
 * size; every argument check comes before the first device call. */
static int plane_io(bioim_handle_t *h, const char *who, const char *name, void *host, size_t bytes, bool write) {
    const StatePlane *pl = find_plane(name);
    if (!pl) return fail(BIOIM_E_ARG, std::string(who) + ": no plane named '" + name + "'");
    const size_t want = plane_bytes(h, *pl);
    if (bytes != want)
        return fail(BIOIM_E_ARG, std::string(who) + ": plane " + name + " holds " + std::to_string(want) +
                                     " bytes, the buffer " + std::to_string(bytes));
    if (want == 0) return 0;   /* the cache plane of a topology without a realize cache */
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));   /* a group step may have run this handle on its side stream */
    if (write) {
        HIPCHK(hipMemcpy(plane_base(h, *pl), host, want, hipMemcpyHostToDevice));
        /* flags set from outside count as live: the next push, RK or
         * OsimModel launch clears them like a default launch's (launch_impl) */
        if (strcmp(name, "cache_ok") == 0) h->cache_live = 1;
    } else {
        HIPCHK(hipMemcpy(host, plane_base(h, *pl), want, hipMemcpyDeviceToHost));
    }
    return 0;
}
/* a plane of one value per env (V its element type) */
template <typename V> static int read_plane(bioim_handle_t *h, const char *who, const char *name, std::vector<V> &out) {
    out.resize((size_t)h->n);
    return plane_io(h, who, name, out.data(), sizeof(V) * out.size(), false);
}

/* ================================================================ C-ABI */
extern "C" {

const char *bioim_last_error(void) { return g_err.c_str(); }
#ifndef BIOIM_BUILD_ID
#define BIOIM_BUILD_ID "unstamped"
#endif
/* sha256 of the kernel sources + hipcc flags (bioimitation/_buildinfo.py) */
const char *bioim_build_id(void) { return BIOIM_BUILD_ID; }
uint64_t bioim_modelpack_size(void) { return sizeof(bioim_modelpack_t); }

int bioim_create(const bioim_modelpack_t *pack, int n_envs, int device, int precision, uint64_t seed,
                 bioim_handle_t **out) {
    if (!pack || !out || n_envs <= 0) return fail(BIOIM_E_ARG, "bioim_create: bad arguments");
    if (precision != 32 && precision != 64) return fail(BIOIM_E_ARG, "bioim_create: precision must be 32 or 64");
    if (pack->magic != BIOIM_PACK_MAGIC || pack->version != BIOIM_PACK_VERSION)
        return fail(BIOIM_E_PACK, "bioim_create: bad ModelPack magic/version");
    if (pack->horizon < 1 || pack->horizon > BIOIM_MAX_HORIZON || pack->nsub < 1 || pack->obs_dim > BIOIM_OBS_MAX ||
        pack->nrows < 2)
        return fail(BIOIM_E_PACK, "bioim_create: ModelPack env fields out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(BIOIM_E_DEVICE, "bioim_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(BIOIM_E_DEVICE, "bioim_create: bad device index");
    HIPCHK(hipSetDevice(device));
    Ops ops{};
    bool found = false;
#define BIOIM_TRY(S, NAME) \
    if (!found) found = bioim_pick_##S(*pack, precision, ops);
    BIOIM_FOR_EACH_TOPOLOGY(BIOIM_TRY)
#undef BIOIM_TRY
    if (!found) return fail(BIOIM_E_NOKERNEL, std::string("bioim_create: no compiled kernel for the topology of ") + pack->env_id);
    bioim_handle_t *h = new bioim_handle();
    h->n = n_envs; h->device = device; h->precision = precision; h->seed = seed;
    h->ndof = pack->ndof; h->nmuscle = pack->nmuscle; h->nact = pack->nact; h->horizon = pack->horizon;
    h->obs_dim = pack->obs_dim; h->info_dim = pack->info_dim; h->nsub = pack->nsub; h->auto_reset = 0;
    h->env_offset = 0;
    h->pert_n = 0; h->pert_ob = -1;
    h->ext_wrench = nullptr; h->ext_k = 0; h->ext_ground = 0; h->ext_body = 0;
    h->reset_tab = nullptr; h->reset_tab_on = 1; h->cache_live = 0;
    h->jr_model = nullptr; h->jr_smodel = nullptr; h->rk_budgeted = 0;
    h->rollout_live = nullptr; h->last_rollout_fused = 0; h->last_rollout_group_fused = 0;
    h->planar = pack_is_planar(*pack) ? 1 : 0;
    h->act_stride = pack->nact; h->obs_stride = pack->obs_dim; h->info_stride = pack->info_dim;
    h->ops = ops;
    memcpy(&h->pack, pack, sizeof(bioim_modelpack_t));
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(BIOIM_E_DEVICE, "bioim_create: stream creation failed");
    }
    h->own_stream = true;
    if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
        bioim_destroy(h);
        return fail(BIOIM_E_DEVICE, "bioim_create: stream/event creation failed");
    }
    int rc = precision == 64 ? alloc_state<double>(h) : alloc_state<float>(h);
    if (rc) { bioim_destroy(h); return rc; }
    *out = h;
    return 0;
}

int bioim_destroy(bioim_handle_t *h) {
    if (!h) return 0;
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->state_buf) hipFree(h->state_buf);
    if (h->model) hipFree(h->model);
    if (h->smodel) hipFree(h->smodel);
    if (h->jr_model) hipFree(h->jr_model);
    if (h->jr_smodel) hipFree(h->jr_smodel);
    if (h->pert_x) hipFree(h->pert_x);
    if (h->pert_y) hipFree(h->pert_y);
    if (h->reset_tab) hipFree(h->reset_tab);
    if (h->rollout_live) hipFree(h->rollout_live);
    if (h->dstate) {
        if (h->precision == 64) delete reinterpret_cast<DState<double> *>(h->dstate);
        else delete reinterpret_cast<DState<float> *>(h->dstate);
    }
    if (h->side) { hipStreamSynchronize(h->side); hipStreamDestroy(h->side); }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int bioim_reset(bioim_handle_t *h, const int32_t *env_ids, const int32_t *ref_index, int n, void *obs) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_reset: null handle");
    int count = env_ids ? n : h->n;
    if (count <= 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    h->ops.launch(h, 1, nullptr, obs, nullptr, nullptr, nullptr, env_ids, ref_index, count, nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

/* The reset table of a handle (LaunchArgs::reset_tab), built once, on the
 * first step that can use it: a scratch handle of the same pack and precision
 * with one env per reference row is reset to row r (mode 1 — the very reset
 * realize, with fiber equilibrium, an auto-reset runs) and its observations
 * are kept.  Muscle models: with the equilibrium fiber lengths; the reset
 * realize depends on the row alone (the held excitations enter only the
 * activation rate, which the observation does not hold; the fiber-velocity
 * root differs from a warm-started one at the rounding level: its start is
 * cold).  Torque models: the held torques enter the observation's q'' only,
 * linearly (q'' = M^-1 (f + tau)), so the row keeps q'' at zero torque (the
 * scratch handle's held controls are 0) and M^-1 at the row's coordinates. */
static int build_reset_table(bioim_handle_t *h) {
    const int nr = h->pack.nrows, nm = h->nmuscle, od = h->obs_dim, nd = h->ndof;
    const size_t R = h->precision == 64 ? 8 : 4, head = nm > 0 ? (size_t)nm : (size_t)nd * nd;
    const int cdim = cache_dim(h);
    const size_t dim = head + od + cdim;   /* = reset_table_dim(h) */
    bioim_handle_t *tmp = nullptr;
    int rc = bioim_create(&h->pack, nr, h->device, h->precision, h->seed, &tmp);
    if (rc) return rc;
    int32_t *d_idx = nullptr;
    void *d_obs = nullptr, *d_tab = nullptr, *d_q = nullptr, *d_v = nullptr, *d_out = nullptr;
    std::vector<int32_t> idx(nr);
    for (int r = 0; r < nr; ++r) idx[r] = r;
    const int sdim = bioim_state_dim(tmp);
    std::vector<double> st((size_t)nr * sdim);
    std::vector<unsigned char> obs((size_t)nr * od * R), tab((size_t)nr * dim * R);
    auto put = [&](unsigned char *dst, double x) {
        if (R == 8) memcpy(dst, &x, 8);
        else { const float f = (float)x; memcpy(dst, &f, 4); }
    };
    auto done = [&](int code) {
        for (void *p : {(void *)d_idx, d_obs, d_q, d_v, d_out})
            if (p) hipFree(p);
        if (code && d_tab) hipFree(d_tab);
        bioim_destroy(tmp);
        return code;
    };
    if (hipMalloc(&d_idx, sizeof(int32_t) * nr) != hipSuccess || hipMalloc(&d_obs, (size_t)nr * od * R) != hipSuccess ||
        hipMalloc(&d_tab, (size_t)nr * dim * R) != hipSuccess ||
        hipMemcpy(d_idx, idx.data(), sizeof(int32_t) * nr, hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(BIOIM_E_DEVICE, "build_reset_table: allocation failed"));
    if ((rc = bioim_reset(tmp, nullptr, d_idx, nr, d_obs)) != 0) return done(rc);
    if (hipStreamSynchronize(tmp->stream) != hipSuccess ||
        hipMemcpy(obs.data(), d_obs, obs.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(BIOIM_E_DEVICE, "build_reset_table: reset realize failed"));
    if ((rc = bioim_get_state(tmp, st.data())) != 0) return done(rc);
    if (nm > 0) {
        const int lce = row_offset(tmp, "lce");
        for (int r = 0; r < nr; ++r)
            for (int m = 0; m < nm; ++m)   /* fiber_length[m] */
                put(tab.data() + ((size_t)r * dim + m) * R, st[(size_t)r * sdim + lce + m]);
    } else {
        /* torque models: M^-1 at each row's coordinates, column k = M^-1 e_k
         * (the inverse-dynamics kernel, BIOIM_ID_MULT_MINV: the realize's
         * mass matrix — at h = 0 no implicit contact or limit terms) */
        const size_t n = (size_t)nr * nd;
        const int q0 = row_offset(tmp, "q");
        std::vector<unsigned char> q(n * nd * R), v(n * nd * R, 0), out(n * nd * R);
        for (int r = 0; r < nr; ++r)
            for (int k = 0; k < nd; ++k) {
                const size_t s_ = (size_t)r * nd + k;   /* state: row r, unit vector e_k */
                for (int d = 0; d < nd; ++d) put(q.data() + (s_ * nd + d) * R, st[(size_t)r * sdim + q0 + d]);
                put(v.data() + (s_ * nd + k) * R, 1.0);
            }
        if (hipMalloc(&d_q, q.size()) != hipSuccess || hipMalloc(&d_v, v.size()) != hipSuccess ||
            hipMalloc(&d_out, out.size()) != hipSuccess ||
            hipMemcpy(d_q, q.data(), q.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_v, v.data(), v.size(), hipMemcpyHostToDevice) != hipSuccess)
            return done(fail(BIOIM_E_DEVICE, "build_reset_table: allocation failed"));
        if ((rc = bioim_id_eval(tmp, BIOIM_ID_MULT_MINV, (int)n, d_q, d_q, d_v, d_out)) != 0) return done(rc);
        if (hipStreamSynchronize(tmp->stream) != hipSuccess ||
            hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return done(fail(BIOIM_E_DEVICE, "build_reset_table: M^-1 columns failed"));
        for (int r = 0; r < nr; ++r)
            for (int k = 0; k < nd; ++k)
                for (int d = 0; d < nd; ++d)   /* M^-1[d][k] = (M^-1 e_k)_d, row-major */
                    memcpy(tab.data() + ((size_t)r * dim + (size_t)d * nd + k) * R,
                           out.data() + (((size_t)r * nd + k) * nd + d) * R, R);
    }
    for (int r = 0; r < nr; ++r)
        memcpy(tab.data() + ((size_t)r * dim + head) * R, obs.data() + (size_t)r * od * R, (size_t)od * R);
    if (cdim > 0) {   /* the reset realize's cache rows (DState::cache, [nr][cdim]) */
        std::vector<unsigned char> crow((size_t)nr * cdim * R);
        if ((rc = plane_io(tmp, "build_reset_table", "cache", crow.data(), crow.size(), false)) != 0) return done(rc);
        for (int r = 0; r < nr; ++r)
            memcpy(tab.data() + ((size_t)r * dim + head + od) * R, crow.data() + (size_t)r * cdim * R, (size_t)cdim * R);
    }
    if (hipMemcpy(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(BIOIM_E_DEVICE, "build_reset_table: upload failed"));
    h->reset_tab = d_tab;
    return done(0);
}
static int ensure_reset_table(bioim_handle_t *h) {
    if (h->reset_tab || !reset_table_wanted(h)) return 0;
    return build_reset_table(h);
}

int bioim_set_reset_table(bioim_handle_t *h, int on) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_set_reset_table: null handle");
    h->reset_tab_on = on ? 1 : 0;
    return 0;
}

int bioim_reset_table_rows(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_reset_table_rows: null handle");
    return h->reset_tab ? h->pack.nrows : 0;
}

int bioim_step(bioim_handle_t *h, const void *actions, void *obs, void *reward, uint8_t *done, void *info) {
    if (!h || !actions || !done) return fail(BIOIM_E_ARG, "bioim_step: null handle/actions/done");
    HIPCHK(hipSetDevice(h->device));
    if (const int rc = ensure_reset_table(h)) return rc;
    h->ops.launch(h, 0, actions, obs, reward, done, info, nullptr, nullptr, 0, nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_set_auto_reset(bioim_handle_t *h, int on) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    h->auto_reset = on ? 1 : 0;
    return 0;
}

int bioim_set_integrator(bioim_handle_t *h, int kind, double accuracy) {
    if (!h || kind < 0 || kind > 1 || (kind == 1 && !(accuracy > 0)))
        return fail(BIOIM_E_ARG, "bioim_set_integrator: kind 0 (semi-implicit) or 1 (RK-Merson, accuracy > 0)");
    if (kind == 1 && h->ext_k > 0)
        return fail(BIOIM_E_ARG, "bioim_set_integrator: external forces are set (bioim_set_external_forces): semi-implicit only");
    if (kind != h->rk) {
        const int np = bioim_pending_count(h);
        if (np < 0) return np;
        if (np > 0) return fail(BIOIM_E_ARG, "bioim_set_integrator: envs are suspended mid-step (bioim_set_rk_budget)");
    }
    h->rk = kind;
    h->rk_acc = kind == 1 ? accuracy : 0.0;
    return 0;
}

int bioim_set_rk_budget(bioim_handle_t *h, int attempts, uint8_t *ready_out) {
    if (!h || attempts < 0) return fail(BIOIM_E_ARG, "bioim_set_rk_budget: null handle or negative budget");
    if (attempts > 0 && h->ext_k > 0)
        return fail(BIOIM_E_ARG, "bioim_set_rk_budget: external forces are set (bioim_set_external_forces): semi-implicit only");
    h->rk_budget = attempts;
    if (attempts > 0) h->rk_budgeted = 1;
    h->ready_out = ready_out;
    return 0;
}

int bioim_set_active_mask(bioim_handle_t *h, const uint8_t *active) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    if (active) {
        /* the step kernel reads active[env] for every env: refuse host memory
         * and memory of another device (a GPU fault otherwise); the length
         * (n bytes) is the caller's contract, checked by VectorEnv */
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, active) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BIOIM_E_ARG, "bioim_set_active_mask: not a device pointer");
        }
        if (at.type != hipMemoryTypeDevice || at.device != h->device)
            return fail(BIOIM_E_ARG, "bioim_set_active_mask: mask must be device memory on the handle's device");
    }
    h->active = active;
    return 0;
}

int bioim_pending_count(bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    std::vector<int32_t> p;
    if (const int rc = read_plane(h, "bioim_pending_count", "pend", p)) return rc;
    int c = 0;
    for (int32_t v : p) c += v != 0;
    return c;
}

int bioim_force_report_dim(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    return h->nact + 6 * h->pack.ncforce + h->pack.nlimit + 6 * h->pack.nsphere;
}

int bioim_set_state_storage(bioim_handle_t *h, void *rows, int capacity, int32_t *count) {
    if (!h || (rows && (capacity <= 0 || !count))) return fail(BIOIM_E_ARG, "bioim_set_state_storage: bad arguments");
    h->traj = rows;
    h->traj_n = rows ? count : nullptr;
    h->traj_cap = rows ? capacity : 0;
    return 0;
}

int bioim_set_force_report(bioim_handle_t *h, void *force_out) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    h->force_out = force_out;
    return 0;
}

int bioim_set_final_obs(bioim_handle_t *h, void *final_obs) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    h->final_obs = final_obs;
    return 0;
}

int bioim_set_io_strides(bioim_handle_t *h, int act_stride, int obs_stride, int info_stride) {
    if (!h || act_stride < h->nact || obs_stride < h->obs_dim || info_stride < h->info_dim)
        return fail(BIOIM_E_ARG, "bioim_set_io_strides: a stride is smaller than the row it holds");
    h->act_stride = act_stride; h->obs_stride = obs_stride; h->info_stride = info_stride;
    return 0;
}

static int g_group_fusion = 1;

int bioim_set_group_fusion(int on) {
    g_group_fusion = on ? 1 : 0;
    return 0;
}

int bioim_group_fused(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_group_fused: null handle");
    return h->last_group_fused ? 1 : 0;
}

/* one step of a group, enqueued (bioim_step_group after its checks; each step
 * of bioim_rollout_group's host loop): the fused two-topology launch where
 * eligible (*fused = 1), else one launch per segment, forked and joined */
static int group_step_enqueue(bioim_handle_t **hs, int nh, const void *actions, void *obs, void *reward, uint8_t *done,
                              void *info, int *fused) {
    const size_t R = hs[0]->precision == 64 ? 8 : 4;
    hipStream_t stream = hs[0]->stream;
    /* two segments whose topology pair has a fused kernel (BIOIM_FUSED_PAIRS)
     * and that run the default step kernels (no push table, semi-implicit):
     * one launch, workgroups [0, B0) segment 0, the rest segment 1 */
    *fused = 0;
    if (nh == 2 && g_group_fusion && hs[0]->pert_n == 0 && hs[1]->pert_n == 0 && !hs[0]->rk && !hs[1]->rk &&
        hs[0]->ext_k == 0 && hs[1]->ext_k == 0) {
        const int rc = bioim_fused_launch(hs[0], hs[1], actions, obs, reward, done, info);
        if (rc < 0) return rc;
        if (rc == 1) {
            HIPCHK(hipGetLastError());
            *fused = 1;
            return 0;
        }
    }
    /* Otherwise one launch per segment, concurrently: segment 0 on the
     * caller's stream (hs[0]), segment i > 0 on handle i's private stream,
     * forked from and joined back into the caller's stream with events.  At
     * 4096 envs per GPU a mixed 50/50 batch gives each segment half the CUs
     * (one 16-env workgroup per CU); in order on one stream the halves would
     * run one after the other. */
    size_t off = 0;
    if (nh > 1) HIPCHK(hipEventRecord(hs[0]->ev_fork, stream));
    for (int i = 0; i < nh; ++i) {
        bioim_handle_t *h = hs[i];
        hipStream_t own = h->stream;
        h->stream = i == 0 ? stream : h->side;
        if (i > 0) HIPCHK(hipStreamWaitEvent(h->side, hs[0]->ev_fork, 0));
        h->ops.launch(h, 0, (const char *)actions + off * h->act_stride * R,
                      obs ? (char *)obs + off * h->obs_stride * R : nullptr,
                      reward ? (char *)reward + off * R : nullptr, done + off,
                      info ? (char *)info + off * h->info_stride * R : nullptr, nullptr, nullptr, 0, nullptr);
        h->stream = own;
        if (i > 0) {
            HIPCHK(hipEventRecord(h->ev_join, h->side));
            HIPCHK(hipStreamWaitEvent(stream, h->ev_join, 0));
        }
        off += (size_t)h->n;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_step_group(bioim_handle_t **hs, int nh, const void *actions, void *obs, void *reward, uint8_t *done,
                     void *info) {
    if (!hs || nh <= 0 || !actions || !done) return fail(BIOIM_E_ARG, "bioim_step_group: bad arguments");
    for (int i = 0; i < nh; ++i) {
        if (!hs[i]) return fail(BIOIM_E_ARG, "bioim_step_group: null handle");
        if (hs[i]->device != hs[0]->device || hs[i]->precision != hs[0]->precision ||
            hs[i]->act_stride != hs[0]->act_stride || hs[i]->obs_stride != hs[0]->obs_stride ||
            hs[i]->info_stride != hs[0]->info_stride)
            return fail(BIOIM_E_ARG, "bioim_step_group: handles differ in device, precision or I/O strides");
    }
    HIPCHK(hipSetDevice(hs[0]->device));
    for (int i = 0; i < nh; ++i)
        if (const int rc = ensure_reset_table(hs[i])) return rc;
    int fused = 0;
    const int rc = group_step_enqueue(hs, nh, actions, obs, reward, done, info, &fused);
    hs[0]->last_group_fused = fused;
    return rc;
}

int bioim_set_perturbation(bioim_handle_t *h, int os_body, int npts, const double *x, const double *y) {
    if (!h || npts < 0 || (npts > 0 && (!x || !y || os_body < 0 || os_body >= h->pack.nosbody)))
        return fail(BIOIM_E_ARG, "bioim_set_perturbation: bad arguments");
    if (npts > 0 && h->ext_k > 0)
        return fail(BIOIM_E_ARG, "bioim_set_perturbation: external forces are set (bioim_set_external_forces); "
                                 "a push is one force slot there");
    for (int k = 0; k + 1 < npts; ++k)
        if (!(x[k] < x[k + 1])) return fail(BIOIM_E_ARG, "bioim_set_perturbation: breakpoints must increase");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    if (h->pert_x) { HIPCHK(hipFree(h->pert_x)); h->pert_x = nullptr; }
    if (h->pert_y) { HIPCHK(hipFree(h->pert_y)); h->pert_y = nullptr; }
    h->pert_n = 0;
    h->pert_ob = -1;
    if (npts == 0) return 0;
    const size_t n = h->n, R = h->precision == 64 ? 8 : 4;
    std::vector<unsigned char> yt(R * n * npts);   /* [npts][n], env index fastest */
    for (size_t e = 0; e < n; ++e)
        for (int k = 0; k < npts; ++k) {
            const double v = y[e * npts + k];
            if (R == 8) reinterpret_cast<double *>(yt.data())[k * n + e] = v;
            else reinterpret_cast<float *>(yt.data())[k * n + e] = (float)v;
        }
    HIPCHK(hipMalloc(&h->pert_x, sizeof(double) * npts));
    HIPCHK(hipMalloc(&h->pert_y, yt.size()));
    HIPCHK(hipMemcpy(h->pert_x, x, sizeof(double) * npts, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->pert_y, yt.data(), yt.size(), hipMemcpyHostToDevice));
    h->pert_n = npts;
    h->pert_ob = os_body;
    return 0;
}

int bioim_set_external_forces(bioim_handle_t *h, int k, const int32_t *os_body, const int32_t *point_frame,
                              const void *wrench) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_set_external_forces: null handle");
    if (k < 0 || k > BIOIM_MAX_EXT) return fail(BIOIM_E_ARG, "bioim_set_external_forces: k must be in [0, BIOIM_MAX_EXT]");
    if (k > 0 && (!os_body || !point_frame || !wrench))
        return fail(BIOIM_E_ARG, "bioim_set_external_forces: null os_body, point_frame or wrench");
    for (int j = 0; j < k; ++j)
        if (os_body[j] < 0 || os_body[j] >= h->pack.nosbody)
            return fail(BIOIM_E_ARG, "bioim_set_external_forces: slot " + std::to_string(j) + ": no OpenSim body " +
                                         std::to_string(os_body[j]));
    for (int j = 0; j < k; ++j)
        if (point_frame[j] != BIOIM_EXT_POINT_BODY && point_frame[j] != BIOIM_EXT_POINT_GROUND)
            return fail(BIOIM_E_ARG, "bioim_set_external_forces: slot " + std::to_string(j) +
                                         ": point_frame must be BIOIM_EXT_POINT_BODY or BIOIM_EXT_POINT_GROUND");
    if (k > 0 && h->pert_n > 0)
        return fail(BIOIM_E_ARG, "bioim_set_external_forces: a perturbation table is set (bioim_set_perturbation); "
                                 "a push is one force slot here");
    if (k > 0 && (h->rk || h->rk_budget > 0))
        return fail(BIOIM_E_ARG, "bioim_set_external_forces: the semi-implicit integrator only (RK-Merson or an RK budget is set)");
    /* the default step kernels' realize cache holds systems formed without
     * these forces or, once they are gone, must not outlive them: the flags
     * are cleared on the handle's stream when the forces are removed (a
     * launch with forces set clears them itself, launch_impl) */
    if (k == 0 && h->ext_k > 0 && cache_dim(h) > 0) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemsetAsync(plane_base(h, *find_plane("cache_ok")), 0, sizeof(int32_t) * (size_t)h->n, h->stream));
        h->cache_live = 0;
    }
    uint64_t body = 0;
    uint32_t ground = 0;
    for (int j = 0; j < k; ++j) {
        body |= (uint64_t)(uint32_t)os_body[j] << (8 * j);
        if (point_frame[j] == BIOIM_EXT_POINT_GROUND) ground |= 1u << j;
    }
    h->ext_k = k; h->ext_body = body; h->ext_ground = ground;
    h->ext_wrench = k > 0 ? wrench : nullptr;
    return 0;
}

int bioim_id_eval(bioim_handle_t *h, int op, int n, const void *q, const void *u, const void *v, void *out) {
    if (!h || n < 0 || op < BIOIM_ID_GRAVITY || op > BIOIM_ID_TOTAL || (n > 0 && (!q || !out)))
        return fail(BIOIM_E_ARG, "bioim_id_eval: bad arguments");
    const bool use_u = op == BIOIM_ID_CORIOLIS || op == BIOIM_ID_RESIDUAL || op == BIOIM_ID_TOTAL;
    const bool use_v = op == BIOIM_ID_MULT_M || op == BIOIM_ID_MULT_MINV || op == BIOIM_ID_RESIDUAL;
    if (n > 0 && ((use_u && !u) || (use_v && !v))) return fail(BIOIM_E_ARG, "bioim_id_eval: missing u or v");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const IdFields<void> c{n, op, q, u, v, out};
    h->ops.id_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_muscle_eval(bioim_handle_t *h, int n, const void *q, const void *u, const void *act, const void *lce,
                      void *length, void *speed, void *dldq, void *fiber, void *tau) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_muscle_eval: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_muscle_eval: negative n");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_muscle_eval: null q");
    if (!length && !speed && !dldq && !fiber && !tau) return fail(BIOIM_E_ARG, "bioim_muscle_eval: no output requested");
    if ((fiber || tau) && !act) return fail(BIOIM_E_ARG, "bioim_muscle_eval: fiber and tau need act");
    if (h->nmuscle <= 0 || !h->ops.ma_launch) return fail(BIOIM_E_ARG, "bioim_muscle_eval: the model has no muscles");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const MaFields<void> c{n, q, u, act, lce, length, speed, dldq, fiber, tau};
    h->ops.ma_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_static_opt(bioim_handle_t *h, int n, const void *q, const void *u, const void *tau, const void *row_weight,
                     double lo, double hi, int passive, void *act, void *residual, void *tau_muscle, void *capacity,
                     int32_t *status) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_static_opt: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_static_opt: negative n");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_static_opt: null q");
    if (!tau) return fail(BIOIM_E_ARG, "bioim_static_opt: null tau");
    if (!act) return fail(BIOIM_E_ARG, "bioim_static_opt: null act");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
        return fail(BIOIM_E_ARG, "bioim_static_opt: the bounds must be finite with lo < hi");
    if (h->nmuscle <= 0) return fail(BIOIM_E_ARG, "bioim_static_opt: the model has no muscles");
    if (h->precision != 64 || !h->ops.so_launch) return fail(BIOIM_E_ARG, "bioim_static_opt: fp64 handles only");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const SoFields<void> c{n, passive, q, u, tau, row_weight, lo, hi, act, residual, tau_muscle, capacity, status};
    h->ops.so_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_cmc(bioim_handle_t *h, int n, const void *q, const void *u, const void *act, const void *lce, const void *q1,
              const void *tau, const void *row_weight, double T, int nsub, double emin, double emax, double ftol,
              int max_iter, void *excitation, void *force, void *force_range, void *predicted, void *state_end,
              void *tau_muscle, void *residual, int32_t *status, int32_t *root_status) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_cmc: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_cmc: negative n");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_cmc: null q");
    if (n > 0 && !u) return fail(BIOIM_E_ARG, "bioim_cmc: null u");
    if (n > 0 && !act) return fail(BIOIM_E_ARG, "bioim_cmc: null act");
    if (n > 0 && !lce) return fail(BIOIM_E_ARG, "bioim_cmc: null lce");
    if (n > 0 && !tau) return fail(BIOIM_E_ARG, "bioim_cmc: null tau");
    if (n > 0 && !excitation) return fail(BIOIM_E_ARG, "bioim_cmc: null excitation");
    if (!std::isfinite(T) || !std::isfinite(ftol) || !std::isfinite(emin) || !std::isfinite(emax) || !(T > 0) ||
        !(emin < emax))
        return fail(BIOIM_E_ARG, "bioim_cmc: T, ftol, emin and emax must be finite with T > 0 and emin < emax");
    if (nsub < 1 || max_iter < 1) return fail(BIOIM_E_ARG, "bioim_cmc: nsub and max_iter must be at least 1");
    if (h->nmuscle <= 0) return fail(BIOIM_E_ARG, "bioim_cmc: the model has no muscles");
    if (h->precision != 64 || !h->ops.cmc_launch) return fail(BIOIM_E_ARG, "bioim_cmc: fp64 handles only");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const CmcFields<void> c{n, nsub, max_iter, q, u, act, lce, q1, tau, row_weight, T, emin, emax, ftol,
                            excitation, force, force_range, predicted, state_end, tau_muscle, residual, status, root_status};
    h->ops.cmc_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_ik_solve(bioim_handle_t *h, int n, int nm, const int32_t *marker_body, const void *marker_loc,
                   const void *weight, const void *x_exp, const void *q0, const void *coord_weight,
                   const void *q_target, double tol, int max_iter, void *q, void *markers, void *err,
                   void *jacobian, int32_t *status) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_ik_solve: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_ik_solve: negative n");
    if (nm < 1 || nm > BIOIM_IK_MAX_MARKERS)
        return fail(BIOIM_E_ARG, "bioim_ik_solve: nm must be in [1, BIOIM_IK_MAX_MARKERS]");
    if (n > 0 && (!marker_body || !marker_loc || !weight)) return fail(BIOIM_E_ARG, "bioim_ik_solve: null marker table");
    if (n > 0 && !x_exp) return fail(BIOIM_E_ARG, "bioim_ik_solve: null x_exp");
    if (n > 0 && !q0) return fail(BIOIM_E_ARG, "bioim_ik_solve: null q0");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_ik_solve: null q");
    if ((coord_weight == nullptr) != (q_target == nullptr))
        return fail(BIOIM_E_ARG, "bioim_ik_solve: coord_weight and q_target go together");
    if (!std::isfinite(tol) || tol < 0) return fail(BIOIM_E_ARG, "bioim_ik_solve: tol must be finite and >= 0");
    if (max_iter < 0) return fail(BIOIM_E_ARG, "bioim_ik_solve: negative max_iter");
    if (h->precision != 64 || !h->ops.ik_launch) return fail(BIOIM_E_ARG, "bioim_ik_solve: fp64 handles only");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const IkFields<void> c{n, nm, max_iter, marker_body, marker_loc, weight, x_exp, q0, coord_weight, q_target, tol,
                           q, markers, err, jacobian, status};
    h->ops.ik_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_joint_reaction(bioim_handle_t *h, int n, const void *q, const void *u, const void *qdd, const void *ft,
                         const void *ext, int flags, int frame, void *reaction, void *point, void *tau_joint,
                         void *muscle_wrench) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_joint_reaction: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_joint_reaction: negative n");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_joint_reaction: null q");
    if (ft && h->nmuscle <= 0) return fail(BIOIM_E_ARG, "bioim_joint_reaction: ft on a model without muscles");
    if (flags & ~BIOIM_JR_CONTACT) return fail(BIOIM_E_ARG, "bioim_joint_reaction: unknown flag bits");
    if (frame < BIOIM_JR_GROUND || frame > BIOIM_JR_PARENT)
        return fail(BIOIM_E_ARG, "bioim_joint_reaction: frame must be BIOIM_JR_GROUND, _CHILD or _PARENT");
    if (!reaction && !point && !tau_joint && !muscle_wrench)
        return fail(BIOIM_E_ARG, "bioim_joint_reaction: no output requested");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const JrFields<void> c{n, flags, frame, q, u, qdd, ft, ext, reaction, point, tau_joint, muscle_wrench};
    if (const int rc = h->ops.jr_launch(h, c)) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_induced_accel(bioim_handle_t *h, int n, const void *q, const void *u, const void *ft, const void *tau_act,
                        const void *ext, int kind, const uint8_t *cactive, const void *cpoint, double force_threshold,
                        void *accel, void *com_accel, void *reaction, void *cpoint_out, uint8_t *cactive_out,
                        int32_t *status) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_induced_accel: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_induced_accel: negative n");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_induced_accel: null q");
    if (ft && h->nmuscle <= 0) return fail(BIOIM_E_ARG, "bioim_induced_accel: ft on a model without muscles");
    if (kind < BIOIM_IA_FORCE || kind > BIOIM_IA_POINT)
        return fail(BIOIM_E_ARG, "bioim_induced_accel: kind must be BIOIM_IA_FORCE or BIOIM_IA_POINT");
    if ((cactive == nullptr) != (cpoint == nullptr))
        return fail(BIOIM_E_ARG, "bioim_induced_accel: cactive and cpoint go together");
    if (!std::isfinite(force_threshold) || force_threshold < 0)
        return fail(BIOIM_E_ARG, "bioim_induced_accel: force_threshold must be finite and >= 0");
    if (!accel && !com_accel && !reaction && !cpoint_out && !cactive_out && !status)
        return fail(BIOIM_E_ARG, "bioim_induced_accel: no output requested");
    if (h->precision != 64 || !h->ops.ia_launch) return fail(BIOIM_E_ARG, "bioim_induced_accel: fp64 handles only");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const IaFields<void> c{n, kind, force_threshold, q, u, ft, tau_act, ext, cpoint, cactive,
                           accel, com_accel, reaction, cpoint_out, cactive_out, status};
    h->ops.ia_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_body_kin(bioim_handle_t *h, int n, const void *q, const void *u, const void *qdd, int npt,
                   const int32_t *pt_body, const void *pt_local, int flags, void *origin, void *com, void *orient,
                   void *rot, void *system, void *momentum, void *energy, void *point) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_body_kin: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_body_kin: negative n");
    if (npt < 0 || npt > BIOIM_BK_MAX_POINTS)
        return fail(BIOIM_E_ARG, "bioim_body_kin: npt must be in [0, BIOIM_BK_MAX_POINTS]");
    if (npt > 0 && (!pt_body || !pt_local)) return fail(BIOIM_E_ARG, "bioim_body_kin: null point table");
    for (int i = 0; i < npt; ++i)
        if (pt_body[i] < -1 || pt_body[i] >= h->pack.nosbody)
            return fail(BIOIM_E_ARG, "bioim_body_kin: a point's body index is outside [-1, nosbody)");
    if (flags & ~BIOIM_BK_LOCAL) return fail(BIOIM_E_ARG, "bioim_body_kin: unknown flag bits");
    if (n > 0 && !q) return fail(BIOIM_E_ARG, "bioim_body_kin: null q");
    if (!origin && !com && !orient && !rot && !system && !momentum && !energy && !point)
        return fail(BIOIM_E_ARG, "bioim_body_kin: no output requested");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    BkFields<void> c{};
    c.n = n; c.npt = npt; c.flags = flags;
    c.q = q; c.u = u; c.qdd = qdd;
    c.origin = origin; c.com = com; c.orient = orient; c.rot = rot;
    c.system = system; c.momentum = momentum; c.energy = energy; c.point = point;
    for (int b = 0; b < h->pack.nosbody; ++b)
        for (int i = 0; i < 3; ++i) c.os_com[b][i] = h->pack.osbody[b].com[i];
    for (int i = 0; i < npt; ++i) {
        c.pt_body[i] = (int8_t)pt_body[i];
        for (int k = 0; k < 3; ++k) c.pt_local[i][k] = static_cast<const double *>(pt_local)[3 * i + k];
    }
    h->ops.bk_launch(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_osim_report_dim(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    return osim_report_dim(h->pack);
}

int bioim_osim(bioim_handle_t *h, int op, const int32_t *env_ids, int n, const void *controls, void *obs, void *report) {
    if (!h || op < BIOIM_OSIM_REALIZE || op > BIOIM_OSIM_INTEGRATE || n < 0 || (n > 0 && !env_ids))
        return fail(BIOIM_E_ARG, "bioim_osim: bad arguments");
    if (n == 0) return 0;
    const int np = bioim_pending_count(h);
    if (np < 0) return np;
    if (np > 0) return fail(BIOIM_E_ARG, "bioim_osim: envs are suspended mid-step (bioim_set_rk_budget)");
    HIPCHK(hipSetDevice(h->device));
    const OsimCall oc{op, controls, report};
    h->ops.launch(h, 2, nullptr, obs, nullptr, nullptr, nullptr, env_ids, nullptr, n, &oc);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_realize_report(bioim_handle_t *h, const int32_t *env_ids, int n, void *report) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_realize_report: null handle");
    if (n < 0) return fail(BIOIM_E_ARG, "bioim_realize_report: negative n");
    if (n > 0 && !env_ids) return fail(BIOIM_E_ARG, "bioim_realize_report: null env_ids");
    if (!report) return fail(BIOIM_E_ARG, "bioim_realize_report: null report");
    if (h->rk_budgeted)
        return fail(BIOIM_E_ARG, "bioim_realize_report: the handle has had an RK budget (envs may be suspended): use bioim_osim");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    const OsimCall oc{BIOIM_OSIM_REALIZE, nullptr, report};
    h->ops.launch(h, 2, nullptr, nullptr, nullptr, nullptr, nullptr, env_ids, nullptr, n, &oc);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_set_env_offset(bioim_handle_t *h, int offset) {
    if (!h || offset < 0) return fail(BIOIM_E_ARG, "bioim_set_env_offset: bad arguments");
    h->env_offset = offset;
    return 0;
}

int bioim_state_dim(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    return row_offset(h, nullptr);
}

/* bioim_copy_state: the flat state rows (bioim_get_state's layout) gathered
 * on the device, one thread per value, on the handle's stream — no
 * synchronization, so a caller can fold them into the copy of a step's
 * outputs (the single-env recorder, envs.py).  bioim_copy_state_rows does
 * the same for a list of envs, bioim_load_state writes such rows back and
 * bioim_clone_envs copies whole envs.
 *
 * The kernels below (rows gather / load, env clone) take the
 * record as a table argument: no topology template, this unit alone holds
 * them.  Each reads its env ids from a device list and skips an id outside
 * [0, N) instead of using it.
 *
 * state_rows_kernel walks the row table (RowTable): row r of `rows` is the
 * flat state row of env ids[r] (ids null: env r), n rows.  Gather: values to
 * double.  LOAD: the inverse, values to the plane's element type (reals to
 * Real, istep / has_last / done through int32_t, t and hrk stay double); the
 * thread of a row's first value also marks the env as at a step boundary
 * (pend) and its realize-cache row as stale (cache_ok). */
extern "C++" {
template <typename V, bool LOAD> DEV void row_value(void *base, size_t j, size_t count, double &v) {
    V *p = reinterpret_cast<V *>(base);
    if constexpr (LOAD) GAT(p, j, count) = (V)v;
    else v = (double)GAT(p, j, count);
}

template <typename Real, bool LOAD>
__global__ void state_rows_kernel(RowTable tb, int n_envs, const int32_t *ids, int n, double *rows) {
    const int dim = tb.end[BIOIM_NROWFIELDS - 1];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)n * dim;
    if (i >= total) return;
    const int r = (int)(i / dim), k = (int)(i % dim);
    const int e = ids ? GAT(ids, r, n) : r;
    if (e < 0 || e >= n_envs) return;
    const size_t N = (size_t)n_envs;
    double v = LOAD ? GAT(rows, i, total) : 0;
    int first = 0;
#pragma unroll
    for (int f = 0; f < BIOIM_NROWFIELDS; ++f) {
        if (k >= first && k < tb.end[f]) {
            const size_t j = (size_t)(k - first) * N + e, count = (size_t)(tb.end[f] - first) * N;
            if (tb.elem[f] == PE_REAL) row_value<Real, LOAD>(tb.base[f], j, count, v);
            else if (tb.elem[f] == PE_I32) row_value<int32_t, LOAD>(tb.base[f], j, count, v);
            else row_value<double, LOAD>(tb.base[f], j, count, v);
        }
        first = tb.end[f];
    }
    if constexpr (LOAD) {
        if (k == 0) {
            GAT(tb.pend, e, N) = 0;       /* a state set from outside is at a step boundary */
            GAT(tb.cache_ok, e, N) = 0;   /* the realize cache belongs to the state it was formed at */
        }
    } else {
        GAT(rows, i, total) = v;
    }
}

/* clone_envs_kernel's view of the cloned planes.  SoA planes are copied as
 * 4- or 8-byte words (bit copies, whatever the element type); end[k] is the
 * running sum of their rows per env, so a thread's row index names its plane. */
struct ClonePlanes {
    void *base[BIOIM_NPLANES];
    int32_t end[BIOIM_NPLANES];
    int32_t wide[BIOIM_NPLANES];   /* 1: 8-byte elements */
    int32_t npl, rows;             /* SoA planes; their rows per env in all */
    void *cache;                   /* the one [N][cache_dim] plane */
    int32_t cache_dim, cache_wide;
};

template <typename W> DEV void clone_word(void *base, size_t to, size_t from, size_t count) {
    W *b = reinterpret_cast<W *>(base);
    GAT(b, to, count) = GAT(b, from, count);
}

/* Pair p copies env src[p]'s record to env dst[p].  The first n * rows
 * threads take the SoA planes with the pair index fastest (a sorted dst
 * writes coalesced), the others the cache rows with the element fastest. */
__global__ void clone_envs_kernel(ClonePlanes pl, int n_envs, const int32_t *src, const int32_t *dst, int n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N = (size_t)n_envs, nsoa = (size_t)n * pl.rows, total = nsoa + (size_t)n * pl.cache_dim;
    if (i >= total) return;
    const bool soa = i < nsoa;
    const size_t j = soa ? i : i - nsoa;
    const int p = soa ? (int)(j % n) : (int)(j / pl.cache_dim);
    const int s = GAT(src, p, n), d = GAT(dst, p, n);
    if (s < 0 || s >= n_envs || d < 0 || d >= n_envs) return;
    if (!soa) {
        const size_t c = j % pl.cache_dim, cd = (size_t)pl.cache_dim;
        if (pl.cache_wide) clone_word<uint64_t>(pl.cache, d * cd + c, s * cd + c, N * cd);
        else clone_word<uint32_t>(pl.cache, d * cd + c, s * cd + c, N * cd);
        return;
    }
    const int row = (int)(j / n);
    int first = 0;
#pragma unroll
    for (int k = 0; k < BIOIM_NPLANES; ++k) {
        if (k < pl.npl && row >= first && row < pl.end[k]) {
            const size_t r = (size_t)(row - first), count = (size_t)(pl.end[k] - first) * N;
            if (pl.wide[k]) clone_word<uint64_t>(pl.base[k], r * N + d, r * N + s, count);
            else clone_word<uint32_t>(pl.base[k], r * N + d, r * N + s, count);
        }
        first = pl.end[k];
    }
}
}  // extern "C++"

/* n flat rows between the device buffer `rows` and the envs env_ids (null:
 * envs 0 .. n - 1), on the handle's stream */
static int state_rows_launch(bioim_handle_t *h, const int32_t *env_ids, int n, double *rows, bool load) {
    HIPCHK(hipSetDevice(h->device));
    const size_t total = (size_t)n * bioim_state_dim(h);
    const int bs = 256;
    auto kernel = h->precision == 64 ? (load ? state_rows_kernel<double, true> : state_rows_kernel<double, false>)
                                     : (load ? state_rows_kernel<float, true> : state_rows_kernel<float, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, h->stream, row_table(h), h->n, env_ids,
                       n, rows);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_copy_state(bioim_handle_t *h, void *device_out) {
    if (!h || !device_out) return fail(BIOIM_E_ARG, "bioim_copy_state: bad arguments");
    return state_rows_launch(h, nullptr, h->n, reinterpret_cast<double *>(device_out), false);
}

int bioim_copy_state_rows(bioim_handle_t *h, const int32_t *env_ids, int n, void *device_out) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_copy_state_rows: null handle");
    if (!device_out) return fail(BIOIM_E_ARG, "bioim_copy_state_rows: null output buffer");
    if (env_ids && (n <= 0 || n > h->n))
        return fail(BIOIM_E_ARG, "bioim_copy_state_rows: n must lie in [1, n_envs] with an id list");
    return state_rows_launch(h, env_ids, env_ids ? n : h->n, reinterpret_cast<double *>(device_out), false);
}

int bioim_load_state(bioim_handle_t *h, const int32_t *env_ids, int n, const void *device_rows) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_load_state: null handle");
    if (!device_rows) return fail(BIOIM_E_ARG, "bioim_load_state: null rows buffer");
    if (env_ids && (n <= 0 || n > h->n))
        return fail(BIOIM_E_ARG, "bioim_load_state: n must lie in [1, n_envs] with an id list");
    return state_rows_launch(h, env_ids, env_ids ? n : h->n, (double *)device_rows, true);   /* a load only reads them */
}

/* bioim_get_state / bioim_set_state: every env's row between the host and
 * the record, through a temporary device buffer and the row kernel;
 * synchronous, on both of the handle's streams */
static int host_rows(bioim_handle_t *h, double *host, bool load) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->side));
    const size_t bytes = sizeof(double) * (size_t)h->n * bioim_state_dim(h);
    double *dev = nullptr;
    HIPCHK(hipMalloc(&dev, bytes));
    hipError_t e = load ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
    const int rc = e == hipSuccess ? state_rows_launch(h, nullptr, h->n, dev, load) : 0;
    if (e == hipSuccess && !rc && !load) e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    hipFree(dev);
    if (rc) return rc;
    HIPCHK(e);
    HIPCHK(es);
    return 0;
}

int bioim_get_state(bioim_handle_t *h, double *host_state) {
    if (!h || !host_state) return fail(BIOIM_E_ARG, "bioim_get_state: bad arguments");
    const int np = bioim_pending_count(h);
    if (np < 0) return np;
    if (np > 0)   /* mid-step: t is the step's end time but q/u/act/lce an accepted RK point */
        return fail(BIOIM_E_ARG, "bioim_get_state: envs are suspended mid-step by the RK budget "
                                 "(step until bioim_pending_count() is 0)");
    return host_rows(h, host_state, false);
}

int bioim_set_state(bioim_handle_t *h, const double *host_state) {
    if (!h || !host_state) return fail(BIOIM_E_ARG, "bioim_set_state: bad arguments");
    return host_rows(h, const_cast<double *>(host_state), true);
}

int bioim_clone_envs(bioim_handle_t *h, const int32_t *src_ids, const int32_t *dst_ids, int n) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_clone_envs: null handle");
    if (!src_ids || !dst_ids) return fail(BIOIM_E_ARG, "bioim_clone_envs: null src or dst id list");
    if (n <= 0 || n > h->n) return fail(BIOIM_E_ARG, "bioim_clone_envs: n must lie in [1, n_envs]");
    HIPCHK(hipSetDevice(h->device));
    ClonePlanes pl{};
    int rows = 0;
    for (const StatePlane &p : g_state_planes) {
        if (!p.cloned) continue;
        const bool wide = plane_elem_bytes(h, p.elem) == 8;
        if (p.layout == PL_ROWS) {
            pl.cache = plane_base(h, p);
            pl.cache_dim = (int32_t)plane_count(h, p.count);
            pl.cache_wide = wide;
            continue;
        }
        rows += (int)plane_count(h, p.count);
        pl.base[pl.npl] = plane_base(h, p);
        pl.end[pl.npl] = rows;
        pl.wide[pl.npl] = wide;
        ++pl.npl;
    }
    for (int k = pl.npl; k < BIOIM_NPLANES; ++k) pl.end[k] = rows;
    pl.rows = rows;
    const size_t total = (size_t)n * ((size_t)rows + pl.cache_dim);
    const int bs = 256;
    hipLaunchKernelGGL(clone_envs_kernel, dim3((unsigned)((total + bs - 1) / bs)), dim3(bs), 0, h->stream, pl, h->n,
                       src_ids, dst_ids, n);
    HIPCHK(hipGetLastError());
    return 0;
}

/* total resets (explicit + in-kernel auto-resets) over the handle's envs */
int bioim_reset_count(bioim_handle_t *h, uint64_t *total) {
    if (!h || !total) return fail(BIOIM_E_ARG, "bioim_reset_count: bad arguments");
    std::vector<int32_t> r;
    if (const int rc = read_plane(h, "bioim_reset_count", "resets", r)) return rc;
    uint64_t sum = 0;
    for (int e = 0; e < h->n; ++e) sum += (uint32_t)r[e];
    *total = sum;
    return 0;
}

/* one of the per-env RK counters of the state (DState::rkev) summed over the envs */
static int rk_counter(bioim_handle_t *h, uint64_t *total, bool fin, const char *who) {
    if (!h || !total) return fail(BIOIM_E_ARG, std::string(who) + ": bad arguments");
    std::vector<uint64_t> r;
    if (const int rc = read_plane(h, who, "rkev", r)) return rc;
    uint64_t sum = 0;
    for (int e = 0; e < h->n; ++e) sum += (uint32_t)(fin ? r[e] >> 32 : r[e]);
    *total = sum;
    return 0;
}

/* dynamics evaluations of the RK integrator so far, summed over the envs */
int bioim_eval_count(bioim_handle_t *h, uint64_t *total) { return rk_counter(h, total, false, "bioim_eval_count"); }

/* env steps the RK integrator finished so far (bioim_step launches whose
 * ready[env] was 1), summed over the envs */
int bioim_finished_count(bioim_handle_t *h, uint64_t *total) {
    return rk_counter(h, total, true, "bioim_finished_count");
}

int bioim_set_rk_counters(bioim_handle_t *h, uint32_t evals, uint32_t finished) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_set_rk_counters: null handle");
    std::vector<uint64_t> v((size_t)h->n, ((uint64_t)finished << 32) | evals);
    return plane_io(h, "bioim_set_rk_counters", "rkev", v.data(), sizeof(uint64_t) * v.size(), true);
}

/* debug / tests: one whole plane of the per-env record (g_state_planes, by
 * name) copied to the host, or from it (plane_io). */
int bioim_debug_plane(bioim_handle_t *h, const char *name, void *host, size_t bytes, int write) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_debug_plane: null handle");
    if (!name || !host) return fail(BIOIM_E_ARG, "bioim_debug_plane: null plane name or host buffer");
    return plane_io(h, "bioim_debug_plane", name, host, bytes, write != 0);
}

int bioim_query(const bioim_handle_t *h, int32_t *out) {
    if (!h || !out) return fail(BIOIM_E_ARG, "bioim_query: bad arguments");
    out[0] = h->n; out[1] = h->obs_dim; out[2] = h->nact; out[3] = h->info_dim;
    out[4] = h->precision; out[5] = h->ops.lanes; out[6] = h->nsub; out[7] = bioim_state_dim(h);
    return 0;
}

int bioim_query_launch(const bioim_handle_t *h, int32_t *out) {
    if (!h || !out) return fail(BIOIM_E_ARG, "bioim_query_launch: bad arguments");
    const int epb = BIOIM_EPB;
    out[0] = h->ops.lanes; out[1] = BIOIM_EPB * h->ops.lanes; out[2] = epb; out[3] = (int32_t)h->ops.lds_bytes;
    out[4] = (h->n + epb - 1) / epb;
    return 0;
}

void *bioim_stream(bioim_handle_t *h) { return h ? (void *)h->stream : nullptr; }

int bioim_set_stream(bioim_handle_t *h, void *s) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    if (h->own_stream && h->stream) {
        hipStreamSynchronize(h->stream);
        hipStreamDestroy(h->stream);
    }
    h->stream = (hipStream_t)s;
    h->own_stream = false;
    return 0;
}

#ifdef BIOIM_WAVETIME
int bioim_debug_wavetime(unsigned long long *out, int n) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavetime), sizeof(unsigned long long) * (n < BIOIM_WAVETIME_N ? n : BIOIM_WAVETIME_N)));
    return 0;
}
/* per thread: [0, n) Newton iterations, [n, 2n) most in one solve, [2n, 3n) bisections */
int bioim_debug_fviter(unsigned *out, int n) {
    HIPCHK(hipDeviceSynchronize());
    const int m = n < BIOIM_WAVETIME_N * 4 ? n : BIOIM_WAVETIME_N * 4;
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fvit), sizeof(unsigned) * m));
    HIPCHK(hipMemcpyFromSymbol(out + n, HIP_SYMBOL(g_fvmax), sizeof(unsigned) * m));
    HIPCHK(hipMemcpyFromSymbol(out + 2 * n, HIP_SYMBOL(g_fvbis), sizeof(unsigned) * m));
    return 0;
}
#endif
#ifdef BIOIM_STAMPS
int bioim_debug_stamps(unsigned long long *out, int reset) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 28));
    if (reset) {
        unsigned long long z[28] = {0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)));
    }
    return 0;
}
#endif

/* bioim_rollout's host-loop path (push table, RK-Merson, force report, state
 * storage, or no rollout kernel for the topology): the existing step kernels,
 * one launch per step.  The three small kernels below do between those
 * launches what rollout_kernel does in its loop; one thread per env (per
 * observation value for the copy), sizes as run-time arguments.
 * rollout_live_init: the stop_at_done mask starts as the caller's mask (or
 * ones).  rollout_freeze_kernel, after step k: a live env that returned done
 * leaves the mask; an env that left it earlier gets its frozen rows.
 * rollout_obs_last_kernel: the last rows of obs_seq also go to obs_last,
 * except for envs the caller masked out. */
extern "C++" {
__global__ void rollout_live_init(uint8_t *live, const uint8_t *active, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) live[e] = !active || active[e] != 0 ? 1 : 0;
}

template <typename Real>
__global__ void rollout_freeze_kernel(uint8_t *live, const uint8_t *active, int n, uint8_t *done, Real *reward, Real *info,
                                      int info_dim, int info_stride, Real *obs, const Real *obs_prev, int obs_dim,
                                      int obs_stride) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || (active && active[e] == 0)) return;
    if (live[e]) {
        if (done[e]) live[e] = 0;
        return;
    }
    if (reward) reward[e] = Real(0);
    done[e] = 1;
    if (info)
        for (int j = 0; j < info_dim; ++j) info[(size_t)e * info_stride + j] = Real(0);
    if (obs && obs_prev)
        for (int j = 0; j < obs_dim; ++j) obs[(size_t)e * obs_stride + j] = obs_prev[(size_t)e * obs_stride + j];
}

template <typename Real>
__global__ void rollout_obs_last_kernel(const uint8_t *active, int n, const Real *obs, Real *obs_last, int obs_dim,
                                        int obs_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * obs_dim) return;
    const size_t e = i / obs_dim, at = e * obs_stride + i % obs_dim;
    if (!active || active[e] != 0) obs_last[at] = obs[at];
}

template <typename Real> static void rollout_host_loop(bioim_handle_t *h, const RolloutCall &c) {
    const size_t n = (size_t)h->n;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const Real *actions = reinterpret_cast<const Real *>(c.actions);
    Real *obs_seq = reinterpret_cast<Real *>(c.obs_seq), *obs_last = reinterpret_cast<Real *>(c.obs_last);
    Real *reward_seq = reinterpret_cast<Real *>(c.reward_seq), *info_seq = reinterpret_cast<Real *>(c.info_seq);
    const uint8_t *const user_active = h->active;
    if (c.stop_at_done) {
        hipLaunchKernelGGL(rollout_live_init, dim3(blocks), dim3(256), 0, h->stream, h->rollout_live, user_active, (int)n);
        h->active = h->rollout_live;
    }
    for (int k = 0; k < c.steps; ++k) {
        Real *obs = obs_seq ? obs_seq + (size_t)k * n * h->obs_stride
                            : (k == c.steps - 1 || c.stop_at_done ? obs_last : nullptr);
        Real *reward = reward_seq ? reward_seq + (size_t)k * n : nullptr;
        uint8_t *done = c.done_seq + (size_t)k * n;
        Real *info = info_seq ? info_seq + (size_t)k * n * h->info_stride : nullptr;
        h->ops.launch(h, 0, actions + (size_t)k * (size_t)c.act_step, obs, reward, done, info, nullptr, nullptr, 0, nullptr);
        if (c.stop_at_done)
            hipLaunchKernelGGL((rollout_freeze_kernel<Real>), dim3(blocks), dim3(256), 0, h->stream, h->rollout_live,
                               user_active, (int)n, done, reward, info, h->info_dim, h->info_stride,
                               obs_seq ? obs : nullptr, obs_seq && k > 0 ? obs - n * h->obs_stride : nullptr, h->obs_dim,
                               h->obs_stride);
    }
    h->active = user_active;
    if (obs_seq && obs_last)
        hipLaunchKernelGGL((rollout_obs_last_kernel<Real>), dim3((unsigned)((n * h->obs_dim + 255) / 256)), dim3(256), 0,
                           h->stream, user_active, (int)n, obs_seq + (size_t)(c.steps - 1) * n * h->obs_stride, obs_last,
                           h->obs_dim, h->obs_stride);
}
}  // extern "C++"

/* the configurations rollout_kernel covers: the default step kernel's
 * (semi-implicit, no push table) without a force report or state storage */
static inline bool rollout_fusable(const bioim_handle_t *h) {
    return h->ops.rollout && !h->rk && h->pert_n == 0 && h->ext_k == 0 && !h->force_out && !h->traj;
}

int bioim_rollout(bioim_handle_t *h, const void *actions, int steps, int64_t action_step_stride, void *obs_seq,
                  void *obs_last, void *reward_seq, uint8_t *done_seq, void *info_seq, int stop_at_done) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_rollout: null handle");
    if (!actions || !done_seq) return fail(BIOIM_E_ARG, "bioim_rollout: null actions or done_seq");
    if (steps <= 0) return fail(BIOIM_E_ARG, "bioim_rollout: steps must be positive");
    if (action_step_stride < 0) return fail(BIOIM_E_ARG, "bioim_rollout: negative action_step_stride");
    if (h->rk && h->rk_budget > 0)
        return fail(BIOIM_E_ARG, "bioim_rollout: a budgeted RK handle suspends envs mid-step, a rollout has no rows for that "
                                 "(bioim_set_rk_budget(h, 0, NULL) first)");
    if (stop_at_done && h->auto_reset)
        return fail(BIOIM_E_ARG, "bioim_rollout: stop_at_done needs auto-reset off (a reset env goes on)");
    HIPCHK(hipSetDevice(h->device));
    if (h->rk) {   /* only an RK handle can hold suspended envs; the count waits for its stream */
        const int np = bioim_pending_count(h);
        if (np < 0) return np;
        if (np > 0) return fail(BIOIM_E_ARG, "bioim_rollout: envs are suspended mid-step (bioim_set_rk_budget)");
    }
    if (const int rc = ensure_reset_table(h)) return rc;
    if (stop_at_done && !h->rollout_live) HIPCHK(hipMalloc(reinterpret_cast<void **>(&h->rollout_live), (size_t)h->n));
    const RolloutCall c{actions, steps, action_step_stride, obs_seq, obs_last, reward_seq, done_seq, info_seq,
                        stop_at_done ? 1 : 0};
    h->last_rollout_fused = rollout_fusable(h) ? 1 : 0;
    if (h->last_rollout_fused) h->ops.rollout(h, c);
    else if (h->precision == 64) rollout_host_loop<double>(h, c);
    else rollout_host_loop<float>(h, c);
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_rollout_fused(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_rollout_fused: null handle");
    return h->last_rollout_fused ? 1 : 0;
}

/* bioim_rollout_group's host-loop path: per step what bioim_step_group
 * enqueues, then (stop_at_done) the freeze kernel per segment on hs[0]'s
 * stream, after the join, on that step's slices at the full-batch pitch */
extern "C++" {
template <typename Real> static int rollout_group_host_loop(bioim_handle_t **hs, int nh, const RolloutCall &c, size_t rows) {
    hipStream_t stream = hs[0]->stream;
    const size_t os = (size_t)hs[0]->obs_stride, is = (size_t)hs[0]->info_stride;
    const Real *actions = reinterpret_cast<const Real *>(c.actions);
    Real *obs_seq = reinterpret_cast<Real *>(c.obs_seq), *obs_last = reinterpret_cast<Real *>(c.obs_last);
    Real *reward_seq = reinterpret_cast<Real *>(c.reward_seq), *info_seq = reinterpret_cast<Real *>(c.info_seq);
    std::vector<const uint8_t *> user_active(nh);
    for (int i = 0; i < nh; ++i) user_active[i] = hs[i]->active;
    if (c.stop_at_done)
        for (int i = 0; i < nh; ++i) {
            bioim_handle_t *h = hs[i];
            if (h->n > 0)
                hipLaunchKernelGGL(rollout_live_init, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, stream,
                                   h->rollout_live, user_active[i], h->n);
            h->active = h->rollout_live;
        }
    int rc = 0;
    for (int k = 0; k < c.steps && !rc; ++k) {
        Real *obs = obs_seq ? obs_seq + (size_t)k * rows * os : (k == c.steps - 1 || c.stop_at_done ? obs_last : nullptr);
        Real *reward = reward_seq ? reward_seq + (size_t)k * rows : nullptr;
        uint8_t *done = c.done_seq + (size_t)k * rows;
        Real *info = info_seq ? info_seq + (size_t)k * rows * is : nullptr;
        int fused = 0;
        rc = group_step_enqueue(hs, nh, actions + (size_t)k * (size_t)c.act_step, obs, reward, done, info, &fused);
        if (rc || !c.stop_at_done) continue;
        size_t off = 0;
        for (int i = 0; i < nh; ++i) {
            bioim_handle_t *h = hs[i];
            Real *so = obs_seq ? obs + off * os : nullptr;
            if (h->n > 0)
                hipLaunchKernelGGL((rollout_freeze_kernel<Real>), dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, stream,
                                   h->rollout_live, user_active[i], h->n, done + off, reward ? reward + off : nullptr,
                                   info ? info + off * is : nullptr, h->info_dim, h->info_stride, so,
                                   so && k > 0 ? so - rows * os : nullptr, h->obs_dim, h->obs_stride);
            off += (size_t)h->n;
        }
    }
    for (int i = 0; i < nh; ++i) hs[i]->active = user_active[i];
    if (rc) return rc;
    if (obs_seq && obs_last) {
        size_t off = 0;
        for (int i = 0; i < nh; ++i) {
            bioim_handle_t *h = hs[i];
            const size_t cnt = (size_t)h->n * h->obs_dim;
            if (cnt > 0)
                hipLaunchKernelGGL((rollout_obs_last_kernel<Real>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream,
                                   user_active[i], h->n, obs_seq + ((size_t)(c.steps - 1) * rows + off) * os,
                                   obs_last + off * os, h->obs_dim, h->obs_stride);
            off += (size_t)h->n;
        }
    }
    return 0;
}
}  // extern "C++"

int bioim_rollout_group(bioim_handle_t **hs, int nh, const void *actions, int steps, int64_t action_step_stride,
                        void *obs_seq, void *obs_last, void *reward_seq, uint8_t *done_seq, void *info_seq,
                        int stop_at_done) {
    if (!hs || nh <= 0) return fail(BIOIM_E_ARG, "bioim_rollout_group: null handle list or nh <= 0");
    for (int i = 0; i < nh; ++i)
        if (!hs[i]) return fail(BIOIM_E_ARG, "bioim_rollout_group: null handle");
    if (!actions || !done_seq) return fail(BIOIM_E_ARG, "bioim_rollout_group: null actions or done_seq");
    if (steps <= 0) return fail(BIOIM_E_ARG, "bioim_rollout_group: steps must be positive");
    if (action_step_stride < 0) return fail(BIOIM_E_ARG, "bioim_rollout_group: negative action_step_stride");
    size_t rows = 0;
    for (int i = 0; i < nh; ++i) {
        const bioim_handle_t *h = hs[i];
        if (h->device != hs[0]->device || h->precision != hs[0]->precision || h->act_stride != hs[0]->act_stride ||
            h->obs_stride != hs[0]->obs_stride || h->info_stride != hs[0]->info_stride)
            return fail(BIOIM_E_ARG, "bioim_rollout_group: handles differ in device, precision or I/O strides");
        if (h->rk && h->rk_budget > 0)
            return fail(BIOIM_E_ARG, "bioim_rollout_group: a budgeted RK handle suspends envs mid-step, a rollout has no rows "
                                     "for that (bioim_set_rk_budget(h, 0, NULL) first)");
        if (stop_at_done && h->auto_reset)
            return fail(BIOIM_E_ARG, "bioim_rollout_group: stop_at_done needs auto-reset off (a reset env goes on)");
        rows += (size_t)h->n;
    }
    if (nh == 1) {   /* one segment: bioim_rollout */
        const int rc = bioim_rollout(hs[0], actions, steps, action_step_stride, obs_seq, obs_last, reward_seq, done_seq,
                                     info_seq, stop_at_done);
        if (rc == 0) hs[0]->last_rollout_group_fused = hs[0]->last_rollout_fused;
        return rc;
    }
    HIPCHK(hipSetDevice(hs[0]->device));
    for (int i = 0; i < nh; ++i) {
        bioim_handle_t *h = hs[i];
        if (h->rk) {   /* only an RK handle can hold suspended envs; the count waits for its stream */
            const int np = bioim_pending_count(h);
            if (np < 0) return np;
            if (np > 0) return fail(BIOIM_E_ARG, "bioim_rollout_group: envs are suspended mid-step (bioim_set_rk_budget)");
        }
        if (const int rc = ensure_reset_table(h)) return rc;
        if (stop_at_done && !h->rollout_live && h->n > 0)
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&h->rollout_live), (size_t)h->n));
    }
    const RolloutCall c{actions, steps, action_step_stride, obs_seq, obs_last, reward_seq, done_seq, info_seq,
                        stop_at_done ? 1 : 0};
    hs[0]->last_rollout_group_fused = 0;
    /* ONE launch of rollout_kernel2 exactly where bioim_step_group would fuse
     * (two segments, fusion on, fp64 and a fused pair — bioim_rollout2_launch
     * answers those two —, no push table, not RK) and neither handle has a
     * force report or state storage */
    if (nh == 2 && g_group_fusion && rollout_fusable(hs[0]) && rollout_fusable(hs[1])) {
        const int rc = bioim_rollout2_launch(hs[0], hs[1], c);
        if (rc < 0) return rc;
        if (rc == 1) {
            HIPCHK(hipGetLastError());
            hs[0]->last_rollout_group_fused = 1;
            return 0;
        }
    }
    const int rc = hs[0]->precision == 64 ? rollout_group_host_loop<double>(hs, nh, c, rows)
                                          : rollout_group_host_loop<float>(hs, nh, c, rows);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

int bioim_rollout_group_fused(const bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "bioim_rollout_group_fused: null handle");
    return h->last_rollout_group_fused ? 1 : 0;
}

int bioim_sync(bioim_handle_t *h) {
    if (!h) return fail(BIOIM_E_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    return 0;
}

}  // extern "C"
#endif  // BIOIM_TOPO_ONLY
