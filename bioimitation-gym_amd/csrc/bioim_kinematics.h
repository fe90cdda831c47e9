// bioim_kinematics.h — phase 1 of the dynamics call: the coordinates into LDS,
// each body's joint-local transform (kin_local), the frames composed down the
// tree (kin_ground, kin_chain), the Plucker columns (kin_column) and the
// bodies' spatial inertias and velocity wrenches (body_inertia).
#pragma once

#include <hip/hip_runtime.h>

#include "bioim_config.h"
#include "bioim_curves.h"
#include "bioim_device.h"
#include "bioim_layout.h"
#include "bioim_math.h"
#include "topologies.h"

/* ------------------------------------------------- the per-lane index record
 * BIOIM_LANEIDX: what a lane reads from the model image's index tables in
 * every dynamics call, read once per launch (lane_index, env_block's prologue;
 * a fused rollout runs that prologue, image staging included, once per step)
 * and kept packed in registers.  A lane past a count (no dof, limit or muscle
 * of its own) carries element 0's values, or an empty mask: the
 * calls read those fields only under the same lane conditions as before.
 * Field widths are checked against the topology where a bit is on. */
DEV constexpr uint32_t li_bits(uint32_t w, int pos, int n) { return (w >> pos) & ((1u << n) - 1u); }
template <class T, typename Real> struct LaneIdx {
    using LY = Lay<T, Real>;
    static constexpr int MPL = LY::MPL, MP = T::MAXPT > 0 ? T::MAXPT : 1;
    static constexpr int NTW = (T::MAXARM + 3) / 4;
    /* LI_COLS: bits 0-15 the LDS word offset of the parent frame of the lane's
     * dof (KB + 18 pslot), 16-23 the dof's body */
    uint32_t cols;
    /* LI_TAU: the dof's TAU gather list, a byte per entry; lim: bits 0-7 the
     * limit lane's coordinate, bit 8 + li set where limit li acts on the dof */
    uint32_t tau[NTW], lim;
    /* LI_PATH, per muscle slot.  path: bits 0-7 pt_off, 8-11 npt, 12-15 nspan,
     * 16 + 4k the span's dof k (0 past nspan).  frame: 4 bits per point slot,
     * its body (point 0's past npt).  pt[j], the slots PT_COND / PT_MOVING
     * allow: bit 0 conditional, 1-5 its coordinate (0: not conditional),
     * bit 6 moving, 8 + 6a the function slot of axis a (5 bits; 0 and bit 5
     * set: none, the point's own location) */
    uint32_t path[MPL], frame[MPL], pt[MPL][MP];

    /* the record as one dynamics call reads it: the words in use made opaque,
     * so that the call's unpacked values and the addresses formed from them
     * are computed in the call (a shift and a mask) and not hoisted out of the
     * substep loop into registers of their own (LI_PATH alone took 21 more
     * registers that way, and the set put the Muscle2D kernels on scratch) */
    template <int LI> DEV LaneIdx call_copy() const {
        LaneIdx c = *this;
        auto hide = [](uint32_t &w) { asm volatile("" : "+v"(w)); };
        if constexpr ((LI & LI_COLS) != 0) hide(c.cols);
        if constexpr ((LI & LI_TAU) != 0) {
#pragma unroll
            for (int i = 0; i < NTW; ++i) hide(c.tau[i]);
            hide(c.lim);
        }
#pragma unroll
        for (int j = 0; j < MPL; ++j) {
            if constexpr ((LI & LI_PATH) != 0 && T::NM > 0) {
                hide(c.path[j]); hide(c.frame[j]);
                sfor<0, MP>([&](auto pI) {
                    constexpr int p = decltype(pI)::value;
                    if constexpr ((((T::PT_COND | T::PT_MOVING) >> p) & 1u) != 0) hide(c.pt[j][p]);
                });
            }
        }
        return c;
    }
    DEV int kp() const { return (int)li_bits(cols, 0, 16); }
    DEV int body() const { return (int)li_bits(cols, 16, 8); }
    DEV int tau_src(int i) const { return (int)li_bits(tau[i / 4], 8 * (i % 4), 8); }
    DEV int lim_coord() const { return (int)li_bits(lim, 0, 8); }
    DEV bool lim_mine(int li) const { return ((lim >> (8 + li)) & 1u) != 0; }
};

template <int LI, class T, typename Real>
DEV void lane_index(const SModel<T, Real> &SM, int lane, LaneIdx<T, Real> &I) {
    using LY = Lay<T, Real>;
    using IX = LaneIdx<T, Real>;
    if constexpr ((LI & LI_COLS) != 0) {
        static_assert(LY::KB + 18 * (T::NB + 1) < 65536 && T::NB < 256, "LI_COLS field widths");
        const int cb = SM.dof_cb[lane < LY::ND ? lane : 0];
        I.cols = (uint32_t)(LY::KB + 18 * SM.body[cb].pslot) | ((uint32_t)cb << 16);
    }
    if constexpr ((LI & LI_TAU) != 0) {
        static_assert(T::NC < 256 && T::NL <= 24, "LI_TAU field widths");
        const int d = lane < LY::ND ? lane : 0;
#pragma unroll
        for (int i = 0; i < IX::NTW; ++i) I.tau[i] = 0;
#pragma unroll
        for (int i = 0; i < T::MAXARM; ++i) I.tau[i / 4] |= (uint32_t)SM.tau_src[d][i] << (8 * (i % 4));
        uint32_t w = (uint32_t)SM.lim_coord[lane < T::NL ? lane : 0];
#pragma unroll
        for (int li = 0; li < T::NL; ++li) w |= (SM.lim_dof[li] == lane ? 1u : 0u) << (8 + li);
        I.lim = w;
    }
    if constexpr ((LI & LI_PATH) != 0 && T::NM > 0) {
        sfor<0, IX::MPL>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            const int m = mslot<T>(lane + j * T::G);
            const SMuscle<Real> &mu = SM.mus[m < T::NM ? m : 0];
            static_assert(T::NPT < 256 && T::MAXPT <= 8 && T::MAXSPAN <= 4 && LY::ND <= 16 && T::NB < 16 && T::NC <= 32 && LY::NSLOT <= 32,
                          "LI_PATH field widths");
            const int po = mu.pt_off, npt = mu.npt, nsp = mu.nspan;
            uint32_t w = (uint32_t)po | (uint32_t)npt << 8 | (uint32_t)nsp << 12, fw = 0;
#pragma unroll
            for (int k = 0; k < T::MAXSPAN; ++k) w |= (uint32_t)(k < nsp ? mu.span[k] : 0) << (16 + 4 * k);
            I.path[j] = w;
            sfor<0, IX::MP>([&](auto pI) {
                constexpr int p = decltype(pI)::value;
                const DPathPt<Real> &pt = SM.pt[po + (p < npt ? p : 0)];
                fw |= (uint32_t)pt.cbody << (4 * p);
                uint32_t pw = 0;
                if constexpr (((T::PT_COND >> p) & 1u) != 0) {
                    const bool cnd = pt.type == BIOIM_PT_COND;
                    pw |= (cnd ? 1u : 0u) | (uint32_t)(cnd ? pt.cond_coord : 0) << 1;
                }
                if constexpr (((T::PT_MOVING >> p) & 1u) != 0) {
                    pw |= (pt.type == BIOIM_PT_MOVING ? 1u : 0u) << 6;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const int f = pt.mf[a];
                        pw |= (f < 0 ? 32u : (uint32_t)f) << (8 + 6 * a);
                    }
                }
                I.pt[j][p] = pw;
            });
            I.frame[j] = fw;
        });
    }
}

/* publish the coordinate values/speeds to LDS (QF/UF): dof lane d writes its
 * coordinate, lane 0 the locked coordinates (default value, zero speed) */
template <class T, typename Real>
DEV void publish_coords(const DModel<Real> &M, const SModel<T, Real> &SM, Real *lds, int lane, Real qd, Real ud) {
    using LY = Lay<T, Real>;
    if (lane < T::ND) {
        const int c = SM.dof_coord[lane];
        lds[LY::QF + c] = qd;
        lds[LY::UF + c] = ud;
    }
    if (lane == 0) {
        sfor<0, T::NC>([&](auto cI) {
            constexpr int c = decltype(cI)::value;
            if constexpr (T::coord_dof[c] < 0) { lds[LY::QF + c] = M.coord_default[c]; lds[LY::UF + c] = 0; }
        });
    }
}

/* ---------------------------------------------------------- kinematics
 * Phase 1a (lane = composite body c): the joint-local part, which depends
 * only on c's own coordinates — the spatial-transform axes (function
 * values and derivatives, the body-fixed rotation sequence, translations),
 * giving the child-in-parent transform, the joint's relative velocity and
 * velocity-product acceleration in the parent frame, and the joint's
 * Plucker columns about the parent origin (accumulated per dof into SL). */

/* a body's dofs as kin_local meets them: the local slot of (body, axis) is
 * the rank of the axis's dof among the body's distinct dofs in axis order */
template <class T> struct BodyDofs {
    static constexpr int dof_of(int b, int ax) {
        const int co = T::axis_coord[b * 6 + ax];
        return co >= 0 ? T::coord_dof[co] : -1;
    }
    static constexpr int slot(int b, int ax) {
        const int d = dof_of(b, ax);
        if (d < 0) return -1;
        int n = 0;
        for (int a = 0; a < ax; ++a) {
            const int e = dof_of(b, a);
            if (e < 0) continue;
            bool seen = false;
            for (int a2 = 0; a2 < a; ++a2) seen = seen || dof_of(b, a2) == e;
            if (e == d) return n;
            n += seen ? 0 : 1;
        }
        return n;
    }
    static constexpr int count(int b) {
        int n = 0;
        for (int ax = 0; ax < 6; ++ax) n = slot(b, ax) + 1 > n ? slot(b, ax) + 1 : n;
        return n;
    }
    static constexpr int max_count() {
        int n = 1;
        for (int b = 0; b < T::NB; ++b) n = count(b) > n ? count(b) : n;
        return n;
    }
    static constexpr int dof(int b, int k) {
        for (int ax = 0; ax < 6; ++ax)
            if (slot(b, ax) == k) return dof_of(b, ax);
        return -1;
    }
    /* every dof is a local dof of exactly one body (its SL row has one writer) */
    static constexpr bool covers_all() {
        for (int d = 0; d < T::ND; ++d) {
            int n = 0;
            for (int b = 0; b < T::NB; ++b)
                for (int k = 0; k < count(b); ++k) n += dof(b, k) == d ? 1 : 0;
            if (n != 1) return false;
        }
        return true;
    }
};

template <class T, typename Real, int FE = 0>
DEV void kin_local(const SModel<T, Real> &SM, Real *lds, int c) {
    using LY = Lay<T, Real>;
    using PL = Planar<T>;
    constexpr unsigned ZR = PL::ZR, ZW = PL::ZW, ZV = PL::ZV;
    constexpr unsigned USED = TopoInfo<T>::axes_used();
    const SBody<Real> &b = SM.body[c];
    Real RFM[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Real wrel[3] = {0, 0, 0}, arel[3] = {0, 0, 0}, pFM[3] = {0, 0, 0}, pd[3] = {0, 0, 0}, pdd[3] = {0, 0, 0};
    Real col[6][3];
    int cd[6];   /* the axis's dof; FE_COLS: its local slot (BodyDofs) */
    sfor<0, 6>([&](auto aI) {
        constexpr int ax = decltype(aI)::value;
        cd[ax] = -1;
        if constexpr (((USED >> ax) & 1u) != 0) {
            /* the axis function's kind, coordinate, dof and spline slot are
             * compile-time facts of (body, axis) (topology_matches checks kind
             * and coordinate per pack): selected by the lane instead of read
             * through the function table, so the coordinate and coefficient
             * loads do not wait on one another */
            int kind = -1, cc = -1, dof = -1, js = -1;
            /* spatial models: an opaque copy of the lane's body, so the
             * selects are recomputed per call (a few VALU ops) instead of
             * hoisted out of the substep loop into 24 registers live across
             * it (the 3D push + RK-Merson kernel otherwise spills 16 B; 1 %
             * slower in 3D, so the planar kernels, far from the register
             * limit, keep the hoisted copies) */
            int cb = c;
            if constexpr (!T::PLANAR) asm volatile("" : "+v"(cb));
            sfor<0, T::NB>([&](auto bI) {
                constexpr int bb = decltype(bI)::value;
                constexpr int k = T::axis_kind[bb * 6 + ax], co = T::axis_coord[bb * 6 + ax];
                constexpr int dc = co >= 0 ? T::coord_dof[co] : -1, jsl = TopoInfo<T>::jslot(bb, ax);
                kind = cb == bb ? k : kind;
                cc = cb == bb ? co : cc;
                constexpr int dl = (FE & FE_COLS) ? BodyDofs<T>::slot(bb, ax) : dc;
                dof = cb == bb ? dl : dof;
                js = cb == bb ? jsl : js;
            });
            const int cs = cc >= 0 ? cc : 0;
            Real qc = lds[LY::QF + cs], uc = lds[LY::UF + cs];
            qc = cc >= 0 ? qc : Real(0);
            uc = cc >= 0 ? uc : Real(0);
            constexpr unsigned KM = TopoInfo<T>::axis_kinds(ax);
            const Real fa = b.fa[ax], fb = b.fb[ax];
            Real f = 0, f1 = 0, f2 = 0;
            if constexpr ((FE & FE_KINDS) && T::PLANAR) {
                /* both forms from the loads above, selected */
                if constexpr ((KM & (1u << (BIOIM_FN_LINEAR + 1))) != 0) {
                    const bool li = kind == BIOIM_FN_LINEAR;
                    const Real lf = fa * qc + fb;
                    f = li ? lf : f; f1 = li ? fa : f1;
                }
                if constexpr ((KM & (1u << (BIOIM_FN_CONST + 1))) != 0) f = kind == BIOIM_FN_CONST ? fb : f;
            } else {
                if constexpr ((KM & (1u << (BIOIM_FN_LINEAR + 1))) != 0) {
                    if (kind == BIOIM_FN_LINEAR) { f = fa * qc + fb; f1 = fa; }
                }
                if constexpr ((KM & (1u << (BIOIM_FN_CONST + 1))) != 0) {
                    if (kind == BIOIM_FN_CONST) f = fb;
                }
            }
            if constexpr ((KM & (1u << (BIOIM_FN_SPLINE + 1))) != 0) {
                /* spline axes: evaluated in phase 0b.  Planar: loaded
                 * unconditionally (slot 0 for the other kinds) and selected,
                 * no branch (same-box Torque2D -3 %, 2D -0.7 % with the
                 * branch-free SL and subtree sums; no gain in 3D, where it
                 * costs registers: profiles/r03/ab_subtree.txt) */
                const int jj = js >= 0 ? js : 0;
                if constexpr (T::PLANAR) {
                    const bool sp = kind == BIOIM_FN_SPLINE;
                    const Real sf = lds[LY::MF + 3 * jj], sf1 = lds[LY::MF + 3 * jj + 1], sf2 = lds[LY::MF + 3 * jj + 2];
                    f = sp ? sf : f; f1 = sp ? sf1 : f1; f2 = sp ? sf2 : f2;
                } else if (kind == BIOIM_FN_SPLINE) {
                    f = lds[LY::MF + 3 * jj]; f1 = lds[LY::MF + 3 * jj + 1]; f2 = lds[LY::MF + 3 * jj + 2];
                }
            }
            cd[ax] = dof;
            Real a[3] = {b.axis[ax][0], b.axis[ax][1], b.axis[ax][2]};
            if constexpr (ax < 3) {
                PL::ang(a);
                Real ucol[3], cr[3];
                mv3m<ZR, ZW>(RFM, a, ucol);
                Real thd = f1 * uc;
                cross3m<ZW, ZW>(wrel, ucol, cr);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    arel[i] += ucol[i] * (f2 * uc * uc) + cr[i] * thd;
                    wrel[i] += ucol[i] * thd;
                    col[ax][i] = ucol[i] * f1;
                }
                PL::ang(arel); PL::ang(wrel); PL::ang(col[ax]);
                Real Rk[9];
                if constexpr (T::PLANAR) {   /* about (0, 0, a_z), a_z = +-1 */
                    Real sn, cn;
                    sincos_rt(f, sn, cn);
                    Rk[0] = cn; Rk[1] = -sn * a[2]; Rk[3] = sn * a[2]; Rk[4] = cn;
                    PL::rot(Rk);
                } else {
                    axis_rot(a, f, Rk);  /* f == 0 (absent axis): identity */
                }
                mm3m<ZR, ZR>(RFM, Rk, RFM);
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    pFM[i] += a[i] * f; pd[i] += a[i] * (f1 * uc); pdd[i] += a[i] * (f2 * uc * uc);
                    col[ax][i] = a[i] * f1;
                }
                PL::lin(pd); PL::lin(pdd); PL::lin(col[ax]);
            }
        }
    });
    Real Rpf[9], Rmb[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { Rpf[i] = b.R_pf[i]; Rmb[i] = b.R_mb[i]; }
    PL::rot(Rpf); PL::rot(Rmb);
    Real dF[3], T9[9], RPB[9], pm[3], pPB[3];
    mv3m<ZR, 0>(RFM, b.p_mb, dF);
    mm3m<ZR, ZR>(Rpf, RFM, T9);
    mm3m<ZR, ZR>(T9, Rmb, RPB);
#pragma unroll
    for (int i = 0; i < 3; ++i) pm[i] = pFM[i] + dF[i];
    mv3m<ZR, 0>(Rpf, pm, pPB);
    Real *lc = lds + LY::LOC + 24 * c;
#pragma unroll
    for (int i = 0; i < 9; ++i) lc[i] = RPB[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) lc[9 + i] = pPB[i] + b.p_pf[i];
    Real t1[3], t2[3], t3[3], o[3];
    mv3m<ZR, ZW>(Rpf, wrel, o);
#pragma unroll
    for (int i = 0; i < 3; ++i) lc[12 + i] = o[i];
    cross3m<ZW, 0>(wrel, dF, t1);
#pragma unroll
    for (int i = 0; i < 3; ++i) t2[i] = pd[i] + t1[i];
    mv3m<ZR, ZV>(Rpf, t2, o);
#pragma unroll
    for (int i = 0; i < 3; ++i) lc[15 + i] = o[i];
    mv3m<ZR, ZW>(Rpf, arel, o);
#pragma unroll
    for (int i = 0; i < 3; ++i) lc[18 + i] = o[i];
    cross3m<ZW, 0>(arel, dF, t2);
    cross3m<ZW, ZV>(wrel, t1, t3);
#pragma unroll
    for (int i = 0; i < 3; ++i) t2[i] = pdd[i] + t2[i] + t3[i];
    mv3m<ZR, ZV>(Rpf, t2, o);
#pragma unroll
    for (int i = 0; i < 3; ++i) lc[21 + i] = o[i];
    /* Plucker columns in the parent frame, linear part at the parent origin;
     * rotations act about the M origin pM = p_pf + R_pf pFM */
    Real pM[3];
    mv3m<ZR, 0>(Rpf, pFM, pM);
#pragma unroll
    for (int i = 0; i < 3; ++i) pM[i] += b.p_pf[i];
    if constexpr ((FE & FE_COLS) != 0) {
        /* per local dof slot k: 0 + the contributions of the axes that move
         * it, in axis order (selects; an axis without a dof matches no slot),
         * then one plain store of the dof's words */
        constexpr int NLS = BodyDofs<T>::max_count();
        static_assert(BodyDofs<T>::covers_all(), "FE_COLS: one body lane stores each dof's SL row");
        Real acc[NLS][6];
#pragma unroll
        for (int k = 0; k < NLS; ++k)
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[k][i] = 0;
        sfor<0, 6>([&](auto aI) {
            constexpr int ax = decltype(aI)::value;
            if constexpr (((USED >> ax) & 1u) != 0) {
                Real v[3], lin[3] = {0, 0, 0};
                if constexpr (ax < 3) {
                    mv3m<ZR, ZW>(Rpf, col[ax], v);
                    cross3m<0, ZW>(pM, v, lin);
                } else {
                    mv3m<ZR, ZV>(Rpf, col[ax], v);
                }
#pragma unroll
                for (int k = 0; k < NLS; ++k) {
                    const bool on = cd[ax] == k;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if constexpr (ax < 3) {
                            if (!((ZW >> i) & 1u)) acc[k][i] = on ? acc[k][i] + v[i] : acc[k][i];
                            if (!((ZV >> i) & 1u)) acc[k][3 + i] = on ? acc[k][3 + i] + lin[i] : acc[k][3 + i];
                        } else {
                            if (!((ZV >> i) & 1u)) acc[k][3 + i] = on ? acc[k][3 + i] + v[i] : acc[k][3 + i];
                        }
                    }
                }
            }
        });
        int cb = c;
        if constexpr (!T::PLANAR) asm volatile("" : "+v"(cb));
        sfor<0, NLS>([&](auto kI) {
            constexpr int k = decltype(kI)::value;
            int dk = -1;
            sfor<0, T::NB>([&](auto bI) {
                constexpr int bb = decltype(bI)::value;
                constexpr int dbk = BodyDofs<T>::dof(bb, k);
                dk = cb == bb ? dbk : dk;
            });
            if (dk >= 0) {
                Real *sl = lds + LY::SL + 6 * dk;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (!((ZW >> i) & 1u)) sl[i] = acc[k][i];
                    if (!((ZV >> i) & 1u)) sl[3 + i] = acc[k][3 + i];
                }
            }
        });
    } else
    sfor<0, 6>([&](auto aI) {
        constexpr int ax = decltype(aI)::value;
        if constexpr (((USED >> ax) & 1u) != 0) {
            /* planar: an axis without a dof accumulates into the sink row
             * SL[ND] (no branch) */
            if (T::PLANAR || cd[ax] >= 0) {
                Real *sl = lds + LY::SL + 6 * (cd[ax] >= 0 ? cd[ax] : LY::ND);
                Real v[3];
                if constexpr (ax < 3) {
                    mv3m<ZR, ZW>(Rpf, col[ax], v);
                    Real lin[3];
                    cross3m<0, ZW>(pM, v, lin);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if (!((ZW >> i) & 1u)) sl[i] += v[i];
                        if (!((ZV >> i) & 1u)) sl[3 + i] += lin[i];
                    }
                } else {
                    mv3m<ZR, ZV>(Rpf, col[ax], v);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (!((ZV >> i) & 1u)) sl[3 + i] += v[i];
                }
            }
        }
    });
}

/* body frame and motion: orientation, origin, angular velocity, spatial
 * velocity at the (shifted) ground origin, and the velocity-product
 * accelerations (zero q'') */
template <typename Real> struct Frame {
    Real R[9], o[3], w[3], vO[3], al[3], aO[3];
};

/* F := F composed with the joint whose parent-frame data is lc (LOC slot).
 * Zero masks: R rotations, w/wrg/al angular, vO/vrel/aO/aa linear (Planar) */
template <class T, typename Real> DEV void compose(Frame<Real> &F, const Real *lc) {
    using PL = Planar<T>;
    constexpr unsigned ZR = PL::ZR, ZW = PL::ZW, ZV = PL::ZV;
    Real R[9], oB[3], w[3], wrg[3], vrel[3], vO[3], al[3], t[3], t2[3], t3[3];
    mm3m<ZR, ZR>(F.R, lc, R);
    mv3m<ZR, 0>(F.R, lc + 9, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) oB[i] = F.o[i] + t[i];
    mv3m<ZR, ZW>(F.R, lc + 12, wrg);
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = F.w[i] + wrg[i];
    mv3m<ZR, ZV>(F.R, lc + 15, vrel);
    cross3m<ZW, 0>(wrg, oB, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) vO[i] = F.vO[i] + vrel[i] - t[i];
    mv3m<ZR, ZW>(F.R, lc + 18, t);
    cross3m<ZW, ZW>(F.w, wrg, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) al[i] = F.al[i] + t2[i] + t[i];
    /* acceleration of the new origin: parent point acceleration
     * + Coriolis 2 wP x vrel + relative acceleration */
    Real vpt[3], aB[3], aa[3];
    cross3m<ZW, 0>(F.w, oB, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) vpt[i] = F.vO[i] + t[i];
    cross3m<ZW, 0>(F.al, oB, t);
    cross3m<ZW, ZV>(F.w, vpt, t2);
    cross3m<ZW, ZV>(F.w, vrel, t3);
    mv3m<ZR, ZV>(F.R, lc + 21, aa);
#pragma unroll
    for (int i = 0; i < 3; ++i) aB[i] = F.aO[i] + t[i] + t2[i] + Real(2) * t3[i] + aa[i];
    Real vB[3];
    cross3m<ZW, 0>(w, oB, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) vB[i] = vO[i] + t[i];
    cross3m<ZW, 0>(al, oB, t);
    cross3m<ZW, ZV>(w, vB, t2);
#pragma unroll
    for (int i = 0; i < 9; ++i) F.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        F.aO[i] = aB[i] - t[i] - t2[i];
        F.o[i] = oB[i]; F.w[i] = w[i]; F.vO[i] = vO[i]; F.al[i] = al[i];
    }
    PL::rot(F.R); PL::ang(F.w); PL::lin(F.vO); PL::ang(F.al); PL::lin(F.aO);
}

/* FE_LEVEL0: compose() for the chain's first level, whose F is the ground
 * frame (R = I, o = (-x0, 0, 0), no motion): the same values without the
 * products with those constants (equal for finite inputs up to the sign of a
 * zero) */
template <class T, typename Real> DEV void compose_ground(Frame<Real> &F, const Real *lc, Real x0) {
    using PL = Planar<T>;
    constexpr unsigned ZW = PL::ZW, ZV = PL::ZV;
    Real oB[3], vB[3], t[3], t2[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) F.R[i] = lc[i];
    oB[0] = lc[9] - x0; oB[1] = lc[10]; oB[2] = lc[11];
    const Real *wrg = lc + 12, *vrel = lc + 15, *al = lc + 18, *aa = lc + 21;
    cross3m<ZW, 0>(wrg, oB, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) { F.o[i] = oB[i]; F.w[i] = wrg[i]; F.vO[i] = vrel[i] - t[i]; F.al[i] = al[i]; }
    cross3m<ZW, 0>(F.w, oB, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) vB[i] = F.vO[i] + t[i];
    cross3m<ZW, 0>(al, oB, t);
    cross3m<ZW, ZV>(F.w, vB, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) F.aO[i] = aa[i] - t[i] - t2[i];
    PL::rot(F.R); PL::ang(F.w); PL::lin(F.vO); PL::ang(F.al); PL::lin(F.aO);
}

/* identity joint (LOC slot NB) and the ground frame (KB/AL slot NB) */
template <class T, typename Real> DEV constexpr bool ground_loc_free() {
    using LY = Lay<T, Real>;
    return LY::LOC + 24 * T::NB >= LY::TAU + LY::TAUN && LY::LOC + 24 * T::NB >= LY::CJ + LY::NS * LY::CJN;
}
template <class T, typename Real> DEV void kin_ground_loc(Real *lds) {
    Real *lc = lds + Lay<T, Real>::LOC + 24 * T::NB;
#pragma unroll
    for (int i = 0; i < 24; ++i) lc[i] = (i < 9 && (i % 4) == 0) ? Real(1) : Real(0);
}
template <class T, typename Real> DEV void kin_ground_const(Real *lds) {
    using LY = Lay<T, Real>;
    Real *kb = lds + LY::KB + 18 * T::NB, *ab = lds + LY::AL + 6 * T::NB;
#pragma unroll
    for (int i = 0; i < 18; ++i) kb[i] = (i < 9 && (i % 4) == 0) ? Real(1) : Real(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) ab[i] = 0;
}
template <class T, typename Real, bool ONCE = false> DEV void kin_ground(Real *lds, Real x0) {
    if constexpr (!ONCE || !ground_loc_free<T, Real>()) kin_ground_loc<T, Real>(lds);
    if constexpr (!ONCE) kin_ground_const<T, Real>(lds);
    lds[Lay<T, Real>::KB + 18 * T::NB + 9] = -x0;
}

/* Phase 1b (lane = body c): compose c's root-to-body joint chain in
 * registers (front-padded with the identity joint, so every lane runs the
 * same DEPTH compositions with no inter-lane dependency) */
template <class T, typename Real, int FE = 0>
DEV void kin_chain(const SModel<T, Real> &SM, Real *lds, int c, Real x0, Frame<Real> &F) {
    using LY = Lay<T, Real>;
#pragma unroll
    for (int i = 0; i < 9; ++i) F.R[i] = (i % 4) == 0 ? Real(1) : Real(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) { F.o[i] = i == 0 ? -x0 : Real(0); F.w[i] = 0; F.vO[i] = 0; F.al[i] = 0; F.aO[i] = 0; }
    sfor<0, TopoInfo<T>::depth()>([&](auto lI) {
        constexpr int lvl = decltype(lI)::value;
        const Real *src = lds + LY::LOC + 24 * SM.chain[c][lvl];
        Real lc[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) lc[i] = src[i];
        Planar<T>::loc(lc);
        if constexpr (lvl == 0 && (FE & FE_LEVEL0) != 0) compose_ground<T, Real>(F, lc, x0);
        else compose<T, Real>(F, lc);
    });
    Real *kb = lds + LY::KB + 18 * c, *ab = lds + LY::AL + 6 * c;
#pragma unroll
    for (int i = 0; i < 9; ++i) kb[i] = F.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        kb[9 + i] = F.o[i]; kb[12 + i] = F.w[i]; kb[15 + i] = F.vO[i];
        ab[i] = F.al[i]; ab[3 + i] = F.aO[i];
    }
}
template <class T, typename Real>
DEV void kin_chain(const SModel<T, Real> &SM, Real *lds, int c, Real x0) {
    Frame<Real> F;
    kin_chain<T, Real>(SM, lds, c, x0, F);
}

/* Phase 0b: the function slots (Lay::MF), one lane each — moving path
 * points' location functions and the joints' spline axes — from the
 * published coordinates; ends with a wave sync when there are any */
template <bool BFK, class T, typename Real>
DEV void fn_slots(const SModel<T, Real> &SM, Real *lds, int lane) {
    using LY = Lay<T, Real>;
    if constexpr (LY::NSLOT > 0) {
        sfor<0, (LY::NSLOT + T::G - 1) / T::G>([&](auto pI) {
            const int f = lane + decltype(pI)::value * T::G;
            if (f < LY::NSLOT) {
                Real v, d1, d2;
                fn_eval_bf<BFK, T, Real>(SM, SM.mf_fn[f], lds[LY::QF + SM.mf_coord[f]], v, d1, d2);
                lds[LY::MF + 3 * f] = v;
                lds[LY::MF + 3 * f + 1] = d1;
                lds[LY::MF + 3 * f + 2] = d2;
            }
        });
        wave_sync();
    }
}

/* Phase 1c (lane = dof): ground Plucker column from the parent frame */
template <class T, typename Real, int LI = 0>
DEV void kin_column(const SModel<T, Real> &SM, Real *lds, int d, const LaneIdx<T, Real> *I = nullptr) {
    using LY = Lay<T, Real>;
    using PL = Planar<T>;
    constexpr unsigned ZR = PL::ZR, ZW = PL::ZW, ZV = PL::ZV;
    const Real *kp;
    if constexpr ((LI & LI_COLS) != 0) kp = lds + I->kp();
    else kp = lds + LY::KB + 18 * SM.body[SM.dof_cb[d]].pslot;
    const Real *sl = lds + LY::SL + 6 * d;
    Real K[12], sc[6];
#pragma unroll
    for (int i = 0; i < 12; ++i) K[i] = kp[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) sc[i] = sl[i];
    PL::rot(K); PL::col(sc);
    Real Sa[3], Sl[3], t[3];
    mv3m<ZR, ZW>(K, sc, Sa);
    mv3m<ZR, ZV>(K, sc + 3, Sl);
    cross3m<ZW, 0>(Sa, K + 9, t);
    Real *S = lds + LY::S + 6 * d;
#pragma unroll
    for (int i = 0; i < 3; ++i) { S[i] = Sa[i]; S[3 + i] = Sl[i] - t[i]; }
}

/* Phase 1c (lane = body): spatial inertia at the ground origin and the
 * Newton-Euler (velocity-product + gravity) wrench */
template <class T, typename Real, bool FROM_FRAME = false>
DEV void body_inertia(const SModel<T, Real> &SM, const DModel<Real> &M, Real *lds, int c, const Frame<Real> *F = nullptr) {
    using LY = Lay<T, Real>;
    using PL = Planar<T>;
    constexpr unsigned ZR = PL::ZR, ZW = PL::ZW, ZV = PL::ZV;
    const SBody<Real> &b = SM.body[c];
    const Real *kb = lds + LY::KB + 18 * c, *ab = lds + LY::AL + 6 * c;
    Real K[18], A[6];
    if constexpr (FROM_FRAME) {   /* FE_INERTIA: the frame kin_chain left in the lane's registers */
#pragma unroll
        for (int i = 0; i < 9; ++i) K[i] = F->R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            K[9 + i] = F->o[i]; K[12 + i] = F->w[i]; K[15 + i] = F->vO[i];
            A[i] = F->al[i]; A[3 + i] = F->aO[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 18; ++i) K[i] = kb[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i] = ab[i];
    }
    PL::frame(K); PL::acc(A);
    const Real *R = K, *o = K + 9, *w = K + 12, *vO = K + 15, *al = A, *aO = A + 3;
    Real cl[3], cG[3];
    mv3m<ZR, 0>(R, b.com, cl);
#pragma unroll
    for (int i = 0; i < 3; ++i) cG[i] = o[i] + cl[i];
    Real Ib[9] = {b.inertia[0], b.inertia[3], b.inertia[4], b.inertia[3], b.inertia[1],
                  b.inertia[5], b.inertia[4], b.inertia[5], b.inertia[2]};
    Real Tm[9], RT[9], IG[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) RT[3 * i + j] = R[3 * j + i];
    mm3m<ZR, 0>(R, Ib, Tm);
    mm3m<0, ZR>(Tm, RT, IG);
    Real m = b.mass, ccd = dot3(cG, cG);
    Real *ic = lds + LY::IC + 10 * c;
    ic[0] = m;
#pragma unroll
    for (int i = 0; i < 3; ++i) ic[1 + i] = m * cG[i];
    ic[4] = IG[0] + m * (ccd - cG[0] * cG[0]);
    ic[5] = IG[4] + m * (ccd - cG[1] * cG[1]);
    ic[6] = IG[8] + m * (ccd - cG[2] * cG[2]);
    ic[7] = IG[1] - m * cG[0] * cG[1];
    ic[8] = IG[2] - m * cG[0] * cG[2];
    ic[9] = IG[5] - m * cG[1] * cG[2];
    Real vc[3], ac[3], t[3], t2[3];
    cross3m<ZW, 0>(w, cG, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) vc[i] = vO[i] + t[i];
    cross3m<ZW, 0>(al, cG, t);
    cross3m<ZW, ZV>(w, vc, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) ac[i] = aO[i] + t[i] + t2[i];
    Real f[3], Iw[3], Ia[3], n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = m * (ac[i] - M.gravity[i]);
    mv3m<0, ZW>(IG, w, Iw);
    mv3m<0, ZW>(IG, al, Ia);
    cross3m<ZW, 0>(w, Iw, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = Ia[i] + t[i];
    cross3(cG, f, t);
    Real *wb = lds + LY::WB + 6 * c;
#pragma unroll
    for (int i = 0; i < 3; ++i) { wb[i] = n[i] + t[i]; wb[3 + i] = f[i]; }
}
