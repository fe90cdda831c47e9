// bioim_curves.h — scalar functions of one variable as the model image holds
// them: the joint functions (natural cubic splines and the other fn_eval
// kinds), the muscles' quintic Bezier curves (curve_eval) and the
// fiber-velocity root on the force-velocity curve (solve_fv).
#pragma once

#include <hip/hip_runtime.h>

#include "bioim_config.h"
#include "bioim_device.h"
#include "bioim_diag.h"
#include "bioim_math.h"
#include "topologies.h"

/* ------------------------------------------------------------ functions */
template <class T, typename Real>
DEV void spline_eval(const SModel<T, Real> &SM, int off, int n, Real q, Real &f, Real &f1, Real &f2) {
    Real x0 = SM.kx[off], xn = SM.kx[off + n - 1];
    if (q < x0) { f = SM.ky[off] + (q - x0) * SM.kb[off]; f1 = SM.kb[off]; f2 = 0; return; }
    if (q > xn) {
        int j = off + n - 1;
        f = SM.ky[j] + (q - xn) * SM.kb[j]; f1 = SM.kb[j]; f2 = 0; return;
    }
    /* interval search: fixed trip count, all loads independent (one LDS wait) */
    int k = 0;
#pragma unroll
    for (int i = 1; i < T::NKMAX - 1; ++i) {
        Real xi = SM.kx[off + (i < n - 1 ? i : 0)];
        k += (i < n - 1 && q > xi) ? 1 : 0;
    }
    int j = off + k;
    Real dx = q - SM.kx[j], b = SM.kb[j], c = SM.kc[j], d = SM.kd[j];
    f = SM.ky[j] + dx * (b + dx * (c + dx * d));
    f1 = b + dx * (Real(2) * c + Real(3) * dx * d);
    f2 = Real(2) * c + Real(6) * dx * d;
}

/* value and first two derivatives of function fi (fi < 0: absent axis, 0) */
template <class T, typename Real>
DEV void fn_eval(const SModel<T, Real> &SM, int fi, Real q, Real &f, Real &f1, Real &f2) {
    f = 0; f1 = 0; f2 = 0;
    if (fi < 0) return;
    const SFn<Real> &F = SM.fn[fi];
    if (F.type == BIOIM_FN_CONST) { f = F.b; }
    else if (F.type == BIOIM_FN_LINEAR) { f = F.a * q + F.b; f1 = F.a; }
    else {
        Real s, s1, s2;
        spline_eval<T, Real>(SM, F.off, F.n, q, s, s1, s2);
        f = F.a * s; f1 = F.a * s1; f2 = F.a * s2;
    }
}

/* fn_eval without branches (phase 0b's function slots): the spline is
 * evaluated at the argument clamped to its knots (interval search and
 * coefficients as in spline_eval) and the linear extrapolation, constant and
 * linear kinds are selected; the same values as fn_eval, in one basic block
 * so the slot's dependent LDS loads are not split by branches */
template <bool BFK, class T, typename Real>
DEV void fn_eval_bf(const SModel<T, Real> &SM, int fi, Real q, Real &f, Real &f1, Real &f2) {
    const SFn<Real> &F = SM.fn[fi < 0 ? 0 : fi];
    const int type = F.type, oo = F.off >= 0 ? F.off : 0, nn = F.n > 1 ? F.n : 1;
    const Real a = F.a, b = F.b;
    const Real x0 = SM.kx[oo], xn = SM.kx[oo + nn - 1];
    const Real qc = q < x0 ? x0 : (q > xn ? xn : q);
    int k = 0;
#pragma unroll
    for (int i = 1; i < T::NKMAX - 1; ++i) {
        const Real xi = SM.kx[oo + (i < nn - 1 ? i : 0)];
        k += (i < nn - 1 && qc > xi) ? 1 : 0;
    }
    const int j = oo + k, jn = oo + nn - 1;
    const Real dx = qc - SM.kx[j], kb = SM.kb[j], kc = SM.kc[j], kd = SM.kd[j];
    Real s0 = SM.ky[j] + dx * (kb + dx * (kc + dx * kd));
    Real s1 = kb + dx * (Real(2) * kc + Real(3) * dx * kd);
    Real s2 = Real(2) * kc + Real(6) * dx * kd;
    const Real ylo = SM.ky[oo], blo = SM.kb[oo], yhi = SM.ky[jn], bhi = SM.kb[jn];
    const bool lo = q < x0, hi = q > xn;
    /* every ?: below picks between plain locals: clang emits a ?: whose arms
     * are expressions as a branch, the loads feeding an arm then sink into
     * it and the branch can no longer be folded into a select */
    const bool con = type == BIOIM_FN_CONST, lin = type == BIOIM_FN_LINEAR, present = fi >= 0;
    if constexpr (BFK) {
        const Real elo = ylo + (q - x0) * blo, ehi = yhi + (q - xn) * bhi, zero = 0;
        s0 = lo ? elo : (hi ? ehi : s0);
        s1 = lo ? blo : (hi ? bhi : s1);
        s2 = lo || hi ? zero : s2;
        const Real vl = a * q + b, vs = a * s0, vs1 = a * s1, vs2 = a * s2;
        f = !present ? zero : (con ? b : (lin ? vl : vs));
        f1 = !present || con ? zero : (lin ? a : vs1);
        f2 = !present || con || lin ? zero : vs2;
    } else {
        s0 = lo ? ylo + (q - x0) * blo : (hi ? yhi + (q - xn) * bhi : s0);
        s1 = lo ? blo : (hi ? bhi : s1);
        s2 = lo || hi ? Real(0) : s2;
        f = !present ? Real(0) : (con ? b : (lin ? a * q + b : a * s0));
        f1 = !present || con ? Real(0) : (lin ? a : a * s1);
        f2 = !present || con || lin ? Real(0) : a * s2;
    }
}

/* fn_eval specialised to the function kinds KM (bit kind+1; bit 0 = absent
 * axis) that can occur at this call site (compile-time, per topology axis) */
template <unsigned KM, class T, typename Real>
DEV void fn_eval_km(const SModel<T, Real> &SM, int fi, Real q, Real &f, Real &f1, Real &f2) {
    constexpr bool ABS = (KM & 1u) != 0, CON = (KM & 2u) != 0, LIN = (KM & 4u) != 0, SPL = (KM & 8u) != 0;
    f = 0; f1 = 0; f2 = 0;
    if constexpr (!CON && !LIN && !SPL) return;
    const SFn<Real> &F = SM.fn[ABS ? (fi < 0 ? 0 : fi) : fi];
    const Real a = F.a, b = F.b;
    const int type = F.type;
    Real v = 0, v1 = 0, v2 = 0;
    if constexpr (LIN && CON) { const bool lin = type == BIOIM_FN_LINEAR; v = lin ? a * q + b : b; v1 = lin ? a : Real(0); }
    else if constexpr (LIN) { v = a * q + b; v1 = a; }
    else if constexpr (CON) { v = b; }
    if constexpr (SPL) {
        if (type == BIOIM_FN_SPLINE) {
            Real s0, s1, s2;
            spline_eval<T, Real>(SM, F.off, F.n, q, s0, s1, s2);
            v = a * s0; v1 = a * s1; v2 = a * s2;
        }
    }
    const bool present = !ABS || fi >= 0;
    f = present ? v : Real(0); f1 = present ? v1 : Real(0); f2 = present ? v2 : Real(0);
}

/* ----------------------------------------------------- smooth curves */

/* a quintic segment in the power basis c[0] + c[1] u + ... + c[5] u^5
 * (converted from the Bezier control points at create time, convert_curve):
 * Horner, 5 FMAs; the derivative 4 */
template <typename Real> DEV Real bez5(const Real *c, Real u) {
    return fma(fma(fma(fma(fma(c[5], u, c[4]), u, c[3]), u, c[2]), u, c[1]), u, c[0]);
}
template <typename Real> DEV Real dbez5(const Real *c, Real u) {
    return fma(fma(fma(fma(Real(5) * c[5], u, Real(4) * c[4]), u, Real(3) * c[3]), u, Real(2) * c[2]), u, c[1]);
}

/* y(x), dy/dx of a SmoothSegmentedFunction.  Branch-free with a fixed trip
 * count (no lane divergence): segment located by comparisons, u(x) started
 * from the segment's 32-interval table by cubic Hermite interpolation (node
 * values ut and slopes mt; start error <= 3.1e-5 over every shipped curve),
 * then Newton steps on the quintic x(u): two reach machine precision in
 * fp64, one is below fp32 rounding (tests/test_curves.py); linear
 * extrapolation outside [x0, x1]. */
template <bool BF = true, typename Real>
DEV void curve_eval(const DCurve<Real> &C, Real x, Real &y, Real &dydx) {
    Real xc = x < C.x0 ? C.x0 : (x > C.x1 ? C.x1 : x);
    int k = 0;
#pragma unroll
    for (int s = 0; s < BIOIM_MAX_CURVESEG - 1; ++s) k += xc > C.xsep[s] ? 1 : 0;
    Real px[6], py[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { px[i] = C.cx[k][i]; py[i] = C.cy[k][i]; }
    Real tt = (xc - C.xa[k]) * C.inv_h[k];
    int i0 = (int)tt;
    i0 = i0 < 0 ? 0 : (i0 > BIOIM_UTAB - 1 ? BIOIM_UTAB - 1 : i0);
    Real fr = tt - Real(i0);
    /* Hermite basis in the form u0 + f (m0 + f (c2 + f c3)) */
    const Real u0 = Real(C.ut[k][i0]), u1 = Real(C.ut[k][i0 + 1]), m0 = Real(C.mt[k][i0]), m1 = Real(C.mt[k][i0 + 1]);
    const Real du = u1 - u0;
    const Real c2 = Real(3) * du - Real(2) * m0 - m1, c3 = m0 + m1 - Real(2) * du;
    Real u = fma(fr, fma(fr, fma(fr, c3, c2), m0), u0);
#pragma unroll
    for (int it = 0; it < Eps<Real>::curve_newton; ++it) u -= (bez5(px, u) - xc) * newton_rcp(dbez5(px, u));
    y = bez5(py, u);
    dydx = dbez5(py, u) * fast_rcp(dbez5(px, u));
    /* linear extrapolation blended in by 0 / 1 weights (every term finite):
     * a load under the condition, or a select of loaded values, made the
     * compiler branch, which split the muscle eval's three independent curve
     * chains into separate basic blocks */
    if constexpr (BF) {
        const Real x0 = C.x0, y0 = C.y0, d0 = C.dydx0, x1 = C.x1, y1 = C.y1, d1 = C.dydx1;
        const Real ylo = y0 + d0 * (x - x0), yhi = y1 + d1 * (x - x1);
        const Real wb = x < x0 ? Real(1) : Real(0), wa = x > x1 ? Real(1) : Real(0), wm = Real(1) - wb - wa;
        y = fma(wb, ylo, fma(wa, yhi, wm * y));
        dydx = fma(wb, d0, fma(wa, d1, wm * dydx));
    } else {   /* the branching form: separate blocks, fewer values live at once */
        if (x < C.x0) { y = C.y0 + C.dydx0 * (x - C.x0); dydx = C.dydx0; }
        if (x > C.x1) { y = C.y1 + C.dydx1 * (x - C.x1); dydx = C.dydx1; }
    }
}

/* root of a*fal*fv(v) + beta*v = rhs (strictly increasing in v), solved in the
 * Bezier parameter of the bracketing segment, warm-started from v0 (the
 * previous substep's root) through the segment's u(x) table; returns v, fv,
 * dfv/dv.  At least two safeguarded Newton steps, then more until
 * converged. */
template <bool BF = true, bool PE = true, typename Real>
DEV void solve_fv(const DCurve<Real> &C, Real afal, Real beta, Real rhs, Real v0, Real &v, Real &fv, Real &dfv) {
    Real g0 = afal * C.y0 + beta * C.x0 - rhs;
    Real g1 = afal * C.y1 + beta * C.x1 - rhs;
    int k = 0;
#pragma unroll
    for (int s = 1; s < BIOIM_MAX_CURVESEG; ++s) k += afal * C.ya[s] + beta * C.xa[s] - rhs <= 0 ? 1 : 0;
    Real px[6], py[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { px[i] = C.cx[k][i]; py[i] = C.cy[k][i]; }
    const Real xa = C.xa[k], xb = C.xb[k];
    Real ga = afal * C.ya[k] + beta * xa - rhs, gb = afal * C.yb[k] + beta * xb - rhs;
    /* both starts computed, one selected (no branch: the table loads and the
     * division stay in the muscle eval's basic block) — the warm start
     * through the segment's u(x) table, or the secant of g over the segment */
    Real u;
    if constexpr (!BF) {
        if (v0 > xa && v0 < xb) {
            Real tt = (v0 - xa) * C.inv_h[k];
            int i0 = (int)tt;
            i0 = i0 < 0 ? 0 : (i0 > BIOIM_UTAB - 1 ? BIOIM_UTAB - 1 : i0);
            Real fr = tt - Real(i0);
            u = C.ut[k][i0] + fr * (C.ut[k][i0 + 1] - C.ut[k][i0]);
        } else {
            u = ga / (ga - gb);
        }
    } else {
        const Real vc = v0 > xa ? (v0 < xb ? v0 : xb) : xa;
        Real tt = (vc - xa) * C.inv_h[k];
        int i0 = (int)tt;
        i0 = i0 < 0 ? 0 : (i0 > BIOIM_UTAB - 1 ? BIOIM_UTAB - 1 : i0);
        Real fr = tt - Real(i0);
        const Real ua = C.ut[k][i0], ub = C.ut[k][i0 + 1];
#if BIOIM_FV_HERMITE
        /* the cubic Hermite start of curve_eval (table slopes mt) */
        const Real ma = C.mt[k][i0], mb = C.mt[k][i0 + 1], dua = ub - ua;
        const Real h2 = Real(3) * dua - Real(2) * ma - mb, h3 = ma + mb - Real(2) * dua;
        const Real ut = fma(fr, fma(fr, fma(fr, h3, h2), ma), ua), us = ga * newton_rcp(ga - gb);
#else
        const Real ut = ua + fr * (ub - ua), us = ga * newton_rcp(ga - gb);
#endif
        u = ((v0 > xa) & (v0 < xb)) ? ut : us;
    }
    const Real half = 0.5;
    u = ((u > Real(0)) & (u < Real(1))) ? u : half;
    /* g(u) = a fal y(u) + beta x(u) - rhs is one quintic in u */
    Real pg[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) pg[i] = afal * py[i] + beta * px[i];
    pg[0] -= rhs;
    Real lo = 0, hi = 1, dprev = 1;
    /* the root lies past an end of the curve (g keeps one sign over it): the
     * result is the linear extrapolation below, whatever the loop finds, so
     * the lane leaves the loop after its first step.  Before round 5 such a
     * lane ran the Newton loop down to the segment's end by bisections (up to
     * ~40 iterations) and its wave — and the launch — waited for it: the
     * raw-action Palsy3D model hit it in 10 % of its waves.
     * PE: the spatial models only (same-box Palsy3D -15 %, C5 -13 %,
     * Running3D -1.5 %; the planar kernels, which rarely meet it, measured
     * +0.5 % with it: profiles/r05/r05k) */
    const bool past_end = PE && BIOIM_FV_PAST_END && ((g0 >= 0) | (g1 <= 0));
    for (int it = 0; it < Eps<Real>::it_max; ++it) {
        Real g = bez5(pg, u);
        if (g > 0) hi = u; else lo = u;
        Real dg = dbez5(pg, u);
        Real un = u - g * newton_rcp(dg);
        /* inclusive bracket: a converged step (un == u == lo or hi after
         * rounding) must not trigger the bisection fallback */
        if (!(un >= lo && un <= hi)) un = Real(0.5) * (lo + hi);
#ifdef BIOIM_WAVETIME
        if (!(u - g * newton_rcp(dg) >= lo && u - g * newton_rcp(dg) <= hi) && diag_tid() < BIOIM_WAVETIME_N * 4) g_fvbis[diag_tid()] += 1;
#endif
        Real du = fabs(un - u);
        u = un;
        /* converged, or stagnating at the rounding level of g */
        if (past_end || (it >= 1 && (du <= Eps<Real>::u_stop || (du <= Real(1e3) * Eps<Real>::u_tol && du >= Real(0.5) * dprev)))) {
#ifdef BIOIM_WAVETIME
            if (diag_tid() < BIOIM_WAVETIME_N * 4) {
                g_fvit[diag_tid()] += it + 1;
                if ((unsigned)(it + 1) > g_fvmax[diag_tid()]) g_fvmax[diag_tid()] = it + 1;
            }
#endif
#ifdef BIOIM_STAMPS
            if (blockIdx.x == 0 && threadIdx.x < 14) atomicAdd(&g_stamps[12], (unsigned long long)(it + 1));
            if (blockIdx.x == 0 && threadIdx.x < 14) atomicAdd(&g_stamps[13], 1ull);
#endif
            break;
        }
#ifdef BIOIM_STAMPS
        if (it == Eps<Real>::it_max - 1 && blockIdx.x == 0 && threadIdx.x < 14) atomicAdd(&g_stamps[14], 1ull);
#endif
        dprev = du;
    }
    v = bez5(px, u);
    fv = bez5(py, u);
    dfv = dbez5(py, u) * fast_rcp(dbez5(px, u));
    if constexpr (!BF) {
        if (g0 >= 0) {
            v = (rhs - afal * (C.y0 - C.dydx0 * C.x0)) / (afal * C.dydx0 + beta);
            fv = C.y0 + C.dydx0 * (v - C.x0); dfv = C.dydx0;
        } else if (g1 <= 0) {
            v = (rhs - afal * (C.y1 - C.dydx1 * C.x1)) / (afal * C.dydx1 + beta);
            fv = C.y1 + C.dydx1 * (v - C.x1); dfv = C.dydx1;
        }
    } else {   /* linear extrapolation past an end (one reciprocal, selected).
                * Reciprocals instead of IEEE divisions here and in the secant
                * start: same-box 2D 0.2772 -> 0.2762 ms, 3D 0.5176 -> 0.5145 ms,
                * C5 unchanged (profiles/r04/r04y; computing this before the
                * Newton loop instead was 2D -0.6 % but C5 +1.2 %) */
        const Real y0 = C.y0, d0 = C.dydx0, x0 = C.x0, y1 = C.y1, d1 = C.dydx1, x1 = C.x1;
        const bool e0 = g0 >= 0, e1 = g1 <= 0;
        const Real yE = e0 ? y0 : y1, dE = e0 ? d0 : d1, xE = e0 ? x0 : x1;
        const Real vE = (rhs - afal * (yE - dE * xE)) * fast_rcp(afal * dE + beta);
        const Real fvE = yE + dE * (vE - xE);
        const bool ext = e0 | e1;
        v = ext ? vE : v; fv = ext ? fvE : fv; dfv = ext ? dE : dfv;
    }
}
