// bioim_math.h — device arithmetic with no knowledge of the model image or the
// LDS layout: compile-time loops, tolerances, 3-vector products (plain and
// zero-masked), lane-group reductions and the wave fence, sin/cos, the
// reciprocals, the tree-sparse LTL solve, the smooth step.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "bioim_config.h"

template <int I, int N, class F>
DEV void sfor(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sfor<I + 1, N>(f);
    }
}

template <typename Real> struct Eps;
template <> struct Eps<float> {
    static constexpr float u_tol = 2e-7f;   /* Bezier parameter tolerance  */
    static constexpr float u_stop = 2e-7f;  /* Newton step after which the root is converged */
    static constexpr float v_tol = 1e-7f;   /* normalized velocity         */
    static constexpr float l_tol = 1e-9f;   /* fiber length (m)            */
    static constexpr float l_stop = 1e-9f;  /* Newton step after which the length is converged */
    static constexpr float h_stop = 0.0f;   /* fiber-equilibrium residual stop (off in fp32) */
    static constexpr int it_max = 24;
    static constexpr int curve_newton = 1; /* from the Hermite start: 5.9e-9 < fp32 rounding */
};
template <> struct Eps<double> {
    static constexpr double u_tol = 1e-15;
    /* a Newton step of at most 1e-11 leaves an error ~ |g''/2g'| 1e-22 in u
     * (quadratic convergence; the smooth curves have |g''/g'| = O(10)) */
    static constexpr double u_stop = 1e-11;
    static constexpr double v_tol = 1e-15;
    static constexpr double l_tol = 1e-15;
    static constexpr double l_stop = 1e-10;
    /* the oracle's residual stop of the reset fiber equilibrium
     * (oracle/bioim_oracle.c muscle_equilibrium, |H| < 1e-12): where the root is
     * ill-conditioned (a tendon at its slack length: H nearly flat in l) the
     * iterate that stop returns is the oracle's, instead of one converged
     * further (round 6: Palsy3D tib_ant_r at reset row 46, 9.2e-12 apart;
     * DESIGN.md 2) */
    static constexpr double h_stop = 1e-12;
    static constexpr int it_max = 60;
    static constexpr int curve_newton = 2; /* from the Hermite start: 8.9e-16 */
};

/* ------------------------------------------------------------- vec3 */
template <typename Real> DEV void cross3(const Real *a, const Real *b, Real *o) {
    Real x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    o[0] = x; o[1] = y; o[2] = z;
}
template <typename Real> DEV Real dot3(const Real *a, const Real *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <typename Real> DEV void mv3(const Real *R, const Real *v, Real *o) {
    Real x = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
    Real y = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
    Real z = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
    o[0] = x; o[1] = y; o[2] = z;
}
template <typename Real> DEV void mm3(const Real *A, const Real *B, Real *C) {
    Real T[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = T[i];
}
/* The same products with compile-time zero masks (bit i: operand entry i
 * is known to be zero): a term with a known-zero factor is left out, so
 * planar models (Planar below) run the 2-D arithmetic through the same
 * code; with empty masks these are exactly mv3 / mm3 / cross3 / dot3
 * (same terms, same order). */
template <unsigned ZA, unsigned ZB, int N, typename Real>
DEV Real sum_m(const Real *a, const Real *b, const int (&ia)[N], const int (&ib)[N], const int (&sg)[N]) {
    Real acc = 0;
    bool first = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (((ZA >> ia[k]) & 1u) || ((ZB >> ib[k]) & 1u)) continue;
        const Real t = a[ia[k]] * b[ib[k]];
        acc = first ? (sg[k] > 0 ? t : -t) : (sg[k] > 0 ? acc + t : acc - t);
        first = false;
    }
    return acc;
}
template <unsigned ZA, unsigned ZB, typename Real> DEV void mv3m(const Real *R, const Real *v, Real *o) {
    Real r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ia[3] = {3 * i, 3 * i + 1, 3 * i + 2}, ib[3] = {0, 1, 2}, sg[3] = {1, 1, 1};
        r[i] = sum_m<ZA, ZB, 3>(R, v, ia, ib, sg);
    }
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}
template <unsigned ZA, unsigned ZB, typename Real> DEV void mm3m(const Real *A, const Real *B, Real *C) {
    Real T[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ia[3] = {3 * i, 3 * i + 1, 3 * i + 2}, ib[3] = {j, 3 + j, 6 + j}, sg[3] = {1, 1, 1};
            T[3 * i + j] = sum_m<ZA, ZB, 3>(A, B, ia, ib, sg);
        }
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = T[i];
}
template <unsigned ZA, unsigned ZB, typename Real> DEV void cross3m(const Real *a, const Real *b, Real *o) {
    const int sg[2] = {1, -1};
    const int ia0[2] = {1, 2}, ib0[2] = {2, 1}, ia1[2] = {2, 0}, ib1[2] = {0, 2}, ia2[2] = {0, 1}, ib2[2] = {1, 0};
    Real x = sum_m<ZA, ZB, 2>(a, b, ia0, ib0, sg), y = sum_m<ZA, ZB, 2>(a, b, ia1, ib1, sg),
         z = sum_m<ZA, ZB, 2>(a, b, ia2, ib2, sg);
    o[0] = x; o[1] = y; o[2] = z;
}
template <unsigned ZA, unsigned ZB, typename Real> DEV Real dot3m(const Real *a, const Real *b) {
    const int ia[3] = {0, 1, 2}, sg[3] = {1, 1, 1};
    return sum_m<ZA, ZB, 3>(a, b, ia, ia, sg);
}

/* Planar topologies (T::PLANAR; the host checks each pack, pack_is_planar):
 * frames rotate about z only, so R13 = R23 = R31 = R32 = 0 and R33 = 1,
 * angular velocities and accelerations lie along z, linear ones in the x-y
 * plane.  These helpers write those zeros over values just read from LDS;
 * in the functions that use them the products with the known zeros then fold
 * away (those functions are compiled without signed zeros / NaN semantics:
 * `#pragma float_control(precise, off)`), so a planar model runs 2-D
 * arithmetic through the same source.  No-ops for spatial topologies. */
template <class T> struct Planar {
    /* zero masks (mv3m / mm3m / cross3m / dot3m): rotation, angular, linear */
    static constexpr unsigned ZR = T::PLANAR ? 0xE4u : 0u, ZW = T::PLANAR ? 0x3u : 0u, ZV = T::PLANAR ? 0x4u : 0u;
    template <typename Real> static DEV void rot(Real *R) {
        if constexpr (T::PLANAR) { R[2] = R[5] = R[6] = R[7] = Real(0); R[8] = Real(1); }
    }
    template <typename Real> static DEV void ang(Real *w) {
        if constexpr (T::PLANAR) { w[0] = w[1] = Real(0); }
    }
    template <typename Real> static DEV void lin(Real *v) {
        if constexpr (T::PLANAR) { v[2] = Real(0); }
    }
    /* frame slot KB: R9 o3 w3 vO3 */
    template <typename Real> static DEV void frame(Real *kb) { rot(kb); ang(kb + 12); lin(kb + 15); }
    /* joint-local slot LOC: R9 p3 wrel3 vrel3 arel3 aa3 */
    template <typename Real> static DEV void loc(Real *lc) { rot(lc); ang(lc + 12); lin(lc + 15); ang(lc + 18); lin(lc + 21); }
    /* acceleration slot AL: alpha3 aO3 */
    template <typename Real> static DEV void acc(Real *ab) { ang(ab); lin(ab + 3); }
    /* Plucker column: Omega3 V3 */
    template <typename Real> static DEV void col(Real *s) { ang(s); lin(s + 3); }
};

DEV void sincos_rt(double x, double &s, double &c);
DEV void sincos_rt(float x, float &s, float &c);
template <typename Real> DEV void axis_rot(const Real *a, Real th, Real *R) {
    Real s, c;
    sincos_rt(th, s, c);
    Real t = Real(1) - c, x = a[0], y = a[1], z = a[2];
    R[0] = t * x * x + c;     R[1] = t * x * y - s * z; R[2] = t * x * z + s * y;
    R[3] = t * x * y + s * z; R[4] = t * y * y + c;     R[5] = t * y * z - s * x;
    R[6] = t * x * z - s * y; R[7] = t * y * z + s * x; R[8] = t * z * z + c;
}

template <int G, typename Real> DEV Real group_sum(Real x) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, G);
    return x;
}
template <int G, typename Real> DEV Real group_max(Real x) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off, G));
    return x;
}
template <int G> DEV bool group_any(bool p) {
    unsigned long long b = __ballot(p);
    int base = (threadIdx.x & 63) & ~(G - 1);
    unsigned long long m = (G == 64) ? ~0ull : ((1ull << G) - 1ull);
    return ((b >> base) & m) != 0ull;
}

template <int G, typename V> DEV V group_min(V x) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) {
        const V y = __shfl_xor(x, off, G);
        x = y < x ? y : x;
    }
    return x;
}

/* sin and cos with one shared range reduction.  fp64: Cody-Waite reduction
 * by pi/2 (three-part constant, exact for |x| < 1e5, far beyond joint
 * angles) and Taylor polynomials on [-pi/4, pi/4] (truncation < 1e-19);
 * agrees with libm to ~1 ulp.  fp32: the device sincosf. */
DEV void sincos_rt(double x, double &s, double &c) {
    const double k = rint(x * 0.63661977236758134308);
    double r = fma(-k, 1.57079632679489655800e+00, x);
    r = fma(-k, 6.12323399573676603587e-17, r);
    r = fma(-k, -1.4973849048591698e-33, r);
    const double r2 = r * r;
    double ps = 2.8114572543455208e-15;                /* 1/17! */
    ps = fma(ps, r2, -7.6471637318198164e-13);         /* -1/15! */
    ps = fma(ps, r2, 1.6059043836821613e-10);          /* 1/13! */
    ps = fma(ps, r2, -2.5052108385441720e-08);         /* -1/11! */
    ps = fma(ps, r2, 2.7557319223985893e-06);          /* 1/9! */
    ps = fma(ps, r2, -1.9841269841269841e-04);         /* -1/7! */
    ps = fma(ps, r2, 8.3333333333333333e-03);          /* 1/5! */
    ps = fma(ps, r2, -1.6666666666666667e-01);         /* -1/3! */
    const double sr = fma(ps * r2, r, r);
    double pc = 1.5619206968586225e-16;                /* 1/18! */
    pc = fma(pc, r2, -4.7794773323873853e-14);         /* -1/16! */
    pc = fma(pc, r2, 1.1470745597729725e-11);          /* 1/14! */
    pc = fma(pc, r2, -2.0876756987868099e-09);         /* -1/12! */
    pc = fma(pc, r2, 2.7557319223985891e-07);          /* 1/10! */
    pc = fma(pc, r2, -2.4801587301587302e-05);         /* -1/8! */
    pc = fma(pc, r2, 1.3888888888888889e-03);          /* 1/6! */
    pc = fma(pc, r2, -4.1666666666666667e-02);         /* -1/4! */
    pc = fma(pc, r2, 0.5);
    const double cr = fma(-pc, r2, 1.0);
    const int q = (int)k & 3;
    const double ss = (q & 1) ? cr : sr, cc = (q & 1) ? sr : cr;
    s = (q & 2) ? -ss : ss;
    c = ((q + 1) & 2) ? -cc : cc;
}
DEV void sincos_rt(float x, float &s, float &c) { sincosf(x, &s, &c); }

#if BIOIM_EXACT_RCP
DEV double newton_rcp(double x) { return 1.0 / x; }
DEV float newton_rcp(float x) { return 1.0f / x; }
DEV double fast_rcp(double x) { return 1.0 / x; }
DEV float fast_rcp(float x) { return 1.0f / x; }
DEV double fast_rsqrt(double x) { return 1.0 / sqrt(x); }
DEV float fast_rsqrt(float x) { return 1.0f / sqrtf(x); }
#else
/* reciprocal for Newton updates (a self-correcting iteration tolerates a
 * last-bits error in the step): hardware rcp plus one refinement */
DEV double newton_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r, 1.0);
    return fma(r, e, r);
}
DEV float newton_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
/* reciprocal to (about) the last bit: hardware rcp plus two refinements —
 * a shorter dependency chain than the IEEE division sequence; used where the
 * divisor is a well-scaled positive quantity (lengths, cosines, time
 * constants, slip speeds) */
DEV double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}
DEV float fast_rcp(float x) {
    float r = __builtin_amdgcn_rcpf(x);
    return fmaf(r, fmaf(-x, r, 1.0f), r);
}
/* 1/sqrt(x) for x > 0: hardware rsq plus two Newton refinements; a length
 * and its inverse then cost one rsq (len = x * rsqrt(x)) instead of an IEEE
 * sqrt and a reciprocal */
DEV double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double hx = 0.5 * x;
    y = fma(y, fma(-hx * y, y, 0.5), y);
    return fma(y, fma(-hx * y, y, 0.5), y);
}
DEV float fast_rsqrt(float x) {
    float y = __builtin_amdgcn_rsqf(x);
    return fmaf(y, fmaf(-0.5f * x * y, y, 0.5f), y);
}
#endif

DEV void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
/* the same fence inside a lane-divergent region: orders this wave's LDS
 * accesses (the active lanes' reads before their writes); lanes of one wave
 * execute in lockstep, so no lane can be behind */
DEV void wave_sync_lanes() { wave_sync(); }

template <int I> DEV constexpr int tri(int k, int l) { return k * (k + 1) / 2 + l; }

/* symmetric 3x3 (xx yy zz xy xz yz) times v, v's known zeros masked (ZB) */
template <unsigned ZB, typename Real> DEV void symvm(const Real *J, const Real *v, Real *o) {
    const int r0[3] = {0, 3, 4}, r1[3] = {3, 1, 5}, r2[3] = {4, 5, 2}, iv[3] = {0, 1, 2}, sg[3] = {1, 1, 1};
    Real x = sum_m<0, ZB, 3>(J, v, r0, iv, sg), y = sum_m<0, ZB, 3>(J, v, r1, iv, sg), z = sum_m<0, ZB, 3>(J, v, r2, iv, sg);
    o[0] = x; o[1] = y; o[2] = z;
}
/* symmetric 3x3 (xx yy zz xy xz yz) times v */
template <typename Real> DEV void symv(const Real *J, const Real *v, Real *o) {
    Real x = J[0] * v[0] + J[3] * v[1] + J[4] * v[2];
    Real y = J[3] * v[0] + J[1] * v[1] + J[5] * v[2];
    Real z = J[4] * v[0] + J[5] * v[1] + J[2] * v[2];
    o[0] = x; o[1] = y; o[2] = z;
}

/* Tree-sparse LTL factorization M = L^T L and solve (Featherstone, Rigid
 * Body Dynamics Algorithms 6.3), unrolled at compile time over the
 * topology's dof tree: entry (k, i) of M is structurally non-zero only when
 * i is k or an ancestor dof of k, and factoring from the leaves up creates
 * no fill-in, so only those entries are touched (2D: 53 of the dense 121
 * multiply-adds, 3D: 257 of 457).  In place on the packed lower M; returns
 * false if not SPD. */
template <class T> struct DofTree {
    /* parent dof: the previous dof of the same body, else the last dof of
     * the nearest ancestor body that has one, else -1 */
    static constexpr int par(int d) {
        for (int e = d - 1; e >= 0; --e)
            if (T::dof_cb[e] == T::dof_cb[d]) return e;
        for (int b = T::parent[T::dof_cb[d]]; b >= 0; b = T::parent[b]) {
            int last = -1;
            for (int e = 0; e < T::ND; ++e)
                if (T::dof_cb[e] == b) last = e;
            if (last >= 0) return last;
        }
        return -1;
    }
    /* i is a proper ancestor dof of k */
    static constexpr bool anc(int k, int i) {
        for (int j = par(k); j >= 0; j = par(j))
            if (j == i) return true;
        return false;
    }
    /* bit l set: l is k or an ancestor dof of k (the structurally non-zero
     * entries (k, l) of row k of M) */
    static constexpr unsigned path_mask(int k) {
        unsigned m = 1u << k;
        for (int j = par(k); j >= 0; j = par(j)) m |= 1u << j;
        return m;
    }
    /* dof 0 is on every dof's root path (phase 3's row stores rely on it) */
    static constexpr bool root_common() {
        for (int k = 0; k < T::ND; ++k)
            if (!(path_mask(k) & 1u)) return false;
        return true;
    }
};

template <class T, int N, typename Real> DEV bool ltl_solve(Real *A, Real *b) {
    using DT = DofTree<T>;
    bool ok = true;
    Real inv[N];
    /* factor: for k = N-1 .. 0 */
    sfor<0, N>([&](auto kk) {
        constexpr int k = N - 1 - decltype(kk)::value;
        Real s = A[tri<0>(k, k)];
        ok = ok && (s > 0);
        const Real sp = s > 0 ? s : Real(1e-30);
        const Real id = fast_rsqrt(sp), d = sp * id;
        inv[k] = id;
        A[tri<0>(k, k)] = d;
        sfor<0, N>([&](auto iI) {
            constexpr int i = decltype(iI)::value;
            if constexpr (DT::anc(k, i)) A[tri<0>(k, i)] *= id;
        });
        sfor<0, N>([&](auto iI) {
            constexpr int i = decltype(iI)::value;
            if constexpr (DT::anc(k, i)) {
                sfor<0, N>([&](auto jI) {
                    constexpr int j = decltype(jI)::value;
                    if constexpr (j == i || DT::anc(i, j)) A[tri<0>(i, j)] -= A[tri<0>(k, i)] * A[tri<0>(k, j)];
                });
            }
        });
    });
    /* L^T y = b, leaves first */
    sfor<0, N>([&](auto ii) {
        constexpr int i = N - 1 - decltype(ii)::value;
        b[i] *= inv[i];
        sfor<0, N>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            if constexpr (DT::anc(i, j)) b[j] -= A[tri<0>(i, j)] * b[i];
        });
    });
    /* L x = y, root first */
    sfor<0, N>([&](auto iI) {
        constexpr int i = decltype(iI)::value;
        sfor<0, N>([&](auto jI) {
            constexpr int j = decltype(jI)::value;
            if constexpr (DT::anc(i, j)) b[i] -= A[tri<0>(i, j)] * b[j];
        });
        b[i] *= inv[i];
    });
    return ok;
}

/* branch-free: the transition polynomial is evaluated everywhere and
 * selected (finite for any x) */
template <bool BF, typename Real> DEV Real smooth_step(Real y0, Real y1, Real x0, Real x1, Real iw, Real x) {
    if constexpr (!BF) {
        if (x <= x0) return y0;
        if (x >= x1) return y1;
    }
    Real t = (x - x0) * iw;   /* iw = 1 / (x1 - x0) */
    const Real v = y0 + (y1 - y0) * t * t * t * (Real(10) + t * (Real(6) * t - Real(15)));
    return x <= x0 ? y0 : (x >= x1 ? y1 : v);
}
template <bool BF, typename Real> DEV Real smooth_step_d(Real y0, Real y1, Real x0, Real x1, Real iw, Real x) {
    if constexpr (!BF) {
        if (x <= x0 || x >= x1) return 0;
    }
    Real t = (x - x0) * iw;
    const Real v = (y1 - y0) * Real(30) * t * t * (Real(1) - t) * (Real(1) - t) * iw, zero = 0;
    return ((x <= x0) | (x >= x1)) ? zero : v;
}
