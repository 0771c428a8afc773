// gaussfit.h — the Gaussian-fit decoder's solver, one body for every place its window comes from: the f32 NCHW heat-maps
// (keypoints_gaussfit.hip gaussfit_kernel), NHWC heat-maps in the workspace (gf_nhwc_fit_kernel, seg_hrnet3) and values the VALU
// output layer evaluates again into LDS (head.hip final_gf_finish_kernel).  gaussfit_plane is parametrised by a functor that
// loads window pixel (row, column) of the plane as f32; everything behind the load is the same instructions.
//
//   window   the pixels with |dx| <= 6 and |dy| <= 6 around the integer arg-max, intersected with the plane: at most 169, so at
//            most 3 per lane (pixel j of the row-major window belongs to lane j % 64, slot j / 64); loaded once, widened to
//            f64, kept in registers.  Coordinates are relative to the arg-max: (u, v) in [-6, 6]^2.
//   start    off = window minimum, A = peak - off, centre = the arg-max, a = c = 1/8 (sigma 2), b = 0
//   solver   Levenberg-Marquardt in f64 with the schedule of pnp.py cpnp_m: lambda 1e-3, x 4 on a rejected step, / 3 (floor
//            1e-9) on an accepted one, at most 10 tries per iteration and 50 iterations, stop when the relative cost decrease
//            is below 1e-14 or no try improves.  A Cholesky factorisation that fails is a rejected step.
//   sums     every lane adds its slots in slot order (an empty slot adds 0.0), then a butterfly of __shfl_xor, offsets 32 .. 1:
//            a + b == b + a, so all 64 lanes end with the same bits and every later decision is uniform.  The order is fixed:
//            a plane's result does not depend on its batch.  tests/gaussfit_ref.py restates it in numpy step for step.
//   solve    the damped 7 x 7 system by a fully unrolled Cholesky, every lane the same; arrays are indexed by constants only,
//            so that they stay in registers (build/resource_usage.json: no scratch).
//   COV      gaussfit_plane<true> (the _cov entries; keypoints_gaussfit_cov.hip, head.hip final_gfcov_finish_kernel): behind the
//            fit, the covariance of the fitted centre as curve_fit reports it, s^2 (J^T J)^-1 with s^2 = cost / (n - 7): one
//            more Jacobian pass at the returned parameters (the same slot order and butterfly), the same Cholesky with lambda
//            0, the x0 and y0 columns of the inverse.  gaussfit_plane<false> is the code it was: every addition sits behind
//            if constexpr.  tests/gaussfit_cov_ref.py restates it.
// Contraction is off inside every function body here (the restatement has no fma) and nowhere else: a file that includes this
// header keeps its own setting for its own code, the loading functor included.  No LDS, no barrier.
#pragma once
#include <hip/hip_runtime.h>

namespace esa {

constexpr int GF_R = 6;            // window radius
constexpr int GF_SLOTS = 3;        // ceil(13 * 13 / 64)
constexpr int GF_P = 7;            // parameters: A, x0, y0, a, b, c, off (x0, y0 relative to the arg-max)
constexpr int GF_T = GF_P * (GF_P + 1) / 2;

__host__ __device__ constexpr int gf_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // packed lower triangle, i >= j

__device__ __forceinline__ double gf_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

struct GfWindow {
    double z[GF_SLOTS], u[GF_SLOTS], v[GF_SLOTS];
    bool m[GF_SLOTS];
};

// residual of slot s at parameters p, and the model's exponential and offsets for the Jacobian
__device__ __forceinline__ double gf_residual(const GfWindow& w, int s, const double* p, double& du, double& dv, double& e) {
#pragma clang fp contract(off)
    du = w.u[s] - p[1];
    dv = w.v[s] - p[2];
    const double q = (p[3] * du) * du + ((2.0 * p[4]) * du) * dv + (p[5] * dv) * dv;
    e = exp(-q);
    return (p[6] + p[0] * e) - w.z[s];
}

__device__ __forceinline__ double gf_cost_of(const GfWindow& w, const double* p) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < GF_SLOTS; ++s) {
        double du, dv, e;
        const double r = gf_residual(w, s, p, du, dv, e);
        const double t = w.m[s] ? r * r : 0.0;
        acc = s == 0 ? t : acc + t;
    }
    return gf_wave_sum(acc);
}

// (H + lam * diag(diag(H) + 1e-12)) d = -g by Cholesky; false when a pivot is not positive (NaN included)
__device__ __forceinline__ bool gf_solve_damped(const double* Hm, const double* g, double lam, double* d) {
#pragma clang fp contract(off)
    double L[GF_T];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < GF_P; ++j) {
        double s = Hm[gf_tri(j, j)] + lam * (Hm[gf_tri(j, j)] + 1e-12);
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[gf_tri(j, k)] * L[gf_tri(j, k)];
        ok = ok && s > 0.0;
        const double dj = sqrt(s);
        L[gf_tri(j, j)] = dj;
#pragma unroll
        for (int i = j + 1; i < GF_P; ++i) {
            double t = Hm[gf_tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[gf_tri(i, k)] * L[gf_tri(j, k)];
            L[gf_tri(i, j)] = t / dj;
        }
    }
    double y[GF_P];
#pragma unroll
    for (int i = 0; i < GF_P; ++i) {
        double t = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t = t - L[gf_tri(i, k)] * y[k];
        y[i] = t / L[gf_tri(i, i)];
    }
#pragma unroll
    for (int i = GF_P - 1; i >= 0; --i) {
        double t = y[i];
#pragma unroll
        for (int k = i + 1; k < GF_P; ++k) t = t - L[gf_tri(k, i)] * d[k];
        d[i] = t / L[gf_tri(i, i)];
    }
    return ok;
}

// J^T J of the model at p, lower triangle packed, the sums as the iteration forms them: every lane its slots in slot order, then
// the butterfly.  For the covariance pass only (the iteration keeps its own loop, which also forms the gradient).
__device__ __forceinline__ void gf_normal_matrix(const GfWindow& w, const double* p, double* N) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < GF_SLOTS; ++s) {
        double du, dv, e;
        (void)gf_residual(w, s, p, du, dv, e);
        const double ae = p[0] * e;
        double J[GF_P];
        J[0] = e;
        J[1] = ae * ((2.0 * p[3]) * du + (2.0 * p[4]) * dv);
        J[2] = ae * ((2.0 * p[4]) * du + (2.0 * p[5]) * dv);
        J[3] = -(ae * (du * du));
        J[4] = -(ae * ((2.0 * du) * dv));
        J[5] = -(ae * (dv * dv));
        J[6] = 1.0;
#pragma unroll
        for (int i = 0; i < GF_P; ++i) J[i] = w.m[s] ? J[i] : 0.0;
#pragma unroll
        for (int i = 0; i < GF_P; ++i)
#pragma unroll
            for (int k = 0; k <= i; ++k) {
                const double t = J[i] * J[k];
                N[gf_tri(i, k)] = s == 0 ? t : N[gf_tri(i, k)] + t;
            }
    }
#pragma unroll
    for (int i = 0; i < GF_T; ++i) N[i] = gf_wave_sum(N[i]);
}

// One wave fits one plane.  load(row, column): the plane's value there as f32, called for window pixels only (inside the
// plane).  bi: the plane's arg-max, row * W + column, the same in every lane.  kp[plane] arrives holding the get_final row (x,
// y, peak); an accepted fit replaces x and y.  fit and hess may be null.  Lane 0 stores.
// COV: also cov f64 [planes][3] = s^2 (Ninv[1][1], Ninv[1][2], Ninv[2][2]) in crop px^2, N = J^T J at the returned parameters, s^2
// = cost / (n - 7), and info f64 [planes][3] = -cov^-1 = (-(cyy / det), cxy / det, -(cxx / det)), det = cxx cyy - cxy cxy (either
// may be null).  cov is NaN x 3 for a rejected fit, n <= 7, a pivot that is not positive or a value that is not finite; info
// where cov is, where det is not positive and where cxx < cov_floor.  The status describes the fit alone.
template <bool COV = false, class Load>
__device__ __forceinline__ void gaussfit_plane(Load load, size_t plane, int H, int W, int bi, float* kp, double* fit, int* status,
                                               double* hess, double* cov = nullptr, double* info = nullptr, double cov_floor = 0.0) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    if ((unsigned)bi >= (unsigned)(H * W)) bi = 0;               // never: the arg-max kernels write an index inside the plane
    const int px = bi % W, py = bi / W;
    const int xlo = max(px - GF_R, 0), xhi = min(px + GF_R, W - 1), ylo = max(py - GF_R, 0), yhi = min(py + GF_R, H - 1);
    const int ww = xhi - xlo + 1, npx = ww * (yhi - ylo + 1);

    GfWindow w;
    bool bad = false;
    double lo = __longlong_as_double(0x7ff0000000000000LL);      // +inf
#pragma unroll
    for (int s = 0; s < GF_SLOTS; ++s) {
        const int j = lane + 64 * s;
        w.m[s] = j < npx;
        const int wy = w.m[s] ? j / ww : 0, wx = w.m[s] ? j % ww : 0;
        const float zf = w.m[s] ? load(ylo + wy, xlo + wx) : 0.f;
        w.z[s] = (double)zf;
        w.u[s] = (double)(xlo + wx - px);
        w.v[s] = (double)(ylo + wy - py);
        bad = bad || !isfinite(zf);
        if (w.m[s] && w.z[s] < lo) lo = w.z[s];
    }
    bad = __any(bad);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(lo, off);
        lo = o < lo ? o : lo;
    }
    const double peak = (double)load(py, px);

    double p[GF_P] = {peak - lo, 0.0, 0.0, 0.125, 0.0, 0.125, lo};
    double cost = 0.0;
    if (!bad) {
        cost = gf_cost_of(w, p);
        double lam = 1e-3;
#pragma unroll 1
        for (int it = 0; it < 50; ++it) {
            double Hm[GF_T], g[GF_P];
#pragma unroll
            for (int s = 0; s < GF_SLOTS; ++s) {
                double du, dv, e;
                const double r0 = gf_residual(w, s, p, du, dv, e);
                const double ae = p[0] * e;
                double J[GF_P];
                J[0] = e;
                J[1] = ae * ((2.0 * p[3]) * du + (2.0 * p[4]) * dv);
                J[2] = ae * ((2.0 * p[4]) * du + (2.0 * p[5]) * dv);
                J[3] = -(ae * (du * du));
                J[4] = -(ae * ((2.0 * du) * dv));
                J[5] = -(ae * (dv * dv));
                J[6] = 1.0;
                const double r = w.m[s] ? r0 : 0.0;
#pragma unroll
                for (int i = 0; i < GF_P; ++i) J[i] = w.m[s] ? J[i] : 0.0;       // an empty slot adds 0.0 to every sum
#pragma unroll
                for (int i = 0; i < GF_P; ++i) {
#pragma unroll
                    for (int k = 0; k <= i; ++k) {
                        const double t = J[i] * J[k];
                        Hm[gf_tri(i, k)] = s == 0 ? t : Hm[gf_tri(i, k)] + t;
                    }
                    const double t = J[i] * r;
                    g[i] = s == 0 ? t : g[i] + t;
                }
            }
#pragma unroll
            for (int i = 0; i < GF_T; ++i) Hm[i] = gf_wave_sum(Hm[i]);
#pragma unroll
            for (int i = 0; i < GF_P; ++i) g[i] = gf_wave_sum(g[i]);

            bool improved = false, done = false;
#pragma unroll 1
            for (int t = 0; t < 10 && !improved; ++t) {
                double d[GF_P], pn[GF_P];
                const bool ok = gf_solve_damped(Hm, g, lam, d);
#pragma unroll
                for (int i = 0; i < GF_P; ++i) pn[i] = p[i] + d[i];
                const double cn = ok ? gf_cost_of(w, pn) : cost;
                if (ok && isfinite(cn) && cn < cost) {
#pragma unroll
                    for (int i = 0; i < GF_P; ++i) p[i] = pn[i];
                    const double l3 = lam / 3.0;
                    lam = l3 > 1e-9 ? l3 : 1e-9;
                    improved = true;
                    done = cost - cn < 1e-14 * (cost > 1e-30 ? cost : 1e-30);
                    cost = cn;
                } else {
                    lam = lam * 4.0;
                }
            }
            if (!improved || done) break;
        }
    }

    // the x0 and y0 columns of (J^T J)^-1 at the solution: N d = e1 and N d = e2 through the iteration's solver, undamped
    double c1[GF_P], c2[GF_P];
    bool cov_ok = false;
    if constexpr (COV) {
        if (!bad) {
            double N[GF_T];
            gf_normal_matrix(w, p, N);
            const double g1[GF_P] = {-0.0, -1.0, -0.0, -0.0, -0.0, -0.0, -0.0}, g2[GF_P] = {-0.0, -0.0, -1.0, -0.0, -0.0, -0.0, -0.0};
            const bool ok1 = gf_solve_damped(N, g1, 0.0, c1);
            const bool ok2 = gf_solve_damped(N, g2, 0.0, c2);
            cov_ok = ok1 && ok2;
        }
    }

    if (lane == 0) {
        int st;
        if (bad) {
            st = 3;
        } else {
            bool fin = isfinite(cost);
#pragma unroll
            for (int i = 0; i < GF_P; ++i) fin = fin && isfinite(p[i]);
            const bool inside = p[1] >= (double)(xlo - px) && p[1] <= (double)(xhi - px) && p[2] >= (double)(ylo - py) &&
                                p[2] <= (double)(yhi - py);
            st = !fin ? 1 : (p[0] > 0.0 && p[3] > 0.0 && p[3] * p[5] - p[4] * p[4] > 0.0 && inside) ? 0 : 2;
        }
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const double cx = (double)px + p[1], cy = (double)py + p[2];
        if (st == 0) {
            kp[plane * 3 + 0] = (float)cx;
            kp[plane * 3 + 1] = (float)cy;
        }
        if (fit) {
            double* f = fit + plane * 8;
            f[0] = st ? nan : p[0];
            f[1] = st ? nan : cx;
            f[2] = st ? nan : cy;
            f[3] = st ? nan : p[3];
            f[4] = st ? nan : p[4];
            f[5] = st ? nan : p[5];
            f[6] = st ? nan : p[6];
            f[7] = st ? nan : cost;
        }
        if (hess) {
            double* h3 = hess + plane * 3;
            h3[0] = st ? nan : -2.0 * p[3];
            h3[1] = st ? nan : -2.0 * p[4];
            h3[2] = st ? nan : -2.0 * p[5];
        }
        status[plane] = st;
        if constexpr (COV) {
            const int dof = npx - GF_P;
            double cxx = nan, cxy = nan, cyy = nan;
            if (st == 0 && cov_ok && dof > 0) {
                const double s2 = cost / (double)dof;
                cxx = s2 * c1[1];
                cxy = s2 * c1[2];
                cyy = s2 * c2[2];
                if (!(isfinite(cxx) && isfinite(cxy) && isfinite(cyy))) cxx = cxy = cyy = nan;
            }
            if (cov) {
                double* c3 = cov + plane * 3;
                c3[0] = cxx;
                c3[1] = cxy;
                c3[2] = cyy;
            }
            if (info) {
                const double det = cxx * cyy - cxy * cxy;
                const bool keep = det > 0.0 && !(cxx < cov_floor);       // NaN cov: det is NaN
                double* i3 = info + plane * 3;
                i3[0] = keep ? -(cyy / det) : nan;
                i3[1] = keep ? cxy / det : nan;
                i3[2] = keep ? -(cxx / det) : nan;
            }
        }
    }
}

}  // namespace esa
