// em_kn.hip -- the HoNa2020 semi-analytic kilonova of Hotokezaka & Nakar (SimpleKilonovaLightCurveModel("HoNa2020"), nmma/em/model.py:59-66,
// :1303-1322): kernel hona2020_lc and its launcher.  Reference arithmetic: HoNa_lc -> setup_HoNa_params -> temp_photosphere_HoNa
// (nmma/em/lightcurve_generation.py:654-771), scipy's solve_ivp / RK45 (scipy/integrate/_ivp/rk.py, base.py) and CubicSpline
// (scipy/interpolate/_cubic.py), the blackbody magnitudes of :43-58 (em_math.h).  Output: source-frame absolute AB magnitudes
// lc[B][M][NS], the contract of me2017_lc / piro2021_lc.  fp64 without contraction (this unit is built with -ffp-contract=off).
//
// One wavefront per row, four rows per workgroup; the waves share nothing and NO workgroup barrier exists: a wave's step count depends on
// its row.  Each wave owns a slice of LDS and orders its accesses with wave-level fences only.  Each lane holds two of the 99 velocity
// shells, l and l + 64; the upper 29 slots are switched off and contribute exact zeros.
//   phase S  per-row scalars (every lane computes the same values) and per-shell be, dbe, searchsorted index, tau, dM, td in the
//            reference's operation order, np.geomspace reproduced (10^linspace with exact end points); log tau / log be reversed -> LDS.
//   phase I  scipy's RK45 as solve_ivp drives it: y0 = 0, first step 0.05 d, min step 10 ulp(t), the step clipped to the last node, six
//            stages + the FSAL stage, scale = atol + max(|y|, |y_new|) rtol, RMS error norm, accept (< 1) with min(10, 0.9 err^-0.2)
//            capped at 1 after a rejection in the same step, reject with max(0.2, 0.9 err^-0.2).  The heating factor depends on the stage
//            time only: once per stage.  The error norm and, after every accepted step, LL = sum over shells of L(y, t) are reduced in a
//            fixed order -- a lane's upper shell onto its lower one, then an xor butterfly 32, 16, .. 1 -- which leaves the same bits in
//            every lane: accept / reject is wave-uniform.  Lane 0 appends (log t, log LL) to the slice.
//            Termination: the loop counts ATTEMPTS in an integer against MAX_ATTEMPTS; nothing floating-point bounds it.  A row that hits
//            that cap, the node cap KMAX, a step below min step, fewer than two nodes or a non-finite log LL is NaN on every node of every
//            filter (scipy raises, or the reference extrapolates garbage: DEVIATIONS.md).
//   phase P  lane 0 solves CubicSpline's not-a-knot system (two nodes: a line; three: the parabola system) by tridiagonal elimination;
//            then nodes in chunks of 128, two per lane in registers: the PPoly value in the bracketing interval (first / last polynomial
//            extrapolate), be = exp(np.interp(2 log t, log tau reversed, log be reversed)), R = be t c, 1 / T = (sigSB / (lbol / (4 pi R R)))^0.25.
//   phase C  bb_abs_mag per (filter, node); afterwards every (row, filter) counts its positive fluxes from what the lane itself stored and
//            a pair with fewer than two rewrites itself as NaN (flux_to_ABmag).
// A row's bits depend on nothing but its own theta.
#include "em_host.h"

namespace nmma {

namespace kn20 {
constexpr int NSH = 99, NGEOM = 100, WAVES = 4, KMAX = 128, NCH = 128, MAX_ATTEMPTS = 4096;
constexpr int SLICE = 2 * NGEOM + 4 * KMAX;       // doubles per wave: log tau [100] | log be [100] | x [KMAX] | y [KMAX] | s [KMAX] | pivots [KMAX]
constexpr double n_idx = 4.5, rtol = 1e-3, atol = 1e-6, first_step = 5e-2 * 86400.0;
// Dormand-Prince tableau as scipy's doubles
constexpr double C2 = 1.0 / 5, C3 = 3.0 / 10, C4 = 4.0 / 5, C5 = 8.0 / 9;
constexpr double A21 = 1.0 / 5, A31 = 3.0 / 40, A32 = 9.0 / 40, A41 = 44.0 / 45, A42 = -56.0 / 15, A43 = 32.0 / 9;
constexpr double A51 = 19372.0 / 6561, A52 = -25360.0 / 2187, A53 = 64448.0 / 6561, A54 = -212.0 / 729;
constexpr double A61 = 9017.0 / 3168, A62 = -355.0 / 33, A63 = 46732.0 / 5247, A64 = 49.0 / 176, A65 = -5103.0 / 18656;
constexpr double B1 = 35.0 / 384, B3 = 500.0 / 1113, B4 = 125.0 / 192, B5 = -2187.0 / 6784, B6 = 11.0 / 84;
constexpr double E1 = -71.0 / 57600, E3 = 71.0 / 16695, E4 = -71.0 / 1920, E5 = 17253.0 / 339200, E6 = -22.0 / 525, E7 = 1.0 / 40;
}  // namespace kn20

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the two shell values of every lane summed over the wave in a fixed order; the same bits in every lane
__device__ __forceinline__ double shell_sum(double lower, double upper) {
    double v = lower + upper;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// luminosity_HoNa (lightcurve_generation.py:676-684)
__device__ __forceinline__ double kn_lum(double E, double t, double td, double be) {
    const double t_dif = td / t;
    const double tmin = t_dif < t ? t_dif : (t_dif != t_dif ? t_dif : t);      // np.minimum
    const double tesc = tmin + be * t;
    return erfc(sqrt(0.5 * t_dif / t)) * E / tesc;
}

// heating_rate_Korobkin_Rosswog (:367-395) with eth = 0.5
__device__ __forceinline__ double kn_heat(double t) {
    const double time_term = 0.5 - 1.0 / kPi * atan((t - 1.3) / 0.11);
    return 2 * 2e18 * 0.5 * pow(time_term, 1.3);
}

__global__ __launch_bounds__(256) void hona2020_lc(const EmDev* __restrict__ Pp, const double* __restrict__ theta, const long B, const long ld,
                                                   double* lc, int* __restrict__ steps) {
    using namespace me17;
    using namespace kn20;
    const EmDev& P = *Pp;
    __shared__ double slices[WAVES][SLICE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long b = (long)blockIdx.x * WAVES + wave;
    if (b >= B) return;            // (whole waves leave; no barrier follows)
    double* ltau = slices[wave];   // log taus[::-1]
    double* lbes = ltau + NGEOM;   // log bes[::-1]
    double* xs = lbes + NGEOM;     // log t_k of the accepted steps
    double* ys = xs + KMAX;        // log LL_k
    double* sd = ys + KMAX;        // the spline's first derivatives
    double* wk = sd + KMAX;        // pivots of the elimination
    const int NS = P.NS, M = P.M;
    const double* row = theta + b * ld;

    // ---- phase S: setup_HoNa_params and the shell arrays of temp_photosphere_HoNa
    const double mej = pow(10.0, apply_slot(P.model_param[0], row)) * msun;
    const double vmax = apply_slot(P.model_param[1], row), vmin = apply_slot(P.model_param[2], row);
    const double vel1 = apply_slot(P.model_param[3], row) * (vmax - vmin) + vmin;
    const double op0 = pow(10.0, apply_slot(P.model_param[4], row)), op1 = pow(10.0, apply_slot(P.model_param[5], row));
    double z = 0.0;
    if (P.redshift_mode == NMMA_Z_SLOT) z = apply_slot(P.redshift, row);
    else if (P.redshift_mode == NMMA_Z_GRID) {
        const double d_eff = apply_slot(P.lumdist, row) * (P.has_h0 ? apply_slot(P.hubble, row) * P.inv_h0_ref : 1.0);
        z = interp_np(d_eff, P.dist_grid, P.z_grid, P.n_cosmo, P.z_grid[0], P.z_grid[P.n_cosmo - 1]);
        if (P.has_h0) z *= d_eff;
    }
    const double ls = log10(vmin), le = log10(vmax), gstep = (le - ls) / (NGEOM - 1);
    auto geom = [&](int i) -> double {          // np.geomspace(vmin, vmax, 100)[i]
        if (i == 0) return vmin;
        if (i == NGEOM - 1) return vmax;
        return pow(10.0, i * gstep + ls);
    };
    const double bej1 = pow(vel1 / vmin, 1 - n_idx), bej2 = pow(vmax / vmin, 1 - n_idx), bej0 = pow(vmin / vmin, 1 - n_idx);
    const double acc1 = op1 * (bej2 - bej1);
    const double tacc0 = -(acc1 + op0 * (bej1 - bej0)), tacc1 = -acc1;
    const double vej_0 = vmin * c_cgs, v3 = pow(vej_0, 3.0);
    const double rho_0 = mej * (n_idx - 3) / (4 * kPi * v3) / (1 - pow(vmax / vmin, 3 - n_idx));
    const double tscale = vej_0 * rho_0 / (n_idx - 1);
    double dM[2], td[2], be[2];
    bool on[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = lane + 64 * q;
        on[q] = k < NSH;
        dM[q] = 0.0; td[q] = 1.0; be[q] = 1.0;
        if (on[q]) {
            const double bk = vmax + vmin - geom(NGEOM - 1 - k);
            const double nxt = k == NSH - 1 ? vmax : vmax + vmin - geom(NGEOM - 2 - k);
            const double dbe = nxt - bk;
            int i = (vmin < bk ? 1 : 0) + (vel1 < bk ? 1 : 0) + (vmax < bk ? 1 : 0);       // np.searchsorted(velocities, bes), left
            if (i > 2) i = 2;                                                            // (the reference raises an IndexError there)
            const double tau_i = i == 0 ? tacc0 : (i == 1 ? tacc1 : 0.0), bej_i = i == 0 ? bej0 : (i == 1 ? bej1 : bej2);
            const double op_im1 = i == 1 ? op0 : op1;                                    // opacities[i - 1]; i == 0 reads the LAST opacity
            const double qk = bk / vmin;
            const double tau = (tau_i + op_im1 * (pow(qk, 1 - n_idx) - bej_i)) * tscale;
            dM[q] = 4. * kPi * v3 * rho_0 * pow(qk, 2 - n_idx) * dbe / vmin;
            td[q] = tau * bk;
            be[q] = bk;
            ltau[NSH - 1 - k] = log(tau);
            lbes[NSH - 1 - k] = log(bk);
        }
    }

    // ---- phase I: RK45 from the first node to the last
    const double t_bound = P.st[NS - 1] * day;
    double t = P.st[0] * day, h_abs = first_step, min_step = 0.0;
    double y[2] = {0.0, 0.0}, f[2];
    {
        const double hf = kn_heat(t);
#pragma unroll
        for (int q = 0; q < 2; ++q) f[q] = on[q] ? -y[q] / t - kn_lum(y[q], t, td[q], be[q]) + dM[q] * hf : 0.0;
    }
    int accepted = 0, rejected = 0, nk = 0;
    bool in_step = false, step_rejected = false, done = false, bad = false;
    for (int attempt = 0; attempt < MAX_ATTEMPTS; ++attempt) {
        if (!in_step) {
            min_step = 10 * (nextafter(t, dinf()) - t);
            if (h_abs < min_step) h_abs = min_step;
            step_rejected = false;
            in_step = true;
        }
        if (h_abs < min_step) break;            // solve_ivp: "Required step size is less than spacing between numbers."
        double t_new = t + h_abs;
        if (t_new - t_bound > 0) t_new = t_bound;
        const double h = t_new - t;
        h_abs = fabs(h);
        double K[7][2], yn[2];
        const double hf2 = kn_heat(t + C2 * h), hf3 = kn_heat(t + C3 * h), hf4 = kn_heat(t + C4 * h), hf5 = kn_heat(t + C5 * h),
                     hf6 = kn_heat(t + 1.0 * h);
        double e2 = 0.0, e2u = 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            auto rhs = [&](double ts, double E, double hf) -> double {
                return on[q] ? -E / ts - kn_lum(E, ts, td[q], be[q]) + dM[q] * hf : 0.0;
            };
            K[0][q] = f[q];
            K[1][q] = rhs(t + C2 * h, y[q] + (K[0][q] * A21) * h, hf2);
            K[2][q] = rhs(t + C3 * h, y[q] + (K[0][q] * A31 + K[1][q] * A32) * h, hf3);
            K[3][q] = rhs(t + C4 * h, y[q] + (K[0][q] * A41 + K[1][q] * A42 + K[2][q] * A43) * h, hf4);
            K[4][q] = rhs(t + C5 * h, y[q] + (K[0][q] * A51 + K[1][q] * A52 + K[2][q] * A53 + K[3][q] * A54) * h, hf5);
            K[5][q] = rhs(t + 1.0 * h, y[q] + (K[0][q] * A61 + K[1][q] * A62 + K[2][q] * A63 + K[3][q] * A64 + K[4][q] * A65) * h, hf6);
            yn[q] = y[q] + h * (K[0][q] * B1 + K[2][q] * B3 + K[3][q] * B4 + K[4][q] * B5 + K[5][q] * B6);
            K[6][q] = rhs(t + h, yn[q], hf6);
            const double ev = K[0][q] * E1 + K[2][q] * E3 + K[3][q] * E4 + K[4][q] * E5 + K[5][q] * E6 + K[6][q] * E7;
            const double r = ev * h / (atol + fmax(fabs(y[q]), fabs(yn[q])) * rtol);
            if (q == 0) e2 = r * r; else e2u = r * r;
        }
        const double err = sqrt(shell_sum(e2, e2u)) / sqrt((double)NSH);
        const double g = 0.9 * pow(err, -0.2);
        if (err < 1) {
            double factor = err == 0 ? 10.0 : (g < 10 ? g : 10.0);
            if (step_rejected && !(factor < 1)) factor = 1;
            h_abs *= factor;
            t = t_new;
#pragma unroll
            for (int q = 0; q < 2; ++q) { y[q] = yn[q]; f[q] = K[6][q]; }
            ++accepted;
            in_step = false;
            if (nk == KMAX) { bad = true; break; }
            const double ll = log(shell_sum(on[0] ? kn_lum(y[0], t, td[0], be[0]) : 0.0, on[1] ? kn_lum(y[1], t, td[1], be[1]) : 0.0));
            if (!(ll - ll == 0.0)) bad = true;
            if (lane == 0) { xs[nk] = log(t); ys[nk] = ll; }
            ++nk;
            if (t - t_bound >= 0) { done = true; break; }
        } else {
            h_abs *= g > 0.2 ? g : 0.2;
            step_rejected = true;
            ++rejected;
        }
    }
    if (steps != nullptr && lane == 0) { steps[2 * b] = accepted; steps[2 * b + 1] = rejected; }
    if (!done || nk < 2) bad = true;
    if (bad) {
        for (long i = lane; i < (long)M * NS; i += 64) lc[b * M * NS + i] = dnan();
        return;
    }
    wave_lds_sync();

    // ---- phase P: CubicSpline(log t, log LL), not-a-knot, by one lane
    const int n = nk;
    if (lane == 0) {
        auto dx = [&](int i) -> double { return xs[i + 1] - xs[i]; };
        auto slope = [&](int i) -> double { return (ys[i + 1] - ys[i]) / (xs[i + 1] - xs[i]); };
        if (n == 2) {
            sd[0] = slope(0);
            sd[1] = slope(0);
        } else {
            double up0;
            if (n == 3) {
                wk[0] = 1.0; up0 = 1.0; sd[0] = 2 * slope(0);
            } else {
                const double d = xs[2] - xs[0];
                wk[0] = dx(1); up0 = d;
                sd[0] = ((dx(0) + 2 * d) * dx(1) * slope(0) + dx(0) * dx(0) * slope(1)) / d;
            }
            double up_prev = up0;
            for (int i = 1; i < n; ++i) {
                double lo, di, up, bi;
                if (i < n - 1) {
                    lo = dx(i); di = 2 * (dx(i - 1) + dx(i)); up = dx(i - 1);
                    bi = 3 * (dx(i) * slope(i - 1) + dx(i - 1) * slope(i));
                } else if (n == 3) {
                    lo = 1.0; di = 1.0; up = 0.0; bi = 2 * slope(1);
                } else {
                    const double d = xs[n - 1] - xs[n - 3];
                    lo = d; di = dx(n - 3); up = 0.0;
                    bi = (dx(n - 2) * dx(n - 2) * slope(n - 3) + (2 * d + dx(n - 2)) * dx(n - 3) * slope(n - 2)) / d;
                }
                const double w = lo / wk[i - 1];
                wk[i] = di - w * up_prev;
                sd[i] = bi - w * sd[i - 1];
                up_prev = up;
            }
            sd[n - 1] = sd[n - 1] / wk[n - 1];
            for (int i = n - 2; i >= 0; --i) sd[i] = (sd[i] - (i == 0 ? up0 : dx(i - 1)) * sd[i + 1]) / wk[i];
        }
    }
    wave_lds_sync();

    // ---- phases P and C over the nodes, 128 at a time, two per lane
    const double opz = 1 + z;
    for (int j0 = 0; j0 < NS; j0 += NCH) {
        double inv_T[2] = {0.0, 0.0}, R[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = j0 + lane + 64 * q;
            if (j >= NS) continue;
            const double tj = P.st[j] * day, lx = log(tj);
            int lo = 0, hi = n;                       // first node beyond lx
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (xs[mid] <= lx) lo = mid + 1; else hi = mid;
            }
            int i = lo - 1;
            i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
            const double dxi = xs[i + 1] - xs[i], sl = (ys[i + 1] - ys[i]) / (xs[i + 1] - xs[i]);
            const double tt = (sd[i] + sd[i + 1] - 2 * sl) / dxi;
            const double c0 = tt / dxi, c1 = (sl - sd[i]) / dxi - tt, s = lx - xs[i];
            const double lbol = exp(ys[i] + sd[i] * s + c1 * (s * s) + c0 * ((s * s) * s));
            const double bph = exp(interp_np(2 * lx, ltau, lbes, NSH, lbes[0], lbes[NSH - 1]));
            R[q] = bph * tj * c_cgs;
            inv_T[q] = pow(sigSB / (lbol / (4 * kPi * R[q] * R[q])), 0.25);
        }
        for (int m = 0; m < M; ++m) {
            const double nu = P.nu0[m] * opz;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = j0 + lane + 64 * q;
                if (j >= NS) continue;
                double F;
                lc[(b * M + m) * NS + j] = bb_abs_mag(nu, inv_T[q], R[q], F);
            }
        }
    }
    // ---- flux_to_ABmag: fewer than two positive fluxes -> the whole curve is NaN (a positive flux left a magnitude below +inf; every
    //      lane reads back the nodes it stored itself)
    for (int m = 0; m < M; ++m) {
        double* dst = lc + (b * M + m) * NS;
        int cnt = 0;
        for (int j = lane; j < NS; j += 64) cnt += dst[j] < dinf() ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
        if (cnt < 2)
            for (int j = lane; j < NS; j += 64) dst[j] = dnan();
    }
}

int launch_hona2020_lc(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, double* lc, int32_t* steps, hipStream_t s) {
    const int64_t groups = (B + kn20::WAVES - 1) / kn20::WAVES;
    if (groups > 0x7fffffffLL) return fail("nmma_em_model_lightcurves: batch too large");
    hipLaunchKernelGGL(hona2020_lc, dim3((unsigned)groups), dim3(64 * kn20::WAVES), 0, s, h->dev_d, theta, (long)B, (long)ld, lc, steps);
    NM_HIP(hipGetLastError());
    return 0;
}

}  // namespace nmma
