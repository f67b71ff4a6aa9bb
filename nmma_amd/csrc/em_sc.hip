// em_sc.hip -- the Piro2021 shock-cooling model (ShockCoolingLightCurveModel, nmma/em/model.py:1230-1277): kernel piro2021_lc and its
// launcher.  Reference arithmetic: sc_bol_lc / sc_lc (nmma/em/lightcurve_generation.py:314-363), the blackbody magnitudes of :43-58 and
// flux_to_ABmag (nmma/em/utils.py:793-811).  Output: source-frame absolute AB magnitudes lc[B][M][NS], the contract of me2017_lc.
//
// The arithmetic, fp64 without contraction (this unit is built with -ffp-contract=off), in the reference's operation order, with
// n = 10, delta = 1.1, kappa = 0.2 and K = (n - 3)(3 - delta) / (4 pi (n - delta)):
//     Me = 10^log10_Menv msun,  Renv = 10^log10_Renv,  Ee = 10^log10_Ee
//     vt  = sqrt((n - 5)(5 - delta) / ((n - 3)(3 - delta)) (2 Ee / Me))          td = sqrt(3 kappa K Me / ((n - 1) vt c))
//     tph = sqrt(3 kappa K Me / (2 (n - 1) vt vt))                               prefactor = pi (n - 1) / (3 (n - 5)) c Renv vt vt / kappa
//     L = t < td  ? prefactor (td / t)^(4 / (n - 2))  : prefactor exp(-0.5 (t t / td / td - 1))                      (0 for a NaN td)
//     R = t < tph ? (tph / t)^(2 / (n - 1)) vt t      : (1 + (delta - 1) / (n - 1) ((t / tph)^2 - 1))^(-1 / (delta - 1)) vt t
//     T = (L / (4 pi R R) / sigSB)^0.25,  T == 0 -> NaN,  1 / T non-finite -> +inf
//     x = min(h nu (1 / T) / kb, 700),  nu = nu0 (1 + z);  F = 2 h / c^2 nu^3 / expm1(x) R R / D^2;  mag = F > 0 ? -2.5 log10 F - 48.6 : +inf
//     a (row, filter) with fewer than two positive F is NaN on every node.
// The model is closed form per node -- no sequential loop as in me2017_lc -- so the work is balanced over items, not rows:
//   one 256-thread workgroup owns a tile of TR rows (8; fewer where the node arrays of a long grid need the LDS);
//   phase A: one lane per row runs the scalar chain (three powers of ten, three square roots, the redshift) into LDS;
//   phase B: (row, node) items strided over all 256 threads: L, R, T -> 1 / T and R per node into LDS (two powers and an exp or a power each);
//   phase C: (row, filter, node) items, node fastest, strided over all 256 threads: with NS nodes in LDS the items of a tile are one
//            contiguous run of lc, so a wave stores 64 consecutive doubles; expm1 and log10 per item.  Positive fluxes are counted per
//            (row, filter) in integer LDS counters (one ballot per wave, one atomic per wave and pair); after a barrier only the pairs
//            with fewer than two overwrite their NS values with NaN -- every other pair pays one store pass and F is never staged.
//   A grid too long for LDS even at one row per tile is walked in chunks of NCH nodes (phases B and C per chunk; the counters span them).
// No operation crosses rows except the integer counters: a row's bits depend on nothing but its own theta.
#include "em_host.h"

namespace nmma {

namespace sc21 {
constexpr double n = 10, delta = 1.1, kappa = 0.2;
constexpr double K = (n - 3) * (3 - delta) / (4 * kPi * (n - delta));       // (0.119 in the paper; the reference keeps the formula)
constexpr double e_L = 4 / (n - 2), e_R = 2 / (n - 1), c_late = (delta - 1) / (n - 1), e_late = -1 / (delta - 1);
constexpr int NSCAL = 6;          // per-row scalars in LDS: vt, td, tph, prefactor, 1 + z, (pad)
constexpr int LDS_BUDGET = 64 * 1024;
}  // namespace sc21

// LDS (bytes) of a tile of TR rows with NCH nodes resident: [scalars TR x NSCAL f64 | 1 / T  TR x NCH f64 | R  TR x NCH f64 | counters TR x M i32]
static inline long sc_lds_bytes(int TR, int NCH, int M) { return (long)TR * (sc21::NSCAL * 8 + 16L * NCH + 4L * M); }

// PROBE: 0 the model; 1 / 2 measurement forms of phase C (nmma_em_set_option "sc_probe"): without its stores / without its transcendentals
template <int PROBE>
__global__ __launch_bounds__(256) void piro2021_lc(const EmDev* __restrict__ Pp, const double* __restrict__ theta, const long B, const long ld,
                                                   const int TR, const int NCH, double* __restrict__ lc) {
    using namespace me17;
    using namespace sc21;
    const EmDev& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* scal = reinterpret_cast<double*>(smem);      // [TR][NSCAL]
    double* inv_t = scal + TR * NSCAL;                   // [TR][NCH]  1 / T
    double* rph = inv_t + TR * NCH;                      // [TR][NCH]  photosphere radius
    int* npos = reinterpret_cast<int*>(rph + TR * NCH);  // [TR][M]    positive fluxes of (row, filter)
    const int tid = threadIdx.x, lane = tid & 63;
    const int NS = P.NS, M = P.M;
    const long b0 = (long)blockIdx.x * TR;
    const int rows = (int)(B - b0 < TR ? B - b0 : TR);

    // ---- phase A: per-row scalars
    for (int i = tid; i < rows * M; i += 256) npos[i] = 0;
    if (tid < rows) {
        const double* row = theta + (b0 + tid) * ld;
        const double Me = pow(10.0, apply_slot(P.model_param[0], row)) * msun;
        const double Renv = pow(10.0, apply_slot(P.model_param[1], row));
        const double Ee = pow(10.0, apply_slot(P.model_param[2], row));
        const double vt = sqrt(((n - 5) * (5 - delta) / ((n - 3) * (3 - delta))) * (2 * Ee / Me));
        const double td = sqrt((3 * kappa * K * Me) / ((n - 1) * vt * c_cgs));
        const double pref = kPi * (n - 1) / (3 * (n - 5)) * c_cgs * Renv * vt * vt / kappa;
        const double tph = sqrt(3 * kappa * K * Me / (2 * (n - 1) * vt * vt));
        double z = 0.0;
        if (P.redshift_mode == NMMA_Z_SLOT) z = apply_slot(P.redshift, row);
        else if (P.redshift_mode == NMMA_Z_GRID) {
            const double d_eff = apply_slot(P.lumdist, row) * (P.has_h0 ? apply_slot(P.hubble, row) * P.inv_h0_ref : 1.0);
            z = interp_np(d_eff, P.dist_grid, P.z_grid, P.n_cosmo, P.z_grid[0], P.z_grid[P.n_cosmo - 1]);
            if (P.has_h0) z *= d_eff;
        }
        double* s = scal + tid * NSCAL;
        s[0] = vt; s[1] = td; s[2] = tph; s[3] = pref; s[4] = 1 + z;
    }

    for (int j0 = 0; j0 < NS; j0 += NCH) {
        const int nch = NS - j0 < NCH ? NS - j0 : NCH;
        __syncthreads();        // the scalars are written; the previous chunk's node arrays are read
        // ---- phase B: photosphere per (row, node)
        for (int i = tid; i < rows * nch; i += 256) {
            const int r = i / nch, jj = i - r * nch;
            const double* s = scal + r * NSCAL;
            const double vt = s[0], td = s[1], tph = s[2], pref = s[3];
            const double t = P.st[j0 + jj] * day;
            double L = 0.0, R = 0.0;          // (np.zeros_like: what a NaN td / tph leaves behind)
            if (t < td) L = pref * pow(td / t, e_L);
            else if (t >= td) L = pref * exp(-0.5 * (t * t / td / td - 1));
            if (t < tph) R = pow(tph / t, e_R) * vt * t;
            else if (t >= tph) { const double q = t / tph; R = pow(1 + c_late * (q * q - 1), e_late) * vt * t; }
            const double sigmaT4 = L / (4 * kPi * R * R);
            double T = pow(sigmaT4 / sigSB, 0.25);
            if (T == 0.0) T = dnan();
            double inv = 1.0 / T;
            if (!(inv - inv == 0.0)) inv = dinf();
            inv_t[r * NCH + jj] = inv;
            rph[r * NCH + jj] = R;
        }
        __syncthreads();
        // ---- phase C: magnitudes per (row, filter, node), node fastest
        const int items = rows * M * nch;
        for (int i = tid; i < items; i += 256) {
            const int rf = i / nch, jj = i - rf * nch;
            const int r = rf / M, f = rf - r * M;
            const double nu = P.nu0[f] * scal[r * NSCAL + 4];
            const double R = rph[r * NCH + jj];
            double F, mag;
            if (PROBE == 2) {
                F = bb_exponent(nu, inv_t[r * NCH + jj]) * R;
                mag = F;
            } else mag = bb_abs_mag(nu, inv_t[r * NCH + jj], R, F);
            const bool pos = F > 0;
            if (PROBE != 1 || mag == 12345.678) lc[((b0 + r) * M + f) * NS + j0 + jj] = mag;
            // count the positive fluxes: the wave's lanes mostly share one (row, filter) -- one atomic for them, one each for the rest
            const int rf0 = __builtin_amdgcn_readfirstlane(rf);
            const unsigned long long active = __ballot(1), same = __ballot(pos && rf == rf0);
            if (pos && rf != rf0) atomicAdd(&npos[rf], 1);
            if (same != 0 && lane == __ffsll((long long)active) - 1) atomicAdd(&npos[rf0], __popcll(same));
        }
    }
    __syncthreads();
    // ---- flux_to_ABmag: fewer than two positive fluxes -> the whole curve is NaN
    for (int rf = 0; rf < rows * M; ++rf) {
        if (npos[rf] >= 2) continue;
        double* dst = lc + (b0 * M + rf) * NS;
        for (int j = tid; j < NS; j += 256) dst[j] = dnan();
    }
}

int launch_piro2021_lc(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, double* lc, hipStream_t s) {
    const EmDev& P = h->dev;
    // rows per tile: 8 (measured: profiles/piro2021.md), halved while the node arrays of the whole grid do not fit the LDS budget;
    // at one row per tile the grid is walked in chunks
    int TR = h->sc_tile > 0 ? h->sc_tile : 8, NCH = P.NS;
    while (TR > 1 && sc_lds_bytes(TR, NCH, P.M) > sc21::LDS_BUDGET) TR /= 2;
    if (sc_lds_bytes(TR, NCH, P.M) > sc21::LDS_BUDGET) NCH = (int)((sc21::LDS_BUDGET - sc_lds_bytes(1, 0, P.M)) / 16);
    if (NCH < 1) return fail("nmma_em_model_lightcurves: too many model filters for the Piro2021 kernel's LDS counters");
    const int64_t tiles = (B + TR - 1) / TR;
    if (tiles > 0x7fffffffLL) return fail("nmma_em_model_lightcurves: batch too large");
    const unsigned lds = (unsigned)sc_lds_bytes(TR, NCH, P.M);
    const dim3 grid((unsigned)tiles), block(256);
    if (h->sc_probe == 1) hipLaunchKernelGGL(piro2021_lc<1>, grid, block, lds, s, h->dev_d, theta, (long)B, (long)ld, TR, NCH, lc);
    else if (h->sc_probe == 2) hipLaunchKernelGGL(piro2021_lc<2>, grid, block, lds, s, h->dev_d, theta, (long)B, (long)ld, TR, NCH, lc);
    else hipLaunchKernelGGL(piro2021_lc<0>, grid, block, lds, s, h->dev_d, theta, (long)B, (long)ld, TR, NCH, lc);
    NM_HIP(hipGetLastError());
    return 0;
}

}  // namespace nmma
