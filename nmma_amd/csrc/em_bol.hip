// em_bol.hip -- bolometric light curves: the Arnett models of SimpleBolometricLightCurveModel (nmma/em/model.py:494-532, arnett_lc /
// arnett_modified_lc, lightcurve_generation.py:65-138) and BasicEMTransient's likelihood (em_likelihood.py:136-263) in ONE kernel,
// bol_logl, with its handle and the nmma_bol_* entry points.  fp64 without contraction (this unit is built with -ffp-contract=off).
//
// The curve.  x = t / tau_m, qA = tau_m / (2 tau_ni), qB = tau_m / (2 tau_co) (the reference's y and y - s), and for q in {qA, qB}
//     S_j(q) = exp(-x_j^2) int_0^{x_j} 2 z exp(z^2 - 2 q z) dz            (the reference: np.exp(-x**2) * quad(...), which overflows for x^2 > 709)
// obeys S_j = a_j S_{j-1} + b_j with a_j = exp(x_{j-1}^2 - x_j^2) and b_j = int_{x_{j-1}}^{x_j} 2 z exp(z^2 - x_j^2 - 2 q z) dz, x_{-1} = 0:
// every exponent is <= 0 and every term is >= 0.  With d = x_j - z the exponent is -(d (x_j + z)) - (2 q) z: two non-positive terms, no
// cancellation.  b_j is a 16-point Gauss-Legendre rule on P equal panels of the interval, P = ceil(max(len / 1, len max(x_j, qA) / 4)):
// on a panel of width w <= 1 centred at c with w |c - q| <= 4 the rule's relative truncation error is <= 1.2e-17.
// Where the integrand has died long before the interval's lower end (qA <= x_j / 4 and d0 = 46 / (x_j - 2 qA) <= x_j / 2) only
// [x_j - d0, x_j] is integrated: the part left out is <= 9e-20 of b_j, and P <= 23 however small tau_m is.  Panel sums are compensated.
//     Lbol_j = Mni ((eps_ni - eps_co) S_j(qA) + eps_co S_j(qB)),  Mni = 10^log10_mni msun;   Arnett_modified: times -expm1(-(t_0 / t_j)^2)
//
// Work split: one wavefront per row of theta, up to four rows per workgroup (fewer where a long grid needs the LDS).  No operation
// crosses waves after the z(d_L) grid is staged, so a row's bits depend on its own theta alone.
//   phase A, lane = node interval, 64 nodes per chunk: (a_j, bA_j, bB_j) per lane, then an inclusive wave scan of the affine maps
//            S -> a S + b (six __shfl_up steps, fixed order) and the carry S_63 of the previous chunk from lane 63.  A supplied curve
//            (nmma_bol_loglike_lc) is loaded instead.  The detector-frame value Lbol / (1 + z)^2 and the observed time
//            t (1 + z) + timeshift of every FINITE node are compacted into the row's LDS arrays (ballot + prefix popcount).
//   phase B, lane = datum, strided over the N epochs: np.interp's formula between the finite nodes, the first / last two of them
//            outside (utils.autocomplete_data, extrapolate = "linear"), detection_term / upper_limit_term of em_math.h, per-lane sums
//            in epoch order, then a five-step xor butterfly.  A NaN sum or fewer than two finite nodes: NMMA_LOGL_FLOOR.
#include "em_host.h"
#include "em_math.h"

namespace nmma {

namespace bol {
constexpr double eps_ni = 3.9e10, eps_co = 6.78e9, tau_ni = 8.8, tau_co = 111.3;     // lightcurve_generation.py:85-88
constexpr double W_MAX = 1.0, K_MAX = 4.0, CUT = 46.0;                               // the panel rule
constexpr double P_LIMIT = 1048576.0;                                                 // panels per interval beyond which the node is NaN (non-finite input)
constexpr int LDS_BUDGET = 64 * 1024;
// 16-point Gauss-Legendre on [0, 1]
__constant__ const double gl_u[16] = {0.005299532504175031, 0.0277124884633837, 0.06718439880608412, 0.1222977958224985, 0.19106187779867811,
                                      0.2709916111713863, 0.35919822461037054, 0.4524937450811813, 0.5475062549188188, 0.6408017753896295,
                                      0.7290083888286136, 0.8089381222013219, 0.8777022041775016, 0.9328156011939159, 0.9722875115366163,
                                      0.994700467495825};
__constant__ const double gl_w[16] = {0.013576229705877019, 0.031126761969323853, 0.047579255841246296, 0.062314485627767015,
                                      0.07479799440828838, 0.08457825969750131, 0.0913017075224618, 0.09472530522753429, 0.09472530522753429,
                                      0.0913017075224618, 0.08457825969750131, 0.07479799440828838, 0.062314485627767015, 0.047579255841246296,
                                      0.031126761969323853, 0.013576229705877019};
}  // namespace bol

struct BolDev {
    int kind, NS, N, n_cosmo, redshift_mode;
    const double *st, *dt, *dv, *ds, *dist_grid, *z_grid;
    nmma_slot tau_m, log10_mni, t_0, timeshift, redshift, lumdist, syserr;
};

// LDS (bytes): [dist_grid | z_grid, n_cosmo f64 each][per row: detector-frame values NS f64 | observed times NS f64]
static inline long bol_lds_bytes(int rows, int NS, int n_cosmo) { return 16L * n_cosmo + (long)rows * 16L * NS; }

// (sum, carry) += v, compensated (Kahan): the sum of the 16 P non-negative terms of an interval carries 2 eps whatever P is
__device__ __forceinline__ void kahan_add(double& sum, double& comp, const double v) {
    const double y = v - comp, t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

// b_j(qA), b_j(qB) of the interval [xp, xj] (see the head of the file); NaN for a non-finite or non-positive tau_m
__device__ __forceinline__ void arnett_interval(const double xp, const double xj, const double qA, const double qB, double& bA, double& bB) {
    using namespace bol;
    double len = xj - xp;
    if (qA <= 0.25 * xj) {
        const double d0 = CUT / (xj - 2.0 * qA);
        if (d0 <= 0.5 * xj && d0 < len) len = d0;
    }
    const double pd = ceil(fmax(len / W_MAX, len * fmax(xj, qA) / K_MAX));
    if (!(pd <= P_LIMIT) || !(qB > 0.0)) { bA = bB = dnan(); return; }
    const int P = pd < 1.0 ? 1 : (int)pd;
    const double w = len / P, two_qA = 2.0 * qA, two_qB = 2.0 * qB;
    double sA = 0.0, cA = 0.0, sB = 0.0, cB = 0.0;
    for (int p = 0; p < P; ++p) {
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const double d = w * (p + gl_u[k]), z = xj - d;
            const double e0 = -(d * (xj + z)), wz = gl_w[k] * z;
            kahan_add(sA, cA, wz * exp(e0 - two_qA * z));
            kahan_add(sB, cB, wz * exp(e0 - two_qB * z));
        }
    }
    bA = 2.0 * w * sA;
    bB = 2.0 * w * sB;
}

// GEN: 0 a supplied curve, 1 Arnett, 2 Arnett_modified.
// MODE: 0 log L; 1 the detector-frame curves (tobs, lbol); 2 the source-frame curve; 3 log L's measurement form without phase B
template <int GEN, int MODE>
__global__ __launch_bounds__(256) void bol_logl(const BolDev P, const double* __restrict__ theta, const long B, const long ld,
                                                const double* __restrict__ lbol_in, double* __restrict__ logl, double* __restrict__ tobs_out,
                                                double* __restrict__ lbol_out) {
    using namespace bol;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* dg = reinterpret_cast<double*>(smem);        // [n_cosmo]
    double* zg = dg + P.n_cosmo;                         // [n_cosmo]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rows_per_wg = blockDim.x >> 6;
    const int NS = P.NS;
    double* cv = zg + P.n_cosmo + (long)wave * 2 * NS;   // [NS] detector-frame values of the finite nodes
    double* ct = cv + NS;                                // [NS] their observed times
    for (int i = tid; i < P.n_cosmo; i += blockDim.x) { dg[i] = P.dist_grid[i]; zg[i] = P.z_grid[i]; }
    __syncthreads();
    const long b = (long)blockIdx.x * rows_per_wg + wave;
    if (b >= B) return;                                  // (whole waves; no barrier follows)
    const double* row = theta + b * ld;

    // ---- per-row scalars, every lane for itself (wave-uniform)
    double z = 0.0;
    if (P.redshift_mode == NMMA_Z_SLOT) z = apply_slot(P.redshift, row);
    else if (P.redshift_mode == NMMA_Z_GRID) z = interp_np(apply_slot(P.lumdist, row), dg, zg, P.n_cosmo, zg[0], zg[P.n_cosmo - 1]);
    const double zp1 = 1 + z, zp1sq = zp1 * zp1, tshift = apply_slot(P.timeshift, row);
    double tau_m = 1.0, qA = 0.0, qB = 0.0, cAm = 0.0, cBm = 0.0, t0 = 0.0;
    if (GEN != 0) {
        tau_m = apply_slot(P.tau_m, row);
        if (!(tau_m > 0.0)) tau_m = dnan();
        const double Mni = pow(10.0, apply_slot(P.log10_mni, row)) * me17::msun;
        qA = tau_m / (2 * tau_ni);
        qB = tau_m / (2 * tau_co);
        cAm = Mni * (eps_ni - eps_co);
        cBm = Mni * eps_co;
        if (GEN == 2) t0 = apply_slot(P.t_0, row);
    }

    // ---- phase A: the curve, 64 nodes per chunk
    double carryA = 0.0, carryB = 0.0;
    int nfin = 0;
    for (int j0 = 0; j0 < NS; j0 += 64) {
        const int j = j0 + lane;
        const bool live = j < NS;
        const double t = live ? P.st[j] : 0.0;
        double L;                                        // source frame
        if (GEN != 0) {
            double a = 1.0, bA = 0.0, bB = 0.0;          // (a lane past the grid: the identity map)
            if (live) {
                const double xj = t / tau_m, xp = j > 0 ? P.st[j - 1] / tau_m : 0.0;
                a = exp((xp - xj) * (xp + xj));
                arnett_interval(xp, xj, qA, qB, bA, bB);
            }
            // inclusive scan of S -> a S + b over the wave: after the step of offset o a lane holds the composition of the 2 o maps ending at it
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double pa = __shfl_up(a, o), pbA = __shfl_up(bA, o), pbB = __shfl_up(bB, o);
                if (lane >= o) { bA = a * pbA + bA; bB = a * pbB + bB; a = a * pa; }
            }
            const double SA = a * carryA + bA, SB = a * carryB + bB;
            carryA = __shfl(SA, 63);
            carryB = __shfl(SB, 63);
            L = cAm * SA + cBm * SB;
            if (GEN == 2) { const double r = t0 / t; L = L * -expm1(-(r * r)); }
        } else {
            L = live ? lbol_in[b * NS + j] : 0.0;
        }
        const double tobs = t * zp1 + tshift, Ldet = L / zp1sq;
        if (MODE == 1 && live) { tobs_out[b * NS + j] = tobs; lbol_out[b * NS + j] = Ldet; }
        if (MODE == 2 && live) lbol_out[b * NS + j] = L;
        if (MODE == 0 || MODE == 3) {
            const bool fin = live && (Ldet - Ldet == 0.0);
            const unsigned long long m = __ballot(fin);
            if (fin) {
                const int pos = nfin + __popcll(m & ((1ull << lane) - 1ull));
                cv[pos] = Ldet;
                ct[pos] = tobs;
            }
            nfin += __popcll(m);
        }
    }
    if (MODE == 1 || MODE == 2) return;
    if (MODE == 3) {                                     // measurement: phase A and its LDS traffic, no likelihood
        if (lane == 0) logl[b] = nfin >= 2 ? cv[nfin - 1] + ct[0] : NMMA_LOGL_FLOOR;
        return;
    }

    // ---- phase B: the likelihood, lane = datum
    if (nfin < 2) {                                      // autocomplete_data: +inf everywhere -> a NaN chi-square -> nan_to_num(-inf)
        if (lane == 0) logl[b] = NMMA_LOGL_FLOOR;
        return;
    }
    const double err = apply_slot(P.syserr, row);
    const double x0 = ct[0], x1 = ct[1], xm = ct[nfin - 2], xn = ct[nfin - 1];
    const double y0 = cv[0], y1 = cv[1], ym = cv[nfin - 2], yn = cv[nfin - 1];
    double chi = 0.0, ul = 0.0;
    for (int i = lane; i < P.N; i += 64) {
        const double td = P.dt[i], m = P.dv[i], unc = P.ds[i];
        double est;
        if (td < x0) est = y0 + (y1 - y0) / (x1 - x0) * (td - x0);
        else if (td > xn) est = yn + (yn - ym) / (xn - xm) * (td - xn);
        else est = interp_np(td, ct, cv, nfin, y0, yn);
        const double sigma = sqrt(unc * unc + err * err);
        if (sigma - sigma == 0.0) chi += detection_term(m, est, sigma, log(sigma), dinf());
        else ul += upper_limit_term(m, est, err);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        chi += __shfl_xor(chi, o);
        ul += __shfl_xor(ul, o);
    }
    const double total = chi + ul;
    if (lane == 0) logl[b] = (total == total) ? total : NMMA_LOGL_FLOOR;
}

}  // namespace nmma

struct nmma_bol_handle {
    nmma::BolDev dev{};
    int device = 0, rows_per_wg = 4, probe = 0, n_dim = 0;
    unsigned lds = 0;
    std::vector<void*> owned;
};

using namespace nmma;

namespace {

hipError_t bol_upload(const double* src, size_t n, const double** dst, std::vector<void*>& owned) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n * sizeof(double), 16));
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (n) e = hipMemcpy(p, src, n * sizeof(double), hipMemcpyHostToDevice);
    *dst = static_cast<const double*>(p);
    return e;
}

template <int GEN, int MODE>
void bol_launch_one(const nmma_bol_handle* h, const double* theta, int64_t B, int64_t ld, const double* lbol_in, double* logl, double* tobs,
                    double* lbol, hipStream_t s) {
    const int R = h->rows_per_wg;
    hipLaunchKernelGGL((bol_logl<GEN, MODE>), dim3((unsigned)((B + R - 1) / R)), dim3(64 * R), h->lds, s, h->dev, theta, (long)B, (long)ld,
                       lbol_in, logl, tobs, lbol);
}

template <int MODE>
void bol_launch_gen(const nmma_bol_handle* h, int gen, const double* theta, int64_t B, int64_t ld, const double* lbol_in, double* logl,
                    double* tobs, double* lbol, hipStream_t s) {
    if (gen == NMMA_BOL_ARNETT) bol_launch_one<1, MODE>(h, theta, B, ld, lbol_in, logl, tobs, lbol, s);
    else if (gen == NMMA_BOL_ARNETT_MODIFIED) bol_launch_one<2, MODE>(h, theta, B, ld, lbol_in, logl, tobs, lbol, s);
    else bol_launch_one<0, MODE>(h, theta, B, ld, lbol_in, logl, tobs, lbol, s);
}

// mode as bol_logl's MODE; gen: the generator, NMMA_BOL_SUPPLIED for nmma_bol_loglike_lc
int bol_call(nmma_bol_handle* h, int gen, int mode, const double* theta, int64_t B, int64_t ld, const double* lbol_in, double* logl,
             double* tobs, double* lbol, void* stream, const char* who) {
    if (!h) return fail(std::string(who) + ": null handle");
    if (B < 0) return fail(std::string(who) + ": negative batch");
    if (B == 0) return 0;
    if (!theta) return fail(std::string(who) + ": null theta");
    if (ld < h->n_dim) return fail(std::string(who) + ": leading dimension smaller than n_dim");
    if ((B + h->rows_per_wg - 1) / h->rows_per_wg > 0x7fffffffLL) return fail(std::string(who) + ": batch too large");
    NM_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == 0 && h->probe == 1) mode = 3;
    if (mode == 0) bol_launch_gen<0>(h, gen, theta, B, ld, lbol_in, logl, tobs, lbol, s);
    else if (mode == 1) bol_launch_gen<1>(h, gen, theta, B, ld, lbol_in, logl, tobs, lbol, s);
    else if (mode == 2) bol_launch_gen<2>(h, gen, theta, B, ld, lbol_in, logl, tobs, lbol, s);
    else bol_launch_gen<3>(h, gen, theta, B, ld, lbol_in, logl, tobs, lbol, s);
    NM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

void nmma_bol_destroy(nmma_bol_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
}

int32_t nmma_bol_create(const nmma_bol_config* c, nmma_bol_handle** out) {
    if (!c || !out) return fail("nmma_bol_create: null argument");
    *out = nullptr;
    if (c->abi_version != NMMA_ABI_VERSION) return fail("nmma_bol_create: ABI version mismatch");
    if (c->model_kind < NMMA_BOL_SUPPLIED || c->model_kind > NMMA_BOL_ARNETT_MODIFIED) return fail("nmma_bol_create: bad model_kind");
    const int NS = c->n_sample_times, N = c->n_data;
    if (NS < 2 || !c->sample_times) return fail("nmma_bol_create: at least two sample_times are required");
    if (N < 1 || !c->data_times || !c->data_values || !c->data_sigmas) return fail("nmma_bol_create: at least one datum is required");
    for (int j = 0; j < NS; ++j) {
        const double t = c->sample_times[j];
        if (!std::isfinite(t) || (j > 0 && !(t > c->sample_times[j - 1]))) return fail("nmma_bol_create: sample_times must be finite and strictly ascending");
    }
    if (c->model_kind == NMMA_BOL_ARNETT && !(c->sample_times[0] >= 0.0)) return fail("nmma_bol_create: Arnett needs every sample time >= 0");
    if (c->model_kind == NMMA_BOL_ARNETT_MODIFIED && !(c->sample_times[0] > 0.0))
        return fail("nmma_bol_create: Arnett_modified divides by the time since the explosion: every sample time must be > 0");
    if (c->redshift_mode < NMMA_Z_ZERO || c->redshift_mode > NMMA_Z_GRID) return fail("nmma_bol_create: bad redshift_mode");
    const bool grid = c->redshift_mode == NMMA_Z_GRID;
    if (grid && (c->n_cosmo < 1 || !c->dist_grid || !c->z_grid)) return fail("nmma_bol_create: redshift grid missing");
    for (int i = 1; grid && i < c->n_cosmo; ++i)
        if (!(c->dist_grid[i] >= c->dist_grid[i - 1])) return fail("nmma_bol_create: dist_grid must not decrease");
    auto slot_ok = [&](const nmma_slot& s) { return s.col < c->n_dim && s.op >= NMMA_OP_IDENT && s.op <= NMMA_OP_ACOS; };
    if (c->n_dim < 0 || !slot_ok(c->tau_m) || !slot_ok(c->log10_mni) || !slot_ok(c->t_0) || !slot_ok(c->timeshift) || !slot_ok(c->redshift) ||
        !slot_ok(c->luminosity_distance) || !slot_ok(c->em_syserr))
        return fail("nmma_bol_create: slot out of range");
    const int n_cosmo = grid ? c->n_cosmo : 0;
    int rows = 4;
    while (rows > 1 && bol_lds_bytes(rows, NS, n_cosmo) > bol::LDS_BUDGET) rows /= 2;
    if (bol_lds_bytes(rows, NS, n_cosmo) > bol::LDS_BUDGET)
        return fail("nmma_bol_create: the grids do not fit the workgroup's LDS (16 bytes per sample time and per redshift-grid node, 64 KiB)");

    int ndev = 0;
    NM_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail("nmma_bol_create: no HIP device (this library has no CPU fallback)");
    if (c->device < 0 || c->device >= ndev) return fail("nmma_bol_create: bad device ordinal");
    NM_HIP(hipSetDevice(c->device));

    auto* h = new nmma_bol_handle();
    h->device = c->device;
    h->rows_per_wg = rows;
    h->n_dim = c->n_dim;
    h->lds = (unsigned)bol_lds_bytes(rows, NS, n_cosmo);
    BolDev& D = h->dev;
    D.kind = c->model_kind; D.NS = NS; D.N = N; D.n_cosmo = n_cosmo; D.redshift_mode = c->redshift_mode;
    D.tau_m = c->tau_m; D.log10_mni = c->log10_mni; D.t_0 = c->t_0; D.timeshift = c->timeshift; D.redshift = c->redshift;
    D.lumdist = c->luminosity_distance; D.syserr = c->em_syserr;
#define NM_BOL_UP(src, n, field)                                                                           \
    do {                                                                                                   \
        const hipError_t _e = bol_upload(src, n, &D.field, h->owned);                                      \
        if (_e != hipSuccess) {                                                                            \
            nmma_bol_destroy(h);                                                                           \
            return fail(std::string("nmma_bol_create: upload " #field " failed: ") + hipGetErrorString(_e)); \
        }                                                                                                  \
    } while (0)
    NM_BOL_UP(c->sample_times, (size_t)NS, st);
    NM_BOL_UP(c->data_times, (size_t)N, dt);
    NM_BOL_UP(c->data_values, (size_t)N, dv);
    NM_BOL_UP(c->data_sigmas, (size_t)N, ds);
    NM_BOL_UP(c->dist_grid, (size_t)n_cosmo, dist_grid);
    NM_BOL_UP(c->z_grid, (size_t)n_cosmo, z_grid);
#undef NM_BOL_UP
    *out = h;
    return 0;
}

int32_t nmma_bol_set_option(nmma_bol_handle* h, const char* name, int32_t value) {
    if (!h || !name) return fail("nmma_bol_set_option: null argument");
    if (std::string(name) != "probe") return fail(std::string("nmma_bol_set_option: unknown option '") + name + "'");
    if (value < 0 || value > 1) return fail("nmma_bol_set_option: probe is 0 or 1");
    h->probe = value;
    return 0;
}

int32_t nmma_bol_loglike(nmma_bol_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* logl_dev, void* stream) {
    if (h && h->dev.kind == NMMA_BOL_SUPPLIED) return fail("nmma_bol_loglike: the handle has no generator (NMMA_BOL_SUPPLIED: nmma_bol_loglike_lc)");
    if (B > 0 && !logl_dev) return fail("nmma_bol_loglike: null output");
    return bol_call(h, h ? h->dev.kind : 0, 0, theta_dev, B, ld, nullptr, logl_dev, nullptr, nullptr, stream, "nmma_bol_loglike");
}

int32_t nmma_bol_lightcurves(nmma_bol_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* obs_times_dev, double* lbol_dev,
                             void* stream) {
    if (h && h->dev.kind == NMMA_BOL_SUPPLIED) return fail("nmma_bol_lightcurves: the handle has no generator (NMMA_BOL_SUPPLIED)");
    if (B > 0 && (!obs_times_dev || !lbol_dev)) return fail("nmma_bol_lightcurves: null output");
    return bol_call(h, h ? h->dev.kind : 0, 1, theta_dev, B, ld, nullptr, nullptr, obs_times_dev, lbol_dev, stream, "nmma_bol_lightcurves");
}

int32_t nmma_bol_model_lightcurves(nmma_bol_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* lbol_dev, void* stream) {
    if (h && h->dev.kind == NMMA_BOL_SUPPLIED) return fail("nmma_bol_model_lightcurves: the handle has no generator (NMMA_BOL_SUPPLIED)");
    if (B > 0 && !lbol_dev) return fail("nmma_bol_model_lightcurves: null output");
    return bol_call(h, h ? h->dev.kind : 0, 2, theta_dev, B, ld, nullptr, nullptr, nullptr, lbol_dev, stream, "nmma_bol_model_lightcurves");
}

int32_t nmma_bol_loglike_lc(nmma_bol_handle* h, const double* theta_dev, int64_t B, int64_t ld, const double* lbol_dev, double* logl_dev,
                            void* stream) {
    if (B > 0 && (!lbol_dev || !logl_dev)) return fail("nmma_bol_loglike_lc: null buffer");
    return bol_call(h, NMMA_BOL_SUPPLIED, 0, theta_dev, B, ld, lbol_dev, logl_dev, nullptr, nullptr, stream, "nmma_bol_loglike_lc");
}

}  // extern "C"
