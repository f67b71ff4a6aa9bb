// em_pl.hip -- power-law flux light curves: the afterglow-plus-host-galaxy model Sr2023 (host_lc, nmma/em/lightcurve_generation.py:284-294,
// arXiv:2303.12849) and synchrotron_powerlaw (:773-783) with flux_to_ABmag (nmma/em/utils.py:793-811).  Kernels powerlaw_lc (the curves,
// the contract of me2017_lc / piro2021_lc) and powerlaw_logl (theta -> log L in one launch, no curve in memory), the side handle
// nmma_pl_handle and the nmma_pl_* entry points.  fp64 without contraction (this unit is built with -ffp-contract=off), the reference's
// operation order.
//
// The arithmetic.  One family:   F_f(t_j) = A_f p_j + C_f,   p_j = t_j^(-alpha),   mag_f(t_j) = ((-2.5 log10 F + r_f) + s)
//     Sr2023:       A_f = a_AG_<f>,  C_f = f_nu_<f>,  r_f = the filter's host magnitude,  s = 0
//     synchrotron:  A_f = F_ref (nu0_f (1 + z))^(-beta),  C_f = 0,  r_f = 16.4,  s = -distance_modulus  (x - d == x + (-d) in fp64; adding
//                   the zero C_f or s changes no bit of a positive F or a finite magnitude)
//     flux_to_ABmag: a node with F <= 0 or a NaN F is +inf; a (row, filter) with fewer than two positive F is NaN on every node.
// The one transcendental that depends on row AND node, p_j, does not depend on the filter: a row needs NS powers, not M NS, and the
// likelihood needs magnitudes -- the logarithm -- only at the two nodes that bracket a datum.  The arithmetic is a power, a multiply, an
// add, a compare and a logarithm per value: nothing a matrix instruction multiplies, so there is none here.
//
// powerlaw_lc: balanced over items like piro2021_lc -- a 256-thread workgroup owns a tile of TR rows (8; fewer, then node chunks, where
//   a long grid needs the LDS); per-row scalars by one lane each, then (row, filter) coefficients and (row, node) powers strided over
//   all threads into LDS, then (row, filter, node) items node fastest (a wave stores 64 consecutive doubles) with the positive fluxes
//   counted in integer LDS counters; only the pairs with fewer than two rewrite themselves as NaN.
//
// powerlaw_logl: one 16-lane group is one row (four rows a wave, sixteen a workgroup).  A row's bits depend on its own theta alone: no
//   wave-uniform decision looks at a neighbour row (counts are ballots masked to the group's 16 lanes), sums are DPP reductions within
//   the 16 lanes in a fixed order.  A group beyond the batch recomputes the last row and stores nothing, so every thread meets every
//   barrier.  The workgroup barriers are where LDS written by other lanes is read:
//     stage    the workgroup copies sample_times, the photometry and the band descriptors into LDS once for its sixteen rows  | barrier
//     phase A  every lane of the group: z (as piro2021_lc), 1 + z, timeshift, distance modulus, redshift correction, E(B-V), alpha; lanes
//              stride the filters: A_f, C_f, r_f, the extinction magnitude (one pow per (row, filter) for the synchrotron model); lanes
//              stride the bands: the band's systematic error (constant or the sampled column)
//     phase B  lanes stride the nodes: p_j = pow(t_j, -alpha) into the row's LDS array (16 x NS doubles a workgroup)           | barrier
//     phase C  per filter, lanes stride the nodes: count 0 < A_f p_j + C_f < inf (multiply, add, compare; a ballot per 16 nodes) -- the
//              NaN rule, combine_detector_data's "fewer than two finite" rule and sanity_check's floor are this one count < 2
//     phase D  lanes stride ALL the data in one pass (datum i on lane i mod 16, the order of em_lc_loglike): bisect the datum's epoch
//              in t_j (1 + z) + timeshift with the exact t_obs[lo] <= t < t_obs[lo + 1] tests, walk to the nearest finite node on either
//              side (the flux test again: autocomplete_data's finite mask), TWO log10, np.interp's form (lerp_np), +inf outside the
//              grid; detection_term_tab / upper_limit_term_tab as em_lc_loglike; the 64 virtual-lane sums of group_total_canon; floor.
//   Grids longer than NMMA_PL_FUSED_MAX_NS (or LDS beyond 64 KiB), averaged bands, time-node systematics, the Pei-1992 law and a sampled
//   Hubble constant take powerlaw_lc + nmma_em_loglike_lc: chosen once, at nmma_pl_create.
#include "em_host.h"
#include "em_lc.h"

namespace nmma {

namespace pl {
constexpr int NSCAL = 4;                   // per-row scalars of powerlaw_lc in LDS: alpha, 1 + z, s, (pad)
constexpr int LDS_BUDGET = 64 * 1024;
constexpr int ROWS = 16, GROUP = 16;       // powerlaw_logl: rows per workgroup, lanes per row
constexpr double R_MJY = 16.4;             // flux_to_ABmag(unit="mJy")
}  // namespace pl

struct PlDev {
    int kind, M;
    nmma_slot alpha, beta, f_ref;
    const nmma_slot *amp, *floor;          // [M] Sr2023
    const double* rmag;                    // [M] Sr2023
};

// the redshift of a row as piro2021_lc forms it
__device__ __forceinline__ double pl_redshift(const EmDev& P, const double* row) {
    double z = 0.0;
    if (P.redshift_mode == NMMA_Z_SLOT) z = apply_slot(P.redshift, row);
    else if (P.redshift_mode == NMMA_Z_GRID) {
        const double d_eff = apply_slot(P.lumdist, row) * (P.has_h0 ? apply_slot(P.hubble, row) * P.inv_h0_ref : 1.0);
        z = interp_np(d_eff, P.dist_grid, P.z_grid, P.n_cosmo, P.z_grid[0], P.z_grid[P.n_cosmo - 1]);
        if (P.has_h0) z *= d_eff;
    }
    return z;
}

// A_f, C_f, r_f of one (row, filter)
__device__ __forceinline__ void pl_coefficients(const PlDev& Q, const EmDev& P, const double* row, const int f, const double zp1, double& A,
                                                double& Cf, double& r) {
    if (Q.kind == NMMA_PL_SR2023) {
        A = apply_slot(Q.amp[f], row);
        Cf = apply_slot(Q.floor[f], row);
        r = Q.rmag[f];
    } else {
        A = apply_slot(Q.f_ref, row) * pow(P.nu0[f] * zp1, -apply_slot(Q.beta, row));
        Cf = 0.0;
        r = pl::R_MJY;
    }
}

// LDS (bytes) of a powerlaw_lc tile of TR rows with NCH nodes resident: [scalars TR x NSCAL | A, C, r  TR x M x 3 | p  TR x NCH | counters TR x M i32]
static inline long pl_lc_lds_bytes(int TR, int NCH, int M) { return (long)TR * (pl::NSCAL * 8 + 24L * M + 8L * NCH + 4L * M); }

__global__ __launch_bounds__(256) void powerlaw_lc(const PlDev Q, const EmDev* __restrict__ Pp, const double* __restrict__ theta, const long B,
                                                   const long ld, const int TR, const int NCH, double* __restrict__ lc) {
    using namespace pl;
    const EmDev& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* scal = reinterpret_cast<double*>(smem);      // [TR][NSCAL]
    double* coef = scal + TR * NSCAL;                    // [TR][M][3]  A, C, r
    double* pw = coef + TR * Q.M * 3;                    // [TR][NCH]   t^(-alpha)
    int* npos = reinterpret_cast<int*>(pw + TR * NCH);   // [TR][M]     positive fluxes of (row, filter)
    const int tid = threadIdx.x, lane = tid & 63;
    const int NS = P.NS, M = Q.M;
    const long b0 = (long)blockIdx.x * TR;
    const int rows = (int)(B - b0 < TR ? B - b0 : TR);

    // ---- per-row scalars
    for (int i = tid; i < rows * M; i += 256) npos[i] = 0;
    if (tid < rows) {
        const double* row = theta + (b0 + tid) * ld;
        double* s = scal + tid * NSCAL;
        s[0] = apply_slot(Q.alpha, row);
        s[1] = 1 + pl_redshift(P, row);
        s[2] = Q.kind == NMMA_PL_SYNCHROTRON ? -distance_modulus(apply_slot(P.lumdist, row)) : 0.0;
    }
    __syncthreads();
    // ---- per (row, filter) coefficients
    for (int i = tid; i < rows * M; i += 256) {
        const int r = i / M, f = i - r * M;
        pl_coefficients(Q, P, theta + (b0 + r) * ld, f, scal[r * NSCAL + 1], coef[i * 3], coef[i * 3 + 1], coef[i * 3 + 2]);
    }
    for (int j0 = 0; j0 < NS; j0 += NCH) {
        const int nch = NS - j0 < NCH ? NS - j0 : NCH;
        if (j0 > 0) __syncthreads();          // the previous chunk's powers are read
        // ---- per (row, node) powers
        for (int i = tid; i < rows * nch; i += 256) {
            const int r = i / nch, jj = i - r * nch;
            pw[r * NCH + jj] = pow(P.st[j0 + jj], -scal[r * NSCAL]);
        }
        __syncthreads();
        // ---- magnitudes per (row, filter, node), node fastest
        const int items = rows * M * nch;
        for (int i = tid; i < items; i += 256) {
            const int rf = i / nch, jj = i - rf * nch;
            const int r = rf / M;
            const double F = coef[rf * 3] * pw[r * NCH + jj] + coef[rf * 3 + 1];
            const bool pos = F > 0;
            lc[(b0 * M + rf) * NS + j0 + jj] = (pos ? -2.5 * log10(F) + coef[rf * 3 + 2] : dinf()) + scal[r * NSCAL + 2];
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

// LDS (bytes) of powerlaw_logl: [st NS | t, m, sigma, sigma_tot, ln sigma_tot  5 x ND | band lim, e_const  2 x NB] f64,
// [band of datum ND | band m, kind  2 x NB] i32 (padded to 8 bytes), then per row [p NS | A, C, r, ext  4 x M | band error NB] f64
__host__ __device__ static inline long pl_logl_shared_doubles(int NS, int ND, int NB) { return (long)NS + 5L * ND + 2L * NB + (ND + 2L * NB + 1) / 2; }
__host__ __device__ static inline long pl_logl_row_doubles(int NS, int M, int NB) { return (long)NS + 4L * M + NB; }
static inline long pl_logl_lds_bytes(int NS, int ND, int NB, int M) {
    return 8 * (pl_logl_shared_doubles(NS, ND, NB) + pl::ROWS * pl_logl_row_doubles(NS, M, NB));
}

__global__ __launch_bounds__(256) void powerlaw_logl(const PlDev Q, const EmDev* __restrict__ Pp, const double* __restrict__ theta, const long B,
                                                     const long ld, const int always_floor, double* __restrict__ logl) {
    using namespace pl;
    const EmDev& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NS = P.NS, M = Q.M, ND = P.n_data, NB = P.n_items;      // (every band has one source: a work item is a band)
    double* stl = reinterpret_cast<double*>(smem);       // [NS]
    double* d_t = stl + NS;                              // [ND] each
    double* d_m = d_t + ND;
    double* d_sig = d_m + ND;
    double* d_sigtot = d_sig + ND;
    double* d_logsig = d_sigtot + ND;
    double* b_lim = d_logsig + ND;                       // [NB] each
    double* b_e = b_lim + NB;
    int* d_band = reinterpret_cast<int*>(b_e + NB);      // [ND]
    int* b_m = d_band + ND;                              // [NB] each
    int* b_kind = b_m + NB;
    const int tid = threadIdx.x, g = tid >> 4, gl = tid & 15, grp = (tid & 63) >> 4;
    double* pw = reinterpret_cast<double*>(smem) + pl_logl_shared_doubles(NS, ND, NB) + (long)g * pl_logl_row_doubles(NS, M, NB);   // [NS]
    double* coef = pw + NS;                              // [M][4]  A, C, r, ext
    double* e_row = coef + 4 * M;                        // [NB]    the band's systematic error for this row

    // ---- stage what the sixteen rows share
    for (int j = tid; j < NS; j += 256) stl[j] = P.st[j];
    for (int i = tid; i < ND; i += 256) {
        d_t[i] = P.dt[i]; d_m[i] = P.dm[i]; d_sig[i] = P.dsig[i]; d_sigtot[i] = P.dsigtot[i]; d_logsig[i] = P.dlogsig[i];
        d_band[i] = P.d_item[i];
    }
    for (int k = tid; k < NB; k += 256) {
        const ItemDesc& it = P.item_desc[k];
        b_lim[k] = it.lim; b_e[k] = it.e_const; b_m[k] = it.m; b_kind[k] = it.kind;
    }
    __syncthreads();

    // ---- phase A: the row's scalars, every lane of the group for itself
    const long b_raw = (long)blockIdx.x * ROWS + g;
    const long b = b_raw < B ? b_raw : B - 1;            // (a group beyond the batch recomputes the last row and stores nothing)
    const double* row = theta + b * ld;
    const double d_l = apply_slot(P.lumdist, row);
    const double z = pl_redshift(P, row);
    const double zp1 = 1 + z, tsh = apply_slot(P.timeshift, row);
    const double dmod = distance_modulus(d_l), rc = redshift_correction(z);
    const double ebv = P.has_ebv ? apply_slot(P.ebv, row) : 0.0;
    const double alpha = apply_slot(Q.alpha, row);
    const double s = Q.kind == NMMA_PL_SYNCHROTRON ? -dmod : 0.0;
    double chk = d_l + z + tsh + ebv;                    // (sample_scalars' finiteness check, with the sampled systematics: em_lc_loglike)
    for (int p = 0; p < P.NP; ++p) chk += apply_slot(P.model_param[p], row);
    for (int k = 0; k < NB; ++k)
        if (b_kind[k] == NMMA_SYS_PARAM) chk += apply_slot(P.sys_slots[P.sys_off[P.item_desc[k].o]], row);
    bool bad = always_floor != 0 || !(chk - chk == 0.0);
    for (int f = gl; f < M; f += GROUP) {
        double A, Cf, r;
        pl_coefficients(Q, P, row, f, zp1, A, Cf, r);
        coef[4 * f] = A; coef[4 * f + 1] = Cf; coef[4 * f + 2] = r;
        coef[4 * f + 3] = extinction_mag(NMMA_EXT_LINEAR, P.ebv_coeff[f], zp1, ebv);
    }
    for (int k = gl; k < NB; k += GROUP)
        e_row[k] = b_kind[k] == NMMA_SYS_PARAM ? apply_slot(P.sys_slots[P.sys_off[P.item_desc[k].o]], row) : b_e[k];
    // ---- phase B: p_j per (row, node)
    for (int j = gl; j < NS; j += GROUP) pw[j] = pow(stl[j], -alpha);
    __syncthreads();

    // ---- phase C: finite nodes per (row, filter) -- fewer than two floor the row
    for (int f = 0; f < M; ++f) {
        const double A = coef[4 * f], Cf = coef[4 * f + 1];
        int nfin = 0;
        for (int j0 = 0; j0 < NS; j0 += GROUP) {
            const int j = j0 + gl;
            const double F = j < NS ? A * pw[j] + Cf : 0.0;
            const unsigned long long m = __ballot(F > 0 && F < dinf());
            nfin += __popcll((m >> (grp * GROUP)) & 0xffffull);
        }
        if (nfin < 2) bad = true;
    }
    if (!(s - s == 0.0)) bad = true;                     // (a non-finite distance modulus: no finite magnitude anywhere)

    // ---- phase D: the likelihood, datum i on lane i mod 16, into virtual lane i mod 64 (group_total_canon)
    const double t_first = stl[0] * zp1 + tsh, t_last = stl[NS - 1] * zp1 + tsh;
    double chi_a[4] = {0.0, 0.0, 0.0, 0.0}, gp_a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < ND; d0 += GROUP) {
        const int di = d0 + gl, h = (d0 / GROUP) & 3;
        if (di >= ND) continue;
        const int k = d_band[di];
        const double* cf = coef + 4 * b_m[k];
        const double A = cf[0], Cf = cf[1], r = cf[2], ext = cf[3];
        const double t = d_t[di];
        auto flux = [&](const int j) { return A * pw[j] + Cf; };
        auto finite_node = [&](const int j) { const double F = flux(j); return F > 0 && F < dinf(); };
        // the detector-frame magnitude of node j (model.py:390-397) from its flux
        auto app = [&](const int j) { double v = (-2.5 * log10(flux(j)) + r) + s; if (ext != 0.0) v = v + ext; return (v + dmod) + rc; };
        double est = dinf();
        if (t != t) est = t;
        else if (t >= t_first && t <= t_last) {
            int lo = 0, hi = NS - 1;                     // t_obs[lo] <= t (<= t_obs[NS - 1])
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (stl[mid] * zp1 + tsh <= t) lo = mid; else hi = mid;
            }
            if (stl[hi] * zp1 + tsh <= t) lo = hi;       // t on the last node
            int jl = lo;                                 // np.interp over the FINITE nodes only, left = right = +inf (utils.py:634-645)
            while (jl >= 0 && !finite_node(jl)) --jl;
            int jr = lo + 1;
            while (jr < NS && !finite_node(jr)) ++jr;
            if (jl >= 0) {
                const double x0 = stl[jl] * zp1 + tsh;
                if (x0 == t) est = app(jl);
                else if (jr < NS) est = lerp_np(t, x0, stl[jr] * zp1 + tsh, app(jl), app(jr));
            }
        }
        const double sd = d_sig[di], e = e_row[k];
        double sig, lsig;
        if (b_kind[k] == NMMA_SYS_CONST) { sig = d_sigtot[di]; lsig = d_logsig[di]; }
        else { sig = sqrt(sd * sd + e * e); lsig = log(sig); }
        double c = 0.0, u = 0.0;
        if (sig - sig == 0.0) c = detection_term_tab(d_m[di], est, sig, lsig, b_lim[k], static_cast<const double*>(kLogPhiTab));
        else u = upper_limit_term_tab(d_m[di], est, e, static_cast<const double*>(kLogPhiTab));
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (h == q) { chi_a[q] += c; gp_a[q] += u; }
    }
    const double chi_tot = group_total_canon<GROUP>(chi_a), gp_tot = group_total_canon<GROUP>(gp_a);
    if (gl == 0 && b_raw < B) {
        double tot = chi_tot + gp_tot;
        if (bad || !(tot - tot == 0.0)) tot = NMMA_LOGL_FLOOR;
        logl[b] = tot;
    }
}

}  // namespace nmma

struct nmma_pl_handle {
    nmma::PlDev dev{};
    nmma_em_handle* em = nullptr;
    int device = 0, fused = 0;
    unsigned lds_logl = 0;
    std::string why;                 // why the handle takes two launches
    std::vector<void*> owned;
    double* lc_ws = nullptr;         // [B][M][NS] curves of the two-launch path
    int64_t lc_cap = 0;
};

using namespace nmma;

namespace {

template <typename T>
hipError_t pl_upload(const T* src, size_t n, const T** dst, std::vector<void*>& owned) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n * sizeof(T), 16));
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (n) e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    *dst = static_cast<const T*>(p);
    return e;
}

int pl_check(nmma_pl_handle* pl, nmma_em_handle* em, const double* theta, int64_t B, int64_t ld, const void* out, const char* who) {
    if (!pl || !em) return fail(std::string(who) + ": null handle");
    if (pl->em != em) return fail(std::string(who) + ": not the em handle this object was created with");
    if (B < 0) return fail(std::string(who) + ": negative batch");
    if (B > 0 && (!theta || !out)) return fail(std::string(who) + ": null buffer");
    if (ld < em->dev.D) return fail(std::string(who) + ": leading dimension smaller than n_dim");
    return 0;
}

int pl_launch_lc(nmma_pl_handle* pl, const double* theta, int64_t B, int64_t ld, double* lc, hipStream_t s, const char* who) {
    const EmDev& P = pl->em->dev;
    // rows per tile: 8 as piro2021_lc, halved while the powers of the whole grid do not fit the LDS budget; at one row per tile the
    // grid is walked in chunks
    int TR = 8, NCH = P.NS;
    while (TR > 1 && pl_lc_lds_bytes(TR, NCH, P.M) > pl::LDS_BUDGET) TR /= 2;
    if (pl_lc_lds_bytes(TR, NCH, P.M) > pl::LDS_BUDGET) NCH = (int)((pl::LDS_BUDGET - pl_lc_lds_bytes(1, 0, P.M)) / 8);
    if (NCH < 1) return fail(std::string(who) + ": too many model filters for the power-law kernel's LDS");
    const int64_t tiles = (B + TR - 1) / TR;
    if (tiles > 0x7fffffffLL) return fail(std::string(who) + ": batch too large");
    hipLaunchKernelGGL(powerlaw_lc, dim3((unsigned)tiles), dim3(256), (unsigned)pl_lc_lds_bytes(TR, NCH, P.M), s, pl->dev, pl->em->dev_d, theta,
                       (long)B, (long)ld, TR, NCH, lc);
    NM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

void nmma_pl_destroy(nmma_pl_handle* pl) {
    if (!pl) return;
    (void)hipSetDevice(pl->device);
    for (void* p : pl->owned) (void)hipFree(p);
    if (pl->lc_ws) (void)hipFree(pl->lc_ws);
    delete pl;
}

int32_t nmma_pl_create(const nmma_pl_config* c, nmma_em_handle* em, nmma_pl_handle** out) {
    if (!c || !em || !out) return fail("nmma_pl_create: null argument");
    *out = nullptr;
    if (c->abi_version != NMMA_ABI_VERSION) return fail("nmma_pl_create: ABI version mismatch");
    if (c->kind != NMMA_PL_SR2023 && c->kind != NMMA_PL_SYNCHROTRON) return fail("nmma_pl_create: bad kind");
    const EmDev& P = em->dev;
    if (P.model_kind != NMMA_MODEL_EXTERNAL || P.union_grid) return fail("nmma_pl_create: the em handle must be of kind NMMA_MODEL_EXTERNAL on its own grid");
    if (c->device != em->device) return fail("nmma_pl_create: the em handle lives on another device");
    const int M = c->n_filters;
    if (M < 1 || M != P.M) return fail("nmma_pl_create: n_filters differs from the em handle's n_model_filters");
    if (P.NS < 2) return fail("nmma_pl_create: at least two sample_times are required");
    for (double t : em->st_host)
        if (!(t > 0.0) || !std::isfinite(t)) return fail("nmma_pl_create: the flux is a power of the time since the trigger: every sample time must be > 0 and finite");
    auto slot_ok = [&](const nmma_slot& s) { return s.col < P.D && s.op >= NMMA_OP_IDENT && s.op <= NMMA_OP_ACOS; };
    if (!slot_ok(c->alpha)) return fail("nmma_pl_create: slot out of range");
    if (c->kind == NMMA_PL_SR2023) {
        if (!c->amp_slots || !c->floor_slots || !c->residual_mag) return fail("nmma_pl_create: Sr2023 needs amp_slots, floor_slots and residual_mag per filter");
        for (int f = 0; f < M; ++f) {
            if (!slot_ok(c->amp_slots[f]) || !slot_ok(c->floor_slots[f])) return fail("nmma_pl_create: slot out of range");
            // (flux_to_ABmag tests `if residual_mag:` -- a host magnitude of exactly 0 would silently become the cgs zero point -48.6)
            if (!std::isfinite(c->residual_mag[f]) || c->residual_mag[f] == 0.0)
                return fail("nmma_pl_create: residual_mag must be finite and not 0 (the reference reads a host magnitude of 0 as 'none given')");
        }
    } else {
        if (!slot_ok(c->beta) || !slot_ok(c->f_ref)) return fail("nmma_pl_create: slot out of range");
    }
    NM_HIP(hipSetDevice(em->device));
    if (c->kind == NMMA_PL_SYNCHROTRON) {      // (an em handle created without filter_nu0 holds zeros)
        std::vector<double> nu0(M);
        NM_HIP(hipMemcpy(nu0.data(), P.nu0, M * sizeof(double), hipMemcpyDeviceToHost));
        for (double nu : nu0)
            if (!(nu > 0.0) || !std::isfinite(nu)) return fail("nmma_pl_create: the synchrotron model needs the em handle's filter_nu0 (Hz, > 0)");
    }
    auto* pl = new nmma_pl_handle();
    pl->em = em;
    pl->device = em->device;
    PlDev& Q = pl->dev;
    Q.kind = c->kind; Q.M = M; Q.alpha = c->alpha; Q.beta = c->beta; Q.f_ref = c->f_ref;
    const bool sr = c->kind == NMMA_PL_SR2023;
#define NM_PL_UP(T, src, field)                                                                            \
    do {                                                                                                   \
        const hipError_t _e = pl_upload<T>(src, sr ? (size_t)M : 0, &Q.field, pl->owned);                  \
        if (_e != hipSuccess) {                                                                            \
            nmma_pl_destroy(pl);                                                                           \
            return fail(std::string("nmma_pl_create: upload " #field " failed: ") + hipGetErrorString(_e)); \
        }                                                                                                  \
    } while (0)
    NM_PL_UP(nmma_slot, c->amp_slots, amp);
    NM_PL_UP(nmma_slot, c->floor_slots, floor);
    NM_PL_UP(double, c->residual_mag, rmag);
#undef NM_PL_UP
    // ---- which path: the one-launch kernel takes what it serves exactly
    const long lds = pl_logl_lds_bytes(P.NS, P.n_data, P.n_items, M);
    if (P.n_items != P.O) pl->why = "an averaged band (several model filters per observed band)";
    else if (P.kmax > 1) pl->why = "time-node systematics";
    else if (P.has_ebv && P.ext_law != NMMA_EXT_LINEAR) pl->why = "the Pei-1992 extinction law";
    else if (P.has_h0) pl->why = "a sampled Hubble constant";
    else if (P.NS > NMMA_PL_FUSED_MAX_NS) pl->why = "a time grid longer than NMMA_PL_FUSED_MAX_NS";
    else if (lds > pl::LDS_BUDGET) pl->why = "photometry beyond the kernel's 64 KiB of LDS";
    pl->fused = pl->why.empty() ? 1 : 0;
    pl->lds_logl = (unsigned)lds;
    *out = pl;
    return 0;
}

int32_t nmma_pl_fused(const nmma_pl_handle* pl, const nmma_em_handle* em) {
    if (!pl || pl->em != em) return -1;
    return pl->fused;
}

int32_t nmma_pl_model_lightcurves(nmma_pl_handle* pl, nmma_em_handle* em, const double* theta_dev, int64_t B, int64_t ld, double* lc_dev,
                                  void* stream) {
    if (pl_check(pl, em, theta_dev, B, ld, lc_dev, "nmma_pl_model_lightcurves")) return 1;
    if (B == 0) return 0;
    NM_HIP(hipSetDevice(pl->device));
    return pl_launch_lc(pl, theta_dev, B, ld, lc_dev, static_cast<hipStream_t>(stream), "nmma_pl_model_lightcurves");
}

int32_t nmma_pl_loglike(nmma_pl_handle* pl, nmma_em_handle* em, const double* theta_dev, int64_t B, int64_t ld, double* logl_dev,
                        void* stream) {
    if (pl_check(pl, em, theta_dev, B, ld, logl_dev, "nmma_pl_loglike")) return 1;
    if (B == 0) return 0;
    NM_HIP(hipSetDevice(pl->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (pl->fused) {
        const int64_t wgs = (B + pl::ROWS - 1) / pl::ROWS;
        if (wgs > 0x7fffffffLL) return fail("nmma_pl_loglike: batch too large");
        hipLaunchKernelGGL(powerlaw_logl, dim3((unsigned)wgs), dim3(256), pl->lds_logl, s, pl->dev, em->dev_d, theta_dev, (long)B, (long)ld,
                           em->always_floor, logl_dev);
        NM_HIP(hipGetLastError());
        return 0;
    }
    const int64_t need = B * em->dev.M * em->dev.NS;
    if (need > pl->lc_cap) {           // (grown on demand, outside any capture)
        if (pl->lc_ws) (void)hipFree(pl->lc_ws);
        pl->lc_ws = nullptr;
        pl->lc_cap = 0;
        NM_HIP(hipMalloc(reinterpret_cast<void**>(&pl->lc_ws), need * sizeof(double)));
        pl->lc_cap = need;
    }
    if (pl_launch_lc(pl, theta_dev, B, ld, pl->lc_ws, s, "nmma_pl_loglike")) return 1;
    return nmma_em_loglike_lc(em, theta_dev, B, ld, pl->lc_ws, logl_dev, stream);
}

}  // extern "C"
