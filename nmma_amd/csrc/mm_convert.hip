// mm_convert.hip -- the step in front of the light curve of a joint GW + EOS + EM analysis, for a batch in one launch: sampled binary and
// EOS parameters -> source-frame masses -> tabulated-EOS look-up (EOS_to_ns_parameters / EOS_to_system_parameters,
// nmma/core/conversion.py:222-237, driven by EoSConverter(method="tabulated"), nmma/eos/eos_processing.py:292-360) or the quasi-universal
// relations (radii_from_qur, :239-270) -> the NR ejecta fits of KilonovaEjectaFitting (:318-766) and log10_E0 from the disk mass
// (grb_energy_conversion, :699-726).  Kernel mm_convert, the handle nmma_mm_handle and the nmma_mm_* entry points.  fp64 without
// contraction (this unit is built with -ffp-contract=off); the scalar arithmetic is mm_math.h's, in the reference's operation order.
//
// The work split.  One 16-lane group is one row (four rows a wave, sixteen a workgroup of 256), the split of powerlaw_logl and the walk
// and dense tasks.  A row's bits depend on its own theta alone: ballots are masked to the group's 16 lanes, sums are group_sum's DPP
// reductions within the 16 lanes in a fixed order, and no decision looks at a neighbour row.  A group beyond the batch recomputes the last
// row and stores nothing, so every thread meets every barrier and every ballot.
//     stage    NMMA_MM_EOS_SINGLE: the workgroup copies the one table (mass | radius | log lambda, 3 x NPAD doubles) into LDS   | barrier
//     copy     lanes stride the D sampled columns of the row into out (a group's loads and stores are consecutive doubles)
//     masses   every lane of the group for itself: component masses, z (column, constant or np.interp on the z(d_L) grid, the look-up of
//              sample_scalars: interp_np with constant ends), the source frame
//     look-up  the tables are padded struct-of-arrays [n_eos][NPAD], NPAD a multiple of 16, the masses padded with +inf.  Per chunk of 16
//              nodes lane l loads mass[c + l] ONCE and compares it with both component masses; the number of nodes <= m is the popcount
//              of the group's 16 ballot bits, summed over the chunks -- np.interp's bracket without a dependent bisection (NPAD / 16
//              coalesced loads instead of log2(n) dependent ones per mass).  The bracket's four values are then read at a group-uniform
//              address and interpolated with lerp_np: the bits are numpy's.  left / right: -inf for log lambda, 0 for the radius.
//     fits     the scalar chain, every lane of the group the same instructions (a SIMD runs them at the cost of one lane)
//     jet      power-law jet only: lanes stride the reference's 100 nodes, y into the row's LDS array                          | barrier
//              lanes stride the 49 Simpson panels; group_sum; Cartwright's last interval
//     store    lane k of the group stores derived quantity k (11 of them), plain stores
#include "em_host.h"
#include "mm_math.h"

namespace nmma {

namespace mmc {
constexpr int ROWS = 16, GROUP = 16;
constexpr int YSTRIDE = 104;               // doubles per row of the jet's node array (100 nodes, padded)
}  // namespace mmc

struct MmDev {
    int D, mass_mode, redshift_mode, n_cosmo, eos_mode, n_eos, npad, fits, spin_mode, jet, wing_is_angle;
    nmma_slot mass_a, mass_b, redshift, lumdist, eos, lambda_1, lambda_2, tov, radius_1, radius_2, r16, alpha, zeta, spin_a, spin_b, eps,
        theta_core, wing, b;
    const double *dist_grid, *z_grid;
    const double *t_mass, *t_radius, *t_loglam;    // [n_eos][npad]
    const int* t_n;                                // [n_eos]
    const double *t_tov, *t_r14, *t_r16;           // [n_eos]
    double log10_msun_erg;
    int out_col[NMMA_MM_N_OUTPUTS];
    int* status;
};

__global__ __launch_bounds__(256) void mm_convert(const MmDev P, const double* __restrict__ theta, const long B, const long ld,
                                                  double* __restrict__ out, const long ld_out) {
    using namespace mmc;
    using namespace mm;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, g = tid >> 4, gl = tid & 15, grp = (tid & 63) >> 4;
    const bool tables = P.eos_mode == NMMA_MM_EOS_TABLES || P.eos_mode == NMMA_MM_EOS_SINGLE;
    const bool single = P.eos_mode == NMMA_MM_EOS_SINGLE;
    const int npad = P.npad;
    double* ynode = smem + (single ? 3 * npad : 0) + g * YSTRIDE;

    // ---- stage: the one table of the single-EOS form
    if (single) {
        for (int i = tid; i < npad; i += 256) {
            smem[i] = P.t_mass[i];
            smem[npad + i] = P.t_radius[i];
            smem[2 * npad + i] = P.t_loglam[i];
        }
        __syncthreads();
    }

    const long b_raw = (long)blockIdx.x * ROWS + g;
    const bool live = b_raw < B;
    const long b = live ? b_raw : B - 1;
    const double* row = theta + b * ld;
    double* orow = out + b * ld_out;

    // ---- copy: the sampled columns
    if (live)
        for (int c = gl; c < P.D; c += GROUP) orow[c] = row[c];

    // ---- masses: detector frame -> source frame (source_frame_masses, :104-117)
    double m1, m2;
    component_masses(P.mass_mode, apply_slot(P.mass_a, row), apply_slot(P.mass_b, row), m1, m2);
    double z = 0.0;
    if (P.redshift_mode == NMMA_Z_SLOT) z = apply_slot(P.redshift, row);
    else if (P.redshift_mode == NMMA_Z_GRID)
        z = interp_np(apply_slot(P.lumdist, row), P.dist_grid, P.z_grid, P.n_cosmo, P.z_grid[0], P.z_grid[P.n_cosmo - 1]);
    const double m1s = m1 / (1 + z), m2s = m2 / (1 + z);

    // ---- EOS: lambda_1, lambda_2, radius_1, radius_2, TOV_mass, R_14, R_16
    double lam1 = 0.0, lam2 = 0.0, r1 = 0.0, r2 = 0.0, mtov = 0.0, r14 = 0.0, r16 = 0.0;
    if (tables) {
        int e = 0;
        bool eos_bad = false;
        if (!single) {
            const double t = trunc(apply_slot(P.eos, row));       // astype(int) truncates
            eos_bad = !(t >= 0.0 && t < (double)P.n_eos);          // (NaN included)
            if (!eos_bad) e = (int)t;
        }
        // (an out-of-range row walks table 0 like its neighbours -- no branch around the ballots -- and its results are replaced below)
        const double* xm = single ? smem : P.t_mass + (long)e * npad;
        const double* xr = single ? smem + npad : P.t_radius + (long)e * npad;
        const double* xl = single ? smem + 2 * npad : P.t_loglam + (long)e * npad;
        const int n = P.t_n[e];
        int cnt1 = 0, cnt2 = 0;
        for (int c0 = 0; c0 < npad; c0 += GROUP) {
            const double mv = xm[c0 + gl];
            const unsigned long long k1 = __ballot(mv <= m1s), k2 = __ballot(mv <= m2s);
            cnt1 += __popcll((k1 >> (grp * GROUP)) & 0xffffull);
            cnt2 += __popcll((k2 >> (grp * GROUP)) & 0xffffull);
        }
        cnt1 = cnt1 < n ? cnt1 : n;            // (+inf counts the padding as well)
        cnt2 = cnt2 < n ? cnt2 : n;
        // np.interp(x, xm, fp, left, right) from the number of nodes <= x: interp_np's cases
        auto interp = [&](const double x, const int cnt, const double* fp, const double left, const double right) {
            if (x != x) return x;
            if (cnt == 0) return left;
            if (x > xm[n - 1]) return right;
            if (cnt == n) return fp[n - 1];
            const int j = cnt - 1;
            if (xm[j] == x) return fp[j];
            return lerp_np(x, xm[j], xm[j + 1], fp[j], fp[j + 1]);
        };
        lam1 = exp(interp(m1s, cnt1, xl, -dinf(), -dinf()));
        lam2 = exp(interp(m2s, cnt2, xl, -dinf(), -dinf()));
        r1 = interp(m1s, cnt1, xr, 0.0, 0.0);
        r2 = interp(m2s, cnt2, xr, 0.0, 0.0);
        mtov = P.t_tov[e]; r14 = P.t_r14[e]; r16 = P.t_r16[e];
        if (eos_bad) {
            lam1 = lam2 = r1 = r2 = mtov = r14 = r16 = 0.0;       // no neutron star anywhere: the fits answer four -inf
            if (gl == 0 && live) atomicOr(P.status, NMMA_MM_STATUS_EOS_RANGE);
        }
    } else if (P.eos_mode == NMMA_MM_EOS_QUR) {
        lam1 = apply_slot(P.lambda_1, row);
        lam2 = apply_slot(P.lambda_2, row);
        r1 = mass_and_compactness_to_radius(m1s, lambda_to_compactness(lam1));
        r2 = mass_and_compactness_to_radius(m2s, lambda_to_compactness(lam2));
        r16 = qur_r16(m1s, m2s, lam1, lam2);
        mtov = apply_slot(P.tov, row);
    } else {
        r1 = apply_slot(P.radius_1, row);
        r2 = apply_slot(P.radius_2, row);
        mtov = apply_slot(P.tov, row);
        r16 = apply_slot(P.r16, row);
    }

    // ---- fits (ejecta_parameter_conversion's array form, :759-766)
    double o[4] = {-dinf(), -dinf(), -dinf(), -dinf()};
    if (P.fits) {
        FitInput f;
        f.m1 = m1s; f.m2 = m2s; f.r1 = r1; f.r2 = r2; f.mtov = mtov; f.r16 = r16;
        f.alpha = apply_slot(P.alpha, row);
        f.zeta = apply_slot(P.zeta, row);
        f.chi = 0.0;
        const bool bns = r1 > 0., nsbh = !bns && r2 > 0.;
        double log10_ejet = 0.0, theta_core = 0.0;
        if (bns) {
            double l10disk;
            bns_ejecta(f, o, l10disk);
            if (P.jet != NMMA_MM_JET_NONE) {
                theta_core = apply_slot(P.theta_core, row);
                log10_ejet = log10_jet_energy(apply_slot(P.eps, row), f.zeta, l10disk, P.log10_msun_erg);
                if (P.jet == NMMA_MM_JET_TOPHAT) o[3] = tophat_log10_e0(log10_ejet, theta_core);
            }
        } else if (nsbh) {
            f.chi = apply_slot(P.spin_a, row);
            if (P.spin_mode == NMMA_MM_SPIN_A_COS_TILT) f.chi = f.chi * apply_slot(P.spin_b, row);
            else if (P.spin_mode == NMMA_MM_SPIN_A_TILT) f.chi = f.chi * cos(apply_slot(P.spin_b, row));
            nsbh_ejecta(f, o);
        }
        // ---- jet: the power-law jet's integral, by the whole group (every group: the barrier is the workgroup's)
        if (P.jet == NMMA_MM_JET_POWERLAW) {
            const double tc = apply_slot(P.theta_core, row), bb = apply_slot(P.b, row);
            const double wing = apply_slot(P.wing, row);
            const double stop = (P.wing_is_angle ? wing / tc : wing) * tc;
            for (int i = gl; i < kJetNodes; i += GROUP) ynode[i] = jet_node_y(jet_node_x(i, stop), tc, bb);
            __syncthreads();
            double part = 0.0;
            for (int k = gl; k < kJetPanels; k += GROUP) part += simpson_panel(k, stop, ynode);
            const double integral = group_sum(part, GROUP) + simpson_last_interval(stop, ynode);
            if (bns) o[3] = powerlaw_log10_e0(log10_ejet, integral);
        }
        if (bns) {                             // "np.where(np.isfinite(converted_ejecta), converted_ejecta, -np.inf)", :739
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = is_finite(o[k]) ? o[k] : -dinf();
        }
    }

    // ---- store: lane k of the group holds derived quantity k
    const double v[NMMA_MM_N_OUTPUTS] = {o[0], o[1], o[2], o[3], lam1, lam2, r1, r2, mtov, r14, r16};
    double mine = 0.0;
    int col = -1;
#pragma unroll
    for (int k = 0; k < NMMA_MM_N_OUTPUTS; ++k)
        if (gl == k) { mine = v[k]; col = P.out_col[k]; }
    if (live && col >= 0) orow[col] = mine;
}

}  // namespace nmma

struct nmma_mm_handle {
    nmma::MmDev dev{};
    int device = 0;
    unsigned lds = 0;
    int64_t min_ld_out = 0;
    std::vector<void*> owned;
};

using namespace nmma;

namespace {

template <typename T>
hipError_t mm_upload(const std::vector<T>& src, const T** dst, std::vector<void*>& owned) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(src.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (!src.empty()) e = hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    *dst = static_cast<const T*>(p);
    return e;
}

}  // namespace

extern "C" {

void nmma_mm_destroy(nmma_mm_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
}

int32_t nmma_mm_create(const nmma_mm_config* c, nmma_mm_handle** out) {
    if (!c || !out) return fail("nmma_mm_create: null argument");
    *out = nullptr;
    if (c->abi_version != NMMA_ABI_VERSION) return fail("nmma_mm_create: ABI version mismatch");
    const int D = c->n_dim;
    if (D < 1) return fail("nmma_mm_create: n_dim must be at least 1");
    if (c->mass_mode != NMMA_MM_CHIRP_MASS_RATIO && c->mass_mode != NMMA_MM_COMPONENT_MASSES) return fail("nmma_mm_create: bad mass_mode");
    if (c->redshift_mode < NMMA_Z_ZERO || c->redshift_mode > NMMA_Z_GRID) return fail("nmma_mm_create: bad redshift_mode");
    if (c->eos_mode < NMMA_MM_EOS_TABLES || c->eos_mode > NMMA_MM_EOS_GIVEN) return fail("nmma_mm_create: bad eos_mode");
    if (c->jet < NMMA_MM_JET_NONE || c->jet > NMMA_MM_JET_POWERLAW) return fail("nmma_mm_create: bad jet form");
    if (c->spin_mode < NMMA_MM_SPIN_CHI || c->spin_mode > NMMA_MM_SPIN_A_TILT) return fail("nmma_mm_create: bad spin_mode");
    if (c->jet != NMMA_MM_JET_NONE && !c->fits) return fail("nmma_mm_create: log10_E0 comes from the disk mass of the ejecta fits: jet needs fits = 1");
    const bool tables = c->eos_mode == NMMA_MM_EOS_TABLES || c->eos_mode == NMMA_MM_EOS_SINGLE;
    // every slot the chosen modes read must name a column of theta (or carry a constant)
    std::vector<const nmma_slot*> used = {&c->mass_a, &c->mass_b};
    if (c->redshift_mode == NMMA_Z_SLOT) used.push_back(&c->redshift);
    if (c->redshift_mode == NMMA_Z_GRID) used.push_back(&c->luminosity_distance);
    if (c->eos_mode == NMMA_MM_EOS_TABLES) used.push_back(&c->eos);
    if (c->eos_mode == NMMA_MM_EOS_QUR) used.insert(used.end(), {&c->lambda_1, &c->lambda_2, &c->tov_mass});
    if (c->eos_mode == NMMA_MM_EOS_GIVEN) used.insert(used.end(), {&c->radius_1, &c->radius_2, &c->tov_mass, &c->r_16});
    if (c->fits) used.insert(used.end(), {&c->alpha, &c->ratio_zeta, &c->spin_a});
    if (c->fits && c->spin_mode != NMMA_MM_SPIN_CHI) used.push_back(&c->spin_b);
    if (c->jet != NMMA_MM_JET_NONE) used.insert(used.end(), {&c->ratio_epsilon, &c->theta_core});
    if (c->jet == NMMA_MM_JET_POWERLAW) used.insert(used.end(), {&c->wing, &c->b});
    for (const nmma_slot* s : used)
        if (s->col >= D || s->op < NMMA_OP_IDENT || s->op > NMMA_OP_ACOS) return fail("nmma_mm_create: slot out of range");
    int64_t min_ld_out = D;
    for (int k = 0; k < NMMA_MM_N_OUTPUTS; ++k) {
        const int col = c->out_col[k];
        if (col < 0) continue;
        if (col < D) return fail("nmma_mm_create: a derived column would overwrite a sampled one");
        for (int j = 0; j < k; ++j)
            if (c->out_col[j] == col) return fail("nmma_mm_create: two derived quantities share a column");
        min_ld_out = std::max<int64_t>(min_ld_out, col + 1);
    }
    if (c->redshift_mode == NMMA_Z_GRID) {
        if (c->n_cosmo < 2 || !c->dist_grid || !c->z_grid) return fail("nmma_mm_create: NMMA_Z_GRID needs dist_grid and z_grid of at least two nodes");
        for (int i = 1; i < c->n_cosmo; ++i)
            if (!(c->dist_grid[i] > c->dist_grid[i - 1])) return fail("nmma_mm_create: dist_grid must be strictly ascending");
    }

    // ---- the tables: checked, padded to a multiple of 16 nodes (masses with +inf), with the per-table constants of EOS_to_ns_parameters
    std::vector<double> tm, tr, tl, tov, r14, r16;
    std::vector<int> tn;
    int npad = 16;
    if (tables) {
        if (c->n_eos < 1 || (c->eos_mode == NMMA_MM_EOS_SINGLE && c->n_eos != 1)) return fail("nmma_mm_create: bad n_eos");
        if (!c->eos_n_nodes || !c->eos_radius || !c->eos_mass || !c->eos_log_lambda) return fail("nmma_mm_create: the EOS arrays are missing");
        int nmax = 0;
        for (int e = 0; e < c->n_eos; ++e) {
            const int n = c->eos_n_nodes[e];
            if (n < 2 || n > NMMA_MM_MAX_NODES)
                return fail("nmma_mm_create: EOS " + std::to_string(e) + " has " + std::to_string(n) + " nodes; 2 .. " + std::to_string(NMMA_MM_MAX_NODES) + " are served");
            nmax = std::max(nmax, n);
        }
        npad = (nmax + 15) / 16 * 16;
        const size_t total = (size_t)c->n_eos * npad;
        tm.assign(total, HUGE_VAL); tr.assign(total, 0.0); tl.assign(total, 0.0);
        size_t off = 0;
        for (int e = 0; e < c->n_eos; ++e) {
            const int n = c->eos_n_nodes[e];
            const double *ms = c->eos_mass + off, *rs = c->eos_radius + off, *ls = c->eos_log_lambda + off;
            for (int i = 0; i < n; ++i) {
                if (!std::isfinite(ms[i]) || !std::isfinite(rs[i])) return fail("nmma_mm_create: EOS " + std::to_string(e) + " holds a non-finite mass or radius");
                // (np.interp is undefined on a table that turns back: the reference would answer garbage silently)
                if (i > 0 && !(ms[i] > ms[i - 1]))
                    return fail("nmma_mm_create: the masses of EOS " + std::to_string(e) + " are not strictly ascending (node " + std::to_string(i) +
                                "): cut the table at its maximum mass");
                if (!std::isfinite(ls[i])) return fail("nmma_mm_create: EOS " + std::to_string(e) + " holds a tidal deformability that is not positive and finite");
                tm[(size_t)e * npad + i] = ms[i]; tr[(size_t)e * npad + i] = rs[i]; tl[(size_t)e * npad + i] = ls[i];
            }
            tn.push_back(n);
            tov.push_back(ms[n - 1]);                              // masses.max()
            r14.push_back(interp_np(1.4, ms, rs, n, 0.0, 0.0));     // np.interp(x=[1.4, 1.6], xp=masses, fp=radii, left=0, right=0)
            r16.push_back(interp_np(1.6, ms, rs, n, 0.0, 0.0));
            off += n;
        }
    }
    unsigned lds = 0;
    if (c->eos_mode == NMMA_MM_EOS_SINGLE) lds += 3u * npad * 8u;
    if (c->jet == NMMA_MM_JET_POWERLAW) lds += mmc::ROWS * mmc::YSTRIDE * 8u;

    NM_HIP(hipSetDevice(c->device));
    auto* h = new nmma_mm_handle();
    h->device = c->device;
    h->lds = lds;
    h->min_ld_out = min_ld_out;
    MmDev& P = h->dev;
    P.D = D; P.mass_mode = c->mass_mode; P.redshift_mode = c->redshift_mode; P.n_cosmo = c->n_cosmo; P.eos_mode = c->eos_mode;
    P.n_eos = tables ? c->n_eos : 0; P.npad = npad; P.fits = c->fits ? 1 : 0; P.spin_mode = c->spin_mode; P.jet = c->jet;
    P.wing_is_angle = c->wing_is_angle ? 1 : 0;
    P.mass_a = c->mass_a; P.mass_b = c->mass_b; P.redshift = c->redshift; P.lumdist = c->luminosity_distance; P.eos = c->eos;
    P.lambda_1 = c->lambda_1; P.lambda_2 = c->lambda_2; P.tov = c->tov_mass; P.radius_1 = c->radius_1; P.radius_2 = c->radius_2; P.r16 = c->r_16;
    P.alpha = c->alpha; P.zeta = c->ratio_zeta; P.spin_a = c->spin_a; P.spin_b = c->spin_b; P.eps = c->ratio_epsilon; P.theta_core = c->theta_core;
    P.wing = c->wing; P.b = c->b;
    P.log10_msun_erg = std::log10(mm::kMsunCgs * (mm::kCCgs * mm::kCCgs));      // np.log10(msun_to_ergs), nmma/core/constants.py
    for (int k = 0; k < NMMA_MM_N_OUTPUTS; ++k) P.out_col[k] = c->out_col[k];
    std::vector<double> dg, zg;
    if (c->redshift_mode == NMMA_Z_GRID) { dg.assign(c->dist_grid, c->dist_grid + c->n_cosmo); zg.assign(c->z_grid, c->z_grid + c->n_cosmo); }
    const std::vector<int> zero_status(1, 0);
    const int* status = nullptr;
#define NM_MM_UP(vec, field)                                                                              \
    do {                                                                                                  \
        const hipError_t _e = mm_upload(vec, &field, h->owned);                                           \
        if (_e != hipSuccess) {                                                                           \
            nmma_mm_destroy(h);                                                                           \
            return fail(std::string("nmma_mm_create: upload " #field " failed: ") + hipGetErrorString(_e)); \
        }                                                                                                 \
    } while (0)
    NM_MM_UP(dg, P.dist_grid); NM_MM_UP(zg, P.z_grid);
    NM_MM_UP(tm, P.t_mass); NM_MM_UP(tr, P.t_radius); NM_MM_UP(tl, P.t_loglam); NM_MM_UP(tn, P.t_n);
    NM_MM_UP(tov, P.t_tov); NM_MM_UP(r14, P.t_r14); NM_MM_UP(r16, P.t_r16);
    NM_MM_UP(zero_status, status);
#undef NM_MM_UP
    P.status = const_cast<int*>(status);
    *out = h;
    return 0;
}

int32_t nmma_mm_convert(nmma_mm_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* out_dev, int64_t ld_out, void* stream) {
    if (!h) return fail("nmma_mm_convert: null handle");
    if (B < 0) return fail("nmma_mm_convert: negative batch");
    if (B == 0) return 0;
    if (!theta_dev || !out_dev) return fail("nmma_mm_convert: null buffer");
    if (ld < h->dev.D) return fail("nmma_mm_convert: leading dimension smaller than n_dim");
    if (ld_out < h->min_ld_out) return fail("nmma_mm_convert: ld_out does not hold the sampled and the derived columns");
    const int64_t wgs = (B + mmc::ROWS - 1) / mmc::ROWS;
    if (wgs > 0x7fffffffLL) return fail("nmma_mm_convert: batch too large");
    NM_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(mm_convert, dim3((unsigned)wgs), dim3(256), h->lds, static_cast<hipStream_t>(stream), h->dev, theta_dev, (long)B, (long)ld,
                       out_dev, (long)ld_out);
    NM_HIP(hipGetLastError());
    return 0;
}

int32_t nmma_mm_status(nmma_mm_handle* h) {
    if (!h) return -1;
    int bits = 0;
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(&bits, h->dev.status, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (bits != 0 && hipMemset(h->dev.status, 0, sizeof(int)) != hipSuccess) return -1;
    return bits;
}

}  // extern "C"
