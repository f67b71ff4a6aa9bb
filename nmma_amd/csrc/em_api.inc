// em_api.inc -- host side of libnmma_hip.so: builds the device tables once
// (nmma_em_create) and launches the kernels.  Included at the end of em_kernels.hip.
#include <chrono>
#include <cstdio>

namespace nmma {

static thread_local std::string g_last_error;

int fail(const std::string& msg) {      // (shared with the other units through nmma_common.h)
    g_last_error = msg;
    return 1;
}

thread_local std::string g_launch_note;      // (declared in em_host.h)

// stack2_redo's LDS geometry (em_lc_loglike's layout for two sets, launch_lc_loglike): decided at create -- a handle whose
// re-evaluation kernel cannot stage one sample's curves has no one-launch form (nmma_em_loglike_stack2 returns 2).
struct Stack2RedoGeo { bool fits, fits32; int stage_dat, slab, lds_lc; };
static Stack2RedoGeo stack2_redo_geometry(const nmma::EmDev& P) {
    using namespace nmma;
    Stack2RedoGeo g{};
    const bool cosmo_lds = P.redshift_mode == NMMA_Z_GRID && P.n_cosmo <= STAGE_COSMO;
    const int grid_bytes = ((P.NS + (cosmo_lds ? 2 * P.n_cosmo : 0)) * 8 + 15) & ~15;
    g.stage_dat = (P.n_data <= 1024) ? 1 : 0;
    const int shared_bytes = g.stage_dat ? ((grid_bytes + 5 * P.n_data * 8 + ((P.n_data + 3) & ~3) * 4 + P.n_items * ITEM_WORDS * 4 + 15) & ~15) : grid_bytes;
    const int base = (P.NS + P.lc_nf_max + 16) * 8;
    g.slab = base + P.M * P.NS * 8;
    const int tab = !(g.stage_dat && shared_bytes - grid_bytes >= STACK2_LDS_BYTES) ? STACK2_LDS_BYTES : 0;
    g.fits32 = g.stage_dat && shared_bytes + 8 * g.slab + tab <= 40 * 1024;
    g.fits = shared_bytes + 4 * g.slab + tab <= LDS_DYNAMIC_MAX;      // (a rarely needed kernel: one workgroup per CU is fine -- em_lc_loglike itself stops at 64 KiB)
    g.lds_lc = shared_bytes + (g.fits32 ? 8 : 4) * g.slab + tab;
    return g;
}

template <typename T>
static hipError_t upload(const std::vector<T>& v, const T** dst, std::vector<void*>& owned) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (!v.empty()) {
        e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    *dst = reinterpret_cast<const T*>(p);
    return hipSuccess;
}

}  // namespace nmma

namespace nmma {

// Extinction magnitudes of the whole batch (Pei 1992 law, lean task): ext_prepass_kernel on the launch stream, before em_logl.
static hipError_t ext_prepass(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, hipStream_t s) {
    if (!h->dev.p92_tab) return hipSuccess;
    {
        // extinction magnitudes of the whole batch first (ext_prepass_kernel), on the same stream
        if (h->ext_cap < B) {
            if (h->ext_ws) (void)hipFree(h->ext_ws);
            h->ext_ws = nullptr; h->ext_cap = 0;
            const int64_t cap = std::max<int64_t>(B, 4096);
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->ext_ws), (size_t)cap * h->dev.M * sizeof(double));
            if (e != hipSuccess) return e;
            h->ext_cap = cap;
            h->dev.ext_tab = h->ext_ws;
            e = hipMemcpy(h->dev_d, &h->dev, sizeof(EmDev), hipMemcpyHostToDevice);     // (rare: only when the batch grows)
            if (e != hipSuccess) return e;
            if (h->band_dev_d) {
                for (EmDev& Pb : h->band_dev) Pb.ext_tab = h->ext_ws;
                e = hipMemcpy(h->band_dev_d, h->band_dev.data(), h->band_dev.size() * sizeof(EmDev), hipMemcpyHostToDevice);
                if (e != hipSuccess) return e;
            }
        }
        hipLaunchKernelGGL(ext_prepass_kernel, dim3((unsigned)((B * h->dev.M + 255) / 256)), dim3(256), 0, s, h->dev_d, theta, (long)B, (long)ld,
                           h->ext_ws);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { g_launch_note = "ext_prepass_kernel"; return e; }
    }
    return hipSuccess;
}

static hipError_t launch_logl(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, double* out,
                              double* chi, double* gp, hipStream_t s) {
    { const hipError_t e = ext_prepass(h, theta, B, ld, s); if (e != hipSuccess) return e; }
    // wave split: 8 MFMA-role + 8 likelihood-role waves for the fast modes (measured best for both tile sizes in
    // round 1), 4 + 8 for the generic item phase (its register budget)
    const int R = choose_r(h, B), KP = h->dev.KP;
#ifdef NMMA_DEV_HEADLINE_ONLY      // development builds: only the BASELINE config-2 instantiation (seconds instead of minutes)
#ifndef NMMA_DEV_FASTM             // (or one other task flavour: -DNMMA_DEV_FASTM=3 ...)
#define NMMA_DEV_FASTM 1
#endif
    if (R == 1 && KP == 1 && (NMMA_DEV_FASTM != 1 || (h->dev.all_fast == 1 && !h->dev.lean_x)))
        return launch_logl_one<1, 1, NMMA_DEV_FASTM ? 8 : 4, 8, NMMA_DEV_FASTM>(h, theta, B, ld, out, chi, gp, s);
    g_last_error = "development build: only em_logl<1,1,8,8,1> is compiled in";
    return hipErrorInvalidValue;
#else
#define NM_LOGL(RR)                                                                                  \
    do {                                                                                             \
        if (h->dev.all_fast == 2)                                                                    \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 2>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 2>(h, theta, B, ld, out, chi, gp, s);      \
        if (h->dev.all_fast == 1 && h->dev.dense && h->dense_plain)                                  \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 9>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 9>(h, theta, B, ld, out, chi, gp, s);      \
        if (h->dev.all_fast == 1 && h->dev.dense)                                                    \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 6>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 6>(h, theta, B, ld, out, chi, gp, s);      \
        if (h->dev.all_fast && h->dev.lean_gen)                                                      \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 5>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 5>(h, theta, B, ld, out, chi, gp, s);      \
        if (h->dev.all_fast && h->dev.lean_x && !h->dev.st_uniform)                                  \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 4>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 4>(h, theta, B, ld, out, chi, gp, s);      \
        if (h->dev.all_fast && h->dev.lean_x)                                                        \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 3>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 3>(h, theta, B, ld, out, chi, gp, s);      \
        if (h->dev.all_fast)                                                                         \
            return KP == 1 ? launch_logl_one<RR, 1, 8, 8, 1>(h, theta, B, ld, out, chi, gp, s)       \
                           : launch_logl_one<RR, 2, 8, 8, 1>(h, theta, B, ld, out, chi, gp, s);      \
        return KP == 1 ? launch_logl_one<RR, 1, 4, 8, 0>(h, theta, B, ld, out, chi, gp, s)           \
                       : launch_logl_one<RR, 2, 4, 8, 0>(h, theta, B, ld, out, chi, gp, s);          \
    } while (0)
    if (R == 2) NM_LOGL(2);
    NM_LOGL(1);
#undef NM_LOGL
#endif
}

template <int MODE, int KP>
static hipError_t launch_aux_one(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, float* coeff,
                                 double* tobs, double* mag, hipStream_t s) {
    constexpr int R = 2, WPB = 4;
    const EmDev& P = h->dev;
    const LdsOff L = lds_layout(MODE, R, P.NC, P.NT, P.NS);
    const int TS = 16 * R;
    const dim3 grid((unsigned)((B + TS - 1) / TS), (unsigned)P.M);
    h->g_x = grid.x; h->g_y = grid.y; h->g_block = 64 * WPB; h->g_tile = TS; h->g_lds = L.total;
    hipLaunchKernelGGL((em_fused<MODE, R, WPB, KP>), grid, dim3(64 * WPB), L.total, s, h->dev_d, theta, (long)B,
                       (long)ld, L, coeff, tobs, mag);
    return hipGetLastError();
}

static hipError_t launch_aux(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, int mode, float* coeff,
                             double* tobs, double* mag, hipStream_t s) {
    const int KP = h->dev.KP;
    if (mode == MODE_COEFF)
        return KP == 1 ? launch_aux_one<MODE_COEFF, 1>(h, theta, B, ld, coeff, tobs, mag, s)
                       : launch_aux_one<MODE_COEFF, 2>(h, theta, B, ld, coeff, tobs, mag, s);
    if (mode == MODE_LC_ABS)
        return KP == 1 ? launch_aux_one<MODE_LC_ABS, 1>(h, theta, B, ld, coeff, tobs, mag, s)
                       : launch_aux_one<MODE_LC_ABS, 2>(h, theta, B, ld, coeff, tobs, mag, s);
    return KP == 1 ? launch_aux_one<MODE_LC, 1>(h, theta, B, ld, coeff, tobs, mag, s)
                   : launch_aux_one<MODE_LC, 2>(h, theta, B, ld, coeff, tobs, mag, s);
}

}  // namespace nmma

using namespace nmma;

extern "C" {

int32_t nmma_abi_version(void) { return NMMA_ABI_VERSION; }

const char* nmma_build_info(void) {
    return "libnmma_hip gfx950 (hipcc, -ffp-contract=off); kernels: em_logl<R,KP,NMW,NVW,FASTM>, em_fused<MODE,R,WPB,KP>";
}

const char* nmma_last_error(void) { return g_last_error.c_str(); }

int32_t nmma_em_create(const nmma_em_config* c, nmma_em_handle** out) {
    if (!c || !out) return fail("nmma_em_create: null argument");
    *out = nullptr;
    if (c->abi_version != NMMA_ABI_VERSION) return fail("nmma_em_create: ABI version mismatch");
    const int M = c->n_model_filters, NP = c->n_params, NH = c->n_hidden, NC = c->n_coeff, NT = c->n_tt;
    const int O = c->n_obs_filters, D = c->n_dim;
    const bool svd = c->model_kind == NMMA_MODEL_SVD;
    std::vector<unsigned char> tab_host;     // host copy of EmDev::tab (the per-item tables of item-staged photometry are cut from it)
    // the lean tasks' table on the SAMPLE grid, stage-1 lerp folded into the rows (built where the task flavour is decided)
    std::vector<unsigned char> ltab_host;
    bool fold = false;
    int fold_bytes = 0, fold_off_b2 = 0, unfold_tab_bytes = 0, unfold_off_b2 = 0;
    if (c->model_kind < NMMA_MODEL_SVD || c->model_kind > NMMA_MODEL_HONA2020) return fail("nmma_em_create: bad model_kind");
    if (M < 1 || NP < 0 || NP > NMMA_MAX_PARAMS) return fail("nmma_em_create: bad model dimensions");
    if (svd && (NP < 1 || NH < 1 || NC < 1 || NC > NMMA_MAX_COEFF || NT < 2))
        return fail("nmma_em_create: bad surrogate dimensions");
    if (O < 0 || D < 1) return fail("nmma_em_create: bad data dimensions");
    if (svd && (!c->W1 || !c->b1 || !c->W2 || !c->b2 || !c->VA || !c->mins || !c->maxs || !c->tt || !c->param_mins ||
                !c->param_maxs))
        return fail("nmma_em_create: null surrogate tensor");
    if (!svd && (c->n_sample_times < 2 || !c->sample_times)) return fail("nmma_em_create: sample_times required");
    // combined model on a union grid: the surrogate's own sample_times next to the combination's (nmma_hip.h)
    const bool union_grid = c->n_base_times > 0;
    bool union_basis_finite = true;
    bool comb_lim = false;       // a combination's handle whose bands have finite detection limits / time-node systematics (and no averaged band)
    if (c->n_base_times < 0 || (union_grid && (!c->base_times || c->n_base_times < 2)))
        return fail("nmma_em_create: base_times must hold at least two times");
    if (union_grid && (!svd || !c->stack_operands || c->n_sample_times < 2 || !c->sample_times))
        return fail("nmma_em_create: base_times (a combined model on a union grid) needs an SVD surrogate handle with stack_operands = 1 and "
                    "the combination's sample_times");
    // model filters the surrogate has nothing for (calc_svd_lc's null output, lightcurve_generation.py:168-169): +inf on every node
    std::vector<char> null_m(M > 0 ? M : 1, 0);
    bool any_null = false;
    if (c->null_filters)
        for (int m = 0; m < M; ++m) if (c->null_filters[m]) { null_m[m] = 1; any_null = true; }
    if (any_null && (!svd || !c->stack_operands))
        return fail("nmma_em_create: null_filters (model filters without a surrogate) need an SVD surrogate handle with stack_operands = 1: "
                    "outside a combination such a band floors every sample");
    if (c->model_kind == NMMA_MODEL_ME2017 && (!c->filter_nu0 || NP != 4))
        return fail("nmma_em_create: Me2017 needs filter_nu0 and its 4 parameters (log10_mej, log10_vej, beta, log10_kappa_r)");
    if (c->model_kind == NMMA_MODEL_PIRO2021) {
        if (!c->filter_nu0 || NP != 3)
            return fail("nmma_em_create: Piro2021 needs filter_nu0 and its 3 parameters (log10_Menv, log10_Renv, log10_Ee)");
        for (int j = 0; j < c->n_sample_times; ++j)       // (the model divides by t: sc_bol_lc, lightcurve_generation.py:333-346)
            if (!(c->sample_times[j] > 0.0)) return fail("nmma_em_create: Piro2021 needs every sample time > 0");
    }
    if (c->model_kind == NMMA_MODEL_HONA2020) {
        if (!c->filter_nu0 || NP != 6)
            return fail("nmma_em_create: HoNa2020 needs filter_nu0 and its 6 parameters (log10_mej, vej_max, vej_min, vej_frac, "
                        "log10_kappa_low_vej, log10_kappa_high_vej)");
        // what the reference or scipy would refuse: the integration runs from the first node to the last with a first step of 0.05 d
        // (solve_ivp: "first_step exceeds bounds"), the spline's and np.interp's abscissae ascend, the model starts at 0.05 d
        const int n = c->n_sample_times;
        for (int j = 0; j < n; ++j)
            if (!(c->sample_times[j] >= 0.05) || (j > 0 && !(c->sample_times[j] > c->sample_times[j - 1])))
                return fail("nmma_em_create: HoNa2020 needs strictly ascending sample times, none below 0.05 d");
        if (!(c->sample_times[n - 1] * 86400.0 - c->sample_times[0] * 86400.0 > 0.05 * 86400.0))
            return fail("nmma_em_create: HoNa2020 needs sample times that span more than the integrator's first step of 0.05 d");
    }
    if (c->redshift_mode == NMMA_Z_GRID && (c->n_cosmo < 2 || !c->dist_grid || !c->z_grid))
        return fail("nmma_em_create: redshift grid missing");
    auto slot_ok = [&](const nmma_slot& s) { return s.col < D && s.op >= 0 && s.op <= NMMA_OP_ACOS; };
    for (int p = 0; p < NP; ++p)
        if (!slot_ok(c->model_param[p])) return fail("nmma_em_create: model_param slot out of range");
    if (!slot_ok(c->luminosity_distance) || !slot_ok(c->redshift) || !slot_ok(c->timeshift) || !slot_ok(c->ebv))
        return fail("nmma_em_create: slot out of range");

    int ndev = 0;
    NM_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail("nmma_em_create: no HIP device (this library has no CPU fallback)");
    if (c->device < 0 || c->device >= ndev) return fail("nmma_em_create: bad device ordinal");
    NM_HIP(hipSetDevice(c->device));

    auto* h = new nmma_em_handle();
    h->device = c->device;
    h->stack2_only = union_grid || any_null;
    EmDev& P = h->dev;
    P.M = M; P.NP = NP; P.KP = (NP + 3) / 4; P.NC = NC; P.NT = NT; P.D = D; P.O = O;
    // records per slice must be a multiple of the deepest prefetch ring (8)
    const int HB = ((NH + 15) / 16 + NSLICE * 8 - 1) / (NSLICE * 8) * (NSLICE * 8);
    P.HB = HB; P.NH_pad = HB * 16;
    P.n_cosmo = c->n_cosmo; P.redshift_mode = c->redshift_mode;
    P.has_h0 = (c->redshift_mode == NMMA_Z_GRID && c->hubble_reference > 0) ? 1 : 0;
    P.n_bands = 1;
    P.hubble = c->hubble_constant;
    P.inv_h0_ref = P.has_h0 ? 1.0 / c->hubble_reference : 0.0;
    if (P.has_h0 && !slot_ok(c->hubble_constant)) return fail("nmma_em_create: hubble_constant slot out of range");
    if (c->extinction_law != NMMA_EXT_LINEAR && c->extinction_law != NMMA_EXT_P92_SMC_HOST)
        return fail("nmma_em_create: unknown extinction_law");
    // (a law only matters when Ebv can be non-zero: a constant-zero slot switches it off, model.py:328-330)
    const bool ebv_zero = c->ebv.col < 0 && c->ebv.value == 0.0;
    const bool p92 = c->extinction_law == NMMA_EXT_P92_SMC_HOST && !ebv_zero;
    if (p92 && !c->filter_nu0) return fail("nmma_em_create: the P92 extinction law needs filter_nu0");
    // per model filter: A / E(B-V) for the linear law, the filter frequency for P92 (see em_math.h:extinction_mag)
    const double* ext_coeff = ebv_zero ? nullptr : (p92 ? c->filter_nu0 : c->ebv_coeff);
    P.has_ebv = ext_coeff != nullptr;
    P.ext_law = p92 ? NMMA_EXT_P92_SMC_HOST : NMMA_EXT_LINEAR;
    for (int p = 0; p < NMMA_MAX_PARAMS; ++p) P.model_param[p] = (p < NP) ? c->model_param[p] : nmma_slot{-1, 0, 0.0};
    P.lumdist = c->luminosity_distance; P.redshift = c->redshift; P.timeshift = c->timeshift; P.ebv = c->ebv;
    if (const char* e = getenv("NMMA_EM_RING")) { const int r = std::atoi(e); if (r >= 1 && r <= 4) h->ring_max = r; }
    if (const char* e = getenv("NMMA_EM_TILE")) {
        int r = 0, w = 0;
        if (sscanf(e, "%d,%d", &r, &w) >= 1) { h->force_r = r; h->force_wpb = w; }
    }
    P.prio_valu = 3; P.prio_mfma = 0;
    P.helpers = 1;
    if (const char* e = getenv("NMMA_EM_HELPERS")) P.helpers = atoi(e) != 0;
    if (const char* e = getenv("NMMA_EM_PRIO")) { int v = 3, m = 0; if (sscanf(e, "%d,%d", &v, &m) >= 1) { P.prio_valu = v; P.prio_mfma = m; } }

#define NM_UP(vec, field)                                                                     \
    do {                                                                                      \
        hipError_t _e = upload(vec, &P.field, h->owned);                                      \
        if (_e != hipSuccess) {                                                               \
            nmma_em_destroy(h);                                                               \
            return fail(std::string("upload " #field " failed: ") + hipGetErrorString(_e));   \
        }                                                                                     \
    } while (0)

    P.model_kind = c->model_kind;
    // ---- pre-swizzled weight records (see em_device.h)
    if (svd) {
        const int KP = P.KP, RECF = rec_floats(KP);
        std::vector<float> wrec((size_t)M * (HB + NPAD_REC) * RECF, 0.f);
        for (int m = 0; m < M; ++m) {
            const float* W1 = c->W1 + (size_t)m * NP * NH;
            const float* b1 = c->b1 + (size_t)m * NH;
            const float* W2 = c->W2 + (size_t)m * NH * NC;
            for (int hb = 0; hb < HB; ++hb) {
                float* r = wrec.data() + ((size_t)m * (HB + NPAD_REC) + hb) * RECF;
                for (int l = 0; l < 64; ++l) {
                    for (int q = 0; q < 4; ++q) {
                        const int hid = hb * 16 + (l >> 4) * 4 + q, coef = l & 15;
                        r[l * 4 + q] = (hid < NH && coef < NC) ? W2[(size_t)hid * NC + coef] : 0.f;
                    }
                    for (int kp = 0; kp < KP; ++kp) {
                        const int p = 4 * kp + (l >> 4), hid = hb * 16 + (l & 15);
                        r[256 + kp * 64 + l] = (p < NP && hid < NH) ? W1[(size_t)p * NH + hid] : 0.f;
                    }
                }
                for (int i = 0; i < 16; ++i) {
                    const int hid = hb * 16 + i;
                    r[256 + 64 * KP + i] = hid < NH ? b1[hid] : 0.f;
                }
            }
        }
        NM_UP(wrec, wrec);
        P.wrec_bytes = (int32_t)(wrec.size() * sizeof(float));
        std::vector<float> b2((size_t)M * 16, 0.f);
        for (int m = 0; m < M; ++m)
            for (int j = 0; j < NC; ++j) b2[m * 16 + j] = c->b2[m * NC + j];
        NM_UP(b2, b2);
    }
    // ---- SVD basis, transposed; spans
    if (svd) {
        std::vector<double> VAt((size_t)M * NC * NT), span((size_t)M * NT), mins(c->mins, c->mins + (size_t)M * NT);
        for (int m = 0; m < M; ++m)
            for (int t = 0; t < NT; ++t) {
                for (int j = 0; j < NC; ++j) VAt[((size_t)m * NC + j) * NT + t] = c->VA[((size_t)m * NT + t) * NC + j];
                span[(size_t)m * NT + t] = c->maxs[(size_t)m * NT + t] - c->mins[(size_t)m * NT + t];
            }
        NM_UP(VAt, VAt); NM_UP(span, span); NM_UP(mins, mins);
        std::vector<double> VArow(c->VA, c->VA + (size_t)M * NT * NC);
        NM_UP(VArow, VA);
        std::vector<double> pmin(c->param_mins, c->param_mins + (size_t)M * NP), pspan((size_t)M * NP);
        for (size_t i = 0; i < pspan.size(); ++i) pspan[i] = c->param_maxs[i] - c->param_mins[i];
        std::vector<double> pinv(pspan.size());
        for (size_t i = 0; i < pspan.size(); ++i) pinv[i] = 1.0 / pspan[i];
        NM_UP(pmin, pmin); NM_UP(pspan, pspan); NM_UP(pinv, pinv);
        std::vector<double> ebvc(M, 0.0);
        if (ext_coeff) ebvc.assign(ext_coeff, ext_coeff + M);
        NM_UP(ebvc, ebv_coeff);
    }
    if (!svd) {
        // models evaluated directly on sample_times: no stage-1 interpolation, no LDS tables
        const int NS = c->n_sample_times;
        P.NS = NS;
        std::vector<double> st(c->sample_times, c->sample_times + NS);
        for (int j = 1; j < NS; ++j)
            if (!(st[j] > st[j - 1])) { nmma_em_destroy(h); return fail("nmma_em_create: sample_times must increase"); }
        NM_UP(st, st);
        h->st_host = st;
        for (int m = 0; m < M; ++m) { h->same_grid.push_back(1); h->ranges.insert(h->ranges.end(), {0, NS - 1, 1, NS}); }
        std::vector<double> nu0(M, 0.0), ebvc(M, 0.0);
        if (c->filter_nu0) nu0.assign(c->filter_nu0, c->filter_nu0 + M);
        if (ext_coeff) ebvc.assign(ext_coeff, ext_coeff + M);
        NM_UP(nu0, nu0); NM_UP(ebvc, ebv_coeff);
    }
    // ---- stage-1 tables: np.interp(sample_times, tt, mag, left=right=inf) (utils.py:642-645)
    if (svd) {
        const int NS = c->n_sample_times > 0 ? c->n_sample_times : NT;
        P.NS = NS;
        std::vector<double> st(NS);
        for (int j = 0; j < NS; ++j) st[j] = c->n_sample_times > 0 ? c->sample_times[j] : c->tt[j];
        for (int j = 1; j < NS; ++j)
            if (!(st[j] > st[j - 1])) { nmma_em_destroy(h); return fail("nmma_em_create: sample_times must increase"); }
        {   // equally spaced grid?  (only used to seed the bracket search)
            const double dt0 = (st[NS - 1] - st[0]) / (NS - 1);
            bool uni = NS >= 2 && dt0 > 0;
            for (int j = 0; j < NS && uni; ++j)
                // (the uniform tasks take the node spacing -- and the dense task a datum's position inside its interval -- from st0 and
                //  dt0: a grid that is only roughly equally spaced takes the table-driven tasks; np.arange / np.linspace are exact to 1e-15)
                if (std::fabs(st[j] - (st[0] + j * dt0)) > 1e-11 * dt0) uni = false;
            P.st_uniform = uni ? 1 : 0;
            P.st0 = st[0];
            P.st_inv_dt = uni ? 1.0 / dt0 : 0.0;
            // unequal spacing: lookup over BG_CELLS equal cells that narrows the lean tasks' bracket search (em_device.h)
            P.bguess = nullptr; P.bg_inv_h = 0.0; P.bg_nbis = 0;
            if (!uni && NS >= 2) {
                const double hcell = (st[NS - 1] - st[0]) / BG_CELLS;
                std::vector<int32_t> bg(BG_CELLS + 1, 0);
                int j = 0, widest = 1;
                for (int q = 0; q <= BG_CELLS; ++q) {
                    const double left = q < BG_CELLS ? st[0] + q * hcell : st[NS - 1];
                    while (j + 1 < NS && st[j + 1] <= left) ++j;
                    bg[q] = j;
                }
                bg[BG_CELLS] = NS - 1;
                for (int q = 0; q < BG_CELLS; ++q) widest = std::max(widest, bg[q + 1] + 2 - (bg[q] - 1));   // search range incl. the slack
                int nb = 0;
                while ((1 << nb) < widest) ++nb;
                P.bg_inv_h = 1.0 / hcell;
                P.bg_nbis = nb;
                NM_UP(bg, bguess);
            }
        }
        std::vector<int32_t> idx((size_t)M * NS), range((size_t)M * 4);
        std::vector<double> dx((size_t)M * NS, 1.0), off((size_t)M * NS, 0.0);
        // Combined model on a UNION grid (nmma_em_config::base_times): the surrogate's own sample_times bt[NB] against the SVD grid
        // (b_*: stage 1, as idx / dx / off below), then the handle's grid against bt (u_*: autocomplete_data(..., extrapolate=inf),
        // model.py:1440-1448 -- np.interp over the surrogate's finite nodes, +inf outside them).  idx / dx / off / range then describe
        // a stage-1 map nobody evaluates: the ranges are replaced by the window of the two-hop map.
        const int NB = union_grid ? c->n_base_times : 0;
        std::vector<int32_t> b_idx((size_t)M * std::max(NB, 1), -1), u_idx((size_t)M * NS, -1);
        std::vector<double> b_dx((size_t)M * std::max(NB, 1), 1.0), b_off((size_t)M * std::max(NB, 1), 0.0), u_dx((size_t)M * NS, 1.0), u_off((size_t)M * NS, 0.0);
        std::vector<int32_t> u_range((size_t)M * 4, 0);
        if (union_grid) {
            const double* bt = c->base_times;
            for (int i = 1; i < NB; ++i)
                if (!(bt[i] > bt[i - 1])) { nmma_em_destroy(h); return fail("nmma_em_create: base_times must increase"); }
            for (int m = 0; m < M; ++m) {
                const double* tt = c->tt + (size_t)m * NT;
                int ilo = -1, ihi = -1;
                for (int i = 0; i < NB; ++i) {
                    const double x = bt[i];
                    if (!(x >= tt[0] && x <= tt[NT - 1])) continue;
                    const int a = (int)(std::upper_bound(tt, tt + NT, x) - tt) - 1;
                    b_idx[(size_t)m * NB + i] = a;
                    if (a < NT - 1) { b_dx[(size_t)m * NB + i] = tt[a + 1] - tt[a]; b_off[(size_t)m * NB + i] = x - tt[a]; }
                    if (ilo < 0) ilo = i;
                    ihi = i;
                }
                // (the nodes of bt inside [tt[0], tt[NT-1]] are contiguous: ilo .. ihi)
                int jlo = -1, jhi = -1, nfin = 0;
                if (ilo >= 0 && ihi > ilo)
                    for (int j = 0; j < NS; ++j) {
                        const double x = st[j];
                        if (!(x >= bt[ilo] && x <= bt[ihi])) continue;
                        int i = (int)(std::upper_bound(bt + ilo, bt + ihi + 1, x) - bt) - 1;
                        if (i >= ihi) i = ihi - 1;                  // x == bt[ihi]: np.interp returns fp[-1]; as a lerp with fraction 1 below
                        u_idx[(size_t)m * NS + j] = i;
                        u_dx[(size_t)m * NS + j] = bt[i + 1] - bt[i];
                        u_off[(size_t)m * NS + j] = x - bt[i];
                        if (x == bt[i + 1]) { u_idx[(size_t)m * NS + j] = i + 1; u_off[(size_t)m * NS + j] = 0.0; if (i + 2 <= ihi) u_dx[(size_t)m * NS + j] = bt[i + 2] - bt[i + 1]; }
                        if (jlo < 0) jlo = j;
                        jhi = j;
                        ++nfin;
                    }
                if (null_m[m]) {              // no value anywhere: an empty window for the curve outputs, no row of the fold below
                    for (int j = 0; j < NS; ++j) u_idx[(size_t)m * NS + j] = -1;
                    jlo = jhi = 0; nfin = 0;
                } else if (nfin < 2) {
                    h->always_floor = 1;       // sanity_check fails for every sample: the surrogate has fewer than two finite nodes
                    if (jlo < 0) jlo = jhi = 0;
                    jhi = jlo;
                }
                u_range[m * 4 + 0] = jlo; u_range[m * 4 + 1] = jhi; u_range[m * 4 + 2] = 0; u_range[m * 4 + 3] = nfin;
            }
        }
        for (int m = 0; m < M; ++m) {
            const double* tt = c->tt + (size_t)m * NT;
            int jlo = -1, jhi = -1, nfin = 0, ident = 1;
            for (int j = 0; j < NS; ++j) {
                const double x = st[j];
                int i = -1;
                if (x >= tt[0] && x <= tt[NT - 1]) {
                    i = (int)(std::upper_bound(tt, tt + NT, x) - tt) - 1;
                    if (i < NT - 1) {
                        dx[(size_t)m * NS + j] = tt[i + 1] - tt[i];
                        off[(size_t)m * NS + j] = x - tt[i];
                        if (off[(size_t)m * NS + j] != 0.0) ident = 0;
                    }
                    if (jlo < 0) jlo = j;
                    jhi = j;
                    ++nfin;
                }
                idx[(size_t)m * NS + j] = i;
            }
            if (nfin < 2 || jhi - jlo + 1 != nfin) {
                if (!union_grid && !null_m[m]) h->always_floor = 1;   // sanity_check fails for every sample (em_likelihood.py:305-311)
                if (jlo < 0) jlo = jhi = 0;
                if (nfin < 2) jhi = jlo;
            }
            // (a null filter: the curve outputs see an empty window -- +inf everywhere -- while the flavour decisions below see the
            //  grid relation of its placeholder tt, the other filters' own)
            range[m * 4 + 0] = null_m[m] ? 0 : jlo; range[m * 4 + 1] = null_m[m] ? 0 : jhi; range[m * 4 + 2] = ident; range[m * 4 + 3] = null_m[m] ? 0 : nfin;
            int same = 1;
            for (int j = jlo; j <= jhi && j < NS; ++j) if (idx[(size_t)m * NS + j] != j) same = 0;
            if (union_grid) {       // the window of the two-hop map; never "the SVD grid itself"
                for (int q = 0; q < 4; ++q) range[m * 4 + q] = u_range[m * 4 + q];
                jlo = u_range[m * 4 + 0]; jhi = u_range[m * 4 + 1]; ident = 0; nfin = u_range[m * 4 + 3];
                same = 0;
            }
            h->same_grid.push_back(same);
            h->ranges.insert(h->ranges.end(), {jlo, jhi, ident, nfin});
        }
        // sanity_check looks at EVERY model filter's light curve (em_likelihood.py:305-311; model.py:381-404: fewer than two
        // finite nodes make the curve all-inf): with finite coefficients a node is finite iff its basis row, span and offset are
        for (int m = 0; m < M; ++m) {
            int n_ok = 0;
            auto node_ok = [&](int ii) {
                bool ok = std::isfinite(c->mins[(size_t)m * NT + ii]) && std::isfinite(c->maxs[(size_t)m * NT + ii]);
                for (int q = 0; q < NC && ok; ++q) ok = std::isfinite(c->VA[((size_t)m * NT + ii) * NC + q]);
                return ok;
            };
            if (null_m[m]) continue;         // (nothing to check: the band's curve is the second transient's)
            if (union_grid) {
                // (the surrogate's own nodes; the handle's grid contains them -- it is the union -- or sees lerps between them.  A basis
                //  with non-finite entries on a union grid is not sorted out node by node: such a handle has no one-launch form)
                for (int i = 0; i < NB; ++i) {
                    const int a = b_idx[(size_t)m * NB + i];
                    if (a < 0) continue;
                    bool ok = node_ok(a);
                    if (ok && a < NT - 1 && b_off[(size_t)m * NB + i] != 0.0) ok = node_ok(a + 1);
                    n_ok += ok ? 1 : 0;
                    if (!ok) union_basis_finite = false;
                }
                if (n_ok < 2) h->always_floor = 1;
                continue;
            }
            for (int j = 0; j < NS; ++j) {
                const int i = idx[(size_t)m * NS + j];
                if (i < 0) continue;
                bool ok = node_ok(i);
                if (ok && i < NT - 1 && off[(size_t)m * NS + j] != 0.0) ok = node_ok(i + 1);
                n_ok += ok ? 1 : 0;
            }
            if (n_ok < 2) h->always_floor = 1;
        }
        NM_UP(st, st); NM_UP(idx, s1_idx); NM_UP(dx, s1_dx); NM_UP(off, s1_off); NM_UP(range, s1_range);
        h->st_host = st;
        P.union_grid = union_grid ? 1 : 0; P.NB = NB;
        if (union_grid) {
            std::vector<double> btv(c->base_times, c->base_times + NB);
            NM_UP(btv, bt); NM_UP(b_idx, b_idx); NM_UP(b_dx, b_dx); NM_UP(b_off, b_off); NM_UP(u_idx, u_idx); NM_UP(u_dx, u_dx); NM_UP(u_off, u_off);
            h->u_idx = u_idx; h->u_dx = u_dx; h->u_off = u_off; h->b_idx = b_idx; h->b_dx = b_dx; h->b_off = b_off;
        }
        // packed tables for em_logl (see em_device.h)
        {
            const int RS = (NC + 2 + 1) & ~1;
            const int o_b2 = NT * RS * 8;                       // right behind the rows: the fast path stages rows + b2 only
            const int o_dx = o_b2 + 16 * 4;
            const int o_of = o_dx + NS * 8, o_i = o_of + NS * 8;
            const int o_inv = (o_i + NS * 4 + 7) / 8 * 8;      // 1 / dx: the lean task multiplies (see DESIGN section 8)
            const int bytes = (o_inv + NS * 8 + 1023) / 1024 * 1024;
            P.tab_fast_bytes = (o_b2 + 16 * 4 + 1023) / 1024 * 1024;
            if (bytes > TAB_MAX_BYTES) {
                nmma_em_destroy(h);
                return fail("nmma_em_create: SVD grid too large for the LDS table buffer (NT*(NC+2)+2.5*NS doubles <= 5120)");
            }
            std::vector<unsigned char> tab((size_t)M * bytes, 0);
            for (int m = 0; m < M; ++m) {
                unsigned char* t = tab.data() + (size_t)m * bytes;
                for (int i = 0; i < NT; ++i) {
                    double rowbuf[NMMA_MAX_COEFF + 4] = {0};
                    for (int j = 0; j < NC; ++j) rowbuf[j] = null_m[m] ? 0.0 : c->VA[((size_t)m * NT + i) * NC + j];
                    rowbuf[NC] = null_m[m] ? 1.0 : c->maxs[(size_t)m * NT + i] - c->mins[(size_t)m * NT + i];
                    rowbuf[NC + 1] = null_m[m] ? HUGE_VAL : c->mins[(size_t)m * NT + i];      // (a null filter: [0 | 1 | +inf] -- no value on any node)
                    std::memcpy(t + (size_t)i * RS * 8, rowbuf, (size_t)RS * 8);
                }
                std::memcpy(t + o_dx, dx.data() + (size_t)m * NS, (size_t)NS * 8);
                std::memcpy(t + o_of, off.data() + (size_t)m * NS, (size_t)NS * 8);
                std::memcpy(t + o_i, idx.data() + (size_t)m * NS, (size_t)NS * 4);
                for (int j = 0; j < NS; ++j) {
                    const double inv = 1.0 / dx[(size_t)m * NS + j];
                    std::memcpy(t + o_inv + (size_t)j * 8, &inv, 8);
                }
                float b2pad[16] = {0};
                for (int j = 0; j < NC; ++j) b2pad[j] = c->b2[m * NC + j];
                std::memcpy(t + o_b2, b2pad, sizeof(b2pad));
            }
            P.tab_row_stride = RS;
            P.tab_bytes = bytes;
            P.tab_off_s1dx = o_dx; P.tab_off_s1of = o_of; P.tab_off_s1i = o_i; P.tab_off_b2 = o_b2;
            P.tab_off_s1inv = o_inv;
            NM_UP(tab, tab);
            tab_host.swap(tab);
        }
    }
    // ---- cosmology grid
    {
        std::vector<double> dg, zg;
        if (c->redshift_mode == NMMA_Z_GRID) {
            dg.assign(c->dist_grid, c->dist_grid + c->n_cosmo);
            zg.assign(c->z_grid, c->z_grid + c->n_cosmo);
            // a sampled Hubble constant: the device interpolates z / d_L (see sample_scalars)
            if (P.has_h0)
                for (int i = 0; i < c->n_cosmo; ++i) {
                    if (!(dg[i] > 0)) { nmma_em_destroy(h); return fail("nmma_em_create: dist_grid must be positive with a sampled Hubble constant"); }
                    zg[i] /= dg[i];
                }
        }
        NM_UP(dg, dist_grid); NM_UP(zg, z_grid);
    }
    // ---- photometry + systematics
    {
        std::vector<int32_t> doff(O + 1, 0);
        for (int o = 0; o <= O; ++o) doff[o] = O > 0 ? c->data_offsets[o] : 0;
        const int N = O > 0 ? doff[O] : 0;
        h->n_obs_total = N;
        std::vector<double> dt(N), dm(N), dsig(N), dsigtot(N, 0.0), dlogsig(N, 0.0), dinvsig(N, 0.0), lim(O), sconst(O, 0.0);
        std::vector<int32_t> nsrc(O), src((size_t)O * NMMA_MAX_SOURCES, 0), group(O), kind(O), snn(O), soff(O + 1, 0);
        std::vector<int32_t> nidx(N, 0);
        std::vector<double> ndx(N, 1.0), noff(N, 0.0);
        std::vector<nmma_slot> slots;
        std::vector<double> node_t;          // node time per slot (0 for single parameters)
        if (N > 0) {
            std::copy(c->data_times, c->data_times + N, dt.begin());
            std::copy(c->data_mags, c->data_mags + N, dm.begin());
            std::copy(c->data_sigmas, c->data_sigmas + N, dsig.begin());
        }
        int kmax = 1, nf_avg_max = 0, nf_max_all = 0;
        for (int o = 0; o < O; ++o) {
            const int nf = doff[o + 1] - doff[o];
            if (nf < 0) { nmma_em_destroy(h); return fail("nmma_em_create: data_offsets must be non-decreasing"); }
            lim[o] = c->detection_limit ? c->detection_limit[o] : HUGE_VAL;
            nsrc[o] = c->n_sources ? c->n_sources[o] : 1;
            if (nsrc[o] < 1 || nsrc[o] > NMMA_MAX_SOURCES) { nmma_em_destroy(h); return fail("nmma_em_create: bad n_sources"); }
            for (int k = 0; k < nsrc[o]; ++k) {
                const int mm = c->sources ? c->sources[o * NMMA_MAX_SOURCES + k] : o;
                if (mm < 0 || mm >= M) { nmma_em_destroy(h); return fail("nmma_em_create: source filter out of range"); }
                src[o * NMMA_MAX_SOURCES + k] = mm;
            }
            if (nsrc[o] > 1) nf_avg_max = std::max(nf_avg_max, nf);
            nf_max_all = std::max(nf_max_all, nf);
            int G = 16;   // >= 16: the group's first 16 lanes each reduce one SVD coefficient
            while (G < nf && G < 64) G <<= 1;
            group[o] = G;
            kind[o] = c->sys_kind ? c->sys_kind[o] : NMMA_SYS_CONST;
            sconst[o] = c->sys_const ? c->sys_const[o] : 0.0;
            soff[o] = (int32_t)slots.size();
            snn[o] = 0;
            if (kind[o] == NMMA_SYS_CONST) {
                for (int i = doff[o]; i < doff[o + 1]; ++i) {
                    dsigtot[i] = std::sqrt(dsig[i] * dsig[i] + sconst[o] * sconst[o]);
                    dlogsig[i] = std::log(dsigtot[i]);
                    dinvsig[i] = 1.0 / dsigtot[i];
                }
            } else {
                const int nn = c->sys_n_nodes[o];
                const int so = c->sys_slot_offsets[o];
                if (nn < 1 || (kind[o] == NMMA_SYS_PARAM && nn != 1) || (kind[o] == NMMA_SYS_NODES && nn < 2)) {
                    nmma_em_destroy(h); return fail("nmma_em_create: bad systematics node count");
                }
                snn[o] = nn;
                kmax = std::max(kmax, nn);
                for (int k = 0; k < nn; ++k) {
                    if (!slot_ok(c->sys_slots[so + k])) { nmma_em_destroy(h); return fail("nmma_em_create: sys slot out of range"); }
                    slots.push_back(c->sys_slots[so + k]);
                    node_t.push_back(kind[o] == NMMA_SYS_NODES ? c->sys_node_times[so + k] : 0.0);
                }
                if (kind[o] == NMMA_SYS_NODES) {
                    const double* xn = c->sys_node_times + so;
                    for (int k = 1; k < nn; ++k)
                        if (!(xn[k] > xn[k - 1])) { nmma_em_destroy(h); return fail("nmma_em_create: sys node times must increase"); }
                    for (int i = doff[o]; i < doff[o + 1]; ++i) {
                        const double t = dt[i];
                        if (t < xn[0]) { nidx[i] = -1; }
                        else if (t >= xn[nn - 1]) { nidx[i] = nn - 1; }
                        else {
                            const int k = (int)(std::upper_bound(xn, xn + nn, t) - xn) - 1;
                            nidx[i] = k; ndx[i] = xn[k + 1] - xn[k]; noff[i] = t - xn[k];
                        }
                    }
                }
            }
        }
        soff[O] = (int32_t)slots.size();
        if (node_t.empty()) node_t.push_back(0.0);
        P.kmax = kmax;
        P.lc_nf_max = nf_max_all;
        P.n_sys_slots = (int32_t)slots.size();
        // Work items in observed-filter order -- except that the bands of NULL filters (nmma_em_config::null_filters: no record stream,
        // mfma_role<.., SKIPNULL> publishes zero coefficients for them before it starts) come first; the tasks file a band's sums under
        // its observed-filter index, so the order of the sum over bands does not change
        std::vector<int32_t> items;
        P.n_items_null = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int o = 0; o < O; ++o) {
                const bool null_band = any_null && nsrc[o] == 1 && null_m[src[o * NMMA_MAX_SOURCES]];
                if (null_band != (pass == 0)) continue;
                for (int k = 0; k < nsrc[o]; ++k) {
                    items.push_back(o); items.push_back(k); items.push_back(src[o * NMMA_MAX_SOURCES + k]); items.push_back(nsrc[o]);
                }
                if (null_band) ++P.n_items_null;
            }
        P.n_items = (int32_t)(items.size() / 4);
        std::vector<ItemDesc> desc(P.n_items), desc_unfolded;
        for (int k = 0; k < P.n_items; ++k) {
            ItemDesc& it = desc[k];
            std::memset(&it, 0, sizeof(it));
            it.o = items[4 * k]; it.ks = items[4 * k + 1]; it.m = items[4 * k + 2]; it.nsrc = items[4 * k + 3];
            it.G = group[it.o]; it.d0 = doff[it.o]; it.nf = doff[it.o + 1] - doff[it.o]; it.kind = kind[it.o];
            it.jlo = h->ranges[it.m * 4 + 0]; it.jhi = h->ranges[it.m * 4 + 1]; it.identity = h->ranges[it.m * 4 + 2];
            it.same_grid = h->same_grid[it.m];
            // (union grid: the TASK's window is the whole grid -- outside the surrogate's own nodes its rows give +inf and the flux sum
            //  is the second transient alone; s1_range keeps the surrogate's window for the curve outputs)
            if (null_m[it.m] || (union_grid && h->ranges[it.m * 4 + 3] >= 2)) { it.jlo = 0; it.jhi = P.NS - 1; }      // (a null filter: +inf rows on the whole grid)
            it.lim = lim[it.o]; it.e_const = sconst[it.o];
            it.ebvc = ext_coeff ? ext_coeff[it.m] : 0.0;
            it.has_ul = 0;
            for (int i = doff[it.o]; i < doff[it.o + 1]; ++i) if (!std::isfinite(dsig[i])) it.has_ul = 1;
            // (sampled time nodes: fewer than two finite node values make sigma_sys infinite, i.e. every datum an upper limit)
            if (it.kind == NMMA_SYS_NODES) it.has_ul = 1;
            // constant systematics: the fast path multiplies by the precomputed 1/sigma_tot (needs sigma_tot > 0 or an
            // upper limit); a sampled systematic (one parameter per filter or shared) is combined per datum in the task
            bool sig_ok = true;
            if (it.kind == NMMA_SYS_CONST) {
                for (int i = doff[it.o]; i < doff[it.o + 1]; ++i) if (!(dsigtot[i] > 0)) sig_ok = false;
            } else {        // one sampled parameter or sampled time nodes: sigma_tot per datum in the task
                for (int i = doff[it.o]; i < doff[it.o + 1]; ++i) dinvsig[i] = dsig[i];    // the slot carries sigma_data
            }
            // (the P92 law is evaluated per sample and filter: by a pre-pass for the lean task, in line by the generic item phase;
            //  the extended task does not have it)
            // (a filter without a single datum -- a model filter nobody observed -- only has its coefficients checked: generic phase)
            it.fast = (svd && sig_ok && NC == 10 && it.nf > 0 && (it.nsrc == 1 || !getenv("NMMA_EM_NO_LEAN_AVG")) && (!p92 || !getenv("NMMA_EM_NO_LEAN_P92")) &&
                       !std::isnan(it.lim) && !(std::isinf(it.lim) && it.lim < 0) && !getenv("NMMA_EM_NO_FAST")) ? 1 : 0;
        }
        h->nf_avg_max = nf_avg_max;
        for (const ItemDesc& it : desc) h->n_ul_items += it.has_ul ? 1 : 0;
        P.all_fast = P.n_items > 0 ? 1 : 0;
        for (const ItemDesc& it : desc) if (!it.fast) P.all_fast = 0;
        bool need_item_dat = false;     // the lean task fits LDS only with item-staged photometry
        std::vector<double> dat4((size_t)4 * std::max(N, 1), 0.0);
        for (int i = 0; i < N; ++i) { dat4[4 * i] = dt[i]; dat4[4 * i + 1] = dm[i]; dat4[4 * i + 2] = dinvsig[i]; dat4[4 * i + 3] = dlogsig[i]; }
        // filters with sampled systematics: the fourth word is the datum's position on the filter's time nodes, node index +
        // fraction of the interval (constant outside the nodes: systematics.py:288-291); 0 for a single parameter
        for (int o = 0; o < O; ++o) {
            if (kind[o] == NMMA_SYS_CONST) continue;
            for (int i = doff[o]; i < doff[o + 1]; ++i) {
                double q = 0.0;
                if (kind[o] == NMMA_SYS_NODES) q = nidx[i] < 0 ? 0.0 : (nidx[i] >= snn[o] - 1 ? (double)(snn[o] - 1) : nidx[i] + std::min(noff[i] / ndx[i], 1.0));
                dat4[4 * i + 3] = q;
            }
        }
        if (P.all_fast) {
            // extended fast kernel (all_fast = 2): time-node systematics, a detection limit,
            // more than LEAN_NF_MAX points in a filter, more photometry than the LDS staging holds, or a NaN epoch
            // somewhere; otherwise the lean task (all_fast = 1), which also takes equally spaced sample_times that differ
            // from the SVD grid (the CLI's --tmin/--tmax/--dt: two-stage interpolation, four basis rows per datum)
            for (const ItemDesc& it : desc)
                if ((it.kind == NMMA_SYS_PARAM && getenv("NMMA_EM_NO_LEAN_SYS")) || (it.kind == NMMA_SYS_NODES && getenv("NMMA_EM_NO_LEAN_NODES")) ||
                    it.nf > LEAN_NF_MAX || (std::isfinite(it.lim) && getenv("NMMA_EM_NO_LEAN_LIM")) || (ext_coeff && getenv("NMMA_EM_NO_LEAN_EXT")) ||
                    (!(it.identity && it.same_grid) && getenv("NMMA_EM_NO_LEAN2")) ||
                    (!P.st_uniform && getenv("NMMA_EM_NO_LEAN_NONUNI")) || N > DAT_MAX || getenv("NMMA_EM_NO_LEAN")) P.all_fast = 2;
            P.any_two = 0;
            for (const ItemDesc& it : desc) if (!(it.identity && it.same_grid)) P.any_two = 1;
            P.lean_x = 0;
            for (const ItemDesc& it : desc) if (it.nf > 32 || it.kind == NMMA_SYS_PARAM) P.lean_x = 1;
            if (!P.st_uniform || ext_coeff) P.lean_x = 1;
            P.p92_tab = p92 ? 1 : 0;
            for (int i = 0; i < N; ++i) if (std::isnan(dt[i])) P.all_fast = 2;
            // sample_times that differ from the SVD grid (every --tmin / --tmax / --dt run, the CLI's log-spaced grid): sample node j is
            // the stage-1 lerp between SVD nodes i, i + 1 (lightcurve_generation.py:177) -- a STATIC linear map of the coefficients.
            // The lean tasks take it folded into their basis rows (round 6; the dense task's A operands have carried it since round 3):
            // one table of NS rows per model filter ON THE SAMPLE GRID,
            //     row_j = [VA_i o span_i + (VA_{i+1} o span_{i+1} - VA_i o span_i) f_j | 1 | mins_i + (mins_{i+1} - mins_i) f_j],  f_j = off_j / dx_j
            // (a node that coincides with an SVD node keeps [VA_i | span_i | mins_i]: the reference's own association), so that a datum
            // reconstructs TWO rows, as on the SVD grid, instead of four, and a ring slot holds NS rows (41 for the CLI grid) instead of
            // NT = 211 + the lerp tables.  Nodes outside the SVD grid (+inf in the reference) lie outside every item's [jlo, jhi] and
            // are never bracketed: zero rows.  The extended task and the generic item phase (all_fast != 1) keep the SVD-grid table
            // and the two-stage arithmetic: the fold is undone below if the handle ends up there.
            if (P.any_two || !P.st_uniform) {
                if (P.all_fast == 1) {
                    const int RSl = 12;                                   // (fast items have NC == 10: rows of [10 | scale | offset])
                    const int NSl = P.NS;
                    fold_off_b2 = NSl * RSl * 8;
                    fold_bytes = (fold_off_b2 + 16 * 4 + 1023) / 1024 * 1024;
                    ltab_host.assign((size_t)M * fold_bytes, 0);
                    const int RS0 = P.tab_row_stride;
                    for (int m = 0; m < M; ++m) {
                        const unsigned char* tm = tab_host.data() + (size_t)m * P.tab_bytes;
                        const double* rows0 = reinterpret_cast<const double*>(tm);
                        const double* s1dx = reinterpret_cast<const double*>(tm + P.tab_off_s1dx);
                        const double* s1of = reinterpret_cast<const double*>(tm + P.tab_off_s1of);
                        const int32_t* s1i = reinterpret_cast<const int32_t*>(tm + P.tab_off_s1i);
                        unsigned char* tl = ltab_host.data() + (size_t)m * fold_bytes;
                        double* rowsl = reinterpret_cast<double*>(tl);
                        // (one folded row: the node at offset `of` behind SVD node i, spacing `dxv`)
                        auto fold_row = [&](const int i, const double of, const double dxv, double* r) {
                            const double* ra = rows0 + (size_t)i * RS0;    // [VA | span | mins] of SVD node i
                            if (of == 0.0 || i + 1 >= NT) { for (int q = 0; q < RSl; ++q) r[q] = ra[q]; return; }
                            const double* rb = ra + RS0;
                            const long double f = (long double)of / (long double)dxv;
                            for (int q = 0; q < 10; ++q) {
                                const long double a = (long double)ra[q] * ra[10], b = (long double)rb[q] * rb[10];
                                r[q] = (double)(a + (b - a) * f);
                            }
                            r[10] = 1.0;
                            r[11] = (double)((long double)ra[11] + ((long double)rb[11] - (long double)ra[11]) * f);
                        };
                        if (null_m[m]) {                                   // no value on any node: the kilonova's magnitude comes out +inf
                            for (int j = 0; j < NSl; ++j) { rowsl[(size_t)j * RSl + 10] = 1.0; rowsl[(size_t)j * RSl + 11] = HUGE_VAL; }
                            std::memcpy(tl + fold_off_b2, tm + P.tab_off_b2, 16 * 4);
                            continue;
                        }
                        for (int j = 0; j < NSl && !union_grid; ++j) {
                            const int i = s1i[j];
                            if (i < 0) continue;                           // outside the SVD grid: never bracketed
                            fold_row(i, s1of[j], s1dx[j], rowsl + (size_t)j * RSl);
                        }
                        // Union grid: the second hop on top -- grid node j between the surrogate's own nodes i, i + 1 (u_*), each a folded
                        // row of its own; a node outside the surrogate's window has NO value there: [0 | 1 | +inf], the kilonova's
                        // magnitude comes out +inf and the flux sum is the second transient alone (lean_task, COMB)
                        for (int j = 0; j < NSl && union_grid; ++j) {
                            double* r = rowsl + (size_t)j * RSl;
                            const int NBh = P.NB;
                            const int i = h->u_idx[(size_t)m * NSl + j];
                            if (i < 0) { r[10] = 1.0; r[11] = HUGE_VAL; continue; }
                            double ra[12], rb[12];
                            fold_row(h->b_idx[(size_t)m * NBh + i], h->b_off[(size_t)m * NBh + i], h->b_dx[(size_t)m * NBh + i], ra);
                            if (h->u_off[(size_t)m * NSl + j] == 0.0) { for (int q = 0; q < RSl; ++q) r[q] = ra[q]; continue; }
                            fold_row(h->b_idx[(size_t)m * NBh + i + 1], h->b_off[(size_t)m * NBh + i + 1], h->b_dx[(size_t)m * NBh + i + 1], rb);
                            const long double g = (long double)h->u_off[(size_t)m * NSl + j] / (long double)h->u_dx[(size_t)m * NSl + j];
                            for (int q = 0; q < 10; ++q) {
                                const long double a = (long double)ra[q] * ra[10], b = (long double)rb[q] * rb[10];
                                r[q] = (double)(a + (b - a) * g);
                            }
                            r[10] = 1.0;
                            r[11] = (double)((long double)ra[11] + ((long double)rb[11] - (long double)ra[11]) * g);
                        }
                        std::memcpy(tl + fold_off_b2, tm + P.tab_off_b2, 16 * 4);
                    }
                    fold = true;
                    unfold_tab_bytes = P.tab_bytes; unfold_off_b2 = P.tab_off_b2;
                    desc_unfolded = desc;
                    for (ItemDesc& it : desc) { it.identity = 1; it.same_grid = 1; }
                    P.any_two = 0;
                    P.tab_bytes = fold_bytes; P.tab_off_b2 = fold_off_b2; P.tab_fast_bytes = fold_bytes;
                } else {
                    // the extended task reads the stage-1 lerp tables next to the basis rows: it stages the whole per-filter table
                    P.tab_fast_bytes = P.tab_bytes;
                }
            }
            // the lean task reads the photometry from LDS only: it must fit next to at least one ring slot for both tile
            // sizes (BASELINE config 4's 2 400 points just do), else the extended task with its global-memory fallback
            // (or, for the lean task with extras, with the epochs only and each item's records in its ring slot: item-staged photometry below)
            if (P.all_fast == 1)
                for (int r = 1; r <= 2; ++r)
                    if (lds_layout_logl_try(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots, 1, true,
                                            P.lean_x ? (ext_coeff ? P.n_items : 1) : 0).total > LDS_DYNAMIC_MAX) {
                        int nf_max = 0;
                        for (const ItemDesc& it : desc) nf_max = std::max(nf_max, (int)it.nf);
                        const int tfb1 = (P.tab_fast_bytes + nf_max * 32 + 1023) / 1024 * 1024;
                        if (P.lean_x && !getenv("NMMA_EM_NO_ITEM_DAT") &&
                            lds_layout_logl_try(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, tfb1, P.n_items, M, NP, 1, N, P.n_sys_slots, 1, true,
                                                ext_coeff ? P.n_items : 1, 8).total <= LDS_DYNAMIC_MAX) need_item_dat = true;
                        else P.all_fast = 2;
                    }
            // averaged bands (several source filters per observed filter) and time-node systematics: the general lean task only
            // (em_logl<.., 5>: a band's tasks sit on its last source item and walk the sources) -- every source of a band on the
            // same node range, the ring deep enough to hold one band's sources together, the task map within its LDS table
            int max_nsrc = 1;
            bool any_nodes = false, any_lim = false;
            for (const ItemDesc& it : desc) {
                max_nsrc = std::max(max_nsrc, (int)it.nsrc);
                any_nodes = any_nodes || it.kind == NMMA_SYS_NODES;
                any_lim = any_lim || std::isfinite(it.lim);
            }
            // Finite detection limits / time-node systematics on a COMBINATION's handle (stack_operands), no averaged band: the
            // combined-model flavours of the lean task carry the truncation mass and the node interpolation themselves (em_logl<.., 7 | 8>,
            // round 6) -- the handle stays in the lean family and serves nmma_em_loglike_stack2 only (the plain lean flavours know
            // neither: those entry points refuse it)
            comb_lim = c->stack_operands && (any_lim || any_nodes) && max_nsrc == 1 && P.all_fast == 1 && !getenv("NMMA_EM_NO_COMB_LIM");
            if (comb_lim) h->stack2_only = true;
            P.lean_gen = (max_nsrc > 1 || ((any_nodes || any_lim) && !comb_lim && P.all_fast == 1)) ? 1 : 0;
            if (P.lean_gen && need_item_dat && P.all_fast == 1) { P.all_fast = 2; need_item_dat = false; }   // (the general lean task stages all records)
            if (P.lean_gen) {
                bool ok = P.all_fast == 1;
                for (size_t k = 0; k < desc.size() && ok; ++k)
                    if (desc[k].ks > 0 && (desc[k].jlo != desc[k - 1].jlo || desc[k].jhi != desc[k - 1].jhi ||
                                           desc[k].identity != desc[k - 1].identity || desc[k].same_grid != desc[k - 1].same_grid)) ok = false;
                bool ok_r[2] = {ok, ok};
                // (the table of log Phi, logphi_tab.h, next to the ring: needed for a band with a finite detection limit; taken for upper
                //  limits alone where it costs neither tile size a ring slot)
                bool want_tab = any_lim || h->n_ul_items > 0;
                if (want_tab && !any_lim)
                    for (int r = 1; r <= 2; ++r) {
                        const LdsW L0 = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                                        P.has_ebv ? P.n_items : 1, h->ring_max, 32, 0, 0);
                        const LdsW L1 = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                                        P.has_ebv ? P.n_items : 1, h->ring_max, 32, 0, LOGPHI_LDS_BYTES);
                        if (L1.total > LDS_DYNAMIC_MAX || L1.nbuf != L0.nbuf || (L1.dat >= 0) != (L0.dat >= 0)) want_tab = false;
                    }
                for (int r = 1; r <= 2 && ok; ++r) {
                    const LdsW Lr = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                                    P.has_ebv ? P.n_items : 1, h->ring_max, 32, 0, want_tab ? LOGPHI_LDS_BYTES : 0);
                    if (Lr.total > LDS_DYNAMIC_MAX || Lr.nbuf < max_nsrc) ok_r[r - 1] = false;
                    if (getenv("NMMA_EM_VERBOSE")) fprintf(stderr, "  R = %d: LDS %d bytes, ring depth %d\n", r, (int)Lr.total, (int)Lr.nbuf);
                    int nt = 0;
                    for (const ItemDesc& it : desc) if (it.ks == it.nsrc - 1) nt += it.nf <= 16 ? 2 * r : 4 * r;
                    if (nt > TMAP_MAX) ok_r[r - 1] = false;
                }
                // (32-sample tiles double the partial-sum slots: when the ring then holds fewer slots than a band has sources,
                //  large batches keep 16-sample tiles -- slower per sample than 32, far faster than the generic item phase)
                if (ok && ok_r[0] && !ok_r[1] && h->force_r != 2) h->force_r = 1;
                else if (!(ok_r[0] && ok_r[1])) ok = false;
                if (getenv("NMMA_EM_VERBOSE"))
                    fprintf(stderr, "nmma_em_create: general lean task (averaged bands: max %d sources per band; time-node systematics: %s): %s "
                                    "(all_fast %d, equally spaced %d, %d items, table %d bytes)\n",
                            max_nsrc, any_nodes ? "yes" : "no", ok ? "taken" : "not taken", (int)P.all_fast, (int)P.st_uniform, (int)P.n_items,
                            (int)P.tab_fast_bytes);
                if (ok) { P.lean_x = 1; P.mass_tab = want_tab ? 1 : 0; }       // (finite limits / upper limits: log Phi from the table in LDS)
                else if (max_nsrc > 1) { P.all_fast = 0; P.lean_gen = 0; P.tab_fast_bytes = P.tab_bytes; }    // generic item phase
                else { P.all_fast = 2; P.lean_gen = 0; }                                                     // time nodes: extended task
            }
            if (P.all_fast == 2 && p92) {       // the extended task has no P92 law: generic item phase
                P.all_fast = 0;
                P.tab_fast_bytes = P.tab_bytes;
            }
            if (P.all_fast != 1) P.p92_tab = 0;
            if (fold && P.all_fast != 1) {
                // not a lean handle after all (extended task / generic item phase): they read the SVD-grid table with its lerp tables
                fold = false;
                for (size_t k = 0; k < desc.size(); ++k) { desc[k].identity = desc_unfolded[k].identity; desc[k].same_grid = desc_unfolded[k].same_grid; }
                P.any_two = 0;
                for (const ItemDesc& it : desc) if (!(it.identity && it.same_grid)) P.any_two = 1;
                P.tab_bytes = unfold_tab_bytes; P.tab_off_b2 = unfold_off_b2; P.tab_fast_bytes = P.tab_bytes;
                ltab_host.clear();
            }
            if (fold) {
                // (the handle's lean tasks are the only readers of EmDev::tab: it now points at the folded table)
                NM_UP(ltab_host, tab);
                if (getenv("NMMA_EM_VERBOSE"))
                    fprintf(stderr, "nmma_em_create: stage-1 lerp folded into the lean tasks' basis rows: %d rows of the sample grid per filter, "
                                    "%d bytes per ring slot (SVD-grid table with lerp tables: %d)\n", (int)P.NS, fold_bytes, unfold_tab_bytes);
            }
            // Pei 1992 in the lean task WITHOUT the pre-pass launch (7.5 us per call next to a 32.6 us likelihood launch): the law's
            // magnitude is E(B-V) times a smooth function of the redshift per filter -- a 14-term Chebyshev series over the handle's
            // redshift range (z comes from the z(d_L) grid: np.interp never leaves it), checked here against the law itself on a dense
            // grid; a range the series does not resolve (or a filter that crosses the law's validity limits inside it) keeps the pre-pass.
            P.p92_cheb = nullptr;
            if (P.p92_tab && P.redshift_mode == NMMA_Z_GRID && !P.has_h0 && c->n_cosmo >= 1 && !getenv("NMMA_EM_NO_P92_SERIES")) {
                double z_lo = c->z_grid[0], z_hi = c->z_grid[0];
                for (int i = 0; i < c->n_cosmo; ++i) { z_lo = std::min(z_lo, c->z_grid[i]); z_hi = std::max(z_hi, c->z_grid[i]); }
                const double mid = 0.5 * (z_lo + z_hi), half = std::max(0.5 * (z_hi - z_lo), 1e-12);
                std::vector<double> rows((size_t)M * 16, 0.0);
                bool ok = std::isfinite(mid) && std::isfinite(half) && z_lo > -1.0;
                constexpr int NCH = 14;
                for (int m = 0; m < M && ok; ++m) {
                    double* row = rows.data() + (size_t)m * 16;
                    row[0] = mid; row[1] = 1.0 / half;
                    double f[NCH];
                    for (int j = 0; j < NCH; ++j) f[j] = p92_smc_ext_mag(c->filter_nu0[m], 1.0 + mid + half * std::cos(kPi * (j + 0.5) / NCH), 1.0);
                    for (int k = 0; k < NCH; ++k) {
                        double acc = 0.0;
                        for (int j = 0; j < NCH; ++j) acc += f[j] * std::cos(kPi * k * (j + 0.5) / NCH);
                        row[2 + k] = acc * (k == 0 ? 1.0 : 2.0) / NCH;
                    }
                    double scale = 0.0, worst = 0.0;
                    for (int i = 0; i <= 512; ++i) {
                        const double z = z_lo + (z_hi - z_lo) * i / 512.0;
                        const double want = p92_smc_ext_mag(c->filter_nu0[m], 1.0 + z, 1.0), got = cheb14_eval(row, z);
                        scale = std::max(scale, std::fabs(want));
                        worst = std::max(worst, std::fabs(got - want));
                    }
                    if (!(worst <= 1e-13 * std::max(scale, 1e-3))) ok = false;
                    if (getenv("NMMA_EM_VERBOSE"))
                        fprintf(stderr, "nmma_em_create: Pei-1992 series, filter %d on z in [%g, %g]: max |error| %.2e mag per unit E(B-V) (largest value %.3g)\n", m, z_lo, z_hi, worst, scale);
                }
                if (ok) {
                    NM_UP(rows, p92_cheb);
                    P.p92_tab = 0;
                }
            }
        }
        // Item-staged photometry: when staging ALL records next to the ring leaves the lean task (em_logl<.., 3 | 4>) a shallower
        // ring than staging the epochs only would, the {t, m, 1/sigma, ln sigma} records travel with their item's basis rows --
        // one table per work item, [prefix of the model filter's table | records] -- and LDS keeps the epochs of all points for
        // stage P.  BASELINE config 4 (12 x 200 points): one ring slot -> two, i.e. the surrogate of item k + 1 overlaps the
        // tasks of item k at all.
        P.dat_in_tab = 0; P.tabi = nullptr; P.tabi_bytes = 0; P.tab_off_dat = 0;
        // (the dense lean task below needs the records per item whether or not the ring gets deeper)
        const int NS = P.NS;
        bool dense_eligible = P.all_fast == 1 && P.lean_x && !P.lean_gen && NC <= 10 && NS <= 256 && !getenv("NMMA_EM_NO_DENSE") &&
                              !c->stack_operands;       // (the combined model's one-launch form is a row-form lean task)
        {
            long rows = 0;
            for (const ItemDesc& it : desc) {
                // (measured in round 6 with the rewritten task too: below ~17 points per filter the unit's set-up outweighs the rows it saves --
                //  config 2 31.1 -> 35.2 us, the real AT2017gfo photometry 47.2 -> 48.2 us when forced onto the dense task)
                if (it.nf <= 16 || it.nsrc != 1) dense_eligible = false;
                rows += ((it.identity && it.same_grid) ? 2L : 4L) * it.nf;       // (a two-stage grid reconstructs four SVD rows per datum)
            }
            // (pays once a sample reconstructs about as many rows as the sample grid has nodes: 6 x 130 points -9 %,
            //  6 x 250 -15 %, 12 x 200 -12 % on the SVD grid; NMMA_EM_DENSE_PCT moves the threshold, in percent of the node count)
            long pct = 100;
            if (const char* ev = getenv("NMMA_EM_DENSE_PCT")) pct = std::max(1, atoi(ev));
            if (!(100 * rows > pct * P.n_items * NS)) dense_eligible = false;
        }
        if (P.all_fast == 1 && P.lean_x && !P.lean_gen && !tab_host.empty() && !getenv("NMMA_EM_NO_ITEM_DAT")) {
            int nf_max = 0;
            for (const ItemDesc& it : desc) nf_max = std::max(nf_max, (int)it.nf);
            const int ext_rows = P.has_ebv ? P.n_items : 1;
            const int tfb0 = P.tab_fast_bytes, tfb1 = (tfb0 + nf_max * 32 + 1023) / 1024 * 1024;
            bool gain = false, ok = true;
            // (does the dense task's layout fit, with a ring of at least two slots?  It carries its own [b2 | records] slots; its records are
            //  the detections padded to whole passes of 32 followed by the upper limits -- dense_records below)
            bool dense_fits = dense_eligible;
            int dense_recmax = 0;
            for (const ItemDesc& it : desc) {
                int nd = 0;
                for (int i = it.d0; i < it.d0 + it.nf; ++i) nd += std::isfinite(dsig[i]) ? 1 : 0;
                dense_recmax = std::max(dense_recmax, ((nd + 31) & ~31) + (it.nf - nd));
            }
            const int tfbd = (tfb0 - P.tab_off_b2 + dense_recmax * 32 + 1023) / 1024 * 1024;
            for (int r = 1; r <= 2 && dense_fits; ++r) {
                // (0 bytes per point next to the ring: the dense task reads a datum's epoch from its item's records)
                const LdsW Ld = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, tfbd, P.n_items, M, NP, 1, N, P.n_sys_slots, ext_rows, h->ring_max, 0,
                                                (NS + 15) & ~15);
                if (Ld.total > LDS_DYNAMIC_MAX || Ld.dat < 0 || Ld.nbuf < std::min(2, (int)P.n_items)) dense_fits = false;
                if (getenv("NMMA_EM_VERBOSE"))
                    fprintf(stderr, "nmma_em_create: dense lean task, R = %d: ring depth %d, LDS %d bytes\n", r, (int)Ld.nbuf, (int)Ld.total);
            }
            dense_eligible = dense_fits;
            for (int r = 1; r <= 2; ++r) {
                const LdsW Ln = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, tfb0, P.n_items, M, NP, 1, N, P.n_sys_slots, ext_rows, h->ring_max);
                const LdsW Ls = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, tfb1, P.n_items, M, NP, 1, N, P.n_sys_slots, ext_rows, h->ring_max, 8);
                const int ln_nbuf = Ln.total <= LDS_DYNAMIC_MAX ? Ln.nbuf : 0;           // (0: all records + one ring slot do not fit at all)
                if (Ls.total > LDS_DYNAMIC_MAX || Ls.dat < 0 || Ls.nbuf < ln_nbuf) ok = false;
                if (Ls.nbuf > ln_nbuf) gain = true;
                if (getenv("NMMA_EM_VERBOSE"))
                    fprintf(stderr, "nmma_em_create: item-staged photometry, R = %d: ring depth %d -> %d (LDS %d -> %d bytes)\n", r, (int)Ln.nbuf,
                            (int)Ls.nbuf, (int)Ln.total, (int)Ls.total);
            }
            if ((ok && gain) || dense_eligible || need_item_dat) {
                std::vector<unsigned char> tabi((size_t)P.n_items * tfb1 + 1024, 0);     // (+ slack: the dense task's copy starts at b2, rounded up to 1 KiB)
                for (int k = 0; k < P.n_items; ++k) {
                    unsigned char* t = tabi.data() + (size_t)k * tfb1;
                    std::memcpy(t, (fold ? ltab_host : tab_host).data() + (size_t)desc[k].m * P.tab_bytes, (size_t)tfb0);
                    std::memcpy(t + tfb0, dat4.data() + (size_t)4 * desc[k].d0, (size_t)desc[k].nf * 32);
                    desc[k].tabi = k;
                }
                P.dat_in_tab = 1; P.tab_off_dat = tfb0; P.tabi_bytes = tfb1; P.tab_fast_bytes = tfb1;
                NM_UP(tabi, tabi);
            }
        }
        // Dense lean task (em_logl<.., 6>): with item-staged photometry, sample_times = the SVD grid, equally spaced, more than 16
        // points in every filter and clearly more row reconstructions per sample (two per datum) than the grid has nodes, the
        // four tasks of (item, 16 samples) reconstruct ALL nodes on the fp64 matrix cores and a datum reads its two node
        // magnitudes.  The ring slot then holds [b2 | records] only (the rows are MFMA operands read from global memory) and the
        // per-wave coefficient slots give way to two node buffers.
        P.dense = 0;
        if (P.dat_in_tab && dense_eligible) {
            // Records of the dense task (round 6: a datum loop of ~20 instructions, em_logl.h:dense_task).  Per item, behind the table prefix:
            //   detections, in the photometry's order: {t, m, 1 / sigma_tot, -(ln sqrt(2 pi) + ln sigma_tot)}   (constant systematics)
            //                                          {t, m, sigma_data, 0}                                    (sampled em_syserr)
            //   padding to a whole pass of 32 slots: {t of the first detection, 0, 0, 0} -- its term is exactly 0 for constant systematics
            //                                          (x = (0 - est) * 0) and masked by its index for sampled ones
            //   upper limits (infinite sigma_data): {t, m, sigma_sys, 0}, evaluated after the loop by the lanes that hold one
            // ItemDesc::pad_i = detections, ItemDesc::has_ul = upper limits (a count here; every other reader tests it against 0).
            int recmax = 0;
            std::vector<int> n_det(P.n_items, 0);
            for (int k = 0; k < P.n_items; ++k) {
                for (int i = desc[k].d0; i < desc[k].d0 + desc[k].nf; ++i) n_det[k] += std::isfinite(dsig[i]) ? 1 : 0;
                recmax = std::max(recmax, ((n_det[k] + 31) & ~31) + (desc[k].nf - n_det[k]));
            }
            const int tfb0 = P.tab_off_dat;
            const int tbi = (tfb0 + recmax * 32 + 1023) / 1024 * 1024;
            std::vector<unsigned char> tabd((size_t)P.n_items * tbi + 1024, 0);     // (+ slack: the task's copy starts at b2, rounded up to 1 KiB)
            for (int k = 0; k < P.n_items; ++k) {
                ItemDesc& it = desc[k];
                unsigned char* t = tabd.data() + (size_t)k * tbi;
                std::memcpy(t, (fold ? ltab_host : tab_host).data() + (size_t)it.m * P.tab_bytes, (size_t)tfb0);
                double* rec = reinterpret_cast<double*>(t + tfb0);
                const bool sampled = it.kind != NMMA_SYS_CONST;
                int w = 0;
                double t_first = 0.0;
                bool have_first = false;
                for (int i = it.d0; i < it.d0 + it.nf; ++i) {
                    if (!std::isfinite(dsig[i])) continue;
                    if (!have_first) { t_first = dt[i]; have_first = true; }
                    rec[4 * w] = dt[i]; rec[4 * w + 1] = dm[i];
                    rec[4 * w + 2] = sampled ? dsig[i] : dinvsig[i];
                    rec[4 * w + 3] = sampled ? 0.0 : -(kNormPdfLogC + dlogsig[i]);
                    ++w;
                }
                for (; w < ((n_det[k] + 31) & ~31); ++w) { rec[4 * w] = t_first; rec[4 * w + 1] = 0.0; rec[4 * w + 2] = 0.0; rec[4 * w + 3] = 0.0; }
                for (int i = it.d0; i < it.d0 + it.nf; ++i) {
                    if (std::isfinite(dsig[i])) continue;
                    rec[4 * w] = dt[i]; rec[4 * w + 1] = dm[i]; rec[4 * w + 2] = it.e_const; rec[4 * w + 3] = 0.0;
                    ++w;
                }
                it.pad_i = n_det[k];
                it.has_ul = it.nf - n_det[k];
                it.tabi = k;
            }
            P.tabi_bytes = tbi;
            NM_UP(tabd, tabi);
            // A sampled systematic (one parameter per filter or shared): sum_i ln sigma_tot,i over a band's detections as Chebyshev series
            // in w = ln e (EmDev::lnsig_tab) -- the datum loop of the dense task then computes 1 / sigma_tot^2 only.  Verified here
            // against the direct sum on 40 points per interval (1e-13 of max(1, |F|)); any band that fails keeps the per-datum logarithm.
            P.lnsig_tab = nullptr; P.lnsig_w0 = std::log(1e-4);
            {
                bool any_param = false, all_param = true;
                for (const ItemDesc& it : desc) {
                    if (it.kind == NMMA_SYS_PARAM) any_param = true;
                    else if (it.kind != NMMA_SYS_CONST) all_param = false;
                }
                if (any_param && all_param && !getenv("NMMA_EM_NO_LNSIG_TAB")) {
                    constexpr int ND = LNSIG_DEG + 1;
                    std::vector<double> tabl((size_t)P.n_items * LNSIG_NI * 16, 0.0);
                    bool ok = true;
                    const long double pi = 3.14159265358979323846264338327950288L;
                    for (int k = 0; k < P.n_items && ok; ++k) {
                        const ItemDesc& it = desc[k];
                        if (it.kind != NMMA_SYS_PARAM) continue;
                        std::vector<long double> sd2;
                        for (int i = it.d0; i < it.d0 + it.nf; ++i) if (std::isfinite(dsig[i])) sd2.push_back((long double)dsig[i] * dsig[i]);
                        auto F = [&](long double w) {
                            const long double e2 = std::exp(2.0L * w);
                            long double acc = 0.0L;
                            for (long double v : sd2) acc += std::log(v + e2);
                            return 0.5L * acc;
                        };
                        for (int q = 0; q < LNSIG_NI && ok; ++q) {
                            const long double a = (long double)P.lnsig_w0 + 0.5L * q, mid = a + 0.25L, half = 0.25L;
                            long double f[ND];
                            for (int j = 0; j < ND; ++j) f[j] = F(mid + half * std::cos(pi * (j + 0.5L) / ND));
                            double* row = tabl.data() + ((size_t)k * LNSIG_NI + q) * 16;
                            for (int n = 0; n < ND; ++n) {
                                long double acc = 0.0L;
                                for (int j = 0; j < ND; ++j) acc += f[j] * std::cos(pi * n * (j + 0.5L) / ND);
                                row[n] = (double)(acc * (n == 0 ? 1.0L : 2.0L) / ND);
                            }
                            for (int t = 0; t < 40 && ok; ++t) {          // the series as the kernel evaluates it (Clenshaw, fp64) against the sum
                                const double x = -1.0 + 2.0 * (t + 0.37) / 40.0;
                                double b1 = 0.0, b2 = 0.0;
                                for (int n = LNSIG_DEG; n >= 1; --n) { const double b0 = 2.0 * x * b1 - b2 + row[n]; b2 = b1; b1 = b0; }
                                const double got = x * b1 - b2 + row[0];
                                const long double want = F(mid + half * (long double)x);
                                if (!(std::fabs((double)((long double)got - want)) <= 1e-13 * std::max(1.0, std::fabs((double)want)))) ok = false;
                            }
                        }
                    }
                    if (ok) NM_UP(tabl, lnsig_tab);
                    if (getenv("NMMA_EM_VERBOSE")) fprintf(stderr, "nmma_em_create: dense task, sum of ln sigma_tot from the Chebyshev table in ln e: %s\n", ok ? "built" : "not accurate enough, not used");
                }
            }
            {
                const int tfbd = (P.tab_off_dat - P.tab_off_b2 + recmax * 32 + 1023) / 1024 * 1024;
                {
                    // A operands on the SAMPLE grid: node j is the stage-1 lerp between SVD nodes i, i + 1 (lightcurve_generation.py:177;
                    // j = i and no lerp when sample_times is the SVD grid), folded into the rows: [VA o span | mins | 0][j] =
                    // row[i] + (row[i + 1] - row[i]) off_j / dx_j.  Nodes outside the SVD grid (+inf in the reference) lie outside
                    // every item's [jlo, jhi] and are never bracketed: zeros.
                    const int n_tt = (NS + 15) / 16;
                    // (column NC multiplies the constant 1 of the B operand: mins; column NC + 1 -- round 6 -- multiplies the SAMPLE's
                    //  offset, extinction + distance modulus + K-correction, so that the node buffer holds apparent magnitudes: 1)
                    auto svd_row = [&](int m, int i, int kc) -> double {
                        const double span = c->maxs[(size_t)m * NT + i] - c->mins[(size_t)m * NT + i];
                        return kc < NC ? c->VA[((size_t)m * NT + i) * NC + kc] * span : (kc == NC ? c->mins[(size_t)m * NT + i] : (kc == NC + 1 ? 1.0 : 0.0));
                    };
                    std::vector<double> dva((size_t)M * n_tt * 3 * 64, 0.0);
                    for (int m = 0; m < M; ++m) {
                        const unsigned char* tm = tab_host.data() + (size_t)m * (fold ? unfold_tab_bytes : P.tab_bytes);
                        const double* s1dx = reinterpret_cast<const double*>(tm + P.tab_off_s1dx);
                        const double* s1of = reinterpret_cast<const double*>(tm + P.tab_off_s1of);
                        const int32_t* s1i = reinterpret_cast<const int32_t*>(tm + P.tab_off_s1i);
                        for (int tt = 0; tt < n_tt; ++tt)
                            for (int step = 0; step < 3; ++step)
                                for (int ln = 0; ln < 64; ++ln) {
                                    const int j = 16 * tt + (ln & 15), kc = 4 * step + (ln >> 4);
                                    double v = 0.0;
                                    if (j < NS && s1i[j] >= 0) {
                                        const int i = s1i[j];
                                        v = svd_row(m, i, kc);
                                        if (s1of[j] != 0.0 && i + 1 < NT && kc <= NC) v = v + (svd_row(m, i + 1, kc) - v) * (s1of[j] / s1dx[j]);
                                    }
                                    dva[(((size_t)m * n_tt + tt) * 3 + step) * 64 + ln] = v;
                                }
                    }
                    NM_UP(dva, dva);
                    P.dense = 1; P.tab_fast_bytes = tfbd;
                    // (constant systematics on an equally spaced grid -- BASELINE config 4 -- take the kernel that holds that variant alone)
                    h->dense_plain = P.st_uniform && !getenv("NMMA_EM_NO_DENSE_PLAIN");
                    for (const ItemDesc& it : desc) if (it.kind != NMMA_SYS_CONST) h->dense_plain = false;
                }
            }
        }
        if (P.all_fast) {
            // lanes per sample of the fast path (two data per lane in registers, further pairs in a loop)
            for (ItemDesc& it : desc) it.G = it.nf <= 32 ? 16 : (it.nf <= 64 ? 32 : 64);
            // tasks per tile of 16 / 32 samples: the lean task takes 8 samples when a filter has <= 16 points, else 4;
            // the extended task 64 / G samples
            for (ItemDesc& it : desc)
                for (int r = 0; r < 2; ++r) {
                    const int ts = 16 * (r + 1);
                    it.ntask[r] = P.all_fast == 1 ? (it.nf <= 16 ? ts / 8 : ts / 4) : ts * it.G / 64;
                }
        }
        NM_UP(dat4, dat4);
        NM_UP(doff, doff); NM_UP(dt, dt); NM_UP(dm, dm); NM_UP(dsig, dsig); NM_UP(dsigtot, dsigtot);
        NM_UP(dlogsig, dlogsig); NM_UP(dinvsig, dinvsig); NM_UP(lim, lim); NM_UP(nsrc, nsrc); NM_UP(src, src); NM_UP(group, group);
        NM_UP(kind, sys_kind); NM_UP(sconst, sys_const); NM_UP(snn, sys_nn); NM_UP(soff, sys_off);
        NM_UP(node_t, sys_node_t);
        NM_UP(slots, sys_slots); NM_UP(nidx, sys_nidx); NM_UP(ndx, sys_ndx); NM_UP(noff, sys_noff);
        NM_UP(items, items);
        {
            std::vector<int32_t> d_item(std::max(N, 1), 0);
            for (int k = 0; k < P.n_items; ++k)
                if (desc[k].ks == 0)
                    for (int i = 0; i < desc[k].nf; ++i) d_item[desc[k].d0 + i] = k;
            NM_UP(d_item, d_item);
        }
        P.n_data = N;
        // The lean tasks' upper limits (norm.logsf = log Phi of the negated residual) read the table of logphi_tab.h from LDS -- decided
        // HERE, once per handle, for both tile sizes and every form of the fused MCMC step (its parked state shares the space): only
        // where the table costs none of them a ring slot or the photometry staging, so that a handle's bits do not depend on the
        // batch size or on how a queue is stepped.  NMMA_EM_NO_UL_TAB=1 keeps scipy's formula (out of line, as before round 5).
        // (round 6: the dense task too -- its table sits behind the node buffers)
        if (P.all_fast == 1 && !P.lean_gen && h->n_ul_items > 0 && !getenv("NMMA_EM_NO_UL_TAB")) {
            bool ok = true;
            const int ext_rows = P.lean_x ? (P.has_ebv ? P.n_items : 1) : 0;
            const int drows = P.dense ? ((NS + 15) & ~15) : 0;
            for (int r = 1; r <= 2; ++r)
                for (int wl = 0; wl <= 16; wl += 8) {
                    const LdsW L0 = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots, ext_rows,
                                                    h->ring_max, P.dense ? 0 : (P.dat_in_tab ? 8 : 32), drows, 0, wl);
                    const LdsW L1 = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots, ext_rows,
                                                    h->ring_max, P.dense ? 0 : (P.dat_in_tab ? 8 : 32), drows, LOGPHI_LDS_BYTES, wl);
                    if (getenv("NMMA_EM_VERBOSE"))
                        fprintf(stderr, "nmma_em_create: log Phi table for upper limits, R = %d, %d lanes per chain: LDS %d -> %d bytes, ring depth %d -> %d\n", r, wl,
                                (int)L0.total, (int)L1.total, (int)L0.nbuf, (int)L1.nbuf);
                    if (L0.total > LDS_DYNAMIC_MAX) continue;       // (this form cannot launch with or without the table)
                    if (L1.total > LDS_DYNAMIC_MAX || L1.nbuf != L0.nbuf || (L1.dat >= 0) != (L0.dat >= 0)) {
                        // (a plain launch decides for the handle; a form of the fused MCMC step gives way instead -- two launches per
                        //  step for those queues, both with the table: every likelihood launch gains more than that form's step did)
                        if (wl == 0) ok = false;
                        else h->walk_tab_mask |= 1 << (2 * (r - 1) + (wl == 16 ? 1 : 0));
                    }
                }
            P.mass_tab = ok ? 1 : 0;
            if (!ok) h->walk_tab_mask = 0;
        }
        // Combined model in one launch (em_logl<.., 7 | 8>, nmma_em_loglike_stack2): the lean task (equally or unequally spaced
        // sample_times), every work item's curve finite on the WHOLE sample grid (the flux sum is then finite wherever the data can
        // bracket, and the window test of the task is the stacked curve's), the table of the flux sum next to a ring of at least one slot
        if (!c->stack_operands) h->stack2_why = "the handle was created without nmma_em_config::stack_operands";
        else if (!svd) h->stack2_why = "not an SVD surrogate handle";
        else if (P.all_fast != 1 || P.lean_gen || P.dense)
            h->stack2_why = "the configuration needs the general task (averaged bands, more "
                            "points per filter than the lean task holds, a surrogate with other than 10 coefficients, a model filter without data)";
        else if (NS < 2 || getenv("NMMA_EM_NO_STACK2")) h->stack2_why = "disabled (NMMA_EM_NO_STACK2) or fewer than two sample times";
        else if (union_grid && (!fold || !union_basis_finite || h->always_floor))
            h->stack2_why = "union grid: the surrogate's basis has non-finite entries on its own sample_times, or fewer than two of them lie on the SVD grid";
        else {
            bool ok = true;
            for (const ItemDesc& it : desc)
                if (it.jlo != 0 || it.jhi != NS - 1 || it.nsrc != 1) {
                    ok = false;
                    h->stack2_why = "a surrogate curve is not finite on the whole sample grid (sample_times reach beyond the SVD grid, or a basis "
                                    "with non-finite entries): the flux sum's window would differ from the surrogate's";
                }
            for (int r = 1; r <= 2 && ok; ++r)
                if (lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                    P.has_ebv ? P.n_items : 1, h->ring_max, P.dat_in_tab ? 8 : 32, 0, STACK2_LDS_BYTES).total > LDS_DYNAMIC_MAX) {
                    ok = false;
                    h->stack2_why = "the flux-sum table does not fit the LDS next to this configuration's tables";
                }
            if (ok && !stack2_redo_geometry(P).fits) {
                ok = false;
                h->stack2_why = "the curves of one sample (filters x sample times) do not fit the LDS staging of the re-evaluation kernel";
            }
            h->stack2_ok = ok ? 1 : 0;
            // log Phi for the flavour's upper limits from the table (round 6: the folded rows leave the room): taken where it costs
            // neither tile size a ring slot or the photometry staging
            P.mass_tab2 = 0;
            if (ok && comb_lim) {          // the truncation mass (and the upper limits time nodes can turn detections into) needs the table: no room for it, no one-launch form
                for (int r = 1; r <= 2; ++r)
                    if (lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                        P.has_ebv ? P.n_items : 1, h->ring_max, P.dat_in_tab ? 8 : 32, 0, STACK2_LDS_BYTES + LOGPHI_LDS_BYTES).total > LDS_DYNAMIC_MAX) ok = false;
                if (!ok) h->stack2_why = "finite detection limits / time-node systematics: the table of log Phi does not fit the LDS next to the flux-sum table";
                h->stack2_ok = ok ? 1 : 0;
                P.mass_tab2 = ok ? 1 : 0;
            } else if (ok && h->n_ul_items > 0 && !getenv("NMMA_EM_NO_UL_TAB")) {
                bool tab_ok = true;
                for (int r = 1; r <= 2; ++r) {
                    const LdsW L0 = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                                    P.has_ebv ? P.n_items : 1, h->ring_max, P.dat_in_tab ? 8 : 32, 0, STACK2_LDS_BYTES);
                    const LdsW L1 = lds_layout_logl(r, lds_ns_arg(P), nf_avg_max, P.tab_bytes, P.tab_fast_bytes, P.n_items, M, NP, 1, N, P.n_sys_slots,
                                                    P.has_ebv ? P.n_items : 1, h->ring_max, P.dat_in_tab ? 8 : 32, 0, STACK2_LDS_BYTES + LOGPHI_LDS_BYTES);
                    if (L1.total > LDS_DYNAMIC_MAX || L1.nbuf != L0.nbuf || (L1.dat >= 0) != (L0.dat >= 0)) tab_ok = false;
                }
                P.mass_tab2 = tab_ok ? 1 : 0;
            }
        }
        NM_UP(desc, item_desc);
        for (int r = 0; r < 2; ++r) {               // fast mode: (item, sample chunk) of every task of one tile, item-major
            std::vector<int32_t> tmap;
            if (P.all_fast)
                for (int k = 0; k < P.n_items; ++k) {
                    // (an averaged band's tasks belong to its last source item; the other sources carry the same count for the
                    //  ring hand-off -- every task of the band signals each of them -- but own no tasks)
                    if (desc[k].ks != desc[k].nsrc - 1) continue;
                    for (int cidx = 0; cidx < desc[k].ntask[r]; ++cidx) tmap.push_back((k << 8) | cidx);
                }
            P.n_tasks[r] = (int32_t)tmap.size();
            if (tmap.empty()) tmap.push_back(0);
            hipError_t _e = upload(tmap, &P.task_map[r], h->owned);
            if (_e != hipSuccess) { nmma_em_destroy(h); return fail(std::string("upload task_map failed: ") + hipGetErrorString(_e)); }
        }
        // Small batches (launch_logl): the bands of the lean family can run as separate workgroups -- band b = the work items
        // [k0, k0 + n) of one observed filter with its own task map (local item index << 8 | sample chunk).
        if (P.all_fast == 1 && P.n_items >= 2) {
            for (int k = 0; k < P.n_items; ++k) {
                if (desc[k].ks != 0) continue;
                h->band_k0.push_back(k);
                h->band_nitems.push_back(desc[k].nsrc);
            }
            // partitions into groups of g = 1, 2, 3 adjacent bands (a group = the contiguous items of its bands); band_grp_*: flat over
            // the partitions, in the order band_dev is built below
            const int nb = (int)h->band_k0.size();
            int prev_groups = -1;
            for (int g = 1; g <= 3; ++g) {
                const int ng = (nb + g - 1) / g;
                if (ng < 2 || ng == prev_groups) continue;
                prev_groups = ng;
                h->lvl_off[g - 1] = (int)h->grp_k0.size();
                h->lvl_n[g - 1] = ng;
                for (int j = 0; j < ng; ++j) {
                    const int b0 = j * g, b1 = std::min(nb, b0 + g);
                    const int k0 = h->band_k0[b0];
                    int nit = 0;
                    for (int b = b0; b < b1; ++b) nit += h->band_nitems[b];
                    h->grp_k0.push_back(k0);
                    h->grp_nitems.push_back(nit);
                    for (int r = 0; r < 2; ++r) {
                        std::vector<int32_t> tm;
                        for (int b = b0; b < b1; ++b) {
                            const int k = h->band_k0[b] + h->band_nitems[b] - 1, kl = k - k0;
                            for (int cidx = 0; cidx < desc[k].ntask[r]; ++cidx) tm.push_back((kl << 8) | cidx);
                        }
                        h->band_ntasks[r].push_back((int)tm.size());
                        if (tm.empty()) tm.push_back(0);
                        const int32_t* dptr = nullptr;
                        hipError_t _e = upload(tm, &dptr, h->owned);
                        if (_e != hipSuccess) { nmma_em_destroy(h); return fail(std::string("upload band task_map failed: ") + hipGetErrorString(_e)); }
                        h->band_tmap[r].push_back(dptr);
                    }
                }
            }
        }
    }
#undef NM_UP
    // SURVEY.md section 8d: F_eval = sum over evaluated (observed filter, source) pairs of
    // 2*NP*NH + 2*NH*NC + 2*NC*NT
    {
        int64_t pairs = 0;
        std::vector<int32_t> ns(O);
        for (int o = 0; o < O; ++o) pairs += c->n_sources ? c->n_sources[o] : 1;
        h->flops_per_eval = svd ? pairs * (2LL * NP * NH + 2LL * NH * NC + 2LL * NC * NT) : 0;
    }
    {   // watchdog words: pinned host memory the kernels write through (read without a device round trip)
        void* wh = nullptr; void* wd = nullptr;
        hipError_t e = hipHostMalloc(&wh, 4 * sizeof(int), hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&wd, wh, 0);
        if (e != hipSuccess) { nmma_em_destroy(h); return fail(std::string("watchdog allocation failed: ") + hipGetErrorString(e)); }
        h->wd_host = static_cast<int*>(wh);
        for (int i = 0; i < 4; ++i) h->wd_host[i] = 0;
        h->dev.watchdog = static_cast<int*>(wd);
    }
    {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, sizeof(EmDev));
        if (e == hipSuccess) e = hipMemcpy(p, &h->dev, sizeof(EmDev), hipMemcpyHostToDevice);
        if (e != hipSuccess) { nmma_em_destroy(h); return fail(std::string("upload EmDev failed: ") + hipGetErrorString(e)); }
        h->owned.push_back(p);
        h->dev_d = reinterpret_cast<EmDev*>(p);
    }
    if (!h->grp_k0.empty()) {
        for (size_t b = 0; b < h->grp_k0.size(); ++b) {
            EmDev Pb = h->dev;
            Pb.items = h->dev.items + 4 * h->grp_k0[b];
            Pb.item_desc = h->dev.item_desc + h->grp_k0[b];
            Pb.n_items = h->grp_nitems[b];
            for (int g = 0; g < 3; ++g)
                if (h->lvl_n[g] > 0 && (int)b >= h->lvl_off[g] && (int)b < h->lvl_off[g] + h->lvl_n[g]) Pb.n_bands = h->lvl_n[g];   // groups of ITS partition
            for (int r = 0; r < 2; ++r) { Pb.task_map[r] = h->band_tmap[r][b]; Pb.n_tasks[r] = h->band_ntasks[r][b]; }
            h->band_dev.push_back(Pb);
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, h->band_dev.size() * sizeof(EmDev));
        if (e == hipSuccess) e = hipMemcpy(p, h->band_dev.data(), h->band_dev.size() * sizeof(EmDev), hipMemcpyHostToDevice);
        if (e != hipSuccess) { nmma_em_destroy(h); return fail(std::string("upload of the per-band EmDev copies failed: ") + hipGetErrorString(e)); }
        h->owned.push_back(p);
        h->band_dev_d = reinterpret_cast<EmDev*>(p);
        if (const char* ev = getenv("NMMA_EM_SPLIT")) h->split_mode = atoi(ev) != 0 ? 1 : 0;
        if (const char* ev = getenv("NMMA_EM_SPLIT_MAX_WG")) h->split_max_wg = std::max(1, atoi(ev));
        if (const char* ev = getenv("NMMA_EM_SPLIT_FILL_WG")) h->split_fill_wg = std::max(1, atoi(ev));
    }
    if (const char* ev = getenv("NMMA_EM_HOST_POLL")) h->host_poll = atoi(ev) != 0 ? 1 : 0;
    if (getenv("NMMA_WALK_NO_FUSE")) h->walk_fuse = 0;
    if (getenv("NMMA_WALK_NO_SPLIT")) h->walk_split = 0;
    if (const char* ev = getenv("NMMA_LC_GROUP")) h->lc_group = atoi(ev);
    if (getenv("NMMA_LC_NO_GROUPS")) h->lc_group = 64;
    if (getenv("NMMA_STACK2_NO_FIXUP")) h->stack2_fixup = 0;
    *out = h;
    return 0;
}

void nmma_em_destroy(nmma_em_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (void* p : h->owned) (void)hipFree(p);
    if (h->chi) (void)hipFree(h->chi);
    if (h->gap_ws) (void)hipFree(h->gap_ws);
    if (h->lc_ws) (void)hipFree(h->lc_ws);
    if (h->ext_ws) (void)hipFree(h->ext_ws);
    if (h->split_ws) (void)hipFree(h->split_ws);
    for (auto& rs : h->regrid_sets) if (rs.dev) (void)hipFree(rs.dev);
    if (h->theta_stage) (void)hipFree(h->theta_stage);
    if (h->out_stage) (void)hipFree(h->out_stage);
    for (auto e : h->ev) (void)hipEventDestroy(e);
    if (h->wd_host) (void)hipHostFree(h->wd_host);
    if (h->theta_pin) (void)hipHostFree(h->theta_pin);
    if (h->out_pin) (void)hipHostFree(h->out_pin);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    delete h;
}

// A tripped hand-off watchdog (see sync_wait in em_kernels.hip) poisons the handle: every later call fails loudly.
static int watchdog_tripped(nmma_em_handle* h, const char* who) {
    volatile int* w = h->wd_host;
    if (!w || w[0] == 0) return 0;
    char buf[320];
    if (w[1] == 950)      // (not a hand-off: nmma_em_loglike_stack2 was promised gap-free curves and met a gap)
        snprintf(buf, sizeof(buf), "%s: an earlier nmma_em_loglike_stack2 call with NMMA_STACK2_GAP_FREE met a non-finite node strictly inside "
                 "the second transient's curves (tile %d, row %d of the tile): those rows were floored instead of re-evaluated -- "
                 "results of that call are invalid; drop the flag for such operands", who, w[2], w[3]);
    else
        snprintf(buf, sizeof(buf), "%s: em_logl hand-off watchdog tripped (code %d, workgroup %d wave %d, counter %d of %d): "
                 "results of that launch are invalid", who, w[1], w[2] / 64, w[2] % 64, w[3] / 65536, w[3] % 65536);
    return fail(buf);
}

static int check_call(nmma_em_handle* h, const void* theta, int64_t B, int64_t ld, const char* who) {
    if (!h) return fail(std::string(who) + ": null handle");
    if (watchdog_tripped(h, who)) return 1;
    if (B < 0) return fail(std::string(who) + ": negative batch");
    if (B > 0 && !theta) return fail(std::string(who) + ": null theta");
    if (ld < h->dev.D) return fail(std::string(who) + ": leading dimension smaller than n_dim");
    return 0;
}
// A handle created with nmma_em_config::base_times (combined model on a union grid) has no meaning for the entry points that take the
// surrogate ALONE as the likelihood's model, in the detector frame: they refuse it.
static int refuse_stack2_only(const nmma_em_handle* h, const char* who) {
    if (!h->stack2_only) return 0;
    return fail(std::string(who) + ": the handle was created with base_times / null_filters / stack_operands under finite detection limits or time-node systematics "
                "(a combined model on a union grid, with bands the surrogate has nothing for, or with terms only its combined-model flavour carries): it serves "
                "nmma_em_loglike_stack2, nmma_em_model_lightcurves, nmma_em_coefficients and the "
                "calls that take curves");
}

static int ensure_lc_ws(nmma_em_handle* h, int64_t B);
static int launch_model_lc(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, double* lc, hipStream_t s);
static int launch_lc_loglike(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, const double* lc,
                             double* out, double* chi, double* gp, hipStream_t s, const double* const* more_sets = nullptr, int n_sets = 1,
                             const unsigned char* bad_rows = nullptr);

static int ensure_scratch(nmma_em_handle* h, int64_t B) {
    if (B <= h->parts_cap) return 0;
    if (h->chi) (void)hipFree(h->chi);
    h->chi = nullptr;
    h->parts_cap = 0;
    NM_HIP(hipMalloc(reinterpret_cast<void**>(&h->chi), B * sizeof(double)));
    h->parts_cap = B;
    return 0;
}

int32_t nmma_em_loglike_parts(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* chi_dev,
                              double* gp_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike_parts")) return 1;
    if (refuse_stack2_only(h, "nmma_em_loglike_parts")) return 1;
    if (B == 0 || h->dev.O == 0) return 0;
    if (!chi_dev || !gp_dev) return fail("nmma_em_loglike_parts: null output");
    NM_HIP(hipSetDevice(h->device));
    if (ensure_scratch(h, B)) return 1;    // the total logL is produced anyway; discard it
    if (h->dev.model_kind != NMMA_MODEL_SVD) {
        if (ensure_lc_ws(h, B)) return 1;
        if (launch_model_lc(h, theta_dev, B, ld, h->lc_ws, static_cast<hipStream_t>(stream))) return 1;
        return launch_lc_loglike(h, theta_dev, B, ld, h->lc_ws, h->chi, chi_dev, gp_dev, static_cast<hipStream_t>(stream));
    }
    NM_HIP(launch_logl(h, theta_dev, B, ld, h->chi, chi_dev, gp_dev, static_cast<hipStream_t>(stream)));
    return 0;
}

int32_t nmma_em_loglike(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* out_dev,
                        void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike")) return 1;
    if (refuse_stack2_only(h, "nmma_em_loglike")) return 1;
    if (B == 0) return 0;
    if (!out_dev) return fail("nmma_em_loglike: null output");
    NM_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // event pairs bracket every prof_stride-th launch (keeps the profiled run launch-for-launch
    // identical to an unprofiled one except for two event records on the sampled launches)
    if (h->dev.model_kind != NMMA_MODEL_SVD) {
        if (ensure_lc_ws(h, B)) return 1;
        if (launch_model_lc(h, theta_dev, B, ld, h->lc_ws, s)) return 1;
        return launch_lc_loglike(h, theta_dev, B, ld, h->lc_ws, out_dev, nullptr, nullptr, s);
    }
    // profiling: an event pair brackets `prof_group` consecutive launches, every `prof_stride`-th group.
    // A pair around ONE ~35 us launch over-reads by the dispatch latency behind the start event (~3 us);
    // bracketing a back-to-back group amortises it (use group 1 when other work is enqueued between launches).
    const long call = h->prof_on ? h->prof_calls++ : 0;
    const long grp = call / h->prof_group, pos = call % h->prof_group;
    const bool prof = h->prof_on && h->prof_n < h->prof_cap && (grp % h->prof_stride) == 0;
    if (prof && pos == 0) NM_HIP(hipEventRecord(h->ev[2 * h->prof_n + 0], s));
    NM_HIP(launch_logl(h, theta_dev, B, ld, out_dev, nullptr, nullptr, s));
    if (prof && pos == h->prof_group - 1) {
        NM_HIP(hipEventRecord(h->ev[2 * h->prof_n + 1], s));
        ++h->prof_n;
    }
    return 0;
}

// Run-time options of a handle (what the environment variables NMMA_WALK_NO_FUSE, NMMA_WALK_NO_SPLIT, NMMA_LC_GROUP,
// NMMA_STACK2_NO_FIXUP set at nmma_em_create): A/B measurements and tests switch them between calls.
int32_t nmma_em_set_option(nmma_em_handle* h, const char* name, int32_t value) {
    if (!h || !name) return fail("nmma_em_set_option: null argument");
    const std::string n(name);
    if (n == "walk_fuse") h->walk_fuse = value < 0 ? 0 : value > 2 ? 2 : (int)value;   // (2: also where two launches measured faster)
    else if (n == "walk_lanes") { if (value != 0 && value != 16) return fail("nmma_em_set_option: walk_lanes is 0 or 16"); h->walk_lanes = value; }
    else if (n == "walk_split") h->walk_split = value != 0;
    else if (n == "lc_group") { if (value != 0 && value != 16 && value != 32 && value != 64) return fail("nmma_em_set_option: lc_group is 0, 16, 32 or 64"); h->lc_group = value; }
    else if (n == "stack2_fixup") h->stack2_fixup = value != 0;
    else if (n == "sc_tile") { if (value < 0 || value > 64) return fail("nmma_em_set_option: sc_tile is 0 .. 64"); h->sc_tile = value; }
    else if (n == "sc_probe") { if (value < 0 || value > 2) return fail("nmma_em_set_option: sc_probe is 0, 1 or 2"); h->sc_probe = value; }
    else return fail("nmma_em_set_option: unknown option '" + n + "'");
    return 0;
}

// The MCMC step fused into the likelihood launch (em_logl<..., WALKF>): every lean task flavour carries it at 16-sample tiles, with 8
// or 16 lanes per chain (up to 16 sampled dimensions) and, for the flavours instantiated with it, the chains' Constraint program
// (n_con_ops > 0: evaluated on an fp64 stack in LDS).  Anything else returns 2 and the caller launches likelihood and walk step separately.
int32_t nmma_em_loglike_walk(nmma_em_handle* h, double* theta_dev, int64_t B, int64_t ld, double* out_dev, const nmma_walk_fuse* wf_dev,
                             uint64_t step, int32_t last, int32_t n_con_ops, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike_walk")) return 1;
    if (refuse_stack2_only(h, "nmma_em_loglike_walk")) return 1;
    if (!out_dev || !wf_dev) return fail("nmma_em_loglike_walk: null argument");
    if (n_con_ops < 0 || n_con_ops > NMMA_CON_MAX_OPS) return fail("nmma_em_loglike_walk: bad n_con_ops");
    if (B == 0) return 0;
    const EmDev& P = h->dev;
    if (P.model_kind != NMMA_MODEL_SVD || P.all_fast != 1 || P.p92_tab || h->prof_on || P.D > 16 || ld != P.D || !h->walk_fuse)
        return 2;
    NM_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (16-sample tiles up to one round of workgroups -- 4096 chains; 32-sample tiles beyond, as the likelihood alone)
    const int KP = P.KP;
    const int R = choose_r(h, B);
    // (A queue small enough for the band split of the likelihood -- up to ~2048 chains for config 2 -- is split here too: the group
    //  that adds a tile's bands runs the tile's MCMC step.  Option "walk_split" = 0: every workgroup walks all bands, as in round 4's
    //  first form, which lost to two launches per step below 2048 chains: 256 chains x 100 steps 3.11 against 2.17 ms.)
    // Lanes per chain: 8 up to 8 sampled dimensions, 16 up to 16.  The second phase of the step gives each round of 64 / lanes chains
    // a likelihood wave of its own (16-sample tiles: two waves for 8 lanes, four for 16; 32-sample tiles: four and eight -- on ONE
    // wave the four rounds cost what the separate walk launch costs, profiles/r05_fused_mcmc_step.md).
    const int flavour = P.dense ? 6 : P.lean_gen ? 5 : !P.lean_x ? 1 : P.st_uniform ? 3 : 4;
    // Which forms exist (round 6: the set was cut from 64 to 40 instantiations by measurement, profiles/r06_instantiations.md):
    //  * 16-sample tiles (up to 4096 chains): 8 or 16 lanes per chain for every lean flavour; with a Constraint program for the plain
    //    lean task and the lean tasks with extras (the flavours of the default priors);
    //  * 32-sample tiles (beyond 4096 chains): 16 lanes per chain ONLY, whatever the number of sampled dimensions (8 lanes gained 0-2 %
    //    over 16 there), no Constraint program (its step gained 0-4 % over two launches at 8 lanes and lost at 16), not the dense task
    //    (1.4 %): those queues take two launches per step.
    const int wt = (R == 2 || P.D > 8 || h->walk_lanes == 16) ? 16 : 8;
    if (R == 2 && (n_con_ops > 0 || flavour == 6)) return 2;
    // (measured exception: the dense lean task with 16 lanes per chain at a full round of workgroups -- config 4's shape with
    //  em_syserr, 9 dimensions, 4096 chains x 100 steps: fused 9.99 ms against 9.87 ms as two launches; 1024 chains: 3.95 against 4.31)
    if (flavour == 6 && wt == 16 && B > 2048 && h->walk_fuse < 2) return 2;
    // (forms whose parked state leaves the log Phi table of the upper limits no room without a ring slot: nmma_em_create)
    if (P.mass_tab && (flavour == 1 || flavour == 3 || flavour == 4) && ((h->walk_tab_mask >> (2 * (R - 1) + (wt == 16 ? 1 : 0))) & 1)) return 2;
    hipError_t e = hipErrorInvalidValue;
#ifdef NMMA_DEV_HEADLINE_ONLY
    if (R == 1 && KP == 1 && flavour == 1 && wt == 8 && n_con_ops == 0) e = launch_logl_one<1, 1, 8, 8, 1, 8>(h, theta_dev, B, ld, out_dev, nullptr, nullptr, s, wf_dev, step, last);
    else return 2;
#else
#define NM_WALK_R1(KK, FF, WW) launch_logl_one<1, KK, 8, 8, FF, WW>(h, theta_dev, B, ld, out_dev, nullptr, nullptr, s, wf_dev, step, last)
#define NM_WALK_R2(KK, FF) launch_logl_one<2, KK, 8, 8, FF, 16>(h, theta_dev, B, ld, out_dev, nullptr, nullptr, s, wf_dev, step, last)
#define NM_WALK_W(KK, FF) (R == 2 ? NM_WALK_R2(KK, FF) : n_con_ops > 0 ? (wt == 8 ? NM_WALK_R1(KK, FF, 72) : NM_WALK_R1(KK, FF, 80)) : (wt == 8 ? NM_WALK_R1(KK, FF, 8) : NM_WALK_R1(KK, FF, 16)))
#define NM_WALK_NOCON(KK, FF) (R == 2 ? NM_WALK_R2(KK, FF) : (wt == 8 ? NM_WALK_R1(KK, FF, 8) : NM_WALK_R1(KK, FF, 16)))
#define NM_WALK_R1ONLY(KK, FF) (wt == 8 ? NM_WALK_R1(KK, FF, 8) : NM_WALK_R1(KK, FF, 16))
    // (with a Constraint program: the plain lean task and the lean tasks with extras -- the flavours of the default priors; the general
    //  and the dense lean task keep two launches per step for constrained prior sets)
    if (n_con_ops > 0 && (flavour == 5 || flavour == 6)) return 2;
    switch (flavour) {
        case 1: e = KP == 1 ? NM_WALK_W(1, 1) : NM_WALK_W(2, 1); break;
        case 3: e = KP == 1 ? NM_WALK_W(1, 3) : NM_WALK_W(2, 3); break;
        case 4: e = KP == 1 ? NM_WALK_W(1, 4) : NM_WALK_W(2, 4); break;
        case 5: e = KP == 1 ? NM_WALK_NOCON(1, 5) : NM_WALK_NOCON(2, 5); break;
        default: e = KP == 1 ? NM_WALK_R1ONLY(1, 6) : NM_WALK_R1ONLY(2, 6); break;
    }
#undef NM_WALK_R1ONLY
#undef NM_WALK_NOCON
#undef NM_WALK_W
#undef NM_WALK_R2
#undef NM_WALK_R1
#endif
    // (the step's parked state enlarges the staging area: a configuration whose tables leave no room for it keeps two launches per step)
    if (e != hipSuccess && g_launch_note.find("more than 159 KiB") != std::string::npos) return 2;
    if (e != hipSuccess) return fail(std::string("nmma_em_loglike_walk: ") + (g_launch_note.empty() ? hipGetErrorString(e) : g_launch_note.c_str()));
    return 0;
}

static int ensure_lc_ws(nmma_em_handle* h, int64_t B) {
    const int64_t need = B * h->dev.M * h->dev.NS;
    if (need <= h->lc_cap) return 0;
    if (h->lc_ws) (void)hipFree(h->lc_ws);
    h->lc_ws = nullptr;
    h->lc_cap = 0;
    NM_HIP(hipMalloc(reinterpret_cast<void**>(&h->lc_ws), need * sizeof(double)));
    h->lc_cap = need;
    return 0;
}

extern "C++" {
// Instantiations: curves staged in LDS (SA) for every form; the unstaged fallback (curves read from memory) only for one
// materialised set and a wave per sample; the 16-lane groups only with the photometry staged (SD) -- a data set too large for
// that takes the wave-per-sample form.
template <int G, int NM>
static int launch_lc_loglike_as(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, const LcSets& sets, int n_sets,
                                const unsigned char* bad_rows, int per_sample, int stage_all, int stage_dat, int lds, double* out, double* chi,
                                double* gp, hipStream_t s) {
    if constexpr (G != 64) {
        return launch_lc_loglike_sd<G, NM, true, true>(h, theta, B, ld, sets, n_sets, bad_rows, per_sample, lds, out, chi, gp, s);
    } else {
        if constexpr (NM == 1) {
            if (!stage_all)
                return stage_dat ? launch_lc_loglike_sd<64, 1, true, false>(h, theta, B, ld, sets, n_sets, bad_rows, per_sample, lds, out, chi, gp, s)
                                 : launch_lc_loglike_sd<64, 1, false, false>(h, theta, B, ld, sets, n_sets, bad_rows, per_sample, lds, out, chi, gp, s);
        }
        return stage_dat ? launch_lc_loglike_sd<64, NM, true, true>(h, theta, B, ld, sets, n_sets, bad_rows, per_sample, lds, out, chi, gp, s)
                         : launch_lc_loglike_sd<64, NM, false, true>(h, theta, B, ld, sets, n_sets, bad_rows, per_sample, lds, out, chi, gp, s);
    }
}
}  // extern "C++"

// lc: the curves (n_sets == 1), or with more_sets the first of n_sets sets whose flux sum is the model (stacked while staged).
static int launch_lc_loglike(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, const double* lc,
                             double* out, double* chi, double* gp, hipStream_t s, const double* const* more_sets, int n_sets,
                             const unsigned char* bad_rows) {
    const EmDev& P = h->dev;
    // LDS: [sample times | cosmology grid | photometry | item descriptors] per block, then per sample app[NS] | estacc | praw | scal
    // and -- when the block's samples fit 64 KiB, which keeps two or more blocks per CU -- all of the sample's curves
    const bool cosmo_lds = P.redshift_mode == NMMA_Z_GRID && P.n_cosmo <= STAGE_COSMO;
    const int grid_bytes = ((P.NS + (cosmo_lds ? 2 * P.n_cosmo : 0)) * 8 + 15) & ~15;
    // the photometry and the item descriptors next to the grids (the kernel's datum loop then never leaves the chip)
    const int stage_dat = (P.n_data <= 1024) ? 1 : 0;
    const int shared_bytes = stage_dat ? ((grid_bytes + 5 * P.n_data * 8 + ((P.n_data + 3) & ~3) * 4 + P.n_items * ITEM_WORDS * 4 + 15) & ~15) : grid_bytes;
    const int base = (P.NS + P.lc_nf_max + 16) * 8, slab = base + P.M * P.NS * 8;
    LcSets sets{};
    sets.p[0] = lc;
    for (int k = 1; k < n_sets; ++k) sets.p[k] = more_sets[k];
    // Lanes per sample (measured at config 3's shape, 8192 rows x 9 filters x 41 nodes, two sets stacked on chip; rocprofv3 kernel
    // times of back-to-back calls, profiles/r04_models_*): 32 lanes 37.4 us, 16 lanes 41.6 us, 64 lanes 48.3 us (one
    // materialised set: 28.1 / 35.8 / 42.1 us).  The instruction count falls with the group size (SQ_INSTS_VALU 14.7 M against
    // 21.8 M for 16 / 64 lanes: the per-sample scalar chain and the partly filled last pass are shared by the samples of a wave),
    // but the LDS slabs of the curves allow ~44 samples per CU whatever the grouping: a wave per sample is bound by VALU issue
    // (84 % busy), 16-lane groups run two waves per SIMD and are bound by one wave's serial latency (58 % busy); two samples per
    // wave sit between the two.  NMMA_LC_GROUP=16|32|64 forces one (a form whose slabs do not fit falls to the next).
    // Up to 2048 rows -- at most two workgroups per CU as waves per sample -- the launch is one workgroup's chain of latencies, and a
    // wave per sample has the shortest chain (three trips over the data instead of five: 18.6-19.9 us against 22.7-23.2 us at config
    // 3's shape and 512-2048 rows; 26.0 = 26.0 at 4096; 45 against 35 at 8192, where a wave per sample needs a second round).  A
    // row's sum does not depend on the grouping (group_total_canon: same bits), so it does not depend on the size of its batch either.
    int want = B <= 2048 ? 64 : 32;
    if (h->lc_group == 16 || h->lc_group == 32 || h->lc_group == 64) want = h->lc_group;      // (nmma_em_set_option "lc_group" / NMMA_LC_GROUP at create)
    // (two sets: the flux-sum table of lc_stack_node borrows the photometry region while the curves are staged; behind the slabs otherwise)
    const int tab = (n_sets == 2 && !(stage_dat && shared_bytes - grid_bytes >= STACK2_LDS_BYTES)) ? STACK2_LDS_BYTES : 0;
    const bool fits16 = stage_dat && shared_bytes + 16 * slab + tab <= 80 * 1024 && chi == nullptr;      // (two blocks per CU)
    // (four blocks per CU; measured in round 6 at 9 filters x 77 nodes and 11 filters x 41 nodes: letting the 32-lane form grow to 54 / 80 / 159 KiB
    //  -- three / two / one block per CU -- is SLOWER than the wave per sample it would replace: 304-375 against 288-312 us for the path)
    const bool fits32 = stage_dat && shared_bytes + 8 * slab + tab <= 40 * 1024 && chi == nullptr;
    const bool fits64 = shared_bytes + 4 * slab + tab <= 64 * 1024;
    if (n_sets > 1 && !fits64) return fail("nmma_em_loglike_lc_sets: the curves of one sample do not fit the LDS staging; stack them with nmma_lc_stack first");
    if (want == 16 && fits16) {
        const int lds = shared_bytes + 16 * slab + tab;
        if (n_sets == 1) return launch_lc_loglike_as<16, 1>(h, theta, B, ld, sets, 1, bad_rows, slab, 1, stage_dat, lds, out, chi, gp, s);
        if (n_sets == 2) return launch_lc_loglike_as<16, 2>(h, theta, B, ld, sets, 2, bad_rows, slab, 1, stage_dat, lds, out, chi, gp, s);
        return launch_lc_loglike_as<16, 0>(h, theta, B, ld, sets, n_sets, bad_rows, slab, 1, stage_dat, lds, out, chi, gp, s);
    }
    if (want <= 32 && fits32) {
        const int lds = shared_bytes + 8 * slab + tab;
        if (n_sets == 1) return launch_lc_loglike_as<32, 1>(h, theta, B, ld, sets, 1, bad_rows, slab, 1, stage_dat, lds, out, chi, gp, s);
        if (n_sets == 2) return launch_lc_loglike_as<32, 2>(h, theta, B, ld, sets, 2, bad_rows, slab, 1, stage_dat, lds, out, chi, gp, s);
        return launch_lc_loglike_as<32, 0>(h, theta, B, ld, sets, n_sets, bad_rows, slab, 1, stage_dat, lds, out, chi, gp, s);
    }
    const int per = fits64 ? slab : base;
    const int lds = shared_bytes + 4 * per + tab;
    if (n_sets == 1) return launch_lc_loglike_as<64, 1>(h, theta, B, ld, sets, 1, bad_rows, per, fits64 ? 1 : 0, stage_dat, lds, out, chi, gp, s);
    if (n_sets == 2) return launch_lc_loglike_as<64, 2>(h, theta, B, ld, sets, 2, bad_rows, per, 1, stage_dat, lds, out, chi, gp, s);
    return launch_lc_loglike_as<64, 0>(h, theta, B, ld, sets, n_sets, bad_rows, per, 1, stage_dat, lds, out, chi, gp, s);
}

static int launch_model_lc(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, double* lc, hipStream_t s) {
    const EmDev& P = h->dev;
    if (P.model_kind == NMMA_MODEL_ME2017) {
        const int per_wave = (7 * P.NS + me17::MPREC) * 8;
        const int lds = per_wave * 4;
        if (lds > 64 * 1024)
            NM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&me2017_lc),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(me2017_lc, dim3((unsigned)((B + 3) / 4)), dim3(256), lds, s, h->dev_d, theta, (long)B,
                           (long)ld, per_wave, lc);
        NM_HIP(hipGetLastError());
        return 0;
    }
    if (P.model_kind == NMMA_MODEL_PIRO2021) return launch_piro2021_lc(h, theta, B, ld, lc, s);
    if (P.model_kind == NMMA_MODEL_HONA2020) return launch_hona2020_lc(h, theta, B, ld, lc, nullptr, s);
    return fail("this handle's model has no light-curve kernel (NMMA_MODEL_EXTERNAL: supply the curves)");
}

int32_t nmma_em_model_lightcurves(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* lc_dev,
                                  void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_model_lightcurves")) return 1;
    if (B == 0) return 0;
    if (!lc_dev) return fail("nmma_em_model_lightcurves: null output");
    NM_HIP(hipSetDevice(h->device));
    if (h->dev.model_kind == NMMA_MODEL_SVD) {
        NM_HIP(launch_aux(h, theta_dev, B, ld, MODE_LC_ABS, nullptr, nullptr, lc_dev, static_cast<hipStream_t>(stream)));
        return 0;
    }
    return launch_model_lc(h, theta_dev, B, ld, lc_dev, static_cast<hipStream_t>(stream));
}

int32_t nmma_em_hona_steps(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, int32_t* steps_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_hona_steps")) return 1;
    if (h->dev.model_kind != NMMA_MODEL_HONA2020) return fail("nmma_em_hona_steps: not a HoNa2020 handle");
    if (B == 0) return 0;
    if (!steps_dev) return fail("nmma_em_hona_steps: null output");
    NM_HIP(hipSetDevice(h->device));
    if (ensure_lc_ws(h, B)) return 1;
    return launch_hona2020_lc(h, theta_dev, B, ld, h->lc_ws, steps_dev, static_cast<hipStream_t>(stream));
}

int32_t nmma_em_loglike_lc(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, const double* lc_dev,
                           double* out_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike_lc")) return 1;
    if (B == 0) return 0;
    if (!lc_dev || !out_dev) return fail("nmma_em_loglike_lc: null buffer");
    NM_HIP(hipSetDevice(h->device));
    return launch_lc_loglike(h, theta_dev, B, ld, lc_dev, out_dev, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int32_t nmma_em_loglike_lc_sets(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, const double* const* lc_dev_sets,
                                int32_t n_sets, const uint8_t* bad_rows_dev, double* out_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike_lc_sets")) return 1;
    if (!lc_dev_sets || n_sets < 1 || n_sets > 8 || !out_dev) return fail("nmma_em_loglike_lc_sets: bad argument (1 .. 8 curve sets)");
    for (int k = 0; k < n_sets; ++k)
        if (!lc_dev_sets[k]) return fail("nmma_em_loglike_lc_sets: null curve set");
    if (B == 0) return 0;
    NM_HIP(hipSetDevice(h->device));
    return launch_lc_loglike(h, theta_dev, B, ld, lc_dev_sets[0], out_dev, nullptr, nullptr, static_cast<hipStream_t>(stream), lc_dev_sets, n_sets,
                             bad_rows_dev);
}

// One NODE of one curve (b, m) per thread -- the curves of a set are contiguous, so a wave covers 64 consecutive nodes whatever
// the grid length (one wave per curve left a third of the lanes idle for the CLI grid's 41 nodes and made every wave a chain of
// load -> exp / log -> store with nothing to overlap: 41 us for 8192 x 9 curves, 0.22 of the HBM roofline; 27.5 us with a node per
// thread; now lc_stack_kernel below, DESIGN 3.4).
// Per-model gap filling as autocomplete_data(connected_times, ref_times, lc, extrapolate=inf) does on a common grid
// (model.py:1440-1448; utils.py:634-645), then stack_magnitudes (model.py:1486-1510): -2.5 * logsumexp_k(-0.4 ln10 mag_k) / ln10.
extern "C++" {
// NPT nodes per thread, 256 nodes apart (coalesced), ALL their loads issued before the first is used: with one node per thread a
// workgroup was a single load -> compute -> store chain and the launch six rounds of such chains (latency, not bandwidth: DESIGN 3.4).
// NM = 2 (kilonova + afterglow, the reference's combined models) is compiled with the model loop unrolled; NM = 0: any count up to 8.
template <int NM, int NPT>
__global__ __launch_bounds__(256) void lc_stack_kernel(const EmDev* __restrict__ Pp, const LcSets sets, const int n_models_rt,
                                                       const long n_nodes, double* __restrict__ out) {
    const EmDev& P = *Pp;
    constexpr int KM = NM > 0 ? NM : 8;
    const int n_models = NM > 0 ? NM : n_models_rt;
    const long g0 = (long)blockIdx.x * (NPT * 256) + threadIdx.x;
    __shared__ __attribute__((aligned(16))) double tab2[NM == 2 ? STACK2_NINT * STACK2_ROW : 2];
    if constexpr (NM == 2) stack2_stage(tab2, threadIdx.x, 256);      // (the loads below are in flight while the table lands)
    double v[NPT][KM];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const long g = g0 + i * 256;
#pragma unroll
        for (int k = 0; k < KM; ++k) v[i][k] = (k < n_models && g < n_nodes) ? sets.p[k][g] : 0.0;
    }
    if constexpr (NM == 2) __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const long g = g0 + i * 256;
        if (g < n_nodes) out[g] = lc_stack_node<KM>(P, sets, n_models, g, v[i], NM == 2 ? tab2 : nullptr);
    }
}
}  // extern "C++"

// stack2_redo's geometry: em_lc_loglike's LDS layout for two sets (launch_lc_loglike) next to em_fused's (lds_layout), whichever is larger.
constexpr long STACK2_REDO_GRID = 512;       // workgroups of the re-evaluation launch (each owns 32 rows of the curve workspace)
extern "C++" {
template <int KP, int G, bool SD>
static int launch_stack2_redo_one(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, const LcSets& sets, const unsigned char* bad_rows,
                                  int per_sample, int lds, const LdsOff& Lf, double* out, hipStream_t s) {
    if (lds > 64 * 1024)
        NM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&stack2_redo<KP, G, SD>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const long n_tiles = (long)((B + 31) / 32);
    const unsigned gx = (unsigned)std::min<long>(n_tiles, STACK2_REDO_GRID);        // (two workgroups per CU; each looks at every gx-th tile's flags)
    hipLaunchKernelGGL((stack2_redo<KP, G, SD>), dim3(gx), dim3(256), lds, s, h->dev_d, theta, (long)B, (long)ld, Lf, h->lc_ws, sets, bad_rows,
                       per_sample, h->always_floor, out, h->gap_ws);
    NM_HIP(hipGetLastError());
    return 0;
}
}  // extern "C++"

static int launch_stack2_redo(nmma_em_handle* h, const double* theta, int64_t B, int64_t ld, const double* lc2, const unsigned char* bad_rows,
                              double* out, hipStream_t s) {
    const EmDev& P = h->dev;
    const Stack2RedoGeo g = stack2_redo_geometry(P);
    if (!g.fits) return fail("nmma_em_loglike_stack2: the curves of one sample do not fit the LDS staging of the re-evaluation kernel");   // (checked at create)
    const bool fits32 = g.fits32;
    const int stage_dat = g.stage_dat, slab = g.slab;
    const LdsOff Lf = lds_layout(MODE_LC_ABS, 2, P.NC, P.NT, P.NS);
    LcSets sets{};
    sets.p[0] = h->lc_ws; sets.p[1] = lc2;
    const int lds = std::max(g.lds_lc, (int)Lf.total);
    const int KP = P.KP;
    if (fits32) return KP == 1 ? launch_stack2_redo_one<1, 32, true>(h, theta, B, ld, sets, bad_rows, slab, lds, Lf, out, s)
                               : launch_stack2_redo_one<2, 32, true>(h, theta, B, ld, sets, bad_rows, slab, lds, Lf, out, s);
    if (stage_dat) return KP == 1 ? launch_stack2_redo_one<1, 64, true>(h, theta, B, ld, sets, bad_rows, slab, lds, Lf, out, s)
                                  : launch_stack2_redo_one<2, 64, true>(h, theta, B, ld, sets, bad_rows, slab, lds, Lf, out, s);
    return KP == 1 ? launch_stack2_redo_one<1, 64, false>(h, theta, B, ld, sets, bad_rows, slab, lds, Lf, out, s)
                   : launch_stack2_redo_one<2, 64, false>(h, theta, B, ld, sets, bad_rows, slab, lds, Lf, out, s);
}

// The combined model of two transients in one launch (em_logl<.., 7>), then the re-evaluation of the rows that kernel flagged.
int32_t nmma_em_loglike_stack2(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, const double* lc2_dev,
                               const uint8_t* bad_rows_dev, double* out_dev, int32_t flags, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike_stack2")) return 1;
    if (!h->stack2_ok) { g_last_error = "nmma_em_loglike_stack2: no one-launch form: " + h->stack2_why; return 2; }
    if (B == 0) return 0;
    if (!lc2_dev || !out_dev) return fail("nmma_em_loglike_stack2: null buffer");
    const EmDev& P = h->dev;
    const int64_t n_nodes = B * P.M * P.NS;
    if (n_nodes >= (int64_t)1 << 32) return fail("nmma_em_loglike_stack2: more than 2^32 curve nodes in one call (split the batch)");
    NM_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B > h->gap_cap) {
        if (h->gap_ws) (void)hipFree(h->gap_ws);
        h->gap_ws = nullptr; h->gap_cap = 0;
        const int64_t cap = (std::max<int64_t>(B, 4096) + 63) / 64 * 64;      // (whole tiles of 16 / 32 rows: the kernel writes every flag of its tiles)
        NM_HIP(hipMalloc(reinterpret_cast<void**>(&h->gap_ws), (size_t)cap));
        h->gap_cap = cap;
    }
    // (NMMA_STACK2_GAP_FREE: no flag array -- the kernel then reports a gap through the handle's watchdog words instead)
    const bool gap_free = (flags & NMMA_STACK2_GAP_FREE) != 0;
    // workspace of the re-evaluation launch: 32 rows of surrogate curves per workgroup (stack2_redo_tile), not B rows
    if (h->stack2_fixup && !gap_free && ensure_lc_ws(h, std::min<int64_t>((B + 31) / 32, STACK2_REDO_GRID) * 32)) return 1;
    NM_HIP(ext_prepass(h, theta_dev, B, ld, s));
    const EmAux aux{lc2_dev, bad_rows_dev, gap_free ? nullptr : h->gap_ws, (flags & NMMA_STACK2_COMPLETED) ? 1 : 0};
    const int R = choose_r(h, B), KP = P.KP;
    hipError_t e = hipErrorInvalidValue;
#ifndef NMMA_DEV_HEADLINE_ONLY
#define NM_ST2(RR, KK, FF) launch_logl_one<RR, KK, 8, 8, FF>(h, theta_dev, B, ld, out_dev, nullptr, nullptr, s, nullptr, 0, 0, aux)
    if (P.st_uniform) {
        if (R == 2) e = KP == 1 ? NM_ST2(2, 1, 7) : NM_ST2(2, 2, 7);
        else e = KP == 1 ? NM_ST2(1, 1, 7) : NM_ST2(1, 2, 7);
    } else {                    // unequally spaced sample_times (the CLI's log-spaced grid): FASTM 4's bracket search
        if (R == 2) e = KP == 1 ? NM_ST2(2, 1, 8) : NM_ST2(2, 2, 8);
        else e = KP == 1 ? NM_ST2(1, 1, 8) : NM_ST2(1, 2, 8);
    }
#undef NM_ST2
#endif
    if (e != hipSuccess) return fail(std::string("nmma_em_loglike_stack2: ") + (g_launch_note.empty() ? hipGetErrorString(e) : g_launch_note.c_str()));
    // Rows that met an interior gap of lc2 (gap_ws, written for every row by the launch above): ONE more launch, stack2_redo -- per
    // flagged tile the surrogate's curves (em_fused's body) and stack + likelihood from curves (em_lc_loglike's body) for the flagged
    // rows; a small grid that finds nothing to do in the usual case.  Option "stack2_fixup" = 0 (measurement only) skips it.
    if (!h->stack2_fixup || gap_free) return 0;
    return launch_stack2_redo(h, theta_dev, B, ld, lc2_dev, bad_rows_dev, out_dev, s);
}


int32_t nmma_lc_stack(nmma_em_handle* h, const double* const* lc_dev_sets, int32_t n_models, int64_t B,
                      double* out_dev, void* stream) {
    if (!h || !lc_dev_sets || n_models < 1 || n_models > 8 || B < 0 || !out_dev) return fail("nmma_lc_stack: bad argument");
    if (B == 0) return 0;
    NM_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    LcSets sets{};
    for (int k = 0; k < n_models; ++k) {
        if (!lc_dev_sets[k]) return fail("nmma_lc_stack: null curve set");
        sets.p[k] = lc_dev_sets[k];
    }
    const long n_curves = (long)B * h->dev.M;
    // asynchronous like the likelihood entry points: no allocation, no copy, no synchronisation per call
    const long n_nodes = n_curves * h->dev.NS;
    if (n_models == 2)
        hipLaunchKernelGGL((lc_stack_kernel<2, 4>), dim3((unsigned)((n_nodes + 1023) / 1024)), dim3(256), 0, s, h->dev_d, sets, n_models, n_nodes,
                           out_dev);
    else
        hipLaunchKernelGGL((lc_stack_kernel<0, 1>), dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, h->dev_d, sets, n_models, n_nodes,
                           out_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("nmma_lc_stack launch failed: ") + hipGetErrorString(e));
    return 0;
}

// One output curve (b, m) per wave: see nmma_lc_regrid in include/nmma_hip.h.
__global__ __launch_bounds__(256) void lc_regrid_kernel(const EmDev* __restrict__ Pp, const double* __restrict__ src, int Ms, int NSs,
                                                        const double* __restrict__ xs, const int* __restrict__ sidx,
                                                        const int* __restrict__ nsrc, long n_curves, double* __restrict__ out) {
    const EmDev& P = *Pp;
    const int lane = threadIdx.x & 63;
    const long cidx = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cidx >= n_curves) return;
    const int NS = P.NS, M = P.M;
    const long b = cidx / M;
    const int m = (int)(cidx - b * M);
    const int ns = nsrc[m];
    double* dst = out + (size_t)cidx * NS;
    for (int j0 = 0; j0 < NS; j0 += 64) {
        const int j = j0 + lane;
        const double x = P.st[j < NS ? j : NS - 1];
        double acc = 0.0;
        for (int k = 0; k < ns; ++k) {
            const double* cur = src + ((size_t)b * Ms + sidx[m * 3 + k]) * NSs;
            // finite nodes of this source curve: count, first, last (uniform over the wave)
            int nfin = 0, first = NSs, last = -1;
            for (int i = lane; i < NSs; i += 64) {
                const double v = cur[i];
                if (v - v == 0.0) { ++nfin; first = i < first ? i : first; last = i > last ? i : last; }
            }
            nfin = (int)wave_sum((double)nfin);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int of = __shfl_xor(first, off), ol = __shfl_xor(last, off);
                first = of < first ? of : first; last = ol > last ? ol : last;
            }
            double v = HUGE_VAL;                       // left = right = +inf; fewer than two finite nodes: all +inf
            if (nfin >= 2 && x >= xs[first] && x <= xs[last]) {
                int lo = first, hi = last;             // xs[lo] <= x <= xs[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (xs[mid] <= x) lo = mid; else hi = mid;
                }
                if (xs[hi] <= x) lo = hi;
                int jl = lo;
                while (jl >= first && !(cur[jl] - cur[jl] == 0.0)) --jl;
                int jr = lo + 1;
                while (jr <= last && !(cur[jr] - cur[jr] == 0.0)) ++jr;
                if (jl >= first) {
                    if (xs[jl] == x) v = cur[jl];
                    else if (jr <= last) v = lerp_np(x, xs[jl], xs[jr], cur[jl], cur[jr]);
                }
            }
            if (x != x) v = x;
            acc = (k == 0) ? v : acc + v;
        }
        double res = HUGE_VAL;
        if (ns == 1) res = acc;
        else if (ns > 1) res = acc / (double)ns;       // utils.average_mags: (a + b [+ c]) / n
        if (j < NS) dst[j] = res;
    }
}

// The same for source grids of up to REGRID_LDS_NODES nodes and output grids of up to REGRID_LDS_OUT (every grid met so far), built for
// the latency chain of one curve instead of its instruction count -- as a search through global memory per output node (the kernel
// above) the call took 95 us for config 3's shape on own grids (8192 x 9 curves, 36 -> 77 nodes: 66 MB of traffic, 8 us at the HBM
// rate), more than the likelihood launch it feeds:
//  * persistent workgroups: the source times, the output times, the filter plan and the BRACKET of every output node in the source
//    grid -- static: it depends on the two grids only; blo[j] = the last source node at or before st[j], -1 before the first, built by
//    the host call and uploaded with the set -- are staged in LDS once per workgroup, not fetched per curve;
//  * a wave walks curves cidx, cidx + n_waves, ...: the first 64 nodes of the NEXT curve's first source are requested before the
//    current curve is worked on (one register), so the global-memory latency of a curve passes behind the previous one;
//  * the finite nodes' count / first / last from wave ballots instead of shuffle reductions.
constexpr int REGRID_LDS_NODES = 1024, REGRID_LDS_OUT = 1024;      // (the layout stays under the 64 KiB a launch may take without asking)
__global__ __launch_bounds__(256) void lc_regrid_lds_kernel(const EmDev* __restrict__ Pp, const double* __restrict__ src, int Ms, int NSs,
                                                            const double* __restrict__ xs, const int* __restrict__ sidx,
                                                            const int* __restrict__ nsrc, const int* __restrict__ blo, long n_curves,
                                                            double* __restrict__ out) {
    const EmDev& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NS = P.NS, M = P.M;
    double* xs_l = reinterpret_cast<double*>(smem);
    double* st_l = xs_l + NSs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* cur = st_l + NS + wave * NSs;
    int* blo_l = reinterpret_cast<int*>(st_l + NS + 4 * NSs);
    int* plan_l = blo_l + NS;                   // [M][4]: source filters 0..2 | number of sources
    for (int i = threadIdx.x; i < NSs; i += 256) xs_l[i] = xs[i];
    for (int j = threadIdx.x; j < NS; j += 256) { st_l[j] = P.st[j]; blo_l[j] = blo[j]; }
    for (int i = threadIdx.x; i < M; i += 256) {
        plan_l[4 * i] = sidx[3 * i]; plan_l[4 * i + 1] = sidx[3 * i + 1]; plan_l[4 * i + 2] = sidx[3 * i + 2]; plan_l[4 * i + 3] = nsrc[i];
    }
    __syncthreads();
    const long n_waves = (long)gridDim.x * 4;
    long cidx = (long)blockIdx.x * 4 + wave;
    if (cidx >= n_curves) return;
    const double qnan = HUGE_VAL - HUGE_VAL;
    // first chunk of the first source of curve (b, m) (NaN where the curve has no such node or no source at all)
    auto head = [&](const long b, const int m) {
        return (plan_l[4 * m + 3] > 0 && lane < NSs) ? src[((size_t)b * Ms + plan_l[4 * m]) * NSs + lane] : qnan;
    };
    // (the curve index as (sample, filter), advanced without a 64-bit division per curve)
    long b = cidx / M;
    int m = (int)(cidx - b * M);
    const long step_b = n_waves / M;
    const int step_m = (int)(n_waves - step_b * M);
    double pre = head(b, m);
    constexpr int JMAX = 4;                      // output nodes per lane held in registers across the sources (a chunk of 256 output nodes)
    for (; cidx < n_curves; cidx += n_waves) {
        const int ns = plan_l[4 * m + 3];
        const double v_head = pre;
        long b_next = b + step_b;
        int m_next = m + step_m;
        if (m_next >= M) { m_next -= M; ++b_next; }
        if (cidx + n_waves < n_curves) pre = head(b_next, m_next);
        double* dst = out + (size_t)cidx * NS;
        for (int jc = 0; jc < NS; jc += 64 * JMAX) {
            double acc[JMAX];
#pragma unroll
            for (int q = 0; q < JMAX; ++q) acc[q] = 0.0;
            for (int k = 0; k < ns; ++k) {
                const double* g = src + ((size_t)b * Ms + plan_l[4 * m + k]) * NSs;
                // the source curve into this wave's LDS; finite nodes: count, first, last (uniform over the wave: ballots)
                int nfin = 0, first = NSs, last = -1;
                for (int i0 = 0; i0 < NSs; i0 += 64) {
                    const int i = i0 + lane;
                    const double v = (k == 0 && i0 == 0) ? v_head : (i < NSs ? g[i] : qnan);
                    if (i < NSs) cur[i] = v;
                    const unsigned long long fm = __ballot(i < NSs && (v - v == 0.0));
                    if (fm != 0) {
                        nfin += __popcll(fm);
                        if (first == NSs) first = i0 + __ffsll((long long)fm) - 1;
                        last = i0 + 63 - __clzll((long long)fm);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the curve is read across lanes below; LDS instructions of a wave execute in order)
                __builtin_amdgcn_wave_barrier();
                const double x_first = nfin >= 2 ? xs_l[first] : 0.0, x_last = nfin >= 2 ? xs_l[last] : 0.0;
                // The usual curve has no hole between its first and last finite node: the bracket is the static one, no walk to the finite
                // neighbours.  That path is STRAIGHT-LINE code over two slots of 64 output nodes at a time (lanes beyond the grid redo its
                // last node): a wave's work per node is one chain of dependent LDS reads and fp64 operations -- with six waves per SIMD the
                // kernel is bound by that chain's latency, and two independent chains interleave.  (np.interp's NaN fallbacks, lerp_np,
                // cannot trigger here: both values are finite and the nodes distinct; a lane whose bracket degenerates -- the last finite
                // node itself, or a node outside the window -- does not use the quotient.)
                const bool solid = nfin >= 2 && nfin == last - first + 1;      // uniform
                if (solid) {
#pragma unroll
                    for (int q0 = 0; q0 < JMAX; q0 += 2) {
                        if (jc + q0 * 64 >= NS) break;             // uniform
                        double vq[2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int j = jc + (q0 + u) * 64 + lane, jj = j < NS ? j : NS - 1;
                            const double x = st_l[jj];
                            const bool inside = x >= x_first && x <= x_last;
                            int lo = blo_l[jj];
                            lo = lo < first ? first : (lo > last ? last : lo);          // (only lanes outside the window are clamped)
                            const int hi = lo + 1 > last ? last : lo + 1;
                            const double x0 = xs_l[lo], y0 = cur[lo];
                            const double r = ((cur[hi] - y0) / (xs_l[hi] - x0)) * (x - x0) + y0;
                            double v = inside ? (x0 == x ? y0 : r) : HUGE_VAL;
                            v = (x != x) ? x : v;
                            vq[u] = v;
                        }
#pragma unroll
                        for (int u = 0; u < 2; ++u) acc[q0 + u] = (k == 0) ? vq[u] : acc[q0 + u] + vq[u];
                    }
                } else {
#pragma unroll
                for (int q = 0; q < JMAX; ++q) {
                    const int j = jc + q * 64 + lane;
                    if (jc + q * 64 >= NS) continue;           // uniform
                    const double x = st_l[j < NS ? j : NS - 1];
                    double v = HUGE_VAL;                       // left = right = +inf; fewer than two finite nodes: all +inf
                    if (nfin >= 2 && x >= x_first && x <= x_last) {
                        const int lo = blo_l[j < NS ? j : NS - 1];               // xs[lo] <= x (< xs[lo + 1]); first <= lo <= last here
                        int jl = lo;
                        while (jl >= first && !(cur[jl] - cur[jl] == 0.0)) --jl;
                        int jr = lo + 1;
                        while (jr <= last && !(cur[jr] - cur[jr] == 0.0)) ++jr;
                        if (jl >= first) {
                            if (xs_l[jl] == x) v = cur[jl];
                            else if (jr <= last) v = lerp_np(x, xs_l[jl], xs_l[jr], cur[jl], cur[jr]);
                        }
                    }
                    if (x != x) v = x;
                    acc[q] = (k == 0) ? v : acc[q] + v;
                }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (before the next source / curve overwrites the curve)
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int q = 0; q < JMAX; ++q) {
                const int j = jc + q * 64 + lane;
                if (j >= NS) continue;
                double res = HUGE_VAL;
                if (ns == 1) res = acc[q];
                else if (ns > 1) res = acc[q] / (double)ns;       // utils.average_mags: (a + b [+ c]) / n
                dst[j] = res;
            }
        }
        b = b_next; m = m_next;
    }
}

// Several curves per wave (every output filter with at most ONE source filter -- no averaged band -- and grids small enough that CG >= 2
// curves fit REGRID_PACK_SLOTS passes of 64 lanes): lc_regrid_lds_kernel is bound by its vector instructions, and a curve of 77 output
// nodes fills 60 % of its two passes (a wave64 instruction costs four cycles of a 16-lane SIMD however many lanes are active).  Here
// a wave takes CG CONSECUTIVE curves: their CG x NSs source nodes are loaded in full passes, the CG x NS output nodes are dealt to the
// lanes as one index range -- consecutive curves are consecutive in `out`, so the stores of a group are one contiguous run -- and the
// per-curve finite range (wave ballots cut to the curve's lanes) sits in LDS for the lanes to pick up.  Same arithmetic per node.
constexpr int REGRID_PACK_CG = 4, REGRID_PACK_SLOTS = 5;
struct RegridMeta { double x_first, x_last; int first, last, solid, nfin; };      // 32 bytes
__global__ __launch_bounds__(256) void lc_regrid_packed_kernel(const EmDev* __restrict__ Pp, const double* __restrict__ src, int Ms, int NSs,
                                                               const double* __restrict__ xs, const int* __restrict__ sidx,
                                                               const int* __restrict__ nsrc, const int* __restrict__ blo, long n_curves,
                                                               double* __restrict__ out, const int CG) {
    const EmDev& P = *Pp;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NS = P.NS, M = P.M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* xs_l = reinterpret_cast<double*>(smem);
    double* st_l = xs_l + NSs;
    double* cur = st_l + NS + wave * (REGRID_PACK_CG * NSs);                         // [CG][NSs] of this wave
    RegridMeta* meta = reinterpret_cast<RegridMeta*>(st_l + NS + 4 * REGRID_PACK_CG * NSs) + wave * REGRID_PACK_CG;
    int* blo_l = reinterpret_cast<int*>(reinterpret_cast<RegridMeta*>(st_l + NS + 4 * REGRID_PACK_CG * NSs) + 4 * REGRID_PACK_CG);
    int* plan_l = blo_l + NS;                   // [M][2]: the source filter | number of sources (0 or 1)
    for (int i = threadIdx.x; i < NSs; i += 256) xs_l[i] = xs[i];
    for (int j = threadIdx.x; j < NS; j += 256) { st_l[j] = P.st[j]; blo_l[j] = blo[j]; }
    for (int i = threadIdx.x; i < M; i += 256) { plan_l[2 * i] = sidx[3 * i]; plan_l[2 * i + 1] = nsrc[i]; }
    __syncthreads();
    const long n_groups = (n_curves + CG - 1) / CG, n_waves = (long)gridDim.x * 4;
    const double qnan = HUGE_VAL - HUGE_VAL;
    // this lane's output nodes: slot q covers the group's flat indices 64 q .. 64 q + 63 = (curve cq, node jq)
    int cq_[REGRID_PACK_SLOTS], jq_[REGRID_PACK_SLOTS];
#pragma unroll
    for (int q = 0; q < REGRID_PACK_SLOTS; ++q) {
        const int idx = q * 64 + lane;
        const int c = (idx >= NS ? 1 : 0) + (idx >= 2 * NS ? 1 : 0) + (idx >= 3 * NS ? 1 : 0);
        cq_[q] = c; jq_[q] = idx - c * NS;
    }
    for (long g = (long)blockIdx.x * 4 + wave; g < n_groups; g += n_waves) {
        const long c0 = g * CG;
        const int ncur = (int)(n_curves - c0 < CG ? n_curves - c0 : CG);
        // source curve of every curve of the group (uniform): offset in doubles, -1 without a source
        long base_[REGRID_PACK_CG];
        {
            long b = c0 / M;
            int m = (int)(c0 - b * M);
#pragma unroll
            for (int c = 0; c < REGRID_PACK_CG; ++c) {
                base_[c] = (c < ncur && plan_l[2 * m + 1] > 0) ? ((long)b * Ms + plan_l[2 * m]) * NSs : -1;
                if (++m >= M) { m = 0; ++b; }
            }
        }
        int nfin_[REGRID_PACK_CG], first_[REGRID_PACK_CG], last_[REGRID_PACK_CG];
#pragma unroll
        for (int c = 0; c < REGRID_PACK_CG; ++c) { nfin_[c] = 0; first_[c] = NSs; last_[c] = -1; }
        const int n_src_nodes = ncur * NSs;
        for (int i0 = 0; i0 < n_src_nodes; i0 += 64) {
            const int idx = i0 + lane;
            const int cs = (idx >= NSs ? 1 : 0) + (idx >= 2 * NSs ? 1 : 0) + (idx >= 3 * NSs ? 1 : 0);
            const int i = idx - cs * NSs;
            long base = base_[0];
#pragma unroll
            for (int c = 1; c < REGRID_PACK_CG; ++c) base = cs == c ? base_[c] : base;
            const bool in = idx < n_src_nodes && base >= 0;
            const double v = in ? src[base + i] : qnan;
            if (idx < n_src_nodes) cur[idx] = v;
            const unsigned long long fm = __ballot(in && (v - v == 0.0));
#pragma unroll
            for (int c = 0; c < REGRID_PACK_CG; ++c) {
                // the bits of curve c in this pass: flat indices [c NSs, (c + 1) NSs) cut to [i0, i0 + 64)
                const int lo = c * NSs - i0, hi = lo + NSs;
                if (c < ncur && hi > 0 && lo < 64) {
                    const int l0 = lo < 0 ? 0 : lo, h0 = hi > 64 ? 64 : hi;
                    const unsigned long long span = (h0 - l0 >= 64 ? ~0ull : ((1ull << (h0 - l0)) - 1ull)) << l0;
                    const unsigned long long mc = fm & span;
                    if (mc != 0) {
                        nfin_[c] += __popcll(mc);
                        const int fb = i0 + __ffsll((long long)mc) - 1 - c * NSs, lb = i0 + 63 - __clzll((long long)mc) - c * NSs;
                        if (first_[c] == NSs) first_[c] = fb;
                        last_[c] = lb;
                    }
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < REGRID_PACK_CG; ++c)
                if (c < ncur) {
                    RegridMeta mt;
                    const bool two = nfin_[c] >= 2;
                    mt.first = first_[c]; mt.last = last_[c]; mt.nfin = nfin_[c];
                    mt.solid = (two && nfin_[c] == last_[c] - first_[c] + 1) ? 1 : 0;
                    mt.x_first = two ? xs_l[first_[c]] : 0.0; mt.x_last = two ? xs_l[last_[c]] : 0.0;
                    meta[c] = mt;
                }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (curves and their ranges are read across lanes below; LDS instructions of a wave execute in order)
        __builtin_amdgcn_wave_barrier();
        const int n_out = ncur * NS;
        double* dst = out + (size_t)c0 * NS;
#pragma unroll
        for (int q = 0; q < REGRID_PACK_SLOTS; ++q) {
            if (q * 64 >= n_out) break;                          // uniform
            const int idx = q * 64 + lane;
            const bool valid = idx < n_out;
            const int c = valid ? cq_[q] : 0, j = valid ? jq_[q] : 0;
            const RegridMeta mt = meta[c];
            const double* cc = cur + c * NSs;
            const double x = st_l[j];
            const bool inside = mt.nfin >= 2 && x >= mt.x_first && x <= mt.x_last;
            int lo = blo_l[j];
            lo = lo < mt.first ? mt.first : (lo > mt.last ? mt.last : lo);          // (only lanes outside the window are clamped)
            lo = lo < 0 ? 0 : (lo > NSs - 1 ? NSs - 1 : lo);                         // (a curve without a finite node: first = NSs, last = -1)
            const int hi = lo + 1 > mt.last ? (mt.last < 0 ? 0 : mt.last) : lo + 1;
            const double x0 = xs_l[lo], y0 = cc[lo];
            const double r = ((cc[hi] - y0) / (xs_l[hi] - x0)) * (x - x0) + y0;
            double v = inside ? (x0 == x ? y0 : r) : HUGE_VAL;
            if (inside && !mt.solid) {
                // a hole between the curve's first and last finite node: walk to the finite neighbours (np.interp over the finite nodes)
                const int lo0 = blo_l[j];
                int jl = lo0;
                while (jl >= mt.first && !(cc[jl] - cc[jl] == 0.0)) --jl;
                int jr = lo0 + 1;
                while (jr <= mt.last && !(cc[jr] - cc[jr] == 0.0)) ++jr;
                v = HUGE_VAL;
                if (jl >= mt.first) {
                    if (xs_l[jl] == x) v = cc[jl];
                    else if (jr <= mt.last) v = lerp_np(x, xs_l[jl], xs_l[jr], cc[jl], cc[jr]);
                }
            }
            v = (x != x) ? x : v;
            if (valid) dst[idx] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (before the next group overwrites the curves)
        __builtin_amdgcn_wave_barrier();
    }
}

int32_t nmma_lc_regrid(nmma_em_handle* h, const double* lc_src_dev, int32_t n_src_filters, int32_t n_src_times,
                       const double* src_times_host, const int32_t* src_index_host, const int32_t* n_sources_host,
                       int64_t B, double* out_dev, void* stream) {
    if (!h || !lc_src_dev || !src_times_host || !src_index_host || !n_sources_host || !out_dev || B < 0 ||
        n_src_filters < 1 || n_src_times < 1)
        return fail("nmma_lc_regrid: bad argument");
    if (B == 0) return 0;
    const int M = h->dev.M;
    for (int i = 1; i < n_src_times; ++i)
        if (!(src_times_host[i] > src_times_host[i - 1])) return fail("nmma_lc_regrid: source times must increase");
    for (int m = 0; m < M; ++m) {
        if (n_sources_host[m] < 0 || n_sources_host[m] > NMMA_MAX_SOURCES) return fail("nmma_lc_regrid: bad n_sources");
        for (int k = 0; k < n_sources_host[m]; ++k)
            if (src_index_host[m * 3 + k] < 0 || src_index_host[m * 3 + k] >= n_src_filters)
                return fail("nmma_lc_regrid: source filter out of range");
    }
    NM_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int NS_out = h->dev.NS;
    const size_t off_blo = (size_t)n_src_times * 8 + (size_t)M * 4 * 4;
    const size_t bytes = off_blo + (size_t)NS_out * 4;
    std::vector<unsigned char> stage(bytes);
    std::memcpy(stage.data(), src_times_host, (size_t)n_src_times * 8);
    std::memcpy(stage.data() + (size_t)n_src_times * 8, src_index_host, (size_t)M * 3 * 4);
    std::memcpy(stage.data() + (size_t)n_src_times * 8 + (size_t)M * 3 * 4, n_sources_host, (size_t)M * 4);
    {   // bracket of every output node in the source grid (static): the last source node at or before it
        std::vector<int32_t> blo(NS_out);
        for (int j = 0; j < NS_out; ++j)
            blo[j] = (int32_t)(std::upper_bound(src_times_host, src_times_host + n_src_times, h->st_host[j]) - src_times_host) - 1;
        std::memcpy(stage.data() + off_blo, blo.data(), (size_t)NS_out * 4);
    }
    // The tables live on the handle, one copy per distinct set: a combined model calls with the same few sets for every batch,
    // so after the first batch a call neither allocates, copies nor synchronises.  (Bounded: beyond 16 sets the oldest goes.)
    unsigned char* d = nullptr;
    for (auto& rs : h->regrid_sets)
        if (rs.host == stage) { d = rs.dev; break; }
    if (d == nullptr) {
        if (h->regrid_sets.size() >= 16) {
            NM_HIP(hipStreamSynchronize(s));          // (nothing may still read the buffer that is dropped)
            (void)hipFree(h->regrid_sets.front().dev);
            h->regrid_sets.erase(h->regrid_sets.begin());
        }
        nmma_em_handle::RegridSet rs;
        NM_HIP(hipMalloc(reinterpret_cast<void**>(&rs.dev), bytes));
        const hipError_t ce = hipMemcpy(rs.dev, stage.data(), bytes, hipMemcpyHostToDevice);      // synchronous: first sight of this set only
        if (ce != hipSuccess) { (void)hipFree(rs.dev); return fail(std::string("nmma_lc_regrid: table upload failed: ") + hipGetErrorString(ce)); }
        rs.host = stage;
        d = rs.dev;
        h->regrid_sets.push_back(std::move(rs));
    }
    const long n_curves = (long)B * M;
    bool single_source = true;      // (no averaged band: every output filter copies at most one source filter)
    for (int m = 0; m < M; ++m) if (n_sources_host[m] > 1) single_source = false;
    const int pack_cg = std::min(REGRID_PACK_CG, (REGRID_PACK_SLOTS * 64) / std::max(NS_out, 1));
    const size_t lds_pack = (size_t)(n_src_times + NS_out + 4 * REGRID_PACK_CG * n_src_times) * 8 + (size_t)4 * REGRID_PACK_CG * sizeof(RegridMeta) +
                            (size_t)(NS_out + 2 * M) * 4;
    static const bool no_pack = getenv("NMMA_REGRID_NO_PACK") != nullptr;      // (A/B measurements)
    if (single_source && pack_cg >= 2 && lds_pack <= 64 * 1024 && !no_pack) {
        const size_t lds = lds_pack;
        const long n_groups = (n_curves + pack_cg - 1) / pack_cg;
        const unsigned gx = (unsigned)std::min<long>((n_groups + 3) / 4, 2048);
        hipLaunchKernelGGL(lc_regrid_packed_kernel, dim3(gx), dim3(256), lds, s, h->dev_d, lc_src_dev,
                           n_src_filters, n_src_times, reinterpret_cast<const double*>(d),
                           reinterpret_cast<const int*>(d + (size_t)n_src_times * 8),
                           reinterpret_cast<const int*>(d + (size_t)n_src_times * 8 + (size_t)M * 3 * 4),
                           reinterpret_cast<const int*>(d + off_blo), n_curves, out_dev, pack_cg);
    } else if (n_src_times <= REGRID_LDS_NODES && NS_out <= REGRID_LDS_OUT) {
        // (persistent workgroups: eight per CU of 256 CUs cover the latency; fewer when the batch is small)
        const size_t lds = (size_t)(5 * n_src_times + NS_out) * 8 + (size_t)(NS_out + 4 * M) * 4;
        // (grids of 1536 .. 4096 workgroups: 39.1 .. 37.7 us at config 3's shape; one workgroup per four curves: 47.6)
        const unsigned gx = (unsigned)std::min<long>((n_curves + 3) / 4, 2048);
        hipLaunchKernelGGL(lc_regrid_lds_kernel, dim3(gx), dim3(256), lds, s, h->dev_d, lc_src_dev,
                           n_src_filters, n_src_times, reinterpret_cast<const double*>(d),
                           reinterpret_cast<const int*>(d + (size_t)n_src_times * 8),
                           reinterpret_cast<const int*>(d + (size_t)n_src_times * 8 + (size_t)M * 3 * 4),
                           reinterpret_cast<const int*>(d + off_blo), n_curves, out_dev);
    }
    else
    hipLaunchKernelGGL(lc_regrid_kernel, dim3((unsigned)((n_curves + 3) / 4)), dim3(256), 0, s, h->dev_d, lc_src_dev,
                       n_src_filters, n_src_times, reinterpret_cast<const double*>(d),
                       reinterpret_cast<const int*>(d + (size_t)n_src_times * 8),
                       reinterpret_cast<const int*>(d + (size_t)n_src_times * 8 + (size_t)M * 3 * 4), n_curves, out_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("nmma_lc_regrid launch failed: ") + hipGetErrorString(e));
    return 0;
}

int32_t nmma_em_loglike_host(nmma_em_handle* h, const double* theta_host, int64_t B, int64_t ld, double* out_host) {
    if (check_call(h, theta_host, B, ld, "nmma_em_loglike_host")) return 1;
    if (refuse_stack2_only(h, "nmma_em_loglike_host")) return 1;
    if (B == 0) return 0;
    if (!out_host) return fail("nmma_em_loglike_host: null output");
    NM_HIP(hipSetDevice(h->device));
    // Device and PINNED host staging buffers plus a private stream: the caller's pageable arrays are copied through
    // pinned memory so that both transfers are asynchronous DMA on the launch stream and the call synchronises once.
    // capacities grow in powers of two from 64 KiB (odd small pinned sizes were seen to copy ten times slower)
    auto grow = [](int64_t need) { int64_t c = 8192; while (c < need) c <<= 1; return c; };
    if (B * ld > h->theta_cap) {
        const int64_t cap = grow(B * ld);
        if (h->theta_stage) (void)hipFree(h->theta_stage);
        if (h->theta_pin) (void)hipHostFree(h->theta_pin);
        h->theta_stage = nullptr; h->theta_pin = nullptr; h->theta_cap = 0;
        NM_HIP(hipMalloc(reinterpret_cast<void**>(&h->theta_stage), cap * sizeof(double)));
        NM_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->theta_pin), cap * sizeof(double), hipHostMallocMapped));
        h->theta_cap = cap;
    }
    if (B > h->out_cap) {
        const int64_t cap = grow(B);
        if (h->out_stage) (void)hipFree(h->out_stage);
        if (h->out_pin) (void)hipHostFree(h->out_pin);
        h->out_stage = nullptr; h->out_pin = nullptr; h->out_cap = 0;
        NM_HIP(hipMalloc(reinterpret_cast<void**>(&h->out_stage), cap * sizeof(double)));
        NM_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->out_pin), cap * sizeof(double), hipHostMallocMapped));
        h->out_cap = cap;
    }
    if (!h->host_stream) NM_HIP(hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
    if ((size_t)(B * ld) * sizeof(double) <= (1u << 20)) {
        // up to ~1 MiB of theta: ZERO-COPY -- the kernel reads theta from and writes logL to pinned host memory over
        // PCIe (each row is read once), so the call is one launch and one stream wait, no DMA packets
        void* th_d = nullptr; void* out_d = nullptr;
        NM_HIP(hipHostGetDevicePointer(&th_d, h->theta_pin, 0));
        NM_HIP(hipHostGetDevicePointer(&out_d, h->out_pin, 0));
        std::memcpy(h->theta_pin, theta_host, (size_t)(B * ld) * sizeof(double));
        // Completion: the kernel's logL stores land in pinned memory microseconds before the runtime's end-of-kernel signal
        // has woken a waiting host thread.  The output is pre-filled with a NaN pattern the kernel never produces (bad rows
        // get the finite floor) and the host spins until every row has been replaced; a kernel that takes suspiciously long
        // falls back to the stream wait (which also catches a failed launch).
        constexpr uint64_t PENDING = 0x7ff8badc0ffee000ull;
        volatile uint64_t* const pending = reinterpret_cast<volatile uint64_t*>(h->out_pin);
        const bool poll = h->host_poll != 0 && B <= 4096;
        if (poll) for (int64_t i = 0; i < B; ++i) pending[i] = PENDING;
        if (nmma_em_loglike(h, static_cast<const double*>(th_d), B, ld, static_cast<double*>(out_d), h->host_stream)) return 1;
        bool landed = false;
        if (poll) {
            const auto t0 = std::chrono::steady_clock::now();
            int64_t i = 0;
            for (unsigned spins = 1;; ++spins) {
                while (i < B && pending[i] != PENDING) ++i;
                if (i == B) { landed = true; break; }
                if ((spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
                __builtin_ia32_pause();
            }
        }
        if (!landed) NM_HIP(hipStreamSynchronize(h->host_stream));
        std::memcpy(out_host, h->out_pin, (size_t)B * sizeof(double));
    } else {
        NM_HIP(hipMemcpy(h->theta_stage, theta_host, B * ld * sizeof(double), hipMemcpyHostToDevice));
        if (nmma_em_loglike(h, h->theta_stage, B, ld, h->out_stage, nullptr)) return 1;
        NM_HIP(hipMemcpy(out_host, h->out_stage, B * sizeof(double), hipMemcpyDeviceToHost));
    }
    return watchdog_tripped(h, "nmma_em_loglike_host");
}

int32_t nmma_em_lightcurves(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* obs_times_dev,
                            double* mag_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_lightcurves")) return 1;
    if (refuse_stack2_only(h, "nmma_em_lightcurves")) return 1;
    if (B == 0) return 0;
    if (!obs_times_dev || !mag_dev) return fail("nmma_em_lightcurves: null output");
    NM_HIP(hipSetDevice(h->device));
    if (h->dev.model_kind != NMMA_MODEL_SVD) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (ensure_lc_ws(h, B)) return 1;
        if (launch_model_lc(h, theta_dev, B, ld, h->lc_ws, s)) return 1;
        hipLaunchKernelGGL(lc_to_detector, dim3((unsigned)B), dim3(64), 0, s, h->dev_d, theta_dev, (long)B, (long)ld,
                           h->lc_ws, obs_times_dev, mag_dev);
        NM_HIP(hipGetLastError());
        return 0;
    }
    NM_HIP(launch_aux(h, theta_dev, B, ld, MODE_LC, nullptr, obs_times_dev, mag_dev, static_cast<hipStream_t>(stream)));
    return 0;
}

int32_t nmma_em_loglike_lc_parts(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, const double* lc_dev,
                                 double* chi_dev, double* gp_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_loglike_lc_parts")) return 1;
    if (B == 0 || h->dev.O == 0) return 0;
    if (!lc_dev || !chi_dev || !gp_dev) return fail("nmma_em_loglike_lc_parts: null buffer");
    NM_HIP(hipSetDevice(h->device));
    if (ensure_scratch(h, B)) return 1;    // the total logL is produced anyway; discard it
    return launch_lc_loglike(h, theta_dev, B, ld, lc_dev, h->chi, chi_dev, gp_dev, static_cast<hipStream_t>(stream));
}

int32_t nmma_em_lightcurves_lc(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, const double* lc_dev,
                               double* obs_times_dev, double* mag_dev, void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_lightcurves_lc")) return 1;
    if (B == 0) return 0;
    if (!lc_dev || !obs_times_dev || !mag_dev) return fail("nmma_em_lightcurves_lc: null buffer");
    if (h->dev.model_kind == NMMA_MODEL_SVD) return fail("nmma_em_lightcurves_lc: an SVD handle evaluates its own curves (nmma_em_lightcurves)");
    NM_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(lc_to_detector, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), h->dev_d, theta_dev, (long)B, (long)ld,
                       lc_dev, obs_times_dev, mag_dev);
    NM_HIP(hipGetLastError());
    return 0;
}

int32_t nmma_em_coefficients(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, float* coeff_dev,
                             void* stream) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_coefficients")) return 1;
    if (B == 0) return 0;
    if (!coeff_dev) return fail("nmma_em_coefficients: null output");
    if (h->dev.model_kind != NMMA_MODEL_SVD) return fail("nmma_em_coefficients: not an SVD model");
    NM_HIP(hipSetDevice(h->device));
    NM_HIP(launch_aux(h, theta_dev, B, ld, MODE_COEFF, coeff_dev, nullptr, nullptr, static_cast<hipStream_t>(stream)));
    return 0;
}

int32_t nmma_em_check(nmma_em_handle* h) {
    if (!h) return fail("nmma_em_check: null handle");
    NM_HIP(hipSetDevice(h->device));
    NM_HIP(hipDeviceSynchronize());
    return watchdog_tripped(h, "nmma_em_check");
}

int32_t nmma_em_debug_timeline(nmma_em_handle* h, const double* theta_dev, int64_t B, int64_t ld, double* out_dev,
                                int64_t* stamps_host) {
    if (check_call(h, theta_dev, B, ld, "nmma_em_debug_timeline")) return 1;
    if (refuse_stack2_only(h, "nmma_em_debug_timeline")) return 1;
    if (!out_dev || !stamps_host || B == 0) return fail("nmma_em_debug_timeline: bad argument");
    NM_HIP(hipSetDevice(h->device));
    long long* d = nullptr;
    NM_HIP(hipMalloc(reinterpret_cast<void**>(&d), 512 * sizeof(long long)));
    NM_HIP(hipMemset(d, 0, 512 * sizeof(long long)));
    h->dbg = d;
    const int rc = nmma_em_loglike(h, theta_dev, B, ld, out_dev, nullptr);
    h->dbg = nullptr;
    if (rc == 0) {
        hipError_t e = hipMemcpy(stamps_host, d, 512 * sizeof(long long), hipMemcpyDeviceToHost);
        (void)hipFree(d);
        if (e != hipSuccess) return fail(std::string("hipMemcpy failed: ") + hipGetErrorString(e));
        return 0;
    }
    (void)hipFree(d);
    return 1;
}

int32_t nmma_em_n_sample_times(const nmma_em_handle* h) { return h ? h->dev.NS : -1; }
int32_t nmma_em_device(const nmma_em_handle* h) { return h ? h->device : -1; }

int64_t nmma_em_flops_per_eval(const nmma_em_handle* h) { return h ? h->flops_per_eval : -1; }

int32_t nmma_em_last_launch_geometry(const nmma_em_handle* h, int32_t* gx, int32_t* gy, int32_t* block,
                                     int32_t* tile, int32_t* lds) {
    if (!h) return fail("nmma_em_last_launch_geometry: null handle");
    if (gx) *gx = h->g_x;
    if (gy) *gy = h->g_y;
    if (block) *block = h->g_block;
    if (tile) *tile = h->g_tile;
    if (lds) *lds = h->g_lds;
    return 0;
}

int32_t nmma_em_profile_begin(nmma_em_handle* h, int32_t max_launches) {
    if (!h || max_launches < 1) return fail("nmma_em_profile_begin: bad argument");
    NM_HIP(hipSetDevice(h->device));
    while ((int)h->ev.size() < 2 * max_launches) {
        hipEvent_t e;
        NM_HIP(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    h->prof_cap = max_launches;
    h->prof_n = 0;
    h->prof_calls = 0;
    if (const char* e = getenv("NMMA_PROFILE_STRIDE")) h->prof_stride = std::max(1, atoi(e));
    h->prof_group = 1;
    if (const char* e = getenv("NMMA_PROFILE_GROUP")) h->prof_group = std::max(1, atoi(e));
    h->prof_on = true;
    return 0;
}

int32_t nmma_em_profile_end(nmma_em_handle* h, double* fused_ms_total, double* combine_ms_total, int32_t* n_launches) {
    if (!h) return fail("nmma_em_profile_end: null handle");
    NM_HIP(hipSetDevice(h->device));
    h->prof_on = false;
    double f = 0.0, cmb = 0.0;   // the filter sum is fused into em_logl: no separate combine kernel
    for (int i = 0; i < h->prof_n; ++i) {
        NM_HIP(hipEventSynchronize(h->ev[2 * i + 1]));
        float ms = 0.f;
        NM_HIP(hipEventElapsedTime(&ms, h->ev[2 * i + 0], h->ev[2 * i + 1]));
        f += ms;
    }
    if (fused_ms_total) *fused_ms_total = f;
    if (combine_ms_total) *combine_ms_total = cmb;
    if (n_launches) *n_launches = h->prof_n * h->prof_group;
    return 0;
}

}  // extern "C"


