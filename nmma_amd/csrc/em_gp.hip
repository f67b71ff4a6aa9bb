// em_gp.hip -- the Gaussian-process surrogate of the SVD light-curve model (interpolation_type "sklearn_gp"): kernel, handle and
// entry points (nmma_gp_*).  Reference: nmma/em/lightcurve_generation.py:180-217 (eval_svd_model, n_coeff calls of gp.predict per
// filter) with sklearn's ConstantKernel * RationalQuadratic (nmma/em/training.py:429-453).
//
// The arithmetic, fp64 without contraction (this unit is built with -ffp-contract=off), in the reference's order:
//     x    = (theta_model - param_mins) / (param_maxs - param_mins)
//     d2_n = sum_p (x_p - X[n][p])^2                     sequential in p (scipy cdist "sqeuclidean")
//     base = 1 + d2_n / den_i,  den_i = (2 alpha_i) l_i^2  formed on the host as sklearn's `2 * alpha * length_scale**2`
//     k_n  = constant_i * base ** (-alpha_i)             ocml pow: its logarithm is carried in extended precision, which the bound
//                                                        alpha = 1e10 needs; exp(-alpha log1p(z)) does NOT reproduce the reference,
//                                                        whose rounding of 1 + z dominates the value there
//     c_i  = y_std_i * (sum_n k_n a_in) + y_mean_i
// then the reference's reconstruction  mag_t = (VA[t, :NC] . c) (maxs_t - mins_t) + mins_t  and np.interp onto sample_times, +inf
// outside tt (calc_svd_lc, extrapolate = inf).
//
// Work split (gp_surrogate<NC>): one 256-thread workgroup per (tile of 16 samples, filter).
//   lane = 4 sample + sub: the sample's four sub-lanes are a DPP quad; the sixteen slots (wave, sub) interleave the training set --
//   slot q takes the points n = q, q + 16, q + 32, ...  -- whatever the batch size and the chunking, so a row's bits depend on
//   nothing but its own theta.
//   X [N][NP] and alpha_ [NC][N] pass through LDS in chunks of GP_CHUNK points (alpha_ transposed to [point][NC]: a lane reads the
//   NC weights of its point from consecutive words; the four distinct points of a wave are broadcast reads).
//   d2 is formed once per (sample, training point) and serves all NC coefficients; a lane carries NC fp64 accumulators in registers
//   (NC is a template parameter: no dynamically indexed arrays, no scratch).  Per (sample, point, coefficient): one IEEE division, one
//   power, two multiplies, one add -- the power is ~95 % of the instruction stream.
//   Reduction in a FIXED order: (s0 + s1) + (s2 + s3) over the quad by DPP, then (w0 + w1) + (w2 + w3) over the waves through LDS.
//   With the 16 x NC coefficients of the tile in LDS (zero-padded to 16) the same workgroup reconstructs the curves: VA[NT][NC] . c for
//   16 samples on v_mfma_f64_16x16x4_f64, one 16-node tile per wave and step, K = NC in steps of 4; then span / mins and the stage-1
//   lerp (bracket by bisection over tt staged in LDS: no per-handle tables, the grids of any nmma_em_handle serve).
#include "em_host.h"

namespace nmma {

constexpr int GP_CHUNK = 128;       // training points per LDS chunk (a multiple of the 16 slots)
constexpr int GP_TILE = 16;         // samples per workgroup

struct GpDev {
    int32_t M, NP, NC, NT;
    const int32_t* n_train;     // [M]
    const int64_t* x_off;       // [M] first point of filter m in the concatenated training sets
    const double* X;            // filter m at x_off[m] * NP: [N_m][NP]
    const double* alpha;        // filter m at x_off[m] * NC: [NC][N_m]
    const double* hyp;          // [M][NC][4]  {den = 2 alpha l^2, -alpha, constant, 0}
    const double* yaff;         // [M][NC][2]  {y_std, y_mean}
    const double* VA;           // [M][NT][NC]
    const double* mins;         // [M][NT]
    const double* span;         // [M][NT]  maxs - mins
    const double* tt;           // [M][NT]
    const double* pmin;         // [M][NP]
    const double* pspan;        // [M][NP]  param_maxs - param_mins
};

// LDS layout (doubles): [xs 16 x 8 | red 4 x 16 x NC | coef 16 x 16 | tts NT | work], work = max(chunk: X CH x NP + alpha CH x NC, curves: 16 x NT)
__host__ __device__ inline int gp_lds_fixed(int NC, int NT) { return GP_TILE * 8 + 4 * GP_TILE * NC + GP_TILE * 16 + NT; }
__host__ __device__ inline int gp_lds_work(int NP, int NC, int NT) {
    const int chunk = GP_CHUNK * (NP + NC), curves = GP_TILE * NT;
    return chunk > curves ? chunk : curves;
}

// v + (v of the lane whose index differs in bit 0 / bit 1 of the quad): both partners form the same sum (addition commutes)
template <int CTRL>
__device__ __forceinline__ double quad_add(const double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int plo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    const int phi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return v + __hiloint2double(phi, plo);
}

template <int NC>
__global__ __launch_bounds__(256) void gp_surrogate(const GpDev G, const EmDev* __restrict__ em, const double* __restrict__ theta,
                                                    const long B, const long ld, double* __restrict__ coeff_out,
                                                    double* __restrict__ lc_out) {
    extern __shared__ double gp_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.y;
    const long tile0 = (long)blockIdx.x * GP_TILE;
    const int NP = G.NP, NT = G.NT, M = G.M;
    const int N = G.n_train[m];
    const double* __restrict__ Xg = G.X + (size_t)G.x_off[m] * NP;
    const double* __restrict__ Ag = G.alpha + (size_t)G.x_off[m] * NC;
    const double* __restrict__ hyp = G.hyp + (size_t)m * NC * 4;

    double* xs = gp_smem;                           // [16][8] normalised inputs
    double* red = xs + GP_TILE * 8;                 // [4][16][NC] wave partial sums
    double* coef = red + 4 * GP_TILE * NC;          // [16][16] the tile's coefficients, zero beyond NC
    double* tts = coef + GP_TILE * 16;              // [NT]
    double* work = tts + NT;
    double* Xc = work;                              // [GP_CHUNK][NP]
    double* Ac = work + GP_CHUNK * NP;              // [GP_CHUNK][NC]

    if (tid < GP_TILE * 8) {
        const int s = tid >> 3, p = tid & 7;
        const long b = tile0 + s;
        double v = 0.0;
        // (rows beyond the batch evaluate x = 0: finite work, nothing stored)
        if (b < B && p < NP) v = (apply_slot(em->model_param[p], theta + b * ld) - G.pmin[m * NP + p]) / G.pspan[m * NP + p];
        xs[tid] = v;
    }
    __syncthreads();

    const int sub = lane & 3, s = lane >> 2, slot = wave * 4 + sub;
    double x[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) x[p] = xs[s * 8 + p];
    double acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0;

    for (int n0 = 0; n0 < N; n0 += GP_CHUNK) {
        const int cn = (N - n0 < GP_CHUNK) ? N - n0 : GP_CHUNK;
        if (n0 > 0) __syncthreads();          // the previous chunk has been consumed
        for (int idx = tid; idx < cn * NP; idx += 256) Xc[idx] = Xg[(size_t)n0 * NP + idx];
        for (int idx = tid; idx < cn * NC; idx += 256) {
            const int i = idx / cn, j = idx - i * cn;
            Ac[j * NC + i] = Ag[(size_t)i * N + n0 + j];
        }
        __syncthreads();
        for (int j = slot; j < cn; j += 16) {
            const double* xr = Xc + j * NP;
            double d2 = 0.0;
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if (p < NP) { const double d = x[p] - xr[p]; d2 += d * d; }
            const double* ar = Ac + j * NC;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const double base = 1.0 + d2 / hyp[i * 4 + 0];
                const double k = hyp[i * 4 + 2] * pow(base, hyp[i * 4 + 1]);
                acc[i] += k * ar[i];
            }
        }
    }

    // ---- fixed-order reduction: the quad, then the four waves
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        double v = quad_add<0xB1>(acc[i]);     // quad_perm [1, 0, 3, 2]
        v = quad_add<0x4E>(v);                 // quad_perm [2, 3, 0, 1]
        if (sub == 0) red[(wave * GP_TILE + s) * NC + i] = v;
    }
    __syncthreads();
    {
        const int sr = tid >> 4, i = tid & 15;       // 256 threads = 16 samples x 16 (padded) coefficients
        double c = 0.0;
        if (i < NC) {
            const double r = (red[(0 * GP_TILE + sr) * NC + i] + red[(1 * GP_TILE + sr) * NC + i]) +
                             (red[(2 * GP_TILE + sr) * NC + i] + red[(3 * GP_TILE + sr) * NC + i]);
            c = G.yaff[((size_t)m * NC + i) * 2] * r + G.yaff[((size_t)m * NC + i) * 2 + 1];
            const long b = tile0 + sr;
            if (coeff_out != nullptr && b < B) coeff_out[((size_t)b * M + m) * NC + i] = c;
        }
        coef[sr * 16 + i] = c;
    }
    if (lc_out == nullptr) return;
    for (int t = tid; t < NT; t += 256) tts[t] = G.tt[(size_t)m * NT + t];
    __syncthreads();

    // ---- reconstruction on the fp64 matrix cores: 16 nodes x 16 samples per v_mfma_f64_16x16x4_f64.  A lane holds
    // A[node lane % 16][k = lane / 16], B[k = lane / 16][sample lane % 16], D[node 4 r + lane / 16][sample lane % 16]
    typedef double f64x4_t __attribute__((ext_vector_type(4)));
    double* magb = work;                            // [16][NT]
    const double* __restrict__ VA = G.VA + (size_t)m * NT * NC;
    const int n_tt = (NT + 15) / 16;
    for (int tile = wave; tile < n_tt; tile += 4) {
        const int t_a = tile * 16 + (lane & 15);
        f64x4_t d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < (NC + 3) / 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);
            const double a = (t_a < NT && k < NC) ? VA[(size_t)t_a * NC + k] : 0.0;
            const double bq = coef[(lane & 15) * 16 + k];
            d = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq, d, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = tile * 16 + 4 * r + (lane >> 4);
            if (t < NT) magb[(lane & 15) * NT + t] = d[r] * G.span[(size_t)m * NT + t] + G.mins[(size_t)m * NT + t];
        }
    }
    __syncthreads();

    // ---- stage 1: np.interp(sample_times, tt, mag, left = right = inf)
    const int NS = em->NS;
    const double* __restrict__ st = em->st;
    const double t_lo = tts[0], t_hi = tts[NT - 1];
    for (int idx = tid; idx < GP_TILE * NS; idx += 256) {
        const int sl = idx / NS, j = idx - sl * NS;
        const long b = tile0 + sl;
        if (b >= B) break;
        const double xq = st[j];
        double v = dinf();
        if (xq >= t_lo && xq <= t_hi) {
            int lo = 0, hi = NT - 1;                // tts[lo] <= xq, and xq < tts[hi] unless xq is the last node
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tts[mid] <= xq) lo = mid; else hi = mid;
            }
            const double* row = magb + sl * NT;
            if (xq >= t_hi) v = row[NT - 1];
            else {
                const double y0 = row[lo];
                const double slope = (row[lo + 1] - y0) / (tts[lo + 1] - tts[lo]);
                v = slope * (xq - tts[lo]) + y0;
            }
        }
        lc_out[((size_t)b * M + m) * NS + j] = v;
    }
}

template <int NC>
static hipError_t gp_launch_nc(const GpDev& G, const EmDev* em_d, const double* theta, int64_t B, int64_t ld, double* coeff, double* lc,
                               int lds, hipStream_t s) {
    hipLaunchKernelGGL(gp_surrogate<NC>, dim3((unsigned)((B + GP_TILE - 1) / GP_TILE), (unsigned)G.M), dim3(256), lds, s, G, em_d, theta,
                       (long)B, (long)ld, coeff, lc);
    return hipGetLastError();
}

}  // namespace nmma

struct nmma_gp_handle {
    nmma::GpDev dev{};
    int device = 0;
    int lds_bytes = 0;
    std::vector<void*> owned;
};

using namespace nmma;

namespace {

template <typename T>
hipError_t gp_upload(const std::vector<T>& v, const T** dst, std::vector<void*>& owned) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (!v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    *dst = reinterpret_cast<const T*>(p);
    return e;
}

int gp_call(nmma_gp_handle* gp, nmma_em_handle* em, const double* theta, int64_t B, int64_t ld, double* coeff, double* lc, void* stream,
            const char* who) {
    if (!gp || !em) return fail(std::string(who) + ": null handle");
    if (B < 0) return fail(std::string(who) + ": negative batch");
    if (B == 0) return 0;
    if (!theta || (!coeff && !lc)) return fail(std::string(who) + ": null buffer");
    if (ld < em->dev.D) return fail(std::string(who) + ": leading dimension smaller than n_dim");
    if (em->device != gp->device) return fail(std::string(who) + ": the two handles live on different devices");
    if (em->dev.NP != gp->dev.NP) return fail(std::string(who) + ": the em handle's n_params differs from the surrogate's");
    if (lc && em->dev.M != gp->dev.M) return fail(std::string(who) + ": the em handle's n_model_filters differs from the surrogate's");
    if ((B + GP_TILE - 1) / GP_TILE > 0x7fffffffLL) return fail(std::string(who) + ": batch too large");
    NM_HIP(hipSetDevice(gp->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const GpDev& G = gp->dev;
    hipError_t e = hipErrorInvalidValue;
    switch (G.NC) {
#define NM_GP_CASE(n) case n: e = gp_launch_nc<n>(G, em->dev_d, theta, B, ld, coeff, lc, gp->lds_bytes, s); break;
        NM_GP_CASE(1) NM_GP_CASE(2) NM_GP_CASE(3) NM_GP_CASE(4) NM_GP_CASE(5) NM_GP_CASE(6) NM_GP_CASE(7) NM_GP_CASE(8)
        NM_GP_CASE(9) NM_GP_CASE(10) NM_GP_CASE(11) NM_GP_CASE(12) NM_GP_CASE(13) NM_GP_CASE(14) NM_GP_CASE(15) NM_GP_CASE(16)
#undef NM_GP_CASE
    }
    NM_HIP(e);
    return 0;
}

}  // namespace

extern "C" {

void nmma_gp_destroy(nmma_gp_handle* gp) {
    if (!gp) return;
    (void)hipSetDevice(gp->device);
    for (void* p : gp->owned) (void)hipFree(p);
    delete gp;
}

int32_t nmma_gp_create(const nmma_gp_config* c, nmma_gp_handle** out) {
    if (!c || !out) return fail("nmma_gp_create: null argument");
    *out = nullptr;
    if (c->abi_version != NMMA_ABI_VERSION) return fail("nmma_gp_create: ABI version mismatch");
    const int M = c->n_model_filters, NP = c->n_params, NC = c->n_coeff, NT = c->n_tt;
    if (M < 1 || NP < 1 || NP > NMMA_MAX_PARAMS || NC < 1 || NC > NMMA_MAX_COEFF || NT < 2) return fail("nmma_gp_create: bad surrogate dimensions");
    if (!c->n_train || !c->X || !c->alpha || !c->constant || !c->length_scale || !c->rq_alpha || !c->y_mean || !c->y_std || !c->VA ||
        !c->mins || !c->maxs || !c->tt || !c->param_mins || !c->param_maxs)
        return fail("nmma_gp_create: null surrogate tensor");
    std::vector<int64_t> x_off(M);
    int64_t total = 0;
    for (int m = 0; m < M; ++m) {
        if (c->n_train[m] < 1) return fail("nmma_gp_create: a filter without training points");
        x_off[m] = total;
        total += c->n_train[m];
    }
    for (int m = 0; m < M; ++m) {
        for (int t = 1; t < NT; ++t)
            if (!(c->tt[(size_t)m * NT + t] > c->tt[(size_t)m * NT + t - 1])) return fail("nmma_gp_create: tt must increase");
        for (int p = 0; p < NP; ++p)
            if (!(c->param_maxs[m * NP + p] - c->param_mins[m * NP + p] != 0.0)) return fail("nmma_gp_create: empty parameter range");
    }
    std::vector<double> hyp((size_t)M * NC * 4, 0.0), yaff((size_t)M * NC * 2);
    for (int q = 0; q < M * NC; ++q) {
        const double l = c->length_scale[q], a = c->rq_alpha[q];
        if (!(l > 0.0) || !(a > 0.0) || !std::isfinite(l) || !std::isfinite(a) || !std::isfinite(c->constant[q]))
            return fail("nmma_gp_create: kernel hyperparameters must be positive and finite");
        hyp[(size_t)q * 4 + 0] = (2.0 * a) * (l * l);       // sklearn: dists / (2 * self.alpha * self.length_scale**2)
        hyp[(size_t)q * 4 + 1] = -a;
        hyp[(size_t)q * 4 + 2] = c->constant[q];
        yaff[(size_t)q * 2 + 0] = c->y_std[q];
        yaff[(size_t)q * 2 + 1] = c->y_mean[q];
    }
    const int lds = (gp_lds_fixed(NC, NT) + gp_lds_work(NP, NC, NT)) * (int)sizeof(double);
    if (lds > 64 * 1024) return fail("nmma_gp_create: the time grid does not fit the workgroup's LDS (n_tt too large)");

    int ndev = 0;
    NM_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail("nmma_gp_create: no HIP device (this library has no CPU fallback)");
    if (c->device < 0 || c->device >= ndev) return fail("nmma_gp_create: bad device ordinal");
    NM_HIP(hipSetDevice(c->device));

    auto* gp = new nmma_gp_handle();
    gp->device = c->device;
    gp->lds_bytes = lds;
    GpDev& G = gp->dev;
    G.M = M; G.NP = NP; G.NC = NC; G.NT = NT;
    std::vector<double> span((size_t)M * NT), pspan((size_t)M * NP);
    for (size_t i = 0; i < span.size(); ++i) span[i] = c->maxs[i] - c->mins[i];
    for (size_t i = 0; i < pspan.size(); ++i) pspan[i] = c->param_maxs[i] - c->param_mins[i];
#define NM_GP_UP(vec, field)                                                                              \
    do {                                                                                                  \
        const hipError_t _e = gp_upload(vec, &G.field, gp->owned);                                        \
        if (_e != hipSuccess) {                                                                           \
            nmma_gp_destroy(gp);                                                                          \
            return fail(std::string("nmma_gp_create: upload " #field " failed: ") + hipGetErrorString(_e)); \
        }                                                                                                 \
    } while (0)
    NM_GP_UP(std::vector<int32_t>(c->n_train, c->n_train + M), n_train);
    NM_GP_UP(x_off, x_off);
    NM_GP_UP(std::vector<double>(c->X, c->X + (size_t)total * NP), X);
    NM_GP_UP(std::vector<double>(c->alpha, c->alpha + (size_t)total * NC), alpha);
    NM_GP_UP(hyp, hyp);
    NM_GP_UP(yaff, yaff);
    NM_GP_UP(std::vector<double>(c->VA, c->VA + (size_t)M * NT * NC), VA);
    NM_GP_UP(std::vector<double>(c->mins, c->mins + (size_t)M * NT), mins);
    NM_GP_UP(span, span);
    NM_GP_UP(std::vector<double>(c->tt, c->tt + (size_t)M * NT), tt);
    NM_GP_UP(std::vector<double>(c->param_mins, c->param_mins + (size_t)M * NP), pmin);
    NM_GP_UP(pspan, pspan);
#undef NM_GP_UP
    *out = gp;
    return 0;
}

int32_t nmma_gp_coefficients(nmma_gp_handle* gp, nmma_em_handle* em, const double* theta_dev, int64_t B, int64_t ld, double* coeff_dev,
                             void* stream) {
    return gp_call(gp, em, theta_dev, B, ld, coeff_dev, nullptr, stream, "nmma_gp_coefficients");
}

int32_t nmma_gp_model_lightcurves(nmma_gp_handle* gp, nmma_em_handle* em, const double* theta_dev, int64_t B, int64_t ld, double* lc_dev,
                                  void* stream) {
    return gp_call(gp, em, theta_dev, B, ld, nullptr, lc_dev, stream, "nmma_gp_model_lightcurves");
}

}  // extern "C"
