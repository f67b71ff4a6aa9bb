// em_mlp.hip -- surrogates of the SVD light-curve model whose network has several hidden layers: kernel, handle and entry points
// (nmma_mlp_*).  Reference: nmma/em/lightcurve_generation.py:180-217 (eval_svd_model calls svd_model["model"](x) on whatever Keras
// model the file holds); the reference's training tutorial builds 6 -> 64 -> 128 -> 64 -> 10.
//
// The arithmetic:
//     x    = (theta_model - param_mins) / (param_maxs - param_mins)      fp64, rounded once to fp32 (what Keras does with a float64 array)
//     h_l  = relu(W_l^T h_{l-1} + b_l),  l = 1 .. L;   c = W_out^T h_L + b_out      fp32 on v_mfma_f32_16x16x4_f32 (exact fp32 FMAs)
// then the reference's reconstruction  mag_t = (VA[t, :NC] . c) (maxs_t - mins_t) + mins_t  in fp64 and np.interp onto sample_times, +inf
// outside tt (calc_svd_lc, extrapolate = inf) -- gp_surrogate's second half, restated here.
//
// Work split (mlp_surrogate): a 512-thread workgroup serves one filter and is persistent over pairs of 16-sample tiles (pair
// blockIdx.x, blockIdx.x + gridDim.x, ...): waves 0-3 take the pair's first tile, waves 4-7 its second, and both halves read the same
// weights -- two waves per SIMD, so one half's LDS reads hide behind the other's MFMAs.  The filter's weights -- all layers -- are staged into LDS ONCE per workgroup; a filter whose
// weights exceed the LDS left beside the activations reads the same blocks from L2 instead (same order, same arithmetic).
//   Transposed form, H_l^T[H_l x 16 samples] = W_l^T . H_{l-1}^T + b_l: an MFMA forms 16 outputs x 16 samples from 4 inputs.  Its
//   accumulator holds, in lane l and register r, output 4 (l / 16) + r of sample l % 16; its B operand wants input k = l / 16 of sample
//   l % 16.  So register r of an accumulator IS the B operand of one k-step of the next layer -- the step that covers the units
//   {16 t + 4 g + r : g = 0 .. 3} of output tile t.  That permutation of k is absorbed into the order the next layer's weights are stored
//   in (mlp_swizzle, at create); activations are never transposed.
//   Activation panel in LDS: [unit tile t][lane][4] fp32 -- a wave writes the accumulator of an output tile with one ds_write_b128
//   per lane, and every wave reads the four k-steps of a 16-unit block back with one ds_read_b128 per lane (no bank conflicts).
//   Weight block (output tile u, unit tile t) in the same shape: [lane][4], lane l register r = W[unit 16 t + 4 (l / 16) + r][output 16 u + l % 16].
//   The four waves of a half split a layer's output tiles (u = wave, wave + 4, ...); the panels ping-pong; one barrier per layer.
//   Summation order of one output: four chains, chain r over the units 16 t + 4 g + r (t ascending; g inside the instruction), chain 0
//   starting from the bias; then (s0 + s1) + (s2 + s3).  It depends on the layer's shape alone: a row's bits are the same whatever
//   the batch, the row's place in it and the grid.
//   With the tile's 16 x NC coefficients in LDS (fp64, zero beyond NC: padded outputs have zero weights and bias) the same workgroup
//   reconstructs the curves: VA[NT][NC] . c on v_mfma_f64_16x16x4_f64, span / mins, and the lerp onto the em handle's sample_times.
// Widths need not be multiples of 16: weights and biases are zero-padded at create, which is exact (relu(0) = 0 feeds zero weights).
#include "em_host.h"

namespace nmma {

constexpr int MLP_TILE = 16;            // samples per tile
constexpr int MLP_MAX_DENSE = 7;        // 6 hidden layers + the output layer
constexpr int MLP_MAX_WIDTH = 256;      // hidden width: the four activation panels (two per tile of the pair) of that width take 64 KiB of LDS

struct MlpFilter {
    int32_t nl;                     // Dense layers, the output layer included
    int32_t resident;               // the weights fit LDS beside the panels
    int32_t kb[MLP_MAX_DENSE];      // padded input width / 16
    int32_t ub[MLP_MAX_DENSE];      // padded output width / 16
    int32_t woff[MLP_MAX_DENSE];    // first float of the layer's blocks [u][t][64 lanes][4] within the filter's weights
    int32_t boff[MLP_MAX_DENSE];    // first float of the layer's padded bias within the filter's biases
    int32_t wtotal, btotal;         // floats
    int64_t wbase, bbase;           // the filter's first float in MlpDev::W / MlpDev::bias
};

struct MlpDev {
    int32_t M, NP, NC, NT;
    int32_t act_floats;             // one activation panel: 16 samples x the widest padded layer of any filter
    int32_t bias_floats;            // LDS words for the biases (the largest filter)
    const MlpFilter* filt;          // [M]
    const float* W;                 // swizzled weights, filters one after the other
    const float* bias;              // padded biases
    const double* VA;               // [M][NT][NC]
    const double* mins;             // [M][NT]
    const double* span;             // [M][NT]  maxs - mins
    const double* tt;               // [M][NT]
    const double* pmin;             // [M][NP]
    const double* pspan;            // [M][NP]  param_maxs - param_mins
};

// LDS layout: [coef 2 x 16 x 16 f64 | tts NT (padded to even) | mag 2 x 16 x NT (even) | panels 2 x 2 | biases | resident weights]
__host__ __device__ inline int mlp_nt_even(int NT) { return (NT + 1) & ~1; }
__host__ __device__ inline int mlp_lds_fixed_bytes(int NT, int act_floats, int bias_floats) {
    return (2 * MLP_TILE * 16 + mlp_nt_even(NT) + 2 * MLP_TILE * mlp_nt_even(NT)) * (int)sizeof(double) + (4 * act_floats + bias_floats) * (int)sizeof(float);
}

// One output tile: 16 outputs x 16 samples over kb blocks of 16 inputs.  wblk: this output tile's weight blocks (LDS or global),
// act: the input panel.  Four independent accumulator chains (one per register of the input blocks), added in a fixed order.
template <typename WP>
__device__ __forceinline__ f32x4 mlp_out_tile(const WP wblk, const f32x4* __restrict__ act, const f32x4 bias, const int kb, const int lane) {
    f32x4 a0 = bias, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
    f32x4 w = wblk[lane], h = act[lane];
    for (int t = 0; t < kb; ++t) {
        const int tn = t + 1 < kb ? t + 1 : t;      // the next block's operands travel while this one's MFMAs run (the last step re-reads its own)
        const f32x4 wn = wblk[tn * 64 + lane], hn = act[tn * 64 + lane];
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[0], h[0], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[1], h[1], a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[2], h[2], a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[3], h[3], a3, 0, 0, 0);
        w = wn; h = hn;
    }
    return (a0 + a1) + (a2 + a3);
}

__global__ __launch_bounds__(512) void mlp_surrogate(const MlpDev G, const EmDev* __restrict__ em, const double* __restrict__ theta,
                                                     const long B, const long ld, double* __restrict__ coeff_out,
                                                     double* __restrict__ lc_out) {
    extern __shared__ __attribute__((aligned(16))) double mlp_smem[];
    const int half = threadIdx.x >> 8, tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;     // tid, wave: within the half
    const int m = blockIdx.y;
    const int NP = G.NP, NC = G.NC, NT = G.NT, M = G.M, NTE = mlp_nt_even(NT);
    const MlpFilter* __restrict__ F = G.filt + m;
    const int nl = F->nl;
    const bool resident = F->resident != 0;

    double* coef = mlp_smem + half * MLP_TILE * 16;     // [16][16] the tile's coefficients, zero beyond NC
    double* tts = mlp_smem + 2 * MLP_TILE * 16;         // [NT]
    double* magb = tts + NTE + half * MLP_TILE * NTE;   // [16][NT]
    float* panels = reinterpret_cast<float*>(tts + NTE + 2 * MLP_TILE * NTE);
    float* panel0 = panels + 2 * half * G.act_floats;
    float* panel1 = panel0 + G.act_floats;
    float* bias_s = panels + 4 * G.act_floats;
    f32x4* w_s = reinterpret_cast<f32x4*>(bias_s + G.bias_floats);
    const gcf32x4p w_g = (gcf32x4p)(uintptr_t)(G.W + F->wbase);

    // ---- once per workgroup: the filter's weights (all layers), its biases, the time grid
    if (resident)
        for (int i = threadIdx.x; i < F->wtotal / 4; i += 512) w_s[i] = w_g[i];
    for (int i = threadIdx.x; i < F->btotal; i += 512) bias_s[i] = G.bias[F->bbase + i];
    if (lc_out != nullptr)
        for (int t = threadIdx.x; t < NT; t += 512) tts[t] = G.tt[(size_t)m * NT + t];

    const long n_pairs = (B + 2 * MLP_TILE - 1) / (2 * MLP_TILE);
    for (long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
        const long tile0 = (2 * pair + half) * MLP_TILE;        // (an odd batch's last pair: the second half works on x = 0 and stores nothing)
        {   // the input block in B-operand order: lane (p / 4) 16 + s, register p % 4 (rows beyond the batch evaluate x = 0: nothing stored)
            const int s = tid >> 4, p = tid & 15;
            const long b = tile0 + s;
            float v = 0.f;
            if (b < B && p < NP) v = (float)((apply_slot(em->model_param[p], theta + b * ld) - G.pmin[m * NP + p]) / G.pspan[m * NP + p]);
            panel0[((p >> 2) * 16 + s) * 4 + (p & 3)] = v;
        }
        __syncthreads();

        float* ain = panel0;
        float* aout = panel1;
        for (int li = 0; li < nl; ++li) {
            const int kb = F->kb[li], ub = F->ub[li], wo = F->woff[li] / 4;
            const float* bl = bias_s + F->boff[li];
            for (int u = wave; u < ub; u += 4) {
                const f32x4 bias = *reinterpret_cast<const f32x4*>(bl + 16 * u + 4 * (lane >> 4));
                const int blk = wo + u * kb * 64;
                const f32x4 d = resident ? mlp_out_tile(w_s + blk, reinterpret_cast<const f32x4*>(ain), bias, kb, lane)
                                         : mlp_out_tile(w_g + blk, reinterpret_cast<const f32x4*>(ain), bias, kb, lane);
                if (li + 1 < nl) {
                    f32x4 h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] = d[r] < 0.f ? 0.f : d[r];        // relu (a NaN stays a NaN, as in the reference)
                    reinterpret_cast<f32x4*>(aout)[u * 64 + lane] = h;
                } else {                            // the output layer: one tile (NC <= 16)
                    const int s = lane & 15;
                    const long b = tile0 + s;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 4 * (lane >> 4) + r;
                        coef[s * 16 + i] = (double)d[r];
                        if (coeff_out != nullptr && b < B && i < NC) coeff_out[((size_t)b * M + m) * NC + i] = (double)d[r];
                    }
                }
            }
            __syncthreads();                        // the layer's panel (or the coefficients) is complete
            float* tmp = ain; ain = aout; aout = tmp;
        }
        if (lc_out == nullptr) continue;

        // ---- reconstruction on the fp64 matrix cores: 16 nodes x 16 samples per v_mfma_f64_16x16x4_f64.  A lane holds
        // A[node lane % 16][k = lane / 16], B[k = lane / 16][sample lane % 16], D[node 4 r + lane / 16][sample lane % 16]
        typedef double f64x4_t __attribute__((ext_vector_type(4)));
        const double* __restrict__ VA = G.VA + (size_t)m * NT * NC;
        const int n_tt = (NT + 15) / 16;
        for (int nt = wave; nt < n_tt; nt += 4) {
            const int t_a = nt * 16 + (lane & 15);
            f64x4_t d = {0.0, 0.0, 0.0, 0.0};
            for (int kk = 0; kk < (NC + 3) / 4; ++kk) {
                const int k = kk * 4 + (lane >> 4);
                const double a = (t_a < NT && k < NC) ? VA[(size_t)t_a * NC + k] : 0.0;
                const double bq = coef[(lane & 15) * 16 + k];
                d = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq, d, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = nt * 16 + 4 * r + (lane >> 4);
                if (t < NT) magb[(lane & 15) * NTE + t] = d[r] * G.span[(size_t)m * NT + t] + G.mins[(size_t)m * NT + t];
            }
        }
        __syncthreads();

        // ---- np.interp(sample_times, tt, mag, left = right = inf).  (The next tile's barriers keep its writes to coef and magb
        // behind these reads.)
        const int NS = em->NS;
        const double* __restrict__ st = em->st;
        const double t_lo = tts[0], t_hi = tts[NT - 1];
        for (int idx = tid; idx < MLP_TILE * NS; idx += 256) {
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
                const double* row = magb + sl * NTE;
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
}

// W [K][H] row-major (a Keras Dense kernel) -> the blocks [u][t][lane][4] the kernel reads, zero where the padding lies
static void mlp_swizzle(const float* W, int K, int H, int kb, int ub, float* dst) {
    for (int u = 0; u < ub; ++u)
        for (int t = 0; t < kb; ++t)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * t + 4 * (l >> 4) + r, o = 16 * u + (l & 15);
                    *dst++ = (k < K && o < H) ? W[(size_t)k * H + o] : 0.f;
                }
}

}  // namespace nmma

struct nmma_mlp_handle {
    nmma::MlpDev dev{};
    int device = 0;
    int lds_bytes = 0;
    int grid_x = 1;                 // persistent workgroups per filter
    std::vector<void*> owned;
};

using namespace nmma;

namespace {

template <typename T>
hipError_t mlp_upload(const std::vector<T>& v, const T** dst, std::vector<void*>& owned) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (!v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    *dst = reinterpret_cast<const T*>(p);
    return e;
}

int mlp_call(nmma_mlp_handle* mlp, nmma_em_handle* em, const double* theta, int64_t B, int64_t ld, double* coeff, double* lc, void* stream,
             const char* who) {
    if (!mlp || !em) return fail(std::string(who) + ": null handle");
    if (B < 0) return fail(std::string(who) + ": negative batch");
    if (B == 0) return 0;
    if (!theta || (!coeff && !lc)) return fail(std::string(who) + ": null buffer");
    if (ld < em->dev.D) return fail(std::string(who) + ": leading dimension smaller than n_dim");
    if (em->device != mlp->device) return fail(std::string(who) + ": the two handles live on different devices");
    if (em->dev.NP != mlp->dev.NP) return fail(std::string(who) + ": the em handle's n_params differs from the surrogate's");
    if (lc && em->dev.M != mlp->dev.M) return fail(std::string(who) + ": the em handle's n_model_filters differs from the surrogate's");
    NM_HIP(hipSetDevice(mlp->device));
    const int64_t tiles = (B + 2 * MLP_TILE - 1) / (2 * MLP_TILE);      // pairs of tiles
    const unsigned gx = (unsigned)std::min<int64_t>(tiles, mlp->grid_x);
    if (mlp->lds_bytes > 64 * 1024)
        NM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_surrogate), hipFuncAttributeMaxDynamicSharedMemorySize, mlp->lds_bytes));
    hipLaunchKernelGGL(mlp_surrogate, dim3(gx, (unsigned)mlp->dev.M), dim3(512), mlp->lds_bytes, static_cast<hipStream_t>(stream), mlp->dev,
                       em->dev_d, theta, (long)B, (long)ld, coeff, lc);
    NM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

void nmma_mlp_destroy(nmma_mlp_handle* mlp) {
    if (!mlp) return;
    (void)hipSetDevice(mlp->device);
    for (void* p : mlp->owned) (void)hipFree(p);
    delete mlp;
}

int32_t nmma_mlp_create(const nmma_mlp_config* c, nmma_mlp_handle** out) {
    if (!c || !out) return fail("nmma_mlp_create: null argument");
    *out = nullptr;
    if (c->abi_version != NMMA_ABI_VERSION) return fail("nmma_mlp_create: ABI version mismatch");
    const int M = c->n_model_filters, NP = c->n_params, NC = c->n_coeff, NT = c->n_tt;
    if (M < 1 || NP < 1 || NP > NMMA_MAX_PARAMS || NC < 1 || NC > NMMA_MAX_COEFF || NT < 2) return fail("nmma_mlp_create: bad surrogate dimensions");
    if (!c->n_layers || !c->widths || !c->weights || !c->weight_offsets || !c->biases || !c->bias_offsets || !c->VA || !c->mins || !c->maxs ||
        !c->tt || !c->param_mins || !c->param_maxs)
        return fail("nmma_mlp_create: null surrogate tensor");
    for (int m = 0; m < M; ++m) {
        for (int t = 1; t < NT; ++t)
            if (!(c->tt[(size_t)m * NT + t] > c->tt[(size_t)m * NT + t - 1])) return fail("nmma_mlp_create: tt must increase");
        for (int p = 0; p < NP; ++p)
            if (!(c->param_maxs[m * NP + p] - c->param_mins[m * NP + p] != 0.0)) return fail("nmma_mlp_create: empty parameter range");
    }

    // ---- per filter: the chain of padded shapes, the swizzled weights and the padded biases
    std::vector<MlpFilter> filt(M);
    std::vector<float> W, bias;
    int act_floats = MLP_TILE * 16, bias_floats = 16;
    for (int m = 0; m < M; ++m) {
        MlpFilter& F = filt[m];
        std::memset(&F, 0, sizeof(F));
        const int L = c->n_layers[m];
        if (L < 1 || L > NMMA_MLP_MAX_HIDDEN)
            return fail("nmma_mlp_create: filter " + std::to_string(m) + ": " + std::to_string(L) + " hidden layers; the kernel serves 1 .. " +
                        std::to_string(NMMA_MLP_MAX_HIDDEN));
        F.nl = L + 1;
        F.wbase = (int64_t)W.size();
        F.bbase = (int64_t)bias.size();
        const float* wsrc = c->weights + c->weight_offsets[m];
        const float* bsrc = c->biases + c->bias_offsets[m];
        int K = NP;
        for (int li = 0; li <= L; ++li) {
            const int H = li < L ? c->widths[m * NMMA_MLP_MAX_HIDDEN + li] : NC;
            if (li < L && (H < 1 || H > MLP_MAX_WIDTH))
                return fail("nmma_mlp_create: filter " + std::to_string(m) + ", hidden layer " + std::to_string(li + 1) + ": width " +
                            std::to_string(H) + " is outside 1 .. " + std::to_string(MLP_MAX_WIDTH) +
                            " (two 16-sample activation panels of the widest layer must fit the workgroup's LDS)");
            F.kb[li] = (K + 15) / 16;
            F.ub[li] = (H + 15) / 16;
            F.woff[li] = F.wtotal;
            F.boff[li] = F.btotal;
            const size_t w0 = W.size(), b0 = bias.size();
            W.resize(w0 + (size_t)F.kb[li] * F.ub[li] * 256);
            mlp_swizzle(wsrc, K, H, F.kb[li], F.ub[li], W.data() + w0);
            bias.resize(b0 + (size_t)F.ub[li] * 16, 0.f);
            std::copy(bsrc, bsrc + H, bias.begin() + b0);
            F.wtotal += F.kb[li] * F.ub[li] * 256;
            F.btotal += F.ub[li] * 16;
            act_floats = std::max(act_floats, MLP_TILE * 16 * F.ub[li]);
            wsrc += (size_t)K * H;
            bsrc += H;
            K = H;
        }
        bias_floats = std::max(bias_floats, (int)F.btotal);
    }
    const int fixed = mlp_lds_fixed_bytes(NT, act_floats, bias_floats);
    if (fixed > LDS_DYNAMIC_MAX) return fail("nmma_mlp_create: the time grid does not fit the workgroup's LDS beside the activation panels (n_tt too large)");
    int w_floats = 0;
    for (MlpFilter& F : filt) {
        F.resident = fixed + F.wtotal * (int)sizeof(float) <= LDS_DYNAMIC_MAX;
        if (F.resident) w_floats = std::max(w_floats, (int)F.wtotal);
    }

    int ndev = 0;
    NM_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail("nmma_mlp_create: no HIP device (this library has no CPU fallback)");
    if (c->device < 0 || c->device >= ndev) return fail("nmma_mlp_create: bad device ordinal");
    NM_HIP(hipSetDevice(c->device));
    int n_cu = 0;
    NM_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));

    auto* mlp = new nmma_mlp_handle();
    mlp->device = c->device;
    mlp->lds_bytes = fixed + w_floats * (int)sizeof(float);
    // one round of workgroups: M filters share the CUs, each workgroup walks its share of the tiles with the weights in place
    mlp->grid_x = std::max(1, n_cu / M);
    MlpDev& G = mlp->dev;
    G.M = M; G.NP = NP; G.NC = NC; G.NT = NT;
    G.act_floats = act_floats;
    G.bias_floats = bias_floats;
    std::vector<double> span((size_t)M * NT), pspan((size_t)M * NP);
    for (size_t i = 0; i < span.size(); ++i) span[i] = c->maxs[i] - c->mins[i];
    for (size_t i = 0; i < pspan.size(); ++i) pspan[i] = c->param_maxs[i] - c->param_mins[i];
#define NM_MLP_UP(vec, field)                                                                               \
    do {                                                                                                    \
        const hipError_t _e = mlp_upload(vec, &G.field, mlp->owned);                                        \
        if (_e != hipSuccess) {                                                                             \
            nmma_mlp_destroy(mlp);                                                                          \
            return fail(std::string("nmma_mlp_create: upload " #field " failed: ") + hipGetErrorString(_e)); \
        }                                                                                                   \
    } while (0)
    NM_MLP_UP(filt, filt);
    NM_MLP_UP(W, W);
    NM_MLP_UP(bias, bias);
    NM_MLP_UP(std::vector<double>(c->VA, c->VA + (size_t)M * NT * NC), VA);
    NM_MLP_UP(std::vector<double>(c->mins, c->mins + (size_t)M * NT), mins);
    NM_MLP_UP(span, span);
    NM_MLP_UP(std::vector<double>(c->tt, c->tt + (size_t)M * NT), tt);
    NM_MLP_UP(std::vector<double>(c->param_mins, c->param_mins + (size_t)M * NP), pmin);
    NM_MLP_UP(pspan, pspan);
#undef NM_MLP_UP
    *out = mlp;
    return 0;
}

int32_t nmma_mlp_coefficients(nmma_mlp_handle* mlp, nmma_em_handle* em, const double* theta_dev, int64_t B, int64_t ld, double* coeff_dev,
                              void* stream) {
    return mlp_call(mlp, em, theta_dev, B, ld, coeff_dev, nullptr, stream, "nmma_mlp_coefficients");
}

int32_t nmma_mlp_model_lightcurves(nmma_mlp_handle* mlp, nmma_em_handle* em, const double* theta_dev, int64_t B, int64_t ld, double* lc_dev,
                                   void* stream) {
    return mlp_call(mlp, em, theta_dev, B, ld, nullptr, lc_dev, stream, "nmma_mlp_model_lightcurves");
}

}  // extern "C"
