"""Time the deep-network surrogate kernel (mlp_surrogate: nmma_mlp_model_lightcurves / nmma_mlp_coefficients) and the two-launch likelihood.

    perf_mlp.py [B]                  HIP-event time per call after warm-up: coefficients, curves, curves + likelihood (EMEngine.loglike)
    perf_mlp.py [B] --launches K     K plain model_lightcurves launches and nothing else (the body of a rocprofv3 --kernel-trace --stats run)

The network is the reference training tutorial's 6 -> 64 -> 128 -> 64 -> 10 in 9 filters, NT = 100, 20 photometry points per filter.
Flop per evaluation: 2 x 17 674 weights x 9 filters (the unpadded network; the kernel's zero padding to multiples of 16 is not counted)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MATRIX_PEAK = 157.3e12       # MI355X, fp32 MFMA, FLOP/s
WIDTHS, N_P, N_C, M, N_T = (64, 128, 64), 6, 10, 9, 100


def model(seed=11):
    rng = np.random.default_rng(seed)
    svd = {}
    for m in range(M):
        t, k = {}, N_P
        for i, h in enumerate(WIDTHS + (N_C,), start=1):
            t[f"W{i}"] = (rng.standard_normal((k, h)) * np.sqrt(2.0 / k)).astype(np.float32)
            t[f"b{i}"] = (0.1 * rng.standard_normal(h)).astype(np.float32)
            k = h
        q, _ = np.linalg.qr(rng.standard_normal((N_T, N_T)))
        t.update(VA=q[:, :N_C].copy(), mins=np.full(N_T, -17.0), maxs=np.full(N_T, -15.0), tt=np.linspace(0.0, 20.0, N_T),
                 param_mins=np.zeros(N_P), param_maxs=np.ones(N_P), n_coeff=N_C)
        svd[f"f{m}"] = t
    return svd


def main():
    import torch
    from nmma_amd.engine import EMEngine
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    batch = int(args[0]) if args else 4096
    svd, names = model(), [f"p{k}" for k in range(N_P)]
    rng = np.random.default_rng(3)
    times = {f: np.sort(rng.uniform(1.0, 19.0, 20)) for f in svd}
    data = (times, {f: -16.0 + 0.3 * rng.standard_normal(20) for f in svd}, {f: np.full(20, 0.2) for f in svd})
    eng = EMEngine(svd, list(svd), names, names, model_kind="svd_mlp", data=data, observed_filters=list(svd))
    theta = torch.as_tensor(rng.uniform(0.0, 1.0, (batch, N_P)), device="cuda:0")
    if "--launches" in sys.argv:
        for _ in range(int(sys.argv[sys.argv.index("--launches") + 1])):
            eng.model_lightcurves(theta)
        torch.cuda.synchronize()
        return eng.close()
    flop = batch * 2 * sum(t[f"W{i}"].size for t in svd.values() for i in range(1, len(WIDTHS) + 2))
    for name, call in (("coefficients", eng.coefficients), ("model_lightcurves", eng.model_lightcurves), ("loglike (two launches)", eng.loglike)):
        t_end = time.perf_counter() + 2.0          # warm clocks: two seconds of untimed launches
        while time.perf_counter() < t_end:
            call(theta)
            torch.cuda.synchronize()
        windows = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call(theta)
            e1.record()
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / 20 * 1e-3)
        med = float(np.median(windows))
        print(f"B={batch} {name}: {med * 1e6:.1f} us per call (5 windows of 20: {min(windows) * 1e6:.1f} .. {max(windows) * 1e6:.1f}), "
              f"{flop:.3e} network flop per call, {flop / med / 1e12:.2f} TFLOP/s = {flop / med / FP32_MATRIX_PEAK * 100:.1f} % of the fp32 MFMA peak")
    eng.close()


if __name__ == "__main__":
    main()
