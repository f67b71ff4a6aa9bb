#!/usr/bin/env python
"""Time the Gaussian-process surrogate kernel (gp_surrogate, nmma_gp_model_lightcurves / nmma_gp_coefficients).

    perf_gp.py [golden|synthetic] [B]      HIP-event time per launch after warm-up, powers per call, share of the fp64 vector peak
    perf_gp.py ... --launches K            K plain launches and nothing else (the body of a rocprofv3 --kernel-trace --stats run)
    perf_gp.py ... --sklearn               no GPU: the rate of the reference's loop (n_coeff calls of gp.predict(return_std=True) per
                                           filter and row, lightcurve_generation.py:206-211) with scikit-learn regressors of the same size

golden: tests/golden/gp_bulla.npz (N = 28, M = 9, NC = 10).  synthetic: N = 2048, NP = 4, M = 9, NC = 10 (Bu2019lm's size).
Flop count per power (FLOP_PER_POWER): the fp64 instructions of one (sample, training point, coefficient) step in the gfx950 ISA of
gp_surrogate<NC> -- division, ocml pow, two multiplies, one add: 171 instructions of which 32 are fused multiply-adds."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOP_PER_POWER = 171 + 32
FP64_VECTOR_PEAK = 78.6e12        # MI355X, fp64 vector, FLOP/s
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gp_bulla.npz")
_KEYS = ("gp_X", "gp_alpha", "gp_const", "gp_ell", "gp_rq_alpha", "gp_ymean", "gp_ystd", "VA", "mins", "maxs", "tt", "param_mins", "param_maxs")


def golden_model():
    with np.load(GOLDEN, allow_pickle=False) as z:
        filters = [str(f) for f in z["filters"]]
        svd = {f: dict({k: z[f"{f}/{k}"] for k in _KEYS}, n_coeff=int(z[f"{f}/n_coeff"])) for f in filters}
        return svd, [str(n) for n in z["model_parameters"]]


def synthetic_model(n=2048, n_p=4, m=9, n_c=10, n_t=100, seed=11):
    rng = np.random.default_rng(seed)
    svd = {}
    for k in range(m):
        svd[f"f{k}"] = dict(gp_X=rng.uniform(size=(n, n_p)), gp_alpha=rng.standard_normal((n_c, n)), gp_const=rng.uniform(0.5, 2.0, n_c),
                            gp_ell=rng.uniform(0.3, 2.0, n_c), gp_rq_alpha=10.0 ** rng.uniform(-2, 1, n_c), gp_ymean=np.zeros(n_c), gp_ystd=np.ones(n_c),
                            VA=rng.standard_normal((n_t, n_c)), mins=np.full(n_t, -20.0), maxs=np.full(n_t, -5.0), tt=np.linspace(0.0, 20.0, n_t),
                            param_mins=np.zeros(n_p), param_maxs=np.ones(n_p), n_coeff=n_c)
    return svd, [f"p{k}" for k in range(n_p)]


def sklearn_rate(svd, rows=8):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RationalQuadratic
    t = next(iter(svd.values()))
    rng = np.random.default_rng(0)
    gps = [GaussianProcessRegressor(kernel=t["gp_const"][i] * RationalQuadratic(t["gp_ell"][i], t["gp_rq_alpha"][i]), optimizer=None, alpha=1e-6)
           .fit(t["gp_X"], rng.standard_normal(len(t["gp_X"]))) for i in range(t["n_coeff"])]
    x = rng.uniform(size=(rows, t["gp_X"].shape[1]))
    t0 = time.perf_counter()
    for row in x:
        for _ in svd:
            for gp in gps:
                gp.predict(np.atleast_2d(row), return_std=True)
    dt = (time.perf_counter() - t0) / rows
    powers = len(svd) * t["n_coeff"] * len(t["gp_X"])
    print(f"sklearn gp.predict loop: {dt * 1e3:.2f} ms per row ({len(svd)} filters x {t['n_coeff']} coefficients, N = {len(t['gp_X'])}), "
          f"{powers / dt / 1e6:.2f} M kernel values/s")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "synthetic"
    batch = int(args[1]) if len(args) > 1 else 4096
    svd, params = golden_model() if which == "golden" else synthetic_model()
    if "--sklearn" in sys.argv:
        return sklearn_rate(svd)
    import torch
    from nmma_amd.engine import EMEngine
    eng = EMEngine(svd, list(svd), params, params, model_kind="svd_gp")
    lo, hi = next(iter(svd.values()))["param_mins"], next(iter(svd.values()))["param_maxs"]
    theta = torch.as_tensor(np.random.default_rng(7).uniform(lo, hi, (batch, len(params))), device="cuda:0")
    if "--launches" in sys.argv:
        for _ in range(int(sys.argv[sys.argv.index("--launches") + 1])):
            eng.model_lightcurves(theta)
        torch.cuda.synchronize()
        return eng.close()
    powers = batch * sum(len(t["gp_X"]) * t["n_coeff"] for t in svd.values())
    for name, call in (("model_lightcurves", eng.model_lightcurves), ("coefficients", eng.coefficients)):
        t_end = time.perf_counter() + 2.0          # warm clocks: two seconds of untimed launches
        while time.perf_counter() < t_end:
            call(theta)
            torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 20
            e0.record()
            for _ in range(n):
                call(theta)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / n * 1e-3)
        med = float(np.median(times))
        print(f"{which} B={batch} {name}: {med * 1e6:.1f} us per launch (5 windows of 20: {min(times) * 1e6:.1f} .. {max(times) * 1e6:.1f}), "
              f"{powers:.3e} powers per call, {powers / med / 1e9:.1f} G powers/s, "
              f"{powers * FLOP_PER_POWER / med / FP64_VECTOR_PEAK * 100:.1f} % of the fp64 vector peak at {FLOP_PER_POWER} flop per power")
    eng.close()


if __name__ == "__main__":
    main()
