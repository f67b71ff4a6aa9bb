#!/usr/bin/env python
"""Time the HoNa2020 kilonova (kernel hona2020_lc, EMEngine(model_kind="hona2020")) at 9 filters x the default 150-node grid with the
photometry of tests/golden/hona2020.npz.

    perf_hona2020.py [B ...]            per batch size (default 4096 65536), HIP-event time per call after two seconds of warm-up:
                                        loglike (curves + likelihood, two launches), model_lightcurves alone (the kernel), and the
                                        kernel on a TWO-node grid [0.05, 14] with one filter -- the same integration (phases S and I)
                                        with next to nothing of phases P and C, which gives the split; then the host route -- the plain
                                        numpy restatement of tools/make_golden_hona2020.py on the first 64 rows (host clock, per row),
                                        the upload of lc[B, M, NS] and loglike_lc for the whole batch
    perf_hona2020.py ... --launches K   K plain model_lightcurves launches and nothing else (the body of a profiler run)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.perf_piro2021 import event_time  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "hona2020.npz")
PARAMS = ["log10_mej", "vej_max", "vej_min", "vej_frac", "log10_kappa_low_vej", "log10_kappa_high_vej"]
BOX = dict(luminosity_distance=(30.0, 55.0), timeshift=(0.07, 0.13), log10_mej=(-3.0, -1.0), vej_max=(0.3, 0.8), vej_min=(0.02, 0.2),
           vej_frac=(0.0, 1.0), log10_kappa_low_vej=(-1.0, 1.5), log10_kappa_high_vej=(-1.0, 1.5))


def main():
    import torch
    from nmma_amd.engine import EMEngine
    args = sys.argv[1:sys.argv.index("--launches")] if "--launches" in sys.argv else sys.argv[1:]
    sizes = [int(a) for a in args if a.isdigit()] or [4096, 65536]
    with np.load(GOLDEN, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    names, filters = [str(n) for n in g["names"]], [str(f) for f in g["filters"]]
    st, grid, nu0 = g["g150/sample_times"], (g["dist_grid"], g["z_grid"]), dict(zip(filters, g["nu0"]))
    data = tuple({f: g[f"data/{f}/{k}"] for f in filters} for k in "tms")
    common = dict(sample_times=st, cosmo_grid=grid, data=data, observed_filters=filters)
    eng = EMEngine(None, filters, PARAMS, names, model_kind="hona2020", filter_nu0=nu0, **common)
    two = EMEngine(None, filters[:1], PARAMS, names, model_kind="hona2020", filter_nu0=nu0, sample_times=st[[0, -1]], cosmo_grid=grid)
    host = EMEngine(None, filters, PARAMS, names, model_kind="external", **common)
    rng = np.random.default_rng(7)
    for batch in sizes:
        theta_np = np.column_stack([rng.uniform(*BOX[n], batch) for n in names])
        theta = torch.as_tensor(theta_np, device="cuda:0")
        if "--launches" in sys.argv:
            for _ in range(int(sys.argv[sys.argv.index("--launches") + 1])):
                eng.model_lightcurves(theta)
            torch.cuda.synchronize()
            continue
        steps = eng.hona_steps(theta).cpu().numpy()
        print(f"B={batch}: accepted steps {steps[:, 0].min()} .. {steps[:, 0].max()} (mean {steps[:, 0].mean():.1f}), rejected up to {steps[:, 1].max()} "
              f"(mean {steps[:, 1].mean():.2f}); NaN rows {int(np.isnan(eng.model_lightcurves(theta).cpu().numpy()).all(axis=(1, 2)).sum())}")
        report = lambda what, t: print(f"B={batch} {what}: {t[0]:.1f} us per call (5 windows of 20: {t[1]:.1f} .. {t[2]:.1f}), {t[0] / batch * 1e3:.1f} ns per row")
        report("loglike (hona2020_lc + likelihood)", event_time(lambda: eng.loglike(theta)))
        report("model_lightcurves (hona2020_lc)", event_time(lambda: eng.model_lightcurves(theta)))
        report("hona2020_lc on the two-node grid, one filter (phases S + I)", event_time(lambda: two.model_lightcurves(theta)))
        # the host route: the numpy restatement row by row (first 64 rows), then upload + likelihood from curves for the batch
        from scipy.special import erfc
        from tools.make_golden_hona2020 import hona_numpy
        zrow = np.interp(theta_np[:, 0], *grid)
        t0 = time.perf_counter()
        for r in range(64):
            hona_numpy(st, dict(zip(names, theta_np[r])), g["nu0"] * (1 + zrow[r]), erfc)
        per_row = (time.perf_counter() - t0) / 64
        lc = eng.model_lightcurves(theta).cpu()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            host.loglike_lc(theta, lc.to("cuda:0"))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        print(f"B={batch} host route: numpy restatement {per_row * 1e3:.2f} ms per row (64 rows timed; {per_row * batch:.1f} s for the batch), "
              f"upload + loglike_lc {min(times) * 1e3:.1f} ms per call (best of 3)")
    for e in (eng, two, host):
        e.close()


if __name__ == "__main__":
    main()
