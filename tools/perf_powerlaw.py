#!/usr/bin/env python
"""Time the Sr2023 power-law model (kernels powerlaw_logl / powerlaw_lc, EMEngine(model_kind="powerlaw")) on a 3-filter and a 9-filter
case: the model's default 150-node grid, a sampled em_syserr, 12 data per filter drawn around a truth curve.

    perf_powerlaw.py [B ...]            per case and batch size (default 4096 65536), HIP-event time per call after two seconds of
                                        warm-up: loglike (one launch), model_lightcurves + loglike_lc (two launches); then what the parent
                                        commit offers -- a vectorised numpy generator (the arithmetic of host_lc for the whole batch; host
                                        clock), the upload of lc[B, M, NS] and loglike_lc on an external-kind engine
    perf_powerlaw.py ... --launches K   K calls of each device form and nothing else (the body of a profiler run: kernel statistics)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.perf_piro2021 import event_time  # noqa: E402
from nmma_amd import synthetic as syn  # noqa: E402

FILTERS9 = ["u", "g", "r", "i", "z", "y", "J", "H", "K"]


def numpy_curves(st, theta, m, host_mag):
    """host_lc + flux_to_ABmag for a batch: lc[B, M, NS]."""
    with np.errstate(all="ignore"):
        flux = theta[:, 4:4 + m, None] * np.power(st[None, None, :], -theta[:, 3, None, None]) + theta[:, 4 + m:4 + 2 * m, None]
        mag = np.where(flux > 0, -2.5 * np.log10(flux) + host_mag, np.inf)
    mag[(flux > 0).sum(axis=2) < 2] = np.nan
    return mag


def main():
    import torch
    from nmma_amd.engine import EMEngine
    args = sys.argv[1:sys.argv.index("--launches")] if "--launches" in sys.argv else sys.argv[1:]
    sizes = [int(a) for a in args if a.isdigit()] or [4096, 65536]
    st, grid, rng = np.geomspace(0.01, 14.0, 150), syn.flat_lcdm_grid(1.0, 200.0), np.random.default_rng(11)
    for filters in (FILTERS9[1:4], FILTERS9):
        m = len(filters)
        names = ["luminosity_distance", "timeshift", "em_syserr", "alpha_AG"] + [f"a_AG_{f}" for f in filters] + [f"f_nu_{f}" for f in filters]
        draw = lambda n: np.column_stack([rng.uniform(40, 80, n), rng.uniform(0.0, 0.1, n), rng.uniform(0.1, 0.5, n), rng.uniform(0.8, 1.4, n)]
                                         + [rng.uniform(80, 200, n) for _ in filters] + [rng.uniform(2, 10, n) for _ in filters])
        truth = numpy_curves(st, draw(1), m, 23.9)[0] + 5 * (5 + np.log10(60.0))
        times = {f: np.sort(rng.uniform(0.1, 12.0, 12)) for f in filters}
        data = (times, {f: np.interp(times[f], st, truth[k]) + 0.1 * rng.standard_normal(12) for k, f in enumerate(filters)},
                {f: np.full(12, 0.1) for f in filters})
        common = dict(sample_times=st, cosmo_grid=grid, data=data, observed_filters=filters, systematics={"mode": "param", "name": "em_syserr"})
        eng = EMEngine(None, filters, names[3:], names, model_kind="powerlaw", powerlaw=dict(model="Sr2023", host_mag=23.9), **common)
        host = EMEngine(None, filters, [], names, model_kind="external", **common)
        assert eng.powerlaw_fused
        for batch in sizes:
            theta_np = draw(batch)
            theta = torch.as_tensor(theta_np, device="cuda:0")
            two = lambda: eng.loglike_lc(theta, eng.model_lightcurves(theta))
            diff = (eng.loglike(theta) - two()).abs().max().item()
            if "--launches" in sys.argv:
                for _ in range(int(sys.argv[sys.argv.index("--launches") + 1])):
                    eng.loglike(theta)
                    two()
                torch.cuda.synchronize()
                continue
            report = lambda what, t: print(f"M={m} B={batch} {what}: {t[0]:.1f} us per call (5 windows of 20: {t[1]:.1f} .. {t[2]:.1f})")
            report("loglike (powerlaw_logl, one launch)", event_time(lambda: eng.loglike(theta)))
            report("model_lightcurves + loglike_lc (two launches)", event_time(two))
            gen, up = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                lc = numpy_curves(st, theta_np, m, 23.9)
                t1 = time.perf_counter()
                host.loglike_lc(theta, torch.as_tensor(lc).to("cuda:0"))
                torch.cuda.synchronize()
                gen.append(t1 - t0)
                up.append(time.perf_counter() - t1)
            print(f"M={m} B={batch} parent route: numpy generator {min(gen) * 1e3:.1f} ms, upload + loglike_lc {min(up) * 1e3:.1f} ms (best of 3); "
                  f"max |one launch - two launches| = {diff:.2e}")
        eng.close()
        host.close()


if __name__ == "__main__":
    main()
