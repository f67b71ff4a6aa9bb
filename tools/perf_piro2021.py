#!/usr/bin/env python
"""Time the Piro2021 shock-cooling model (kernel piro2021_lc, EMEngine(model_kind="piro2021")) at 9 filters x the default 100-node grid
with the photometry of tests/golden/piro2021.npz.

    perf_piro2021.py [B ...]            per batch size (default 4096 65536), HIP-event time per call after two seconds of warm-up:
                                        loglike (curves + likelihood, two launches), model_lightcurves alone (the kernel), the kernel's
                                        measurement forms (phase C without its stores / without its transcendentals: option "sc_probe")
                                        and its tile sizes (option "sc_tile"); then the host route for the same rows -- a vectorised
                                        numpy generate_lightcurve_batch, the upload of lc[B, M, NS] and loglike_lc -- on the host clock
                                        around a device synchronise
    perf_piro2021.py ... --launches K   K plain model_lightcurves launches and nothing else (the body of a profiler run)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "piro2021.npz")
PARAMS = ["log10_Menv", "log10_Renv", "log10_Ee"]
CENTRE = dict(luminosity_distance=40.0, timeshift=0.05, log10_Menv=-1.7, log10_Renv=13.3, log10_Ee=49.6)


def numpy_curves(st, p, nu0, z):
    """sc_bol_lc / sc_lc for a batch: {parameter: [B]} -> mag[B, M, NS] (the arithmetic of lightcurve_generation.py:314-363, :43-58)."""
    msun, c, h, kb, sig, D = 1.988409870698051e33, 2.99792458e10, 6.62607015e-27, 1.380649e-16, 5.6703744191844314e-05, 10 * 3.085677581491367e18
    n, delta, kappa = 10, 1.1, 0.2
    K = (n - 3) * (3 - delta) / (4 * np.pi * (n - delta))
    t = (st * 86400.0)[None, :]
    Me, Renv, Ee = (10 ** p["log10_Menv"] * msun)[:, None], (10 ** p["log10_Renv"])[:, None], (10 ** p["log10_Ee"])[:, None]
    with np.errstate(all="ignore"):
        vt = np.sqrt(((n - 5) * (5 - delta) / ((n - 3) * (3 - delta))) * (2 * Ee / Me))
        td = np.sqrt((3 * kappa * K * Me) / ((n - 1) * vt * c))
        tph = np.sqrt(3 * kappa * K * Me / (2 * (n - 1) * vt * vt))
        pref = np.pi * (n - 1) / (3 * (n - 5)) * c * Renv * vt * vt / kappa
        L = np.where(t < td, pref * np.power(td / t, 4 / (n - 2)), pref * np.exp(-0.5 * (t * t / td / td - 1)))
        R = np.where(t < tph, np.power(tph / t, 2 / (n - 1)) * vt * t, np.power(1 + (delta - 1) / (n - 1) * ((t / tph) ** 2 - 1), -1 / (delta - 1)) * vt * t)
        T = np.power(L / (4 * np.pi * R * R) / sig, 0.25)
        T[T == 0.0] = np.nan
        inv = 1.0 / T
        inv[~np.isfinite(inv)] = np.inf
        nu = nu0[None, :, None] * (1 + z)[:, None, None]
        F = 2.0 * h / c ** 2 * nu ** 3 / np.expm1(np.clip(h * nu * inv[:, None, :] / kb, None, 700)) * R[:, None, :] * R[:, None, :] / D ** 2
        mag = np.where(F > 0, -2.5 * np.log10(np.where(F > 0, F, 1.0)) - 48.6, np.inf)
    mag[(F > 0).sum(axis=2) < 2] = np.nan
    return mag


def event_time(call, n=20, windows=5):
    import torch
    t_end = time.perf_counter() + 2.0          # warm clocks: two seconds of untimed calls
    while time.perf_counter() < t_end:
        call()
        torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / n * 1e3)
    return float(np.median(times)), min(times), max(times)


def main():
    import torch
    from nmma_amd.engine import EMEngine
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [4096, 65536]
    with np.load(GOLDEN, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    names, filters = [str(n) for n in g["names"]], [str(f) for f in g["filters"]]
    st, grid = g["g100/sample_times"], (g["dist_grid"], g["z_grid"])
    data = tuple({f: g[f"data/{f}/{k}"] for f in filters} for k in "tms")
    common = dict(sample_times=st, cosmo_grid=grid, data=data, observed_filters=filters)
    eng = EMEngine(None, filters, PARAMS, names, model_kind="piro2021", filter_nu0=dict(zip(filters, g["nu0"])), **common)
    host = EMEngine(None, filters, PARAMS, names, model_kind="external", **common)
    rng = np.random.default_rng(7)
    for batch in sizes:
        theta_np = np.column_stack([rng.uniform(CENTRE[n] - 0.4, CENTRE[n] + 0.4, batch) if n.startswith("log10") else
                                    rng.uniform(0.75 * CENTRE[n], 1.25 * CENTRE[n], batch) for n in names])
        theta = torch.as_tensor(theta_np, device="cuda:0")
        if "--launches" in sys.argv:
            for _ in range(int(sys.argv[sys.argv.index("--launches") + 1])):
                eng.model_lightcurves(theta)
            torch.cuda.synchronize()
            continue
        items = batch * len(filters) * len(st)
        report = lambda what, t: print(f"B={batch} {what}: {t[0]:.1f} us per call (5 windows of 20: {t[1]:.1f} .. {t[2]:.1f}), "
                                       f"{items / t[0]:.0f} magnitudes/us, {items * 8 / t[0] * 1e-6:.3f} TB/s of curve stores")
        report("loglike (piro2021_lc + likelihood)", event_time(lambda: eng.loglike(theta)))
        report("model_lightcurves (piro2021_lc)", event_time(lambda: eng.model_lightcurves(theta)))
        for probe, what in ((1, "phase C without stores"), (2, "phase C without transcendentals")):
            eng.set_option("sc_probe", probe)
            report(f"piro2021_lc, {what}", event_time(lambda: eng.model_lightcurves(theta)))
        eng.set_option("sc_probe", 0)
        for tile in (2, 4, 8, 16, 32):
            eng.set_option("sc_tile", tile)
            report(f"piro2021_lc, {tile} rows per tile", event_time(lambda: eng.model_lightcurves(theta)))
        eng.set_option("sc_tile", 0)
        # the host route: numpy curves for the whole batch, upload, likelihood from curves
        p = {n: theta_np[:, k] for k, n in enumerate(names)}
        zrow = np.interp(p["luminosity_distance"], *grid)
        want = eng.loglike(theta).cpu().numpy()
        times, parts = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            lc = numpy_curves(st, p, g["nu0"], zrow)
            t1 = time.perf_counter()
            got = host.loglike_lc(theta, torch.as_tensor(lc).to("cuda:0"))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            times.append(t2 - t0)
            parts.append((t1 - t0, t2 - t1))
        k = int(np.argmin(times))
        rel = np.abs(got.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
        print(f"B={batch} host route (numpy generate_lightcurve_batch + upload + loglike_lc): {times[k] * 1e3:.1f} ms per call (best of 3; "
              f"numpy {parts[k][0] * 1e3:.1f} ms, upload + likelihood {parts[k][1] * 1e3:.1f} ms); worst relative difference to the device route {rel.max():.2e}")
    eng.close()
    host.close()


if __name__ == "__main__":
    main()
