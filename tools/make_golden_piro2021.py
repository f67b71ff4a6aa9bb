#!/usr/bin/env python
"""Golden data for the Piro2021 shock-cooling model (``ShockCoolingLightCurveModel``, kernel ``piro2021_lc``) from the reference's own
code.

Runs only in the build container (imports the reference under oracle/ref_harness.py; needs mpmath for the error measurement).  Steps:

1. candidate theta rows are drawn from a seeded box and sorted into the classes the kernel's branches make (CLASSES below); rows with a
   node whose reference ``L`` is subnormal are rejected (the relative rounding error of such an ``L`` is unbounded); the first rows of
   every class are kept, then ordinary rows around TRUTH (the rows whose log L is finite);
2. for three grids -- ``[0.5, 2, 3.5]`` with filter r, ``geomspace(1/24, 3.5, 65)`` with g, r, i and the model's default grid with the
   nine built-in Sloan / 2MASS names -- the reference's ``sc_bol_lc`` and ``sc_lc`` give the source-frame curves at the redshift
   ``np.interp(d_L, dist_grid, z_grid)`` of every row (the same number a sampled ``redshift`` column holds in the tests);
3. the terms of the tests' bound are recorded per row and node: ``xi = h (1 + z) / (kb T)`` (the clipped exponent of filter f is
   ``min(nu0_f xi, 700)``) and ``a = 0.5 (t / td)^2`` on the nodes at or after ``td``, 0 before;
4. the reference's curves are compared with an mpmath evaluation (50 digits) of the same closed form on the same doubles: the largest
   ``|mag - mag_mp| / (eps (1 + x + a) 2.5 / ln 10 + (2.5 / ln 10) 2 2^-1074 / F)`` is the K of numpy's own arithmetic (printed, stored
   as ``k_numpy``; the tests give the kernel four times that);
5. photometry is drawn around the reference model's detector-frame curves at TRUTH, and the reference's
   ``EMTransientLikelihood.log_likelihood`` around its ``ShockCoolingLightCurveModel`` is recorded for every row.

The file is written only if every class holds at least two rows and log L is finite on at least eight rows and floored on at least two.
Output: tests/golden/piro2021.npz -- ARRAYS ONLY (no pickles, no reference source).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from nmma_amd import synthetic as syn  # noqa: E402

SEED, PER_CLASS, N_ORDINARY = 20261127, 2, 12
FILTERS9 = ["u", "g", "r", "i", "z", "y", "J", "H", "K"]
GRIDS = {"g3": (np.array([0.5, 2.0, 3.5]), ["r"]), "g65": (np.geomspace(1.0 / 24.0, 3.5, 65), ["g", "r", "i"]),
         "g100": (np.geomspace(1.0 / 24.0, 3.5, 100), FILTERS9)}
NAMES = ["luminosity_distance", "timeshift", "log10_Menv", "log10_Renv", "log10_Ee"]
TRUTH = dict(luminosity_distance=40.0, timeshift=0.05, log10_Menv=-1.7, log10_Renv=13.3, log10_Ee=49.6)
BOX = dict(log10_Menv=(-4.5, 0.5), log10_Renv=(11.0, 15.0), log10_Ee=(47.0, 51.5))
CLASSES = ("td_inside", "td_before", "td_after", "tph_inside", "tph_before", "tph_after", "td_gt_tph", "L_zero", "some_inf", "all_nan_g3")
EPS, TINY = np.finfo(np.float64).eps, 2.0 ** -1074
MAG_PER_REL = 2.5 / np.log(10.0)


def timescales(ref, p):
    """(td, tph) in seconds as ``sc_bol_lc`` forms them (lightcurve_generation.py:319-344)."""
    msun, c = ref.lightcurve_generation.msun_cgs, ref.lightcurve_generation.c_cgs
    Me, Ee = 10 ** p["log10_Menv"] * msun, 10 ** p["log10_Ee"]
    n, delta, kappa = 10, 1.1, 0.2
    K = (n - 3) * (3 - delta) / (4 * np.pi * (n - delta))
    vt = np.sqrt(((n - 5) * (5 - delta) / ((n - 3) * (3 - delta))) * (2 * Ee / Me))
    return np.sqrt((3 * kappa * K * Me) / ((n - 1) * vt * c)), np.sqrt(3 * kappa * K * Me / (2 * (n - 1) * vt * vt))


def reference_curves(ref, st, p, nu_host, filters):
    """``(mag[M, NS], lbol[NS], Rs[NS])`` from the reference's sc_bol_lc / sc_lc."""
    lg = ref.lightcurve_generation
    with np.errstate(all="ignore"):
        lbol, Rs = lg.sc_bol_lc(st, p, compute_Rs=True)
        mag = lg.sc_lc(lbol, Rs, nu_host, filters)
    return np.array([mag[f] for f in filters]), lbol, Rs


def mp_curves(ref, st, p, nu_host):
    """The same closed form in 50-digit arithmetic on the same doubles: mag[M, NS] (rounded to double at the very end)."""
    import mpmath as mp
    mp.mp.dps = 50
    lg = ref.lightcurve_generation
    f = mp.mpf
    Me, Renv, Ee = f(10) ** f(p["log10_Menv"]) * f(lg.msun_cgs), f(10) ** f(p["log10_Renv"]), f(10) ** f(p["log10_Ee"])
    n, delta, kappa, c = f(10), f(1.1), f(0.2), f(lg.c_cgs)
    K = (n - 3) * (3 - delta) / (4 * mp.pi * (n - delta))
    vt = mp.sqrt((n - 5) * (5 - delta) / ((n - 3) * (3 - delta)) * (2 * Ee / Me))
    td, tph = mp.sqrt(3 * kappa * K * Me / ((n - 1) * vt * c)), mp.sqrt(3 * kappa * K * Me / (2 * (n - 1) * vt * vt))
    pref = mp.pi * (n - 1) / (3 * (n - 5)) * c * Renv * vt * vt / kappa
    out = np.empty((len(nu_host), len(st)))
    for j, days in enumerate(st):
        t = f(float(days)) * 86400
        L = pref * (td / t) ** (4 / (n - 2)) if t < td else pref * mp.exp(-(t * t / td / td - 1) / 2)
        R = (tph / t) ** (2 / (n - 1)) * vt * t if t < tph else (1 + (delta - 1) / (n - 1) * ((t / tph) ** 2 - 1)) ** (-1 / (delta - 1)) * vt * t
        T = (L / (4 * mp.pi * R * R) / f(lg.sigSB)) ** f(0.25)
        for k, nu in enumerate(nu_host):
            x = min(f(lg.h) * f(float(nu)) / T / f(lg.kb), f(700))
            F = 2 * f(lg.h) / c ** 2 * f(float(nu)) ** 3 / mp.expm1(x) * R * R / f(lg.D) ** 2
            out[k, j] = float(-2.5 * mp.log10(F) - f(48.6))
    return out


def classify(ref, p, z, nu0):
    """The row's classes, or None when a node's reference L is subnormal on one of the grids."""
    td, tph = timescales(ref, p)
    st = GRIDS["g100"][0] * 86400.0
    got = {"td_inside": st[0] <= td <= st[-1], "td_before": td < st[0], "td_after": td > st[-1],
           "tph_inside": st[0] <= tph <= st[-1], "tph_before": tph < st[0], "tph_after": tph > st[-1], "td_gt_tph": td > tph}
    for key, (grid, filters) in GRIDS.items():
        mag, lbol, _ = reference_curves(ref, grid, p, np.array([nu0[f] for f in filters]) * (1 + z), filters)
        if np.any((lbol > 0) & (lbol < np.finfo(np.float64).tiny)):
            return None
        if key == "g100":
            got["L_zero"] = bool(np.any(lbol == 0.0))
            got["some_inf"] = bool(np.any(np.isposinf(mag)) and np.all(np.isfinite(mag).sum(axis=1) >= 2))
        if key == "g3":
            got["all_nan_g3"] = bool(np.all(np.isnan(mag)))
    return {c for c in CLASSES if got[c]}


def reference_likelihood(ref, grid, data):
    ref.utils.get_all_bandpass_metadata = lambda: []
    ref.utils.M4OPT_INSTALLED = False        # the mocked import 'succeeds'; the real package is absent
    m = ref.model.ShockCoolingLightCurveModel("Piro2021", filters=list(FILTERS9))
    m.redshift_func = lambda p: np.interp(p["luminosity_distance"], grid[0], grid[1])
    m.check_vs_priors = lambda priors: None
    if data is None:
        return m, None
    times, mags, sigmas = data
    handler = ref.systematics.FilterSystematicsHandler(list(FILTERS9), error_budget=1.0, light_curve_times=times)
    lik = ref.em_likelihood.EMTransientLikelihood(m, (times, mags, sigmas, 0.0), handler, ref.base.PriorDict({n: object() for n in NAMES}),
                                                  filters=list(FILTERS9), detection_limit=np.inf)
    return m, lik


def main():
    ref = ref_harness.reference_modules()
    rng = np.random.default_rng(SEED)
    grid = syn.flat_lcdm_grid(1.0, 200.0)
    model, _ = reference_likelihood(ref, grid, None)
    assert np.array_equal(model.model_times, GRIDS["g100"][0])
    nu0 = dict(zip(FILTERS9, np.asarray(model.nu_0s, float)))
    out = {"names": np.array(NAMES), "dist_grid": grid[0], "z_grid": grid[1], "filters": np.array(FILTERS9),
           "nu0": np.array([nu0[f] for f in FILTERS9])}

    # ---- rows: PER_CLASS + 1 per class from seeded candidates, then ordinary rows around TRUTH
    rows, members = [], {c: 0 for c in CLASSES}
    for _ in range(20000):
        if all(v > PER_CLASS for v in members.values()):
            break
        p = {k: float(rng.uniform(*BOX[k])) for k in BOX}
        p.update(luminosity_distance=float(rng.uniform(5.0, 150.0)), timeshift=float(rng.uniform(-0.02, 0.1)))
        cls = classify(ref, p, float(np.interp(p["luminosity_distance"], *grid)), nu0)
        if cls and any(members[c] <= PER_CLASS for c in cls):
            rows.append(p)
            for c in cls:
                members[c] += 1
    for _ in range(N_ORDINARY):
        while True:
            p = {k: TRUTH[k] + float(rng.uniform(-0.4, 0.4)) for k in BOX}
            p.update(luminosity_distance=float(rng.uniform(30.0, 55.0)), timeshift=TRUTH["timeshift"] + float(rng.uniform(-0.03, 0.03)))
            cls = classify(ref, p, float(np.interp(p["luminosity_distance"], *grid)), nu0)
            if cls is not None:
                break
        rows.append(p)
        for c in cls:
            members[c] += 1
    print("rows:", len(rows), "classes:", members)
    theta = np.array([[p[n] for n in NAMES] for p in rows])
    z = np.interp(theta[:, 0], *grid)
    out["theta"], out["redshift"] = theta, z

    # ---- curves, bound terms and numpy's own K
    k_numpy = 0.0
    for key, (st, filters) in GRIDS.items():
        nus = np.array([nu0[f] for f in filters])
        curves = np.empty((len(rows), len(filters), len(st)))
        xi, a = np.empty((len(rows), len(st))), np.zeros((len(rows), len(st)))
        for r, p in enumerate(rows):
            curves[r], lbol, Rs = reference_curves(ref, st, p, nus * (1 + z[r]), filters)
            lg = ref.lightcurve_generation
            with np.errstate(all="ignore"):
                T = np.power(lbol / (4 * np.pi * Rs * Rs) / lg.sigSB, 0.25)
                xi[r] = np.where(T > 0, lg.h * (1 + z[r]) / (lg.kb * T), np.inf)
            td, _ = timescales(ref, p)
            late = st * 86400.0 >= td
            a[r, late] = 0.5 * (st[late] * 86400.0 / td) ** 2
            fin = np.isfinite(curves[r])
            if fin.any():
                hp = mp_curves(ref, st, p, nus * (1 + z[r]))
                x = np.minimum(nus[:, None] * xi[r][None, :], 700.0)
                flux = 10.0 ** (-(curves[r] + 48.6) / 2.5)
                with np.errstate(all="ignore"):
                    unit = EPS * (1 + x + a[r][None, :]) * MAG_PER_REL + MAG_PER_REL * 2 * TINY / flux
                k_numpy = max(k_numpy, float(np.max(np.abs(curves[r] - hp)[fin] / unit[fin])))
        out[f"{key}/sample_times"], out[f"{key}/filters"] = st, np.array(filters)
        out[f"{key}/curves"], out[f"{key}/xi"], out[f"{key}/a"] = curves, xi, a
        print(f"{key}: NS={len(st)} M={len(filters)}  NaN curves {int(np.isnan(curves).all(axis=2).sum())}  +inf entries {int(np.isposinf(curves).sum())}"
              f"  K(numpy) so far {k_numpy:.2f}")
    out["k_numpy"] = np.array(k_numpy)

    # ---- photometry around the reference's own detector-frame curves at TRUTH, and log L of every row
    truth = dict(TRUTH)
    obs_times, lc = model.gen_detector_lc(dict(truth))
    times, mags, sigmas = {}, {}, {}
    for k, f in enumerate(FILTERS9):
        n = 5 + k
        times[f] = np.sort(rng.uniform(0.2, 3.0, n))
        mags[f] = np.interp(times[f], obs_times, lc[f]) + 0.1 * rng.standard_normal(n)
        sigmas[f] = np.full(n, 0.1)
        out[f"data/{f}/t"], out[f"data/{f}/m"], out[f"data/{f}/s"] = times[f], mags[f], sigmas[f]
    _, lik = reference_likelihood(ref, grid, (times, mags, sigmas))
    with np.errstate(all="ignore"):
        logl = np.array([lik.log_likelihood(dict(p)) for p in rows])
    floor = -np.finfo(np.float64).max
    out["logl"] = logl
    n_floor = int(np.sum(logl <= floor))
    print(f"log L: {len(logl) - n_floor} finite in ({logl[logl > floor].min():.2f}, {logl[logl > floor].max():.2f}), {n_floor} floored")
    if any(v < 2 for v in members.values()) or len(logl) - n_floor < 8 or n_floor < 2 or not np.isfinite(k_numpy):
        raise SystemExit("refusing to write the golden file: a class holds fewer than two rows, or too few finite / floored log L")
    path = os.path.join(ROOT, "tests", "golden", "piro2021.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
