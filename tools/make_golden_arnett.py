#!/usr/bin/env python
"""Golden data for the bolometric Arnett models (``SimpleBolometricLightCurveModel``, kernel ``bol_logl``).

Runs only in the build container (imports the reference under oracle/ref_harness.py; needs mpmath and scipy).  Per grid (2 nodes, the
model's 40, 130 nodes over a shorter span) and model (Arnett, Arnett_modified) it records for every row of ``theta``:

* ``ref``: the reference's own ``arnett_lc`` / ``arnett_modified_lc`` curve (QUADPACK through ``np.vectorize``);
* ``mp``: the closed form ``exp(-2xq)(1 + 2q D(x - q)) - exp(-x^2)(1 - 2q D(q))``, D the Dawson function, in 50-digit mpmath;
* ``coef``: the relative error bound of the kernel's curve per node, ``1e-14 + eps (32 + 8 E + |c|)`` with E the
  mean exponent magnitude under the integrand and c = dlnS / dlnx, each the larger of the two integrals';
* ``k_ref``: the reference's worst ``|ref - mp| / (coef |mp|)`` over everything recorded.

For the likelihood cases (data variant x redshift source x systematic error, CASES below) it records the log L of the reference's
``EMTransientLikelihood`` -> ``BasicEMTransient``, the log L of the same formulas (numpy ``autocomplete_data`` + scipy terms) on the
mpmath curves, and the first-order propagation of the curve bound into log L per row.

The file is written only if at least eight rows have a finite log L in every case and no row makes the reference's ``exp(z^2)``
overflow.  Output: tests/golden/arnett.npz -- ARRAYS ONLY (no pickles, no reference source).
"""
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from nmma_amd import synthetic as syn  # noqa: E402

SEED = 20261126
NAMES = ["tau_m", "log10_mni", "t_0", "timeshift", "redshift", "luminosity_distance", "em_syserr"]
GRIDS = {"g2": np.array([0.005, 20.0]), "g40": np.linspace(0.005, 20.0, 40), "g130": np.linspace(2.5, 9.0, 130)}
MODELS = ("Arnett", "Arnett_modified")
BUDGET = 1e-4
EPS = np.finfo(np.float64).eps
FLOOR = -np.finfo(np.float64).max
TAU_NI, TAU_CO = 8.8, 111.3
# (grid, model, data variant, z source, systematic error): every variant x source x error on the default grid, the other grids once
CASES = [("g40", "Arnett_modified", d, z, s) for d in ("real", "limits", "one", "many") for z in ("column", "grid", "none") for s in ("const", "sampled")]
CASES += [("g2", "Arnett_modified", "real", "column", "const"), ("g130", "Arnett_modified", "real", "column", "const"),
          ("g130", "Arnett", "limits", "grid", "sampled")]


def case_key(case):
    return "/".join(case)


def mp_curve(st, p, model):
    import mpmath as mp
    mp.mp.dps = 50
    f = mp.mpf

    def dawson(v):
        return mp.sqrt(mp.pi) / 2 * mp.exp(-v * v) * mp.erfi(v)

    def S(x, q):
        return mp.exp(-2 * x * q) * (1 + 2 * q * dawson(x - q)) - mp.exp(-x * x) * (1 - 2 * q * dawson(q))

    tau, mni = f(p["tau_m"]), f(10) ** f(p["log10_mni"]) * f(1.988409870698051e33)
    eni, eco = f(3.9e10), f(6.78e9)
    qa, qb = tau / (2 * f(TAU_NI)), tau / (2 * f(TAU_CO))
    out = np.empty(len(st))
    for j, t in enumerate(st):
        x = f(float(t)) / tau
        L = mni * ((eni - eco) * S(x, qa) + eco * S(x, qb))
        if model == "Arnett_modified":
            L *= -mp.expm1(-(f(p["t_0"]) / f(float(t))) ** 2)
        out[j] = float(L)
    return out


def bound_coefficients(st, p):
    """1e-14 + eps (32 + 8 E + |c|) per node: E = int 2z |e| exp(e) / int 2z exp(e) over [0, x], e = z^2 - x^2 - 2qz; c = 2x^2 (exp(-2qx) / S - 1)."""
    from scipy.integrate import quad
    tau = p["tau_m"]
    out = np.empty(len(st))
    for j, t in enumerate(st):
        x, worst = t / tau, 0.0
        for q in (tau / (2 * TAU_NI), tau / (2 * TAU_CO)):
            pts = [v for v in (x - 40.0 / max(x, 1.0), x - 4.0 / max(x, 1.0)) if 0 < v < x]
            den = quad(lambda z: 2 * z * np.exp(z * z - x * x - 2 * q * z), 0, x, points=pts or None, epsabs=0, epsrel=1e-10, limit=200)[0]
            num = quad(lambda z: 2 * z * (x * x - z * z + 2 * q * z) * np.exp(z * z - x * x - 2 * q * z), 0, x, points=pts or None, epsabs=0,
                       epsrel=1e-10, limit=200)[0]
            worst = max(worst, 8 * num / den + abs(2 * x * x * (np.exp(-2 * q * x) / den - 1)))
        out[j] = 1e-14 + EPS * (32 + worst)
    return out


def redshift_of(p, source, grid):
    return {"column": p["redshift"], "grid": float(np.interp(p["luminosity_distance"], *grid)), "none": 0.0}[source]


def numpy_terms(data, tobs, ldet, err):
    """(log L, per-datum |d term / d est|, per-datum |term|, node weights) of the reference's formulas on a detector-frame curve."""
    from scipy.stats import norm
    t, m, unc = data
    x0, x1, xm, xn = tobs[[0, 1, -2, -1]]
    ia = np.clip(np.searchsorted(tobs, t, side="right") - 1, 0, len(tobs) - 2)
    ia = np.where(t < x0, 0, np.where(t > xn, len(tobs) - 2, ia))
    wb = (t - tobs[ia]) / (tobs[ia + 1] - tobs[ia])
    est = np.interp(t, tobs, ldet)
    est = np.where(t < x0, ldet[0] + (ldet[1] - ldet[0]) / (x1 - x0) * (t - x0), est)
    est = np.where(t > xn, ldet[-1] + (ldet[-1] - ldet[-2]) / (xn - xm) * (t - xn), est)
    sigma = np.sqrt(unc ** 2 + err ** 2)
    det = np.isfinite(sigma)
    term, slope = np.empty(len(t)), np.empty(len(t))
    with np.errstate(all="ignore"):
        xs = (m - est) / np.where(det, sigma, err)
        term[det] = norm.logpdf(m[det], est[det], sigma[det])
        slope[det] = np.abs(xs[det]) / sigma[det]
        term[~det] = norm.logsf(m[~det], est[~det], err)
        slope[~det] = np.exp(norm.logpdf(xs[~det]) - norm.logsf(xs[~det])) / err
    slope = np.where(np.isfinite(slope), slope, np.abs(xs) / err)            # (deep in the tail: pdf / sf -> x)
    return term[det].sum() + term[~det].sum(), slope, np.abs(term), (ia, 1 - wb, wb)


def main():
    ref = ref_harness.reference_modules()
    ref.utils.get_all_bandpass_metadata = lambda: []
    ref.utils.M4OPT_INSTALLED = False
    lg = ref.lightcurve_generation
    rng = np.random.default_rng(SEED)
    grid = syn.flat_lcdm_grid(20.0, 2000.0)
    with open(os.path.join(ref_harness.REFERENCE_ROOT, "example_files", "lbol", "ztf23bqun", "23bqun_bbdata.csv")) as fh:
        table = list(csv.DictReader(fh))
    raw = {k: np.array([float(r[k]) for r in table]) for k in ("phase", "Lbb", "Lbb_unc")}
    order = np.argsort(raw["phase"])
    real = tuple(raw[k][order] for k in ("phase", "Lbb", "Lbb_unc"))
    limits = (real[0], real[1], real[2].copy())
    limits[2][[3, 8]] = np.inf
    many = tuple(np.concatenate([a + (0.13 * k if i == 0 else 0.0) for k in range(7)])[:70] for i, a in enumerate(real))
    srt = np.argsort(many[0], kind="stable")
    datasets = {"real": real, "limits": limits, "one": tuple(a[5:6] for a in real), "many": tuple(a[srt] for a in many)}

    rows = []
    for i in range(20):
        p = dict(tau_m=rng.uniform(1, 5), log10_mni=rng.uniform(-4, 0), t_0=rng.uniform(1, 10), timeshift=rng.uniform(-8, -2), redshift=0.0,
                 luminosity_distance=rng.uniform(50, 1500), em_syserr=rng.uniform(1e39, 2e40))
        if i >= 16:
            p["tau_m"] = 0.8
        if i % 5 == 2:
            p["redshift"] = float(rng.uniform(0.01, 0.3))
        rows.append({k: float(v) for k, v in p.items()})
    # rows near the data: the fit region, where log L is of order the number of epochs
    for i in range(4):
        rows[i].update(tau_m=7.0 + 0.5 * i, log10_mni=-1.1 + 0.05 * i, t_0=6.0 + i, timeshift=-6.0 + 0.5 * i)
    theta = np.array([[p[n] for n in NAMES] for p in rows])
    if np.any((GRIDS["g40"][-1] / theta[:, 0]) ** 2 > 709):
        raise SystemExit("refusing to write: a row makes the reference's exp(z^2) overflow")
    out = {"names": np.array(NAMES), "theta": theta, "dist_grid": grid[0], "z_grid": grid[1], "budget": np.array(BUDGET)}
    for name, d in datasets.items():
        out[f"data/{name}/t"], out[f"data/{name}/v"], out[f"data/{name}/s"] = d

    # ---- curves, bound coefficients, the reference's own error in units of the bound
    curves, k_ref = {}, 0.0
    for gkey, st in GRIDS.items():
        out[f"{gkey}/sample_times"] = st
        coef = np.array([bound_coefficients(st, p) for p in rows])
        out[f"{gkey}/coef"] = coef
        for model in MODELS:
            fn = lg.arnett_lc if model == "Arnett" else lg.arnett_modified_lc
            refc = np.array([fn(st, dict(p)) for p in rows])
            mpc = np.array([mp_curve(st, p, model) for p in rows])
            curves[gkey, model] = (refc, mpc)
            out[f"{gkey}/{model}/ref"], out[f"{gkey}/{model}/mp"] = refc, mpc
            k = float(np.max(np.abs(refc - mpc) / (coef * np.abs(mpc))))
            k_ref = max(k_ref, k)
            print(f"{gkey} {model}: reference vs mpmath worst {np.max(np.abs(refc / mpc - 1)):.2e} relative = {k:.2f} bounds; coef in "
                  f"({coef.min():.2e}, {coef.max():.2e})")
    out["k_ref"] = np.array(k_ref)

    # ---- log L per case
    for case in CASES:
        gkey, model, dkey, zsrc, sys_mode = case
        st, data = GRIDS[gkey], datasets[dkey]
        m = ref.model.SimpleBolometricLightCurveModel(model, sample_times=st)
        m.check_vs_priors = lambda priors: None
        m.redshift_func = lambda p, zsrc=zsrc: redshift_of(p, zsrc, grid)
        handler = ref.systematics.SystematicsHandler(None, BUDGET, data[0])
        priors = ref.base.PriorDict({n: object() for n in NAMES if n != "em_syserr" or sys_mode == "sampled"})
        lik = ref.em_likelihood.EMTransientLikelihood(m, data + (0.0,), handler, priors)
        assert type(lik.sub_model).__name__ == "BasicEMTransient"
        refc, mpc = curves[gkey, model]
        coef = out[f"{gkey}/coef"]
        logl_ref, logl_mp, tol = np.empty(len(rows)), np.empty(len(rows)), np.empty(len(rows))
        for r, p in enumerate(rows):
            with np.errstate(all="ignore"):
                logl_ref[r] = lik.log_likelihood(dict(p))
            z = redshift_of(p, zsrc, grid)
            err = p["em_syserr"] if sys_mode == "sampled" else BUDGET
            tobs, ldet = st * (1 + z) + p["timeshift"], mpc[r] / (1 + z) ** 2
            total, slope, mag, (ia, wa, wb) = numpy_terms(data, tobs, ldet, err)
            logl_mp[r] = total if np.isfinite(total) else FLOOR
            spread = np.abs(wa) * np.abs(ldet[ia]) * coef[r, ia] + np.abs(wb) * np.abs(ldet[ia + 1]) * coef[r, ia + 1]
            tol[r] = float(np.sum(slope * spread) + 8 * EPS * np.sum(np.maximum(mag, 1.0)))
        key = case_key(case)
        out[f"{key}/logl_ref"], out[f"{key}/logl_mp"], out[f"{key}/tol"] = logl_ref, logl_mp, tol
        finite = logl_mp > FLOOR
        print(f"{key}: {int(finite.sum())} finite log L in ({logl_mp[finite].min():.3e}, {logl_mp[finite].max():.3e}); reference differs by "
              f"{np.max(np.abs(logl_ref - logl_mp)[finite] / tol[finite]):.2f} tolerances at worst")
        if finite.sum() < 8 or not np.array_equal(finite, logl_ref > FLOOR):
            raise SystemExit(f"refusing to write: {key} has fewer than eight finite rows, or the reference floors other rows")
    out["cases"] = np.array([case_key(c) for c in CASES])
    path = os.path.join(ROOT, "tests", "golden", "arnett.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; k_ref =", k_ref)


if __name__ == "__main__":
    main()
