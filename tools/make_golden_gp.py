#!/usr/bin/env python
"""Golden data for the Gaussian-process surrogate (``interpolation_type="sklearn_gp"``), from the reference's own code with REAL
``GaussianProcessRegressor`` objects.

Runs only in the build container (imports the reference under oracle/ref_harness.py; needs scikit-learn).  Steps:

1. the SVD model of the 28 POSSIS curves of ``nmma/tests/data/bulla`` as ``tools/make_golden_bulla.py`` builds it (the reference's
   readers, ``interpolate_data`` and ``generate_svd_model``);
2. ``SklearnGPTrainingModel.training_func`` (nmma/em/training.py:429-453) trains N_COEFF regressors per filter on its ``cAmat``;
3. ``nmma_amd.em.io.extract_gp_arrays`` takes the plain arrays out of them; the five-line fp64 restatement of ``gp.predict`` is
   checked against ``gp.predict`` for every stored row;
4. photometry is drawn around the model's own curves at one parameter point; for a seeded set of theta rows the reference's
   ``calc_svd_lc`` (source-frame curves) and its ``EMTransientLikelihood.log_likelihood`` are recorded;
5. for every row the coefficient bound of the device tests -- ``2 (N + 8) eps S_i + eps |c_i|`` -- is pushed through the
   reference's likelihood (all coefficients shifted by + and by - the bound): the file is written only if that moves log L by
   less than 1e-7 |log L| on every row, so that the 1e-6 parity of log L is a fair condition.

Output: tests/golden/gp_bulla.npz -- ARRAYS ONLY (no pickles, no reference source).
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from nmma_amd import synthetic as syn  # noqa: E402
from nmma_amd.em import io as em_io  # noqa: E402
from tools.make_golden_bulla import FILTERS, N_COEFF, reference_svd_model  # noqa: E402

SEED, N_ROWS = 20261126, 32
NAMES = ["luminosity_distance", "timeshift", "log10_mej_dyn", "log10_mej_wind"]
TRUTH = dict(luminosity_distance=40.0, timeshift=0.1, log10_mej_dyn=-2.2, log10_mej_wind=-1.3)
SAMPLE_TIMES = np.arange(0.1, 23.0, 0.5)        # the last nodes lie beyond the training grid (21 d): +inf there
EPS = np.finfo(np.float64).eps


def gp_restatement(x, t, n_coeff):
    """``(c[NC], S[NC])``: the coefficients of one filter at the normalised input ``x`` in the reference's operation order, and
    ``S_i = sum_n |k_n a_in|``."""
    d2 = np.zeros(len(t["gp_X"]))
    for p in range(len(x)):
        d2 = d2 + (x[p] - t["gp_X"][:, p]) ** 2
    c, s = np.empty(n_coeff), np.empty(n_coeff)
    for i in range(n_coeff):
        base = 1.0 + d2 / (2.0 * t["gp_rq_alpha"][i] * t["gp_ell"][i] ** 2)
        terms = (t["gp_const"][i] * base ** (-t["gp_rq_alpha"][i])) * t["gp_alpha"][i]
        c[i] = t["gp_ystd"][i] * np.sum(terms) + t["gp_ymean"][i]
        s[i] = np.sum(np.abs(terms))
    return c, s


class _ShiftedGP:
    """A regressor whose prediction is moved by a constant (the bound's propagation through the reference's likelihood)."""

    def __init__(self, gp, shift):
        self.gp, self.shift = gp, shift

    def predict(self, x, return_std=False):
        y = self.gp.predict(x) + self.shift
        return (y, None) if return_std else y


def reference_objects(svd_ref, parameters, grid, data):
    ref = ref_harness.reference_modules()
    ref.utils.get_all_bandpass_metadata = lambda: [{"name": n} for n in FILTERS]
    m = object.__new__(ref.model.SVDLightCurveModel)
    m.model, m.model_parameters, m.filters = "Bu2019lm_sparse", list(parameters), list(FILTERS)
    m.svd_mag_model, m.mag_ncoeff, m.lbol_ncoeff, m.good_parameters = svd_ref, None, None, True
    m.default_filts = list(FILTERS)
    m.lambdas = m.nu_0s = np.ones(len(FILTERS))
    m.model_times = SAMPLE_TIMES
    m.redshift_func = lambda p: np.interp(p["luminosity_distance"], grid[0], grid[1])
    m.check_vs_priors = lambda priors: None
    if data is None:
        return ref, m, None
    times, mags, sigmas = data
    handler = ref.systematics.FilterSystematicsHandler(list(FILTERS), systematics_file=None, error_budget=1.0, light_curve_times=times)
    lik = ref.em_likelihood.EMTransientLikelihood(m, (times, mags, sigmas, 0.0), handler, ref.base.PriorDict({n: object() for n in NAMES}),
                                                  filters=list(FILTERS), detection_limit={f: np.inf for f in FILTERS})
    return ref, m, lik


def main():
    parameters, svd = reference_svd_model()
    tr = importlib.import_module("nmma.em.training")
    trainer = object.__new__(tr.SklearnGPTrainingModel)
    trainer.n_coeff, trainer.ncpus, trainer.svd_model = N_COEFF, 1, svd
    out = {"filters": np.array(FILTERS), "model_parameters": np.array(parameters), "names": np.array(NAMES), "sample_times": SAMPLE_TIMES}
    svd_ref, flat = {}, {}
    for f in FILTERS:
        m = svd[f]
        tr.SklearnGPTrainingModel.training_func(trainer, np.asarray(m["param_array_postprocess"], float), m["cAmat"], f)
        t = em_io.extract_gp_arrays(m["gps"], where=f)
        t.update(VA=np.ascontiguousarray(m["VA"][:, :N_COEFF]), n_coeff=N_COEFF,
                 **{k: np.asarray(m[k], float) for k in ("mins", "maxs", "tt", "param_mins", "param_maxs")})
        flat[f] = t
        svd_ref[f] = dict(VA=m["VA"], n_coeff=N_COEFF, gps=m["gps"], **{k: m[k] for k in ("mins", "maxs", "tt", "param_mins", "param_maxs")})
        print(f"{f:8s} l [{t['gp_ell'].min():.3g}, {t['gp_ell'].max():.3g}]  alpha [{t['gp_rq_alpha'].min():.3g}, {t['gp_rq_alpha'].max():.3g}]  "
              f"|alpha_| max {np.abs(t['gp_alpha']).max():.3g}")
        for k, v in t.items():
            out[f"{f}/{k}"] = np.asarray(v)

    grid = syn.flat_lcdm_grid(1.0, 200.0)
    out["dist_grid"], out["z_grid"] = grid
    rng = np.random.default_rng(SEED)
    ref, model, _ = reference_objects(svd_ref, parameters, grid, None)

    # photometry around the model's own curves at TRUTH
    truth = dict(TRUTH)
    truth["redshift"] = float(np.interp(truth["luminosity_distance"], grid[0], grid[1]))
    obs_times, lc = model.gen_detector_lc(dict(truth))
    times, mags, sigmas = {}, {}, {}
    for k, f in enumerate(FILTERS):
        n = 6 + 2 * k
        times[f] = np.sort(rng.uniform(0.8, 16.0, n))
        mags[f] = np.interp(times[f], obs_times, lc[f]) + 0.15 * rng.standard_normal(n)
        sigmas[f] = np.full(n, 0.15)
        out[f"data/{f}/t"], out[f"data/{f}/m"], out[f"data/{f}/s"] = times[f], mags[f], sigmas[f]
    ref, model, lik = reference_objects(svd_ref, parameters, grid, (times, mags, sigmas))

    # theta rows: away from the best fit (there the terms cancel and the bound's propagation is no longer small against log L)
    pmin, pmax = flat[FILTERS[0]]["param_mins"], flat[FILTERS[0]]["param_maxs"]
    theta = np.empty((N_ROWS, len(NAMES)))
    theta[:, 0] = rng.uniform(25.0, 70.0, N_ROWS)
    theta[:, 1] = rng.uniform(-0.4, 0.4, N_ROWS)
    for k, n in enumerate(parameters):
        theta[:, NAMES.index(n)] = rng.uniform(pmin[k], pmax[k], N_ROWS)
    theta[-4:, NAMES.index(parameters[0])] += 0.3 * (pmax[0] - pmin[0])       # four rows extrapolate
    out["theta"] = theta

    coeff = np.empty((N_ROWS, len(FILTERS), N_COEFF))
    bound = np.empty_like(coeff)
    curves = np.empty((N_ROWS, len(FILTERS), len(SAMPLE_TIMES)))
    logl = np.empty(N_ROWS)
    worst_restatement, worst_prop = 0.0, 0.0
    for r, row in enumerate(theta):
        p = dict(zip(NAMES, (float(v) for v in row)))
        plist = [p[n] for n in parameters]
        for k, f in enumerate(FILTERS):
            x = (np.array(plist) - flat[f]["param_mins"]) / (flat[f]["param_maxs"] - flat[f]["param_mins"])
            c, s = gp_restatement(x, flat[f], N_COEFF)
            coeff[r, k] = [svd_ref[f]["gps"][i].predict(np.atleast_2d(x)).item() for i in range(N_COEFF)]
            bound[r, k] = 2.0 * (len(flat[f]["gp_X"]) + 8) * EPS * s + EPS * np.abs(coeff[r, k])
            worst_restatement = max(worst_restatement, float(np.max(np.abs(c - coeff[r, k]) / bound[r, k])))
        mab = ref.lightcurve_generation.calc_svd_lc(SAMPLE_TIMES, plist, svd_ref, mag_ncoeff=None, filters=list(FILTERS))
        curves[r] = [mab[f] for f in FILTERS]
        logl[r] = lik.log_likelihood(dict(p))
        moved = 0.0
        for sign in (1.0, -1.0):
            for k, f in enumerate(FILTERS):
                svd_ref[f]["gps"] = [_ShiftedGP(g, sign * bound[r, k, i]) for i, g in enumerate(svd[f]["gps"])]
            moved = max(moved, abs(lik.log_likelihood(dict(p)) - logl[r]))
            for f in FILTERS:
                svd_ref[f]["gps"] = svd[f]["gps"]
        worst_prop = max(worst_prop, moved / abs(logl[r]))
        print(f"row {r:2d} logL {logl[r]:14.6f}  bound moves it by {moved:.3e} ({moved / abs(logl[r]):.2e} relative)")
    print(f"restatement vs gp.predict: worst |difference| / bound = {worst_restatement:.3f}")
    print(f"largest propagated bound on log L: {worst_prop:.3e} relative")
    if not np.all(np.isfinite(logl)) or worst_restatement > 1.0 or worst_prop >= 1e-7:
        raise SystemExit("refusing to write the golden file: a row breaks the conditions above (draw theta further from the best fit)")
    out.update(coeff=coeff, curves=curves, logl=logl)
    path = os.path.join(ROOT, "tests", "golden", "gp_bulla.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
