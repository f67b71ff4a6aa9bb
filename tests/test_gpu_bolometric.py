"""The bolometric path on the device (kernel ``bol_logl``, ``BolometricEngine``, ``SimpleBolometricLightCurveModel``,
``BasicEMTransient``) against tests/golden/arnett.npz (tools/make_golden_arnett.py): 50-digit mpmath curves of the closed form, the
reference's own QUADPACK curves and its ``EMTransientLikelihood`` log L.

Curve bound per node: ``coef |L|`` with ``coef = 1e-14 + eps (32 + 8 E + |c|)``, stored by the tool; against the
reference the reference's own error, ``k_ref`` bounds, is added.  log L: the first-order propagation of that bound through the
interpolation and the terms plus 8 eps per datum, stored per row (``tol``).  Worst measured ratios (MI355X): curves 0.059 of the bound
against mpmath, 0.869 of (1 + k_ref) bounds against the reference; log L 0.184 of the tolerance against mpmath, 0.268 against the reference."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FLOOR = -np.finfo(np.float64).max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arnett.npz")
CASES = [("g40", "Arnett_modified", d, z, s) for d in ("real", "limits", "one", "many") for z in ("column", "grid", "none") for s in ("const", "sampled")]
CASES += [("g2", "Arnett_modified", "real", "column", "const"), ("g130", "Arnett_modified", "real", "column", "const"),
          ("g130", "Arnett", "limits", "grid", "sampled")]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["names"] = [str(n) for n in g["names"]]
    return g


def make_engine(g, gkey, model, dkey=None, zsrc="column", sys_mode="const"):
    """Columns the case does not use are renamed, so the engine takes z from the next source and the constant error budget."""
    from nmma_amd.engine import BolometricEngine
    hide = {"column": (), "grid": ("redshift",), "none": ("redshift", "luminosity_distance")}[zsrc] + (("em_syserr",) if sys_mode == "const" else ())
    names = ["unused_" + n if n in hide else n for n in g["names"]]
    data = tuple(g[f"data/{dkey}/{k}"] for k in "tvs") if dkey else None
    return BolometricEngine(model, names, g[f"{gkey}/sample_times"], data=data, cosmo_grid=(g["dist_grid"], g["z_grid"]),
                            error_budget=float(g["budget"]))


def in_batches(call, theta, batch):
    return np.concatenate([call(theta[i:i + batch]) for i in range(0, len(theta), batch)])


@pytest.mark.parametrize("against", ["mp", "ref"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("gkey", ["g2", "g40", "g130"])          # the minimum; one chunk; two chunk carries and a partial chunk
@pytest.mark.parametrize("model", ["Arnett", "Arnett_modified"])
def test_curves(golden, model, gkey, batch, against):
    g = golden
    eng = make_engine(g, gkey, model)
    got = in_batches(eng.model_lightcurves, g["theta"], batch)
    eng.close()
    bound = g[f"{gkey}/coef"] * np.abs(g[f"{gkey}/{model}/mp"]) * (1.0 + (float(g["k_ref"]) if against == "ref" else 0.0))
    ratio = np.abs(got - g[f"{gkey}/{model}/{against}"]) / bound
    print(f"{model} {gkey} B={batch} vs {against}: worst error / bound = {ratio.max():.3f}")
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("against", ["mp", "ref"])
@pytest.mark.parametrize("case", CASES, ids="/".join)
def test_log_likelihood(golden, case, against):
    g, key = golden, "/".join(case)
    eng = make_engine(g, *case)
    got = eng.loglike(g["theta"])
    eng.close()
    want = g[f"{key}/logl_{against}"]
    tol = g[f"{key}/tol"] * (1.0 + (float(g["k_ref"]) if against == "ref" else 0.0))
    fin = want > FLOOR
    print(f"{key} vs {against}: worst error / tolerance = {np.max(np.abs(got - want)[fin] / tol[fin]):.3f}")
    assert np.array_equal(got > FLOOR, fin) and np.all(np.abs(got - want)[fin] <= tol[fin])


def numpy_log_likelihood(t, m, unc, tobs, ldet, err):
    """utils.autocomplete_data (extrapolate="linear") and BasicEMTransient's terms; (log L, sum of |term|)."""
    from scipy.stats import norm
    mask = np.isfinite(ldet)
    if mask.sum() < 2:
        return FLOOR, 0.0
    x, y = tobs[mask], ldet[mask]
    est = np.interp(t, x, y)
    lo, hi = t < x[0], t > x[-1]
    est[lo] = y[0] + (y[1] - y[0]) / (x[1] - x[0]) * (t[lo] - x[0])
    est[hi] = y[-1] + (y[-1] - y[-2]) / (x[-1] - x[-2]) * (t[hi] - x[-1])
    sigma = np.sqrt(unc ** 2 + err ** 2)
    det = np.isfinite(sigma)
    terms = np.concatenate([norm.logpdf(m[det], est[det], sigma[det]), norm.logsf(m[~det], est[~det], err)])
    return terms.sum(), np.abs(terms).sum()


def test_supplied_curves(golden):
    """NaN / inf at interior and edge nodes, a row left with two finite nodes and one left with one (floored)."""
    g = golden
    lbol = g["g40/Arnett_modified/mp"][:6].copy()
    lbol[0, [5, 17, 18]] = np.nan
    lbol[1, [0, 39]] = np.nan, np.inf
    lbol[2, :2] = np.nan
    lbol[3, 1:] = np.nan
    lbol[5, 3:38] = -np.inf
    theta, st = g["theta"][:6], g["g40/sample_times"]
    eng = make_engine(g, "g40", None, "limits", "column", "sampled")
    got = eng.loglike_lc(theta, lbol)
    eng.close()
    assert got[3] == FLOOR and np.all(got[[0, 1, 2, 4, 5]] > FLOOR)
    data = tuple(g[f"data/limits/{k}"] for k in "tvs")
    for r, th in enumerate(theta):
        p = dict(zip(g["names"], th))
        want, mag = numpy_log_likelihood(*data, st * (1 + p["redshift"]) + p["timeshift"], lbol[r] / (1 + p["redshift"]) ** 2, p["em_syserr"])
        assert abs(got[r] - want) <= 8 * EPS * max(mag, 1.0), (r, got[r], want)


def test_rows_do_not_depend_on_the_batch(golden):
    g = golden
    theta = g["theta"]
    eng = make_engine(g, "g130", "Arnett_modified", "many", "grid", "sampled")
    idx = [3, 17, 0, 12, 9, 16, 5, 19, 8]
    batch = eng.loglike(theta[idx]).view(np.int64), eng.model_lightcurves(theta[idx]).view(np.int64)
    alone = in_batches(eng.loglike, theta[idx], 1).view(np.int64), in_batches(eng.model_lightcurves, theta[idx], 1).view(np.int64)
    eng.close()
    assert np.array_equal(batch[0], alone[0]) and np.array_equal(batch[1], alone[1])


def test_public_surface(golden):
    from nmma_amd.em.em_likelihood import EMTransientLikelihood
    from nmma_amd.em.model import SimpleBolometricLightCurveModel
    from nmma_amd.em.systematics import SystematicsHandler
    from tests.helpers import SimplePrior
    g, key = golden, "g40/Arnett_modified/real/column/const"
    names = g["names"][:5]
    data = tuple(g[f"data/real/{k}"] for k in "tvs") + (0.0,)
    lik = EMTransientLikelihood(SimpleBolometricLightCurveModel("Arnett_modified"), data,
                                SystematicsHandler(None, float(g["budget"]), data[0]), {n: SimplePrior(0.0, 1.0) for n in names})
    theta = g["theta"][:, :5]
    got = lik.log_likelihood_batch(theta)
    assert lik.parameter_names() == names and np.all(np.abs(got - g[f"{key}/logl_mp"]) <= g[f"{key}/tol"])
    row = 2                                                                  # (a row with a non-zero redshift)
    p = dict(zip(names, theta[row]))
    assert lik.log_likelihood(p) == got[row]
    tobs, lbol = lik.sub_model.light_curve_model.gen_detector_lc(p)
    want = g["g40/Arnett_modified/mp"][row] / (1 + p["redshift"]) ** 2
    assert p["redshift"] > 0 and np.array_equal(tobs, g["g40/sample_times"] * (1 + p["redshift"]) + p["timeshift"])
    assert np.all(np.abs(lbol - want) <= g["g40/coef"][row] * np.abs(want))
