"""The Gaussian-process surrogate (``interpolation_type="sklearn_gp"``, ``EMEngine(model_kind="svd_gp")``) on the device against
the fp64 numpy restatement of ``gp.predict`` and against tests/golden/gp_bulla.npz (the reference's own sklearn regressors,
tools/make_golden_gp.py).  No sklearn here.

Coefficient bound (derived, not measured): ``2 (N + 8) eps S_i + eps |c_i|`` with ``S_i = sum_n |k_n a_in|`` -- two summations of N
terms in unknown order plus a few ulp per term for the power and the two products, and one rounding of the affine
``y_std (...) + y_mean``.  The sum's error is scaled by ``y_std``: the synthetic rows use ``y_std`` of 1 or 0.5 (an exact scaling,
never above 1), so the bound holds as stated."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_bulla.npz")
_GP = ("gp_X", "gp_alpha", "gp_const", "gp_ell", "gp_rq_alpha", "gp_ymean", "gp_ystd")
_SVD = ("VA", "mins", "maxs", "tt", "param_mins", "param_maxs")

#: (constant, length scale, alpha, y_mean, y_std): the optimiser's bounds are the normal case (alpha = 1e10, alpha = 1e-10, l = 1e-10).
#: With l = 1e-10 AND alpha = 1e10 every k_n underflows to 0 and the coefficient is exactly y_mean; l = 1e-10 with a small alpha does
#: not underflow ((1e19) ** -0.4 = 2.5e-8) and is one more ordinary row.
HYPER = [(1.7, 0.8, 0.3, 0.0, 1.0), (0.9, 1.5, 1e10, 0.0, 1.0), (2.3, 0.6, 1e-10, 0.0, 1.0), (1.1, 1e-10, 1e10, -1.25, 0.5),
         (0.5, 0.3, 2.5, 0.75, 0.5), (1.3, 1e-10, 0.4, 0.25, 1.0)]


def restatement(theta_model, t, n_coeff):
    """(c[B, NC], S[B, NC]) of one filter, in the reference's operation order."""
    x = (theta_model - t["param_mins"]) / (t["param_maxs"] - t["param_mins"])
    d2 = np.zeros((len(x), len(t["gp_X"])))
    for p in range(x.shape[1]):
        d2 = d2 + (x[:, p, None] - t["gp_X"][None, :, p]) ** 2
    c, s = np.empty((len(x), n_coeff)), np.empty((len(x), n_coeff))
    for i in range(n_coeff):
        base = 1.0 + d2 / (2.0 * t["gp_rq_alpha"][i] * t["gp_ell"][i] ** 2)
        terms = (t["gp_const"][i] * base ** (-t["gp_rq_alpha"][i])) * t["gp_alpha"][i][None, :]
        c[:, i] = t["gp_ystd"][i] * terms.sum(axis=1) + t["gp_ymean"][i]
        s[:, i] = np.abs(terms).sum(axis=1)
    return c, s


def synthetic_filter(seed, n, n_p, n_c, first, n_t=5):
    rng = np.random.default_rng(seed)
    hyper = np.array([HYPER[(first + i) % len(HYPER)] for i in range(n_c)])
    return dict(gp_X=rng.uniform(0.0, 1.0, (n, n_p)), gp_alpha=rng.standard_normal((n_c, n)) * 3.0,
                gp_const=hyper[:, 0].copy(), gp_ell=hyper[:, 1].copy(), gp_rq_alpha=hyper[:, 2].copy(), gp_ymean=hyper[:, 3].copy(),
                gp_ystd=hyper[:, 4].copy(), VA=rng.standard_normal((n_t, n_c)), mins=rng.uniform(-20, -10, n_t), maxs=rng.uniform(-5, 0, n_t),
                tt=np.linspace(0.0, 2.0, n_t), param_mins=np.full(n_p, -1.0), param_maxs=np.full(n_p, 2.0), n_coeff=n_c)


def make_engine(svd, n_p):
    from nmma_amd.engine import EMEngine
    names = [f"p{k}" for k in range(n_p)]
    return EMEngine(svd, list(svd), names, names, model_kind="svd_gp")


def check_coefficients(got, theta, svd, n_c):
    for m, t in enumerate(svd.values()):
        want, s = restatement(theta, t, n_c)
        tol = 2.0 * (len(t["gp_X"]) + 8) * EPS * s + EPS * np.abs(want)
        err = np.abs(got[:, m] - want)
        print(f"filter {m}: N = {len(t['gp_X'])}, worst error / bound = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert np.all(err <= tol)
        dead = (s == 0.0).all(axis=0)            # every kernel value underflows: exactly y_mean, not NaN
        assert np.array_equal(dead, (t["gp_ell"][:n_c] == 1e-10) & (t["gp_rq_alpha"][:n_c] == 1e10))
        assert np.array_equal(got[:, m, dead], np.broadcast_to(t["gp_ymean"][:n_c][dead], got[:, m, dead].shape))


# N crosses the sub-lane (4), slot (16) and LDS-chunk (128) edges; every N, NP, NC and B of the issue appears
@pytest.mark.parametrize("n,n_p,n_c,batch,first", [
    (1, 1, 1, 1, 0), (15, 4, 10, 17, 0), (16, 8, 16, 100, 1), (17, 1, 10, 1, 2), (28, 4, 1, 100, 3), (257, 8, 10, 17, 0),
    (257, 4, 16, 100, 2), (16, 1, 1, 17, 4), (28, 8, 16, 1, 1), (1, 4, 10, 100, 3), (15, 8, 1, 1, 1), (17, 4, 16, 17, 4)])
def test_coefficients_match_the_restatement(n, n_p, n_c, batch, first):
    svd = {"f0": synthetic_filter(1000 + n, n, n_p, n_c, first)}
    theta = np.random.default_rng(77 + batch).uniform(-1.2, 2.2, (batch, n_p))
    eng = make_engine(svd, n_p)
    got = eng.coefficients(theta).cpu().numpy()
    eng.close()
    assert got.dtype == np.float64 and got.shape == (batch, 1, n_c)
    check_coefficients(got, theta, svd, n_c)


@pytest.mark.parametrize("sizes,n_p,n_c", [((17, 257), 4, 10), ((28, 1), 8, 16)])
def test_two_filters_with_different_training_sets(sizes, n_p, n_c):
    svd = {f"f{k}": synthetic_filter(2000 + 10 * k + n, n, n_p, n_c, k) for k, n in enumerate(sizes)}
    theta = np.random.default_rng(5).uniform(-1.2, 2.2, (100, n_p))
    eng = make_engine(svd, n_p)
    got = eng.coefficients(theta).cpu().numpy()
    eng.close()
    check_coefficients(got, theta, svd, n_c)


def test_rows_do_not_depend_on_the_batch():
    """Rows of a B = 100 call are bit-identical to the same rows evaluated at B = 1 and B = 17 (other tile neighbours, a
    ragged last tile): coefficients and curves."""
    svd = {f"f{k}": synthetic_filter(3000 + k, n, 4, 10, k) for k, n in enumerate((257, 28))}
    theta = np.random.default_rng(9).uniform(-1.2, 2.2, (100, 4))
    eng = make_engine(svd, 4)
    full_c, full_lc = eng.coefficients(theta).cpu().numpy(), eng.model_lightcurves(theta).cpu().numpy()
    for lo, hi in ((0, 1), (99, 100), (0, 17), (40, 57)):
        assert np.array_equal(eng.coefficients(theta[lo:hi]).cpu().numpy(), full_c[lo:hi])
        assert np.array_equal(eng.model_lightcurves(theta[lo:hi]).cpu().numpy(), full_lc[lo:hi])
    eng.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["filters"] = [str(f) for f in g["filters"]]
    g["names"] = [str(n) for n in g["names"]]
    g["model_parameters"] = [str(n) for n in g["model_parameters"]]
    g["svd"] = {f: dict({k: g[f"{f}/{k}"] for k in _GP + _SVD}, n_coeff=int(g[f"{f}/n_coeff"])) for f in g["filters"]}
    return g


def test_golden_coefficients_and_curves(golden):
    """Coefficients against the stored ``gp.predict`` values with the coefficient bound; source-frame curves against the stored
    ``calc_svd_lc`` output.  At an SVD node t the coefficient bound propagates as ``sum_i |VA_ti| bound_i span_t``, the dot product's
    order adds ``(NC + 4) eps (sum_i |VA_ti c_i| span_t + |mins_t|)``; a sample time is a convex combination of its two bracketing
    nodes (same operations on both sides): the larger of their bounds plus 4 eps of the larger magnitude for the lerp's own roundings."""
    from nmma_amd.engine import EMEngine
    g = golden
    svd, theta, st = g["svd"], g["theta"], g["sample_times"]
    cols = [g["names"].index(n) for n in g["model_parameters"]]
    eng = EMEngine(svd, g["filters"], g["model_parameters"], g["names"], sample_times=st, cosmo_grid=(g["dist_grid"], g["z_grid"]),
                   model_kind="svd_gp")
    got_c, got_lc = eng.coefficients(theta).cpu().numpy(), eng.model_lightcurves(theta).cpu().numpy()
    eng.close()
    assert np.array_equal(np.isinf(got_lc), np.isinf(g["curves"])) and np.isinf(g["curves"]).any() and not np.isnan(got_lc).any()
    for m, f in enumerate(g["filters"]):
        t = svd[f]
        n_c = t["n_coeff"]
        c, s = restatement(theta[:, cols], t, n_c)
        bound = 2.0 * (len(t["gp_X"]) + 8) * EPS * s + EPS * np.abs(g["coeff"][:, m])
        assert np.all(np.abs(got_c[:, m] - g["coeff"][:, m]) <= bound)
        span, va = t["maxs"] - t["mins"], np.abs(t["VA"][:, :n_c])
        node_tol = (bound @ va.T) * span + (n_c + 4) * EPS * ((np.abs(c) @ va.T) * span + np.abs(t["mins"]))          # [B, NT]
        node_mag = np.abs((c @ t["VA"][:, :n_c].T) * span + t["mins"])
        fin = np.isfinite(g["curves"][0, m])
        i = np.clip(np.searchsorted(t["tt"], st[fin], side="right") - 1, 0, len(t["tt"]) - 2)
        tol = np.maximum(node_tol[:, i], node_tol[:, i + 1]) + 4 * EPS * np.maximum(node_mag[:, i], node_mag[:, i + 1])
        err = np.abs(got_lc[:, m][:, fin] - g["curves"][:, m][:, fin])
        print(f"{f}: worst curve error / bound = {np.max(err / tol):.3f}")
        assert np.all(err <= tol)


def test_golden_log_likelihood_through_the_plugin(golden, tmp_path):
    """``SVDLightCurveModel(interpolation_type="sklearn_gp")`` from the flat ``.npz`` + ``EMTransientLikelihood`` against the reference's
    log L, 1e-6 relative (the tool has checked that the coefficient bound moves log L by less than 1e-7 |log L| on every row)."""
    from nmma_amd.em import io as em_io
    from nmma_amd.em.em_likelihood import EMTransientLikelihood
    from nmma_amd.em.model import SVDLightCurveModel
    from nmma_amd.em.systematics import FilterSystematicsHandler
    from tests.helpers import SimplePrior
    g = golden
    path = str(tmp_path / "Bu2019lm_sparse.npz")
    em_io.save_svd_model(path, g["svd"], g["model_parameters"])
    model = SVDLightCurveModel("Bu2019lm_sparse", svd_path=path, interpolation_type="sklearn_gp", filters=g["filters"],
                               sample_times=g["sample_times"], cosmo_grid=(g["dist_grid"], g["z_grid"]))
    times, mags, sigmas = ({f: g[f"data/{f}/{k}"] for f in g["filters"]} for k in "tms")
    handler = FilterSystematicsHandler(g["filters"], systematics_file=None, error_budget=1.0, light_curve_times=times)
    lik = EMTransientLikelihood(model, (times, mags, sigmas, 0.0), handler, {n: SimplePrior(0.0, 1.0) for n in g["names"]},
                                filters=g["filters"])
    got = lik.log_likelihood_batch(g["theta"], g["names"])
    rel = np.abs(got - g["logl"]) / np.maximum(1.0, np.abs(g["logl"]))
    print(f"log L: worst relative difference {rel.max():.3e}")
    assert np.all(rel <= 1e-6)
    assert lik.log_likelihood(dict(zip(g["names"], g["theta"][3]))) == got[3]
    # the other outputs of the engine: per-filter pieces add up to log L; detector-frame curves are the source-frame ones moved by one
    # constant per row (distance modulus and redshift term), +inf where those are
    eng = lik.sub_model.engine(g["names"])
    chi, gp = (x.cpu().numpy() for x in eng.loglike_parts(g["theta"]))
    assert chi.shape == (len(g["filters"]), len(got))
    assert np.allclose(chi.sum(axis=0) + gp.sum(axis=0), got, rtol=1e-12, atol=0.0)
    tobs, mag = (x.cpu().numpy() for x in eng.lightcurves(g["theta"]))
    lc = eng.model_lightcurves(g["theta"]).cpu().numpy()
    fin = np.isfinite(lc)
    assert np.array_equal(np.isfinite(mag), fin) and tobs.shape == (len(got), len(g["sample_times"]))
    shift = np.where(fin, mag - np.where(fin, lc, 0.0), np.nan)
    assert np.nanmax(np.nanmax(shift, axis=(1, 2)) - np.nanmin(shift, axis=(1, 2))) < 1e-11
