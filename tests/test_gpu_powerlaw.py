"""The power-law flux models on the device (kernels ``powerlaw_lc`` / ``powerlaw_logl``, ``EMEngine(model_kind="powerlaw")``,
``PowerLawFluxLightCurveModel``) against tests/golden/powerlaw.npz: the reference's own ``host_lc`` / ``synchrotron_powerlaw`` curves,
``combine_detector_data``, ``MultiFilterTransient`` log L and ``stack_magnitudes`` (tools/make_golden_powerlaw.py).

Curve bound.  Device and host run the same IEEE operations on the same doubles except ``pow`` and ``log10``.  Documented errors: OpenCL's
fp64 ``pow`` <= 16 ulp and ``log10`` <= 3 ulp (what ocml implements), glibc's ``pow`` <= 1 ulp and ``log10`` <= 2 ulp; a correctly rounded
multiply or add is half an ulp on each side.  With eps = 2^-52 >= 1 ulp, ``p = t^(-alpha)``, ``F = A p + C``::

    |d(A p)| <= (16 + 1 + 1) eps |A p|,   |dF| <= 18 eps |A p| + eps |F|,   rel(F) = |dF| / |F|
    |d mag|  <= (2.5 / ln 10) rel(F) + (3 + 2 + 1) eps |2.5 log10 F| + eps |mag|        (the logarithms, the product with -2.5, the sum with r_f)

``|2.5 log10 F| = |mag - r_f|``.  The synchrotron amplitude ``A = F_ref pow(nu, -beta)`` carries 18 eps of its own (36 on ``A p``) and the
subtracted distance modulus ``5 (5 + log10 d_L)`` 5 (3 + 2) eps |log10 d_L| + 2 eps |dmod| + eps |mag|.

log L bound.  An estimate moves by ``dm`` = the curve bound of the row's worst node plus 8 eps |m| (distance modulus, redshift
correction and np.interp's four operations, both sides); a detection's term by ``|x| / sigma dm`` (x = (m - est) / sigma) plus, under a
finite limit, ``(|b| + 1) / sigma dm`` (the inverse Mills ratio of log Phi) and the log Phi table's 4.7e-16; an upper limit's by
``(|x| + 1) / sigma_sys dm``; every term 4 eps (x^2 + |ln sigma| + 1) of its own arithmetic; the sum N eps sum |term|."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MAG_PER_REL = 2.5 / np.log(10.0)
FLOOR = -np.finfo(np.float64).max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "powerlaw.npz")
ROWS_PER_WG = 16
# likelihood cases: grid, observed bands, sampled em_syserr, the path nmma_pl_fused must report
CASES = {"plain": ("g5", "gri", False, True), "syserr": ("g5", "gri", True, True), "avg": ("g5", "grio", False, False),
         "edge": ("g256", "gri", True, True), "long": ("g257", "gri", True, False)}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["filters"] = [str(f) for f in g["filters"]]
    g["sr/names"], g["syn/names"] = [str(n) for n in g["sr/names"]], [str(n) for n in g["syn/names"]]
    g["data"] = tuple({f: g[f"data/{f}/{k}"] for f in "grio"} for k in "tms")
    g["syn/data"] = (g["data"][0], {f: g[f"syn/data/{f}/m"] for f in "gri"}, g["data"][2])
    return g


def make_engine(g, model="sr", key="g5", z_mode="grid", bands=None, sampled_error=False):
    """z_mode "slot": a sampled ``redshift`` column behind the golden ones; "grid": z from the distance grid."""
    from nmma_amd.engine import EMEngine
    names = g[f"{model}/names"] + (["redshift"] if z_mode == "slot" else [])
    kw = {}
    if bands:
        data = g["data"] if model == "sr" else g["syn/data"]
        limit = dict(zip("gri", g["limit" if model == "sr" else "syn/limit"]))
        kw = dict(data=tuple({f: d[f] for f in bands} for d in data), observed_filters=list(bands), detection_limit=limit,
                  sources={f: ["r", "i"] if f == "o" else [f] for f in bands},
                  systematics={"mode": "param", "name": "em_syserr"} if sampled_error else {"mode": "budget", "values": {f: 0.3 for f in bands}})
    if model == "sr":
        spec = dict(model="Sr2023", host_mag=g["host_mag"])
        params = ["alpha_AG"] + [f"a_AG_{f}" for f in g["filters"]] + [f"f_nu_{f}" for f in g["filters"]]
        st = g[f"sr/{key}/sample_times"]
    else:
        spec, params, st = dict(model="synchrotron_powerlaw"), ["alpha_time", "beta_freq", "F_ref"], g["sr/g5/sample_times"]
        kw["filter_nu0"] = dict(zip(g["filters"], g["syn/nu0"]))
    return EMEngine(None, g["filters"], params, names, sample_times=st, cosmo_grid=(g["dist_grid"], g["z_grid"]), model_kind="powerlaw",
                    powerlaw=spec, **kw)


def theta_of(g, model, z_mode):
    return np.column_stack([g[f"{model}/theta"], g[f"{model}/redshift"]]) if z_mode == "slot" else g[f"{model}/theta"]


def in_batches(call, theta, batch):
    """``call`` on every row: alone (batch 1), or as row 0 .. of batches of ``batch`` rows filled up cyclically (one full workgroup + a row)."""
    out = []
    for i in range(0, len(theta), batch):
        idx = (i + np.arange(batch)) % len(theta)
        out.append(call(theta[idx]).cpu().numpy()[:min(batch, len(theta) - i)])
    return np.concatenate(out)


def same_patterns(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isneginf(got).any()


def sr_curve_bound(g, key, want):
    th, st = g["sr/theta"], g[f"sr/{key}/sample_times"]
    ap = th[:, 4:7, None] * (st[None, None, :] ** -th[:, 3, None, None])
    F = ap + th[:, 7:10, None]
    with np.errstate(all="ignore"):
        return MAG_PER_REL * EPS * (18.0 * np.abs(ap) + np.abs(F)) / np.abs(F) + EPS * (6.0 * np.abs(want - g["host_mag"][None, :, None]) + np.abs(want))


def logl_bound(tobs, det, dm, data, bands, limit, err):
    """The docstring's log L bound for ONE row: detector-frame reference curves ``det[M, NS]`` on ``tobs``, estimate error ``dm``."""
    times, mags, sigmas = data
    tol, terms, n = 0.0, 0.0, 0
    for f in bands:
        src = [1, 2] if f == "o" else ["gri".index(f)]
        est = np.mean([np.interp(times[f], tobs[np.isfinite(det[k])], det[k][np.isfinite(det[k])], left=np.inf, right=np.inf) for k in src], axis=0)
        sig = np.sqrt(sigmas[f] ** 2 + err ** 2)
        lim = limit.get(f, np.inf)
        with np.errstate(all="ignore"):
            x = np.where(np.isfinite(sig), (mags[f] - est) / sig, (mags[f] - est) / err)
            x = np.where(np.isfinite(x), x, 0.0)
            scale = np.where(np.isfinite(sig), sig, err)
            mills = (np.abs((lim - est) / sig) + 1.0) if np.isfinite(lim) else 0.0
        tol += np.sum(((np.abs(x) + np.where(np.isfinite(sig), mills, 1.0)) / scale) * dm + 4 * EPS * (x * x + np.abs(np.log(scale)) + 1.0))
        tol += 4.7e-16 * len(x) * np.isfinite(lim)
        terms += np.sum(0.5 * x * x + np.abs(np.log(scale)) + 1.0)
        n += len(x)
    return tol + n * EPS * terms


@pytest.mark.parametrize("batch", [1, ROWS_PER_WG + 1])
@pytest.mark.parametrize("key", ["g5", "g256", "g257"])
def test_sr2023_curves_match_the_reference(golden, key, batch):
    g = golden
    eng = make_engine(g, key=key)
    got = in_batches(eng.model_lightcurves, g["sr/theta"], batch)
    eng.close()
    want = g[f"sr/{key}/curves"]
    assert same_patterns(got, want) and np.isnan(want).any() and np.isposinf(want).any()
    fin, tol = np.isfinite(want), sr_curve_bound(g, key, want)
    print(f"Sr2023 {key} B={batch}: {int(fin.sum())} finite magnitudes, worst error / bound = {np.max(np.abs(got - want)[fin] / tol[fin]):.3f}")
    assert np.all(np.abs(got - want)[fin] <= tol[fin])


@pytest.mark.parametrize("z_mode", ["slot", "grid"])
def test_synchrotron_curves_and_detector_frame_match_the_reference(golden, z_mode):
    g = golden
    eng = make_engine(g, "syn", z_mode=z_mode)
    theta = theta_of(g, "syn", z_mode)
    got = eng.model_lightcurves(theta).cpu().numpy()
    tobs, det = (x.cpu().numpy() for x in eng.lightcurves(theta))
    eng.close()
    want = g["syn/curves"]
    assert same_patterns(got, want) and same_patterns(det, g["syn/detector"]) and np.isnan(want).any()
    dmod = 5.0 * (5.0 + np.log10(g["syn/theta"][:, 0]))[:, None, None]
    fin = np.isfinite(want)
    tol = MAG_PER_REL * EPS * 37.0 + EPS * (6.0 * np.abs(want + dmod - 16.4) + 25.0 * np.abs(np.log10(g["syn/theta"][:, 0]))[:, None, None]
                                            + 2.0 * np.abs(dmod) + 2.0 * np.abs(want))
    print(f"synchrotron z={z_mode}: worst error / bound = {np.max(np.abs(got - want)[fin] / tol[fin]):.3f} (source frame), "
          f"{np.max(np.abs(det - g['syn/detector'])[fin] / (tol + 4 * EPS * np.abs(g['syn/detector']))[fin]):.3f} (detector frame)")
    assert np.all(np.abs(got - want)[fin] <= tol[fin])
    assert np.all(np.abs(det - g["syn/detector"])[fin] <= (tol + 4 * EPS * np.abs(g["syn/detector"]))[fin])
    assert np.all(np.abs(tobs - g["syn/tobs"]) <= 2 * EPS * np.abs(g["syn/tobs"]))


@pytest.mark.parametrize("z_mode", ["slot", "grid"])
@pytest.mark.parametrize("case", list(CASES))
def test_log_likelihood_matches_the_reference_on_both_paths(golden, case, z_mode):
    """The path the handle reports, log L against the reference's within the bound (floor pattern identical), the two-launch form on
    the same handle to the same bound, and every row bit-identical alone and inside a batch of a full workgroup plus one."""
    import torch
    g = golden
    key, bands, sampled, fused = CASES[case]
    eng = make_engine(g, key=key, z_mode=z_mode, bands=bands, sampled_error=sampled)
    assert eng.powerlaw_fused is fused
    theta = theta_of(g, "sr", z_mode)
    alone = in_batches(eng.loglike, torch.as_tensor(theta, device="cuda:0"), 1)
    batched = in_batches(eng.loglike, torch.as_tensor(theta, device="cuda:0"), ROWS_PER_WG + 1)
    th = torch.as_tensor(theta, device="cuda:0")
    two = eng.loglike_lc(th, eng.model_lightcurves(th)).cpu().numpy()
    eng.close()
    assert np.array_equal(alone.view(np.int64), batched.view(np.int64))
    want = g[f"logl/{case}"]
    assert np.array_equal(alone == FLOOR, want == FLOOR) and np.array_equal(two == FLOOR, want == FLOOR) and (want == FLOOR).any()
    # the detector-frame reference curves of the case's grid: combine_detector_data's arithmetic on the golden source-frame curves
    src, z = g[f"sr/{key}/curves"], g["sr/redshift"]
    tobs = g[f"sr/{key}/sample_times"][None, :] * (1 + z[:, None]) + g["sr/theta"][:, 1, None]
    with np.errstate(all="ignore"):
        det = src + (5.0 * (5.0 + np.log10(g["sr/theta"][:, 0])) - 2.5 * np.log10(1 + z))[:, None, None]
        node_tol = np.where(np.isfinite(src), sr_curve_bound(g, key, src), 0.0).max(axis=(1, 2)) + 8 * EPS * np.abs(np.where(np.isfinite(det), det, 0.0)).max(axis=(1, 2))
    limit = dict(zip("gri", g["limit"]))
    worst = 0.0
    for b in np.flatnonzero(want != FLOOR):
        tol = logl_bound(tobs[b], det[b], node_tol[b], g["data"], bands, limit, g["sr/theta"][b, 2] if sampled else 0.3)
        worst = max(worst, abs(alone[b] - want[b]) / tol, abs(two[b] - want[b]) / tol, abs(alone[b] - two[b]) / tol)
    print(f"log L {case} z={z_mode} fused={fused}: worst |difference| / bound = {worst:.3f} (reference, two-launch form)")
    assert worst <= 1.0


@pytest.mark.parametrize("z_mode", ["slot", "grid"])
def test_synchrotron_log_likelihood_is_fused_and_floors_like_the_reference(golden, z_mode):
    import torch
    g = golden
    eng = make_engine(g, "syn", z_mode=z_mode, bands="gri", sampled_error=True)
    th = torch.as_tensor(theta_of(g, "syn", z_mode), device="cuda:0")
    got, two = eng.loglike(th).cpu().numpy(), eng.loglike_lc(th, eng.model_lightcurves(th)).cpu().numpy()
    assert eng.powerlaw_fused is True
    eng.close()
    want = g["logl/syn"]
    assert np.array_equal(got == FLOOR, want == FLOOR) and np.array_equal(two == FLOOR, want == FLOOR) and (want == FLOOR).any()
    limit = dict(zip("gri", g["syn/limit"]))
    ok = want != FLOOR
    dm = 40.0 * EPS * 30.0           # (the synchrotron curve bound at |mag|, |dmod| <= 30: 37 eps of flux, the logarithms and the sums)
    tol = np.array([logl_bound(g["syn/tobs"][b], g["syn/detector"][b], dm, g["syn/data"], "gri", limit, g["syn/theta"][b, 2]) for b in np.flatnonzero(ok)])
    print(f"synchrotron log L z={z_mode}: worst |difference| / bound = {np.max(np.abs(got - want)[ok] / tol):.3f}, vs two launches {np.max(np.abs(got - two)[ok] / tol):.3f}")
    assert np.all(np.abs(got - want)[ok] <= tol) and np.all(np.abs(got - two)[ok] <= tol)


def test_combination_with_an_external_model_matches_stack_magnitudes(golden):
    """``ExternalLightCurveModel`` + ``Sr2023`` through ``CombinedLightCurveModelContainer``: the stacked curves against the reference's
    ``stack_magnitudes`` of the same two sets (the flux sum adds 8 eps |mag| to the curve bound), and the likelihood of the combination
    against ``loglike_lc`` fed with the golden stack, on the rows whose Sr2023 half has a light curve in every filter."""
    import torch
    from nmma_amd.em.em_likelihood import EMTransientLikelihood
    from nmma_amd.em.model import CombinedLightCurveModelContainer, ExternalLightCurveModel, PowerLawFluxLightCurveModel
    from nmma_amd.em.systematics import FilterSystematicsHandler
    from tests.helpers import SimplePrior
    g = golden
    grid, st, names = (g["dist_grid"], g["z_grid"]), g["sr/g5/sample_times"], g["sr/names"]
    sr = PowerLawFluxLightCurveModel("Sr2023", filters=g["filters"], sample_times=st, host_mag=g["host_mag"], cosmo_grid=grid)
    const = ExternalLightCurveModel("const", g["filters"], st, cosmo_grid=grid,
                                    generate_lightcurve_batch=lambda t, p: {f: np.full((len(p["timeshift"]), len(t)), float(g["comb/const"])) for f in g["filters"]})
    both = CombinedLightCurveModelContainer([const, sr], cosmo_grid=grid)
    ext = {"const": torch.full((len(g["sr/theta"]), 3, len(st)), float(g["comb/const"]), dtype=torch.float64)}
    got = both.stacked_lightcurves_abs(torch.as_tensor(g["sr/theta"], device="cuda:0"), names, ext).cpu().numpy()
    want, own = g["comb/stacked"], g["sr/g5/curves"]
    good = ~np.isnan(own).any(axis=(1, 2))          # (rows whose Sr2023 half has a light curve in every filter)
    assert same_patterns(got[good], want[good]) and np.isfinite(want[good]).all()
    tol = sr_curve_bound(g, "g5", own) + 8 * EPS * np.abs(want)
    print(f"combination: worst stacked error / bound = {np.max((np.abs(got - want) / tol)[good]):.3f}")
    assert np.all((np.abs(got - want) <= tol)[good])
    data = tuple({f: d[f] for f in "gri"} for d in g["data"])
    handler = FilterSystematicsHandler(g["filters"], systematics_file=None, error_budget=0.3, light_curve_times=data[0])
    limit = dict(zip("gri", g["limit"]))
    lik = EMTransientLikelihood(both, data + (0.0,), handler, {n: SimplePrior(0.0, 1.0) for n in names if n != "em_syserr"}, filters=g["filters"], detection_limit=limit)
    logl = lik.log_likelihood_batch(g["sr/theta"], names)
    eng = make_engine(g, bands="gri")
    ref = eng.loglike_lc(g["sr/theta"][good], torch.as_tensor(want[good])).cpu().numpy()
    eng.close()
    z = g["sr/redshift"]
    tobs = st[None, :] * (1 + z[:, None]) + g["sr/theta"][:, 1, None]
    det = want + (5.0 * (5.0 + np.log10(g["sr/theta"][:, 0])) - 2.5 * np.log10(1 + z))[:, None, None]
    bound = np.array([logl_bound(tobs[b], det[b], tol[b].max() + 8 * EPS * np.abs(det[b]).max(), g["data"], "gri", limit, 0.3) for b in np.flatnonzero(good)])
    print(f"combination: worst |log L difference| / bound = {np.max(np.abs(logl[good] - ref) / bound):.3f}")
    assert np.all(ref != FLOOR) and np.all(np.abs(logl[good] - ref) <= bound)
