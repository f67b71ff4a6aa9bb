"""The HoNa2020 kilonova on the device (kernel ``hona2020_lc``, ``EMEngine(model_kind="hona2020")``,
``SimpleKilonovaLightCurveModel("HoNa2020")``) against tests/golden/hona2020.npz: the reference's own ``HoNa_lc`` curves, scipy's
step counts and the reference's ``EMTransientLikelihood`` log L (tools/make_golden_hona2020.py).

Curve bound: ``4 k_numpy (S_row + eps (1 + x) 2.5 / ln 10)``.  S_row is the largest change of any magnitude of the row under the twelve
one-ulp nudges of its six parameters -- the reference's own conditioning through the adaptive integration and the spline -- and the second
term is the per-node floor of the Piro2021 bound (``x = min(h nu / (kb T), 700)``, the amplification by ``expm1``).  ``k_numpy`` = 1.607
is what a plain-loop numpy restatement in the kernel's summation order reaches against the reference in those units; the kernel gets
four times that (DESIGN.md section 3.3b's convention): its libm and reduction order are ulp-level perturbations of the kind the nudges
measure.  Rows on an accept / reject tie of the step controller are not in the file."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MAG_PER_REL = 2.5 / np.log(10.0)
FLOOR = -np.finfo(np.float64).max
WAVES = 4           # rows per workgroup of hona2020_lc
PARAMS = ["log10_mej", "vej_max", "vej_min", "vej_frac", "log10_kappa_low_vej", "log10_kappa_high_vej"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hona2020.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["names"], g["filters"] = [str(n) for n in g["names"]], [str(f) for f in g["filters"]]
    g["data"] = tuple({f: g[f"data/{f}/{k}"] for f in g["filters"]} for k in "tms")
    return g


def make_engine(g, key, z_mode="grid", with_data=False):
    """z_mode "slot": a sampled ``redshift`` column behind the golden ones; "grid": z from the distance grid."""
    from nmma_amd.engine import EMEngine
    filters = [str(f) for f in g[f"{key}/filters"]]
    kw = dict(data=g["data"], observed_filters=filters) if with_data else {}
    return EMEngine(None, filters, PARAMS, g["names"] + (["redshift"] if z_mode == "slot" else []), sample_times=g[f"{key}/sample_times"],
                    cosmo_grid=(g["dist_grid"], g["z_grid"]), model_kind="hona2020", filter_nu0=dict(zip(g["filters"], g["nu0"])), **kw)


def curves_in_batches(eng, theta, batch):
    return np.concatenate([eng.model_lightcurves(theta[i:i + batch]).cpu().numpy() for i in range(0, len(theta), batch)])


def check_logl(got, want):
    assert np.array_equal(got == FLOOR, want == FLOOR) and (want == FLOOR).any() and not (want == FLOOR).all()
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"log L: worst relative difference {rel[want != FLOOR].max():.3e}")
    assert np.all(rel[want != FLOOR] <= 1e-6)


@pytest.mark.parametrize("z_mode", ["slot", "grid"])
@pytest.mark.parametrize("batch", [1, WAVES + 1])
@pytest.mark.parametrize("key", ["g3", "g65", "g150"])          # (NS, M) = (3, 1), (65, 3), (150, 9)
def test_curves_match_the_reference(golden, key, batch, z_mode):
    g = golden
    theta = np.column_stack([g["theta"], g["redshift"]]) if z_mode == "slot" else g["theta"]
    eng = make_engine(g, key, z_mode)
    got = curves_in_batches(eng, theta, batch)
    eng.close()
    want = g[f"{key}/curves"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isneginf(got).any()
    nus = np.array([g["nu0"][g["filters"].index(str(f))] for f in g[f"{key}/filters"]])
    x = np.minimum(nus[None, :, None] * g[f"{key}/xi"][:, None, :], 700.0)
    tol = 4.0 * float(g["k_numpy"]) * (g[f"{key}/S"][:, None, None] + EPS * (1.0 + x) * MAG_PER_REL)
    fin = np.isfinite(want)
    err = np.abs(got - want)
    print(f"{key} B={batch} z={z_mode}: {int(fin.sum())} finite magnitudes, worst error / bound = {np.max(err[fin] / tol[fin]):.3f}")
    assert fin.all() and np.all(err <= tol)


@pytest.mark.parametrize("key", ["g3", "g65", "g150"])
def test_steps_equal_scipys(golden, key):
    """Accepted and rejected steps of every row: off by one rule of solve_ivp's controller and these differ."""
    eng = make_engine(golden, key)
    got = eng.hona_steps(golden["theta"]).cpu().numpy()
    eng.close()
    assert np.array_equal(got, golden[f"{key}/steps"])


def test_rows_do_not_depend_on_the_batch(golden):
    """Alone, in batches of one workgroup + 1, and scattered over a batch of 203 (other neighbours, a ragged last workgroup): the same bits."""
    theta = golden["theta"]
    eng = make_engine(golden, "g150")
    alone = curves_in_batches(eng, theta, 1).view(np.int64)
    idx = (np.arange(203) * 7 + 3) % len(theta)
    big = eng.model_lightcurves(theta[idx]).cpu().numpy().view(np.int64)
    groups = curves_in_batches(eng, theta, WAVES + 1).view(np.int64)
    eng.close()
    assert np.array_equal(groups, alone) and np.array_equal(big, alone[idx])


def test_log_likelihood_matches_the_reference_and_the_curves_path(golden):
    """log L against the reference's (1e-6 relative, floored rows floor); the same handle's ``loglike_lc`` fed with its own
    ``model_lightcurves`` gives the same bits."""
    import torch
    g = golden
    eng = make_engine(g, "g150", with_data=True)
    theta = torch.as_tensor(g["theta"], device="cuda:0")
    got = eng.loglike(theta)
    via_curves = eng.loglike_lc(theta, eng.model_lightcurves(theta))
    eng.close()
    check_logl(got.cpu().numpy(), g["logl"])
    assert np.array_equal(got.cpu().numpy().view(np.int64), via_curves.cpu().numpy().view(np.int64))


def test_factory_likelihood_and_combination(golden):
    """``create_light_curve_model_from_args(..., device_models=("HoNa2020",))`` + ``EMTransientLikelihood`` give the reference's log L;
    combined with a constant-curve ``ExternalLightCurveModel`` on the same grid the likelihood equals ``EMEngine.stack`` of the two sets
    pushed through ``loglike_lc``."""
    import torch
    from nmma_amd.em.em_likelihood import EMTransientLikelihood
    from nmma_amd.em.model import (CombinedLightCurveModelContainer, ExternalLightCurveModel, SimpleKilonovaLightCurveModel,
                                   create_light_curve_model_from_args)
    from nmma_amd.em.systematics import FilterSystematicsHandler
    from tests.helpers import SimplePrior
    g = golden
    grid = (g["dist_grid"], g["z_grid"])
    priors = {n: SimplePrior(0.0, 1.0) for n in g["names"]}

    def likelihood(model):
        handler = FilterSystematicsHandler(g["filters"], systematics_file=None, error_budget=1.0, light_curve_times=g["data"][0])
        return EMTransientLikelihood(model, g["data"] + (0.0,), handler, priors, filters=g["filters"])

    model = create_light_curve_model_from_args("HoNa2020", SimpleNamespace(), filters=g["filters"], device_models=("HoNa2020",))
    assert isinstance(model, SimpleKilonovaLightCurveModel) and np.array_equal(model.model_times, g["g150/sample_times"])
    model.cosmo_grid = grid
    got = likelihood(model).log_likelihood_batch(g["theta"], g["names"])
    check_logl(got, g["logl"])

    const = ExternalLightCurveModel("const", g["filters"], model.model_times, cosmo_grid=grid,
                                    generate_lightcurve_batch=lambda st, p: {f: np.full((len(p["timeshift"]), len(st)), -13.0) for f in g["filters"]})
    both = likelihood(CombinedLightCurveModelContainer([model, const], cosmo_grid=grid)).log_likelihood_batch(g["theta"], g["names"])
    eng = make_engine(g, "g150", with_data=True)
    own = eng.model_lightcurves(g["theta"])
    want = eng.loglike_lc(g["theta"], eng.stack([own, torch.full_like(own, -13.0)])).cpu().numpy()
    eng.close()
    rel = np.abs(both - want) / np.maximum(1.0, np.abs(want))
    print(f"combination: worst relative difference {rel[want != FLOOR].max():.3e}; rows moved by the second model: {int(np.sum(both != got))}")
    assert np.array_equal(both == FLOOR, want == FLOOR) and np.all(rel[want != FLOOR] <= 1e-6) and np.any(both != got)
