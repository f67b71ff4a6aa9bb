"""Host side of the bolometric path: ``SimpleBolometricLightCurveModel``, the plain ``SystematicsHandler``,
``setup_bolometric_lc_data`` and the sub-model ``EMTransientLikelihood`` picks (no GPU: nothing here builds an engine)."""
import numpy as np
import pytest

from nmma_amd.em.em_likelihood import BasicEMTransient, EMTransientLikelihood, MultiFilterTransient, build_bolometric_likelihood
from nmma_amd.em.model import SimpleBolometricLightCurveModel
from nmma_amd.em.systematics import FilterSystematicsHandler, SystematicsHandler
from nmma_amd.em.utils import setup_bolometric_lc_data
from tests.helpers import SimplePrior

TABLE = {"phase": np.array([3.0, 1.0, 2.0]), "Lbb": np.array([3e41, 1e41, 2e41]), "Lbb_unc": np.array([3e39, 1e39, np.inf])}
PRIORS = {n: SimplePrior(0.0, 1.0) for n in ("tau_m", "log10_mni", "t_0", "timeshift")}


def test_model_construction_and_grids():
    m = SimpleBolometricLightCurveModel()
    assert m.model == "Arnett" and m.model_parameters == ["tau_m", "log10_mni"] and m.filters is None
    assert np.array_equal(m.model_times, np.linspace(0.005, 20.0, 40))
    m = SimpleBolometricLightCurveModel("Arnett_modified", sample_times=[0.5, 1.0, 4.0])
    assert m.model_parameters == ["tau_m", "log10_mni", "t_0"] and np.array_equal(m.model_times, [0.5, 1.0, 4.0])
    assert np.array_equal(SimpleBolometricLightCurveModel(sample_times=[0.0, 1.0]).model_times, [0.0, 1.0])     # t = 0 is a node of Arnett


@pytest.mark.parametrize("build,match", [
    (lambda: SimpleBolometricLightCurveModel("Arnett", sample_times=[1.0, 0.5, 2.0]), "ascending"),
    (lambda: SimpleBolometricLightCurveModel("Arnett", sample_times=[1.0]), "ascending"),
    (lambda: SimpleBolometricLightCurveModel("Arnett", sample_times=[-1.0, 1.0]), ">= 0"),
    (lambda: SimpleBolometricLightCurveModel("Arnett_modified", sample_times=[0.0, 1.0]), "> 0"),
    (lambda: SimpleBolometricLightCurveModel("Piro2021"), "Arnett"),
    (lambda: SystematicsHandler({"time_nodes": 4, "prior": "Uniform(0, 1)"}, None, TABLE["phase"]), "time-node"),
    (lambda: build_bolometric_likelihood(TABLE, 0.0, PRIORS, systematics_file={"time_range": "lin 1 5 3", "prior": "Uniform(0, 1)"}), "time-node"),
    (lambda: EMTransientLikelihood(SimpleBolometricLightCurveModel(), setup_bolometric_lc_data(TABLE, 0.0),
                                   FilterSystematicsHandler(["g"], None, 1.0, TABLE["phase"]), PRIORS), "plain SystematicsHandler"),
    (lambda: EMTransientLikelihood(SimpleBolometricLightCurveModel(), setup_bolometric_lc_data(TABLE, 0.0),
                                   SystematicsHandler(None, None, TABLE["phase"]), PRIORS, detection_limit=1e40), "detection_limit")])
def test_refusals(build, match):
    with pytest.raises(ValueError, match=match):
        build()


def test_setup_bolometric_lc_data_sorts_by_phase():
    structured = np.array(list(zip(TABLE["phase"], TABLE["Lbb"], TABLE["Lbb_unc"])), dtype=[("phase", float), ("Lbb", float), ("Lbb_unc", float)])
    for table in (TABLE, structured):
        t, v, s, trig = setup_bolometric_lc_data(table, 0.25)
        assert np.array_equal(t, [0.75, 1.75, 2.75]) and np.array_equal(v, [1e41, 2e41, 3e41]) and np.array_equal(s, [1e39, np.inf, 3e39])
        assert trig == 0.25


def test_likelihood_picks_its_sub_model():
    lik = build_bolometric_likelihood(TABLE, 0.0, dict(PRIORS, em_syserr=SimplePrior(0.0, 1e40)), em_model="Arnett_modified")
    sub = lik.sub_model
    assert isinstance(sub, BasicEMTransient) and sub.systematics_handler.sampled and sub._engine is None
    assert lik.parameter_names() == ["tau_m", "log10_mni", "t_0", "timeshift", "em_syserr"]
    assert np.array_equal(sub.light_curve_times, [1.0, 2.0, 3.0]) and sub.light_curve_model.model == "Arnett_modified"
    assert lik.parameter_conversion({"tau_m": 2.0})["tau_m"] == 2.0
    plain = build_bolometric_likelihood(TABLE, 0.0, PRIORS).sub_model.systematics_handler
    assert not plain.sampled and plain.error_budget_value == 1e-4 and np.array_equal(plain({}), np.full(3, 1e-4))
    # photometry per filter goes where it went
    from nmma_amd.em.model import ShockCoolingLightCurveModel
    data = ({"g": np.array([1.0])}, {"g": np.array([20.0])}, {"g": np.array([0.1])}, 0.0)
    lik = EMTransientLikelihood(ShockCoolingLightCurveModel(filters=["g"]), data, FilterSystematicsHandler(["g"], None, 1.0, data[0]),
                                {n: SimplePrior(0.0, 1.0) for n in ("log10_Menv", "log10_Renv", "log10_Ee")})
    assert isinstance(lik.sub_model, MultiFilterTransient)
