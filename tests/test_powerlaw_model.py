"""``PowerLawFluxLightCurveModel`` (Sr2023, synchrotron_powerlaw) on the host side: construction and the factory (no GPU)."""
from types import SimpleNamespace

import numpy as np
import pytest

from nmma_amd.em import HostGalaxyLightCurveModel, PowerLawFluxLightCurveModel
from nmma_amd.em.model import DEVICE_MODEL_CLASSES, HOST_ONLY_MODELS, CombinedLightCurveModelContainer, create_light_curve_model_from_args

ST = np.array([0.5, 1.0, 2.0, 4.0])


def test_parameter_names_follow_the_filters_and_host_mag_is_per_filter():
    m = PowerLawFluxLightCurveModel("Sr2023", filters="g,r,i", sample_times=ST)
    assert HostGalaxyLightCurveModel is PowerLawFluxLightCurveModel
    assert m.model_parameters == ["alpha_AG", "a_AG_g", "a_AG_r", "a_AG_i", "f_nu_g", "f_nu_r", "f_nu_i"]
    assert np.array_equal(m.host_mag, [23.9] * 3) and m.gpu_model_kind == "powerlaw"
    m = PowerLawFluxLightCurveModel("Sr2023", filters=["g", "r"], sample_times=ST, host_mag=[23.0, 22.5])
    kw = m.engine_kwargs()
    assert np.array_equal(m.host_mag, [23.0, 22.5]) and kw["model_kind"] == "powerlaw" and kw["powerlaw"]["model"] == "Sr2023"
    assert kw["ebv_coeff"] == {"g": 0.0, "r": 0.0}          # extinction is implicit in the host-galaxy model
    s = PowerLawFluxLightCurveModel("synchrotron_powerlaw", filters=["g", "X"], sample_times=ST, filter_lambdas={"X": 1e-9})
    assert s.model_parameters[:3] == ["alpha_time", "beta_freq", "F_ref"] and s.filter_nu0["X"] == pytest.approx(2.99792458e17)


@pytest.mark.parametrize("kwargs, message", [
    (dict(host_mag=0), "not 0"), (dict(host_mag=[23.9, 0.0]), "not 0"), (dict(host_mag=[23.9] * 3), "one value per filter"),
    (dict(sample_times=[0.0, 1.0]), "> 0"), (dict(sample_times=[-1.0, 1.0]), "> 0"), (dict(filters=None), "filters"),
    (dict(model="synchrotron_powerlaw", filters=["g", "X"]), "wavelengths"), (dict(model="PL_BB_fixedT"), "one of")])
def test_construction_refuses(kwargs, message):
    with pytest.raises(ValueError, match=message):
        PowerLawFluxLightCurveModel(**{**dict(model="Sr2023", filters=["g", "r"], sample_times=ST), **kwargs})


def test_factory_builds_sr2023_on_the_device_only_when_asked():
    assert "Sr2023" in HOST_ONLY_MODELS and DEVICE_MODEL_CLASSES["Sr2023"] is PowerLawFluxLightCurveModel
    m = create_light_curve_model_from_args("Sr2023", SimpleNamespace(), filters=["g", "r"], sample_times=ST, device_models=("Sr2023",))
    assert isinstance(m, PowerLawFluxLightCurveModel) and m.model_parameters[0] == "alpha_AG"
    with pytest.raises(ValueError, match="evaluated on the host"):
        create_light_curve_model_from_args("Sr2023", SimpleNamespace(), filters=["g", "r"], sample_times=ST)
    grb = SimpleNamespace(model_parameters=["E0"], generate_lightcurve=lambda st, p: {})
    both = create_light_curve_model_from_args("TrPi2018,Sr2023", SimpleNamespace(), filters=["g", "r"], sample_times=ST,
                                              host_models={"TrPi2018": grb}, device_models=("Sr2023",))
    assert isinstance(both, CombinedLightCurveModelContainer) and isinstance(both.lc_models[1], PowerLawFluxLightCurveModel)
