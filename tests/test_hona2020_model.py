"""Host side of the HoNa2020 kilonova: the defaults and refusals of ``SimpleKilonovaLightCurveModel("HoNa2020")`` and the factory's
``device_models`` (no GPU: nothing here builds an engine)."""
from types import SimpleNamespace

import numpy as np
import pytest

from nmma_amd.em.model import (DEVICE_MODEL_CLASSES, HOST_ONLY_MODELS, SimpleKilonovaLightCurveModel, SVDLightCurveModel,
                               create_light_curve_model_from_args)


def test_class_defaults():
    m = SimpleKilonovaLightCurveModel("HoNa2020", filters="g,r")
    assert m.model == "HoNa2020" and m.filters == ["g", "r"] and m.gpu_model_kind == "hona2020"
    assert m.model_parameters == ["log10_mej", "vej_max", "vej_min", "vej_frac", "log10_kappa_low_vej", "log10_kappa_high_vej"]
    assert np.array_equal(m.model_times, np.geomspace(0.05, 14.0, 150))
    kw = m.engine_kwargs()
    assert kw["model_kind"] == "hona2020" and kw["filter_nu0"]["g"] == pytest.approx(2.99792458e8 / 4866.46e-10, rel=1e-15)
    st = np.array([0.05, 1.0, 2.0])
    m = SimpleKilonovaLightCurveModel("HoNa2020", filters=["ztfg"], sample_times=st, filter_lambdas={"ztfg": 4.8e-7})
    assert np.array_equal(m.model_times, [0.05, 1.0, 2.0]) and np.array_equal(st, [0.05, 1.0, 2.0]) and m.filter_nu0["ztfg"] == 2.99792458e8 / 4.8e-7
    me = SimpleKilonovaLightCurveModel("Me2017", filters=["g"])                  # unchanged
    assert me.gpu_model_kind == "me2017" and me.model_parameters == ["log10_mej", "log10_vej", "beta", "log10_kappa_r"]
    assert np.array_equal(me.model_times, np.geomspace(0.01, 14.0, 150))


@pytest.mark.parametrize("kwargs,match", [
    (dict(filters=["g"], sample_times=[0.04, 1.0]), "0.05 days"), (dict(filters=["g"], sample_times=[2.0, 1.0]), "ascending"),
    (dict(filters=["g"], sample_times=[1.0, 1.0, 2.0]), "ascending"), (dict(filters=["g"], sample_times=[1.0]), "ascending"),
    (dict(filters=["g"], sample_times=[1.0, 1.04]), "first step"), (dict(filters=["g"], sample_times=[1.0, 1.05]), "first step"),
    (dict(filters=["ztfg"]), "effective wavelengths")])
def test_class_refusals(kwargs, match):
    with pytest.raises(ValueError, match=match):
        SimpleKilonovaLightCurveModel("HoNa2020", **kwargs)


def test_factory_device_models(monkeypatch):
    args = SimpleNamespace()
    assert HOST_ONLY_MODELS == ("TrPi2018", "Piro2021", "PL_BB_fixedT", "Sr2023", "Arnett") and "HoNa2020" in DEVICE_MODEL_CLASSES
    m = create_light_curve_model_from_args("HoNa2020", args, filters=["g", "r"], device_models=("HoNa2020",))
    assert isinstance(m, SimpleKilonovaLightCurveModel) and m.model == "HoNa2020" and len(m.model_times) == 150
    m = create_light_curve_model_from_args("HoNa2020", SimpleNamespace(em_tmin=0.1, em_tmax=3.0, em_nsteps=7), filters=["g"],
                                           device_models=("HoNa2020",))
    assert np.array_equal(m.model_times, np.linspace(0.1, 3.0, 7))
    # the default is as before: the name falls through to the SVD surrogate's loader
    seen = []
    monkeypatch.setattr(SVDLightCurveModel, "__init__", lambda self, name, **kw: seen.append(name))
    create_light_curve_model_from_args("HoNa2020", args, filters=["g"], sample_times=np.array([1.0, 2.0]))
    assert seen == ["HoNa2020"]
    me = create_light_curve_model_from_args("Me2017", args, filters=["g"], sample_times=np.array([1.0, 2.0]), device_models=("HoNa2020",))
    assert isinstance(me, SimpleKilonovaLightCurveModel) and me.model == "Me2017"
