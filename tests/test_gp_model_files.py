"""Loading a Gaussian-process surrogate (``interpolation_type="sklearn_gp"``): the flat ``.npz``, the reference's joblib layout,
and the kernels that are refused.  CPU only."""
import os

import numpy as np
import pytest

from nmma_amd.em import io as em_io
from nmma_amd.em.model import SVDLightCurveModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_bulla.npz")


def _kernel(outer="Product", k1="ConstantKernel", k2="RationalQuadratic", length_scale=0.7):
    """A stand-in with sklearn's class names and attributes (the loader tells kernels by name: no sklearn needed to refuse one)."""
    mk = lambda name, text, **kw: type(name, (), dict(kw, __repr__=lambda self: text))()
    return mk(outer, f"{outer}({k1}, {k2}(length_scale={length_scale}))", k1=mk(k1, k1, constant_value=1.5),
              k2=mk(k2, k2, length_scale=length_scale, alpha=0.2))


def _regressor(kernel, n=6, n_p=2, seed=0):
    rng = np.random.default_rng(seed)
    return type("GaussianProcessRegressor", (), dict(kernel_=kernel, X_train_=rng.uniform(size=(n, n_p)), alpha_=rng.standard_normal(n),
                                                     _y_train_mean=0.0, _y_train_std=1.0))()


def test_flat_file_round_trip_and_construction(tmp_path):
    with np.load(GOLDEN, allow_pickle=False) as z:
        filters = [str(f) for f in z["filters"]][:2]
        svd = {f: dict({k: z[f"{f}/{k}"] for k in em_io._GP_KEYS + em_io._SVD_KEYS}, n_coeff=int(z[f"{f}/n_coeff"])) for f in filters}
    path = str(tmp_path / "Bu2019lm_sparse.npz")
    em_io.save_svd_model(path, svd, ["log10_mej_dyn", "log10_mej_wind"])
    back, params = em_io.load_svd_model(path)
    assert params == ["log10_mej_dyn", "log10_mej_wind"] and em_io.is_gp_model(back)
    for f in filters:
        for k in em_io._GP_KEYS + em_io._SVD_KEYS:
            assert back[f][k].dtype == np.float64 and np.array_equal(back[f][k], svd[f][k])
    model = SVDLightCurveModel("Bu2019lm_sparse", svd_path=str(tmp_path), interpolation_type="sklearn_gp", svd_mag_ncoeff=7)
    kw = model.engine_kwargs()
    assert kw["model_kind"] == "svd_gp" and kw["n_coeff"] == 7 and model.filters == filters
    with pytest.raises(ValueError, match="does not match the model file"):
        SVDLightCurveModel("Bu2019lm_sparse", svd_path=path, interpolation_type="keras")


@pytest.mark.parametrize("kernel,found", [
    (_kernel(length_scale=np.array([0.5, 0.9])), "RationalQuadratic"),        # anisotropic
    (_kernel(k2="RBF"), "RBF"),
    (_kernel(outer="Sum"), "Sum"),
])
def test_other_kernels_are_refused_with_the_kernel_named(kernel, found):
    with pytest.raises(ValueError, match="ConstantKernel \\* RationalQuadratic") as err:
        em_io.extract_gp_arrays([_regressor(_kernel()), _regressor(kernel)])
    assert "coefficient 1" in str(err.value) and found in str(err.value)


def test_api_gp_is_refused_with_its_own_message():
    with pytest.raises(ValueError, match="api_gp.*out of scope"):
        SVDLightCurveModel("Bu2019lm_sparse", svd_path="unused", interpolation_type="api_gp")


def test_reference_joblib_layout_loads_to_the_regressors_arrays(tmp_path):
    """``{model}.joblib`` + ``{model}/{filter with ':' -> '_'}.joblib`` holding real fitted regressors (what training.py:419-427 writes)."""
    joblib = pytest.importorskip("joblib")
    gpr = pytest.importorskip("sklearn.gaussian_process")
    from sklearn.gaussian_process.kernels import RationalQuadratic
    rng = np.random.default_rng(3)
    meta, fitted = {}, {}
    os.makedirs(tmp_path / "Toy")
    for filt in ("ps1::z", "ztfr"):
        x, n_t = rng.uniform(size=(12, 2)), 4
        gps = [gpr.GaussianProcessRegressor(kernel=1.0 * RationalQuadratic(1.0, 0.1), optimizer=None, normalize_y=bool(i)).fit(x, rng.standard_normal(12))
               for i in range(3)]
        meta[filt.replace(":", "_")] = dict(VA=rng.standard_normal((n_t, 3)), mins=np.zeros(n_t), maxs=np.ones(n_t), tt=np.arange(n_t, dtype=float),
                                            param_mins=np.zeros(2), param_maxs=np.ones(2), n_coeff=3)
        joblib.dump(gps, tmp_path / "Toy" / (filt.replace(":", "_") + ".joblib"), compress=9)
        fitted[filt] = gps
    joblib.dump(meta, tmp_path / "Toy.joblib")
    model = SVDLightCurveModel("Toy", svd_path=str(tmp_path), interpolation_type="sklearn_gp", model_parameters=["a", "b"])
    assert sorted(model.svd_mag_model) == ["ps1::z", "ztfr"] and os.path.isfile(tmp_path / "Toy.npz")
    for filt, gps in fitted.items():
        t = model.svd_mag_model[filt]
        assert np.array_equal(t["gp_X"], gps[0].X_train_)
        for i, gp in enumerate(gps):
            assert np.array_equal(t["gp_alpha"][i], gp.alpha_)
            assert (t["gp_const"][i], t["gp_ell"][i], t["gp_rq_alpha"][i]) == (gp.kernel_.k1.constant_value, gp.kernel_.k2.length_scale, gp.kernel_.k2.alpha)
            assert (t["gp_ymean"][i], t["gp_ystd"][i]) == (gp._y_train_mean, gp._y_train_std)
    assert model.svd_mag_model["ztfr"]["gp_ystd"][1] != 1.0       # (normalize_y: a non-trivial mean and scale are carried)
