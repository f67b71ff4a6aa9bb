"""Surrogates with several hidden layers (``EMEngine(model_kind="svd_mlp")``, kernel ``mlp_surrogate``) on the device against a plain
fp64 numpy forward of the same fp32 weights.  The coefficient tolerance is derived, not measured: with eps = 2^-24, d_0 = eps |x| and
``d_l = (K_l + 2) eps (|W_l|^T a_{l-1} + |b_l|) + |W_l|^T d_{l-1}``, where a_l is the forward of absolute values and K_l the layer's
input width padded to 16 (the kernel's dot products run over the padded width; relu is 1-Lipschitz)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def network(rng, n_p, widths, n_c):
    """He-normal fp32 kernels, biases of order 0.1: ``{W1, b1, ..., Wn, bn}``, the last pair the linear output layer."""
    t, k = {}, n_p
    for i, h in enumerate(tuple(widths) + (n_c,), start=1):
        t[f"W{i}"] = (rng.standard_normal((k, h)) * np.sqrt(2.0 / k)).astype(np.float32)
        t[f"b{i}"] = (0.1 * rng.standard_normal(h)).astype(np.float32)
        k = h
    return t


def synthetic_filter(seed, n_p, widths, n_c, n_t=21):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n_t, n_t)))
    mins = rng.uniform(-17.0, -16.0, n_t)
    return dict(network(rng, n_p, widths, n_c), VA=q[:, :n_c].copy(), mins=mins, maxs=mins + rng.uniform(1.5, 2.5, n_t),
                tt=np.linspace(0.5, 10.5, n_t), param_mins=np.full(n_p, -1.0), param_maxs=np.full(n_p, 2.0), n_coeff=n_c)


def forward(theta_model, t):
    """(c_ref, d_out): the fp64 forward and the propagated bound of the docstring, both [B, NC]."""
    x = (theta_model - t["param_mins"]) / (t["param_maxs"] - t["param_mins"])
    h, a, d = x, np.abs(x), EPS32 * np.abs(x)
    n = sum(k.startswith("W") for k in t)
    for i in range(1, n + 1):
        w, b = t[f"W{i}"].astype(np.float64), t[f"b{i}"].astype(np.float64)
        k_pad = 16 * ((w.shape[0] + 15) // 16)
        h = h @ w + b
        a_next = a @ np.abs(w) + np.abs(b)
        d = (k_pad + 2) * EPS32 * a_next + d @ np.abs(w)
        a = a_next
        if i < n:
            h = np.maximum(h, 0.0)
    return h, d


def make_engine(svd, n_p, **kw):
    from nmma_amd.engine import EMEngine
    names = [f"p{k}" for k in range(n_p)]
    return EMEngine(svd, list(svd), names, names, model_kind="svd_mlp", **kw)


def thetas(seed, batch, n_p):
    return np.random.default_rng(seed).uniform(-1.2, 2.2, (batch, n_p))


@pytest.mark.parametrize("n_p,widths,n_c,batch", [
    (6, (64, 128, 64), 10, 33),         # the reference tutorial's network
    (1, (16, 16), 1, 1),                # the smallest
    (8, (20, 36), 16, 17),              # padding; both maxima of the ABI
    (4, (256, 16, 256), 10, 100),       # wide - narrow - wide, several tiles
    (3, (16,) * 6, 10, 16),             # the depth limit
    (4, (256, 256), 10, 40),            # 256 KiB of weights: beyond LDS, the blocks are read from L2
    (6, (2048,), 10, 5)])               # beyond the kernel's width: refused, never approximated
def test_coefficients_within_the_propagated_bound(n_p, widths, n_c, batch):
    from nmma_amd._lib import NMMAHipError
    svd = {"f0": synthetic_filter(100 + n_p + len(widths), n_p, widths, n_c)}
    if max(widths) > 256:
        with pytest.raises(NMMAHipError, match=r"filter 0, hidden layer 1: width 2048 is outside 1 \.\. 256"):
            make_engine(svd, n_p)
        return
    theta = thetas(7 + batch, batch, n_p)
    eng = make_engine(svd, n_p)
    got = eng.coefficients(theta).cpu().numpy()
    eng.close()
    assert got.dtype == np.float64 and got.shape == (batch, 1, n_c)
    want, bound = forward(theta, svd["f0"])
    err = np.abs(got[:, 0] - want)
    print(f"widths {widths}: worst error / bound = {np.max(err / bound):.2e}")
    assert np.all(err <= bound)


def test_filters_with_different_architectures():
    svd = {"deep": synthetic_filter(21, 6, (64, 128, 64), 10), "flat": synthetic_filter(22, 6, (32,), 10)}
    theta = thetas(3, 40, 6)
    eng = make_engine(svd, 6)
    both = eng.coefficients(theta).cpu().numpy()
    eng.close()
    for m, f in enumerate(svd):
        eng = make_engine({f: svd[f]}, 6)
        assert np.array_equal(eng.coefficients(theta).cpu().numpy()[:, 0], both[:, m]), f
        eng.close()
        want, bound = forward(theta, svd[f])
        assert np.all(np.abs(both[:, m] - want) <= bound)


def test_rows_do_not_depend_on_the_batch():
    """Rows of a B = 100 call are bit-identical to the same rows at B = 1 and B = 17 (other tile neighbours, the other half of the
    workgroup, a ragged last tile): coefficients and curves."""
    svd = {"deep": synthetic_filter(31, 4, (64, 128, 64), 10), "wide": synthetic_filter(32, 4, (256, 16, 256), 10)}
    theta = thetas(9, 100, 4)
    eng = make_engine(svd, 4)
    full_c, full_lc = eng.coefficients(theta).cpu().numpy(), eng.model_lightcurves(theta).cpu().numpy()
    assert np.isfinite(full_lc).all()
    for lo, hi in ((0, 1), (99, 100), (0, 17), (40, 57)):
        assert np.array_equal(eng.coefficients(theta[lo:hi]).cpu().numpy(), full_c[lo:hi])
        assert np.array_equal(eng.model_lightcurves(theta[lo:hi]).cpu().numpy(), full_lc[lo:hi])
    eng.close()


def test_curves_and_log_likelihood_through_the_plugin():
    """``SVDLightCurveModel`` picks the deep-network engine for a dict with three hidden layers per filter.  Curves against
    ``VA . c_ref``, span / mins and ``np.interp`` with the same +inf pattern: a finite magnitude lies within ``(maxs - mins) |VA| d_out``
    plus 8 eps64 of the magnitude (at a sample time: the larger of its two bracketing nodes' bounds, the lerp being a convex
    combination).  log L against the likelihood-from-curves entry point fed the numpy curves, 1e-6 relative."""
    import torch
    from nmma_amd.em.em_likelihood import EMTransientLikelihood
    from nmma_amd.em.model import SVDLightCurveModel
    from nmma_amd.em.systematics import FilterSystematicsHandler
    from tests.helpers import SimplePrior
    filters, names = ["ztfg", "ztfr"], [f"p{k}" for k in range(5)]
    svd = {f: synthetic_filter(41 + k, 5, (48, 96, 24), 10) for k, f in enumerate(filters)}
    st = np.linspace(0.0, 12.0, 49)                 # tt spans 0.5 .. 10.5: +inf on both sides
    theta = thetas(11, 37, 5)
    want_lc = np.empty((len(theta), 2, len(st)))
    tol = np.empty_like(want_lc)
    for m, f in enumerate(filters):
        t = svd[f]
        c, d = forward(theta, t)
        span = t["maxs"] - t["mins"]
        mag = (c @ t["VA"].T) * span + t["mins"]                                    # [B, NT]
        node_tol = (d @ np.abs(t["VA"]).T) * span + 8 * EPS64 * np.abs(mag)
        i = np.clip(np.searchsorted(t["tt"], st, side="right") - 1, 0, len(t["tt"]) - 2)
        for b in range(len(theta)):
            want_lc[b, m] = np.interp(st, t["tt"], mag[b], left=np.inf, right=np.inf)
        tol[:, m] = np.maximum(node_tol[:, i], node_tol[:, i + 1]) + 8 * EPS64 * np.maximum(np.abs(mag[:, i]), np.abs(mag[:, i + 1]))
    model = SVDLightCurveModel("deep", svd_mag_model=svd, interpolation_type="tensorflow", filters=filters, model_parameters=names,
                               sample_times=st)
    assert model.engine_kwargs()["model_kind"] == "svd_mlp"
    # photometry: row 0's numpy curve with unit-variance-scale scatter; the other rows' curves differ by a few tenths of a magnitude
    rng = np.random.default_rng(5)
    times = {f: np.sort(rng.uniform(1.0, 10.0, 20)) for f in filters}
    mags = {f: np.interp(times[f], st[np.isfinite(want_lc[0, m])], want_lc[0, m][np.isfinite(want_lc[0, m])]) + 0.3 * rng.standard_normal(20)
            for m, f in enumerate(filters)}
    sigmas = {f: np.full(20, 0.2) for f in filters}
    handler = FilterSystematicsHandler(filters, systematics_file=None, error_budget=1.0, light_curve_times=times)
    lik = EMTransientLikelihood(model, (times, mags, sigmas, 0.0), handler, {n: SimplePrior(-2.0, 3.0) for n in names}, filters=filters)
    got = lik.log_likelihood_batch(theta, names)
    eng = lik.sub_model.engine(names)
    got_lc = eng.model_lightcurves(theta).cpu().numpy()
    want = eng.loglike_lc(theta, torch.as_tensor(want_lc)).cpu().numpy()
    fin = np.isfinite(want_lc)
    assert np.array_equal(np.isfinite(got_lc), fin) and np.array_equal(np.isposinf(got_lc), ~fin) and (~fin).any()
    err = np.abs(got_lc[fin] - want_lc[fin])
    print(f"curves: worst error / bound = {np.max(err / tol[fin]):.2e}")
    assert np.all(err <= tol[fin])
    print(f"log L from the numpy curves: {want.min():.2f} .. {want.max():.2f}")
    assert np.all((np.abs(want) >= 10.0) & (np.abs(want) <= 100.0))                 # unfloored, of order 10 to 100 on every row
    rel = np.abs(got - want) / np.abs(want)
    print(f"log L: worst relative difference {rel.max():.3e}")
    assert np.all(rel <= 1e-6)
