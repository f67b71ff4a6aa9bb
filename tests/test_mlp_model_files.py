"""Model files whose network has more than two Dense layers: the chain reader (a name -> array dict in the legacy HDF5 layout, so no
HDF5 writer is needed) and the flat ``.npz``."""
import numpy as np
import pytest

from nmma_amd.em import io as em_io


def legacy(names, shapes, seed=0):
    """``model_weights/<layer>/<layer>/{kernel,bias}:0`` datasets, inserted in plain string order of the names (h5py's visiting order)."""
    rng = np.random.default_rng(seed)
    layers = {n: (rng.standard_normal(s).astype(np.float32), rng.standard_normal(s[1]).astype(np.float32)) for n, s in zip(names, shapes)}
    d = {}
    for n in sorted(names):
        d[f"model_weights/{n}/{n}/bias:0"], d[f"model_weights/{n}/{n}/kernel:0"] = layers[n][1], layers[n][0]
    return d, [a for n in names for a in layers[n]]


@pytest.mark.parametrize("names,shapes", [
    (("dense_9", "dense_10", "dense_11", "dense_12"), ((6, 64), (64, 128), (128, 64), (64, 10))),    # the tutorial; string order is wrong
    (("dense", "dense_1", "dense_2", "dense_10"), ((32, 32), (32, 32), (32, 32), (32, 32))),         # only the names decide
    (("dense_3", "dense_2", "dense_1"), ((6, 64), (64, 128), (128, 10))),                            # names disagree: the one order that chains
    (("dense_4", "dense_5"), ((3, 2048), (2048, 10)))])                                              # two layers: today's four arrays
def test_chain_reader_orders_the_layers(names, shapes):
    d, want = legacy(names, shapes)
    got = em_io._dense_chain(d, "test")
    assert len(got) == 2 * len(names)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(g, w)


def test_chain_reader_refuses_shapes_that_do_not_chain():
    d, _ = legacy(("dense", "dense_1", "dense_2"), ((6, 64), (48, 32), (32, 10)))
    with pytest.raises(ValueError, match=r"do not chain: \(6, 64\), \(48, 32\), \(32, 10\)"):
        em_io._dense_chain(d, "test")


def test_npz_round_trip_of_a_deep_network(tmp_path):
    rng = np.random.default_rng(1)
    shapes = ((6, 64), (64, 128), (128, 64), (64, 10))
    t = {f"{c}{i + 1}": rng.standard_normal(s if c == "W" else s[1]).astype(np.float32) for i, s in enumerate(shapes) for c in "Wb"}
    t.update(VA=rng.standard_normal((30, 10)), mins=rng.random(30), maxs=1.0 + rng.random(30), tt=np.linspace(0.0, 20.0, 30),
             param_mins=np.zeros(6), param_maxs=np.ones(6), n_coeff=10)
    path = str(tmp_path / "deep.npz")
    em_io.save_svd_model(path, {"ztfr": t}, [f"p{k}" for k in range(6)])
    back, params = em_io.load_svd_model(path)
    assert params == [f"p{k}" for k in range(6)] and em_io.is_deep_model(back)
    for k in ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"):
        assert back["ztfr"][k].dtype == np.float32 and np.array_equal(back["ztfr"][k], t[k]), k
    assert [w.shape for w, _ in em_io.dense_chain(back["ztfr"])] == list(shapes)
