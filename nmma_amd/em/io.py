"""On-disk formats of the EM path.

* ``save_svd_model`` / ``load_svd_model``: the flat tensor file (one ``.npz``) this
  framework reads -- ``{filter}/W1,b1,W2,b2,VA,mins,maxs,tt,param_mins,param_maxs,n_coeff``; a network with more Dense layers
  carries ``W3,b3, ...`` as well (the last pair is the linear output layer).
* ``convert_reference_model``: reads the reference's own layout
  (``{model}.joblib`` + ``{model}[_tf]/{filter}.keras|.h5``, nmma/em/model.py:593-696)
  and writes the flat file: ``.joblib`` through joblib, legacy ``.h5`` networks through h5py or,
  without it, the built-in reader ``em/hdf5_lite.py``; ``.keras`` archives need keras.
* ``load_em_observations`` / ``write_em_observations``: light-curve data files in the reference's formats (nmma/em/io.py:16-184):
  ``time filter mag mag_error`` rows, the forced-photometry CSV, model tables, ``.json`` in standard or model form.
"""
from __future__ import annotations

import os
import re
from datetime import datetime, timezone

import numpy as np

_KEYS = ("W1", "b1", "W2", "b2", "VA", "mins", "maxs", "tt", "param_mins", "param_maxs")


#: a Gaussian-process surrogate (interpolation_type "sklearn_gp") holds these instead of the network's W1, b1, W2, b2:
#: gp_X [N][NP], gp_alpha [NC][N], gp_const / gp_ell / gp_rq_alpha / gp_ymean / gp_ystd [NC]
_GP_KEYS = ("gp_X", "gp_alpha", "gp_const", "gp_ell", "gp_rq_alpha", "gp_ymean", "gp_ystd")
_SVD_KEYS = ("VA", "mins", "maxs", "tt", "param_mins", "param_maxs")


def dense_chain(tensors):
    """``[(W1, b1), ..., (Wn, bn)]`` of one filter's tensors: the Dense layers in order, the last one linear."""
    chain = []
    while f"W{len(chain) + 1}" in tensors:
        i = len(chain) + 1
        chain.append((np.asarray(tensors[f"W{i}"]), np.asarray(tensors[f"b{i}"])))
    return chain


def is_deep_model(svd_model):
    """True when any filter's network has more than two Dense layers (served by ``EMEngine(model_kind="svd_mlp")``)."""
    return any("W3" in t for t in svd_model.values())


def is_gp_model(svd_model):
    return bool(svd_model) and all("gp_X" in t for t in svd_model.values())


def save_svd_model(path, svd_model, model_parameters=None):
    flat = {}
    for filt, t in svd_model.items():
        n_c = int(t["n_coeff"])
        deep = tuple(f"{c}{i + 1}" for i in range(2, len(dense_chain(t))) for c in "Wb")
        for k in (_GP_KEYS + _SVD_KEYS if "gp_X" in t else _KEYS + deep):
            a = np.asarray(t[k])
            if k == "VA":
                a = a[:, :n_c]
            flat[f"{filt}/{k}"] = a
        flat[f"{filt}/n_coeff"] = np.int64(n_c)
    if model_parameters is not None:
        flat["__model_parameters__"] = np.array(list(model_parameters))
    np.savez_compressed(path, **flat)


def load_svd_model(path):
    """Returns ``(svd_model, model_parameters or None)``."""
    svd, params = {}, None
    with np.load(path, allow_pickle=False) as z:
        for name in z.files:
            if name == "__model_parameters__":
                params = [str(x) for x in z[name]]
                continue
            filt, key = name.rsplit("/", 1)
            svd.setdefault(filt, {})[key] = z[name]
    for filt, t in svd.items():
        t["n_coeff"] = int(t["n_coeff"])
        for k in [k for k in t if re.fullmatch(r"[Wb]\d+", k)]:
            t[k] = np.ascontiguousarray(t[k], dtype=np.float32)
        for k in _SVD_KEYS + _GP_KEYS:
            if k in t:
                t[k] = np.ascontiguousarray(t[k], dtype=np.float64)
    return svd, params


def extract_gp_arrays(gps, where="GP surrogate"):
    """The plain arrays of one filter's fitted ``GaussianProcessRegressor`` list (``svd_model[filt]["gps"]``, one per SVD coefficient):
    ``gp_X [N][NP]`` (``X_train_``, shared by the coefficients), ``gp_alpha [NC][N]`` (``alpha_``) and per coefficient the kernel's
    constant, length scale and alpha with the target's mean and scale.  Only ``ConstantKernel * RationalQuadratic`` with a scalar length
    scale is accepted -- what nmma/em/training.py:431-436 builds and the device kernel evaluates; the classes are told by name, so
    sklearn is needed only to unpickle the objects."""
    X, alpha, hyper = None, [], {k: [] for k in ("gp_const", "gp_ell", "gp_rq_alpha", "gp_ymean", "gp_ystd")}
    for i, gp in enumerate(gps):
        kern = getattr(gp, "kernel_", None)
        k1, k2 = getattr(kern, "k1", None), getattr(kern, "k2", None)
        if (type(kern).__name__ != "Product" or type(k1).__name__ != "ConstantKernel" or type(k2).__name__ != "RationalQuadratic"
                or np.ndim(k2.length_scale) != 0):
            raise ValueError(f"{where}, coefficient {i}: only ConstantKernel * RationalQuadratic with a scalar length scale is evaluated "
                             f"on the device (nmma/em/training.py:431-436); found kernel {kern!r}")
        Xi = np.asarray(gp.X_train_, dtype=np.float64)
        if X is None:
            X = Xi
        elif Xi.shape != X.shape or not np.array_equal(Xi, X):
            raise ValueError(f"{where}: the coefficients' regressors were fitted on different training sets")
        a = np.asarray(gp.alpha_, dtype=np.float64)
        if a.ndim != 1 and not (a.ndim == 2 and a.shape[1] == 1):
            raise ValueError(f"{where}, coefficient {i}: a regressor with {a.shape[1:]} targets; one per coefficient is expected")
        alpha.append(a.reshape(-1))
        hyper["gp_const"].append(float(k1.constant_value))
        hyper["gp_ell"].append(float(k2.length_scale))
        hyper["gp_rq_alpha"].append(float(k2.alpha))
        hyper["gp_ymean"].append(float(np.asarray(gp._y_train_mean).reshape(-1)[0]))
        hyper["gp_ystd"].append(float(np.asarray(gp._y_train_std).reshape(-1)[0]))
    if X is None:
        raise ValueError(f"{where}: no regressors")
    out = {"gp_X": np.ascontiguousarray(X), "gp_alpha": np.ascontiguousarray(np.stack(alpha))}
    out.update({k: np.array(v, dtype=np.float64) for k, v in hyper.items()})
    return out


def convert_reference_gp_model(svd_path, model, out_path=None, filters=None):
    """Read the reference's sklearn_gp layout -- ``{model}.joblib`` plus ``{model}/{filter with ':' -> '_'}.joblib``, each a list of
    fitted regressors (nmma/em/model.py:623-625, training.py:419-427) -- into the flat arrays, and write the flat ``.npz`` when
    ``out_path`` is given (a machine without sklearn then loads that)."""
    import joblib
    core = "_".join(c for c in model.split("_") if c != "tf")
    meta = joblib.load(os.path.join(svd_path, f"{core}.joblib"))
    meta = {k.replace("_", ":"): v for k, v in meta.items()}          # model.py:604-606
    svd = {}
    for filt in (filters or list(meta)):
        if filt not in meta:
            continue
        path = os.path.join(svd_path, core, filt.replace(":", "_") + ".joblib")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no Gaussian-process file for filter {filt}: {path}")
        m = meta[filt]
        t = extract_gp_arrays(joblib.load(path), where=path)
        t.update({k: np.asarray(m[k], float) for k in _SVD_KEYS})
        t["n_coeff"] = min(int(m["n_coeff"]), t["gp_alpha"].shape[0])
        svd[filt] = t
    if out_path is not None:
        save_svd_model(out_path, svd)
    return svd


def _h5_datasets(path):
    """``{"group/.../name": array}`` of a legacy Keras ``.h5`` file: through h5py when it is importable, else through the built-in
    reader of the HDF5 subset such files use (``em/hdf5_lite.py``; the build image has no h5py)."""
    try:
        import h5py
        if not isinstance(getattr(h5py, "File", None), type):        # (a stand-in module, e.g. the test harness' import stubs)
            raise ImportError("h5py is not the real package")
    except ImportError:
        from . import hdf5_lite
        return hdf5_lite.read_datasets(path)
    out = {}
    with h5py.File(path, "r") as f:
        def visit(name, obj):
            if isinstance(obj, h5py.Dataset):
                out[name] = np.array(obj)
        f.visititems(visit)
    return out


def _layer_order_key(name):
    """Keras numbers its layers ``dense, dense_1, ..., dense_9, dense_10``: the suffix compares as a number, no suffix first."""
    m = re.fullmatch(r"(.*?)(?:_(\d+))?", name)
    return m.group(1), -1 if m.group(2) is None else int(m.group(2))


def _chain_in_order(named, where):
    """``named``: ``{layer name: (kernel, bias)}``.  The flat ``(W1, b1, ..., Wn, bn)`` in the order of the layers' names when the
    shapes chain that way; else in the one order in which they do chain; else a ValueError that lists the shapes."""
    layers = [named[k] for k in sorted(named, key=_layer_order_key)]
    if len(layers) < 2:
        raise ValueError(f"{where}: expected two or more Dense layers, found {len(layers)}")
    for w, b in layers:
        if w.ndim != 2 or b.shape != (w.shape[1],):
            raise ValueError(f"{where}: a Dense layer with kernel {w.shape} and bias {b.shape}")
    chains = lambda seq: all(seq[i][0].shape[1] == seq[i + 1][0].shape[0] for i in range(len(seq) - 1))
    if not chains(layers):
        # depth-first over the orders that chain (a handful of layers): exactly one must exist
        found = []

        def extend(seq, rest):
            if not rest:
                found.append(seq)
            for i, nxt in enumerate(rest):
                if len(found) < 2 and (not seq or seq[-1][0].shape[1] == nxt[0].shape[0]):
                    extend(seq + [nxt], rest[:i] + rest[i + 1:])
        extend([], layers)
        if len(found) != 1:
            raise ValueError(f"{where}: layer shapes do not chain"
                             + (" in one order only" if found else "") + ": " + ", ".join(str(w.shape) for w, _ in layers))
        layers = found[0]
    return tuple(a for layer in layers for a in layer)


def _dense_weights_from_h5(path):
    """(W1, b1, ..., Wn, bn) of a Keras model of Dense (and Dropout) layers saved as legacy HDF5; see ``_dense_chain``."""
    return _dense_chain(_h5_datasets(path), path)


def _dense_chain(datasets, where):
    """(W1, b1, ..., Wn, bn) of the Dense layers among ``datasets`` (name -> array) in the legacy HDF5 layout
    (``[model_weights/]<layer>/<layer>/{kernel,bias}:0``, nmma/em/training.py:353-364; what ``keras.saving.load_model`` reads at
    nmma/em/model.py:635-648).  The layers are ordered by their names, the numeric suffix compared as a number (``dense_9`` before
    ``dense_10``), and the shapes must chain; two layers give ``W1, b1, W2, b2`` as before."""
    layers = {}
    for name, arr in datasets.items():
        parts = name.split("/")
        if parts[0] == "model_weights":          # a full model file (keras model.save): model_weights/<layer>/<layer>/{kernel,bias}:0
            parts = parts[1:]
        if len(parts) < 2 or parts[0] == "optimizer_weights":
            continue                             # (a weights-only file, model.save_weights, has the layer groups at the root)
        leaf = parts[-1].split(":")[0]
        if leaf in ("kernel", "bias"):
            layers.setdefault(parts[0], {})[leaf] = np.asarray(arr)
    return _chain_in_order({k: (v["kernel"], v["bias"]) for k, v in layers.items() if "kernel" in v and "bias" in v}, where)


def _dense_pair(datasets, where):
    """(W1, b1, ..., Wn, bn) of the Dense layers among ``datasets`` (name -> array) in a ``.keras`` archive's layout
    (``layers/<name>/vars/{0,1}``): groups that hold exactly one 2-D kernel and one 1-D bias of matching width, ordered as in
    ``_dense_chain``."""
    groups = {}
    for name, arr in datasets.items():
        parent = name.rsplit("/", 1)[0] if "/" in name else ""
        groups.setdefault(parent, []).append(np.asarray(arr))
    dense = {}
    for parent, members in groups.items():
        if len(members) != 2:
            continue
        k = next((a for a in members if a.ndim == 2), None)
        b = next((a for a in members if a.ndim == 1), None)
        if k is not None and b is not None and b.shape[0] == k.shape[1]:
            parts = parent.split("/")
            dense[parts[1] if parts[0] == "layers" and len(parts) > 1 else parent] = (k, b)
    return _chain_in_order(dense, where)


def _check_archive_activations(config, where):
    """Refuse a ``.keras`` archive whose ``config.json`` names a hidden activation other than relu or a non-linear output: the device
    kernels evaluate relu hidden layers and a linear output, nothing else."""
    def dense_configs(node):
        if isinstance(node, dict):
            if node.get("class_name") == "Dense" and isinstance(node.get("config"), dict):
                yield node["config"]
            for v in node.values():
                yield from dense_configs(v)
        elif isinstance(node, list):
            for v in node:
                yield from dense_configs(v)
    acts = [c.get("activation") for c in dense_configs(config)]
    acts = [a.get("config", a.get("class_name")) if isinstance(a, dict) else a for a in acts]
    if any(a != "relu" for a in acts[:-1]) or (acts and acts[-1] not in ("linear", None)):
        raise ValueError(f"{where}: Dense activations {acts}; only relu hidden layers and a linear output layer are evaluated")


def _dense_weights_from_keras_archive(path):
    """(W1, b1, ..., Wn, bn) of a ``.keras`` archive (Keras 3: a zip holding ``config.json`` and ``model.weights.h5``; what
    nmma/em/training.py saves today and nmma/em/model.py:635-643 loads first).  With keras importable the model is loaded as the
    reference does; without it the weights file inside the archive is read directly (h5py or the built-in HDF5 reader) and the
    Dense layers are ordered by name and shape; ``config.json``, where readable, must name relu hidden layers and a linear output.  The archive layout (``layers/<name>/vars/{0,1}``) is from Keras' public sources, NOT
    pinned here -- keras is absent from the build image and the reference tree holds no ``.keras`` file."""
    try:
        import keras
        if not hasattr(getattr(keras, "saving", None), "load_model") or not isinstance(getattr(keras, "Model", None), type):
            raise ImportError("keras is not the real package")
        net = keras.saving.load_model(path, compile=False)
        dense = [l for l in net.layers if l.get_weights()]
        acts = [getattr(getattr(l, "activation", None), "__name__", None) for l in dense]
        if any(a != "relu" for a in acts[:-1]) or acts[-1] != "linear":
            raise ValueError(f"{path}: Dense activations {acts}; only relu hidden layers and a linear output layer are evaluated")
        return tuple(a for l in dense for a in l.get_weights())
    except ImportError:
        pass
    import zipfile
    with zipfile.ZipFile(path) as z:
        inner = next((n for n in z.namelist() if n.endswith("model.weights.h5")), None)
        if inner is None:
            raise ValueError(f"{path}: no model.weights.h5 in the archive")
        raw = z.read(inner)
        try:
            import json
            config = json.loads(z.read("config.json"))
        except (KeyError, ValueError):
            config = None
    if config is not None:
        _check_archive_activations(config, path)
    try:
        import h5py
        if not isinstance(getattr(h5py, "File", None), type):
            raise ImportError
        import io as _io
        data = {}
        with h5py.File(_io.BytesIO(raw), "r") as f:
            f.visititems(lambda name, obj: data.__setitem__(name, np.array(obj)) if isinstance(obj, h5py.Dataset) else None)
    except ImportError:
        from . import hdf5_lite
        data = hdf5_lite.read_datasets(data=raw)
    data = {k: v for k, v in data.items() if not k.startswith("optimizer")}
    return _dense_pair(data, path)


def convert_reference_model(svd_path, model, out_path, filters=None, interpolation_type="tensorflow"):
    """Read the reference's model files and write the flat tensor file."""
    import joblib
    core = "_".join(c for c in model.split("_") if c != "tf")
    meta = joblib.load(os.path.join(svd_path, f"{core}.joblib"))
    meta = {k.replace("_", ":"): v for k, v in meta.items()}          # model.py:604-606
    spec = "_tf" if interpolation_type == "tensorflow" else ""
    svd = {}
    for filt in (filters or list(meta)):
        base = os.path.join(svd_path, f"{model}{spec}", filt.replace(":", "_"))
        if os.path.isfile(base + ".keras"):
            net = _dense_weights_from_keras_archive(base + ".keras")
        elif os.path.isfile(base + ".h5"):
            net = _dense_weights_from_h5(base + ".h5")
        else:
            raise FileNotFoundError(f"no .keras/.h5 network for filter {filt} under {base}")
        m = meta[filt]
        svd[filt] = dict({f"{'Wb'[i % 2]}{i // 2 + 1}": np.float32(a) for i, a in enumerate(net)},
                         VA=np.asarray(m["VA"], float), mins=np.asarray(m["mins"], float),
                         maxs=np.asarray(m["maxs"], float), tt=np.asarray(m["tt"], float),
                         param_mins=np.asarray(m["param_mins"], float),
                         param_maxs=np.asarray(m["param_maxs"], float), n_coeff=int(m["n_coeff"]))
    save_svd_model(out_path, svd)
    return svd


def _to_mjd(token, time_format=None):
    """One time token -> MJD: an ISO / ISOT date (UTC), else a number in ``time_format`` (``mjd`` -- the default -- ``jd``, ``unix``:
    the leap-second-free ones of the astropy ``Time`` formats the reference's ``--time-format`` takes, io.py:130-136)."""
    try:
        value = float(token)
    except ValueError:
        dt = datetime.fromisoformat(str(token).strip().replace("Z", "+00:00"))
        if dt.tzinfo is None:
            dt = dt.replace(tzinfo=timezone.utc)
        return dt.timestamp() / 86400.0 + 40587.0
    fmt = (time_format or "mjd").lower()
    if fmt == "mjd":
        return value
    if fmt == "jd":
        return value - 2400000.5
    if fmt == "unix":
        return value / 86400.0 + 40587.0
    raise ValueError(f"time format {time_format!r} is not one of mjd, jd, unix")


def _read_observation_rows(path, time_format):
    """``time filter mag mag_error`` rows (io.py:116-144): comment lines and a ``time`` / ``mjd`` header are skipped."""
    rows = {}
    with open(path) as fh:
        for line in fh:
            parts = line.split()
            if not parts or parts[0].startswith(("#", "time", "mjd")):
                continue
            t, filt, mag, err = _to_mjd(parts[0], time_format), parts[1], float(parts[2]), float(parts[3])
            rows.setdefault(filt, []).append((t, mag, err))
    if not rows:
        raise ValueError(f"no photometry rows in {path}")
    return rows


def _read_survey_csv(path):
    """The forced-photometry CSV the reference falls back to (io.py:101-114): columns ``mjd, filter, mag_corr, magerr,
    limiting_mag``; rows without a magnitude are upper limits at ``limiting_mag`` (infinite error)."""
    import csv
    rows = {}
    with open(path, newline="") as fh:
        for rec in csv.DictReader(fh):
            mag = float(rec["mag_corr"]) if rec["mag_corr"].strip() not in ("", "nan", "NaN") else np.nan
            err = float(rec["magerr"]) if rec["magerr"].strip() else np.nan
            if np.isnan(mag):
                mag, err = float(rec["limiting_mag"]), np.inf
            rows.setdefault(rec["filter"], []).append((float(rec["mjd"]), mag, err))
    return rows


def _read_model_table(path):
    """A model light curve as text (io.py:85-97): header ``time f1 f2 ... [f1_error ...]``, one row per epoch."""
    with open(path) as fh:
        lines = [ln for ln in (raw.strip() for raw in fh) if ln]
    header = lines[0].lstrip("#").split()
    table = np.array([[float(v) for v in ln.split()] for ln in lines[1:] if not ln.startswith("#")])
    cols = dict(zip(header, table.T))
    time = cols.pop("time")
    return {f: {"time": time, "mag": v, "mag_error": cols.get(f + "_error", np.zeros_like(time))}
            for f, v in cols.items() if not f.endswith("_error")}


def _decode_json(obj):
    """bilby's JSON encoding of arrays and complex numbers (``{"__array__": true, "content": [...]}``), as the reference's reader
    decodes it (io.py:60-61)."""
    if isinstance(obj, dict):
        if obj.get("__array__"):
            return np.asarray(obj["content"])
        if obj.get("__complex__"):
            return complex(obj["real"], obj["imag"])
    return obj


def _read_json(path):
    import json
    with open(path) as fh:
        data = json.load(fh, object_hook=_decode_json)
    if "time" in data:          # a model light curve: one time axis, one column per filter (io.py:64-73)
        time = data["time"]
        data = {k: {"time": time, "mag": v, "mag_error": data.get(f"{k}_error", np.zeros_like(np.asarray(time, float)))}
                for k, v in data.items() if k != "time" and not k.endswith("_error")}
    return data


def load_em_observations(filename, args=None, format="observations", filters=None):
    """Light-curve data in the reference's standard form ``{filter: {"time": mjd[], "mag": [], "mag_error": []}}`` (io.py:16-55) from

    * a dict (returned as it is) or a Namespace (its ``light_curve_data``),
    * a ``.json`` file in the standard form or in the model form (``time`` + one column per filter [+ ``<filter>_error``]),
    * a text file of ``time filter mag mag_error`` rows (``format="observations"``; ISO times or numbers in ``args.time_format``;
      an infinite error marks an upper limit), or -- when that does not parse -- the forced-photometry CSV
      (``mjd, filter, mag_corr, magerr, limiting_mag``),
    * a text table ``time f1 f2 ...`` (``format="model"``).

    Text observations come back sorted by time within each filter; ``filters`` keeps only the named ones."""
    import argparse
    if isinstance(filename, dict):
        return filename
    if isinstance(filename, argparse.Namespace) or (args is None and hasattr(filename, "light_curve_data")):
        args, filename = filename, filename.light_curve_data
        if isinstance(filename, dict):
            return filename
    if filename is None:
        raise ValueError("No filename provided for lightcurve data.")
    filename = os.fspath(filename)
    if filename.endswith(".json"):
        data = _read_json(filename)
    elif "obs" in format:
        try:
            rows = _read_observation_rows(filename, getattr(args, "time_format", None))
        except Exception:
            rows = _read_survey_csv(filename)
        data = {}
        for filt, r in rows.items():
            a = np.array(sorted(r))
            data[filt] = {"time": a[:, 0], "mag": a[:, 1], "mag_error": a[:, 2]}
    elif "model" in format:
        data = _read_model_table(filename)
    else:
        raise ValueError("Standard format is not supported for reading from csv files. Please use json files instead.")
    return {filt: {k: np.array(v) for k, v in sub.items()} for filt, sub in data.items() if filters is None or filt in filters}


def _isot(mjd):
    dt = datetime.fromtimestamp(round((float(mjd) - 40587.0) * 86400.0 * 1000.0) / 1000.0, tz=timezone.utc)
    return dt.strftime("%Y-%m-%dT%H:%M:%S.") + f"{dt.microsecond // 1000:03d}"


def write_em_observations(filename, data, format="observations"):
    """The reverse (io.py:146-184): ``.json`` in the standard form; ``.txt`` / ``.dat`` as observation rows (ISOT time, filter,
    magnitude and error with three decimals, sorted by time) or as a model table."""
    import json
    directory = os.path.dirname(os.fspath(filename))
    if directory:
        os.makedirs(directory, exist_ok=True)
    filename = os.fspath(filename)
    if filename.endswith(".json"):
        with open(filename, "w") as fh:
            json.dump({f: {k: np.asarray(v).tolist() for k, v in sub.items()} for f, sub in data.items()}, fh, indent=2)
        return
    if not filename.endswith((".txt", ".dat")):
        return
    if format == "observations":
        rows = sorted((float(t), f, float(m), float(e)) for f, sub in data.items()
                      for t, m, e in zip(sub["time"], sub["mag"], sub["mag_error"]))
        with open(filename, "w") as fh:
            fh.write("#time filter mag mag_error\n")
            for t, f, m, e in rows:
                fh.write(f"{_isot(t)} {f} {m:.3f} {e:.3f}\n")
    elif format == "model":
        names = list(data)
        with_err = [f for f in names if not np.all(np.isnan(np.asarray(data[f]["mag_error"], float)))]
        time = np.asarray(data[names[-1]]["time"], float)
        cols = [np.asarray(data[f]["mag"], float) for f in names] + [np.asarray(data[f]["mag_error"], float) for f in with_err]
        with open(filename, "w") as fh:
            fh.write("#time " + " ".join(names + [f + "_error" for f in with_err]) + "\n")
            for i, t in enumerate(time):
                fh.write(f"{t:.5f} " + " ".join(f"{c[i]:.3f}" for c in cols) + "\n")
    else:
        raise ValueError(f"unknown light-curve file format {format!r}")
