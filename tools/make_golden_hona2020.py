#!/usr/bin/env python
"""Golden data for the HoNa2020 kilonova (``SimpleKilonovaLightCurveModel("HoNa2020")``, kernel ``hona2020_lc``) from the reference's own
code.

Runs only in the build container (imports the reference under oracle/ref_harness.py; needs scipy).  Steps:

1. candidate theta rows are drawn from a seeded box and sorted into CLASSES (rejected steps, ``vej_frac`` exactly 0 / 1, the first
   shell's ``searchsorted`` index 0 or 1); the first rows of every class are kept, then ordinary rows around TRUTH;
2. for three grids -- ``[0.5, 2, 3.5]`` with filter r, ``geomspace(0.05, 14, 65)`` with g, r, i and the model's default grid with the
   nine built-in names -- the reference's ``HoNa_lc``, called on a COPY of the times (it scales its argument in place) at the
   host-frame frequencies ``nu0 (1 + z)``, gives the source-frame curves; a wrapper around ``lightcurve_generation.solve_ivp`` records
   the accepted and rejected steps;
3. S per row and grid: the largest change of any finite magnitude under the twelve one-ulp nudges of the six parameters -- the
   reference's own conditioning, the yardstick of the tests' bound.  A row for which a nudge changes a step count sits on an
   accept / reject tie and is left out (at most a quarter of the candidates; every class keeps two rows);
4. ``hona_numpy`` below restates the whole algorithm in plain loops in the kernel's summation order; its largest
   ``|mag - mag_ref| / (S + eps (1 + x) 2.5 / ln 10)`` is stored as ``k_numpy`` (the tests give the kernel four times that), and its
   step counts must equal scipy's;
5. photometry is drawn around the truth row's detector-frame curves and the reference's ``EMTransientLikelihood.log_likelihood`` is
   recorded for every row, around its ``SimpleKilonovaLightCurveModel`` constructed as "Me2017" and rebound to ``HoNa_lc`` (the
   reference's own wiring of the model cannot run: DEVIATIONS.md).

Output: tests/golden/hona2020.npz -- ARRAYS ONLY (no pickles, no reference source).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from nmma_amd import synthetic as syn  # noqa: E402

SEED, PER_CLASS, N_ORDINARY = 20261128, 2, 10
FILTERS9 = ["u", "g", "r", "i", "z", "y", "J", "H", "K"]
GRIDS = {"g3": (np.array([0.5, 2.0, 3.5]), ["r"]), "g65": (np.geomspace(0.05, 14.0, 65), ["g", "r", "i"]),
         "g150": (np.geomspace(0.05, 14.0, 150), FILTERS9)}
PARAMS = ["log10_mej", "vej_max", "vej_min", "vej_frac", "log10_kappa_low_vej", "log10_kappa_high_vej"]
NAMES = ["luminosity_distance", "timeshift"] + PARAMS
TRUTH = dict(luminosity_distance=40.0, timeshift=0.1, log10_mej=-1.6, vej_max=0.5, vej_min=0.1, vej_frac=0.4,
             log10_kappa_low_vej=0.7, log10_kappa_high_vej=-0.2)
BOX = dict(log10_mej=(-3.0, -1.0), vej_max=(0.3, 0.8), vej_min=(0.02, 0.2), vej_frac=(0.0, 1.0), log10_kappa_low_vej=(-1.0, 1.5),
           log10_kappa_high_vej=(-1.0, 1.5))
CLASSES = ("no_reject", "two_rejects", "frac_0", "frac_1", "first_i0", "first_i1")
EPS = np.finfo(np.float64).eps
MAG_PER_REL = 2.5 / np.log(10.0)

# cgs constants (nmma/core/constants.py with astropy's CODATA-2018 values)
MSUN, C_CGS, H_CGS, KB, SIGSB, D10PC, DAY = 1.988409870698051e33, 2.99792458e10, 6.62607015e-27, 1.380649e-16, 5.6703744191844314e-05, \
    10 * 3.085677581491367e18, 86400.0
# Dormand-Prince tableau as scipy's doubles (scipy/integrate/_ivp/rk.py)
RK_C = [0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1]
RK_A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
        [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]]
RK_B = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]
RK_E = [-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]
N_SHELL, MAX_ATTEMPTS, MAX_NODES = 99, 4096, 128


def wave_sum(v):
    """The kernel's reduction of 99 shell values: shells 64 .. 98 onto 0 .. 34, then a butterfly over the 64 lanes."""
    w = v[:64].copy()
    w[:N_SHELL - 64] += v[64:]
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[idx ^ off]
    return w[0]


def shells(p):
    """Phase S: (bes, dMs, tds, taus, first shell's searchsorted index), lightcurve_generation.py:661-745 with n = 4.5."""
    n = 4.5
    mej = 10 ** p["log10_mej"] * MSUN
    vmax, vmin = p["vej_max"], p["vej_min"]
    vel = [vmin, p["vej_frac"] * (vmax - vmin) + vmin, vmax]
    opac = [10 ** p["log10_kappa_low_vej"], 10 ** p["log10_kappa_high_vej"]]
    ls, le = np.log10(vmin), np.log10(vmax)
    step = (le - ls) / 99
    geom = [vmin] + [float(np.power(10.0, i * step + ls)) for i in range(1, 99)] + [vmax]
    bes = np.array([vmax + vmin - geom[99 - k] for k in range(N_SHELL)])
    nxt = np.append(bes[1:], vmax)
    dbe = nxt - bes
    bej = [float(np.power(v / vmin, 1 - n)) for v in vel]
    acc1 = opac[1] * (bej[2] - bej[1])
    tau_accum = [-(acc1 + opac[0] * (bej[1] - bej[0])), -acc1, 0.0]
    vej_0 = vmin * C_CGS
    v3 = float(np.power(vej_0, 3))
    rho_0 = mej * (n - 3) / (4 * np.pi * v3) / (1 - float(np.power(vmax / vmin, 3 - n)))
    scale = vej_0 * rho_0 / (n - 1)
    taus, dMs, first_i = np.empty(N_SHELL), np.empty(N_SHELL), None
    for k in range(N_SHELL):
        i = min(int(vel[0] < bes[k]) + int(vel[1] < bes[k]) + int(vel[2] < bes[k]), 2)
        first_i = i if k == 0 else first_i
        q = bes[k] / vmin
        taus[k] = (tau_accum[i] + opac[i - 1] * (float(np.power(q, 1 - n)) - bej[i])) * scale
        dMs[k] = 4. * np.pi * v3 * rho_0 * float(np.power(q, 2 - n)) * dbe[k] / vmin
    return bes, dMs, taus * bes, taus, first_i


def hona_numpy(st_days, p, nu_host, erfc):
    """``(mag[M, NS], accepted, rejected)`` of one row: the kernel's algorithm in the kernel's order (NaN everywhere for a failed row)."""
    bes, dMs, tds, taus, _ = shells(p)
    ts = np.asarray(st_days, float) * DAY
    nan = np.full((len(nu_host), len(ts)), np.nan)

    def lum(E, t):
        t_dif = tds / t
        return erfc(np.sqrt(0.5 * t_dif / t)) * E / (np.minimum(t, t_dif) + bes * t)

    def rhs(t, E):
        heat = 2 * 2e18 * 0.5 * float(np.power(0.5 - 1.0 / np.pi * np.arctan((t - 1.3) / 0.11), 1.3))
        return -E / t - lum(E, t) + dMs * heat

    with np.errstate(all="ignore"):
        t, t_bound, h_abs, y = ts[0], ts[-1], 5e-2 * DAY, np.zeros(N_SHELL)
        f = rhs(t, y)
        xs, ys, acc, rej, in_step, done = [], [], 0, 0, False, False
        for _ in range(MAX_ATTEMPTS):
            if not in_step:
                min_step = 10 * (np.nextafter(t, np.inf) - t)
                h_abs, rejected, in_step = max(h_abs, min_step), False, True
            if h_abs < min_step:
                return nan, acc, rej
            t_new = t + h_abs
            if t_new - t_bound > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = abs(h)
            K = [f]
            for s in range(1, 6):
                dy = K[0] * RK_A[s][0]
                for j in range(1, s):
                    dy = dy + K[j] * RK_A[s][j]
                K.append(rhs(t + RK_C[s] * h, y + dy * h))
            up = K[0] * RK_B[0]
            for j in (2, 3, 4, 5):
                up = up + K[j] * RK_B[j]
            y_new = y + h * up
            K.append(rhs(t + h, y_new))
            e = K[0] * RK_E[0]
            for j in (2, 3, 4, 5, 6):
                e = e + K[j] * RK_E[j]
            r = e * h / (1e-6 + np.maximum(np.abs(y), np.abs(y_new)) * 1e-3)
            err = np.sqrt(wave_sum(r * r)) / N_SHELL ** 0.5
            if err < 1:
                g = 0.9 * err ** -0.2
                factor = 10.0 if err == 0 else (g if g < 10 else 10.0)
                h_abs *= min(1, factor) if rejected else factor
                t, y, f, acc, in_step = t_new, y_new, K[6], acc + 1, False
                if len(xs) == MAX_NODES:
                    return nan, acc, rej
                xs.append(np.log(t))
                ys.append(np.log(wave_sum(lum(y, t))))
                if t - t_bound >= 0:
                    done = True
                    break
            else:
                g = 0.9 * err ** -0.2
                h_abs *= g if g > 0.2 else 0.2
                rejected, rej = True, rej + 1
        if not done or len(xs) < 2 or not np.all(np.isfinite(ys)):
            return nan, acc, rej
        # ---- phase P: not-a-knot spline (scipy CubicSpline's system, plain tridiagonal elimination), photosphere, 1 / T
        x, yv, n = np.array(xs), np.array(ys), len(xs)
        dx, slope = np.diff(x), np.diff(yv) / np.diff(x)
        if n == 2:
            sd = np.array([slope[0], slope[0]])
        else:
            lo, di, upd, b = np.zeros(n), np.empty(n), np.zeros(n), np.empty(n)
            if n == 3:
                di[0], upd[0], b[0] = 1.0, 1.0, 2 * slope[0]
                lo[2], di[2], b[2] = 1.0, 1.0, 2 * slope[1]
            else:
                d = x[2] - x[0]
                di[0], upd[0], b[0] = dx[1], d, ((dx[0] + 2 * d) * dx[1] * slope[0] + dx[0] ** 2 * slope[1]) / d
                d = x[-1] - x[-3]
                lo[-1], di[-1], b[-1] = d, dx[-2], (dx[-1] ** 2 * slope[-2] + (2 * d + dx[-1]) * dx[-2] * slope[-1]) / d
            for i in range(1, n - 1):
                lo[i], di[i], upd[i] = dx[i], 2 * (dx[i - 1] + dx[i]), dx[i - 1]
                b[i] = 3 * (dx[i] * slope[i - 1] + dx[i - 1] * slope[i])
            for i in range(1, n):
                w = lo[i] / di[i - 1]
                di[i] = di[i] - w * upd[i - 1]
                b[i] = b[i] - w * b[i - 1]
            sd = np.empty(n)
            sd[-1] = b[-1] / di[-1]
            for i in range(n - 2, -1, -1):
                sd[i] = (b[i] - upd[i] * sd[i + 1]) / di[i]
        lt_rev, lb_rev = np.log(taus[::-1]), np.log(bes[::-1])
        inv_T, R = np.empty(len(ts)), np.empty(len(ts))
        for j, tj in enumerate(ts):
            lx = np.log(tj)
            i = int(np.clip(np.searchsorted(x, lx, side="right") - 1, 0, n - 2))
            tt = (sd[i] + sd[i + 1] - 2 * slope[i]) / dx[i]
            c0, c1, s = tt / dx[i], (slope[i] - sd[i]) / dx[i] - tt, lx - x[i]
            lbol = np.exp(yv[i] + sd[i] * s + c1 * (s * s) + c0 * ((s * s) * s))
            be = np.exp(np.interp(2 * lx, lt_rev, lb_rev))
            R[j] = be * tj * C_CGS
            inv_T[j] = np.power(SIGSB / (lbol / (4 * np.pi * R[j] * R[j])), 0.25)
        # ---- phase C: blackbody magnitudes
        mag = np.empty((len(nu_host), len(ts)))
        for k, nu in enumerate(nu_host):
            ex = np.minimum(H_CGS * nu * inv_T / KB, 700)
            F = 2.0 * H_CGS / (C_CGS * C_CGS) * (nu * nu * nu) / np.expm1(ex) * R * R / (D10PC * D10PC)
            mag[k] = np.where(F > 0, -2.5 * np.log10(F) + (-48.6), np.inf) if np.sum(F > 0) >= 2 else np.nan
    return mag, acc, rej


class StepCounter:
    """Wraps ``lightcurve_generation.solve_ivp``: accepted steps from ``out.t``, rejected ones from the right-hand-side count
    (RK45 spends one evaluation at the start and six per attempt)."""

    def __init__(self, lg):
        self.inner, self.accepted, self.rejected = lg.solve_ivp, 0, 0
        lg.solve_ivp = self

    def __call__(self, *a, **k):
        out = self.inner(*a, **k)
        self.accepted = len(out.t) - 1
        self.rejected = (out.nfev - 1) // 6 - self.accepted
        assert out.status == 0 and (out.nfev - 1) % 6 == 0, (out.status, out.nfev)
        return out


def reference_row(ref, counter, st, p, nu_host, filters):
    """``(mag[M, NS], accepted, rejected)`` from the reference's HoNa_lc on a copy of the times."""
    with np.errstate(all="ignore"):
        mag = ref.lightcurve_generation.HoNa_lc(np.array(st, float), dict(p), nu_host, filters)
    return np.array([mag[f] for f in filters]), counter.accepted, counter.rejected


def nudges(p):
    for k in PARAMS:
        for way in (-np.inf, np.inf):
            q = dict(p)
            q[k] = float(np.nextafter(p[k], way))
            yield q


def measure_row(ref, counter, p, z, nu0):
    """Per grid ``(mag, accepted, rejected, S)``, or None for a row on an accept / reject tie (or with a non-finite magnitude)."""
    res = {}
    for key, (st, filters) in GRIDS.items():
        nus = np.array([nu0[f] for f in filters]) * (1 + z)
        mag, acc, rej = reference_row(ref, counter, st, p, nus, filters)
        if not np.all(np.isfinite(mag)):
            return None
        S = 0.0
        for q in nudges(p):
            m2, a2, r2 = reference_row(ref, counter, st, q, nus, filters)
            if (a2, r2) != (acc, rej):
                return None
            S = max(S, float(np.max(np.abs(m2 - mag))))
        res[key] = (mag, acc, rej, S)
    return res


def classify(p, res):
    rej = res["g150"][2]
    first_i = shells(p)[4]
    return {c for c, hit in (("no_reject", rej == 0), ("two_rejects", rej >= 2), ("frac_0", p["vej_frac"] == 0.0), ("frac_1", p["vej_frac"] == 1.0),
                             ("first_i0", first_i == 0), ("first_i1", first_i == 1)) if hit}


def reference_likelihood(ref, grid, data):
    ref.utils.get_all_bandpass_metadata = lambda: []
    ref.utils.M4OPT_INSTALLED = False        # the mocked import 'succeeds'; the real package is absent
    m = ref.model.SimpleKilonovaLightCurveModel("Me2017", filters=list(FILTERS9), sample_times=GRIDS["g150"][0].copy())
    m.model, m.model_parameters = "HoNa2020", list(PARAMS)
    m.lc_func = lambda st, p, nu, f: ref.lightcurve_generation.HoNa_lc(st.copy(), p, nu, f)
    m.redshift_func = lambda p: np.interp(p["luminosity_distance"], grid[0], grid[1])
    m.check_vs_priors = lambda priors: None
    if data is None:
        return m, None
    times, mags, sigmas = data
    handler = ref.systematics.FilterSystematicsHandler(list(FILTERS9), error_budget=1.0, light_curve_times=times)
    lik = ref.em_likelihood.EMTransientLikelihood(m, (times, mags, sigmas, 0.0), handler, ref.base.PriorDict({n: object() for n in NAMES}),
                                                  filters=list(FILTERS9), detection_limit=np.inf)
    return m, lik


def main():
    from scipy.special import erfc
    ref = ref_harness.reference_modules()
    counter = StepCounter(ref.lightcurve_generation)
    rng = np.random.default_rng(SEED)
    grid = syn.flat_lcdm_grid(1.0, 200.0)
    model, _ = reference_likelihood(ref, grid, None)
    nu0 = dict(zip(FILTERS9, np.asarray(model.nu_0s, float)))
    assert np.array_equal(np.geomspace(0.07, 0.61, 100)[1:-1], [np.power(10.0, i * ((np.log10(0.61) - np.log10(0.07)) / 99) + np.log10(0.07)) for i in range(1, 99)])

    def draw(kind):
        if kind == "box":
            p = {k: float(rng.uniform(*BOX[k])) for k in BOX}
            p["vej_frac"] = float(rng.choice([0.0, 1.0, p["vej_frac"], p["vej_frac"]]))
            p.update(luminosity_distance=float(rng.uniform(5.0, 150.0)), timeshift=float(rng.uniform(-0.02, 0.2)))
        else:
            p = {k: TRUTH[k] + float(rng.uniform(-0.15, 0.15)) * (BOX[k][1] - BOX[k][0]) * 0.5 for k in BOX}
            p.update(luminosity_distance=float(rng.uniform(30.0, 55.0)), timeshift=TRUTH["timeshift"] + float(rng.uniform(-0.03, 0.03)))
        return p

    rows, results, members, tried, excluded = [dict(TRUTH)], [], {c: 0 for c in CLASSES}, 0, 0
    results.append(measure_row(ref, counter, rows[0], float(np.interp(TRUTH["luminosity_distance"], *grid)), nu0))
    assert results[0] is not None, "the truth row sits on an accept / reject tie"
    for c in classify(rows[0], results[0]):
        members[c] += 1
    n_ordinary = 0
    while tried < 400 and (any(v <= PER_CLASS for v in members.values()) or n_ordinary < N_ORDINARY):
        box = any(v <= PER_CLASS for v in members.values())
        p = draw("box" if box else "truth")
        if box and not any(members[c] <= PER_CLASS for c in ("frac_0",) * (p["vej_frac"] == 0.0) + ("frac_1",) * (p["vej_frac"] == 1.0)
                           + ("no_reject", "two_rejects", "first_i0", "first_i1")):
            continue
        tried += 1
        res = measure_row(ref, counter, p, float(np.interp(p["luminosity_distance"], *grid)), nu0)
        if res is None:
            excluded += 1
            continue
        cls = classify(p, res)
        if box and not any(members[c] <= PER_CLASS for c in cls):
            continue
        rows.append(p)
        results.append(res)
        n_ordinary += 0 if box else 1
        for c in cls:
            members[c] += 1
    # two rows whose photometry lies outside the model's observer-frame times (the curves do not depend on the time shift): floored
    for src, shift in ((1, 1.0), (2, -3.0)):
        rows.append(dict(rows[src], timeshift=shift))
        results.append(results[src])
    print(f"rows: {len(rows)} of {tried} candidates, {excluded} left out on a tie; classes: {members}")
    theta = np.array([[p[n] for n in NAMES] for p in rows])
    z = np.interp(theta[:, 0], *grid)
    out = {"names": np.array(NAMES), "dist_grid": grid[0], "z_grid": grid[1], "filters": np.array(FILTERS9),
           "nu0": np.array([nu0[f] for f in FILTERS9]), "theta": theta, "redshift": z}

    k_numpy = 0.0
    for key, (st, filters) in GRIDS.items():
        nus = np.array([nu0[f] for f in filters])
        curves = np.array([res[key][0] for res in results])
        steps = np.array([[res[key][1], res[key][2]] for res in results], dtype=np.int32)
        S = np.array([res[key][3] for res in results])
        for r, p in enumerate(rows):
            mine, acc, rej = hona_numpy(st, p, nus * (1 + z[r]), erfc)
            assert (acc, rej) == tuple(steps[r]), (key, r, acc, rej, steps[r])
            lg = ref.lightcurve_generation
            with np.errstate(all="ignore"):
                inv_T, _ = lg.temp_photosphere_HoNa(*lg.setup_HoNa_params(np.array(st, float), dict(p)), 4.5)
            xi = H_CGS * (1 + z[r]) * inv_T / KB             # the clipped exponent of filter f is min(nu0_f xi, 700)
            x = np.minimum(nus[:, None] * xi[None, :], 700.0)
            k_numpy = max(k_numpy, float(np.max(np.abs(mine - curves[r]) / (S[r] + EPS * (1 + x) * MAG_PER_REL))))
            out.setdefault(f"{key}/xi", []).append(xi)
        out[f"{key}/xi"] = np.array(out[f"{key}/xi"])
        out[f"{key}/sample_times"], out[f"{key}/filters"] = st, np.array(filters)
        out[f"{key}/curves"], out[f"{key}/steps"], out[f"{key}/S"] = curves, steps, S
        print(f"{key}: NS={len(st)} M={len(filters)}  steps accepted {steps[:, 0].min()} .. {steps[:, 0].max()}, rejected up to {steps[:, 1].max()}"
              f"  S {S.min():.2e} .. {S.max():.2e}  K(numpy) so far {k_numpy:.3f}")
    out["k_numpy"] = np.array(k_numpy)

    # ---- photometry around the reference's own detector-frame curves at TRUTH, and log L of every row
    obs_times, lc = model.gen_detector_lc(dict(TRUTH))
    times, mags, sigmas = {}, {}, {}
    for k, f in enumerate(FILTERS9):
        n = 5 + k
        times[f] = np.sort(rng.uniform(0.3, 12.0, n))
        mags[f] = np.interp(times[f], obs_times, lc[f]) + 0.1 * rng.standard_normal(n)
        sigmas[f] = np.full(n, 0.1)
        out[f"data/{f}/t"], out[f"data/{f}/m"], out[f"data/{f}/s"] = times[f], mags[f], sigmas[f]
    _, lik = reference_likelihood(ref, grid, (times, mags, sigmas))
    with np.errstate(all="ignore"):
        logl = np.array([lik.log_likelihood(dict(p)) for p in rows])
    floor = -np.finfo(np.float64).max
    out["logl"] = logl
    n_floor = int(np.sum(logl <= floor))
    print(f"log L: {len(logl) - n_floor} finite in ({logl[logl > floor].min():.2f}, {logl[logl > floor].max():.2f}), {n_floor} floored")
    if any(v < 2 for v in members.values()) or 4 * excluded > tried or len(logl) - n_floor < 8 or n_floor < 2 or not np.isfinite(k_numpy):
        raise SystemExit("refusing to write the golden file: a class holds fewer than two rows, more than a quarter of the candidates sat on "
                         "a tie, or too few finite / floored log L")
    path = os.path.join(ROOT, "tests", "golden", "hona2020.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
