#!/usr/bin/env python
"""Time the bolometric likelihood (kernel bol_logl, BolometricEngine) for Arnett_modified on the model's 40-node grid with the epochs of
tests/golden/arnett.npz, rows drawn from the example's prior box.

    perf_arnett.py [B ...]            per batch size (default 4096 65536), HIP-event time per call after two seconds of warm-up: loglike
                                      (one launch), its measurement form without the likelihood phase (option "probe": the share of the
                                      curve generator), lightcurves; then -- a COMPARISON, not a requirement -- the host route a user had:
                                      the reference's formula vectorised in numpy with scipy.special.dawsn standing in for quad, the
                                      upload of lbol[B, NS] and loglike_lc, on the host clock around a device synchronise
    perf_arnett.py ... --launches K   K plain loglike launches and nothing else (the body of a profiler run)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "arnett.npz")
NAMES = ["tau_m", "log10_mni", "t_0", "timeshift"]
BOX = dict(tau_m=(1.0, 5.0), log10_mni=(-4.0, 0.0), t_0=(1.0, 10.0), timeshift=(-8.0, -2.0))


def numpy_curves(st, p):
    """arnett_modified_lc for a batch with the closed form of the two integrals: {parameter: [B]} -> lbol[B, NS]."""
    from scipy.special import dawsn
    tau = p["tau_m"][:, None]
    mni = (10 ** p["log10_mni"] * 1.988409870698051e33)[:, None]
    x = st[None, :] / tau

    def S(q):
        return np.exp(-2 * x * q) * (1 + 2 * q * dawsn(x - q)) - np.exp(-x * x) * (1 - 2 * q * dawsn(q))

    lbol = mni * ((3.9e10 - 6.78e9) * S(tau / (2 * 8.8)) + 6.78e9 * S(tau / (2 * 111.3)))
    return lbol * -np.expm1(-(p["t_0"][:, None] / st[None, :]) ** 2)


def event_time(call, n=20, windows=5):
    import torch
    t_end = time.perf_counter() + 2.0          # warm clocks: two seconds of untimed calls
    while time.perf_counter() < t_end:
        call()
        torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / n * 1e3)
    return float(np.median(times)), min(times), max(times)


def main():
    import torch
    from nmma_amd.engine import BolometricEngine
    sizes = [int(a) for i, a in enumerate(sys.argv) if i > 0 and a.isdigit() and sys.argv[i - 1] != "--launches"] or [4096, 65536]
    with np.load(GOLDEN, allow_pickle=False) as z:
        st, data = z["g40/sample_times"], tuple(z[f"data/real/{k}"] for k in "tvs")
    eng = BolometricEngine("Arnett_modified", NAMES, st, data=data)
    host = BolometricEngine(None, NAMES, st, data=data)
    rng = np.random.default_rng(7)
    for batch in sizes:
        theta_np = np.column_stack([rng.uniform(*BOX[n], batch) for n in NAMES])
        theta = torch.as_tensor(theta_np, device="cuda:0")
        if "--launches" in sys.argv:
            for _ in range(int(sys.argv[sys.argv.index("--launches") + 1])):
                eng.loglike(theta)
            torch.cuda.synchronize()
            continue
        report = lambda what, t: print(f"B={batch} {what}: {t[0]:.1f} us per call (5 windows of 20: {t[1]:.1f} .. {t[2]:.1f}), "
                                       f"{batch * len(st) / t[0]:.0f} nodes/us")
        report("loglike (bol_logl)", event_time(lambda: eng.loglike(theta)))
        eng.set_option("probe", 1)
        report("bol_logl without the likelihood phase", event_time(lambda: eng.loglike(theta)))
        eng.set_option("probe", 0)
        report("lightcurves (phase A + stores)", event_time(lambda: eng.lightcurves(theta)))
        p = {n: theta_np[:, k] for k, n in enumerate(NAMES)}
        want = eng.loglike(theta).cpu().numpy()
        times, parts = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            lc = numpy_curves(st, p)
            t1 = time.perf_counter()
            got = host.loglike_lc(theta, torch.as_tensor(lc).to("cuda:0"))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            times.append(t2 - t0)
            parts.append((t1 - t0, t2 - t1))
        k = int(np.argmin(times))
        rel = np.abs(got.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
        print(f"B={batch} host route (numpy + dawsn, upload, loglike_lc): {times[k] * 1e3:.1f} ms per call (best of 3; numpy {parts[k][0] * 1e3:.1f} ms, "
              f"upload + likelihood {parts[k][1] * 1e3:.1f} ms); worst relative difference to the device route {rel.max():.2e}")
    eng.close()
    host.close()


if __name__ == "__main__":
    main()
