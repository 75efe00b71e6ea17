"""Cost of the mask in a fit with missing observations: the headline shape (200 trials x 1000 bins x 100 channels, 5
latents, the initialisation of bench.py) fitted without a mask and as a masked fit with 0 % and 20 % of the entries
missing, the three sessions alternating EM iteration by EM iteration in one process.  Prints one JSON line: milliseconds
per EM iteration (median of --reps after --warmup) of each, the ratios to the unmasked iteration, and milliseconds per
mstep_accum Newton launch (the library's per-launch events, a short phase of its own: they keep the M-step off its graph).

    python tools/masked_fit_bench.py [--reps 15 --warmup 5] [--parent-lib PATH/libvlgp_hip.so]
    python tools/masked_fit_bench.py --only masked20     (one session alone, for a kernel trace under rocprofv3)

--parent-lib: the unmasked session runs on another build of the library (the parent commit's) loaded beside this one;
without it the unmasked session is this build's own (the same device code: profiles/masked_fit/device_code_compare.txt)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def other_build(path):
    """A second libvlgp_hip.so with the binding's signatures (vlgp_amd._lib.load keeps one library per process)."""
    from vlgp_amd import _lib

    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.vlgp_abi_version() == _lib.ABI_VERSION
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prof-steps", type=int, default=4)
    ap.add_argument("--fraction", type=float, default=0.2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", choices=["unmasked", "masked0", "masked20"], default=None)
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import bench
    from vlgp_amd import _lib
    from vlgp_amd.api import FitSession

    trials, a0, b0, (n_trials, n_bins, N, L) = bench.build_inputs("C3")
    total = args.warmup + args.reps + args.prof_steps + 2
    rng = np.random.default_rng(0)
    masks = {"masked0": [np.zeros(tr["y"].shape, dtype=bool) for tr in trials],
             "masked20": [rng.random(tr["y"].shape) < args.fraction for tr in trials]}
    this_lib = _lib.load()
    names = [args.only] if args.only else ["unmasked", "masked0", "masked20"]
    sessions = {}
    for name in names:
        mine = [{"y": tr["y"], "mu": tr["mu"].copy()} for tr in trials]
        kw = dict(device=0, verbose=False, a=a0.copy(), b=b0.copy(), max_iter=total, min_iter=total)
        if name == "unmasked":
            if args.parent_lib:
                _lib._lib = other_build(args.parent_lib)
            try:
                sessions[name] = FitSession(mine, L, **kw)
            finally:
                _lib._lib = this_lib
        else:
            sessions[name] = FitSession(mine, L, missing=masks[name], **kw)

    def step(sess):
        t0 = time.perf_counter()
        sess.em_iteration()
        sess.eng.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(args.warmup):
        for sess in sessions.values():
            step(sess)
    times = {name: [] for name in sessions}
    for _ in range(args.reps):
        for name, sess in sessions.items():  # alternating
            times[name].append(step(sess))
    launch = {}
    for name, sess in sessions.items():  # per-launch events on: the Newton launches of mstep_accum
        sess.eng.profile(True)
        sess.eng.profile_reset()
        for _ in range(args.prof_steps):
            step(sess)
        n, ms, _ = sess.eng.profile_get(_lib.PROF_MSTEP)
        launch[name] = {"launches": n, "ms_per_launch": ms / max(n, 1)}
        sess.eng.profile(False)
    out = {"shape": [n_trials, n_bins, N, L], "fraction_missing": args.fraction, "reps": args.reps,
           "unmasked_build": args.parent_lib or "this build"}
    for name in sessions:
        out[name] = {"ms_per_em_iteration": statistics.median(times[name]), "runs_ms": [round(t, 3) for t in times[name]],
                     "mstep_accum_newton": launch[name]}
    if "unmasked" in sessions:
        base = out["unmasked"]["ms_per_em_iteration"]
        for name in sessions:
            if name != "unmasked":
                out[name]["ratio_to_unmasked"] = out[name]["ms_per_em_iteration"] / base
                out[name]["launch_ratio_to_unmasked"] = (launch[name]["ms_per_launch"]
                                                         / max(launch["unmasked"]["ms_per_launch"], 1e-300))
    for sess in sessions.values():
        sess.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
