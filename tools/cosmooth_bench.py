"""Co-smoothing timing: leave_group_out with a few channel folds against leave_one_out on the same test set.

Synthetic parameters from vlgp_amd.synth (no fit), the shape of tools/loo_bench.py: 40 trials x 1000 bins x 100 Poisson
channels, L = 5, every channel predicted once.  Prints one JSON line: device-synchronised wall time of each call (median
of --reps after one warm-up), the replicas each needed and its score.
    python tools/cosmooth_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 3 --folds 5 10]
    python tools/cosmooth_bench.py --only 5      (one warm-up and one timed 5-fold run, for a kernel trace under rocprofv3)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=100)
    ap.add_argument("--latents", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--folds", type=int, nargs="+", default=[5, 10])
    ap.add_argument("--only", type=int, default=0, help="time this fold count alone, once (0: leave_one_out too)")
    args = ap.parse_args()
    from vlgp_amd import evaluation, get_config, synth

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L = args.channels, args.latents
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    runs = {}
    if not args.only:
        runs["leave_one_out"] = lambda: evaluation.leave_one_out(trials, params, config, path="batched")
    for k in ([args.only] if args.only else args.folds):
        runs["leave_group_out_%d" % k] = (lambda k=k: evaluation.leave_group_out(trials, params, config, n_folds=k,
                                                                                  path="batched"))
    reps = 1 if args.only else args.reps
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "n_iter": config["max_iter"]}
    for name, call in runs.items():
        call()  # warm-up (code objects, allocations)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = call()  # returns after the last device copy
            times.append(time.perf_counter() - t0)
        out[name] = {"s": statistics.median(times), "runs_s": times, "path": res["path"],
                     "replicas": len(res.get("groups", res["channels"])),
                     "mean_bits_per_spike": float(np.nanmean(res["bits_per_spike"]))}
        if "co_bps" in res:
            out[name]["co_bps"] = res["co_bps"]
    if "leave_one_out" in out:
        for name in runs:
            if name != "leave_one_out":
                out[name]["speedup_over_leave_one_out"] = out["leave_one_out"]["s"] / out[name]["s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
