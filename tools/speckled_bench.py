"""Speckled hold-out timing: leave_entries_out with 5 entry folds against leave_group_out with 5 channel folds on the
test set of tools/cosmooth_bench.py (40 trials x 1000 bins x 100 Poisson channels, L = 5, synthetic parameters), the two
calls alternating in one process.  Prints one JSON line: device-synchronised wall time of each call (median of --reps
after one warm-up each), their ratio and the scores.
    python tools/speckled_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 3 --folds 5]
    python tools/speckled_bench.py --only entries     (one warm-up and one timed call, for a kernel trace under rocprofv3)"""
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
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--only", choices=["entries", "groups"], default=None)
    args = ap.parse_args()
    from vlgp_amd import evaluation, get_config, synth

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L = args.channels, args.latents
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    calls = {"groups": lambda: evaluation.leave_group_out(trials, params, config, n_folds=args.folds, path="batched"),
             "entries": lambda: evaluation.leave_entries_out(trials, params, config, n_folds=args.folds)}
    if args.only:
        calls = {args.only: calls[args.only]}
    times = {name: [] for name in calls}
    res = {}
    for call in calls.values():
        call()  # warm-up (code objects, allocations)
    for _ in range(1 if args.only else args.reps):
        for name, call in calls.items():  # alternating
            t0 = time.perf_counter()
            res[name] = call()  # returns after the last device copy
            times[name].append(time.perf_counter() - t0)
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "n_iter": config["max_iter"],
           "folds": args.folds}
    for name in calls:
        score = res[name]["co_bps" if name == "groups" else "speckled_bps"]
        out[name] = {"s": statistics.median(times[name]), "runs_s": times[name], "score_bps": score,
                     "n_failed": res[name]["n_failed"]}
    if not args.only:
        out["entries_over_groups"] = out["entries"]["s"] / out["groups"]["s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
