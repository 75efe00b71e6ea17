"""Leave-one-neuron-out timing: batched (one replicated E-step) against sequential (one E-step per channel).

Synthetic parameters from vlgp_amd.synth (no fit): 40 trials x 1000 bins x 100 Poisson channels, L = 5, omega and
sigma at the defaults, every channel left out.  Prints one JSON line: device-synchronised wall time of each path
(median of --reps after one warm-up), and the largest difference between the two results.
    python tools/loo_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 3] [--path batched]
(--path batched alone: one warm-up and one timed batched run, for a kernel trace under rocprofv3.)"""
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
    ap.add_argument("--path", default="both", choices=("both", "batched", "sequential"))
    args = ap.parse_args()
    from vlgp_amd import evaluation, get_config, synth

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L = args.channels, args.latents
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    paths = ("batched", "sequential") if args.path == "both" else (args.path,)
    reps = args.reps if args.path == "both" else 1
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "n_iter": config["max_iter"]}
    res = {}
    for p in paths:
        evaluation.leave_one_out(trials, params, config, path=p)  # warm-up (code objects, allocations)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res[p] = evaluation.leave_one_out(trials, params, config, path=p)  # returns after the last device copy
            times.append(time.perf_counter() - t0)
        out[p + "_s"] = statistics.median(times)
        out[p + "_runs_s"] = times
        out[p + "_path"] = res[p]["path"]
    if len(res) == 2:
        b, s = res["batched"], res["sequential"]
        out["max_abs_diff_rate"] = max(float(np.max(np.abs(x - z))) for x, z in zip(b["rate"], s["rate"]))
        out["max_abs_diff_ll"] = float(np.max(np.abs(b["ll"] - s["ll"])))
        out["speedup"] = out["sequential_s"] / out["batched_s"]
        out["mean_bits_per_spike"] = float(np.nanmean(b["bits_per_spike"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
