"""Forward-prediction timing: evaluation.forward_prediction on a synthetic test set.

Synthetic parameters from vlgp_amd.synth (no fit), the shape the issue names: 200 trials x 1000 bins x 100 Poisson
channels, L = 5, the last 100 bins of every trial predicted from the first 900.  Prints one JSON line: the wall time of the
whole call (median of --reps after one warm-up; it returns after the last device copy), and of its device part alone --
Engine.forecast on the resident held-in set (launches, the copies of G_ext in and of the results out, the wait), median
of --reps after one warm-up -- with the ranks of the held-in prior.
    python tools/forward_bench.py [--trials 200 --bins 1000 --channels 100 --latents 5 --forward 100 --reps 3]
    python tools/forward_bench.py --only-call    (one warm-up and one timed call, for a kernel trace under rocprofv3)"""
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
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=100)
    ap.add_argument("--latents", type=int, default=5)
    ap.add_argument("--forward", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-call", action="store_true")
    args = ap.parse_args()
    from vlgp_amd import evaluation, get_config, synth
    from vlgp_amd.api import SET_TRIALS, _extended

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L, nf = args.channels, args.latents, args.forward
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "n_forward": nf,
           "n_iter": config["max_iter"]}
    reps = 1 if args.only_call else args.reps

    def call():
        return evaluation.forward_prediction(trials, params, config, nf)

    call()  # warm-up (code objects, allocations)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    out["forward_prediction_s"] = statistics.median(times)
    out["forward_prediction_runs_s"] = times
    out.update(fp_bps=res["fp_bps"], fp_bps_past=res["fp_bps_past"], n_failed=res["n_failed"],
               off_fixed_point_max=float(np.max(res["off_fixed_point"])))
    if not args.only_call:
        T_in = args.bins - nf
        ext = {T_in: np.ascontiguousarray(_full(args.bins, params)[:, T_in:])}
        with _extended(trials, [T_in] * args.trials, nf, params, config, None, 0) as (eng, _, _, _, _):
            out["ranks_held_in"] = [int(r) for r in eng.prior_ranks(T_in)]
            runs = []
            for _ in range(reps):
                eng.synchronize()
                t0 = time.perf_counter()
                eng.forecast(SET_TRIALS, ext)
                runs.append(1e3 * (time.perf_counter() - t0))
            out["engine_forecast_ms"] = statistics.median(runs)
            out["engine_forecast_runs_ms"] = [round(r, 4) for r in runs]
    print(json.dumps(out))


def _full(T, params):
    """The factor of length T as forward_prediction builds it (on an engine of its own: the timed one keeps its priors)."""
    from vlgp_amd import Engine

    with Engine.for_params(params) as other:
        other.build_prior([T], params["omega"], params["sigma"])
        return other.get_prior(T)


if __name__ == "__main__":
    main()
