"""Cost of the posterior-predictive scores (vlgp_predictive) at 12 and 20 quadrature nodes beside the plug-in scores
(vlgp_loglik) on the same resident set.

The test set of tools/cosmooth_bench.py: 40 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth, no fit),
L = 5, scored as a plain set and as 5 group replicas (channel folds); the posterior comes from a zero start and the
configuration's E-step iterations, as evaluation.leave_group_out infers it.  Prints one JSON line; per set kind
- estep_ms: device-synchronised wall time of the inference that precedes the scores (one call);
- loglik_ms, predictive12_ms, predictive20_ms: device-synchronised wall time of Engine.loglik and Engine.predictive
  with the sums alone -- the call's allocation, its launches, the copy of the sums out and the wait --, median of --reps
  after one warm-up call, the three calls alternating inside every repetition; *_rate_ms: the same asking for the
  per-entry arrays (loglik: rate; predictive: rate and lpd), which adds their device-to-host copies;
- entries: the (row, channel) entries a call scores, and predictive*_ns_per_entry from the sums-only time.
The kernels' own times come from a trace of one call each:
    python tools/predictive_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 7 --folds 5]
    rocprofv3 --kernel-trace --stats -- python tools/predictive_bench.py --only-call
Every figure is a measured value on the machine the command ran on, not a target."""
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
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-call", action="store_true", help="one warm-up and one timed call of each, for a kernel trace")
    args = ap.parse_args()
    from vlgp_amd import get_config, synth
    from vlgp_amd.evaluation import SET_REPLICAS, SET_TEST, _resident, _zero_start, channel_folds

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L = args.channels, args.latents
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    reps = 1 if args.only_call else args.reps
    rows = args.trials * args.bins
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "n_iter": config["max_iter"],
           "reps": reps, "what": "measured wall times, device-synchronised; not targets"}

    def clock(call):
        eng.synchronize()
        t0 = time.perf_counter()
        call()  # (returns after the copy of its results out)
        return 1e3 * (time.perf_counter() - t0)

    def score(set_id, entries):
        calls = {"loglik": lambda: eng.loglik(set_id), "predictive12": lambda: eng.predictive(set_id, n_nodes=12),
                 "predictive20": lambda: eng.predictive(set_id, n_nodes=20),
                 "loglik_rate": lambda: eng.loglik(set_id, want_rate=True),
                 "predictive12_rate": lambda: eng.predictive(set_id, n_nodes=12, want_rate=True, want_lpd=True),
                 "predictive20_rate": lambda: eng.predictive(set_id, n_nodes=20, want_rate=True, want_lpd=True)}
        runs = {name: [] for name in calls}
        for call in calls.values():
            call()  # warm-up: code objects
        for _ in range(reps):
            for name, call in calls.items():
                runs[name].append(clock(call))
        got = {"entries": entries}
        for name, r in runs.items():
            got[name + "_ms"] = statistics.median(r)
            got[name + "_runs_ms"] = [round(t, 4) for t in r]
        for n in (12, 20):
            got["predictive%d_ns_per_entry" % n] = 1e6 * got["predictive%d_ms" % n] / entries
        ll, lpd = calls["loglik"]()[0][:, 0].sum(), calls["predictive20"]()[0][:, 0].sum()
        got["sum_ll"], got["sum_lpd20"] = float(ll), float(lpd)
        return got

    with _resident(trials, params, _zero_start(trials, L), 0) as eng:
        t = clock(lambda: eng.estep(SET_TEST, config["max_iter"], config["dmu_bound"], True))
        out["plain"] = dict(estep_ms=t, **score(SET_TEST, rows * N))
        eng.upload(SET_TEST, _zero_start(trials, L))
        eng.replicate(SET_TEST, SET_REPLICAS, groups=channel_folds(N, args.folds, 0))
        t = clock(lambda: eng.estep(SET_REPLICAS, config["max_iter"], config["dmu_bound"], True))
        out["groups_%d" % args.folds] = dict(estep_ms=t, **score(SET_REPLICAS, rows * N))
        eng.free_units(SET_REPLICAS)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
