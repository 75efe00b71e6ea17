"""Cost of the calibration sums (vlgp_calibration) beside the posterior-predictive scores (vlgp_predictive) on the same
resident set.

The test set of tools/predictive_bench.py at the headline fold: 40 synthetic trials x 1000 bins x 100 Poisson channels
(vlgp_amd.synth, no fit), L = 5, scored as a plain set and as 5 group replicas (channel folds); the posterior comes from
a zero start and the configuration's E-step iterations, as evaluation.leave_group_out infers it.  Prints one JSON line
(and writes it to --out when given); per set kind
- predictive12_ms, calibration12_ms: device-synchronised wall time of Engine.predictive and Engine.calibration (10 bins,
  levels 0.5 and 0.9, 12 nodes) with the sums alone -- the call's allocation, its launches, the copy of the sums out and
  the wait --, median of --reps after one warm-up call, the calls alternating inside every repetition; *_entries_ms: the
  same asking for the per-entry arrays (predictive: rate and lpd; calibration: cdf);
- entries, mean_count, max_count_seen: the (row, channel) entries a call scores and their counts: an entry costs 1 + y
  masses where vlgp_predictive evaluates one, and the lanes of a wave run to the largest count among their 64 rows;
  mean_wave_max: the mean over the waves (64 consecutive rows of a channel) of that largest count;
- ratio = calibration12_ms / predictive12_ms beside 1 + mean_count and 1 + mean_wave_max;
- summary: pooled PIT histogram, coverage and dispersion of the call, to show what was computed.
    python tools/calibration_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 7 --folds 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -- python tools/calibration_bench.py --only-call
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
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--only-call", action="store_true", help="one warm-up and one timed call of each, for a kernel trace")
    args = ap.parse_args()
    from vlgp_amd import get_config, synth
    from vlgp_amd.evaluation import SET_REPLICAS, SET_TEST, _resident, _zero_start, calibration_from_sums, channel_folds

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L = args.channels, args.latents
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    reps = 1 if args.only_call else args.reps
    rows = args.trials * args.bins
    full = rows - rows % 64  # (a wave: 64 consecutive rows of one channel)
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "n_iter": config["max_iter"],
           "reps": reps, "n_bins": 10, "levels": [0.5, 0.9], "n_nodes": 12, "entries": rows * N,
           "mean_count": float(y.mean()), "max_count_seen": float(y.max()),
           "mean_wave_max": float(y[:full].reshape(-1, 64, N).max(axis=1).mean()),
           "what": "measured wall times, device-synchronised; not targets"}

    def clock(call):
        eng.synchronize()
        t0 = time.perf_counter()
        call()  # (returns after the copy of its results out)
        return 1e3 * (time.perf_counter() - t0)

    def score(set_id):
        calls = {"predictive12": lambda: eng.predictive(set_id, n_nodes=12),
                 "calibration12": lambda: eng.calibration(set_id, n_nodes=12),
                 "predictive12_entries": lambda: eng.predictive(set_id, n_nodes=12, want_rate=True, want_lpd=True),
                 "calibration12_entries": lambda: eng.calibration(set_id, n_nodes=12, want_cdf=True)}
        runs = {name: [] for name in calls}
        for call in calls.values():
            call()  # warm-up: code objects
        for _ in range(reps):
            for name, call in calls.items():
                runs[name].append(clock(call))
        got = {}
        for name, r in runs.items():
            got[name + "_ms"] = statistics.median(r)
            got[name + "_runs_ms"] = [round(t, 4) for t in r]
        got["ratio"] = got["calibration12_ms"] / got["predictive12_ms"]
        got["one_plus_mean_count"] = 1.0 + out["mean_count"]
        got["one_plus_mean_wave_max"] = 1.0 + out["mean_wave_max"]
        cal = calibration_from_sums(calls["calibration12"]()[0], 10, (0.5, 0.9))
        got["summary"] = {"pit_all": [round(float(p), 5) for p in cal["pit_all"]],
                          "coverage_all": [round(float(c), 5) for c in cal["coverage_all"]],
                          "dispersion_all": cal["dispersion_all"], "skipped": int(cal["skipped"].sum())}
        return got

    with _resident(trials, params, _zero_start(trials, L), 0) as eng:
        t = clock(lambda: eng.estep(SET_TEST, config["max_iter"], config["dmu_bound"], True))
        out["plain"] = dict(estep_ms=t, **score(SET_TEST))
        eng.upload(SET_TEST, _zero_start(trials, L))
        eng.replicate(SET_TEST, SET_REPLICAS, groups=channel_folds(N, args.folds, 0))
        t = clock(lambda: eng.estep(SET_REPLICAS, config["max_iter"], config["dmu_bound"], True))
        out["groups_%d" % args.folds] = dict(estep_ms=t, **score(SET_REPLICAS))
        eng.free_units(SET_REPLICAS)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
