"""Cost of the lag moments (vlgp_lag_moments) beside their NumPy statement on the same data.

The headline fold: 160 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth, no fit), L = 5, max_lag = 20,
as a plain set; the posterior comes from a zero start and the configuration's E-step iterations.  Prints one JSON line
(and writes it to --out when given):
- vb_ms, map_ms: device-synchronised wall time of Engine.lag_moments with vb = 1 (all four kernels: lag_rows, lag_task,
  lag_moments, lag_finish) and vb = 0 (the last two alone, without the reads of c) -- the call's allocation, its launches,
  the copy of the three tables out and the wait --, median of --reps after one warm-up call, the calls alternating;
- c_workspace_bytes: rows (max_lag + 1) L doubles;
- numpy_s: one evaluation of tests/lag_numpy.py on the first --numpy-trials trials (the statement is dense per trial), and
  err: max |device - statement| / max(1, largest |statement| entry) per lag of a device call on those trials alone;
- rms_excess_all: of the vb call, to show what was computed.
Per-kernel times come from a kernel trace of this script (profiles/lag_moments/README.md has the command).
    python tools/lag_bench.py [--trials 160 --bins 1000 --channels 100 --latents 5 --max-lag 20 --reps 7] [--out FILE]
Every figure is a measured value on the machine the command ran on, not a target."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=160)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=100)
    ap.add_argument("--latents", type=int, default=5)
    ap.add_argument("--max-lag", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-trials", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import lag_numpy as LN
    from vlgp_amd import get_config, synth
    from vlgp_amd.evaluation import SET_TEST, _lag_summary, _resident, _zero_start

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L, K = args.channels, args.latents, args.max_lag
    y = np.concatenate([t["y"] for t in trials])
    rows = len(y)
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "rows": rows, "max_lag": K,
           "c_workspace_bytes": 8 * rows * (K + 1) * L, "n_iter": config["max_iter"], "reps": args.reps,
           "what": "measured wall times, device-synchronised; not targets"}

    def clock(call):
        eng.synchronize()
        t0 = time.perf_counter()
        call()  # (returns after the copy of its results out)
        return 1e3 * (time.perf_counter() - t0)

    with _resident(trials, params, _zero_start(trials, L), 0) as eng:
        eng.estep(SET_TEST, config["max_iter"], config["dmu_bound"], True)
        post = eng.download(SET_TEST, ("mu", "v"))
        calls = {"vb": lambda: eng.lag_moments(SET_TEST, K, vb=True), "map": lambda: eng.lag_moments(SET_TEST, K, vb=False)}
        dev = {name: call() for name, call in calls.items()}  # warm-up: code objects
        runs = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, call in calls.items():
                runs[name].append(clock(call))
        out["ranks"] = [int(r) for r in eng.prior_ranks(args.bins)]
    for name, r in runs.items():
        out[name + "_ms"] = statistics.median(r)
        out[name + "_runs_ms"] = [round(t, 4) for t in r]
    out["n_failed"] = dev["vb"][3]
    n_np = max(min(args.numpy_trials, args.trials), 1)
    few = [dict(tr, x=None, w=None, mu=post["mu"][i * args.bins:(i + 1) * args.bins], v=post["v"][i * args.bins:(i + 1) * args.bins])
           for i, tr in enumerate(trials[:n_np])]
    par = dict(a=params["a"], b=params["b"], noise=params["noise"], gauss=np.zeros(N, dtype=bool))
    with _resident(few, params, few, 0) as eng:
        small = eng.lag_moments(SET_TEST, K)
        prior = {args.bins: eng.get_prior(args.bins)}
    t0 = time.perf_counter()
    want = LN.lag_moments(few, par, prior, K)
    out["numpy_trials"], out["numpy_s"] = n_np, time.perf_counter() - t0
    out["err"] = max(float(np.max(np.abs(d - w).max(axis=1) / np.maximum(1.0, np.abs(w).max(axis=1))))
                     for d, w in zip(small[:2], want[:2]))
    out["count_equal"] = bool(np.array_equal(small[2], want[2]))
    summary = _lag_summary(*dev["vb"][:3])
    out["rms_excess_all"] = summary["rms_excess_all"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
