"""Cost of the pair moments (vlgp_pair_moments, vlgp_pair_moments_cov) beside their NumPy statement on the same arrays.

The held-out fold of DESIGN 4.11: 40 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth, no fit),
L = 5, as a plain set; the posterior comes from a zero start and the configuration's E-step iterations.  Prints one JSON
line (and writes it to --out when given):
- own_v_ms, supplied_cov_ms: device-synchronised wall time of Engine.pair_moments under the set's own mu, v and under a
  supplied mu and full covariance per row (diag(v) plus a random positive semi-definite matrix) -- the call's allocation,
  the copy of the moments in, its two launches, the copy of the two matrices out and the wait --, median of --reps after
  one warm-up call, the calls alternating inside every repetition;
- numpy_own_v_s, numpy_supplied_cov_s: one evaluation of tests/pair_numpy.py on the same arrays, in blocks of --block rows
  (the statement holds a (rows, N, N) array);
- err_*: max |device - statement| / max(1, largest |statement| entry) of the two matrices at this size;
- rms_excess: of the own-v call, to show what was computed.
    python tools/pair_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 7] [--out FILE]
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
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=100)
    ap.add_argument("--latents", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--block", type=int, default=2000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import pair_numpy as PN
    from vlgp_amd import get_config, synth
    from vlgp_amd.evaluation import SET_TEST, _pair_summary, _resident, _zero_start

    trials, truth = synth.make_trials(args.trials, args.bins, args.channels, args.latents, seed=0, return_truth=True)
    N, L = args.channels, args.latents
    y = np.concatenate([t["y"] for t in trials])
    rows = len(y)
    params = {"ydim": N, "zdim": L, "xdim": 1, "a": truth["a"], "b": np.log(np.maximum(y.mean(0, keepdims=True), 1e-3)),
              "noise": np.ones(N), "sigma": np.full(L, 1.0), "omega": np.full(L, get_config()["omega_bound"][1]),
              "rank": 50, "likelihood": np.array(["poisson"] * N)}
    config = get_config()
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "rows": rows, "pairs": N * (N + 1) // 2,
           "n_iter": config["max_iter"], "reps": args.reps, "what": "measured wall times, device-synchronised; not targets"}

    def clock(call):
        eng.synchronize()
        t0 = time.perf_counter()
        call()  # (returns after the copy of its results out)
        return 1e3 * (time.perf_counter() - t0)

    with _resident(trials, params, _zero_start(trials, L), 0) as eng:
        eng.estep(SET_TEST, config["max_iter"], config["dmu_bound"], True)
        post = eng.download(SET_TEST, ("mu", "v"))
        rng = np.random.default_rng(1)
        B = 0.1 * rng.standard_normal((rows, L, L))
        cov = PN.diag_cov(post["v"]) + B @ B.transpose(0, 2, 1)
        packed = eng._moments(SET_TEST, post["mu"], cov)[1]
        calls = {"own_v": lambda: eng.pair_moments(SET_TEST, vb=True),
                 "supplied_cov": lambda: eng.pair_moments(SET_TEST, mu=post["mu"], cov=packed)}
        dev = {name: call() for name, call in calls.items()}  # warm-up: code objects
        runs = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, call in calls.items():
                runs[name].append(clock(call))
    for name, r in runs.items():
        out[name + "_ms"] = statistics.median(r)
        out[name + "_runs_ms"] = [round(t, 4) for t in r]
    gauss = np.zeros(N, dtype=bool)
    for name, c in (("own_v", PN.diag_cov(post["v"])), ("supplied_cov", cov)):
        t0 = time.perf_counter()
        want = [np.zeros((N, N)), np.zeros((N, N))]
        for r0 in range(0, rows, args.block):
            sl = slice(r0, r0 + args.block)
            got = PN.pair_moments(y[sl], None, post["mu"][sl], c[sl], params["a"], params["b"], params["noise"], gauss)
            want[0] += got[0]
            want[1] += got[1]
        out["numpy_%s_s" % name] = time.perf_counter() - t0
        out["err_" + name] = max(float(np.abs(d - w).max() / max(1.0, np.abs(w).max())) for d, w in zip(dev[name], want))
    summary = _pair_summary(*dev["own_v"], np.full((N, N), float(rows)))
    out["rms_excess"], out["mean_excess"] = summary["rms_excess"], summary["mean_excess"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
