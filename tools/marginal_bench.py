"""Cost of the importance weights of the marginal likelihood (vlgp_marginal) beside the variational bound (vlgp_elbo) on
the same resident set, and how the effective sample size of the estimate is distributed over the trials.

A test fold of the headline workload: 200 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth), L = 5;
fit on the first 160 for --fit-iters EM iterations, the last 40 held out; their posterior comes from a zero start and
--infer-iters E-step iterations, as evaluation.marginal_loglik(infer=True) infers it.  Prints one JSON line:
- marginal_ms / elbo_ms: device-synchronised wall time of Engine.marginal (--samples draws; the copy of the normals in,
  the launches, the copy of log_w out and the wait) and of Engine.elbo, median of --reps after one warm-up call;
- marginal_ns_per_eval / elbo_ns_per_eval: those times per (row, channel, sample) and per (row, channel): whole calls, an
  upper bound of the row kernels' own cost (the kernel times come from a trace, below);
- ess_K64 / ess_K512: min, quartiles and max of the per-trial effective sample size at 64 and 512 draws, with the mean gap
  iwae - elbo_mc per trial.
    python tools/marginal_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --samples 64 --reps 5
                                    --fit-iters 30 --infer-iters 50]
    rocprofv3 --kernel-trace --stats -- python tools/marginal_bench.py --only-call
(--only-call: the inference, one warm-up and one timed call of each, for a kernel trace.)"""
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
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=30)
    ap.add_argument("--infer-iters", type=int, default=50)
    ap.add_argument("--only-call", action="store_true")
    args = ap.parse_args()
    from vlgp_amd import evaluation, fit, synth
    from vlgp_amd.evaluation import SET_TEST, _resident, _zero_start, weights_summary

    N, L, K = args.channels, args.latents, args.samples
    every = synth.make_trials(5 * args.trials, args.bins, N, L, seed=0)
    np.random.seed(0)
    fitted = fit([{"y": t["y"]} for t in every[:4 * args.trials]], L, verbose=False, max_iter=args.fit_iters,
                 min_iter=args.fit_iters)
    params, config = fitted["params"], fitted["config"]
    trials = [{"y": t["y"]} for t in every[4 * args.trials:]]
    rows = args.trials * args.bins
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "samples": K,
           "fit_iters": args.fit_iters, "n_iter": args.infer_iters, "omega": np.asarray(params["omega"]).tolist()}
    reps = 1 if args.only_call else args.reps
    rng = np.random.default_rng(0)

    def timed(call):
        call()  # warm-up: code object, buffers
        runs = []
        for _ in range(reps):
            eng.synchronize()
            t0 = time.perf_counter()
            call()
            runs.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(runs), [round(r, 4) for r in runs]

    with _resident(trials, params, _zero_start(trials, L), 0) as eng:
        out["n_failed_estep"] = int(eng.estep(SET_TEST, args.infer_iters, config["dmu_bound"], True))
        out["ranks"] = eng.unit_ranks(SET_TEST).max(axis=0).tolist()
        # how far the inferred posterior is from the E-step's fixed point: |G m - mu|^2 / |mu|^2 (vlgp_forecast's report)
        terms = eng.forecast(SET_TEST, {args.bins: eng.get_prior(args.bins)[:, -1:, :]})[2]
        out["off_fixed_point_max"] = float(np.max(terms[:, :, 0] / terms[:, :, 1]))
        eps = rng.standard_normal((args.trials, L, 50, K))
        out["marginal_ms"], out["marginal_runs_ms"] = timed(lambda: eng.marginal(SET_TEST, eps))
        out["elbo_ms"], out["elbo_runs_ms"] = timed(lambda: eng.elbo(SET_TEST))
        out["marginal_ns_per_eval"] = 1e6 * out["marginal_ms"] / (rows * N * K)
        out["elbo_ns_per_eval"] = 1e6 * out["elbo_ms"] / (rows * N)
        if not args.only_call:
            log_w = np.concatenate([eng.marginal(SET_TEST, rng.standard_normal((args.trials, L, 50, 64)))[0]
                                    for _ in range(8)], axis=1)
            for n in (64, 512):
                iwae, mc, ess = weights_summary(log_w[:, :n])
                q = np.percentile(ess, [0, 25, 50, 75, 100])
                out["ess_K%d" % n] = {"min": q[0], "q25": q[1], "median": q[2], "q75": q[3], "max": q[4],
                                      "median_std_log_w": float(np.median(np.std(log_w[:, :n], axis=1))),
                                      "mean_gap_iwae_minus_elbo_mc": float(np.mean(iwae - mc)),
                                      "total_elbo_mc": float(np.sum(mc)),
                                      "total_iwae": float(np.sum(iwae))}
            tot = evaluation.elbo_from_terms(*eng.elbo(SET_TEST)[:2], eng.unit_ranks(SET_TEST))
            out["elbo"] = tot["elbo"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
