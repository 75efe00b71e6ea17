"""Cost of the joint Laplace posterior (vlgp_joint_laplace) on a held-out fold, and what its proposal does to the effective
sample size of the importance-weighted marginal likelihood beside the mean-field proposal of vlgp_marginal.

A test fold of the headline workload: 200 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth), L = 5;
fit on the first 160 for --fit-iters EM iterations, the last 40 held out; their mean-field posterior comes from a zero
start and --infer-iters E-step iterations, as evaluation.marginal_loglik(infer=True) infers it.  Prints one JSON line:
- mode_ms: device-synchronised wall time of Engine.joint_laplace without draws (the Newton iteration, stats, mu, v and
  their copies out), joint_ms: with --samples draws, marginal_ms: Engine.marginal on the same normals; median of --reps
  after one warm-up call;
- D, n_newton, converged, the final decrements;
- ess_joint / ess_posterior: min, quartiles and max of the per-trial effective sample size of the two proposals on the
  same normals, and how many trials sit below 1.5;
- laplace beside iwae of both proposals, per trial and in total.
    python tools/joint_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --samples 64 --reps 5
                                 --fit-iters 30 --infer-iters 50]
    rocprofv3 --kernel-trace --stats -- python tools/joint_bench.py --only-call
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
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--only-call", action="store_true")
    args = ap.parse_args()
    from vlgp_amd import fit, synth
    from vlgp_amd.evaluation import SET_TEST, _resident, _zero_start, weights_summary

    N, L, K = args.channels, args.latents, args.samples
    every = synth.make_trials(5 * args.trials, args.bins, N, L, seed=0)
    np.random.seed(0)
    fitted = fit([{"y": t["y"]} for t in every[:4 * args.trials]], L, verbose=False, max_iter=args.fit_iters,
                 min_iter=args.fit_iters)
    params, config = fitted["params"], fitted["config"]
    trials = [{"y": t["y"]} for t in every[4 * args.trials:]]
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "samples": K,
           "fit_iters": args.fit_iters, "n_iter": args.infer_iters, "max_iter": args.max_iter, "tol": args.tol,
           "omega": np.asarray(params["omega"]).tolist()}
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

    def spread(ess):
        q = np.percentile(ess, [0, 25, 50, 75, 100])
        return {"min": q[0], "q25": q[1], "median": q[2], "q75": q[3], "max": q[4], "below_1.5": int(np.sum(ess < 1.5))}

    with _resident(trials, params, _zero_start(trials, L), 0) as eng:
        out["n_failed_estep"] = int(eng.estep(SET_TEST, args.infer_iters, config["dmu_bound"], True))
        out["ranks"] = eng.unit_ranks(SET_TEST).max(axis=0).tolist()
        eps = rng.standard_normal((args.trials, L, int(params["rank"]), K))
        kw = {"max_iter": args.max_iter, "tol": args.tol}
        out["mode_ms"], out["mode_runs_ms"] = timed(lambda: eng.joint_laplace(SET_TEST, **kw))
        out["joint_ms"], out["joint_runs_ms"] = timed(lambda: eng.joint_laplace(SET_TEST, eps=eps, **kw))
        out["marginal_ms"], out["marginal_runs_ms"] = timed(lambda: eng.marginal(SET_TEST, eps))
        if not args.only_call:
            joint = eng.joint_laplace(SET_TEST, eps=eps, **kw)
            log_w_mf = eng.marginal(SET_TEST, eps)[0]
            iwae_j, _, ess_j = weights_summary(joint["log_w"])
            iwae_m, _, ess_m = weights_summary(log_w_mf)
            out.update(D=joint["D"].tolist(), n_newton=joint["n_newton"].tolist(), n_failed=joint["n_failed"],
                       converged=int(np.sum(joint["converged"])), decrement_max=float(np.max(joint["decrement"])),
                       ess_joint=spread(ess_j), ess_posterior=spread(ess_m),
                       std_log_w_joint=float(np.median(np.std(joint["log_w"], axis=1))),
                       std_log_w_posterior=float(np.median(np.std(log_w_mf, axis=1))),
                       total_laplace=float(np.sum(joint["laplace"])), total_iwae_joint=float(np.sum(iwae_j)),
                       total_iwae_posterior=float(np.sum(iwae_m)),
                       laplace=joint["laplace"].tolist(), iwae_joint=iwae_j.tolist(), iwae_posterior=iwae_m.tolist(),
                       ess_joint_per_trial=ess_j.tolist(), ess_posterior_per_trial=ess_m.tolist())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
