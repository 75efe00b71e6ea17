"""Cost of the per-row covariance of the joint Laplace posterior (vlgp_joint_posterior) beside vlgp_joint_laplace's mu, v,
one speckled fold scored under it end to end, and what the joint posterior does to the held-out scores and to their
calibration beside the mean-field posterior.

The test fold of tools/joint_bench.py: 200 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth), L = 5;
fit on the first 160 for --fit-iters EM iterations, the last 40 held out, their mean-field posterior from a zero start
and --infer-iters E-step iterations.  Prints one JSON line:
- laplace_ms: device-synchronised wall time of Engine.joint_laplace without draws (Newton iteration, stats, mu, v and
  their copies out); posterior_ms: Engine.joint_posterior (the same with cov in place of v: the full-column solves of
  joint_cov and L (L + 1) / 2 doubles per row out); median of --reps after one warm-up call;
- fold_ms: one speckled fold of evaluation's posterior="joint" path on the resident set -- replicate_masked of one
  replica, the E-step, Engine.joint_posterior, the predictive scorer under its mu, cov, free -- and its parts;
  fold_mean_field_ms: the same fold under the mean-field posterior (replicate, E-step, vlgp_predictive, free);
- with --scores: speckled_bps of leave_entries_out(predictive=True) and pit_all, coverage_all, dispersion_all of
  calibration(how="entries") over --folds folds, posterior "mean_field" beside "joint", and the Newton counts.
    python tools/joint_cov_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 5 --fit-iters 30
                                     --infer-iters 50 --folds 5 --scores]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=30)
    ap.add_argument("--infer-iters", type=int, default=50)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--scores", action="store_true")
    args = ap.parse_args()
    from vlgp_amd import evaluation as EV
    from vlgp_amd import fit, synth

    N, L = args.channels, args.latents
    every = synth.make_trials(5 * args.trials, args.bins, N, L, seed=0)
    np.random.seed(0)
    fitted = fit([{"y": t["y"]} for t in every[:4 * args.trials]], L, verbose=False, max_iter=args.fit_iters,
                 min_iter=args.fit_iters)
    params, config = fitted["params"], fitted["config"]
    trials = [{"y": t["y"]} for t in every[4 * args.trials:]]
    rows = args.trials * args.bins
    out = {"trials": args.trials, "bins": args.bins, "channels": N, "latents": L, "fit_iters": args.fit_iters,
           "n_iter": args.infer_iters, "folds": args.folds}
    held = EV.entry_folds(rows, N, args.folds, 0) == 0
    scorer = EV._log_scorer(12)

    def timed(call):
        call()  # warm-up: code object, buffers
        runs = []
        for _ in range(args.reps):
            eng.synchronize()
            t0 = time.perf_counter()
            call()
            eng.synchronize()
            runs.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(runs), [round(r, 4) for r in runs]

    def mean_field_fold():
        return EV._replica_chunk(eng, args.infer_iters, config["dmu_bound"], True, scorer=scorer, held_out=held[None])

    def parts():
        """The steps of _joint_fold, each timed once."""
        t = [time.perf_counter()]

        def lap():
            eng.synchronize()
            t.append(time.perf_counter())
        eng.replicate(EV.SET_TEST, EV.SET_REPLICAS, held_out=held[None])
        lap()
        eng.estep(EV.SET_REPLICAS, args.infer_iters, config["dmu_bound"], True)
        lap()
        joint = eng.joint_posterior(EV.SET_REPLICAS)
        lap()
        scorer(eng, EV.SET_REPLICAS, True, mu=joint["mu"], cov=joint["cov"])
        lap()
        eng.free_units(EV.SET_REPLICAS)
        lap()
        ms = np.diff(t) * 1e3
        return dict(zip(("replicate_ms", "estep_ms", "joint_posterior_ms", "predictive_cov_ms", "free_ms"), ms.round(3).tolist()))

    with EV._resident(trials, params, EV._zero_start(trials, L), 0) as eng:
        out["n_failed_estep"] = int(eng.estep(EV.SET_TEST, args.infer_iters, config["dmu_bound"], True))
        out["laplace_ms"], out["laplace_runs_ms"] = timed(lambda: eng.joint_laplace(EV.SET_TEST))
        out["posterior_ms"], out["posterior_runs_ms"] = timed(lambda: eng.joint_posterior(EV.SET_TEST))
        post = eng.joint_posterior(EV.SET_TEST)
        out.update(D=post["D"].tolist(), n_newton=post["n_newton"].tolist(), n_failed=post["n_failed"])
        a2 = params["a"] ** 2
        full = np.einsum("ln,tlm,mn->tn", params["a"], post["cov"], params["a"])
        diag = np.einsum("ln,tl->tn", a2, np.diagonal(post["cov"], axis1=1, axis2=2))
        ratio = full / diag
        out["s2_full_over_diagonal"] = dict(zip(("min", "q25", "median", "q75", "max"),
                                                np.percentile(ratio, [0, 25, 50, 75, 100]).tolist()))
        eng.upload(EV.SET_TEST, EV._zero_start(trials, L))
        out["fold_ms"], out["fold_runs_ms"] = timed(
            lambda: EV._joint_fold(eng, held, args.infer_iters, config["dmu_bound"], True, scorer))
        out["fold_parts"] = parts()
        out["fold_mean_field_ms"], out["fold_mean_field_runs_ms"] = timed(mean_field_fold)
    if args.scores:
        for posterior in EV.POSTERIORS:
            t0 = time.perf_counter()
            leo = EV.leave_entries_out(trials, params, config, n_folds=args.folds, n_iter=args.infer_iters, predictive=True,
                                       posterior=posterior)
            cal = EV.calibration(trials, params, config, how="entries", n_folds=args.folds, n_iter=args.infer_iters,
                                 posterior=posterior)
            res = {"speckled_bps": leo["speckled_bps"], "ll": float(np.sum(leo["ll"])), "n_failed": leo["n_failed"],
                   "pit_all": cal["pit_all"].tolist(), "pit_max_deviation": float(np.max(np.abs(cal["pit_all"] * 10 - 1.0))),
                   "levels": cal["levels"].tolist(), "coverage_all": cal["coverage_all"].tolist(),
                   "dispersion_all": cal["dispersion_all"], "skipped": int(np.sum(cal["skipped"])),
                   "seconds": round(time.perf_counter() - t0, 2)}
            if posterior == "joint":
                res.update(n_newton_max=int(np.max(leo["n_newton"])), converged=int(np.sum(leo["converged"])),
                           of=int(leo["converged"].size))
            out[posterior] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
