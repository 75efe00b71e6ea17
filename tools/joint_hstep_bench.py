"""What the hyperparameter step of the Laplace EM (vlgp_amd.refit_joint(..., hstep=True)) costs and what it does, at the
fold of DESIGN.md 4.16.  Reported, not gated.

The fold of tools/joint_em_bench.py: 200 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth), L = 5; fit
on the first 160 for --fit-iters EM iterations, the last 40 held out.  Two sets of numbers:
- per iteration of the loop on the 160 training trials, device-synchronised, the variants alternating in every
  repetition, median of --reps: posterior_ms (Engine.joint_posterior), posterior_window_ms (the same call with
  window=config["window"]: the window moments on top), mstep_cov_ms, optimize_ms (gp.optimize_joint on the host),
  prior_ms (Engine.build_prior for the new omega and the download of the factors), iteration_ms (E-step with moments,
  M-step, optimiser, prior);
- refit_joint with and without hstep from the same mean-field fit: the evidence and omega traces, and on the 40 held-out
  trials the sum of the Laplace evidence and marginal_bps of marginal_loglik(proposal="joint").
Writes profiles/joint_hstep/joint_hstep_bench.json and prints the JSON line.
    python tools/joint_hstep_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 5 --fit-iters 30
                                       --refit-iters 10 --samples 64]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=100)
    ap.add_argument("--latents", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=30)
    ap.add_argument("--refit-iters", type=int, default=10)
    ap.add_argument("--samples", type=int, default=64)
    args = ap.parse_args()

    import vlgp_amd as V
    from vlgp_amd import api, evaluation as EV, gp, synth
    from vlgp_amd import engine as E

    N, L = args.channels, args.latents
    every = synth.make_trials(5 * args.trials, args.bins, N, L, seed=0)
    np.random.seed(0)
    fitted = V.fit([{"y": t["y"]} for t in every[:4 * args.trials]], L, verbose=False, max_iter=args.fit_iters,
                   min_iter=args.fit_iters)
    params, config, train = fitted["params"], fitted["config"], fitted["trials"]
    test = [{"y": t["y"]} for t in every[4 * args.trials:]]
    window = int(config["window"])
    out = {"train_trials": len(train), "test_trials": len(test), "bins": args.bins, "channels": N, "latents": L,
           "rank": int(params["rank"]), "window": window, "fit_iters": args.fit_iters, "refit_iters": args.refit_iters,
           "samples": args.samples, "Mniter": int(config["Mniter"]), "reps": args.reps,
           "omega_mean_field": np.asarray(params["omega"]).tolist()}

    m_args = (int(config["Mniter"]), config["use_hessian"], config["eps"], config["learning_rate"], config["da_bound"],
              config["db_bound"])
    names = ("posterior_ms", "posterior_window_ms", "mstep_cov_ms", "optimize_ms", "prior_ms", "iteration_ms")
    pieces = {k: [] for k in names}
    lengths = sorted({int(tr["y"].shape[0]) for tr in train})
    with E.Engine.for_params(params, 0) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, [{k: tr.get(k) for k in ("y", "x", "mu", "v", "w")} for tr in train])
        bound = dict(params)
        api.bind_priors(eng, train, bound)
        for rep in range(args.reps + 1):  # (the first is the warm-up: code objects, buffers)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.joint_posterior(0)
            eng.synchronize()
            t1 = time.perf_counter()
            post = eng.joint_posterior(0, window=window)
            eng.synchronize()
            t2 = time.perf_counter()
            eng.mstep_cov(0, post["mu"], post["cov"], *m_args)
            eng.synchronize()
            t3 = time.perf_counter()
            omega, reached = gp.optimize_joint(post["window_moments"], post["n_windows"], params, config)
            t4 = time.perf_counter()
            eng.build_prior(lengths, omega, params["sigma"])
            factors = {T: eng.get_prior(T) for T in lengths}
            eng.synchronize()
            t5 = time.perf_counter()
            for T in lengths:  # every repetition from the same parameters and factors
                eng.set_prior(T, bound["cholesky"][T])
            eng.set_params(params["a"], params["b"], params["noise"])
            if rep:
                for k, dt in zip(names, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t5 - t1)):
                    pieces[k].append(1e3 * dt)
        out["n_windows"] = int(post["n_windows"])
        out["n_newton_max"] = int(np.max(post["n_newton"]))
        out["omega_first_step"] = np.asarray(omega).tolist()
        out["factor_bytes"] = int(sum(G.nbytes for G in factors.values()))
    for k, runs in pieces.items():
        out[k] = round(statistics.median(runs), 3)
        out[k.replace("_ms", "_runs_ms")] = [round(r, 3) for r in runs]

    for tag, kw in (("refit_joint", {}), ("refit_joint_hstep", {"hstep": True})):
        t0 = time.perf_counter()
        refit = V.refit_joint(train, params, config, max_iter=args.refit_iters, verbose=False, **kw)
        trace = refit["config"]["runtime"]["joint"]
        out[tag] = {"seconds": round(time.perf_counter() - t0, 2), "laplace": trace["laplace"], "n_newton": trace["n_newton"],
                    "converged": [bool(c) for c in trace["converged"]],
                    "omega": [np.asarray(o).tolist() for o in trace.get("omega", [])],
                    "omega_returned": np.asarray(refit["params"]["omega"]).tolist()}
        jp = EV.joint_posterior(test, refit["params"], config)
        ml = EV.marginal_loglik(test, refit["params"], config, n_samples=args.samples, proposal="joint")
        out[tag]["held_out"] = {"laplace_total": jp["total"], "marginal_bps": ml["marginal_bps"],
                                "ess_median": float(np.median(ml["ess"])), "n_failed": int(jp["n_failed"]) + int(ml["n_failed"])}
    jp = EV.joint_posterior(test, params, config)
    ml = EV.marginal_loglik(test, params, config, n_samples=args.samples, proposal="joint")
    out["mean_field_fit"] = {"held_out": {"laplace_total": jp["total"], "marginal_bps": ml["marginal_bps"],
                                          "ess_median": float(np.median(ml["ess"])),
                                          "n_failed": int(jp["n_failed"]) + int(ml["n_failed"])}}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles", "joint_hstep"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "joint_hstep", "joint_hstep_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
