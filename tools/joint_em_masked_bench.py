"""What the mask costs the covariance M-step and a Laplace EM iteration (vlgp_mstep_cov_masked, refit_joint(missing=)), at
the fold of DESIGN.md 4.16.  Reported, not gated.

The fold of tools/joint_em_bench.py: 160 synthetic training trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth),
L = 5, a mean-field fit of --fit-iters EM iterations for the parameters and the start.  Three variants resident on one
handle, timed alternately in every repetition, device-synchronised, median of --reps:
  unmasked      Engine.joint_posterior + Engine.mstep_cov on the plain set
  masked_empty  Engine.joint_posterior + Engine.mstep_cov_masked on a masked fit set with no bit set
  masked_20     the same with 20 % of the entries missing at random
Per variant mstep_ms (packing, the upload of mu | cov and config["Mniter"] Newton iterations), posterior_ms and
iteration_ms (posterior + evidence + M-step + get_params: one iteration of refit_joint's loop).  The M-step of every
variant takes the moments of its own posterior; every repetition starts from the same parameters.
Writes <out>/joint_em_masked_bench.json (default profiles/joint_em_masked) and prints the JSON line.
    python tools/joint_em_masked_bench.py [--trials 160 --bins 1000 --channels 100 --latents 5 --reps 5 --fit-iters 30
                                           --fraction 0.2 --out profiles/joint_em_masked]"""
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
    ap.add_argument("--trials", type=int, default=160)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=100)
    ap.add_argument("--latents", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=30)
    ap.add_argument("--fraction", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_em_masked"))
    args = ap.parse_args()

    import vlgp_amd as V
    from vlgp_amd import api, synth
    from vlgp_amd import engine as E

    N, L = args.channels, args.latents
    every = synth.make_trials(args.trials, args.bins, N, L, seed=0)
    np.random.seed(0)
    fitted = V.fit([{"y": t["y"]} for t in every], L, verbose=False, max_iter=args.fit_iters, min_iter=args.fit_iters)
    params, config, train = fitted["params"], fitted["config"], fitted["trials"]
    rows = sum(tr["y"].shape[0] for tr in train)
    out = {"train_trials": len(train), "bins": args.bins, "channels": N, "latents": L, "fit_iters": args.fit_iters,
           "Mniter": int(config["Mniter"]), "reps": args.reps, "fraction": args.fraction}
    m_args = (int(config["Mniter"]), config["use_hessian"], config["eps"], config["learning_rate"], config["da_bound"],
              config["db_bound"])
    rng = np.random.default_rng(1)
    masks = {"masked_empty": np.zeros((rows, N), bool), "masked_20": rng.random((rows, N)) < args.fraction}
    variants = ("unmasked", "masked_empty", "masked_20")
    sets = {"unmasked": 0, "masked_empty": 2, "masked_20": 3}
    times = {v: {"posterior_ms": [], "mstep_ms": [], "iteration_ms": []} for v in variants}
    with E.Engine.for_params(params, 0) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, [{k: tr.get(k) for k in ("y", "x", "mu", "v", "w")} for tr in train])
        for name, mask in masks.items():
            eng.replicate(0, sets[name], held_out=mask[None])
        api.bind_priors(eng, train, dict(params))
        for rep in range(args.reps + 1):  # (the first is the warm-up: code objects, buffers)
            for name in variants:
                sid = sets[name]
                mstep = eng.mstep_cov if name == "unmasked" else eng.mstep_cov_masked
                eng.set_params(params["a"], params["b"], params["noise"])
                eng.synchronize()
                t0 = time.perf_counter()
                post = eng.joint_posterior(sid)
                eng.synchronize()
                t1 = time.perf_counter()
                evidence = float(np.sum(post["laplace"]))
                t2 = time.perf_counter()
                bad = mstep(sid, post["mu"], post["cov"], *m_args)
                eng.synchronize()
                t3 = time.perf_counter()
                eng.get_params()
                t4 = time.perf_counter()
                if rep:
                    times[name]["posterior_ms"].append(1e3 * (t1 - t0))
                    times[name]["mstep_ms"].append(1e3 * (t3 - t2))
                    times[name]["iteration_ms"].append(1e3 * (t4 - t0))
                out[name] = {"evidence": evidence, "n_newton_max": int(np.max(post["n_newton"])), "n_failed": int(post["n_failed"]),
                             "mstep_singular": int(bad)}
    for name in variants:
        for k, runs in times[name].items():
            out[name][k] = round(statistics.median(runs), 3)
            out[name][k.replace("_ms", "_runs_ms")] = [round(r, 3) for r in runs]
    base = out["unmasked"]
    for name in variants[1:]:
        out[name]["mstep_vs_unmasked"] = round(out[name]["mstep_ms"] / base["mstep_ms"], 4)
        out[name]["iteration_vs_unmasked"] = round(out[name]["iteration_ms"] / base["iteration_ms"], 4)
    line = json.dumps(out)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "joint_em_masked_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
