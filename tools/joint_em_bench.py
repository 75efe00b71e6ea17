"""What a Laplace EM iteration (vlgp_amd.refit_joint) costs and what it buys, at the headline fold of DESIGN.md 4.11.
Reported, not gated.

The fold of tools/joint_bench.py: 200 synthetic trials x 1000 bins x 100 Poisson channels (vlgp_amd.synth), L = 5; fit on
the first 160 for --fit-iters EM iterations, the last 40 held out.  Two sets of numbers:
- per iteration of the loop on the 160 training trials, device-synchronised, median of --reps: joint_posterior_ms
  (Engine.joint_posterior: the Newton E-step and mu, cov out), mstep_cov_ms (Engine.mstep_cov: packing, the upload of
  mu | cov and config["Mniter"] Newton iterations of vlgp_mstep_cov), upload_ms (a pageable host-to-device copy of the bytes
  of mu | cov, timed apart: the hand-over through the host that moments kept on the device would save), rest_ms (what is
  left of the iteration: the evidence, get_params);
- on the 40 held-out trials, the sum of the Laplace evidence (evaluation.joint_posterior) and marginal_bps of
  marginal_loglik(proposal="joint") under the mean-field fit's parameters and under the refitted ones.
Writes profiles/joint_em/joint_em_bench.json and profiles/joint_em/README.md, and prints the JSON line.
    python tools/joint_em_bench.py [--trials 40 --bins 1000 --channels 100 --latents 5 --reps 5 --fit-iters 30
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

README = """# Laplace EM (`vlgp_mstep_cov`, `vlgp_amd.refit_joint`)

| file | how it was made | what it shows |
|---|---|---|
| `joint_em_bench.json` | `python tools/joint_em_bench.py` on one MI355X | the numbers below |
| `measured_errors.txt` | `tests/test_gpu_joint_em.py -s` on one MI355X | every case's largest error against the NumPy statement (the `diag-*` cases against `vlgp_mstep`); the tests hold a hundred times the largest |
| `resource_usage.txt` | `tools/resource_usage.py --all vlgp_amd/csrc/mstep.hip` | registers, scratch and occupancy of every `mstep_cov_accum<LT, PT>`: no scratch and at most 128 VGPRs for `LT <= 5, PT <= 2` |
| `device_code_compare.txt` | `tools/compare_device_code.py` on `--save-temps` builds of the parent and of this commit | every pre-existing kernel identical in body and descriptor |
| `bench_ab.jsonl` | `python bench.py --gpus 1 --steps 20 --warmup 5` in the parent's tree and this one alternately on one box, parent first, three runs each | the headline did not move beyond the parent's own spread |

## `joint_em_bench.json`

%s
"""


def write_readme(out):
    """profiles/joint_em/README.md from the numbers of one run."""
    tr = out["refit_trace"]
    n_it = len(tr["laplace"]) - 1
    if n_it >= 1 and tr["laplace"][-1] < tr["laplace"][-2]:
        stop = ("the evidence of the training trials fell at iteration %d (%.1f after %.1f, Newton counts %s, converged %s), so "
                "the loop returned the parameters and the posterior of iteration %d: for Poisson channels the Laplace evidence "
                "is no bound that the M-step's expected log-likelihood would raise, and nothing guarantees the ascent"
                % (n_it, tr["laplace"][-1], tr["laplace"][-2], tr["n_newton"], [int(c) for c in tr["converged"]], n_it - 1))
    else:
        stop = "the loop stopped at iteration %d (evidence %.1f)" % (n_it, tr["laplace"][-1])
    a, b = out["mean_field_fit"], out["refit_joint"]
    table = "\n".join([
        "%d training trials x %d bins x %d channels, L = %d, Mniter = %d; median of %d, ms per iteration of the loop:"
        % (out["train_trials"], out["bins"], out["channels"], out["latents"], out["Mniter"], out["reps"]), "",
        "| `joint_posterior` | `mstep_cov` (packing, upload, Newton iterations) | of which a host-to-device copy of `mu`, `cov` (%.1f MB), timed apart | rest | iteration |"
        % (out["moment_bytes"] / 1e6), "|---|---|---|---|---|",
        "| %.1f | %.1f | %.1f | %.1f | %.1f |" % tuple(out[k] for k in ("joint_posterior_ms", "mstep_cov_ms", "upload_ms", "rest_ms", "iteration_ms")),
        "", "`refit_joint(max_iter=%d)` from the mean-field fit of %d EM iterations: evidence of the training trials %s; %s."
        % (out["refit_iters"], out["fit_iters"], " -> ".join("%.1f" % e for e in tr["laplace"]), stop),
        "", "On the %d held-out trials:" % out["test_trials"],
        "", "| parameters | sum of `laplace` | `marginal_bps(proposal=\"joint\")` | median ESS of %d |" % out["samples"], "|---|---|---|---|",
        "| the mean-field fit's | %.2f | %.4f | %.1f |" % (a["laplace_total"], a["marginal_bps"], a["ess_median"]),
        "| refitted | %.2f | %.4f | %.1f |" % (b["laplace_total"], b["marginal_bps"], b["ess_median"])])
    with open(os.path.join(ROOT, "profiles", "joint_em", "README.md"), "w") as f:
        f.write(README % table)


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
    ap.add_argument("--readme-only", action="store_true", help="rewrite the README from the JSON file of an earlier run")
    args = ap.parse_args()
    if args.readme_only:
        write_readme(json.load(open(os.path.join(ROOT, "profiles", "joint_em", "joint_em_bench.json"))))
        return
    import torch

    import vlgp_amd as V
    from vlgp_amd import api, evaluation as EV, synth
    from vlgp_amd import engine as E

    N, L = args.channels, args.latents
    every = synth.make_trials(5 * args.trials, args.bins, N, L, seed=0)
    np.random.seed(0)
    fitted = V.fit([{"y": t["y"]} for t in every[:4 * args.trials]], L, verbose=False, max_iter=args.fit_iters,
                   min_iter=args.fit_iters)
    params, config, train = fitted["params"], fitted["config"], fitted["trials"]
    test = [{"y": t["y"]} for t in every[4 * args.trials:]]
    out = {"train_trials": len(train), "test_trials": len(test), "bins": args.bins, "channels": N, "latents": L,
           "fit_iters": args.fit_iters, "refit_iters": args.refit_iters, "samples": args.samples, "Mniter": int(config["Mniter"]),
           "reps": args.reps}

    # ---- one iteration of the loop, piece by piece
    m_args = (int(config["Mniter"]), config["use_hessian"], config["eps"], config["learning_rate"], config["da_bound"],
              config["db_bound"])
    pieces = {k: [] for k in ("joint_posterior_ms", "mstep_cov_ms", "upload_ms", "rest_ms", "iteration_ms")}
    with E.Engine.for_params(params, 0) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(0, [{k: tr.get(k) for k in ("y", "x", "mu", "v", "w")} for tr in train])
        api.bind_priors(eng, train, dict(params))
        for rep in range(args.reps + 1):  # (the first is the warm-up: code objects, buffers)
            eng.synchronize()
            t0 = time.perf_counter()
            post = eng.joint_posterior(0)
            eng.synchronize()
            t1 = time.perf_counter()
            evidence = float(np.sum(post["laplace"]))
            t2 = time.perf_counter()
            eng.mstep_cov(0, post["mu"], post["cov"], *m_args)
            eng.synchronize()
            t3 = time.perf_counter()
            eng.get_params()
            t4 = time.perf_counter()
            packed = E.pack_cov(post["cov"], post["mu"].shape[0], L)
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            held = [torch.from_numpy(arr).to("cuda") for arr in (post["mu"], packed)]
            torch.cuda.synchronize()
            t6 = time.perf_counter()
            del held
            eng.set_params(params["a"], params["b"], params["noise"])  # every repetition from the same parameters
            if rep:
                pieces["joint_posterior_ms"].append(1e3 * (t1 - t0))
                pieces["mstep_cov_ms"].append(1e3 * (t3 - t2))
                pieces["upload_ms"].append(1e3 * (t6 - t5))
                pieces["rest_ms"].append(1e3 * ((t2 - t1) + (t4 - t3)))
                pieces["iteration_ms"].append(1e3 * (t4 - t0))
        out["moment_bytes"] = int(post["mu"].nbytes + packed.nbytes)
        out["n_newton_max"] = int(np.max(post["n_newton"]))
        out["evidence_train_start"] = evidence
    for k, runs in pieces.items():
        out[k] = round(statistics.median(runs), 3)
        out[k.replace("_ms", "_runs_ms")] = [round(r, 3) for r in runs]

    # ---- what the refit buys on held-out trials
    t0 = time.perf_counter()
    refit = V.refit_joint(train, params, config, max_iter=args.refit_iters, verbose=False)
    out["refit_seconds"] = round(time.perf_counter() - t0, 2)
    out["refit_trace"] = refit["config"]["runtime"]["joint"]
    for tag, p in (("mean_field_fit", params), ("refit_joint", refit["params"])):
        jp = EV.joint_posterior(test, p, config)
        ml = EV.marginal_loglik(test, p, config, n_samples=args.samples, proposal="joint")
        out[tag] = {"laplace_total": jp["total"], "laplace_bps": jp["laplace_bps"], "marginal_total": ml["total"],
                    "marginal_bps": ml["marginal_bps"], "ess_median": float(np.median(ml["ess"])),
                    "n_failed": int(jp["n_failed"]) + int(ml["n_failed"])}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles", "joint_em"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "joint_em", "joint_em_bench.json"), "w") as f:
        f.write(line + "\n")
    write_readme(out)
    print(line)


if __name__ == "__main__":
    main()
