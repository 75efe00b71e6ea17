"""Every output of the seven scoring entry points on one seeded set, saved for a bit-for-bit comparison of two builds.

    python tools/eval_bits.py OUT.npz              one E-step on a ragged set, then loglik, predictive, calibration, elbo,
                                                   forecast, marginal, joint_laplace and both marginal_loglik proposals
                                                   (130 draws); then the three row scores with every per-entry output on
                                                   group replicas and on a speckled masked set of it, one E-step each
    python tools/eval_bits.py --compare A.npz B.npz   np.array_equal(..., equal_nan=True) on every array; exit status 1
                                                   if the files differ in their names or in any array
Nothing is fitted: the parameters are seeded, the prior factors come from the device for fixed time scales.  Run it from
each build's own tree (it imports the package beside it)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = [1, 7, 64, 65, 130, 130]
N, L, RANK, K, SET = 14, 3, 20, 130, 0
OMEGA = [2e-2, 5e-3, 1e-3]
N_EXT = 5
GROUPS = [[0, 5, 13], [2], [7, 8]]  # the group replicas; N_FOLDS speckled folds make the masked set
N_FOLDS = 3


def row_scores(eng, set_id, prefix):
    out = {}
    out["loglik_sums"], out["loglik_rate"] = eng.loglik(set_id, want_rate=True)
    out["pred_sums"], out["pred_rate"], out["pred_lpd"] = eng.predictive(set_id, want_rate=True, want_lpd=True)
    out["cal_sums"], out["cal_cdf"] = eng.calibration(set_id, want_cdf=True)
    return {prefix + k: v for k, v in out.items()}


def outputs():
    from vlgp_amd import engine as E
    from vlgp_amd import evaluation, synth

    rng = np.random.default_rng(3)
    trials = synth.make_trials(len(LENGTHS), max(LENGTHS), N, L, seed=3, lengths=LENGTHS)
    y = np.concatenate([t["y"] for t in trials])
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": RANK, "a": 0.3 * rng.standard_normal((L, N)),
              "b": np.log(np.maximum(y.mean(0), 1e-3))[None, :], "noise": np.ones(N), "omega": np.asarray(OMEGA),
              "sigma": np.ones(L), "likelihood": np.array(["poisson"] * N)}
    config = {"method": "VB", "max_iter": 1, "dmu_bound": 5.0, "rank": RANK}
    units = [{"y": t["y"], "x": None, **{k: np.zeros((t["y"].shape[0], L)) for k in ("mu", "v", "w")}} for t in trials]
    eps = rng.standard_normal((len(units), L, RANK, K))
    out = {}
    with E.Engine.for_params(params) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET, units)
        held = sorted(set(LENGTHS))
        eng.build_prior([T + N_EXT for T in held], params["omega"], params["sigma"])
        ext = {}
        for T in held:  # the factor of length T + N_EXT, split into the prior of the set and its extension rows
            full = eng.get_prior(T + N_EXT)
            eng.set_prior(T, np.ascontiguousarray(full[:, :T]))
            ext[T] = np.ascontiguousarray(full[:, T:])
        out["estep_failed"] = np.array([eng.estep(SET, 1, 5.0, True)])
        state = eng.download(SET, ("mu", "v", "w"))
        out.update({"state_" + k: v for k, v in state.items()})
        out.update(row_scores(eng, SET, ""))
        out["elbo_sums"], out["elbo_terms"], n, out["elbo_rows"] = eng.elbo(SET, want_rows=True)
        out["elbo_failed"] = np.array([n])
        out["fc_mu"], out["fc_v"], out["fc_terms"], n = eng.forecast(SET, ext)
        out["fc_failed"] = np.array([n])
        out["mg_log_w"], n, out["mg_parts"] = eng.marginal(SET, eps, want_parts=True)
        out["mg_failed"] = np.array([n])
        joint = eng.joint_laplace(SET, eps=eps)
        out.update({"jl_" + k: np.asarray(v) for k, v in joint.items()})
        folds = evaluation.entry_folds(sum(LENGTHS), N, N_FOLDS, 5)
        held = np.stack([folds == k for k in range(N_FOLDS)])
        for name, how in (("grp_", {"groups": GROUPS}), ("msk_", {"held_out": held})):
            eng.replicate(SET, 2, **how)
            out[name + "estep_failed"] = np.array([eng.estep(2, 1, 5.0, True)])
            out.update(row_scores(eng, 2, name))
            eng.free_units(2)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    fitted = [dict(tr, **{k: state[k][off[i]:off[i + 1]] for k in ("mu", "v", "w")}) for i, tr in enumerate(trials)]
    for proposal in ("posterior", "joint"):
        for infer in (True, False):
            got = evaluation.marginal_loglik(fitted, dict(params), config, n_samples=K, seed=7, infer=infer,
                                             proposal=proposal)
            out.update({"ml_%s_%d_%s" % (proposal, infer, k): np.asarray(v) for k, v in got.items()})
    return out


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    if not same:
        print("different names:", sorted(set(A.files) ^ set(B.files)))
    for k in sorted(set(A.files) & set(B.files)):
        eq = np.array_equal(A[k], B[k], equal_nan=True)
        same = same and eq
        print("%-28s %-14s %s" % (k, A[k].shape, "equal" if eq else "DIFFERENT"))
    print("%d arrays: %s" % (len(A.files), "all equal" if same else "NOT all equal"))
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    np.savez(sys.argv[1], **outputs())
