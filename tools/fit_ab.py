"""Bits of a fit and of the held-out routines, for a same-box A/B of two trees (tools/ab_old_new.sh: the parent in
_ab_old/).  Runs ten small cases once in whichever vlgp_amd is importable from the CURRENT directory and saves every
array of the results to an .npz; with --compare it reports, case by case, how many arrays of two such files are equal
byte for byte (NaN at equal positions counts as equal).

    (cd _ab_old && python ../tools/fit_ab.py --out ../build/fit_ab_old.npz)
    python tools/fit_ab.py --out build/fit_ab_new.npz
    python tools/fit_ab.py --compare build/fit_ab_old.npz build/fit_ab_new.npz

Every case: synth.make_trials, N = 8, L = 2, max_iter = min_iter = 3.  Saved per trial: mu, v, w, dmu, x, missing; params
with every cholesky[T] and params["initial"]; config with its runtime lists, the wall-clock timers (*_elapsed) left out.

  a  plain, 3 trials x 80 bins, window 40            f  as a, history=1, last channel Gaussian, x given
  b  plain, 3 x 100 bins, window 40 (overlaps)       g  masked (20 % missing), 3 x 80 bins, window 40
  c  as b, constrain_loading="svd"                   h  as g, constrain_latent=True
  d  plain, no window (Hstep=False)                  i  masked, no window (Hstep=False)
  e  as a, track_elbo=True                           j  leave_one_out (batched, sequential), leave_group_out (3 folds),
                                                        leave_entries_out (3 folds, max_replicas=2), impute: fit of a
a, d, g, i take the default initialisation (factor analysis, projection); the others are given a, b.  Without a window
there is no H-step: gp.optimize works on window-sized segments."""
import argparse
import os
import sys

import numpy as np

N, L = 8, 2


def flatten(obj, prefix, out):
    """Every array, number, string and list of them under ``obj`` into ``out`` as ``prefix/key/...``."""
    if obj is None or callable(obj):
        return
    if isinstance(obj, dict):
        for k in list(obj.keys()):  # (the lazy prior dicts of a fit answer keys() and [], not items())
            if not str(k).endswith("_elapsed"):
                flatten(obj[k], "%s/%s" % (prefix, k), out)
    elif isinstance(obj, (list, tuple)) and any(isinstance(v, (dict, list, tuple, np.ndarray)) for v in obj):
        for i, v in enumerate(obj):
            flatten(v, "%s/%d" % (prefix, i), out)
    else:
        arr = np.array(obj)  # a copy: x may be a zero-stride view
        out[prefix] = np.array(repr(obj)) if arr.dtype == object else arr


def given(trials, seed=0):
    rng = np.random.default_rng(seed)
    y = np.concatenate([tr["y"] for tr in trials])
    return {"a": 0.3 * rng.standard_normal((L, N)), "b": np.log(np.maximum(y.mean(axis=0, keepdims=True), 1e-2))}


def run_cases():
    import masked_fit_numpy as MF
    import vlgp_amd
    from vlgp_amd import evaluation, synth

    out = {}

    def fit(case, n_bins, init=True, missing=False, x=False, **kw):
        trials = synth.make_trials(3, n_bins, N, L, seed=1, n_gauss=1 if x else 0)
        if x:
            for tr in trials:
                tr["x"] = np.ones((n_bins, 1, N))
        if init:
            kw.update(given(trials))
        if missing:
            kw["missing"] = MF.random_missing(trials, 0.2, 2)
        np.random.seed(3)  # the subsample of the initialisation and the overlaps of the cut draw from the global state
        res = vlgp_amd.fit(trials, L, verbose=False, max_iter=3, min_iter=3, **kw)
        flatten(res, case, out)
        return res

    res_a = fit("a", 80, init=False, window=40)
    fit("b", 100, window=40)
    fit("c", 100, window=40, constrain_loading="svd")
    fit("d", 80, init=False, window=None, Hstep=False)
    fit("e", 80, window=40, track_elbo=True)
    fit("f", 80, x=True, window=40, history=1, lik=["poisson"] * (N - 1) + ["gaussian"])
    fit("g", 80, init=False, missing=True, window=40, constrain_latent=False)
    fit("h", 80, missing=True, window=40, constrain_latent=True)
    fit("i", 80, init=False, missing=True, window=None, Hstep=False)

    test = synth.make_trials(2, 80, N, L, seed=4)
    params, config = res_a["params"], res_a["config"]
    for path in ("batched", "sequential"):
        flatten(evaluation.leave_one_out(test, params, config, path=path), "j/leave_one_out/" + path, out)
    flatten(evaluation.leave_group_out(test, params, config, n_folds=3), "j/leave_group_out", out)
    flatten(evaluation.leave_entries_out(test, params, config, n_folds=3, max_replicas=2), "j/leave_entries_out", out)
    flatten(evaluation.impute(test, params, config, MF.random_missing(test, 0.2, 5)), "j/impute", out)
    return out


def compare(path_a, path_b):
    with np.load(path_a) as fa, np.load(path_b) as fb:
        a, b = {k: fa[k] for k in fa.files}, {k: fb[k] for k in fb.files}
    print("parent package: %s" % str(a.pop("package")))
    print("this package:   %s" % str(b.pop("package")))
    bad = sorted(set(a) ^ set(b))
    for case in sorted({k.split("/")[0] for k in a}):
        keys = [k for k in sorted(a) if k.split("/")[0] == case and k in b]
        equal = numbers = nans = 0
        for k in keys:
            x, y = a[k], b[k]
            same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
            if not same and x.dtype == y.dtype and x.shape == y.shape and x.dtype.kind == "f":
                nan = np.isnan(x) & np.isnan(y)  # NaN payloads may differ: equal where both are NaN, bytes elsewhere
                same = bool(np.all(nan | (x.view(np.uint64) == y.view(np.uint64)))) if x.dtype == np.float64 else False
            equal += same
            numbers += x.size
            nans += int(np.isnan(x).sum()) if x.dtype.kind == "f" else 0
            if not same:
                bad.append(k)
        print("%-54s %3d arrays, %3d equal (%d numbers, %d NaN at equal positions)" % (case, len(keys), equal, numbers, nans))
    print("arrays: %d compared" % len(set(a) & set(b)))
    if bad:
        print("RESULT: DIFFERENT: " + ", ".join(bad))
        return 1
    print("RESULT: every array equal byte for byte")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="build/fit_ab.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tests")]
    import vlgp_amd

    out = run_cases()
    out["package"] = np.array(os.path.relpath(os.path.dirname(vlgp_amd.__file__),
                                              os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **out)
    print("%d arrays -> %s" % (len(out) - 1, args.out))


if __name__ == "__main__":
    main()
