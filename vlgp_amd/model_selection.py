"""Choice of the number of latents by cross-validated co-smoothing.

``cross_validate`` holds out folds of trials, fits every candidate ``n_factors`` on the others and scores it on the
held-out trials with ``evaluation.leave_group_out``: the latents of a test trial are inferred from all channels but a
fold, that fold is predicted, and the prediction is scored in bits per spike.  Trial folds and channel folds are drawn
once and shared by every candidate, so the candidates are compared on paired folds.  One process, one GPU.

With ``score="speckled_bps"`` the held-out trials are scored by ``evaluation.leave_entries_out`` instead: folds of single
(bin, channel) entries are left out of the inference and predicted (the reference's ``gmap_speckled_cv`` scheme).  The fit
itself sees whole training trials, never a mask: the trials are held out, the speckle is applied to the test trials.

With ``score="marginal_bps"`` the held-out trials are scored as a whole by ``evaluation.marginal_loglik``: the
importance-weighted marginal likelihood in bits per spike.  Nothing is left out of the inference and no replica is made,
so the score has no limit on the number of latents.
"""
import numpy as np

from .api import fit
from .evaluation import channel_folds, leave_entries_out, leave_group_out, marginal_loglik

__all__ = ["cross_validate", "trial_folds"]


def trial_folds(n_trials, n_folds, seed=0):
    """``n_folds`` contiguous blocks (sizes differing by at most one) of a seeded permutation of ``range(n_trials)``."""
    n_trials, n_folds = int(n_trials), int(n_folds)
    if not 2 <= n_folds <= n_trials:
        raise ValueError("need 2 <= n_trial_folds <= number of trials, got %d folds for %d trials" % (n_folds, n_trials))
    perm = np.random.default_rng(seed).permutation(n_trials)
    return [[int(i) for i in block] for block in np.array_split(perm, n_folds)]


def _fresh(trials, index):
    """New trial dicts holding copies of the observations (and regressors) of ``trials[i]``, nothing else."""
    out = []
    for i in index:
        tr = {"y": np.array(trials[i]["y"], dtype=float)}
        if trials[i].get("x") is not None:
            tr["x"] = np.array(trials[i]["x"], dtype=float)
        out.append(tr)
    return out


def _seeded_fit(seed, trials, n_factors, **kwargs):
    """``fit`` with NumPy's global generator seeded (``fit`` draws the subsample of its factor-analysis start from it, as
    the reference does), the caller's generator state put back afterwards: the same arguments give the same fit."""
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        return fit(trials, n_factors, **kwargs)
    finally:
        np.random.set_state(state)


def best_candidate(n_factors_list, mean_co_bps):
    """The candidate with the largest mean; the smallest ``n_factors`` among equals; never one whose mean is NaN
    (None when every mean is NaN)."""
    best = None
    for n, m in zip(n_factors_list, mean_co_bps):
        if np.isnan(m):
            continue
        if best is None or m > best[1] or (m == best[1] and n < best[0]):
            best = (n, m)
    return None if best is None else best[0]


def cross_validate(trials, n_factors_list, n_trial_folds=4, n_channel_folds=5, seed=0, n_iter=None, device=0,
                   score="co_bps", predictive=False, n_nodes=12, proposal="posterior", **fit_kwargs):
    """Score every ``n_factors`` of ``n_factors_list`` by co-smoothing bits per spike on held-out trials.

    For every trial fold and candidate: ``fit`` on fresh copies of the other trials (``fit_kwargs`` are ``fit``'s),
    then ``leave_group_out`` on copies of the fold with the fit's parameters and the shared channel folds (``n_iter``
    E-step iterations, default the fit's ``max_iter``).  Every fit starts with ``np.random.seed(seed)`` (the state of
    the caller's generator is restored), so a second call returns the same bits.  A ``missing`` among ``fit_kwargs`` (one
    mask per trial of ``trials``) is cut to the training trials of every fold; the held-out trials are scored as they are.  The caller's trial dicts are not
    written and their posteriors are not read.  A candidate whose fit or evaluation raises is recorded as NaN for that
    fold, the exception text goes into ``errors`` and the sweep continues.

    Returns a dict: ``n_factors``; ``trial_folds`` (test-trial indices per fold); ``channel_folds``; ``co_bps``
    (candidates, trial folds); ``bits_per_spike`` (candidates, trial folds, N), per channel in plain order;
    ``n_failed`` (candidates, trial folds); ``mean_co_bps`` (candidates); ``best``; ``errors``, a list of
    ``(n_factors, fold, text)``.

    ``score="speckled_bps"`` scores every trial fold with ``leave_entries_out(n_folds=n_channel_folds, seed=seed)``
    instead (the entry folds depend on the fold's row count alone, so the candidates still share them).  The dict then
    holds ``speckled_bps`` and ``mean_speckled_bps`` where the default has ``co_bps`` and ``mean_co_bps``, ``score``, and
    no ``channel_folds``; ``best`` follows ``mean_speckled_bps``.

    ``score="marginal_bps"`` scores every trial fold with ``marginal_loglik(n_samples=n_channel_folds * 16, seed=seed)``:
    this score has no channel folds, so ``n_channel_folds`` sets the number of draws instead -- 16 for every replica the
    other scores would have inferred, 80 at the default (``marginal_loglik``'s own default is 64).  The
    dict holds ``marginal_bps`` (candidates, trial folds) and ``mean_marginal_bps``, ``ess_min`` (candidates, trial
    folds), the smallest per-trial effective sample size of the fold -- near 1 the fold's estimate rests on single
    draws and should not be trusted --, ``n_failed``, ``best``, ``errors`` and ``score``; no ``channel_folds`` and no
    per-channel ``bits_per_spike``.

    ``predictive=True`` scores ``co_bps`` and ``speckled_bps`` with the posterior-predictive density
    (``evaluation``'s docstring), ``n_nodes`` quadrature nodes per Poisson entry; ``marginal_bps`` is a score of whole
    trials with no plug-in form to replace, and raises ``ValueError`` with it.

    ``proposal`` is ``marginal_loglik``'s and is passed through to ``score="marginal_bps"`` alone: ``"joint"`` draws from
    the joint Laplace posterior of every held-out trial (``evaluation.joint_posterior``), whose effective sample size
    does not collapse when the latents are coupled through the loadings.  With another score ``proposal="joint"`` raises
    ``ValueError``."""
    if proposal not in ("posterior", "joint"):
        raise ValueError("proposal must be 'posterior' or 'joint', got %r" % (proposal,))
    if proposal != "posterior" and score != "marginal_bps":
        raise ValueError("proposal=%r applies to score='marginal_bps', not to %r" % (proposal, score))
    if score not in ("co_bps", "speckled_bps", "marginal_bps"):
        raise ValueError("score must be 'co_bps', 'speckled_bps' or 'marginal_bps', got %r" % (score,))
    if predictive and score == "marginal_bps":
        raise ValueError("predictive=True applies to the per-entry scores 'co_bps' and 'speckled_bps', not to 'marginal_bps'")
    if "comm" in fit_kwargs:
        raise ValueError("cross_validate runs on one process: it takes no comm")
    n_factors_list = [int(n) for n in n_factors_list]
    if not n_factors_list or min(n_factors_list) < 1:
        raise ValueError("n_factors_list must hold positive integers")
    N = int(trials[0]["y"].shape[1])
    t_folds = trial_folds(len(trials), n_trial_folds, seed)
    speckled, marginal = score == "speckled_bps", score == "marginal_bps"
    c_folds = None if speckled or marginal else channel_folds(N, n_channel_folds, seed)
    order = np.arange(N) if c_folds is None else np.argsort([c for g in c_folds for c in g])  # channel-list -> plain order
    shape = (len(n_factors_list), len(t_folds))
    co_bps = np.full(shape, np.nan)
    bps = np.full(shape + (N,), np.nan)
    ess_min = np.full(shape, np.nan)
    n_failed = np.zeros(shape, dtype=int)
    errors = []
    for f, test_idx in enumerate(t_folds):
        held = set(test_idx)
        train_idx = [i for i in range(len(trials)) if i not in held]
        if fit_kwargs.get("missing") is not None:  # fit's per-trial mask follows the training trials
            fold_kwargs = dict(fit_kwargs, missing=[fit_kwargs["missing"][i] for i in train_idx])
        else:
            fold_kwargs = fit_kwargs
        for c, n in enumerate(n_factors_list):
            try:
                fitted = _seeded_fit(seed, _fresh(trials, train_idx), n, device=device, verbose=False, **fold_kwargs)
                if marginal:
                    got = marginal_loglik(_fresh(trials, test_idx), fitted["params"], fitted["config"],
                                          n_samples=int(n_channel_folds) * 16, seed=seed, n_iter=n_iter, device=device,
                                          proposal=proposal)
                elif speckled:
                    got = leave_entries_out(_fresh(trials, test_idx), fitted["params"], fitted["config"],
                                            n_folds=n_channel_folds, seed=seed, n_iter=n_iter, device=device,
                                            predictive=predictive, n_nodes=n_nodes)
                else:
                    got = leave_group_out(_fresh(trials, test_idx), fitted["params"], fitted["config"], groups=c_folds,
                                          n_iter=n_iter, device=device, predictive=predictive, n_nodes=n_nodes)
            except Exception as err:  # (the sweep goes on: one candidate's failure is a result, not the end)
                errors.append((n, f, "%s: %s" % (type(err).__name__, err)))
                continue
            co_bps[c, f] = got[score]
            n_failed[c, f] = got["n_failed"]
            if marginal:
                ess_min[c, f] = np.min(got["ess"])
            else:
                bps[c, f] = got["bits_per_spike"][order]
    mean = np.array([np.mean(row) for row in co_bps])  # (NaN as soon as one fold of the candidate failed)
    if marginal:
        return {"n_factors": n_factors_list, "trial_folds": t_folds, "score": score, "marginal_bps": co_bps,
                "ess_min": ess_min, "n_failed": n_failed, "mean_marginal_bps": mean,
                "best": best_candidate(n_factors_list, mean), "errors": errors}
    if speckled:
        return {"n_factors": n_factors_list, "trial_folds": t_folds, "score": score, "speckled_bps": co_bps,
                "bits_per_spike": bps, "n_failed": n_failed, "mean_speckled_bps": mean,
                "best": best_candidate(n_factors_list, mean), "errors": errors}
    return {"n_factors": n_factors_list, "trial_folds": t_folds, "channel_folds": c_folds, "co_bps": co_bps,
            "bits_per_spike": bps, "n_failed": n_failed, "mean_co_bps": mean,
            "best": best_candidate(n_factors_list, mean), "errors": errors}
