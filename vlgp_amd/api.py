"""``fit`` / ``transform`` with the reference's call contract (vlgp/api.py:18-76,171-184).

``fit(trials, n_factors, **kwargs) -> {"trials", "params", "config"}``: the
caller's trial dicts are mutated in place and returned; mu, v, dmu are updated
in place, w is replaced; numerical failures never raise.  The whole EM loop
runs on the GPU between one upload and one download.
"""
import contextlib
import copy
import logging

import numpy as np

from . import engine as E
from . import gp
from .preprocess import fill_params, fill_trials, get_config, get_params, initialize
from .util import _per_trial_entries, segment_starts

__all__ = ["fit", "transform", "forecast", "refit_joint", "FitSession", "bind_priors"]

logger = logging.getLogger(__name__)

SET_TRIALS, SET_SEGMENTS = 0, 1
# a fit with missing observations works on masked fit sets (one-replica vlgp_replicate_masked) of the two above
SET_TRIALS_MASKED, SET_SEGMENTS_MASKED = 2, 3


def _echo(msg):
    print(msg, flush=True)


def _segment_dicts(trials, ys, starts, window):
    """The window-sized segments of the dict interface (util.cut_trials), trial-major: host-side NumPy views of every
    trial's x, mu, w, v and of ``ys[i]`` -- the y to slice trial ``i``'s from, which need not be ``tr["y"]`` -- at the start
    rows ``starts[i]``."""
    segs = []
    for tr, y, trial_starts in zip(trials, ys, starts):
        for s in trial_starts:
            sl = slice(int(s), int(s) + window)
            segs.append({k: (y if k == "y" else tr[k])[sl] for k in ("y", "x", "mu", "w", "v")})
    # the per-segment dmu buffers fill_trials would otherwise allocate one by one (4000 at C3): views of one block
    if segs:
        block = np.zeros((len(segs), window, segs[0]["mu"].shape[1]))
        for i, sg in enumerate(segs):
            sg["dmu"] = block[i]
    return segs


def _segments(trials, window, eng):
    """Cut the resident trials into window-sized segments (util.cut_trials):
    host-side NumPy views for the dict interface, one device cut for the data."""
    per_trial, starts, row0 = [], [], 0
    for tr in trials:
        T = tr["y"].shape[0]
        if T < window:
            # the reference would cut a shorter segment here and then fail in gp.optimize (np.stack of
            # unequal segments); the device cut needs equal lengths, so say it up front
            raise ValueError("trial of %d bins is shorter than window=%d; pass a smaller window" % (T, window))
        per_trial.append([int(s) for s in segment_starts(T, window)])
        starts.extend(row0 + s for s in per_trial[-1])
        row0 += T
    segs = _segment_dicts(trials, [tr["y"] for tr in trials], per_trial, window)
    starts = np.asarray(starts, dtype=np.int64)
    # Overlapping neighbours (a trial length that is not a multiple of the window, vlgp/util.py:482-496): in the reference
    # they are views of the same rows, visited one after the other.  The device keeps independent copies, stored
    # stage-major (stage = position in a chain of overlapping neighbours) so that the E-step can run stage by stage with
    # the shared rows handed over in between (vlgp_set_overlaps); `unit_of` maps a segment of this list to its unit.
    n = len(segs)
    over = np.zeros(n, dtype=np.int64)          # rows segment i shares with segment i - 1
    if n > 1:
        gap = starts[1:] - starts[:-1]
        over[1:] = np.where((gap > 0) & (gap < window), window - gap, 0)
    if not over.any():
        eng.cut(SET_TRIALS, SET_SEGMENTS, starts, window)
        return E.DeviceTrials(segs, eng, SET_SEGMENTS, parent_set=SET_TRIALS)
    stage = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        stage[i] = stage[i - 1] + 1 if over[i] else 0
    order = np.argsort(stage, kind="stable")    # unit u holds segment order[u]
    unit_of = np.empty(n, dtype=np.int64)
    unit_of[order] = np.arange(n)
    n_stages = int(stage.max()) + 1
    stage_start = np.searchsorted(stage[order], np.arange(n_stages + 1)).astype(np.int32)
    linked = np.flatnonzero(over)               # segment i shares over[i] rows with segment i - 1
    linked = linked[np.argsort(stage[linked], kind="stable")]
    links = np.stack([unit_of[linked - 1], unit_of[linked], over[linked]], axis=1).astype(np.int32)
    link_start = np.searchsorted(stage[linked], np.arange(n_stages + 1)).astype(np.int32)
    eng.cut(SET_TRIALS, SET_SEGMENTS, starts[order], window)
    eng.set_overlaps(SET_SEGMENTS, stage_start, links, link_start)
    return E.DeviceTrials(segs, eng, SET_SEGMENTS, parent_set=SET_TRIALS, unit_of=unit_of)


def _masked_inputs(trials, missing, comm, track_elbo, config, kwargs):
    """What ``fit(..., missing=)`` refuses, before an engine exists and before a trial dict is touched.  Returns the
    mask per trial and the private copies of y the fit works on."""
    lik = kwargs.get("lik", "poisson")
    if any(k == "gaussian" for k in (lik if isinstance(lik, list) else [lik])):
        raise ValueError("fit(missing=...) takes Poisson channels only: a Gaussian channel's update needs "
                         "per-channel masked Gram matrices")
    if kwargs.get("history", 0) > 0:
        raise ValueError("fit(missing=...) takes no history: the regressors would be built from missing counts")
    if comm is not None and comm.world > 1:
        raise ValueError("fit(missing=...) runs on one rank: it takes no comm with world > 1")
    if track_elbo:
        raise ValueError("fit(missing=...) takes no track_elbo: the bound of a masked set is not computed")
    if config["constrain_loading"] == "svd":
        raise ValueError("fit(missing=...) takes no constrain_loading='svd': it rests on segments being views of trials")
    missing = [np.array(m, dtype=bool) for m in _per_trial_entries(missing, trials, "missing", bool)]
    window = config["window"]
    if window and any(tr["y"].shape[0] % window for tr in trials):
        raise ValueError("fit(missing=...) needs trial lengths that are multiples of window=%d: overlapping "
                         "segments share rows, which a masked set cannot" % window)
    n_obs = sum((~m).sum(axis=0) for m in missing)
    if np.any(n_obs == 0):
        raise ValueError("channel(s) %s have no observed entry" % np.flatnonzero(n_obs == 0).tolist())
    # private copies of y, the holes filled with the channel's mean over its observed entries: the initialisation
    # (factor analysis, initial latents, b = log mean y) works on them, and they are what the device holds -- the
    # masked row passes of the E-step leave an entry out by a zero coefficient, under which a NaN in the caller's y
    # would survive.  The fill value reaches no result after the initialisation; the caller's values at missing entries
    # are never read.
    y_sum = sum(np.where(m, 0.0, tr["y"]).sum(axis=0) for tr, m in zip(trials, missing))
    y_mean = y_sum / n_obs
    return missing, [np.where(m, y_mean[None, :], tr["y"]).astype(float) for tr, m in zip(trials, missing)]


def _ones_for_broadcast_x(trials):
    """The reference leaves a writable np.ones((T, xdim, N)) in every trial that came without regressors: make it of the
    zero-stride view the fit worked on."""
    for tr in trials:
        x = tr.get("x")
        if isinstance(x, np.ndarray) and not x.flags.writeable and x.size and all(st == 0 for st in x.strides):
            tr["x"] = np.ones(x.shape)


class FitSession:
    """The three phases of api.fit as separate calls.

    ``FitSession(...)``  api.py:27-60 -- config, params, initialisation, upload,
                         prior factor, w, v, segmentation
    ``run()``            api.py:64 -- core.vem on the segments
    ``finish()``         api.py:66-76 -- full-length prior, w, v, inference, download

    ``bench.py`` drives ``em_iteration`` directly to time single EM iterations;
    ``fit`` is ``FitSession(...).run().finish()``.

    ``missing`` (``fit``'s docstring) varies six steps and nothing else: the argument checks, ``_initialize``,
    ``_resident_trials``, ``_cut_segments``, ``_segments_to_trials`` and ``_after_inference``.
    """

    def __init__(self, trials, n_factors, device=0, comm=None, verbose=True, track_elbo=False, missing=None, **kwargs):
        self.echo = echo = _echo if verbose else None
        self.track_elbo = bool(track_elbo)
        self.trials = trials
        self.config = config = get_config(**kwargs)
        self.missing = None
        if missing is not None:
            self.missing, self._y_filled = _masked_inputs(trials, missing, comm, self.track_elbo, config, kwargs)
            self._mask_rows = np.concatenate(self.missing, axis=0)
        logger.info("\n".join("{} : {}".format(k, v) for k, v in config.items()))
        kwargs["omega_bound"] = config["omega_bound"]
        self.params = params = get_params(trials, n_factors, **kwargs)
        self.comm = comm
        self.eng = None
        self.runtime = E.new_runtime()
        # the reference leaves a writable np.ones((T, xdim, N)) in every trial that came without regressors
        # (preprocess.py:43-44); the fit itself works on a zero-stride view, the real arrays are made on the way out
        self.materialize_x = bool(kwargs.get("materialize_x", True))

        if echo:
            echo("Initializing")
        eng = E.Engine.for_params(params, device)
        self.eng = eng
        try:
            multi = comm is not None and comm.world > 1
            if multi:
                comm.attach(eng)
            self._initialize(multi)
            if echo:
                echo("Initialized")
            fill_params(params)
            for key in ("a", "b", "noise", "omega", "sigma"):
                params[key] = np.array(params[key], dtype=float)
            if multi:
                self._replicate_params()
            eng.set_params(params["a"], params["b"], params["noise"])
            self.dev_trials = self._resident_trials()
            self._prior_w_v()
            if config["window"]:
                self.segs = self._cut_segments(config["window"])
                E.make_cholesky(self.segs, params, config)
                fill_trials(self.segs)
            else:
                self.segs = self.dev_trials
            self._snapshot_initial()
            E._push_params(eng, params)
        except Exception:
            self.close()
            raise

    def _initialize(self, multi):
        """preprocess.initialize and what it leaves in the trials.  Plain: the trials go to the device here, which does
        the two full passes over y.  Masked: on the filled copies of y, all on the host; nothing is uploaded yet."""
        trials, params, config, eng = self.trials, self.params, self.config, self.eng
        if self.missing is not None:
            work = [dict(tr, y=y) for tr, y in zip(trials, self._y_filled)]
            initialize(work, params, config)
            fill_trials(work)
            for tr, wk in zip(trials, work):  # the caller's dicts get what initialize leaves; their y stays theirs
                tr.update({k: v for k, v in wk.items() if k != "y"})
            return
        # sharded fit: the subsample, the factor analysis and b = log mean y are pooled over the ranks
        plan = initialize(trials, params, config, defer_latent=True, pool=eng if multi else None)
        fill_trials(trials)
        eng.upload(SET_TRIALS, trials)
        if plan is not None:
            # the two full passes over y of preprocess.initialize, on the device: mu = transform(y), b = log mean y
            colsum = eng.project_latent(SET_TRIALS, plan["proj"], plan["shift"])
            if plan["need_b"]:
                if multi:
                    eng.allreduce_host(colsum)
                params["b"] = np.log(np.maximum(colsum[None, :] / plan["rows"], config["eps"]))

    def _resident_trials(self):
        """The set of the full-length trials.  Plain: ``SET_TRIALS`` as ``_initialize`` uploaded it.  Masked: the trials
        as they are now with the filled y, and their masked fit set (one replica: the same rows, one mask bit per entry)."""
        if self.missing is None:
            return E.DeviceTrials(self.trials, self.eng, SET_TRIALS)
        self.eng.upload(SET_TRIALS, [dict(tr, y=y) for tr, y in zip(self.trials, self._y_filled)])
        self.eng.replicate(SET_TRIALS, SET_TRIALS_MASKED, held_out=self._mask_rows[None])
        return E.DeviceTrials(self.trials, self.eng, SET_TRIALS_MASKED)

    def _cut_segments(self, window):
        """The set the EM loop works on.  Plain: a device cut of ``SET_TRIALS``, overlaps included.  Masked: a plain set of
        its own (a host cut: y, x, mu, v, w) and its masked fit set; trial lengths are multiples of the window, so the
        segments' rows, in order, are the trials' rows."""
        if self.missing is None:
            return _segments(self.trials, window, self.eng)
        self.dev_trials.pull(("mu", "v", "w"))
        segs = _segment_dicts(self.trials, self._y_filled, [range(0, y.shape[0], window) for y in self._y_filled], window)
        self.eng.upload(SET_SEGMENTS, segs)
        self.eng.replicate(SET_SEGMENTS, SET_SEGMENTS_MASKED, held_out=self._mask_rows[None])
        return E.DeviceTrials(segs, self.eng, SET_SEGMENTS_MASKED)

    def _segments_to_trials(self):
        """The segments' posterior back into the full-length trials.  Plain: a device merge.  Masked: through the host
        (same rows, same order), then the trials' masked fit set again from it."""
        eng = self.eng
        if self.missing is None:
            eng.merge(SET_SEGMENTS)
            if self.segs.detached:  # constrain_loading "svd": the trials kept their pre-rotation mu (core.py:407-408)
                eng.stash_mu(SET_TRIALS, restore=True)
            return
        got = eng.download(SET_SEGMENTS_MASKED, ("mu", "v", "w"))
        row = 0
        for tr in self.trials:
            T = tr["y"].shape[0]
            for k in ("mu", "v"):
                tr[k][...] = got[k][row:row + T]
            tr["w"] = got["w"][row:row + T].copy()
            row += T
        eng.free_units(SET_SEGMENTS_MASKED)
        eng.free_units(SET_TRIALS_MASKED)
        self.dev_trials = self._resident_trials()

    def _after_inference(self):
        """Plain: the bound of the full-length trials, when tracked.  Masked: every trial carries its mask."""
        if self.missing is not None:
            for tr, m in zip(self.trials, self.missing):
                tr["missing"] = m
        elif self.track_elbo:  # the bound of the full-length trials under the final posterior, summed over the ranks
            final = E._elbo_totals(self.eng, SET_TRIALS, self.config["method"] == "VB")
            if self.eng.world > 1:
                self.eng.allreduce_host(final)
            self.runtime["elbo_final"] = float(final[0])
            self.config["runtime"] = self.runtime

    def _prior_w_v(self):
        """Prior factor, w and v of the full-length trials under the current parameters."""
        E.make_cholesky(self.dev_trials, self.params, self.config)
        E.update_w(self.dev_trials, self.params, self.config)
        E.update_v(self.dev_trials, self.params, self.config)

    def _snapshot_initial(self):
        # params["initial"] = deepcopy(params) (api.py:60): every key, the segment-length factors included.  The
        # resident factor is downloaded for it when a window is set (one (L, window, rank) array); without a
        # window it is every full-length factor: those are rebuilt on the host when somebody reads them
        params = self.params
        snapshot = {k: v for k, v in params.items() if k != "cholesky"}
        chol = params["cholesky"]
        if isinstance(chol, E._LazyPrior):
            # no window: the full-length factors of the initial omega, factored on first access (engine._InitialPrior)
            chol = chol.materialize() if self.config["window"] else E._InitialPrior(
                chol._lengths, params["omega"], params["sigma"], params["rank"])
        snapshot["cholesky"] = chol
        params["initial"] = copy.deepcopy(snapshot)

    def _replicate_params(self):
        """Every rank must start from the same a, b, noise: keep rank 0's."""
        p, eng = self.params, self.eng
        for key in ("a", "b", "noise"):
            buf = np.ascontiguousarray(p[key], dtype=float)
            if eng.rank != 0:
                buf = np.zeros_like(buf)
            eng.allreduce_host(buf)
            p[key] = buf

    def em_iteration(self):
        """One EM iteration on the segments; True when the stopping rule fires."""
        if self.track_elbo:
            return E.em_iteration(self.segs, self.params, self.config, self.runtime, self.echo, track_elbo=True)
        return E.em_iteration(self.segs, self.params, self.config, self.runtime, self.echo)

    def run(self):
        if self.echo:
            self.echo("Fitting")
        for _ in range(self.config["max_iter"]):
            if self.em_iteration():
                break
        return self

    def finish(self):
        params, config, echo = self.params, self.config, self.echo
        try:
            if self.segs is not self.dev_trials:
                self._segments_to_trials()
            self._prior_w_v()
            if echo:
                echo("Inferring")
            E.infer(self.dev_trials, params, config, echo=echo)
            self._after_inference()
            self.dev_trials.pull()
            if self.materialize_x:
                _ones_for_broadcast_x(self.trials)
            if isinstance(params["cholesky"], E._LazyPrior):
                params["cholesky"] = params["cholesky"].materialize()
            if echo:
                echo("Done")
        finally:
            self.close()
        return {"trials": self.trials, "params": params, "config": config}

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None


def fit(trials, n_factors, device=0, comm=None, verbose=True, track_elbo=False, missing=None, **kwargs):
    """Variational-EM fit of vLGP on one MI355X (or one rank of several).

    Same arguments as the reference: ``lik``, ``history``, ``a``, ``b``,
    ``noise``, ``sigma``, ``omega`` and every ``get_config`` key.  Extra:
    ``device`` (GPU index), ``comm`` (a :class:`vlgp_amd.dist.Comm` when the
    trials are sharded over ranks), ``verbose``, ``ichol`` ("device"/"host": who builds the prior
    factor -- the device kernel is bit-identical to the reference's on the NumPy 2.2 / AVX-512 / OpenBLAS
    stack the golden vectors were captured on, "host" uses this host's own NumPy: INTEGRATION.md),
    ``materialize_x`` (default True: trials that came
    without regressors get a writable ``np.ones((T, xdim, N))`` back, as the reference leaves them),
    ``track_elbo`` (default False: nothing extra runs and no key is added.  True: ``config["runtime"]["elbo"]``
    gets the variational lower bound after every E-step, ``"elbo_ell"`` / ``"elbo_kl"`` its two parts, and
    ``"elbo_final"`` the bound of the full-length trials after the final inference; all summed over the ranks.  The
    per-iteration trace is the objective of the SEGMENT set the EM loop works on -- segments of a trial whose length
    is not a multiple of the window overlap -- not of the trials; see ``vlgp_amd.evaluation.elbo``),
    ``missing`` (default None: today's fit.  A list per trial of (T, N) bool arrays, True where the observation is
    absent, as ``evaluation.impute`` takes it: those entries' likelihood terms are left out of the E-step, the M-step and
    the initialisation, and what ``y`` holds there is never read.  Poisson channels, no ``history``, one rank, no
    ``track_elbo``, no ``constrain_loading="svd"``, trial lengths multiples of ``window``; each is a ``ValueError``
    otherwise.  Every returned trial carries its ``missing`` array.  INTEGRATION.md, "Fit with missing observations").
    """
    return FitSession(trials, n_factors, device=device, comm=comm, verbose=verbose, track_elbo=track_elbo,
                      missing=missing, **kwargs).run().finish()


def bind_priors(eng, trials, params):
    """Give the engine a prior factor for every trial length: ``params["cholesky"]``'s where it has one, the
    rest built on the device (and added to ``params["cholesky"]``, a new dict)."""
    chol = dict(params.get("cholesky") or {})
    lengths = sorted({int(tr["y"].shape[0]) for tr in trials})
    missing = [T for T in lengths if T not in chol]
    have = [T for T in lengths if T in chol]
    if missing:
        eng.build_prior(missing, params["omega"], params["sigma"])
        for T in missing:
            chol[T] = eng.get_prior(T)
    for T in have:
        eng.set_prior(T, chol[T])
    params["cholesky"] = chol


def transform(trials, params, config, device=0):
    """Infer latents of new trials with fitted parameters (vlgp/api.py:171-184).

    Unlike the reference (which raises KeyError for a trial length it has no
    factor for), missing prior factors are built on the fly."""
    initialize(trials, params, config)
    fill_trials(trials)
    with E.Engine.for_params(params, device) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET_TRIALS, trials)
        dev = E.DeviceTrials(trials, eng, SET_TRIALS)
        bind_priors(eng, trials, params)
        E.infer(dev, params, config)
        dev.pull()
    return trials


def refit_joint(trials, params, config, max_iter=20, tol=1e-6, newton_iter=50, newton_tol=1e-10, device=0, verbose=True,
                comm=None, missing=None, hstep=False):
    """Laplace EM: refit ``a``, ``b`` and ``noise`` (with ``hstep=True`` also ``omega``) under the joint Laplace posterior
    of every whole trial.

    ``trials, params, config`` as ``fit`` or ``transform`` return them.  By default ``omega``, ``sigma`` and the prior
    factors are those of ``params`` and are not re-estimated; no loading constraint is applied, the fixed prior sets the
    scale.  With ``E_k`` the sum over trials of the Laplace evidence under ``params_k``:

    1. ``post_k`` = the joint posterior of every trial under ``params_k`` (``Engine.joint_posterior``, ``newton_iter``
       factorisations at most, decrement ``newton_tol``), started from the caller's ``mu, w`` every time;
    2. ``runtime["joint"]``: ``"laplace"`` gets ``E_k``, ``"n_newton"`` the largest count of the iteration,
       ``"converged"`` whether every trial did;
    3. if ``k >= 1`` and ``E_k - E_{k-1} <= tol |E_k|``: stop with ``(params_k, post_k)`` if ``E_k >= E_{k-1}``, else with
       ``(params_{k-1}, post_{k-1})``;
    4. if ``k == max_iter``: stop with ``(params_k, post_k)``;
    5. else ``params_{k+1}`` = ``Engine.mstep_cov`` of ``post_k`` with ``config``'s M-step settings.

    So the returned posterior is the posterior of the returned parameters.  For all-Gaussian channels the E-step is exact
    and this is GPFA's EM in the low-rank prior.  A trial whose ``H`` cannot be factored raises ``VlgpError`` before an
    M-step sees its rows.  A ``comm`` and trials without ``mu`` or ``w`` raise ``ValueError``.

    ``missing``: a list per trial of (T, N) bool arrays, True where the observation is absent, as ``fit`` and
    ``evaluation.impute`` take it; by default the trials' own ``missing`` arrays when every trial carries one, as the
    trials of ``fit(..., missing=)`` do (some trials carrying one and some not is a ``ValueError``).  The same loop on a
    masked fit set: the posterior does not see the missing entries, ``E_k`` is the evidence of the observed ones, the
    M-step is ``Engine.mstep_cov_masked`` (every channel over its observed rows) and ``w`` sums over a row's observed
    channels.  What ``y`` holds at a missing entry is never read.  Poisson channels only, and every channel needs an
    observed entry: each a ``ValueError`` otherwise.  Every returned trial carries its ``missing`` array.

    ``hstep=True`` learns the GP timescales under the same posterior.  Step 1 also returns the window
    moments of ``post_k`` (``Engine.joint_posterior(..., window=config["window"])``) and step 5 becomes: ``a, b, noise`` from
    the covariance M-step of ``post_k``; ``omega`` from ``gp.optimize_joint`` on ``post_k``'s moments; the prior factors
    rebuilt on the device for the new ``omega`` before the next E-step.  Where step 3 goes back to ``params_{k-1}`` the
    previous ``omega`` and its factors come back with it.  ``runtime["joint"]["omega"]`` gets ``omega_k``, one (L,) array
    per iteration; the returned ``params`` carries the returned ``omega`` and the ``cholesky`` that belongs to it.
    ``sigma`` and ``gp_noise`` are not re-estimated.  Works with ``missing`` as well.  ``config["window"]`` outside
    2 ... 64, ``params["rank"] > 64`` and no trial as long as the window are a ``ValueError`` each.

    Returns a new ``{"trials", "params", "config"}``; the caller's dicts are not modified.  Every trial copy has ``mu``
    (the mode), ``v`` (the diagonal of ``cov``), ``cov`` (T, L, L) and ``w`` from ``update_w`` at that ``mu`` under the
    returned parameters; ``params`` has the new ``a, b, noise, da, db``; ``config["runtime"]["joint"]`` the trace."""
    if comm is not None:
        raise ValueError("refit_joint runs on one rank: vlgp_mstep_cov takes no communicator (comm must be None)")
    if missing is None:
        carried = [tr.get("missing") is not None for tr in trials]
        if any(carried) and not all(carried):
            raise ValueError("refit_joint: trial %d carries 'missing' and trial %d does not: pass missing= for all of them"
                             % (carried.index(True), carried.index(False)))
        if any(carried):
            missing = [tr["missing"] for tr in trials]
    for i, tr in enumerate(trials):
        if tr.get("mu") is None or tr.get("w") is None:
            raise ValueError("refit_joint: trial %d has no 'mu' / 'w': pass trials as fit or transform return them" % i)
    if missing is not None:
        if np.any(np.asarray(params["likelihood"]) == "gaussian"):
            raise ValueError("refit_joint(missing=...) takes Poisson channels only: a Gaussian channel's update needs "
                             "per-channel masked Gram matrices")
        missing = [np.array(m, dtype=bool) for m in _per_trial_entries(missing, trials, "missing", bool)]
        n_obs = sum((~m).sum(axis=0) for m in missing)
        if np.any(n_obs == 0):
            raise ValueError("refit_joint(missing=...): channel(s) %s have no observed entry" % np.flatnonzero(n_obs == 0).tolist())
    echo = _echo if verbose else (lambda msg: None)
    L = int(params["zdim"])
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    window = None
    if hstep:  # the limits of the compiled window-moments kernel (vlgp_joint_posterior_moments), before an engine exists
        window = int(config["window"])
        if not 2 <= window <= 64:
            raise ValueError("refit_joint(hstep=True): config['window'] = %d, need 2 <= window <= 64" % window)
        if int(params["rank"]) > 64:
            raise ValueError("refit_joint(hstep=True): params['rank'] = %d, at most 64 is supported" % int(params["rank"]))
        if max(lengths, default=0) < window:
            raise ValueError("refit_joint(hstep=True): no trial is as long as the window (%d)" % window)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"], "w": tr["w"],
              "v": tr["v"] if tr.get("v") is not None else np.zeros((T, L))} for tr, T in zip(trials, lengths)]
    work = SET_TRIALS  # the set the loop runs on
    if missing is not None:
        # private copies of y with 0.0 in the holes: the by-row passes behind update_w leave an entry out by a zero
        # coefficient, under which a NaN in the caller's y would survive.  The fill value reaches no result.
        for u, m in zip(units, missing):
            u["y"] = np.where(m, 0.0, u["y"]).astype(float)
        mask_rows = np.concatenate(missing, axis=0)
        work = SET_TRIALS_MASKED
    trace = {"laplace": [], "n_newton": [], "converged": []}
    m_args = (int(config["Mniter"]), config["use_hessian"], config["eps"], config["learning_rate"], config["da_bound"],
              config["db_bound"])
    out_params = dict(params)
    with E.Engine.for_params(params, device) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET_TRIALS, units)
        if missing is not None:  # the masked fit set: the same rows, one mask bit per entry, the source's mu, v, w
            eng.replicate(SET_TRIALS, SET_TRIALS_MASKED, held_out=mask_rows[None])
        mstep = eng.mstep_cov if missing is None else eng.mstep_cov_masked
        bind_priors(eng, trials, out_params)  # (its own dict: the caller's params["cholesky"] stays as it is)
        cur = (np.array(params["a"], dtype=float), np.array(params["b"], dtype=float), np.array(params["noise"], dtype=float),
               None, None)
        # with hstep: omega_k and the factors that belong to it, on the host ({T: (L, T, R)}) to go back to
        hyper = (np.array(params["omega"], dtype=float), out_params["cholesky"]) if hstep else None
        prior_lengths = sorted(set(lengths))
        if hstep:
            trace["omega"] = []
        prev = None  # (parameters, posterior, evidence, omega and factors) of the iteration before
        k = 0
        while True:
            post = eng.joint_posterior(work, max_iter=newton_iter, tol=newton_tol, window=window)
            if post["n_failed"]:
                raise E.VlgpError("refit_joint: H of %d trial(s) could not be factored at iteration %d"
                                  % (post["n_failed"], k))
            ev = float(np.sum(post["laplace"]))
            trace["laplace"].append(ev)
            trace["n_newton"].append(int(np.max(post["n_newton"])))
            trace["converged"].append(bool(np.all(post["converged"])))
            if hstep:
                trace["omega"].append(hyper[0].copy())
            echo("refit_joint %d: laplace %.6f, Newton %d%s" % (k, ev, trace["n_newton"][-1],
                                                              "" if trace["converged"][-1] else " (not converged)"))
            if prev is not None and ev - prev[2] <= tol * abs(ev):
                if not ev >= prev[2]:
                    cur, post = prev[0], prev[1]
                    eng.set_params(*cur[:3])
                    if hstep:  # the previous omega and its factors, as they were
                        hyper = prev[3]
                        for T in prior_lengths:
                            eng.set_prior(T, hyper[1][T])
                break
            if k == max_iter:
                break
            prev = (cur, post, ev, hyper)
            bad = mstep(work, post["mu"], post["cov"], *m_args)
            if bad:
                logger.error("%d Newton systems were singular (gradient step taken)", bad)
            cur = eng.get_params()
            if hstep:
                omega, _ = gp.optimize_joint(post["window_moments"], post["n_windows"], dict(out_params, omega=hyper[0]), config)
                eng.build_prior(prior_lengths, omega, params["sigma"])
                hyper = (omega, {T: eng.get_prior(T) for T in prior_lengths})
            k += 1
        # w of the mode under the returned parameters, which the engine holds
        v = np.ascontiguousarray(np.diagonal(post["cov"], axis1=1, axis2=2))
        if missing is not None:
            eng.free_units(SET_TRIALS_MASKED)  # (its source takes no new contents while a replica aliases its rows)
        eng.upload(SET_TRIALS, [dict(u, mu=post["mu"][s:e], v=v[s:e]) for u, s, e in zip(units, bounds[:-1], bounds[1:])])
        if missing is not None:
            eng.replicate(SET_TRIALS, SET_TRIALS_MASKED, held_out=mask_rows[None])
        eng.update_w(work)
        w = eng.download(work, ("w",))["w"]
    out_trials = []
    for i, (tr, s, e) in enumerate(zip(trials, bounds[:-1], bounds[1:])):
        out_trials.append(dict(tr, mu=post["mu"][s:e].copy(), v=v[s:e].copy(), cov=post["cov"][s:e].copy(), w=w[s:e].copy()))
        if missing is not None:
            out_trials[-1]["missing"] = missing[i]
    a, b, noise, da, db = cur
    out_params.update(a=a, b=b, noise=noise)
    if da is not None:
        out_params.update(da=da, db=db)
    if hstep:
        out_params.update(omega=hyper[0], cholesky=dict(hyper[1]))
    out_config = dict(config)
    out_config["runtime"] = dict(config.get("runtime") or {}, joint=trace)
    return {"trials": out_trials, "params": out_params, "config": out_config}


def _full_factors(eng, lengths, params):
    """``{T: (L, T, R)}`` for the listed lengths: ``params["cholesky"][T]`` where present, the rest built on the device
    from ``omega, sigma`` as ``bind_priors`` builds them.  Leaves the engine's prior table empty, ``params`` as it is."""
    chol = params.get("cholesky") or {}
    out = {T: np.asarray(chol[T], dtype=float) for T in lengths if T in chol}
    missing = [T for T in lengths if T not in out]
    if missing:
        eng.build_prior(missing, params["omega"], params["sigma"])
        for T in missing:
            out[T] = eng.get_prior(T)
        eng.clear_prior()
    return out


@contextlib.contextmanager
def _extended(trials, held_in, n_ext, params, config, n_iter, device):
    """What ``forecast`` and ``evaluation.forward_prediction`` share.  Trial ``i`` is held in up to row ``held_in[i]``
    and extended by ``n_ext`` rows: the factor of length ``held_in[i] + n_ext`` gives its first rows as the prior of the
    held-in length and its last ``n_ext`` as the extension rows; the latents are inferred on the held-in rows from a
    zero start (``n_iter`` sweeps, default ``config["max_iter"]``, as ``evaluation.leave_group_out`` infers its own)
    and carried forward by ``Engine.forecast``.  Yields ``(eng, mu_ext, v_ext, fit_terms, n_failed)`` with the held-in
    rows still resident as set ``SET_TRIALS``; ``n_failed`` adds the E-step's failed updates and the failed tasks of
    the extension."""
    L = int(params["zdim"])
    n_iter = int(config["max_iter"] if n_iter is None else n_iter)
    vb = config["method"] == "VB"
    units = [{"y": tr["y"][:T], "x": None if tr.get("x") is None else tr["x"][:T],
              "mu": np.zeros((T, L)), "v": np.zeros((T, L)), "w": np.zeros((T, L))} for tr, T in zip(trials, held_in)]
    with E.Engine.for_params(params, device) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        full = _full_factors(eng, sorted({T + n_ext for T in held_in}), params)
        for T, G in full.items():  # (distinct total lengths give distinct held-in lengths: nothing collides)
            eng.set_prior(T - n_ext, G[:, :T - n_ext])
        eng.upload(SET_TRIALS, units)
        n_failed = eng.estep(SET_TRIALS, n_iter, config["dmu_bound"], vb)
        mu_ext, v_ext, terms, bad = eng.forecast(SET_TRIALS, {T - n_ext: G[:, T - n_ext:] for T, G in full.items()}, vb=vb)
        yield eng, mu_ext, v_ext, terms, int(n_failed) + int(bad)


def forecast(trials, params, config, n_ahead, n_iter=None, device=0):
    """Latents of new trials with fitted parameters, and their forecast ``n_ahead`` bins past the end of every trial
    (``vlgp_amd.evaluation``'s module docstring defines the extension).

    The prior of a trial of ``T`` bins is the first ``T`` rows of the factor of length ``T + n_ahead``
    (``params["cholesky"][T + n_ahead]`` where present, otherwise built from ``omega, sigma`` on the device); its last
    ``n_ahead`` rows carry the posterior forward.  Inference starts from zero and runs ``n_iter`` E-step iterations
    (default ``config["max_iter"]``).  ``trials`` (``y``, and ``x`` with regressors) and ``params`` are not modified.

    Returns a list with one dict per trial: ``mu``, ``v``, ``w`` (T, L) of the observed bins and ``mu_ahead``,
    ``v_ahead`` (n_ahead, L).  No rates: there are no future regressors.  A (trial, latent) whose posterior could not be
    factored has NaN in its ``mu_ahead``, ``v_ahead`` column."""
    if isinstance(n_ahead, bool) or not isinstance(n_ahead, (int, np.integer)) or n_ahead < 1:
        raise ValueError("n_ahead must be an integer >= 1, got %r" % (n_ahead,))
    n_ahead = int(n_ahead)
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    with _extended(trials, lengths, n_ahead, params, config, n_iter, device) as (eng, mu_ext, v_ext, _, _):
        state = eng.download(SET_TRIALS, ("mu", "v", "w"))
    bounds = np.cumsum([0] + lengths)
    out = []
    for i in range(len(trials)):
        rows, ahead = slice(bounds[i], bounds[i + 1]), slice(i * n_ahead, (i + 1) * n_ahead)
        out.append({"mu": state["mu"][rows].copy(), "v": state["v"][rows].copy(), "w": state["w"][rows].copy(),
                    "mu_ahead": mu_ext[ahead].copy(), "v_ahead": v_ext[ahead].copy()})
    return out


def sample_posterior(trial, params, nsamples, reg=1e-6, rng=None, device=0):
    """Draw ``nsamples`` latent trajectories from the variational posterior of one trial
    (vlgp/api.py:142-168): independent Gaussians per latent with mean ``mu[:, l]`` and covariance
    ``(K_l^-1 + W_l)^-1``, ``K_l = G_l G_l'`` the low-rank prior of this trial length.

    The reference forms the T x T matrices (two dense inverses per latent plus
    ``multivariate_normal``'s SVD: O(T^3)).  With ``H = G'WG`` (r x r) the same covariance is
    ``G (I + H)^-1 G'`` (the reference's ``reg`` regulariser set to zero; it only exists to make
    ``K`` invertible), so a draw is ``mu + G L^-T eps`` with ``L L' = I + H`` and ``eps ~ N(0, I_r)``:
    O(T r^2) per latent, computed on the GPU (``vlgp_sample_posterior``).  ``reg`` is accepted and ignored.
    The standard normal draws come from ``rng`` (a ``numpy.random.Generator``/``RandomState``) or, like
    the reference, the global NumPy state: ``(r_l, nsamples)`` values per latent, in latent order.

    Returns an array of shape (nsamples, bins, nfactors)."""
    del reg
    mu = np.ascontiguousarray(trial["mu"], dtype=float)
    w = np.ascontiguousarray(trial["w"], dtype=float)
    nbins, nfactors = mu.shape
    G = np.ascontiguousarray(params["cholesky"][nbins], dtype=float)
    R = G.shape[-1]
    if rng is None:
        normal = np.random.standard_normal
    elif hasattr(rng, "standard_normal"):
        normal = rng.standard_normal
    else:  # anything with normal(loc, scale, size)
        normal = lambda shape: rng.normal(size=shape)
    eps = np.zeros((nfactors, R, int(nsamples)))
    for l in range(nfactors):
        nz = np.flatnonzero(np.any(G[l] != 0.0, axis=0))  # columns ichol_gauss left at zero carry nothing
        r = int(nz[-1]) + 1 if nz.size else 1
        eps[l, :r] = normal((r, int(nsamples)))
    out = np.empty((int(nsamples), nbins, nfactors))
    import ctypes as C

    from ._lib import dptr

    # the latents are independent: more than a handle holds (16) go through in groups
    for l0 in range(0, nfactors, 16):
        sl = slice(l0, min(l0 + 16, nfactors))
        nl = sl.stop - sl.start
        mu_c, w_c, G_c, eps_c = (np.ascontiguousarray(arr) for arr in (mu[:, sl], w[:, sl], G[sl], eps[sl]))
        out_c = out if nl == nfactors else np.empty((int(nsamples), nbins, nl))
        with E.Engine(2, nl, 1, R, device=device) as eng:
            bad = C.c_int(0)
            eng._ck(eng.lib.vlgp_sample_posterior(eng.h, nbins, dptr(mu_c), dptr(w_c), dptr(G_c), int(nsamples),
                                                  dptr(eps_c), dptr(out_c), C.byref(bad)))
            if bad.value:
                logger.error("I + G'WG was not positive definite for %d latent(s): their draws equal the mean",
                             bad.value)
        if out_c is not out:
            out[:, :, sl] = out_c
    return out
