"""Held-out evaluation of a vLGP fit: log-likelihood and leave-one-neuron-out prediction on the GPU.

Definitions (the tests hold the code to them).  For channel ``n`` at row ``t`` of a posterior ``(mu, v)``:

- plug-in rate, Poisson: ``trunc_exp(a[:, n] . mu[t] + b[:, n] . x[t, :, n] + 1/2 (a[:, n] ** 2) . v[t])`` -- the rate
  the E-step itself uses (``esplit_pass``).  Under MAP (``method != "VB"``) the ``v`` term is left out: the E-step keeps
  ``v`` at 0 there.
- plug-in mean, Gaussian: ``eta = a[:, n] . mu[t] + b[:, n] . x[t, :, n]``.
- log-likelihood of ``y[t, n]``: Poisson ``y log rate - rate - lgamma(y + 1)``; Gaussian
  ``-1/2 log(2 pi noise[n]) - (y - eta) ** 2 / (2 noise[n])``.
- leave-one-out for channel ``n``: ``transform`` with ``a[:, n] = 0`` (every other parameter unchanged), started from
  ``mu = v = w = 0`` (channel ``n`` cannot leak in through the factor-analysis start), ``n_iter`` E-step iterations;
  channel ``n`` is then predicted from those latents with its ORIGINAL loading.  Its regressors (its own spike history
  when ``history > 0``) enter its prediction as the model defines: only the latents are inferred without it.
- bits per spike of a Poisson channel: ``(LL_model - LL_null) / (sum y * ln 2)``, ``LL_null`` the log-likelihood of a
  constant rate at the channel's mean count over the evaluated rows (the ``lgamma`` terms cancel).  Gaussian channels,
  and channels without a spike, get NaN.

Every sum is a fixed-order device reduction (``vlgp_loglik``): the results are the same bits on every run.
"""
import math

import numpy as np

from . import engine as E
from ._lib import VlgpError
from .api import bind_priors

__all__ = ["loglik", "leave_one_out", "plan_chunks", "bits_per_spike", "REPLICA_BUDGET_BYTES"]

SET_TEST, SET_REPLICAS = 0, 2

# Device memory the batched leave-one-out may hold in replicas at once.  A replica costs about ten doubles per
# (row, latent): its mu, v, w, dmu and the split E-step's scratch (latent-major copies, residual projections, factors)
# -- 16 MB at 40 trials x 1000 bins, L = 5, so the 100 replicas of that test set take about 1.6 GB and fit in one chunk.
REPLICA_BUDGET_BYTES = 2 << 30
_DOUBLES_PER_ROW_LATENT = 10


def plan_chunks(channels, max_replicas):
    """Split ``channels`` into consecutive chunks of at most ``max_replicas``: every channel exactly once, in order."""
    channels = list(channels)
    step = max(int(max_replicas), 1)
    return [channels[i:i + step] for i in range(0, len(channels), step)]


def default_max_replicas(rows, n_latents, budget=REPLICA_BUDGET_BYTES):
    """Replicas of a ``rows``-row test set that fit ``budget`` bytes (at least one)."""
    per = _DOUBLES_PER_ROW_LATENT * 8 * max(int(rows), 1) * max(int(n_latents), 1)
    return max(int(budget // per), 1)


def bits_per_spike(sums, rows, gauss=None):
    """Per channel: ``(ll, ll_null, n_spikes, bits_per_spike)`` from ``vlgp_loglik``'s Poisson sums
    (``sum ll, sum y, sum rate, sum lgamma(y + 1)``) over ``rows`` rows.  Gaussian channels (``gauss``) get NaN."""
    sums = np.asarray(sums, dtype=float)
    ll, ny, lg = sums[:, 0], sums[:, 1], sums[:, 3]
    gauss = np.zeros(len(ll), dtype=bool) if gauss is None else np.asarray(gauss, dtype=bool)
    ybar = ny / float(rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        ll_null = np.where(ny > 0, ny * np.log(ybar), 0.0) - rows * ybar - lg
        bps = (ll - ll_null) / (ny * math.log(2.0))
    bps = np.where(gauss | ~(ny > 0), np.nan, bps)
    ll_null = np.where(gauss, np.nan, ll_null)
    return ll, ll_null, ny, bps


def _engine(params, device):
    gauss = np.asarray(params["likelihood"]) == "gaussian"
    return E.Engine(params["ydim"], params["zdim"], params["xdim"], params["rank"], gauss, device=device), gauss


def loglik(fit, per_channel=False, device=0):
    """Log-likelihood of a fit's own trials under their own posterior (``mu``, ``v``): a float, or the per-channel
    sums with ``per_channel=True``.

    Replaces the reference's ``vlgp.evaluation.loglik`` (same call: the ``fit`` result dict in, a float out), which
    exponentiates the rate twice and expects shapes ``fit`` does not produce.  Here the rate is the E-step's own plug-in
    rate (module docstring), the Poisson term includes ``-lgamma(y + 1)``, Gaussian channels are scored with their
    noise variance, and the sum runs over every (row, channel) of every trial."""
    trials, params, config = fit["trials"], fit["params"], fit.get("config") or {}
    vb = config.get("method", "VB") == "VB"
    L = params["zdim"]
    units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"], "v": tr.get("v", np.zeros((tr["y"].shape[0], L))),
              "w": None} for tr in trials]
    eng, _ = _engine(params, device)
    with eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET_TEST, units)
        sums, _ = eng.loglik(SET_TEST, vb=vb)
    per = sums[:, 0].copy()
    return per if per_channel else float(np.sum(per))


def _is_refusal(err):
    text = str(err)
    return "status -3" in text and "replicated set" in text


def leave_one_out(trials, params, config, channels=None, n_iter=None, path="auto", max_replicas=None, device=0):
    """Leave-one-neuron-out prediction of held-out trials (module docstring for the definitions).

    ``trials``: dicts with ``y`` (T, N) and, with regressors, ``x`` (T, xdim, N); their ``mu``, ``v``, ``w`` are not
    read or written.  ``channels``: the channels to leave out in turn (default all).  ``n_iter``: E-step iterations
    (default ``config["max_iter"]``, as ``core.infer``).  ``path``: ``"batched"`` runs every left-out channel as a replica
    of the test set in one E-step (``vlgp_replicate_units``), ``max_replicas`` at a time (default: what
    ``REPLICA_BUDGET_BYTES`` holds); ``"sequential"`` runs one E-step per channel with its loading zeroed; ``"auto"``
    takes the batched path unless the device refuses it (the split E-step cannot run the configuration, e.g. L > 10).
    Both paths give the same bits when they run the same E-step kernels.

    Returns a dict: ``channels``; ``rate``, a list per trial of (T, len(channels)) plug-in rates (Gaussian: means);
    per channel ``ll``, ``ll_null``, ``n_spikes``, ``bits_per_spike``; ``n_failed`` (singular posterior updates);
    ``path`` (``"batched"`` or ``"sequential"``)."""
    if path not in ("auto", "batched", "sequential"):
        raise ValueError("path must be 'auto', 'batched' or 'sequential'")
    N, L = int(params["ydim"]), int(params["zdim"])
    channels = list(range(N)) if channels is None else [int(c) for c in channels]
    if not channels or len(set(channels)) != len(channels) or min(channels) < 0 or max(channels) >= N:
        raise ValueError("channels must be distinct indices in [0, %d)" % N)
    n_iter = int(config["max_iter"] if n_iter is None else n_iter)
    vb = config["method"] == "VB"
    dmu_bound = config["dmu_bound"]
    a = np.array(params["a"], dtype=float)
    b = np.array(params["b"], dtype=float)
    noise = np.array(params["noise"], dtype=float)
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    rows = int(sum(lengths))
    units = [{"y": tr["y"], "x": tr.get("x"), "mu": np.zeros((T, L)), "v": np.zeros((T, L)), "w": np.zeros((T, L))}
             for tr, T in zip(trials, lengths)]
    K = len(channels)
    rate = np.empty((rows, K))
    sums = np.empty((K, 4))
    n_failed = 0
    used = "batched" if path != "sequential" else "sequential"
    eng, gauss = _engine(params, device)
    with eng:
        eng.set_params(a, b, noise)
        eng.upload(SET_TEST, units)
        bind_priors(eng, trials, dict(params))  # (a copy: the caller's params["cholesky"] stays as it is)
        if used == "batched":
            cap = default_max_replicas(rows, L) if max_replicas is None else int(max_replicas)
            done = 0
            try:
                for chunk in plan_chunks(channels, cap):
                    eng.replicate(SET_TEST, SET_REPLICAS, chunk)
                    n_failed += eng.estep(SET_REPLICAS, n_iter, dmu_bound, vb)
                    s, r = eng.loglik(SET_REPLICAS, vb=vb, want_rate=True)
                    eng.free_units(SET_REPLICAS)
                    sums[done:done + len(chunk)] = s
                    rate[:, done:done + len(chunk)] = r
                    done += len(chunk)
            except VlgpError as err:
                if path == "batched" or not _is_refusal(err):
                    raise
                if SET_REPLICAS in eng.sets:
                    eng.free_units(SET_REPLICAS)
                used, n_failed = "sequential", 0
        if used == "sequential":
            for i, n in enumerate(channels):
                a_out = a.copy()
                a_out[:, n] = 0.0
                eng.set_params(a_out, b, noise)
                eng.upload(SET_TEST, units)  # (mu = v = w = 0 again)
                n_failed += eng.estep(SET_TEST, n_iter, dmu_bound, vb)
                eng.set_params(a, b, noise)
                s, r = eng.loglik(SET_TEST, vb=vb, want_rate=True)
                sums[i] = s[n]
                rate[:, i] = r[:, n]
    ll, ll_null, ny, bps = bits_per_spike(sums, rows, gauss[channels])
    bounds = np.cumsum([0] + lengths)
    return {
        "channels": channels,
        "rate": [rate[bounds[i]:bounds[i + 1]].copy() for i in range(len(trials))],
        "ll": ll, "ll_null": ll_null, "n_spikes": ny, "bits_per_spike": bps,
        "n_failed": int(n_failed), "path": used,
    }
