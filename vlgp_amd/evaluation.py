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
- leave-group-out (co-smoothing) for a set ``g`` of channels: the same with ``a[:, g] = 0`` -- one inference for the
  whole set -- and every channel of ``g`` predicted from those latents with its original loading.  Singleton groups are
  leave-one-out, bit for bit.
- leave-entries-out (speckled hold-out) for a set ``S`` of single (row, channel) entries: the E-step with the likelihood
  terms of the entries of ``S`` removed -- their working residual ``res[t, n]`` and curvature ``U[t, n]`` are 0, and with
  them their contributions to ``y . a``, to ``w`` and to the Gaussian constant of ``w`` -- from ``mu = v = w = 0``,
  ``n_iter`` iterations; every entry of ``S`` is then predicted from those latents with its channel's loading.  Nothing
  else changes: the regressors ``x`` enter as the caller gave them, so with ``history > 0`` they hold the held-out counts
  of earlier bins, as in leave-one-out.  A set that is constant along the rows is leave-group-out, bit for bit.  A row
  with every entry held out has ``w = 0``: its latents come from the prior and the neighbouring rows alone.
- ``entry_folds``: ``np.random.default_rng(seed).permutation(rows * N).reshape(rows, N) % n_folds`` -- every entry in
  exactly one fold, fold sizes differing by at most one.  ``leave_entries_out`` runs one replica per fold.
- speckled bits per spike of a Poisson channel: as below, with the sums over the channel's held-out entries (all folds)
  and ``LL_null`` a constant rate at the channel's mean count over those entries; ``speckled_bps`` pools the channels
  as ``co_bps`` does.
- bits per spike of a Poisson channel: ``(LL_model - LL_null) / (sum y * ln 2)``, ``LL_null`` the log-likelihood of a
  constant rate at the channel's mean count over the evaluated rows (the ``lgamma`` terms cancel).  Gaussian channels,
  and channels without a spike, get NaN.
- co-smoothing bits per spike: ``co_bps = (sum ll - sum ll_null) / (sum n_spikes * ln 2)``, the sums over the Poisson
  channels with at least one spike (in channel-list order); NaN when there is none.

Variational lower bound (``elbo``).  For one trial of length ``T``, latent ``l``, ``G = params["cholesky"][T][l]`` with
its all-zero columns dropped (``T x r``), ``w = w[:, l]``, ``mu = mu[:, l]``:

- ``H = I_r + G' diag(w) G``, ``S = H^-1``; the posterior the E-step works with is ``q(x_l) = N(mu, G S G')``, whose
  diagonal is the stored ``v[:, l]``.
- ``beta = argmin |G beta - mu|``; ``off_prior = |mu - G beta|^2 / max(|mu|^2, tiny)`` is reported: the KL against a
  rank-``r`` prior exists only for ``mu`` in the range of ``G``.
- ``KL[trial, l] = 1/2 (tr S + beta'beta - r + log det H)``.
- expected log-likelihood of ``y[t, n]``, ``eta = a[:, n] . mu[t] + b[:, n] . x[t, :, n]``,
  ``s = 1/2 (a[:, n] ** 2) . v[t]``: Poisson ``y eta - trunc_exp(eta + s) - lgamma(y + 1)``; Gaussian
  ``-1/2 log(2 pi noise[n]) - ((y - eta) ** 2 + 2 s) / (2 noise[n])``.
- ``ELBO = sum E_q log p(y | x) - sum KL``.  Under MAP (``method != "VB"``: a point estimate, no entropy) ``elbo`` and
  ``kl`` are NaN and ``log_joint = sum log p(y | mu) - 1/2 sum beta'beta`` is reported instead.

Forward prediction (``forward_prediction``, ``vlgp_amd.forecast``): a posterior extended past its observed bins.  Take
one unit and one latent ``l``.  ``G`` is the compact prior factor bound to the unit's length (``T_in x r``; compact: the
leading non-zero columns, as everywhere in the engine), ``G_ext`` (``n_ext x R``) holds the rows of the same
factorisation that belong to the unobserved bins, ``mu``, ``v``, ``w`` are the unit's stored posterior columns.

- working gradient, the E-step's own residual: ``g[t] = sum_n a[l, n] res[t, n]``; Poisson
  ``res = y - trunc_exp(eta + 1/2 (a ** 2) . v)``, Gaussian ``res = (y - eta) / noise``, ``eta = a . mu + (b x)``; the
  ``v`` term is dropped under MAP.
- weight-space posterior: ``x = G beta`` with ``beta ~ N(0, I_r)`` a priori; ``H = I_r + G' diag(w) G``, ``S = H^-1``,
  ``beta_hat = S G' (g + w o mu)``.  ``G beta_hat`` is exactly the next unclipped Newton iterate of the E-step (push-through
  identity ``(I + G G' W)^-1 G = G (I + G'WG)^-1``); at the E-step's fixed point ``beta_hat = G' g``.  Neither the
  least-squares form ``argmin |G beta - mu|`` (top-row slices of a pivoted factor reach ``cond(G) = 5e8``) nor the bare
  fixed-point form ``G' g`` (1e8 in relative size three sweeps from a cold start) is used.
- extension: ``mu_ext = G_ext[:, :r] beta_hat``;
  ``v_ext[t] = |Lc^-1 G_ext[t, :r]'|^2 + sum_{c >= r} G_ext[t, c]^2`` with ``Lc Lc' = H``.  A column that is zero on every
  held-in row but not on the extension rows is a weight the data never saw: it keeps its prior variance of 1, which
  is the second term.  Under MAP ``v_ext = 0``.
- convergence report per (unit, latent): ``{|G beta_hat - mu|^2, |mu|^2}``; their ratio is ``off_fixed_point``.
- forward-predicted rate of channel ``n`` at an extension row: the plug-in rate above, evaluated with ``mu_ext``,
  ``v_ext`` and that row's own regressors.  With ``history > 0`` those regressors contain the held-out spikes, so the
  prediction is ONE STEP AHEAD: bin ``t`` is predicted from the latents inferred on the held-in bins and the spikes up
  to ``t - 1``.
- ``bits_per_spike_past``: bits per spike against a constant rate at the channel's mean count over the HELD-IN rows --
  what is known at prediction time -- NaN where that mean is 0 and for Gaussian channels.

Marginal likelihood (``marginal_loglik``, ``vlgp_marginal``): the importance-sampling (IWAE) estimate of
``log p(y_trial)`` with the fitted posterior as proposal.  For one unit of length ``T`` and latent ``l``:

- ``G`` (``T x r``) is the compact prior factor bound to the unit's length; ``mu, v, w`` are the unit's stored columns.
- ``g``, ``z = g + w o mu``, ``H = I_r + G' diag(w) G = Lc Lc'`` and ``m = H^-1 G' z`` are exactly those of the forward
  prediction above (``m`` is its ``beta_hat``).  Under MAP the ``v`` term of ``g`` is dropped, and the proposal
  ``N(m, H^-1)`` is then the Laplace approximation of the MAP fit.
- draw ``k`` takes ``eps_k`` in ``R^r`` (standard normals supplied by the host), ``d = Lc^-T eps_k`` and
  ``beta_k = m + d``.
- ``c[u, l, k] = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H``: ``log N(beta; 0, I) - log N(beta; m, H^-1)``.
- the path is ``x_k[t, l] = G[t, :] . beta_k``.
- ``ll[u, k] = sum_t sum_n log p(y[t, n] | eta = a[:, n] . x_k[t] + (b x)_tn)`` with no ``v`` term, because ``x_k`` is a
  sample: Poisson ``y eta - trunc_exp(eta) - lgamma(y + 1)``; Gaussian
  ``-1/2 log(2 pi noise[n]) - (y - eta) ** 2 / (2 noise[n])``.
- ``log_w[u, k] = ll[u, k] + sum_l c[u, l, k]``.
- per unit ``iwae = logsumexp_k(log_w) - log K``, ``elbo_mc = mean_k log_w`` and ``ess = (sum w)^2 / sum w^2``.

``mean_k w`` is unbiased for ``p(y_u)`` whatever ``mu, v, w`` hold; the stored posterior only decides the variance of the
estimate, which ``ess`` (between 1 and ``K``) reports: near 1 a single draw carries the sum and ``iwae`` is little more
than that draw's ``log_w``.

Joint Laplace posterior (``joint_posterior``, ``marginal_loglik(proposal="joint")``, ``vlgp_joint_laplace``).  Every
posterior above is mean-field over latents; the posterior over ALL prior weights ``beta = (beta_1 ... beta_L)`` of a unit
is log-concave and of small dimension ``D = sum_l r_l`` (at most 512 here), so a joint Newton iteration finds its mode.
With ``G_l`` (``T x r_l``) the compact prior factor of latent ``l`` and the stacked index ``(l, i)`` latent-major:

- ``x[t, l] = G_l[t, :] . beta_l`` and ``eta[t, n] = a_n . x[t] + (b x)_tn`` -- no ``v`` term: the model of ``ll`` above.
- Poisson channels: ``lam = trunc_exp(eta)``, ``ll = y eta - lam - lgamma(y + 1)``, ``res = y - lam``, ``cur = lam``.
  Gaussian channels: ``ll = -log(2 pi noise_n) / 2 - (y - eta) ** 2 / (2 noise_n)``, ``res = (y - eta) / noise_n``,
  ``cur = 1 / noise_n``.
- objective ``f(beta) = 1/2 |beta|^2 - sum_t sum_n ll``; gradient ``grad_l f = beta_l - G_l' g[:, l]`` with
  ``g[t, l] = sum_n a[l, n] res[t, n]``.
- Hessian ``H[(l, i), (l', j)] = delta + sum_t G_l[t, i] c[t, l, l'] G_l'[t, j]`` with
  ``c[t, l, l'] = sum_n a[l, n] a[l', n] cur[t, n]``; its diagonal blocks are ``I + G_l' diag(w_l) G_l`` with the engine's
  own ``w``.  ``H = Lc Lc'``.
- the mode ``beta_hat`` is the zero of ``grad f``, unique while no ``eta`` is above the clamp of ``trunc_exp``: results are
  pinned by stationarity, not by the path taken.
- Newton start: the mean-field centres ``m_l`` above from the set's current ``mu, w``, with the ``v`` term dropped.
  Step ``d = H^-1 grad f``; a unit stops when its decrement ``grad f' H^-1 grad f <= tol`` or after ``max_iter``
  factorisations.  The trial point ``beta - s d``, ``s = 1``, is accepted when
  ``f(beta - s d) <= f(beta) - 1e-4 s decrement + 2 ** -46 (1/2 |beta - s d|^2 + sum |ll terms|)`` (the last term: the
  rounding of the sum); otherwise ``s`` is halved, and below ``2 ** -30`` the unit stops where it stands, not converged.
- ``laplace = ll(beta_hat) - 1/2 |beta_hat|^2 - 1/2 log det H(beta_hat)``, the Laplace evidence ``log p(y_unit)``.
- ``mu[t, l] = G_l[t, :] . beta_hat_l`` and ``v[t, l] = G_l[t, :] (H^-1)_ll G_l[t, :]'``.
- draw ``k``: ``beta_k = beta_hat + Lc^-T eps_k``, ``c_k = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H``,
  ``log_w[u, k] = ll(beta_k) + c_k``; ``mean_k exp(log_w)`` is unbiased for ``p(y_u)`` whatever ``beta_hat`` is.

Posterior-predictive density (``predictive=True`` in ``loglik``, ``leave_one_out``, ``leave_group_out``,
``leave_entries_out``, ``forward_prediction``; ``Engine.predictive``, ``vlgp_predictive``).  The plug-in log-likelihood
above sees the posterior variance ``v`` only through the mean of the rate: a posterior that is confidently wrong and one
that is honestly uncertain score the same when their means agree.  The predictive score integrates the likelihood over
the posterior of the linear predictor instead,

    ``lpd[t, n] = log int p(y[t, n] | eta) N(eta; m, s2) d eta``,
    ``m = a[:, n] . mu[t] + b[:, n] . x[t, :, n]``, ``s2 = (a[:, n] ** 2) . v[t]`` (``s2 = 0`` under MAP).

- Gaussian channel: ``lpd = -1/2 log(2 pi (noise[n] + s2)) - (y - m) ** 2 / (2 (noise[n] + s2))``; ``rate = m``.
- Poisson channel: ``rate = trunc_exp(m + s2 / 2)``, the plug-in rate, which is also the predictive mean below the clamp
  of ``trunc_exp``.  With ``s2 < 1e-30``, ``lpd`` is the plug-in log-likelihood above: MAP fits and ``v == 0`` reproduce
  the plug-in score.  Otherwise the Poisson-lognormal integral has no closed form and is taken by a Gauss-Hermite rule
  CENTRED AT THE MODE of the integrand (at the posterior mean the 12-point rule is off by more than 3 nats where ``y``
  disagrees with the mean).  With ``ex(e) = exp(min(e, 10))``, ``(x_q, w_q) = hermgauss(n_nodes)``, ``z_q = sqrt(2) x_q``
  and ``lwa_q = log(w_q / sqrt(pi)) + x_q ** 2`` (``hermite_nodes``):

  - start ``e = min(log y, m + y s2)`` if ``y > ex(m)``, else ``e = m``; eight Newton steps
    ``e -= (y - ex(e) - (e - m) / s2) / (-ex(e) - 1 / s2)`` on ``g(e) = y e - ex(e) - (e - m) ** 2 / (2 s2)``.  The start
    lies right of the mode or one bounded step left of it, ``g'`` is decreasing and concave, so the iteration then
    descends monotonically.  The fixed count and the start are part of the definition; the centre only decides the
    accuracy of the rule, never its validity.
  - ``h = s2 ex(e) + 1``, ``tau = sqrt(s2) / sqrt(h)``, ``eta_q = e + tau z_q``, ``c_q = min(eta_q, 10)``,
    ``t_q = lwa_q + y c_q - exp(c_q) - (eta_q - m) ** 2 / (2 s2)``.
  - ``lpd = -1/2 log h + logsumexp_q t_q - lgamma(y + 1)``.  ``n_nodes = 1`` is the Laplace approximation.

  Accuracy against a brute-force integral, worst absolute error in ``lpd`` over ``m`` in [-8, 5], ``sqrt(s2)`` in
  [0.02, 1], ``y`` in [0, 100]: 1.5e-6 at 12 nodes, 2.0e-8 at 20 (``tests/test_predictive_host.py`` holds the definition
  to 1e-5 and 1e-7).  Far outside that regime the rule degrades: at ``sqrt(s2) = 3, y = 0`` and 12 nodes it is off by 0.06
  for ``m = 9``, and for ``m = 11`` eight Newton steps from ``e = m`` no longer reach the mode: several nats.
- The sums keep ``vlgp_loglik``'s slots with ``sum lpd`` in the first, so every score built on them (``bits_per_spike``,
  ``co_bps``, ``speckled_bps``, ``fp_bps``) is computed as before and the null model is unchanged; a result scored this
  way carries ``"density": "predictive"``.  By Jensen's inequality ``lpd`` of a Poisson entry is never below its
  expected log-likelihood (``elbo``'s per-entry term).

Calibration of the predictive distribution (``calibration``, ``calibration_from_sums``, ``Engine.calibration``,
``vlgp_calibration``).  A log score ranks models; it does not say whether the predictive distribution is the right one.
Per scored entry, with ``m``, ``s2`` and ``rate`` as above:

- Poisson channel, ``k = y``: ``p(j) = exp(lpd)`` of the count ``j``, exactly the predictive mass above (the mode-centred
  ``n_nodes``-point rule, or the plug-in Poisson mass when ``s2 < 1e-30``); ``lo = F(k - 1) = sum_{j < k} p(j)`` added in the
  order ``j = 0, 1, ...``, ``hi = lo + p(k)``, then both clipped to ``<= 1``.  One Gauss-Hermite rule centred at ``m`` on
  the Poisson distribution function is NOT used: at 12 nodes it is off by 2e-2 at ``sqrt(s2) = 0.3``.  The sum of masses
  is within 8e-9 of a dense trapezoid for ``sqrt(s2) <= 0.5`` at 12 nodes, 1.2e-6 at 1.0 (4e-11 at 32 nodes).
- Gaussian channel: ``lo = hi = 1/2 erfc(-(y - m) / sqrt(2 (noise[n] + s2)))``.
- PIT histogram, ``n_bins = J``, edges ``e_j = j / J`` (the non-randomised PIT of Czado, Gneiting & Held 2009): an entry
  with ``hi > lo`` adds ``clip((e_{j+1} - lo) / (hi - lo), 0, 1) - clip((e_j - lo) / (hi - lo), 0, 1)`` to bin ``j``, one with
  ``hi == lo`` adds 1 to bin ``min(J - 1, floor(lo J))``: every entry adds total mass 1.
- coverage of the central interval of level ``c``, ``a = (1 - c) / 2``: covered iff ``hi >= a`` and ``lo < 1 - a`` -- for
  counts exactly ``q_a <= y <= q_{1-a}`` with ``q_p = min{k : F(k) >= p}``.
- Pearson term ``(y - mean) ** 2 / var``: Poisson ``mean = rate``, ``var = mean + mean ** 2 expm1(s2)`` (the clamp of
  ``trunc_exp`` enters ``var`` only through ``mean``); Gaussian ``mean = m``, ``var = noise[n] + s2``.
- a Poisson entry with ``y`` negative, not an integer, not finite or ``> max_count`` is skipped: it adds 1 to ``skipped``
  and nothing else, and its ``lo, hi`` are NaN.
- per slot the device sums ``W = n_bins + n_levels + 3`` columns, ``pit_0 ... | covered_0 ... | pearson | entries |
  skipped``; ``calibration_from_sums`` turns them into frequencies.

Held-out scores under the joint posterior (``posterior="joint"`` in ``leave_entries_out``, ``leave_group_out`` and
``calibration``; ``joint_posterior(held_out=, cov=)``; ``vlgp_joint_posterior``, ``vlgp_predictive_cov``,
``vlgp_calibration_cov``).  The joint Laplace posterior above, computed with the fold's entries held out -- a held-out
entry ``(t, n)`` has no term in ``ll``, ``res = cur = 0``, and what ``y`` holds there is never read -- and reported with
the covariance of the latents of every bin, ``cov[t, l, l'] = G_l[t, :] (H^-1)_{l l'} G_l'[t, :]'``, whose diagonal is
``v``.  A held-out entry is then scored with the predictive density and distribution function above at
``m = a_n . mu_t + (b x)_tn`` and ``s2 = max(0, a_n' cov[t] a_n)``: the coupling between latents counts, where the
mean-field ``s2 = (a_n^2) . v_t`` drops it.  One fold at a time: a masked replica of the test set, the E-step, the Newton
iteration (from ``beta = 0``: the mode does not depend on the start), the score, free.

Residual correlations (``residual_correlation``, ``Engine.pair_moments``, ``vlgp_pair_moments``,
``vlgp_pair_moments_cov``).  Every score above is a statement about one (bin, channel) marginal; this
one asks whether PAIRS of channels co-fluctuate more than the model says once the latents are accounted for -- the usual
sign of too few latents.  For row ``t`` with the posterior ``N(mu_t, C_t)`` of its latents -- ``C_t = diag(v_t)`` (0 under
MAP) for the mean-field posterior, the full ``cov[t]`` for the joint one -- and ``c[n, m] = a_n' C_t a_m``:

- predictive mean ``e_n``: the ``rate`` above, ``trunc_exp(m_n + max(0, c[n, n]) / 2)`` Poisson and ``m_n`` Gaussian; scale
  ``s_n``: ``e_n`` Poisson, 1 Gaussian; residual ``d_n = y[t, n] - e_n``.
- predictive covariance ``K[n, m] = s_n s_m f(c[n, m])`` with ``f = expm1`` when both channels are Poisson (the
  covariance of two lognormal rates) and the identity otherwise; on the diagonal the observation variance is added,
  ``K[n, n] += e_n`` Poisson and ``noise[n]`` Gaussian.  ``K[n, n]`` is the variance of the Pearson term above.
- ``resid[n, m] = sum_t live_tn live_tm d_n d_m`` and ``model[n, m] = sum_t live_tn live_tm K[n, m]``; ``count[n, m]`` is
  the number of rows in the sums.  Every entry of a plain set is live; under ``how="channels"`` the entries of the fold,
  scored under the posterior inferred without it.  A row of a trial whose joint posterior failed (non-finite ``mu`` or
  ``cov``) is dead for every channel.
- ``residual_corr = resid / sqrt(model_nn model_mm)``, ``model_corr = model / sqrt(model_nn model_mm)`` and
  ``excess_corr``, their difference: 0 in expectation under the model, whatever the posterior's width.  ``se_null =
  1 / sqrt(count)`` is a rough scale for it only: the rows of a trial are not independent.
  ``dispersion[n] = resid_nn / model_nn`` is the ratio of the summed squared residual to the summed predictive variance
  (``calibration``'s ``dispersion`` is the mean of the per-entry ratios: the two agree where the variance is constant).

Residual autocorrelation (``residual_autocorrelation``, ``Engine.lag_moments``, ``vlgp_lag_moments``).  The same question
along time: does a channel's residual at row ``t`` still predict the one at row ``t + k`` of the same trial?  The posterior
of latent ``l`` has the covariance ``S_l = G_l (I + G_l' W_l G_l)^-1 G_l'``; ``v`` is its diagonal, ``c_l(t, s)`` its entry
``(t, s)``, with ``w`` recomputed from ``mu, v`` over the entries the posterior saw (every entry of a plain set, the ones a
replica does not hold out).  With ``q_n(t, s) = sum_l a_ln^2 c_l(t, s)`` and ``e, s, d`` as above:

- ``resid[k, n] = sum d_tn d_{t+k,n}``, ``model[k, n] = sum s_tn s_{t+k,n} f(q_n(t, t + k))`` (``f = expm1`` Poisson, the
  identity Gaussian; at ``k = 0`` plus ``e_tn`` or ``noise[n]``), ``count[k, n]`` the pairs summed: the ``t`` with ``t + k``
  in the same trial and both entries live.  Under MAP ``c = 0``.
- ``residual_acf = resid / count / var`` with ``var[n] = model[0, n] / count[0, n]``, ``model_acf`` the same of ``model``,
  ``excess_acf`` their difference, ``se_null = 1 / sqrt(count)``, ``dispersion = resid[0] / model[0]``; NaN where
  ``count`` is 0 (a lag longer than every trial) or ``var`` is not positive.

Every sum is a fixed-order device reduction (``vlgp_loglik``, ``vlgp_elbo``, ``vlgp_forecast``, ``vlgp_marginal``,
``vlgp_predictive``, ``vlgp_calibration``, ``vlgp_joint_laplace``, ``vlgp_joint_posterior``, ``vlgp_pair_moments`` and the
``_cov`` scores): the results are the same bits on every run.
"""
import contextlib
import math

import numpy as np

from . import engine as E
from ._lib import ERR_STATE, VlgpError
from .api import _extended, bind_priors
from .engine import hermite_nodes
from .util import _per_trial_entries

__all__ = ["loglik", "leave_one_out", "leave_group_out", "channel_folds", "co_bits_per_spike", "plan_chunks",
           "bits_per_spike", "REPLICA_BUDGET_BYTES", "elbo", "elbo_from_terms", "forward_prediction", "entry_folds",
           "entry_scores", "leave_entries_out", "impute", "marginal_loglik", "weights_summary", "hermite_nodes",
           "joint_posterior", "calibration", "calibration_from_sums", "residual_correlation",
           "residual_autocorrelation"]

SAMPLE_CHUNK = 64  # draws per device call: one lane per sample (csrc/marginal.hip)

SET_TEST, SET_FORWARD, SET_REPLICAS = 0, 1, 2
_PREDICTIVE_KEY = ({}, {"density": "predictive"})  # what a result dict gains when it was scored with predictive=True

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


def default_max_replicas(rows, n_latents, budget=REPLICA_BUDGET_BYTES, mask_channels=0, gauss=False, extra_bytes=0):
    """Replicas of a ``rows``-row test set that fit ``budget`` bytes (at least one).  ``mask_channels``: the channel count
    of a replica with per-entry masks (``Engine.replicate(held_out=...)``), which adds one 64-bit word per row and 64
    channels and, with a Gaussian channel (``gauss``), the per-row constant of ``w``: one double per (row, latent).
    ``extra_bytes``: what the score of a replica takes beside it (``lag_moments``' workspace)."""
    rows, n_latents = max(int(rows), 1), max(int(n_latents), 1)
    per = _DOUBLES_PER_ROW_LATENT * 8 * rows * n_latents + int(extra_bytes)
    if mask_channels:
        per += 8 * rows * ((int(mask_channels) + 63) // 64) + (8 * rows * n_latents if gauss else 0)
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


@contextlib.contextmanager
def _resident(trials, params, units, device, priors=True):
    """An engine that holds ``params`` and ``units`` (the trials' y, x and a posterior) as set ``SET_TEST`` and, with
    ``priors``, a prior factor for every trial length (``bind_priors``); closed on exit."""
    with E.Engine.for_params(params, device) as eng:
        eng.set_params(params["a"], params["b"], params["noise"])
        eng.upload(SET_TEST, units)
        if priors:
            bind_priors(eng, trials, dict(params))  # (a copy: the caller's params["cholesky"] stays as it is)
        yield eng


def _zero_start(trials, L):
    """The units of a held-out inference: the trials' y and x with ``mu = v = w = 0``."""
    return [{"y": tr["y"], "x": tr.get("x"), **{k: np.zeros((tr["y"].shape[0], L)) for k in ("mu", "v", "w")}}
            for tr in trials]


def _score(eng, set_id, vb, density, want_rate=True, mu=None, cov=None):
    """``(sums, rate)`` of a resident set under ``density``: None for the plug-in density (``vlgp_loglik``), else the
    number of quadrature nodes of the posterior-predictive density (``vlgp_predictive``; with ``mu, cov`` under that
    posterior of the latents, ``vlgp_predictive_cov``)."""
    if density is None:
        return eng.loglik(set_id, vb=vb, want_rate=want_rate)
    return eng.predictive(set_id, n_nodes=density, vb=vb, want_rate=want_rate, mu=mu, cov=cov)[:2]


def _density(predictive, n_nodes):
    """The ``density`` of ``_score`` from the public pair of arguments (``n_nodes`` is checked even when a MAP fit would
    never reach the quadrature)."""
    if not predictive:
        return None
    E.hermite_nodes(n_nodes)
    return int(n_nodes)


def _log_scorer(density=None):
    """The scorer of the log scores, as the chunk loops take it: ``scorer(eng, set_id, vb) -> (sums, rate)`` by ``_score``
    under ``density`` (``mu=, cov=``: under that posterior, ``_joint_fold``); ``width`` columns of sums per slot;
    ``predictive``: which ``_PREDICTIVE_KEY`` its results carry."""
    def scorer(eng, set_id, vb, mu=None, cov=None):
        return _score(eng, set_id, vb, density, mu=mu, cov=cov)
    scorer.width, scorer.predictive = 4, density is not None
    return scorer


def _calibration_scorer(n_bins, levels, n_nodes, max_count):
    """The scorer of ``calibration``: ``Engine.calibration``'s sums, ``width = n_bins + len(levels) + 3`` columns per slot,
    and no per-entry output (None where the log scorer returns the rates).  The arguments are checked here."""
    n_bins, levels, max_count = E.check_calibration_args(n_bins, levels, max_count)
    E.hermite_nodes(n_nodes)

    def scorer(eng, set_id, vb, mu=None, cov=None):
        sums, _ = eng.calibration(set_id, n_bins=n_bins, levels=levels, n_nodes=int(n_nodes), vb=vb, max_count=max_count,
                                  mu=mu, cov=cov)
        return sums, None
    scorer.width, scorer.predictive = n_bins + len(levels) + 3, True
    return scorer


def _replica_chunk(eng, n_iter, dmu_bound, vb, posterior=False, scorer=None, **which):
    """One chunk of replicas of ``SET_TEST`` (``which``: ``Engine.replicate``'s ``groups=`` or ``held_out=``): made,
    inferred, scored (``scorer``, default ``_log_scorer()``) and freed.  Returns ``(sums, rate, n_failed, posterior)``, the
    posterior (``mu, v, w`` of the replicas' rows) only on request."""
    eng.replicate(SET_TEST, SET_REPLICAS, **which)
    n_failed = eng.estep(SET_REPLICAS, n_iter, dmu_bound, vb)
    sums, rate = (scorer or _log_scorer())(eng, SET_REPLICAS, vb)
    post = eng.download(SET_REPLICAS, ("mu", "v", "w")) if posterior else None
    eng.free_units(SET_REPLICAS)
    return sums, rate, n_failed, post


POSTERIORS = ("mean_field", "joint")


def _check_posterior(posterior, predictive=True):
    """``posterior`` of the held-out scores: ``"mean_field"``, the E-step's ``mu, v``, or ``"joint"``, the joint Laplace
    posterior with its covariance, which only a predictive density can use."""
    if posterior not in POSTERIORS:
        raise ValueError("posterior must be 'mean_field' or 'joint', got %r" % (posterior,))
    if posterior == "joint" and not predictive:
        raise ValueError("posterior='joint' needs predictive=True: the plug-in density has no use for a covariance")
    return posterior == "joint"


def _joint_fold(eng, held, n_iter, dmu_bound, vb, scorer, max_iter=50, tol=1e-10):
    """One fold under the joint posterior: ``SET_TEST`` replicated once with the entries ``held`` (bool (rows, N)) held
    out, the E-step as ``_replica_chunk`` runs it, the joint Laplace posterior of the replica from there
    (``Engine.joint_posterior``: the held-out entries reach neither), the fold scored under its ``mu, cov``, the replica
    freed.  Returns ``(sums (N, scorer.width), rate (rows, N) or None, n_failed, converged, n_newton)``, the last two per
    trial; ``n_failed`` counts failed E-step updates and failed trials."""
    eng.replicate(SET_TEST, SET_REPLICAS, held_out=held[None])
    n_failed = eng.estep(SET_REPLICAS, n_iter, dmu_bound, vb)
    joint = eng.joint_posterior(SET_REPLICAS, max_iter=max_iter, tol=tol)
    sums, rate = scorer(eng, SET_REPLICAS, vb, mu=joint["mu"], cov=joint["cov"])
    eng.free_units(SET_REPLICAS)
    return sums[0], rate, int(n_failed) + int(joint["n_failed"]), joint["converged"], joint["n_newton"]


def _joint_folds(trials, params, config, masks, n_iter, device, scorer):
    """``_joint_fold`` for every mask of ``masks`` (bool (rows, N) each, pairwise disjoint) in order, from a zero start:
    ``(sums (n_folds, N, scorer.width), rate (rows, N), n_failed, extra, gauss)`` -- ``rate`` holds every entry's rate
    from the fold that holds it out, NaN elsewhere; ``extra`` is ``converged`` and ``n_newton``, (n_folds, trials)."""
    L, N = int(params["zdim"]), int(params["ydim"])
    n_iter = int(config["max_iter"] if n_iter is None else n_iter)
    vb = config["method"] == "VB"
    rows = int(sum(int(tr["y"].shape[0]) for tr in trials))
    sums, conv, newton = [], [], []
    rate = np.full((rows, N), np.nan)
    n_failed = 0
    with _resident(trials, params, _zero_start(trials, L), device) as eng:
        for held in masks:
            s, r, bad, c, n = _joint_fold(eng, held, n_iter, config["dmu_bound"], vb, scorer)
            sums.append(s)
            conv.append(c)
            newton.append(n)
            n_failed += bad
            if r is not None:
                rate[held] = r[held]
        gauss = eng.gauss.copy()
    return np.stack(sums), rate, int(n_failed), {"converged": np.stack(conv), "n_newton": np.stack(newton)}, gauss


def _group_masks(groups, rows, N):
    """A channel fold as a mask of entries: constant along the rows."""
    for g in groups:
        held = np.zeros((rows, N), dtype=bool)
        held[:, g] = True
        yield held


def _per_trial(arr, lengths):
    """A (rows, ...) array cut into one copy per trial."""
    bounds = np.cumsum([0] + list(lengths))
    return [arr[bounds[i]:bounds[i + 1]].copy() for i in range(len(lengths))]


def _no_missing(trials, what):
    """A fit with missing observations (``fit(..., missing=)``) leaves the mask in every trial: a score over every (row,
    channel) would count whatever ``y`` holds at the missing entries."""
    if any(tr.get("missing") is not None for tr in trials):
        raise ValueError("%s: the trials carry 'missing' (a fit with missing observations); scoring every entry would "
                         "count the values stored at the missing ones" % what)


def loglik(fit, per_channel=False, device=0, predictive=False, n_nodes=12):
    """Log-likelihood of a fit's own trials under their own posterior (``mu``, ``v``): a float, or the per-channel
    sums with ``per_channel=True``.

    Replaces the reference's ``vlgp.evaluation.loglik`` (same call: the ``fit`` result dict in, a float out), which
    exponentiates the rate twice and expects shapes ``fit`` does not produce.  Here the rate is the E-step's own plug-in
    rate (module docstring), the Poisson term includes ``-lgamma(y + 1)``, Gaussian channels are scored with their
    noise variance, and the sum runs over every (row, channel) of every trial.  ``predictive=True`` scores every entry
    with the posterior-predictive density instead (module docstring), ``n_nodes`` quadrature nodes per Poisson entry."""
    trials, params, config = fit["trials"], fit["params"], fit.get("config") or {}
    _no_missing(trials, "loglik")
    density = _density(predictive, n_nodes)
    vb = config.get("method", "VB") == "VB"
    L = params["zdim"]
    units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"], "v": tr.get("v", np.zeros((tr["y"].shape[0], L))),
              "w": None} for tr in trials]
    with _resident(trials, params, units, device, priors=False) as eng:
        sums, _ = _score(eng, SET_TEST, vb, density, want_rate=False)
    per = sums[:, 0].copy()
    return per if per_channel else float(np.sum(per))


def elbo_from_terms(row_sums, kl_terms, ranks, vb=True, n_failed=0, mu_sq=None, row_ell=None, offsets=None):
    """Assemble ``vlgp_elbo``'s two device arrays into the result dict (pure host code).

    ``row_sums`` (N, 4): column 0 is the expected log-likelihood per channel.  ``kl_terms`` (units, L, 4):
    ``log det H, tr S, beta'beta, |mu - G beta|^2`` per (unit, latent); NaN where the factorisation failed.  ``ranks``
    (units, L): the effective rank ``r`` of each pair's prior factor.  ``mu_sq`` (units, L): ``|mu|^2``, for
    ``off_prior`` (NaN without it).  ``row_ell`` (rows) with ``offsets`` (units + 1): per-row expected log-likelihood
    and the units' row ranges, for ``elbo_per_trial``.

    Returns ``elbo``, ``ell``, ``kl`` (units, L), ``ell_per_channel``, ``off_prior`` (units, L), ``n_failed``; under MAP
    (``vb`` false) ``elbo`` and ``kl`` are NaN and ``log_joint = ell - 1/2 sum beta'beta`` is added; with ``row_ell``
    also ``elbo_per_trial`` (``log_joint_per_trial`` under MAP).  A failed pair's NaN reaches every total it enters."""
    row_sums = np.asarray(row_sums, dtype=float)
    terms = np.asarray(kl_terms, dtype=float)
    ranks = np.asarray(ranks, dtype=float)
    if terms.ndim != 3 or terms.shape[2] != 4 or ranks.shape != terms.shape[:2]:
        raise ValueError("kl_terms must be (units, L, 4) with ranks (units, L)")
    logdet, tr_s, bb, resid = (terms[:, :, k] for k in range(4))
    ell_ch = row_sums[:, 0].copy()
    ell = float(np.sum(ell_ch))
    if vb:
        kl = 0.5 * (tr_s + bb - ranks + logdet)
    else:
        kl = np.full(ranks.shape, np.nan)
    if mu_sq is None:
        off = np.full(ranks.shape, np.nan)
    else:
        off = resid / np.maximum(np.asarray(mu_sq, dtype=float), np.finfo(float).tiny)
    out = {"elbo": ell - float(np.sum(kl)), "ell": ell, "kl": kl, "ell_per_channel": ell_ch, "off_prior": off,
           "n_failed": int(n_failed)}
    if not vb:
        out["log_joint"] = ell - 0.5 * float(np.sum(bb))
    if row_ell is not None:
        offsets = np.asarray(offsets, dtype=np.int64)
        if offsets.shape != (terms.shape[0] + 1,):
            raise ValueError("offsets must hold units + 1 row bounds")
        ell_unit = np.array([np.sum(row_ell[offsets[i]:offsets[i + 1]]) for i in range(terms.shape[0])])
        if vb:
            out["elbo_per_trial"] = ell_unit - np.sum(kl, axis=1)
        else:
            out["log_joint_per_trial"] = ell_unit - 0.5 * np.sum(bb, axis=1)
    return out


def elbo(fit, per_trial=False, device=0):
    """Variational lower bound of a fit's own trials under their own posterior ``mu, v, w``, the fit's parameters and
    ``params["cholesky"]`` (module docstring for the definitions); lengths without a factor there are built from
    ``omega, sigma`` as ``transform`` does.  Same calling shape as ``loglik``.

    Returns a dict: ``elbo``, ``ell``, ``kl`` (trials, L), ``ell_per_channel``, ``off_prior`` (trials, L), ``n_failed``
    (pairs whose ``H`` or ``G'G`` was not positive definite: their terms, and the totals, are NaN); under MAP ``elbo``
    and ``kl`` are NaN and ``log_joint`` holds the penalised log joint.  ``per_trial=True`` adds ``elbo_per_trial``:
    the device leaves the expected log-likelihood of every row (channels summed in order) in the same launch and the
    rows of a trial are added on the host -- no second reduction kernel, no call per trial."""
    trials, params, config = fit["trials"], fit["params"], fit.get("config") or {}
    _no_missing(trials, "elbo")
    vb = config.get("method", "VB") == "VB"
    L = params["zdim"]

    def zeros(tr):
        return np.zeros((tr["y"].shape[0], L))

    units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"],
              "v": tr["v"] if tr.get("v") is not None else zeros(tr),
              "w": tr["w"] if tr.get("w") is not None else zeros(tr)} for tr in trials]
    with _resident(trials, params, units, device) as eng:
        sums, terms, bad, row_ell = eng.elbo(SET_TEST, vb=vb, want_rows=per_trial)
        ranks = eng.unit_ranks(SET_TEST)
        offsets = eng.sets[SET_TEST][2]
    mu_sq = np.array([np.sum(np.asarray(tr["mu"], dtype=float) ** 2, axis=0) for tr in trials])
    return elbo_from_terms(sums, terms, ranks, vb=vb, n_failed=bad, mu_sq=mu_sq, row_ell=row_ell,
                           offsets=offsets if per_trial else None)


def _is_refusal(err):
    return err.status == ERR_STATE and "replicated set" in err.detail


def _leave_out_sums(trials, params, config, groups, n_iter, path, max_replicas, device, scorer):
    """For every group of validated ``groups`` one inference without it from a zero start, then its channels scored by
    ``scorer`` with their original loadings: ``(sums (channels, scorer.width), rate (rows, channels), n_failed, path,
    gauss)``, the channels those of the groups concatenated; ``rate`` is left unwritten by a scorer without per-entry
    output."""
    L = int(params["zdim"])
    channels = [c for g in groups for c in g]
    n_iter = int(config["max_iter"] if n_iter is None else n_iter)
    vb = config["method"] == "VB"
    dmu_bound = config["dmu_bound"]
    a = np.array(params["a"], dtype=float)
    b = np.array(params["b"], dtype=float)
    noise = np.array(params["noise"], dtype=float)
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    rows = int(sum(lengths))
    units = _zero_start(trials, L)
    rate = np.empty((rows, len(channels)))
    sums = np.empty((len(channels), scorer.width))
    n_failed = 0
    used = "batched" if path != "sequential" else "sequential"
    with _resident(trials, params, units, device) as eng:
        if used == "batched":
            cap = default_max_replicas(rows, L) if max_replicas is None else int(max_replicas)
            done = 0
            try:
                for chunk in plan_chunks(groups, cap):
                    n = sum(len(g) for g in chunk)
                    sums[done:done + n], r, bad, _ = _replica_chunk(eng, n_iter, dmu_bound, vb, scorer=scorer, groups=chunk)
                    if r is not None:
                        rate[:, done:done + n] = r
                    n_failed += bad
                    done += n
            except VlgpError as err:
                if path == "batched" or not _is_refusal(err):
                    raise
                if SET_REPLICAS in eng.sets:
                    eng.free_units(SET_REPLICAS)
                used, n_failed = "sequential", 0
        if used == "sequential":
            done = 0
            for g in groups:
                a_out = a.copy()
                a_out[:, g] = 0.0
                eng.set_params(a_out, b, noise)
                eng.upload(SET_TEST, units)  # (mu = v = w = 0 again)
                n_failed += eng.estep(SET_TEST, n_iter, dmu_bound, vb)
                eng.set_params(a, b, noise)
                s, r = scorer(eng, SET_TEST, vb)
                sums[done:done + len(g)] = s[g]
                if r is not None:
                    rate[:, done:done + len(g)] = r[:, g]
                done += len(g)
    return sums, rate, int(n_failed), used, eng.gauss[channels]


def _leave_out_sums_joint(trials, params, config, groups, n_iter, device, scorer):
    """``_leave_out_sums`` under the joint posterior, one group at a time (``_joint_folds``): its first three values, the
    path ``"joint"``, ``gauss`` of the channels, and ``converged``, ``n_newton`` per (group, trial)."""
    channels = [c for g in groups for c in g]
    rows, N = int(sum(int(tr["y"].shape[0]) for tr in trials)), int(params["ydim"])
    got, rate, n_failed, extra, gauss = _joint_folds(trials, params, config, _group_masks(groups, rows, N), n_iter, device,
                                                     scorer)
    sums = np.concatenate([got[k][g] for k, g in enumerate(groups)], axis=0)
    return sums, rate[:, channels], n_failed, "joint", gauss[channels], extra


def _leave_out(trials, params, config, groups, n_iter, path, max_replicas, device, scorer, joint=False):
    """What ``leave_one_out`` and ``leave_group_out`` share, for validated ``groups`` and a log scorer
    (``_leave_out_sums``; ``joint``: ``_leave_out_sums_joint``).  Returns ``channels`` (the groups concatenated), ``rate``
    per trial, ``ll``, ``ll_null``, ``n_spikes``, ``bits_per_spike``, ``n_failed``, ``path``."""
    extra = {}
    if joint:
        sums, rate, n_failed, used, gauss, extra = _leave_out_sums_joint(trials, params, config, groups, n_iter, device, scorer)
    else:
        sums, rate, n_failed, used, gauss = _leave_out_sums(trials, params, config, groups, n_iter, path, max_replicas,
                                                            device, scorer)
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    ll, ll_null, ny, bps = bits_per_spike(sums, int(sum(lengths)), gauss)
    return {
        "channels": [c for g in groups for c in g],
        "rate": _per_trial(rate, lengths),
        "ll": ll, "ll_null": ll_null, "n_spikes": ny, "bits_per_spike": bps,
        "n_failed": n_failed, "path": used, **_PREDICTIVE_KEY[scorer.predictive], **extra,
    }


def leave_one_out(trials, params, config, channels=None, n_iter=None, path="auto", max_replicas=None, device=0,
                  predictive=False, n_nodes=12):
    """Leave-one-neuron-out prediction of held-out trials (module docstring for the definitions).

    ``trials``: dicts with ``y`` (T, N) and, with regressors, ``x`` (T, xdim, N); their ``mu``, ``v``, ``w`` are not
    read or written.  ``channels``: the channels to leave out in turn (default all).  ``n_iter``: E-step iterations
    (default ``config["max_iter"]``, as ``core.infer``).  ``path``: ``"batched"`` runs every left-out channel as a replica
    of the test set in one E-step (``Engine.replicate``), ``max_replicas`` at a time (default: what
    ``REPLICA_BUDGET_BYTES`` holds); ``"sequential"`` runs one E-step per channel with its loading zeroed; ``"auto"``
    takes the batched path unless the device refuses it (the split E-step cannot run the configuration, e.g. L > 10).
    Both paths give the same bits when they run the same E-step kernels.

    Returns a dict: ``channels``; ``rate``, a list per trial of (T, len(channels)) plug-in rates (Gaussian: means);
    per channel ``ll``, ``ll_null``, ``n_spikes``, ``bits_per_spike``; ``n_failed`` (singular posterior updates);
    ``path`` (``"batched"`` or ``"sequential"``).  ``predictive=True``: ``ll`` and everything derived from it score the
    posterior-predictive density (module docstring; ``n_nodes`` quadrature nodes per Poisson entry) in place of the plug-in
    one -- ``rate`` and the null model stay -- and the dict carries ``"density": "predictive"``."""
    if path not in ("auto", "batched", "sequential"):
        raise ValueError("path must be 'auto', 'batched' or 'sequential'")
    N = int(params["ydim"])
    channels = list(range(N)) if channels is None else [int(c) for c in channels]
    if not channels or len(set(channels)) != len(channels) or min(channels) < 0 or max(channels) >= N:
        raise ValueError("channels must be distinct indices in [0, %d)" % N)
    return _leave_out(trials, params, config, [[c] for c in channels], n_iter, path, max_replicas, device,
                      _log_scorer(_density(predictive, n_nodes)))


def channel_folds(n_channels, n_folds, seed=0):
    """``n_folds`` sorted index lists that partition ``range(n_channels)``, sizes differing by at most one: the
    channels in the order of ``np.random.default_rng(seed).permutation(n_channels)``, dealt round-robin.  A
    deterministic function of its arguments."""
    n_channels, n_folds = int(n_channels), int(n_folds)
    if not 1 <= n_folds <= n_channels:
        raise ValueError("need 1 <= n_folds <= n_channels, got %d folds for %d channels" % (n_folds, n_channels))
    perm = np.random.default_rng(seed).permutation(n_channels)
    return [sorted(int(c) for c in perm[f::n_folds]) for f in range(n_folds)]


def co_bits_per_spike(ll, ll_null, n_spikes):
    """``(sum ll - sum ll_null) / (sum n_spikes * ln 2)`` over the channels with a finite ``ll_null`` (Poisson) and at
    least one spike; NaN when there is none."""
    ll, ll_null, ny = (np.asarray(x, dtype=float) for x in (ll, ll_null, n_spikes))
    use = np.isfinite(ll_null) & (ny > 0)
    if not use.any():
        return float("nan")
    return float((np.sum(ll[use]) - np.sum(ll_null[use])) / (np.sum(ny[use]) * math.log(2.0)))


def _check_groups(groups, N):
    groups = [[int(c) for c in g] for g in groups]
    flat = [c for g in groups for c in g]
    if not groups or any(not g for g in groups):
        raise ValueError("every group needs at least one channel")
    if min(flat) < 0 or max(flat) >= N:
        raise ValueError("group channels must lie in [0, %d)" % N)
    if len(set(flat)) != len(flat):
        raise ValueError("groups must be pairwise disjoint sets of distinct channels")
    if any(len(g) == N for g in groups):
        raise ValueError("a group may not hold every channel: nothing would be left to infer the latents from")
    return groups


def leave_group_out(trials, params, config, groups=None, n_folds=5, seed=0, n_iter=None, path="auto",
                    max_replicas=None, device=0, predictive=False, n_nodes=12, posterior="mean_field"):
    """Leave-group-out (co-smoothing) prediction of held-out trials (module docstring for the definitions).

    As ``leave_one_out``, with a set of channels where it has one.  ``groups``: a list of channel lists, non-empty,
    pairwise disjoint, none holding every channel (default ``channel_folds(N, min(n_folds, N), seed)``).  For every
    group the latents are inferred from a zero start, ``n_iter`` E-step iterations, with the group's loadings zeroed, and
    every channel of the group is predicted from them with its original loading.  ``path``: ``"batched"`` runs one
    replica of the test set per group in one E-step (``vlgp_replicate_groups``), ``max_replicas`` whole groups at a
    time; ``"sequential"`` one E-step per group; ``"auto"`` the batched path unless the device refuses it.

    Returns a dict: ``groups``; ``channels``, the groups concatenated in order; ``group_of``, the group index of each of
    those channels; ``rate``, a list per trial of (T, len(channels)); per channel ``ll``, ``ll_null``, ``n_spikes``,
    ``bits_per_spike``; ``co_bps``; ``n_failed``; ``path``.  ``predictive``, ``n_nodes``: as ``leave_one_out``.

    ``posterior="joint"`` (needs ``predictive=True``, else ``ValueError``) scores every group under the joint Laplace
    posterior of the trials inferred without it -- mean and full covariance of the latents per bin (module docstring) --
    one group at a time in order, the group held out as a mask of entries that is constant along the rows (``path`` and
    ``max_replicas`` are then not read; ``path`` is reported as ``"joint"``).  The dict gains ``converged`` and
    ``n_newton``, (groups, trials), and ``n_failed`` also counts trials whose ``H`` could not be factored."""
    if path not in ("auto", "batched", "sequential"):
        raise ValueError("path must be 'auto', 'batched' or 'sequential'")
    joint = _check_posterior(posterior, predictive)
    N = int(params["ydim"])
    groups = _check_groups(channel_folds(N, min(int(n_folds), N), seed) if groups is None else groups, N)
    out = _leave_out(trials, params, config, groups, n_iter, path, max_replicas, device,
                     _log_scorer(_density(predictive, n_nodes)), joint=joint)
    out.update(groups=groups, group_of=[k for k, g in enumerate(groups) for _ in g],
               co_bps=co_bits_per_spike(out["ll"], out["ll_null"], out["n_spikes"]))
    return out


def entry_folds(rows, n_channels, n_folds, seed=0):
    """A (rows, n_channels) integer array of fold indices, every entry in exactly one fold and fold sizes differing by
    at most one: ``np.random.default_rng(seed).permutation(rows * n_channels).reshape(rows, n_channels) % n_folds``.  A
    deterministic function of its arguments."""
    rows, n_channels, n_folds = int(rows), int(n_channels), int(n_folds)
    if rows < 1 or n_channels < 1 or not 1 <= n_folds <= rows * n_channels:
        raise ValueError("need rows, n_channels >= 1 and 1 <= n_folds <= rows * n_channels, got %d folds for %d x %d entries"
                         % (n_folds, rows, n_channels))
    return np.random.default_rng(seed).permutation(rows * n_channels).reshape(rows, n_channels) % n_folds


def entry_scores(sums, n_entries, gauss=None):
    """Scores of a speckled hold-out from the masked ``vlgp_loglik`` sums (pure host code).  ``sums`` (n_folds, N, 4):
    per (fold, channel) ``sum ll, sum y, sum rate, sum lgamma(y + 1)`` over the entries that fold holds out;
    ``n_entries`` (N): held-out entries per channel, all folds.  Returns a dict: per channel ``ll``, ``ll_null`` (a
    constant rate at the channel's mean count over its held-out entries), ``n_spikes``, ``n_entries``,
    ``bits_per_spike`` (NaN for Gaussian channels and channels without a held-out spike); ``ll_per_fold`` (n_folds, N);
    ``speckled_bps``, pooled by ``co_bits_per_spike``'s rule.  The folds are added in fold order."""
    sums = np.asarray(sums, dtype=float)
    if sums.ndim != 3 or sums.shape[2] != 4:
        raise ValueError("sums must be (n_folds, N, 4)")
    n_entries = np.asarray(n_entries, dtype=float)
    if n_entries.shape != (sums.shape[1],):
        raise ValueError("n_entries must hold one count per channel")
    gauss = np.zeros(sums.shape[1], dtype=bool) if gauss is None else np.asarray(gauss, dtype=bool)
    tot = np.zeros(sums.shape[1:])
    for k in range(sums.shape[0]):
        tot += sums[k]
    ll, ny, lg = tot[:, 0], tot[:, 1], tot[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        ybar = np.where(n_entries > 0, ny / np.where(n_entries > 0, n_entries, 1.0), 0.0)
        ll_null = np.where(ny > 0, ny * np.log(np.where(ny > 0, ybar, 1.0)), 0.0) - n_entries * ybar - lg
        bps = (ll - ll_null) / (ny * math.log(2.0))
    bps = np.where(gauss | ~(ny > 0), np.nan, bps)
    ll_null = np.where(gauss, np.nan, ll_null)
    return {"ll": ll, "ll_null": ll_null, "n_spikes": ny, "n_entries": n_entries.astype(np.int64),
            "bits_per_spike": bps, "ll_per_fold": sums[:, :, 0].copy(),
            "speckled_bps": co_bits_per_spike(ll, ll_null, ny)}


def _entries_out(trials, params, config, held_out, n_iter, max_replicas, device, posterior=False, scorer=None):
    """One replica per mask of ``held_out`` (bool (n_rep, rows, N)) from a zero start, ``max_replicas`` at a time, scored by
    ``scorer`` (default ``_log_scorer()``; without per-entry output ``rate`` stays NaN):
    ``(sums (n_rep, N, scorer.width), rate (rows, N), n_failed, posterior, gauss)``, the posterior (mu, v, w of every
    replica, (n_rep, rows, L) each) only on request.  The masks of one call are pairwise disjoint, so the rate of every
    entry has one source."""
    L = int(params["zdim"])
    n_iter = int(config["max_iter"] if n_iter is None else n_iter)
    vb = config["method"] == "VB"
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    rows, N = int(sum(lengths)), int(params["ydim"])
    units = _zero_start(trials, L)
    n_rep = held_out.shape[0]
    scorer = scorer or _log_scorer()
    sums = np.empty((n_rep, N, scorer.width))
    rate = np.full((rows, N), np.nan)
    post = {k: np.empty((n_rep, rows, L)) for k in ("mu", "v", "w")} if posterior else None
    n_failed = 0
    with _resident(trials, params, units, device) as eng:
        cap = max_replicas
        if cap is None:
            cap = default_max_replicas(rows, L, mask_channels=N, gauss=bool(eng.gauss.any()))
        cap = max(int(cap), 1)
        for k0 in range(0, n_rep, cap):
            chunk = held_out[k0:k0 + cap]
            s, r, bad, got = _replica_chunk(eng, n_iter, config["dmu_bound"], vb, posterior=posterior, scorer=scorer,
                                            held_out=chunk)
            n_failed += bad
            if posterior:
                for key in post:
                    post[key][k0:k0 + len(chunk)] = got[key].reshape(len(chunk), rows, L)
            sums[k0:k0 + len(chunk)] = s
            if r is not None:
                mine = chunk.any(axis=0)
                rate[mine] = r[mine]
        gauss = eng.gauss.copy()
    return sums, rate, int(n_failed), post, gauss


def _entry_masks(trials, params, folds, n_folds, seed):
    """``(F, held)`` of a speckled hold-out: the fold of every entry over the concatenated rows (``folds`` per trial, -1
    for an entry never held out; default ``entry_folds``) and the bool masks (n_folds, rows, N) of the folds."""
    rows, N = int(sum(int(tr["y"].shape[0]) for tr in trials)), int(params["ydim"])
    if folds is None:
        F = entry_folds(rows, N, n_folds, seed)
        n_folds = int(n_folds)
    else:
        F = np.concatenate(_per_trial_entries(folds, trials, "folds", int), axis=0)
        if F.min() < -1:
            raise ValueError("fold indices are >= 0, or -1 for an entry that is never held out")
        n_folds = int(F.max()) + 1
        if n_folds < 1:
            raise ValueError("folds hold no entry out")
    return F, np.stack([F == k for k in range(n_folds)])


def leave_entries_out(trials, params, config, folds=None, n_folds=5, seed=0, n_iter=None, max_replicas=None, device=0,
                      predictive=False, n_nodes=12, posterior="mean_field"):
    """Speckled hold-out on held-out trials: single (row, channel) entries left out of the inference and predicted
    (module docstring for the definitions).

    ``trials``: as ``leave_group_out``.  ``folds``: a list per trial of (T, N) integer arrays, the fold every entry is
    held out in, ``-1`` for an entry that is never held out; the folds run from 0 to the largest index given
    (``n_folds`` and ``seed`` are then not read).  Default: ``entry_folds`` over the concatenated rows, cut per trial.
    One replica of the test set per fold (``vlgp_replicate_masked``) from a zero start, ``n_iter`` E-step iterations
    (default ``config["max_iter"]``), ``max_replicas`` at a time (default: what ``REPLICA_BUDGET_BYTES`` holds; the
    chunking changes no bit).  There is no sequential path: a configuration the split E-step refuses (e.g. L > 10)
    raises ``VlgpError`` with the device's reason.

    Returns a dict: ``folds``; ``rate``, per trial (T, N), NaN where never held out (Gaussian: means); per channel
    ``ll``, ``ll_null``, ``n_spikes``, ``n_entries``, ``bits_per_spike``; ``ll_per_fold`` (n_folds, N);
    ``speckled_bps``; ``n_failed``.  ``predictive``, ``n_nodes``: as ``leave_one_out``.

    ``posterior="joint"`` (needs ``predictive=True``, else ``ValueError``) scores every fold under the joint Laplace
    posterior of the trials inferred without it, as ``leave_group_out`` does: one fold at a time in fold order
    (``max_replicas`` is then not read), the dict gaining ``converged`` and ``n_newton``, (n_folds, trials)."""
    density = _density(predictive, n_nodes)
    joint = _check_posterior(posterior, predictive)
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    F, held = _entry_masks(trials, params, folds, n_folds, seed)
    extra = {}
    if joint:
        sums, rate, n_failed, extra, gauss = _joint_folds(trials, params, config, held, n_iter, device, _log_scorer(density))
    else:
        sums, rate, n_failed, _, gauss = _entries_out(trials, params, config, held, n_iter, max_replicas, device,
                                                      scorer=_log_scorer(density))
    out = entry_scores(sums, (F >= 0).sum(axis=0), gauss)
    out.update(folds=_per_trial(F, lengths), rate=_per_trial(rate, lengths), n_failed=n_failed,
               **_PREDICTIVE_KEY[density is not None], **extra)
    return out


def impute(trials, params, config, missing, n_iter=None, device=0):
    """Inference on trials with holes: ``missing`` is a list per trial of (T, N) bool arrays, True where the
    observation is absent (an artifact-blanked bin, a channel dead for part of a trial; the value stored in ``y``
    there is not read by the inference).  One E-step from a zero start with those entries' likelihood terms removed
    (module docstring: leave-entries-out with the one fold ``missing``), ``n_iter`` iterations (default
    ``config["max_iter"]``).

    Returns a dict of per-trial lists: ``mu``, ``v``, ``w`` (T, L) and ``rate`` (T, N), the model's prediction at the
    missing entries (Gaussian: means) and NaN elsewhere; and ``n_failed``."""
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    held = np.concatenate(_per_trial_entries(missing, trials, "missing", bool), axis=0)[None]
    _, rate, n_failed, post, _ = _entries_out(trials, params, config, held, n_iter, 1, device, posterior=True)
    return {"mu": _per_trial(post["mu"][0], lengths), "v": _per_trial(post["v"][0], lengths),
            "w": _per_trial(post["w"][0], lengths), "rate": _per_trial(rate, lengths), "n_failed": n_failed}


def calibration_from_sums(sums, n_bins, levels):
    """Calibration summaries from ``vlgp_calibration``'s sums (pure host code).  ``sums`` (..., W) with
    ``W = n_bins + len(levels) + 3`` columns ``pit_0 ... | covered_0 ... | pearson | entries | skipped`` per slot; the
    leading axes are the slots and are kept.

    Returns a dict: ``pit`` (..., n_bins), each slot's histogram divided by its ``entries`` (a calibrated slot is flat at
    ``1 / n_bins``); ``coverage`` (..., len(levels)), the share of entries inside each central interval; ``dispersion``,
    ``pearson / entries`` (1 when the predictive variance is right, above it when the counts are over-dispersed against the
    model); ``entries`` and ``skipped`` per slot (integers); ``levels``; and ``pit_all``, ``coverage_all``,
    ``dispersion_all``, the same from the columns summed over every slot.  A slot without an entry gives NaN."""
    sums = np.asarray(sums, dtype=float)
    levels = np.asarray(levels, dtype=float).reshape(-1)
    J, C = int(n_bins), len(levels)
    if sums.ndim < 1 or sums.shape[-1] != J + C + 3:
        raise ValueError("sums must have n_bins + len(levels) + 3 = %d columns, got shape %r" % (J + C + 3, sums.shape))
    tot = sums.reshape(-1, J + C + 3).sum(axis=0)

    def ratio(x, n):
        n = np.asarray(n, dtype=float)[..., None]
        return np.where(n > 0, x / np.where(n > 0, n, 1.0), np.nan)

    pit, cov, pearson, entries = sums[..., :J], sums[..., J:J + C], sums[..., J + C:J + C + 1], sums[..., J + C + 1]
    return {"pit": ratio(pit, entries), "pit_all": ratio(tot[:J], tot[J + C + 1]),
            "coverage": ratio(cov, entries), "coverage_all": ratio(tot[J:J + C], tot[J + C + 1]), "levels": levels.copy(),
            "dispersion": ratio(pearson, entries)[..., 0],
            "dispersion_all": float(ratio(tot[J + C:J + C + 1], tot[J + C + 1])[0]),
            "entries": np.rint(entries).astype(np.int64), "skipped": np.rint(sums[..., J + C + 2]).astype(np.int64)}


def calibration(trials, params, config, how="in_sample", groups=None, folds=None, n_folds=5, seed=0, n_bins=10,
                levels=(0.5, 0.9), n_nodes=12, max_count=4096, n_iter=None, max_replicas=None, device=0,
                posterior="mean_field"):
    """Calibration of the predictive distribution, per channel (module docstring for the definitions): PIT histogram,
    coverage of the central intervals ``levels`` and Pearson dispersion.

    ``how="in_sample"``: the trials' own posterior ``mu, v``, as ``loglik`` scores it.  ``how="channels"``: co-smoothing --
    ``leave_group_out``'s inference (``groups``, default ``channel_folds(N, min(n_folds, N), seed)``; batched unless the
    device refuses the replicas), every channel scored under the posterior inferred without its group.
    ``how="entries"``: speckled -- ``leave_entries_out``'s inference (``folds``, default ``entry_folds`` with ``n_folds``
    and ``seed``), every entry scored under the posterior of the fold that holds it out.  ``n_iter``, ``max_replicas``: as
    there.  ``n_nodes``: quadrature nodes per Poisson mass; ``max_count``: Poisson entries above it are skipped, not
    scored.  Trials that carry ``missing`` raise ``ValueError``.

    Returns ``calibration_from_sums``' dict with one slot per channel, the replicas or folds added in order, plus
    ``n_failed`` (failed E-step updates; 0 in sample).  A channel no group holds has no entry: NaN.

    ``posterior="joint"``: the same three questions asked of the joint Laplace posterior, mean and full covariance of the
    latents per bin.  In sample it is the posterior of the trials' own data, the Newton iteration started from their stored
    ``mu, w``; for ``"channels"`` and ``"entries"`` the one of ``leave_group_out`` and ``leave_entries_out`` with
    ``posterior="joint"``, one fold at a time.  An entry of a trial whose ``H`` could not be factored is skipped and
    counted in ``skipped``.  The dict gains ``converged`` and ``n_newton``, per (fold, trial) or, in sample, per trial, and
    ``n_failed`` also counts the failed trials."""
    if how not in ("in_sample", "channels", "entries"):
        raise ValueError("how must be 'in_sample', 'channels' or 'entries', got %r" % (how,))
    joint = _check_posterior(posterior)
    _no_missing(trials, "calibration")
    scorer = _calibration_scorer(n_bins, levels, n_nodes, max_count)
    N, L = int(params["ydim"]), int(params["zdim"])
    n_failed, extra = 0, {}
    if joint:
        rows = int(sum(int(tr["y"].shape[0]) for tr in trials))
        if how == "in_sample":
            with _posterior(trials, params, config, False, n_iter, device) as (eng, _):
                post = eng.joint_posterior(SET_TEST)
                sums, _ = scorer(eng, SET_TEST, True, mu=post["mu"], cov=post["cov"])
            n_failed, extra = post["n_failed"], {"converged": post["converged"], "n_newton": post["n_newton"]}
        elif how == "channels":
            groups = _check_groups(channel_folds(N, min(int(n_folds), N), seed) if groups is None else groups, N)
            got, _, n_failed, extra, _ = _joint_folds(trials, params, config, _group_masks(groups, rows, N), n_iter, device,
                                                      scorer)
            sums = np.zeros((N, scorer.width))
            for k, g in enumerate(groups):
                sums[g] = got[k][g]
        else:
            _, held = _entry_masks(trials, params, folds, n_folds, seed)
            got, _, n_failed, extra, _ = _joint_folds(trials, params, config, held, n_iter, device, scorer)
            sums = np.zeros((N, scorer.width))
            for k in range(got.shape[0]):
                sums += got[k]
    elif how == "in_sample":
        units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"], "v": tr.get("v", np.zeros((tr["y"].shape[0], L))),
                  "w": None} for tr in trials]
        with _resident(trials, params, units, device, priors=False) as eng:
            sums, _ = scorer(eng, SET_TEST, config.get("method", "VB") == "VB")
    elif how == "channels":
        groups = _check_groups(channel_folds(N, min(int(n_folds), N), seed) if groups is None else groups, N)
        got, _, n_failed, _, _ = _leave_out_sums(trials, params, config, groups, n_iter, "auto", max_replicas, device,
                                                 scorer)
        sums = np.zeros((N, scorer.width))
        sums[[c for g in groups for c in g]] = got
    else:
        _, held = _entry_masks(trials, params, folds, n_folds, seed)
        got, _, n_failed, _, _ = _entries_out(trials, params, config, held, n_iter, max_replicas, device, scorer=scorer)
        sums = np.zeros((N, scorer.width))
        for k in range(got.shape[0]):
            sums += got[k]
    out = calibration_from_sums(sums, n_bins, levels)
    out["n_failed"] = int(n_failed)
    out.update(extra)
    return out


def _pair_summary(resid, model, count):
    """Residual correlations from the pair moments (pure host code).  ``resid``, ``model`` (N, N): ``Engine.pair_moments``'
    sums; ``count`` (N, N): the rows in each sum, 0 or NaN for a pair that was never scored.

    Returns a dict: ``resid``, ``model``, ``count`` with NaN at the pairs never scored; ``residual_corr``, ``model_corr``,
    ``excess_corr`` and ``se_null`` (N, N) and ``dispersion`` (N) by the module docstring, NaN where the pair or one of its
    two variances was not scored; over the scored pairs ``n > m`` with a finite ``excess_corr``: ``n_pairs``, and
    ``rms_excess``, ``mean_excess`` (NaN without a pair)."""
    resid, model, count = (np.array(x, dtype=float) for x in (resid, model, count))
    if resid.ndim != 2 or resid.shape[0] != resid.shape[1] or model.shape != resid.shape or count.shape != resid.shape:
        raise ValueError("resid, model and count must be (N, N), got %r, %r, %r" % (resid.shape, model.shape, count.shape))
    scored = count > 0  # (False for NaN)
    resid, model, count = (np.where(scored, x, np.nan) for x in (resid, model, count))
    var = np.diagonal(model)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.sqrt(var[:, None] * var[None, :])
        norm = np.where(norm > 0, norm, np.nan)
        residual_corr, model_corr = resid / norm, model / norm
        dispersion = np.diagonal(resid) / np.where(var > 0, var, np.nan)
        se_null = 1.0 / np.sqrt(count)
    excess = residual_corr - model_corr
    low = excess[np.tril_indices(len(var), -1)]
    low = low[np.isfinite(low)]
    return {"resid": resid, "model": model, "count": count, "residual_corr": residual_corr, "model_corr": model_corr,
            "excess_corr": excess, "se_null": se_null, "dispersion": dispersion, "n_pairs": int(low.size),
            "rms_excess": float(np.sqrt(np.mean(low * low))) if low.size else float("nan"),
            "mean_excess": float(np.mean(low)) if low.size else float("nan")}


def _pair_scorer():
    """``Engine.pair_moments`` as ``_joint_fold`` takes a scorer: per replica ``resid | model | count`` stacked, (n_rep, 3, N,
    N) -- ``count`` the rows of the posterior that are not dead -- and no per-entry output."""
    def scorer(eng, set_id, vb, mu=None, cov=None):
        resid, model = eng.pair_moments(set_id, vb=vb, mu=mu, cov=cov)
        resid, model = resid.reshape((-1,) + resid.shape[-2:]), model.reshape((-1,) + model.shape[-2:])
        rows = eng.sets[set_id][1] // resid.shape[0]
        alive = np.full(resid.shape[0], rows)
        if mu is not None:
            ok = np.isfinite(mu).all(axis=1) & np.isfinite(cov.reshape(len(mu), -1)).all(axis=1)
            alive = ok.reshape(resid.shape[0], rows).sum(axis=1)
        count = np.broadcast_to(alive[:, None, None].astype(float), resid.shape)
        return np.stack([resid, model, count], axis=1), None
    scorer.width, scorer.predictive = 3, True
    return scorer


def residual_correlation(trials, params, config, how="in_sample", groups=None, n_folds=5, seed=0, posterior="mean_field",
                         n_iter=None, device=0):
    """Residual correlations between channels: do pairs co-fluctuate beyond what the model's predictive distribution says
    (module docstring for the definitions)?

    ``how="in_sample"``: the trials' own posterior ``mu, v``, every pair of channels over every row.  ``how="channels"``:
    the honest version -- every fold of ``groups`` (default ``channel_folds(N, min(n_folds, N), seed)``) held out as a mask
    that is constant along the rows, the latents inferred without it from a zero start (``n_iter`` E-step iterations,
    default ``config["max_iter"]``), and the pairs WITHIN the fold scored; a pair across two folds is never scored.
    ``posterior="joint"``: the same under the joint Laplace posterior with its full covariance per bin -- in sample the one
    of the trials' own data started from their stored ``mu, w``, for ``"channels"`` one fold at a time as
    ``leave_group_out`` runs it; the rows of a trial whose ``H`` could not be factored drop out of every sum and of
    ``count``.  Trials that carry ``missing`` raise ``ValueError``.

    Returns ``_pair_summary``' dict plus ``n_failed`` (failed E-step updates and failed trials; 0 in
    sample under the mean-field posterior) and, under the joint posterior, ``converged`` and ``n_newton`` per (fold, trial)
    or, in sample, per trial."""
    if how not in ("in_sample", "channels"):
        raise ValueError("how must be 'in_sample' or 'channels', got %r" % (how,))
    joint = _check_posterior(posterior)
    _no_missing(trials, "residual_correlation")
    scorer = _pair_scorer()
    N, L = int(params["ydim"]), int(params["zdim"])
    rows = int(sum(int(tr["y"].shape[0]) for tr in trials))
    n_failed, extra = 0, {}
    if how == "channels":
        groups = _check_groups(channel_folds(N, min(int(n_folds), N), seed) if groups is None else groups, N)
        if joint:
            got, _, n_failed, extra, _ = _joint_folds(trials, params, config, _group_masks(groups, rows, N), n_iter, device,
                                                      scorer)
        else:
            vb = config["method"] == "VB"
            n_it = int(config["max_iter"] if n_iter is None else n_iter)
            got = []
            with _resident(trials, params, _zero_start(trials, L), device) as eng:
                cap = default_max_replicas(rows, L, mask_channels=N, gauss=bool(eng.gauss.any()))
                for chunk in plan_chunks(list(_group_masks(groups, rows, N)), cap):
                    s, _, bad, _ = _replica_chunk(eng, n_it, config["dmu_bound"], vb, scorer=scorer, held_out=np.stack(chunk))
                    got.extend(s)
                    n_failed += bad
        total = np.full((3, N, N), np.nan)
        for k, g in enumerate(groups):
            total[np.ix_(range(3), g, g)] = got[k][np.ix_(range(3), g, g)]
    elif joint:
        with _posterior(trials, params, config, False, n_iter, device) as (eng, _):
            post = eng.joint_posterior(SET_TEST)
            total = scorer(eng, SET_TEST, True, mu=post["mu"], cov=post["cov"])[0][0]
        n_failed, extra = post["n_failed"], {"converged": post["converged"], "n_newton": post["n_newton"]}
    else:
        units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"], "v": tr.get("v", np.zeros((tr["y"].shape[0], L))),
                  "w": None} for tr in trials]
        with _resident(trials, params, units, device, priors=False) as eng:
            total = scorer(eng, SET_TEST, config.get("method", "VB") == "VB")[0][0]
    out = _pair_summary(*total)
    out["n_failed"] = int(n_failed)
    out.update(extra)
    return out


def _lag_summary(resid, model, count):
    """Residual autocorrelations from the lag moments (pure host code).  ``resid``, ``model``, ``count`` (K + 1, N):
    ``Engine.lag_moments``' sums; a (lag, channel) with ``count`` 0 or NaN was never scored.

    Returns a dict: ``resid``, ``model``, ``count`` with NaN where nothing was scored; ``residual_acf``, ``model_acf``,
    ``excess_acf`` and ``se_null`` (K + 1, N) and ``dispersion`` (N) by the module docstring, NaN where ``count`` is 0 or
    the channel's variance ``model[0] / count[0]`` is not positive; ``rms_excess`` (N) over the lags ``1 ... K`` with a
    finite excess, ``rms_excess_all`` over those of every channel and ``n_scored``, their number."""
    resid, model, count = (np.array(x, dtype=float) for x in (resid, model, count))
    if resid.ndim != 2 or model.shape != resid.shape or count.shape != resid.shape:
        raise ValueError("resid, model and count must be (K + 1, N), got %r, %r, %r" % (resid.shape, model.shape, count.shape))
    scored = count > 0  # (False for NaN)
    resid, model, count = (np.where(scored, x, np.nan) for x in (resid, model, count))
    with np.errstate(divide="ignore", invalid="ignore"):
        var = model[0] / count[0]
        var = np.where(var > 0, var, np.nan)
        residual_acf, model_acf = resid / count / var, model / count / var
        se_null = 1.0 / np.sqrt(count)
        dispersion = resid[0] / np.where(model[0] > 0, model[0], np.nan)
    excess = residual_acf - model_acf
    sq = np.where(np.isfinite(excess[1:]), excess[1:], 0.0) ** 2
    n_fin = np.isfinite(excess[1:]).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rms = np.where(n_fin > 0, np.sqrt(sq.sum(axis=0) / n_fin), np.nan)
    n_all = int(n_fin.sum())
    return {"resid": resid, "model": model, "count": count, "residual_acf": residual_acf, "model_acf": model_acf,
            "excess_acf": excess, "se_null": se_null, "dispersion": dispersion, "rms_excess": rms,
            "rms_excess_all": float(np.sqrt(sq.sum() / n_all)) if n_all else float("nan"), "n_scored": n_all}


def _lag_scorer(max_lag):
    """``Engine.lag_moments`` as ``_replica_chunk`` takes a scorer: per replica ``resid | model | count`` stacked, (n_rep, 3,
    K + 1, N), and no per-entry output; ``n_failed`` adds up the (unit, latent) pairs without a factor."""
    def scorer(eng, set_id, vb, mu=None, cov=None):
        resid, model, count, bad = eng.lag_moments(set_id, max_lag, vb=vb)
        scorer.n_failed += bad
        return np.stack([x.reshape((-1,) + x.shape[-2:]) for x in (resid, model, count)], axis=1), None
    scorer.width, scorer.predictive, scorer.n_failed = 3, True, 0
    return scorer


def _lag_replica_bytes(rows, L, max_lag):
    """Device bytes one more replica adds to a ``lag_moments`` call: ``w`` and the cross-time covariances ``c``."""
    return 8 * int(rows) * int(L) * (int(max_lag) + 2)


def residual_autocorrelation(trials, params, config, max_lag=20, how="in_sample", groups=None, n_folds=5, seed=0,
                             n_iter=None, device=0):
    """Residual autocorrelation of every channel: does its residual at bin ``t`` still predict the one at ``t + k``,
    ``k = 0 ... max_lag`` (at most 64), beyond what the predictive distribution says (module docstring)?  Excess at
    lags 1-3 is what spike-history regressors (``history=``) absorb; slow positive excess over many lags says the GP
    timescales ``omega`` are too smooth.  Pairs of bins never cross a trial.

    ``how="in_sample"``: the trials' own ``mu, v``.  ``how="channels"``: every fold of ``groups`` (default
    ``channel_folds(N, min(n_folds, N), seed)``) held out as a mask that is constant along the rows, the latents inferred
    without it from a zero start (``n_iter`` E-step iterations, default ``config["max_iter"]``), each channel taken from
    the replica that held it out.  The mean-field posterior only.  Trials that carry ``missing`` raise ``ValueError``.

    Returns ``_lag_summary``'s dict plus ``n_failed``: failed E-step updates and (trial, latent) pairs whose ``H`` had no
    factor (their trials are in no sum)."""
    if how not in ("in_sample", "channels"):
        raise ValueError("how must be 'in_sample' or 'channels', got %r" % (how,))
    max_lag = int(max_lag)
    if not 0 <= max_lag <= 64:
        raise ValueError("max_lag = %d, need 0 <= max_lag <= 64" % max_lag)
    _no_missing(trials, "residual_autocorrelation")
    scorer = _lag_scorer(max_lag)
    N, L = int(params["ydim"]), int(params["zdim"])
    rows = int(sum(int(tr["y"].shape[0]) for tr in trials))
    vb = config.get("method", "VB") == "VB"
    n_failed = 0
    if how == "channels":
        groups = _check_groups(channel_folds(N, min(int(n_folds), N), seed) if groups is None else groups, N)
        n_it = int(config["max_iter"] if n_iter is None else n_iter)
        got = []
        with _resident(trials, params, _zero_start(trials, L), device) as eng:
            cap = default_max_replicas(rows, L, mask_channels=N, gauss=bool(eng.gauss.any()),
                                       extra_bytes=_lag_replica_bytes(rows, L, max_lag))
            for chunk in plan_chunks(list(_group_masks(groups, rows, N)), cap):
                s, _, bad, _ = _replica_chunk(eng, n_it, config["dmu_bound"], vb, scorer=scorer, held_out=np.stack(chunk))
                got.extend(s)
                n_failed += bad
        total = np.full((3, max_lag + 1, N), np.nan)
        for k, g in enumerate(groups):
            total[:, :, g] = got[k][:, :, g]
    else:
        units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"], "v": tr.get("v", np.zeros((tr["y"].shape[0], L))),
                  "w": None} for tr in trials]
        with _resident(trials, params, units, device) as eng:
            total = scorer(eng, SET_TEST, vb)[0][0]
    out = _lag_summary(*total)
    out["n_failed"] = int(n_failed) + scorer.n_failed
    return out


def forward_prediction(trials, params, config, n_forward, n_iter=None, device=0, predictive=False, n_nodes=12):
    """Forward prediction of held-out trials: the last ``n_forward`` bins of every trial predicted from its first bins
    (module docstring for the definitions).

    ``trials``: dicts with ``y`` (T, N) and, with regressors, ``x`` (T, xdim, N); ``n_forward``: an integer with
    ``1 <= n_forward < min T``.  For every trial length ``T`` the full factor is ``params["cholesky"][T]`` where present,
    otherwise built from ``omega, sigma`` on the device; its first ``T - n_forward`` rows are the prior of the held-in
    rows, its last ``n_forward`` rows extend the posterior.  The latents are inferred on the held-in rows from a zero
    start, ``n_iter`` E-step iterations (default ``config["max_iter"]``), as ``leave_group_out`` infers its own; the
    forward rows are then scored by ``vlgp_loglik`` under ``mu_ahead, v_ahead``.  Neither ``params`` nor the trials are
    modified.

    Returns a dict: per trial ``mu_ahead``, ``v_ahead`` (n_forward, L) and ``rate`` (n_forward, N; Gaussian: means); per
    channel ``ll``, ``ll_null``, ``n_spikes``, ``bits_per_spike`` (``bits_per_spike``'s null: the channel's mean count
    over the forward rows, comparable with ``leave_group_out``) and ``ll_null_past``, ``bits_per_spike_past`` (null: the
    mean count over the held-in rows); ``fp_bps`` and ``fp_bps_past``, pooled by ``co_bits_per_spike``'s rule;
    ``off_fixed_point`` (trials, L); ``n_failed`` (failed E-step updates plus (trial, latent) extensions whose ``H`` had
    a pivot that was not positive: their NaN reaches every number they enter).  ``predictive``, ``n_nodes``: as
    ``leave_one_out`` -- here the two densities part most, since ``v_ahead`` grows with every bin ahead."""
    density = _density(predictive, n_nodes)
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    if isinstance(n_forward, bool) or not isinstance(n_forward, (int, np.integer)):
        raise ValueError("n_forward must be an integer, got %r" % (n_forward,))
    if not lengths or not 1 <= n_forward < min(lengths):
        raise ValueError("need 1 <= n_forward < the shortest trial (%s bins), got %d"
                         % (min(lengths) if lengths else "no", n_forward))
    nf = int(n_forward)
    vb = config["method"] == "VB"
    held_in = [T - nf for T in lengths]
    with _extended(trials, held_in, nf, params, config, n_iter, device) as (eng, mu_ext, v_ext, terms, n_failed):
        ahead = [{"y": tr["y"][T:], "x": None if tr.get("x") is None else tr["x"][T:],
                  "mu": mu_ext[i * nf:(i + 1) * nf], "v": v_ext[i * nf:(i + 1) * nf], "w": None}
                 for i, (tr, T) in enumerate(zip(trials, held_in))]
        eng.upload(SET_FORWARD, ahead)
        sums, rate = _score(eng, SET_FORWARD, vb, density)
        gauss = eng.gauss.copy()
    ahead_rows = [nf] * len(trials)
    rows = nf * len(trials)
    ll, ll_null, ny, bps = bits_per_spike(sums, rows, gauss)
    past = np.sum([np.sum(np.asarray(tr["y"][:T], dtype=float), axis=0) for tr, T in zip(trials, held_in)], axis=0) \
        / float(sum(held_in))
    known = ~gauss & (past > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ll_null_past = np.where(known, ny * np.log(np.where(known, past, 1.0)) - rows * past - sums[:, 3], np.nan)
        bps_past = np.where(known & (ny > 0), (ll - ll_null_past) / (ny * math.log(2.0)), np.nan)
        off = terms[:, :, 0] / np.maximum(terms[:, :, 1], np.finfo(float).tiny)
    return {
        "mu_ahead": _per_trial(mu_ext, ahead_rows), "v_ahead": _per_trial(v_ext, ahead_rows),
        "rate": _per_trial(rate, ahead_rows),
        "ll": ll, "ll_null": ll_null, "n_spikes": ny, "bits_per_spike": bps,
        "ll_null_past": ll_null_past, "bits_per_spike_past": bps_past,
        "fp_bps": co_bits_per_spike(ll, ll_null, ny), "fp_bps_past": co_bits_per_spike(ll, ll_null_past, ny),
        "off_fixed_point": off, "n_failed": int(n_failed), **_PREDICTIVE_KEY[density is not None],
    }


def weights_summary(log_w):
    """Per unit, from importance weights ``log_w`` (units, K) or (K,): ``(iwae, elbo_mc, ess)`` with
    ``iwae = logsumexp_k(log_w) - log K``, ``elbo_mc = mean_k log_w`` and ``ess = (sum w)^2 / sum w^2`` (pure host code).
    The largest ``log_w`` of a row is taken out before the exponential, so values near -1e5 lose nothing; a row that
    holds a NaN gives NaN three times."""
    log_w = np.asarray(log_w, dtype=float)
    if log_w.ndim not in (1, 2) or log_w.shape[-1] < 1:
        raise ValueError("log_w must be (units, K) or (K,) with K >= 1")
    K = log_w.shape[-1]
    top = np.max(log_w, axis=-1)  # (NaN where the row holds one)
    shift = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.exp(log_w - shift[..., None])
        s1, s2 = np.sum(w, axis=-1), np.sum(w * w, axis=-1)
        iwae = shift + np.log(s1) - math.log(K)
        ess = s1 * s1 / s2
    bad = np.isnan(top)
    return np.where(bad, np.nan, iwae), np.where(bad, np.nan, np.mean(log_w, axis=-1)), np.where(bad, np.nan, ess)


@contextlib.contextmanager
def _posterior(trials, params, config, infer, n_iter, device, estep=True):
    """``(eng, n_failed)``: a ``_resident`` engine whose ``SET_TEST`` holds the trials' posterior -- with ``infer`` from a
    zero start and ``n_iter`` E-step iterations (default ``config["max_iter"]``; ``n_failed`` its failed updates), else the
    trials' stored ``mu, v, w`` (``n_failed = 0``).  ``estep=False`` leaves the zero start as it is: the caller's E-step
    runs on a replica of the set."""
    L = int(params["zdim"])
    if infer:
        units = _zero_start(trials, L)
    else:
        units = [{"y": tr["y"], "x": tr.get("x"), "mu": tr["mu"],
                  **{k: tr[k] if tr.get(k) is not None else np.zeros((tr["y"].shape[0], L)) for k in ("v", "w")}}
                 for tr in trials]
    n_iter = int(config["max_iter"] if n_iter is None else n_iter)
    with _resident(trials, params, units, device) as eng:
        yield eng, eng.estep(SET_TEST, n_iter, config["dmu_bound"], config["method"] == "VB") if infer and estep else 0


def _evidence_bps(total, sums, rows, gauss):
    """``(total - LL_null) / (n_spikes ln 2)`` of an evidence ``total`` over ``rows`` rows, ``LL_null`` the constant-rate
    null of ``bits_per_spike`` from ``vlgp_loglik``'s ``sums``; NaN unless every channel is Poisson and there is a spike."""
    _, ll_null, ny, _ = bits_per_spike(sums, rows, gauss)
    if gauss.any() or not np.sum(ny) > 0:
        return float("nan")
    return float((total - np.sum(ll_null)) / (np.sum(ny) * math.log(2.0)))


def marginal_loglik(trials, params, config, n_samples=64, seed=0, rng=None, infer=True, n_iter=None, device=0,
                    proposal="posterior", max_iter=50, tol=1e-10):
    """Importance-weighted estimate of the marginal log-likelihood ``log p(y_trial)`` of every trial, the fitted
    posterior as proposal (module docstring for the definitions).

    ``infer=True`` is for held-out trials: the posterior comes from a zero start and ``n_iter`` E-step iterations
    (default ``config["max_iter"]``), as ``leave_group_out`` infers its own, and the dicts' ``mu, v, w`` are not read.
    ``infer=False`` is for a fit's own trials and uses their stored ``mu, v, w``.  The normals come from ``rng`` (a
    ``numpy.random.Generator``; default ``np.random.default_rng(seed)``) in sample chunks of 64: chunk ``c`` is
    ``rng.standard_normal((n_trials, L, R, min(64, left)))``, so the first samples are the same whatever ``n_samples`` is
    and host memory does not grow with it.  Trials that carry ``missing`` raise ``ValueError``.  Neither ``params`` nor
    the trials are modified.

    Returns a dict: ``log_w`` (trials, n_samples); per trial ``iwae``, ``elbo_mc``, ``ess`` (``weights_summary``);
    ``total``, the sum of ``iwae``; ``elbo``, the deterministic ``vlgp_elbo`` value of the same posterior, and
    ``gap = total - elbo`` (NaN under MAP, where there is no bound); ``marginal_bps = (total - LL_null) /
    (n_spikes ln 2)`` with ``LL_null`` the constant-rate null of ``bits_per_spike`` over all evaluated rows, NaN unless
    every channel is Poisson; ``n_failed`` (failed E-step updates plus (trial, latent) pairs whose ``H`` could not be
    factored: such a trial's ``log_w`` is NaN, and so is every number it enters).

    ``proposal="joint"`` draws from the joint Laplace posterior ``N(beta_hat, H^-1)`` of every trial instead
    (``joint_posterior``; ``max_iter`` and ``tol`` are its Newton iteration's), with the same normals, the same chunks of 64
    and the same keys, plus per trial ``laplace``, the Laplace evidence, and ``converged``.  The Newton iteration runs once
    and the device walks the chunks itself, so the normals of all chunks are held at once.  ``elbo`` and ``gap`` still
    describe the mean-field posterior the Newton iteration started from.  Any other ``proposal`` raises ``ValueError``."""
    _no_missing(trials, "marginal_loglik")
    if proposal not in ("posterior", "joint"):
        raise ValueError("proposal must be 'posterior' or 'joint', got %r" % (proposal,))
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
        raise ValueError("n_samples must be an integer >= 1, got %r" % (n_samples,))
    K, L, R = int(n_samples), int(params["zdim"]), int(params["rank"])
    vb = config["method"] == "VB"
    rng = np.random.default_rng(seed) if rng is None else rng
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    log_w = np.empty((len(trials), K))
    with _posterior(trials, params, config, infer, n_iter, device) as (eng, n_failed):
        chunks = []
        for k0 in range(0, K, SAMPLE_CHUNK):
            kc = min(SAMPLE_CHUNK, K - k0)
            eps = rng.standard_normal((len(trials), L, R, kc))
            if proposal == "joint":
                chunks.append(eps)  # (one call: the Newton iteration runs once, the device walks the chunks itself)
            else:
                log_w[:, k0:k0 + kc], bad, _ = eng.marginal(SET_TEST, eps, vb=vb)
        if proposal == "joint":
            joint = eng.joint_laplace(SET_TEST, max_iter=max_iter, tol=tol, eps=np.concatenate(chunks, axis=3))
            log_w[:], bad = joint["log_w"], joint["n_failed"]
        bound = elbo_from_terms(*eng.elbo(SET_TEST, vb=vb)[:2], eng.unit_ranks(SET_TEST), vb=vb)["elbo"]
        sums, _ = eng.loglik(SET_TEST, vb=vb)
        gauss = eng.gauss.copy()
    iwae, elbo_mc, ess = weights_summary(log_w)
    total = float(np.sum(iwae))
    out = {"log_w": log_w, "iwae": iwae, "elbo_mc": elbo_mc, "ess": ess, "total": total, "elbo": bound,
           "gap": total - bound, "marginal_bps": _evidence_bps(total, sums, sum(lengths), gauss),
           "n_failed": int(n_failed) + int(bad)}
    if proposal == "joint":
        out.update(laplace=joint["laplace"], converged=joint["converged"])
    return out


def joint_posterior(trials, params, config, infer=True, n_iter=None, max_iter=50, tol=1e-10, device=0, held_out=None,
                    cov=None):
    """The joint Laplace posterior of every trial: the mode of the posterior over all prior weights of the trial, found by
    a damped Newton iteration on the device (module docstring for the definitions).

    ``infer=True`` is for held-out trials: an E-step from a zero start, ``n_iter`` iterations (default
    ``config["max_iter"]``) as ``marginal_loglik`` runs it, gives the mean-field centres the Newton iteration starts from;
    ``infer=False`` starts from the trials' stored ``mu, w``.  The mode does not depend on the start.  ``max_iter``: most
    factorisations of ``H`` per trial; ``tol``: the Newton decrement at which a trial stops.  Trials that carry ``missing``
    raise ``ValueError``.  Neither ``params`` nor the trials are modified.

    Returns a dict: per trial ``mu``, ``v`` (T, L) -- ``v`` includes the coupling between latents, whatever
    ``config["method"]`` is --, ``laplace`` (the Laplace evidence ``log p(y_trial)``), ``converged``, ``n_newton``; and
    over all trials ``total``, the sum of ``laplace``; ``laplace_bps = (total - LL_null) / (n_spikes ln 2)`` by
    ``marginal_loglik``'s null model, NaN unless every channel is Poisson; ``n_failed`` (failed E-step updates plus trials
    whose ``H`` could not be factored: their numbers are NaN, and so is ``total``).

    ``cov=True`` adds per trial ``cov`` (T, L, L), the covariance of the latents of every bin, whose diagonal is ``v``
    (``vlgp_joint_posterior``).  ``held_out``: per trial a (T, N) bool, True where an entry is held out -- neither the
    E-step nor the Newton iteration sees those entries, whatever ``y`` holds there, and ``laplace`` is the evidence of the
    others; ``cov`` then defaults to True, the E-step runs on a masked replica of the trials (``infer=False`` starts it
    from the stored posterior), and ``laplace_bps`` is NaN: its null model counts every entry."""
    _no_missing(trials, "joint_posterior")
    vb = config["method"] == "VB"
    lengths = [int(tr["y"].shape[0]) for tr in trials]
    want_cov = held_out is not None if cov is None else bool(cov)
    if held_out is not None:
        held = np.concatenate(_per_trial_entries(held_out, trials, "held_out", bool), axis=0)
    with _posterior(trials, params, config, infer, n_iter, device, estep=held_out is None) as (eng, n_failed):
        sid = SET_TEST
        if held_out is not None:
            sid = SET_REPLICAS
            eng.replicate(SET_TEST, sid, held_out=held[None])
            n_iter = int(config["max_iter"] if n_iter is None else n_iter)
            n_failed = eng.estep(sid, n_iter, config["dmu_bound"], vb) if infer else 0
        if want_cov or held_out is not None:
            joint = eng.joint_posterior(sid, max_iter=max_iter, tol=tol)
            joint["v"] = np.ascontiguousarray(np.diagonal(joint["cov"], axis1=1, axis2=2))
        else:
            joint = eng.joint_laplace(sid, max_iter=max_iter, tol=tol)
        if held_out is not None:
            eng.free_units(sid)
        sums = None if held_out is not None else eng.loglik(SET_TEST, vb=vb)[0]
        gauss = eng.gauss.copy()
    total = float(np.sum(joint["laplace"]))
    out = {"mu": _per_trial(joint["mu"], lengths), "v": _per_trial(joint["v"], lengths), "laplace": joint["laplace"],
           "converged": joint["converged"], "n_newton": joint["n_newton"], "total": total,
           "laplace_bps": float("nan") if held_out is not None else _evidence_bps(total, sums, sum(lengths), gauss),
           "n_failed": int(n_failed) + int(joint["n_failed"])}
    if want_cov:
        out["cov"] = _per_trial(joint["cov"], lengths)
    return out
