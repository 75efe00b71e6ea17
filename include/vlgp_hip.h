/*
 * vlgp_hip.h -- C ABI of libvlgp_hip.so, the MI355X (gfx950) engine behind the
 * variational-EM hot path of catniplab/vlgp.
 *
 * The reference has no FFI: its seam is the Python contract
 *     estep|mstep|hstep|update_w|update_v|make_cholesky|infer(trials, params, config) -> None
 * (vlgp/core.py:22-471, vlgp/gp.py:65-162).  Each entry point below names the
 * reference function it replaces.  The Python host (vlgp_amd/engine.py) binds
 * these with ctypes; see INTEGRATION.md for the stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point is IEEE double
 *   - every function returns an int status: 0 = ok, <0 = error (text via
 *     vlgp_last_error); nothing throws across the boundary
 *   - caller owns host buffers; the library owns device buffers behind the
 *     opaque handle; one host thread per handle; one handle per GPU
 *   - all work is enqueued on the handle's own HIP stream; calls that return
 *     host data synchronise that stream, the others are asynchronous
 *   - numerical failures never return an error: a non-positive pivot in a
 *     Cholesky zeroes that latent's update for that unit (reference:
 *     vlgp/core.py:92-94,112-113,194-196) and is counted in *n_failed
 *
 * Data model
 *   unit      one trial or one fixed-length segment: T_m time bins
 *   unit set  M units packed back to back in row-major arrays
 *               y   (rows, N)      observations          rows = sum T_m
 *               x   (rows, P, N)   regressors (NULL = all ones, P must be 1)
 *               mu, v, w, dmu (rows, L)
 *             addressed through a CSR-style offsets[M+1]; VLGP_MAX_SETS slots
 *   params    a (L, N) loading, b (P, N) bias/regression, noise (N)
 *   prior     per distinct unit length T: G (L, T, R), K_l ~= G_l G_l^T
 */
#ifndef VLGP_HIP_H
#define VLGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLGP_ABI_VERSION 3
#define VLGP_MAX_SETS 4
#define VLGP_MAX_L 64             /* latents per handle.  The reference has no bound (vlgp/core.py:76,106; gp.py:82);
                                     up to 10 the specialised kernels run, up to 16 the register-resident generic
                                     ones, above that loop-based fallbacks (slow, same results) */
#define VLGP_MAX_XDIM 64          /* regressors per channel (1 + history, vlgp/preprocess.py:53): up to 8 specialised */
#define VLGP_MAX_RANK 64          /* R <= 64 (the reference hard-codes 50, preprocess.py:75) */
#define VLGP_UNIQUE_ID_BYTES 128

#define VLGP_OK 0
#define VLGP_ERR_ARG (-1)         /* bad argument / shape */
#define VLGP_ERR_HIP (-2)         /* HIP runtime error (no GPU, OOM, launch failure) */
#define VLGP_ERR_STATE (-3)       /* call sequence error (missing prior, empty set ...) */
#define VLGP_ERR_COMM (-4)        /* RCCL error */

typedef struct vlgp_ctx vlgp_ctx;

/* ---- lifetime --------------------------------------------------------- */
int vlgp_abi_version(void);
int vlgp_device_count(int* count);
/* gauss_mask[n] != 0 marks a Gaussian channel, 0 a Poisson one
 * (params["likelihood"], vlgp/preprocess.py:59-64). */
int vlgp_create(int device, int N, int L, int P, int R, const uint8_t* gauss_mask,
                vlgp_ctx** out);
int vlgp_destroy(vlgp_ctx* ctx);
/* Last error text of this handle (or of the failed vlgp_create when ctx is NULL). */
const char* vlgp_last_error(vlgp_ctx* ctx);
int vlgp_synchronize(vlgp_ctx* ctx);
/* Drains the main stream only: an M-step begun with vlgp_mstep_begin keeps running on its lane (vlgp_synchronize
 * waits for it too).  The EM loop uses it to time the E-step (core.py:307-315) with the M-step already enqueued. */
int vlgp_synchronize_main(vlgp_ctx* ctx);

/* ---- unit sets -------------------------------------------------------- */
/* Replaces the list-of-dicts the reference passes around (trial dict keys
 * y, x, mu, w, v; vlgp/preprocess.py:38-46).  x == NULL means x == 1, P == 1
 * (what preprocess.initialize builds when the user gives no regressors);
 * mu, v, w may be NULL (zero-filled). */
int vlgp_upload_units(vlgp_ctx* ctx, int set, int M, const int64_t* offsets,
                      const double* y, const double* x, const double* mu,
                      const double* v, const double* w);
/* util.cut_trials (vlgp/util.py:457-499): build set `dst` of M_dst units of
 * `window` rows each, unit k starting at row src_row_start[k] of set `src`.
 * When the segments tile `src` exactly (no overlap) `dst` aliases the same
 * device arrays, as the reference's NumPy views do; otherwise rows are copied
 * and segments are independent ("Hard parts"). */
int vlgp_cut_units(vlgp_ctx* ctx, int src, int dst, int M_dst,
                   const int64_t* src_row_start, int window);
/* Write mu and v of a cut set back into its source set (no-op when aliased;
 * with overlapping segments later segments win, in order). */
int vlgp_merge_units(vlgp_ctx* ctx, int cut_set);
/* Overlapping segments of a copied cut (trial lengths that are not multiples of the window).  In the reference they are
 * NumPy VIEWS of the same trial rows (vlgp/util.py:482-496): core.estep runs them one after the other, segment k + 1
 * starting from the mu, v that segment k left in the shared rows (vlgp/core.py:123-126), and an in-place constraint
 * (vlgp/core.py:374-388,413-416) touches a shared row once per segment that holds it.  The caller orders the units of
 * the cut STAGE-MAJOR (stage = position in a chain of overlapping neighbours; stage_start[n_stages + 1] unit indices)
 * and lists the links (first unit, second unit, shared rows), sorted by the stage of their second unit
 * (link_start[n_stages + 1]).  vlgp_estep then runs stage by stage, copying the shared rows forward before and back
 * after each stage; vlgp_apply_latent_map applies its map a second time to the shared rows.  vlgp_unshare_mu: mu stops
 * being shared (constrain_loading "svd" rebinds every segment's mu, vlgp/core.py:407-408); v stays shared. */
int vlgp_set_overlaps(vlgp_ctx* ctx, int set, int n_stages, const int* stage_start, int n_links,
                      const int* links, const int* link_start);
int vlgp_unshare_mu(vlgp_ctx* ctx, int set);
/* restore == 0: keep a device-side copy of the set's mu; restore != 0: write it back.  For the one place where
 * the reference DETACHES segments from their trials: constrain_loading == "svd" rebinds every segment's mu
 * (vlgp/core.py:407-408, `trial["mu"] = trial["mu"] @ us`), after which the parent trials keep the values they
 * had at that moment -- the final inference of fit starts from those. */
int vlgp_stash_mu(vlgp_ctx* ctx, int set, int restore);
/* Any of the output pointers may be NULL. */
int vlgp_download_units(vlgp_ctx* ctx, int set, double* mu, double* v, double* w,
                        double* dmu);
int vlgp_free_units(vlgp_ctx* ctx, int set);

/* ---- held-out evaluation ---------------------------------------------- */
/* Leave-one-neuron-out replicas (no counterpart in the reference, whose evaluation.loglik is broken).  Set `dst` becomes
 * n_rep replicas of set `src`, replica-major (unit k M_src + m is unit m of replica k), replica k leaving channel
 * channel[k] out of its E-step: vlgp_estep on `dst` runs what it would run with a[:, channel[k]] = 0 for replica k,
 * bit for bit.  y and x (and x.b) are ALIASED to `src`; mu, v, w, dmu start as copies of src's.  `src` must be a plain
 * uploaded set (not a cut, no overlap stages).  While a replica set exists, vlgp_upload_units and vlgp_free_units on
 * `src` return VLGP_ERR_STATE, and so does a cut or a replicate call whose destination is `src`.
 * WHICH ENTRY POINT TAKES WHICH KIND OF SET is one table, DESIGN.md 4.6 (csrc/api.hip holds it as data).  In short: a
 * replicated set takes vlgp_estep (split E-step only: a configuration that kernel family cannot run -- L > 10, N > 1024,
 * long units at R above its limit, short units at effective rank > 32 -- is VLGP_ERR_STATE, never another kernel),
 * vlgp_download_units, vlgp_upload_units, vlgp_free_units and vlgp_loglik; a masked set of ONE replica
 * (vlgp_replicate_masked) also takes the entry points a fit runs; every other entry point refuses a replicated set
 * with VLGP_ERR_STATE.  The same as vlgp_replicate_groups (below) with one channel per group. */
int vlgp_replicate_units(vlgp_ctx* ctx, int src, int dst, int n_rep, const int* channel);
/* Speckled hold-out: replicas that leave single (row, channel) ENTRIES out -- the general form of vlgp_replicate_groups
 * (declared at the end of this header), whose groups are masks that are constant along the rows.  held_out is
 * (n_rep, rows_src, nw) words, nw = (N + 63) / 64: bit n & 63 of word n >> 6 is set when replica k leaves entry (row, n) of
 * `src` out.  vlgp_estep on `dst` then runs for replica k the E-step with the likelihood terms of those entries removed:
 * their working residual and curvature are 0, and with them their contributions to y.a, to w and to the Gaussian constant of
 * w; everything else -- the regressors x as the caller gave them included -- is untouched.  A mask constant along the rows
 * gives the bits of vlgp_replicate_groups.  A set bit at a position >= N is VLGP_ERR_ARG, the message naming the replica
 * and the row, nothing changed; a replica with no bit set, a row with every bit set (there w == 0: the prior alone) and a
 * channel held out on every row are legal.  src, dst, aliasing, lifetime and the entry points that accept the set are those
 * of vlgp_replicate_groups.  Costs one mask word per (row, 64 channels) and, with a Gaussian channel on the handle, L
 * doubles per row for the constant of w.
 * vlgp_loglik on such a set: sums (n_rep, N, 4), slot (k, n) holding the four sums of channel n over exactly the rows where
 * replica k holds (row, n) out (an empty slot: four zeros); rate (rows_src, N) or NULL, NaN where no replica holds the
 * entry out, else written from the replica that does -- asking for rate when two replicas hold the same entry out is
 * VLGP_ERR_ARG (decided when the set is made).  At most 65535 replicas.
 *
 * ONE replica (n_rep == 1) makes a masked fit set: the rows and units of `src`, a set bit meaning "this entry of y is
 * missing".  Besides the entry points above it takes the ones a fit runs: vlgp_update_w and vlgp_update_v (w of a row
 * sums over its observed channels, through the split E-step's by-row passes), vlgp_norms, vlgp_norms_begin,
 * vlgp_norms_end, vlgp_apply_latent_map, vlgp_latent_moments, vlgp_hstep_prepare, vlgp_hstep_begin,
 * vlgp_hstep_objective, vlgp_hstep_end (all of them read mu, v, w, dmu alone) and vlgp_mstep, vlgp_mstep_begin,
 * vlgp_mstep_end: the M-step of every channel over its observed rows only -- mu'y, x'y, every gradient and Hessian sum
 * and the noise variance (mean and variance over the channel's own observed rows; the number of observed rows per
 * channel is counted when the set is made).  What y holds at a missing entry, NaN included, reaches no sum; with no bit
 * set a, b, da, db are those of `src`, bit for bit, and noise is that of its two-pass form.  A channel with no observed
 * row keeps a, b, noise and is not counted in *n_failed.  The masked M-step is VLGP_ERR_STATE, the message naming the
 * reason, with a Gaussian channel on the handle, on the loop-based kernels (P > 8, VLGP_MSTEP_GENERIC), beyond 10
 * latents and with more than one rank.  The Laplace EM takes it too: vlgp_joint_posterior (the Newton E-step never
 * reads a missing entry) and vlgp_mstep_cov_masked (that M-step under the posterior's covariance per row; a set
 * without a mask goes to vlgp_mstep_cov).  vlgp_elbo, vlgp_forecast, vlgp_project_units, cuts, merges, stashes and
 * overlaps refuse a masked fit set like every replicated set; a group-replica set and a masked set of several
 * replicas are refused by all of the above (the whole table: DESIGN.md 4.6). */
int vlgp_replicate_masked(vlgp_ctx* ctx, int src, int dst, int n_rep, const uint64_t* held_out);
/* Plug-in rate and log-likelihood of the observations under the set's current posterior (mu, v):
 *   Poisson   rate = trunc_exp(a_n.mu_t + (b x)_tn + 1/2 (a_n^2).v_t)  (the E-step's rate; vb == 0 drops the v term)
 *             ll = y log rate - rate - lgamma(y + 1);   sums[n] = {sum ll, sum y, sum rate, sum lgamma(y + 1)}
 *   Gaussian  rate = eta = a_n.mu_t + (b x)_tn
 *             ll = -log(2 pi noise_n) / 2 - (y - eta)^2 / (2 noise_n);   sums[n] = {sum ll, sum y, sum eta, sum y^2}
 * Plain set: rate (rows, N) row-major or NULL, sums (N, 4), channels in plain order.  Replicated set: one slot per
 * (replica, left-out channel) pair, in the order of the channel list the set was made with -- pair p is channel[p] under
 * the posterior of the replica that leaves it out, on the source rows: rate (rows_src, n_pairs) or NULL, sums
 * (n_pairs, 4).  A set made by vlgp_replicate_units has n_pairs == n_rep.  At most 65535 pairs per set (VLGP_ERR_ARG
 * beyond).  A set made by vlgp_replicate_masked: see there.  Sums cover this handle's units only (no reduction over ranks) and are bitwise reproducible (fixed-order
 * two-stage reduction, no atomics). */
int vlgp_loglik(vlgp_ctx* ctx, int set, int vb, double* rate, double* sums);
/* Terms of the variational lower bound of a set that is not replicated (VLGP_ERR_STATE otherwise) under its
 * current posterior (mu, v, w), the current parameters and the prior factors the set's lengths are bound to.
 *   row_sums (N, 4): per channel, with eta = a_n.mu_t + (b x)_tn and s = 1/2 (a_n^2).v_t (s = 0 when vb == 0),
 *     Poisson   {sum E_q log p, sum y, sum rate, sum y s},  E_q log p = y eta - trunc_exp(eta + s) - lgamma(y + 1)
 *     Gaussian  {sum E_q log p, sum y, sum eta, sum s / noise_n},
 *               E_q log p = -log(2 pi noise_n) / 2 - ((y - eta)^2 + 2 s) / (2 noise_n)
 *   row_ell (rows) or NULL: per row the sum of E_q log p over the channels (the per-unit split is the caller's sum)
 *   kl_terms (units, L, 4): with G the compact (T, r) prior factor of the unit's length and latent,
 *     H = I_r + G' diag(w) G and beta = argmin |G beta - mu|:  {log det H, tr H^-1, beta'beta, |mu - G beta|^2};
 *     KL[q || p] = (tr H^-1 + beta'beta - r + log det H) / 2.  A pivot of H or G'G that is not positive makes the four
 *     terms of that (unit, latent) NaN; *n_failed (may be NULL) counts those pairs.
 * Waits for a pending M-step and norms pass; changes no unit state, no parameter and nothing vlgp_hstep_prepare built.
 * This handle's units only (no reduction over ranks); fixed-order reductions, no atomics: the same bits on every run. */
int vlgp_elbo(vlgp_ctx* ctx, int set, int vb, double* row_sums, double* row_ell, double* kl_terms, int* n_failed);
/* Forward prediction: carries the posterior of every (unit, latent) of a plain uploaded set past the unit's last row.
 * With G (T, r) the compact prior factor the unit's length is bound to, mu, v, w the unit's columns and g the E-step's
 * working gradient
 * (g[t] = sum_n a[l, n] res[t, n]; res = y - trunc_exp(eta + 1/2 (a^2).v) Poisson, (y - eta) / noise Gaussian; the v term
 * dropped when vb == 0):
 *   H = I_r + G' diag(w) G = Lc Lc',   beta = H^-1 G' (g + w o mu)      (G beta is the next unclipped Newton iterate)
 *   mu_ext = G_ext[:, :r] beta,   v_ext[t] = |Lc^-1 G_ext[t, :r]'|^2 + sum_{c >= r} G_ext[t, c]^2   (0 when vb == 0)
 *   fit_terms = {|G beta - mu|^2, |mu|^2}
 * lengths[n_lengths], strictly increasing, lists every unit length of the set; n_ext[k] >= 1 rows extend a unit of
 * lengths[k]; G_ext holds the blocks (L, n_ext[k], R) back to back in the order of lengths: the rows of the factorisation
 * whose first lengths[k] rows are the prior of that length.  mu_ext, v_ext (sum over the units of their n_ext, L),
 * unit-major; fit_terms (M, L, 2) and n_failed may be NULL.  A pivot of H that is not positive and finite makes the task's
 * mu_ext, v_ext and fit_terms NaN and is counted in *n_failed.  A cut or replicated set, parameters not set or a length
 * without a prior: VLGP_ERR_STATE; a length that is not listed, n_ext < 1 or a null output: VLGP_ERR_ARG, the message
 * naming the offender, nothing changed.  Waits for a pending M-step and norms pass; changes no unit state, no parameter
 * and nothing vlgp_hstep_prepare built.  Fixed-order reductions, no atomics: the same bits on every run. */
int vlgp_forecast(vlgp_ctx* ctx, int set, int vb, int n_lengths, const int* lengths, const int* n_ext,
                  const double* G_ext, double* mu_ext, double* v_ext, double* fit_terms, int* n_failed);
/* Importance weights of the marginal likelihood log p(y_unit) of every unit of a set that is not replicated (DESIGN.md
 * 4.6: VLGP_ERR_STATE otherwise), the fitted posterior as proposal (the IWAE estimate).  Per (unit, latent), with G, mu, v,
 * w, g, H = Lc Lc' and m = H^-1 G' (g + w o mu) exactly as in vlgp_forecast (vb == 0 drops the v term of g: the Laplace
 * approximation of a MAP fit), draw k of n_samples takes eps_k (r standard normals supplied by the caller):
 *   d = Lc^-T eps_k,  beta_k = m + d,  x_k[t, l] = G[t, :] . beta_k
 *   c[u, l, k] = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H       (log N(beta; 0, I) - log N(beta; m, H^-1))
 *   ll[u, k] = sum_t sum_n log p(y[t, n] | eta = a_n . x_k[t] + (b x)_tn)   (no v term: x_k is a sample)
 *     Poisson y eta - trunc_exp(eta) - lgamma(y + 1);   Gaussian -log(2 pi noise_n) / 2 - (y - eta)^2 / (2 noise_n)
 *   log_w[u, k] = ll[u, k] + sum_l c[u, l, k]
 * eps is (units, L, R, n_samples), the sample index contiguous; rows >= r of a (unit, latent) are never read.  log_w
 * (units, n_samples); parts (units, n_samples, 2) = {ll, sum_l c}, whose two entries add to log_w, or NULL.  mean_k
 * exp(log_w[u, k]) is unbiased for p(y_u) whatever mu, v, w hold: they decide its variance alone.  A pivot of H that is not
 * positive and finite makes the unit's log_w NaN and is counted in *n_failed (may be NULL).  The samples are walked 64 at
 * a time: the call's device memory does not grow with n_samples, and sample k's numbers are the same bits whatever
 * n_samples is.  n_samples < 1 or a null eps or log_w: VLGP_ERR_ARG, the message naming the offender; parameters not
 * set or a length without a prior: VLGP_ERR_STATE.  Waits for a pending M-step and norms pass; changes no unit state, no
 * parameter and nothing vlgp_hstep_prepare built.  Fixed-order sums, no atomics: the same bits on every run. */
int vlgp_marginal(vlgp_ctx* ctx, int set, int vb, int n_samples, const double* eps, double* log_w, double* parts,
                  int* n_failed);
/* Joint Laplace posterior of every unit of a set that is not replicated (VLGP_ERR_STATE otherwise; 4.11):
 * the mode of the posterior over ALL prior weights beta = (beta_1 ... beta_L) of a unit by a damped Newton iteration, the
 * Laplace evidence, latent variances that include the coupling between latents, and joint Gaussian draws for the
 * importance weights of vlgp_marginal.  For a unit of T rows, G_l (T x r_l) the compact prior factor of latent l, the
 * stacked index (l, i) latent-major, D = sum_l r_l:
 *   x[t, l] = G_l[t, :] . beta_l,   eta[t, n] = a_n . x[t] + (b x)_tn          (no v term: the model of vlgp_marginal's ll)
 *   Poisson   lam = trunc_exp(eta),  ll = y eta - lam - lgamma(y + 1),  res = y - lam,  cur = lam
 *   Gaussian  ll = -log(2 pi noise_n) / 2 - (y - eta)^2 / (2 noise_n),  res = (y - eta) / noise_n,  cur = 1 / noise_n
 *   f(beta) = 1/2 |beta|^2 - sum_t sum_n ll
 *   grad_l f = beta_l - G_l' g[:, l],   g[t, l] = sum_n a[l, n] res[t, n]
 *   H[(l, i), (l', j)] = delta + sum_t G_l[t, i] c[t, l, l'] G_l'[t, j],   c[t, l, l'] = sum_n a[l, n] a[l', n] cur[t, n]
 *   H = Lc Lc'; the mode is the zero of grad f, unique while no eta is above the clamp of trunc_exp.
 * Start: the mean-field centres m_l = H_l^-1 G_l' (g + w o mu)_l of vlgp_forecast from the set's current mu, w, vb = 0.
 * Step: d = H^-1 grad f, decrement = grad f' H^-1 grad f.  A unit stops converged when decrement <= tol, and not
 * converged after max_iter factorisations of H.  The trial point beta - s d, s = 1, is accepted when
 *   f(beta - s d) <= f(beta) - 1e-4 s decrement + 2^-46 (1/2 |beta - s d|^2 + sum of the absolute terms of ll),
 * the last term being the rounding of the sum f is; otherwise s is halved, and a unit whose s falls below 2^-30 stops
 * where it stands, not converged.  f never increases beyond that rounding.  Then
 *   laplace = ll(beta) - 1/2 |beta|^2 - 1/2 log det H(beta)
 *   mu[t, l] = G_l[t, :] . beta_l,   v[t, l] = G_l[t, :] (H^-1)_ll G_l[t, :]'
 *   draw k:  beta_k = beta + Lc^-T eps_k,  c_k = -1/2 |beta_k|^2 + 1/2 |eps_k|^2 - 1/2 log det H,
 *            log_w[u, k] = ll(beta_k) + c_k;  mean_k exp(log_w) is unbiased for p(y_u) wherever beta stands.
 * beta (units, L, R), entries at or beyond r_l zero; stats (units, 8) = {laplace, ll(beta), |beta|^2, log det H, final
 * decrement, factorisations taken, converged 0/1, D}; mu, v (rows, L); eps (units, L, R, n_samples) and log_w
 * (units, n_samples) as in vlgp_marginal, rows >= r_l of eps never read; parts (units, n_samples, 2) = {ll, c}, whose two
 * entries add to log_w.  n_samples == 0 computes the mode only: eps, log_w and parts are then ignored.  beta, mu, v, parts
 * and n_failed may be NULL.  The samples are walked 64 at a time: device memory does not grow with n_samples, and sample
 * k's numbers are the same bits whatever n_samples is.  A pivot of H that is not positive and finite makes the unit's
 * stats[0 .. 4], mu, v and log_w NaN and is counted in *n_failed; a unit that ran out of iterations is no failure: it
 * reports converged = 0 and is scored where it stands.  D > 512 for any unit, parameters not set or a length without a
 * prior: VLGP_ERR_STATE (the message names D); max_iter < 1, tol not > 0, n_samples < 0, a null stats, or n_samples > 0
 * with a null eps or log_w: VLGP_ERR_ARG, the message naming the offender, nothing changed.  Waits for a pending M-step
 * and norms pass; changes no unit state, no parameter and nothing vlgp_hstep_prepare built.  Fixed-order sums, no atomics
 * on doubles: the same bits on every run. */
int vlgp_joint_laplace(vlgp_ctx* ctx, int set, int max_iter, double tol, int n_samples, const double* eps, double* beta,
                       double* stats, double* mu, double* v, double* log_w, double* parts, int* n_failed);
/* The joint Laplace posterior of vlgp_joint_laplace with the covariance of every row, also with entries held out
 * (DESIGN.md 4.14).  The model, the objective, the Newton iteration and its acceptance rule, beta (units, L, R), stats
 * (units, 8) and mu (rows, L) are vlgp_joint_laplace's; there are no draws.
 *   cov[t; l, l'] = G_l[t, :] (H^-1)_{l l'} G_l'[t, :]'   at the mode,
 * cov (rows, L (L + 1) / 2), the pair (l, l'), l' <= l, at l (l + 1) / 2 + l'; the pairs (l, l) are vlgp_joint_laplace's v.
 * Takes what vlgp_joint_laplace takes and a masked set of ONE replica (vlgp_replicate_masked with n_rep == 1); group
 * replicas and masked sets of several replicas are VLGP_ERR_STATE.  On a masked set a held-out entry (t, n)
 * contributes nothing: its term is left out of ll and of the sum of absolute terms, its res = cur = 0, so it is absent from
 * g, c, H and laplace, and what y holds there (NaN included) reaches no sum; with no bit set every output is the plain
 * set's, bit for bit, given the same start.  Start: a plain set as vlgp_joint_laplace; a masked set at beta = 0 (the
 * mean-field centres would read every y; the mode does not depend on the start, the count of factorisations does).
 * A unit with a pivot that is not positive and finite: stats[0 .. 4] NaN, its rows of mu and cov NaN, counted in *n_failed.
 * beta, mu, cov and n_failed may be NULL; a null stats, max_iter < 1 or tol not > 0: VLGP_ERR_ARG naming the argument;
 * D > 512: VLGP_ERR_STATE.  Waits and state as vlgp_joint_laplace: nothing changes.  Fixed-order sums, no atomics on
 * doubles: the same bits on every run. */
int vlgp_joint_posterior(vlgp_ctx* ctx, int set, int max_iter, double tol, double* beta, double* stats, double* mu,
                         double* cov, int* n_failed);
/* vlgp_joint_posterior with the window moments of the hyperparameter step of the Laplace EM, formed from
 * the factor of H while it is still on the device.  Everything vlgp_joint_posterior returns, this call returns bit for
 * bit.  For a unit of T rows the windows of `window` rows start at s = k window, k = 0 ... T / window - 1, and, when window
 * does not divide T, once more at s = T - window (it overlaps its neighbour); a unit shorter than the window has none.
 *   S[l] = sum over units and windows of  m[s : s + window] m[s : s + window]' + G_l[s : s + window, :] (H^-1)_ll G_l[s : s + window, :]'
 * with m = column l of mu: S (L, window, window), symmetric to the bit (the entries above the diagonal are copies of
 * their mirror images), the units added in unit order; *n_windows: the number of windows of the set.  y is not read by
 * the moments: a masked fit set is taken as vlgp_joint_posterior takes it.  A unit whose factorisation failed makes S NaN
 * and is counted in *n_failed.  Limits: 2 <= window <= 64 (VLGP_ERR_ARG), no prior factor of the set with a rank above 64
 * and at least one unit as long as the window (VLGP_ERR_STATE each); a null S or n_windows: VLGP_ERR_ARG; all of them
 * before anything is written.  Waits, state and the sets taken as vlgp_joint_posterior. */
int vlgp_joint_posterior_moments(vlgp_ctx* ctx, int set, int max_iter, double tol, double* beta, double* stats, double* mu,
                                 double* cov, int* n_failed, int window, double* S, int64_t* n_windows);
/* Posterior-predictive log density of every observation under the set's current posterior: where vlgp_loglik scores an
 * entry with the plug-in density p(y | E_q[rate]), this integrates the likelihood over the posterior of its linear
 * predictor,
 *   lpd[t, n] = log int p(y[t, n] | eta) N(eta; m, s2) d eta,   m = a_n.mu_t + (b x)_tn,   s2 = (a_n^2).v_t
 * (s2 = 0 when vb == 0).  The caller passes the quadrature nodes: with (x_q, w_q) the n_nodes-point Gauss-Hermite rule,
 *   z[q] = sqrt(2) x_q,   lwa[q] = log(w_q / sqrt(pi)) + x_q^2.
 *   Gaussian  lpd = -log(2 pi (noise_n + s2)) / 2 - (y - m)^2 / (2 (noise_n + s2));   rate = m
 *   Poisson   rate = trunc_exp(m + s2 / 2): vlgp_loglik's rate, and the predictive mean below the clamp of trunc_exp.
 *             s2 < 1e-30:  lpd = y log rate - rate - lgamma(y + 1), vlgp_loglik's expression (MAP fits, v == 0).
 *             Otherwise the rule is centred at the mode of the integrand g(e) = y e - ex(e) - (e - m)^2 / (2 s2),
 *             ex(e) = exp(min(e, 10)):
 *               e = min(log y, m + y s2) if y > ex(m), else e = m;
 *               eight times  e -= (y - ex(e) - (e - m) / s2) / (-ex(e) - 1 / s2);
 *               h = s2 ex(e) + 1,  tau = sqrt(s2) / sqrt(h),  eta_q = e + tau z[q],  c_q = min(eta_q, 10),
 *               t_q = lwa[q] + y c_q - exp(c_q) - (eta_q - m)^2 / (2 s2),
 *               lpd = -log(h) / 2 + logsumexp_q t_q - lgamma(y + 1).
 *             The start and the fixed count of Newton steps are part of the definition; the centre decides the accuracy of
 *             the rule, never its validity.  Against the exact integral the worst error over m in [-8, 5], sqrt(s2) in
 *             [0.02, 1], y in [0, 100] is 1.5e-6 at 12 nodes and 2e-8 at 20; far outside that regime the rule degrades
 *             (sqrt(s2) = 3, y = 0 at 12 nodes: 0.06 at m = 9; at m = 11 the eight steps no longer reach the mode and the
 *             error is several nats).  n_nodes == 1 is the Laplace approximation.
 * sums has vlgp_loglik's slots for every kind of set, slot 0 now holding sum lpd: Poisson {sum lpd, sum y, sum rate,
 * sum lgamma(y + 1)}, Gaussian {sum lpd, sum y, sum m, sum y^2}.  rate and lpd have vlgp_loglik's rate layout and may be
 * NULL; on a set made by vlgp_replicate_masked they are NaN where no replica holds the entry out, and asking for either when
 * two replicas hold the same entry out is VLGP_ERR_ARG.  n_nodes outside [1, 64] or a null z, lwa or sums: VLGP_ERR_ARG,
 * the message naming the offender, nothing changed.  Takes the sets vlgp_loglik takes.  Waits for a pending
 * M-step and norms pass; changes no unit state, no parameter and nothing vlgp_hstep_prepare built.  This handle's units
 * only; fixed-order sums, no atomics: the same bits on every run. */
int vlgp_predictive(vlgp_ctx* ctx, int set, int vb, int n_nodes, const double* z, const double* lwa, double* rate,
                    double* lpd, double* sums);
/* Calibration of the predictive distribution of vlgp_predictive: is the distribution the model reports the one the counts
 * follow?  Per entry, with m, s2 and rate as vlgp_predictive has them:
 *   Poisson   k = y;  p(j) = exp(lpd of the count j), exactly vlgp_predictive's value for y = j (the mode-centred n_nodes-point
 *             rule, or the plug-in Poisson mass when s2 < 1e-30);  lo = F(k - 1) = sum_{j < k} p(j), added in the order
 *             j = 0, 1, ... (0 at k = 0);  hi = lo + p(k);  then both are clipped to <= 1.
 *             mean = rate = trunc_exp(m + s2 / 2),  var = mean + mean^2 expm1(s2): the clamp of trunc_exp enters var only
 *             through mean.
 *             An entry with y negative, not an integer, not finite or > max_count is skipped: it adds 1 to `skipped` and
 *             nothing else, its cdf is NaN.  The device's loop over counts is bounded by max_count whatever memory holds.
 *   Gaussian  lo = hi = erfc(-(y - m) / sqrt(2 (noise_n + s2))) / 2;  mean = m,  var = noise_n + s2.
 * Per slot of vlgp_loglik (the same slots for every kind of set) sums holds W = n_bins + n_levels + 3 columns,
 *   pit_0 ... pit_{n_bins - 1} | covered_0 ... covered_{n_levels - 1} | pearson | entries | skipped:
 *   pit      the non-randomised PIT histogram (Czado, Gneiting & Held 2009) with edges e_j = j / n_bins: an entry with
 *            hi > lo adds clip((e_{j+1} - lo) / (hi - lo), 0, 1) - clip((e_j - lo) / (hi - lo), 0, 1) to bin j, one with
 *            hi == lo adds 1 to bin min(n_bins - 1, floor(lo n_bins)); every entry adds total mass 1.
 *   covered  entries inside the central interval of level c = levels[i]: hi >= a and lo < 1 - a, a = (1 - c) / 2; for counts
 *            exactly q_a <= y <= q_{1-a} with q_p = min{k : F(k) >= p}.
 *   pearson  sum (y - mean)^2 / var;  entries, skipped: counts.
 * cdf (entries, 2) = lo | hi in the per-entry layout of vlgp_predictive's rate, or NULL; on a set made by
 * vlgp_replicate_masked NaN where no replica holds the entry out, and asking for it when two replicas hold the same entry
 * out is VLGP_ERR_ARG (the sums alone are fine).  z, lwa: the node tables of vlgp_predictive.  Limits: 1 <= n_nodes <= 64,
 * 1 <= n_bins <= 32, 0 <= n_levels <= 4 with every level in (0, 1), 1 <= max_count <= 65536; outside them, or with a null
 * z, lwa or sums: VLGP_ERR_ARG, the message naming the argument, nothing changed.  The cost of an entry is 1 + y masses.
 * Takes the sets vlgp_loglik takes.  Waits for a pending M-step and norms pass; changes no unit state, no
 * parameter and nothing vlgp_hstep_prepare built.  This handle's units only; fixed-order sums, no atomics: the same bits on
 * every run. */
int vlgp_calibration(vlgp_ctx* ctx, int set, int vb, int n_nodes, const double* z, const double* lwa, int n_bins,
                     int n_levels, const double* levels, int max_count, double* cdf, double* sums);
/* vlgp_predictive and vlgp_calibration under a posterior of the latents the CALLER supplies, a mean and a full L x L
 * covariance per row (vlgp_joint_posterior's mu, cov; any other Gaussian will do): the siblings with vb = 1 and, for the
 * entry (t, n) scored under row `mrow` of the posterior's set (DESIGN.md 4.12's table: the row itself for a plain set,
 * replica k's copy of it, k rows + t, for group replicas and masked sets),
 *   m  = a_n . mu[mrow] + (b x)_tn                      the chain of vlgp_predictive's m
 *   q  = sum_l a_ln (sum_l' C[mrow; l, l'] a_l'n)       the inner sums first, each a chain of fused multiply-adds from 0
 *                                                       over l' = 0 ... L - 1; then the outer one over l = 0 ... L - 1
 *   s2 = max(0, q),   rate = trunc_exp(fma(1/2, s2, m)) Poisson, m Gaussian.
 * mu (rows of the posterior's set, L) and cov (the same rows, L (L + 1) / 2), the pair (l, l'), l' <= l, at
 * l (l + 1) / 2 + l' as vlgp_joint_posterior packs it, are host arrays; both are required (a null one: VLGP_ERR_ARG naming
 * it).  The calls are stateless: nothing is attached to the set and no set state changes; the set's own mu, v are not read.
 * Everything else is the sibling's: the node tables, slots, layouts, limits, the sets taken, the refusal of
 * per-entry output from overlapping masks, the s2 < 1e-30 plug-in branch, the waits, the fixed-order sums.
 * An entry whose m or q is not finite (the rows of a unit vlgp_joint_posterior failed on): vlgp_predictive_cov writes NaN
 * to its lpd and rate and lets the NaN into sums[., 0] and sums[., 2] (sum y and the fourth column stay); vlgp_calibration_cov
 * skips it as it skips a count it cannot score -- cdf NaN, 1 added to `skipped`, nothing else; no bin is computed from it. */
int vlgp_predictive_cov(vlgp_ctx* ctx, int set, int n_nodes, const double* z, const double* lwa, const double* mu,
                        const double* cov, double* rate, double* lpd, double* sums);
int vlgp_calibration_cov(vlgp_ctx* ctx, int set, int n_nodes, const double* z, const double* lwa, const double* mu,
                         const double* cov, int n_bins, int n_levels, const double* levels, int max_count, double* cdf,
                         double* sums);

/* Pair moments of the predictive distribution: do pairs of channels co-fluctuate more than the model
 * says?  For every row t scored under row `mrow` of the posterior's set (the table of DESIGN.md 4.12), with the Gaussian
 * posterior N(mu[mrow], C) of the latents -- C = diag(v[mrow]) (0 when vb == 0) for vlgp_pair_moments, the packed cov[mrow]
 * of vlgp_predictive_cov for the sibling -- and c[n, m] = a_n' C a_m:
 *   e_n = the rate of vlgp_predictive / vlgp_predictive_cov (Poisson trunc_exp(m_n + max(0, c[n, n]) / 2), Gaussian m_n)
 *   s_n = e_n Poisson, 1 Gaussian;   f = expm1 when both channels are Poisson, else the identity
 *   K[n, m] = s_n s_m f(c[n, m]);   K[n, n] += e_n Poisson, noise_n Gaussian;   d_n = y_tn - e_n
 *   resid[n, m] = sum_t live_tn live_tm d_n d_m,   model[n, m] = sum_t live_tn live_tm K[n, m]
 * resid, model: host arrays (N, N) for a plain set or a tiling cut, every entry live; (n_rep, N, N) for a set made by
 * vlgp_replicate_masked, an entry live where its replica holds it out (what y holds elsewhere is never read).  Both are
 * required and both come back symmetric to the bit.  Under a supplied posterior a row whose mu or cov holds a non-finite
 * value is dead for every channel: it adds nothing.  Refused (VLGP_ERR_STATE): a copied cut, and group replicas
 * ("replicate with held_out=: a pair needs both channels in one replica").  The calls only read: no set state changes.
 * The rows are summed in a fixed order without atomics: the same bits on every run. */
int vlgp_pair_moments(vlgp_ctx* ctx, int set, int vb, double* resid, double* model);
int vlgp_pair_moments_cov(vlgp_ctx* ctx, int set, const double* mu, const double* cov, double* resid, double* model);

/* Lag moments of the predictive distribution: does a channel's residual at row t still predict its
 * residual at row t + k once the latents are accounted for?  For every unit (a trial, or a window of a tiling cut) of the
 * set, latent l and lags k = 0 ... max_lag, under the mean-field posterior of the set's own mu, v:
 *   w_tl = sum over the entries n the posterior saw of a_ln^2 (rate_tn Poisson, 1 / noise_n Gaussian), vlgp_update_w's
 *          formula recomputed from mu, v (the stored w is not read)
 *   H_l = I + G_l' diag(w_.l) G_l = Lc Lc',  u_t = Lc^-1 G_l[t]',  c_l(t, s) = u_t . u_s,  q_n(t, s) = sum_l a_ln^2 c_l(t, s)
 *   e, s, d = y - e as vlgp_pair_moments has them;  f = expm1 Poisson, the identity Gaussian
 *   resid[k, n] = sum d_tn d_{t+k,n},  model[k, n] = sum s_tn s_{t+k,n} f(q_n(t, t + k)),  count[k, n] = the pairs summed,
 *   over the t with t + k in the same unit and both entries live;  model[0, n] += e_tn Poisson, noise_n Gaussian.
 * vb == 0: c == 0, so model[k >= 1] = 0.  resid, model, count: host arrays (max_lag + 1, N) for a plain set or a tiling
 * cut, where every entry is seen and live; (n_rep, max_lag + 1, N) for a set made by vlgp_replicate_masked, where an entry
 * is live where its replica holds it out and seen where it does not (what y holds at an entry that is not live is never
 * read).  A (unit, latent) whose H has a pivot that is not positive and finite is counted in *n_failed (may be NULL), and
 * its unit adds nothing to any sum.  Priors are bound as vlgp_elbo binds them.  0 <= max_lag <= 64, effective ranks
 * <= 64; the workspace of c takes n_rep rows (max_lag + 1) L doubles of device memory: beyond 4 GiB the call is refused
 * with the bytes it would need (VLGP_ERR_STATE).  Refused (VLGP_ERR_STATE): a copied cut, group replicas ("replicate
 * with held_out="), more than one rank.  The call only reads: no set state changes.  Fixed-order sums without atomics:
 * the same bits on every run. */
int vlgp_lag_moments(vlgp_ctx* ctx, int set, int vb, int max_lag, double* resid, double* model, double* count,
                     int* n_failed);

/* ---- parameters ------------------------------------------------------- */
int vlgp_set_params(vlgp_ctx* ctx, const double* a, const double* b, const double* noise);
/* Any pointer may be NULL.  da, db are the last M-step increments
 * (params["da"], params["db"], vlgp/core.py:201,219). */
int vlgp_get_params(vlgp_ctx* ctx, double* a, double* b, double* noise, double* da,
                    double* db);

/* ---- prior factor ----------------------------------------------------- */
/* gp.make_cholesky (vlgp/gp.py:150-162) + math.ichol_gauss (vlgp/math.py:76-126)
 * on the device: REPLACES the whole prior table with one factor per listed
 * length, G_l = ichol_gauss(T, omega_l, R) * sigma_l. */
int vlgp_build_prior(vlgp_ctx* ctx, int n_lengths, const int* lengths,
                     const double* omega, const double* sigma);
/* Inject a host-made factor G (L, T, R) for length T (adds/replaces one entry). */
int vlgp_set_prior(vlgp_ctx* ctx, int T, const double* G);
int vlgp_clear_prior(vlgp_ctx* ctx);
/* G (L, T, R) out; rank_out (L) = number of non-zero columns per latent (may be NULL). */
int vlgp_get_prior(vlgp_ctx* ctx, int T, double* G, int* rank_out);

/* ---- E-step ----------------------------------------------------------- */
/* core.update_w (vlgp/core.py:419-442).  This and vlgp_update_v take a masked fit set (vlgp_replicate_masked), no other
 * replicated set. */
int vlgp_update_w(vlgp_ctx* ctx, int set);
/* core.update_v (vlgp/core.py:445-471); vb == 0 is the reference's early
 * return for method != "VB". */
int vlgp_update_v(vlgp_ctx* ctx, int set, int vb, int* n_failed);
/* core.estep -> core.infer_single_trial (vlgp/core.py:22-126): n_iter inner
 * iterations for every unit of the set.  n_failed may be NULL (no sync then). */
int vlgp_estep(vlgp_ctx* ctx, int set, int n_iter, double dmu_bound, int vb,
               int* n_failed);
/* Wait for the launches of the most recent vlgp_estep call -- NOT for what has been queued behind them on the
 * same stream since (vlgp_hstep_prepare: the timers of core.vem bracket the E-step alone, vlgp/core.py:308-312). */
int vlgp_estep_wait(vlgp_ctx* ctx);

/* ---- M-step ----------------------------------------------------------- */
/* core.mstep (vlgp/core.py:129-249) over the concatenation of all units of
 * the set.  With a communicator attached the sufficient statistics are
 * all-reduced over ranks once per Newton iteration.  A masked fit set (vlgp_replicate_masked, one replica): every
 * channel over its observed rows only; see there for its limits.  Other replicated sets: VLGP_ERR_STATE. */
int vlgp_mstep(vlgp_ctx* ctx, int set, int n_iter, int use_hessian, double eps,
               double learning_rate, double da_bound, double db_bound, int* n_failed);

/* Asynchronous form: vlgp_mstep_begin enqueues the whole M-step on the handle's
 * second stream (after everything already queued) and returns; the H-step
 * objective, vlgp_build_prior, vlgp_norms may run meanwhile (they touch neither a, b
 * nor the rows the M-step reads for writing).  vlgp_mstep_end waits, reports the
 * failure count and the device time in ms.  Every other entry point that reads or
 * writes parameters or unit state joins a pending M-step first. */
int vlgp_mstep_begin(vlgp_ctx* ctx, int set, int n_iter, int use_hessian, double eps,
                     double learning_rate, double da_bound, double db_bound);
int vlgp_mstep_end(vlgp_ctx* ctx, int* n_failed, double* device_ms);

/* core.mstep under a full Gaussian posterior per row: the M-step of an EM whose E-step is the joint
 * Laplace posterior (vlgp_joint_posterior).  mu (rows, L) and cov (rows, L (L + 1) / 2), pair (l, l'), l' <= l, at
 * l (l + 1) / 2 + l' as vlgp_joint_posterior packs it, are host arrays over the rows of the set; they are uploaded once
 * and stay on the device for all n_iter Newton iterations.  The set's own mu and v are not read.  With q_tn = C_t a_n
 * and s2_tn = a_n . q_tn:
 *   eta = mu a + x b,   r = exp(min(eta + s2 / 2, 10)),   noise = var(y - eta) at the parameters entering the last iteration;
 *   Poisson channel:   grad_a = mu'y_n - sum_t r_tn (mu_t + q_tn),   nhess_a = sum_t r_tn [(mu_t + q_tn)(mu_t + q_tn)' + C_t],
 *                      grad_b, nhess_b, eps, learning_rate, da_bound, db_bound, da, db as vlgp_mstep;
 *   Gaussian channel:  vlgp_mstep's alternating least squares with mu'mu + sum_t C_t for mu'mu + diag(sum_t v_t).
 * A cov without off-diagonal entries gives vlgp_mstep on a set whose v is its diagonal, to rounding.
 * Takes plain sets and cuts; replicated and masked sets: VLGP_ERR_STATE.  L > 10, P > 8,
 * VLGP_MSTEP_GENERIC set or a communicator of more than one rank: VLGP_ERR_STATE with the reason.  A null mu or cov or
 * n_iter < 1: VLGP_ERR_ARG naming the argument.  A non-finite value in mu or cov (the rows of a unit whose Newton
 * iteration failed) is found by a first pass on the device: VLGP_ERR_ARG naming the first such row.  After any of these
 * no parameter has changed.  Waits for a pending M-step and norms pass and returns when the parameters are written;
 * *n_failed (may be NULL) counts the channels whose system was not positive definite.  Fixed-order sums, no atomics on
 * doubles: the same bits on every run. */
int vlgp_mstep_cov(vlgp_ctx* ctx, int set, const double* mu, const double* cov, int n_iter, int use_hessian,
                   double eps, double learning_rate, double da_bound, double db_bound, int* n_failed);
/* vlgp_mstep_cov of a masked fit set (vlgp_replicate_masked with one replica): every channel over the
 * rows where it is observed -- mu'y, x'y, every gradient and Hessian sum above with sum_t running over the observed rows
 * of channel n, and noise = the variance of y - eta over those rows.  mu, cov over the rows of the set (the source's
 * rows), as vlgp_joint_posterior on that set returns them; the set's own mu, v are not read.  What y holds at a missing
 * entry, NaN included, reaches no sum; with no bit set a, b, da, db are vlgp_mstep_cov's on the source set, bit for bit,
 * and noise is that of its two-pass form (VLGP_NOISE_PASSES).  A channel with no observed row keeps a, b, noise, steps by
 * 0 and is not counted in *n_failed, whatever eps is.
 * Takes a masked fit set only: a set without a mask is VLGP_ERR_STATE naming vlgp_mstep_cov, group replicas and masked
 * sets of several replicas are refused as replicated.  A Gaussian channel on the handle, L > 10, P > 8,
 * VLGP_MSTEP_GENERIC set or more than one rank: VLGP_ERR_STATE with the reason.  A null mu or cov or n_iter < 1:
 * VLGP_ERR_ARG naming the argument; a non-finite value in mu or cov: VLGP_ERR_ARG naming the first such row.  After any
 * of these no parameter has changed.  Everything else as vlgp_mstep_cov. */
int vlgp_mstep_cov_masked(vlgp_ctx* ctx, int set, const double* mu, const double* cov, int n_iter, int use_hessian,
                          double eps, double learning_rate, double da_bound, double db_bound, int* n_failed);

/* ---- H-step ----------------------------------------------------------- */
/* The objective scipy's L-BFGS-B minimises in gp.optimze1d (vlgp/gp.py:100-123):
 * construct_posterior_cov (gp.py:126-147) + elbo (gp.py:12-43), mask [0,1,0].
 * n_eval independent evaluations in one call: evaluation e uses latent
 * latent[e] and log-parameters logp[3e..3e+2] = log(sigma^2, omega, eps).
 * Outputs the UN-negated ll[e] and dll[3e..3e+2] summed over all units of the
 * set (and over ranks).  Every unit must have exactly `window` rows, window <= 1024 (4 ... 64: low-rank
 * or dense round kernels; 65 ... 128: workgroup-per-segment kernels; above: generic kernels, matrices in global memory)
 * (windows <= 50 -- 50 is the reference's default -- share a dedicated kernel). */
int vlgp_hstep_objective(vlgp_ctx* ctx, int set, int window, double dt, int n_eval,
                         const int* latent, const double* logp, double* ll,
                         double* dll);

/* Brackets the objective calls of one gp.optimize run (vlgp/gp.py:65-97), during
 * which the set's mu and w do not change: the per-latent second-moment matrices
 * sum_i mu_i mu_i' that the quadratic terms of every evaluation share are then built
 * once (by the first objective call) instead of on every call.  The caller must not
 * modify the set between begin and end.  Optional: without it every
 * vlgp_hstep_objective call is self-contained.  The H-step reads mu and w alone: all four calls take a masked fit set
 * (vlgp_replicate_masked) as any set. */
int vlgp_hstep_begin(vlgp_ctx* ctx, int set, int window);
int vlgp_hstep_end(vlgp_ctx* ctx);
/* Optional, before vlgp_hstep_begin: enqueue what the bracket builds from the units alone (those second moments and
 * the latent-major copy of w the round kernels read) right away -- core.vem runs the H-step after the E-step
 * (vlgp/core.py:320-327), and both are final once the E-step is done, so called there they are ready before the
 * first objective call instead of in front of its round.  Dropped if any entry point that may change the units runs
 * before vlgp_hstep_begin; a no-op for sets the round kernels do not take. */
int vlgp_hstep_prepare(vlgp_ctx* ctx, int set, int window);

/* ---- constraints / norms --------------------------------------------- */
/* mu <- (mu - shift) @ map for every unit (map (L, L) row-major, shift (L) or
 * NULL).  Covers core.constrain_loading (vlgp/core.py:392-416: map = s I, or
 * the SVD factor) and core.constrain_latent (vlgp/core.py:366-389).  This, the norms and vlgp_latent_moments below
 * read mu, v, dmu alone and take a masked fit set (vlgp_replicate_masked). */
int vlgp_apply_latent_map(vlgp_ctx* ctx, int set, const double* map, const double* shift);
/* out[0] = sum mu^2, out[1] = sum dmu^2 over the set (and over ranks):
 * the convergence test of core.vem (vlgp/core.py:300-305,350-354). */
int vlgp_norms(vlgp_ctx* ctx, int set, double out[2]);
/* The same in two halves: vlgp_norms_begin enqueues the sums (one kernel, results in mapped host memory) behind
 * everything already queued and returns; vlgp_norms_end waits for them.  core.vem takes the norms after the M- and
 * H-step (vlgp/core.py:350-354), but mu and dmu are final once the E-step (and constrain_latent) are done: begun
 * there -- even while the E-step still runs -- nothing is left to wait for at the end of the iteration.  Every entry
 * point that writes unit state waits for a pending pass first. */
int vlgp_norms_begin(vlgp_ctx* ctx, int set);
int vlgp_norms_end(vlgp_ctx* ctx, double out[2]);
/* Initial latents of preprocess.initialize (vlgp/preprocess.py:30-41) on the device: for every row of the
 * set mu = y . proj - shift, proj (N, L) row-major the posterior-mean map of the factor-analysis fit
 * (FactorAnalysis.transform: (y - mean) W'Psi^-1 (I + W Psi^-1 W')^-1), shift = mean . proj (L).
 * colsum (N, may be NULL) receives the column sums of y over THIS rank's rows (b = log mean y). */
int vlgp_project_units(vlgp_ctx* ctx, int set, const double* proj, const double* shift, double* colsum);
/* Column sums over the set (and ranks): sum1[l] = sum mu[:,l], sum2[l] = sum mu[:,l]^2,
 * *count = number of rows.  For core.constrain_latent. */
int vlgp_latent_moments(vlgp_ctx* ctx, int set, double* sum1, double* sum2, double* count);

/* ---- posterior draws --------------------------------------------------- */
/* api.sample_posterior (vlgp/api.py:142-168) for one trial of T bins: out (nsamples, T, L) row-major,
 * out[s, :, l] = mu[:, l] + G_l Lc^-T eps[l, :, s] with Lc Lc' = I + G_l' diag(w[:, l]) G_l -- a draw from
 * N(mu_l, (K_l^-1 + W_l)^-1), K_l = G_l G_l', without any T x T matrix.  Host arrays: mu, w (T, L);
 * G (L, T, R) = params["cholesky"][T]; eps (L, R, nsamples) standard normal draws (rows beyond a latent's
 * effective rank are ignored). */
int vlgp_sample_posterior(vlgp_ctx* ctx, int T, const double* mu, const double* w, const double* G,
                          int nsamples, const double* eps, double* out, int* n_failed);

/* ---- multi-GPU (RCCL over xGMI) --------------------------------------- */
/* Rank 0 makes the id, every rank passes the same id to vlgp_comm_init. */
int vlgp_comm_unique_id(char id[VLGP_UNIQUE_ID_BYTES]);
int vlgp_comm_init(vlgp_ctx* ctx, const char id[VLGP_UNIQUE_ID_BYTES], int rank, int world);
/* Second communicator (its own unique id) for the M-step lane, so that its
 * all-reduces may overlap the H-step's; without it a multi-rank M-step runs
 * its collectives un-overlapped on the first communicator's stream order. */
int vlgp_comm_init_aux(vlgp_ctx* ctx, const char id[VLGP_UNIQUE_ID_BYTES]);
/* 1 when the ranks share the host-side exchange segment for the H-step round sums (single node,
 * world > 1): the H-step then issues no RCCL collective, so the M-step lane may run concurrently with
 * it across ranks (its communicator is the only one in flight). */
int vlgp_comm_host_exchange(vlgp_ctx* ctx);
/* Transport behind the handle's all-reduces: 0 none (single rank), 1 RCCL, 2 host shared memory
 * (VLGP_COMM_TRANSPORT=shm, a test vehicle: several ranks on one GPU). */
int vlgp_comm_transport(vlgp_ctx* ctx);
/* Ranks RCCL itself reports (ncclCommCount) for the handle's two communicators -- main lane and M-step lane; 0 when no
 * RCCL communicator is attached (single rank, or the shared-memory test transport), -1 if the query failed. */
int vlgp_comm_rccl_ranks(vlgp_ctx* ctx, int* main_lane, int* m_lane);
/* In-place sum over ranks of n host doubles (staged through the device, on the
 * handle's stream, synchronous).  With no communicator attached it is a no-op.
 * n == 0 is a pure barrier. */
int vlgp_comm_allreduce_host(vlgp_ctx* ctx, double* buf, int n);

/* ---- measurement ------------------------------------------------------ */
/* HIP-event timing of the kernels an entry point launches, on the handle's
 * stream.  kind: 0 = E-step kernel, 1 = M-step statistics kernel,
 * 2 = H-step objective kernel, 3 = prior (ichol) kernel. */
#define VLGP_PROF_ESTEP 0
#define VLGP_PROF_MSTEP 1
#define VLGP_PROF_HSTEP 2
#define VLGP_PROF_PRIOR 3
/* the fast E-step kernel by instantiation (register-array size 16 / 24 / 32), the long-unit kernel and the
 * generic kernel; kind 0 reports the sum of all E-step kernels */
#define VLGP_PROF_ESTEP_RA16 4
#define VLGP_PROF_ESTEP_RA24 5
#define VLGP_PROF_ESTEP_RA32 6
#define VLGP_PROF_ESTEP_LONG 7
#define VLGP_PROF_ESTEP_GENERIC 8
#define VLGP_PROF_ESTEP_PASS 9     /* split E-step: one (T x N) pass over all rows (sampled: one sweep per call) */
#define VLGP_PROF_ESTEP_FACTOR 10  /* split E-step: factor + variance launch, units = (unit, latent) tasks */
#define VLGP_PROF_ESTEP_MEAN 11    /* split E-step: mean-update launch, units = (unit, latent) tasks */
#define VLGP_PROF_HSTEP_LR 12      /* H-step: the low-rank round kernel (hstep_round_lr), units = segment-evaluations;
                                    * kind 2 then counts only the dense round kernel */
#define VLGP_PROF_HSTEP_TAB 13     /* H-step: the tables kernel in front of a low-rank round, units = evaluations */
#define VLGP_PROF_KINDS 14
int vlgp_profile_enable(vlgp_ctx* ctx, int on);
int vlgp_profile_reset(vlgp_ctx* ctx);
/* launches, total milliseconds and work units recorded for `kind` since the last
 * reset.  Units: E-step = unit-sweeps (units x inner iterations), M-step = rows
 * streamed, H-step = segment-evaluations, prior = factors built. */
int vlgp_profile_get(vlgp_ctx* ctx, int kind, int64_t* launches, double* total_ms, double* units);
/* E-step phase anatomy: when enabled, thread 0 of every workgroup adds its
 * shader-clock cycles per phase into 8 counters (0 staging, 1 y.a pass + first
 * factor, 2 residual pass, 3 mean update, 4 curvature pass, 5 factor + variance).
 * `out` may be NULL; on != 0 also zeroes the counters. */
int vlgp_debug_phase_clock(vlgp_ctx* ctx, int on, uint64_t out[8]);
/* Element-wise probe of the device arithmetic the prior kernel relies on being bit-identical to the
 * reference's NumPy (vlgp/math.py:113-119): kind 0 out = exp(a) as np.exp computes it, 1 out = sqrt(a),
 * 2 out = a / b, 3 out = fma(a, b, out); and of the exponentials every Poisson rate goes through (csrc/fast_exp.h,
 * tables in LDS as the kernels hold them): 4 out = fast_exp(clamp10(a)), 5 fast_exp_tab<false>(clamp10(a)),
 * 6 trunc_exp_tab64(a), 7 fast_exp_tab256<false>(clamp10(a)), 8 trunc_exp_tab256(a).  Host arrays of n doubles; b is
 * read by kinds 2, 3 only and may be NULL otherwise. */
int vlgp_debug_npx(vlgp_ctx* ctx, int kind, int64_t n, const double* a, const double* b, double* out);
/* Which implementation ran the most recent vlgp_estep / vlgp_update_w / vlgp_update_v of this handle (the
 * reference has one serial loop, vlgp/core.py:123-126; the library picks a kernel family by set shape, and the
 * parity tests assert that the family they mean to check is the one that ran). */
#define VLGP_PATH_ESTEP_NONE 0
#define VLGP_PATH_ESTEP_SPLIT 1    /* chip-wide launches per phase (many short units) */
#define VLGP_PATH_ESTEP_FAST 2     /* persistent workgroup per unit, register-resident factors */
#define VLGP_PATH_ESTEP_LONG 3     /* long units (T > 64), one workgroup per trial */
#define VLGP_PATH_ESTEP_GENERIC 4  /* generic kernels (rank > 50 slots, L > 10, ...) */
#define VLGP_PATH_ESTEP_LSPLIT 5   /* long units as chip-wide launches: one workgroup per (unit, latent) task */
#define VLGP_PATH_ESTEP_SPLIT_MIXED 6 /* SPLIT whose per-latent launches carried lane-per-task and wave-per-task blocks in one grid */
int vlgp_debug_last_estep_path(vlgp_ctx* ctx, int* path);
/* Same for the most recent vlgp_hstep_objective call: which kernel family evaluated the per-segment terms. */
#define VLGP_PATH_HSTEP_NONE 0
#define VLGP_PATH_HSTEP_LOWRANK 1  /* exact low-rank (Woodbury) round, sixteen segments per workgroup (hstep_lr.h) */
#define VLGP_PATH_HSTEP_DENSE 2    /* one wave per segment, blocked elimination on the matrix pipe (hstep_mfma.h) */
#define VLGP_PATH_HSTEP_BIG 3      /* windows 65 ... 128: one workgroup per segment */
#define VLGP_PATH_HSTEP_GENERIC 4  /* generic kernels (any window; the reference's omega retry) */
#define VLGP_PATH_HSTEP_OLD 5      /* round-1 kernels behind their debug switches */
#define VLGP_PATH_HSTEP_MIXED 6    /* one round, two launches: low-rank kernel up to rank 32, dense kernel for the rougher evaluations */
int vlgp_debug_last_hstep_path(vlgp_ctx* ctx, int* path);
/* The library's debug / test switches (environment VLGP_*; DESIGN.md section 7 lists them, csrc/ctx.h holds the table)
 * have ONE lifetime: all of them are read when the handle is created and again by this call, and by nothing else -- no
 * launch reads the environment.  A test that sets or unsets one on a live handle calls this afterwards.  A malformed or
 * out-of-range value is reported on stderr and the switch keeps its default.  Nothing in production needs it. */
int vlgp_debug_reload_switches(vlgp_ctx* ctx);
/* The value the handle currently holds for the switch `name` ("VLGP_..."): a flag 0 / 1, a tri-state -1 (unset) / 0 / 1,
 * an integer or a real.  VLGP_ERR_ARG for a name the table does not hold. */
int vlgp_debug_switch(vlgp_ctx* ctx, const char* name, double* value);
/* What the library holds at this moment, over every handle of the process: out[0] device blocks, out[1] their bytes,
 * out[2] pinned / mapped host blocks, out[3] their bytes.  Every allocation of the library is counted (csrc/dev_mem.h),
 * so a test of lifetimes asserts equalities instead of watching the free memory of a shared card.  No handle needed. */
int vlgp_debug_live_memory(int64_t out[4]);
/* Counters of the H-step objective calls since the handle was created: out[0] evaluations that took the low-rank round,
 * out[1] the sum of their predicted ranks (even + odd block), out[2] evaluations that took the dense round,
 * out[3] low-rank rounds re-run densely because a rank exceeded the prediction. */
int vlgp_debug_hstep_stats(vlgp_ctx* ctx, double out[4]);
/* What the most recent vlgp_hstep_objective call on this handle launched, as launch_hstep_impl decided it: the values are
 * noted where the launcher settles them, nothing is computed for the report and no launch depends on it.  All slots are 0
 * before the first call; a call refused for its arguments leaves the report of the call before it.
 * out, VLGP_HSTEP_PLAN_LEN ints, at the slots VLGP_HP_*:
 *   PATH, VLGP_PATH_HSTEP_*;  RERUN, 1 when this is the dense round that repeated a low-rank round whose rank exceeded
 *   the host's prediction (out[3] of vlgp_debug_hstep_stats counts them);
 *   round kernels (paths LOWRANK, DENSE, MIXED): TC the compiled window (50, 64), NB the segment blocks per evaluation
 *   of the first launch, WLM 1 when the round read w latent-major;  LOWRANK and MIXED also: N_LR and N_ROUGH, the
 *   evaluations on the low-rank and on the dense kernel, RMAX the largest predicted rank, CLASS the register class the
 *   round was compiled for (16, 24, 28, 32), TABG 1 when the tables stayed in global memory, FUSED 1 when the workgroups
 *   factored the kernel blocks themselves (no tables launch), LDS the dynamic LDS of the low-rank launch in doubles,
 *   RCAP + e the columns evaluation e < 16 had room for (its predicted rank, at least 4; 0: a rough one);
 *   generic kernels (path GENERIC): NW waves per workgroup of the segment kernel, TM_GLOBAL 1 when the K block's
 *   matrices but the factor lay in global memory, HUGE 1 when the factor did too;  path BIG: the path only.
 * Slots a path does not use hold 0, except that a round whose K did not factor leaves its slots beside those of the
 * generic kernels that then ran. */
#define VLGP_HP_PATH 0
#define VLGP_HP_TC 1
#define VLGP_HP_N_LR 2
#define VLGP_HP_N_ROUGH 3
#define VLGP_HP_RMAX 4
#define VLGP_HP_CLASS 5
#define VLGP_HP_TABG 6
#define VLGP_HP_FUSED 7
#define VLGP_HP_NB 8
#define VLGP_HP_LDS 9
#define VLGP_HP_WLM 10
#define VLGP_HP_NW 11
#define VLGP_HP_TM_GLOBAL 12
#define VLGP_HP_HUGE 13
#define VLGP_HP_RERUN 14
#define VLGP_HP_RCAP 15            /* 16 slots */
#define VLGP_HSTEP_PLAN_LEN 31
int vlgp_debug_hstep_plan(vlgp_ctx* ctx, int out[VLGP_HSTEP_PLAN_LEN]);
/* What vlgp_mstep would launch on this handle for a set of `rows` rows (rows >= 1), computed by the functions the launches
 * themselves use; launches nothing, needs no set.  out[0] G, the workgroups along the rows (partial sums per statistic),
 * [1] rows per workgroup, [2] CT channels per tile, [3] S row slices per workgroup, [4] threads per workgroup, [5] channel
 * tiles; [6] LT, [7] PT, the compiled accumulator sizes (0, 0: the loop-based kernels take the set, and of the
 * geometry they use G and the rows per workgroup only); [8] 1 when the Newton accumulation of a set with x == 1 is the EXACT
 * instantiation; [9] FIXED (0: the general solve) and [10] ANYG of the single-rank sum + solve launch; [11] 1 when the noise
 * variance takes two passes over the rows, 0 when it comes from the moments.  G depends on the device's compute units and
 * on VLGP_MSTEP_WG_PER_CU: the shape tests assert through this that they reach the geometry they name. */
int vlgp_debug_mstep_plan(vlgp_ctx* ctx, int64_t rows, int out[12]);
/* What vlgp_estep (mode 1 | 2 | 4 | 8, or without the 8: vb off), vlgp_update_w (mode 4) or vlgp_update_v (mode 1 | 8) with
 * `n_iter` sweeps would launch for the resident set `set` on this handle: launch_estep itself runs its dispatch with every
 * kernel family deciding as it does before a launch, and reports instead of launching.  Binds the set's priors (they must
 * exist when the mode needs them); launches no E-step kernel, changes no unit state.  It reports ONE launch_estep call:
 * n_iter = 0, which vlgp_estep answers without a launch, is planned as if launched, and a set staged with
 * vlgp_set_overlaps (vlgp_estep runs launch_estep once per stage, each with its own lengths and cuts) is an error.
 * out, VLGP_ESTEP_PLAN_LEN ints, at the slots VLGP_EP_*:
 *   FAMILY, VLGP_PATH_ESTEP_*;  DECLINE, why the split E-step declined, VLGP_ESPLIT_* (0: it took the set);
 *   split families: LT, REC, MAXRA, USE_LANE, MIX, MAXRA_HI (maxra of the mixed or hi launch; 0: none), RTOP of the
 *   lane-per-task launch (13, 14; 0: none), LO_SHG (1 when the rank <= 16 launch shares G per workgroup), N_LANES,
 *   CUT ... CUT + n_lanes the cuts (unit indices), CS of the row passes, NJ of the y pass (4, 8; 0: the lane-per-row
 *   form; -1: no y pass in this mode), RANK + l the rank and CLASS + l the class (VLGP_ECLASS_*) of latent l < 16;
 *   fast: LT, RP, RA;   generic: LT, SMALL, RG;   long: the family only.
 * Slots a family does not use hold 0. */
#define VLGP_EP_FAMILY 0
#define VLGP_EP_DECLINE 1
#define VLGP_EP_LT 2
#define VLGP_EP_REC 3
#define VLGP_EP_MAXRA 4
#define VLGP_EP_USE_LANE 5
#define VLGP_EP_MIX 6
#define VLGP_EP_MAXRA_HI 7
#define VLGP_EP_RTOP 8
#define VLGP_EP_LO_SHG 9
#define VLGP_EP_N_LANES 10
#define VLGP_EP_CUT 11             /* n_lanes + 1 slots, at most 5 */
#define VLGP_EP_CS 16
#define VLGP_EP_NJ 17
#define VLGP_EP_RP 18
#define VLGP_EP_RA 19
#define VLGP_EP_SMALL 20
#define VLGP_EP_RG 21
#define VLGP_EP_RANK 22            /* 16 slots */
#define VLGP_EP_CLASS 38           /* 16 slots */
#define VLGP_ESTEP_PLAN_LEN 54
#define VLGP_ESPLIT_TAKEN 0
#define VLGP_ESPLIT_OFF 1          /* VLGP_ESTEP_SPLIT=0 */
#define VLGP_ESPLIT_GENERIC 2      /* VLGP_ESTEP_GENERIC */
#define VLGP_ESPLIT_L 3            /* L > 10 */
#define VLGP_ESPLIT_N 4            /* N > 1024 */
#define VLGP_ESPLIT_LSPLIT_OFF 5   /* long units, VLGP_ESTEP_LSPLIT=0 */
#define VLGP_ESPLIT_LONG_RANK 6    /* long units, prior rank above the long-unit split limit */
#define VLGP_ESPLIT_LONG_FEW 7     /* long units, fewer than 128 tasks */
#define VLGP_ESPLIT_SMALL_SET 8    /* short units: one generation of persistent workgroups */
#define VLGP_ESPLIT_RANK 9         /* short units at effective prior rank above 32 */
#define VLGP_ESPLIT_REC 10         /* channel records longer than 34 doubles */
#define VLGP_ECLASS_LANE 0         /* lane-per-task launch (estep_lane.h) */
#define VLGP_ECLASS_LO 1           /* wave-per-task, rank <= 16 (in a mixed launch: rides in the hi class) */
#define VLGP_ECLASS_HI 2           /* wave-per-task, rank > 16 */
int vlgp_debug_estep_plan(vlgp_ctx* ctx, int set, int mode, int n_iter, int out[VLGP_ESTEP_PLAN_LEN]);


/* ---- held-out evaluation: groups of channels --------------------------- */
/* Leave-group-out replicas (co-smoothing): as vlgp_replicate_units, but replica k leaves out the channels
 * channel[group_start[k] .. group_start[k+1]) -- vlgp_estep on `dst` runs for replica k what it would run on the units of
 * `src` with a[:, g] = 0 for every g of that group, bit for bit.  group_start has n_rep + 1 non-decreasing entries,
 * group_start[0] == 0; every group is non-empty, its channels distinct and in [0, N) (two replicas may share a channel):
 * otherwise VLGP_ERR_ARG, the message naming the replica, and nothing is changed.  src, dst, aliasing, lifetime and the
 * entry points that accept the set are those of vlgp_replicate_units.  vlgp_loglik scores the set per (replica, channel)
 * pair, n_pairs = group_start[n_rep], in the order of channel[]. */
int vlgp_replicate_groups(vlgp_ctx* ctx, int src, int dst, int n_rep, const int* group_start, const int* channel);

#ifdef __cplusplus
}
#endif
#endif /* VLGP_HIP_H */
