"""The cases of tests/test_gpu_lag.py and of the conditioning test of tests/test_lag_host.py: the smallest shapes at which
the kernels of csrc/lags.hip can still go wrong.  Not a test file.

What the shapes cross: unit lengths 1, 2, K, K + 1, 63, 64, 65, 127-129 and ragged mixes (lag_task's tiles of 64 rows and
their halo of K rows; lags longer than some units of a set but not others); max_lag 0, 1, 31, 32, 63, 64 (the groups of 8
lags and the partial last group); effective ranks 1, mid and 64 from prior factors cut to exact ranks
(joint_shapes.factor); L in {1, 2, 5, 8, 9, 10} (lag_rows' eight latents at a time); N in {1, 63, 64, 65, 129, 130}
(channel tiles, two and three mask words); Gaussian channels interleaved, with and without regressors; row counts around
the 128 rows a wave takes of a small set (LAG_MIN_CHUNK: test_lag_host.py holds the layout to that), with units that
straddle the chunks; masked sets of several replicas with speckled and whole-channel masks, a replica that holds nothing
out and a channel that no replica holds out.

A case: lengths, N, L, P, K, R, ranks (cycled over the latents, clipped to min(T, R)), and for a masked set its kind and
number of replicas."""
import functools

import numpy as np

import joint_shapes as JS
import lag_numpy as LN

CASES = {
    #  name          lengths                      N    L   P  K   R   ranks          masked
    "one":          ((1, 2, 5),                   1,   1,  1, 1,  4,  (3,),          None),
    "lag0":         ((1, 2, 63, 64, 65),          63,  2,  1, 0,  10, (1, 7),        None),
    "lag1":         ((1, 2, 3, 64, 65),           64,  2,  2, 1,  10, (10, 1),       None),
    "lag31":        ((31, 32, 33, 1, 127),        65,  5,  1, 31, 64, (1, 20, 64),   None),
    "lag32":        ((32, 33, 128, 2),            129, 8,  2, 32, 24, (24, 5, 1),    None),
    "lag63":        ((63, 64, 65, 129, 5),        130, 9,  1, 63, 64, (64, 33, 2),   None),
    "lag64":        ((64, 65, 128, 129, 1, 2),    65,  10, 1, 64, 64, (64, 1, 40),   None),
    "chunks":       ((100, 29, 127, 1, 130),      100, 5,  1, 20, 30, (30, 12, 17),  None),
    "speckled":     ((100, 60),                   130, 5,  2, 20, 20, (20, 9),       ("speckled", 3)),
    "folds":        ((40, 50, 33),                65,  3,  1, 8,  12, (12, 6),       ("folds", 2)),
    "folds_words":  ((65, 7),                     129, 2,  1, 64, 16, (16,),         ("folds", 3)),
}
PLAIN = [k for k, c in CASES.items() if c[-1] is None]
MASKED = [k for k, c in CASES.items() if c[-1] is not None]


@functools.lru_cache(maxsize=None)
def problem(name):
    """``(units, par, prior, R)``: units with a random posterior (y, x or None, mu, v, w), the parameters with alternating
    likelihoods, and the prior factor (L, T, R) of every length at its exact ranks."""
    lengths, N, L, P, K, R, ranks, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    gauss = (np.arange(N) % 2 == 1)
    a = 0.3 * rng.standard_normal((L, N)) * (5.0 / L if L > 5 else 1.0)
    b = np.concatenate([np.where(gauss, 0.5, 0.3)[None] + 0.2 * rng.standard_normal((1, N)), -0.05 * rng.random((P - 1, N))])
    noise = np.where(gauss, 0.5 + rng.random(N), 1.0)
    # timescales from one bin to seven: the first latent's factor reaches any rank asked of it, the smooth ones stop at
    # their own and couple rows many lags apart
    om = np.geomspace(2.0, 0.02, L) if L > 1 else np.array([0.3])
    prior = {T: np.stack([JS.factor(T, om[l], R, min(ranks[l % len(ranks)], T, R)) for l in range(L)])
             for T in sorted(set(lengths))}
    units = []
    for T in lengths:
        x = None if P == 1 else np.concatenate([np.ones((T, 1, N)), rng.poisson(0.5, (T, P - 1, N)).astype(float)], axis=1)
        mu = 0.4 * rng.standard_normal((T, L))
        eta = mu @ a + (b[0] if x is None else np.einsum("tpn,pn->tn", x, b))
        y = np.where(gauss, eta + rng.standard_normal((T, N)), rng.poisson(np.exp(eta)).astype(float))
        units.append({"y": y, "x": x, "mu": mu, "v": 0.02 + 0.2 * rng.random((T, L)), "w": rng.uniform(0.05, 2.0, (T, L))})
    return units, dict(a=a, b=b, noise=noise, gauss=gauss), prior, R


def masks(name):
    """(n_rep, rows, N) bool: what each replica holds out.  folds: replica k the channels n % (n_rep + 1) == k, so the
    channels n % (n_rep + 1) == n_rep are held out by nobody; speckled: 40 % of the entries, the last replica none."""
    lengths, N = CASES[name][0], CASES[name][1]
    kind, n_rep = CASES[name][-1]
    rows = sum(lengths)
    held = np.zeros((n_rep, rows, N), dtype=bool)
    if kind == "folds":
        for k in range(n_rep):
            held[k][:, k::n_rep + 1] = True
    else:
        held = np.random.default_rng(5).random((n_rep, rows, N)) < 0.4
        held[n_rep - 1] = False
    return held


def per_unit(arr, lengths):
    at = np.cumsum([0] + list(lengths))
    return [arr[at[i]:at[i + 1]] for i in range(len(lengths))]


def with_posterior(units, mu, v):
    """The units with the rows of ``mu, v`` (concatenated) in place of their own."""
    lengths = [u["y"].shape[0] for u in units]
    return [dict(u, mu=m, v=s) for u, m, s in zip(units, per_unit(mu, lengths), per_unit(v, lengths))]


@functools.lru_cache(maxsize=None)
def statement(name, vb=True):
    """The plain case's ``(resid, model, count, n_failed)`` by tests/lag_numpy.py, computed once."""
    units, par, prior, _ = problem(name)
    return LN.lag_moments(units, par, prior, CASES[name][4], vb=vb)
