"""The case table of tests/test_joint_shapes_host.py and tests/test_gpu_joint_shapes.py: unit sets whose prior factors have
EXACT ranks, chosen so that every size csrc/joint.hip treats differently is crossed by one case.  Not a test file.

Factors.  oracle.ichol_gauss(T, omega, R) at a rough omega (0.5 ... 3) fills all min(T, R) columns; every column from r on
is then zeroed.  The NumPy statement (joint_numpy.Unit, through forecast_numpy.rank) and the device (prior_rank_kernel
behind vlgp_set_prior) both take the last non-zero column for the rank, so both see rank r, and a row of a cut factor
keeps its norm <= 1.  Every unit of a set has its own length, hence its own factors and its own rank pattern: one engine
call runs several D, and Dmax != D for all units but one.

What each case is the only one to reach (the loops are those of csrc/joint.hip):
  D_255_to_288        joint_factor's `ii += 256` second pass (ld = D + 1 > 256); at D = 256 the row of that second pass is
                      the gradient row alone; D = 255 is the largest single pass; D = 288 = 9 panels of JT_NB, no ragged one;
                      joint_assemble at i0 = 60 and j0 = 60 (rank 64 against 64, 63 and 1); joint_init at rs = 65.
  D_511_512_33        joint_factor's third pass (ld = 513 = 2 * 256 + 1: the gradient row again alone in it); the panel's
                      LDS request of 513 * 33 + 32 doubles = 135 688 bytes; every lane of joint_var / joint_cov / joint_draw
                      live in every latent; D = 33 beside Dmax = 512 (a buffer stride of Dmax + 1, a row stride of D + 1).
  LR_512_small_D      L R = 512 (as in every case at R = 64, L = 8): the `e += 256` loops of joint_decide and joint_stats make
                      a second pass; here alone with D <= 45, so that it walks four latents of a few weights each and the
                      zero padding of beta and dvec between them.
  rows_256_257_600    the `t += 256` loops of joint_decide and joint_stats: one pass exactly (256), one row into the second
                      (257), a third (600); N = 70, so a masked set of it has two mask words per row.  joint_stats' sum is
                      the reported ll.  joint_decide's only judges trial points, and at this case (as at every case with
                      counts drawn from the model) the first 256 rows alone judge every one of them alike:
  late_rows_300       joint_decide's `t += 256` second pass where it decides: the rows from 256 on carry counts near 30
                      against a model at 0.7, and the iteration judged by the first 256 rows alone (DecideOnFirstRows)
                      rejects a step the whole sum takes and does not converge (tests/test_joint_shapes_host.py).
  L16_npair_136       npair = 136 blocks of joint_assemble per unit, the packed c and cov at 136 per row.
  L11_D_512           L = 11, the latent count of the D = 550 refusal of tests/test_gpu_joint.py, at [50] * 10 + [12]: D = 512
                      from ranks of 50, R = 50.
  panel_32_64_224     D an exact multiple of JT_NB below 256: one panel, two, seven, none of them ragged.
  halving             a start far from the mode (mu = 3 N(0, 1), rates near 100) from which the NumPy iteration rejects a
                      full step in both units.
"""
import functools

import numpy as np

import joint_cov_numpy as JC
import joint_numpy as JN
from oracle import vlgp_oracle as O

K_DRAWS = 3


def _case(R, L, N, units, seed, n_gauss=0, start=0.3, loading=0.3, rate=0.7, omega=None, late=None):
    """omega: per latent (default: rough, omega(L)); late: the mean of the Poisson counts of rows 256 on (default: the model's)."""
    return {"R": R, "L": L, "N": N, "units": units, "seed": seed, "n_gauss": n_gauss, "start": start, "loading": loading,
            "rate": rate, "omega": omega, "late": late}


CASES = {
    # units: (length, ranks per latent)
    "D_255_to_288": _case(64, 8, 8, [(70, [64, 63, 1, 64, 31, 30, 1, 1]), (80, [64, 64, 64, 60, 1, 1, 1, 1]),
                                     (90, [64, 64, 64, 61, 1, 1, 1, 1]), (100, [64, 64, 64, 64, 8, 8, 8, 8])], seed=21,
                          n_gauss=2),
    "D_511_512_33": _case(64, 8, 8, [(65, [64] * 7 + [63]), (130, [64] * 8), (64, [26, 1, 1, 1, 1, 1, 1, 1])], seed=22),
    "LR_512_small_D": _case(64, 8, 6, [(20, [1, 2, 3, 4, 5, 6, 7, 8]), (45, [9, 1, 8, 2, 7, 3, 6, 9])], seed=23),
    "rows_256_257_600": _case(16, 3, 70, [(256, [16, 9, 1]), (257, [16, 16, 16]), (600, [5, 16, 12])], seed=24, n_gauss=20),
    "L16_npair_136": _case(50, 16, 8, [(60, [1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6, 5, 4, 3, 2]),
                                       (33, [9, 9, 1, 1, 5, 5, 2, 2, 7, 7, 3, 3, 8, 8, 4, 4])], seed=25),
    "L11_D_512": _case(50, 11, 8, [(130, [50] * 10 + [12]), (55, [40] * 10 + [1])], seed=26),
    "panel_32_64_224": _case(64, 4, 5, [(70, [8, 8, 8, 8]), (66, [61, 1, 1, 1]), (100, [64, 64, 64, 32])], seed=27),
    # (smooth factors, so that 16 columns reach the last rows, and counts near 30 in rows 256 on, where the model has 0.7;
    # the seed chosen on the CPU, among those that separate the whole sum from the first 256 rows, for the smallest lambda_max(H))
    "late_rows_300": _case(16, 2, 8, [(300, [16, 7]), (257, [9, 16])], seed=52, omega=[0.8e-3, 1.5e-3], late=30.0),
    # (seed, loading and rate chosen on the CPU so that both units reject one full step and converge within 13 factorisations)
    "halving": _case(50, 2, 8, [(50, [21, 50]), (30, [30, 9])], seed=29, start=3.0, loading=0.1, rate=100.0),
}
MASKED = ("D_511_512_33", "rows_256_257_600")


def dims(name):
    """D of every unit of the case, from the table."""
    return [sum(r) for _, r in CASES[name]["units"]]


def omega(L):
    return np.linspace(0.5, 3.0, L) if L > 1 else np.array([1.0])


def factor(T, om, R, r):
    """(T, R): oracle.ichol_gauss's factor with every column from r on zeroed."""
    G = O.ichol_gauss(T, om, R)
    G[:, r:] = 0.0
    return G


@functools.lru_cache(maxsize=None)
def problem(name):
    """(units, params, gauss) of a case, as tests/test_gpu_marginal._engine takes them: Poisson counts (and n_gauss Gaussian
    channels, the last ones) drawn from the model under the cut factors, a random mean-field posterior (mu, v, w) to
    start from, and params["cholesky"] = {T: (L, T, R)}.  The loadings shrink with L and N so that lambda(H) stays of the
    order of those of tests/test_gpu_joint.py."""
    c = CASES[name]
    R, L, N = c["R"], c["L"], c["N"]
    rng = np.random.default_rng(c["seed"])
    gauss = np.zeros(N, bool)
    if c["n_gauss"]:
        gauss[N - c["n_gauss"]:] = True
    a = c["loading"] * rng.standard_normal((L, N)) * min(1.0, 5.0 / L) * min(1.0, np.sqrt(8.0 / N))
    b = np.log(c["rate"]) + 0.3 * rng.standard_normal((1, N))
    noise = np.where(gauss, 0.5 + rng.random(N), 1.0)
    om = omega(L) if c["omega"] is None else np.asarray(c["omega"], float)
    prior, units = {}, []
    for T, ranks in c["units"]:
        assert T not in prior and len(ranks) == L and all(1 <= r <= min(T, R) for r in ranks), (name, T, ranks)
        prior[T] = np.stack([factor(T, om[l], R, r) for l, r in enumerate(ranks)])
        lat = np.stack([prior[T][l] @ rng.standard_normal(R) for l in range(L)], axis=1)
        eta = lat @ a + b
        y = np.where(gauss, eta + np.sqrt(noise) * rng.standard_normal((T, N)), rng.poisson(np.exp(eta)).astype(float))
        if c["late"] is not None:
            y[256:] = rng.poisson(c["late"], y[256:].shape)
        units.append({"y": y, "x": None, "mu": c["start"] * rng.standard_normal((T, L)), "v": 0.05 * rng.random((T, L)),
                      "w": rng.uniform(0.05, 2.0, (T, L))})
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": R, "a": a, "b": b, "noise": noise, "cholesky": prior}
    return units, params, gauss


def draws(name):
    """(units, L, R, K_DRAWS) standard normals."""
    c = CASES[name]
    return np.random.default_rng(c["seed"] + 100).standard_normal((len(c["units"]), c["L"], c["R"], K_DRAWS))


def _args(params, gauss):
    return params["a"], params["b"], params["noise"], gauss, params["cholesky"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The statement of the plain set, computed once and shared: joint_cov_numpy.statement's per-unit dicts (which are
    joint_numpy.statement's plus cov), with the draws of joint_numpy.draws on draws(name) (log_w, ll_k, c_k, scale_k) and
    ``halvings``, the number of trial points the unit's iteration rejected."""
    units, params, gauss = problem(name)
    calls, plain_f = [], JN.Unit.f

    def counted(self, beta):
        calls.append(id(self))
        return plain_f(self, beta)

    JN.Unit.f = counted
    try:
        st = JC.statement(units, *_args(params, gauss))
    finally:
        JN.Unit.f = plain_f
    eps = draws(name)
    for i, s in enumerate(st):
        # newton: per factorisation that is not the last, f once at beta and once per trial point; one trial is accepted
        s["halvings"] = calls.count(id(s["unit"])) - 2 * (s["n_newton"] - 1) if s["converged"] else -1
        s["log_w"], s["ll_k"], s["c_k"], s["scale_k"], _ = JN.draws(s["unit"], s["beta"], s["Lc"], eps[i])
    return st


class DecideOnFirstRows:
    """A unit whose f and sum of absolute terms leave out the rows from `rows` on while its gradient and Hessian are whole:
    what joint_decide would judge a trial point by if its `t += 256` loop made one pass.  For joint_numpy.newton."""

    def __init__(self, U, rows=256):
        self.U, self.rows, self.grad, self.hessian = U, rows, U.grad, U.hessian

    def _terms(self, beta):
        return self.U.terms(self.U.paths(beta))[0][:self.rows]

    def f(self, beta):
        return 0.5 * float(beta @ beta) - float(self._terms(beta).sum())

    def abs_terms(self, beta):
        return float(np.abs(self._terms(beta)).sum() + 0.5 * beta @ beta)


def mask(name):
    """The "random" mask of tests/test_gpu_joint_cov.py over the rows of the case: bool (rows, N), a fifth of it set."""
    rows = sum(T for T, _ in CASES[name]["units"])
    return np.random.default_rng(3).random((rows, CASES[name]["N"])) < 0.2


@functools.lru_cache(maxsize=None)
def masked_reference(name):
    """The statement of the set without the entries of mask(name), started at beta = 0."""
    units, params, gauss = problem(name)
    return JC.statement(units, *_args(params, gauss), held=mask(name))
