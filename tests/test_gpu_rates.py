"""The Poisson rates on the device, element by element.

1. The device build of csrc/fast_exp.h through probe kinds 4 ... 8 of vlgp_debug_npx: the designed sample, clamp,
   special-value and monotonicity checks of tests/test_fast_exp.py with the same bounds (the header's: 2 / 1.5 ulp),
   and the device's bits against the CPU build's.
2. The copies of those functions the compiler inlined into the real kernels: one Poisson channel with a = 1, b = 0,
   x = 1, v = 0 makes the curvature w[t, 0] = rate(mu[t, 0]) exactly (oracle.curvature_unit), so vlgp_update_w returns
   the rate of every kernel family element by element; each case ASSERTS the family that ran.  Bounds: 2 ulp for the
   fast_exp families (fast, long), 1.5 ulp for the split row passes (split, long_split), 2 ulp for the families on the
   device library's exp (generic, vlgp_loglik) -- they must not be looser than the hand-written ones.  (The split
   passes form w from a^2 / 2: exact with the loading 2, one more rounding below 2^-1021 with the loading 1 -- see
   SPLIT_LOADING.)  Measured on an MI355X: fast 0.8082, long 0.8082, generic 0.8132, loglik 0.8132, split and
   long_split 1.2777 ulp (loading 1: 1.2678 where rate / 2 is normal, 2.2777 below); the probe's bits equal the CPU's.
3. The M-step judged per channel (each column against its own size, not the array's largest entry) over rates from
   e^-5 to e^9.5, and the all-Poisson noise of channels whose residual is constant.

Special values (NaN, +-inf) differ between the functions; the three-way table is in tests/test_fast_exp.py.
Known edge, not changed here: `y log(rate)` in csrc/evaluate.hip is NaN for y = 0 once eta < -745.13 (the rate
underflows to 0); no fit reaches that, and the tests below read the rates, not the log-likelihood sums, there.
"""
import ctypes as C

import numpy as np
import pytest

import test_fast_exp as F
from oracle import vlgp_oracle as O

gpu = pytest.mark.gpu  # per test: the conditioning check of the M-step case below runs without a GPU

STAGE = 1e-9  # the project's stage tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def V():
    import vlgp_amd

    return vlgp_amd


@pytest.fixture(scope="module")
def fx():
    return F.Harness()


@pytest.fixture(scope="module")
def probe(V):
    from vlgp_amd._lib import dptr

    eng = V.Engine(4, 2, 1, 50)

    def f(kind, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros_like(x)
        eng._ck(eng.lib.vlgp_debug_npx(eng.h, int(kind), C.c_int64(x.size), dptr(x), None, dptr(out)))
        return out

    yield f
    eng.close()


# ------------------------------------------------------------------ 1. the header as compiled for the device
@gpu
def test_probe_rejects_unknown_kinds(V):
    from vlgp_amd._lib import dptr

    x, out = np.zeros(4), np.zeros(4)
    with V.Engine(4, 2, 1, 50) as eng:
        for kind in (-1, 9):
            with pytest.raises(V.VlgpError):
                eng._ck(eng.lib.vlgp_debug_npx(eng.h, kind, C.c_int64(4), dptr(x), None, dptr(out)))
        for kind in (2, 3):  # these read b
            with pytest.raises(V.VlgpError):
                eng._ck(eng.lib.vlgp_debug_npx(eng.h, kind, C.c_int64(4), dptr(x), None, dptr(out)))


@gpu
def test_device_accuracy_on_the_designed_sample(probe):
    F.check_accuracy(probe)


@gpu
def test_device_clamps(probe):
    F.check_clamp(probe)


@gpu
def test_device_special_values_are_pinned(probe):
    F.check_special(probe)


@gpu
def test_device_monotone_across_every_cell_boundary(probe):
    F.check_monotone(probe)


@gpu
def test_device_bits_equal_the_cpu_build(probe, fx):
    """Every operation of the header is a correctly rounded fma, add, multiply, rint or ldexp: the device build and the
    g++ build give the same bits on the designed sample, the subnormal range, the clamp and the special values."""
    x = np.concatenate([F.designed_sample(), F.denormal_sample(), F.monotone_grid()[::40],
                        np.array([10.0, np.nextafter(10.0, 11.0), 11.0, 700.0, 1e300, -745.0, -746.0, -1e4, -1e300,
                                  np.nan, np.inf, -np.inf])])
    differing = {}
    for kind in F.KINDS:
        d, c = probe(kind, x), fx(kind, x)
        ne = ~((F.bits(d) == F.bits(c)) | (np.isnan(d) & np.isnan(c)))
        if ne.any():
            differing[F.KINDS[kind]] = (int(ne.sum()), x[ne][:8].tolist())
    assert not differing, "device and CPU bits differ (count, first inputs): %r of %d elements" % (differing, x.size)


# ------------------------------------------------------------------ 2. the rates inside the real kernels
def kernel_sample():
    """The designed sample (finite), the subnormal range and the clamp's inputs."""
    return np.concatenate([F.designed_sample(), F.denormal_sample(),
                           np.array([10.0, np.nextafter(10.0, 11.0), 11.0, 700.0, 1e300])])


@pytest.fixture(scope="module")
def kref():
    return F.Reference(kernel_sample())


def _as_units(values, T, L=1):
    """`values` as column 0 of the mu of units of T bins (the last unit padded with zeros); other latents 0."""
    n_units = -(-values.size // T)
    col = np.zeros(n_units * T)
    col[:values.size] = values
    mu = np.zeros((n_units * T, L))
    mu[:, 0] = col
    return [{"y": np.zeros((T, 1)), "mu": mu[m * T:(m + 1) * T].copy()} for m in range(n_units)]


def _rates_via_update_w(V, values, T, L, want_path, chunk_units=None, want_loglik=False, loading=1.0):
    """w[:, 0] / loading^2 of vlgp_update_w (and the rate of vlgp_loglik) for one Poisson channel with a[0] = loading (a
    power of two: mu = values / loading, eta = mu a and the division of w are exact), the other loadings 0, b = 0,
    x = 1, v = 0; the kernel family of every call asserted."""
    units = _as_units(values / loading, T, L)
    chunk_units = chunk_units or len(units)
    a = np.zeros((L, 1))
    a[0, 0] = loading
    w, rate = [], []
    with V.Engine(1, L, 1, 50) as eng:
        eng.set_params(a, np.zeros((1, 1)), np.ones(1))
        for lo in range(0, len(units), chunk_units):
            part = units[lo:lo + chunk_units]
            eng.upload(0, part)
            eng.update_w(0)
            assert eng.last_estep_path == want_path, (eng.last_estep_path, want_path, len(part), T, L)
            got = eng.download(0, keys=("w",))["w"]
            assert not got[:, 1:].any()  # rate * 0^2
            w.append(got[:, 0].copy())
            if want_loglik:
                rate.append(eng.loglik(0, vb=True, want_rate=True)[1][:, 0].copy())
    w = np.concatenate(w)[:values.size] / loading ** 2
    return (w, np.concatenate(rate)[:values.size]) if want_loglik else w


def _assert_within(kref, got, bound, what):
    err, at = F.worst(kref, got)
    print("%-36s %.4f ulp at eta = %r (bound %.1f)" % (what, err, at, bound))
    assert err < bound, (what, err, at)


# The split row passes keep a^2 / 2 in their channel records (the exponent is one chain b + mu.a + v.(a^2 / 2)) and
# store w = 2 (sum rate a^2 / 2).  With a = 1 the product rate / 2 is subnormal for rate < 2^-1021 and is rounded to the
# 2^-1074 grid once more: w is then NOT the rate exactly, it carries up to one more unit of 2^-1074 (measured 2.2777 ulp
# at eta = -707.7344, where the exponential itself is 1.2777 ulp off -- same bits as the probe).  That is arithmetic of
# the sum, not of the exponential, and 4e-308 in absolute terms.  So the split families are held to the header's
# 1.5 ulp on EVERY element with the loading 2 (rate * 2 and the division by 4 are exact; mu = eta / 2: the same eta
# reaches the exponential), and with the loading 1 to 1.5 ulp wherever rate / 2 is normal and to 1.5 + 1 below.
SPLIT_LOADING = 2.0


def _assert_split_family(V, kref, T, L, want_path, what, chunk_units=None):
    w = _rates_via_update_w(V, kref.x, T, L, want_path, chunk_units=chunk_units, loading=SPLIT_LOADING)
    _assert_within(kref, w, 1.5, what + ", a = 2")
    w1 = _rates_via_update_w(V, kref.x, T, L, want_path, chunk_units=chunk_units)
    err = kref.ulp_error(w1)
    low = kref.rounded < 2.0 ** -1021
    assert low.sum() > 1000 and (~low).sum() > 60000
    print("%-36s %.4f ulp where rate / 2 is normal, %.4f below" % (what + ", a = 1", err[~low].max(), err[low].max()))
    assert err[~low].max() < 1.5, (what, err[~low].max())
    assert err[low].max() < 1.5 + 1.0, (what, err[low].max())


@gpu
def test_rates_of_the_fast_kernel_and_loglik(V, kref, monkeypatch):
    """estep_fast_kernel (fast_exp behind clamp10): sets below the split E-step's size rule, 250 units of 64 bins per
    call.  vlgp_loglik's plug-in rate (the device library's exp) on the same sets: 2 ulp as well."""
    monkeypatch.delenv("VLGP_ESTEP_SPLIT", raising=False)
    w, rate = _rates_via_update_w(V, kref.x, 64, 1, "fast", chunk_units=250, want_loglik=True)
    _assert_within(kref, w, 2.0, "fast (estep_fast_kernel)")
    _assert_within(kref, rate, 2.0, "vlgp_loglik rate")


@gpu
def test_rates_of_the_fast_kernel_five_latents(V, kref, monkeypatch):
    monkeypatch.delenv("VLGP_ESTEP_SPLIT", raising=False)
    w = _rates_via_update_w(V, kref.x, 50, 5, "fast", chunk_units=300)
    _assert_within(kref, w, 2.0, "fast, L = 5")


@gpu
def test_rates_of_the_generic_kernel(V, kref):
    """More than sixteen latents: estep_kernel, on the device library's exp.  Held to 2 ulp like the hand-written ones."""
    w = _rates_via_update_w(V, kref.x, 64, 17, "generic", chunk_units=250)
    _assert_within(kref, w, 2.0, "generic (estep_kernel, L = 17)")


@gpu
def test_rates_of_the_long_kernels(V, kref, monkeypatch):
    """Units above 64 bins: the persistent long-unit kernel (fast_exp) while (units x latents) < 128, the task-parallel
    launch sequence (trunc_exp_tab256 row passes) from there on and when forced."""
    monkeypatch.delenv("VLGP_ESTEP_SPLIT", raising=False)
    monkeypatch.delenv("VLGP_ESTEP_LSPLIT", raising=False)
    n_units = -(-kref.x.size // 1000)
    assert n_units < 128
    w = _rates_via_update_w(V, kref.x, 1000, 1, "long")
    _assert_within(kref, w, 2.0, "long (estep_long_kernel)")
    _assert_split_family(V, kref, 300, 1, "long_split", "long_split (by size)")  # more than 128 (unit, latent) tasks
    monkeypatch.setenv("VLGP_ESTEP_SPLIT", "1")
    monkeypatch.setenv("VLGP_ESTEP_LSPLIT", "1")
    _assert_split_family(V, kref, 1000, 1, "long_split", "long_split (forced)")


@gpu
def test_rates_of_the_split_passes(V, kref, monkeypatch):
    """esplit_pass (trunc_exp_tab256, the headline path): forced onto small sets (300 units of 50 bins per call, which
    the size rule gives to the fast kernel), and taken by itself (the whole sample as one set of more than 512 units)."""
    monkeypatch.setenv("VLGP_ESTEP_SPLIT", "1")
    _assert_split_family(V, kref, 50, 1, "split", "split (forced, small sets)", chunk_units=300)
    monkeypatch.delenv("VLGP_ESTEP_SPLIT")
    assert kref.x.size > 512 * 50
    _assert_split_family(V, kref, 50, 1, "split", "split (by size)")
    _assert_split_family(V, kref, 50, 5, "split", "split (by size, L = 5)")


@gpu
def test_rates_of_the_split_pass_with_regressors(V, kref, monkeypatch):
    """The HASXB variant of the row pass: mu = 0, two regressors, b = (0, 1), the sample in x[:, 1, 0] -- eta = x.b."""
    monkeypatch.delenv("VLGP_ESTEP_SPLIT", raising=False)
    T = 50
    units = _as_units(kref.x, T, 1)
    for u in units:
        x = np.ones((T, 2, 1))
        x[:, 1, 0] = u["mu"][:, 0]
        u["x"] = x
        u["mu"] = np.zeros((T, 1))
    got = {}
    for loading in (SPLIT_LOADING, 1.0):  # (mu = 0: the loading scales w alone, eta = x.b is the sample either way)
        with V.Engine(1, 1, 2, 50) as eng:
            eng.set_params(np.full((1, 1), loading), np.array([[0.0], [1.0]]), np.ones(1))
            eng.upload(0, units)
            eng.update_w(0)
            assert eng.last_estep_path == "split"
            got[loading] = eng.download(0, keys=("w",))["w"][:kref.x.size, 0] / loading ** 2
    _assert_within(kref, got[SPLIT_LOADING], 1.5, "split, regressors (HASXB), a = 2")
    err = kref.ulp_error(got[1.0])
    low = kref.rounded < 2.0 ** -1021
    print("%-36s %.4f ulp where rate / 2 is normal, %.4f below" % ("split, regressors (HASXB), a = 1", err[~low].max(), err[low].max()))
    assert err[~low].max() < 1.5 and err[low].max() < 1.5 + 1.0


# ------------------------------------------------------------------ 3. M-step per channel; noise
def mstep_spread_problem(seed=41, n_units=320, T=50, N=16, L=5, lo=-5.0, hi=9.3):
    """Channels whose baselines spread the log-rate from -5 to 9.3 (eta = mu a + b within about +-0.5 of it: from -5.5
    to 9.8, below the clamp), 16 000 rows: the quietest channel expects ~110 spikes."""
    rng = np.random.default_rng(seed)
    rows = n_units * T
    mu = 0.8 * rng.standard_normal((rows, L))
    v = 0.02 + 0.05 * rng.random((rows, L))
    a_true = 0.08 * rng.standard_normal((L, N))
    b_true = np.linspace(lo, hi, N)[None, :]
    eta = mu @ a_true + b_true
    y = rng.poisson(np.exp(eta)).astype(float)
    a0 = a_true + 0.02 * rng.standard_normal((L, N))
    b0 = b_true + 0.05 * rng.standard_normal((1, N))
    return y, mu, v, a0, b0, eta


def per_channel_error(a, b, a_ref, b_ref):
    """Largest error of any channel, each judged on its own scale: a[:, n] against max |a_ref[:, n]|, b[:, n] against
    max(|b_ref[:, n]|, 1)."""
    ea = np.abs(a - a_ref).max(axis=0) / np.abs(a_ref).max(axis=0)
    eb = np.abs(b - b_ref).max(axis=0) / np.maximum(np.abs(b_ref).max(axis=0), 1.0)
    return ea, eb


MSTEP_ITERS = 3


def test_mstep_spread_case_is_well_conditioned():
    """The condition the per-channel comparison rests on (no GPU needed, checked on the oracle alone): perturbing every
    mu by one ulp moves no channel by more than a tenth of the tolerance."""
    y, mu, v, a0, b0, eta = mstep_spread_problem()
    assert eta.min() < -5.0 and 9.5 < eta.max() < 10.0
    assert 80 < y.sum(axis=0).min() < 200  # the quietest channel's spike count
    x = np.ones((y.shape[0], 1, y.shape[1]))
    gauss = np.zeros(y.shape[1], dtype=bool)
    base = O.mstep_arrays(y, x, mu, v, a0, b0, gauss, MSTEP_ITERS)
    rng = np.random.default_rng(1)
    moved = O.mstep_arrays(y, x, np.nextafter(mu, np.where(rng.random(mu.shape) < 0.5, -np.inf, np.inf)), v, a0, b0,
                           gauss, MSTEP_ITERS)
    ea, eb = per_channel_error(moved[0], moved[1], base[0], base[1])
    print("one-ulp perturbation of mu: a %.2e, b %.2e per channel at worst" % (ea.max(), eb.max()))
    assert ea.max() < 0.1 * STAGE and eb.max() < 0.1 * STAGE



@gpu
@pytest.mark.parametrize("generic", [False, True])
def test_mstep_per_channel_over_nine_decades_of_rate(V, generic, monkeypatch):
    """Three Newton iterations of the M-step (the kernel compiled for L = 5, P = 1, and the loop-based kernels forced by
    VLGP_MSTEP_GENERIC=1) on channels whose log-rates spread from -5.5 to 9.8 (final spread; see
    mstep_spread_problem), against oracle.mstep_arrays PER CHANNEL at the stage tolerance 1e-9: a gross error confined
    to the quiet channels is invisible under the max-norm of the other M-step tests.  Every channel is compared."""
    if generic:
        monkeypatch.setenv("VLGP_MSTEP_GENERIC", "1")
    else:
        monkeypatch.delenv("VLGP_MSTEP_GENERIC", raising=False)
    with V.Engine(4, 2, 1, 50) as probe:  # a handle created now, as V.mstep's is, holds the setting
        assert probe.switch("VLGP_MSTEP_GENERIC") == float(generic)
    y, mu, v, a0, b0, _ = mstep_spread_problem()
    T, N, L = 50, y.shape[1], mu.shape[1]
    x = np.ones((y.shape[0], 1, N))
    gauss = np.zeros(N, dtype=bool)
    want = O.mstep_arrays(y, x, mu, v, a0, b0, gauss, MSTEP_ITERS)
    units = [{"y": y[s:s + T], "x": np.ones((T, 1, N)), "mu": mu[s:s + T], "v": v[s:s + T],
              "w": np.zeros((T, L))} for s in range(0, y.shape[0], T)]
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": 50, "a": a0.copy(), "b": b0.copy(), "noise": np.ones(N),
              "likelihood": np.array(["poisson"] * N), "cholesky": {}, "gp_noise": 1e-4, "dt": 1}
    V.mstep(units, params, V.get_config(Mniter=MSTEP_ITERS))
    ea, eb = per_channel_error(params["a"], params["b"], want[0], want[1])
    print("per channel: a %s\n             b %s" % (np.array2string(ea, precision=1), np.array2string(eb, precision=1)))
    assert ea.shape == (N,) and eb.shape == (N,)
    assert ea.max() < STAGE, (int(np.argmax(ea)), ea.max())
    assert eb.max() < STAGE, (int(np.argmax(eb)), eb.max())


@gpu
@pytest.mark.parametrize("n_iter", [1, 3])
def test_noise_of_constant_residual_channels_is_not_negative(V, n_iter):
    """All-Poisson sets take noise = var(y - eta) from sums (noise_stats_kernel: s2 / n - mean^2).  A silent channel
    and a constant-count channel with zero loading have a constant residual after one iteration (the noise is
    taken at the parameters the iteration starts from), so the two terms cancel completely: the result must not come
    out below zero, and every channel matches the oracle's two-pass variance to 1e-9 of the largest noise."""
    rng = np.random.default_rng(17)
    N, L, T, M = 12, 3, 50, 24
    a = 0.3 * rng.standard_normal((L, N))
    a[:, [2, 7, 9]] = 0.0
    b = np.log(0.6) + 0.3 * rng.standard_normal((1, N))
    b[0, 7] = np.log(3.0)
    b[0, 9] = 1.0986122886681098 + 1e-3
    units = []
    for _ in range(M):
        mu = rng.standard_normal((T, L))
        yv = rng.poisson(np.exp(mu @ a + b)).astype(float)
        yv[:, 2] = 0.0   # silent
        yv[:, 7] = 3.0   # constant count
        yv[:, 9] = 3.0
        units.append({"y": yv, "x": np.ones((T, 1, N)), "mu": mu, "v": 0.05 * rng.random((T, L)), "w": np.zeros((T, L))})
    cat = lambda k: np.concatenate([u[k] for u in units], axis=0)
    gauss = np.zeros(N, dtype=bool)
    want = O.mstep_arrays(cat("y"), cat("x"), cat("mu"), cat("v"), a, b, gauss, n_iter)[4]
    params = {"ydim": N, "zdim": L, "xdim": 1, "rank": 50, "a": a.copy(), "b": b.copy(), "noise": np.ones(N),
              "likelihood": np.array(["poisson"] * N), "cholesky": {}, "gp_noise": 1e-4, "dt": 1}
    V.mstep(units, params, V.get_config(Mniter=n_iter))
    noise = params["noise"]
    print("noise of the constant-residual channels (2, 7, 9): %r; oracle %r" % (noise[[2, 7, 9]], want[[2, 7, 9]]))
    if n_iter == 1:
        assert np.all(want[[2, 7, 9]] < 1e-25)
    assert np.all(noise >= 0.0), noise
    assert np.abs(noise - want).max() <= STAGE * want.max(), (noise, want)
